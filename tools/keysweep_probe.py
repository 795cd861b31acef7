"""How long sg_param_keys_sweep takes (exact parameter keys): at C6's pool -- 1M resources' maps,
param_table_log2 = 29, a 2^28-word key ring -- with 1M candidate Strings of which 200k are live on the device,
next to C6's batch time from the same run; and the token server's value table on an engine with a cluster param
rule.  Per sweep: sg_param_keys_stats and the three device scans in ms.  Writes profiles/exact_keys/sweep_c6.json.

    python tools/keysweep_probe.py"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np
import torch
torch.zeros(1, device="cuda")
import bench
from sentinel_amd import engine as E, tracegen as T, _abi as A

out = {}
dev = torch.device("cuda", 0)
cfg, n_entries, gb, kw, var, name = bench.CONFIGS[3]
assert cfg == 6
n_entries = 33_000_000  # two batches of 2^25 events: the first untimed, the second timed
t0 = time.time()
w = T.Workload(6, seed=T.SEED_BASE + 6, n_entries=n_entries, variant=var)
ev = w.events
print("trace: %d events in %.1f s" % (len(ev), time.time() - t0), flush=True)
eng = E.Engine(device=0, max_resources=max(w.n_res, 1 << 10), max_slot_chain_size=0, max_batch_events=gb,
               aux_node_capacity=1 << 20, **kw)
w.install(eng)
# the trace's own keys are of an exact kind (they never enter the dictionary): the candidates are 1M Strings interned
# here, of which the first 200k are then sent through the param rules of the trace's resources
names = [b"cand-%07d" % i for i in range(1_000_000)]
t0 = time.time(); keys = eng.param_intern_many(names); t_intern = time.time() - t0
r = bench.run_batches(eng, ev, gb, dev, cfg_key=None, args_keyed=True)
out["c6_batches"] = {k: r[k] for k in ("value", "ms_per_batch", "stage_ms_mean", "batches_timed", "batch_events")}
print(json.dumps(out["c6_batches"]), flush=True)
live = keys[:200_000]
evl = np.zeros(len(live), dtype=A.EVENT_DTYPE)
evl["ts"] = int(ev["ts"].max()) + 1 + np.arange(len(live)) // 1000
evl["res_id"] = ev["res_id"][:len(live)]  # spread over the trace's resources
evl["count"], evl["kind"], evl["flags"], evl["aux"] = 1, A.EV_ENTRY, A.F_HAS_ARG, live
eng.submit(evl)
pool = eng.param_pool()
sweeps = []
for i in range(4):
    if i == 2:
        eng.param_intern_many(names)  # touch everything again: the next two sweeps repeat the measurement
    st = eng.param_keys_sweep()
    st["scan_ms"] = dict(zip(("maps", "ring", "pval"), eng.keysweep_scans()))
    sweeps.append(st)
    print(json.dumps(st), flush=True)
out["c6_sweeps"] = sweeps
out["c6_pool"] = pool
out["c6_maps"] = "1M resources: a rule map and a thread-count map each"
out["intern_1M_via_python_s"] = t_intern
eng.close()
del eng
torch.cuda.empty_cache()

# the token server's value table: an engine with one cluster param rule, 60k values requested
eng = E.Engine(device=0, max_resources=64, status_ring_log2=20)
eng.register("abc")
eng.load_param_rules([A.param_rule("abc", 0, 5, cluster_mode=True, cluster_flow_id=17,
                                   cluster_threshold_type=A.CLUSTER_THRESHOLD_GLOBAL)])
vals = eng.param_intern_many([b"tv-%06d" % i for i in range(60_000)])
reqs = np.zeros(len(vals), dtype=A.PARAM_TOKEN_REQ_DTYPE)
reqs["ts"], reqs["flow_id"], reqs["acquire_count"], reqs["n_values"] = 1_700_000_000_000, 17, 1, 1
reqs["value_off"] = np.arange(len(vals))
eng.cluster_request_param_array(reqs, vals)
ps = []
for i in range(3):
    st = eng.param_keys_sweep()
    st["scan_ms"] = dict(zip(("maps", "ring", "pval"), eng.keysweep_scans()))
    ps.append(st)
    print(json.dumps(st), flush=True)
out["pval_sweeps"] = ps
os.makedirs(os.path.join(ROOT, "profiles", "exact_keys"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "exact_keys", "sweep_c6.json"), "w") as f:
    json.dump(out, f, indent=1)
print("done")
