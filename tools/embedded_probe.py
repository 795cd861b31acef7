"""What the embedded token server costs: a C4 trace at 1M resources with 1 % of the resources -- drawn by event
count, so hot ones are among them -- given a cluster flow rule in place of their local one, in synchronous batches of
2^22 events, with sg_cluster_embedded on against off on the same build and the same rules.  Prints one JSON line: ms a
batch of either leg (the mean of the batches after the first), the requests and answers of the last batch, where the
eligible segments were decided, and the device times of the extraction, the token call and the scatter.

usage: python tools/embedded_probe.py [batches]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from sentinel_amd import _abi as A  # noqa: E402
from sentinel_amd import engine as E  # noqa: E402
from sentinel_amd import tracegen as T  # noqa: E402

BATCH = 1 << 22
N_RES = 1_000_000
nb = int(sys.argv[1]) if len(sys.argv) > 1 else 4
w = T.Workload(4, n_entries=(BATCH * nb) // 2 + 200_000, n_res=N_RES)
ev = np.array(w.events[:BATCH * nb], dtype=A.EVENT_DTYPE, copy=True)
assert len(ev) == BATCH * nb, "trace too short"
names = w.names()
cnt = np.bincount(ev["res_id"], minlength=N_RES)
rng = np.random.default_rng(2)
# 1 % of the resources: the 100 hottest of every 10,000 by rank would be all hot; every 100th by rank takes hot and
# cold ones alike (rank 0, 100, 200, ...)
rank = np.argsort(-cnt, kind="stable")
elig = rank[::100]
per_s = cnt[elig] / 2.0 / max(1e-3, (int(ev["ts"][-1]) - int(ev["ts"][0])) / 1000.0)  # entries a second
ptr, n = w.flow
old = (A.SgFlowRule * n).from_address(ptr)
is_el = np.zeros(N_RES, dtype=bool)
is_el[elig] = True
ids = {nm: i for i, nm in enumerate(names)}
rules = [r for r in old if not is_el[ids[r.resource.decode()]]]
for k, (r, q) in enumerate(zip(elig, per_s)):  # a threshold of half the resource's rate: about half of the requests OK
    rules.append(A.flow_rule(names[int(r)], max(1.0, float(q) / 2), cluster_mode=True, cluster_flow_id=10_000 + k,
                             cluster_threshold_type=A.CLUSTER_THRESHOLD_GLOBAL, cluster_fallback_to_local=False))
out = {"batch_events": BATCH, "batches": nb, "eligible_resources": int(len(elig)),
       "eligible_event_share": round(float(cnt[elig].sum()) / len(ev), 4),
       "hottest_eligible_segment_events": int((ev["res_id"][BATCH:2 * BATCH] == elig[0]).sum())}
words = {}
for mode in ("on", "off"):
    eng = E.Engine(max_resources=1 << 20, max_slot_chain_size=0, status_ring_log2=26, max_batch_events=BATCH,
                   cluster_max_allowed_qps=1 << 30)
    w.install(eng)
    eng.load_flow_rules(rules)
    if mode == "on":
        eng.cluster_embedded(True)
    ms, dec = [], []
    for i in range(nb):
        t = time.perf_counter()
        dec.append(eng.submit(ev[i * BATCH:(i + 1) * BATCH]))
        ms.append((time.perf_counter() - t) * 1e3)
    leg = {"ms_per_batch": round(float(np.mean(ms[1:])), 3), "ms_batches": [round(x, 3) for x in ms]}
    if mode == "on":
        leg["last_batch"] = eng.cluster_embedded_stats()
        leg["device_ms"] = {k: round(v, 4) for k, v in eng.cluster_embedded_ms().items()}
    words[mode] = np.concatenate(dec)
    out[mode] = leg
    eng.close()
out["words_changed_by_the_mode"] = int((words["on"] != words["off"]).sum())
out["ms_on_minus_off"] = round(out["on"]["ms_per_batch"] - out["off"]["ms_per_batch"], 3)
print(json.dumps(out))
