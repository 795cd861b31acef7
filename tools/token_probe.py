"""Token-server probes on one box.

Flow mode: bench.token_line under each SG_TOK_* setting given as an argument
(e.g. "SG_TOK_WIDE=512" "SG_TOK_WIDE=1024" "SG_TOK_LIGHT=0,SG_TOK_WIDE=1024"); one JSON line each.

Param mode (first argument `param`): a Zipf value stream over N GLOBAL param flows for T seconds of trace time,
one sg_cluster_request_param_tokens call per tick; prints requests/s (the first call apart: it allocates) and
sg_cluster_param_table_stats.  --fresh is the share of requests that carry a never-seen value, which sets how
many distinct (flow, value) pairs the stream brings.  --device feeds the calls as device tensors through
Engine.cluster_request_param_ptr (uploaded before the clock starts); --multi SHARE gives that share of the requests
two or three values, which keeps their flows on the one-lane-per-flow owner (k_ptok_flow) for the call; the owners'
counters are printed with the table's.  A failed call ends the stream and is reported, not raised.
    python tools/token_probe.py param --flows 64 --seconds 60 --rate 1000            # stays under 2^16 claims
    python tools/token_probe.py param --flows 64 --seconds 40 --rate 100000 --fresh 0.55   # > 2M pairs"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def flow_mode(variants):
    import bench
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    for k, var in enumerate(variants or [""]):
        env = dict(kv.split("=") for kv in var.split(",") if kv)
        for kk in ("SG_TOK_WIDE", "SG_TOK_LIGHT"):
            os.environ.pop(kk, None)
        os.environ.update(env)
        r = bench.token_line(dev, cpu_requests=2_000_000 if k == 0 else 0)
        print(json.dumps({"variant": var, **r}), flush=True)


def param_mode(argv):
    import numpy as np
    from sentinel_amd import _abi as A
    from sentinel_amd import engine as E

    ap = argparse.ArgumentParser(prog="token_probe.py param")
    ap.add_argument("--flows", type=int, default=64)
    ap.add_argument("--seconds", type=int, default=60, help="trace time")
    ap.add_argument("--rate", type=int, default=1000, help="requests per trace second")
    ap.add_argument("--tick-ms", type=int, default=1000, help="trace time per device call")
    ap.add_argument("--values", type=int, default=10_000_000, help="recurring values per flow (Zipf ranks)")
    ap.add_argument("--zipf", type=float, default=1.1)
    ap.add_argument("--fresh", type=float, default=0.0, help="share of requests with a never-seen value")
    ap.add_argument("--device", action="store_true", help="device tensors through cluster_request_param_ptr")
    ap.add_argument("--multi", type=float, default=0.0, help="share of requests with two or three values")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--label", default="")
    a = ap.parse_args(argv)

    shapes = [(10, 1000), (5, 500), (2, 1000), (1, 200)]
    rules = [A.param_rule("abc", 0, 20, cluster_mode=True, cluster_flow_id=1000 + i,
                          cluster_threshold_type=A.CLUSTER_THRESHOLD_GLOBAL, cluster_sample_count=shapes[i % 4][0],
                          cluster_window_interval_ms=shapes[i % 4][1]) for i in range(a.flows)]
    if a.device:  # (torch's HIP context first, as flow_mode does)
        import torch
        torch.zeros(1, device="cuda")
    eng = E.Engine(max_resources=64, cluster_max_allowed_qps=2_000_000_000)
    eng.register("abc")
    eng.load_param_rules(rules)
    rng = np.random.default_rng(a.seed)
    t0 = 1_700_000_000_000
    per = max(1, a.rate * a.tick_ms // 1000)
    calls, fresh_pairs, counter = [], 0, 0
    for c in range(a.seconds * 1000 // a.tick_ms):
        f = rng.integers(0, a.flows, per)
        v = np.minimum(rng.zipf(a.zipf, per), a.values).astype(np.uint64)
        fr = rng.random(per) < a.fresh
        nf = int(fr.sum())
        v[fr] = (np.uint64(1) << np.uint64(39)) | (np.uint64(counter) + np.arange(nf, dtype=np.uint64))
        counter += nf
        fresh_pairs += nf
        arr = np.zeros(per, dtype=A.PARAM_TOKEN_REQ_DTYPE)
        arr["ts"] = t0 + c * a.tick_ms + np.sort(rng.integers(0, a.tick_ms, per))
        arr["flow_id"], arr["acquire_count"], arr["n_values"] = 1000 + f, 1, 1
        arr["value_off"] = np.arange(per, dtype=np.uint64)
        vals = (f.astype(np.uint64) << np.uint64(40)) | v
        if a.multi > 0:  # the extra values of a request follow the call's first values
            nv = np.where(rng.random(per) < a.multi, rng.integers(2, 4, per), 1)
            extra = nv - 1
            arr["n_values"] = nv
            total = per + int(extra.sum())
            allv = np.zeros(total, dtype=np.uint64)
            start = np.cumsum(nv) - nv
            arr["value_off"] = start
            allv[start] = vals
            rest = np.ones(total, dtype=bool)
            rest[start] = False
            owner = np.repeat(np.arange(per), extra)
            allv[rest] = (f[owner].astype(np.uint64) << np.uint64(40)) | rng.integers(1, 50, len(owner)).astype(np.uint64)
            vals = allv
        calls.append((arr, vals, nf))
    if a.device:
        dev = [(torch.from_numpy(arr.view(np.uint8).copy()).cuda(), torch.from_numpy(vals.view(np.int64).copy()).cuda(),
                torch.empty(len(arr) * A.TOKEN_RES_DTYPE.itemsize, dtype=torch.uint8, device="cuda"))
               for arr, vals, _ in calls]
        torch.cuda.synchronize()
    status = np.zeros(8, dtype=np.int64)
    call_ms = []
    done, fresh_done, err, first_s, t_run = 0, 0, None, 0.0, 0.0
    for c, (arr, vals, nf) in enumerate(calls):
        t = time.perf_counter()
        try:
            if a.device:
                tq, tv, to = dev[c]
                eng.cluster_request_param_ptr(tq.data_ptr(), len(arr), tv.data_ptr(), len(vals), to.data_ptr())
                out = None
            else:
                out = eng.cluster_request_param_array(arr, vals)
        except E.SentinelError as exc:
            err = {"call": c, "requests_before": done, "fresh_pairs_before": fresh_done, "error": str(exc),
                   "call_s": round(time.perf_counter() - t, 3)}
            break
        dt = time.perf_counter() - t
        if c == 0:
            first_s = dt
        else:
            t_run += dt
        done += len(arr)
        fresh_done += nf
        call_ms.append(dt * 1000.0)
        if out is None:  # (outside the clock)
            out = dev[c][2].cpu().numpy().view(A.TOKEN_RES_DTYPE)
        status += np.bincount(np.clip(out["status"], -1, 6) + 1, minlength=8)[:8]
    timed = done - (len(calls[0][0]) if done else 0)
    stats = eng.cluster_param_table_stats() if hasattr(eng, "cluster_param_table_stats") else None
    owners = eng.cluster_param_owner_stats() if hasattr(eng, "cluster_param_owner_stats") else None
    med = float(np.median(call_ms[1:])) if len(call_ms) > 1 else None
    print(json.dumps({"mode": "param", "label": a.label, "flows": a.flows, "trace_seconds": a.seconds, "rate": a.rate,
                      "tick_ms": a.tick_ms, "fresh": a.fresh, "multi": a.multi, "device": bool(a.device), "requests": done, "fresh_pairs": fresh_pairs,
                      "first_call_s": round(first_s, 4), "timed_requests": timed, "timed_s": round(t_run, 4),
                      "requests_per_s": round(timed / t_run) if t_run > 0 else None,
                      "ok": int(status[A.TOKEN_OK + 1]), "blocked": int(status[A.TOKEN_BLOCKED + 1]),
                      "call_ms_median": round(med, 4) if med is not None else None,
                      "call_ms_min": round(min(call_ms[1:]), 4) if len(call_ms) > 1 else None,
                      "table": stats, "owners": owners, "failed": err}), flush=True)
    eng.close()


if __name__ == "__main__":
    if sys.argv[1:2] == ["param"]:
        param_mode(sys.argv[2:])
    else:
        flow_mode(sys.argv[1:])
