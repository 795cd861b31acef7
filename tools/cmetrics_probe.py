"""What one sg_cluster_metrics call costs: wall time and the device time of each stage.

Fills the token server's (flowId, value) table with --pairs distinct pairs spread evenly over --flows GLOBAL param
flows (calls of at most --call requests, all inside one window, every value asked once or --repeat times so that it
passes and is live), then reads the metrics --reads times and prints one JSON line: the table's statistics, the
first read apart (it allocates the scratch), and for the others the median wall time and the median device time of
each stage (HIP events, Engine.cluster_metrics_last()).  scan_table_gbps is the table's bytes (slots x 272) over the
scan's time, the rate to hold against a stream copy; scan_touched_gbps counts only what the scan has to read: 16 B
of every slot, and of a claimed slot the stamps and counts of the buckets that count.
    python tools/cmetrics_probe.py --flows 64 --pairs 2000000
    python tools/cmetrics_probe.py --flows 10000 --pairs 30000"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    from sentinel_amd import _abi as A
    from sentinel_amd import engine as E

    ap = argparse.ArgumentParser()
    ap.add_argument("--flows", type=int, default=64)
    ap.add_argument("--pairs", type=int, default=2_000_000, help="distinct (flow, value) pairs put into the table")
    ap.add_argument("--call", type=int, default=2_000_000, help="requests per token call")
    ap.add_argument("--repeat", type=int, default=1, help="times every pair is asked (its sum)")
    ap.add_argument("--reads", type=int, default=5)
    ap.add_argument("--top", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--label", default="")
    a = ap.parse_args()

    rules = [A.param_rule("abc", 0, 1000, cluster_mode=True, cluster_flow_id=1000 + i,
                          cluster_threshold_type=A.CLUSTER_THRESHOLD_GLOBAL) for i in range(a.flows)]
    eng = E.Engine(max_resources=64, cluster_max_allowed_qps=2_000_000_000)
    eng.register("abc")
    eng.load_param_rules(rules)
    rng = np.random.default_rng(a.seed)
    t0 = 1_700_000_000_000
    pair = np.arange(a.pairs, dtype=np.uint64)
    sent = 0
    t_fill = time.perf_counter()
    for _ in range(a.repeat):
        order = rng.permutation(a.pairs)
        for lo in range(0, a.pairs, a.call):
            p = pair[order[lo:lo + a.call]]
            arr = np.zeros(len(p), dtype=A.PARAM_TOKEN_REQ_DTYPE)
            arr["ts"] = t0 + 100 + (sent + np.arange(len(p))) * 500 // (a.pairs * a.repeat)
            arr["flow_id"] = 1000 + (p % np.uint64(a.flows)).astype(np.int64)
            arr["acquire_count"] = 1 + (p % np.uint64(3)).astype(np.int32)
            arr["n_values"] = 1
            arr["value_off"] = np.arange(len(p), dtype=np.uint64)
            res = eng.cluster_request_param_array(arr, (p // np.uint64(a.flows)) | (np.uint64(1) << np.uint64(40)))
            assert (res["status"] == A.TOKEN_OK).all()
            sent += len(p)
    t_fill = time.perf_counter() - t_fill
    now = t0 + 700
    walls, lasts = [], []
    for _ in range(a.reads + 1):
        t = time.perf_counter()
        rows = eng.cluster_metrics(now, top=a.top)
        walls.append((time.perf_counter() - t) * 1e3)
        lasts.append(eng.cluster_metrics_last())
    assert len(rows) == a.flows and int(rows["n_top"].min()) == min(a.top, a.pairs // a.flows)
    med = lambda k: statistics.median(x[k] for x in lasts[1:])
    stats = eng.cluster_param_table_stats()
    last = lasts[-1]
    scan_s = med("scan_ms") / 1e3
    buckets = 6  # the fill spans six 100 ms buckets: a claimed slot costs their stamps, and one count
    touched = last["slots"] * 16 + last["candidates"] * (buckets * 8 + 8)
    print(json.dumps({
        "label": a.label, "flows": a.flows, "pairs": a.pairs, "repeat": a.repeat, "top": a.top,
        "capacity": stats["capacity"], "table_bytes": stats["capacity"] * 272, "rehashes": stats["rehashes"],
        "candidates": last["candidates"], "chunks": last["chunks"], "fill_s": round(t_fill, 3),
        "first_read_wall_ms": round(walls[0], 3), "read_wall_ms": round(statistics.median(walls[1:]), 3),
        "read_wall_ms_all": [round(w, 3) for w in walls[1:]],
        "call_ms": round(med("wall_ms"), 3),
        **{k: round(med(k), 4) for k in ("rows_ms", "scan_ms", "group_ms", "select_ms", "merge_ms")},
        "scan_table_gbps": round(last["slots"] * 272 / scan_s / 1e9, 1) if scan_s else None,
        "scan_touched_gbps": round(touched / scan_s / 1e9, 1) if scan_s else None,
    }), flush=True)


if __name__ == "__main__":
    main()
