"""Token server with the flows dealt over K namespaces, at the size of bench.token_line: its request stream (10k
GLOBAL flowIds, Zipf(1.1), 2^21-request calls, requests and results in HBM), the flows dealt round-robin over
K namespaces whose limits are all above the traffic.  No limit binds, so the results of every K must equal those
of K = 1 request for request; one JSON line per (K, run) with the rate, and a last line with the ratios to K = 1.

usage: tools/ns_probe.py [--k 1,8,256] [--runs 3] [--requests 16000000] [--pkg DIR]
  --pkg DIR: import sentinel_amd from DIR (another build of the package, e.g. the parent commit's, for an A/B of
             the single-namespace line; K = 1 makes none of the namespace calls)
  SG_TOK_NS=1 in the environment: the grouped limiter for K = 1 too."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", default="1,8,256")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--requests", type=int, default=16_000_000)
    ap.add_argument("--batch", type=int, default=1 << 21)
    ap.add_argument("--flows", type=int, default=10_000)
    ap.add_argument("--seconds", type=int, default=60)
    ap.add_argument("--pkg", default=ROOT)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg))
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    from sentinel_amd import _abi as A
    from sentinel_amd import engine as E

    # bench.token_line's flows and requests
    rng = np.random.default_rng(20240601 + 15)
    n_flows, n_req = a.flows, a.requests
    fids = np.arange(1_000_001, 1_000_001 + n_flows)
    rules = [A.flow_rule("r%d" % f, float(int(np.exp(rng.uniform(np.log(1e3), np.log(1e5))))), cluster_mode=True,
                         cluster_flow_id=int(f), cluster_threshold_type=A.CLUSTER_THRESHOLD_GLOBAL,
                         cluster_sample_count=int(rng.choice([1, 2, 5, 10])),
                         cluster_window_interval_ms=int(rng.choice([500, 1000, 2000]))) for f in fids]
    p = 1.0 / np.arange(1, n_flows + 1) ** 1.1
    p /= p.sum()
    reqs = np.zeros(n_req, dtype=A.TOKEN_REQ_DTYPE)
    reqs["ts"] = 1_700_000_000_000 + np.sort(rng.integers(0, a.seconds * 1000, n_req))
    reqs["flow_id"] = fids[rng.choice(n_flows, n_req, p=p)]
    reqs["acquire_count"] = rng.integers(1, 4, n_req)
    reqs["prioritized"] = rng.random(n_req) < 0.2
    rq, rs = A.TOKEN_REQ_DTYPE.itemsize, A.TOKEN_RES_DTYPE.itemsize
    dq = torch.from_numpy(reqs.view(np.uint8)).to(dev)
    dr = torch.empty(n_req * rs, dtype=torch.uint8, device=dev)
    cuts = list(range(0, n_req, a.batch)) + [n_req]
    names = ["r%d" % f for f in fids]

    first, rates, ok = None, {}, True
    for K in [int(x) for x in a.k.split(",")]:
        for run in range(a.runs):
            eng = E.Engine(device=dev.index, max_resources=max(1 << 14, n_flows + 16), cluster_max_allowed_qps=10 ** 9)
            eng.register_many(names)
            if K > 1:  # rank i -> namespace i % K ("default" is one of the K)
                for k in range(1, K):
                    eng.cluster_namespace("ns-%d" % k, 1e9)
                    eng.cluster_assign_flows("ns-%d" % k, fids[k::K])
            eng.load_flow_rules(rules)
            dr.zero_()
            eng.cluster_request_ptr(dq.data_ptr(), cuts[1], dr.data_ptr())  # first call untimed
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for x, y in zip(cuts[1:-1], cuts[2:]):
                eng.cluster_request_ptr(dq.data_ptr() + x * rq, y - x, dr.data_ptr() + x * rs)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            eng.close()
            res = dr.cpu().numpy()
            if first is None:
                first = res
            same = bool(np.array_equal(res, first))
            ok = ok and same
            st = res.view(np.int32).reshape(-1, 4)[:, 0]
            rate = (n_req - cuts[1]) / dt
            rates.setdefault(K, []).append(rate)
            print(json.dumps({"tag": a.tag, "namespaces": K, "run": run, "token_requests_per_s": rate,
                              "ms_per_call": dt / (len(cuts) - 2) * 1e3, "equal_to_first": same,
                              "status_counts": {str(s): int(c) for s, c in zip(*np.unique(st, return_counts=True))}}),
                  flush=True)
    ks = sorted(rates)
    med = {k: float(np.median(rates[k])) for k in ks}
    print(json.dumps({"tag": a.tag, "median_rate": med, "ratio_to_first_k": {k: med[k] / med[ks[0]] for k in ks},
                      "all_results_equal": ok}), flush=True)
    if not ok:
        raise SystemExit("results differ between namespace counts")


if __name__ == "__main__":
    main()
