#!/usr/bin/env python3
"""Cache lines k_lite's minute-window and exception-sum accesses need on a C4 batch, counted on the host from the trace.

usage: tools/lite_lines.py [--batch-events N] [--batch K] [--out FILE.json]

The bench's seeded C4 trace (bench.make_trace), batch K (default 1: the second one, so the first is its history).  A
segment is k_lite's when its resource has at most LANE_MAX events in the batch (C4's programs are all lite-eligible).
Counted:
  * segments, events, distinct (resource, second) pairs: one minute bucket written per pair;
  * carried-over seconds: segments whose first event falls in the second the resource last wrote in the batch before
    (the only bucket reads the stale rule keeps);
  * exc_advance bucket reads of the resources with an exception-count breaker, before (one bucket per second elapsed
    since the last advance, none from 60 s on) and after the early exit (the walk ends where the sum reaches 0).  The
    sum is taken as if every TRACE were effective (its ENTRY passed), so "after" is an upper bound;
  * fixed lines a segment: 2-3 rule lines and one Seg line (what a descriptor and a carried list entry would save).
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from sentinel_amd import _abi as A  # noqa: E402
from sentinel_amd import tracegen as T  # noqa: E402

LANE_MAX = 256


def exc_count_resources(w):
    """Resource ids that carry an EXCEPTION_COUNT breaker (rule -> resource by its name pointer, as Workload._subset)."""
    ptr, n = w.degrade
    size = C.sizeof(A.SgDegradeRule)
    f = A.SgDegradeRule.grade
    raw = np.frombuffer((C.c_char * (n * size)).from_address(ptr), dtype=np.uint8).reshape(n, size)
    grade = np.ascontiguousarray(raw[:, f.offset:f.offset + f.size]).view({1: np.uint8, 4: np.int32}[f.size])[:, 0]
    rptr = np.frombuffer((C.c_char * (n * size)).from_address(ptr), dtype=np.uint64).reshape(n, size // 8)[:, 0]
    names = np.frombuffer((C.c_char * (8 * w.n_res)).from_address(w.names_ptr), dtype=np.uint64)
    order = np.argsort(names)
    rid = order[np.minimum(np.searchsorted(names[order], rptr), w.n_res - 1)]
    assert (names[rid] == rptr).all()
    return np.unique(rid[grade == A.DEGRADE_GRADE_EXCEPTION_COUNT])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-events", type=int, default=1 << 25)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--resources", type=int, default=1_000_000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    B, K, R = a.batch_events, a.batch, a.resources
    w, ev = bench.make_trace(R, B, K + 1, T.SEED_BASE + 4)
    cur, hist = ev[K * B:(K + 1) * B], ev[:K * B]
    res = cur["res_id"].astype(np.int64)
    sec = cur["ts"] // 1000
    n_ev = np.bincount(res, minlength=R)
    lite = (n_ev > 0) & (n_ev <= LANE_MAX)
    m = lite[res]
    s0 = int(hist["ts"][0] // 1000)
    key = res[m] * (1 << 20) + (sec[m] - s0)  # events are time-ordered: a resource's keys ascend
    pairs = np.unique(key)
    # the second each resource last wrote before the batch, the first it writes in it
    last = np.full(R, -1, dtype=np.int64)
    last[hist["res_id"]] = hist["ts"] // 1000  # (later rows overwrite earlier ones)
    first = np.full(R, -1, dtype=np.int64)
    first[res[::-1]] = sec[::-1]
    carried = int((lite & (first == last)).sum())

    # exc_advance: one advance per (resource, second) pair of a resource with an exception-count breaker
    xr = np.zeros(R, dtype=bool)
    xr[exc_count_resources(w)] = True
    pk = pairs[xr[pairs >> 20]]
    pres, psec = pk >> 20, (pk & ((1 << 20) - 1)) + s0
    newres = np.r_[True, pres[1:] != pres[:-1]]
    prev = np.where(newres, last[pres], np.r_[0, psec[:-1]])  # the second of the resource's previous advance
    have = prev >= 0
    gap = psec - prev
    before = np.where(have & (gap < 60), gap, 0)
    # the last second at or before prev with a TRACE of the resource (whole trace so far): the walk from prev - 59
    # ends there, or at T - 60 if that comes first; a sum of 0 (no such second inside the window) reads nothing
    tr = ev[:(K + 1) * B]
    tr = tr[(tr["kind"] == A.EV_TRACE) & xr[tr["res_id"]]]
    tkey = np.unique(tr["res_id"].astype(np.int64) * (1 << 20) + (tr["ts"] // 1000 - s0))
    q = pres * (1 << 20) + (prev - s0)
    i = np.searchsorted(tkey, q, side="right") - 1
    hit = (i >= 0) & have
    tl = np.where(hit, tkey[np.maximum(i, 0)], -1)
    same = hit & ((tl >> 20) == pres)
    lsec = (tl & ((1 << 20) - 1)) + s0
    inwin = same & (lsec >= prev - 59)
    stop = np.minimum(lsec, psec - 60)
    after = np.where(inwin & have & (gap < 60), np.maximum(stop - (prev - 59) + 1, 0), 0)
    out = {
        "batch_events": B, "batch": K, "lane_max": LANE_MAX,
        "lite_segments": int(lite.sum()), "lite_events": int(n_ev[lite].sum()),
        "segments_le_7_events": int((lite & (n_ev <= 7)).sum()),
        "resource_second_pairs": int(len(pairs)), "carried_over_seconds": carried,
        "exc_count_segments": int((lite & xr).sum()),
        "exc_advance_reads_before": int(before.sum()), "exc_advance_reads_after_upper_bound": int(after.sum()),
        "rule_and_seg_lines": [int(lite.sum()) * 3, int(lite.sum()) * 4],
    }
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
