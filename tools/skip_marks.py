"""Forward-link exchanges of the C4 headline batch, counted on the host from bench.py's trace (DESIGN.md section 5,
"Side tables only where a 500 ms bucket can hold a skip"; profiles/bucket_marks/marks.json).

usage: python tools/skip_marks.py [--gpu]      -> one JSON line

Batches 0..2 of the trace; the figures are batch 2's with the hot ids batch 1 leaves (resources of >= n / 8192 events):
the hot ids and their share of the events, the hot EXIT / TRACEs that name an ENTRY of the batch (one exchange each),
the ids whose bound (k_hot_bmax's, from tile boundaries) and whose true largest 500 ms bucket exceed their owner's skip
threshold (by segment length, as QPS-DefaultController programs are binned), and the exchanges of the marked and the
unmarked ids.  No GPU is needed; --gpu also submits the three batches and adds the engine's sgx_hot_marked counts."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
import bench  # noqa: E402
from sentinel_amd import tracegen as T  # noqa: E402

GB = 1 << 25
TILE = 4096
w, ev = bench.make_trace(1_000_000, GB, 3, T.SEED_BASE + 4)
out = {}
if "--gpu" in sys.argv:
    from sentinel_amd import engine as E
    eng = E.Engine(max_resources=1 << 20, max_slot_chain_size=0, param_table_log2=16, status_ring_log2=28,
                   max_batch_events=GB)
    w.install(eng)
    out["hot_marked"] = []
    for b in range(3):
        eng.submit(ev[b * GB:(b + 1) * GB])
        out["hot_marked"].append(eng.hot_marked())
    eng.close()
prev, cur = ev[GB:2 * GB], ev[2 * GB:3 * GB]
cnt_prev = np.bincount(prev["res_id"], minlength=1_000_000)
hot_ids = np.nonzero(cnt_prev >= max(64, GB // 8192))[0]
out["hot_ids"] = int(len(hot_ids))
hid_of = np.full(1_000_000, -1, dtype=np.int64)
hid_of[hot_ids] = np.arange(len(hot_ids))
hid = hid_of[cur["res_id"]]
hot = hid >= 0
out["hot_event_share"] = float(hot.mean())
ref = (cur["aux"] & np.uint64(0xFFFFFFFFFFFF)).astype(np.int64)
inb = (cur["kind"] != 0) & (ref != 0xFFFFFFFFFFFF) & (ref >= 2 * GB)
names_entry = np.zeros(GB, dtype=bool)
names_entry[inb] = cur["kind"][ref[inb] - 2 * GB] == 0
xch = hot & inb & names_entry
out["exchanges_all_hot"] = int(xch.sum())
out["hot_exit_trace"] = int((hot & (cur["kind"] != 0)).sum())
# the bound: per tile counts of every hot id, buckets opened by a tile's first event
nh, nt = len(hot_ids), GB // TILE
C = np.bincount((np.arange(GB)[hot] // TILE) * nh + hid[hot], minlength=nt * nh).reshape(nt, nh)
P = np.concatenate([np.zeros((1, nh), dtype=np.int64), np.cumsum(C, axis=0)])  # P[t] = events in tiles < t
fb = cur["ts"][::TILE] // 500
edges = np.nonzero(np.concatenate([[True], fb[1:] != fb[:-1]]))[0]
nxt = np.concatenate([edges[1:], [nt]])
bmax = np.max(P[nxt] - P[np.maximum(edges - 1, 0)], axis=0)
bk = cur["ts"] // 500
truemax = np.zeros(nh, dtype=np.int64)
for k in np.unique(bk):
    i0, i1 = np.searchsorted(bk, k), np.searchsorted(bk, k, side="right")
    truemax = np.maximum(truemax, np.bincount(hid[i0:i1][hot[i0:i1]], minlength=nh))
length = P[-1]
thr = np.where(length <= 65536, 8192, np.where(length <= (1 << 23), 16384, 32768))
marked = bmax > thr
out["buckets_opened"] = int(len(edges))
out["marked_by_bound"] = int(marked.sum())
out["marked_by_true_count"] = int((truemax > thr).sum())
out["marked_share_of_events"] = (np.sort(length[marked])[::-1] / GB).round(4).tolist()
per_id = np.bincount(hid[xch], minlength=nh)
out["exchanges_marked"] = int(per_id[marked].sum())
out["exchanges_unmarked"] = int(per_id[~marked].sum())
out["unmarked_share_of_exchanges"] = float(per_id[~marked].sum() / max(1, per_id.sum()))
out["largest_unmarked_bound_over_thr"] = float(np.max((bmax / thr)[~marked])) if (~marked).any() else None
print(json.dumps(out))
