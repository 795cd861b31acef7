"""What tracking the global inbound node (sg_track_inbound, inbound.hip) costs: C4 batches of 2^25 events (or
2^`log2`) through sg_submit, timed with tracking off and on in one process on the same build.  Prints one JSON line:
ms a batch of either leg (wall, and the decide stage's device time, which holds the pass), the difference, the
decisions' equality and what the pass of the last batch saw.  With --ext the batches go through sg_submit_ex with
contexts and origins (C4-ext), so the aux post pass runs beside it; its kernels' device times come from a kernel trace
of this script (rocprofv3 --kernel-trace --stats, no counters in the same run).

usage: python tools/inbound_probe.py [batches] [log2 of the batch] [--ext]
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

argv = [a for a in sys.argv[1:] if a != "--ext"]
use_ext = "--ext" in sys.argv[1:]
nb = int(argv[0]) if len(argv) > 0 else 4
BATCH = 1 << (int(argv[1]) if len(argv) > 1 else 25)
w = T.Workload(4, n_entries=(BATCH * nb) // 2 + 200_000, n_res=1_000_000)
ev = np.array(w.events[:BATCH * nb], dtype=A.EVENT_DTYPE, copy=True)
assert len(ev) == BATCH * nb, "trace too short"
out = {"batch_events": BATCH, "batches": nb, "call": "sg_submit_ex (C4-ext)" if use_ext else "sg_submit (C4)"}
words = {}
for track in (False, True):
    eng = E.Engine(max_resources=1 << 20, max_slot_chain_size=0, status_ring_log2=27, max_batch_events=BATCH,
                   aux_node_capacity=(1 << 24) if use_ext else (1 << 16))
    w.install(eng)
    ext = None
    if use_ext:
        io, ic = w.intern_names(eng, 16, 4)
        ext = T.ext_for(ev, io, ic, seed=T.SEED_BASE + 61)
    if track:
        eng.track_inbound(True)
    ms, dec, decide_ms = [], [], []
    for i in range(nb):
        a, b = i * BATCH, (i + 1) * BATCH
        t = time.perf_counter()
        dec.append(eng.submit(ev[a:b]) if ext is None else eng.submit_ex(ev[a:b], ext[a:b]))
        ms.append((time.perf_counter() - t) * 1e3)
        decide_ms.append(eng.timings()[1])
    words[track] = np.concatenate(dec)
    leg = {"ms_per_batch": round(float(np.mean(ms[1:])), 3), "ms_batches": [round(x, 3) for x in ms],
           "decide_ms_per_batch": round(float(np.mean(decide_ms[1:])), 3)}
    if track:
        parts, visited, updates = eng.inbound_last()
        leg["last_batch"] = {"partials": parts, "records_visited": visited, "updates_counted": updates}
        leg["cur_thread_num"] = eng.read_inbound_node()["thread"]
    out["tracking_on" if track else "tracking_off"] = leg
    eng.close()
out["decisions_equal"] = bool(np.array_equal(words[False], words[True]))
out["decide_ms_added"] = round(out["tracking_on"]["decide_ms_per_batch"] - out["tracking_off"]["decide_ms_per_batch"], 3)
out["ms_added"] = round(out["tracking_on"]["ms_per_batch"] - out["tracking_off"]["ms_per_batch"], 3)
print(json.dumps(out))
