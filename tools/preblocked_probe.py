"""What the cooperative route of pre-blocked ENTRYs buys: a C4 trace in batches of 2^22 events with 1 % of the ENTRYs
carrying SG_F_BLOCKED_UPSTREAM, timed with SG_UBLK=1 (a marked resource keeps its cooperative owner) and SG_UBLK=0
(the placement before: a marked resource is walked by one lane) on the same build.  Prints one JSON line: ms a batch
of either leg (the mean of the batches after the first, which sets the marks), their ratio, the hottest segment's
length and where it was decided.

usage: python tools/preblocked_probe.py [batches]
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
nb = int(sys.argv[1]) if len(sys.argv) > 1 else 4
w = T.Workload(4, n_entries=(BATCH * nb) // 2 + 200_000, n_res=1_000_000)
ev = np.array(w.events[:BATCH * nb], dtype=A.EVENT_DTYPE, copy=True)
assert len(ev) == BATCH * nb, "trace too short"
rng = np.random.default_rng(1)
flag = (ev["kind"] == A.EV_ENTRY) & (rng.random(len(ev)) < 0.01)
ev["flags"][flag] |= A.F_BLOCKED_UPSTREAM
# references past the end of the replayed prefix do not occur: an EXIT follows its ENTRY
hot = int(np.argmax(np.bincount(ev["res_id"][:BATCH])))
hot_len = int((ev["res_id"][BATCH:2 * BATCH] == hot).sum())
hot_flagged = bool(flag[:BATCH][ev["res_id"][:BATCH] == hot].any())
out = {"batch_events": BATCH, "batches": nb, "flagged_share": 0.01, "hottest_segment_events": hot_len,
       "hottest_resource_flagged_in_first_batch": hot_flagged}
words = {}
for ublk in ("1", "0"):
    os.environ["SG_UBLK"] = ublk  # (read once per engine)
    eng = E.Engine(max_resources=1 << 20, max_slot_chain_size=0, status_ring_log2=26, max_batch_events=BATCH)
    w.install(eng)
    ms, dec = [], []
    for i in range(nb):
        t = time.perf_counter()
        dec.append(eng.submit(ev[i * BATCH:(i + 1) * BATCH]))
        ms.append((time.perf_counter() - t) * 1e3)
    coop, lane, nwords = eng.preblocked_stats()
    words[ublk] = np.concatenate(dec)
    out["ublk%s" % ublk] = {"ms_per_batch": round(float(np.mean(ms[1:])), 3), "ms_batches": [round(x, 3) for x in ms],
                            "marked_segments_cooperative": coop, "marked_segments_lane": lane,
                            "words_written_ahead": nwords,
                            "hottest_segment_bin": "cooperative (J8 / J16)" if (coop and hot_flagged) else "lane"}
    eng.close()
out["decisions_equal"] = bool(np.array_equal(words["1"], words["0"]))
out["ratio_ublk0_over_ublk1"] = round(out["ublk0"]["ms_per_batch"] / out["ublk1"]["ms_per_batch"], 2)
print(json.dumps(out))
