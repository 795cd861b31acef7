"""(CPU, oracle only) The traces of tests/test_gpu_preblocked.py reach what its cases are about.

The device tests compare with the oracle; these conditions keep them from being vacuous.  They are computed from
the oracle's decisions and the traces alone:
  * >= 50 words of status 6 on segments of each owner class (by the segment lengths the pinned bins of
    test_gpu_counts.OWNERS / BIN_MODES / HOT_BINS send to the one-wave, 256-, 512- and 1,024-lane owners);
  * >= 10 flagged ENTRYs with word 4 in the mix case (the param rule blocks first);
  * >= 10 EXITs / TRACEs naming a pre-blocked ENTRY of their own batch, and >= 10 naming one of an earlier batch;
  * a flagged run longer than two tiles of the widest owner (2 x 1,024 positions) that spans a 500 ms bucket edge;
  * a flagged zero-count ENTRY between two BLOCK_FLOW words of its resource inside one 500 ms bucket (ZERO traces);
  * >= 200 entries the authority rules block that the caller did not flag;
  * the placement trace keeps every segment under 5,000 events (SG_UBLK=0 walks it with one lane).
"""
import numpy as np
import pytest

import preblocked_util as P
from sentinel_amd import _abi as A

ENTRY = A.EV_ENTRY
# the traces and mixes test_gpu_preblocked.py runs
CASES = [("c2", "MIXED"), ("c3", "MIXED"), ("c4", "MIXED"), ("c2", "ZERO"), ("c3", "ZERO"), ("c4", "ZERO"),
         ("c2hot", "MIXED"), ("c4hot", "MIXED"), ("c2hot", "ZERO"), ("c4hot", "ZERO")]
# segment lengths by owner under the "coop" / "skip" bins (J1 <= 40 < J4 <= 400 < J8 / J16) and HOT_BINS (J4 <= 2000)
CLASSES = {"J1": (0, 40), "J4": (40, 400), "J4hot": (400, 2000), "wide": (2000, 1 << 31)}


def _status6_by_class(ref):
    """Words of status 6 per owner class of the segment they lie in."""
    ev, st = ref.ev, ref.do & 0xFF
    out = dict.fromkeys(CLASSES, 0)
    for a, b in zip(ref.cuts[:-1], ref.cuts[1:]):
        cnt = np.bincount(ev["res_id"][a:b], minlength=ref.w.n_res)
        six = np.bincount(ev["res_id"][a:b][st[a:b] == A.BLOCK_UPSTREAM], minlength=ref.w.n_res)
        for k, (lo, hi) in CLASSES.items():
            out[k] += int(six[(cnt > lo) & (cnt <= hi)].sum())
    return out


@pytest.mark.parametrize("trace,mix", CASES)
def test_flagged_traces_reach_their_cases(trace, mix):
    ref = P.reference(trace, mix)
    ev, st = ref.ev, ref.do & 0xFF
    ent = ev["kind"] == ENTRY
    assert ref.mask.sum() > 0.08 * ent[:ref.cuts[2]].sum() and not ref.mask[ref.cuts[2]:].any()
    assert (st[ref.mask] == A.BLOCK_UPSTREAM).all()  # (no param rules here: the flag always decides)
    by_class = _status6_by_class(ref)
    hot = trace.endswith("hot")
    for k, n in by_class.items():  # the 12-resource traces hold long segments only
        assert n >= 50 or (hot and k != "wide"), (trace, mix, by_class)
    same, earlier = P.named_preblocked(ev, ref.do, ref.cuts, ref.mask)
    assert same >= 10 and earlier >= 10, (same, earlier)
    # the runs: on the hottest resource of each flagged batch, longer than two tiles of the widest owner, over an edge
    for k in (0, 1):
        a, b = int(ref.cuts[k]), int(ref.cuts[k + 1])
        res = int(np.argmax(np.bincount(ev["res_id"][a:b], minlength=ref.w.n_res)))
        length, spans = P.longest_run(ev, a, b, res, ref.mask)
        assert length > 2 * P.WIDEST and spans, (trace, k, res, length, spans)
    # the third batch: no flag, and the marked hot resources are still there (stickiness)
    assert len(P.marked_segments(ref, 2, 2000)) >= 1
    if mix == "ZERO":
        assert (ref.mask & (ev["count"] == 0)).sum() >= 10
        assert P.zero_between_flow_blocks(ev, ref.do, ref.mask, stop=1) >= 1
    else:
        assert (st[ent] == A.BLOCK_FLOW).sum() > 10_000 and (st[ent] == A.PASS).sum() > 1_000


def test_mix_trace_reaches_param_first():
    ref = P.mix_reference()
    w4 = w6 = named = 0
    for ev, do, m in zip(ref.batches, ref.do, ref.masks):
        st = do & 0xFF
        w4 += int((m & (st == A.BLOCK_PARAM)).sum())
        w6 += int((m & (st == A.BLOCK_UPSTREAM)).sum())
        assert (st[m] != A.PASS).all() and np.isin(st[m], (A.BLOCK_PARAM, A.BLOCK_UPSTREAM)).all()
    assert w4 >= 10 and w6 >= 50, (w4, w6)
    for k in (0, 1):  # x0: one long run over a bucket edge in each flagged batch
        ev = ref.batches[k]
        length, spans = P.longest_run(ev, 0, len(ev), 0, ref.masks[k])
        assert length > 2 * P.WIDEST and spans, (k, length, spans)
    assert not ref.masks[2].any()
    # EXITs across batches name flagged ENTRYs (global references)
    allev = np.concatenate(ref.batches)
    cuts = np.cumsum([0] + [len(e) for e in ref.batches])
    same, earlier = P.named_preblocked(allev, np.concatenate(ref.do), cuts, np.concatenate(ref.masks))
    assert same >= 10 and earlier >= 10, (same, earlier)
    assert any(v > 0 for v in ref.threads[0])  # thread-count maps are live


def test_authority_trace_reaches_status_7():
    ref = P.authority_reference()
    st = ref.do & 0xFF
    assert (ref.blk & ~ref.caller & (st == A.BLOCK_UPSTREAM)).sum() >= 200
    assert (ref.blk & ref.caller).sum() >= 10
    assert ((ref.want & 0xFF) == A.BLOCK_AUTHORITY).sum() >= 200 and ((ref.want & 0xFF) == A.BLOCK_UPSTREAM).sum() >= 200
    # WHITE and BLACK lists both block and both let entries through on the hot resources
    for k, res in enumerate(ref.hot[:4]):
        m = (ref.ev["kind"] == ENTRY) & (ref.ev["res_id"] == res)
        assert 10 <= ref.blk[m].sum() < m.sum(), (k, res)
    # the PX_ORIGIN resource sees pre-blocked entries and its origin rule decides some
    m = (ref.ev["kind"] == ENTRY) & (ref.ev["res_id"] == ref.origin_res)
    assert ref.mask[m].sum() >= 10 and (st[m] == A.BLOCK_FLOW).sum() >= 10
    assert sum(1 for v in ref.origin_nodes.values() if v is not None) >= 16


def test_placement_trace_is_short_enough_for_one_lane():
    ref = P.reference("c4flat", "MIXED")
    for a, b in zip(ref.cuts[:-1], ref.cuts[1:]):
        assert np.bincount(ref.ev["res_id"][a:b]).max() < 5000
    marked = P.marked_segments(ref, 0, 128)
    assert sum(1 for n in marked.values() if n <= 1024) >= 10 and sum(1 for n in marked.values() if n > 1024) >= 1
