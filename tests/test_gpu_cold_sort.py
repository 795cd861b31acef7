"""The cold region of the hot / cold group stage: key layouts of the cold sort, and the side tables built on demand.

Cold sort (kernels.hip: the cold (key, index) pairs through stable 8-bit LSD passes over the bits of
max_resources - 1): keys that share their low 10 bits, a single crowded residue class mod 1024, and the key widths
around 11, 20 and 21 bits.  Side tables (forward links, bst[]): built only for the hot ids and the cold
1,024-position blocks of segments whose owner can skip frozen stretches (BIN_J4 / BIN_J8 / BIN_J16, marked by
k_seg_bin, which runs ahead of the record kernels); SG_DEBUG_FLAGS 32768 builds them everywhere.

Seeded traces, SG_RADIX_BELOW=0 (every batch on the hot / cold stage), batches of at least two 4,096-event tiles
(one tile is k_cold_small's).  An engine's first batch has no hot ids: all of it is cold.  Every decision, and the
second and minute windows of the touched resources, against the oracle.
"""
import numpy as np
import pytest

import pyoracle as O
from sentinel_amd import _abi as A
from sentinel_amd import engine as E
from sentinel_amd import tracegen as T

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000_000


def _trace(plan, seed):
    """plan: per batch (1 s of trace time each) {resource: ENTRYs}.  Every ENTRY gets its EXIT after 1..399 ms (so
    part of a batch's EXITs name ENTRYs of the batch before) and 5 % a TRACE just before it.  -> events, batch cuts"""
    rng = np.random.default_rng(seed)
    ts, res, kind, ref_of, rt = [], [], [], [], []
    for b, spec in enumerate(plan):
        for r, k in spec.items():
            t = T0 + b * 1000 + np.sort(rng.integers(0, 1000, k))
            d = rng.integers(1, 400, k)
            tr = rng.random(k) < 0.05
            base = len(ts)
            n = k + k + int(tr.sum())
            ts.extend(t.tolist() + (t + d).tolist() + (t[tr] + d[tr] - 1).tolist())
            res.extend([r] * n)
            kind.extend([A.EV_ENTRY] * k + [A.EV_EXIT] * k + [A.EV_TRACE] * int(tr.sum()))
            ref_of.extend([-1] * k + list(range(base, base + k)) + [base + j for j in np.nonzero(tr)[0]])
            rt.extend([0] * k + d.tolist() + [0] * int(tr.sum()))
    ts, res, kind, ref_of, rt = map(np.asarray, (ts, res, kind, ref_of, rt))
    # event order: time, then ENTRY before the EXIT / TRACE of the same millisecond (an EXIT follows its ENTRY)
    order = np.lexsort((kind, ts))
    pos = np.empty(len(order), dtype=np.int64)
    pos[order] = np.arange(len(order))
    ev = np.zeros(len(order), dtype=A.EVENT_DTYPE)
    ev["ts"] = ts[order]
    ev["res_id"] = res[order]
    ev["count"] = 1
    ev["kind"] = kind[order]
    ref = ref_of[order]
    aux = np.full(len(order), A.REF_NONE, dtype=np.uint64)
    has = ref >= 0
    aux[has] = pos[ref[has]].astype(np.uint64)
    ex = ev["kind"] == A.EV_EXIT
    aux[ex] |= rt[order][ex].astype(np.uint64) << np.uint64(48)
    ev["aux"] = aux
    cuts = np.searchsorted(ev["ts"], T0 + 1000 * np.arange(len(plan) + 1))
    cuts[-1] = len(ev)
    return ev, cuts


def _check(ev, cuts, max_resources, n_names, flow=None):
    """Replays the batches on a fresh engine and a fresh oracle (C4's names and rules over n_names resources; flow:
    (resource id, QPS) rules instead of C4's flow rules), compares them, returns the engine's frozen span count."""
    assert (np.diff(cuts) > 4096).all()  # at least two tiles a batch
    w = T.Workload(4, n_res=n_names, n_entries=1000)
    eng = E.Engine(max_resources=max_resources, max_slot_chain_size=0, status_ring_log2=24)
    orc = O.Oracle(max_slot_chain_size=0)
    for x in (eng, orc):
        w.install(x)
        if flow:
            names = w.names()
            x.load_flow_rules([A.flow_rule(names[r], q) for r, q in flow])
    for b, (a, e) in enumerate(zip(cuts[:-1], cuts[1:])):
        dg, do = eng.submit(ev[a:e]), orc.submit(ev[a:e])
        bad = np.nonzero(dg != do)[0]
        assert not len(bad), ("batch", b, int(a + bad[0]), ev[a + bad[0]], hex(dg[bad[0]]), hex(do[bad[0]]), len(bad))
    for r in np.unique(ev["res_id"]):
        g, o = eng.read_node(int(r)), orc.read_node(int(r))
        assert g["thread"] == o["thread"], r
        np.testing.assert_array_equal(g["second"][:2], o["second"][:2], err_msg="second window of res %d" % r)
        np.testing.assert_array_equal(g["minute"], o["minute"], err_msg="minute window of res %d" % r)
    spans = eng.spans_total()
    eng.close()
    orc.close()
    return spans


# ---- 1. few high bits, shared low bits, unused residues: 12-bit keys, r / r + 1024 / r + 2048 / r + 3072 interleaved in
# time, no resource congruent to 7 mod 1024; half of them stay below the hot threshold (64 events), so the second and
# third batch keep cold events whose EXITs and TRACEs name ENTRYs of the batch before
def _shared_low_bits():
    lows = list(range(8, 48))
    plan = []
    for b in range(3):
        spec = {}
        for j, r in enumerate(lows):
            for hi in range(4):
                spec[r + 1024 * hi] = 20 if (j + hi + b) % 2 else 100
        plan.append(spec)
    ev, cuts = _trace(plan, seed=21)
    assert not (ev["res_id"] % 1024 == 7).any()
    assert ((ev["kind"] != A.EV_ENTRY) & (ev["aux"] & np.uint64(A.REF_NONE) < cuts[1]) &
            (np.arange(len(ev)) >= cuts[1])).any()  # references across the first batch boundary
    return ev, cuts


def test_shared_low_bits(monkeypatch):
    monkeypatch.setenv("SG_RADIX_BELOW", "0")
    ev, cuts = _shared_low_bits()
    _check(ev, cuts, 4096, 4096)


# ---- 6. the same trace with SG_DEBUG_FLAGS 32768: the side tables everywhere
def test_shared_low_bits_tables_everywhere(monkeypatch):
    monkeypatch.setenv("SG_RADIX_BELOW", "0")
    monkeypatch.setenv("SG_DEBUG_FLAGS", "32768")
    ev, cuts = _shared_low_bits()
    _check(ev, cuts, 4096, 4096)


# ---- 2. one crowded residue class: 300 resources congruent to 5 mod 1024 of about 120 events each, ~36k events (several
# tiles) in one residue class of the low 10 key bits, every other one empty
def test_one_crowded_residue_class(monkeypatch):
    monkeypatch.setenv("SG_RADIX_BELOW", "0")
    ids = [5 + 1024 * j for j in range(300)]
    ev, cuts = _trace([{r: 66 for r in ids}, {r: 66 for r in ids[::2]}], seed=22)
    assert (ev["res_id"] % 1024 == 5).all() and cuts[1] > 32768
    _check(ev, cuts, 1 << 20, ids[-1] + 1)


# ---- 3. width edges: 11-bit keys (two passes), 20-bit and 21-bit keys (three)
@pytest.mark.parametrize("max_resources", [2048, 1 << 20, (1 << 20) + 1])
def test_key_width_edges(max_resources, monkeypatch):
    monkeypatch.setenv("SG_RADIX_BELOW", "0")
    rng = np.random.default_rng(23)
    ids = np.sort(rng.choice(2048, 150, replace=False))
    plan = [{int(r): int(k) for r, k in zip(ids, rng.integers(5, 90, len(ids)))} for _ in range(2)]
    ev, cuts = _trace(plan, seed=24)
    _check(ev, cuts, max_resources, 2048)


# ---- 4. / 5. a cold segment that skips: the first batch (all cold) holds two resources of 6,000 ENTRYs each under a
# QPS rule of 5 (long frozen stretches; 12k events: a cooperative owner) and 300 short resources (k_lite's)
LONG = (3, 1500)


def _skip_trace(dup):
    plan = [{**{r: 6000 for r in LONG}, **{r: 12 for r in range(100, 400)}}]
    ev, cuts = _trace(plan, seed=25)
    if dup:  # a second EXIT for a few ENTRYs of short resources, at the end of the batch.  Resources 200 .. 299:
        # in the cold region's key order their segments lie thousands of positions from the two long ones, so they
        # share no 1,024-position block with them (a marked block gets its neighbours' links too)
        ex = np.nonzero((ev["kind"] == A.EV_EXIT) & (ev["res_id"] >= 200) & (ev["res_id"] < 300))[0]
        d = ev[ex[:: len(ex) // 20]].copy()
        d["ts"] = ev["ts"][-1]
        ev = np.concatenate([ev, d])
        cuts = np.array([0, len(ev)])
    return ev, cuts


def test_cold_segment_skips(monkeypatch):
    monkeypatch.setenv("SG_RADIX_BELOW", "0")
    monkeypatch.setenv("SG_SKIP_MIN", "16")
    ev, cuts = _skip_trace(False)
    assert _check(ev, cuts, 2048, 2048, flow=[(r, 5) for r in LONG]) > 0  # the cold tables exist where an owner skips


def test_duplicate_exits_in_short_segments_keep_skipping(monkeypatch):
    # BF_MULTI_LINK protects the skipping owners' links only: duplicates inside k_lite's segments do not raise it
    monkeypatch.setenv("SG_RADIX_BELOW", "0")
    monkeypatch.setenv("SG_SKIP_MIN", "16")
    ev, cuts = _skip_trace(True)
    assert _check(ev, cuts, 2048, 2048, flow=[(r, 5) for r in LONG]) > 0
