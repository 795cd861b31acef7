"""Side tables only where a 500 ms bucket can hold a skip.

k_seg_bin marks a hot id for the side tables (forward links, bst[]) only if its segment's owner is a skipping one
(BIN_J4 / J8 / J16) and k_hot_bmax's upper bound of the id's events in any one 500 ms bucket exceeds that owner's
threshold (SG_SKIP_MIN * NW / 16); the segment carries SEG_TABS, and an owner without it never skips.  The bound is
taken at tile boundaries: a bucket's count widened by at most one 4,096-event tile on each side.

Seeded traces, SG_RADIX_BELOW=0 (every batch on the hot / cold stage), every batch above 4,096 events, at least three
batches (an engine's first batch has no hot ids).  Every decision, thread, the second and minute windows of every
touched resource against the oracle; the frozen span count and the marked hot ids batch by batch.

Thresholds: SG_SKIP_MIN=8000 on the 256-lane owner (J4) and SG_SKIP_MIN=4000 on the 512-lane one (J8) both give 2,000.
"""
import numpy as np
import pytest

import pyoracle as O
from sentinel_amd import _abi as A
from sentinel_amd import engine as E
from sentinel_amd import tracegen as T

gpu = pytest.mark.gpu

T0 = 1_700_000_000_000  # (a multiple of 500: batch-relative buckets are the engine's absolute ones)
TILE = 4096
THR = 2000
RES_A, RES_B, RES_C = 3, 1500, 1700  # the burst, the even one, the one that alternates
FILL = range(100, 400)


class Trace:
    """Groups of ENTRYs with their EXITs (and TRACEs), then one time-ordered event array."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.ts, self.res, self.kind, self.ref, self.rt = [], [], [], [], []
        self.n = 0

    def add(self, res, k, t_lo, t_hi, rt_lo, rt_hi, n_trace=0):
        """k ENTRYs of res at sorted uniform times in [t_lo, t_hi) ms of the trace, each with its EXIT rt in
        [rt_lo, rt_hi) ms later, the first n_trace of them with a TRACE in the EXIT's millisecond."""
        t = T0 + np.sort(self.rng.integers(t_lo, t_hi, k))
        d = self.rng.integers(rt_lo, rt_hi, k)
        ids = self.n + np.arange(k)
        self.ts += [t, t + d, t[:n_trace] + d[:n_trace]]
        self.res += [np.full(2 * k + n_trace, res)]
        self.kind += [np.full(k, A.EV_ENTRY), np.full(k, A.EV_EXIT), np.full(n_trace, A.EV_TRACE)]
        self.ref += [np.full(k, -1), ids, ids[:n_trace]]
        self.rt += [np.zeros(k, dtype=np.int64), d, np.zeros(n_trace, dtype=np.int64)]
        self.n += 2 * k + n_trace

    def events(self, batch_ms, n_batches):
        ts, res, kind, ref, rt = (np.concatenate(x).astype(np.int64) for x in (self.ts, self.res, self.kind, self.ref, self.rt))
        keep = ts < T0 + batch_ms * n_batches  # (an EXIT past the trace's end is dropped)
        assert keep[kind == A.EV_ENTRY].all()
        # event order: time, then ENTRY before the EXIT / TRACE of the same millisecond (an EXIT follows its ENTRY)
        order = np.lexsort((kind, ts))
        order = order[keep[order]]
        pos = np.full(len(ts), -1, dtype=np.int64)
        pos[order] = np.arange(len(order))
        ev = np.zeros(len(order), dtype=A.EVENT_DTYPE)
        ev["ts"] = ts[order]
        ev["res_id"] = res[order]
        ev["count"] = 1
        ev["kind"] = kind[order]
        r = ref[order]
        aux = np.full(len(order), A.REF_NONE, dtype=np.uint64)
        has = r >= 0
        aux[has] = pos[r[has]].astype(np.uint64)
        ex = ev["kind"] == A.EV_EXIT
        aux[ex] |= rt[order][ex].astype(np.uint64) << np.uint64(48)
        ev["aux"] = aux
        cuts = np.searchsorted(ev["ts"], T0 + batch_ms * np.arange(n_batches + 1))
        cuts[-1] = len(ev)
        return ev, cuts


def _widened(ev, cuts, res):
    """Per batch: (the most events of res in one 500 ms bucket, the same widened by one 4,096-event tile of the batch
    on each side of the bucket: no tile-boundary bound can exceed it)."""
    out = []
    for a, e in zip(cuts[:-1], cuts[1:]):
        b = ev[a:e]
        bkt = b["ts"] // 500
        mine = np.concatenate([[0], np.cumsum(b["res_id"] == res)])
        true = wide = 0
        for k in np.unique(bkt):
            i0, i1 = np.searchsorted(bkt, k), np.searchsorted(bkt, k, side="right")
            true = max(true, int(mine[i1] - mine[i0]))
            wide = max(wide, int(mine[min(len(b), i1 + TILE)] - mine[max(0, i0 - TILE)]))
        out.append((true, wide))
    return out


def _run(ev, cuts, flow):
    """Replays the batches on a fresh engine and a fresh oracle (C4's names; flow: (resource id, QPS) rules), compares
    them, returns per batch the engine's frozen span count and its marked hot ids."""
    assert (np.diff(cuts) > TILE).all()
    w = T.Workload(4, n_res=2048, n_entries=1000)
    eng = E.Engine(max_resources=2048, max_slot_chain_size=0, status_ring_log2=24)
    orc = O.Oracle(max_slot_chain_size=0)
    for x in (eng, orc):
        w.install(x)
        names = w.names()
        x.load_flow_rules([A.flow_rule(names[r], q) for r, q in flow])
    spans, marks, last = [], [], 0
    for b, (a, e) in enumerate(zip(cuts[:-1], cuts[1:])):
        dg, do = eng.submit(ev[a:e]), orc.submit(ev[a:e])
        bad = np.nonzero(dg != do)[0]
        assert not len(bad), ("batch", b, int(a + bad[0]), ev[a + bad[0]], hex(dg[bad[0]]), hex(do[bad[0]]), len(bad))
        s = eng.spans_total()
        spans.append(s - last)
        last = s
        marks.append(eng.hot_marked())
    for r in np.unique(ev["res_id"]):
        g, o = eng.read_node(int(r)), orc.read_node(int(r))
        assert g["thread"] == o["thread"], r
        np.testing.assert_array_equal(g["second"][:2], o["second"][:2], err_msg="second window of res %d" % r)
        np.testing.assert_array_equal(g["minute"], o["minute"], err_msg="minute window of res %d" % r)
    eng.close()
    orc.close()
    return spans, marks


def _env(monkeypatch, skip_min=8000, j4_max=65536, j1_max=None, flags=None):
    monkeypatch.setenv("SG_RADIX_BELOW", "0")
    monkeypatch.setenv("SG_SKIP_MIN", str(skip_min))
    monkeypatch.setenv("SG_J4_MAX", str(j4_max))  # (pinned bins: segments above SG_J1_MAX events on the 256-lane owner)
    if j1_max is not None:
        monkeypatch.setenv("SG_J1_MAX", str(j1_max))
    if flags is not None:
        monkeypatch.setenv("SG_DEBUG_FLAGS", str(flags))


# ---- 1. / 2. / 4. / 5. bursty against even: batches of 2 s (4 buckets).  A: 3,000 ENTRYs and their EXITs inside one
# bucket; B: 3,000 ENTRYs evenly over the 4 buckets; 300 short resources of 300 ENTRYs as filler (192k events a batch:
# a tile is ~45 ms, so B's bound stays below the threshold).  prev: A and B each end a batch with 30 ENTRYs whose EXITs
# fall into the next one.  c_burst: the batches in which C (3,000 ENTRYs, even otherwise) comes as one burst.
def _bursty(n_batches=3, prev=False, c_burst=None, seed=31):
    tr = Trace(seed)
    for b in range(n_batches):
        o = b * 2000
        tr.add(RES_A, 3000, o + 1000, o + 1150, 1, 300, n_trace=20)  # [1000, 1450) of the third bucket
        for q in range(4):
            tr.add(RES_B, 750, o + 500 * q, o + 500 * q + 500, 1, 200, n_trace=5)
        if prev:
            tr.add(RES_A, 30, o + 1960, o + 2000, 100, 300)
            tr.add(RES_B, 30, o + 1960, o + 2000, 100, 300)
        if c_burst is not None:
            if b in c_burst:
                tr.add(RES_C, 3000, o + 500, o + 650, 1, 300)
            else:
                for q in range(4):
                    tr.add(RES_C, 750, o + 500 * q, o + 500 * q + 500, 1, 200)
        for r in FILL:
            tr.add(r, 300, o, o + 2000, 1, 400, n_trace=15)
    return tr.events(2000, n_batches)


FLOW_AB = [(RES_A, 5), (RES_B, 5), (RES_C, 5)]
_cache = {}


def _case1_spans(monkeypatch):
    """(computed once, shared: cases 1, 2 and 4 compare against it)"""
    if "c1" not in _cache:
        _env(monkeypatch)
        ev, cuts = _bursty()
        _cache["c1"] = _run(ev, cuts, FLOW_AB)
    return _cache["c1"]


@gpu
def test_bursty_marked_even_not(monkeypatch):
    spans, marks = _case1_spans(monkeypatch)
    assert sum(spans) > 0
    assert marks == [0, 1, 1]  # no hot ids in the first batch; then A alone (B and the filler are hot and unmarked)
    assert spans[1] > 0 and spans[2] > 0  # A's stretches are skipped through the hot tables


@gpu
def test_skipping_unchanged_against_tables_everywhere(monkeypatch):
    ref = _case1_spans(monkeypatch)
    _env(monkeypatch, flags=32768)
    ev, cuts = _bursty()
    spans, marks = _run(ev, cuts, FLOW_AB)
    assert spans == ref[0]
    assert marks == [0, 0, 0]  # (nothing is marked where everything is built)


# ---- 3. edges of the bound: bursts of threshold - 1, threshold, threshold + 1 events in one bucket, 2 x threshold
# straddling a bucket boundary evenly (threshold in each: no skip, but no tile boundary separates the halves), and a
# second 2 x threshold burst inside one bucket, which does skip (the 256-lane owner leaves its round machine for the
# skip only when the record threshold + 1,024 positions on is still in the round, so a burst much shorter than that
# is streamed), each on its own resource; ~1,000 filler events.  14,000 events over 20 s: a tile spans several buckets,
# so every tile opens one.  A burst is all its resource has in a batch: its bound is the burst itself, tiles or not.
EDGE = {600: THR - 1, 601: THR, 602: THR + 1, 603: 2 * THR, 604: 2 * THR}
STRADDLE = 603


def _edges(seed=33):
    tr = Trace(seed)
    for b in range(3):
        o = b * 20000
        for j, (r, k) in enumerate(EDGE.items()):
            s = o + 2000 + 3000 * j  # (a bucket's start)
            if r == STRADDLE:
                tr.add(r, k // 4, s + 400, s + 450, 1, 50)
                tr.add(r, k // 4, s + 500, s + 550, 1, 50)
            else:
                tr.add(r, k // 2, s, s + 100, 1, 300, n_trace=k % 2)
        for r in range(100, 200):
            tr.add(r, 5, o, o + 20000, 1, 400)
    return tr.events(20000, 3)


@gpu
@pytest.mark.parametrize("owner", ["J4", "J8"])
def test_edges_of_the_bound(owner, monkeypatch):
    ev, cuts = _edges()
    flow = [(r, 5) for r in EDGE]
    kw = dict(skip_min=8000, j4_max=65536, j1_max=512) if owner == "J4" else dict(skip_min=4000, j4_max=1024, j1_max=512)
    _env(monkeypatch, flags=32768, **kw)
    ref, _ = _run(ev, cuts, flow)
    _env(monkeypatch, **kw)
    monkeypatch.delenv("SG_DEBUG_FLAGS")
    spans, marks = _run(ev, cuts, flow)
    assert spans == ref
    assert sum(spans) > 0  # (the 2 x threshold burst inside one bucket)
    assert marks == [0, 3, 3]  # threshold + 1 and both of 2 x threshold; not threshold - 1, not threshold


# ---- 4. duplicate EXITs: a second EXIT for a few ENTRYs of the last batch, at its end
def _with_dups(res):
    ev, cuts = _bursty()
    ref = (ev["aux"] & np.uint64(A.REF_NONE)).astype(np.int64)
    ex = np.nonzero((ev["kind"] == A.EV_EXIT) & (ev["res_id"] == res) & (ref >= cuts[2]) & (ref < len(ev)))[0]
    d = ev[ex[:: len(ex) // 10]].copy()
    d["ts"] = ev["ts"][-1]
    ev = np.concatenate([ev, d])
    cuts = cuts.copy()
    cuts[-1] = len(ev)
    return ev, cuts


@gpu
def test_duplicate_exits_in_unmarked_hot_id_keep_skipping(monkeypatch):
    ref = _case1_spans(monkeypatch)
    _env(monkeypatch)
    ev, cuts = _with_dups(RES_B)
    spans, marks = _run(ev, cuts, FLOW_AB)
    assert marks == [0, 1, 1]
    assert spans[2] > 0 and spans[:2] == ref[0][:2]  # B's links are not built: its duplicates do not stop A


@gpu
def test_duplicate_exits_in_marked_hot_id_stop_skipping(monkeypatch):
    ref = _case1_spans(monkeypatch)
    _env(monkeypatch)
    ev, cuts = _with_dups(RES_A)
    spans, marks = _run(ev, cuts, FLOW_AB)
    assert marks == [0, 1, 1]
    assert spans[2] == 0 and spans[:2] == ref[0][:2]  # BF_MULTI_LINK: that batch streams


# ---- 5. references into the batch before (RC_PREV -> BST_STATIC) in A and in B; C turns from unmarked to marked and back
@gpu
def test_prev_references_and_marks_that_change(monkeypatch):
    _env(monkeypatch)
    ev, cuts = _bursty(n_batches=4, prev=True, c_burst=(1, 3), seed=35)
    ref = (ev["aux"] & np.uint64(A.REF_NONE)).astype(np.int64)
    for r in (RES_A, RES_B):
        for k in (1, 2, 3):
            i = np.arange(cuts[k], cuts[k + 1])
            assert ((ev["res_id"][i] == r) & (ev["kind"][i] != A.EV_ENTRY) & (ref[i] < cuts[k])).any()
    spans, marks = _run(ev, cuts, FLOW_AB)
    assert marks == [0, 2, 1, 2]
    assert min(spans[1:]) > 0
    _env(monkeypatch, flags=32768)
    assert _run(ev, cuts, FLOW_AB)[0] == spans


# ---- 6. what the traces hold (no GPU): per resource the most events in one 500 ms bucket, and the same widened by one
# 4,096-event tile on each side, against the threshold
def test_traces_hold_what_the_gpu_cases_assert():
    ev, cuts = _bursty()
    assert (np.diff(cuts) > TILE).all()
    for true, wide in _widened(ev, cuts, RES_A):
        assert true > THR
    for true, wide in _widened(ev, cuts, RES_B):
        assert 1400 < true and wide <= THR
    for r in FILL:
        assert max(w for _, w in _widened(ev, cuts, r)) <= THR
    ev, cuts = _bursty(n_batches=4, prev=True, c_burst=(1, 3), seed=35)
    for r, above in ((RES_A, [1, 1, 1, 1]), (RES_B, [0, 0, 0, 0]), (RES_C, [0, 1, 0, 1])):
        for (true, wide), up in zip(_widened(ev, cuts, r), above):
            assert (true > THR) if up else (wide <= THR), (r, true, wide)
    ev, cuts = _edges()
    assert (np.diff(cuts) > TILE).all()
    nb = (ev["ts"][cuts[1] - 1] - ev["ts"][0]) // 500
    assert nb > 2 * (cuts[1] // TILE + 1)  # sparse: more buckets than tiles, a tile spans several
    for r, k in EDGE.items():
        for true, wide in _widened(ev, cuts, r):
            assert wide == k  # the burst is all the resource has: exact, whatever the tiles
            assert true == (k // 2 if r == STRADDLE else k)
    assert EDGE[600] <= THR and EDGE[601] <= THR and EDGE[602] > THR and EDGE[603] > THR and EDGE[604] > THR
