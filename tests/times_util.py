"""Traces whose clock idles, sits on bucket edges and spans up to 2^31 - 1 ms in one batch, and their oracle results
(helper of test_gpu_times.py).

tracegen's traces start at a multiple of 60 s and, but for c1 / c4long, end less than a second later.  with_times()
sends the timestamps of a finished trace through a monotone non-decreasing map, so the submission order stays the time
order and every EXIT / TRACE still follows its ENTRY; everything else (the RT in aux included: it is input data, not
derived from ts) stays.  reference() replays such a trace through the oracle once per process, as counts_util does.
"""
import functools

import numpy as np

import counts_util as U
import pyoracle as O
from sentinel_amd import _abi as A

T0 = U.T0
PHASE = 137  # added last: batch origins sit mid-bucket, (t / 500) % 2 and (t / 1000) % 60 start out of phase
SPAN_MAX = 0x7FFFFFFF  # the largest dt (last event - first event of one batch, ms) sg_submit accepts
GAP_CYCLE = (499, 500, 501, 999, 1000, 1001, 1500, 59_500, 60_000, 60_001, 61_000, 120_000, 3_600_000)
FAR_GAPS = (2_592_000_000, 1 << 31)  # 30 days at the second batch boundary, 2^31 ms at the third
MODES = ("GAPS", "LONG", "FAR")


def edge_snap(ts):
    """EDGE: every second 500 ms bucket collapses onto its first or its last millisecond."""
    b = ts // 500
    return np.where(b % 4 == 1, b * 500, np.where(b % 4 == 3, b * 500 + 499, ts))


def gap_positions(cuts):
    """Each batch boundary and four points inside each batch [a, e): a + (e - a) * k // 5, k = 0..4, but position 0
    (distinct positions, ascending: the short batches of the small-call cycle give fewer than five)."""
    pos = {int(a + (e - a) * k // 5) for a, e in zip(cuts[:-1], cuts[1:]) for k in range(5)}
    pos.discard(0)
    return sorted(pos)


def with_times(events, cuts, mode):
    """A copy of the trace with ts warped: the idle gaps of GAP_CYCLE at gap_positions(cuts) in turn (everything from
    a position on moves by its gap), EDGE on the result, then per mode
      LONG: one more gap at the middle of the last batch, sized so that the batch's last event is exactly SPAN_MAX ms
            after its first;
      FAR:  FAR_GAPS at cuts[1] and cuts[2] (legal: the span limit is per batch);
    and PHASE last.  (EDGE before the gaps would snap 0.25 % of c2's ENTRYs: test_times_trace_shape wants a fifth.)"""
    assert mode in MODES
    ev = np.array(events, dtype=A.EVENT_DTYPE, copy=True)
    n = len(ev)
    step = np.zeros(n, dtype=np.int64)  # step[i]: what event i and all later ones move by
    for k, p in enumerate(gap_positions(cuts)):
        step[p] += GAP_CYCLE[k % len(GAP_CYCLE)]
    # EDGE after the gaps: the dense traces' ENTRYs all lie in their first 400 ms, one bucket; the gaps spread them
    # over many, and those are what collapses (a gap never shrinks by more than 998 ms: the map stays monotone)
    ts = edge_snap(ev["ts"].astype(np.int64) + np.cumsum(step))
    if mode == "FAR":
        assert len(cuts) >= 4
        far = np.zeros(n, dtype=np.int64)
        far[cuts[1]] = FAR_GAPS[0]
        far[cuts[2]] = FAR_GAPS[1]
        ts = ts + np.cumsum(far)
    if mode == "LONG":
        a, e = int(cuts[-2]), int(cuts[-1])
        mid = a + (e - a) // 2
        assert a < mid < e
        more = SPAN_MAX - int(ts[e - 1] - ts[a])
        assert more > 0
        ts[mid:] += more
    ev["ts"] = ts + PHASE
    return ev


sample = U.sample
hot_values = U.hot_values


def reference(name, mode, batches=3, snapshots=False):
    """The trace `name` warped by `mode`, replayed through the oracle in `batches` (once per process)."""
    return _reference(name, mode, batches, snapshots)


@functools.lru_cache(maxsize=None)
def _reference(name, mode, batches, snapshots):
    w = U.workload(name)
    r = U.Ref()
    r.w = w
    r.cuts = U.cuts_of(len(w.events), batches)
    r.ev = with_times(w.events, r.cuts, mode)
    r.t_end = int(r.ev["ts"][-1])
    orc = O.Oracle(max_slot_chain_size=0)
    w.install(orc)
    r.do = np.concatenate([orc.submit(r.ev[a:b]) for a, b in zip(r.cuts[:-1], r.cuts[1:])])
    r.sample = sample(r.ev, w.n_res)
    r.nodes = {int(x): orc.read_node(int(x)) for x in r.sample}
    r.snapshots = {}
    if snapshots:
        for now in (r.t_end + 10, r.t_end + 1500, r.t_end + 70000):
            r.snapshots[now] = U.sorted_snapshot(orc.snapshot(now, cap=1 << 18))
    r.threads = []
    if name in U.PARAM_TRACES:  # last: the oracle's get moves the value in its LRU order
        r.threads = [(res, keys, [orc.param_thread_count(res, 0, k) for k in keys])
                     for res, keys in hot_values(r.ev, w.n_res)]
    orc.close()
    return r


sorted_snapshot = U.sorted_snapshot
entry_status = U.entry_status


# ---------------------------------------------------------------- the head owner's trace (test_gpu_head), warped
@functools.lru_cache(maxsize=None)
def head_reference(mode):
    import test_gpu_head as H
    spec = H._spec()
    ev0, cuts = H._trace(spec)
    r = U.Ref()
    r.names = ["head-%d" % i for i in range(len(spec))]
    r.rules = [A.flow_rule(n, **kw) for n, (kw, *_) in zip(r.names, spec)]
    r.cuts = cuts
    r.ev = with_times(ev0, cuts, mode)
    orc = O.Oracle(max_slot_chain_size=0)
    for n in r.names:
        orc.register(n)
    orc.load_flow_rules(r.rules)
    r.do = np.concatenate([orc.submit(r.ev[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
    r.nodes = [orc.read_node(i) for i in range(len(r.names))]
    orc.close()
    return r


# ---------------------------------------------------------------- toAddCount past 2^31 and 2^32; the strict > of the window
# ParamFlowChecker.passDefaultLocalCheck (ParamFlowChecker.java:160-185), durationInSec 1, burst 0: a value seen
# passTime > 1000 ms after its last refill gets toAddCount = (int) (passTime * tokenCount / 1000) tokens on top of
# what it had left; newQps = (rest + toAddCount > maxCount ? maxCount : rest + toAddCount) - acquire; < 0 blocks.
WRAP_T1 = 444_516_351  # batch 1 starts this long after batch 0, batch 2 (1 << 31) + 1 after batch 1: 30 days in all
WRAP_CASES = {
    # name: (rule count, [(batch, ms into the batch, acquire)], the verdicts derived by hand)
    # A: 30 idle days at 1000 / s: 2,592,000,000 * 1000 / 1000 = 2,592,000,000 is in (2^31, 2^32): the int is
    #    -1,702,967,296, 999 + that - 1 < 0: blocked, and again a millisecond later (lastAddTokenTime did not move)
    "A": (1000, [(0, 200, 1), (2, 200, 1), (2, 201, 1)], [A.PASS, A.BLOCK_PARAM, A.BLOCK_PARAM]),
    # B: 2^31 + 1 idle ms at 2000 / s: 2 * (2^31 + 1) = 2^32 + 2, the int is 2.  The first acquire of 1990 left 10
    #    tokens: 10 + 2 - 13 < 0 blocks (a saturating conversion would refill to 2000 and pass), 10 + 2 - 12 = 0 passes
    "B": (2000, [(1, 200, 1990), (2, 200, 13), (2, 200, 12)], [A.PASS, A.BLOCK_PARAM, A.PASS]),
    # C: 5 / s used up in one millisecond; at exactly 1000 ms passTime > 1000 is false and no token is left: blocked;
    #    at 1001 ms toAddCount = 5005 / 1000 = 5: passes
    "C": (5, [(1, 200, 1)] * 5 + [(1, 1200, 1), (1, 1201, 1)], [A.PASS] * 5 + [A.BLOCK_PARAM, A.PASS]),
}
WRAP_FILL = (0, 600, 9000)  # filler ENTRYs a batch: short segments, more than a lane bin holds, more than k_pq's narrow owner
WRAP_KEYS = {"A": 1, "B": 2, "C": 3}
WRAP_FILL_KEYS = 64  # distinct filler values (far below a map's 4,000: nothing is evicted), keys 100 ..


def wrap_names():
    """case x kind ("p": the param rule alone -- k_pq and the value-parallel passes, k_lane with SG_PQ=0; "m": a flow
    rule that never blocks beside it -- k_lite<true> for the short segments, k_jac with the pre / post passes for the
    long ones) x filler size."""
    return ["wrap-%s-%s-%d" % (c, kind, f) for c in WRAP_CASES for kind in "pm" for f in WRAP_FILL]


def wrap_rules():
    prules, frules = [], []
    for n in wrap_names():
        _, c, kind, _ = n.split("-")
        prules.append(A.param_rule(n, 0, WRAP_CASES[c][0]))
        if kind == "m":
            frules.append(A.flow_rule(n, 1e9))
    return prules, frules


def wrap_trace():
    """(events, cuts, {resource name: indices of its case ENTRYs in order})."""
    starts = (T0 + PHASE, T0 + PHASE + WRAP_T1, T0 + PHASE + WRAP_T1 + (1 << 31) + 1)
    rows = []  # (ts, order, res, key, count, case tag)
    for res, n in enumerate(wrap_names()):
        _, c, _, f = n.split("-")
        f = int(f)
        for b, t0 in enumerate(starts):
            for i in range(f):  # filler: spread over 1.4 s, round-robin over its values
                rows.append((t0 + i * 1400 // f, 0, res, 100 + (i + b) % WRAP_FILL_KEYS, 1, -1))
        for k, (b, ms, acq) in enumerate(WRAP_CASES[c][1]):
            rows.append((starts[b] + ms, 1 + k, res, WRAP_KEYS[c], acq, k))
    rows.sort(key=lambda x: (x[0], x[1], x[2]))
    ev = np.zeros(len(rows), dtype=A.EVENT_DTYPE)
    ev["ts"] = [x[0] for x in rows]
    ev["res_id"] = [x[2] for x in rows]
    ev["aux"] = [x[3] for x in rows]
    ev["count"] = [x[4] for x in rows]
    ev["kind"] = A.EV_ENTRY
    ev["flags"] = A.F_HAS_ARG
    cuts = np.searchsorted(ev["ts"], list(starts) + [1 << 62]).astype(np.int64)
    tag = np.asarray([x[5] for x in rows])
    at = {n: np.nonzero((ev["res_id"] == res) & (tag >= 0))[0] for res, n in enumerate(wrap_names())}
    return ev, cuts, at


@functools.lru_cache(maxsize=None)
def wrap_reference():
    r = U.Ref()
    r.names = wrap_names()
    r.ev, r.cuts, r.at = wrap_trace()
    orc = O.Oracle(max_slot_chain_size=0)
    for n in r.names:
        orc.register(n)
    prules, frules = wrap_rules()
    orc.load_flow_rules(frules)
    orc.load_param_rules(prules)
    r.do = np.concatenate([orc.submit(r.ev[a:b]) for a, b in zip(r.cuts[:-1], r.cuts[1:])])
    r.nodes = [orc.read_node(i) for i in range(len(r.names))]
    orc.close()
    return r


# ---------------------------------------------------------------- the span limit itself
SPAN_NAMES = ("span-q", "span-rl", "span-d")


def span_rules():
    flow = [A.flow_rule("span-q", 2),
            A.flow_rule("span-rl", 10, control_behavior=A.CONTROL_BEHAVIOR_RATE_LIMITER, max_queueing_time_ms=500)]
    degrade = [A.degrade_rule("span-d", 10, 2, grade=A.DEGRADE_GRADE_RT)]
    return flow, degrade


def span_batch(last_dt, base=0, t0=T0 + PHASE):
    """A few ENTRYs on the three resources at the batch's first millisecond t0 (the QPS rule blocks its third, the rate
    limiter queues, six slow calls trip the RT breaker), one more ENTRY on each last_dt ms later.  base: the global
    index of the batch's first event (an EXIT names its ENTRY by it)."""
    rows = [(t0, 0, A.EV_ENTRY, 0)] * 3 + [(t0, 1, A.EV_ENTRY, 0)] * 3
    d0 = len(rows)
    rows += [(t0, 2, A.EV_ENTRY, 0)] * 6
    rows += [(t0, 2, A.EV_EXIT, A.aux_exit(base + d0 + k, 200)) for k in range(6)]
    rows += [(t0, 2, A.EV_ENTRY, 0)] * 6  # the fifth check at that average RT opens the breaker
    rows += [(t0 + last_dt, r, A.EV_ENTRY, 0) for r in range(3)]
    return _rows(rows)


def span_next(base_t):
    """The batch after it: the same resources 1 ms and 700 ms after base_t."""
    return _rows([(base_t + d, r, A.EV_ENTRY, 0) for d in (1, 1, 700) for r in range(3)])


def span_wide(pos, n=4097):
    """n ENTRYs round-robin on the three resources; from position pos on they are 2^31 ms later."""
    ev = _rows([(T0 + PHASE, i % 3, A.EV_ENTRY, 0) for i in range(n)])
    ev["ts"][pos:] += SPAN_MAX + 1
    return ev


def _rows(rows):
    ev = np.zeros(len(rows), dtype=A.EVENT_DTYPE)
    ev["ts"] = [x[0] for x in rows]
    ev["res_id"] = [x[1] for x in rows]
    ev["kind"] = [x[2] for x in rows]
    ev["aux"] = [x[3] for x in rows]
    ev["count"] = 1
    return ev


@functools.lru_cache(maxsize=None)
def span_reference():
    """The accepted batch (last event at dt = SPAN_MAX) and the batch after it through the oracle."""
    r = U.Ref()
    a = span_batch(SPAN_MAX)
    r.parts = [a, span_next(int(a["ts"][-1]))]
    orc = O.Oracle(max_slot_chain_size=0)
    for n in SPAN_NAMES:
        orc.register(n)
    flow, degrade = span_rules()
    orc.load_flow_rules(flow)
    orc.load_degrade_rules(degrade)
    r.do = [orc.submit(p) for p in r.parts]
    r.nodes = [orc.read_node(i) for i in range(3)]
    orc.close()
    return r
