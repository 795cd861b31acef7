"""Parity with idle gaps, bucket-edge times and long batch spans on every decide owner.

tracegen's traces start at a multiple of 60 s and (but for c1 / c4long) end within a second, so the time-dependent
paths had seen one clock shape only: milliseconds advancing through consecutive 500 ms buckets from an aligned
origin.  Here the traces of the other suites get their timestamps warped (times_util.with_times: EDGE collapses every
second bucket onto its first or last millisecond, idle gaps of 499 ms .. 1 h at each batch boundary and four points
inside each batch, PHASE moves the origin to 137 ms past a bucket start; LONG stretches the last batch to the largest
span sg_submit accepts, 2^31 - 1 ms; FAR puts 30 days and 2^31 ms between batches) and run through the same owners
and switches.  What that reaches: LeapArray bucket resets and values()' strict > filter, getPreviousWindow for
WarmUp's previousPassQps, coolDownTokens, latestPassedTime + cost <= now, the degrade cut that ends after timeWindow,
the running 60 s exception sum and the minute-bucket prefetch, the borrow ring's future windows, ParamFlowChecker's
passTime * tokenCount / (durationInSec * 1000) with its (int) cast -- and the 32-bit batch-relative time every owner
decodes (SEv.dt, JEv.dt, k_tiny, HdSlot.dt, tdt, gdt) at its last value.

Every comparison is exact and against the oracle alone: all 32 bits of every decision word, the thread count, second
window and minute window of the 50 hottest and 300 random resources, the borrow ring of prioritized traces, the param
thread counts of param traces.  The hot traces (c2hot, c4hot) run in five batches: in three or four, the cycle's 1000
and 60,001 ms gaps fall on batch boundaries only, and the shape test wants each gap inside a hot segment.  The CPU test
at the end keeps the device tests from being vacuous.

What these tests found when they were written (all at the last values of the 32-bit batch-relative time, fixed in the
kernels; GAPS, FAR, the toAddCount wrap and the span refusals found nothing):
* decide.hip, k_jac's round machine (the open / frozen stretches that follow a hot segment round by round) kept the
  round's exclusive end as an int32 clamped to INT32_MAX and took "dt >= end" for "past the round": an event at
  dt = INT32_MAX, the last one LONG allows, was past every round, the machine opened its round again and again and the
  kernel did not return (c2 x LONG on the cooperative bins).  The end is now the round's last millisecond, inclusive.
* head.hip, found by reading the same arithmetic before its LONG cases ran: the statistics wave's bucket of an event,
  (dt + t0 % 500) / 500, and the bucket's end, start + 500, overflowed int32 within 499 ms of INT32_MAX once the batch
  origin sits mid-bucket (PHASE): the windows of a wrong bucket, or a bucket loop that claimed no event and did not
  end; the WarmUpRateLimiter round's "at or past the second's end" had the same clamped ">=" as k_jac; the rate
  limiter's lattice took t - (L - Q) in int32 with L - Q < 0 and t near INT32_MAX, and the frozen-round branch, which
  commits without verification, read the wrapped difference as "no lattice point: every ENTRY blocks".
"""
import numpy as np
import pytest

import times_util as TU
from sentinel_amd import _abi as A
from sentinel_amd import engine as E

gpu = pytest.mark.gpu

# decide-bin modes, as test_gpu_parity.BIN_MODES
BIN_MODES = {
    "default": {},
    "coop": {"SG_LANE_MAX": "0", "SG_J1_MAX": "40", "SG_J4_MAX": "400"},
    "lane": {"SG_DEBUG_FLAGS": "2"},
    "skip": {"SG_LANE_MAX": "0", "SG_J1_MAX": "40", "SG_J4_MAX": "400", "SG_SKIP_MIN": "16"},
}
HOT_BINS = {"SG_LANE_MAX": "0", "SG_J1_MAX": "40", "SG_J4_MAX": "2000"}  # test_frozen_skip_hot_resources
# one owner width for every cooperative segment, and the one-lane-per-segment kernel
OWNERS = {
    "J1": {"SG_LANE_MAX": "0", "SG_J1_MAX": "1000000000"},
    "J4": {"SG_LANE_MAX": "0", "SG_J1_MAX": "40", "SG_J4_MAX": "1000000000"},
    "J16": {"SG_LANE_MAX": "0", "SG_J1_MAX": "40", "SG_J4_MAX": "2000"},
    "lane": {"SG_DEBUG_FLAGS": "2"},
}
HOT_BATCHES = 5
SMALL_ENVS = [{"SG_TINY": "1"}, {"SG_TINY": "0"}, {"SG_RADIX_BELOW": "0"}]
SMALL_IDS = ["tiny", "no_tiny", "no_radix"]


def _setenv(monkeypatch, *envs):
    for env in envs:
        for k, v in env.items():
            monkeypatch.setenv(k, v)


@pytest.fixture(params=sorted(BIN_MODES))
def bin_mode(request, monkeypatch):
    _setenv(monkeypatch, BIN_MODES[request.param])
    return request.param


def _same_words(dg, do, ev):
    bad = np.nonzero(dg != do)[0]
    if len(bad):
        i = bad[0]
        raise AssertionError("decision mismatch at event %d (%s): gpu=%08x oracle=%08x; %d mismatches"
                             % (i, ev[i], dg[i], do[i], len(bad)))


def _same_node(g, o, what, borrow=False):
    assert g["has_chain"] == o["has_chain"], what
    assert g["thread"] == o["thread"], (what, g["thread"], o["thread"])
    np.testing.assert_array_equal(g["second"][:2], o["second"][:2], err_msg="second window of %s" % (what,))
    np.testing.assert_array_equal(g["minute"], o["minute"], err_msg="minute window of %s" % (what,))
    if borrow:
        np.testing.assert_array_equal(g["borrow"][:2], o["borrow"][:2], err_msg="borrow ring of %s" % (what,))


def _run(ref, borrow=False, **engine_kw):
    """The reference's trace through a fresh engine, batch for batch; everything compared with the oracle's."""
    w = ref.w
    engine_kw.setdefault("max_resources", max(64, w.n_res))
    eng = E.Engine(max_slot_chain_size=0, status_ring_log2=24, **engine_kw)
    w.install(eng)
    dg = np.concatenate([eng.submit(ref.ev[a:b]) for a, b in zip(ref.cuts[:-1], ref.cuts[1:])])
    _same_words(dg, ref.do, ref.ev)
    for r in ref.sample:
        _same_node(eng.read_node(int(r)), ref.nodes[int(r)], "res %d" % r, borrow)
    for res, keys, want in ref.threads:
        got = [eng.param_thread_count(res, 0, k) for k in keys]
        assert got == want, ("thread counts of res %d" % res, got, want)
    return eng, dg


# ---------------------------------------------------------------- 1. flow and degrade owners, every bin mode
@gpu
@pytest.mark.parametrize("mode", TU.MODES)
@pytest.mark.parametrize("trace", ["c2", "c3", "c4"])
def test_flow_degrade_times(trace, mode, bin_mode):
    _run(TU.reference(trace, mode))[0].close()


@gpu
@pytest.mark.parametrize("trace", ["c2", "c4"])
def test_times_without_open_stretches(trace, monkeypatch):
    # the Jacobi iteration alone (debug flag 64 turns the all-pass open stretches off)
    _setenv(monkeypatch, BIN_MODES["coop"], {"SG_DEBUG_FLAGS": "64"})
    _run(TU.reference(trace, "GAPS"))[0].close()


# ---------------------------------------------------------------- 2. frozen-stretch skip across gaps
@gpu
@pytest.mark.parametrize("skip_min", ["16", "1000"])
@pytest.mark.parametrize("mode", ["GAPS", "LONG"])
@pytest.mark.parametrize("trace", ["c2hot", "c4hot"])
def test_frozen_skip_times(trace, mode, skip_min, monkeypatch):
    # a gap ends a frozen stretch (the next event opens another bucket's round) but must not end skipping
    _setenv(monkeypatch, HOT_BINS, {"SG_SKIP_MIN": skip_min})
    eng, _ = _run(TU.reference(trace, mode, batches=HOT_BATCHES))
    assert eng.spans_total() > 0
    eng.close()


# ---------------------------------------------------------------- 3. one owner width for everything
@gpu
@pytest.mark.parametrize("owner", sorted(OWNERS))
def test_owner_widths_long_span(owner, monkeypatch):
    _setenv(monkeypatch, OWNERS[owner])
    _run(TU.reference("c4hot", "LONG", batches=HOT_BATCHES))[0].close()


# ---------------------------------------------------------------- 4. the head owner
@gpu
@pytest.mark.parametrize("owner", ["head", "coop"])
@pytest.mark.parametrize("mode", ["GAPS", "LONG"])
def test_head_owner_times(mode, owner, monkeypatch):
    # test_gpu_head's spec and trace, its three batches warped; the owner on and off (debug flag 16384)
    _setenv(monkeypatch, {"SG_LANE_MAX": "0", "SG_J1_MAX": "40", "SG_J4_MAX": "2000"})
    if owner == "coop":
        monkeypatch.setenv("SG_DEBUG_FLAGS", "16384")
    ref = TU.head_reference(mode)
    eng = E.Engine(max_resources=256, max_slot_chain_size=0, status_ring_log2=24)
    assert list(eng.register_many(ref.names)) == list(range(len(ref.names)))
    eng.load_flow_rules(ref.rules)
    dg = np.concatenate([eng.submit(ref.ev[a:e]) for a, e in zip(ref.cuts[:-1], ref.cuts[1:])])
    _same_words(dg, ref.do, ref.ev)
    for r in range(len(ref.names)):
        _same_node(eng.read_node(r), ref.nodes[r], "head-%d" % r)
    eng.close()


# ---------------------------------------------------------------- 5. param owners
@gpu
@pytest.mark.parametrize("mode", TU.MODES)
def test_param_times(mode, bin_mode):
    _run(TU.reference("c5", mode))[0].close()


@gpu
def test_param_times_maps_evict():
    # 16 resources over 200k values: every map fills and evicts its LRU values (k_pq)
    _run(TU.reference("c5evict", "GAPS", batches=4))[0].close()


PARAM_SWITCHES = [None, "SG_PV", "SG_PVT", "SG_MIX", "SG_PQ"]


@gpu
@pytest.mark.parametrize("switch", PARAM_SWITCHES)
@pytest.mark.parametrize("mode", ["GAPS", "FAR"])
def test_mixed_rule_times(mode, switch, monkeypatch):
    # C6 (flow + degrade + param on every resource); each switch off once (SG_PV=0 k_pq's passes, SG_PVT=0 the serial
    # post pass, SG_MIX=0 / SG_PQ=0 one lane)
    if switch:
        monkeypatch.setenv(switch, "0")
    _run(TU.reference("c6", mode), param_table_log2=24)[0].close()


# ---------------------------------------------------------------- 6. the toAddCount wrap
WRAP_ENVS = {"default": {}, "lane": BIN_MODES["lane"], "coop": BIN_MODES["coop"], "SG_PV": {"SG_PV": "0"},
             "SG_PVT": {"SG_PVT": "0"}, "SG_MIX": {"SG_MIX": "0"}, "SG_PQ": {"SG_PQ": "0"}}


@gpu
@pytest.mark.parametrize("env", sorted(WRAP_ENVS))
def test_to_add_count_wrap(env, monkeypatch):
    # (int) (passTime * tokenCount / 1000) in (2^31, 2^32) and just above 2^32, and passTime == / > the window, on
    # segments of 1 - 7, 600 and 9,000 events of a param-only and a param + flow resource: k_pq narrow / wide with the
    # value-parallel passes (default) and without (SG_PV / SG_PVT), k_lite<true> and k_jac with the pre / post passes,
    # k_lane (SG_PQ / SG_MIX / the lane bins)
    _setenv(monkeypatch, WRAP_ENVS[env])
    ref = TU.wrap_reference()
    eng = E.Engine(max_resources=64, max_slot_chain_size=0, status_ring_log2=24, param_table_log2=20)
    assert list(eng.register_many(ref.names)) == list(range(len(ref.names)))
    prules, frules = TU.wrap_rules()
    eng.load_flow_rules(frules)
    eng.load_param_rules(prules)
    dg = np.concatenate([eng.submit(ref.ev[a:e]) for a, e in zip(ref.cuts[:-1], ref.cuts[1:])])
    _same_words(dg, ref.do, ref.ev)
    for r in range(len(ref.names)):
        _same_node(eng.read_node(r), ref.nodes[r], ref.names[r])
    eng.close()


# ---------------------------------------------------------------- 7. prioritized entries
@gpu
@pytest.mark.parametrize("trace,batches", [("prio1", 4), ("prio2", 3)])
def test_prioritized_times(trace, batches, bin_mode):
    # tryOccupyNext's future windows, addWaitingRequest / addOccupiedPass across gaps; the borrow ring compared
    ref = TU.reference(trace, "GAPS", batches=batches)
    eng, dg = _run(ref, borrow=True)
    if trace == "prio1":
        st = dg[ref.ev["kind"] == A.EV_ENTRY] & 0xFF
        assert (st == A.PASS_WAIT).sum() > 0
    eng.close()


# ---------------------------------------------------------------- 8. small synchronous calls
@gpu
@pytest.mark.parametrize("env", SMALL_ENVS, ids=SMALL_IDS)
def test_small_call_times(env, monkeypatch):
    # k_tiny, the radix group stage and the hot / cold group stage on batches of 1 .. 4,097 events
    _setenv(monkeypatch, env)
    _run(TU.reference("c4small", "GAPS", batches="cycle"))[0].close()


# ---------------------------------------------------------------- 9. origin and context nodes
@gpu
def test_ext_post_pass_times():
    # test_gpu_aux.test_ext_post_pass_parity's cfg = 4 trace and batches, warped: the aux post pass (aux.hip)
    import pyoracle as O
    import test_gpu_aux as X
    from sentinel_amd import tracegen as T
    n_res = 3000
    w = T.Workload(4, seed=T.SEED_BASE + 44, n_res=n_res, n_entries=400_000)
    cuts = np.linspace(0, len(w.events), 3).astype(np.int64)
    ev = TU.with_times(w.events, cuts, "GAPS")
    eng = E.Engine(max_resources=4096, max_slot_chain_size=0, status_ring_log2=24, aux_node_capacity=1 << 17)
    orc = O.Oracle(max_slot_chain_size=0)
    io, ic = X._install(w, eng, [orc])
    ext = T.ext_for(ev, io, ic, seed=5)
    dg = np.concatenate([eng.submit_ex(ev[a:b], ext[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
    do = np.concatenate([orc.submit_ex(ev[a:b], ext[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
    cnt = np.bincount(ev["res_id"], minlength=n_res)
    assert cnt.max() > 2 * 4096 and ((cnt > 256) & (cnt <= 4096)).sum() > 10  # every post-pass shape ran
    rng = np.random.default_rng(3)
    sample = np.unique(np.concatenate([np.argsort(-cnt)[:12], rng.choice(np.nonzero(cnt)[0], 60, replace=False)]))
    assert X._compare(eng, orc, ev, dg, do, n_res, io, ic, sample) > 300
    st = do[ev["kind"] == A.EV_ENTRY] & 0xFF
    assert (st == A.PASS).sum() > 1000 and (st == A.BLOCK_FLOW).sum() > 1000
    eng.close()
    orc.close()


# ---------------------------------------------------------------- 10. snapshot
@gpu
def test_snapshot_after_gaps():
    ref = TU.reference("c4", "GAPS", snapshots=True)
    eng, _ = _run(ref)
    assert len(ref.snapshots) == 3
    for now, want in ref.snapshots.items():
        np.testing.assert_array_equal(TU.sorted_snapshot(eng.snapshot(now, cap=1 << 18)), want)
    eng.close()


# ---------------------------------------------------------------- 11. the span limit itself
def _span_engine():
    eng = E.Engine(max_resources=64, max_slot_chain_size=0, status_ring_log2=24)
    assert list(eng.register_many(list(TU.SPAN_NAMES))) == [0, 1, 2]
    flow, degrade = TU.span_rules()
    eng.load_flow_rules(flow)
    eng.load_degrade_rules(degrade)
    return eng


def _span_submit(eng, parts, pipelined):
    if not pipelined:
        return [eng.submit(p) for p in parts]
    parts = [np.ascontiguousarray(p) for p in parts]
    outs = [np.zeros(len(p), dtype=np.uint32) for p in parts]
    for p, o in zip(parts, outs):  # both in flight
        eng.submit_ptr(p.ctypes.data, len(p), o.ctypes.data, sync=False)
    eng.sync()
    return outs


def _span_accepted(eng, pipelined):
    """The batch whose last event is SPAN_MAX ms after its first, and the batch after it: equal to the oracle."""
    ref = TU.span_reference()
    for p, dg, do in zip(ref.parts, _span_submit(eng, ref.parts, pipelined), ref.do):
        _same_words(dg, do, p)
    for r in range(3):
        _same_node(eng.read_node(r), ref.nodes[r], TU.SPAN_NAMES[r])


def _span_refused(eng, bad, pipelined):
    with pytest.raises(E.SentinelError) as ei:
        _span_submit(eng, [bad], pipelined)
    assert ei.value.code == A.SG_EINVAL and "span" in str(ei.value), str(ei.value)


SPAN_PATHS = SMALL_ENVS + [{}]
SPAN_IDS = SMALL_IDS + ["pipelined"]


@gpu
@pytest.mark.parametrize("env", SPAN_PATHS, ids=SPAN_IDS)
def test_span_limit_accepted(env, monkeypatch):
    _setenv(monkeypatch, env)
    eng = _span_engine()
    _span_accepted(eng, pipelined=not env)
    eng.close()


@gpu
@pytest.mark.parametrize("env", SPAN_PATHS, ids=SPAN_IDS)
def test_span_limit_refused_is_a_noop(env, monkeypatch):
    # last event at dt = 2^31: SG_EINVAL naming the span; then the accepted batch gives what a fresh engine gives (the
    # oracle never saw the refused one): words, windows, thread counts -- and the EXITs' references, which count
    # events from the engine's start, still name their ENTRYs
    _setenv(monkeypatch, env)
    eng = _span_engine()
    _span_refused(eng, TU.span_batch(TU.SPAN_MAX + 1), pipelined=not env)
    _span_accepted(eng, pipelined=not env)
    eng.close()


@gpu
def test_span_limit_refused_behind_a_batch_in_flight():
    # two batches in flight: the accepted batch queued first, the oversized one behind it.  The second submit takes the
    # first batch's verdict and returns; the oversized batch's error surfaces at the next call (sg_sync), which still
    # finishes the first batch: its words are the oracle's, and the batch after it is decided as if the refused one had
    # never been queued
    ref = TU.span_reference()
    eng = _span_engine()
    a = np.ascontiguousarray(ref.parts[0])
    bad = np.ascontiguousarray(TU.span_batch(TU.SPAN_MAX + 1, base=len(a), t0=int(a["ts"][-1]) + 1))
    out_a, out_bad = np.zeros(len(a), dtype=np.uint32), np.zeros(len(bad), dtype=np.uint32)
    eng.submit_ptr(a.ctypes.data, len(a), out_a.ctypes.data, sync=False)
    eng.submit_ptr(bad.ctypes.data, len(bad), out_bad.ctypes.data, sync=False)
    with pytest.raises(E.SentinelError) as ei:
        eng.sync()
    assert ei.value.code == A.SG_EINVAL and "span" in str(ei.value), str(ei.value)
    _same_words(out_a, ref.do[0], a)
    _same_words(eng.submit(ref.parts[1]), ref.do[1], ref.parts[1])
    for r in range(3):
        _same_node(eng.read_node(r), ref.nodes[r], TU.SPAN_NAMES[r])
    eng.close()


@gpu
@pytest.mark.parametrize("pos", [1, 2048, 4096])
@pytest.mark.parametrize("env", SPAN_PATHS, ids=SPAN_IDS)
def test_span_limit_refused_wide(env, pos, monkeypatch):
    # 4,097 events with the oversized step at the second, a middle and the last position
    _setenv(monkeypatch, env)
    eng = _span_engine()
    _span_refused(eng, TU.span_wide(pos), pipelined=not env)
    _span_accepted(eng, pipelined=not env)
    eng.close()


# ---------------------------------------------------------------- CPU: the traces reach what the cases are about
def _floor(st, statuses, floor, what):
    for s in statuses:
        assert int((st == s).sum()) >= floor, (what, s, np.bincount(st, minlength=8))


STATUSES = {
    "c2": (A.PASS, A.BLOCK_FLOW), "c3": (A.PASS, A.BLOCK_FLOW), "c4": (A.PASS, A.BLOCK_FLOW, A.BLOCK_DEGRADE),
    "c4hot": (A.PASS, A.BLOCK_FLOW, A.BLOCK_DEGRADE), "c5": (A.PASS, A.BLOCK_PARAM),
    "c6": (A.PASS, A.BLOCK_FLOW, A.BLOCK_DEGRADE, A.BLOCK_PARAM),
}
CASES = [(t, m, 3) for t in ("c2", "c3", "c4", "c5") for m in TU.MODES] + \
        [("c4hot", m, HOT_BATCHES) for m in ("GAPS", "LONG")] + [("c6", m, 3) for m in ("GAPS", "FAR")]


def _check_map(ev0, ev, cuts, mode):
    """with_times kept the order, every EXIT / TRACE after its ENTRY, and everything but ts."""
    ts = ev["ts"].astype(np.int64)
    assert (np.diff(ts) >= 0).all()
    for f in ("res_id", "count", "kind", "flags", "aux"):
        assert np.array_equal(ev0[f], ev[f])
    ref = (ev["aux"] & np.uint64(A.REF_NONE)).astype(np.int64)
    named = np.nonzero((ev["kind"] != A.EV_ENTRY) & (ref != A.REF_NONE) & (ref < len(ev)))[0]
    assert len(named) and (ref[named] < named).all() and (ts[ref[named]] <= ts[named]).all()
    spans = [int(ts[e - 1] - ts[a]) for a, e in zip(cuts[:-1], cuts[1:]) if e > a]
    assert max(spans) <= TU.SPAN_MAX
    if mode == "LONG":
        assert spans[-1] == TU.SPAN_MAX
    else:
        assert max(spans) < 1 << 27
    if mode == "FAR":
        assert ts[cuts[1]] - ts[cuts[1] - 1] > 1 << 31 and ts[cuts[2]] - ts[cuts[2] - 1] > 1 << 31


def test_times_trace_shape():
    """(CPU, oracle only) the warp is what it says, and every trace and mode above reaches the verdicts its case is
    meant to reach."""
    # the map: monotone, EXITs after their ENTRYs, LONG's last batch spans exactly 2^31 - 1 ms, FAR's boundaries exceed
    # 2^31 ms while no batch does
    for trace, mode, batches in CASES + [("c2hot", "LONG", HOT_BATCHES), ("c4small", "GAPS", "cycle")]:
        ref = TU.reference(trace, mode, batches=batches)
        _check_map(ref.w.events, ref.ev, ref.cuts, mode)
    for mode in ("GAPS", "LONG"):
        import test_gpu_head as H
        href = TU.head_reference(mode)
        _check_map(H._trace(H._spec())[0], href.ev, href.cuts, mode)

    # every gap of the cycle occurs inside some batch of the hot traces and splits a segment of more than 2,000 events
    # (EDGE moves either side of a gap by up to 499 ms, so the interval realised across a gap is its cycle value
    # snapped to bucket edges: `exact` collects the realised intervals)
    exact = {}
    for trace in ("c2hot", "c4hot"):
        ref = TU.reference(trace, "GAPS", batches=HOT_BATCHES)
        ts, res = ref.ev["ts"].astype(np.int64), ref.ev["res_id"]
        inside = set()
        exact[trace] = set()
        for k, p in enumerate(TU.gap_positions(ref.cuts)):
            gap = TU.GAP_CYCLE[k % len(TU.GAP_CYCLE)]
            assert gap - 998 <= ts[p] - ts[p - 1] <= gap + 1000
            exact[trace].add(int(ts[p] - ts[p - 1]))
            b = int(np.searchsorted(ref.cuts, p, side="right")) - 1
            a, e = int(ref.cuts[b]), int(ref.cuts[b + 1])
            if p == a:
                continue
            before, after = np.bincount(res[a:p], minlength=16), np.bincount(res[p:e], minlength=16)
            if ((before > 0) & (after > 0) & (before + after > 2000)).any():
                inside.add(gap)
        assert inside == set(TU.GAP_CYCLE), (trace, sorted(set(TU.GAP_CYCLE) - inside))
        # the intervals between two consecutive events of a hot trace include, exactly, a bucket + 1 ms, a second and
        # a minute with the millisecond on either side of each, one and two minutes and an hour
        assert exact[trace] >= {501, 999, 1000, 1001, 60_000, 60_001, 61_000, 120_000, 3_600_000}, (trace, exact[trace])
    # 499 and 500 ms exactly (the last millisecond of a bucket to the next bucket's, a bucket start to the next start)
    # are realised on the small-call trace, whose 130 gaps go round the cycle ten times
    ref = TU.reference("c4small", "GAPS", batches="cycle")
    ts = ref.ev["ts"].astype(np.int64)
    small = {int(ts[p] - ts[p - 1]) for p in TU.gap_positions(ref.cuts)}
    assert small >= {499, 500, 501, 999, 1000, 1001, 1500, 60_000, 60_001}, sorted(small)

    # edge snapping: at least a fifth of the ENTRYs on a snapped edge after PHASE, and some millisecond holds more than
    # 64 events of one resource
    for trace, mode, batches in CASES:
        ev = TU.reference(trace, mode, batches=batches).ev
        ent = ev["kind"] == A.EV_ENTRY
        on_edge = np.isin(ev["ts"][ent] % 500, (TU.PHASE, TU.PHASE - 1))
        assert on_edge.mean() >= 0.2, (trace, mode, on_edge.mean())
        _, per_ms = np.unique(ev["ts"].astype(np.int64) * (1 << 20) + ev["res_id"], return_counts=True)
        assert per_ms.max() > 64, (trace, mode, per_ms.max())

    # status floors, in every batch of FAR too
    for trace, mode, batches in CASES:
        ref = TU.reference(trace, mode, batches=batches)
        _floor(TU.entry_status(ref), STATUSES[trace], 1000, (trace, mode))
        for a, e in zip(ref.cuts[:-1], ref.cuts[1:]):
            if trace == "c3":  # words that carry a wait, in every batch
                assert int(((ref.do[a:e] >> 16) > 0).sum()) >= 1000, (trace, mode, int(a))
            if mode == "FAR":
                ent = ref.ev["kind"][a:e] == A.EV_ENTRY
                _floor(ref.do[a:e][ent] & 0xFF, STATUSES[trace], 1000, (trace, mode, int(a)))
    _floor(TU.entry_status(TU.reference("c2hot", "GAPS", batches=HOT_BATCHES)), (A.PASS, A.BLOCK_FLOW), 1000, "c2hot")
    _floor(TU.entry_status(TU.reference("c5evict", "GAPS", batches=4)), (A.PASS, A.BLOCK_PARAM), 1000, "c5evict")
    _floor(TU.entry_status(TU.reference("prio1", "GAPS", batches=4)), (A.PASS_WAIT,), 100, "prio1")
    _floor(TU.entry_status(TU.reference("prio2", "GAPS")), (A.PASS, A.BLOCK_FLOW, A.PASS_WAIT), 1000, "prio2")
    _floor(TU.entry_status(TU.reference("c4small", "GAPS", batches="cycle")), (A.PASS, A.BLOCK_FLOW), 1000, "c4small")
    for mode in ("GAPS", "LONG"):
        href = TU.head_reference(mode)
        for a, e in zip(href.cuts[:-1], href.cuts[1:]):  # in every batch
            ent = href.ev["kind"][a:e] == A.EV_ENTRY
            _floor(href.do[a:e][ent] & 0xFF, (A.PASS, A.BLOCK_FLOW), 1000, ("head", mode, int(a)))
            assert int(((href.do[a:e] >> 16) > 0).sum()) >= 1000, ("head", mode, int(a))

    # a breaker reopened across a gap: on c4 x GAPS, at every gap of at least 60 s, some resource's last ENTRY before
    # the gap is BLOCK_DEGRADE and its first ENTRY after it is PASS
    ref = TU.reference("c4", "GAPS")
    ts, res, st = ref.ev["ts"].astype(np.int64), ref.ev["res_id"], ref.do & 0xFF
    ent = np.nonzero(ref.ev["kind"] == A.EV_ENTRY)[0]
    long_gaps = np.nonzero(np.diff(ts) >= 60_000)[0] + 1
    assert len(long_gaps) >= 4
    for p in long_gaps:
        before, after = ent[ent < p][::-1], ent[ent >= p]
        rb, ib = np.unique(res[before], return_index=True)  # (first in reversed order: the last before the gap)
        ra, ia = np.unique(res[after], return_index=True)
        _, xb, xa = np.intersect1d(rb, ra, return_indices=True)
        reopened = (st[before[ib[xb]]] == A.BLOCK_DEGRADE) & (st[after[ia[xa]]] == A.PASS)
        assert reopened.sum() > 0, int(p)

    # the toAddCount wrap: the oracle says what ParamFlowChecker.java:160-185 gives by hand, on every resource
    ref = TU.wrap_reference()
    for n in ref.names:
        want = TU.WRAP_CASES[n.split("-")[1]][2]
        got = (ref.do[ref.at[n]] & 0xFF).tolist()
        assert got == list(want), (n, got, want)
    spans = [int(ref.ev["ts"][e - 1] - ref.ev["ts"][a]) for a, e in zip(ref.cuts[:-1], ref.cuts[1:])]
    assert len(spans) == 3 and max(spans) < 2000
    assert 1 << 31 < 2_592_000_000 * 1000 // 1000 < 1 << 32 and ((1 << 31) + 1) * 2000 // 1000 == (1 << 32) + 2
    seg = np.bincount(ref.ev["res_id"][ref.cuts[2]:], minlength=len(ref.names))
    assert (seg <= 8).sum() == 6 and ((seg > 256) & (seg <= 8192)).sum() == 6 and (seg > 8192).sum() == 6

    # the span limit: the accepted batch ends exactly SPAN_MAX after its start with all three resources there, the
    # QPS rule and the breaker block in it, the rate limiter queues, and the batch after it is decided on that state
    ref = TU.span_reference()
    a = ref.parts[0]
    assert int(a["ts"][-1] - a["ts"][0]) == TU.SPAN_MAX and set(a["res_id"][-3:].tolist()) == {0, 1, 2}
    st = ref.do[0] & 0xFF
    assert (st == A.BLOCK_FLOW).any() and (st == A.BLOCK_DEGRADE).any() and ((ref.do[0] >> 16) > 0).any()
    assert (st[-3:] == A.PASS).all() and ((ref.do[1] & 0xFF) == A.BLOCK_FLOW).any()
    bad = TU.span_batch(TU.SPAN_MAX + 1)
    assert int(bad["ts"][-1] - bad["ts"][0]) == 1 << 31
    for pos in (1, 2048, 4096):
        w = TU.span_wide(pos)
        assert len(w) == 4097 and int(w["ts"][pos] - w["ts"][pos - 1]) == 1 << 31 and (np.diff(w["ts"]) >= 0).all()
