"""Parity with acquire, exit and trace counts other than 1 on every decide owner.

tracegen emits count = 1 everywhere, so a kernel that counted ENTRYs where it should sum their counts, or that wrapped
a 32-bit partial sum, would pass the unit-count suites.  Here the traces of those suites get their counts redrawn
(counts_util.with_counts: MIXED 1/2/3/7, ZERO with 2 % zero acquires, BIG with 2 % acquires of 65,535; EXITs release
their ENTRY's count unless told otherwise) and run through the same owners and switches; one resource takes 70,000 and
300,000 acquires of 65,535 inside one 500 ms bucket, so its pass / block sums exceed 2^32.  Reference: the counts of
SphU.entry(name, type, count, args) reach DefaultController.canPass(node, acquireCount, prioritized)
(DefaultController.java:49-81), StatisticNode.tryOccupyNext / addWaitingRequest / addOccupiedPass
(StatisticNode.java:293-341), ParamFlowChecker.passDefaultLocalCheck / passThrottleLocalCheck (acquireCount against the
token count), StatisticSlot's addPassRequest(count) / increaseBlockQps(count) (StatisticSlot.java:54-173),
Entry.exit(count) -> addRtAndSuccess(rt, count) and Tracer.trace(t, count) -> increaseExceptionQps(count).

Every comparison is exact: all 32 bits of every decision word (status, rule slot, wait), the thread count, the second
window, the minute window and -- for prioritized entries -- the borrow ring of the 50 hottest and 300 random resources.
The CPU test at the end keeps the device tests from being vacuous (the oracle's verdicts contain what each case is
meant to reach).

What these tests found when they were written (all in decide.hip, fixed there):
* k_jac's frozen stretch never ended on a zero-count ENTRY at its first position (it passes a saturated
  DefaultController, the stretch stops at it having committed nothing and was entered at it again): C2 / C4 with ZERO
  on the cooperative bins did not return;
* the ends of a frozen stretch / of the round machine summed the lanes' 32-bit unit sums in 32 bits within a wave: one
  wave's share of 300,000 blocked acquires of 65,535 (a one-wave owner's 1.97e10, a 256-lane owner's 4.9e9, 64 skipped
  block sums of 1,024 * 65,535 plus the stretch's edges on the wide owners) wrapped, the bucket's block count came out
  4 * 2^32 short ("block_sat": a rule of count 1 blocks every acquire of 65,535 without saturating the round,
  so that trace is decided by the Jacobi iteration, whose sums are 64-bit; the saturated form is the one that reaches
  the stretch);
* k_lite's per-second minute-window deltas are int32: a segment of more than 32,767 events a second on one lane
  (debug flag 2) wrapped them.
"""
import numpy as np
import pytest

import counts_util as U
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
@pytest.mark.parametrize("mix", ["MIXED", "ZERO"])
@pytest.mark.parametrize("trace", ["c2", "c3", "c4"])
def test_flow_degrade_counts(trace, mix, bin_mode):
    _run(U.reference(trace, mix))[0].close()


@gpu
@pytest.mark.parametrize("trace", ["c2", "c4"])
def test_counts_without_open_stretches(trace, monkeypatch):
    # the Jacobi iteration alone (debug flag 64 turns the all-pass open stretches off): mu[][], fu_m, q_units
    _setenv(monkeypatch, BIN_MODES["coop"], {"SG_DEBUG_FLAGS": "64"})
    _run(U.reference(trace, "MIXED"))[0].close()


# ---------------------------------------------------------------- 2. frozen-stretch skip with counts
@gpu
@pytest.mark.parametrize("skip_min", ["16", "1000"])
@pytest.mark.parametrize("mix,flags", [("MIXED", None), ("ZERO", None), ("MIXED", "32768")])
@pytest.mark.parametrize("trace", ["c2hot", "c4hot"])
def test_frozen_skip_counts(trace, mix, flags, skip_min, monkeypatch):
    # a skipped span's blocked units are the bst[] count sums of its 1,024-position blocks (k_grp_records /
    # k_block_sums); debug flag 32768 builds the side tables everywhere.  A zero acquire passes inside a saturated
    # stretch (0 + 0 > count is false), so BF_ZERO_CNT turns skipping off for the batch.
    _setenv(monkeypatch, HOT_BINS, {"SG_SKIP_MIN": skip_min})
    if flags:
        monkeypatch.setenv("SG_DEBUG_FLAGS", flags)
    eng, _ = _run(U.reference(trace, mix))
    if mix == "ZERO":
        assert eng.spans_total() == 0
    else:
        assert eng.spans_total() > 0  # the block sums were used
    eng.close()


# ---------------------------------------------------------------- 3. sums past 2^32
def _run_wide(case):
    ref = U.wide_reference(case)
    eng = E.Engine(max_resources=64, max_slot_chain_size=0, status_ring_log2=24)
    assert eng.register("wide") == 0
    eng.load_flow_rules(U.wide_rules(case))
    dg = eng.submit(ref.ev)
    _same_words(dg, ref.do, ref.ev)
    _same_node(eng.read_node(0), ref.node, "wide/" + case)
    eng.close()


@gpu
@pytest.mark.parametrize("case", ["pass", "block", "block_sat"])
@pytest.mark.parametrize("owner", sorted(OWNERS))
def test_wide_sums(owner, case, monkeypatch):
    # 70,000 passes / 300,000 blocks of 65,535 in one 500 ms bucket: 4.59e9 and 1.97e10 units in one stretch
    _setenv(monkeypatch, OWNERS[owner])
    _run_wide(case)


@gpu
@pytest.mark.parametrize("case", ["block", "block_sat"])
@pytest.mark.parametrize("owner", ["J1", "J4", "J16"])
def test_wide_sums_skipped(owner, case, monkeypatch):
    # the blocked stretch skipped: 293 block sums of up to 1,024 * 65,535
    _setenv(monkeypatch, OWNERS[owner], {"SG_SKIP_MIN": "16"})
    _run_wide(case)


def _same_aux(g, o, t_end, what):
    """An origin / context node against the oracle's, as test_gpu_aux._check_aux."""
    assert g is not None and o is not None, what
    assert g["thread"] == o["thread"], (what, g["thread"], o["thread"])
    np.testing.assert_array_equal(g["second"], o["second"][:2], err_msg="second window of %s" % what)
    m = o["minute"]
    for q in range(2):  # per second parity, the latest second with pass must be the device's history
        ws, ps = g["mhist"][q]
        live = (m[:, 0] >= 0) & (m[:, 0] > t_end - 60_000) & ((m[:, 0] // 1000) % 2 == q) & (m[:, 1] > 0)
        if ws >= 0 and ws > t_end - 59_000:
            k = np.nonzero(m[:, 0] == ws)[0]
            assert len(k) == 1 and m[k[0], 1] == ps, (what, q, ws, ps)
            assert not (live & (m[:, 0] > ws)).any(), (what, q)
        else:
            assert not (live & (m[:, 0] > t_end - 58_000)).any(), (what, q)


@gpu
def test_wide_sums_origin_and_context_nodes():
    # the aux post-pass (aux.hip) sums the same 4.59e9 units into the origin node and the context's DefaultNode
    ref = U.wide_reference("pass", origin=True)
    eng = E.Engine(max_resources=64, max_slot_chain_size=0, status_ring_log2=24, aux_node_capacity=1 << 17)
    assert eng.register("wide") == 0
    eng.load_flow_rules(U.wide_rules("pass", origin=True))
    oid, cid = eng.intern_origin("app-0"), eng.intern_context("ctx-0")
    assert (ref.ext["origin_id"] == oid).all() and (ref.ext["context_id"] == cid).all()
    dg = eng.submit_ex(ref.ev, ref.ext)
    _same_words(dg, ref.do, ref.ev)
    _same_node(eng.read_node(0), ref.node, "wide/origin")
    t_end = int(ref.ev["ts"][-1])
    _same_aux(eng.read_aux_node(0, 0, oid), ref.origin_node, t_end, "wide/app-0")
    _same_aux(eng.read_aux_node(0, 1, cid), ref.context_node, t_end, "wide/ctx-0")
    assert ref.origin_node["second"][:2, 1].max() == 70_000 * 65_535
    eng.close()


# ---------------------------------------------------------------- 4. param owners
@gpu
@pytest.mark.parametrize("mix", ["MIXED", "ZERO", "BIG"])
def test_param_counts(mix, bin_mode):
    # param_default_check: acquire > maxCount blocks outright, else acquire comes off the tokens; hot items;
    # THREAD-grade rules whose exits release their argument
    _run(U.reference("c5", mix))[0].close()


@gpu
def test_param_counts_maps_evict():
    # 16 resources over 200k values: every map fills and evicts its LRU values (k_pq)
    _run(U.reference("c5evict", "MIXED", batches=4))[0].close()


@gpu
@pytest.mark.parametrize("switch", [None, "SG_PV", "SG_PVT", "SG_MIX", "SG_PQ"])
@pytest.mark.parametrize("mix", ["MIXED", "BIG"])
def test_mixed_rule_counts(mix, switch, monkeypatch):
    # C6 (flow + degrade + param on every resource): the value-parallel pre / post passes carry acquire | hit << 16;
    # each switch off once (SG_PV=0 k_pq's passes, SG_PVT=0 the serial post pass, SG_MIX=0 / SG_PQ=0 one lane)
    if switch:
        monkeypatch.setenv(switch, "0")
    _run(U.reference("c6", mix), param_table_log2=24)[0].close()


# ---------------------------------------------------------------- 5. prioritized entries
@gpu
@pytest.mark.parametrize("trace,batches", [("prio1", 4), ("prio2", 3)])
def test_prioritized_counts(trace, batches, bin_mode):
    # tryOccupyNext / addWaitingRequest / addOccupiedPass with acquire > 1, the borrow ring compared
    ref = U.reference(trace, "MIXED", batches=batches)
    eng, dg = _run(ref, borrow=True)
    if trace == "prio1":
        st = dg[ref.ev["kind"] == A.EV_ENTRY] & 0xFF
        assert (st == A.PASS_WAIT).sum() > 0
    eng.close()


# ---------------------------------------------------------------- 6. exit and trace counts of their own
@gpu
@pytest.mark.parametrize("batches", [8, 2])
def test_exit_and_trace_counts_of_their_own(batches, bin_mode):
    # 30 % of the EXITs with a count other than their ENTRY's, TRACE counts 1-3, on the long minute-window trace
    # whose exception-count breakers read the running exception sum
    _run(U.reference("c4long", "MIXED", batches=batches, exit_own=0.3, trace_choices=(1, 2, 3)))[0].close()


# ---------------------------------------------------------------- 7. small synchronous calls
@gpu
@pytest.mark.parametrize("env", [{"SG_TINY": "1"}, {"SG_TINY": "0"}, {"SG_RADIX_BELOW": "0"}],
                         ids=["tiny", "no_tiny", "no_radix"])
@pytest.mark.parametrize("mix", ["MIXED", "ZERO"])
def test_small_call_counts(mix, env, monkeypatch):
    # k_tiny, the radix group stage and the hot / cold group stage on batches of 1 .. 4,097 events
    _setenv(monkeypatch, env)
    _run(U.reference("c4small", mix, batches="cycle"))[0].close()


# ---------------------------------------------------------------- 8. snapshot
@gpu
def test_snapshot_after_counts():
    ref = U.reference("c4", "MIXED", snapshots=True)
    eng, _ = _run(ref)
    for now, want in ref.snapshots.items():
        np.testing.assert_array_equal(U.sorted_snapshot(eng.snapshot(now, cap=1 << 18)), want)
    eng.close()


# ---------------------------------------------------------------- CPU: the traces reach what the cases are about
def _has(ref, *statuses, floor=1000):
    st = U.entry_status(ref)
    for s in statuses:
        assert int((st == s).sum()) > floor, (s, np.bincount(st, minlength=8))


def test_counts_trace_shape():
    """(CPU, oracle only) every trace and mix above reaches the verdicts its case is meant to reach."""
    for mix, (choices, _) in U.MIXES.items():  # the mixes are what they say
        ev = U.reference("c4hot", mix).ev
        assert set(np.unique(ev["count"][ev["kind"] == A.EV_ENTRY]).tolist()) == set(choices)
    for mix in ("MIXED", "ZERO"):
        for trace in ("c2", "c3"):
            _has(U.reference(trace, mix), A.PASS, A.BLOCK_FLOW, floor=100_000)
        _has(U.reference("c4", mix), A.PASS, A.BLOCK_FLOW, A.BLOCK_DEGRADE)
        _has(U.reference("c4hot", mix), A.PASS, A.BLOCK_FLOW, A.BLOCK_DEGRADE)
        _has(U.reference("c2hot", mix), A.PASS, A.BLOCK_FLOW)
        _has(U.reference("c4small", mix, batches="cycle"), A.PASS, A.BLOCK_FLOW, floor=100)
    _has(U.reference("c4hot", "BIG"), A.PASS, A.BLOCK_FLOW)  # (no degrade block: BIG is not used on C2 / C4)
    for mix in ("MIXED", "ZERO", "BIG"):
        _has(U.reference("c5", mix), A.PASS, A.BLOCK_PARAM)
    _has(U.reference("c5evict", "MIXED", batches=4), A.PASS, A.BLOCK_PARAM)
    for mix in ("MIXED", "BIG"):
        _has(U.reference("c6", mix), A.PASS, A.BLOCK_FLOW, A.BLOCK_DEGRADE, A.BLOCK_PARAM)
    _has(U.reference("prio1", "MIXED", batches=4), A.PASS_WAIT, floor=0)
    _has(U.reference("prio2", "MIXED", batches=3), A.PASS, A.BLOCK_FLOW)

    # an EXIT releases its ENTRY's count; with exit_own some do not, and the TRACE counts are 1-3
    for ref, own in ((U.reference("c4", "MIXED"), False),
                     (U.reference("c4long", "MIXED", batches=8, exit_own=0.3, trace_choices=(1, 2, 3)), True)):
        ev = ref.ev
        ex = np.nonzero((ev["kind"] == A.EV_EXIT) & ((ev["aux"] & np.uint64(A.REF_NONE)) != np.uint64(A.REF_NONE)))[0]
        differ = ev["count"][ex] != ev["count"][(ev["aux"][ex] & np.uint64(A.REF_NONE)).astype(np.int64)]
        assert differ.any() == own and differ.mean() < 0.3

    # sums past 2^32: every acquire of 65,535 passes, both buckets hold 70,000 * 65,535
    ref = U.wide_reference("pass")
    assert ((ref.do & 0xFF) == A.PASS).all()
    assert ref.node["second"][:2, 1].max() == ref.node["minute"][:, 1].max() == 70_000 * 65_535 == 4_587_450_000
    assert 70_000 * 65_535 > 1 << 32
    assert len(np.unique(ref.ev["ts"] // 500)) == 1
    for case, n_pass in (("block", 0), ("block_sat", 1)):  # all but the ENTRYs that fit under the rule are blocked
        ref = U.wide_reference(case)
        assert ((ref.do & 0xFF) == A.PASS).sum() == n_pass and ((ref.do & 0xFF) == A.BLOCK_FLOW).sum() == 300_000 - n_pass
        assert ref.node["second"][:2, 2].max() == (300_000 - n_pass) * 65_535 > 1 << 32
    ref = U.wide_reference("pass", origin=True)
    assert ((ref.do & 0xFF) == A.PASS).all()
    for node in (ref.origin_node, ref.context_node):
        assert node is not None and node["second"][:2, 1].max() == 70_000 * 65_535

    # exit / trace counts of their own: counts above 1 reached the minute window's exception sums
    ref = U.reference("c4long", "MIXED", batches=8, exit_own=0.3, trace_choices=(1, 2, 3))
    ev = ref.ev
    tr = np.nonzero((ev["kind"] == A.EV_TRACE) & np.isin(ev["res_id"], ref.sample))[0]
    passed = np.isin(ref.do[(ev["aux"][tr] & np.uint64(A.REF_NONE)).astype(np.int64)] & 0xFF, (A.PASS, A.PASS_WAIT))
    tr = tr[passed & (ev["count"][tr] > 0)]  # the effective TRACEs
    exc_sum = n_eff = 0
    for r in ref.sample:
        m = ref.nodes[int(r)]["minute"]
        kept = m[m[:, 0] >= 0]
        mine = tr[ev["res_id"][tr] == r]
        n_eff += int(np.isin(ev["ts"][mine] // 1000 * 1000, kept[:, 0]).sum())  # in a second the window still holds
        exc_sum += int(kept[:, 3].sum())
    assert n_eff > 1000 and exc_sum > n_eff, (exc_sum, n_eff)

    # every ZERO trace: a zero-count ENTRY in every batch that holds an ENTRY (BF_ZERO_CNT raised batch by batch),
    # down to the small calls' batches of one event; only that trace's tail of EXITs has batches without ENTRYs
    for trace, batches in (("c2", 3), ("c3", 3), ("c4", 3), ("c2hot", 3), ("c4hot", 3), ("c5", 3), ("c4small", "cycle")):
        ref = U.reference(trace, "ZERO", batches=batches)
        ent = ref.ev["kind"] == A.EV_ENTRY
        zero = ent & (ref.ev["count"] == 0)
        n_with = 0
        for a, b in zip(ref.cuts[:-1], ref.cuts[1:]):
            assert zero[a:b].any() or (batches == "cycle" and not ent[a:b].any()), (trace, a, b)
            n_with += bool(zero[a:b].any())
        assert n_with >= (3 if batches == 3 else 20), (trace, n_with)
