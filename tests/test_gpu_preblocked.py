"""Pre-blocked ENTRYs -- SG_F_BLOCKED_UPSTREAM, or an origin the resource's authority rule rejects -- on the
cooperative owners (DESIGN.md §5 "Pre-blocked entries on the cooperative owners").

Such an ENTRY used to send its resource to one lane for the engine's life.  Now its record carries RF_UBLK, its word is
written ahead of the decide stage (decide.hip k_ublk_words) and the owners (k_jac at every width, k_fill) count it as a
block and evaluate nothing for it -- the class an XF_MIX segment's param-blocked ENTRYs already were.  Everything is
compared with the event-sequential oracle, which honours the flag itself: all 32 bits of every decision word, thread
count, second and minute window of the 50 hottest and 300 random resources, the origin / context nodes where
sg_submit_ex is used, the param thread-count maps where param rules are loaded.  The authority rules are checked by
flag emulation (tests/test_gpu_authority.py): status 7 where the oracle says 6 and the caller did not flag.

tests/test_preblocked_host.py (CPU) shows from the oracle's decisions alone that the traces reach what the cases are
about; tests/preblocked_util.py builds them.
"""
import ctypes as C

import numpy as np
import pytest

import counts_util as U
import preblocked_util as P
import pyoracle as O
import test_gpu_counts as GC
from sentinel_amd import _abi as A
from sentinel_amd import engine as E

pytestmark = pytest.mark.gpu

ENTRY = A.EV_ENTRY
OWNER_SETS = {
    "J1": GC.OWNERS["J1"], "J4": GC.OWNERS["J4"], "J16": GC.OWNERS["J16"],
    "coop": GC.BIN_MODES["coop"], "skip": GC.BIN_MODES["skip"], "hot": GC.HOT_BINS,
}


def _device_replay(eng, ev, cuts, ext=None):
    """Every batch from device buffers, back to back through the two-stage pipeline, one sync at the end: batch k + 1's
    group stage sets its marks while batch k's decide stage runs."""
    import torch
    dev = torch.device("cuda", 0)
    n = len(ev)
    d_ev = torch.from_numpy(np.ascontiguousarray(ev).view(np.uint8).copy()).to(dev)
    d_out = torch.zeros(n, dtype=torch.int32, device=dev)
    d_ext = None if ext is None else torch.from_numpy(np.ascontiguousarray(ext).view(np.uint8).copy()).to(dev)
    for a, b in zip(cuts[:-1], cuts[1:]):
        a, b = int(a), int(b)
        if ext is None:
            eng.submit_ptr(d_ev.data_ptr() + a * 24, b - a, d_out.data_ptr() + a * 4, sync=False)
        else:
            eng.submit_ex_ptr(d_ev.data_ptr() + a * 24, d_ext.data_ptr() + a * 16, b - a, d_out.data_ptr() + a * 4,
                              sync=False)
    eng.sync()
    return d_out.cpu().numpy().view(np.uint32)


def _engine(ref, **kw):
    kw.setdefault("max_resources", max(64, ref.w.n_res))
    eng = E.Engine(max_slot_chain_size=0, status_ring_log2=24, **kw)
    ref.w.install(eng)
    return eng


def _check(eng, ref, dg, want=None):
    GC._same_words(dg, ref.do if want is None else want, ref.ev)
    for r in ref.sample:
        GC._same_node(eng.read_node(int(r)), ref.nodes[int(r)], "res %d" % r)


def _run(ref, device=True):
    eng = _engine(ref)
    if device:
        dg = _device_replay(eng, ref.ev, ref.cuts)
    else:
        dg = np.concatenate([eng.submit(ref.ev[a:b]) for a, b in zip(ref.cuts[:-1], ref.cuts[1:])])
    _check(eng, ref, dg)
    return eng


# ---------------------------------------------------------------- 1. upstream flags through sg_submit
@pytest.mark.parametrize("trace", ["c2", "c3", "c4"])
@pytest.mark.parametrize("owner", sorted(OWNER_SETS))
def test_upstream_flags_on_every_owner(owner, trace, monkeypatch):
    # three batches, the first two with flagged ENTRYs (a ~10 % share and, on the hottest resources, runs of more than
    # two 1,024-position tiles over a 500 ms bucket edge), EXITs and TRACEs naming them in their own batch and in the
    # next one (status ring); the third batch carries no flag: the marks are sticky (7. below)
    GC._setenv(monkeypatch, OWNER_SETS[owner])
    ref = P.reference(trace, "MIXED")
    eng = _run(ref)
    coop, lane, words = eng.preblocked_stats()
    # with SG_LANE_MAX=0 every marked segment of a cooperative program is a cooperative owner's; C3 holds programs
    # outside the owners' limits (PF_SERIAL), C2 / C4 none
    marked = len(P.marked_segments(ref, 2, 0))
    assert coop + lane == marked and coop > 0, (coop, lane, marked)
    if trace != "c3":
        assert lane == 0
    assert words == 0  # (no flagged ENTRY in the last batch)
    eng.close()


@pytest.mark.parametrize("trace", ["c2", "c3", "c4"])
def test_upstream_flags_with_zero_counts(trace, monkeypatch):
    # a zero acquire passes a saturated stage; BF_ZERO_CNT turns span skipping off for the batch
    GC._setenv(monkeypatch, OWNER_SETS["coop"])
    _run(P.reference(trace, "ZERO")).close()


@pytest.mark.parametrize("trace", ["c2", "c3", "c4"])
def test_upstream_flags_hot_cold_group_stage(trace, monkeypatch):
    # the hot / cold group stage (k_grp_first marks, k_grp_records builds the records) instead of the radix one
    GC._setenv(monkeypatch, OWNER_SETS["coop"], {"SG_RADIX_BELOW": "0"})
    eng = _run(P.reference(trace, "MIXED"))
    assert eng.preblocked_stats()[0] > 0
    eng.close()


def test_upstream_flags_words_written_per_batch():
    # sync submits: the counts of each batch.  Every flagged ENTRY of a cooperative bin's segment gets its word from
    # k_ublk_words, the others (short segments of the default bins) from lane_entry
    ref = P.reference("c4", "MIXED")
    eng = _engine(ref)
    for k, (a, b) in enumerate(zip(ref.cuts[:-1], ref.cuts[1:])):
        dg = eng.submit(ref.ev[a:b])
        GC._same_words(dg, ref.do[a:b], ref.ev[a:b])
        coop, lane, words = eng.preblocked_stats()
        segs = P.marked_segments(ref, k, 128)  # (a batch below SHARD_BATCH: the lane bins end at 128 events)
        assert coop == len(segs), (k, coop, len(segs))
        assert words == int(ref.mask[a:b][np.isin(ref.ev["res_id"][a:b], list(segs))].sum()), (k, words)
    eng.close()


@pytest.mark.parametrize("flags", ["16384", "0"])
@pytest.mark.parametrize("owner", ["J1", "J4", "J16"])
def test_head_programs_yield(owner, flags, monkeypatch):
    # C3's single-rule THREAD-grade and rate-limiter programs are k_head's (XF_HEADT / XF_HEADR); a marked one is the
    # cooperative owner's, with k_head on (0) and off (debug flag 16384) alike
    GC._setenv(monkeypatch, OWNER_SETS[owner], {"SG_DEBUG_FLAGS": flags})
    _run(P.reference("c3", "MIXED")).close()


@pytest.mark.parametrize("trace", ["c2", "c4"])
def test_without_open_stretches(trace, monkeypatch):
    GC._setenv(monkeypatch, OWNER_SETS["coop"], {"SG_DEBUG_FLAGS": "64"})
    _run(P.reference(trace, "MIXED")).close()


# ---------------------------------------------------------------- 2. frozen and skipped spans
@pytest.mark.parametrize("trace,mix,flags,skip_min", [
    ("c2hot", "MIXED", None, "16"), ("c2hot", "ZERO", None, "16"), ("c2hot", "MIXED", "32768", "16"),
    ("c4hot", "MIXED", None, "16"), ("c4hot", "ZERO", None, "16"), ("c4hot", "MIXED", "32768", "16"),
    ("c2hot", "MIXED", None, "1000"), ("c4hot", "MIXED", None, "1000"), ("c4hot", "ZERO", None, "1000")])
def test_frozen_and_skipped_spans(trace, mix, flags, skip_min, monkeypatch):
    # 12 saturated resources: the flagged ENTRYs lie inside frozen stretches and skipped spans (k_fill leaves their
    # words alone), the zero-count ones of ZERO between BLOCK_FLOW words (a zero acquire passes a saturated stage: a
    # flagged one must not)
    GC._setenv(monkeypatch, GC.HOT_BINS, {"SG_SKIP_MIN": skip_min})
    if flags:
        monkeypatch.setenv("SG_DEBUG_FLAGS", flags)
    eng = _run(P.reference(trace, mix))
    assert eng.preblocked_stats()[0] == len(P.marked_segments(P.reference(trace, mix), 2, 0))
    if mix == "MIXED":
        assert eng.spans_total() > 0
    eng.close()


# ---------------------------------------------------------------- 3. authority rules through sg_submit_ex
@pytest.mark.parametrize("env", [{}, {"SG_RADIX_BELOW": "0"}, GC.BIN_MODES["skip"]], ids=["default", "hot_cold", "skip"])
def test_authority_rules_on_the_cooperative_owners(env, monkeypatch):
    GC._setenv(monkeypatch, env)
    ref = P.authority_reference()
    eng = _engine(ref, aux_node_capacity=1 << 18)
    io, ic = ref.w.intern_names(eng, P.N_ORIGINS, P.N_CONTEXTS)
    assert np.array_equal(io, ref.io) and np.array_equal(ic, ref.ic)
    P.load_extra_flow(eng, ref.w, ref.extra_flow)
    assert eng.load_authority_rules([A.authority_rule(*t) for t in ref.tuples]) == len(ref.tuples)
    dg = _device_replay(eng, ref.ev, ref.cuts, ref.ext)
    _check(eng, ref, dg, want=ref.want)
    st = dg & 0xFF
    np.testing.assert_array_equal(st == A.BLOCK_AUTHORITY, ref.blk & ~ref.caller & ((ref.do & 0xFF) == A.BLOCK_UPSTREAM))
    t_end = int(ref.ev["ts"][-1])
    for (res, k), o in ref.origin_nodes.items():
        if o is not None:
            GC._same_aux(eng.read_aux_node(res, 0, int(io[k])), o, t_end, "origin app-%d of %d" % (k, res))
    for (res, k), o in ref.context_nodes.items():
        if o is not None:
            GC._same_aux(eng.read_aux_node(res, 1, int(ic[k])), o, t_end, "context ctx-%d of %d" % (k, res))
    # the resource whose flow rule reads an origin node (PX_ORIGIN) stays on a lane; the other marked ones do not
    lane_max = 0 if env.get("SG_LANE_MAX") == "0" else 128
    segs = P.marked_segments(ref, 2, 0)
    long_ = {r for r, n in segs.items() if n > lane_max and r != ref.origin_res}
    coop, lane, _ = eng.preblocked_stats()
    assert ref.origin_res in segs and segs[ref.origin_res] > 128
    assert (coop, lane) == (len(long_), len(segs) - len(long_)), (coop, lane, len(long_), len(segs))
    eng.close()


# ---------------------------------------------------------------- 4. mix: param rules first
@pytest.mark.parametrize("pv", ["1", "0"])
def test_mix_param_rules_first(pv, monkeypatch):
    # XF_MIX resources (tests/test_gpu_mix.py's rules): a flagged ENTRY still takes the param check and its tokens; the
    # param rule's block wins (word 4), else the word is 6; the thread-count maps count neither
    monkeypatch.setenv("SG_PV", pv)
    ref = P.mix_reference()
    eng = E.Engine(max_resources=64, max_slot_chain_size=0, param_table_log2=22, status_ring_log2=24)
    for nm in P.MIX_NAMES:
        eng.register(nm)
    f, d, p = ref.rules
    eng.load_flow_rules(f)
    eng.load_degrade_rules(d)
    eng.load_param_rules(p)
    w4 = w6 = 0
    for k, (ev, do, m) in enumerate(zip(ref.batches, ref.do, ref.masks)):
        dg = eng.submit(ev)
        GC._same_words(dg, do, ev)
        w4 += int((m & ((dg & 0xFF) == A.BLOCK_PARAM)).sum())
        w6 += int((m & ((dg & 0xFF) == A.BLOCK_UPSTREAM)).sum())
        assert eng.preblocked_stats()[0] >= 1, k  # x0's segment (and the other long ones) on their owners
    assert w4 >= 10 and w6 >= 50
    for res in range(len(P.MIX_NAMES)):
        GC._same_node(eng.read_node(res), ref.nodes[res], "mix res %d" % res)
    for res, keys in ref.thread_keys.items():
        got = [eng.param_thread_count(res, 0, int(k)) for k in keys]
        assert got == ref.threads[res], ("thread counts of res %d" % res)
    eng.close()


# ---------------------------------------------------------------- 5. placement
def _j1_segments(eng):
    # SG_DEBUG=1 SG_PROF_BIN=2: [4] counts the segments k_jac<1> decided (tests/test_gpu_lane_boundary.py)
    fn = E.lib().sgx_debug_counters
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    buf = (C.c_ulonglong * 64)()
    assert fn(eng.h, buf, 64) == 64
    return int(buf[4])


def test_placement(monkeypatch):
    # the same trace with SG_UBLK=1 and SG_UBLK=0 (every segment under 5,000 events: one lane walks the marked ones):
    # equal words; the one-wave owner decides the marked segments of its lengths only with the switch on
    ref = P.reference("c4flat", "MIXED")
    lane_max, j1_max = 128, 1024
    GC._setenv(monkeypatch, {"SG_DEBUG": "1", "SG_PROF_BIN": "2", "SG_LANE_MAX": str(lane_max), "SG_J1_MAX": str(j1_max)})

    def replay(ublk, with_stats):
        monkeypatch.setenv("SG_UBLK", ublk)
        eng = _engine(ref)
        dg, stats = [], []
        for a, b in zip(ref.cuts[:-1], ref.cuts[1:]):
            dg.append(eng.submit(ref.ev[a:b]))
            if with_stats:
                stats.append(eng.preblocked_stats())
        dg = np.concatenate(dg)
        _check(eng, ref, dg)
        n_j1 = _j1_segments(eng)
        eng.close()
        return dg, n_j1, stats

    # every C4 program is cooperative (flow + degrade stages inside the owners' limits, no param rule)
    per_batch = [P.marked_segments(ref, k, lane_max) for k in range(3)]
    want_j1 = sum(1 for segs in per_batch for n in segs.values() if n <= j1_max)
    assert want_j1 >= 10
    # the one-wave owner's segment counter first: it needs nothing but the switch, and without the cooperative route
    # (the switch unknown, every marked resource on a lane) both engines count the same
    on, off = replay("1", False), replay("0", False)
    assert np.array_equal(on[0], off[0])
    assert on[1] - off[1] == want_j1, (on[1], off[1], want_j1)
    on, off = replay("1", True), replay("0", True)
    assert [s[0] for s in on[2]] == [len(segs) for segs in per_batch], (on[2], per_batch)
    assert all(s == [0, 0, 0] for s in off[2]), off[2]  # SG_UBLK=0: PM_LANE, no PM_UBLK mark at all


# ---------------------------------------------------------------- 6. what stays on a lane
def _lane_trace(seed, n_per, names, t0=U.T0, span_ms=1200, gbase=0):
    """n_per ENTRYs a resource over span_ms, each with an EXIT naming it, ~10 % flagged."""
    rng = np.random.default_rng(seed)
    nr = len(names)
    n = n_per * nr
    res = np.repeat(np.arange(nr, dtype=np.uint32), n_per)
    te = t0 + np.sort(rng.integers(0, span_ms, n))
    rng.shuffle(res)
    rt = rng.integers(0, 40, n)
    ts = np.concatenate([te, te + rt])
    kind = np.concatenate([np.zeros(n, dtype=np.int64), np.full(n, A.EV_EXIT, dtype=np.int64)])
    order = np.lexsort((kind, ts))
    pos = np.empty(2 * n, dtype=np.int64)
    pos[order] = np.arange(2 * n)
    ev = np.zeros(2 * n, dtype=A.EVENT_DTYPE)
    ev["ts"] = ts[order]
    ev["res_id"] = np.concatenate([res, res])[order]
    ev["count"] = 1
    ev["kind"] = kind[order]
    aux = np.zeros(2 * n, dtype=np.uint64)
    aux[pos[n:]] = (rt.astype(np.uint64) << np.uint64(48)) | (gbase + pos[:n]).astype(np.uint64)
    ev["aux"] = aux
    fl = np.zeros(2 * n, dtype=np.uint8)
    fl[pos[:n]] = np.where(rng.random(n) < 0.10, A.F_BLOCKED_UPSTREAM, 0)
    ev["flags"] = fl
    return ev


def test_still_lanes():
    # PF_PQ-only, prioritized, RELATE and NullContext resources with flagged ENTRYs: decided as before (lane_entry /
    # k_pq), none of them counted among the cooperative owners' marked segments
    names = ("pq", "prio", "rel", "relb", "nullc")
    eng = E.Engine(max_resources=64, max_slot_chain_size=0, param_table_log2=20, status_ring_log2=22,
                   aux_node_capacity=1 << 14)
    orc = O.Oracle(max_slot_chain_size=0)
    ev = _lane_trace(5, 3000, names)
    n = len(ev)
    ent = ev["kind"] == ENTRY
    rng = np.random.default_rng(6)
    is_res = lambda nm: ev["res_id"] == names.index(nm)
    ev["flags"][ent & is_res("prio") & (rng.random(n) < 0.2)] |= A.F_PRIORITIZED
    pq = ent & is_res("pq")
    keys = np.array([O.param_key(str(v), "long") for v in range(40)], dtype=np.uint64)
    ev["flags"][pq] |= A.F_HAS_ARG
    ev["aux"][pq] = keys[rng.integers(0, len(keys), int(pq.sum()))]
    ext = np.zeros(n, dtype=A.EXT_DTYPE)
    for x in (eng, orc):
        for nm in names:
            x.register(nm)
        x.load_flow_rules([A.flow_rule("prio", 400), A.flow_rule("rel", 300, strategy=A.STRATEGY_RELATE, ref_resource="relb"),
                           A.flow_rule("relb", 500), A.flow_rule("nullc", 350)])
        x.load_param_rules([A.param_rule("pq", 0, 20)])
        nc = None
        for k in range(A.MAX_CONTEXTS + 1):
            nc = x.intern_context("filler%d" % k)
        assert nc == A.MAX_CONTEXTS + 1
    # a tenth of nullc's ENTRYs (and their EXITs) come in the NullContext
    ref_i = (ev["aux"] & np.uint64(A.REF_NONE)).astype(np.int64)
    src = np.where(ent, np.arange(n), np.minimum(ref_i, n - 1))
    pick = is_res("nullc") & (rng.random(n) < 0.1)[src]
    ext["context_id"][pick] = nc
    cuts = np.array([0, n // 2, n])
    for a, b in zip(cuts[:-1], cuts[1:]):
        dg, do = eng.submit_ex(ev[a:b], ext[a:b]), orc.submit_ex(ev[a:b], ext[a:b])
        GC._same_words(dg, do, ev[a:b])
        coop, lane, words = eng.preblocked_stats()
        assert (coop, words) == (0, 0) and lane >= len(names) - 1, (coop, lane, words)  # (rel and relb: one segment)
    flagged = ent & ((ev["flags"] & A.F_BLOCKED_UPSTREAM) != 0)
    for nm in names:  # every kind saw its flags
        assert (flagged & is_res(nm)).sum() >= 50, nm
    for r in range(len(names)):
        GC._same_node(eng.read_node(r), orc.read_node(r), names[r])
    eng.close()
    orc.close()
