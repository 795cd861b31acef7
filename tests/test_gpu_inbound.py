"""The global inbound node (Constants.ENTRY_NODE) on the device: sg_track_inbound, inbound.hip.

The reference is inbound_util's: the trace and the *oracle's* decisions give a one-resource stream, a second oracle
replays it (tests/test_inbound_host.py checks that scheme against a sequential model).  Every case compares the node
after *every* batch, so thread counts are non-zero, and asserts that the decisions and a sample of ClusterNodes equal
the oracle's: tracking changed nothing else.
"""
import functools

import numpy as np
import pytest

import counts_util as CU
import inbound_util as IU
import preblocked_util as PU
import pyoracle as O
from sentinel_amd import _abi as A
from sentinel_amd import engine as E
from sentinel_amd import metric_log as ML
from sentinel_amd import tracegen as T

pytestmark = pytest.mark.gpu


def _engine(w, track=True, **kw):
    kw.setdefault("max_resources", max(64, w.n_res))
    kw.setdefault("max_slot_chain_size", 0)
    eng = E.Engine(status_ring_log2=22, **kw)
    w.install(eng)
    if track:
        eng.track_inbound(True)
    return eng


def _same_cluster_nodes(eng, nodes):
    for r, o in nodes.items():
        g = eng.read_node(int(r))
        np.testing.assert_array_equal(g["second"][:2], o["second"][:2], err_msg="ClusterNode %d" % r)
        np.testing.assert_array_equal(g["minute"], o["minute"], err_msg="ClusterNode %d" % r)
        assert g["thread"] == o["thread"], "ClusterNode %d" % r


def _run(eng, ev, do, cuts, nodes, ext=None, want=None, null_ctx=None):
    """The batches through the engine, the node against the replay oracle after each; returns (derived, replay)."""
    d = IU.derive(ev, do, cuts, null_ctx=null_ctx)
    rp = IU.Replay(d)
    dg = []
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        a, b = int(a), int(b)
        dg.append(eng.submit(ev[a:b]) if ext is None else eng.submit_ex(ev[a:b], ext[a:b]))
        rp.feed(k)
        IU.assert_node_equal(eng.read_inbound_node(), rp.node(), "after batch %d of %d" % (k, len(cuts) - 1))
    np.testing.assert_array_equal(np.concatenate(dg), do if want is None else want)
    _same_cluster_nodes(eng, nodes)
    return d, rp


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _counts_case(name, mix, batches):
    """A counts_util reference with SG_F_ENTRY_OUT on 30 % of the resources (the flag changes no decision, so the
    cached oracle run stands)."""
    r = CU.reference(name, mix, batches=batches)
    c = Case()
    c.w, c.cuts, c.do, c.nodes = r.w, r.cuts, r.do, r.nodes
    c.ev, c.out_res = IU.mark_out(r.ev, r.w.n_res, frac=0.3)
    return c


@functools.lru_cache(maxsize=None)
def _plain_case(name, batches=3, out_frac=0.3):
    """A counts_util workload as generated (counts of 1), replayed through the oracle here."""
    w = CU.workload(name)
    c = Case()
    c.w = w
    c.ev, c.out_res = IU.mark_out(w.events, w.n_res, frac=out_frac if w.n_res > 1 else 0.0)
    c.cuts = CU.cuts_of(len(c.ev), batches)
    orc = O.Oracle(max_slot_chain_size=0)
    w.install(orc)
    c.do = np.concatenate([orc.submit(c.ev[a:b]) for a, b in zip(c.cuts[:-1], c.cuts[1:])])
    c.nodes = {int(x): orc.read_node(int(x)) for x in CU.sample(c.ev, w.n_res, k=50)}
    orc.close()
    return c


# ---------------------------------------------------------------- the traces
@pytest.mark.parametrize("batches", [3, "cycle"])
def test_c4small(batches):
    # three synchronous batches; the size cycle of the small-call test: k_tiny and the batched path alternate on one node
    c = _counts_case("c4small", "MIXED", batches)
    eng = _engine(c.w)
    d, rp = _run(eng, c.ev, c.do, c.cuts, c.nodes)
    assert d.updates > 10_000 and d.blocks > 0 and d.exits > 0 and len(c.out_res) > 100
    assert d.updates < int((c.ev["kind"] != A.EV_TRACE).sum())  # the OUT events were left out
    if batches == "cycle":
        assert min(np.diff(c.cuts)) <= 256 < max(np.diff(c.cuts))
    rp.close()


def test_c4hot_big_counts_and_merged_partials():
    # 12 resources, 300k entries with acquire / exit counts up to 65,535: J8 / J16 owners, frozen spans and k_fill;
    # more than one workgroup's partial is merged.  (The BIG mix draws 65,535 for 2 % of the events: a bucket's sums reach
    # some 10^8 here, not 2^32; test_wide_sums_past_2_32 below is the case whose sums do.)
    c = _counts_case("c4hot", "BIG", 3)
    eng = _engine(c.w)
    d, rp = _run(eng, c.ev, c.do, c.cuts, c.nodes)
    last = eng.inbound_last()
    assert last[0] > 1, last
    assert last[1] == c.cuts[-1] - c.cuts[-2] and 0 < last[2] <= last[1], last
    node = rp.node()
    assert max(node["second"][:2, 1:6].max(), node["minute"][:, 1:6].max()) > 1 << 24
    rp.close()


@pytest.mark.parametrize("case", ["pass", "block_sat"])
def test_wide_sums_past_2_32(case):
    # counts_util's one-bucket trace: 70,000 (passing) / 300,000 (all but one blocked) ENTRYs of 65,535 in one 500 ms
    # bucket: the bucket's pass / block sum passes 2^32 (the 32-bit tile sums are folded into 64 bits between tiles)
    r = CU.wide_reference(case)
    cuts = np.array([0, len(r.ev)], dtype=np.int64)
    eng = E.Engine(max_resources=64, max_slot_chain_size=0, status_ring_log2=22)
    assert eng.register("wide") == 0
    eng.load_flow_rules(CU.wide_rules(case))
    eng.track_inbound(True)
    d, rp = _run(eng, r.ev, r.do, cuts, {0: r.node})
    node = rp.node()
    assert node["second"][:2, 1:3].max() > 1 << 32 and eng.inbound_last()[0] > 1
    rp.close()


def test_prio1_priority_waits_and_minute_wrap():
    # one resource, a 100 s span in three batches: SG_PASS_WAIT entries (the thread alone) and minute slots that wrap
    c = _plain_case("prio1")
    eng = _engine(c.w)
    d, rp = _run(eng, c.ev, c.do, c.cuts, c.nodes)
    assert d.waits > 100 and int(c.ev["ts"][-1] - c.ev["ts"][0]) > 60_000
    rp.close()


# ---------------------------------------------------------------- a hand-built trace
def _hand_built():
    """Resource 0 (IN, a QPS rule of 4) and resource 1 (OUT).  Times are offsets from CU.T0 (a whole second, an even
    500 ms index)."""
    rows = []

    def entry(t, res, count=1):
        rows.append((CU.T0 + t, res, count, A.EV_ENTRY, A.F_ENTRY_OUT if res == 1 else 0, 0))
        return len(rows) - 1

    def exit_(t, res, ref, rt, count=1):
        rows.append((CU.T0 + t, res, count, A.EV_EXIT, A.F_ENTRY_OUT if res == 1 else 0, A.aux_exit(ref, rt)))

    # batch 0 spans more than 60 s: the minute slot of second 1 is taken again by second 61; second 30 stays behind
    e0 = entry(0, 0)
    e1 = entry(100, 0, 3)
    e2 = entry(150, 0)            # blocked: the third of the second
    o0 = entry(160, 1)
    e3 = entry(600, 0)            # blocked (second-window slot 1)
    e4 = entry(1200, 0, 2)
    exit_(1250, 0, e0, 1250)
    e5 = entry(30_000, 0)
    e6 = entry(30_400, 0)
    exit_(30_450, 1, o0, 7)
    e7 = entry(61_300, 0)         # second 1's minute slot again, a later window
    e8 = entry(61_800, 0)         # the batch's last windows: 61,500 and 61,000
    b0 = len(rows)
    # batch 1 starts in those windows (adds): EXITs of batch 0's ENTRYs, passed and blocked, one without a reference
    exit_(61_900, 0, e1, 4999, 3)     # rt clipped to 4,900
    exit_(61_950, 0, e2, 10)          # of a blocked ENTRY: not effective
    exit_(61_960, 0, A.REF_NONE, 33)  # no reference, the resource has its chain: effective
    e9 = entry(61_990, 0)
    exit_(62_100, 0, e4, 900, 2)
    exit_(62_100, 0, e3, 5)           # blocked ENTRY
    e10 = entry(62_700, 0)
    b1 = len(rows)
    # batch 2 starts later (resets), in even 500 ms windows only: second-window slot 1 keeps 62,500
    exit_(75_000, 0, e5, 12)
    e11 = entry(75_010, 0, 4)
    entry(75_015, 0)              # blocked: the second holds 4
    exit_(75_020, 0, A.REF_NONE, 0, 0)
    exit_(76_100, 0, e10, 60000)
    e12 = entry(76_120, 1)
    exit_(76_130, 1, e12, 3)
    exit_(76_140, 0, e11, 1, 4)
    ev = np.zeros(len(rows), dtype=A.EVENT_DTYPE)
    for i, (ts, res, cnt, kind, fl, aux) in enumerate(rows):
        ev[i] = (ts, res, cnt, kind, fl, aux)
    return ev, np.array([0, b0, b1, len(rows)], dtype=np.int64)


def test_hand_built_gaps_wraps_and_earlier_batches():
    ev, cuts = _hand_built()
    names, rules = ["in", "out"], [A.flow_rule("in", 4)]
    orc = O.Oracle(max_slot_chain_size=0)
    eng = E.Engine(max_resources=64, max_slot_chain_size=0, status_ring_log2=22)
    for x in (orc, eng):
        assert [x.register(nm) for nm in names] == [0, 1]
        x.load_flow_rules(rules)
    eng.track_inbound(True)
    do = np.concatenate([orc.submit(ev[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
    st = do & 0xFF
    assert (st[ev["kind"] == A.EV_ENTRY] == A.BLOCK_FLOW).sum() >= 3
    nodes = {0: orc.read_node(0), 1: orc.read_node(1)}
    d, rp = _run(eng, ev, do, cuts, nodes)
    node = eng.read_inbound_node()
    ws = node["minute"][:, 0]
    slot = lambda sec: (CU.T0 // 1000 + sec) % 60
    assert slot(1) == slot(61)
    assert ws[slot(61)] == CU.T0 + 61_000 and ws[slot(30)] == CU.T0 + 30_000 and ws[slot(75)] == CU.T0 + 75_000
    assert node["second"][1, 0] == CU.T0 + 62_500 and node["second"][0, 0] == CU.T0 + 76_000
    assert node["second"][0, 7] == 1 and node["minute"][slot(62), 7] == 900  # min rt
    assert node["minute"][slot(61), 5] == 4900 + 33                         # the 4,999 was clipped
    orc.close()
    rp.close()


# ---------------------------------------------------------------- blocks of every kind
def test_preblocked_and_authority_blocks_count():
    # SG_F_BLOCKED_UPSTREAM and an authority rule's blocks (status 6 and 7) through sg_submit_ex with origins and contexts
    ref = PU.authority_reference(name="c4flat")
    ev, out_res = IU.mark_out(ref.ev, ref.w.n_res, frac=0.3)
    eng = _engine(ref.w, aux_node_capacity=1 << 18)
    io, ic = ref.w.intern_names(eng, PU.N_ORIGINS, PU.N_CONTEXTS)
    assert np.array_equal(io, ref.io) and np.array_equal(ic, ref.ic)
    PU.load_extra_flow(eng, ref.w, ref.extra_flow)
    assert eng.load_authority_rules([A.authority_rule(*t) for t in ref.tuples]) == len(ref.tuples)
    d, rp = _run(eng, ev, ref.want, ref.cuts, ref.nodes, ext=ref.ext)
    st = (ref.want & 0xFF)[(ev["kind"] == A.EV_ENTRY) & ((ev["flags"] & A.F_ENTRY_OUT) == 0)]
    assert (st == A.BLOCK_UPSTREAM).sum() > 100 and (st == A.BLOCK_AUTHORITY).sum() > 100 and d.blocks > 200
    rp.close()


def test_param_blocks_count():
    # a C6-style trace: hot-parameter rules, status 4
    w = T.Workload(6, n_entries=40_000, n_res=500, n_param_values=5_000)
    ev, out_res = IU.mark_out(w.events, w.n_res, frac=0.3)
    cuts = CU.cuts_of(len(ev), 3)
    orc = O.Oracle(max_slot_chain_size=0)
    w.install(orc)
    do = np.concatenate([orc.submit(ev[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
    nodes = {int(x): orc.read_node(int(x)) for x in CU.sample(ev, w.n_res, k=50)}
    orc.close()
    st = (do & 0xFF)[(ev["kind"] == A.EV_ENTRY) & ((ev["flags"] & A.F_ENTRY_OUT) == 0)]
    assert (st == A.BLOCK_PARAM).sum() > 100
    eng = _engine(w, param_table_log2=20)
    d, rp = _run(eng, ev, do, cuts, nodes)
    rp.close()


def test_submit_ex_contexts_and_null_contexts():
    # origins, named contexts and NullContext ids (above SG_MAX_CONTEXTS): SG_NO_CHECK entries and their exits are
    # not counted
    w = T.Workload(4, n_entries=20_000, n_res=500)
    ev, out_res = IU.mark_out(w.events, w.n_res, frac=0.3)
    cuts = CU.cuts_of(len(ev), 3)
    orc = O.Oracle(max_slot_chain_size=0)
    w.install(orc)
    eng = _engine(w, aux_node_capacity=1 << 18)
    io, ic = w.intern_names(orc, 16, 4)
    io2, ic2 = w.intern_names(eng, 16, 4)
    assert np.array_equal(io, io2) and np.array_equal(ic, ic2)
    ic_all = np.concatenate([ic, np.array([0, A.MAX_CONTEXTS + 1, A.MAX_CONTEXTS + 7], dtype=np.uint32)])
    ext = T.ext_for(ev, np.concatenate([io, np.zeros(1, dtype=np.uint32)]), ic_all, seed=T.SEED_BASE + 77)
    null_ctx = ext["context_id"] > A.MAX_CONTEXTS
    do = np.concatenate([orc.submit_ex(ev[a:b], ext[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
    nodes = {int(x): orc.read_node(int(x)) for x in CU.sample(ev, w.n_res, k=50)}
    orc.close()
    st = (do & 0xFF)[ev["kind"] == A.EV_ENTRY]
    assert (st == A.NO_CHECK).sum() > 1_000 and null_ctx.sum() > 2_000
    d, rp = _run(eng, ev, do, cuts, nodes, ext=ext, null_ctx=null_ctx)
    rp.close()


def test_switch_off_leaves_the_node_empty():
    c = _counts_case("c4small", "MIXED", 3)
    eng = _engine(c.w, switch_on=0)
    for a, b in zip(c.cuts[:-1], c.cuts[1:]):
        d = eng.submit(c.ev[a:b])
        assert ((d[c.ev["kind"][a:b] == A.EV_ENTRY] & 0xFF) == A.NO_CHECK).all()
    node = eng.read_inbound_node()
    assert (node["second"][:, 0] == -1).all() and (node["minute"][:, 0] == -1).all() and node["thread"] == 0
    assert node["has_chain"] == 1 and eng.inbound_last()[2] == 0


# ---------------------------------------------------------------- the pipeline
def test_async_batches_equal_the_synchronous_run():
    c = _counts_case("c4small", "MIXED", 3)
    d = IU.derive(c.ev, c.do, c.cuts)
    rp = IU.Replay(d)
    for k in range(3):
        rp.feed(k)
    eng = _engine(c.w)
    ev = np.ascontiguousarray(c.ev)
    out = np.zeros(len(ev), dtype=np.uint32)
    for a, b in zip(c.cuts[:-1], c.cuts[1:]):
        a, b = int(a), int(b)
        eng.submit_ptr(ev.ctypes.data + a * 24, b - a, out.ctypes.data + a * 4, sync=False)
    eng.sync()
    np.testing.assert_array_equal(out, c.do)
    IU.assert_node_equal(eng.read_inbound_node(), rp.node(), "async")
    _same_cluster_nodes(eng, c.nodes)
    rp.close()


@pytest.mark.parametrize("tiny", [False, True])
def test_a_malformed_batch_leaves_the_node_alone(tiny):
    # timestamps going back, between two good batches (tiny: in calls of at most 256 events, k_tiny's own check)
    c = _counts_case("c4small", "MIXED", 3)
    cuts = np.array([0, 200, 400, 600]) if tiny else c.cuts
    n = int(cuts[-1])
    ev, do = c.ev[:n], c.do[:n]
    d = IU.derive(ev, do, cuts)
    rp = IU.Replay(d)
    eng = _engine(c.w)
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        a, b = int(a), int(b)
        if k == 1:
            bad = ev[a:b].copy()
            bad["ts"] = bad["ts"][-1] + np.arange(len(bad), dtype=np.int64)[::-1]  # every ts below the one before
            before = eng.read_inbound_node()
            with pytest.raises(E.SentinelError) as ei:
                eng.submit(bad)
            assert ei.value.code == A.SG_EINVAL
            IU.assert_node_equal(eng.read_inbound_node(), before, "after the refused batch")
        np.testing.assert_array_equal(eng.submit(ev[a:b]), do[a:b])
        rp.feed(k)
        IU.assert_node_equal(eng.read_inbound_node(), rp.node(), "after batch %d" % k)
    rp.close()


# ---------------------------------------------------------------- snapshots, the metric log, the getters
def _replayed(c, track):
    eng = _engine(c.w, track=track)
    for a, b in zip(c.cuts[:-1], c.cuts[1:]):
        eng.submit(c.ev[a:b])
    return eng


def _by_time(rows):
    return rows[np.argsort(rows["timestamp"], kind="stable")]


def test_snapshot_rows_and_the_metric_log(tmp_path):
    c = _counts_case("c4small", "MIXED", 3)
    rp = IU.Replay(IU.derive(c.ev, c.do, c.cuts))
    for k in range(3):
        rp.feed(k)
    on, off, small, logged = (_replayed(c, t) for t in (True, False, True, True))
    fields = [f for f in A.METRIC_NODE_DTYPE.names if f not in ("res_id", "reserved")]
    n_inb = n_capped = 0
    for i, now in enumerate((c.w.t_end + 10, c.w.t_end + 1500, c.w.t_end + 70_000)):
        got = on.snapshot(now, cap=1 << 18)
        mine = got["res_id"] == A.RES_TOTAL_INBOUND
        want = _by_time(rp.orc.snapshot(now))
        inb = _by_time(got[mine])
        for f in fields:
            np.testing.assert_array_equal(inb[f], want[f], err_msg="%s at %d" % (f, now))
        assert mine.sum() == 0 or (np.nonzero(mine)[0] >= (~mine).sum()).all()  # after the ClusterNodes' rows
        np.testing.assert_array_equal(CU.sorted_snapshot(got[~mine]), CU.sorted_snapshot(off.snapshot(now, cap=1 << 18)))
        n_inb += int(mine.sum())
        # a cap below the row count still reports the full count (the third engine takes the same snapshots in step)
        buf = np.zeros(2, dtype=A.METRIC_NODE_DTYPE)
        assert small.snapshot_to(now, buf.ctypes.data, 2) == len(got)
        if len(got) > 2:
            n_capped += 1
            np.testing.assert_array_equal(buf, got[:2])
    assert n_inb > 0 and n_capped > 0
    # MetricTimerListener: the node's line is the last of its second, under the reference's name
    names = {i: nm for i, nm in enumerate(c.w.names())}
    wr = ML.MetricWriter(1 << 26, base_dir=str(tmp_path), app_name="app", pid=1, now_ms=CU.T0 - 5000)
    assert ML.MetricTimerListener(logged, wr, names).run(c.w.t_end + 1500) > 0
    wr.close()
    lines = [ML.MetricNode.from_fat_string(l) for l in open(wr.cur_metric_file, encoding="utf-8") if l.strip()]
    seconds = sorted({m.timestamp for m in lines})
    assert seconds
    for ts in seconds:
        grp = [m.resource for m in lines if m.timestamp == ts]
        assert grp.count(A.TOTAL_IN_RESOURCE_NAME) == 1 and grp[-1] == A.TOTAL_IN_RESOURCE_NAME, (ts, grp[-3:])
    rp.close()


def test_inbound_metrics_against_the_replay_oracle():
    c = _counts_case("c4small", "MIXED", 3)
    eng = _engine(c.w)
    d, rp = _run(eng, c.ev, c.do, c.cuts, c.nodes)  # (the raw node first: the oracle's getters reset its bucket)
    t_last = int(c.ev["ts"][-1])
    keys = {0: "pass_qps", 1: "block_qps", 2: "success_qps", 3: "exception_qps", 4: "total_qps", 5: "avg_rt",
            6: "min_rt", 13: "max_success_qps", 15: "cur_thread_num"}
    before = eng.read_inbound_node()
    for now in (t_last, t_last + 600, t_last + 2000):
        got = eng.inbound_metrics(now)
        for which, key in keys.items():
            assert got[key] == rp.orc.metric(0, now, which), (now, key)
    assert eng.inbound_metrics(t_last)["pass_qps"] > 0 and before["thread"] == eng.inbound_metrics(t_last)["cur_thread_num"]
    IU.assert_node_equal(eng.read_inbound_node(), before, "a read-back resets no bucket")
    rp.close()


def test_off_by_default():
    c = _counts_case("c4small", "MIXED", 3)
    eng = _engine(c.w, track=False)
    with pytest.raises(E.SentinelError) as ei:
        eng.read_inbound_node()
    assert ei.value.code == A.SG_ESTATE
    eng.track_inbound(False)  # the same value twice: a no-op
    a, b = int(c.cuts[0]), int(c.cuts[1])
    np.testing.assert_array_equal(eng.submit(c.ev[a:b]), c.do[a:b])
    snap = eng.snapshot(c.w.t_end + 1500, cap=1 << 18)
    assert len(snap) > 0 and (snap["res_id"] != A.RES_TOTAL_INBOUND).all()
    with pytest.raises(E.SentinelError) as ei:
        eng.track_inbound(True)  # after the first batch
    assert ei.value.code == A.SG_ESTATE
    with pytest.raises(E.SentinelError):
        eng.read_inbound_node()


def test_turned_off_stops_counting_and_stays_readable():
    c = _counts_case("c4small", "MIXED", 3)
    eng = _engine(c.w)
    eng.track_inbound(True)  # twice: a no-op
    eng.submit(c.ev[:int(c.cuts[1])])
    first = eng.read_inbound_node()
    assert first["thread"] > 0
    eng.track_inbound(False)
    eng.submit(c.ev[int(c.cuts[1]):int(c.cuts[2])])
    IU.assert_node_equal(eng.read_inbound_node(), first, "after tracking was turned off")
    with pytest.raises(E.SentinelError) as ei:
        eng.track_inbound(True)
    assert ei.value.code == A.SG_ESTATE
