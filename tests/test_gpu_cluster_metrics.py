"""sg_cluster_metrics / sg_param_key_value on the device (sentinel_amd/csrc/cmetrics.hip, engine.cpp) against the
sequential model of tests/cmetrics_util.py, bit for bit: every row of every read, and after every read the decisions
of the rest of the stream against the oracle, which was never read (the read-back property).

The scenarios live in cmetrics_util.py, where test_cluster_metrics_host.py pins the model to the oracle on the same
streams.  Window edges: a valid cluster rule has windowIntervalMs % sampleCount == 0, so a bucket's start + interval
is the start of the same slot's next window and the read-back's reset empties the bucket at that instant; the reads at
start + interval - 1, + 0 and + 1 pin that (the strict > of isWindowDeprecated cannot keep it).  Chunk edges: where in
a chunk a winner lands follows the order in which the scan's waves append, which a test cannot set; the chunk cases
place 7 winners at random among C - 1, C, C + 1 and 2 C + 1 candidates (C from the diagnostics getter) instead.
ClusterMetricNodeGenerator: csrv/flow/statistic/ClusterMetricNodeGenerator.java:39-105."""
import numpy as np
import pytest

import pyoracle as O
from sentinel_amd import _abi as A
from sentinel_amd import engine as E
from sentinel_amd import token_server as TS

import cmetrics_util as U

pytestmark = pytest.mark.gpu

CHUNK = 4096  # the chunk-* scenarios are built around it; the getter must agree


def _pair(monkeypatch, env=None, **cfg):
    monkeypatch.setenv("SG_PTOK_MIN", "0")  # the value-parallel owner at these sizes, whatever the default is
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, str(v))
    cfg.setdefault("cluster_max_allowed_qps", U.BIG)
    eng = E.Engine(max_resources=64, **cfg)
    orc = O.Oracle(**cfg)
    for x in (eng, orc):
        x.register("abc")
    return eng, orc


PLAIN = sorted(k for k in U.SCENARIOS if k.startswith(("edges-", "top-", "occupy", "wide-", "reloads")) and
               k != "top-rehash")


@pytest.mark.parametrize("name", PLAIN)
def test_rows_and_later_decisions(name, monkeypatch):
    eng, orc = _pair(monkeypatch)
    steps = U.SCENARIOS[name]()
    model, reads, _ = U.run(steps, orc, eng)
    assert reads and not model.mismatches
    if name.startswith("edges-"):
        # the read after the idle gap: nothing is listed while the values' slots still sit in the table
        idle = [got for now, got in reads if not got["n_top"].any() and not got["pass_qps"].any()]
        assert idle and eng.cluster_param_table_stats()["claimed_ub"] > 0
        assert any(got["n_top"].max() >= 2 for _, got in reads)
    if name == "occupy":
        # reads: t + 800, t + 999 (before the transfer window), t + 1000, t + 1199 (inside it, before any request),
        # then t + 1000 again after the request that made the transfer
        qps = [float(got[got["flow_id"] == 98765][0]["pass_qps"]) for _, got in reads]
        assert qps[:5] == [5.0, 5.0, 4.0, 4.0, 5.0]  # bucket 0 emptied on the copy (- 2) and the occupied pass in it (+ 1)
    if name == "wide-sums":
        got = reads[0][1][0]
        assert [int(k) for k in got["top_key"][:3]] == [0x10, 0x30, 0x20]
        assert got["top_qps"][0] == float(2 ** 32 + 1) and 2.0 ** 31 < got["top_qps"][1] < 2.0 ** 32


def test_empty_and_small_inputs(monkeypatch):
    eng, orc = _pair(monkeypatch)
    T = U.T0
    assert len(eng.cluster_metrics(T)) == 0 and eng.cluster_metrics_count(T) == 0      # no cluster rules
    steps = [("flow_rules", [U.fspec(9, 5), U.fspec(3, 5, 2, 500)]),
             ("param_rules", [U.pspec(40, 5), U.pspec(20, 5, 16, 1600), U.pspec(30, 5)]),
             ("read", T, 5, None, None),                                                # rules with no traffic
             ("flow", U.flow_reqs([(T + i, 3 + 6 * (i % 2), 1, False) for i in range(12)])),
             U.param_reqs([(T + i, 20 + 10 * (i % 3), 1, [i % 4]) for i in range(30)]),
             ("read", T + 40, 5, None, None)]
    tail = [("flow", U.flow_reqs([(T + 50 + i, 3, 1, False) for i in range(4)])),
            U.param_reqs([(T + 60 + i, 20, 1, [i % 2]) for i in range(6)])]
    model, reads, _ = U.run(steps + tail, orc, eng)
    zero = reads[0][1]
    assert [int(f) for f in zero["flow_id"]] == [3, 9, 20, 30, 40]
    assert [int(k) for k in zero["kind"]] == [A.CM_FLOW] * 2 + [A.CM_PARAM] * 3
    assert not zero["pass_qps"].any() and not zero["block_qps"].any() and not zero["n_top"].any()
    assert (zero["res_id"] == eng.resource_id("abc")).all()
    full = eng.cluster_metrics(T + 40)
    assert eng.cluster_metrics_count(T + 40) == 5 == len(full)
    cut = eng.cluster_metrics(T + 40, cap=2)                                            # cap below n truncates
    assert len(cut) == 2 and cut.tobytes() == full[:2].tobytes()
    for top in (0, 9):
        with pytest.raises(E.SentinelError) as ei:
            eng.cluster_metrics(T, top=top)
        assert ei.value.code == A.SG_EINVAL
    with pytest.raises(E.SentinelError) as ei:
        eng.cluster_metrics(T, ns="nobody")
    assert ei.value.code == A.SG_ENOTFOUND
    more = U.flow_reqs([(T + 70 + i, 3 + 6 * (i % 2), 1, False) for i in range(8)])     # and the decisions go on
    U._same(eng.cluster_request_array(more), orc.cluster_request_array(more), more, "after the refused reads")


def test_three_namespaces(monkeypatch):
    eng, orc = _pair(monkeypatch)
    steps, ns = U.namespaces()
    for name, ids in ns.items():
        if name != "default":
            eng.cluster_namespace(name, U.BIG)
            eng.cluster_assign_flows(name, ids)
    model, reads, _ = U.run(steps, orc, eng)
    sizes = [len(got) for _, got in reads]
    assert sizes == [2, 3, 2, 7, 7], sizes
    assert any(got["n_top"].any() for _, got in reads)


def _reads_equal(a, b):
    assert len(a) == len(b)
    for (ta, ga), (tb, gb) in zip(a, b):
        assert ta == tb and ga.tobytes() == gb.tobytes(), (ta, ga, gb)


def test_rows_do_not_depend_on_the_tables_capacity(monkeypatch):
    """The same history on an engine whose table starts at 2^10 slots and rehashes and grows between the reads."""
    steps = U.SCENARIOS["top-rehash"]()
    eng, orc = _pair(monkeypatch)
    _, reads, _ = U.run(steps, orc, eng)
    small, orc2 = _pair(monkeypatch, env={"SG_PV_LOG2": 10})
    _, reads2, _ = U.run(U.SCENARIOS["top-rehash"](), orc2, small)
    s = small.cluster_param_table_stats()
    print("small table:", s)
    assert s["rehashes"] > 0 and s["resizes"] > 0 and eng.cluster_param_table_stats()["rehashes"] == 0
    _reads_equal(reads, reads2)


def test_rows_do_not_depend_on_the_owner(monkeypatch):
    """The same stream (multi-value requests, a value listed twice) with SG_PTOK_VP=0 and with the default."""
    eng, orc = _pair(monkeypatch)
    _, reads, _ = U.run(U.SCENARIOS["owners"](), orc, eng)
    st = eng.cluster_param_owner_stats()
    assert st["value_parallel_requests"] > 0 and st["flow_lane_requests"] > 0, st
    lane, orc2 = _pair(monkeypatch, env={"SG_PTOK_VP": 0})
    _, reads2, _ = U.run(U.SCENARIOS["owners"](), orc2, lane)
    assert lane.cluster_param_owner_stats()["value_parallel_requests"] == 0
    _reads_equal(reads, reads2)
    assert all(got["n_top"].max() == 5 for _, got in reads)


@pytest.mark.parametrize("count", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_chunk_edges(count, monkeypatch):
    eng, orc = _pair(monkeypatch)
    model, reads, _ = U.run(U.SCENARIOS["chunk-%d" % count](), orc, eng)
    last = eng.cluster_metrics_last()
    print("chunk case %d:" % count, last)
    assert last["chunk_size"] == CHUNK
    assert last["candidates"] == count + 2                       # flow 700's values and flow 701's two
    assert last["chunks"] == (count + CHUNK - 1) // CHUNK + 1    # ... in chunks of at most C, one flow a chunk
    top = reads[1][1][reads[1][1]["flow_id"] == 700][0]
    assert top["n_top"] == 8 and list(top["top_qps"][:7]) == [9.0, 9.0, 8.0, 8.0, 8.0, 7.0, 6.0]


def test_hot_flow_beside_many_small_flows(monkeypatch):
    eng, orc = _pair(monkeypatch)
    model, reads, _ = U.run(U.SCENARIOS["hot-and-many"](), orc, eng)
    last = eng.cluster_metrics_last()
    print("hot flow beside small flows:", last, eng.cluster_param_table_stats())
    now, got = reads[0]
    live = {fid: len(m.read(now, 1 << 30)) for fid, m in model.pflows.items()}  # values with a sum > 0, flow by flow
    assert len(got) == 3001 and live[1000] > 69_000 and got["n_top"][0] == 5
    assert last["candidates"] == sum(live.values())
    assert last["chunks"] == sum((v + CHUNK - 1) // CHUNK for v in live.values()) > 1000 + 16
    assert 1 <= max(v for fid, v in live.items() if fid != 1000) <= 3


# every class ParamFlowRuleUtil.parseItemValue types (ParamFlowRuleUtil.java:85-121): text, class, the class reported
VALUES = [("hello", "java.lang.String", "java.lang.String"), ("", None, "java.lang.String"),
          ("-17", "int", "int"), ("2147483647", "java.lang.Integer", "int"),
          ("123456789012", "long", "long"), ("-5", "java.lang.Long", "long"),
          ("576460752303423488", "long", "long"), ("-9223372036854775808", "java.lang.Long", "long"),
          ("1.5", "double", "double"), ("-0.0", "java.lang.Double", "double"), ("1e300", "double", "double"),
          ("0.1", "float", "float"), ("-3.5", "java.lang.Float", "float"),
          ("-3", "byte", "byte"), ("127", "java.lang.Byte", "byte"),
          ("-32768", "short", "short"), ("7", "java.lang.Short", "short"),
          ("true", "boolean", "boolean"), ("FALSE", "java.lang.Boolean", "boolean"), ("x", "char", "char")]
HASHED = {"java.lang.String", "double"}


def _same_value(cls, text, want):
    if cls in ("double", "float"):
        a, b = float(text), float(want)
        if cls == "float":
            a, b = np.float32(a), np.float32(b)
        return a == b and np.signbit(a) == np.signbit(b)
    if cls == "boolean":
        return text == want.lower()
    return text == want


def test_param_key_value_round_trips(monkeypatch):
    eng, _ = _pair(monkeypatch)
    for text, cls, rep in VALUES:
        key = eng.param_intern(text, cls)
        got = eng.param_key_value(key)
        assert got is not None and got[0] == rep and _same_value(rep, got[1], text), (text, cls, key, got)
        assert eng.param_intern(got[1], got[0]) == key, (text, cls, got)  # the answer names the same value
    fresh, _ = _pair(monkeypatch)  # nothing interned: the pure keys alone
    for text, cls, rep in VALUES:
        key = E.param_key(text, cls)
        got = fresh.param_key_value(key)
        hashed = rep in HASHED or (rep == "long" and not -(1 << 59) <= int(text) < (1 << 59))
        if hashed and not (rep == "long"):
            assert got is None, (text, cls, got)  # a pure hashed key has no entry
        elif not hashed:
            assert got is not None and got[0] == rep and _same_value(rep, got[1], text), (text, cls, key, got)
    assert fresh.param_key_value(0) is None
    import ctypes as C
    fn = E._cmetrics("sg_param_key_value")
    ct, val = C.create_string_buffer(32), C.create_string_buffer(8)
    assert fn(eng.h, eng.param_intern("hello"), ct, 32, val, 5) == A.SG_EINVAL   # a buffer too small for "hello" + NUL
    assert fn(eng.h, eng.param_intern("hello"), ct, 32, val, 6) == 5 and val.value == b"hello"
    assert fn(eng.h, eng.param_intern("hello"), ct, 4, val, 8) == A.SG_EINVAL


def test_metric_list_over_a_replay_clock(monkeypatch):
    eng, orc = _pair(monkeypatch)
    T = U.T0 - U.T0 % 1000 + 1000
    clock = iter([T + 500, T + 900])
    srv = TS.TokenServer(eng, flow_namespaces={601: "shop"}, clock=lambda: next(clock), param_key=eng.param_intern)
    srv.resource_names[eng.resource_id("abc")] = "abc"
    texts = ["alice", "bob", "carol"]
    keys = [int(eng.param_intern(t)) for t in texts]
    ghost = E.param_key("nobody-interned-this")  # a pure hashed key: it does not resolve
    assert eng.param_key_value(ghost) is None
    rows = [(T + i, 600, 1 + i % 3, [keys[i % 3]]) for i in range(9)] + [(T + 20, 600, 4, [ghost]), (T + 21, 601, 2, [keys[0]])]
    steps = [("flow_rules", [U.fspec(7, 10)]), ("param_rules", [U.pspec(600, 50), U.pspec(601, 50)]),
             ("flow", U.flow_reqs([(T + i, 7, 2, False) for i in range(7)])), U.param_reqs(rows),
             ("read", T + 500, 5, None, None), U.param_reqs([(T + 600, 600, 1, [keys[1]])])]
    model, reads, _ = U.run(steps, orc, eng)
    ml = srv.metric_list("default")           # the clock: T + 500
    assert list(ml) == ["abc"]
    nodes = {n["flowId"]: n for n in ml["abc"]}
    assert sorted(nodes) == [7, 600]          # 601 belongs to "shop"
    want = model.pflows[600].read(T + 500, 5)
    names = {keys[0]: "alice", keys[1]: "bob", keys[2]: "carol", ghost: "#%016x" % ghost}
    assert nodes[600]["topParams"] == {names[k]: s / 1.0 for k, s in want} and len(want) == 4
    assert list(nodes[600]["topParams"]) == [names[k] for k, _ in want]   # hottest first
    assert nodes[7]["passQps"] == model.flows[7].read(T + 500)[0] / 1.0 and nodes[7]["topParams"] == {}
    assert set(nodes[7]) == {"timestamp", "resourceName", "flowId", "passQps", "blockQps", "rt", "topParams"}
    assert nodes[7]["timestamp"] == T + 500 and nodes[7]["rt"] == 0 and nodes[7]["resourceName"] == "abc"
    shop = srv.metric_list("shop")            # the clock: T + 900
    assert [n["flowId"] for n in shop["abc"]] == [601] and shop["abc"][0]["topParams"] == {"alice": 2.0}
    assert srv.metric_list("nowhere", now=T) == {}
    with pytest.raises(ValueError):
        srv.metric_list("")
    _, arr, vals = U.param_reqs([(T + 950 + i, 600 + i % 2, 1, [keys[i % 3]]) for i in range(6)])
    U._same(eng.cluster_request_param_array(arr, vals), U.oracle_param(orc, arr, vals), arr, "after metric_list")
