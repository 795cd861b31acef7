"""Per-namespace request limiters and connected counts of the token server on the device.

Every namespace has its own GlobalRequestLimiter (csrv/flow/statistic/limit/GlobalRequestLimiter.java:30-80) and
its own connected count (csrv/flow/rule/ClusterFlowRuleManager.java:308-317); a token request tries the limiter of
its flowId's namespace only (csrv/flow/ClusterFlowChecker.java:50-53, ClusterParamFlowChecker.java:37-40).

The expected result is one pyoracle.Oracle per namespace (an oracle is one namespace): created with the
namespace's limit, loaded with its rules only, fed its requests in order (a call with none for it is skipped), the
results scattered back.  Requests with an unknown flowId or acquire_count <= 0 go to the first oracle.  Status,
remaining and wait of every request must be identical.
"""
import numpy as np
import pytest

import pyoracle as O
from sentinel_amd import _abi as A
from sentinel_amd import engine as E

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000_123
TS = T0 - T0 % 1000
OK, TMR, BL = A.TOKEN_OK, A.TOKEN_TOO_MANY_REQUEST, A.TOKEN_BLOCKED


def _rule(fid, count, res="abc", **kw):
    kw.setdefault("cluster_threshold_type", A.CLUSTER_THRESHOLD_GLOBAL)
    return A.flow_rule(res, count, cluster_mode=True, cluster_flow_id=fid, **kw)


class NsOracles:
    """K oracles, one a namespace.  limits: {namespace: integer limit} in order (the first takes the requests
    that belong to no namespace); flow_ns: {flowId: namespace}."""

    def __init__(self, limits, flow_ns):
        self.names = list(limits)
        self.orc = {}
        for ns, lim in limits.items():
            self.orc[ns] = O.Oracle(cluster_max_allowed_qps=int(lim))
            self.orc[ns].register("abc")
        self.flow_ns = dict(flow_ns)

    def load_flow_rules(self, rules):
        for ns, o in self.orc.items():
            o.load_flow_rules([r for r in rules if self.flow_ns.get(int(r.cluster_flow_id), self.names[0]) == ns])

    def load_param_rules(self, rules):
        for ns, o in self.orc.items():
            o.load_param_rules([r for r in rules if self.flow_ns.get(int(r.cluster_flow_id), self.names[0]) == ns])

    def set_connected(self, fid, n):
        self.orc[self.flow_ns.get(fid, self.names[0])].cluster_set_connected(fid, n)

    def ns_of_requests(self, reqs):
        """Namespace position of every request (0 for a request no rule names or that is not valid)."""
        pos = {ns: k for k, ns in enumerate(self.names)}
        lut = {f: pos[ns] for f, ns in self.flow_ns.items()}
        k = np.array([lut.get(int(f), 0) for f in reqs["flow_id"]], dtype=np.int64)
        k[reqs["acquire_count"] <= 0] = 0
        return k

    def request_array(self, reqs):
        reqs = np.ascontiguousarray(reqs, dtype=A.TOKEN_REQ_DTYPE)
        out = np.zeros(len(reqs), dtype=A.TOKEN_RES_DTYPE)
        k = self.ns_of_requests(reqs)
        for j, ns in enumerate(self.names):
            sel = np.nonzero(k == j)[0]
            if len(sel):
                out[sel] = self.orc[ns].cluster_request_array(reqs[sel])
        return out

    def request(self, reqs):
        arr = np.zeros(len(reqs), dtype=A.TOKEN_REQ_DTYPE)
        for i, (ts, fid, acq, pr) in enumerate(reqs):
            arr[i] = (ts, fid, acq, int(pr))
        out = self.request_array(arr)
        return [(int(o["status"]), int(o["remaining"]), int(o["wait_in_ms"])) for o in out]

    def request_param(self, reqs):
        out = [None] * len(reqs)
        for ns in self.names:
            sel = [i for i, r in enumerate(reqs) if self.flow_ns.get(r[1], self.names[0]) == ns]
            if sel:
                for i, o in zip(sel, self.orc[ns].cluster_request_param([reqs[i] for i in sel])):
                    out[i] = o
        return out


def _engine(limits, flow_ns, **cfg):
    """An engine with the namespaces of limits (a "default" entry is the configured limit) and their flowIds."""
    if "default" in limits:
        cfg["cluster_max_allowed_qps"] = int(limits["default"])
    cfg.setdefault("max_resources", 64)
    eng = E.Engine(**cfg)
    eng.register("abc")
    for ns, lim in limits.items():
        if ns != "default":
            eng.cluster_namespace(ns, lim)
    for ns in limits:
        fids = [f for f, n in flow_ns.items() if n == ns]
        if fids and ns != "default":
            eng.cluster_assign_flows(ns, fids)
    return eng


def _assert_same(got, want, base=0):
    for k in ("status", "remaining", "wait_in_ms"):
        bad = np.nonzero(got[k] != want[k])[0]
        assert len(bad) == 0, "%s of request %d: gpu %s oracles %s (%d mismatches)" % (
            k, base + bad[0], got[bad[0]], want[bad[0]], len(bad))


# ---- 1. two limiters
def test_two_limiters():
    limits, flow_ns = {"a": 3, "b": 3}, {7: "a", 8: "b"}
    eng, orc = _engine(limits, flow_ns), NsOracles(limits, flow_ns)
    rules = [_rule(7, 100), _rule(8, 100)]
    eng.load_flow_rules(rules)
    orc.load_flow_rules(rules)
    reqs = [(TS, 7 + (i & 1), 1, False) for i in range(10)] + \
           [(TS + 999, 7, 1, False), (TS + 999, 8, 1, False), (TS + 1000, 7, 1, False), (TS + 1000, 8, 1, False)]
    got = eng.cluster_request(reqs)
    assert got == orc.request(reqs)
    for f in (7, 8):
        assert [s for (s, _, _), r in zip(got, reqs) if r[1] == f] == [OK] * 3 + [TMR] * 2 + [TMR, OK]


# ---- 2. the default namespace
@pytest.mark.parametrize("extra", [0, 3])
def test_default_namespace(extra):
    eng = E.Engine(max_resources=64, cluster_max_allowed_qps=3)
    eng.register("abc")
    orc = NsOracles({"default": 3}, {})
    for k in range(extra):  # registered, never assigned a flow
        assert eng.cluster_namespace("idle-%d" % k, 1) == k + 1
    rules = [_rule(7, 100), _rule(8, 2)]
    eng.load_flow_rules(rules)
    orc.load_flow_rules(rules)
    reqs = [(TS, 0, 1, False), (TS, 7, 0, False), (TS, 9, 1, False)] + [(TS, 7, 1, False)] * 2 + \
           [(TS + 5, 8, 1, False)] * 3 + [(TS + 999, 7, 1, False), (TS + 1000, 7, 1, False), (TS + 1000, 8, 1, False)]
    got = eng.cluster_request(reqs)
    assert got == orc.request(reqs)
    # the unassigned flows 7 and 8 share cfg.cluster_max_allowed_qps = 3
    assert [s for s, _, _ in got] == [A.TOKEN_BAD_REQUEST, A.TOKEN_BAD_REQUEST, A.TOKEN_NO_RULE_EXISTS,
                                     OK, OK, OK, TMR, TMR, TMR, OK, OK]


# ---- 3 / 4. random parity
def _random_requests(rng, n, fids, t0, bad_frac=0.02):
    ts = t0 + np.cumsum(rng.integers(0, 4, n))
    p = 1.0 / np.arange(1, len(fids) + 1) ** 1.1
    p /= p.sum()
    fid = np.asarray(fids)[rng.choice(len(fids), n, p=p)]
    acq = rng.integers(1, 4, n)
    pri = rng.random(n) < 0.3
    bad = rng.random(n)
    fid = np.where(bad < bad_frac / 2, 10 ** 9 + 7, fid)  # no rule
    acq = np.where((bad >= bad_frac / 2) & (bad < bad_frac), 0, acq)  # bad request
    out = np.zeros(n, dtype=A.TOKEN_REQ_DTYPE)
    out["ts"], out["flow_id"], out["acquire_count"], out["prioritized"] = ts, fid, acq, pri
    return out


CUTS = [(0, 1), (1, 5000), (5000, 30000), (30000, 60000)]
FIVE = {"default": -1, "ns-a": 120, "ns-b": 40, "ns-c": 3, "ns-d": 0}
_stream_cache = {}


def _stream(limits):
    """The recipe of test_gpu_cluster.test_random_parity: 40 flows, 60,000 requests; the flows dealt to the
    namespaces round-robin by rank.  (rules, connected counts, requests, flow_ns, the oracles' results): computed
    once per limit set, shared and left unchanged."""
    key = tuple(limits.items())
    if key in _stream_cache:
        return _stream_cache[key]
    rng = np.random.default_rng(20240601 + 31)
    fids = list(range(101, 141))
    names = list(limits)
    flow_ns = {f: names[i % len(names)] for i, f in enumerate(fids)}
    rules = []
    for f in fids:
        sc = int(rng.choice([1, 2, 5, 10, 20]))
        win = int(rng.choice([500, 1000, 2000]))
        thr = A.CLUSTER_THRESHOLD_GLOBAL if f % 3 else A.CLUSTER_THRESHOLD_AVG_LOCAL
        rules.append(_rule(f, float(rng.integers(5, 200)), res="r%d" % f, cluster_sample_count=sc,
                           cluster_window_interval_ms=win, cluster_threshold_type=thr))
    conn = {f: int(f % 5) for f in fids if f % 3 == 0}
    reqs = _random_requests(rng, 60_000, fids, T0)
    orc = NsOracles(limits, flow_ns)
    orc.load_flow_rules(rules)
    for f, c in conn.items():
        orc.set_connected(f, c)
    want = np.concatenate([orc.request_array(reqs[a:b]) for a, b in CUTS])
    want.setflags(write=False)
    reqs.setflags(write=False)
    _stream_cache[key] = (rules, conn, reqs, flow_ns, want, orc.ns_of_requests(reqs))
    return _stream_cache[key]


def _run_stream(limits, eng):
    rules, conn, reqs, flow_ns, want, _ = _stream(limits)
    eng.load_flow_rules(rules)
    for f, c in conn.items():
        eng.cluster_set_connected(f, c)
    for a, b in CUTS:
        _assert_same(eng.cluster_request_array(reqs[a:b]), want[a:b], a)


@pytest.mark.parametrize("light", [None, "0", "1000000"])
def test_random_parity_five_namespaces(light, monkeypatch):
    if light is not None:
        monkeypatch.setenv("SG_TOK_LIGHT", light)
    rules, conn, reqs, flow_ns, want, k = _stream(FIVE)
    # the oracles' own results: every limiter regime is in the stream
    valid = (reqs["acquire_count"] > 0) & (reqs["flow_id"] < 10 ** 9)
    frac = [float(np.mean(want["status"][valid & (k == j)] == TMR)) for j in range(5)]
    print("TOO_MANY_REQUEST fraction per namespace:", frac)
    assert frac[0] == 0.0 and 0.10 <= frac[1] <= 0.90 and 0.10 <= frac[2] <= 0.90 and frac[4] == 1.0, frac
    d = want["status"][valid & (k == 0)]
    assert (d == OK).sum() > 0 and (d == BL).sum() > 0
    _run_stream(FIVE, _engine(FIVE, flow_ns))


def test_forced_grouped_path_single_namespace(monkeypatch):
    # SG_TOK_NS=1: the namespace-grouped limiter with the one namespace "default"
    monkeypatch.setenv("SG_TOK_NS", "1")
    limits = {"default": 400}
    want = _stream(limits)[4]
    assert 0 < (want["status"] == TMR).sum() < len(want)
    _run_stream(limits, _engine(limits, {}))


# ---- 5. many small namespaces (more than one 8-bit radix pass)
def test_many_small_namespaces():
    rng = np.random.default_rng(20240601 + 32)
    K = 300
    names = ["n%03d" % k for k in range(K)]
    limits = {ns: (2 if k % 2 else -1) for k, ns in enumerate(names)}
    fids = [5001 + k for k in range(K)]
    flow_ns = dict(zip(fids, names))
    rules = [_rule(f, 1000, res="r%d" % f) for f in fids]
    n = 20_000
    reqs = np.zeros(n, dtype=A.TOKEN_REQ_DTYPE)
    reqs["ts"] = T0 + np.cumsum(rng.integers(0, 4, n))
    reqs["flow_id"] = np.asarray(fids)[rng.integers(0, K, n)]
    reqs["acquire_count"] = 1
    orc = NsOracles(limits, flow_ns)
    orc.load_flow_rules(rules)
    eng = _engine(limits, flow_ns, max_resources=512)
    eng.load_flow_rules(rules)
    cuts = np.cumsum([0, 1, 63, 64, 65, 4096])
    cuts = list(cuts) + [n]
    want = np.concatenate([orc.request_array(reqs[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
    odd = (reqs["flow_id"] - 5001) % 2 == 1
    f_odd, f_even = np.mean(want["status"][odd] == TMR), np.mean(want["status"][~odd] == TMR)
    print("TOO_MANY_REQUEST fraction: odd %.3f even %.3f" % (f_odd, f_even))
    assert 0.05 <= f_odd <= 0.95 and f_even == 0.0
    for a, b in zip(cuts[:-1], cuts[1:]):
        _assert_same(eng.cluster_request_array(reqs[a:b]), want[a:b], a)


# ---- 6. flow and param requests share a namespace's limiter
def test_flow_and_param_requests_share_the_limiter():
    limits, flow_ns = {"a": 4, "b": 4}, {7: "a", 8: "b", 17: "a", 18: "b"}
    eng, orc = _engine(limits, flow_ns), NsOracles(limits, flow_ns)
    frules = [_rule(7, 100), _rule(8, 100)]
    prules = [A.param_rule("abc", 0, 100, cluster_mode=True, cluster_flow_id=f,
                           cluster_threshold_type=A.CLUSTER_THRESHOLD_GLOBAL) for f in (17, 18)]
    for x in (eng, orc):
        x.load_flow_rules(frules)
        x.load_param_rules(prules)
    key = E.param_key("u1")
    seen = set()
    for step in range(10):
        t = TS + step * 200
        fr = [(t, 7, 1, False), (t, 8, 1, False), (t + 1, 8, 1, False)]
        pr = [(t + 2, 17, 1, [key]), (t + 2, 17, 1, [key]), (t + 3, 18, 1, [key])]
        got = eng.cluster_request(fr)
        assert got == orc.request(fr)
        gotp = eng.cluster_request_param(pr)
        assert gotp == orc.request_param(pr)
        seen |= {("f", s) for s, _, _ in got} | {("p", s) for s, _, _ in gotp}
    assert seen >= {("f", OK), ("f", TMR), ("p", OK), ("p", TMR)}


# ---- 7. a namespace with no candidate in a call keeps its limiter
def test_idle_namespace_keeps_its_window():
    limits, flow_ns = {"a": 1_000_000, "b": 3}, {7: "a", 8: "b"}
    eng, orc = _engine(limits, flow_ns), NsOracles(limits, flow_ns)
    rules = [_rule(7, 100), _rule(8, 100)]
    for x in (eng, orc):
        x.load_flow_rules(rules)
    calls = [[(TS, 8, 1, False)] * 3,
             [(TS + 500 + i // 20, 7, 1, False) for i in range(2000)],
             [(TS + 900, 8, 1, False)], [(TS + 999, 8, 1, False)], [(TS + 1000, 8, 1, False)],
             [(TS + 1001, 8, 1, False)]]
    got = [eng.cluster_request(c) for c in calls]
    assert got == [orc.request(c) for c in calls]
    # b's three of TS still count at TS + 900 and TS + 999; TS + 1000 falls into the slot of TS's bucket, which
    # LeapArray.currentWindow resets (as in test_two_limiters), so it and TS + 1001 pass
    assert [g[0][0] for g in got[2:]] == [TMR, TMR, OK, OK]


# ---- 8. connected counts
def test_namespace_connected_counts():
    limits, flow_ns = {"a": -1, "b": -1}, {7: "a", 8: "b", 9: "a"}
    eng, orc = _engine(limits, flow_ns), NsOracles(limits, flow_ns)
    avg = dict(cluster_threshold_type=A.CLUSTER_THRESHOLD_AVG_LOCAL)
    rules = [_rule(7, 2, **avg), _rule(8, 2, **avg)]
    for x in (eng, orc):
        x.load_flow_rules(rules)
    eng.cluster_set_namespace_connected("a", 3)
    eng.cluster_set_namespace_connected("b", 1)
    orc.set_connected(7, 3)
    orc.set_connected(8, 1)
    reqs = [(TS, f, 1, False) for f in (7, 8) for _ in range(8)]
    got = eng.cluster_request(reqs)
    assert got == orc.request(reqs)
    assert [s for s, _, _ in got] == [OK] * 6 + [BL] * 2 + [OK] * 2 + [BL] * 6
    # a flow of "a" loaded after the call starts with the namespace's count
    rules.append(_rule(9, 2, **avg))
    for x in (eng, orc):
        x.load_flow_rules(rules)
    for f, c in ((7, 3), (8, 1), (9, 3)):
        orc.set_connected(f, c)
    reqs = [(TS + 2000, f, 1, False) for f in (7, 8, 9) for _ in range(8)]
    got = eng.cluster_request(reqs)
    assert got == orc.request(reqs)
    assert [s for s, _, _ in got][16:] == [OK] * 6 + [BL] * 2
    # the per-flow call overrides the namespace's count for that flow; the last call wins
    eng.cluster_set_connected(7, 1)
    orc.set_connected(7, 1)
    reqs = [(TS + 4000, f, 1, False) for f in (7, 9) for _ in range(8)]
    got = eng.cluster_request(reqs)
    assert got == orc.request(reqs)
    assert [s for s, _, _ in got] == [OK] * 2 + [BL] * 6 + [OK] * 6 + [BL] * 2
    eng.cluster_set_namespace_connected("a", 2)
    orc.set_connected(7, 2)
    orc.set_connected(9, 2)
    reqs = [(TS + 6000, f, 1, False) for f in (7, 9) for _ in range(8)]
    got = eng.cluster_request(reqs)
    assert got == orc.request(reqs)
    assert [s for s, _, _ in got] == ([OK] * 4 + [BL] * 4) * 2


# ---- 9. a limit change keeps the window (RequestLimiter.setQpsAllowed; canPass: sum + 1 <= qpsAllowed,
# RequestLimiter.java:72-87).  Written out by hand: an oracle's limit is fixed at its creation
def test_limit_change_keeps_the_window():
    eng = E.Engine(max_resources=64)
    eng.register("abc")
    a = eng.cluster_namespace("a", 5)
    c = eng.cluster_namespace("c", 2.5)
    assert (a, c) == (1, 2)
    eng.cluster_assign_flows("a", [7])
    eng.cluster_assign_flows("c", [8])
    eng.load_flow_rules([_rule(7, 100), _rule(8, 100)])
    assert [s for s, _, _ in eng.cluster_request([(TS, 7, 1, False)] * 5)] == [OK] * 5
    assert eng.cluster_namespace("a", 8) == a  # five of the window's eight are taken
    assert [s for s, _, _ in eng.cluster_request([(TS + 10, 7, 1, False)] * 5)] == [OK] * 3 + [TMR] * 2
    assert eng.cluster_namespace_qps("a", TS + 10) == (8.0, 8.0)
    # a fractional limit: 0 + 1 <= 2.5, 1 + 1 <= 2.5, 2 + 1 > 2.5
    assert [s for s, _, _ in eng.cluster_request([(TS + 20, 8, 1, False)] * 4)] == [OK] * 2 + [TMR] * 2
    # lowered below what the window holds: nothing passes until the window has moved on
    eng.cluster_namespace("a", 2)
    assert [s for s, _, _ in eng.cluster_request([(TS + 30, 7, 1, False), (TS + 999, 7, 1, False)] +
                                                [(TS + 1000, 7, 1, False)] * 3)] == [TMR, TMR, OK, OK, TMR]


# ---- 10. read-back and errors
def test_namespace_qps_read_back():
    eng = E.Engine(max_resources=64, cluster_max_allowed_qps=77)
    eng.register("abc")
    eng.cluster_namespace("a", 10)
    eng.cluster_assign_flows("a", [7])
    eng.load_flow_rules([_rule(7, 1000), _rule(8, 1000)])
    assert eng.cluster_namespace_qps("a", TS) == (0.0, 10.0)
    assert eng.cluster_namespace_qps("default", TS) == (0.0, 77.0)
    st = [s for s, _, _ in eng.cluster_request([(TS, 7, 1, False)] * 4 + [(TS + 300, 7, 1, False)] * 8 +
                                               [(TS + 300, 8, 1, False)] * 2)]
    assert st == [OK] * 4 + [OK] * 6 + [TMR] * 2 + [OK] * 2
    # the passes of the last second, not the refused requests; unchanged by reading
    for _ in range(2):
        assert eng.cluster_namespace_qps("a", TS + 300) == (10.0, 10.0)
        assert eng.cluster_namespace_qps("default", TS + 300) == (2.0, 77.0)
        assert eng.cluster_namespace_qps("a", TS + 999)[0] == 10.0
        assert eng.cluster_namespace_qps("a", TS + 1000)[0] == 6.0   # the bucket of TS is the slot of TS + 1000
        assert eng.cluster_namespace_qps("a", TS + 1299)[0] == 6.0
        assert eng.cluster_namespace_qps("a", TS + 1300)[0] == 0.0
    # ... and the limiter still holds what it held: four free again at TS + 1000
    assert [s for s, _, _ in eng.cluster_request([(TS + 1000, 7, 1, False)] * 5)] == [OK] * 4 + [TMR]


def _code(fn, *a):
    with pytest.raises(E.SentinelError) as ei:
        fn(*a)
    return ei.value.code


def test_namespace_errors():
    eng = E.Engine(max_resources=64)
    assert eng.cluster_namespace("default", 30000) == 0
    assert _code(eng.cluster_namespace, "", 1) == A.SG_EINVAL
    assert _code(eng.cluster_namespace, None, 1) == A.SG_EINVAL
    assert eng.cluster_namespace("a", 1) == 1 and eng.cluster_namespace("b", 1) == 2
    assert eng.cluster_namespace("a", 9) == 1  # idempotent
    assert _code(eng.cluster_assign_flows, "nope", [7]) == A.SG_ENOTFOUND
    assert _code(eng.cluster_assign_flows, "a", [7, 0]) == A.SG_EINVAL
    assert _code(eng.cluster_assign_flows, "a", [-7]) == A.SG_EINVAL
    eng.cluster_assign_flows("a", [7, 8])
    eng.cluster_assign_flows("a", [7])  # the same namespace: a no-op
    assert _code(eng.cluster_assign_flows, "b", [9, 7]) == A.SG_ESTATE
    eng.cluster_assign_flows("b", [9])  # (nothing of the refused call was assigned)
    assert _code(eng.cluster_set_namespace_connected, "nope", 1) == A.SG_ENOTFOUND
    assert _code(eng.cluster_namespace_qps, "nope", TS) == A.SG_ENOTFOUND
    for k in range(3, 1024):
        assert eng.cluster_namespace("n%d" % k, -1) == k
    assert _code(eng.cluster_namespace, "one-too-many", 1) == A.SG_ECAPACITY
    assert eng.cluster_namespace("n1023", 5) == 1023  # a registered one still takes a new limit
