"""PARAM_FLOW token requests from device buffers, decided per (flowId, value) chain (sentinel_amd/csrc/ptok.h,
cluster.hip k_ptok_*, engine.cpp sg_cluster_request_param_tokens).

Every request's (status, remaining, wait) is compared with the oracle's.  The base stream: 10 GLOBAL flows with
count 5 + 3 i whose (sampleCount, windowIntervalMs) cycle through SHAPES, 3 calls of 4,099 single-value requests of
about 2 s each (ts steps of 0 or 1 ms), Zipf(1.3) values capped at 2,000 and tagged with the flow, acquire 1 to 3:
more distinct pairs a call than one 1024-lane workgroup has lanes, and a longest chain longer than a wave (both
asserted on the stream).  A parity case asserts on the oracle's results that OK and BLOCKED are each at least 20 % of
every call that is a full stream (so a broken sum cannot hide behind a stream that blocks nothing); the calls that
are built to be something else (a single request, a call in which nothing reaches the flow stage, the little calls
around a refusal) are exempt, and say so where they are built.
SG_PTOK_MIN is pinned to 0 so that the value-parallel owner runs at these sizes whatever the default is.
ClusterParamFlowChecker.acquireClusterToken: csrv/flow/ClusterParamFlowChecker.java:42-88."""
import numpy as np
import pytest
import torch

import pyoracle as O
from sentinel_amd import _abi as A
from sentinel_amd import engine as E

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000_000
OK, BL = A.TOKEN_OK, A.TOKEN_BLOCKED
GLOBAL, AVG_LOCAL = A.CLUSTER_THRESHOLD_GLOBAL, A.CLUSTER_THRESHOLD_AVG_LOCAL
SHAPES = [(10, 1000), (5, 500), (2, 1000), (1, 200), (16, 1600)]  # (sampleCount, windowIntervalMs)
FIDS = [100 + i for i in range(10)]
N_CALL = 4099
BIG = 10_000_000  # a namespace limit no stream here reaches


def _prule(fid, count, items=None, thr=GLOBAL, shape=(10, 1000)):
    return A.param_rule("abc", 0, count, cluster_mode=True, cluster_flow_id=fid, cluster_threshold_type=thr,
                        items=items or (), cluster_sample_count=shape[0], cluster_window_interval_ms=shape[1])


def _base_rules():
    return [_prule(fid, 5 + 3 * i, shape=SHAPES[i % 5]) for i, fid in enumerate(FIDS)]


def _call(rng, t0, n=N_CALL, fids=FIDS):
    """One call of n single-value requests from t0 on: (PARAM_TOKEN_REQ_DTYPE rows, uint64 values)."""
    arr = np.zeros(n, dtype=A.PARAM_TOKEN_REQ_DTYPE)
    arr["ts"] = t0 + np.cumsum(rng.integers(0, 2, n))
    f = rng.integers(0, len(fids), n)
    arr["flow_id"] = np.asarray(fids, dtype=np.int64)[f]
    arr["acquire_count"] = rng.integers(1, 4, n)
    arr["n_values"] = 1
    arr["value_off"] = np.arange(n, dtype=np.uint64)
    vals = (np.minimum(rng.zipf(1.3, n), 2000).astype(np.uint64)) | (arr["flow_id"].astype(np.uint64) << np.uint64(32))
    return arr, vals


def _base_calls(seed=7):
    rng = np.random.default_rng(seed)
    return [_call(rng, T0 + 2500 * k) for k in range(3)]


def _oracle_call(orc, arr, vals):
    want = np.zeros(max(1, len(arr)), dtype=A.TOKEN_RES_DTYPE)
    v = np.ascontiguousarray(vals if len(vals) else np.zeros(1), dtype=np.uint64)
    assert O.lib().or_cluster_request_param_tokens(orc.h, arr.ctypes.data, len(arr), v.ctypes.data, len(vals),
                                                   want.ctypes.data) == 0
    return want[: len(arr)]


def _engine(monkeypatch, rules, env=None, **cfg):
    monkeypatch.setenv("SG_PTOK_MIN", "0")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, str(v))
    eng = E.Engine(max_resources=64, **cfg)
    eng.register("abc")
    eng.load_param_rules(rules)
    return eng


def _oracle(rules, **cfg):
    orc = O.Oracle(**cfg)
    orc.register("abc")
    orc.load_param_rules(rules)
    return orc


def _device_call(eng, arr, vals):
    """The call through device tensors: nothing of it is host memory."""
    n, nv = len(arr), len(vals)
    t = torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).cuda()
    v = torch.from_numpy(np.ascontiguousarray(vals, dtype=np.uint64).view(np.int64).copy()).cuda() if nv else \
        torch.zeros(1, dtype=torch.int64, device="cuda")
    out = torch.full((max(1, n) * A.TOKEN_RES_DTYPE.itemsize,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # (the engine's own stream reads the tensors)
    eng.cluster_request_param_ptr(t.data_ptr(), n, v.data_ptr(), nv, out.data_ptr())
    return out.cpu().numpy().view(A.TOKEN_RES_DTYPE)[:n]


def _equal(got, want, arr, what):
    for f in ("status", "remaining", "wait_in_ms"):
        bad = np.flatnonzero(got[f] != want[f])
        assert not len(bad), (what, f, int(bad[0]), arr[bad[0]], got[bad[0]], want[bad[0]], len(bad))


def _both_ways(want, what):
    n = len(want)
    ok, bl = int((want["status"] == OK).sum()), int((want["status"] == BL).sum())
    print("%s: %d requests, %.1f %% OK, %.1f %% BLOCKED" % (what, n, 100.0 * ok / n, 100.0 * bl / n))
    assert ok >= 0.2 * n and bl >= 0.2 * n, (what, n, ok, bl)


def _stats(eng):
    s = eng.cluster_param_owner_stats()
    return s["value_parallel_requests"], s["flow_lane_requests"], s["flows_kept_serial"]


@pytest.fixture(scope="module")
def base():
    """The base stream and the oracle's answers to it, computed once and left unchanged."""
    calls = _base_calls()
    orc = _oracle(_base_rules(), cluster_max_allowed_qps=BIG)
    want = [_oracle_call(orc, a, v) for a, v in calls]
    for k, ((a, v), w) in enumerate(zip(calls, want)):
        _both_ways(w, "base call %d" % k)
        pairs, counts = np.unique(v, return_counts=True)
        assert len(pairs) > 1024 and counts.max() > 64, (len(pairs), counts.max())
        a.setflags(write=False), v.setflags(write=False), w.setflags(write=False)
    return calls, want


# ---- 1. device tensors, every request on the value-parallel owner
def test_base_stream_from_device_tensors(base, monkeypatch):
    calls, want = base
    eng = _engine(monkeypatch, _base_rules(), cluster_max_allowed_qps=BIG)
    assert _stats(eng) == (0, 0, 0)
    for k, ((a, v), w) in enumerate(zip(calls, want)):
        _equal(_device_call(eng, a, v), w, a, "call %d" % k)
    assert _stats(eng) == (3 * N_CALL, 0, 0)
    assert set(eng.cluster_param_table_stats()) == {"capacity", "claimed_ub", "live_kept", "rehashes", "resizes",
                                                    "rehash_us", "max_capacity"}


# ---- 2. the same from host arrays
def test_base_stream_from_host_arrays(base, monkeypatch):
    calls, want = base
    eng = _engine(monkeypatch, _base_rules(), cluster_max_allowed_qps=BIG)
    for k, ((a, v), w) in enumerate(zip(calls, want)):
        _equal(eng.cluster_request_param_array(a, v), w, a, "call %d" % k)
    assert _stats(eng) == (3 * N_CALL, 0, 0)


# ---- 3. a fresh pair asked many times in the call where it first appears
def test_fresh_pair_asked_many_times_in_its_first_call(monkeypatch):
    """200 lanes meet on one (flow, value) the table does not hold: a pair claimed twice would split its counts over
    two slots and pass too much, here or in the two calls that ask it again."""
    rng = np.random.default_rng(31)
    fresh = np.uint64(0xF00D) | (np.uint64(FIDS[5]) << np.uint64(32))
    calls = []
    for k in range(3):
        a, v = _call(rng, T0 + 600 * k, n=1200)
        at = np.sort(rng.choice(1200, 200, replace=False))
        a["flow_id"][at] = FIDS[5]
        v[at] = fresh
        calls.append((a, v))
    eng = _engine(monkeypatch, _base_rules(), cluster_max_allowed_qps=BIG)
    orc = _oracle(_base_rules(), cluster_max_allowed_qps=BIG)
    for k, (a, v) in enumerate(calls):
        w = _oracle_call(orc, a, v)
        _both_ways(w, "fresh call %d" % k)
        at = np.flatnonzero(v == fresh)
        assert len(at) == 200
        print("fresh pair, call %d: %d OK, %d BLOCKED" % (k, (w["status"][at] == OK).sum(), (w["status"][at] == BL).sum()))
        if k == 0:
            assert {OK, BL} <= set(w["status"][at].tolist())
        _equal(_device_call(eng, a, v), w, a, "call %d" % k)
    assert _stats(eng) == (3 * 1200, 0, 0)


# ---- 4. hot items, AVG_LOCAL and a threshold of 0
def test_hot_items_avg_local_and_threshold_zero(monkeypatch):
    lo, hi = O.param_key("cheap", "java.lang.String"), O.param_key("vip", "java.lang.String")
    items = [("cheap", "java.lang.String", 1), ("vip", "java.lang.String", 40)]
    rules = [_prule(201, 6, items=items), _prule(202, 6, items=items, shape=(5, 500)),
             _prule(203, 3, thr=AVG_LOCAL), _prule(204, 2, thr=AVG_LOCAL, shape=(2, 1000)),
             _prule(205, 0), _prule(206, 9, shape=(16, 1600))]
    fids = [201, 202, 203, 204, 205, 206]
    eng = _engine(monkeypatch, rules, cluster_max_allowed_qps=BIG)
    orc = _oracle(rules, cluster_max_allowed_qps=BIG)
    rng = np.random.default_rng(41)
    seen_hot = set()
    for k, conn in enumerate([1, 4, 2]):
        for x in (eng, orc):
            x.cluster_set_connected(203, conn)
            x.cluster_set_connected(204, conn + 1)
        a, v = _call(rng, T0 + 1500 * k, n=3001, fids=fids)
        hot = np.flatnonzero((a["flow_id"] <= 202) & (rng.random(len(a)) < 0.5))
        v[hot] = np.where(rng.random(len(hot)) < 0.5, np.uint64(lo), np.uint64(hi))
        w = _oracle_call(orc, a, v)
        _both_ways(w, "hot call %d" % k)
        assert set(w["status"][a["flow_id"] == 205].tolist()) == {BL}  # threshold 0
        for key in (lo, hi):
            seen_hot |= {(key == lo, int(s)) for s in w["status"][v == np.uint64(key)]}
        _equal(_device_call(eng, a, v), w, a, "call %d" % k)
    assert seen_hot == {(True, OK), (True, BL), (False, OK), (False, BL)}
    assert _stats(eng) == (3 * 3001, 0, 0)


# ---- 5. requests that never reach the flow stage
def test_requests_rejected_before_the_flow_stage(monkeypatch):
    eng = _engine(monkeypatch, _base_rules(), cluster_max_allowed_qps=1500)
    orc = _oracle(_base_rules(), cluster_max_allowed_qps=1500)
    rng = np.random.default_rng(51)
    staged = 0
    for k in range(2):
        a, v = _call(rng, T0 + 2500 * k)
        kind = rng.integers(0, 40, len(a))
        a["flow_id"][kind == 0] = 0
        a["flow_id"][kind == 1] = 77777  # no rule
        a["acquire_count"][kind == 2] = 0
        a["n_values"][kind == 3] = 0
        w = _oracle_call(orc, a, v)
        _both_ways(w, "rejects call %d" % k)
        assert set(w["status"].tolist()) >= {OK, BL, A.TOKEN_BAD_REQUEST, A.TOKEN_NO_RULE_EXISTS,
                                             A.TOKEN_TOO_MANY_REQUEST}
        staged += int(((w["status"] == OK) | (w["status"] == BL)).sum())
        _equal(_device_call(eng, a, v), w, a, "call %d" % k)
    assert _stats(eng) == (staged, 0, 0)
    # a call in which no request reaches the flow stage (exempt from the 20 % rule: it has no OK and no BLOCKED)
    a, v = _call(rng, T0 + 5000, n=300)
    a["flow_id"][0::3] = 0
    a["flow_id"][1::3] = 77777
    a["n_values"][2::3] = 0
    w = _oracle_call(orc, a, v)
    assert not ({OK, BL} & set(w["status"].tolist()))
    _equal(_device_call(eng, a, v), w, a, "nothing staged")
    assert _stats(eng) == (staged, 0, 0)
    a, v = _call(rng, T0 + 8000)
    w = _oracle_call(orc, a, v)
    _both_ways(w, "after the rejects")
    _equal(_device_call(eng, a, v), w, a, "after")


# ---- 6. sizes
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1025, 4097])
def test_call_sizes(n, monkeypatch):
    """Calls of n requests (the little ones are exempt from the 20 % rule); flow FIDS[9] has exactly one request a
    call."""
    eng = _engine(monkeypatch, _base_rules(), cluster_max_allowed_qps=BIG)
    orc = _oracle(_base_rules(), cluster_max_allowed_qps=BIG)
    rng = np.random.default_rng(60 + n)
    for k in range(3):
        a, v = _call(rng, T0 + (n + 50) * k, n=n, fids=FIDS[:9])  # (a call spans at most n ms: the clock goes on)
        if n >= 2:
            a["flow_id"][n // 2] = FIDS[9]
            v[n // 2] = np.uint64(5) | (np.uint64(FIDS[9]) << np.uint64(32))
        w = _oracle_call(orc, a, v)
        if n >= 1025:
            _both_ways(w, "size %d call %d" % (n, k))
        _equal(_device_call(eng, a, v), w, a, "call %d" % k)
    assert _stats(eng) == (3 * n, 0, 0)


# ---- 7. both owners in one call
def _multi_call(rng, t0, n, multi_fids):
    """A call in which every flow of multi_fids gets multi-value requests (2 to 3 values, some repeating one)."""
    a, v1 = _call(rng, t0, n=n)
    is_multi = np.isin(a["flow_id"], multi_fids) & (rng.random(n) < 0.3)
    for fid in multi_fids:  # at least one in every such flow
        is_multi[np.flatnonzero(a["flow_id"] == fid)[0]] = True
    vals, off = [], np.zeros(n, dtype=np.uint64)
    for i in range(n):
        off[i] = len(vals)
        vals.append(int(v1[i]))
        if is_multi[i]:
            for _ in range(int(rng.integers(1, 3))):
                tag = int(a["flow_id"][i]) << 32
                vals.append(int(v1[i]) if rng.random() < 0.3 else (int(rng.integers(1, 30)) | tag))
            a["n_values"][i] = len(vals) - int(off[i])
    a["value_off"] = off
    return a, np.array(vals, dtype=np.uint64)


def test_mixed_owners(monkeypatch):
    multi_fids = [FIDS[1], FIDS[4], FIDS[7]]
    eng = _engine(monkeypatch, _base_rules(), cluster_max_allowed_qps=BIG)
    orc = _oracle(_base_rules(), cluster_max_allowed_qps=BIG)
    rng = np.random.default_rng(71)
    lane = 0
    for k in range(3):
        a, v = _multi_call(rng, T0 + 2500 * k, N_CALL, multi_fids)
        w = _oracle_call(orc, a, v)
        _both_ways(w, "mixed call %d" % k)
        m = a["n_values"] > 1
        assert {OK, BL} <= set(w["status"][m].tolist())
        lane += int(np.isin(a["flow_id"], multi_fids).sum())
        _equal(_device_call(eng, a, v), w, a, "call %d" % k)
        assert _stats(eng) == ((k + 1) * N_CALL - lane, lane, 3 * (k + 1))
    assert lane > 0 and lane < 3 * N_CALL


# ---- 8. the clock goes back between calls
def test_clock_gone_back_between_calls(monkeypatch):
    eng = _engine(monkeypatch, _base_rules(), cluster_max_allowed_qps=BIG)
    orc = _oracle(_base_rules(), cluster_max_allowed_qps=BIG)
    rng = np.random.default_rng(81)
    a1, v1 = _call(rng, T0)
    a2, v2 = _call(rng, int(a1["ts"][-1]) - 700)
    a3, v3 = _call(rng, int(a2["ts"][-1]) + 40)
    # the flows the second call finds with a stamp after their first request: the window start of their latest
    # request of the first call lies later
    back_fids = []
    for i, fid in enumerate(FIDS):
        wlen = SHAPES[i % 5][1] // SHAPES[i % 5][0]
        last = int(a1["ts"][a1["flow_id"] == fid].max())
        if last - last % wlen > int(a2["ts"][a2["flow_id"] == fid].min()):
            back_fids.append(fid)
    back, n_back = len(back_fids), int(np.isin(a2["flow_id"], back_fids).sum())
    assert back >= 5
    for k, (a, v) in enumerate([(a1, v1), (a2, v2), (a3, v3)]):
        w = _oracle_call(orc, a, v)
        _both_ways(w, "clock call %d" % k)
        _equal(_device_call(eng, a, v), w, a, "call %d" % k)
        if k == 0:
            assert _stats(eng) == (N_CALL, 0, 0)
        if k == 1:
            assert _stats(eng) == (2 * N_CALL - n_back, n_back, back)
    assert _stats(eng) == (3 * N_CALL - n_back, n_back, back)  # later in time: every flow is back


# ---- 9. the switch
def test_switch_off_keeps_every_flow_on_the_lane_owner(base, monkeypatch):
    calls, want = base
    eng = _engine(monkeypatch, _base_rules(), env={"SG_PTOK_VP": 0}, cluster_max_allowed_qps=BIG)
    for k, ((a, v), w) in enumerate(zip(calls, want)):
        _equal(_device_call(eng, a, v), w, a, "call %d" % k)
    assert _stats(eng) == (0, 3 * N_CALL, 0)


# ---- 10. small tables
def test_small_table_rehashes_and_grows(base, monkeypatch):
    """The base stream through a table of 64 slots that grows to 4,096.  The capacity policy (pvtab.h) refuses a call
    that lists more values than half of the maximum capacity less the live ones, and a base call lists 4,099: so
    the stream goes in pieces of 512 requests, in the same order (the clock never goes back, so the oracle's answers
    to the whole calls are the answers to the pieces)."""
    calls, want = base
    eng = _engine(monkeypatch, _base_rules(), env={"SG_PV_LOG2": 6, "SG_PV_MAX_LOG2": 12},
                  cluster_max_allowed_qps=BIG)
    assert eng.cluster_param_table_stats()["capacity"] == 64
    for k, ((a, v), w) in enumerate(zip(calls, want)):
        for lo in range(0, len(a), 512):
            pa = a[lo: lo + 512].copy()
            pa["value_off"] -= lo
            _equal(_device_call(eng, pa, v[lo: lo + 512]), w[lo: lo + 512], pa, "call %d from %d" % (k, lo))
    st = eng.cluster_param_table_stats()
    assert st["rehashes"] >= 3 and st["resizes"] >= 1 and st["capacity"] <= 4096
    assert _stats(eng) == (3 * N_CALL, 0, 0)


def test_refused_call_from_device_buffers_changes_nothing(monkeypatch):
    """64 slots that cannot grow (little calls by design: exempt from the 20 % rule, OK and BLOCKED both occur)."""
    rules = [_prule(41, 4), _prule(42, 4, shape=(2, 1000))]
    eng = _engine(monkeypatch, rules, env={"SG_PV_LOG2": 6, "SG_PV_MAX_LOG2": 6}, cluster_max_allowed_qps=50)
    orc = _oracle(rules, cluster_max_allowed_qps=50)

    def call(reqs):
        return A.param_token_arrays(reqs)

    vals = list(range(70, 80))
    a, v = call([(T0 + i, 41 + i % 2, 1, [vals[i % 10]]) for i in range(30)])
    _equal(_device_call(eng, a, v), _oracle_call(orc, a, v), a, "before")
    table, owners = eng.cluster_param_table_stats(), eng.cluster_param_owner_stats()
    assert (table["capacity"], table["claimed_ub"]) == (64, 30) and owners["value_parallel_requests"] == 30
    a, v = call([(T0 + 40 + i, 41, 1, [100 + i]) for i in range(40)])  # 10 live + 40 listed > half of 64
    with pytest.raises(E.SentinelError) as ei:
        _device_call(eng, a, v)
    assert ei.value.code == A.SG_ENOMEM
    assert eng.cluster_param_table_stats() == table and eng.cluster_param_owner_stats() == owners
    a, v = call([(T0 + 100 + i, 41 + i % 2, 1, [vals[i % 10]]) for i in range(22)])
    w = _oracle_call(orc, a, v)
    assert set(w["status"].tolist()) >= {OK, BL, A.TOKEN_TOO_MANY_REQUEST}
    _equal(_device_call(eng, a, v), w, a, "after")
    for sec in range(1, 4):
        a, v = call([(T0 + sec * 1000 + 7 * i, 41 + sec % 2, 1, [vals[i % 4]]) for i in range(20)])
        w = _oracle_call(orc, a, v)
        assert {OK, BL} <= set(w["status"].tolist())
        _equal(_device_call(eng, a, v), w, a, sec)


# ---- 11. errors from device buffers
def test_errors_from_device_buffers_change_nothing(base, monkeypatch):
    calls, want = base
    eng = _engine(monkeypatch, _base_rules(), cluster_max_allowed_qps=BIG)
    (a0, v0), (a1, v1) = calls[0], calls[1]
    _equal(_device_call(eng, a0, v0), want[0], a0, "call 0")
    table, owners = eng.cluster_param_table_stats(), eng.cluster_param_owner_stats()
    bad = a1.copy()
    bad["value_off"][len(bad) // 2] = len(v1)  # one past the last value
    with pytest.raises(E.SentinelError) as ei:
        _device_call(eng, bad, v1)
    assert ei.value.code == A.SG_EINVAL
    bad = a1.copy()
    bad["ts"][len(bad) // 2] = bad["ts"][len(bad) // 2 - 1] - 1  # unordered
    with pytest.raises(E.SentinelError) as ei:
        _device_call(eng, bad, v1)
    assert ei.value.code == A.SG_EINVAL
    assert eng.cluster_param_table_stats() == table and eng.cluster_param_owner_stats() == owners
    _equal(_device_call(eng, a1, v1), want[1], a1, "call 1")  # the oracle never saw the bad calls
    _equal(_device_call(eng, calls[2][0], calls[2][1]), want[2], calls[2][0], "call 2")
