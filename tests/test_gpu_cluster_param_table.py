"""The token server's (flowId, value) table drops expired values and grows (sentinel_amd/csrc/pvtab.h,
cluster.hip k_pv_rehash, engine.cpp pv_make_room).

The reference's ClusterParameterLeapArray clears a bucket's value map on every window reset
(csrv/flow/statistic/metric/ClusterParameterLeapArray.java:30-58), so ClusterParamMetric.getSum
(ClusterParamMetric.java:53-85) serves any number of distinct values over time; so does the oracle's cp_val.
Every test replays a stream through the engine and the oracle and requires equal (status, remaining, wait) for
every request, across rehashes that drop dead slots, grow the table, follow a rule load or precede a sweep.
The tests with small tables set SG_PV_LOG2 / SG_PV_MAX_LOG2 before the engine is created."""
import numpy as np
import pytest

import pyoracle as O
from sentinel_amd import _abi as A
from sentinel_amd import engine as E

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000_000
OK, BL = A.TOKEN_OK, A.TOKEN_BLOCKED
GLOBAL, AVG_LOCAL = A.CLUSTER_THRESHOLD_GLOBAL, A.CLUSTER_THRESHOLD_AVG_LOCAL
SHAPES = [(10, 1000), (5, 500), (2, 1000), (1, 200)]  # (sampleCount, windowIntervalMs)


def _prule(fid, count, items=None, thr=GLOBAL, shape=(10, 1000)):
    return A.param_rule("abc", 0, count, cluster_mode=True, cluster_flow_id=fid, cluster_threshold_type=thr,
                        items=items or (), cluster_sample_count=shape[0], cluster_window_interval_ms=shape[1])


def _pair(rules, sizes=None, monkeypatch=None, **cfg):
    if sizes:
        monkeypatch.setenv("SG_PV_LOG2", str(sizes[0]))
        monkeypatch.setenv("SG_PV_MAX_LOG2", str(sizes[1]))
    eng = E.Engine(max_resources=64, **cfg)
    orc = O.Oracle(**cfg)
    for x in (eng, orc):
        x.register("abc")
        x.load_param_rules(rules)
    return eng, orc


def _same(eng, orc, reqs, what=""):
    got = eng.cluster_request_param(reqs)
    want = orc.cluster_request_param(reqs)
    bad = [i for i in range(len(reqs)) if got[i] != want[i]]
    assert not bad, (what, bad[0], reqs[bad[0]], got[bad[0]], want[bad[0]], len(bad))
    return got


def _same_arrays(eng, orc, ts, fid, vals, what=""):
    """One single-value request per element (acquire 1), through the array entry points of both sides."""
    n = len(ts)
    arr = np.zeros(n, dtype=A.PARAM_TOKEN_REQ_DTYPE)
    arr["ts"], arr["flow_id"], arr["acquire_count"], arr["n_values"] = ts, fid, 1, 1
    arr["value_off"] = np.arange(n, dtype=np.uint64)
    vals = np.ascontiguousarray(vals, dtype=np.uint64)
    got = eng.cluster_request_param_array(arr, vals)
    want = np.zeros(n, dtype=A.TOKEN_RES_DTYPE)
    assert O.lib().or_cluster_request_param_tokens(orc.h, arr.ctypes.data, n, vals.ctypes.data, n,
                                                   want.ctypes.data) == 0
    for f in ("status", "remaining", "wait_in_ms"):
        bad = np.flatnonzero(got[f] != want[f])
        assert not len(bad), (what, f, int(bad[0]), arr[bad[0]], got[bad[0]], want[bad[0]], len(bad))
    return got["status"]


def _colliding_doubles():
    """Two doubles with one sg_param_key word (test_gpu_exact_keys.py): the word is mix64, a bijection, with its
    top four bits cut off, so inverting mix64 on mix64(bits(1.5)) ^ (h << 60) gives the second double."""
    import math
    import struct

    m64, c1, c2 = (1 << 64) - 1, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB

    def mix(x):
        x ^= x >> 30
        x = x * c1 & m64
        x ^= x >> 27
        x = x * c2 & m64
        return x ^ (x >> 31)

    def unshift(y, sh):  # inverse of x -> x ^ (x >> sh)
        x = y
        for _ in range(64 // sh + 1):
            x = y ^ (x >> sh)
        return x

    def unmix(y):
        y = unshift(y, 31) * pow(c2, -1, 1 << 64) & m64
        y = unshift(y, 27) * pow(c1, -1, 1 << 64) & m64
        return unshift(y, 30)

    b1 = struct.unpack("<Q", struct.pack("<d", 1.5))[0]
    for h in range(1, 16):
        d2 = struct.unpack("<d", struct.pack("<Q", unmix(mix(b1) ^ (h << 60))))[0]
        if math.isfinite(d2) and float(repr(d2)) == d2:
            return "1.5", repr(d2)
    raise AssertionError("no finite colliding double")


# ---- 1. default sizes: more (flow, value) pairs over time than the table has slots
def test_more_pairs_than_slots_at_default_sizes():
    """145,280 pairs through the default 131,072 slots.  With a table that never releases a slot, pv_find finds it
    full in one of the last calls (flag 2) and the call returns SG_ENOMEM."""
    nf, ticks, fresh, recur = 64, 30, 75, 20
    rules = [_prule(100 + i, 5, shape=SHAPES[i % 4]) for i in range(nf)]
    eng, orc = _pair(rules, cluster_max_allowed_qps=10_000_000)
    st0 = eng.cluster_param_table_stats()
    assert (st0["capacity"], st0["claimed_ub"], st0["rehashes"], st0["max_capacity"]) == (1 << 17, 0, 0, 1 << 24)
    rng = np.random.default_rng(11)
    flows = np.arange(nf, dtype=np.int64)
    seen, statuses = 0, set()
    for tick in range(ticks):
        # per flow: `fresh` never-seen values once or twice each, `recur` recurring values 1..8 times each
        f_new = np.repeat(flows, fresh)
        v_new = (f_new.astype(np.uint64) << np.uint64(40)) | (np.uint64(tick * fresh) + np.tile(np.arange(fresh, dtype=np.uint64), nf))
        twice = rng.random(len(f_new)) < 0.5
        f_rec = np.repeat(flows, recur)
        v_rec = (f_rec.astype(np.uint64) << np.uint64(40)) | np.uint64(1 << 30) | np.tile(np.arange(recur, dtype=np.uint64), nf)
        times = rng.integers(1, 9, len(f_rec))
        f = np.concatenate([f_new, f_new[twice], np.repeat(f_rec, times)])
        v = np.concatenate([v_new, v_new[twice], np.repeat(v_rec, times)])
        ts = T0 + tick * 1000 + np.sort(rng.integers(0, 1000, len(f)))
        p = rng.permutation(len(f))
        s = _same_arrays(eng, orc, ts, 100 + f[p], v[p], "tick %d" % tick)
        statuses |= set(int(x) for x in np.unique(s))
        seen += nf * fresh + (nf * recur if tick == 0 else 0)
    assert seen == nf * (ticks * fresh + recur) and seen > (1 << 17)  # 145,280 pairs, 131,072 slots
    assert statuses >= {OK, BL}
    st = eng.cluster_param_table_stats()
    assert st["rehashes"] >= 1
    assert st["claimed_ub"] <= st["capacity"] // 2 and st["claimed_ub"] < seen // 2
    assert 0 < st["live_kept"] < 3 * nf * (fresh + recur)  # a rehash keeps about the last second's values


# ---- 2. reclaim without growth
def test_reclaim_without_growth(monkeypatch):
    shapes = {21: (10, 1000), 22: (2, 1000), 23: (1, 200)}
    eng, orc = _pair([_prule(fid, 2, shape=s) for fid, s in shapes.items()], (8, 8), monkeypatch)
    assert eng.cluster_param_table_stats()["capacity"] == 256
    pairs = set()
    statuses = set()
    nxt = 1000
    for tick in range(60):
        for call in range(3):  # the same three buckets every second: last second's values die as they are reset
            t = T0 + tick * 1000 + call * 100
            reqs = []
            for k in range(9):
                fid = 21 + (tick + call + k) % 3
                reqs.append((t + k, fid, 1, [nxt]))
                pairs.add((fid, nxt))
                nxt += 1
            reqs.append((t + 9, 21 + tick % 3, 1, [7]))  # asked in all three calls of a second: the third blocks
            pairs.add((21 + tick % 3, 7))
            statuses |= {s for s, _, _ in _same(eng, orc, reqs, (tick, call))}
    assert len(pairs) > 1500 and statuses >= {OK, BL}
    st = eng.cluster_param_table_stats()
    assert st["capacity"] == 256 and st["max_capacity"] == 256
    assert st["rehashes"] >= 5 and st["resizes"] == 0
    assert st["live_kept"] <= 30 and st["claimed_ub"] <= 128


# ---- 3. growth inside one call, and the moved counts decide
def test_growth_inside_one_call(monkeypatch):
    eng, orc = _pair([_prule(31, 3), _prule(32, 3, shape=(1, 200))], (6, 12), monkeypatch)
    assert eng.cluster_param_table_stats()["capacity"] == 64
    a = list(range(500, 540))
    got = _same(eng, orc, [(T0 + i, 31, 1, [v]) for i, v in enumerate(a + a)], "first")  # 80 listed values > 32
    assert {s for s, _, _ in got} == {OK}
    st = eng.cluster_param_table_stats()
    assert st["resizes"] == 1 and st["capacity"] == 512 and st["live_kept"] == 0
    got = _same(eng, orc, [(T0 + 300 + i, 31, 1, [v]) for i, v in enumerate(a + a)], "second")
    assert [s for s, _, _ in got] == [OK] * 40 + [BL] * 40  # two passes before, threshold 3
    # 200 values of another flow: the 40 live slots move, with their three passes each
    _same(eng, orc, [(T0 + 400 + i // 2, 32, 1, [9000 + i]) for i in range(200)], "third")
    st = eng.cluster_param_table_stats()
    assert st["resizes"] == 2 and st["live_kept"] == 40 and st["capacity"] == 1024
    got = _same(eng, orc, [(T0 + 600 + i, 31, 1, [v]) for i, v in enumerate(a)], "moved counts block")
    assert {s for s, _, _ in got} == {BL}
    got = _same(eng, orc, [(T0 + 1350 + i, 31, 1, [v]) for i, v in enumerate(a)], "a window later")
    assert {s for s, _, _ in got} == {OK}
    st = eng.cluster_param_table_stats()
    cap = st["capacity"]
    assert st["resizes"] >= 1 and cap & (cap - 1) == 0 and cap <= 4096 and st["max_capacity"] == 4096


# ---- 4. a refused call changes nothing
def test_refusal_changes_nothing(monkeypatch):
    eng, orc = _pair([_prule(41, 4), _prule(42, 4, shape=(2, 1000))], (6, 6), monkeypatch, cluster_max_allowed_qps=50)
    vals = list(range(70, 80))
    _same(eng, orc, [(T0 + i, 41 + i % 2, 1, [vals[i % 10]]) for i in range(30)], "before")  # 30 of the 50 a second
    before = eng.cluster_param_table_stats()
    assert (before["capacity"], before["claimed_ub"], before["rehashes"]) == (64, 30, 0)
    with pytest.raises(E.SentinelError) as ei:  # 10 live values + 40 listed > half of the 64 slots
        eng.cluster_request_param([(T0 + 40 + i, 41, 1, [100 + i]) for i in range(40)])
    assert ei.value.code == A.SG_ENOMEM
    assert eng.cluster_param_table_stats() == before
    # the oracle never saw the refused call: 20 more pass the limiter, then TOO_MANY_REQUEST; the windows and
    # the counts are as they were (threshold 4: values asked 3 times before)
    got = _same(eng, orc, [(T0 + 100 + i, 41 + i % 2, 1, [vals[i % 10]]) for i in range(22)], "after")
    assert [s for s, _, _ in got][20:] == [A.TOKEN_TOO_MANY_REQUEST] * 2 and {s for s, _, _ in got[:20]} >= {OK}
    st = eng.cluster_param_table_stats()
    assert st["rehashes"] == 1 and st["live_kept"] == 10 and st["capacity"] == 64
    for sec in range(1, 5):  # five asks a value, threshold 4; every call needs another rehash of the full table
        got = _same(eng, orc, [(T0 + sec * 1000 + 7 * i, 41 + sec % 2, 1, [vals[i % 4]]) for i in range(20)], sec)
        assert {s for s, _, _ in got} >= {OK, BL}
    assert eng.cluster_param_table_stats()["capacity"] == 64


# ---- 5. shapes that can go wrong across a rehash
def test_shapes_across_rehashes(monkeypatch):
    vip = O.param_key("vip", "java.lang.String")
    rules = [_prule(51, 2, items=[("vip", "java.lang.String", 5)]),  # multi-value requests, a hot item
             _prule(52, 2, thr=AVG_LOCAL, shape=(5, 500)),            # connected count changes on the way
             _prule(53, 2, shape=(1, 200)), _prule(54, 3, shape=(16, 1600)),
             _prule(55, 2, shape=(2, 1000)),                           # idle for three intervals, then back
             _prule(56, 1), _prule(57, 1),                             # the boundary values
             _prule(58, 1000, shape=(1, 200))]                         # never-seen values: forces the rehashes
    eng, orc = _pair(rules, (6, 9), monkeypatch, cluster_max_allowed_qps=1_000_000)
    for x in (eng, orc):
        x.cluster_set_connected(52, 2)
    rng = np.random.default_rng(5)
    t, nxt, statuses, multi = T0, 1 << 20, set(), set()
    idle_from, idle_to = T0 + 1500, T0 + 1500 + 3 * 1000 + 200
    marks = {}  # the boundary requests' statuses
    w0 = T0 + 2000  # a window start of flows 56 / 57 (T0 is a multiple of 1000)
    special = {w0: [("x0", 56, 901), ("y0", 57, 902)], w0 + 999: [("x1", 56, 901)], w0 + 1000: [("y1", 57, 902)]}
    conn3 = False
    while t < T0 + 6000:
        step = int(rng.integers(20, 90))
        for ts in sorted(s for s in special if t < s <= t + step):  # a call of its own at the exact time
            got = _same(eng, orc, [(ts, fid, 1, [v]) for _, fid, v in special[ts]], ("special", ts - T0))
            for (name, _, _), g in zip(special[ts], got):
                marks[name] = g[0]
        t += step
        if t >= T0 + 3000 and not conn3:
            for x in (eng, orc):
                x.cluster_set_connected(52, 3)
            conn3 = True
        last = min([s for s in special if s > t], default=t + 1000) - 1  # (a call never runs past a boundary request)
        reqs, ts = [], t
        for _ in range(int(rng.integers(25, 45))):
            ts = min(ts + int(rng.integers(0, 2)), last)
            fid = int(rng.choice([51, 51, 52, 52, 53, 54, 54, 55, 58, 58, 58, 58, 58]))
            if fid == 55 and idle_from <= ts < idle_to:
                fid = 58
            if fid == 58:
                vs = [nxt]
                nxt += 1
            elif fid == 51 and rng.random() < 0.4:
                vs = [vip if rng.random() < 0.5 else int(rng.integers(1, 5))] + [int(x) for x in rng.integers(1, 5, int(rng.integers(1, 3)))]
            elif fid == 51:
                vs = [vip if rng.random() < 0.3 else int(rng.integers(1, 5))]
            else:
                vs = [int(rng.integers(1, 6))]
            reqs.append((ts, fid, int(rng.integers(1, 3)), vs))
        got = _same(eng, orc, reqs, t - T0)
        statuses |= {s for s, _, _ in got}
        multi |= {g[0] for r, g in zip(reqs, got) if len(r[3]) > 1}
        t = ts
    assert statuses >= {OK, BL} and multi >= {OK, BL}
    # at w + interval - 1 the bucket stamped w still counts; at w + interval its reset comes first
    assert (marks["x0"], marks["x1"], marks["y0"], marks["y1"]) == (OK, BL, OK, OK)
    st = eng.cluster_param_table_stats()
    assert st["rehashes"] >= 5 and st["resizes"] >= 1 and st["capacity"] <= 512


# ---- 6. a rule load on a grown table keeps its capacity
def test_rule_load_on_a_grown_table():
    eng, orc = _pair([_prule(16, 2), _prule(17, 1), _prule(18, 3)], cluster_max_allowed_qps=10_000_000)
    n = 70_000  # more listed values than half of the 2^17 slots: the table grows before the call runs
    k = np.arange(n)
    _same_arrays(eng, orc, T0 + k // 100, 16 + k % 3, 1 + k % 50, "grow")
    st = eng.cluster_param_table_stats()
    assert st["resizes"] == 1 and st["capacity"] == 1 << 19 and st["claimed_ub"] == n
    rules2 = [_prule(16, 4), _prule(16, 3), _prule(19, 2)]  # 16 stays (last rule wins), 17 and 18 go, 19 comes
    for x in (eng, orc):
        x.load_param_rules(rules2)
    st = eng.cluster_param_table_stats()
    assert st["capacity"] == 1 << 19 and st["claimed_ub"] == 50  # the 50 live values of flow 16
    t = T0 + 720
    reqs = [(t + i, [16, 17, 19][i % 3], 1, [1 + i % 60]) for i in range(600)]
    got = _same(eng, orc, reqs, "after the load")
    assert {s for s, _, _ in got} >= {OK, BL, A.TOKEN_NO_RULE_EXISTS}
    for x in (eng, orc):
        x.load_param_rules(rules2 + [_prule(17, 1)])
    got = _same(eng, orc, [(t + 700 + i, 16 + i % 4, 1, [1 + i % 7]) for i in range(200)], "17 is back")
    assert {s for s, _, _ in got} >= {OK, BL}
    assert eng.cluster_param_table_stats()["capacity"] == 1 << 19


# ---- 7. the key sweep scans a grown table
def test_sweep_on_a_grown_table(monkeypatch):
    D1, D2, DBL = _colliding_doubles() + ("java.lang.Double",)
    monkeypatch.setenv("SG_PV_LOG2", "6")
    monkeypatch.setenv("SG_PV_MAX_LOG2", "12")
    rules = [_prule(17, 2), _prule(18, 1000)]
    eng = E.Engine(max_resources=64, status_ring_log2=20)
    orc = O.Oracle()
    for x in (eng, orc):
        x.register("abc")
        x.load_param_rules(rules)
    assert E.param_key(D1, DBL) == E.param_key(D2, DBL), "premise: the two doubles share sg_param_key's word"
    k1, k2 = eng.param_intern(D1, DBL), eng.param_intern(D2, DBL)
    assert k1 != k2
    got = _same(eng, orc, [(T0 + i, 17, 1, [k1 if i % 2 == 0 else k2]) for i in range(6)], "pair")
    assert [s for s, _, _ in got] == [OK] * 4 + [BL] * 2  # two tokens a value
    _same(eng, orc, [(T0 + 10 + i // 8, 18, 1, [5000 + i]) for i in range(300)], "grow")
    st = eng.cluster_param_table_stats()
    assert st["resizes"] >= 1 and st["capacity"] > 1024 and st["live_kept"] == 2
    eng.param_keys_sweep()
    ks = eng.param_keys_sweep()  # both values' slots moved to the grown table: the sweep finds and keeps both
    assert (ks["candidates"], ks["held"], ks["dropped"], ks["entries"]) == (2, 2, 0, 2)
    assert (eng.param_intern(D1, DBL), eng.param_intern(D2, DBL)) == (k1, k2)
    got = _same(eng, orc, [(T0 + 60 + i, 17, 1, [k1 if i % 2 == 0 else k2]) for i in range(4)], "pair again")
    assert [s for s, _, _ in got] == [BL] * 4
