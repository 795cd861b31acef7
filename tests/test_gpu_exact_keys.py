"""Exact parameter keys on the device: sg_param_intern, hot items through the dictionary, and the sweep
(sentinel_amd/csrc/pkeys.h, keysweep.hip).

ParamFlowChecker's maps compare values with equals() (ParameterMetric.java:88-104, ParamFlowChecker.java:121-248);
sg_param_key's word is a hash for Strings, large longs and doubles.  For doubles a collision can be built: the
hash is mix64 (a bijection) with its top four bits cut off, so inverting mix64 on mix64(bits(1.5)) ^ (h << 60)
gives another double with the key of 1.5.  The tests below use such a pair.  The oracle takes keys as opaque
words, so it judges the engine on the interned keys.

Shapes: the single-workgroup batch (k_tiny) and the batched path, a 20,000-event param-only segment (k_pq and
the value-parallel passes), an SG_ARG_LIST; for the sweep a map that grew several times (its abandoned regions
still hold old keys), a 2-bucket map, 0 / 1 / > 65,536 candidates, thread-count maps, the key ring and the token
server's value table."""
import ctypes as C
import math
import struct
from collections import OrderedDict

import numpy as np
import pytest

import pyoracle as O
from sentinel_amd import _abi as A
from sentinel_amd import engine as E

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000_000
M64 = (1 << 64) - 1
C1, C2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
DBL = "java.lang.Double"


def _mix64(x):
    x ^= x >> 30
    x = x * C1 & M64
    x ^= x >> 27
    x = x * C2 & M64
    return x ^ (x >> 31)


def _unshift(y, s):  # inverse of x -> x ^ (x >> s)
    x = y
    for _ in range(64 // s + 1):
        x = y ^ (x >> s)
    return x


def _unmix64(y):
    y = _unshift(y, 31) * pow(C2, -1, 1 << 64) & M64
    y = _unshift(y, 27) * pow(C1, -1, 1 << 64) & M64
    return _unshift(y, 30)


def _colliding_doubles():
    b1 = struct.unpack("<Q", struct.pack("<d", 1.5))[0]
    for h in range(1, 16):
        b2 = _unmix64(_mix64(b1) ^ (h << 60))
        d2 = struct.unpack("<d", struct.pack("<Q", b2))[0]
        if math.isfinite(d2) and float(repr(d2)) == d2:
            return "1.5", repr(d2)
    raise AssertionError("no finite colliding double")


D1, D2 = _colliding_doubles()
PROBE = [("abc", "java.lang.String"), (D1, DBL), (D2, DBL), ("600000000000000000000", "long"), ("7", "int")]


class Pair:
    """The engine and the oracle side by side: same resources, same events, every decision compared."""

    def __init__(self, names, rules, orc_rules=None, **cfg):
        cfg.setdefault("status_ring_log2", 20)
        self.eng = E.Engine(max_resources=64, max_slot_chain_size=0, **cfg)
        self.orc = O.Oracle(max_slot_chain_size=0)
        for nm in names:
            assert self.eng.register(nm) == self.orc.register(nm)
        assert self.eng.load_param_rules(rules) == self.orc.load_param_rules(rules if orc_rules is None else orc_rules)
        self.names = list(names)
        self.gbase = 0
        self.t = T0

    def submit(self, ev, orc_key=None, ext=None, args=None):
        """orc_key: {engine key: oracle key} for the values the oracle sees under a stand-in."""
        evo = ev
        if orc_key:
            evo = ev.copy()
            ent = (evo["kind"] == A.EV_ENTRY) & ((evo["flags"] & A.F_HAS_ARG) != 0)
            for k, v in orc_key.items():
                evo["aux"][ent & (ev["aux"] == np.uint64(k))] = v
        if ext is None:
            dg, do = self.eng.submit(ev), self.orc.submit(evo)
        else:
            dg, do = self.eng.submit_ex(ev, ext, args), self.orc.submit_ex(evo, ext, args)
        bad = np.nonzero(dg != do)[0]
        assert not len(bad), ("event", int(bad[0]), ev[bad[0]], hex(dg[bad[0]]), hex(do[bad[0]]), len(bad))
        self.gbase += len(ev)
        self.t = int(ev["ts"].max()) + 1
        return dg

    def nodes_equal(self):
        for r in range(len(self.names)):
            g, o = self.eng.read_node(r), self.orc.read_node(r)
            assert g["thread"] == o["thread"], r
            np.testing.assert_array_equal(g["second"][:2], o["second"][:2])
            np.testing.assert_array_equal(g["minute"], o["minute"])


def _entries(ts, res, keys):
    ev = np.zeros(len(keys), dtype=A.EVENT_DTYPE)
    ev["ts"], ev["res_id"], ev["count"], ev["kind"] = ts, res, 1, A.EV_ENTRY
    ev["flags"] = A.F_HAS_ARG
    ev["aux"] = np.asarray(keys, dtype=np.uint64)
    return ev


def _entry_exit(p, res, keys):
    """ENTRY then EXIT (releasing its argument) of every key, at the pair's clock."""
    ev = np.zeros(2 * len(keys), dtype=A.EVENT_DTYPE)
    for i, k in enumerate(keys):
        ev[2 * i] = (p.t, res, 1, A.EV_ENTRY, A.F_HAS_ARG, k)
        ev[2 * i + 1] = (p.t, res, 1, A.EV_EXIT, A.F_EXIT_ARGS, A.aux_exit(p.gbase + 2 * i, 1))
    return ev


def _pair_keys(eng):
    assert E.param_key(D1, DBL) == E.param_key(D2, DBL), "premise: the two doubles share sg_param_key's word"
    k1, k2 = eng.param_intern(D1, DBL), eng.param_intern(D2, DBL)
    assert k1 != k2 and k1 == E.param_key(D1, DBL) and (k2 >> 60) == 4
    return k1, k2


# ---- 1. colliding doubles are two values
@pytest.mark.parametrize("tiny", ["1", "0"])
def test_colliding_doubles_alternating_in_one_second(tiny, monkeypatch):
    monkeypatch.setenv("SG_TINY", tiny)  # 1: the single-workgroup batch (k_tiny); 0: the batched path
    p = Pair(["r"], [A.param_rule("r", 0, 1)])
    k1, k2 = _pair_keys(p.eng)
    d = p.submit(_entries(T0 + np.arange(8) * 10, 0, [k1, k2] * 4))
    # a token bucket of 1 per value and second: the first entry of each value passes
    assert list(d & 0xFF) == [A.PASS, A.PASS] + [A.BLOCK_PARAM] * 6
    p.nodes_equal()


def test_colliding_doubles_in_a_long_param_segment():
    p = Pair(["r"], [A.param_rule("r", 0, 1)])
    k1, k2 = _pair_keys(p.eng)
    keys = np.array([k1, k2] + [p.eng.param_intern("v%d" % i) for i in range(48)], dtype=np.uint64)
    rng = np.random.default_rng(3)
    n = 20_000
    ev = _entries(T0 + np.sort(rng.integers(0, 3000, n)), 0, keys[rng.integers(0, 50, n)])
    d = p.submit(ev)
    assert p.eng.pv_last()["segments"] > 0  # the value-parallel passes ran, k_pq folded the statistics
    # ~400 accesses of each value over 3 s: its bucket of one token refills a second after its last refill, so
    # each of the pair passes three times (a shared bucket would give the two of them three passes together)
    for k in (k1, k2):
        assert int(((d[ev["aux"] == k] & 0xFF) == A.PASS).sum()) == 3
    p.nodes_equal()


def test_colliding_doubles_as_elements_of_one_list():
    p = Pair(["r"], [A.param_rule("r", 0, 1)])
    k1, k2 = _pair_keys(p.eng)
    ev = np.zeros(4, dtype=A.EVENT_DTYPE)
    ev["ts"], ev["count"], ev["kind"] = T0 + np.arange(4), 1, A.EV_ENTRY
    # args[0] = the Collection [d1, d2], [d2], [d1], [d2, d1]: every element is checked on its own bucket
    ext, table = A.ext_tables(4, {0: [[k1, k2]], 1: [k2], 2: [k1], 3: [[k2, k1]]})
    d = p.submit(ev, ext=ext, args=table)
    assert list(d & 0xFF) == [A.PASS] + [A.BLOCK_PARAM] * 3
    p.nodes_equal()


# ---- 2. colliding hot items keep their own counts
def test_colliding_hot_items_keep_their_counts():
    stand_in = "2.5"  # the oracle computes item keys itself: it gets a second value that collides with nothing
    assert O.param_key(stand_in, DBL) != O.param_key(D1, DBL)
    p = Pair(["r"], [A.param_rule("r", 0, 2, items=[(D1, DBL, 1), (D2, DBL, 5)])],
             orc_rules=[A.param_rule("r", 0, 2, items=[(D1, DBL, 1), (stand_in, DBL, 5)])])
    k1, k2 = _pair_keys(p.eng)
    k3 = p.eng.param_intern("3.5", DBL)
    assert p.eng.param_keys_stats()["pinned"] == 2
    keys = [k1, k2, k3] * 8
    d = p.submit(_entries(T0 + np.arange(len(keys)) * 5, 0, keys), orc_key={k2: O.param_key(stand_in, DBL)})
    passed = lambda k: int(sum((x & 0xFF) == A.PASS for x, kk in zip(d, keys) if kk == k))
    assert (passed(k1), passed(k2), passed(k3)) == (1, 5, 2)
    p.nodes_equal()
    # the items of a rule that a load removes are unpinned
    p.eng.load_param_rules([A.param_rule("r", 0, 2)])
    assert p.eng.param_keys_stats()["pinned"] == 0


# ---- 3. the sweep is exact and bounded
def test_sweep_keeps_exactly_what_the_device_holds():
    rules = [A.param_rule("q", 0, 50, items=[("pinned-item", "java.lang.String", 7)]),
             A.param_rule("t", 0, 10, grade=A.FLOW_GRADE_THREAD),
             A.param_rule("d", 0, 50)]
    p = Pair(["q", "t", "d", "z"], rules, status_ring_log2=10, param_table_log2=16)
    eng = p.eng
    Q, TH, DD, Z = 0, 1, 2, 3
    names = ["s%d" % i for i in range(6000)]
    key_of = dict(zip(names, (int(k) for k in eng.param_intern_many(names))))
    assert all(k == E.param_key(s) for s, k in key_of.items())  # nothing collides: the pure keys
    k1, k2 = _pair_keys(eng)
    th = {s: eng.param_intern(s) for s in ("th%d" % i for i in range(5))}
    ring_only = eng.param_intern("ring-only")
    assert eng.param_keys_stats()["entries"] == 6000 + 2 + 5 + 1 + 1 and eng.param_keys_stats()["pinned"] == 1

    lru = OrderedDict()  # the rule map of q as the test's own LRU of capacity 4000 (duration 1 s)
    order = np.random.default_rng(11).permutation(6000)
    for c in range(0, 6000, 500):  # 1000 events a batch: the 1024-slot ring holds a batch
        chunk = [names[i] for i in order[c:c + 500]]
        p.submit(_entry_exit(p, Q, [key_of[s] for s in chunk]))
        for s in chunk:
            lru[s] = True
            lru.move_to_end(s)
            if len(lru) > 4000:
                lru.popitem(last=False)
    pool = eng.param_pool()
    # q's map moved from region to region as it grew (k_pm_grow) and nothing compacted the pool: the regions it
    # left still hold its first keys, which the LRU evicted since -- a linear scan of the pool would keep them
    assert pool["compactions"] == 0 and pool["device_compactions"] == 0 and pool["taken"] > 1000
    p.submit(_entries(p.t, TH, list(th.values())))  # five thread counts that are never released
    p.submit(_entry_exit(p, DD, [k2]))              # a 2-bucket map holding the alternate of the colliding pair
    for _ in range(2):                              # 2,048 ENTRYs without an argument: the key ring turns over
        ev = np.zeros(1024, dtype=A.EVENT_DTYPE)
        ev["ts"], ev["res_id"], ev["count"], ev["kind"] = p.t, Z, 1, A.EV_ENTRY
        p.submit(ev)
    p.submit(_entries(p.t, Z, [ring_only]))         # held by the key ring alone (z has no param rule)

    st = eng.param_keys_sweep()
    assert (st["sweeps"], st["candidates"], st["dropped"]) == (1, 0, 0)  # the first sweep drops nothing
    st = eng.param_keys_sweep()
    keep = set(lru) | set(th) | {"ring-only"}
    assert st["candidates"] == 6000 + 2 + 5 + 1
    assert st["held"] == len(keep) + 1 and st["dropped"] == 2000 + 1  # + d2 held; the 2000 evicted and d1 dropped
    assert st["entries"] == len(keep) + 1 + 1 and st["pinned"] == 1 and st["displaced"] == 1
    # every survivor interns to its old key, the alternate included, though the owner of its pure key is gone
    for s in lru:
        assert eng.param_intern(s) == key_of[s]
    assert [eng.param_intern(s) for s in th] == list(th.values())
    assert eng.param_intern(D2, DBL) == k2 != E.param_key(D2, DBL)
    assert eng.param_keys_stats()["entries"] == len(keep) + 2
    # a dropped value is interned anew, under its pure key
    gone = [s for s in names if s not in lru]
    assert len(gone) == 2000 and all(eng.param_intern(s) == E.param_key(s) for s in gone[:200])
    assert eng.param_intern(D1, DBL) == k1
    # survivors and returners decide as the oracle does
    back = [key_of[s] for s in gone[:200]] + [key_of[s] for s in list(lru)[:200]] + [k1, k2]
    p.submit(_entries(p.t, Q, back + back))
    p.submit(_entries(p.t, TH, list(th.values()) * 3))
    p.submit(_entries(p.t, DD, [k1, k2] * 30))
    p.nodes_equal()
    for pr in PROBE:
        assert E.param_key(*pr) == O.param_key(*pr)


def test_sweep_with_one_candidate_and_with_many():
    p = Pair(["q"], [A.param_rule("q", 0, 50)], status_ring_log2=10, param_table_log2=14)
    eng = p.eng
    eng.param_intern("only")
    assert eng.param_keys_sweep()["candidates"] == 0
    st = eng.param_keys_sweep()
    assert (st["candidates"], st["held"], st["dropped"], st["entries"]) == (1, 0, 1, 0)
    # more than 65,536 candidates: bitmap words and the table's wrap-around; 40 of them live on the device
    names = ["m%d" % i for i in range(70_000)]
    keys = eng.param_intern_many(names)
    assert len(set(int(k) for k in keys)) == 70_000
    live = list(range(0, 70_000, 1750))
    p.submit(_entry_exit(p, 0, [int(keys[i]) for i in live]))
    for _ in range(2):
        ev = np.zeros(1024, dtype=A.EVENT_DTYPE)
        ev["ts"], ev["count"], ev["kind"] = p.t, 1, A.EV_ENTRY
        p.submit(ev)
    eng.param_keys_sweep()
    st = eng.param_keys_sweep()
    assert (st["candidates"], st["held"], st["dropped"], st["entries"]) == (70_000, 40, 70_000 - 40, 40)
    assert [int(k) for k in eng.param_intern_many([names[i] for i in live])] == [int(keys[i]) for i in live]
    d = p.submit(_entries(p.t, 0, [int(keys[i]) for i in live]))
    assert ((d & 0xFF) == A.PASS).all()


# ---- 4. the token server
def test_token_server_counts_the_colliding_pair_apart():
    rules = [A.param_rule("abc", 0, 2, cluster_mode=True, cluster_flow_id=17,
                          cluster_threshold_type=A.CLUSTER_THRESHOLD_GLOBAL)]
    eng = E.Engine(max_resources=64, status_ring_log2=20)
    orc = O.Oracle()
    for x in (eng, orc):
        x.register("abc")
        x.load_param_rules(rules)
    k1, k2 = _pair_keys(eng)
    reqs = [(T0 + i, 17, 1, [k1 if i % 2 == 0 else k2]) for i in range(8)]
    got = eng.cluster_request_param(reqs)
    assert got == orc.cluster_request_param(reqs)
    assert [s for s, _, _ in got] == [A.TOKEN_OK] * 4 + [A.TOKEN_BLOCKED] * 4  # two tokens a value
    eng.param_keys_sweep()
    st = eng.param_keys_sweep()  # both values' slots are claimed: the sweep keeps both
    assert (st["candidates"], st["held"], st["dropped"], st["entries"]) == (2, 2, 0, 2)
    assert (eng.param_intern(D1, DBL), eng.param_intern(D2, DBL)) == (k1, k2)


# ---- 5. errors and the empty engine
def test_null_engine_and_an_engine_without_param_rules():
    before = [E.param_key(*pr) for pr in PROBE]
    L = E.lib()
    out = C.c_uint64()
    assert L.sg_param_intern(None, b"x", None, C.byref(out)) == A.SG_EINVAL
    vals = (C.c_char_p * 1)(b"x")
    assert L.sg_param_intern_batch(None, vals, None, 1, C.byref(out)) == A.SG_EINVAL
    assert L.sg_param_keys_sweep(None) == A.SG_EINVAL
    assert L.sg_param_keys_stats(None, C.byref(out), 1) == 0
    assert E.param_key("x") == O.param_key("x")  # sg_param_key keeps accepting a NULL engine
    eng = E.Engine(max_resources=64, status_ring_log2=20)
    assert eng.param_intern(None) == 0 and eng.param_intern("7", "int") == E.param_key("7", "int")
    keys = eng.param_intern_many(["e%d" % i for i in range(100)] + [D1, D2], ["java.lang.String"] * 100 + [DBL, DBL])
    assert len(set(int(k) for k in keys)) == 102 and eng.param_keys_stats()["entries"] == 102
    assert eng.param_keys_sweep()["dropped"] == 0
    st = eng.param_keys_sweep()  # no param rules: no maps, no key ring; everything untouched goes
    assert (st["candidates"], st["held"], st["dropped"], st["entries"]) == (102, 0, 102, 0)
    assert [E.param_key(*pr) for pr in PROBE] == before
