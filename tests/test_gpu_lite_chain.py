"""k_lite's memory chain: minute buckets stored without a load where they are provably stale, the exception sum's
early exit, and a chunk's decision words held in registers.

Every case is a short script of rule loads, batches and metric snapshots, run through the engine and through the
oracle; after every batch all 32 bits of every decision word and the thread count, second window and minute window
of every resource are compared exactly, after every snapshot its rows.  The engines run with SG_LITE_CHECK=1: k_lite
then reads the window start of every minute bucket it stores without a load and the batch fails (BF_LITE_STALE) if one
was not stale, so a passing case also says that the stale rule held on every bucket it met.  SG_TINY=0
sends these small synchronous batches through the batched pipeline, whose lane bins k_lite serves.

What decides whether a bucket's load may be skipped is the second the resource last wrote (the second window, read at
node_load) and the highest second a snapshot touched; the cases walk the boundary on both: the same second, the next
one, the same slot a minute or two later, a snapshot in / before / after the next event's second and a minute ahead
of it on its slot (the additions are then lost, as LeapArray loses them), the clock gone back, and the resource
written by another owner (k_jac<1>, k_jac<4>, k_lane, k_lite<true>) in between.

The CPU test at the end keeps the device tests from being vacuous: the oracle's own verdicts in these cases contain
passes, flow blocks, degrade blocks and effective TRACEs.
"""
import functools

import numpy as np
import pytest

import pyoracle as O
from sentinel_amd import _abi as A
from sentinel_amd import engine as E

gpu = pytest.mark.gpu

T0 = 1_700_000_000_000  # a multiple of 60 s
N_RES = 24
NAMES = ["lite-%d" % i for i in range(N_RES)]
BASE_ENV = {"SG_TINY": "0", "SG_LITE_CHECK": "1"}
# a segment of up to 16 events on k_lite, up to 40 on k_jac<1>, up to 400 on k_jac<4> (as the existing suites pin them)
OWNER_ENV = {"SG_LANE_MAX": "16", "SG_J1_MAX": "40", "SG_J4_MAX": "400"}


# ---------------------------------------------------------------- traces
class Plan:
    """Builds batches event by event; an EXIT / TRACE names its ENTRY by the key entry() returned (any batch)."""

    def __init__(self):
        self.base = 0
        self.gidx = {}
        self.open = {}
        self.cur = []
        self.nkey = 0

    def entry(self, ts, res, count=1, flags=0, arg=0):
        key = self.nkey
        self.nkey += 1
        self.cur.append((ts, res, A.EV_ENTRY, count, flags, key, arg))
        self.open.setdefault(res, []).append(key)
        return key

    def exit(self, ts, res, key=None, rt=5, count=1):
        self.cur.append((ts, res, A.EV_EXIT, count, 0, key, rt))

    def trace(self, ts, res, key=None, count=1):
        self.cur.append((ts, res, A.EV_TRACE, count, 0, key, 0))

    def cut(self):
        rows = sorted(self.cur, key=lambda r: r[0])  # stable: ties keep submission order
        self.cur = []
        ev = np.zeros(len(rows), dtype=A.EVENT_DTYPE)
        for i, (ts, res, kind, count, flags, key, x) in enumerate(rows):
            if kind == A.EV_ENTRY:
                self.gidx[key] = self.base + i
        for i, (ts, res, kind, count, flags, key, x) in enumerate(rows):
            ev[i] = (ts, res, count, kind, flags, 0)
            if kind == A.EV_ENTRY:
                ev["aux"][i] = x
            else:
                ref = A.REF_NONE if key is None else self.gidx[key]
                assert ref == A.REF_NONE or ref < self.base + i
                ev["aux"][i] = A.aux_exit(ref, x) if kind == A.EV_EXIT else ref
        self.base += len(rows)
        return ev

    def burst(self, rng, res, ts0, n, step=37, flags=0, arg=None):
        """n events of res from ts0 on, ENTRY / EXIT / TRACE mixed; EXITs name an open ENTRY of this or an earlier
        batch, or none."""
        for i in range(n):
            ts = ts0 + i * step
            q = rng.random()
            opened = self.open.get(res, [])
            if i == 0 or q < 0.5 or not opened:
                a = 0 if arg is None else arg[int(rng.integers(len(arg)))]
                self.entry(ts, res, count=int(rng.choice([1, 1, 2, 3])), flags=flags | (A.F_HAS_ARG if arg else 0), arg=a)
            elif q < 0.75:
                self.exit(ts, res, opened.pop(int(rng.integers(len(opened)))), rt=int(rng.integers(1, 80)),
                          count=int(rng.choice([1, 2])))
            elif q < 0.82:
                self.exit(ts, res, None, rt=int(rng.integers(1, 80)))
            else:
                self.trace(ts, res, opened[int(rng.integers(len(opened)))], count=int(rng.choice([1, 2])))


def std_rules(which=range(N_RES)):
    """Rule shapes k_lite takes, by resource index mod 6 (4: no rule at all)."""
    flow, deg = [], []
    for i in which:
        n, k = NAMES[i], i % 6
        if k == 0:
            flow.append(A.flow_rule(n, 3))
        elif k == 1:
            flow.append(A.flow_rule(n, 2, grade=A.FLOW_GRADE_THREAD))
            deg.append(A.degrade_rule(n, 20, 1, grade=A.DEGRADE_GRADE_RT))
        elif k == 2:
            flow.append(A.flow_rule(n, 5))
            deg.append(A.degrade_rule(n, 0.3, 2, grade=A.DEGRADE_GRADE_EXCEPTION_RATIO))
        elif k == 3:
            flow.append(A.flow_rule(n, 4))
            deg.append(A.degrade_rule(n, 2, 1, grade=A.DEGRADE_GRADE_EXCEPTION_COUNT))
        elif k == 5:
            flow += [A.flow_rule(n, 6), A.flow_rule(n, 3, grade=A.FLOW_GRADE_THREAD)]
            deg += [A.degrade_rule(n, 30, 1, grade=A.DEGRADE_GRADE_RT),
                    A.degrade_rule(n, 3, 1, grade=A.DEGRADE_GRADE_EXCEPTION_COUNT)]
    return [("flow", flow), ("degrade", deg)]


# ---------------------------------------------------------------- cases: name -> (env, steps)
GAPS = (300, 1000, 60_000, 120_000, 61_000, 200_000)  # same second, the next, the same slot twice, 61 s, > 60 s


def case_continuity():
    # resource i: its last event of batch k in second S, its first of batch k + 1 GAPS[i % 6] later
    p, rng, steps = Plan(), np.random.default_rng(1), std_rules()
    at = {r: T0 + 5_000 for r in range(N_RES)}
    for b in range(4):
        for r in range(N_RES):
            n = int(rng.integers(1, 9))
            p.burst(rng, r, at[r], n, step=40)  # (stays inside one second: 8 * 40 ms)
            at[r] += GAPS[(r + b) % 6] if (r + b) % 6 else 320
        steps.append(("batch", p.cut()))
    return {}, steps


def case_snapshots():
    # a snapshot between two batches: now in the next event's second, one before, one after, a minute ahead on its slot
    p, rng, steps = Plan(), np.random.default_rng(2), std_rules()
    for r in range(N_RES):
        p.burst(rng, r, T0 + 2_000 + 13 * r, 6, step=150)
    steps.append(("batch", p.cut()))
    nxt = T0 + 10_000
    for k, now in enumerate((nxt + 400, nxt - 600, nxt + 1_400, nxt + 60_300)):
        steps.append(("snap", now + 4_000 * k))
        for r in range(N_RES):
            p.burst(rng, r, nxt + 4_000 * k + 7 * r, 5, step=190)
        steps.append(("batch", p.cut()))
        steps.append(("snap", nxt + 4_000 * k + 2_500))
    return {}, steps


def case_owners():
    # batch k on k_jac<1> (17 .. 40 events) or k_jac<4> (41 .. 400), batch k + 1 on k_lite (<= 16), and back; resource 7
    # takes a prioritized ENTRY in the first batch (PM_PRIO is sticky: k_lane from then on) beside lite ones
    p, rng, steps = Plan(), np.random.default_rng(3), std_rules()
    t = T0 + 3_000
    for b, sizes in enumerate(((30, 6), (5, 70), (90, 9), (8, 28), (12, 3))):
        for r in range(N_RES):
            n = sizes[r % 2]
            fl = A.F_PRIORITIZED if (r == 7 and b == 0) else 0
            p.burst(rng, r, t + 3 * r, n, step=max(1, 1_900 // n), flags=fl)
        steps.append(("batch", p.cut()))
        t += (2_500, 3_000, 60_000, 2_200)[b % 4]
    return OWNER_ENV, steps


def case_clock_back():
    # the second batch starts earlier than the first ended: by 3 s (other slots) on even resources, by 60 s (the same
    # slots: detached buckets, the additions are lost) on odd ones.  No exception-count breaker here: with the clock
    # gone back its running sum is not the oracle's window sum.
    p, rng = Plan(), np.random.default_rng(4)
    res = [r for r in range(N_RES) if r % 6 in (0, 1, 2, 4)]
    steps = std_rules(res)
    for r in res:
        p.burst(rng, r, T0 + 70_000 + 11 * r, 6, step=400)
    steps.append(("batch", p.cut()))
    for r in res:
        p.burst(rng, r, T0 + 70_000 + 11 * r - (3_000 if r % 2 == 0 else 60_000), 6, step=400)
    steps.append(("batch_backward", p.cut()))
    return {}, steps


def case_exc_count():
    n = NAMES
    deg = [A.degrade_rule(n[r], 2, 2, grade=A.DEGRADE_GRADE_EXCEPTION_COUNT) for r in range(8)]
    p, steps = Plan(), [("flow", [A.flow_rule(n[0], 50)]), ("degrade", deg)]
    A0 = T0 + 4_000
    # 0: a window sum of zero (entries over many seconds, no TRACE)
    for s in (0, 1, 7, 30, 65, 66, 120):
        p.exit(A0 + 1_000 * s + 50, 0, p.entry(A0 + 1_000 * s, 0), rt=9)
    # 1: the sum reaches zero mid-advance: TRACEs in seconds 0 and 1, an event at 30 s, the next at 65 s
    k = p.entry(A0, 1)
    p.trace(A0 + 10, 1, k)
    k = p.entry(A0 + 1_000, 1)
    p.trace(A0 + 1_010, 1, k)
    p.entry(A0 + 30_000, 1)
    p.entry(A0 + 65_000, 1)
    p.entry(A0 + 65_500, 1)
    # 2, 3, 4: two TRACEs in second 0, an ENTRY at 30 s, the next ENTRY 59 / 60 / 61 s after the TRACEs
    for r, late in ((2, 59_000), (3, 60_000), (4, 61_000)):
        k = p.entry(A0, r)
        p.trace(A0 + 5, r, k, count=2)
        p.entry(A0 + 30_000, r)
    steps.append(("batch", p.cut()))
    for r, late in ((2, 59_000), (3, 60_000), (4, 61_000)):
        p.entry(A0 + late, r)
        p.entry(A0 + late + 300, r)
    # 5: trips at its threshold (2), blocked inside timeWindow (2 s), trips again at its end (the exceptions are still
    # in the minute window, the last time at 59 s), passes once they have left it and that cut is over
    k = p.entry(A0 + 62_000, 5)
    p.trace(A0 + 62_010, 5, k)
    p.entry(A0 + 62_020, 5)
    p.trace(A0 + 62_030, 5, k)
    for dt in (62_040, 63_000, 64_039, 64_040, 66_100, 121_999, 124_000, 125_000):
        p.entry(A0 + dt, 5)
    steps.append(("batch", p.cut()))
    # 8: traffic with TRACEs under no rule, the breaker loaded afterwards (the first full sum)
    k = p.entry(A0 + 130_000, 8)
    p.trace(A0 + 130_010, 8, k, count=3)
    p.entry(A0 + 131_000, 8)
    steps.append(("batch", p.cut()))
    steps.append(("degrade", deg + [A.degrade_rule(n[8], 2, 1, grade=A.DEGRADE_GRADE_EXCEPTION_COUNT)]))
    for dt in (131_500, 132_000, 133_600, 191_000):
        p.entry(A0 + dt, 8)
        p.entry(A0 + dt, 0)
    steps.append(("batch", p.cut()))
    return {}, steps


def case_reloads():
    # the rules of a resource change between batches; the same traffic shape goes on
    n = NAMES
    p, rng, steps = Plan(), np.random.default_rng(6), []
    keys = [E.param_key("v%d" % i) for i in range(3)]
    t = [T0 + 8_000]

    def batch():
        for r in range(6):
            p.burst(rng, r, t[0] + 5 * r, 9, step=130, arg=keys if r == 4 else None)
        steps.append(("batch", p.cut()))
        t[0] += 1_400

    f = {r: [A.flow_rule(n[r], 3)] for r in range(6)}
    d = {r: [A.degrade_rule(n[r], 20, 1, grade=A.DEGRADE_GRADE_RT)] for r in range(6)}

    def load(param=None):
        steps.append(("flow", sum(f.values(), [])))
        steps.append(("degrade", sum(d.values(), [])))
        if param is not None:
            steps.append(("param", param))

    load()
    batch()
    f[0] = [A.flow_rule(n[0], 1)]                                                            # flow count changed
    d[1] = [A.degrade_rule(n[1], 0.2, 1, grade=A.DEGRADE_GRADE_EXCEPTION_RATIO)]             # RT -> ratio
    f[2], d[2] = [], []                                                                      # rules removed
    f[3] = [A.flow_rule(n[3], 4), A.flow_rule(n[3], 2, grade=A.FLOW_GRADE_THREAD)]           # a second flow ...
    d[3] = d[3] + [A.degrade_rule(n[3], 2, 1, grade=A.DEGRADE_GRADE_EXCEPTION_COUNT)]        # ... and breaker
    load(param=[A.param_rule(n[4], 0, 2)])                                                   # k_lite<true>
    batch()
    batch()
    d[1] = [A.degrade_rule(n[1], 1, 1, grade=A.DEGRADE_GRADE_EXCEPTION_COUNT)]               # ratio -> count
    f[5] = [A.flow_rule(n[5], 20, control_behavior=A.CONTROL_BEHAVIOR_WARM_UP)]              # leaves k_lite
    load(param=[A.param_rule(n[4], 0, 2), A.param_rule(n[4], 0, 5, duration_in_sec=2)])      # away from lite
    batch()
    batch()
    d[1] = [A.degrade_rule(n[1], 20, 1, grade=A.DEGRADE_GRADE_RT)]                           # count -> RT
    f[5] = [A.flow_rule(n[5], 3)]                                                            # back on k_lite
    load(param=[])
    batch()
    t[0] += 60_000
    batch()
    return {}, steps


SEG_LENS = (1, 2, 3, 4, 5, 7, 8, 9, 255, 256)


def case_seg_lengths():
    # chunk edges of the held decision words (LITE_CH = 4) and the lane bins' longest segment; EXITs naming an ENTRY
    # of the batch, of the previous batch, and none
    p, rng, steps = Plan(), np.random.default_rng(7), std_rules()
    for b in range(3):
        for r, ln in enumerate(SEG_LENS):
            p.burst(rng, (r + 3 * b) % len(SEG_LENS), T0 + 9_000 + 1_300 * b + r, ln, step=max(1, 1_200 // ln))
        steps.append(("batch", p.cut()))
    return {"SG_LANE_MAX": "256", "SG_J1_MAX": "4096", "SG_J4_MAX": "65536"}, steps


def case_long_lane():
    # debug flag 2: every segment on one lane.  600 events of one resource; EXITs past position 256 name ENTRYs past
    # position 256 (their verdict is read back from the decision words: held ones and stored ones)
    p, rng, steps = Plan(), np.random.default_rng(8), std_rules()
    for r, ln in ((0, 600), (5, 300), (3, 9)):
        p.burst(rng, r, T0 + 9_000 + r, ln, step=max(1, 2_400 // ln))
    steps.append(("batch", p.cut()))
    for r, ln in ((0, 290), (5, 5)):
        p.burst(rng, r, T0 + 12_500 + r, ln, step=3)
    steps.append(("batch", p.cut()))
    return {"SG_DEBUG_FLAGS": "2"}, steps


CASES = {
    "continuity": case_continuity,
    "snapshots": case_snapshots,
    "owners": case_owners,
    "clock_back": case_clock_back,
    "exc_count": case_exc_count,
    "reloads": case_reloads,
    "seg_lengths": case_seg_lengths,
    "long_lane": case_long_lane,
}


# ---------------------------------------------------------------- running a case
def _sorted_rows(a):
    return a[np.lexsort((a["timestamp"], a["res_id"]))]


def _play(x, steps, expect=None):
    """The steps through an engine or an oracle; returns [(what, result)] and, given the oracle's, compares as it goes."""
    out = []
    for i, (what, arg) in enumerate(steps):
        if what == "flow":
            x.load_flow_rules(arg)
        elif what == "degrade":
            x.load_degrade_rules(arg)
        elif what == "param":
            x.load_param_rules(arg)
        elif what == "snap":
            rows = _sorted_rows(x.snapshot(arg, cap=1 << 14))
            if expect is not None:
                np.testing.assert_array_equal(rows, expect[len(out)][1], err_msg="snapshot at %d (step %d)" % (arg, i))
            out.append((what, rows))
        else:
            if what == "batch_backward" and expect is not None:  # decided, then reported
                with pytest.raises(E.SentinelError) as ei:
                    x.submit(arg)
                assert ei.value.code == A.SG_EINVAL and "non-decreasing" in str(ei.value)
                dec = None
            else:
                dec = x.submit(arg)
            nodes = [x.read_node(r) for r in range(N_RES)]
            if expect is not None:
                do, no = expect[len(out)][1]
                if dec is not None:
                    bad = np.nonzero(dec != do)[0]
                    assert not len(bad), "step %d: decision of event %d (%s): gpu=%08x oracle=%08x; %d differ" % (
                        i, bad[0], arg[bad[0]], dec[bad[0]], do[bad[0]], len(bad))
                for r in range(N_RES):
                    g, o = nodes[r], no[r]
                    assert g["has_chain"] == o["has_chain"] and g["thread"] == o["thread"], (i, r, g["thread"], o["thread"])
                    np.testing.assert_array_equal(g["second"][:2], o["second"][:2],
                                                  err_msg="second window of res %d after step %d" % (r, i))
                    np.testing.assert_array_equal(g["minute"], o["minute"],
                                                  err_msg="minute window of res %d after step %d" % (r, i))
            out.append((what, (dec, nodes)))
    return out


@functools.lru_cache(maxsize=None)
def _case(name):
    env, steps = CASES[name]()
    orc = O.Oracle(max_slot_chain_size=0)
    for k, nm in enumerate(NAMES):
        assert orc.register(nm) == k
    want = _play(orc, steps)
    orc.close()
    return env, steps, want


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_lite_chain(name, monkeypatch):
    env, steps, want = _case(name)
    for k, v in {**BASE_ENV, **env}.items():
        monkeypatch.setenv(k, v)
    eng = E.Engine(max_resources=64, max_slot_chain_size=0, status_ring_log2=16)
    assert list(eng.register_many(NAMES)) == list(range(N_RES))
    _play(eng, steps, expect=want)  # (a bucket that was not stale fails its batch: BF_LITE_STALE under SG_LITE_CHECK)
    eng.close()


# ---------------------------------------------------------------- CPU: the cases reach what they are about
def test_lite_chain_cases_shape():
    """(CPU, oracle only) the oracle's verdicts in these cases contain passes, flow blocks, degrade blocks and
    effective TRACEs; the cases with a point of their own reach it."""
    for name in sorted(CASES):
        env, steps, want = _case(name)
        st, exc, k = [], 0, 0
        for what, arg in steps:
            if what in ("batch", "batch_backward", "snap"):
                if what != "snap":
                    dec, nodes = want[k][1]
                    st.append(dec[arg["kind"] == A.EV_ENTRY] & 0xFF)
                    exc = max(exc, max(int(nd["minute"][:, 3].max()) for nd in nodes))
                k += 1
        st = np.concatenate(st)
        need = [A.PASS, A.BLOCK_FLOW] if name == "clock_back" else [A.PASS, A.BLOCK_DEGRADE] if name == "exc_count" \
            else [A.PASS, A.BLOCK_FLOW, A.BLOCK_DEGRADE]
        for s in need:
            assert int((st == s).sum()) > 0, (name, s, np.bincount(st, minlength=8))
        assert exc > 0, name  # an effective TRACE reached a minute bucket
    # the exception-count timeline is the one its comments describe
    env, steps, want = _case("exc_count")
    batches = [(arg, w[1][0]) for (what, arg), w in zip([s for s in steps if s[0] in ("batch", "snap")], want)]

    def verdicts(b, res):
        ev, dec = batches[b]
        return [int(x) & 0xFF for x in dec[(ev["res_id"] == res) & (ev["kind"] == A.EV_ENTRY)]]

    assert verdicts(0, 0) == [A.PASS] * 7                                       # a sum of zero never trips
    assert verdicts(0, 1) == [A.PASS, A.PASS, A.BLOCK_DEGRADE, A.PASS, A.PASS]  # 2 at 30 s, 0 at 65 s
    assert verdicts(1, 2)[0] == A.BLOCK_DEGRADE                                 # 59 s: still in the window
    assert verdicts(1, 3) == [A.PASS, A.PASS] and verdicts(1, 4) == [A.PASS, A.PASS]
    assert verdicts(1, 5) == [A.PASS, A.PASS, A.BLOCK_DEGRADE, A.BLOCK_DEGRADE, A.BLOCK_DEGRADE, A.BLOCK_DEGRADE,
                              A.BLOCK_DEGRADE, A.BLOCK_DEGRADE, A.PASS, A.PASS]
    assert verdicts(2, 8) == [A.PASS, A.PASS] and verdicts(3, 8)[0] == A.BLOCK_DEGRADE and verdicts(3, 8)[-1] == A.PASS
    # the snapshot a minute ahead of the next batch loses that batch's additions on its slot
    env, steps, want = _case("snapshots")
    assert sum(len(w[1]) for w in want if w[0] == "snap") > 0
    # the long segment's late EXITs name ENTRYs past position 256
    env, steps, want = _case("long_lane")
    ev = steps[2][1]
    seg = np.nonzero(ev["res_id"] == 0)[0]
    late = [i for i in seg[256:] if ev["kind"][i] == A.EV_EXIT and (int(ev["aux"][i]) & A.REF_NONE) != A.REF_NONE
            and (int(ev["aux"][i]) & A.REF_NONE) >= seg[256]]
    assert len(late) > 10
