"""Rule reloads on live state (helper of test_gpu_reload.py): scripts of loads and batches, played identically on an
Engine and an Oracle.

A script is a list of steps:

    ("flow" | "degrade" | "param", rules)   a load; its n_loaded return is compared
    ("intern_origin", name)
    ("batch", events)                       sg_submit; ("batch", events, {res: origin}) goes through sg_submit_ex
    ("async", [events, ...])                each part through submit_ptr(sync=False), no sync before the next step
    ("fail", kind, rules, code)             engine only: the load raises SentinelError(code); the oracle skips the step

After every batch all 32 bits of every decision and has_chain / thread / second[:2] / minute of every resource of the
script are compared; an async step is compared after the step that follows it (a load or an intern: both drain and
move no node), or after the final sync.  At the end the snapshot rows are compared.

The traffic comes from one generator (Trace): 24 resources in four size classes, which the owner environment of the
existing suites (SG_LANE_MAX=16, SG_J1_MAX=40, SG_J4_MAX=400) places on k_lite, k_jac<1>, k_jac<4> and the wider
owners / k_head.  A batch is 6,000 .. 10,000 events over 1.2 .. 2 s, ENTRY / EXIT / TRACE mixed as by
test_gpu_lite_chain.Plan.burst (acquire counts 1 .. 3; EXITs name ENTRYs of the batch, of earlier batches, and none).

Every load of a script may carry a counterfactual (Script.cf): the steps that stand in its place when the CPU test
plays the oracle a second time, and the resources whose decisions must then differ.
"""
import functools

import numpy as np
import pytest

import pyoracle as O
from sentinel_amd import _abi as A
from sentinel_amd import engine as E
from test_gpu_lite_chain import Plan

T0 = 1_700_000_000_000  # a multiple of 60 s
LOADS = ("flow", "degrade", "param")

# ---------------------------------------------------------------- resources and owner modes
LITE, J1, J4, WIDE = range(0, 8), range(8, 14), range(14, 20), range(20, 24)
CLASSES = {"lite": LITE, "j1": J1, "j4": J4, "wide": WIDE}
N_TRAFFIC = 24
# beside the 24 with traffic: never entered (24), seen only in EXIT / TRACE events (25), first entered late (26)
R_NEVER, R_EXIT_ONLY, R_LATE = 24, 25, 26
NAMES = ["rl-%d" % i for i in range(27)]
# events per batch of one resource: (lowest, highest drawn), and what its owner's bin allows
SIZES = {"lite": (10, 16), "j1": (17, 40), "j4": (60, 220), "wide": (1400, 1600)}  # (a wide resource: one event a ms)
LIMITS = {"lite": (1, 16), "j1": (17, 40), "j4": (41, 400), "wide": (401, 1 << 30)}

COOP = {"SG_LANE_MAX": "16", "SG_J1_MAX": "40", "SG_J4_MAX": "400", "SG_TINY": "0"}
MODES = {
    "default": {},
    "coop": COOP,
    "skip": {**COOP, "SG_SKIP_MIN": "16"},
    "lane": {"SG_DEBUG_FLAGS": "2"},
    "hotcold": {**COOP, "SG_RADIX_BELOW": "0"},
    "headoff": {**COOP, "SG_DEBUG_FLAGS": "16384"},
}


def cls_of(r):
    for k, v in CLASSES.items():
        if r in v:
            return k
    return None


def scaled(r, lite, j1, j4, wide):
    return {"lite": lite, "j1": j1, "j4": j4, "wide": wide}[cls_of(r)]


def qps(r, f=1.0):
    """About half of the tokens a second that resource r's ENTRYs ask for, times f."""
    return max(1.0, float(int(scaled(r, 8, 8, 35, 400) * f)))


def threads(r, f=1.0):
    return max(1.0, float(int(scaled(r, 8, 8, 30, 300) * f)))


# ---------------------------------------------------------------- traffic
def burst(p, rng, res, ts0, n, step, arg=None, once=True):
    """Plan.burst's mix of ENTRY / EXIT / TRACE (its draws made n at a time).  once: no ENTRY is named by two TRACEs
    of one batch (the second one names none instead); a batch with such an ENTRY (BF_MULTI_LINK) skips no frozen
    stretch."""
    q, pick, xa = rng.random(n).tolist(), rng.random(n).tolist(), rng.random(n).tolist()
    cnt, rt = rng.choice([1, 1, 2, 3], n).tolist(), rng.integers(1, 80, n).tolist()
    opened, traced = p.open.setdefault(res, []), set()
    for i in range(n):
        ts = ts0 + i * step
        if i == 0 or q[i] < 0.5 or not opened:
            p.entry(ts, res, count=cnt[i], flags=A.F_HAS_ARG if arg else 0, arg=arg[int(pick[i] * len(arg))] if arg else 0)
        elif q[i] < 0.75:
            # (with args, often Entry.exit(count, args): the param thread counts go down)
            key = opened.pop(int(pick[i] * len(opened)))
            p.cur.append((ts, res, A.EV_EXIT, min(cnt[i], 2), A.F_EXIT_ARGS if arg and xa[i] < 0.6 else 0, key, rt[i]))
        elif q[i] < 0.82:
            p.exit(ts, res, None, rt=rt[i])
        else:
            key = opened[int(pick[i] * len(opened))]
            if once and key in traced:
                key = None
            traced.add(key)
            p.trace(ts, res, key, count=min(cnt[i], 2))


class Trace:
    def __init__(self, seed, args=None, span=(1650, 2000), once=True):
        """args: {res: [param keys]}; those resources' ENTRYs carry one of them as args[0]."""
        self.p, self.rng, self.t, self.args, self.span = Plan(), np.random.default_rng(seed), T0 + 5_000, args or {}, span
        self.once = once
        self.late_on, self.nb = False, 0

    def skip(self, ms):
        self.t += ms

    def batch(self):
        p, rng = self.p, self.rng
        span = int(rng.integers(self.span[0], self.span[1] + 1))
        for r in range(N_TRAFFIC):
            lo, hi = SIZES[cls_of(r)]
            n = int(rng.integers(lo, hi + 1))
            if r in LITE:
                # a lite burst is dense (a second holds several EXITs), at the batch's end and at the next one's start
                # in turns: what lies between two batches finds half of the lite resources in mid-burst
                late = (r // 4 + self.nb) % 2 == 0
                burst(p, rng, r, self.t + (span - 30 - 30 * n if late else r), n, 30, self.args.get(r), self.once)
            else:
                burst(p, rng, r, self.t + r, n, max(1, (span - 30) // n), self.args.get(r), self.once)
        for k in range(4):  # a resource that is never entered, yet named by events
            p.exit(self.t + 100 + 300 * k, R_EXIT_ONLY, None, rt=7)
            p.trace(self.t + 150 + 300 * k, R_EXIT_ONLY, None)
        if self.late_on:
            burst(p, rng, R_LATE, self.t + 40, 9, span // 10, None, self.once)
        ev = p.cut()
        self.t += span
        self.nb += 1
        return ev


class Script:
    def __init__(self, name, seed, args=None, cfg=None, skip_modes=None, once=True):
        self.name, self.steps, self.cf, self.same, self.cfg = name, [], {}, set(), cfg or {}
        self.skip_modes = skip_modes or {}  # mode -> why the mode cannot reach the script's point
        self.tr = Trace(seed, args, once=once)
        self.once = once
        self.has_param = self.has_rl = False

    def load(self, kind, rules, cf=None, about=None):
        """cf: the steps in this load's place in the counterfactual play ([]: the load omitted); about: the resources
        whose decisions must differ then (at least one of every size class among them)."""
        if cf == "same":  # the list this kind loaded last: a no-op beside another kind's change
            self.same.add(len(self.steps))
        elif cf is not None:
            self.cf[len(self.steps)] = (cf, list(about))
        self.steps.append((kind, rules))

    def batch(self, origins=None):
        ev = self.tr.batch()
        self.steps.append(("batch", ev) if origins is None else ("batch", ev, origins))

    def run_async(self, k):
        self.steps.append(("async", [self.tr.batch() for _ in range(k)]))

    def add(self, *step):
        self.steps.append(step)


# ---------------------------------------------------------------- playing a script
def sorted_rows(a):
    return a[np.lexsort((a["timestamp"], a["res_id"]))]


def _load(x, kind, rules):
    return {"flow": x.load_flow_rules, "degrade": x.load_degrade_rules, "param": x.load_param_rules}[kind](rules)


def _submit(x, st):
    if len(st) == 2:
        return x.submit(st[1])
    ev = st[1]
    ext = np.zeros(len(ev), dtype=A.EXT_DTYPE)
    for r, name in st[2].items():
        ext["origin_id"][ev["res_id"] == r] = x.intern_origin(name)
    return x.submit_ex(ev, ext)


def _nodes(x, n_res):
    return [x.read_node(r) for r in range(n_res)]


def _compare(i, ev, dec, nodes, want):
    do, no = want
    bad = np.nonzero(dec != do)[0]
    assert not len(bad), "step %d: decision of event %d (%s): gpu=%08x oracle=%08x; %d differ, on resources %s" % (
        i, bad[0], ev[bad[0]], dec[bad[0]], do[bad[0]], len(bad), np.unique(ev["res_id"][bad])[:12])
    for r, (g, o) in enumerate(zip(nodes, no)):
        assert g["has_chain"] == o["has_chain"] and g["thread"] == o["thread"], (i, r, g["thread"], o["thread"])
        np.testing.assert_array_equal(g["second"][:2], o["second"][:2], err_msg="second window of res %d after step %d" % (r, i))
        np.testing.assert_array_equal(g["minute"], o["minute"], err_msg="minute window of res %d after step %d" % (r, i))


def t_end(steps):
    return max(int(p["ts"][-1]) for st in steps if st[0] in ("batch", "async")
               for p in (st[1] if st[0] == "async" else [st[1]]))


def play(x, steps, expect=None, n_res=len(NAMES)):
    """The steps through an oracle (expect None: returns one result per step) or through an engine, compared with the
    oracle's results as it goes."""
    out, pend = [], None
    for i, st in enumerate(steps):
        what, res = st[0], None
        if what in LOADS:
            res = _load(x, what, st[1])
            assert expect is None or res == expect[i], "step %d: n_loaded %d, the oracle's %d" % (i, res, expect[i])
        elif what == "intern_origin":
            x.intern_origin(st[1])
        elif what == "fail":
            if expect is not None:
                with pytest.raises(E.SentinelError) as ei:
                    _load(x, st[1], st[2])
                assert ei.value.code == st[3], (i, ei.value.code, str(ei.value))
        elif what == "batch":
            assert pend is None, "an async step is followed by a step that drains and moves no node"
            dec = _submit(x, st)
            res = (dec, _nodes(x, n_res))
            if expect is not None:
                _compare(i, st[1], dec, res[1], expect[i])
        elif what == "async":
            assert pend is None
            if expect is None:
                res = (np.concatenate([x.submit(p) for p in st[1]]), _nodes(x, n_res))
            else:
                outs = [np.zeros(len(p), dtype=np.uint32) for p in st[1]]
                for p, o in zip(st[1], outs):
                    x.submit_ptr(p.ctypes.data, len(p), o.ctypes.data, sync=False)
                pend = (i, outs)
                out.append(None)
                continue
        else:
            raise ValueError(what)
        if pend is not None:  # the step above drained
            j, outs = pend
            _compare(j, np.concatenate(steps[j][1]), np.concatenate(outs), _nodes(x, n_res), expect[j])
            pend = None
        out.append(res)
    if pend is not None:
        x.sync()
        j, outs = pend
        _compare(j, np.concatenate(steps[j][1]), np.concatenate(outs), _nodes(x, n_res), expect[j])
    rows = sorted_rows(x.snapshot(t_end(steps) + 1_500, cap=1 << 16))
    if expect is not None:
        np.testing.assert_array_equal(rows, expect[len(steps)], err_msg="final snapshot")
    out.append(rows)
    return out


def new_oracle():
    orc = O.Oracle(max_slot_chain_size=0)
    for k, nm in enumerate(NAMES):  # every name up front: a refused load interns nothing that the oracle lacks
        assert orc.register(nm) == k
    return orc


def oracle_play(steps):
    orc = new_oracle()
    want = play(orc, steps)
    orc.close()
    return want


def engine_play(sc, want, **cfg):
    """Plays the script on a fresh engine against the oracle's results; returns the frozen span slots its owners
    recorded (spans_total)."""
    eng = E.Engine(**{"max_resources": 64, "max_slot_chain_size": 0, "status_ring_log2": 18, **sc.cfg, **cfg})
    try:
        assert list(eng.register_many(NAMES)) == list(range(len(NAMES)))
        play(eng, sc.steps, expect=want)
        return eng.spans_total()
    finally:
        eng.close()


# ---------------------------------------------------------------- the scripts
def _rt(r, window=2, rt=10):
    return A.degrade_rule(NAMES[r], rt, window, grade=A.DEGRADE_GRADE_RT)  # (the EXITs' rt: 1 .. 79 ms)


def _ratio(r, window=2, ratio=0.1):
    return A.degrade_rule(NAMES[r], ratio, window, grade=A.DEGRADE_GRADE_EXCEPTION_RATIO)


def _count(r, window=2, f=1.0):
    # a fraction of the exceptions one batch brings: the minute window holds more from the second batch on, and a
    # window that has rolled out (70 s) reaches it again inside one batch
    return A.degrade_rule(NAMES[r], max(1, int(scaled(r, 1, 2, 8, 60) * f)), window, grade=A.DEGRADE_GRADE_EXCEPTION_COUNT)


def _warm(r, count, period=2):
    return A.flow_rule(NAMES[r], count, control_behavior=A.CONTROL_BEHAVIOR_WARM_UP, warm_up_period_sec=period)


def _wrl(r, count, period=2, queue=400):
    return A.flow_rule(NAMES[r], count, control_behavior=A.CONTROL_BEHAVIOR_WARM_UP_RATE_LIMITER,
                       warm_up_period_sec=period, max_queueing_time_ms=queue)


def _rl(r, count, queue=300):
    return A.flow_rule(NAMES[r], count, control_behavior=A.CONTROL_BEHAVIOR_RATE_LIMITER, max_queueing_time_ms=queue)


ALL = range(N_TRAFFIC)


def script_flow_state():
    """DefaultController counts change under a saturated bucket; WarmUp / WarmUpRateLimiter go cold on a changed field
    and on a permuted list, and stay warm on an equal list."""
    s = Script("flow_state", 11)
    s.has_rl = True

    def flows(f=1.0, period=2, queue=400):
        return [A.flow_rule(NAMES[r], qps(r, f)) if r % 3 == 0 else _warm(r, qps(r, 2), period) if r % 3 == 1
                else _wrl(r, qps(r, 2), period, queue) for r in ALL]

    warm = [r for r in ALL if r % 3]
    s.load("flow", flows())
    s.load("degrade", [_rt(r) for r in ALL if r % 4 == 0])
    s.batch()
    s.batch()
    s.load("flow", flows(0.5, 3, 300), cf=[], about=ALL)  # inside the 500 ms bucket the batch before filled
    s.batch()
    s.batch()
    same = flows(0.5, 3, 300)
    s.load("flow", same, cf=[("flow", same[::-1])], about=warm)  # an equal list: a no-op, warm
    s.batch()
    s.load("flow", same[::-1], cf=[], about=warm)  # the same rules, another List: cold
    s.batch()
    s.batch()
    return s


def script_carry():
    """Loads of one kind keep the controller / breaker state of the other kinds, though every rule_off shifts; so
    does the recompile at the first sg_intern_origin of a rule's limit_app."""
    keys = [E.param_key("c%d" % i) for i in range(6)]
    par = [r for r in ALL if r % 6 == 3]
    s = Script("carry", 12, args={r: keys for r in par + [0]}, once=False)  # (TRACEs name an ENTRY twice here)
    s.has_param = s.has_rl = True
    late = (6, 12, 18, 21)  # (one of every class) also hold a rule of an origin that is interned mid-script
    flow = [A.flow_rule(NAMES[r], qps(r)) if r % 3 == 0 else _warm(r, qps(r, 3)) if r % 3 == 1 else _rl(r, qps(r))
            for r in ALL] + [A.flow_rule(NAMES[r], 1, limit_app="late-app") for r in late]
    # (breakers that trip now and then: the flow controllers below them go on deciding)
    deg = [_rt(r, 3, 45) if r % 2 == 0 else _ratio(r, 3, 0.4) if r % 4 == 1 else _count(r, 3, 4) for r in ALL if r >= 4]
    prm = [A.param_rule(NAMES[r], 0, scaled(r, 1, 1, 4, 40), duration_in_sec=2) for r in par]
    stateful = [r for r in ALL if r % 3]
    s.load("flow", flow)
    s.load("degrade", deg)
    s.load("param", prm)
    s.batch()
    s.batch()
    deg2 = [_rt(r, 3, 45) for r in range(4)] + deg  # lower-numbered resources only: every later rule_off moves
    s.load("degrade", deg2, cf=[("degrade", deg2), ("flow", flow[::-1])], about=stateful)
    s.batch()
    prm2 = [A.param_rule(NAMES[0], 0, 1, duration_in_sec=2)] + prm
    s.load("param", prm2, cf=[("param", prm2), ("flow", flow[::-1]), ("degrade", deg2[::-1])], about=ALL)
    s.batch()
    s.steps.append(("intern_origin", "late-app"))
    s.cf[len(s.steps) - 1] = ([("intern_origin", "late-app"), ("flow", flow[::-1]), ("degrade", deg2[::-1])], list(ALL))
    s.batch()
    s.batch()
    return s


def script_breakers():
    """A degrade reload during a cut re-opens RT, ratio and count breakers; a flow reload leaves them cut;
    EXCEPTION_COUNT comes to a resource whose minute window holds exceptions, leaves while TRACEs go on, and comes back
    20 s and 70 s later -- on lite, J1, J4 and wide resources."""
    s = Script("breakers", 13)

    def flows(f):
        return [A.flow_rule(NAMES[r], qps(r, f)) for r in ALL]

    def degs(window, late, keep=True):
        return [_rt(r, window) if r % 4 == 0 else _ratio(r, window) if r % 4 == 1 else _count(r, window)
                for r in ALL if r % 4 < 2 or (r % 4 == 2 and keep) or (r % 4 == 3 and late)]

    cut = [r for r in ALL if r % 4 < 3]
    exc = [r for r in ALL if r % 4 >= 2]
    s.load("flow", flows(1.6))
    s.load("degrade", degs(2, False))
    s.batch()
    s.load("degrade", degs(3, False), cf=[], about=cut)
    s.batch()
    s.load("flow", flows(1.3), cf=[("flow", flows(1.3)), ("degrade", degs(3, False)[::-1])], about=cut)
    s.batch()
    s.load("degrade", degs(3, True), cf=[], about=[r for r in ALL if r % 4 == 3])
    s.batch()
    s.load("degrade", degs(3, False, False), cf=[], about=exc)
    s.batch()
    s.tr.skip(20_000)
    s.load("degrade", degs(3, True), cf=[], about=exc)
    s.batch()
    s.load("degrade", degs(3, False, False), cf=[], about=exc)
    s.batch()
    s.tr.skip(70_000)
    s.load("degrade", degs(3, True), cf=[], about=exc)
    s.batch()
    return s


def script_owners():
    """Resources change owner on reload with THREAD counts and open entries in flight: THREAD head <-> THREAD + RT
    breaker; RateLimiter head <-> RateLimiter + a second flow rule; QPS -> QPS + param (XF_MIX / XF_PLITE) -> param
    only (k_pq, XF_PVPQ) -> none; QPS <-> limit_app "other" (PF_SERIAL, k_lane)."""
    keys = [E.param_key("o%d" % i) for i in range(5)]
    mix = [r for r in ALL if r % 4 == 2]
    s = Script("owners", 14, args={r: keys for r in mix})
    s.has_param = s.has_rl = True

    def load(stage, first=False):
        flow, deg, prm = [], [], []
        for r in ALL:
            k = r % 4
            if k == 0:
                flow.append(A.flow_rule(NAMES[r], threads(r), grade=A.FLOW_GRADE_THREAD))
                if stage in (1, 2):
                    deg.append(_rt(r, 4))
            elif k == 1:
                flow.append(_rl(r, qps(r)))
                if stage in (1, 2):
                    flow.append(A.flow_rule(NAMES[r], threads(r, 0.8), grade=A.FLOW_GRADE_THREAD))
            elif k == 2:
                if stage < 2:
                    flow.append(A.flow_rule(NAMES[r], qps(r, 0.6)))
                if stage in (1, 2):
                    prm.append(A.param_rule(NAMES[r], 0, scaled(r, 3, 3, 10, 100)))
            else:
                flow.append(A.flow_rule(NAMES[r], qps(r), limit_app="other" if stage in (1, 2) else None))
        cf = None if first else []
        s.load("flow", flow, cf=cf, about=[r for r in ALL if r % 4 in ((2,) if stage == 2 else (1, 3))])
        s.load("degrade", deg, cf=cf if stage != 2 else "same", about=[r for r in ALL if r % 4 == 0])
        s.load("param", prm, cf=cf if stage != 2 else "same", about=mix)

    load(0, True)
    s.batch()
    s.batch()
    load(1)
    s.batch()
    load(2)
    s.batch()
    s.batch()
    load(3)
    s.batch()
    s.batch()
    return s


def script_relate():
    """STRATEGY_RELATE comes to wide resources with history, is re-pointed and removed; references to a resource never
    entered, seen only in EXIT / TRACE events, first entered after the load; a member with a param rule."""
    keys = [E.param_key("r%d" % i) for i in range(5)]
    a, b, c = 20, 21, 22
    s = Script("relate", 15, args={14: keys})
    s.has_param = True

    def flows(ref):
        fl = [A.flow_rule(NAMES[r], qps(r, 0.6)) for r in ALL if ref is None or r not in (a, 0, 8, 14)]
        if ref is not None:  # (a passes while the referenced node's pass QPS is below 150; its own rule lets 240 pass)
            fl += [A.flow_rule(NAMES[a], 150, strategy=A.STRATEGY_RELATE, ref_resource=NAMES[ref]),
                   A.flow_rule(NAMES[0], 2, strategy=A.STRATEGY_RELATE, ref_resource=NAMES[R_NEVER]),
                   A.flow_rule(NAMES[8], 2, strategy=A.STRATEGY_RELATE, ref_resource=NAMES[R_EXIT_ONLY]),
                   A.flow_rule(NAMES[14], 6, strategy=A.STRATEGY_RELATE, ref_resource=NAMES[R_LATE])]
        return fl

    s.load("flow", flows(None))
    s.load("degrade", [_rt(r) for r in ALL if r % 4 == 3])  # (not on b, c: their windows hold passes)
    s.load("param", [A.param_rule(NAMES[14], 0, 12)])
    s.batch()
    s.batch()
    s.load("flow", flows(b), cf=[], about=[a, 0, 14])  # (8 passes either way in this batch: see the last load)
    s.tr.late_on = True
    s.batch()
    s.load("flow", flows(c), cf=[], about=[a])
    s.batch()
    s.load("flow", flows(None), cf=[], about=[a, 0, 8, 14])
    s.batch()
    s.batch()
    return s


def script_param_lifetime():
    """An unchanged param rule in a changed list keeps its token buckets, a changed one starts fresh; a resource
    that loses its rules loses its metric and thread-count maps; the empty list clears everything."""
    vals = ["p%d" % i for i in range(24)]  # more than a new map's first region (PM_MIN_NB * PM_BKT = 16): it grows
    keys = [E.param_key(v) for v in vals]
    par = [r for r in ALL if r % 2 == 0] + [21, 23]  # (every wide resource; 21 and 23 beside a flow rule: XF_MIX)
    s = Script("param_lifetime", 16, args={r: keys[:6] if r in LITE else keys for r in par})  # (lite: values that recur)
    s.has_param = True

    def grp(r):  # 0, 2: the rule stays as it is; 4: one field changes; 6: the resource loses its rule and gets it back
        return {20: 0, 21: 4, 22: 6, 23: 2}.get(r, (r + 4) % 8 if r in LITE else r % 8)

    def rule(r, f=1):
        return A.param_rule(NAMES[r], 0, scaled(r, 3, 3, 3, 9) * f, duration_in_sec=2,
                            items=[(vals[0], "java.lang.String", scaled(r, 1, 2, 3, 20)), (vals[1], "java.lang.String", 0)])

    def rules(keep=lambda r: True, f=lambda r: 1):
        # (group 6 also holds a THREAD-grade rule: its thread-count map goes and comes back with the metric)
        return [rule(r, f(r)) for r in par if keep(r)] + \
            [A.param_rule(NAMES[r], 0, scaled(r, 2, 2, 4, 30), grade=A.FLOW_GRADE_THREAD) for r in par if keep(r) and grp(r) == 6]

    s.load("flow", [A.flow_rule(NAMES[r], qps(r)) for r in ALL if r % 2])
    s.load("degrade", [_rt(r) for r in ALL if r % 4 == 1])
    s.load("param", rules())
    s.batch()
    s.batch()
    l1 = rules(lambda r: grp(r) != 6, lambda r: 3 if grp(r) == 4 else 1)
    # fresh buckets everywhere instead: the unchanged rules (groups 0, 2) must then decide otherwise
    s.load("param", l1, cf=[("param", []), ("param", l1)], about=[r for r in par if grp(r) in (0, 2)])
    s.batch()
    l2 = rules(f=lambda r: 3 if grp(r) == 4 else 1)
    s.load("param", l2, cf=[], about=[r for r in par if grp(r) == 6])
    s.batch()
    s.load("param", [], cf=[], about=par)
    s.batch()
    s.load("param", rules(), cf=[], about=par)
    s.batch()
    s.batch()
    return s


def script_async():
    """Two and three sg_submit_async batches, then a load of each kind: the load's drain decides the grouped batch
    under the old programs and the old component table."""
    keys = [E.param_key("a%d" % i) for i in range(5)]
    par = [r for r in ALL if r % 6 == 4]
    s = Script("async", 17, args={r: keys for r in par}, once=False)
    s.has_param = s.has_rl = True

    def flows(f, ref):
        # (a component of two J4 resources: its one lane stays short)
        # (... and lite limits that let a burst's ENTRYs through to the breakers)
        f = {r: f * (3 if r in LITE else 1) for r in ALL}
        return [A.flow_rule(NAMES[r], qps(r, f[r])) if r % 3 else _rl(r, qps(r, f[r])) for r in ALL if r != 14] + \
            [A.flow_rule(NAMES[14], 15, strategy=A.STRATEGY_RELATE, ref_resource=NAMES[ref])]

    def degs(w):
        return [_rt(r, w) if r % 4 == 0 or r in LITE else _count(r, w) for r in ALL if r % 2 == 0]

    def prms(f):
        return [A.param_rule(NAMES[r], 0, scaled(r, 1, 2, 6, 60) * f) for r in par]

    s.load("flow", flows(1.5, 17))
    s.load("degrade", degs(2))
    s.load("param", prms(1))
    s.run_async(2)
    s.load("flow", flows(1.0, 19), cf=[], about=ALL)
    s.run_async(3)
    s.load("degrade", degs(3), cf=[], about=[r for r in ALL if r % 2 == 0])
    s.run_async(2)
    s.load("param", prms(3), cf=[], about=par)
    s.batch()
    return s


FAIL_WIDE = 21  # 15 flow rules and one param rule: one more rule of any kind is its 17th


def script_failed_load():
    """Refused loads (a 17th rule on one resource, max_rules) leave the engine as it was."""
    keys = [E.param_key("f%d" % i) for i in range(5)]
    par = [4, 12, 16, FAIL_WIDE, 22]
    s = Script("failed_load", 18, args={r: keys for r in par + [2]}, cfg={"max_rules": 96})
    s.has_param = True
    many = [A.flow_rule(NAMES[FAIL_WIDE], 10_000 + k, grade=A.FLOW_GRADE_THREAD) for k in range(14)]
    flow = [A.flow_rule(NAMES[r], qps(r)) for r in ALL if r != 22] + many + \
        [A.flow_rule(NAMES[10], 1, limit_app="appA"), A.flow_rule(NAMES[15], 2, limit_app="appA")]
    deg = [_rt(r) if r % 4 == 0 else _count(r) for r in ALL if r % 2 == 0 and r != 22]  # (22: param rules only, k_pq)
    prm = [A.param_rule(NAMES[r], 0, scaled(r, 1, 1, 4, 40), duration_in_sec=2) for r in par]
    s.load("flow", flow)
    s.load("degrade", deg)
    s.load("param", prm)
    s.batch()
    s.batch()
    # flow: 17 distinct rules on one resource; an origin that only the surviving list names is interned afterwards
    s.add("fail", "flow", flow[:8] + [A.flow_rule(NAMES[3], 50 + k) for k in range(17)], A.SG_ENOTSUP)
    s.add("intern_origin", "appA")
    s.batch(origins={10: "appA", 15: "appA"})
    # param: a second param rule on FAIL_WIDE, a rule on a lower-numbered resource, one dropped elsewhere
    s.add("fail", "param", [A.param_rule(NAMES[2], 0, 1)] + [q for q in prm if q.resource != NAMES[12].encode()] +
          [A.param_rule(NAMES[FAIL_WIDE], 0, 7, duration_in_sec=3)], A.SG_ENOTSUP)
    s.batch(origins={10: "appA"})
    s.add("fail", "degrade", deg[3:] + [_rt(FAIL_WIDE, 5)], A.SG_ENOTSUP)
    s.batch()
    s.add("fail", "degrade", [A.degrade_rule(NAMES[r], 20 + k, 1) for r in ALL if r != FAIL_WIDE for k in range(3)],
          A.SG_ECAPACITY)
    s.batch()
    return s


SCRIPTS = {
    "flow_state": script_flow_state,
    "carry": script_carry,
    "breakers": script_breakers,
    "owners": script_owners,
    "relate": script_relate,
    "param_lifetime": script_param_lifetime,
    "async": script_async,
    "failed_load": script_failed_load,
}


@functools.lru_cache(maxsize=None)
def script(name):
    """The script and the oracle's results of its steps (played once per process)."""
    sc = SCRIPTS[name]()
    return sc, oracle_play(sc.steps)
