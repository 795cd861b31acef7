"""The rule managers (sentinel_amd/csrc/rules.h) and the rule compiler (sentinel_amd/csrc/compile.h) on the CPU (no
GPU needed): tests/rules_host.cpp loads rule lists with the builders the engine uses and compiles them with the
compiler it uses.

(a) the compiled order of every resource against the oracle's (oracle/pyoracle.py Oracle.rule_order), on lists
    generated from fixed seeds; (b) a hand-written table of compiled programs: which owner bits (PF_* / XF_* / PX_*)
    and which DRule fields a rule set gives; (c) the size pre-check the loaders run and the compiler agree on every
    list; (d) the carry-over of rule states across a reload of one kind."""
import os
import random
import struct
import subprocess

import pytest

import pyoracle as O
from sentinel_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "rules_host.cpp")
HIPCC = "/opt/rocm/bin/hipcc"

PF_EXC_COUNT, PF_WARM, PF_PQ, PF_SERIAL, PF_RL, PF_RT, PF_FROZEN, PF_J16 = 1, 2, 4, 8, 16, 32, 64, 128
XF_PTHREAD, XF_MIX, XF_PLITE, XF_PVPQ, XF_HEADT, XF_HEADR, XF_EMB = 1, 2, 4, 8, 16, 32, 64
PX_MULTI, PX_ORIGIN, PX_CHAIN = 1, 2, 4
PB_INIT_ONLY = 0xFF
NO_ID = 0xFFFFFFFF
QPS, THREAD = A.FLOW_GRADE_QPS, A.FLOW_GRADE_THREAD
DEFAULT, WARM_UP, RATE_LIMITER, WARM_UP_RL = 0, 1, 2, 3
NAN = float("nan")
KINDS = {"flow": 0, "degrade": 1, "param": 2}  # Oracle.rule_order's kind


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("rules") / "rules_host")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "--offload-arch=gfx950", "-o", out, SRC], check=True,
                   capture_output=True)
    return out


# ------------------------------------------------------------------------------------------------ the program's text
def hx(b):
    return "-" if b is None else "=" + (b.encode() if isinstance(b, str) else b).hex()


def unhx(t):
    return bytes.fromhex(t[1:]).decode()


def dbits(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", x))[0]


def flow_line(r):
    return " ".join([hx(r.resource), hx(r.limit_app), hx(r.ref_resource), dbits(r.count)] + [str(v) for v in (
        r.grade, r.strategy, r.control_behavior, r.warm_up_period_sec, r.max_queueing_time_ms, r.cluster_mode,
        r.cluster_flow_id, r.cluster_threshold_type, r.cluster_fallback_to_local, r.cluster_strategy,
        r.cluster_sample_count, r.cluster_window_interval_ms)])


def degrade_line(r):
    return " ".join([hx(r.resource), hx(r.limit_app), dbits(r.count), str(r.time_window), str(r.grade)])


def param_line(r):
    f = [hx(r.resource), hx(r.limit_app), dbits(r.count)] + [str(v) for v in (
        r.duration_in_sec, r.grade, r.param_idx, r.has_param_idx, r.control_behavior, r.max_queueing_time_ms,
        r.burst_count, r.cluster_mode, r.cluster_flow_id, r.cluster_threshold_type, r.cluster_fallback_to_local,
        r.cluster_sample_count, r.cluster_window_interval_ms, r.n_items)]
    for k in range(r.n_items):
        it = r.items[k]
        f += [hx(it.object), hx(it.class_type), str(it.count), str(it.has_count)]
    return " ".join(f)


LINE = {"flow": flow_line, "degrade": degrade_line, "param": param_line}


class Script:
    """Commands for rules_host; run() gives one parsed block a command."""

    def __init__(self, **env):
        self.lines = []
        self.env(**env)

    def env(self, R=64, max_rules=1024, cold=3, mix_on=1, mix_pq=0, pv_on=1, pv_pq=1, emb_on=0):
        self.lines.append("env %d %d %d %d %d %d %d %d" % (R, max_rules, cold, mix_on, mix_pq, pv_on, pv_pq, emb_on))

    def forget(self, name):
        self.lines.append("forget " + hx(name))

    def origin(self, name):
        self.lines.append("origin " + hx(name))

    def context(self, name):
        self.lines.append("context " + hx(name))

    def load(self, kind, rules):
        self.lines.append("%s %d" % (kind, len(rules)))
        self.lines += [LINE[kind](r) for r in rules]

    def compile(self, keep_par=0, keep_flow=0, keep_deg=0):
        self.lines.append("compile %d %d %d" % (keep_par, keep_flow, keep_deg))

    def mark(self):
        self.lines.append("mark")

    def why(self, rule):
        self.lines += ["why", flow_line(rule)]

    def run(self, binary):
        r = subprocess.run([binary], input="\n".join(self.lines) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        blocks, cur = [], []
        for ln in r.stdout.splitlines():
            if ln == "done":
                blocks.append(cur)
                cur = []
            else:
                cur.append(ln)
        return blocks


def parse_load(block):
    """-> (kept, {src: hash}, {resource name: [src, ...]})"""
    kept, hashes, order = None, {}, {}
    for ln in block:
        f = ln.split()
        if f[0] == "loaded":
            kept = int(f[2])
        elif f[0] == "h":
            hashes[int(f[2])] = int(f[3])
        elif f[0] == "order":
            order[unhx(f[2])] = [int(x) for x in f[3:]]
    return kept, hashes, order


def kv(fields):
    return {k: int(v, 16) if k in ("count", "slope") else int(v) for k, v in (x.split("=") for x in fields)}


def parse_compile(block):
    c = {"prog": {}, "rules": [], "rst": [], "hot": [], "comp": {}, "emb": {}, "members": [], "emitted": {}}
    for ln in block:
        f = ln.split()
        if f[0] in ("limits", "embshape", "compiled"):
            c[f[0]] = (int(f[1]), unhx(f[2]))
        elif f[0] == "emitted":
            c["emitted"][unhx(f[1])] = (int(f[2]), int(f[3]))
        elif f[0] == "emitted-total":
            c["emitted_total"] = int(f[1])
        elif f[0] == "prog":
            c["prog"][unhx(f[1])] = kv(f[2:])
        elif f[0] == "rule":
            c["rules"].append(kv(f[2:]))
        elif f[0] == "rst":
            c["rst"].append(tuple(int(x) for x in f[2:]))
        elif f[0] == "hot":
            c["hot"].append((int(f[2]), int(f[3])))
        elif f[0] == "comp":
            c["comp"][int(f[1])] = int(f[2])
        elif f[0] == "members":
            c["members"] = [int(x) for x in f[1:]]
        elif f[0] == "emb":
            c["emb"][int(f[1])] = int(f[2])
        elif f[0] == "flags":
            c["flags"] = kv(f[1:])
    return c


def compiled(binary, env=None, origins=(), contexts=(), flow=None, degrade=None, param=None):
    """One compile of the given lists (param, flow, degrade loaded in that order)."""
    s = Script(**(env or {}))
    for o in origins:
        s.origin(o)
    for c in contexts:
        s.context(c)
    for kind, rules in (("param", param), ("flow", flow), ("degrade", degrade)):
        if rules is not None:
            s.load(kind, rules)
    s.compile()
    c = parse_compile(s.run(binary)[-1])
    check_limits(c, (env or {}).get("max_rules", 1024))
    return c


def check_limits(c, max_rules):
    """The pre-check's count of every resource is what the compiler emits for it with the size refusal left out
    (accepted or refused), and the pre-check and the compiler refuse exactly what those emitted counts say."""
    want = (0, "")
    for name, (emitted, counted) in c["emitted"].items():  # id order
        assert counted == emitted, name
        if emitted > 16 and want == (0, ""):
            want = (A.SG_ENOTSUP, "more than 16 rules on one resource: " + name)
    assert c["emitted_total"] == sum(e for e, _ in c["emitted"].values())
    if want == (0, "") and c["emitted_total"] > max_rules:
        want = (A.SG_ECAPACITY, "compiled rule table exceeds max_rules")
    assert c["limits"] == want and c["compiled"] == want
    for name, p in c["prog"].items():
        assert p["ncompiled"] == p["np"] + p["nf"] + p["nd"] == c["emitted"][name][0]


def rules_of(c, name):
    p = c["prog"][name]
    return c["rules"][p["off"]: p["off"] + p["np"] + p["nf"] + p["nd"]]


# ------------------------------------------------------------------------------------- (a) order against the oracle
NAMES = [("one-é", 1), ("two-资源", 2), ("r12", 12), ("r13-\U0001F600", 13), ("r16", 16)]
LAS = [None, "", "default", "appA", "other", "appÜ", "\U0001F680"]


def valid_rule(kind, rng, res, count, cluster=None):
    la = rng.choice(LAS)
    if cluster is None:
        cluster = rng.random() < 0.3
    if kind == "flow":
        beh = rng.choice([DEFAULT, DEFAULT, WARM_UP, RATE_LIMITER, WARM_UP_RL])
        strat = 0 if cluster else rng.choice([0, 0, 0, A.STRATEGY_RELATE, A.STRATEGY_CHAIN])
        return A.flow_rule(res, count, grade=rng.choice([QPS, QPS, THREAD]), limit_app=la, strategy=strat,
                           ref_resource=None if strat == 0 and rng.random() < 0.7 else rng.choice(["r12", "ctx-é", "two-资源"]),
                           control_behavior=beh, warm_up_period_sec=rng.choice([1, 10]),
                           max_queueing_time_ms=rng.choice([1, 500]), cluster_mode=cluster,
                           cluster_flow_id=rng.randrange(1, 1 << 40) if cluster else rng.choice([0, 0, 7]),
                           cluster_fallback_to_local=rng.random() < 0.5, cluster_sample_count=rng.choice([1, 10]),
                           cluster_window_interval_ms=1000)
    if kind == "degrade":
        return A.degrade_rule(res, count, rng.choice([1, 5, 60]), grade=rng.choice([0, 1, 2]), limit_app=la)
    items = [(str(rng.randrange(100)), rng.choice(["int", "java.lang.String", None]), rng.choice([0, 5, None, -1]))
             for _ in range(rng.choice([0, 0, 1, 3]))]
    return A.param_rule(res, rng.choice([0, 0, 1, 2, -1, -2]), count, grade=rng.choice([QPS, QPS, THREAD]),
                        duration_in_sec=rng.choice([1, 2, 60]), burst_count=rng.choice([0, 3]),
                        control_behavior=rng.choice([DEFAULT, RATE_LIMITER]), max_queueing_time_ms=rng.choice([0, 100]),
                        items=items, limit_app=la, cluster_mode=cluster,
                        cluster_flow_id=rng.randrange(1, 1 << 40) if cluster else 0,
                        cluster_fallback_to_local=rng.random() < 0.5)


def invalid_rules(kind):
    """One rule for every branch of the kind's isValidRule."""
    if kind == "flow":
        f = A.flow_rule
        cl = dict(cluster_mode=True, cluster_flow_id=5)
        return [f(None, 1), f("", 1), f(" \t", 1), f("bad", -1), f("bad", NAN), f("bad", 1, grade=-1),
                f("bad", 1, strategy=-1), f("bad", 1, control_behavior=-1),
                f("bad", 1, cluster_mode=True, cluster_flow_id=0), f("bad", 1, cluster_mode=True, cluster_flow_id=-3),
                f("bad", 1, cluster_sample_count=0, **cl), f("bad", 1, cluster_window_interval_ms=0, **cl),
                f("bad", 1, cluster_sample_count=3, cluster_window_interval_ms=1000, **cl),
                f("bad", 1, strategy=A.STRATEGY_RELATE, ref_resource="r12", **cl),
                f("bad", 1, strategy=A.STRATEGY_RELATE), f("bad", 1, strategy=A.STRATEGY_CHAIN, ref_resource=" "),
                f("bad", 1, control_behavior=WARM_UP, warm_up_period_sec=0),
                f("bad", 1, control_behavior=RATE_LIMITER, max_queueing_time_ms=0),
                f("bad", 1, control_behavior=WARM_UP_RL, warm_up_period_sec=0),
                f("bad", 1, control_behavior=WARM_UP_RL, max_queueing_time_ms=0)]
    if kind == "degrade":
        d = A.degrade_rule
        return [d(None, 1, 1), d("", 1, 1), d("  ", 1, 1), d("bad", -1, 1), d("bad", NAN, 1), d("r12", NAN, 5),
                d("bad", 1, 0), d("bad", 1, -1)]
    p = A.param_rule
    cl = dict(cluster_mode=True, cluster_flow_id=5)
    return [p(None, 0, 1), p("", 0, 1), p(" ", 0, 1), p("bad", 0, -1), p("bad", 0, NAN), p("bad", 0, 1, grade=-1),
            p("bad", None, 1), p("bad", 0, 1, burst_count=-1), p("bad", 0, 1, control_behavior=-1),
            p("bad", 0, 1, duration_in_sec=0), p("bad", 0, 1, max_queueing_time_ms=-1),
            p("bad", 0, 1, cluster_sample_count=0, **cl), p("bad", 0, 1, cluster_window_interval_ms=0, **cl),
            p("bad", 0, 1, cluster_sample_count=3, **cl), p("bad", 0, 1, cluster_mode=True, cluster_flow_id=0)]


def spread(h, cap):
    h &= 0xFFFFFFFF
    return (h ^ (h >> 16)) & (cap - 1)


def same_bucket(binary, kind, n):
    """n rules of resource "bucket9" whose hashes share a bucket of a 16-, 32- and 64-slot HashSet: candidates that
    differ in their count, chosen by the hashes the program reports."""
    rng = random.Random(99)
    cand = [valid_rule(kind, rng, "bucket9", float(c), cluster=False) for c in range(1, 1501)]
    s = Script()
    s.load(kind, cand)
    _, hashes, _ = parse_load(s.run(binary)[-1])
    by = {}
    for src in sorted(hashes):
        by.setdefault(spread(hashes[src], 64), []).append(src)
    best = max(by.values(), key=len)
    assert len(best) >= n
    return [cand[i] for i in best[:n]]


_LISTS = {}


def generated(binary, kind, seed):
    """The list of a (kind, seed): resources with 1, 2, 12, 13 and 16 distinct rules, 9 rules sharing a bucket, exact
    duplicates, rules equal under equals() with limit_app spelled null / "" / "default", invalid rules of every branch,
    NaN counts, negative param_idx, cluster rules among local ones -- shuffled."""
    if (kind, seed) in _LISTS:
        return _LISTS[(kind, seed)]
    rng = random.Random(seed)
    rules = []
    for name, k in NAMES:
        rules += [valid_rule(kind, rng, name, float(rng.randrange(1000) * 100 + j)) for j in range(k)]
    rules += same_bucket(binary, kind, 9)
    extra = [valid_rule(kind, rng, rng.choice(["dup-a", "dup-é\U0001F600"]), float(j)) for j in range(6)]
    for r in extra[:3]:  # one rule, limit_app spelled three ways: equal under equals()
        r.limit_app = None
    rules += extra + extra[:4]  # exact duplicates (the same structs again)
    for la in ("", "default"):
        for r in extra[:3]:
            rules.append(respell(kind, r, la))
    rules += invalid_rules(kind)
    if kind == "param":
        rules += [A.param_rule("neg", -1, 5), A.param_rule("neg", -3, 5), A.param_rule("neg", -1, 5)]
    rng.shuffle(rules)
    _LISTS[(kind, seed)] = rules
    return rules


def respell(kind, r, la):
    c = type(r)()
    for name, _ in r._fields_:
        setattr(c, name, getattr(r, name))
    c.limit_app = la.encode()
    if kind == "param":
        c._items = r._items
    return c


def names_of(rules):
    out = []
    for r in rules:
        n = r.resource
        if n is not None and n.strip(b" \t\n\r\f\v") and n.decode() not in out:
            out.append(n.decode())
    return out


CASES = [(k, s) for k in KINDS for s in (1, 2, 3)]


@pytest.mark.parametrize("kind,seed", CASES, ids=["%s-seed%d" % c for c in CASES])
def test_compiled_order_matches_oracle(binary, kind, seed):
    rules = generated(binary, kind, seed)
    s = Script()
    s.load(kind, rules)
    kept, _, order = parse_load(s.run(binary)[-1])
    orc = O.Oracle()
    n_orc = {"flow": orc.load_flow_rules, "degrade": orc.load_degrade_rules, "param": orc.load_param_rules}[kind](rules)
    assert kept == n_orc
    sizes = set()
    for name in names_of(rules):
        want = orc.rule_order(orc.register(name), KINDS[kind])
        assert order.get(name, []) == want, name
        sizes.add(len(want))
    assert {1, 2, 9, 12, 13, 16} <= sizes  # the HashSet's resize and 8-in-a-bucket branches are in the list
    orc.close()


# --------------------------------------------------------------------------------------- (b) known compiled programs
def only(c, name):
    r = rules_of(c, name)
    assert len(r) == 1
    return c["prog"][name], r[0]


def test_flow_one_qps_default(binary):
    p, d = only(compiled(binary, flow=[A.flow_rule("a", 10)]), "a")
    assert p["pflags"] == PF_FROZEN | PF_J16 and p["xf"] == 0 and p["multi"] == 0
    assert (d["kind"], d["grade"], d["behavior"], d["la_kind"], d["ref"], d["chain_ctx"]) == (1, QPS, 0, 0, NO_ID, NO_ID)


def test_flow_one_thread_default_is_head_t(binary):
    p, _ = only(compiled(binary, flow=[A.flow_rule("a", 10, grade=THREAD)]), "a")
    assert p["xf"] == XF_HEADT and p["pflags"] == PF_J16


def test_flow_one_rate_limiter_is_head_r(binary):
    c = compiled(binary, flow=[A.flow_rule("a", 10, control_behavior=RATE_LIMITER)])
    p, _ = only(c, "a")
    assert p["xf"] == XF_HEADR and p["pflags"] == PF_RL
    assert c["flags"]["any_head"] == 1


def test_flow_warm_up_rate_limiter_count_0_is_no_head(binary):
    p, _ = only(compiled(binary, flow=[A.flow_rule("a", 0, control_behavior=WARM_UP_RL)]), "a")
    assert p["pflags"] == PF_RL | PF_WARM and p["xf"] == 0


def test_flow_three_rate_limiters_are_serial(binary):
    c = compiled(binary, flow=[A.flow_rule("a", k, control_behavior=RATE_LIMITER) for k in (1, 2, 3)])
    assert c["prog"]["a"]["pflags"] == PF_RL | PF_SERIAL


def test_five_flow_or_five_degrade_rules_are_serial(binary):
    c = compiled(binary, flow=[A.flow_rule("a", k) for k in range(5)], degrade=[A.degrade_rule("b", k, 1) for k in range(5)])
    assert c["prog"]["a"]["pflags"] == PF_SERIAL | PF_FROZEN
    assert c["prog"]["b"]["pflags"] == PF_SERIAL | PF_FROZEN | PF_RT
    four = compiled(binary, flow=[A.flow_rule("a", k) for k in range(4)], degrade=[A.degrade_rule("b", k, 1) for k in range(4)])
    assert not four["prog"]["a"]["pflags"] & PF_SERIAL and not four["prog"]["b"]["pflags"] & PF_SERIAL


def test_three_flow_rules_lose_j16(binary):
    assert compiled(binary, flow=[A.flow_rule("a", k) for k in range(3)])["prog"]["a"]["pflags"] == PF_FROZEN
    assert compiled(binary, flow=[A.flow_rule("a", k) for k in range(2)])["prog"]["a"]["pflags"] == PF_FROZEN | PF_J16


def test_flow_limit_app_other_and_origin(binary):
    # "other" beside a cluster-only rule of an interned origin: hot_n counts the skipped origin
    c = compiled(binary, origins=["appA", "appB"],
                 flow=[A.flow_rule("a", 10, limit_app="other"),
                       A.flow_rule("a", 5, limit_app="appB", cluster_mode=True, cluster_flow_id=9, cluster_fallback_to_local=False),
                       A.flow_rule("a", 5, limit_app="never-seen", cluster_mode=True, cluster_flow_id=10, cluster_fallback_to_local=False),
                       A.flow_rule("b", 10, limit_app="appA")])
    p, d = only(c, "a")
    assert p["pflags"] & PF_SERIAL and p["multi"] == PX_ORIGIN
    assert d["la_kind"] == 2 and d["hot_n"] == 1 and c["hot"][d["hot_off"]] == (2, 0)
    p, d = only(c, "b")
    assert p["pflags"] & PF_SERIAL and p["multi"] == PX_ORIGIN
    assert (d["la_kind"], d["la_origin"], d["hot_n"]) == (1, 1, 0)


def test_flow_chain_on_default_context(binary):
    c = compiled(binary, contexts=["ctx"],
                 flow=[A.flow_rule("a", 10, strategy=A.STRATEGY_CHAIN, ref_resource="sentinel_default_context"),
                       A.flow_rule("b", 10, strategy=A.STRATEGY_CHAIN, ref_resource="ctx"),
                       A.flow_rule("c", 10, strategy=A.STRATEGY_CHAIN, ref_resource="unseen")])
    for name, ctx in (("a", 0), ("b", 1), ("c", NO_ID)):
        p, d = only(c, name)
        assert p["multi"] == PX_CHAIN and p["pflags"] & PF_SERIAL and d["chain_ctx"] == ctx


def test_flow_relate_component(binary):
    # a -> b with a < b; c names itself
    c = compiled(binary, flow=[A.flow_rule("a", 10, strategy=A.STRATEGY_RELATE, ref_resource="b"),
                               A.flow_rule("c", 10, strategy=A.STRATEGY_RELATE, ref_resource="c")])
    ids = {n: p["id"] for n, p in c["prog"].items()}
    assert ids == {"a": 0, "b": 1, "c": 2}
    assert c["comp"] == {1: 0} and c["members"] == [0, 1] and c["flags"]["any_multi"] == 1
    assert c["prog"]["a"]["multi"] == PX_MULTI and c["prog"]["a"]["pflags"] & PF_SERIAL
    assert c["prog"]["b"]["multi"] == 0 and not c["prog"]["b"]["pflags"] & PF_SERIAL
    assert c["prog"]["c"]["multi"] == 0 and rules_of(c, "c")[0]["ref"] == NO_ID
    assert rules_of(c, "a")[0]["ref"] == 1
    alone = compiled(binary, flow=[A.flow_rule("c", 10, strategy=A.STRATEGY_RELATE, ref_resource="c")])
    assert alone["flags"]["comp"] == 0 and alone["flags"]["any_multi"] == 0


def test_flow_relate_unknown_reference_forms_no_component(binary):
    # The list builder registers a RELATE rule's ref_resource, so a load never hands the compiler a name without an
    # id: the name is taken out of the id map after the load, or max_resources lowered to the reference's id
    rules = [A.flow_rule("a", 10, strategy=A.STRATEGY_RELATE, ref_resource="b")]
    gone, beyond = Script(), Script()
    for s in (gone, beyond):
        s.load("flow", rules)
    gone.forget("b")
    beyond.env(R=1)
    for s in (gone, beyond):
        s.compile()
        c = parse_compile(s.run(binary)[-1])
        assert c["compiled"] == (0, "")
        p, d = only(c, "a")
        assert d["ref"] == NO_ID and d["strategy"] == A.STRATEGY_RELATE
        assert p["multi"] == 0 and p["pflags"] == PF_FROZEN | PF_J16
        assert c["comp"] == {} and c["members"] == [] and c["flags"]["comp"] == 0 and c["flags"]["any_multi"] == 0


def test_flow_warm_up_constants(binary):
    p, d = only(compiled(binary, flow=[A.flow_rule("a", 10, control_behavior=WARM_UP, warm_up_period_sec=10)]), "a")
    assert p["pflags"] & PF_WARM
    assert (d["warning_token"], d["max_token"], d["count_div_cold"]) == (50, 100, 3)
    assert d["slope"] == int(dbits((3 - 1.0) / 10.0 / (100 - 50)), 16) == int(dbits(0.004), 16)


@pytest.mark.parametrize("pv_on,pv_pq", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_param_alone_on_idx_0_is_pq(binary, pv_on, pv_pq):
    c = compiled(binary, env=dict(pv_on=pv_on, pv_pq=pv_pq), param=[A.param_rule("a", 0, 5)])
    p, d = only(c, "a")
    # (PF_SERIAL beside PF_PQ: param rules outside XF_MIX are never the cooperative owners'; PF_PQ names k_pq)
    assert p["pflags"] == PF_PQ | PF_SERIAL | PF_FROZEN | PF_J16
    assert p["xf"] == (XF_PVPQ if pv_on and pv_pq else 0)
    assert (d["kind"], d["param_idx"], d["token_count"], d["duration_sec"]) == (0, 0, 5, 1)


def test_param_on_idx_1_is_serial(binary):
    p, _ = only(compiled(binary, param=[A.param_rule("a", 1, 5)]), "a")
    assert p["pflags"] & PF_SERIAL and not p["pflags"] & PF_PQ and p["xf"] == 0


def test_param_qps_and_thread_pq_only_when_thread_is_checked_last(binary):
    seen = set()
    for count in range(1, 40):
        rules = [A.param_rule("a", 0, count), A.param_rule("a", 0, count, grade=THREAD)]
        s = Script()
        s.load("param", rules)
        s.compile()
        blocks = s.run(binary)
        order = parse_load(blocks[-2])[2]["a"]
        p = parse_compile(blocks[-1])["prog"]["a"]
        assert p["xf"] == XF_PTHREAD
        thread_last = order[-1] == 1
        assert bool(p["pflags"] & PF_PQ) == thread_last and p["pflags"] & PF_SERIAL
        seen.add(thread_last)
    assert seen == {True, False}


def test_param_beside_flow_rule_is_mix(binary):
    lists = dict(param=[A.param_rule("a", 0, 5)], flow=[A.flow_rule("a", 10)])
    c = compiled(binary, env=dict(mix_on=1), **lists)
    p = c["prog"]["a"]
    assert p["xf"] == XF_MIX | XF_PLITE and not p["pflags"] & (PF_SERIAL | PF_PQ) and c["flags"]["any_mix"] == 1
    c = compiled(binary, env=dict(mix_on=0), **lists)
    p = c["prog"]["a"]
    assert p["xf"] == 0 and p["pflags"] & PF_SERIAL and c["flags"]["any_mix"] == 0


def test_param_cluster_rules_without_fallback_are_one_init_only_rule(binary):
    cl = dict(cluster_mode=True, cluster_fallback_to_local=False)
    c = compiled(binary, param=[A.param_rule("a", 0, 5, cluster_flow_id=1, **cl), A.param_rule("a", 2, 5, cluster_flow_id=2, **cl)])
    p, d = only(c, "a")
    assert p["np"] == 1 and d["behavior"] == PB_INIT_ONLY and d["burst"] == 0b101


CLUSTER_FLOW = dict(cluster_mode=True, cluster_flow_id=77, cluster_fallback_to_local=False)


def test_cluster_flow_rule_without_fallback_has_no_flow_stage(binary):
    c = compiled(binary, flow=[A.flow_rule("a", 10, **CLUSTER_FLOW)], degrade=[A.degrade_rule("a", 1, 1)])
    p = c["prog"]["a"]
    assert (p["nf"], p["nd"], p["xf"]) == (0, 1, 0) and c["emb"] == {}


def test_cluster_flow_rule_embedded(binary):
    c = compiled(binary, env=dict(emb_on=1), flow=[A.flow_rule("a", 10, **CLUSTER_FLOW)], degrade=[A.degrade_rule("a", 1, 1)])
    p = c["prog"]["a"]
    assert (p["nf"], p["nd"], p["xf"]) == (0, 1, XF_EMB) and c["emb"] == {0: 77} and c["embshape"] == (0, "")


def _cl(res="a", fid=77, **kw):
    return A.flow_rule(res, 10, **{**CLUSTER_FLOW, "cluster_flow_id": fid, **kw})


WHY = [
    ("it is not the only flow rule of its resource", dict(flow=[_cl(), A.flow_rule("a", 5)])),
    ("it is not QPS grade", dict(flow=[_cl(grade=THREAD)])),
    ("its limitApp is not \"default\"", dict(flow=[_cl(limit_app="appA")])),
    ("another flow rule uses its flowId", dict(flow=[_cl(), _cl(res="b")])),
    ("its resource has param rules", dict(flow=[_cl()], param=[A.param_rule("a", 0, 5)])),
    ("its resource is in a STRATEGY_RELATE component",
     dict(flow=[_cl(), A.flow_rule("b", 5, strategy=A.STRATEGY_RELATE, ref_resource="a")])),
    ("cluster_fallback_to_local is not decided in embedded mode", dict(flow=[_cl(cluster_fallback_to_local=True)])),
]


@pytest.mark.parametrize("why,lists", WHY, ids=[w[0] for w in WHY])
def test_embedded_shape_refusals(binary, why, lists):
    c = compiled(binary, env=dict(emb_on=1), **lists)
    assert c["embshape"] == (A.SG_ENOTSUP, "embedded token server: cluster flow rule 77 on a is outside the supported "
                                           "shape: " + why)
    assert not c["prog"]["a"]["xf"] & XF_EMB and 0 not in c["emb"]


def test_embedded_shape_strategy_reason(binary):
    # FlowRuleUtil.isValidRule drops a cluster rule whose strategy is not DIRECT, so no load reaches this reason:
    # the shape test is asked about the record directly
    rule = _cl(strategy=A.STRATEGY_RELATE, ref_resource="b")
    s = Script(emb_on=1)
    s.load("flow", [rule])
    s.why(rule)
    blocks = s.run(binary)
    assert parse_load(blocks[-2])[0] == 0
    assert blocks[-1] == ["why " + hx("its strategy is not DIRECT")]


# ------------------------------------------------------------------------------------------------------- (c) limits
# compiled() checks every compile against the DRules the compiler emits with its refusal left out (check_limits);
# here the lists built to land on the limits, with the counts and the refusals they must give
@pytest.mark.parametrize("kind,seed", CASES, ids=["%s-seed%d" % c for c in CASES])
def test_limits_precheck_agrees_with_compiler_on_generated_lists(binary, kind, seed):
    rules = generated(binary, kind, seed)
    c = compiled(binary, **{kind: rules})
    assert c["compiled"] == (0, "") and max(e for e, _ in c["emitted"].values()) <= 16
    assert c["emitted_total"] > 30
    c = compiled(binary, env=dict(max_rules=30), **{kind: rules})
    assert c["limits"] == c["compiled"] == (A.SG_ECAPACITY, "compiled rule table exceeds max_rules")


def _on_a(c):
    """(DRules emitted for resource a, the refusal of the pre-check, of the compiler)"""
    return c["emitted"]["a"][0], c["limits"], c["compiled"]


def test_limits_16_and_17_rules_on_a_resource(binary):
    ok, too_many = (0, ""), (A.SG_ENOTSUP, "more than 16 rules on one resource: a")
    cl = dict(cluster_mode=True, cluster_fallback_to_local=False)
    flows = [A.flow_rule("a", k) for k in range(17)]
    assert _on_a(compiled(binary, flow=flows[:16])) == (16, ok, ok)
    assert _on_a(compiled(binary, flow=flows)) == (17, too_many, too_many)
    # 17 raw flow rules, one of them cluster-only: 16 compiled
    assert _on_a(compiled(binary, flow=flows[:16] + [A.flow_rule("a", 1, cluster_flow_id=3, **cl)])) == (16, ok, ok)
    # across kinds: 6 + 6 + 4 = 16, and one more of any kind
    mixed = dict(param=[A.param_rule("a", 0, k) for k in range(6)], flow=flows[:6], degrade=[A.degrade_rule("a", k, 1) for k in range(4)])
    assert _on_a(compiled(binary, **mixed)) == (16, ok, ok)
    mixed["degrade"].append(A.degrade_rule("a", 9, 1))
    assert _on_a(compiled(binary, **mixed)) == (17, too_many, too_many)
    # 17 raw param rules: a run of cluster rules without fallback on fixed indices is one compiled rule
    params = [A.param_rule("a", k % 3, k, cluster_flow_id=100 + k, **cl) for k in range(17)]
    assert _on_a(compiled(binary, param=params)) == (1, ok, ok)
    assert _on_a(compiled(binary, param=[A.param_rule("a", 0, k) for k in range(17)])) == (17, too_many, too_many)
    # a negative index never joins a run
    neg = [A.param_rule("a", -1, k, cluster_flow_id=100 + k, **cl) for k in range(17)]
    assert _on_a(compiled(binary, param=neg)) == (17, too_many, too_many)


def test_limits_17_raw_param_rules_with_runs_between_local_rules(binary):
    # 9 cluster rules without fallback among 8 local ones: the HashSet order decides which of the 9 are neighbours;
    # the expected count is told from that order
    cl = dict(cluster_mode=True, cluster_fallback_to_local=False)
    rules = [A.param_rule("a", k % 3, k, cluster_flow_id=100 + k, **cl) for k in range(9)] + [A.param_rule("a", 0, k) for k in range(8)]
    s = Script()
    s.load("param", rules)
    s.compile()
    blocks = s.run(binary)
    order = parse_load(blocks[-2])[2]["a"]
    assert sorted(order) == list(range(17))
    want = sum(1 for k, src in enumerate(order) if not (src < 9 and k > 0 and order[k - 1] < 9))
    assert want <= 16  # (17 only if no two of the 9 were neighbours)
    c = parse_compile(blocks[-1])
    check_limits(c, 1024)
    assert _on_a(c) == (want, (0, ""), (0, ""))


def test_limits_max_rules_and_one_more(binary):
    flows = [A.flow_rule("r%d" % (k // 10), k) for k in range(21)]
    c = compiled(binary, env=dict(max_rules=20), flow=flows[:20])
    assert (c["emitted_total"], c["limits"], c["compiled"]) == (20, (0, ""), (0, ""))
    c = compiled(binary, env=dict(max_rules=20), flow=flows)
    refused = (A.SG_ECAPACITY, "compiled rule table exceeds max_rules")
    assert (c["emitted_total"], c["limits"], c["compiled"]) == (21, refused, refused)


# --------------------------------------------------------------------------------------------------- (d) carry-over
def marked(i):
    return (1000 + i, 2000 + i, 3000 + i, 4000 + i)


PARAM_INIT, FLOW_INIT, DEG_INIT = (0, 0, 0, 0), (0, 0, -1, 0), (0, 0, 0, 0)


def test_carry_over_of_rule_states(binary):
    s = Script()
    s.load("param", [A.param_rule("a", 0, 5)])
    s.load("flow", [A.flow_rule("a", 1), A.flow_rule("a", 2), A.flow_rule("b", 1)])
    s.load("degrade", [A.degrade_rule("a", 1, 1), A.degrade_rule("b", 1, 1)])
    s.compile()  # a: param 0, flow 1 2, degrade 3; b: flow 4, degrade 5
    s.mark()
    # flow rules reloaded, a gains one: b's rule_off shifts.  Param and degrade states follow their resource, flow
    # states reset
    s.load("flow", [A.flow_rule("a", 1), A.flow_rule("a", 2), A.flow_rule("a", 3), A.flow_rule("b", 1)])
    s.compile(keep_par=1, keep_flow=0, keep_deg=1)  # a: param 0, flow 1 2 3, degrade 4; b: flow 5, degrade 6
    s.mark()
    # param rules reloaded, b gains one: its flow and degrade states move behind it
    s.load("param", [A.param_rule("a", 0, 5), A.param_rule("b", 0, 7)])
    s.compile(keep_par=0, keep_flow=1, keep_deg=1)  # a: param 0, flow 1 2 3, degrade 4; b: param 5, flow 6, degrade 7
    s.mark()
    # degrade rules reloaded, a gains one: param and flow states follow their resource, degrade states reset
    s.load("degrade", [A.degrade_rule("a", 1, 1), A.degrade_rule("a", 2, 1), A.degrade_rule("b", 1, 1)])
    s.compile(keep_par=1, keep_flow=1, keep_deg=0)  # a: param 0, flow 1 2 3, degrade 4 5; b: param 6, flow 7, degrade 8
    s.mark()
    # a kept kind whose count changed on one resource: that resource's rules of the kind start afresh, all else stays
    s.load("flow", [A.flow_rule("a", 1), A.flow_rule("b", 1)])
    s.compile(keep_par=1, keep_flow=1, keep_deg=1)  # a: param 0, flow 1, degrade 2 3; b: param 4, flow 5, degrade 6
    blocks = s.run(binary)
    c1, c2, c3, c4, c5 = (parse_compile(blocks[i]) for i in (4, 7, 10, 13, 16))
    assert c1["rst"] == [PARAM_INIT, FLOW_INIT, FLOW_INIT, DEG_INIT, FLOW_INIT, DEG_INIT]
    assert c2["prog"]["b"]["off"] == 5
    assert c2["rst"] == [marked(0), FLOW_INIT, FLOW_INIT, FLOW_INIT, marked(3), FLOW_INIT, marked(5)]
    assert (c3["prog"]["b"]["off"], c3["prog"]["b"]["np"]) == (5, 1)
    assert c3["rst"] == [PARAM_INIT, marked(1), marked(2), marked(3), marked(4), PARAM_INIT, marked(5), marked(6)]
    assert c4["rst"] == [marked(0), marked(1), marked(2), marked(3), DEG_INIT, DEG_INIT, marked(5), marked(6), DEG_INIT]
    assert c5["rst"] == [marked(0), FLOW_INIT, marked(4), marked(5), marked(6), marked(7), marked(8)]
