"""The authority rules on the CPU (no GPU needed): tests/authority_host.cpp compiles
sentinel_amd/csrc/authority.h -- the rule compiler sg_load_authority_rules uses and the lookup the kernels run
-- and prints verdicts, which are compared with the restatement of AuthorityRuleManager.loadAuthorityConf /
AuthorityRuleChecker.passCheck below (core/slots/block/authority/AuthorityRuleManager.java:105-157,
AuthorityRuleChecker.java:30-65).  Also here: sg_authority_rule's layout against ctypes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from sentinel_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "authority_host.cpp")
WHITE, BLACK = A.AUTHORITY_WHITE, A.AUTHORITY_BLACK


# ---- the reference, restated ---------------------------------------------------------------------------------
def java_split(s):
    """java.lang.String.split(","): trailing empty tokens are dropped, nothing is trimmed."""
    out = s.split(",")
    while out and out[-1] == "":
        out.pop()
    return out


def is_blank(s):
    return s is None or s.strip(" \t\n\r\f\v") == ""


def kept_rules(rules):
    """loadAuthorityConf: {resource: (limit_app, strategy)} -- the first valid rule of every resource."""
    kept = {}
    for resource, limit_app, strategy in rules:
        if is_blank(resource) or is_blank(limit_app) or strategy < 0:
            continue
        kept.setdefault(resource, (limit_app, strategy))
    return kept


def pass_check(limit_app, strategy, origin):
    """AuthorityRuleChecker.passCheck."""
    if not origin or not limit_app:
        return True
    contain = limit_app.find(origin) > -1
    if contain:
        contain = origin in java_split(limit_app)
    if strategy == BLACK and contain:
        return False
    if strategy == WHITE and not contain:
        return False
    return True


def blocks(kept, resource, origin):
    rule = kept.get(resource)
    return rule is not None and not pass_check(rule[0], rule[1], origin)


# ---- the program ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("authority") / "authority_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-o", out, SRC], check=True, capture_output=True)
    return out


def _hex(s):
    return "-" if s is None else "=" + s.encode().hex()


class Script:
    """Commands for authority_host and what each answer means."""

    def __init__(self):
        self.lines, self.kinds = [], []

    def load(self, rules):
        self.lines.append("load %d" % len(rules))
        self.lines += ["%d %s %s" % (st, _hex(r), _hex(l)) for r, l, st in rules]
        self.kinds.append("loaded")

    def intern(self, name):
        self.lines.append("intern " + _hex(name))
        self.kinds.append("id")

    def check(self, resource, origin_id):
        self.lines.append("check %s %d" % (_hex(resource), origin_id))
        self.kinds.append("v")

    def run(self, binary):
        r = subprocess.run([binary], input="\n".join(self.lines) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-500:] + r.stderr[-500:]
        out = [ln.split() for ln in r.stdout.splitlines()]
        assert [o[0] for o in out] == self.kinds
        return [int(o[1]) for o in out]


def _verdicts(binary, rules, origins, queries):
    """Intern origins in order, load rules, check every (resource, origin name); -> (n_loaded, ids, verdicts)."""
    s = Script()
    for o in origins:
        s.intern(o)
    s.load(rules)
    ids = {"": 0}
    for i, o in enumerate(dict.fromkeys(o for o in origins if o)):
        ids[o] = i + 1
    for res, o in queries:
        s.check(res, ids[o])
    out = s.run(binary)
    return out[len(origins)], out[:len(origins)], out[len(origins) + 1:]


KNOWN = [
    # AuthorityRuleCheckerTest.java:25-54, origin appA
    ("appA,appB", WHITE, "appA", False),
    ("appB", WHITE, "appA", True),
    ("appA", BLACK, "appA", True),
    ("appC", BLACK, "appA", False),
    # AuthoritySlotTest.java
    ("appA,appC", BLACK, "appA", True),
    ("appB, appE", WHITE, "appA", True),
    ("appB, appE", WHITE, "appE", True),   # the token is " appE"
    ("appB, appE", WHITE, " appE", False),
    # derived from the checker's code
    ("appA,appB", WHITE, "", False),       # the empty origin passes
    ("appA,appB", WHITE, "app", True),     # a substring is not a member
    ("appA,appB", BLACK, "app", False),
    ("appA,appB", BLACK, "appA,appB", False),  # an origin with a comma is never a member
    ("appA,appB", WHITE, "appA,appB", True),
    (",appA", BLACK, "appA", True),
    (",appA", WHITE, "appB", True),
    ("appA,,appB", BLACK, "appB", True),
    ("appA,,appB", WHITE, "appA", False),
    ("appA,", BLACK, "appA", True),
    ("appA,", WHITE, "appA", False),
    (",", WHITE, "appA", True),            # no token at all: a WHITE list nobody is on
    (",", BLACK, "appA", False),
    ("appA", 2, "appA", False),            # a strategy that is neither: valid, never blocks
    ("appB", 2, "appA", False),
]


def test_known_answers(binary):
    rules = [("res%d" % i, la, st) for i, (la, st, _, _) in enumerate(KNOWN)]
    origins = list(dict.fromkeys(o for _, _, o, _ in KNOWN))
    queries = [("res%d" % i, o) for i, (_, _, o, _) in enumerate(KNOWN)]
    n, _, got = _verdicts(binary, rules, origins, queries)
    assert n == len(KNOWN)
    want = [int(b) for _, _, _, b in KNOWN]
    assert got == want
    # and the restatement agrees with the known answers
    assert [int(blocks(kept_rules(rules), r, o)) for r, o in queries] == want


def test_invalid_rules_are_dropped_and_the_first_rule_wins(binary):
    rules = [
        ("a", "  ", BLACK),      # blank limit_app
        ("a", None, BLACK),
        ("", "appA", BLACK),     # blank resource
        (" \t", "appA", BLACK),
        (None, "appA", BLACK),
        ("a", "appA", -1),       # negative strategy
        ("a", "appB", BLACK),    # the first valid rule of a
        ("a", "appA", BLACK),    # ignored
        ("b", "appA", WHITE),
        ("b", "appB", WHITE),    # ignored
    ]
    queries = [("a", "appA"), ("a", "appB"), ("b", "appA"), ("b", "appB"), ("c", "appA"), ("", "appA")]
    n, _, got = _verdicts(binary, rules, ["appA", "appB"], queries)
    assert n == 2
    assert got == [0, 1, 0, 1, 0, 0]
    assert got == [int(blocks(kept_rules(rules), r, o)) for r, o in queries]


def test_empty_list_clears(binary):
    s = Script()
    s.intern("appA")
    s.load([("a", "appA", BLACK)])
    s.check("a", 1)
    s.load([])
    s.check("a", 1)
    assert s.run(binary) == [1, 1, 1, 0, 0]


def test_late_interning(binary):
    rules = [("a", "late,appA", BLACK), ("b", "late", WHITE), ("c", "appA", WHITE)]
    s = Script()
    s.intern("appA")                       # id 1
    s.load(rules)
    for res in "abc":
        s.check(res, 2)                    # nobody is 2 yet; as an id on no list: a, b, c = 0, 1, 1
    s.intern("other")                      # id 2: listed nowhere
    for res in "abc":
        s.check(res, 2)
    s.intern("late")                       # id 3
    for res in "abc":
        s.check(res, 3)
    for res in "abc":
        s.check(res, 2)                    # the unlisted name's verdicts did not move
    s.intern("late")                       # idempotent
    out = s.run(binary)
    assert out == [1, 3, 0, 1, 1, 2, 0, 1, 1, 3, 1, 0, 1, 0, 1, 1, 3]
    kept = kept_rules(rules)
    assert [int(blocks(kept, r, "late")) for r in "abc"] == [1, 0, 1]
    assert [int(blocks(kept, r, "other")) for r in "abc"] == [0, 1, 1]
    # the interned ids are those of a run without any rules
    s2 = Script()
    for nm in ("appA", "other", "late", "late"):
        s2.intern(nm)
    assert s2.run(binary) == [1, 2, 3, 3]


def test_random_rule_sets(binary):
    rng = np.random.default_rng(20240607)
    names = ["appA", "appB", "appC", "app", "a", " appA", "appA ", "x,y", "svc-%d" % 7, "Z"]
    total = 0
    s = Script()
    want = []
    for rnd in range(40):
        pool = ["r%d" % i for i in range(12)]
        rules = []
        for _ in range(int(rng.integers(0, 16))):
            toks = [names[int(k)] if rng.random() < 0.85 else "" for k in rng.integers(0, len(names), int(rng.integers(0, 5)))]
            la = ",".join(toks)
            if rng.random() < 0.05:
                la = None
            st = int(rng.choice([WHITE, BLACK, BLACK, WHITE, 2, -1]))
            res = pool[int(rng.integers(0, len(pool)))] if rng.random() < 0.95 else " "
            rules.append((res, la, st))
        # some origins are interned before the load, the rest after it (late interning); ids stay dense
        order = [names[int(k)] for k in rng.permutation(len(names))]
        cut = int(rng.integers(0, len(order) + 1))
        ids = {"": 0}
        for o in order[:cut]:
            s.intern("R%d|%s" % (rnd, o))
        s.load([(r if is_blank(r) else "R%d|%s" % (rnd, r), None if la is None else
                 ",".join("" if t == "" else "R%d|%s" % (rnd, t) for t in la.split(",")), st) for r, la, st in rules])
        for o in order[cut:]:
            s.intern("R%d|%s" % (rnd, o))
        base = rnd * len(names)
        for i, o in enumerate(order):
            ids[o] = base + i + 1
        want += [base + i + 1 for i in range(cut)] + [len(kept_rules(rules))] + [base + i + 1 for i in range(cut, len(order))]
        kept = kept_rules(rules)
        for res in pool:
            for o in [""] + names:
                s.check("R%d|%s" % (rnd, res), ids[o])
                want.append(int(blocks(kept, res, o)))
                total += 1
    assert total >= 4000
    got = s.run(binary)
    assert got == want


def test_struct_layout_matches_the_c_compiler(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "sentinel_gpu.h"\n'
        'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(sg_authority_rule), offsetof(sg_authority_rule, resource),'
        ' offsetof(sg_authority_rule, limit_app), offsetof(sg_authority_rule, strategy),'
        ' offsetof(sg_authority_rule, reserved));\n'
        '  printf("%d %d %d\\n", SG_AUTHORITY_WHITE, SG_AUTHORITY_BLACK, SG_BLOCK_AUTHORITY); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True,
                   capture_output=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    R = A.SgAuthorityRule
    assert [int(x) for x in out[:5]] == [ctypes.sizeof(R), R.resource.offset, R.limit_app.offset, R.strategy.offset,
                                         R.reserved.offset]
    assert [int(x) for x in out[5:]] == [A.AUTHORITY_WHITE, A.AUTHORITY_BLACK, A.BLOCK_AUTHORITY]
