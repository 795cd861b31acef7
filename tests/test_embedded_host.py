"""The embedded token server's test traces reach what the GPU cases are about (CPU; tests/embedded_util.py builds them
from the oracle alone), the shared request test (sentinel_amd/csrc/embedded.h) against a sequential model, and the
export.

Every GPU case of tests/test_gpu_embedded.py asserts nothing about its own trace: the conditions are checked here, on
the reference side -- at least 10 % of the requests OK and at least 10 % BLOCKED in every batch that has requests, and
at least one of each status the case names.
"""
import os
import subprocess

import numpy as np
import pytest

import embedded_util as X
from sentinel_amd import _abi as A
from sentinel_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _shares_ok(case, what):
    sh = X.shares(case)
    assert sh, what
    for k, (n, ok, bl) in enumerate(sh):
        assert ok >= 0.10 and bl >= 0.10, (what, k, n, ok, bl)


def _total(case):
    tot = {k: 0 for k in X.STATUSES}
    for an in case.answers:
        for k, v in X.answer_counts(an).items():
            tot[k] += v
    return tot


def test_owners_trace():
    c = X.owners_case()
    assert len(c.names) == 64 and len(c.eligible) == 8 and len(c.cuts) == 4
    assert 55_000 <= len(c.ev) <= 65_000 and 2900 <= int(c.ev["ts"][-1] - c.ev["ts"][0]) <= 3300
    assert all(5 <= t <= 50 for t in c.thresholds.values())
    # two (here: all) of the eligible resources have an RT or an exception-ratio breaker
    brk = {r.resource.decode() for r in c.degrade_rules
           if r.grade in (A.DEGRADE_GRADE_RT, A.DEGRADE_GRADE_EXCEPTION_RATIO)}
    assert sum(c.names[r] in brk for r in c.eligible) >= 2
    _shares_ok(c, "owners")
    assert all(len(rq) > 500 for rq in c.reqs)
    # an eligible segment of more than 2,000 events in every batch (the 1,024-lane owner's under the J16 owner set),
    # and eligible segments of at most 128 events (the lane bins' with the default bins)
    for a, b in zip(c.cuts[:-1], c.cuts[1:]):
        cnt = np.bincount(c.ev["res_id"][a:b], minlength=64)[sorted(c.eligible)]
        assert cnt.max() > 2000 and 0 < cnt.min() <= 128, cnt
    # EXITs and TRACEs name BLOCKED ENTRYs of their own batch and of the batch before
    ref = (c.ev["aux"] & np.uint64(A.REF_NONE)).astype(np.int64)
    i = np.nonzero((c.ev["kind"] != A.EV_ENTRY) & (ref < len(c.ev)))[0]
    i = i[c.blocked[ref[i]]]
    same = np.searchsorted(c.cuts, i, side="right") == np.searchsorted(c.cuts, ref[i], side="right")
    assert same.sum() >= 100 and (~same).sum() >= 5, (same.sum(), (~same).sum())
    assert {A.EV_EXIT, A.EV_TRACE} <= set(c.ev["kind"][i].tolist())
    # a breaker blocks entries that got a token, on an eligible resource
    got = (c.status == A.TOKEN_OK) & ((c.want & 0xFF) == A.BLOCK_DEGRADE)
    assert got.sum() >= 1
    # the mode changes words: W0 (today's decision of the same rules) differs
    assert (c.want != c.w0).sum() >= 1000


def test_long_trace():
    c = X.long_case()
    assert 75_000 <= len(c.ev) <= 85_000
    _shares_ok(c, "long")
    # runs of BLOCKED ENTRYs longer than two tiles of the widest owner, and breaker blocks after the cut
    b = c.blocked[c.ev["kind"] == A.EV_ENTRY]
    runs = np.diff(np.nonzero(np.diff(np.concatenate([[0], b.astype(np.int8), [0]])))[0])[::2]
    assert runs.max() > 2048, runs.max()
    assert ((c.want & 0xFF) == A.BLOCK_DEGRADE).sum() >= 100


@pytest.mark.parametrize("variant", ["flags", "chain", "nullctx", "off"])
def test_not_made_traces(variant):
    c = X.not_made_case(variant)
    ent = c.ev["kind"] == A.EV_ENTRY
    elig = ent & np.isin(c.ev["res_id"], list(c.eligible))
    skipped = elig & ~c.req_mask
    st = c.w0 & 0xFF
    if variant == "off":
        assert c.req_mask.sum() == 0 and (st[ent] == A.NO_CHECK).all()
        return
    _shares_ok(c, variant)
    assert skipped.sum() >= 100, skipped.sum()
    if variant == "flags":
        assert (skipped & c.auth_blk).sum() >= 20 and (skipped & ~c.auth_blk).sum() >= 100
        assert ((c.want & 0xFF) == X.BLOCK_AUTHORITY).sum() >= 20
    elif variant == "chain":
        assert (st[skipped] == A.NO_CHECK).all()
        assert 0 < len(np.unique(c.ev["res_id"][skipped])) < len(c.eligible)  # some eligible resources got a chain
    else:
        assert (st[skipped] == A.NO_CHECK).all() and c.nullctx[skipped].all()


def test_prioritized_trace():
    c = X.prio_case()
    _shares_ok(c, "prio")
    tot = _total(c)
    assert tot["should_wait"] >= 20, tot
    sw = c.status == A.TOKEN_SHOULD_WAIT
    assert c.prio[sw].all()  # only prioritized entries can get the answer
    assert ((c.want[sw] >> 16) > 0).sum() >= 10  # passes with a wait


def test_zero_avg_local_interleaved_limiter_traces():
    z = X.zero_case()
    _shares_ok(z, "zero")
    assert _total(z)["bad_request"] == int((z.zero & z.req_mask).sum()) >= 50
    assert ((z.want[z.zero & z.req_mask] & 0xFF) != A.BLOCK_FLOW).all()
    a = X.avg_local_case()
    _shares_ok(a, "avg_local")
    assert np.array_equal(a.status, X.owners_case().status)  # count / 3 x 3 connected: the same budget
    i = X.interleaved_case()
    _shares_ok(i, "interleaved")
    assert sorted(i.ext_answers) == [0, 1, 2]
    assert not np.array_equal(i.status, X.owners_case().status)  # the external calls took tokens
    lm = X.limiter_case()
    _shares_ok(lm, "limiter")
    for k, an in enumerate(lm.answers):  # refusals in the middle of every batch, in both namespaces
        t = np.nonzero(an["status"] == A.TOKEN_TOO_MANY_REQUEST)[0]
        assert len(t) >= 20 and t[0] > 0 and t[-1] < len(an) - 1, (k, len(t))
        for ns in ("ns-a", "ns-b"):
            fids = [f for f, n in lm.flow_ns.items() if n == ns]
            assert np.isin(lm.reqs[k]["flow_id"][t], fids).any(), (k, ns)
    refused = lm.status == A.TOKEN_TOO_MANY_REQUEST
    assert ((lm.want[refused] & 0xFF) != A.BLOCK_FLOW).all()
    t = X.toggled_case()
    assert len(t.reqs[0]) == 0 and np.array_equal(t.want[:t.cuts[1]], t.w0[:t.cuts[1]])
    _shares_ok(t, "toggled")


def test_small_batches_trace():
    c = X.small_case()
    sizes = np.diff(c.cuts)
    assert (sizes[1:-1] == X.SMALL_SIZE).all() and X.SMALL_SIZE <= 256 and len(sizes) == X.SMALL_BATCHES + 2
    _shares_ok(c, "small")
    assert all(len(rq) >= 10 for rq in c.reqs)
    # the small batches' words differ from today's decision of the same rules (what k_tiny would give)
    a, b = int(c.cuts[1]), int(c.cuts[-2])
    assert (c.want[a:b] != c.w0[a:b]).sum() >= 50
    # EXITs in the small batches name BLOCKED ENTRYs of earlier batches
    ref = (c.ev["aux"] & np.uint64(A.REF_NONE)).astype(np.int64)
    i = a + np.nonzero((c.ev["kind"][a:b] != A.EV_ENTRY) & (ref[a:b] < len(c.ev)))[0]
    i = i[c.blocked[ref[i]]]
    assert (np.searchsorted(c.cuts, i, side="right") != np.searchsorted(c.cuts, ref[i], side="right")).sum() >= 5


# ---------------------------------------------------------------- the shared header, on the CPU
def test_request_test_against_a_sequential_model(tmp_path):
    exe = tmp_path / "embedded_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), os.path.join(ROOT, "tests", "embedded_host.cpp")],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok" in out.stdout


# ---------------------------------------------------------------- the ABI
def test_export_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "sentinel_gpu.h")).read()
    assert "int sg_cluster_embedded(sg_engine* e, int32_t on);" in hdr
    assert "sg_cluster_embedded" in E.EXPORTS
    if os.path.exists(E.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", E.LIB_PATH], capture_output=True, text=True, check=True).stdout
        syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
        assert {"sg_cluster_embedded", "sgx_embedded_last"} <= syms
    assert hasattr(E.Engine, "cluster_embedded") and hasattr(E.Engine, "cluster_embedded_stats")
    assert len(E.Engine.EMBEDDED_STATS) == 12
