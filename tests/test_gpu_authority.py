"""AuthoritySlot on the device (sg_load_authority_rules, SG_BLOCK_AUTHORITY) against the reference semantics.

The oracle has no authority rules, and needs none: an authority verdict is a pure function of (rule, origin),
so the restatement of AuthorityRuleChecker.passCheck in tests/test_authority_host.py computes it, and the oracle
gets the same trace with SG_F_BLOCKED_UPSTREAM set on exactly the entries the rules block -- the flag is honoured
where AuthoritySlot sits (after ParamFlowSlot, before FlowSlot; param/slots/HotParamSlotChainBuilder.java:38-51).
The engine gets the rules and the trace as is.  Its decisions must be the oracle's with status 7 in place of 6 on
the entries the caller did not flag, and every node must be bit-identical.
"""
import numpy as np
import pytest

import pyoracle as O
import test_gpu_context_args as CA
from sentinel_amd import _abi as A
from sentinel_amd import engine as E
from test_authority_host import KNOWN, blocks, kept_rules

pytestmark = pytest.mark.gpu

T0 = CA.T0
WHITE, BLACK = A.AUTHORITY_WHITE, A.AUTHORITY_BLACK
ENTRY = A.EV_ENTRY


def _rules_of(tuples):
    return [A.authority_rule(r, la, st) for r, la, st in tuples]


# ---- 1. known answers through the engine -------------------------------------------------------------------------
@pytest.mark.parametrize("tiny", ["1", "0"])
def test_known_answers_through_the_engine(tiny, monkeypatch):
    monkeypatch.setenv("SG_TINY", tiny)  # "1": one k_tiny launch; "0": the batched path (group stage + k_lane)
    eng = E.Engine(max_resources=64, max_slot_chain_size=0)
    ids = {"": 0}
    for _, _, o, _ in KNOWN:
        if o and o not in ids:
            ids[o] = eng.intern_origin(o)
    assert sorted(ids.values()) == list(range(len(ids)))
    tuples = [("res%d" % i, la, st) for i, (la, st, _, _) in enumerate(KNOWN)]
    res = [eng.register(r) for r, _, _ in tuples]
    assert eng.load_authority_rules(_rules_of(tuples)) == len(KNOWN)
    # per case: the ENTRY, and an EXIT naming it (effective only if the ENTRY passed)
    n = 2 * len(KNOWN)
    ev = np.zeros(n, dtype=A.EVENT_DTYPE)
    ext = np.zeros(n, dtype=A.EXT_DTYPE)
    for i, (_, _, o, _) in enumerate(KNOWN):
        ev[2 * i] = (T0 + 2 * i, res[i], 1, ENTRY, 0, 0)
        ev[2 * i + 1] = (T0 + 2 * i + 1, res[i], 1, A.EV_EXIT, 0, A.aux_exit(2 * i, 1))
        ext["origin_id"][2 * i:2 * i + 2] = ids[o]
    d = eng.submit_ex(ev, ext)
    want = np.full(n, A.NOT_ENTRY, dtype=np.uint32)
    want[0::2] = [A.BLOCK_AUTHORITY if b else A.PASS for _, _, _, b in KNOWN]
    np.testing.assert_array_equal(d, want)  # (rule slot 0, wait 0: the word is the status)
    for i, (_, _, _, b) in enumerate(KNOWN):
        g = eng.read_node(res[i])
        m = g["minute"]
        live = m[:, 0] >= 0
        assert (int(m[live, 1].sum()), int(m[live, 2].sum()), int(m[live, 4].sum())) == ((0, 1, 0) if b else (1, 0, 1)), i
        assert g["thread"] == 0, i


# ---- 2. parity with the oracle by flag emulation -----------------------------------------------------------------
N_RES, N_ENTRIES, SEED = 48, 8000, 5


def _authority_tuples(n_res):
    """Rules on half the resources (those whose param rules block most): WHITE and BLACK, one-name and three-name
    lists, a padded token, a name no event carries, a list everybody is on; and rules the loader must drop."""
    kinds = [("appA", WHITE), ("appB,appC,appD", BLACK), ("appA, appB,appC", WHITE), ("appZ", BLACK), ("appA", BLACK),
             ("appA,appB,appC,appD", WHITE)]
    out = [("r0", "  ", BLACK), (" ", "appA", BLACK), ("r1", "appA", -1)]        # invalid: dropped
    with_rule = [i for i in range(n_res) if i % 4 < 2]
    for k, i in enumerate(with_rule):
        out.append(("r%d" % i,) + kinds[k % len(kinds)])
    out += [("r0", "appZ", WHITE), ("r1", "appA,appB,appC,appD", BLACK)]         # second rules: ignored
    return out, len(with_rule)


def _blocked_by_rules(ev, ext, kept, name_of):
    """Per event: an ENTRY the authority rules block (AuthorityRuleChecker.passCheck restated)."""
    out = np.zeros(len(ev), dtype=bool)
    for i in np.nonzero(ev["kind"] == ENTRY)[0]:
        out[i] = blocks(kept, "r%d" % ev["res_id"][i], name_of[int(ext["origin_id"][i])])
    return out


def _names(x, n_res, null_ctx):
    io = [x.intern_origin(o) for o in CA.ORIGINS]
    ic = [x.intern_context(c) for c in CA.CONTEXTS]
    for i in range(n_res):
        x.register("r%d" % i)
    nc = None
    if null_ctx:
        for k in range(A.MAX_CONTEXTS + 1 - len(CA.CONTEXTS)):
            nc = x.intern_context("filler%d" % k)
        assert nc == A.MAX_CONTEXTS + 1
    return io, ic, nc


def _load(x, n_res):
    flow, param, deg = CA._rules(n_res)
    x.load_flow_rules(flow)
    x.load_param_rules(param)
    x.load_degrade_rules(deg)


def _oracle_side(n_res=N_RES, n_entries=N_ENTRIES, seed=SEED):
    """The trace, the oracle's decisions under flag emulation and what they must show (no GPU involved)."""
    orc = O.Oracle(max_slot_chain_size=0)
    io, ic, nc = _names(orc, n_res, True)
    _load(orc, n_res)
    ev, ext, table = CA._trace(seed, n_res, n_entries, io, ic, null_ctx=nc)
    tuples, n_kept = _authority_tuples(n_res)
    kept = kept_rules(tuples)
    assert len(kept) == n_kept
    name_of = dict(zip(io, CA.ORIGINS))
    name_of[0] = ""
    blk = _blocked_by_rules(ev, ext, kept, name_of)
    caller = (ev["kind"] == ENTRY) & ((ev["flags"] & A.F_BLOCKED_UPSTREAM) != 0)
    ev_o = ev.copy()
    ev_o["flags"][blk] |= A.F_BLOCKED_UPSTREAM
    do = orc.submit_ex(ev_o, ext, table)
    st = do & 0xFF
    # the input exercises what it must (from the oracle's decisions alone)
    null = ext["context_id"] == nc
    assert (blk & ~caller & (st == A.BLOCK_UPSTREAM)).sum() >= 200
    assert (blk & (st == A.BLOCK_PARAM)).sum() >= 10
    assert (blk & caller).sum() >= 10
    assert (blk & null).sum() >= 10 and (st[blk & null] == A.NO_CHECK).all()
    hit = set(ev["res_id"][blk].tolist())
    assert sum(1 for r in kept if int(r[1:]) not in hit) >= 5
    want = do.copy()
    want[blk & ~caller & (st == A.BLOCK_UPSTREAM)] = A.BLOCK_AUTHORITY
    return dict(orc=orc, io=io, ic=ic, nc=nc, ev=ev, ext=ext, table=table, tuples=tuples, n_kept=n_kept, blk=blk,
                caller=caller, do=do, want=want)


@pytest.fixture(scope="module")
def side():
    return _oracle_side()


def _engine(side, n_res=N_RES):
    eng = E.Engine(max_resources=64, max_slot_chain_size=0, status_ring_log2=22)
    io, ic, nc = _names(eng, n_res, True)
    assert (io, ic, nc) == (side["io"], side["ic"], side["nc"])
    _load(eng, n_res)
    assert eng.load_authority_rules(_rules_of(side["tuples"])) == side["n_kept"]
    return eng


def _check_nodes(eng, orc, n_res, io, ic, origins=CA.ORIGINS):
    for r in range(n_res):
        g, o = eng.read_node(r), orc.read_node(r)
        assert g["thread"] == o["thread"], (r, g["thread"], o["thread"])
        np.testing.assert_array_equal(g["second"][:2], o["second"][:2], err_msg="second window of res %d" % r)
        np.testing.assert_array_equal(g["minute"], o["minute"], err_msg="minute window of res %d" % r)
        for kind, ids, names, read in ((0, io, origins, orc.read_origin_node), (1, ic, CA.CONTEXTS, orc.read_default_node)):
            for i, nm in zip(ids, names):
                ga, oa = eng.read_aux_node(r, kind, int(i)), read(r, nm)
                if oa is None:
                    assert ga is None or (ga["thread"] == 0 and (ga["second"][:, 0] < 0).all()), (r, kind, nm)
                    continue
                assert ga is not None and ga["thread"] == oa["thread"], (r, kind, nm)
                np.testing.assert_array_equal(ga["second"], oa["second"][:2], err_msg="node %d/%d/%s" % (r, kind, nm))


def _check_decisions(side, dg):
    ev, want, do = side["ev"], side["want"], side["do"]
    bad = np.nonzero(dg != want)[0]
    assert len(bad) == 0, "decision mismatch at event %d (%s): gpu=%08x want=%08x; %d mismatches" % (
        bad[0], ev[bad[0]], dg[bad[0]], want[bad[0]], len(bad))
    st = dg & 0xFF
    ent = ev["kind"] == ENTRY
    mapped = np.where(st == A.BLOCK_AUTHORITY, (dg & ~np.uint32(0xFF)) | np.uint32(A.BLOCK_UPSTREAM), dg)
    np.testing.assert_array_equal(mapped, do)
    np.testing.assert_array_equal(st == A.BLOCK_AUTHORITY, ent & ((do & 0xFF) == A.BLOCK_UPSTREAM) & ~side["caller"])
    np.testing.assert_array_equal(st == A.BLOCK_UPSTREAM, ent & ((do & 0xFF) == A.BLOCK_UPSTREAM) & side["caller"])
    assert (side["caller"][st == A.BLOCK_UPSTREAM]).all()


@pytest.mark.parametrize("way", ["one_batch", "hot_cold", "tiny", "pipeline"])
def test_parity_with_the_oracle_by_flag_emulation(side, way, monkeypatch):
    if way == "hot_cold":
        monkeypatch.setenv("SG_RADIX_BELOW", "0")
    eng = _engine(side)
    ev, ext, table = side["ev"], side["ext"], side["table"]
    n = len(ev)
    if way in ("one_batch", "hot_cold"):
        dg = eng.submit_ex(ev, ext, table)
    elif way == "tiny":  # batches of 1..256 events, each one k_tiny launch (the args table is shared: offsets hold)
        rng = np.random.default_rng(1)
        dg, a = [], 0
        while a < n:
            b = min(n, a + int(rng.integers(1, 257)))
            dg.append(eng.submit_ex(ev[a:b], ext[a:b], table))
            a = b
        dg = np.concatenate(dg)
    else:  # device buffers, back to back through the two-stage pipeline, one sync at the end
        import torch
        dev = torch.device("cuda", 0)
        d_ev = torch.from_numpy(np.ascontiguousarray(ev).view(np.uint8).copy()).to(dev)
        d_ext = torch.from_numpy(np.ascontiguousarray(ext).view(np.uint8).copy()).to(dev)
        d_tab = torch.from_numpy(np.ascontiguousarray(table).view(np.uint8).copy()).to(dev)
        d_out = torch.zeros(n, dtype=torch.int32, device=dev)
        cuts = np.linspace(0, n, 6).astype(np.int64)
        for a, b in zip(cuts[:-1], cuts[1:]):
            eng.submit_ex_ptr(d_ev.data_ptr() + int(a) * 24, d_ext.data_ptr() + int(a) * 16, int(b - a),
                              d_out.data_ptr() + int(a) * 4, sync=False, args_ptr=d_tab.data_ptr(), n_args=len(table))
        eng.sync()
        dg = d_out.cpu().numpy().view(np.uint32)
    _check_decisions(side, dg)
    _check_nodes(eng, side["orc"], N_RES, side["io"], side["ic"])


# ---- 3. rule and origin changes between batches ------------------------------------------------------------------
def _mini(seed, t_start, gbase, n_res, n_entries, origin_ids):
    """A small time-ordered batch: ENTRYs with origins, their EXITs (global references), ~4 % caller flags."""
    rng = np.random.default_rng(seed)
    raw, t = [], float(t_start)
    for k in range(n_entries):
        t += rng.exponential(4.0)
        ms = int(t)
        res = int(rng.integers(0, n_res))
        o = int(origin_ids[int(rng.integers(0, len(origin_ids)))])
        fl = A.F_BLOCKED_UPSTREAM if rng.random() < 0.04 else 0
        rt = int(rng.exponential(25.0))
        raw.append((ms, 0, ENTRY, res, k, fl, 0, o))
        raw.append((ms + rt, 1, A.EV_EXIT, res, k, 0, rt, o))
    raw.sort(key=lambda r: (r[0], r[1]))
    ev = np.zeros(len(raw), dtype=A.EVENT_DTYPE)
    ext = np.zeros(len(raw), dtype=A.EXT_DTYPE)
    pos = {}
    for i, (ms, _, kind, res, k, fl, rt, o) in enumerate(raw):
        ev[i] = (T0 + ms, res, 1, kind, fl, 0)
        ext["origin_id"][i] = o
        if kind == ENTRY:
            pos[k] = i
        else:
            ev["aux"][i] = A.aux_exit(gbase + pos[k], rt)
    return ev, ext, int(raw[-1][0]) + 1


def test_rule_and_origin_changes_between_batches():
    import torch
    dev = torch.device("cuda", 0)
    n_res = 8
    eng = E.Engine(max_resources=64, max_slot_chain_size=0, status_ring_log2=22)
    orc = O.Oracle(max_slot_chain_size=0)
    names = {0: ""}
    for x in (eng, orc):
        for nm in ("appA", "appB"):
            names[x.intern_origin(nm)] = nm
        for i in range(n_res):
            x.register("r%d" % i)
        # even resources: a flow rule; odd ones: a DegradeRule only (authority still precedes DegradeSlot)
        x.load_flow_rules([A.flow_rule("r%d" % i, 6) for i in range(0, n_res, 2)])
        x.load_degrade_rules([A.degrade_rule("r%d" % i, 10, 1) for i in range(1, n_res, 2)])
    assert sorted(names) == [0, 1, 2]
    state = dict(t=0, gbase=0, kept={}, dg=[], want=[], n7=[])

    def batch(seed, async_=False):
        ev, ext, t_end = _mini(seed, state["t"], state["gbase"], n_res, 300, sorted(names))
        blk = _blocked_by_rules(ev, ext, state["kept"], names)
        caller = (ev["kind"] == ENTRY) & ((ev["flags"] & A.F_BLOCKED_UPSTREAM) != 0)
        ev_o = ev.copy()
        ev_o["flags"][blk] |= A.F_BLOCKED_UPSTREAM
        do = orc.submit_ex(ev_o, ext)
        want = do.copy()
        want[blk & ~caller & ((do & 0xFF) == A.BLOCK_UPSTREAM)] = A.BLOCK_AUTHORITY
        state["want"].append(want)
        state["n7"].append(int((want == A.BLOCK_AUTHORITY).sum()))
        state["t"], state["gbase"] = t_end, state["gbase"] + len(ev)
        if not async_:
            state["dg"].append(eng.submit_ex(ev, ext))
            return None
        d_ev = torch.from_numpy(ev.view(np.uint8).copy()).to(dev)
        d_ext = torch.from_numpy(ext.view(np.uint8).copy()).to(dev)
        d_out = torch.zeros(len(ev), dtype=torch.int32, device=dev)
        eng.submit_ex_ptr(d_ev.data_ptr(), d_ext.data_ptr(), len(ev), d_out.data_ptr(), sync=False)
        return d_ev, d_ext, d_out

    def load(tuples):
        state["kept"] = kept_rules(tuples)
        return eng.load_authority_rules(_rules_of(tuples))

    batch(31)                                                        # 1. no authority rules yet
    black = [("r%d" % i, "late,appB", BLACK) for i in range(4)]
    assert load(black) == 4                                          # 2. names `late`, not interned yet
    held = batch(32, async_=True)                                    # 3. in flight ...
    late = eng.intern_origin("late")                                 # 4. ... while `late` gets its id
    assert late == orc.intern_origin("late") == 3
    names[late] = "late"
    eng.sync()
    state["dg"].append(held[2].cpu().numpy().view(np.uint32))
    batch(33)                                                        # 5. carries `late`: blocked on r0..r3
    assert load(black) == 4                                          # 6. the equal list: a no-op
    batch(34)
    assert load([("r%d" % i, "late", WHITE) for i in range(2, n_res)]) == n_res - 2   # 7. replaced
    batch(35)
    assert load([]) == 0                                             # 8. cleared
    batch(36)
    assert state["n7"][0] == 0 and state["n7"][5] == 0 and min(state["n7"][1:5]) >= 20, state["n7"]
    for k, (g, w) in enumerate(zip(state["dg"], state["want"])):
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, "batch %d: mismatch at event %d: gpu=%08x want=%08x; %d mismatches" % (
            k + 1, bad[0], g[bad[0]], w[bad[0]], len(bad))
    ids = sorted(i for i in names if i)
    _check_nodes(eng, orc, n_res, ids, [], origins=[names[i] for i in ids])


# ---- 4. Constants.ON == false ------------------------------------------------------------------------------------
def test_switch_off_ignores_the_rules():
    eng = E.Engine(max_resources=64, max_slot_chain_size=0, switch_on=0)
    a = eng.intern_origin("appA")
    r = eng.register("r")
    assert eng.load_authority_rules([A.authority_rule("r", "appA", BLACK)]) == 1
    ev = np.zeros(6, dtype=A.EVENT_DTYPE)
    ev["ts"], ev["res_id"], ev["count"], ev["kind"] = T0 + np.arange(6), r, 1, ENTRY
    ext = np.zeros(6, dtype=A.EXT_DTYPE)
    ext["origin_id"] = a
    np.testing.assert_array_equal(eng.submit_ex(ev, ext), np.full(6, A.NO_CHECK, dtype=np.uint32))
