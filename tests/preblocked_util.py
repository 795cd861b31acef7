"""Traces with pre-blocked ENTRYs, and their oracle results (helper of test_gpu_preblocked.py / test_preblocked_host.py).

A pre-blocked ENTRY is one SystemSlot or AuthoritySlot stopped before FlowSlot: it carries SG_F_BLOCKED_UPSTREAM, or
its resource's authority rule rejects its origin.  flag() sets the caller's flag on a ~10 % random share of a
counts_util trace's ENTRYs and, on the hottest resources of every flagged batch, on one run of consecutive ENTRYs
that covers more than two tiles of the widest cooperative owner (1,024 positions a tile) and spans a 500 ms bucket
edge.  reference() replays the flagged trace through the oracle once per process -- the oracle honours the flag
itself -- and keeps what the device is compared with.

The authority rules have no oracle of their own and need none (tests/test_gpu_authority.py): the verdict is a pure
function of (rule, origin), test_authority_host.blocks() restates it, the oracle gets the flag on the entries the
rules block, and the device must answer status 7 where the oracle says 6 and the caller did not flag.
"""
import functools

import numpy as np

import counts_util as U
import pyoracle as O
from sentinel_amd import _abi as A
from sentinel_amd import engine as E
from sentinel_amd import tracegen as T
from test_authority_host import blocks, kept_rules

# counts_util's shapes at 150,000 entries a second: a batch of a third of the trace spans about a second, so every batch
# holds 500 ms bucket edges (counts_util's own traces last ~600 ms in all) and the hot resources still saturate
RATE = 150_000.0
TRACES = {
    "c2": (2, dict(n_entries=400_000, rate=RATE)),
    "c3": (3, dict(n_entries=400_000, n_res=20_000, variant=T.V_WARM_RL, rate=RATE)),
    "c4": (4, dict(n_entries=400_000, n_res=50_000, rate=RATE)),
    "c2hot": (2, dict(n_entries=300_000, n_res=12, rate=RATE)),
    "c4hot": (4, dict(n_entries=300_000, n_res=12, rate=RATE)),
    "c4flat": (4, dict(n_entries=30_000, n_res=400, rate=RATE)),  # the placement test: no segment above 5,000 events
}


@functools.lru_cache(maxsize=None)
def workload(name):
    config, kw = TRACES[name]
    return T.Workload(config, **kw)


TILE = {"J1": 64, "J4": 256, "J8": 512, "J16": 1024}  # positions a tile of k_jac<NW, 1>
WIDEST = TILE["J16"]
FLAG_SEED = 23
SHARE = 0.10
N_HOT = 4
ENTRY = A.EV_ENTRY
REF_NONE = np.uint64(A.REF_NONE)


def runs_for(ev, a, b, n_res, n_hot=N_HOT, tile=WIDEST):
    """Per hottest resource of the batch [a, b): the batch-relative event indices of a window of more than two tiles
    of its segment, centred on a 500 ms bucket edge (None where the segment has no such window)."""
    res = ev["res_id"][a:b]
    cnt = np.bincount(res, minlength=n_res)
    half = tile + tile // 8 + 1
    out = []
    for r in np.argsort(-cnt, kind="stable")[:n_hot]:
        idx = np.nonzero(res == r)[0]
        bk = ev["ts"][a:b][idx] // 500
        edge = np.nonzero(bk[1:] != bk[:-1])[0] + 1
        edge = edge[(edge >= half) & (edge + half <= len(idx))]
        out.append((int(r), idx[edge[len(edge) // 2] - half:edge[len(edge) // 2] + half] if len(edge) else None))
    return out


def flag(ev, cuts, n_res, flagged_batches, seed=FLAG_SEED, share=SHARE, n_hot=N_HOT, tile=WIDEST):
    """The mask of the ENTRYs to pre-block: in the batches named, a random share and the runs of runs_for()."""
    m = np.zeros(len(ev), dtype=bool)
    ent = ev["kind"] == ENTRY
    rng = np.random.default_rng(seed)
    draw = rng.random(len(ev)) < share
    for k in flagged_batches:
        a, b = int(cuts[k]), int(cuts[k + 1])
        m[a:b] = draw[a:b]
        for _, idx in runs_for(ev, a, b, n_res, n_hot, tile):
            if idx is not None:
                m[a + idx] = True
    return m & ent


def longest_run(ev, a, b, res, mask):
    """The longest run of consecutive flagged ENTRYs of res in the batch [a, b), as the positions of its segment it
    covers (first to last ENTRY of the run; the EXITs and TRACEs between them lie inside it), and whether the longest
    run spans a 500 ms bucket edge."""
    idx = a + np.nonzero(ev["res_id"][a:b] == res)[0]
    ent = np.nonzero(ev["kind"][idx] == ENTRY)[0]  # segment positions of the ENTRYs
    f = mask[idx[ent]]
    best, spans, k = 0, False, 0
    while k < len(f):
        if not f[k]:
            k += 1
            continue
        j = k
        while j + 1 < len(f) and f[j + 1]:
            j += 1
        length = int(ent[j] - ent[k] + 1)
        if length > best:
            best = length
            spans = bool(ev["ts"][idx[ent[k]]] // 500 != ev["ts"][idx[ent[j]]] // 500)
        k = j + 1
    return best, spans


class Ref(U.Ref):
    pass


def reference(name, mix, batches=3, flagged=(0, 1)):
    """The counts_util trace `name` with the counts of `mix`, pre-blocked ENTRYs in the batches `flagged`, replayed
    through the oracle (once per process)."""
    return _reference(name, mix, batches, tuple(flagged))


@functools.lru_cache(maxsize=None)
def _reference(name, mix, batches, flagged):
    w = workload(name)
    choices, p = U.MIXES[mix]
    r = Ref()
    r.w = w
    r.cuts = U.cuts_of(len(w.events), batches)
    r.ev = U.with_counts(w.events, choices, p, U.COUNT_SEED, zero_in=r.cuts if mix == "ZERO" else None)
    r.mask = flag(r.ev, r.cuts, w.n_res, flagged)
    r.ev["flags"][r.mask] |= A.F_BLOCKED_UPSTREAM
    r.ev.setflags(write=False)
    orc = O.Oracle(max_slot_chain_size=0)
    w.install(orc)
    r.do = np.concatenate([orc.submit(r.ev[a:b]) for a, b in zip(r.cuts[:-1], r.cuts[1:])])
    # every resource with a long segment (the cooperative owners' under SG_LANE_MAX=0 and the default bins alike: the
    # hottest 50) plus a random sample
    r.sample = U.sample(r.ev, w.n_res)
    r.nodes = {int(x): orc.read_node(int(x)) for x in r.sample}
    r.threads = []
    orc.close()
    return r


def marked_segments(ref, upto, lane_max, eligible=None):
    """Segments of batch `upto` whose resource has seen a pre-blocked ENTRY in a batch <= upto (the mark is sticky) and
    that hold more than lane_max events, as {resource: length}; eligible: only these resources."""
    ev, cuts = ref.ev, ref.cuts
    seen = np.unique(ev["res_id"][:cuts[upto + 1]][ref.mask[:cuts[upto + 1]]])
    cnt = np.bincount(ev["res_id"][cuts[upto]:cuts[upto + 1]], minlength=ref.w.n_res)
    return {int(r): int(cnt[r]) for r in seen if cnt[r] > lane_max and (eligible is None or int(r) in eligible)}


def named_preblocked(ev, do, cuts, mask):
    """(same batch, earlier batch): EXITs / TRACEs whose reference names a pre-blocked ENTRY (one the oracle answered
    with status 6)."""
    ref = (ev["aux"] & REF_NONE).astype(np.int64)
    i = np.nonzero((ev["kind"] != ENTRY) & (ref != A.REF_NONE) & (ref < len(ev)))[0]
    i = i[mask[ref[i]] & ((do[ref[i]] & 0xFF) == A.BLOCK_UPSTREAM)]
    batch_of = np.searchsorted(cuts, i, side="right")
    same = batch_of == np.searchsorted(cuts, ref[i], side="right")
    return int(same.sum()), int((~same).sum())


def zero_between_flow_blocks(ev, do, mask, stop=None):
    """Flagged zero-count ENTRYs whose resource has a BLOCK_FLOW word before and after them inside their 500 ms
    bucket (counting ends at `stop`)."""
    st = do & 0xFF
    n = 0
    for i in np.nonzero(mask & (ev["count"] == 0))[0]:
        same = np.nonzero((ev["res_id"] == ev["res_id"][i]) & (ev["ts"] // 500 == ev["ts"][i] // 500) &
                          (st == A.BLOCK_FLOW))[0]
        n += bool(len(same) and same[0] < i < same[-1])
        if stop is not None and n >= stop:
            break
    return n


# ---------------------------------------------------------------- authority rules (sg_submit_ex)
N_ORIGINS, N_CONTEXTS = 16, 4
EXT_SEED = 31
ORIGIN_RULE_RES = 2  # rank (by events) of the resource that gets a flow rule on an origin: it must stay on a lane


def authority_tuples(names, hot):
    """WHITE and BLACK lists on the hot resources: a BLACK list of three origins, a WHITE list that lets most through,
    a one-name BLACK list, a WHITE list of one name (blocks nearly every origin)."""
    kinds = [("app-1,app-2,app-3", A.AUTHORITY_BLACK),
             (",".join("app-%d" % k for k in range(2, N_ORIGINS)), A.AUTHORITY_WHITE),
             ("app-5", A.AUTHORITY_BLACK), ("app-0", A.AUTHORITY_WHITE)]
    return [(names[int(r)],) + kinds[k % len(kinds)] for k, r in enumerate(hot)]


@functools.lru_cache(maxsize=None)
def authority_reference(name="c4", mix="MIXED", batches=3, n_hot=12):
    """The trace through sg_submit_ex with origins and contexts, authority rules on the n_hot hottest resources, the
    caller's flag on a ~3 % share besides, and one PX_ORIGIN flow rule on a hot resource."""
    w = workload(name)
    choices, p = U.MIXES[mix]
    r = Ref()
    r.w = w
    r.cuts = U.cuts_of(len(w.events), batches)
    r.ev = U.with_counts(w.events, choices, p, U.COUNT_SEED)
    n = len(r.ev)
    names = w.names()
    cnt = np.bincount(r.ev["res_id"], minlength=w.n_res)
    r.hot = [int(x) for x in np.argsort(-cnt, kind="stable")[:n_hot]]
    r.tuples = authority_tuples(names, r.hot)
    r.origin_res = r.hot[ORIGIN_RULE_RES]
    r.origin_rule = A.flow_rule(names[r.origin_res], 50.0, limit_app="app-4")
    orc = O.Oracle(max_slot_chain_size=0)
    w.install(orc)
    io, ic = w.intern_names(orc, N_ORIGINS, N_CONTEXTS)
    r.io, r.ic = io, ic
    r.ext = T.ext_for(r.ev, io, ic, seed=EXT_SEED)
    ent = r.ev["kind"] == ENTRY
    r.caller = ent & (np.random.default_rng(FLAG_SEED + 1).random(n) < 0.03)
    r.ev["flags"][r.caller] |= A.F_BLOCKED_UPSTREAM
    kept = kept_rules(r.tuples)
    name_of = {int(i): "app-%d" % k for k, i in enumerate(io)}
    res_of = {names[x]: x for x in r.hot}
    r.blk = np.zeros(n, dtype=bool)
    for res_name, (la, st) in kept.items():
        bad = np.array([int(i) for i in io if blocks(kept, res_name, name_of[int(i)])], dtype=np.uint32)
        r.blk |= ent & (r.ev["res_id"] == res_of[res_name]) & np.isin(r.ext["origin_id"], bad)
    ev_o = r.ev.copy()
    ev_o["flags"][r.blk] |= A.F_BLOCKED_UPSTREAM
    r.mask = r.blk | r.caller
    r.ev.setflags(write=False)
    r.extra_flow = [r.origin_rule]
    load_extra_flow(orc, w, r.extra_flow)
    r.do = np.concatenate([orc.submit_ex(ev_o[a:b], r.ext[a:b]) for a, b in zip(r.cuts[:-1], r.cuts[1:])])
    st = r.do & 0xFF
    r.want = r.do.copy()
    r.want[r.blk & ~r.caller & (st == A.BLOCK_UPSTREAM)] = A.BLOCK_AUTHORITY
    r.sample = U.sample(r.ev, w.n_res)
    r.nodes = {int(x): orc.read_node(int(x)) for x in r.sample}
    r.origin_nodes = {(x, k): orc.read_origin_node(x, "app-%d" % k) for x in r.hot for k in range(N_ORIGINS)}
    r.context_nodes = {(x, k): orc.read_default_node(x, "ctx-%d" % k) for x in r.hot for k in range(N_CONTEXTS)}
    orc.close()
    return r


def load_extra_flow(x, w, extra):
    """The workload's flow rules again with `extra` appended (load_flow_rules replaces the whole list)."""
    import ctypes as C
    ptr, n = w.flow
    old = (A.SgFlowRule * n).from_address(ptr)
    x.load_flow_rules(list(old) + list(extra))


# ---------------------------------------------------------------- the mix trace (tests/test_gpu_mix.py's rule shape)
MIX_NAMES = ("x0", "x1", "x2", "x3", "x4", "x5")


def mix_rules(flow_count=1e5):
    import test_gpu_mix as M
    return M._mix_rules(flow_count)


@functools.lru_cache(maxsize=None)
def mix_reference(n_batches=3, n_entries=40_000, flow_count=1e5):
    """test_gpu_mix._synthetic batches (x0 a long segment, params on args[0]) with ~10 % of the ENTRYs and one long
    run on x0 flagged; the oracle's words, nodes and thread-count maps."""
    import test_gpu_mix as M
    r = Ref()
    orc = O.Oracle(max_slot_chain_size=0)
    for nm in MIX_NAMES:
        orc.register(nm)
    f, d, p = M._mix_rules(flow_count)
    orc.load_flow_rules(f)
    orc.load_degrade_rules(d)
    orc.load_param_rules(p)
    r.rules = (f, d, p)
    # the generator ends every call with the EXITs still pending, so its calls are laid end to end (global
    # references) and cut again elsewhere: EXITs then name ENTRYs of the batch before
    parts, t, gbase = [], M.T0, 0
    for b in range(n_batches):
        parts.append(M._synthetic(400 + b, n_entries, gbase, len(MIX_NAMES), t=t))
        gbase += len(parts[-1])
        t = int(parts[-1]["ts"].max()) + 1
    allev = np.concatenate(parts)
    cuts = np.linspace(0, len(allev), n_batches + 1).astype(np.int64) + np.array([0] + [1500] * (n_batches - 1) + [0])
    m = flag(allev, cuts, len(MIX_NAMES), range(n_batches - 1), n_hot=1)
    allev["flags"][m] |= A.F_BLOCKED_UPSTREAM
    r.batches = [allev[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    r.masks = [m[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    r.do = [orc.submit(ev) for ev in r.batches]
    r.nodes = [orc.read_node(k) for k in range(len(MIX_NAMES))]
    r.thread_keys = {}
    r.threads = {}
    for res in (0, 1, 2):
        m = (allev["res_id"] == res) & (allev["kind"] == ENTRY) & ((allev["flags"] & A.F_HAS_ARG) != 0)
        keys = np.unique(allev["aux"][m])[:800]
        r.thread_keys[res] = keys
        r.threads[res] = [orc.param_thread_count(res, 0, int(k)) for k in keys]
    orc.close()
    return r
