"""Traces for the embedded token server and their expected results, built from the unchanged oracle (helper of
test_gpu_embedded.py / test_embedded_host.py).

With sg_cluster_embedded on, an ENTRY that reaches FlowSlot on a resource whose only flow rule is a cluster rule asks
the engine's own token server (FlowRuleChecker.passClusterCheck, FlowRuleChecker.java:126-187).  The oracle has no such
mode: it decides a cluster rule as a process without a TokenService does, and serves tokens through
cluster_request_array.  The expected result is put together from the two, in the steps of the issue:

  W0    the trace through an oracle with the rules as loaded.  ENTRYs with status 5, 6 or 7 make no request
        (authority rules by flag emulation, tests/test_gpu_authority.py: the oracle gets SG_F_BLOCKED_UPSTREAM on the
        entries test_authority_host.blocks() rejects).
  reqs  the other ENTRYs of the eligible resources, batch by batch, through token oracles -- one per namespace, as
        NsOracles in tests/test_gpu_cluster_ns.py -- in event order; external calls between batches go to the same
        oracles.
  D     a second oracle replaying the trace with SG_F_BLOCKED_UPSTREAM added to the BLOCKED ENTRYs: it counts that
        block exactly as a FlowException (do_entry, sentinel_oracle.c:1821-1854).
  want  SG_BLOCK_FLOW | slot << 8 where the flag was added; D's word with the wait ORed in where the answer was
        SHOULD_WAIT and D passed; SG_BLOCK_AUTHORITY where D says 6 for an authority-emulated flag; D's word otherwise.

Compared on the device: all 32 bits of every word, read_node of every resource, and the token state by one more
external request per flowId on both sides.
"""
import ctypes as C
import functools

import numpy as np

import pyoracle as O
from sentinel_amd import _abi as A
from sentinel_amd import tracegen as T

ENTRY = A.EV_ENTRY
NO_REQUEST = (A.NO_CHECK, A.BLOCK_UPSTREAM, 7)  # statuses of W0 whose ENTRY never reaches FlowSlot
BLOCK_AUTHORITY = 7
STATUSES = {"ok": A.TOKEN_OK, "blocked": A.TOKEN_BLOCKED, "should_wait": A.TOKEN_SHOULD_WAIT,
            "too_many_request": A.TOKEN_TOO_MANY_REQUEST, "bad_request": A.TOKEN_BAD_REQUEST,
            "fail": A.TOKEN_FAIL, "no_rule_exists": A.TOKEN_NO_RULE_EXISTS}
T0 = 1_700_000_000_000


def cluster_rule(name, fid, count, **kw):
    kw.setdefault("cluster_threshold_type", A.CLUSTER_THRESHOLD_GLOBAL)
    kw.setdefault("cluster_fallback_to_local", False)
    return A.flow_rule(name, count, cluster_mode=True, cluster_flow_id=fid, **kw)


class TokenOracles:
    """One oracle a namespace (an oracle is one namespace with one GlobalRequestLimiter).  limits: {namespace:
    limit} in order, the first takes the requests no namespace claims; flow_ns: {flowId: namespace}."""

    def __init__(self, limits, flow_ns, names, rules):
        self.names = list(limits)
        self.flow_ns = dict(flow_ns)
        self.orc = {}
        for ns, lim in limits.items():
            o = O.Oracle(cluster_max_allowed_qps=int(lim))
            for nm in names:
                o.register(nm)
            o.load_flow_rules([r for r in rules if r.cluster_mode and
                               self.flow_ns.get(int(r.cluster_flow_id), self.names[0]) == ns])
            self.orc[ns] = o

    def set_connected(self, fid, n):
        self.orc[self.flow_ns.get(fid, self.names[0])].cluster_set_connected(fid, n)

    def request_array(self, reqs):
        reqs = np.ascontiguousarray(reqs, dtype=A.TOKEN_REQ_DTYPE)
        out = np.zeros(len(reqs), dtype=A.TOKEN_RES_DTYPE)
        pos = {ns: k for k, ns in enumerate(self.names)}
        lut = {f: pos[ns] for f, ns in self.flow_ns.items()}
        k = np.array([lut.get(int(f), 0) for f in reqs["flow_id"]], dtype=np.int64)
        k[reqs["acquire_count"] <= 0] = 0
        for j, ns in enumerate(self.names):
            sel = np.nonzero(k == j)[0]
            if len(sel):
                out[sel] = self.orc[ns].cluster_request_array(reqs[sel])
        return out

    def close(self):
        for o in self.orc.values():
            o.close()


class Case:
    """What a test needs of one trace: the inputs for the engine and the expected results."""


def token_reqs(ev, fid_of_res):
    """The sg_token_req records of the ENTRYs `ev` (already selected), in order."""
    r = np.zeros(len(ev), dtype=A.TOKEN_REQ_DTYPE)
    r["ts"] = ev["ts"]
    r["flow_id"] = fid_of_res[ev["res_id"]]
    r["acquire_count"] = ev["count"]
    r["prioritized"] = (ev["flags"] & A.F_PRIORITIZED) != 0
    return r


def limiter_qps(reqs, ans, now):
    """RequestLimiter.getQps at `now` (UnaryLeapArray(10, 1000), csrv/flow/statistic/limit/RequestLimiter.java): the
    requests that passed the limiter -- every answer the flow gave -- in the buckets still valid at `now`."""
    passed = np.isin(ans["status"], (A.TOKEN_OK, A.TOKEN_BLOCKED, A.TOKEN_SHOULD_WAIT))
    ws = reqs["ts"] - reqs["ts"] % 100
    return float((passed & (ws > now - now % 100 - 1000) & (ws <= now)).sum())


def expect(case, oracle_cfg=None, d_fallback_mask=None):
    """Fill in the expected side of `case` (see the module docstring).  case needs: names, flow_rules, degrade_rules,
    ev, cuts, eligible {res: flowId}; optional: ext, auth_blk (mask of the authority-emulated flags), limits, flow_ns,
    connected {flowId: n}, external {batch index: [reqs before that batch]}, n_origins / n_contexts (names to intern),
    first_on (the batch before which the mode is switched on; default 0)."""
    cfg = dict(max_slot_chain_size=0)
    cfg.update(oracle_cfg or {})
    ev, cuts = case.ev, case.cuts
    n = len(ev)
    ext = getattr(case, "ext", None)
    auth_blk = getattr(case, "auth_blk", np.zeros(n, dtype=bool))
    limits = getattr(case, "limits", {"default": 30000})
    flow_ns = getattr(case, "flow_ns", {})
    external = getattr(case, "external", {})
    nres = len(case.names)
    fid_of_res = np.zeros(nres, dtype=np.int64)
    for r, f in case.eligible.items():
        fid_of_res[r] = f
    is_elig = np.zeros(nres, dtype=bool)
    is_elig[list(case.eligible)] = True

    def oracle():
        o = O.Oracle(**cfg)
        for nm in case.names:
            o.register(nm)
        for k in range(getattr(case, "n_contexts", 0)):
            o.intern_context("filler%d" % k)
        for k in range(getattr(case, "n_origins", 0)):
            o.intern_origin("app-%d" % k)
        o.load_flow_rules(case.flow_rules)
        if case.degrade_rules:
            o.load_degrade_rules(case.degrade_rules)
        return o

    def replay(o, e):
        out = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            out.append(o.submit(e[a:b]) if ext is None else o.submit_ex(e[a:b], ext[a:b]))
        return np.concatenate(out)

    ev_o = ev.copy()
    ev_o["flags"][auth_blk] |= A.F_BLOCKED_UPSTREAM
    o = oracle()
    case.w0 = replay(o, ev_o)
    o.close()
    ent = ev["kind"] == ENTRY
    case.req_mask = ent & is_elig[ev["res_id"]] & ~np.isin(case.w0 & 0xFF, NO_REQUEST)
    case.req_mask[:cuts[getattr(case, "first_on", 0)]] = False  # (toggling: the mode is switched on before this batch)
    tok = TokenOracles(limits, flow_ns, case.names, case.flow_rules)
    for f, c in getattr(case, "connected", {}).items():
        tok.set_connected(f, c)
    case.reqs, case.answers, case.ext_answers = [], [], {}
    status = np.full(n, 99, dtype=np.int32)
    wait = np.zeros(n, dtype=np.int64)
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        if k in external:
            case.ext_answers[k] = tok.request_array(external[k])
        idx = a + np.nonzero(case.req_mask[a:b])[0]
        rq = token_reqs(ev[idx], fid_of_res)
        an = tok.request_array(rq) if len(rq) else np.zeros(0, dtype=A.TOKEN_RES_DTYPE)
        case.reqs.append(rq)
        case.answers.append(an)
        status[idx] = an["status"]
        wait[idx] = an["wait_in_ms"]
    case.status = status
    blocked = status == A.TOKEN_BLOCKED
    # Part B's reference, (iii): refused ENTRYs the local rule blocks are flagged in D as well
    if d_fallback_mask is not None:
        blocked = blocked | d_fallback_mask(case)
    ev_d = ev_o.copy()
    ev_d["flags"][blocked] |= A.F_BLOCKED_UPSTREAM
    o = oracle()
    case.d = replay(o, ev_d)
    want = case.d.copy()
    st = case.d & 0xFF
    want[auth_blk & ((ev["flags"] & A.F_BLOCKED_UPSTREAM) == 0) & (st == A.BLOCK_UPSTREAM)] = BLOCK_AUTHORITY
    want[blocked] = A.BLOCK_FLOW | (0 << 8)  # the cluster rule is its resource's only flow rule: slot 0
    sw = (status == A.TOKEN_SHOULD_WAIT) & (st == A.PASS)
    want[sw] |= (np.minimum(wait[sw], 0xFFFF).astype(np.uint32) << np.uint32(16))
    case.want = want
    case.blocked = blocked
    case.nodes = [o.read_node(r) for r in range(nres)]
    o.close()
    # the token state: one more request per flowId after the trace
    t_end = int(ev["ts"][-1]) + 7
    case.probe = np.zeros(len(case.eligible), dtype=A.TOKEN_REQ_DTYPE)
    for i, f in enumerate(sorted(case.eligible.values())):
        case.probe[i] = (t_end, f, 1, 0)
    case.probe_answers = tok.request_array(case.probe)
    case.ns_qps = {}
    allr = np.concatenate(case.reqs + [case.probe] + [external[k] for k in sorted(external)])
    alla = np.concatenate(case.answers + [case.probe_answers] + [case.ext_answers[k] for k in sorted(external)])
    pos = {ns: k for k, ns in enumerate(tok.names)}
    nsk = np.array([pos[flow_ns.get(int(f), tok.names[0])] for f in allr["flow_id"]], dtype=np.int64)
    for ns in tok.names:
        m = nsk == pos[ns]
        case.ns_qps[ns] = limiter_qps(allr[m], alla[m], t_end)
    tok.close()
    return case


def answer_counts(an):
    return {k: int((an["status"] == v).sum()) for k, v in STATUSES.items()}


def shares(case):
    """Per batch with requests: (requests, OK share, BLOCKED share)."""
    out = []
    for an in case.answers:
        if len(an):
            out.append((len(an), float((an["status"] == A.TOKEN_OK).mean()), float((an["status"] == A.TOKEN_BLOCKED).mean())))
    return out


def workload_rules(w, cluster):
    """The workload's flow rules with those of the resources in `cluster` ({name: rule}) replaced."""
    ptr, n = w.flow
    old = (A.SgFlowRule * n).from_address(ptr)
    return [r for r in old if r.resource.decode() not in cluster] + list(cluster.values())


def struct_list(w, kind, struct):
    ptr, n = getattr(w, kind)
    return list((struct * n).from_address(ptr)) if n else []


# ---------------------------------------------------------------- the owners' trace
# A 64-resource C4 workload, ~57,000 events over ~3.1 s.  Eligible: eight resources by rank of their ENTRY count, with
# GLOBAL thresholds between 5 and 50 a second chosen so that about a sixth of the requests get a token -- rank 1
# (~1,100 entries a second against 50: a segment of more than 2,000 events a batch, the 1,024-lane owner's under the
# J16 owner set) down to rank 60 (~24 a second against 5).  Every C4 resource has a breaker: RT, exception ratio or
# exception count by resource id modulo 3.
OWNER_RANKS = (1, 8, 12, 16, 20, 30, 45, 60)
OWNER_THRESHOLDS = (50, 50, 40, 30, 30, 20, 10, 5)
FID0 = 9000


@functools.lru_cache(maxsize=None)
def owners_workload():
    return T.Workload(4, n_entries=28_000, n_res=64, rate=9300.0)


def _owners_base(batches=3):
    w = owners_workload()
    c = Case()
    c.w = w
    c.names = w.names()
    c.ev = w.events.copy()
    c.cuts = np.linspace(0, len(c.ev), batches + 1).astype(np.int64)
    cnt = np.bincount(c.ev["res_id"][c.ev["kind"] == ENTRY], minlength=w.n_res)
    rank = np.argsort(-cnt, kind="stable")
    c.eligible = {int(rank[k]): FID0 + i for i, k in enumerate(OWNER_RANKS)}
    c.thresholds = {int(rank[k]): t for k, t in zip(OWNER_RANKS, OWNER_THRESHOLDS)}
    c.flow_rules = workload_rules(w, {c.names[r]: cluster_rule(c.names[r], f, c.thresholds[r])
                                      for r, f in c.eligible.items()})
    c.degrade_rules = struct_list(w, "degrade", A.SgDegradeRule)
    return c


@functools.lru_cache(maxsize=None)
def owners_case():
    return expect(_owners_base())


@functools.lru_cache(maxsize=None)
def zero_case():
    """The owners' trace with ~5 % of the eligible ENTRYs acquiring 0: BAD_REQUEST before the limiter, the entry
    passes FlowSlot."""
    c = _owners_base()
    rng = np.random.default_rng(41)
    m = (c.ev["kind"] == ENTRY) & np.isin(c.ev["res_id"], list(c.eligible)) & (rng.random(len(c.ev)) < 0.05)
    c.ev["count"][m] = 0
    c.zero = m
    return expect(c)


@functools.lru_cache(maxsize=None)
def avg_local_case():
    """AVG_LOCAL thresholds with three connected clients: the thresholds a third, the same token budget."""
    c = _owners_base()
    c.flow_rules = workload_rules(c.w, {c.names[r]: cluster_rule(c.names[r], f, c.thresholds[r] / 3.0,
                                                                 cluster_threshold_type=A.CLUSTER_THRESHOLD_AVG_LOCAL)
                                        for r, f in c.eligible.items()})
    c.connected = {f: 3 for f in c.eligible.values()}
    return expect(c)


@functools.lru_cache(maxsize=None)
def interleaved_case():
    """External token requests for the same flowIds between the batches (and before the first)."""
    c = _owners_base()
    c.external = {}
    fids = sorted(c.eligible.values())
    for k in range(3):
        t = int(c.ev["ts"][c.cuts[k]]) - (1 if k else 50)
        t = max(t, int(c.ev["ts"][c.cuts[k] - 1]) if k else t)
        rq = np.zeros(3 * len(fids), dtype=A.TOKEN_REQ_DTYPE)
        for i, f in enumerate(fids * 3):
            rq[i] = (t, f, 1 + (i % 3), 0)
        c.external[k] = rq
    return expect(c)


@functools.lru_cache(maxsize=None)
def limiter_case():
    """Two namespaces whose limiters (900 and 250 requests a second against ~1,350 and ~380) refuse requests in the
    middle of every batch;
    rules without fallback, so a refused ENTRY passes FlowSlot."""
    c = _owners_base()
    fids = sorted(c.eligible.values())
    c.limits = {"ns-a": 900, "ns-b": 250}
    c.flow_ns = {f: ("ns-a" if i % 2 == 0 else "ns-b") for i, f in enumerate(fids)}
    return expect(c)


@functools.lru_cache(maxsize=None)
def prio_case():
    """A tenth of the eligible ENTRYs prioritized: the token server lets them borrow from the next window
    (SHOULD_WAIT with a wait) until the occupy ratio is used up."""
    c = _owners_base()
    rng = np.random.default_rng(43)
    m = (c.ev["kind"] == ENTRY) & np.isin(c.ev["res_id"], list(c.eligible)) & (rng.random(len(c.ev)) < 0.10)
    c.ev["flags"][m] |= A.F_PRIORITIZED
    c.prio = m
    return expect(c)


# ---------------------------------------------------------------- one long segment
@functools.lru_cache(maxsize=None)
def long_case(n_entries=40_000):
    """About 80,000 events on one eligible resource with an RT breaker, over 1.2 s in two batches:
    threshold 8,000 a second, so a sampling window's tokens are gone early in every 100 ms and long runs of BLOCKED
    ENTRYs lie inside the owner's frozen stretches; the breaker (avg RT 20 > 10) cuts in the second second."""
    rng = np.random.default_rng(47)
    n = n_entries
    te = T0 + np.sort(rng.integers(0, 1200, n))
    rt = rng.integers(5, 36, n)
    ts = np.concatenate([te, te + rt])
    kind = np.concatenate([np.zeros(n, dtype=np.int64), np.full(n, A.EV_EXIT, dtype=np.int64)])
    order = np.lexsort((kind, ts))
    pos = np.empty(2 * n, dtype=np.int64)
    pos[order] = np.arange(2 * n)
    ev = np.zeros(2 * n, dtype=A.EVENT_DTYPE)
    ev["ts"] = ts[order]
    ev["count"] = 1
    ev["kind"] = kind[order]
    aux = np.zeros(2 * n, dtype=np.uint64)
    aux[pos[n:]] = (rt.astype(np.uint64) << np.uint64(48)) | pos[:n].astype(np.uint64)
    ev["aux"] = aux
    c = Case()
    c.names = ["long"]
    c.ev = ev
    c.cuts = np.array([0, (2 * n * 3) // 5, 2 * n], dtype=np.int64)
    c.eligible = {0: FID0}
    c.flow_rules = [cluster_rule("long", FID0, 8000)]
    c.degrade_rules = [A.degrade_rule("long", 10, 1, grade=A.DEGRADE_GRADE_RT)]
    return expect(c)


# ---------------------------------------------------------------- requests not made
N_ORIGINS = 4


@functools.lru_cache(maxsize=None)
def not_made_case(variant):
    """The owners' trace through sg_submit_ex with what keeps an ENTRY from FlowSlot: "flags" -- the caller's
    SG_F_BLOCKED_UPSTREAM on a tenth of the eligible ENTRYs and a BLACK authority list on two eligible resources;
    "chain" -- max_slot_chain_size 40 of 64 resources; "nullctx" -- a tenth of the eligible ENTRYs (with their EXITs
    and TRACEs) in a NullContext; "off" -- Constants.ON false."""
    c = _owners_base()
    n = len(c.ev)
    ent = c.ev["kind"] == ENTRY
    elig = np.isin(c.ev["res_id"], list(c.eligible))
    rng = np.random.default_rng(53)
    c.ext = np.zeros(n, dtype=A.EXT_DTYPE)
    c.oracle_cfg = {}
    if variant == "flags":
        c.n_origins = N_ORIGINS
        ref = (c.ev["aux"] & np.uint64(A.REF_NONE)).astype(np.int64)
        isref = ~ent & (ref != A.REF_NONE) & (ref < n)
        src = np.where(isref, ref, np.arange(n))
        c.ext["origin_id"] = (1 + rng.integers(0, N_ORIGINS, n))[src]  # ids 1..N_ORIGINS: "app-0".. in intern order
        black = sorted(c.eligible)[:2]
        c.auth_tuples = [(c.names[r], "app-1,app-2", A.AUTHORITY_BLACK) for r in black]
        c.auth_blk = ent & np.isin(c.ev["res_id"], black) & np.isin(c.ext["origin_id"], (2, 3))
        c.ev["flags"][ent & elig & (rng.random(n) < 0.10)] |= A.F_BLOCKED_UPSTREAM
    elif variant == "chain":
        c.oracle_cfg = {"max_slot_chain_size": 40}
    elif variant == "nullctx":
        c.n_contexts = A.MAX_CONTEXTS + 1
        ref = (c.ev["aux"] & np.uint64(A.REF_NONE)).astype(np.int64)
        isref = ~ent & (ref != A.REF_NONE) & (ref < n)
        src = np.where(isref, ref, np.arange(n))
        pick = (elig & (rng.random(n) < 0.10))[src] & elig
        c.ext["context_id"][pick] = A.MAX_CONTEXTS + 1
        c.nullctx = pick
    elif variant == "off":
        c.oracle_cfg = {"switch_on": 0}
    else:
        raise ValueError(variant)
    return expect(c, c.oracle_cfg)


@functools.lru_cache(maxsize=None)
def toggled_case():
    """The owners' trace with the mode switched on between the first and the second batch."""
    c = _owners_base()
    c.first_on = 1
    return expect(c)


SMALL_START, SMALL_SIZE, SMALL_BATCHES = 6000, 250, 9


@functools.lru_cache(maxsize=None)
def small_case():
    """The first third of the owners' trace as one batch of 6,000 events, nine synchronous batches of 250 events (at
    most 256: the size the one-workgroup k_tiny path takes when no eligible rule is loaded) and the rest; EXITs of the
    small batches name ENTRYs of the batches before.  A 250-event batch spans ~13 ms, less than a 100 ms sampling
    window, so with the owners' thresholds some of them would hold no OK at all: here the hottest eligible resource
    keeps 50 a second (mostly BLOCKED) and the next four get 5,000 (always OK), so every batch holds both answers."""
    c = _owners_base()
    end = int(c.cuts[1])
    c.ev = c.ev[:end].copy()
    el = list(c.eligible)
    c.thresholds = dict(c.thresholds)
    for r in el[1:5]:
        c.thresholds[r] = 5000
    c.flow_rules = workload_rules(c.w, {c.names[r]: cluster_rule(c.names[r], f, c.thresholds[r])
                                        for r, f in c.eligible.items()})
    c.cuts = np.array([0] + [SMALL_START + k * SMALL_SIZE for k in range(SMALL_BATCHES + 1)] + [end], dtype=np.int64)
    return expect(c)
