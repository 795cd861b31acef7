"""The reference for the token server's cluster metrics (helper of test_cluster_metrics_host.py and
test_gpu_cluster_metrics.py).

The oracle decides token requests and has no metric read, so the expected rows come from a sequential model of
ClusterMetricLeapArray (csrv/flow/statistic/metric/ClusterMetricLeapArray.java:35-91) and ClusterParameterLeapArray
(ClusterParameterLeapArray.java:30-58), driven by the request stream and the *oracle's* results (never the device's):

    FLOW   OK           currentWindow(ts); PASS += count, PASS_REQUEST += 1
           BLOCKED      currentWindow(ts); BLOCK += count
           SHOULD_WAIT  currentWindow(ts); occupyCounter[PASS] += count, occupyCounter[PASS_REQUEST] += 1, hasOccupied:
                        the next reset of an existing bucket starts from PASS = PASS_REQUEST = the counters
           other        nothing (the request never reached the flow's metric)
    PARAM  OK           per listed value: currentWindow(ts), then addValue to the current bucket (a duplicate twice)
           BLOCKED      currentWindow(ts) (ClusterParamMetric.getSum calls it before it reads)

While it is fed, the model re-derives the verdict of every non-prioritized FLOW request and of every PARAM request from
its own windows (ClusterFlowChecker.java:67-80, ClusterParamFlowChecker.java:60-84) and counts the ones that differ from
the oracle's: test_cluster_metrics_host.py requires zero on the streams the GPU tests use.

read() is the read-back rule of sg_cluster_metrics: with w = interval / n, i = (now / w) % n and ws = now - now % w,
bucket i counts as empty if its start is < ws (a FLOW bucket that exists is reset to the pending occupy transfer), a
bucket never created or with a start >= ws is taken as it is, then every bucket with now - start > interval is left
out; a param flow's values are ordered by (sum descending, key ascending) and the first `top` with a sum > 0 listed.
"""
import numpy as np

from sentinel_amd import _abi as A

OK, BLOCKED, WAIT = A.TOKEN_OK, A.TOKEN_BLOCKED, A.TOKEN_SHOULD_WAIT
GLOBAL = A.CLUSTER_THRESHOLD_GLOBAL


def d2i(x):
    """Java's (int) of a double."""
    if x != x:
        return 0
    if x >= 2147483647.0:
        return 2147483647
    if x <= -2147483648.0:
        return -2147483648
    return int(x)


class FlowMetric:
    """ClusterMetric of one cluster flow rule."""

    def __init__(self, n=10, interval=1000, count=0.0, thr_type=GLOBAL, connected=0, exceed=1.0):
        self.n, self.interval, self.count, self.thr_type, self.connected, self.exceed = n, interval, count, thr_type, \
            connected, exceed
        self.w = interval // n
        self.b = [None] * n  # {"ws", "pass", "block", "req"}
        self.occ_pass = self.occ_req = 0
        self.has_occ = False

    def current(self, now):
        i, ws = (now // self.w) % self.n, now - now % self.w
        old = self.b[i]
        if old is None:
            self.b[i] = {"ws": ws, "pass": 0, "block": 0, "req": 0}
            return self.b[i]
        if ws == old["ws"]:
            return old
        if ws > old["ws"]:
            old.update(ws=ws, block=0)
            old["pass"] = old["req"] = 0
            if self.has_occ:  # transferOccupyToBucket
                old["pass"], old["req"] = self.occ_pass, self.occ_req
                self.occ_pass = self.occ_req = 0
                self.has_occ = False
            return old
        return {"ws": ws, "pass": 0, "block": 0, "req": 0}  # a time before the slot's window: a detached bucket

    def valid(self, now):
        return [b for b in self.b if b is not None and not now - b["ws"] > self.interval]

    def threshold(self):
        return (self.count if self.thr_type == GLOBAL else self.count * float(self.connected)) * self.exceed

    def derive(self, now, acq):
        """(status, remaining) of a non-prioritized request at now, before it is counted."""
        self.current(now)
        nr = self.threshold() - sum(b["req"] for b in self.valid(now)) / (self.interval / 1000.0) - acq
        return (OK, d2i(nr)) if nr >= 0 else (BLOCKED, 0)

    def feed(self, now, acq, status):
        if status not in (OK, BLOCKED, WAIT):
            return
        cur = self.current(now)
        if status == OK:
            cur["pass"] += acq
            cur["req"] += 1
        elif status == BLOCKED:
            cur["block"] += acq
        else:
            self.occ_pass += acq
            self.occ_req += 1
            self.has_occ = True

    def read(self, now):
        """(pass sum, block sum) at now under the read-back rule; nothing changes."""
        i, ws = (now // self.w) % self.n, now - now % self.w
        sp = sb = 0
        for j, b in enumerate(self.b):
            if b is None:
                continue
            start, p, k = b["ws"], b["pass"], b["block"]
            if j == i and start < ws:
                start, p, k = ws, (self.occ_pass if self.has_occ else 0), 0
            if now - start > self.interval:
                continue
            sp += p
            sb += k
        return sp, sb


class ParamMetric:
    """ClusterParamMetric of one cluster param rule; hot: {key: count} of the parsed exclusive items."""

    def __init__(self, n=10, interval=1000, count=0.0, thr_type=GLOBAL, connected=0, hot=None):
        self.n, self.interval, self.count, self.thr_type, self.connected = n, interval, count, thr_type, connected
        self.hot = dict(hot or {})
        self.w = interval // n
        self.ws = [-1] * n
        self.m = [dict() for _ in range(n)]

    def current(self, now):
        i, ws = (now // self.w) % self.n, now - now % self.w
        if self.ws[i] < 0 or ws > self.ws[i]:
            self.ws[i] = ws
            self.m[i] = {}
        return i

    def total(self, now, key):
        return sum(self.m[j].get(key, 0) for j in range(self.n)
                   if self.ws[j] >= 0 and not now - self.ws[j] > self.interval)

    def derive(self, now, acq, values):
        """(status, remaining) of a request at now, before it is counted (remaining of a multi-value pass: -1)."""
        nr = -1.0
        for v in values:
            self.current(now)
            raw = float(self.hot[v]) if v in self.hot else self.count
            thr = raw if self.thr_type == GLOBAL else raw * float(self.connected)
            nr = thr - self.total(now, v) / (self.interval / 1000.0) - float(acq)
            if nr < 0:
                return BLOCKED, 0
        return OK, d2i(nr if len(values) == 1 else -1.0)

    def feed(self, now, acq, values, status):
        if status not in (OK, BLOCKED):
            return
        i = self.current(now)
        if status == OK:
            for v in values:
                self.m[i][v] = self.m[i].get(v, 0) + acq

    def read(self, now, top):
        """[(key, sum)] of the `top` hottest values at now under the read-back rule; nothing changes."""
        i, ws = (now // self.w) % self.n, now - now % self.w
        sums = {}
        for j in range(self.n):
            start = self.ws[j]
            if start < 0 or (j == i and start < ws) or now - start > self.interval:
                continue
            for k, c in self.m[j].items():
                sums[k] = sums.get(k, 0) + c
        order = sorted(((k, s) for k, s in sums.items() if s > 0), key=lambda x: (-x[1], x[0]))
        return order[:top]


class Model:
    """flows / pflows: {flowId: FlowMetric / ParamMetric}.  mismatches: derived verdicts that differ from the
    oracle's, as (kind, request index in its call, derived, oracle's); derived counts the verdicts derived."""

    def __init__(self, flows=None, pflows=None):
        self.flows, self.pflows = dict(flows or {}), dict(pflows or {})
        self.mismatches, self.derived = [], 0

    def feed_flow(self, reqs, res):
        for i in range(len(reqs)):
            q, o = reqs[i], res[i]
            m = self.flows.get(int(q["flow_id"]))
            st = int(o["status"])
            if m is None or st not in (OK, BLOCKED, WAIT):
                continue
            now, acq = int(q["ts"]), int(q["acquire_count"])
            if not q["prioritized"]:
                got = m.derive(now, acq)
                self.derived += 1
                if got != (st, int(o["remaining"])):
                    self.mismatches.append(("flow", i, got, (st, int(o["remaining"]))))
            m.feed(now, acq, st)

    def feed_param(self, reqs, vals, res):
        for i in range(len(reqs)):
            q, o = reqs[i], res[i]
            m = self.pflows.get(int(q["flow_id"]))
            st = int(o["status"])
            if m is None or st not in (OK, BLOCKED):
                continue
            now, acq = int(q["ts"]), int(q["acquire_count"])
            values = [int(v) for v in vals[int(q["value_off"]):int(q["value_off"]) + int(q["n_values"])]]
            got = m.derive(now, acq, values)
            self.derived += 1
            want = (st, int(o["remaining"]))
            if got[0] != want[0] or (len(values) == 1 and got[1] != want[1]):
                self.mismatches.append(("param", i, got, want))
            m.feed(now, acq, values, st)

    def read(self, now, top=5, only=None):
        """The expected rows: (kind, flowId, pass_qps, block_qps, [(key, qps)]), flow rules by flowId, then param
        rules by flowId; only: the flowIds to list (a namespace's), None: all."""
        rows = []
        for fid in sorted(self.flows):
            if only is not None and fid not in only:
                continue
            m = self.flows[fid]
            p, b = m.read(now)
            isec = m.interval / 1000.0
            rows.append((A.CM_FLOW, fid, p / isec, b / isec, []))
        for fid in sorted(self.pflows):
            if only is not None and fid not in only:
                continue
            m = self.pflows[fid]
            isec = m.interval / 1000.0
            rows.append((A.CM_PARAM, fid, 0.0, 0.0, [(k, s / isec) for k, s in m.read(now, top)]))
        return rows


def rows_of(got):
    """A.CLUSTER_METRIC_DTYPE rows in the shape Model.read returns (the unused top slots must be zero)."""
    out = []
    for r in got:
        k = int(r["n_top"])
        assert not r["top_key"][k:].any() and not r["top_qps"][k:].any() and r["rt"] == 0 and r["reserved"] == 0, r
        out.append((int(r["kind"]), int(r["flow_id"]), float(r["pass_qps"]), float(r["block_qps"]),
                    [(int(r["top_key"][j]), float(r["top_qps"][j])) for j in range(k)]))
    return out


def assert_rows(got, want, now, what=""):
    g = rows_of(got)
    assert len(g) == len(want), (what, len(g), len(want))
    for a, b in zip(g, want):
        assert a == b, (what, now, a, b)
    assert all(int(r["timestamp"]) == now for r in got), what


def flow_reqs(rows):
    """[(ts, flowId, acquire, prioritized)] -> A.TOKEN_REQ_DTYPE."""
    out = np.zeros(len(rows), dtype=A.TOKEN_REQ_DTYPE)
    for i, (ts, fid, acq, pr) in enumerate(rows):
        out[i] = (ts, fid, acq, int(pr))
    return out


# ---- scenarios: the streams of test_gpu_cluster_metrics.py, replayed against the oracle alone by
# test_cluster_metrics_host.py.  A scenario is a list of steps:
#   ("flow_rules", [spec])  ("param_rules", [spec])  ("connected", flowId, n)
#   ("flow", A.TOKEN_REQ_DTYPE rows)  ("param", A.PARAM_TOKEN_REQ_DTYPE rows, uint64 values)
#   ("read", now, top, namespace or None, flowIds of the namespace or None)
# spec: dict(fid, count, n, interval, thr, res) and for a param rule items = [(text, class, count)].
T0 = 1_700_000_000_000
BIG = 10_000_000  # cluster_max_allowed_qps: a namespace limit no stream here reaches


def fspec(fid, count, n=10, interval=1000, thr=GLOBAL, res="abc"):
    return dict(fid=fid, count=count, n=n, interval=interval, thr=thr, res=res)


def pspec(fid, count, n=10, interval=1000, thr=GLOBAL, res="abc", items=()):
    return dict(fid=fid, count=count, n=n, interval=interval, thr=thr, res=res, items=list(items))


def flow_rules(specs):
    return [A.flow_rule(s["res"], s["count"], cluster_mode=True, cluster_flow_id=s["fid"],
                        cluster_threshold_type=s["thr"], cluster_sample_count=s["n"],
                        cluster_window_interval_ms=s["interval"]) for s in specs]


def param_rules(specs):
    return [A.param_rule(s["res"], 0, s["count"], cluster_mode=True, cluster_flow_id=s["fid"],
                         cluster_threshold_type=s["thr"], items=s["items"], cluster_sample_count=s["n"],
                         cluster_window_interval_ms=s["interval"]) for s in specs]


def param_reqs(rows):
    """[(ts, flowId, acquire, [keys])] -> ("param", rows, values)."""
    arr, vals = A.param_token_arrays(rows)
    return ("param", arr, vals)


def oracle_param(orc, arr, vals):
    import pyoracle as O
    want = np.zeros(max(1, len(arr)), dtype=A.TOKEN_RES_DTYPE)
    v = np.ascontiguousarray(vals if len(vals) else np.zeros(1), dtype=np.uint64)
    assert O.lib().or_cluster_request_param_tokens(orc.h, arr.ctypes.data, len(arr), v.ctypes.data, len(vals),
                                                   want.ctypes.data) == 0
    return want[: len(arr)]


def _same(got, want, reqs, what):
    for f in ("status", "remaining", "wait_in_ms"):
        bad = np.flatnonzero(got[f] != want[f])
        assert not len(bad), (what, f, int(bad[0]), reqs[bad[0]], got[bad[0]], want[bad[0]], len(bad))


def run(steps, orc, eng=None, key_of=None):
    """Replay a scenario on the oracle (and the engine): every call's results must equal the oracle's, every read's
    rows the model's.  Returns (model, [(now, rows read from the engine)], the oracle's results call by call).
    key_of(text, class) -> key: how hot items are keyed (default: the pure key)."""
    import pyoracle as O
    key_of = key_of or O.param_key
    model, reads, results = Model(), [], []
    last_read = -1
    for k, step in enumerate(steps):
        kind = step[0]
        if kind == "flow_rules":
            for x in (orc, eng):
                if x is not None:
                    x.load_flow_rules(flow_rules(step[1]))
            old, model.flows = model.flows, {}
            for s in step[1]:  # the metric (and its window shape) of a flowId that stays is kept
                m = old.get(s["fid"]) or FlowMetric(s["n"], s["interval"])
                m.count, m.thr_type = float(s["count"]), s["thr"]
                model.flows[s["fid"]] = m
        elif kind == "param_rules":
            for x in (orc, eng):
                if x is not None:
                    x.load_param_rules(param_rules(step[1]))
            old, model.pflows = model.pflows, {}
            for s in step[1]:
                m = old.get(s["fid"]) or ParamMetric(s["n"], s["interval"])
                m.count, m.thr_type = float(s["count"]), s["thr"]
                m.hot = {key_of(t, c): n for t, c, n in s["items"]}
                model.pflows[s["fid"]] = m
        elif kind == "connected":
            for x in (orc, eng):
                if x is not None:
                    x.cluster_set_connected(step[1], step[2])
            for d in (model.flows, model.pflows):
                if step[1] in d:
                    d[step[1]].connected = step[2]
        elif kind == "flow":
            want = orc.cluster_request_array(step[1])
            model.feed_flow(step[1], want)
            results.append(want)
            if eng is not None:
                _same(eng.cluster_request_array(step[1]), want, step[1], "step %d (after read at step %d)" % (k, last_read))
        elif kind == "param":
            want = oracle_param(orc, step[1], step[2])
            model.feed_param(step[1], step[2], want)
            results.append(want)
            if eng is not None:
                _same(eng.cluster_request_param_array(step[1], step[2]), want, step[1],
                      "step %d (after read at step %d)" % (k, last_read))
        elif kind == "read":
            _, now, top, ns, only = step
            last_read = k
            if eng is not None:
                got = eng.cluster_metrics(now, ns=ns, top=top)
                assert_rows(got, model.read(now, top, only), now, "step %d" % k)
                reads.append((now, got))
        else:
            raise AssertionError(kind)
    assert steps[-1][0] in ("flow", "param"), "a scenario ends with traffic: the decisions after its last read are checked"
    return model, reads, results


SHAPES = [(10, 1000), (1, 1000), (16, 1600), (2, 500)]
# A valid cluster rule has windowIntervalMs % sampleCount == 0, so a bucket's start + interval falls into the bucket's
# own slot: at that instant the read-back's reset (bucket i with a start < ws) empties the bucket before
# isWindowDeprecated's strict > could keep it.  The reads at start + interval - 1, + 0 and + 1 pin exactly that.


def window_edges(shape):
    """One param flow (500) and one flow rule (7) of the shape, a param flow (501) of another: traffic over every
    bucket of one interval, reads at the window start, around a bucket's start + interval, earlier than the newest
    window and after an idle gap; then values that were hot one interval earlier must be gone."""
    n, interval = shape
    w = interval // n
    T = T0 - T0 % (interval * 2) + interval * 2
    other = (10, 1000) if shape != (10, 1000) else (5, 500)
    steps = [("flow_rules", [fspec(7, 12, n, interval)]),
             ("param_rules", [pspec(500, 5, n, interval), pspec(501, 6, *other)])]

    def traffic(t0, buckets, tag):
        fl, pa = [], []
        for b in buckets:
            for off in sorted({0, w // 2, w - 1}):
                ts = t0 + b * w + off
                fl += [(ts, 7, 1 + b % 3, False), (ts, 7, 2, False)]
                pa += [(ts, 500, 1 + b % 3, [0xA000 + tag + b]), (ts, 500, 1, [0xC0DE]), (ts, 501, 2, [0xB000 + b % 4])]
        return [("flow", flow_reqs(fl)), param_reqs(pa)]

    def read(t):
        return ("read", t, 5, None, None)

    steps += traffic(T, range(n), 0)
    first = 0 if n == 1 else 1  # a bucket of the first interval: its start + interval - 1, + 0, + 1
    steps += [read(T + (n - 1) * w), read(T + interval - 1), read(T + interval), read(T + interval + 1),
              read(T + first * w + interval - 1), read(T + first * w + interval), read(T + first * w + interval + 1),
              read(T + w // 2)]  # (earlier than the newest window)
    steps += traffic(T + interval, range(min(2, n)), 0x100)  # new values; the first interval's go stale bucket by bucket
    steps += [read(T + interval + min(2, n) * w - 1), read(T + 2 * interval - 1), read(T + 2 * interval),
              read(T + w - 1)]  # (the clock far behind the windows)
    steps += [read(T + 9 * interval + 7)]  # idle for longer than the interval: nothing counts, the slots still sit there
    steps += traffic(T + 12 * interval, range(min(3, n)), 0x200)
    steps += [read(T + 12 * interval + min(3, n) * w - 1)]
    steps += traffic(T + 12 * interval + n * w, range(min(2, n)), 0x300)
    return steps


def top_boundary(top, m, filler=0):
    """One param flow (600) with m live values read with `top`: sums with ties inside the list and across its end,
    keys whose order is not the order of insertion.  filler > 0: a second flow (601) gets that many values first,
    one second earlier (dead by the time of the reads), so that a small table rehashes and grows between the reads."""
    T = T0 - T0 % 1000 + 5000
    steps = [("param_rules", [pspec(600, 1000), pspec(601, 1000, 5, 500)])]
    if filler:
        for part in range(2):
            steps.append(param_reqs([(T - 3000 + part, 601, 1, [0xF0000 + part * filler + i]) for i in range(filler)]))
    sums = [3, 3, 2, 2, 2, 1, 1, 1, 1, 1][:m]  # ties at every list end used: top 1 (3,3), 5 (2|1 ..), 8 (1,1)
    keys = [((7919 * (i + 1)) % 997) << 20 | (0xFFFF - i) for i in range(m)]  # neither ascending nor descending
    steps.append(param_reqs([(T + i, 600, s, [k]) for i, (k, s) in enumerate(zip(keys, sums))]))
    steps.append(("read", T + 20, top, None, None))
    if filler:
        # (more values than half of the table the first rehash chose: the next rehash falls between the reads)
        steps.append(param_reqs([(T + 30 + i // (2 * filler), 601, 1, [0xE0000 + i]) for i in range(3 * filler + 100)]))
        steps.append(("read", T + 40, top, None, None))
    steps.append(param_reqs([(T + 50, 600, 1, [keys[-1]]), (T + 51, 600, 1, [keys[0]])]))
    steps.append(("read", T + 60, top, None, None))
    steps.append(param_reqs([(T + 70, 600, 2, [keys[0]])]))
    return steps


def occupy():
    """A flow rule whose prioritized requests get SHOULD_WAIT (the sequence of ClusterFlowCheckerTest): reads before
    the transfer window, inside it before any request (the copy carries the occupied pass), and after a request
    made the transfer."""
    t = T0 - T0 % 1000
    f = 98765

    def call(ts, *pri):
        return ("flow", flow_reqs([(ts, f, 1, p) for p in pri]))

    return [("flow_rules", [fspec(f, 5, 5, 1000), fspec(7, 3, 2, 500)]),
            call(t, False, False), call(t + 200, False), call(t + 400, True, False, True),
            call(t + 600, False, False), call(t + 800, False, True, False),
            ("read", t + 800, 5, None, None), ("read", t + 999, 5, None, None),   # before the transfer window
            ("read", t + 1000, 5, None, None), ("read", t + 1199, 5, None, None),  # inside it, before any request
            ("flow", flow_reqs([(t + 1000, f, 1, False), (t + 1000, 7, 1, False)])),  # the request that transfers
            ("read", t + 1000, 5, None, None), ("read", t + 1150, 5, None, None),
            call(t + 1200, False, True, False), call(t + 1400, True, True),
            ("read", t + 1500, 5, None, None),
            call(t + 1600, False, False, True), call(t + 2100, False, True)]


def chunk_edges(count, top=5, seed=3):
    """One param flow (700) with `count` live values of sum 1 to 3 and a few winners with larger sums (ties among
    them), next to a small flow (701)."""
    rng = np.random.default_rng(seed + count)
    T = T0 - T0 % 1000 + 3000
    keys = rng.permutation(np.arange(1, count + 1, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(1 << 40))
    assert len(np.unique(keys)) == count
    acq = rng.integers(1, 4, count)
    win = rng.choice(count, 7, replace=False)
    acq[win] = [9, 9, 8, 8, 8, 7, 6]
    rows = [(T + i * 600 // count, 700, int(a), [int(k)]) for i, (k, a) in enumerate(zip(keys, acq))]
    return [("param_rules", [pspec(700, 100), pspec(701, 100, 2, 500)]), param_reqs(rows),
            param_reqs([(T + 610, 701, 2, [5]), (T + 611, 701, 1, [6])]),
            ("read", T + 700, top, None, None), ("read", T + 700, 8, None, None),
            param_reqs([(T + 800, 700, 3, [int(keys[0])]), (T + 801, 701, 1, [5])])]


def hot_and_many(hot=70_000, small=3_000, seed=11):
    """One hot flow of about `hot` values beside `small` flows of 1-3 values, in one table."""
    rng = np.random.default_rng(seed)
    T = T0 - T0 % 1000 + 2000
    specs = [pspec(1000, 50)] + [pspec(2000 + i, 50) for i in range(small)]
    n = hot + 2 * small
    arr = np.zeros(n, dtype=A.PARAM_TOKEN_REQ_DTYPE)
    arr["ts"] = T + np.arange(n) * 700 // n
    fid = np.full(n, 1000, dtype=np.int64)
    at = np.sort(rng.choice(n, 2 * small, replace=False))
    fid[at] = 2000 + rng.integers(0, small, 2 * small)
    arr["flow_id"] = fid
    arr["acquire_count"] = rng.integers(1, 4, n)
    arr["n_values"] = 1
    arr["value_off"] = np.arange(n, dtype=np.uint64)
    vals = np.where(fid == 1000, rng.permutation(n).astype(np.uint64) + np.uint64(1), rng.integers(1, 4, n).astype(np.uint64))
    tail = param_reqs([(T + 900, 1000, 1, [int(vals[0])]), (T + 900, 2000, 1, [1])])
    return [("param_rules", specs), ("param", arr, vals.astype(np.uint64)), ("read", T + 800, 5, None, None), tail]


def wide_sums():
    """Sums of 2^32 + 1 and 5, and one between 2^31 and 2^32: the order follows the 64-bit sum."""
    T = T0 - T0 % 1000 + 1000
    M = 2147483647
    rows = [(T, 800, M, [0x10]), (T + 1, 800, 5, [0x20]), (T + 2, 800, M, [0x30]), (T + 3, 800, M, [0x10]),
            (T + 4, 800, 1000, [0x30]), (T + 5, 800, 3, [0x10])]
    return [("param_rules", [pspec(800, 1e12)]), param_reqs(rows), ("read", T + 10, 5, None, None),
            ("read", T + 10, 2, None, None), param_reqs([(T + 20, 800, 7, [0x20])])]


def owners(seed=5):
    """A random stream over 10 flows of five shapes with multi-value requests, some listing a value twice."""
    rng = np.random.default_rng(seed)
    shapes = [(10, 1000), (5, 500), (2, 1000), (1, 200), (16, 1600)]
    fids = [100 + i for i in range(10)]
    steps = [("param_rules", [pspec(f, 5 + 3 * i, *shapes[i % 5]) for i, f in enumerate(fids)])]
    for k in range(3):
        rows, t = [], T0 + 1500 * k
        for _ in range(1500):
            t += int(rng.integers(0, 2))
            f = int(rng.choice(fids))
            nv = 1 if rng.random() < 0.9 else int(rng.integers(2, 4))
            vs = [int(min(rng.zipf(1.3), 300)) | (f << 32) for _ in range(nv)]
            if nv > 1 and rng.random() < 0.5:
                vs[-1] = vs[0]
            rows.append((t, f, int(rng.integers(1, 4)), vs))
        steps.append(param_reqs(rows))
        steps.append(("read", t, 5, None, None))
    steps.append(param_reqs([(t + 1, fids[0], 1, [1 | (fids[0] << 32)])]))
    return steps


def reloads():
    """Dropping a param flow removes its row, a new flow that takes the freed index shows none of the old flow's
    values, a flow that stays keeps its counts; the same for flow rules."""
    T = T0 - T0 % 1000 + 1000
    a, b, c, d = pspec(600, 6), pspec(601, 5, 5, 500), pspec(602, 4), pspec(603, 5, 2, 1000)

    def tr(t, fids):
        return [("flow", flow_reqs([(t + i, 7 + i % 2, 1, False) for i in range(6)])),
                param_reqs([(t + i, f, 1 + i % 2, [0x50 + i % 3]) for i in range(8) for f in fids])]

    return [("flow_rules", [fspec(7, 2), fspec(8, 3, 5, 500)]), ("param_rules", [a, b, c])] + tr(T, [600, 601, 602]) + \
        [("read", T + 50, 5, None, None),
         ("flow_rules", [fspec(8, 4, 5, 500), fspec(9, 2)]), ("param_rules", [d, a])] + tr(T + 100, [600, 603]) + \
        [("read", T + 150, 5, None, None), ("param_rules", [a, b])] + tr(T + 200, [600, 601]) + \
        [("read", T + 250, 5, None, None)] + tr(T + 300, [600, 601])


def namespaces():
    """Flows of three namespaces (the third is "default": never assigned)."""
    T = T0 - T0 % 1000 + 1000
    ns = {"blue": [11, 511], "green": [12, 512, 513], "default": [13, 514]}
    fl = [(T + i, 11 + i % 3, 1, False) for i in range(9)]
    pa = [(T + i, 511 + i % 4, 1 + i % 2, [0x70 + i % 5]) for i in range(24)]
    steps = [("flow_rules", [fspec(11, 5), fspec(12, 5), fspec(13, 2)]),
             ("param_rules", [pspec(511, 9), pspec(512, 9), pspec(513, 9), pspec(514, 3)]),
             ("flow", flow_reqs(fl)), param_reqs(pa)]
    for name, ids in ns.items():
        steps.append(("read", T + 100, 5, name, set(ids)))
    steps += [("read", T + 100, 5, None, None), ("read", T + 100, 5, "", None),
              ("flow", flow_reqs([(T + 200 + i, 11 + i % 3, 1, False) for i in range(6)])),
              param_reqs([(T + 200 + i, 511 + i % 4, 1, [0x70 + i % 5]) for i in range(8)])]
    return steps, ns


SCENARIOS = {
    **{"edges-%d-%d" % s: (lambda s=s: window_edges(s)) for s in SHAPES},
    **{"top-%d-%d" % (t, m): (lambda t=t, m=m: top_boundary(t, m)) for t in (1, 5, 8)
       for m in sorted({1, max(1, t - 1), t, t + 1})},
    "top-rehash": lambda: top_boundary(5, 6, filler=400),
    "occupy": occupy,
    **{"chunk-%d" % c: (lambda c=c: chunk_edges(c)) for c in (4095, 4096, 4097, 8193)},
    "hot-and-many": hot_and_many,
    "wide-sums": wide_sums,
    "owners": owners,
    "reloads": reloads,
    "namespaces": lambda: namespaces()[0],
}
