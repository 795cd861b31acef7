"""The token server front-end with per-namespace request limiters (TokenServer(namespace_qps=...)).

ClusterServerConfigManager.getMaxAllowedQps(namespace) -> GlobalRequestLimiter of the namespace
(csrv/flow/statistic/limit/GlobalRequestLimiter.java:30-55); ConnectionManager.getConnectedCount(namespace)
(csrv/flow/rule/ClusterFlowRuleManager.java:308-317).
"""
import asyncio

import numpy as np
import pytest

from sentinel_amd import _abi as A
from sentinel_amd import token_server as S


class _NsStub:
    """Records, in order, every call that reaches the device boundary."""

    def __init__(self):
        self.calls = []

    def cluster_namespace(self, name, qps):
        self.calls.append(("namespace", name, qps))
        return len([c for c in self.calls if c[0] == "namespace"])

    def cluster_assign_flows(self, name, fids):
        self.calls.append(("assign", name, sorted(int(f) for f in fids)))

    def cluster_set_namespace_connected(self, name, n):
        self.calls.append(("ns_connected", name, n))

    def cluster_set_connected(self, fid, n):
        self.calls.append(("connected", fid, n))

    def cluster_request_array(self, reqs):
        self.calls.append(("request", len(reqs)))
        out = np.zeros(len(reqs), dtype=A.TOKEN_RES_DTYPE)
        out["remaining"] = reqs["flow_id"]
        return out


async def _client(port, frames, n_resp):
    r, w = await asyncio.open_connection("127.0.0.1", port)
    w.write(b"".join(frames))
    await w.drain()
    dec, out = S.FrameDecoder(), []
    while len(out) < n_resp:
        data = await asyncio.wait_for(r.read(65536), 10)
        assert data
        out += [S.decode_response(b) for b in dec.feed(data)]
    return r, w, out


async def _until(cond):
    for _ in range(2000):
        if cond():
            return
        await asyncio.sleep(0.001)
    assert cond()


def test_namespace_qps_registers_assigns_and_counts_per_namespace():
    async def run():
        stub = _NsStub()
        srv = S.TokenServer(stub, flow_namespaces={11: "ns-a", 12: "ns-b", 13: "ns-a", 14: "elsewhere"},
                            namespace_qps={"ns-a": 3, "ns-b": 100.5}, clock=lambda: 1000)
        # registered and assigned before anything is served
        assert stub.calls == [("namespace", "ns-a", 3), ("namespace", "ns-b", 100.5),
                              ("assign", "ns-a", [11, 13]), ("assign", "ns-b", [12])]
        del stub.calls[:]
        port = await srv.start(port=0)
        r1, w1, a = await _client(port, [S.encode_ping_request(1, "ns-a"), S.encode_flow_request(2, 11, 1, False)], 2)
        assert a[0] == (1, S.MSG_TYPE_PING, S.RESPONSE_STATUS_OK, 1) and a[1] == (2, 1, A.TOKEN_OK, (11, 0))
        assert stub.calls == [("ns_connected", "ns-a", 1), ("request", 1)]  # one call for the namespace's two flows
        r2, w2, b = await _client(port, [S.encode_ping_request(3, "ns-a"), S.encode_ping_request(4, "ns-b"),
                                         S.encode_ping_request(5, "elsewhere")], 3)
        assert [x[3] for x in b] == [2, 1, 1]
        # a namespace without a limiter of its own keeps the per-flow calls
        assert stub.calls[2:] == [("ns_connected", "ns-a", 2), ("ns_connected", "ns-b", 1), ("connected", 14, 1)]
        del stub.calls[:]
        w2.close()
        await _until(lambda: len(stub.calls) >= 3)
        assert sorted(stub.calls) == [("connected", 14, 0), ("ns_connected", "ns-a", 1), ("ns_connected", "ns-b", 0)]
        w1.close()
        await srv.stop()

    asyncio.run(run())


def test_without_namespace_qps_no_namespace_call():
    async def run():
        stub = _NsStub()
        srv = S.TokenServer(stub, flow_namespaces={11: "ns-a", 12: "ns-b", 13: "ns-a"}, clock=lambda: 1000)
        assert stub.calls == []
        port = await srv.start(port=0)
        r1, w1, a = await _client(port, [S.encode_ping_request(1, "ns-a"), S.encode_flow_request(2, 12, 1, False)], 2)
        w1.close()
        await _until(lambda: len(stub.calls) >= 5)
        await srv.stop()
        assert stub.calls == [("connected", 11, 1), ("connected", 13, 1), ("request", 1),
                              ("connected", 11, 0), ("connected", 13, 0)]

    asyncio.run(run())


@pytest.mark.gpu
def test_server_on_device_two_namespaces_match_oracles():
    # two socket clients, one a namespace, limits 3 and 100; modelled on test_token_server's device test
    import pyoracle as O
    from sentinel_amd import engine as E

    T0 = 1_700_000_000_000
    avg = dict(cluster_mode=True, cluster_threshold_type=A.CLUSTER_THRESHOLD_AVG_LOCAL)
    rules = [A.flow_rule("abc", c, cluster_flow_id=fid, **avg) for fid, c in ((101, 20), (102, 5), (201, 50))]
    flow_ns = {101: "ns-a", 102: "ns-a", 201: "ns-b"}
    limits = {"ns-a": 3, "ns-b": 100}
    eng = E.Engine(max_resources=64)
    eng.register("abc")
    eng.load_flow_rules(rules)
    tick = [T0]

    def clock():
        tick[0] += 37
        return tick[0]

    async def run():
        srv = S.TokenServer(eng, flow_namespaces=flow_ns, namespace_qps=limits, clock=clock, record=True)
        port = await srv.start(port=0)
        rng = np.random.default_rng(7)
        conns, got = [], []
        for c, (ns, fids) in enumerate((("ns-a", [101, 102, 999]), ("ns-b", [201, 999]))):
            conns.append(await _client(port, [S.encode_ping_request(c * 1000, ns)], 1))
            assert conns[-1][2][0] == (c * 1000, S.MSG_TYPE_PING, S.RESPONSE_STATUS_OK, 1)
        # several rounds, so that the clock crosses the limiter's one-second window
        for rnd in range(12):
            waits = []
            for c, fids in enumerate(([101, 102, 999], [201, 999])):
                frames = [S.encode_flow_request(c * 1000 + 1 + rnd * 25 + i, int(rng.choice(fids)),
                                                int(rng.integers(1, 4)), bool(rng.random() < 0.2)) for i in range(25)]
                r, w, _ = conns[c]
                w.write(b"".join(frames))
                waits.append(r)
            for r in waits:
                dec, out = S.FrameDecoder(), []
                while len(out) < 25:
                    data = await asyncio.wait_for(r.read(65536), 10)
                    assert data
                    out += [S.decode_response(b) for b in dec.feed(data)]
                got += out
            tick[0] += 150
        for _, w, _ in conns:
            w.close()
        await srv.stop()
        return srv, got

    srv, got = asyncio.run(run())
    orcs = {}
    for ns, lim in limits.items():
        orcs[ns] = O.Oracle(cluster_max_allowed_qps=lim)
        orcs[ns].register("abc")
        orcs[ns].load_flow_rules([r for r in rules if flow_ns[int(r.cluster_flow_id)] == ns])
        for fid, n in flow_ns.items():
            if n == ns:
                orcs[ns].cluster_set_connected(fid, 1)  # one client pinged every namespace
    by_xid = {}
    for xids, reqs, res in srv.submitted:
        ns_of = [flow_ns.get(int(f), "ns-a") for f in reqs["flow_id"]]
        want = [None] * len(reqs)
        for ns in limits:
            sel = [i for i, n in enumerate(ns_of) if n == ns]
            if sel:
                w = orcs[ns].cluster_request([(int(r["ts"]), int(r["flow_id"]), int(r["acquire_count"]),
                                               bool(r["prioritized"])) for r in reqs[sel]])
                for i, o in zip(sel, w):
                    want[i] = o
        dev = [(int(o["status"]), int(o["remaining"]), int(o["wait_in_ms"])) for o in res]
        assert dev == want
        by_xid.update(zip(xids, dev))
    assert len(got) == 600 and len(by_xid) == 600 and len(srv.batches) < 600
    for xid, typ, st, data in got:
        assert (st,) + tuple(data) == by_xid[xid]
    a = {s for x, (s, _, _) in by_xid.items() if x < 1000}
    b = {s for x, (s, _, _) in by_xid.items() if x >= 1000}
    assert a >= {A.TOKEN_OK, A.TOKEN_TOO_MANY_REQUEST, A.TOKEN_NO_RULE_EXISTS}
    assert b >= {A.TOKEN_OK, A.TOKEN_NO_RULE_EXISTS} and A.TOKEN_TOO_MANY_REQUEST not in b
