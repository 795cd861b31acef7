"""TokenServer's key_sweep_s: the tick loop sweeps the engine's parameter key dictionary between device calls
(no GPU needed: a stub service records the order of the calls).  key_sweep_s = 0 sweeps after every tick; None
(the default), or a service without param_keys_sweep, never sweeps."""
import asyncio

import numpy as np

from sentinel_amd import _abi as A
from sentinel_amd import token_server as S


class _Service:
    def __init__(self):
        self.calls = []

    def cluster_set_connected(self, fid, n):
        pass

    def cluster_request_param_array(self, reqs, vals):
        self.calls.append(("param", [int(v) for v in vals]))
        out = np.zeros(len(reqs), dtype=A.TOKEN_RES_DTYPE)
        out["status"] = A.TOKEN_OK
        return out


class _Sweeping(_Service):
    def __init__(self, fail=False):
        super().__init__()
        self.fail = fail

    def param_keys_sweep(self):
        self.calls.append(("sweep",))
        if self.fail:
            raise RuntimeError("device error")


async def _ask(port, frames):
    r, w = await asyncio.open_connection("127.0.0.1", port)
    dec, out = S.FrameDecoder(), []
    for f in frames:  # one tick a frame: wait for each answer
        w.write(f)
        await w.drain()
        n = len(out) + 1
        while len(out) < n:
            data = await asyncio.wait_for(r.read(65536), 10)
            assert data
            out += [S.decode_response(b) for b in dec.feed(data)]
    w.close()
    return out


def _run(service, **kw):
    async def run():
        srv = S.TokenServer(service, clock=lambda: 1000, param_key=lambda text, cls: len(text), **kw)
        port = await srv.start(port=0)
        out = await _ask(port, [S.encode_param_flow_request(i, 17, 1, [(S.PARAM_TYPE_STRING, "v" * (i + 1))])
                                for i in range(3)])
        await srv.stop()
        return srv, out
    return asyncio.run(run())


def test_sweep_after_every_tick_between_device_calls():
    svc = _Sweeping()
    srv, out = _run(svc, key_sweep_s=0)
    assert [o[2] for o in out] == [A.TOKEN_OK] * 3
    assert svc.calls == [("param", [1]), ("sweep",), ("param", [2]), ("sweep",), ("param", [3]), ("sweep",)]
    assert srv.sweeps == 3 and not srv.errors


def test_no_sweep_by_default_or_without_the_call():
    svc = _Sweeping()
    srv, _ = _run(svc)
    assert [c[0] for c in svc.calls] == ["param"] * 3 and srv.sweeps == 0
    plain = _Service()
    srv, _ = _run(plain, key_sweep_s=0)
    assert [c[0] for c in plain.calls] == ["param"] * 3 and srv.sweeps == 0 and srv.key_sweep_s is None


def test_a_failing_sweep_is_recorded_and_the_loop_keeps_serving():
    svc = _Sweeping(fail=True)
    srv, out = _run(svc, key_sweep_s=0)
    assert [o[2] for o in out] == [A.TOKEN_OK] * 3
    assert srv.sweeps == 0 and len(srv.errors) == 3


def test_a_long_period_does_not_sweep_yet():
    svc = _Sweeping()
    srv, _ = _run(svc, key_sweep_s=3600.0)
    assert [c[0] for c in svc.calls] == ["param"] * 3 and srv.sweeps == 0
