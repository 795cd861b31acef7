"""Python binding of libsentinel_gpu.so (include/sentinel_gpu.h).

The engine is the product: every decision is taken by the HIP kernels behind the
C ABI.  There is no CPU fallback -- if the library or a gfx950 device is missing
this module raises instead of computing anything.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _abi as A

_HERE = os.path.dirname(os.path.abspath(__file__))
# SG_LIB_PATH: diagnostics only (e.g. a -DSG_KPROF build for tools/hotprobe.py)
LIB_PATH = os.environ.get("SG_LIB_PATH") or os.path.join(_HERE, "libsentinel_gpu.so")
_lib = None

# every entry point declared in include/sentinel_gpu.h
EXPORTS = (
    "sg_config_default", "sg_engine_create", "sg_engine_destroy", "sg_register_resources", "sg_resource_id",
    "sg_load_flow_rules", "sg_load_degrade_rules", "sg_load_param_rules", "sg_param_key", "sg_submit",
    "sg_submit_async", "sg_sync", "sg_snapshot_metrics", "sg_cluster_set_connected_count",
    "sg_cluster_request_tokens", "sg_cluster_request_param_tokens", "sg_read_node", "sg_last_error", "sg_last_timings",
    "sg_submit_ex", "sg_submit_ex_async", "sg_intern_origin", "sg_intern_context", "sg_param_thread_count",
    "sg_cluster_namespace", "sg_cluster_assign_flows", "sg_cluster_set_namespace_connected",
    "sg_cluster_namespace_qps", "sg_load_authority_rules", "sg_param_intern", "sg_param_intern_batch",
    "sg_param_keys_sweep", "sg_param_keys_stats", "sg_cluster_param_table_stats",
    "sg_track_inbound", "sg_read_inbound_node", "sg_inbound_metrics",
    "sg_cluster_metrics", "sg_param_key_value", "sg_cluster_embedded",
)


class SentinelError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"sentinel_gpu error {code}: {msg}")
        self.code = code


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SentinelError(A.SG_EDEVICE, f"{LIB_PATH} is not built (run __graft_entry__.build())")
        L = C.CDLL(LIB_PATH)
        P = C.c_void_p
        L.sg_config_default.argtypes = [C.POINTER(A.SgConfig)]
        L.sg_engine_create.argtypes = [C.POINTER(A.SgConfig), C.POINTER(C.c_void_p)]
        L.sg_engine_destroy.argtypes = [P]
        L.sg_register_resources.argtypes = [P, C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_uint32)]
        L.sg_resource_id.argtypes = [P, C.c_char_p, C.POINTER(C.c_uint32)]
        L.sg_load_flow_rules.argtypes = [P, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        L.sg_load_degrade_rules.argtypes = [P, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        L.sg_load_param_rules.argtypes = [P, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        L.sg_load_authority_rules.argtypes = [P, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        L.sg_param_key.argtypes = [P, C.c_char_p, C.c_char_p, C.POINTER(C.c_uint64)]
        L.sg_param_intern.argtypes = [P, C.c_char_p, C.c_char_p, C.POINTER(C.c_uint64)]
        L.sg_param_intern_batch.argtypes = [P, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_uint32,
                                            C.POINTER(C.c_uint64)]
        L.sg_param_keys_sweep.argtypes = [P]
        L.sg_param_keys_stats.argtypes = [P, C.POINTER(C.c_uint64), C.c_int]
        L.sg_submit.argtypes = [P, C.c_void_p, C.c_uint64, C.c_void_p]
        L.sg_submit_async.argtypes = [P, C.c_void_p, C.c_uint64, C.c_void_p]
        L.sg_sync.argtypes = [P]
        L.sg_submit_ex.argtypes = [P, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
        L.sg_submit_ex_async.argtypes = [P, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
        L.sg_intern_origin.argtypes = [P, C.c_char_p, C.POINTER(C.c_uint32)]
        L.sg_intern_context.argtypes = [P, C.c_char_p, C.POINTER(C.c_uint32)]
        L.sg_snapshot_metrics.argtypes = [P, C.c_int64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.sg_cluster_set_connected_count.argtypes = [P, C.c_int64, C.c_int32]
        L.sg_cluster_request_tokens.argtypes = [P, C.c_void_p, C.c_uint64, C.c_void_p]
        L.sg_cluster_request_param_tokens.argtypes = [P, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
        L.sg_cluster_param_table_stats.argtypes = [P, C.POINTER(C.c_uint64), C.c_int]
        L.sg_cluster_namespace.argtypes = [P, C.c_char_p, C.c_double, C.POINTER(C.c_uint32)]
        L.sg_cluster_assign_flows.argtypes = [P, C.c_char_p, C.POINTER(C.c_int64), C.c_uint32]
        L.sg_cluster_set_namespace_connected.argtypes = [P, C.c_char_p, C.c_int32]
        L.sg_cluster_namespace_qps.argtypes = [P, C.c_char_p, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.sg_read_node.argtypes = [P, C.c_uint32, C.c_int64, C.POINTER(A.SgNodeState)]
        L.sg_last_error.restype = C.c_char_p
        L.sg_last_timings.argtypes = [P, C.POINTER(C.c_double), C.c_int]
        _lib = L
    return _lib


# the global inbound node's entry points, bound on first use: SG_LIB_PATH may name an older build of the library (the
# A/B runs of bench.py against a parent commit), which loads as long as nothing asks it for them
_INBOUND_ARGS = {
    "sg_track_inbound": lambda: [C.c_void_p, C.c_int32],
    "sg_read_inbound_node": lambda: [C.c_void_p, C.c_int64, C.POINTER(A.SgNodeState)],
    "sg_inbound_metrics": lambda: [C.c_void_p, C.c_int64, C.POINTER(C.c_double), C.c_int],
}


def _inbound(name):
    fn = getattr(lib(), name)
    if fn.argtypes is None:
        fn.argtypes = _INBOUND_ARGS[name]()
    return fn


# the cluster metrics' entry points, bound on first use for the same reason
_CMETRICS_ARGS = {
    "sg_cluster_metrics": lambda: [C.c_void_p, C.c_char_p, C.c_int64, C.c_uint32, C.c_void_p, C.c_uint64,
                                   C.POINTER(C.c_uint64)],
    "sg_param_key_value": lambda: [C.c_void_p, C.c_uint64, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t],
}


def _cmetrics(name):
    fn = getattr(lib(), name)
    if fn.argtypes is None:
        fn.argtypes = _CMETRICS_ARGS[name]()
    return fn


# the embedded token server's entry point, bound on first use for the same reason
def _embedded():
    fn = lib().sg_cluster_embedded
    if fn.argtypes is None:
        fn.argtypes = [C.c_void_p, C.c_int32]
    return fn


def _check(rc: int):
    if rc != 0:
        raise SentinelError(rc, (lib().sg_last_error() or b"").decode(errors="replace"))


def default_config(**kw) -> A.SgConfig:
    cfg = A.SgConfig()
    lib().sg_config_default(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def param_key(value, class_type="java.lang.String") -> int:
    out = C.c_uint64()
    _check(lib().sg_param_key(None, None if value is None else str(value).encode(),
                              None if class_type is None else class_type.encode(), C.byref(out)))
    return out.value


class Engine:
    """One MI355X engine (one shard of resources on one GPU)."""

    def __init__(self, **cfg):
        self._cfg = default_config(**cfg)
        h = C.c_void_p()
        _check(lib().sg_engine_create(C.byref(self._cfg), C.byref(h)))
        self.h = h
        self.n_events = 0

    def close(self):
        if getattr(self, "h", None):
            lib().sg_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- resources / rules
    def register(self, name: str) -> int:
        return self.register_many([name])[0]

    def register_many(self, names) -> np.ndarray:
        arr = (C.c_char_p * max(1, len(names)))(*[n.encode() if isinstance(n, str) else n for n in names])
        out = np.zeros(len(names), dtype=np.uint32)
        _check(lib().sg_register_resources(self.h, arr, len(names), out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def register_ptrs(self, names_ptr, n: int):
        _check(lib().sg_register_resources(self.h, C.cast(names_ptr, C.POINTER(C.c_char_p)), n, None))

    def resource_id(self, name: str) -> int:
        out = C.c_uint32()
        _check(lib().sg_resource_id(self.h, name.encode(), C.byref(out)))
        return out.value

    def _load(self, fn, rules, struct):
        if isinstance(rules, tuple):  # (pointer, n) straight from tracegen
            ptr, n = rules
        else:
            arr = (struct * max(1, len(rules)))(*rules)
            ptr, n = C.cast(arr, C.c_void_p), len(rules)
        out = C.c_uint32()
        _check(fn(self.h, ptr, n, C.byref(out)))
        return out.value

    def load_flow_rules(self, rules) -> int:
        return self._load(lib().sg_load_flow_rules, rules, A.SgFlowRule)

    def load_degrade_rules(self, rules) -> int:
        return self._load(lib().sg_load_degrade_rules, rules, A.SgDegradeRule)

    def load_param_rules(self, rules) -> int:
        return self._load(lib().sg_load_param_rules, rules, A.SgParamRule)

    def load_authority_rules(self, rules) -> int:
        """AuthorityRuleManager.loadRules: A.authority_rule(...) list (empty: clear); returns the rules kept."""
        return self._load(lib().sg_load_authority_rules, rules, A.SgAuthorityRule)

    # ---- exact parameter keys (sg_param_intern: equal keys only for equal values; keys belong to this engine)
    def param_intern(self, value, class_type="java.lang.String") -> int:
        """The value's key from the engine's dictionary: param_key()'s word unless another live value owns it.
        Callable from any thread.  See include/sentinel_gpu.h for how long a key may be used (the epoch rule)."""
        out = C.c_uint64()
        _check(lib().sg_param_intern(self.h, None if value is None else str(value).encode(),
                                     None if class_type is None else class_type.encode(), C.byref(out)))
        return out.value

    def param_intern_many(self, values, class_types="java.lang.String") -> np.ndarray:
        """sg_param_intern_batch: values (str / bytes / None each) with one class type for all, or one each."""
        n = len(values)
        enc = [v if v is None or isinstance(v, bytes) else str(v).encode() for v in values]
        vals = (C.c_char_p * max(1, n))(*enc)
        if class_types is None or isinstance(class_types, str):
            ct = None if class_types is None else class_types.encode()
            types = (C.c_char_p * max(1, n))(*([ct] * n))
        else:
            types = (C.c_char_p * max(1, n))(*[None if t is None else t.encode() for t in class_types])
        out = np.zeros(n, dtype=np.uint64)
        _check(lib().sg_param_intern_batch(self.h, vals, types, n, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def param_keys_sweep(self) -> dict:
        """sg_param_keys_sweep: drop the dictionary entries the device no longer holds; returns param_keys_stats().
        Waits for every submitted batch; call it from the submitting thread."""
        _check(lib().sg_param_keys_sweep(self.h))
        return self.param_keys_stats()

    def param_keys_stats(self) -> dict:
        out = (C.c_uint64 * 8)()
        k = lib().sg_param_keys_stats(self.h, out, 8)
        names = ("entries", "displaced", "pinned", "sweeps", "candidates", "held", "dropped", "sweep_us")
        return {names[i]: int(out[i]) for i in range(k)}

    def keysweep_scans(self):
        """The last sweep's device scans in ms: (maps, key ring, token server values); diagnostics export
        sgx_keysweep_scans."""
        fn = lib().sgx_keysweep_scans
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        out = (C.c_double * 3)()
        if fn(self.h, out) != 0:
            raise SentinelError(A.SG_EDEVICE, "sgx_keysweep_scans failed")
        return tuple(out)

    # ---- decisions
    def submit(self, events: np.ndarray) -> np.ndarray:
        ev = np.ascontiguousarray(events, dtype=A.EVENT_DTYPE)
        out = np.zeros(len(ev), dtype=np.uint32)
        _check(lib().sg_submit(self.h, ev.ctypes.data, len(ev), out.ctypes.data))
        self.n_events += len(ev)
        return out

    def submit_ex(self, events: np.ndarray, ext: np.ndarray = None, args: np.ndarray = None) -> np.ndarray:
        """sg_submit_ex: ext = A.EXT_DTYPE per event (or None), args = A.ARG_DTYPE table (see A.ext_tables)."""
        ev = np.ascontiguousarray(events, dtype=A.EVENT_DTYPE)
        ex = None if ext is None else np.ascontiguousarray(ext, dtype=A.EXT_DTYPE)
        ar = None if args is None or len(args) == 0 else np.ascontiguousarray(args, dtype=A.ARG_DTYPE)
        out = np.zeros(len(ev), dtype=np.uint32)
        _check(lib().sg_submit_ex(self.h, ev.ctypes.data, None if ex is None else ex.ctypes.data, len(ev),
                                  None if ar is None else ar.ctypes.data, 0 if ar is None else len(ar), out.ctypes.data))
        self.n_events += len(ev)
        return out

    def intern_origin(self, name: str) -> int:
        out = C.c_uint32()
        _check(lib().sg_intern_origin(self.h, name.encode(), C.byref(out)))
        return out.value

    def intern_context(self, name: str) -> int:
        out = C.c_uint32()
        _check(lib().sg_intern_context(self.h, name.encode(), C.byref(out)))
        return out.value

    def submit_ptr(self, ev_ptr: int, n: int, out_ptr: int, sync: bool = True):
        """Device (or host) pointers, e.g. torch tensors' data_ptr()."""
        if sync:
            _check(lib().sg_submit(self.h, C.c_void_p(ev_ptr), n, C.c_void_p(out_ptr)))
        else:
            _check(lib().sg_submit_async(self.h, C.c_void_p(ev_ptr), n, C.c_void_p(out_ptr)))
        self.n_events += n

    def submit_ex_ptr(self, ev_ptr: int, ext_ptr: int, n: int, out_ptr: int, sync: bool = True, args_ptr: int = 0,
                      n_args: int = 0):
        """sg_submit_ex(_async) on device (or host) pointers."""
        fn = lib().sg_submit_ex if sync else lib().sg_submit_ex_async
        _check(fn(self.h, C.c_void_p(ev_ptr), C.c_void_p(ext_ptr) if ext_ptr else None, n,
                  C.c_void_p(args_ptr) if args_ptr else None, n_args, C.c_void_p(out_ptr)))
        self.n_events += n

    def sync(self):
        _check(lib().sg_sync(self.h))

    def timings(self):
        """Device time of the last submit in ms: [group, decide, post, total] (sg_last_timings)."""
        ms = (C.c_double * 4)()
        k = lib().sg_last_timings(self.h, ms, 4)
        return list(ms[:k])

    def timing_log(self, cap: int = 4096) -> np.ndarray:
        """Stage times of every batch decided since the last call, [n, 4] ms (group, decide, post,
        total); diagnostics export sgx_timing_log, drains the pipeline first."""
        buf = (C.c_double * (4 * cap))()
        fn = lib().sgx_timing_log
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        k = fn(self.h, buf, cap)
        return np.frombuffer(buf, dtype=np.float64, count=4 * k).reshape(k, 4).copy()

    def gap_log(self, cap: int = 4096) -> np.ndarray:
        """How long each stream stood empty before every batch decided since the last call, [n, 2] ms: the group
        stream from the previous batch's group end to this batch's group start, the decide stream from the previous
        batch's post end to this batch's decide start (0, 0 for the engine's first batch); diagnostics export
        sgx_gap_log, drains the pipeline first."""
        buf = (C.c_double * (2 * cap))()
        fn = lib().sgx_gap_log
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        k = fn(self.h, buf, cap)
        return np.frombuffer(buf, dtype=np.float64, count=2 * k).reshape(k, 2).copy()

    def spans_total(self) -> int:
        """Frozen span slots the cooperative kernels recorded so far (diagnostics export sgx_spans_total)."""
        fn = lib().sgx_spans_total
        fn.restype = C.c_ulonglong
        fn.argtypes = [C.c_void_p]
        return int(fn(self.h))

    def hot_marked(self) -> int:
        """Hot ids whose side tables (forward links, bst[]) the last batch built: those whose owner can skip a frozen
        stretch inside some 500 ms bucket (diagnostics export sgx_hot_marked; 0 where the tables are built
        everywhere)."""
        fn = lib().sgx_hot_marked
        fn.restype = C.c_uint
        fn.argtypes = [C.c_void_p]
        return int(fn(self.h))

    def preblocked_stats(self):
        """Where the last collected batch placed the resources that have seen a pre-blocked ENTRY
        (SG_F_BLOCKED_UPSTREAM, or one its authority rule blocks): [0] their segments in cooperative bins, [1] in
        lane bins, [2] pre-blocked decision words written ahead of the cooperative owners (diagnostics export
        sgx_preblocked_last; drains the pipeline first)."""
        fn = lib().sgx_preblocked_last
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        out = np.zeros(3, dtype=np.uint64)
        if fn(self.h, out.ctypes.data, 3) != 3:
            raise SentinelError(A.SG_EDEVICE, "sgx_preblocked_last failed")
        return [int(v) for v in out]

    def read_aux_node(self, res: int, kind: int, node_id: int):
        """An origin (kind 0, origin id) / context (kind 1, context id) node of res: second window [2, 8], thread,
        minute pass history [2, 2] ({ws, pass} per second parity); None if absent (diagnostics export
        sgx_read_aux_node)."""
        fn = lib().sgx_read_aux_node
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        out = np.zeros(21, dtype=np.int64)
        rc = fn(self.h, res, kind, node_id, out.ctypes.data)
        if rc < 0:
            raise SentinelError(A.SG_EDEVICE, "sgx_read_aux_node failed")
        if rc == 0:
            return None
        return {"second": out[:16].reshape(2, 8), "thread": int(out[16]), "mhist": out[17:21].reshape(2, 2)}

    def pv_last(self) -> dict:
        """The last batch's value-parallel pre pass (diagnostics export sgx_pv_last): pre pass segments,
        accesses, blocked stretches its walk jumped; post pass segments eligible, ops, segments committed."""
        fn = lib().sgx_pv_last
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p]
        out = np.zeros(7, dtype=np.uint64)
        if fn(self.h, out.ctypes.data) != 0:
            raise SentinelError(A.SG_EDEVICE, "sgx_pv_last failed")
        return {"segments": int(out[0]), "accesses": int(out[1]), "ranges": int(out[2]),
                "post_segments": int(out[3]), "post_ops": int(out[4]), "post_done": int(out[5]),
                "walk_max": int(out[6])}

    def param_pool(self) -> dict:
        """The param map bucket pool (diagnostics export sgx_param_pool): size, taken, taken at the last compaction,
        compactions between batches, compactions a batch ran on the device when its growth found the pool short."""
        fn = lib().sgx_param_pool
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p]
        out = np.zeros(5, dtype=np.uint64)
        if fn(self.h, out.ctypes.data) != 0:
            raise SentinelError(A.SG_EDEVICE, "sgx_param_pool failed")
        return {"buckets": int(out[0]), "taken": int(out[1]), "floor": int(out[2]), "compactions": int(out[3]),
                "device_compactions": int(out[4])}

    def param_compact(self):
        """Compact the param map pool now, between batches (diagnostics export sgx_param_compact: the same
        on-device compaction a submit runs once growth took half of the free pool)."""
        fn = lib().sgx_param_compact
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p]
        if fn(self.h) != 0:
            raise SentinelError(A.SG_EDEVICE, "sgx_param_compact failed")

    def param_thread_count(self, res: int, idx: int, key: int, with_presence: bool = False):
        """ParameterMetric.getThreadCount (sg_param_thread_count): the value's count in the thread-count map of
        paramIdx idx, 0 if absent; with_presence: (count, present).  Does not reorder the map's LRU."""
        fn = lib().sg_param_thread_count
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_uint32, C.c_int32, C.c_uint64, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
        c, p = C.c_int64(), C.c_int32()
        _check(fn(self.h, res, idx, key, C.byref(c), C.byref(p)))
        return (c.value, bool(p.value)) if with_presence else c.value

    def read_node(self, res: int, now: int = 0) -> dict:
        st = A.SgNodeState()
        _check(lib().sg_read_node(self.h, res, now, C.byref(st)))
        return A.node_state_to_numpy(st)

    # ---- the global inbound node, Constants.ENTRY_NODE (sg_track_inbound)
    def track_inbound(self, on: bool = True):
        """Count every EntryType.IN entry and exit on the global inbound node as StatisticSlot does.  Off by default;
        turning it on is accepted only before the first batch (SentinelError SG_ESTATE afterwards), off at any time."""
        _check(_inbound("sg_track_inbound")(self.h, 1 if on else 0))

    def read_inbound_node(self, now: int = 0) -> dict:
        """The node's windows and thread count, as read_node gives a ClusterNode's (SG_ESTATE if never tracked)."""
        st = A.SgNodeState()
        _check(_inbound("sg_read_inbound_node")(self.h, int(now), C.byref(st)))
        return A.node_state_to_numpy(st)

    def inbound_metrics(self, now: int) -> dict:
        """What SystemRuleManager / SystemStatusListener read of the node at now (sg_inbound_metrics); a read-back."""
        out = (C.c_double * 9)()
        k = _inbound("sg_inbound_metrics")(self.h, int(now), out, 9)
        if k != 9:
            raise SentinelError(A.SG_ESTATE, (lib().sg_last_error() or b"").decode(errors="replace"))
        names = ("pass_qps", "block_qps", "success_qps", "exception_qps", "total_qps", "avg_rt", "min_rt",
                 "max_success_qps", "cur_thread_num")
        return {names[i]: float(out[i]) for i in range(k)}

    def inbound_last(self):
        """The inbound pass of the last collected batch: [0] workgroups that left a partial, [1] records visited,
        [2] updates counted (diagnostics export sgx_inbound_last; drains the pipeline first)."""
        fn = lib().sgx_inbound_last
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        out = np.zeros(3, dtype=np.uint64)
        if fn(self.h, out.ctypes.data, 3) != 3:
            raise SentinelError(A.SG_ESTATE, "sgx_inbound_last failed (the inbound node was never tracked)")
        return [int(v) for v in out]

    def snapshot(self, now: int, cap: int = 1 << 16) -> np.ndarray:
        out = np.zeros(cap, dtype=A.METRIC_NODE_DTYPE)
        n = C.c_uint64()
        _check(lib().sg_snapshot_metrics(self.h, int(now), out.ctypes.data, cap, C.byref(n)))
        return out[: min(cap, n.value)]

    def snapshot_to(self, now: int, out_ptr: int, cap: int) -> int:
        """sg_snapshot_metrics into caller memory (a device pointer stays on the device); returns the
        number of MetricNode rows produced (only min(n, cap) are written)."""
        n = C.c_uint64()
        _check(lib().sg_snapshot_metrics(self.h, int(now), C.c_void_p(out_ptr), cap, C.byref(n)))
        return n.value

    # ---- token server (sg_cluster_*; DefaultTokenService.requestToken, csrv/flow/DefaultTokenService.java:37-48)
    # ---- embedded token server: ClusterStateManager's server state (sg_cluster_embedded)
    EMBEDDED_STATS = ("requests", "ok", "blocked", "should_wait", "too_many_request", "bad_request", "fail",
                      "no_rule_exists", "words_ahead", "coop_segments", "lane_segments", "late_segments")

    def cluster_embedded(self, on: bool = True):
        """Decide the flow rules' cluster rules on the decision path with this engine's own token server (embedded
        mode).  Off by default: a cluster rule is then decided as without a TokenService.  SentinelError SG_ENOTSUP,
        with nothing changed, if a loaded cluster flow rule lies outside the supported shape (sentinel_gpu.h)."""
        _check(_embedded()(self.h, 1 if on else 0))

    def cluster_embedded_stats(self) -> dict:
        """The embedded token server's part of the last collected batch: token requests issued, answers by status,
        BLOCKED words written ahead of the cooperative owners, segments of embedded resources in cooperative bins, in
        lane bins and in the late lane pass (always 0: fallback rules are not taken).  Diagnostics export
        sgx_embedded_last; drains the pipeline first."""
        fn = lib().sgx_embedded_last
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        k = len(self.EMBEDDED_STATS)
        out = np.zeros(k, dtype=np.uint64)
        if fn(self.h, out.ctypes.data, k) != k:
            raise SentinelError(A.SG_EDEVICE, "sgx_embedded_last failed")
        return {name: int(v) for name, v in zip(self.EMBEDDED_STATS, out)}

    def cluster_embedded_ms(self):
        """Device times [ms] of the embedded steps in the last collected batch that made requests: the extraction
        (with the host's wait for the request count), the token call, the answers' scatter (diagnostics export
        sgx_embedded_ms; drains the pipeline first).  For synchronous batches only: the engine keeps one set of timing
        events, so with a second embedded batch decided before the first is collected the values are stale or 0."""
        fn = lib().sgx_embedded_ms
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        out = np.zeros(3, dtype=np.float64)
        if fn(self.h, out.ctypes.data, 3) != 3:
            raise SentinelError(A.SG_EDEVICE, "sgx_embedded_ms failed")
        return {"extract": float(out[0]), "token_call": float(out[1]), "scatter": float(out[2])}

    def cluster_set_connected(self, flow_id: int, n: int):
        _check(lib().sg_cluster_set_connected_count(self.h, int(flow_id), int(n)))

    # ---- namespaces: a GlobalRequestLimiter and a connected count each (csrv/flow/statistic/limit/
    # GlobalRequestLimiter.java:30-80, ConnectionManager.getConnectedCount(namespace))
    def cluster_namespace(self, name, max_qps: float) -> int:
        """Register a namespace, or change a registered one's limit (its window stays); returns its dense id."""
        out = C.c_uint32()
        _check(lib().sg_cluster_namespace(self.h, None if name is None else str(name).encode(), float(max_qps),
                                          C.byref(out)))
        return out.value

    def cluster_assign_flows(self, name: str, flow_ids):
        """The flowIds (cluster flow rules and cluster param rules alike) of a registered namespace."""
        ids = np.ascontiguousarray(flow_ids, dtype=np.int64).reshape(-1)
        _check(lib().sg_cluster_assign_flows(self.h, name.encode(), ids.ctypes.data_as(C.POINTER(C.c_int64)), len(ids)))

    def cluster_set_namespace_connected(self, name: str, n: int):
        _check(lib().sg_cluster_set_namespace_connected(self.h, name.encode(), int(n)))

    def cluster_namespace_qps(self, name: str, now: int):
        """(GlobalRequestLimiter.getCurrentQps at now, getMaxAllowedQps) of the namespace; a read-back."""
        cur, lim = C.c_double(), C.c_double()
        _check(lib().sg_cluster_namespace_qps(self.h, name.encode(), int(now), C.byref(cur), C.byref(lim)))
        return cur.value, lim.value

    # ---- cluster/server/metricList: a ClusterMetricNode per flowId (csrv/flow/statistic/ClusterMetricNodeGenerator.java)
    def cluster_metrics(self, now: int, ns=None, top: int = 5, cap: int = None) -> np.ndarray:
        """sg_cluster_metrics at now: A.CLUSTER_METRIC_DTYPE rows, the cluster flow rules' flowIds ascending, then the
        cluster param rules' with their `top` hottest values (sum descending, key ascending).  ns: a registered
        namespace's flows only (None: every flow).  A read-back: no later decision depends on the call.  cap: rows
        to return at most (None: all)."""
        n = C.c_uint64()
        fn = _cmetrics("sg_cluster_metrics")
        nsb = None if ns is None else str(ns).encode()
        want = 4096 if cap is None else int(cap)
        out = np.zeros(max(1, want), dtype=A.CLUSTER_METRIC_DTYPE)
        _check(fn(self.h, nsb, int(now), int(top), out.ctypes.data, want, C.byref(n)))
        if cap is None and n.value > want:  # (more flows than the first buffer holds: once more, with room for all)
            want = n.value
            out = np.zeros(want, dtype=A.CLUSTER_METRIC_DTYPE)
            _check(fn(self.h, nsb, int(now), int(top), out.ctypes.data, want, C.byref(n)))
        return out[: min(want, n.value)]

    def cluster_metrics_count(self, now: int, ns=None, top: int = 5) -> int:
        """The number of rows cluster_metrics would return (sg_cluster_metrics with cap 0)."""
        n = C.c_uint64()
        _check(_cmetrics("sg_cluster_metrics")(self.h, None if ns is None else str(ns).encode(), int(now), int(top),
                                               None, 0, C.byref(n)))
        return n.value

    def cluster_metrics_last(self) -> dict:
        """The last cluster_metrics call (diagnostics export sgx_cluster_metrics_last): candidates, chunks, the chunk
        size, table slots scanned, per-stage device times in ms (HIP events) and the call's wall time in ms."""
        fn = lib().sgx_cluster_metrics_last
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int]
        out = (C.c_double * 10)()
        if fn(self.h, out, 10) != 10:
            raise SentinelError(A.SG_EDEVICE, "sgx_cluster_metrics_last failed")
        names = ("candidates", "chunks", "chunk_size", "slots", "rows_ms", "scan_ms", "group_ms", "select_ms",
                 "merge_ms", "wall_ms")
        d = {names[i]: float(out[i]) for i in range(10)}
        for k in names[:4]:
            d[k] = int(d[k])
        return d

    def param_key_value(self, key: int):
        """sg_param_key_value: (class_type, text) of the value behind a parameter key, or None when the key is of a
        hashed kind (String, double, a long outside +-2^59) and no dictionary entry owns it."""
        fn = _cmetrics("sg_param_key_value")
        ct = C.create_string_buffer(32)
        cap = 256
        while True:
            val = C.create_string_buffer(cap)
            rc = fn(self.h, int(key), ct, len(ct), val, cap)
            if rc >= 0:
                return ct.value.decode(), val.raw[:rc].decode(errors="replace")
            if rc == A.SG_ENOTFOUND:
                return None
            if rc == A.SG_EINVAL and cap < (1 << 24):
                cap *= 16
                continue
            _check(rc)

    def cluster_request_array(self, reqs: np.ndarray) -> np.ndarray:
        """reqs: A.TOKEN_REQ_DTYPE array (time-ordered) -> A.TOKEN_RES_DTYPE array."""
        reqs = np.ascontiguousarray(reqs, dtype=A.TOKEN_REQ_DTYPE)
        out = np.zeros(len(reqs), dtype=A.TOKEN_RES_DTYPE)
        _check(lib().sg_cluster_request_tokens(self.h, reqs.ctypes.data, len(reqs), out.ctypes.data))
        return out

    def cluster_request_ptr(self, req_ptr: int, n: int, out_ptr: int):
        """Device (or host) buffers: n A.TOKEN_REQ_DTYPE rows at req_ptr -> A.TOKEN_RES_DTYPE rows at out_ptr."""
        _check(lib().sg_cluster_request_tokens(self.h, C.c_void_p(req_ptr), n, C.c_void_p(out_ptr)))

    def cluster_request(self, reqs):
        """reqs: list of (ts, flow_id, acquire, prioritized) -> list of (status, remaining, wait)."""
        arr = np.zeros(len(reqs), dtype=A.TOKEN_REQ_DTYPE)
        for i, (ts, fid, acq, pr) in enumerate(reqs):
            arr[i] = (ts, fid, acq, int(pr))
        out = self.cluster_request_array(arr)
        return [(int(o["status"]), int(o["remaining"]), int(o["wait_in_ms"])) for o in out]

    # ---- TokenService.requestParamToken (csrv/flow/DefaultTokenService.java:50-61)
    def cluster_request_param_array(self, reqs: np.ndarray, values: np.ndarray) -> np.ndarray:
        """reqs: A.PARAM_TOKEN_REQ_DTYPE (time-ordered), values: uint64 keys -> A.TOKEN_RES_DTYPE array."""
        reqs = np.ascontiguousarray(reqs, dtype=A.PARAM_TOKEN_REQ_DTYPE)
        values = np.ascontiguousarray(values, dtype=np.uint64)
        out = np.zeros(len(reqs), dtype=A.TOKEN_RES_DTYPE)
        _check(lib().sg_cluster_request_param_tokens(self.h, reqs.ctypes.data, len(reqs), values.ctypes.data,
                                                     len(values), out.ctypes.data))
        return out

    def cluster_request_param_ptr(self, req_ptr: int, n: int, values_ptr: int, n_values: int, out_ptr: int):
        """Device (or host) buffers: n A.PARAM_TOKEN_REQ_DTYPE rows at req_ptr and n_values uint64 keys at values_ptr
        -> A.TOKEN_RES_DTYPE rows at out_ptr."""
        _check(lib().sg_cluster_request_param_tokens(self.h, C.c_void_p(req_ptr), n, C.c_void_p(values_ptr), n_values,
                                                     C.c_void_p(out_ptr)))

    def cluster_request_param(self, reqs):
        """reqs: list of (ts, flow_id, acquire, [value keys]) -> list of (status, remaining, wait)."""
        arr, vals = A.param_token_arrays(reqs)
        out = self.cluster_request_param_array(arr, vals)
        return [(int(o["status"]), int(o["remaining"]), int(o["wait_in_ms"])) for o in out]

    def cluster_param_table_stats(self) -> dict:
        """sg_cluster_param_table_stats: the (flowId, value) table behind cluster_request_param.  It drops the
        values no window holds any more and grows from 2^SG_PV_LOG2 up to 2^SG_PV_MAX_LOG2 slots; a call that
        cannot fit raises SentinelError(SG_ENOMEM) with nothing changed."""
        out = (C.c_uint64 * 7)()
        k = lib().sg_cluster_param_table_stats(self.h, out, 7)
        names = ("capacity", "claimed_ub", "live_kept", "rehashes", "resizes", "rehash_us", "max_capacity")
        return {names[i]: int(out[i]) for i in range(k)}

    def cluster_param_owner_stats(self) -> dict:
        """Who decided the flow-stage requests of cluster_request_param so far (sg_cluster_param_table_stats [7..9]):
        the value-parallel owner (one lane per (flowId, value) chain), the one-lane-per-flow owner, and how many
        times a flow stayed with the latter because a call held a multi-value request of it or began before one of
        its window stamps.  SG_PTOK_VP=0 leaves every flow to the one-lane owner."""
        out = (C.c_uint64 * 10)()
        k = lib().sg_cluster_param_table_stats(self.h, out, 10)
        names = ("value_parallel_requests", "flow_lane_requests", "flows_kept_serial")
        return {names[i - 7]: int(out[i]) for i in range(7, k)}
