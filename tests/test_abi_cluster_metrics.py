"""sg_cluster_metric has the layout the bindings assume: the C compiler's sizeof and offsets (tests/abi_cluster_metric.c)
against the ctypes struct and the numpy dtype of sentinel_amd/_abi.py.  CPU-only."""
import ctypes as C
import os
import subprocess

from sentinel_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cluster_metric_layout_matches_header(tmp_path):
    exe = tmp_path / "abi_cluster_metric"
    subprocess.run(["gcc", "-O0", "-o", str(exe), os.path.join(ROOT, "tests", "abi_cluster_metric.c")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in out.splitlines())}
    assert got["sg_cluster_metric"] == C.sizeof(A.SgClusterMetric) == A.CLUSTER_METRIC_DTYPE.itemsize
    for name in ("res_id", "pass_qps", "n_top", "top_key", "top_qps"):
        assert got["cm." + name] == getattr(A.SgClusterMetric, name).offset == A.CLUSTER_METRIC_DTYPE.fields[name][1], name
    assert got["SG_CLUSTER_TOP_MAX"] == A.CLUSTER_TOP_MAX == A.CLUSTER_METRIC_DTYPE.fields["top_key"][0].shape[0]
    assert got["SG_CM_PARAM"] == A.CM_PARAM == 1 and A.CM_FLOW == 0
