"""The decide stage's chains from a rocprofv3 --kernel-trace CSV of a pipelined bench.py run: per batch, on the device
clock, the start and end of k_lite, k_jac<1>, k_jac<8>, k_jac<4>, k_fill and k_post_w relative to the batch's
k_resolve, with the hardware queue of each; then the medians, and how long k_jac<1> ends after the later of
k_jac<8> and k_jac<4> (the margin by which J1's chain, not an owner's, bounds the stage).
tools/timeline.py lists every kernel of a batch from its k_rs_first on (the group stage's clock, which in a pipelined
run is another batch's than the decide kernels beside it) and tools/rocpd_timeline.py one batch of a rocpd database;
neither gives medians over batches or the owners' ends against each other, which is all this one does.
usage: python tools/decide_chains.py kernel_trace.csv [batches to skip at the front, default 2]"""
import csv
import statistics
import sys

NAMES = ["k_lite<false>", "k_jac<1,", "k_jac<8,", "k_jac<4,", "k_fill", "k_post_w"]


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    skip = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    ks = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].replace("void ", "").replace("sg::", ""),
                 r.get("Queue_Id", "?")) for r in rows)
    # a decide stage: from a k_resolve to the k_post_w that follows it (the next batch's group kernels lie between)
    starts = [i for i, k in enumerate(ks) if k[2].startswith("k_resolve")]
    per = {n: [] for n in NAMES}
    margin = []
    for bi, i0 in enumerate(starts):
        t0 = ks[i0][0]
        got = {}
        for s, e, n, q in ks[i0:]:
            for key in NAMES:
                if n.startswith(key) and key not in got:
                    got[key] = (s - t0, e - t0, q)
            if n.startswith("k_post_w"):
                break
        if len(got) < len(NAMES) or bi < skip:
            continue
        print("batch %2d  " % bi + "  ".join("%s q%s %.3f-%.3f" % (k.rstrip(",").replace("<false>", ""), got[k][2], got[k][0] / 1e6,
                                                                got[k][1] / 1e6) for k in NAMES))
        for k in NAMES:
            per[k].append(got[k])
        margin.append(got["k_jac<1,"][1] - max(got["k_jac<8,"][1], got["k_jac<4,"][1]))
    if not margin:
        sys.exit("no complete decide stage found")
    print("batches: %d (ms after the batch's k_resolve)" % len(margin))
    for k in NAMES:
        st, en = [g[0] / 1e6 for g in per[k]], [g[1] / 1e6 for g in per[k]]
        du = [b - a for a, b in zip(st, en)]
        print("  %-14s start median %.3f  end median %.3f  dur median %.3f (min %.3f max %.3f)" % (
            k.rstrip(","), statistics.median(st), statistics.median(en), statistics.median(du), min(du), max(du)))
    m = [x / 1e6 for x in margin]
    print("  k_jac<1> end - max(k_jac<8> end, k_jac<4> end): median %.3f ms (min %.3f max %.3f)" % (
        statistics.median(m), min(m), max(m)))
    last = {k: statistics.median([g[1] / 1e6 for g in per[k]]) for k in NAMES[:4]}
    print("  last owner to end (median): %s at %.3f ms" % (max(last, key=last.get).rstrip(","), max(last.values())))


if __name__ == "__main__":
    main()
