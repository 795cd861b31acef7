// ptok.h -- the value-parallel owner of the token server's param flows: the walk of one (flow, value) chain, the
// flow's stamp merge and the eligibility predicate, shared by the kernels of cluster.hip (k_ptok_elig, k_ptok_keys,
// k_ptok_chain) and tests/ptok_host.cpp, which runs them next to a literal restatement of k_ptok_flow's loop.
//
// Reference: ClusterParamFlowChecker.acquireClusterToken (csrv/flow/ClusterParamFlowChecker.java:42-88) reads
// ClusterParamMetric.getSum(value) (ClusterParamMetric.java:53-85) after metric.currentWindow(), and adds the
// acquire count to the current bucket's map on a pass.
//
// Why a value can be walked alone.  k_ptok_flow reads cnt[j] of a value only while pv.ws[j] == F.fws[j] and
// now - F.fws[j] <= interval, after pf_current(now).  Let every stamp of the flow be <= now at the flow's first
// flow-stage request of a call (pt_clock_ok); the requests of a call are ordered by ts, so this then holds at every
// later request too (a stamp written at now' is <= now' <= now).  Then
//   - ws(now) = now - now % wlen is >= the stamp of slot idx(now) (that stamp is <= now, of the same slot, hence a
//     multiple of wlen at most ws(now)), so after pf_current(now) the flow's stamp of idx(now) is exactly ws(now);
//   - a count stamped w in slot j is read at now iff w >= 0 and now < w + interval.  If: the flow's stamp of j is a
//     copy source of w and only moves forward in steps of the interval; a larger one w' >= w + interval would be
//     <= now, contradicting now < w + interval, so the stamps are equal, and now - w < interval is not deprecated.
//     Only if: at now >= w + interval either the flow's stamp moved (unequal), or it is still w and then
//     now - w > interval (deprecated), or now == w + interval, where idx(now) == j and pf_current just reset it.
// So a value's verdicts follow from its own earlier passes, its threshold, interval and n alone, and the value's
// stamps written by the walk (ws(now) at idx(now) on a pass) equal the flow's: pvtab.h's dead-slot rule holds.
// The flow's final stamps are the slot-wise maximum of the old ones and ws(ts) at idx(ts) over every request of
// the flow that reached the flow stage, blocked ones included (pf_current runs before the check).
//
// Two things couple the chains of a flow, and such flows stay with k_ptok_flow for the call: a request of more
// than one value (all-or-nothing over its values), and a first flow-stage ts below one of the flow's stamps (the
// clock went back between calls: the param path orders requests inside one call only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_types.h"

#define PT_FN __host__ __device__

namespace sg {

// why a flow stays with k_ptok_flow for a call (bits of its word in the per-call flag array)
#define PT_MULTI 1u   // one of its requests lists more than one value
#define PT_CLOCK 2u   // its first flow-stage request lies before one of its window stamps

struct PtWin {
    int idx;
    int64_t ws;
};
PT_FN inline PtWin pt_window(int32_t n, int32_t interval, int64_t now) {  // pf_current's slot and window start
    const int64_t wlen = interval / n;
    PtWin w;
    w.idx = (int)((now / wlen) % n);
    w.ws = now - now % wlen;
    return w;
}
// the flow's stamps allow the walk: none lies after the first flow-stage request of the call
PT_FN inline bool pt_clock_ok(const PFlow& F, int64_t first_ts) {
    for (int j = 0; j < F.n && j < CP_MAXN; ++j)
        if (F.fws[j] > first_ts) return false;
    return true;
}
// getRawThreshold and the AVG_LOCAL factor: the exclusive item's count, else rule.count
PT_FN inline double pt_threshold(const PFlow& F, const PHot* hot, uint64_t key) {
    double raw = F.count;
    for (uint32_t h = 0; h < F.nhot; ++h)
        if (hot[F.hoff + h].key == key) { raw = (double)hot[F.hoff + h].count; break; }
    return F.thr_type == SG_CLUSTER_THRESHOLD_GLOBAL ? raw : raw * (double)F.connected;
}

struct PtChain {  // a value's PVal stamps and counts, private to the chain's lane for the call
    int64_t ws[CP_MAXN];
    int64_t cnt[CP_MAXN];
};
// One request of the chain: k_ptok_flow's `next` (the caller blocks on next < 0, else remaining = (int) next),
// with the pass already added when it is not negative.
PT_FN inline double pt_step(PtChain& c, int32_t n, int32_t interval, double isec, double thr, int64_t now,
                            int32_t acquire) {
    int64_t sum = 0;
    for (int j = 0; j < n; ++j)
        if (c.ws[j] >= 0 && now < c.ws[j] + interval) sum += c.cnt[j];
    const double next = thr - (double)sum / isec - (double)acquire;
    if (!(next < 0)) {
        const PtWin w = pt_window(n, interval, now);
        if (c.ws[w.idx] != w.ws) { c.ws[w.idx] = w.ws; c.cnt[w.idx] = 0; }
        c.cnt[w.idx] += acquire;
    }
    return next;
}
// The stamp merge, one flow-stage request at a time (the kernel does the same maximum with an atomic).
PT_FN inline void pt_merge(PFlow& F, int64_t ts) {
    const PtWin w = pt_window(F.n, F.interval, ts);
    if (F.fws[w.idx] < w.ws) F.fws[w.idx] = w.ws;
}

}  // namespace sg
