// cmetrics.hip -- the token server's cluster metrics (sg_cluster_metrics): what cluster/server/metricList reads.
//
// Reference (csrv/ = sentinel-cluster/sentinel-cluster-server-default/.../cluster/):
//   ClusterMetricNodeGenerator   csrv/flow/statistic/ClusterMetricNodeGenerator.java:39-105
//   ClusterMetric.getAvg         csrv/flow/statistic/metric/ClusterMetric.java:53-72
//   ClusterParamMetric.getTopValues   csrv/flow/statistic/metric/ClusterParamMetric.java:91-133
//
// A read-back: every kernel here reads CFlow / CBkt / PFlow / PVal and writes the call's own scratch only.  The
// reset that the reference's currentWindow() would make is applied to a copy (the copy rule, cm_flow_row and
// cm_param_mask below).
//
//   k_cm_flow     one lane per CFlow: the row's pass / block QPS under the copy rule;
//   k_cm_pmask    one lane per PFlow: the buckets of the flow that count at `now` as a bit mask, and the row's head;
//   k_cm_scan     grid-stride over the value table, one lane a slot: an empty slot costs its 16-byte head, a claimed
//                 one the stamps of the flow's counting buckets, a live one those buckets' counts; the slots with a
//                 sum > 0 are appended to a compact candidate list (flow index, sum, key), one atomic a wave;
//   (the stable radix pair sort of kernels.hip groups the candidates by flow index)
//   k_cm_bounds   the flows' first sorted positions, as k_tok_bounds takes them;
//   k_cm_chunks   a flow's segment is cut into chunks of at most CM_CHUNK candidates (their counts, then a scan);
//   k_cm_select   one wave per chunk: every lane streams its share into a sorted list of SG_CLUSTER_TOP_MAX entries
//                 in registers, the wave merges the lanes' lists by rounds of an arg-max over the list heads and
//                 leaves one partial list;
//   k_cm_merge    one wave per param flow: the same selection over the flow's partial lists, into the row.
// The order is total -- (sum descending, key ascending, unsigned), and a flow's keys are distinct -- so the rows do
// not depend on the order in which the scan appended, on the table's capacity or on where a value's slot lies.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sentinel_gpu.h"
#include "cmwin.h"
#include "dev_types.h"
#include "launch.h"

namespace sg {

#define CM_CHUNK 4096u  // candidates of one flow per select wave
#define CM_TOP SG_CLUSTER_TOP_MAX
static_assert(sizeof(PVal) == 272 && sizeof(PVal) % sizeof(uint4) == 0, "k_cm_scan reads a slot's head as one uint4");
static_assert(sizeof(sg_cluster_metric) == 184, "sg_cluster_metric layout");

// ---- the copy rule
// FLOW: sums of PASS and BLOCK over the buckets that count at now, bucket i = (now / w) % n reset on a copy
__device__ __forceinline__ void cm_flow_row(const CFlow& F, const CBkt* __restrict__ b, int64_t now, int64_t* pass,
                                            int64_t* block) {
    const int64_t w = F.interval / F.n;
    const int cur = (int)((now / w) % F.n);
    const int64_t ws = now - now % w;
    int64_t sp = 0, sb = 0;
    for (int j = 0; j < F.n; ++j) {
        int64_t start = b[j].ws, p = b[j].c[CF_PASS], k = b[j].c[CF_BLOCK];
        if (j == cur && start >= 0 && start < ws) {  // resetWindowTo on the copy: empty, plus the pending occupy transfer
            start = ws;
            p = F.has_occ ? F.occ_pass : 0;
            k = 0;
        }
        if (CM_SKIPPED(start, now, F.interval)) continue;
        sp += p;
        sb += k;
    }
    *pass = sp;
    *block = sb;
}
// PARAM: bit j set iff bucket j of the flow counts at now (bucket i with a start < ws is emptied on the copy)
__device__ __forceinline__ uint32_t cm_param_mask(const PFlow& F, int64_t now) {
    const int n = F.n < CP_MAXN ? F.n : CP_MAXN;
    const int64_t w = F.interval / F.n;
    const int cur = (int)((now / w) % F.n);
    const int64_t ws = now - now % w;
    uint32_t m = 0;
    for (int j = 0; j < n; ++j) {
        const int64_t start = F.fws[j];
        if (j == cur && start < ws) continue;
        if (!CM_SKIPPED(start, now, F.interval)) m |= 1u << j;
    }
    return m;
}

__device__ __forceinline__ void cm_row_head(sg_cluster_metric& r, int64_t now, int64_t flow_id, uint32_t kind) {
    r.timestamp = now;
    r.flow_id = flow_id;
    r.res_id = 0xFFFFFFFFu;  // (the host knows the rule's resource)
    r.kind = kind;
    r.pass_qps = 0.0;
    r.block_qps = 0.0;
    r.rt = 0;
    r.n_top = 0;
    r.reserved = 0;
#pragma unroll
    for (int k = 0; k < CM_TOP; ++k) { r.top_key[k] = 0; r.top_qps[k] = 0.0; }
}

__global__ __launch_bounds__(256) void k_cm_flow(const CFlow* __restrict__ flows, uint32_t nflows,
                                                 const CBkt* __restrict__ bkts, int64_t now,
                                                 sg_cluster_metric* __restrict__ rows) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nflows) return;
    const CFlow F = flows[f];
    int64_t pass, block;
    cm_flow_row(F, bkts + F.boff, now, &pass, &block);
    sg_cluster_metric r;
    cm_row_head(r, now, F.flow_id, SG_CM_FLOW);
    const double isec = F.interval / 1000.0;  // LeapArray.getIntervalInSecond
    r.pass_qps = (double)pass / isec;
    r.block_qps = (double)block / isec;
    rows[f] = r;
}

__global__ __launch_bounds__(256) void k_cm_pmask(const PFlow* __restrict__ flows, uint32_t nflows, int64_t now,
                                                  uint32_t* __restrict__ mask, sg_cluster_metric* __restrict__ rows) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nflows) return;
    mask[f] = cm_param_mask(flows[f], now);
    sg_cluster_metric r;
    cm_row_head(r, now, flows[f].flow_id, SG_CM_PARAM);
    rows[f] = r;
}

// cnt[0] += candidates (they are written while their index is below cap; the host reads cnt[0] and refuses more)
__global__ __launch_bounds__(256) void k_cm_scan(const PVal* __restrict__ tab, uint64_t n_slots,
                                                 const PFlow* __restrict__ flows, uint32_t nflows,
                                                 const uint32_t* __restrict__ mask, uint32_t* __restrict__ cflow,
                                                 uint32_t* __restrict__ cidx, int64_t* __restrict__ csum,
                                                 uint64_t* __restrict__ ckey, uint32_t cap, uint32_t* __restrict__ cnt) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n_slots; base += stride) {  // (uniform in a wave)
        const uint64_t i = base + threadIdx.x;
        int64_t sum = 0;
        uint64_t key = 0;
        uint32_t f = PV_EMPTY;
        if (i < n_slots) {
            const uint4 head = *reinterpret_cast<const uint4*>(&tab[i]);  // key, flow, pad
            f = head.z;
            if (f != PV_EMPTY && f < nflows) {
                key = (uint64_t)head.x | ((uint64_t)head.y << 32);
                uint32_t m = mask[f];
                const PFlow* F = &flows[f];
                while (m) {
                    const int j = __ffs((int)m) - 1;
                    m &= m - 1;
                    if (tab[i].ws[j] == F->fws[j]) sum += tab[i].cnt[j];
                }
            }
        }
        const bool has = sum > 0;
        const uint64_t b = __ballot(has);
        if (!b) continue;
        const int leader = __ffsll((long long)b) - 1;
        uint32_t at = 0;
        if ((int)lane == leader) at = atomicAdd(&cnt[0], (uint32_t)__popcll(b));
        at = __shfl(at, leader, 64) + (uint32_t)__popcll(b & lt);
        if (has && at < cap) {
            cflow[at] = f;
            cidx[at] = at;
            csum[at] = sum;
            ckey[at] = key;
        }
    }
}

// bounds[f] = the first sorted position of flow f (lower_bound of the keys), f = 0 .. nflows
__global__ __launch_bounds__(256) void k_cm_bounds(const uint32_t* __restrict__ skeys, uint32_t n, uint32_t nflows,
                                                   uint32_t* __restrict__ bounds) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    const int64_t prev = i == 0 ? -1 : (int64_t)skeys[i - 1];
    const int64_t k = i == n ? (int64_t)nflows : (int64_t)skeys[i];
    const int64_t top = k < (int64_t)nflows ? k : (int64_t)nflows;
    for (int64_t f = prev + 1; f <= top; ++f) bounds[f] = (uint32_t)i;
}
// nch[f] = chunks of flow f, f < nflows; nch[nflows] = 0 (the scan over nflows + 1 words leaves the total there)
__global__ __launch_bounds__(256) void k_cm_chunks(const uint32_t* __restrict__ bounds, uint32_t nflows,
                                                   uint32_t* __restrict__ nch) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f > nflows) return;
    nch[f] = f < nflows ? (bounds[f + 1] - bounds[f] + CM_CHUNK - 1) / CM_CHUNK : 0u;
}

// ---- the selection: (sum, key) entries, sum == 0: none.  a before b: larger sum, then smaller key (unsigned)
struct CmTop {
    int64_t s[CM_TOP];
    uint64_t k[CM_TOP];
};
__device__ __forceinline__ bool cm_before(int64_t sa, uint64_t ka, int64_t sb, uint64_t kb) {
    return sa > sb || (sa == sb && ka < kb);
}
__device__ __forceinline__ void cm_clear(CmTop& L) {
#pragma unroll
    for (int k = 0; k < CM_TOP; ++k) { L.s[k] = 0; L.k[k] = ~0ull; }
}
__device__ __forceinline__ void cm_insert(CmTop& L, int64_t s, uint64_t key) {
    if (!cm_before(s, key, L.s[CM_TOP - 1], L.k[CM_TOP - 1])) return;
    L.s[CM_TOP - 1] = s;
    L.k[CM_TOP - 1] = key;
#pragma unroll
    for (int k = CM_TOP - 1; k > 0; --k) {
        const bool sw = cm_before(L.s[k], L.k[k], L.s[k - 1], L.k[k - 1]);
        const int64_t ts = L.s[k];
        const uint64_t tk = L.k[k];
        L.s[k] = sw ? L.s[k - 1] : ts;
        L.k[k] = sw ? L.k[k - 1] : tk;
        L.s[k - 1] = sw ? ts : L.s[k - 1];
        L.k[k - 1] = sw ? tk : L.k[k - 1];
    }
}
// The wave's first top_n entries over all lanes' lists, in order, into out (every lane gets them): a round takes
// the arg-max over the list heads and the lane that owns it moves its list up (entries are distinct: one owner).
__device__ __forceinline__ void cm_wave_merge(CmTop& L, uint32_t top_n, CmTop& out) {
    cm_clear(out);
#pragma unroll
    for (int r = 0; r < CM_TOP; ++r) {
        if ((uint32_t)r >= top_n) break;  // (uniform)
        int64_t bs = L.s[0];
        uint64_t bk = L.k[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int64_t ys = __shfl_xor(bs, o, 64);
            const uint64_t yk = __shfl_xor(bk, o, 64);
            const bool take = cm_before(ys, yk, bs, bk);
            bs = take ? ys : bs;
            bk = take ? yk : bk;
        }
        out.s[r] = bs;
        out.k[r] = bk;
        if (bs > 0 && L.s[0] == bs && L.k[0] == bk) {
#pragma unroll
            for (int k = 0; k + 1 < CM_TOP; ++k) { L.s[k] = L.s[k + 1]; L.k[k] = L.k[k + 1]; }
            L.s[CM_TOP - 1] = 0;
            L.k[CM_TOP - 1] = ~0ull;
        }
    }
}

// one wave per chunk; coff[f] = the first chunk of flow f, coff[nflows] = chunks in all
__global__ __launch_bounds__(64) void k_cm_select(const uint32_t* __restrict__ sv, const uint32_t* __restrict__ bounds,
                                                  const uint32_t* __restrict__ coff, uint32_t nflows,
                                                  const int64_t* __restrict__ csum, const uint64_t* __restrict__ ckey,
                                                  uint32_t top_n, int64_t* __restrict__ psum,
                                                  uint64_t* __restrict__ pkey) {
    const uint32_t c = blockIdx.x, lane = threadIdx.x;
    if (c >= coff[nflows]) return;
    uint32_t lo = 0, hi = nflows;  // the last f with coff[f] <= c (its coff[f + 1] > c: it has this chunk)
    while (lo + 1 < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (coff[mid] <= c) lo = mid; else hi = mid;
    }
    const uint32_t f = lo;
    const uint32_t p0 = bounds[f] + (c - coff[f]) * CM_CHUNK;
    const uint32_t p1 = min(p0 + CM_CHUNK, bounds[f + 1]);
    CmTop L, out;
    cm_clear(L);
    for (uint32_t p = p0 + lane; p < p1; p += 64) {
        const uint32_t ci = sv[p];
        cm_insert(L, csum[ci], ckey[ci]);
    }
    cm_wave_merge(L, top_n, out);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < CM_TOP; ++k) { psum[(uint64_t)c * CM_TOP + k] = out.s[k]; pkey[(uint64_t)c * CM_TOP + k] = out.k[k]; }
    }
}

// one wave per param flow: its partial lists -> the row
__global__ __launch_bounds__(64) void k_cm_merge(const uint32_t* __restrict__ coff, const PFlow* __restrict__ flows,
                                                 uint32_t nflows, const int64_t* __restrict__ psum,
                                                 const uint64_t* __restrict__ pkey, uint32_t top_n,
                                                 sg_cluster_metric* __restrict__ rows) {
    const uint32_t f = blockIdx.x, lane = threadIdx.x;
    if (f >= nflows) return;
    const uint64_t e0 = (uint64_t)coff[f] * CM_TOP, e1 = (uint64_t)coff[f + 1] * CM_TOP;
    if (e0 == e1) return;  // (the row is zero already)
    CmTop L, out;
    cm_clear(L);
    for (uint64_t q = e0 + lane; q < e1; q += 64) {
        const int64_t s = psum[q];
        if (s > 0) cm_insert(L, s, pkey[q]);
    }
    cm_wave_merge(L, top_n, out);
    if (lane == 0) {
        const double isec = flows[f].interval / 1000.0;  // LeapArray.getIntervalInSecond
        uint32_t nt = 0;
#pragma unroll
        for (int k = 0; k < CM_TOP; ++k) {
            if (out.s[k] > 0) {
                rows[f].top_key[k] = out.k[k];
                rows[f].top_qps[k] = (double)out.s[k] / isec;
                ++nt;
            }
        }
        rows[f].n_top = nt;
    }
}

uint32_t cm_chunk() { return CM_CHUNK; }

// The FLOW rows (rows[0, ncf)) and the param flows' masks and row heads (prows[0, npf)).
hipError_t launch_cm_rows(const CFlow* cflows, uint32_t ncf, const CBkt* bkts, const PFlow* pflows, uint32_t npf,
                          int64_t now, uint32_t* mask, sg_cluster_metric* rows, sg_cluster_metric* prows,
                          hipStream_t st) {
    if (ncf) hipLaunchKernelGGL(k_cm_flow, dim3((ncf + 255) / 256), dim3(256), 0, st, cflows, ncf, bkts, now, rows);
    if (npf) hipLaunchKernelGGL(k_cm_pmask, dim3((npf + 255) / 256), dim3(256), 0, st, pflows, npf, now, mask, prows);
    return hipGetLastError();
}
// cnt: one word, zeroed here; the candidate arrays hold cap entries
hipError_t launch_cm_scan(const PVal* tab, uint64_t n_slots, const PFlow* flows, uint32_t nflows, const uint32_t* mask,
                          uint32_t* cflow, uint32_t* cidx, int64_t* csum, uint64_t* ckey, uint32_t cap, uint32_t* cnt,
                          hipStream_t st) {
    hipError_t rc = hipMemsetAsync(cnt, 0, 4, st);
    if (rc != hipSuccess) return rc;
    if (!n_slots || !nflows) return hipSuccess;
    const uint64_t wg = (n_slots + 255) / 256;
    hipLaunchKernelGGL(k_cm_scan, dim3((uint32_t)(wg > 8192 ? 8192 : wg)), dim3(256), 0, st, tab, n_slots, flows, nflows,
                       mask, cflow, cidx, csum, ckey, cap, cnt);
    return hipGetLastError();
}
// skeys / svals: the n candidates sorted by flow index.  bounds, nch, coff: nflows + 2 words each; psum / pkey:
// CM_TOP entries for each of n / CM_CHUNK + nflows chunks.  ev[0] is recorded between the chunk table and the select.
hipError_t launch_cm_select(const uint32_t* skeys, const uint32_t* svals, uint32_t n, const PFlow* flows, uint32_t nflows,
                            const int64_t* csum, const uint64_t* ckey, uint32_t top_n, uint32_t* bounds, uint32_t* nch,
                            uint32_t* coff, uint32_t* part, int64_t* psum, uint64_t* pkey, sg_cluster_metric* prows,
                            hipEvent_t* ev, hipStream_t st) {
    if (!n || !nflows) return hipSuccess;
    hipLaunchKernelGGL(k_cm_bounds, dim3((n + 256) / 256), dim3(256), 0, st, skeys, n, nflows, bounds);
    hipLaunchKernelGGL(k_cm_chunks, dim3((nflows + 256) / 256), dim3(256), 0, st, bounds, nflows, nch);
    hipError_t rc = launch_scan(nch, coff, (uint64_t)nflows + 1, part, nullptr, st);
    if (rc == hipSuccess) rc = hipEventRecord(ev[0], st);
    if (rc != hipSuccess) return rc;
    const uint32_t max_chunks = n / CM_CHUNK + nflows;  // sum of ceil(len / CM_CHUNK) over the non-empty flows, at most
    hipLaunchKernelGGL(k_cm_select, dim3(max_chunks), dim3(64), 0, st, svals, bounds, coff, nflows, csum, ckey, top_n,
                       psum, pkey);
    if ((rc = hipEventRecord(ev[1], st)) != hipSuccess) return rc;
    hipLaunchKernelGGL(k_cm_merge, dim3(nflows), dim3(64), 0, st, coff, flows, nflows, psum, pkey, top_n, prows);
    return hipGetLastError();
}

}  // namespace sg
