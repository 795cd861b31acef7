// keysweep.hip -- which candidate keys of the parameter key dictionary (pkeys.h) does the device still hold?
//
// The dictionary's entries are dropped like the reference's LRU maps drop values: a key no device structure
// holds any more can be given to another value.  A sweep (sg_param_keys_sweep, between batches) uploads the
// candidates' keys as an open-addressing table (a power of two slots, at most half full, PK_EMPTY = free, the
// candidate's index beside each key) and a zeroed bitmap of one bit per candidate; the kernels below set a
// candidate's bit when its key is
//   * a live key of a ParameterMetric map (rule maps and thread-count maps): walked from the map headers, so the
//     regions a map grew out of (k_pm_grow) do not count, and with pm_live(), so an evicted or erased key does
//     not count either -- a kept key that is not live is a leak, a dropped one that is live a wrong decision;
//   * a word of the key ring: a later EXIT with args reads its ENTRY's key there;
//   * the key of a claimed slot of the token server's (flow, value) table.
// Nothing else on the device outlives a batch with a key in it (hot items are pinned on the host).
//
// Atomics execute at the memory side and drop the line from L2, and the ring is mostly NO_KEY or repeats of
// few keys: a lane reads the mark word first and only sets a bit that is still clear (the plain read may be
// stale: then the atomic sets a set bit again).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chain.h"
#include "dev_types.h"
#include "launch.h"
#include "pmap.h"

namespace sg {

struct KsTab {
    const uint64_t* key;   // [mask + 1], PK_EMPTY = free
    const uint32_t* idx;   // candidate index of the slot's key
    uint32_t mask;
    uint32_t* marks;       // one bit per candidate
};

__device__ __forceinline__ void ks_mark(const KsTab& T, uint64_t key) {
    if (key == PK_EMPTY) return;  // (= NO_KEY: never a candidate)
    uint32_t h = (uint32_t)mix64(key) & T.mask;
    for (uint32_t probe = 0; probe <= T.mask; ++probe) {  // bounded by the table: it is never full
        const uint64_t k = T.key[h];
        if (k == PK_EMPTY) return;
        if (k == key) {
            const uint32_t i = T.idx[h], bit = 1u << (i & 31);
            if (!(T.marks[i >> 5] & bit)) atomicOr(&T.marks[i >> 5], bit);
            return;
        }
        h = (h + 1) & T.mask;
    }
}

// slot s (bucket s / 8, key s % 8) of map m
__device__ __forceinline__ void ks_slot(const KsTab& T, const PMap& m, const PBucket* __restrict__ B,
                                        const uint64_t* __restrict__ bm, uint64_t s) {
    const PBucket* b = B + m.base + (s >> 3);
    const uint64_t key = b->key[s & 7];
    if (key == PK_EMPTY) return;
    if (pm_live(m, bm + m.bm, b->stamp[s & 7])) ks_mark(T, key);
}

// The maps: a wavefront takes four consecutive maps at a time.  A new map has PM_MIN_NB = 2 buckets (16 keys) and
// most maps of a large pool stay that small, so each quarter of the wave first reads the 16 keys of one map's
// first two buckets; what a map holds beyond them (up to map_buckets(200000) buckets) the whole wave then
// walks, 64 keys a step.  A header that does not fit the pool or the rings is skipped.
#define KS_WG 256
__global__ __launch_bounds__(KS_WG) void k_ks_maps(const PMap* __restrict__ pmap, uint32_t nm,
                                                   const PBucket* __restrict__ B, uint64_t pool_nb,
                                                   const uint64_t* __restrict__ bm, uint64_t bm_words, KsTab T) {
    const uint32_t lane = threadIdx.x & 63, quad = lane >> 4, ql = lane & 15;
    const uint64_t wave = ((uint64_t)blockIdx.x * KS_WG + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * KS_WG) >> 6;
    const uint64_t ngroups = ((uint64_t)nm + 3) / 4;
    auto fits = [&](const PMap& m) {
        return m.nb >= 1 && m.base + m.nb <= pool_nb && m.rb_log2 >= 6 && m.rb_log2 < 40 &&
               m.bm + ((1ull << m.rb_log2) >> 6) <= bm_words;
    };
    for (uint64_t g = wave; g < ngroups; g += nwaves) {
        const uint64_t mine = g * 4 + quad;
        if (mine < nm) {
            const PMap m = pmap[mine];
            if (fits(m) && ql < (uint64_t)m.nb * PM_BKT) ks_slot(T, m, B, bm, ql);
        }
        for (uint32_t q = 0; q < 4; ++q) {  // (uniform over the wave)
            const uint64_t id = g * 4 + q;
            if (id >= nm) break;
            if (pmap[id].nb <= 2) continue;
            const PMap m = pmap[id];
            if (!fits(m)) continue;
            const uint64_t ns = (uint64_t)m.nb * PM_BKT;
            for (uint64_t s = 16 + lane; s < ns; s += 64) ks_slot(T, m, B, bm, s);
        }
    }
}

__global__ __launch_bounds__(KS_WG) void k_ks_ring(const uint64_t* __restrict__ ring, uint64_t n, KsTab T) {
    const uint64_t stride = (uint64_t)gridDim.x * KS_WG;
    for (uint64_t i = (uint64_t)blockIdx.x * KS_WG + threadIdx.x; i < n; i += stride) ks_mark(T, ring[i]);
}

__global__ __launch_bounds__(KS_WG) void k_ks_pval(const PVal* __restrict__ tab, uint64_t n, KsTab T) {
    const uint64_t stride = (uint64_t)gridDim.x * KS_WG;
    for (uint64_t i = (uint64_t)blockIdx.x * KS_WG + threadIdx.x; i < n; i += stride)
        if (tab[i].flow != PV_EMPTY) ks_mark(T, tab[i].key);
}

static inline uint32_t ks_grid(uint64_t items) {  // enough workgroups to fill the chip, no more than the work
    const uint64_t wg = (items + KS_WG - 1) / KS_WG;
    return (uint32_t)(wg < 1 ? 1 : wg > 4096 ? 4096 : wg);
}

// The three scans on st; ev (optional): four events recorded before, between and after them (their durations
// are the sweep's per-scan timings).  Null structures (no param rules, no cluster param rules) are skipped.
hipError_t launch_keysweep(const PMap* pmap, uint32_t nm, const PBucket* pbkt, uint64_t pool_nb, const uint64_t* pbm,
                           uint64_t bm_words, const uint64_t* key_ring, uint64_t ring_n, const PVal* pvtab,
                           uint64_t pv_n, const uint64_t* tkey, const uint32_t* tidx, uint32_t tmask, uint32_t* marks,
                           hipEvent_t* ev, hipStream_t st) {
    KsTab T;
    T.key = tkey; T.idx = tidx; T.mask = tmask; T.marks = marks;
    hipError_t rc;
    if (ev && (rc = hipEventRecord(ev[0], st)) != hipSuccess) return rc;
    if (pmap && nm && pbkt && pbm)  // 64 maps a workgroup
        hipLaunchKernelGGL(k_ks_maps, dim3(ks_grid(((uint64_t)nm + 3) / 4 * 64)), dim3(KS_WG), 0, st, pmap, nm, pbkt,
                           pool_nb, pbm, bm_words, T);
    if (ev && (rc = hipEventRecord(ev[1], st)) != hipSuccess) return rc;
    if (key_ring && ring_n)
        hipLaunchKernelGGL(k_ks_ring, dim3(ks_grid(ring_n)), dim3(KS_WG), 0, st, key_ring, ring_n, T);
    if (ev && (rc = hipEventRecord(ev[2], st)) != hipSuccess) return rc;
    if (pvtab && pv_n) hipLaunchKernelGGL(k_ks_pval, dim3(ks_grid(pv_n)), dim3(KS_WG), 0, st, pvtab, pv_n, T);
    if (ev && (rc = hipEventRecord(ev[3], st)) != hipSuccess) return rc;
    return hipGetLastError();
}

} // namespace sg
