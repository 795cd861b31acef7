// inbound.hip -- the global inbound node (Constants.ENTRY_NODE) brought up to date from a batch's verdicts.
//
// StatisticSlot counts every EntryType.IN entry and its exit twice: on the resource's ClusterNode and on one global
// node (StatisticSlot.java:72-76, 89-92, 107-110, 158-161).  Nothing the chain decides reads that node (the SystemSlot
// check stays with the caller), so it is a pure reduction over the committed verdicts, run after every owner of the
// batch has finished -- and one that every inbound event of the batch takes part in: 62 bucket slots (2 of the second
// window, 60 of the minute window) instead of aux.hip's node per (resource, origin).
//
// The rule per event is aux.h stat_what's, the merge rule aux.hip's: per bucket slot the batch leaves the latest
// window W any of its events falls in, holding the sums of the events of W (LeapArray.currentWindow resets a bucket to
// a later window in place); "a later window replaces, the same window adds" is associative and commutative, so the
// records -- which are in resource order, not in time order -- can be cut anywhere:
//   * k_inb_tiles  : a grid-stride walk over tiles of INB_TILE records.  A workgroup keeps the 62 slots in LDS (window
//                    index relative to the batch, pass, block, success, rt, min rt), merges a tile in two phases (the
//                    latest window of every slot, then the sums of that window; a thread first adds up its own runs of
//                    equal window and kind, and adds them to one of 16 copies of the sums), and folds the tile's 32-bit
//                    sums into 64-bit accumulators that thread i keeps for slot i.  It leaves one InbPart and its
//                    thread-count delta.
//   * k_inb_commit : one workgroup merges the partials the same way (maximum and sums in registers, the loads of
//                    eight partials in flight: the merge is bound by load latency) and commits the 62 slots as
//                    aux_commit does: a later window resets the bucket (min rt = statistic_max_rt), the same window
//                    adds, an older one is dropped as LeapArray.currentWindow drops it.
// Exception and occupied pass stay 0 and the borrow ring stays empty: nothing in the reference adds to them here.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aux.h"
#include "launch.h"

using namespace sg;

#define INB_EPT (INB_TILE / 256)  // records a thread holds of a tile

// The tile's sums are kept in INB_COPIES copies, a lane adding to copy (lane & 15): nearly every lane of a wave adds
// to the same one or two windows, and LDS atomics on one address are served one lane at a time.
#define INB_COPIES 16
struct InbLds {
    int32_t W[64];
    uint32_t s[4][64][INB_COPIES];  // pass, block, success, rt
    uint32_t minrt[64][INB_COPIES];
    int32_t thread;
    uint32_t visited, updates;
};

// the minute-window slot of relative second si (m0 = the batch's base second mod 60)
__device__ __forceinline__ uint32_t inb_mslot(uint32_t m0, uint32_t si) { return 2u + (m0 + si % 60u) % 60u; }

// a thread's run of `what` updates in window wi into the tile's sums (phase 2: the windows are final)
__device__ __forceinline__ void inb_flush(InbLds& L, uint32_t m0, uint32_t what, int32_t wi, uint32_t cnt, uint32_t rt,
                                          uint32_t mn) {
    if (wi < 0) return;
    const uint32_t p = (uint32_t)wi & 1u, si = (uint32_t)wi >> 1, m = inb_mslot(m0, si);
    const bool in_s = L.W[p] == wi, in_m = L.W[m] == (int32_t)si;
    const uint32_t c = what == AW_PASS ? 0u : what == AW_BLOCK ? 1u : 2u, k = threadIdx.x & (INB_COPIES - 1);
    if (in_s && cnt) atomicAdd(&L.s[c][p][k], cnt);
    if (in_m && cnt) atomicAdd(&L.s[c][m][k], cnt);
    if (what != AW_EXIT) return;
    if (in_s) { if (rt) atomicAdd(&L.s[3][p][k], rt); atomicMin(&L.minrt[p][k], mn); }
    if (in_m) { if (rt) atomicAdd(&L.s[3][m][k], rt); atomicMin(&L.minrt[m][k], mn); }
}

__global__ __launch_bounds__(256) void k_inb_tiles(const SEv* __restrict__ recs, const uint32_t* __restrict__ dec,
                                                   uint32_t n, const sg_event* __restrict__ ev,
                                                   const uint32_t* __restrict__ vals, const NodeInfo* __restrict__ info,
                                                   const sg_event_ext* __restrict__ ext, uint32_t max_ctx,
                                                   int32_t switch_on, int64_t t0, InbPart* __restrict__ part) {
    __shared__ InbLds L;
    const uint32_t t = threadIdx.x;
    // windows relative to an even 500 ms index at or before t0 (a relative index keeps the bucket's parity, and the
    // second of 500 ms index w is w >> 1)
    const int64_t b500 = (t0 / 500) & ~1ll;
    const uint32_t off0 = (uint32_t)(t0 - b500 * 500);  // < 1000: dt + off0 < 2^32
    const uint32_t m0 = (uint32_t)((b500 / 2) % 60);
    if (t < 64) L.W[t] = -1;
    for (uint32_t i = t; i < 4u * 64u * INB_COPIES; i += 256u) (&L.s[0][0][0])[i] = 0;
    for (uint32_t i = t; i < 64u * INB_COPIES; i += 256u) (&L.minrt[0][0])[i] = 0xFFFFFFFFu;
    if (t == 0) { L.thread = 0; L.visited = 0; L.updates = 0; }
    // slot t's 64-bit accumulators (t < INB_SLOTS)
    int32_t AW = -1;
    uint64_t A0 = 0, A1 = 0, A2 = 0, A3 = 0;
    uint32_t AM = 0xFFFFFFFFu;
    int32_t dthread = 0;
    uint32_t nupd = 0, nvis = 0;
    __syncthreads();
    const uint32_t ntile = (n + INB_TILE - 1) / INB_TILE;
    for (uint32_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const uint32_t base = tile * INB_TILE;
        uint32_t wh[INB_EPT], cz[INB_EPT];
        int32_t wi[INB_EPT];
        // ---- the tile's updates; phase 1: the latest window of every slot
#pragma unroll
        for (int j = 0; j < INB_EPT; ++j) {
            const uint32_t p = base + (uint32_t)j * 256u + t;
            wh[j] = AW_NONE;
            cz[j] = 0;
            wi[j] = 0;
            if (p >= n) continue;
            ++nvis;
            const SEv r = recs[p];
            if (r.flags & SG_F_ENTRY_OUT) continue;  // EntryType.OUT: the ClusterNode alone
            if (r.kind == SG_EV_EXIT && r.code == RC_BATCH && r.x >= n) continue;  // (never: a position of this batch)
            // the rare case, an EXIT naming no ENTRY: effective iff its resource has a chain -- the resource from the
            // submitted event (a RELATE component's segment holds several), a NullContext has none
            bool chain = false;
            if (r.kind == SG_EV_EXIT && r.code == RC_NONE && switch_on != 0) {
                const uint32_t oi = vals[p] & 0x7FFFFFFFu;
                if (oi < n && !(ext && ext[oi].context_id > max_ctx)) chain = (info[ev[oi].res_id].flags & NI_CHAIN) != 0;
            }
            uint32_t tag;
            const uint32_t w = stat_what(r, p, recs, dec, chain, &tag);
            if (w == AW_NONE) continue;
            ++nupd;
            if (w == AW_PASS || w == AW_WAIT) ++dthread;
            else if (w == AW_EXIT) --dthread;
            if (w == AW_WAIT) continue;  // PriorityWaitException: the thread alone (StatisticSlot.java:82-92)
            const uint32_t rel = (uint32_t)r.dt + off0;
            const int32_t x = (int32_t)(rel / 500u);
            wh[j] = w;
            wi[j] = x;
            cz[j] = (uint32_t)r.cnt | ((uint32_t)r.rt << 16);
            const uint32_t si = (uint32_t)x >> 1, m = inb_mslot(m0, si);
            if (x > L.W[x & 1]) atomicMax(&L.W[x & 1], x);
            if ((int32_t)si > L.W[m]) atomicMax(&L.W[m], (int32_t)si);
        }
        __syncthreads();
        // ---- phase 2: the sums of the events in those windows; a thread adds up its runs of one kind and window first
        {
            int32_t rw[3] = {-1, -1, -1};  // run per kind (pass, block, exit): window, count, rt, min rt
            uint32_t rc[3] = {0, 0, 0};
            uint32_t rrt = 0, rmn = 0xFFFFFFFFu;
#pragma unroll
            for (int j = 0; j < INB_EPT; ++j) {
                if (wh[j] == AW_NONE) continue;
                const uint32_t c = cz[j] & 0xFFFFu, rt = cz[j] >> 16;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    if (wh[j] != (uint32_t)(k + 1)) continue;  // AW_PASS = 1, AW_BLOCK = 2, AW_EXIT = 3
                    if (rw[k] != wi[j]) {
                        inb_flush(L, m0, k + 1, rw[k], rc[k], rrt, rmn);
                        rw[k] = wi[j];
                        rc[k] = 0;
                        if (k == 2) { rrt = 0; rmn = 0xFFFFFFFFu; }
                    }
                    rc[k] += c;
                    if (k == 2) { rrt += rt; rmn = rt < rmn ? rt : rmn; }
                }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) inb_flush(L, m0, k + 1, rw[k], rc[k], rrt, rmn);
        }
        __syncthreads();
        // ---- the tile into slot t's 64-bit accumulators; the LDS slot cleared for the next tile
        if (t < INB_SLOTS) {
            const int32_t w = L.W[t];
            if (w >= 0) {  // (few slots a tile: the others' threads pass)
                uint64_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
                uint32_t mn = 0xFFFFFFFFu;
                for (uint32_t i = 0; i < INB_COPIES; ++i) {
                    const uint32_t k = (i + t) & (INB_COPIES - 1);  // (neighbouring slots on different banks)
                    s0 += L.s[0][t][k]; s1 += L.s[1][t][k]; s2 += L.s[2][t][k]; s3 += L.s[3][t][k];
                    mn = L.minrt[t][k] < mn ? L.minrt[t][k] : mn;
                    L.s[0][t][k] = 0; L.s[1][t][k] = 0; L.s[2][t][k] = 0; L.s[3][t][k] = 0;
                    L.minrt[t][k] = 0xFFFFFFFFu;
                }
                if (w > AW) { AW = w; A0 = A1 = A2 = A3 = 0; AM = 0xFFFFFFFFu; }
                if (w == AW) {
                    A0 += s0; A1 += s1; A2 += s2; A3 += s3;
                    AM = mn < AM ? mn : AM;
                }
                L.W[t] = -1;
            }
        }
        __syncthreads();
    }
    if (dthread) atomicAdd(&L.thread, dthread);
    if (nvis) atomicAdd(&L.visited, nvis);
    if (nupd) atomicAdd(&L.updates, nupd);
    __syncthreads();
    InbPart& P = part[blockIdx.x];
    if (t < 64) {
        const bool on = t < INB_SLOTS;
        P.W[t] = on ? AW : -1;
        P.s[t][0] = on ? A0 : 0; P.s[t][1] = on ? A1 : 0; P.s[t][2] = on ? A2 : 0; P.s[t][3] = on ? A3 : 0;
        P.minrt[t] = on ? AM : 0xFFFFFFFFu;
    }
    if (t == 0) { P.thread = L.thread; P.visited = L.visited; P.updates = L.updates; P.pad = 0; }
}

struct InbMerge {
    int32_t W[64];
    unsigned long long s[64][4];
    uint32_t minrt[64];
    int32_t thread;
    uint32_t parts, visited, updates;
};

// 1,024 threads: thread t takes slot t & 63 of the partials (t >> 6) + 16 i, eight loads in flight at a time, and keeps
// its maximum / sums in registers; one LDS atomic a thread ends each phase
#define INB_CT 1024u
#define INB_CU 8
__global__ __launch_bounds__(INB_CT) void k_inb_commit(const InbPart* __restrict__ part, uint32_t nparts, int64_t t0,
                                                       int32_t max_rt, InbNode* __restrict__ node) {
    __shared__ InbMerge M;
    const uint32_t t = threadIdx.x, sl = t & 63u, q = t >> 6;
    if (t < 64) {
        M.W[t] = -1;
        M.s[t][0] = M.s[t][1] = M.s[t][2] = M.s[t][3] = 0;
        M.minrt[t] = 0xFFFFFFFFu;
    }
    if (t == 0) { M.thread = 0; M.parts = 0; M.visited = 0; M.updates = 0; }
    __syncthreads();
    // phase 1: the latest window of every slot over the partials
    int32_t mw = -1;
    for (uint32_t g0 = q; g0 < nparts; g0 += (INB_CT / 64u) * INB_CU) {
        int32_t w[INB_CU];
#pragma unroll
        for (int j = 0; j < INB_CU; ++j) {
            const uint32_t g = g0 + (uint32_t)j * (INB_CT / 64u);
            w[j] = g < nparts ? part[g].W[sl] : -1;
        }
#pragma unroll
        for (int j = 0; j < INB_CU; ++j) mw = w[j] > mw ? w[j] : mw;
    }
    if (mw >= 0) atomicMax(&M.W[sl], mw);
    __syncthreads();
    // phase 2: the sums of that window (the slots no event fell in are passed over); the thread deltas and counters
    const int32_t W = M.W[sl];
    if (W >= 0) {
        unsigned long long a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        uint32_t mn = 0xFFFFFFFFu;
        for (uint32_t g0 = q; g0 < nparts; g0 += (INB_CT / 64u) * INB_CU) {
            unsigned long long v[INB_CU][4];
            uint32_t m[INB_CU];
            bool hit[INB_CU];
#pragma unroll
            for (int j = 0; j < INB_CU; ++j) {
                const uint32_t g = g0 + (uint32_t)j * (INB_CT / 64u);
                const bool ok = g < nparts;
                const InbPart& P = part[ok ? g : 0u];
                hit[j] = ok && P.W[sl] == W;
                v[j][0] = P.s[sl][0]; v[j][1] = P.s[sl][1]; v[j][2] = P.s[sl][2]; v[j][3] = P.s[sl][3];
                m[j] = P.minrt[sl];
            }
#pragma unroll
            for (int j = 0; j < INB_CU; ++j) {
                if (!hit[j]) continue;
                a0 += v[j][0]; a1 += v[j][1]; a2 += v[j][2]; a3 += v[j][3];
                mn = m[j] < mn ? m[j] : mn;
            }
        }
        if (a0) atomicAdd(&M.s[sl][0], a0);
        if (a1) atomicAdd(&M.s[sl][1], a1);
        if (a2) atomicAdd(&M.s[sl][2], a2);
        if (a3) atomicAdd(&M.s[sl][3], a3);
        if (mn != 0xFFFFFFFFu) atomicMin(&M.minrt[sl], mn);
    }
    if (t < nparts) {  // (nparts <= INB_MAX_WG = INB_CT)
        const InbPart& P = part[t];
        if (P.thread) atomicAdd(&M.thread, P.thread);
        if (P.visited) { atomicAdd(&M.parts, 1u); atomicAdd(&M.visited, P.visited); }
        if (P.updates) atomicAdd(&M.updates, P.updates);
    }
    __syncthreads();
    // commit: slot t onto its bucket (LeapArray.currentWindow, LeapArray.java:117-208)
    if (t < INB_SLOTS && M.W[t] >= 0) {
        const int64_t b500 = (t0 / 500) & ~1ll;
        const int64_t ws = t < 2 ? (b500 + M.W[t]) * 500 : (b500 / 2 + M.W[t]) * 1000;
        Bkt* bp = t < 2 ? &node->sec[t] : &node->minb[t - 2];
        Bkt b = *bp;
        const int64_t mrt = M.minrt[t] == 0xFFFFFFFFu ? INT64_MAX : (int64_t)M.minrt[t];
        bool store = true;
        if (ws > b.ws) {  // a new or a later window: reset (no borrowed pass: the node's borrow ring is empty), then set
            b.ws = ws;
            b.pass = (int64_t)M.s[t][0];
            b.block = (int64_t)M.s[t][1];
            b.exc = 0;
            b.succ = (int64_t)M.s[t][2];
            b.rt = (int64_t)M.s[t][3];
            b.occ = 0;
            b.minrt = mrt < max_rt ? mrt : max_rt;
        } else if (ws == b.ws) {
            b.pass += (int64_t)M.s[t][0];
            b.block += (int64_t)M.s[t][1];
            b.succ += (int64_t)M.s[t][2];
            b.rt += (int64_t)M.s[t][3];
            if (mrt < b.minrt) b.minrt = mrt;
        } else {
            store = false;  // an older window than the bucket's: lost, as a detached bucket
        }
        if (store) *bp = b;
    }
    if (t == 0) {
        node->thread += M.thread;
        node->last[0] = M.parts;
        node->last[1] = M.visited;
        node->last[2] = M.updates;
    }
}

static_assert(INB_MAX_WG <= INB_CT, "k_inb_commit reads one partial's counters a thread");

namespace sg {
// recs / dec: the batch's n sorted records and their final decisions; ev / vals: the submitted events and every sorted
// position's submission index (for the resource of an EXIT that names no ENTRY); part: INB_MAX_WG partials
hipError_t launch_inbound(const SEv* recs, const uint32_t* dec, uint64_t n, const sg_event* ev, const uint32_t* vals,
                          const DevState& S, const DevCfg& cfg, int64_t t0, InbPart* part, InbNode* node, hipStream_t st) {
    if (n == 0 || n >= (1ull << 32)) return hipErrorInvalidValue;
    const uint32_t ntile = (uint32_t)((n + INB_TILE - 1) / INB_TILE);
    const uint32_t g = ntile < INB_MAX_WG ? ntile : INB_MAX_WG;
    hipLaunchKernelGGL(k_inb_tiles, dim3(g), dim3(256), 0, st, recs, dec, (uint32_t)n, ev, vals, S.info, S.ext, S.max_ctx,
                       cfg.switch_on, t0, part);
    hipLaunchKernelGGL(k_inb_commit, dim3(1), dim3(INB_CT), 0, st, part, g, t0, cfg.max_rt, node);
    return hipGetLastError();
}
} // namespace sg
