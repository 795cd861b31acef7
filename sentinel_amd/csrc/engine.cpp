// engine.cpp -- host side of the MI355X decision engine: the C ABI of
// include/sentinel_gpu.h, the rule loaders and the per-batch launch pipeline.
// The rule managers (validation, de-duplication, java.util.HashSet ordering,
// FlowRuleComparator sort) are rules.h, the compiler of the device tables is
// compile.h.  All decisions are taken on the device, by the HIP kernels of the
// group stage (kernels.hip) and of the decide owners (decide.hip, head.hip,
// param.hip, pvalue.hip, aux.hip, inbound.hip, cluster.hip); nothing here
// evaluates a rule.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/sentinel_gpu.h"
#include "authority.h"
#include "compile.h"
#include "dev_types.h"
#include "embedded.h"
#include "launch.h"
#include "pkeys.h"
#include "pmap.h"  // (pm_buckets: sg_param_thread_count)
#include "pvtab.h"
#include "rules.h"

using namespace sg;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIPCHK(x)                                                                                        \
    do {                                                                                                 \
        hipError_t _e = (x);                                                                             \
        if (_e != hipSuccess) return fail(SG_EDEVICE, std::string(#x ": ") + hipGetErrorString(_e));    \
    } while (0)

// ---- param value keys (ParamFlowRuleUtil.parseItemValue typing, ParamFlowRuleUtil.java:85-121)
uint64_t mix64(uint64_t x) { return pk::mix64(x); }
// the pure key of a value (sg_param_key): typing and hashing are pkeys.h's, which the dictionary shares
uint64_t param_key(const char* v, const char* t) { return pk::pure_key<pk::StdHash>(v, t); }

template <class T> void dfree(T*& p) {
    if (p) (void)hipFree(p);
    p = nullptr;
}
// a buffer that holds too little: freed, and allocated again for max(need, floor) elements of elem bytes
template <class T> hipError_t grow(T*& p, uint64_t& cap, uint64_t need, uint64_t floor, size_t elem = sizeof(T)) {
    dfree(p);
    cap = 0;
    const uint64_t c = std::max(need, floor);
    const hipError_t rc = hipMalloc(&p, c * elem);
    if (rc == hipSuccess) cap = c;
    return rc;
}

} // namespace

// =====================================================================================
#define TMAP_KEY (1ull << 63)  // pmap_key of a thread-count map: TMAP_KEY | res << 8 | paramIdx
constexpr int EMB_LAST_WORDS = 12;  // sgx_embedded_last: [0] requests, [1..7] answers (EMB_A_*), [8] words written ahead,
                                    // [9] XF_EMB segments in cooperative bins, [10] in lane bins, [11] in the late lane pass
struct sg_engine {
    sg_config cfg;
    int device = 0;
    hipStream_t stream = nullptr;
    double last_ms[4] = {0, 0, 0, 0};

    // resources
    std::unordered_map<std::string, uint32_t> ids;
    std::vector<std::string> names;
    uint32_t n_chains = 0;

    // rule managers
    bool flow_loaded = false, deg_loaded = false, par_loaded = false;
    std::vector<std::string> last_flow, last_deg, last_par; // equality keys of the last loaded lists
    std::vector<FlowR> flows;
    std::vector<DegR> degs;
    std::vector<ParamR> params;
    std::vector<std::vector<int>> res_flow, res_deg, res_par; // compiled order per resource
    std::map<std::string, uint32_t> psid_of;                   // "res\x00eqkey" -> param state id
    uint32_t next_psid = 1;
    // ParameterMetric maps (dev_types.h PMap): one region per rule state (psid) and per (resource, paramIdx)
    // thread-count map, laid out in one slot pool rebuilt whenever the set of maps changes
    std::map<uint32_t, uint32_t> rmap_cap;                      // psid -> CacheMap capacity
    std::set<uint64_t> tmaps;                                   // res << 8 | paramIdx
    std::vector<uint64_t> pmap_key;                             // map index -> psid, or TMAP_KEY | res << 8 | idx
    std::unordered_map<uint32_t, uint32_t> pmap_index;         // psid -> map index
    std::vector<uint32_t> tm_base;                              // per resource: Prog.tm_base
    uint64_t n_pslot = 0;                                       // bucket slots in the pool (param_table_log2 bound)
    uint64_t pool_nb = 0;                                       // pool buckets (regions grow into it: k_pm_grow)
    unsigned long long* d_pool_next = nullptr;
    uint4* d_pmoves = nullptr;  // k_pm_grow's move list (one entry a map) + its count word at [pmoves_cap]
    PBucket* d_pbkt2 = nullptr;  // the other pool of the device compaction (compact_pmaps), and its values
    PData* d_pdat2 = nullptr;
    uint32_t* d_pcwork = nullptr;  // its scratch: sizes, offsets, scan partials (3 x pmoves_cap + 4096 words)
    uint64_t pmoves_cap = 0;                  // next free pool bucket
    unsigned long long* h_pool_next = nullptr;                  // pinned copy, refreshed by every batch (compaction)
    uint64_t n_compact = 0;                                     // pool compactions (diagnostics)
    uint64_t pool2_nb = 0;                                      // buckets of d_pbkt2 / d_pdat2 (= pool_nb once laid out)
    uint32_t n_dev_rules = 0;

    // device state
    Bkt* d_sec = nullptr;
    Bkt* d_minb = nullptr;
    int64_t snap_hi = -1;  // highest second of a metrics snapshot's `now` (DevCfg.snap_hi)
    NodeInfo* d_info = nullptr;
    Prog* d_prog = nullptr;
    DRule* d_rules = nullptr;
    RState* d_rstate = nullptr;
    DHot* d_hot = nullptr;
    PMap* d_pmap = nullptr;
    PBucket* d_pbkt = nullptr;
    PData* d_pdat = nullptr;
    uint64_t* d_pbm = nullptr;
    uint32_t* d_ppre = nullptr;
    uint32_t* d_tmid = nullptr;
    uint8_t* d_ring = nullptr;
    uint32_t rules_cap = 0, hot_cap = 0;

    // batch scratch: two slots, so that the group stage of batch k+1 (on gstream) runs while the
    // decide stage of batch k (on stream) is still in flight.  Every user of these arrays is handed its slot.
    struct BatchSlot {
        sg_event* d_ev = nullptr;
        uint32_t* d_out = nullptr;
        uint32_t *d_k0 = nullptr, *d_v0 = nullptr, *d_k1 = nullptr, *d_v1 = nullptr;
        uint32_t *d_hist = nullptr, *d_part = nullptr, *d_flag = nullptr, *d_pos = nullptr, *d_order = nullptr;
        uint32_t *d_posof = nullptr, *d_dec = nullptr, *d_blkcnt = nullptr, *d_prev = nullptr;
        SEv *d_recs = nullptr, *d_rec_o = nullptr;
        uint32_t* d_ccnt = nullptr;    // hot / cold group stage: per-tile cold counts, the cold segments' tile scratch
        bool radix = false;            // this batch took the radix group stage (d_posof), else the hot / cold one
        uint32_t nhot = 0;             // ... with these hot ids (its words and P in d_flag / d_pos)
        uint32_t hot_marked = 0;       // ... of which k_seg_bin marked this many for the side tables (BS_HOT_MARKED)
        uint32_t ublk_coop = 0, ublk_lane = 0;  // PM_UBLK segments in cooperative / lane bins (BS_UBLK, BS_UBLK_LANE)
        uint32_t emb_ub = 0, emb_coop = 0, emb_lane = 0;  // XF_EMB segments: their events (an upper bound of the batch's
                                                          // token requests), those in cooperative / lane bins (BS_EMB ..)
        Seg* d_segs = nullptr;
        uint64_t* d_cand = nullptr;
        uint32_t* d_bsmall = nullptr;  // the batch's small words (dev_types.h BS_*)
        sg_event_ext* d_ext = nullptr; // sg_submit_ex host inputs staged in HBM
        sg_arg* d_args = nullptr;
        uint64_t ext_cap = 0, args_cap = 0;
        // sg_submit_ex: the aux.hip post-pass lists k_seg_bin builds (counts at BS_AUX)
        uint32_t* d_ashort = nullptr;
        uint64_t *d_apiece = nullptr, *d_amulti = nullptr, *d_along = nullptr;
        uint64_t aux_cap_n = 0;
        uint32_t* d_mix = nullptr;     // XF_MIX segments of the cooperative bins: [0, nmix0) narrow, [mix_cap, ..) wide
        uint64_t mix_cap = 0;
        Link* d_link = nullptr;        // frozen-stretch skipping side tables (DevState.link/bst/pend/spans)
        uint32_t *d_bst = nullptr, *d_pend = nullptr;
        Span* d_spans = nullptr;
        hipEvent_t* ev = nullptr;      // the batch's event set (evset[]): group start/end, decide start/end, post end
        hipEvent_t last_post = nullptr;  // post end of the last batch decided from this slot: the next group stage to
                                         // fill the slot waits for it on the device
        hipEvent_t lent = nullptr;       // the slot's arrays were the scratch of the other slot's embedded token call,
                                         // which ends here on the engine stream: the next group stage waits for it too
        uint32_t* h_head = nullptr;    // pinned: d_bsmall[0..BS_HEAD_WORDS) as the group stage left it (copied on gstream)
        // What the decide stage needs of the group part's locals: it may run inside the next submit, after
        // e->gbase and e->epoch have moved on, so nothing of these is re-read from the engine.
        struct Grouped {
            uint64_t n = 0, n_args = 0, gbase = 0, ring_mask = 0;
            const sg_event* dev_ev = nullptr;
            const sg_event_ext* dev_ext = nullptr;
            const sg_arg* dev_args = nullptr;
            uint32_t *out = nullptr, *dev_out = nullptr, *vin = nullptr;
            uint32_t epoch = 0, skip_min = 0, lane_max = 0, mb = 0;
            bool ext = false, host_out = false, force_lane = false;
            int set = 0;               // index of its event set and flag mirror
        } g;
    } slot[2];
    int cur = 0;                 // slot of the next batch
    int last = -1;               // slot of the last batch handed to the decide stage
    int grouped = -1;            // slot of a batch whose group stage is enqueued and whose head is not read yet: the
                                 // next call that touches the engine hands it to the decide stage (handoff())
    int held_rc = 0;             // an error a diagnostics export met while draining (it cannot return one): the next
    std::string held_msg;        // ABI call that drains or submits returns it
    bool handoff_late = true;    // SG_HANDOFF=0: every batch is handed off inside the call that submits it
    // Event sets and flag mirrors rotate over four batches: the batch being grouped, the one being decided, the one
    // being collected, and the one before that, whose end events the collected batch's gaps are measured from.
    static constexpr int N_SETS = 4;
    hipEvent_t evset[N_SETS][5] = {};
    uint32_t* h_mirror = nullptr;  // pinned, N_SETS x BS_MIRROR_WORDS of d_bsmall as the decide stage left it
    uint64_t seq = 0;              // batches handed to the decide stage so far (batch i has set i % N_SETS)
    struct InFlight { int set; uint32_t hot_marked, ublk_coop, ublk_lane, emb_coop, emb_lane; };
    std::deque<InFlight> inflight;  // handed off, not yet collected (timings, flags), oldest first
    hipStream_t gstream = nullptr;
    std::vector<std::array<double, 4>> tlog;  // per batch [group, decide, post, total] ms, by collect()
    std::vector<std::array<double, 2>> glog;  // per batch [group-stream idle, decide-stream idle] ms before it
    std::string fatal;           // non-empty: a batch left device state inconsistent; every later submit fails
    uint32_t* d_prio = nullptr;  // [res] sticky PM_* marks (DevState.prio)
    // hot / cold group stage (kernels.hip k_grp_*): [sort key] -> hot id of the next batch (0xFFFF: cold), the ids'
    // keys, and how many (the host learns it with the batch's head)
    uint16_t* d_hot_tab = nullptr;
    uint32_t* d_hot_list = nullptr;
    uint32_t nhot = 0;
    uint32_t* d_hot_part = nullptr;  // the hot scan's per-chunk partials ((max tiles / 64 + 2) x HOT_MAX words)
    uint32_t* d_hot_hb = nullptr;    // per hot id: first sorted position, total (2 x HOT_MAX words)
    // which side tables (forward links, bst[]) the batch being grouped needs (k_seg_bin): one word per hot id, then
    // one bit per 1024-position block of the cold region, then per hot id the most events one 500 ms bucket can hold
    // (k_hot_bmax; d_edges: its bucket-opening tiles, count first)
    uint32_t* d_need = nullptr;
    uint64_t need_words = 0;
    uint32_t* d_edges = nullptr;
    uint32_t hot_marked_last = 0;  // hot ids marked for the side tables in the last collected batch (sgx_hot_marked)
    uint32_t ublk_last[3] = {0, 0, 0};  // sgx_preblocked_last: PM_UBLK segments in cooperative / lane bins, RF_UBLK words
    // Embedded token server (embedded.h; ClusterStateManager's server state): emb_on: the mode; emb_n: resources whose
    // program is XF_EMB (0: every batch takes the usual path); d_emb_flow: [res] the flowId of an XF_EMB resource;
    // d_emb_side: the side words of the batch being decided (DevState.emb), d_emb_idx: its requests' batch indices,
    // d_emb_cnt / d_emb_part: the extraction's tile counts and scan partials.  All allocated on first use.
    bool emb_on = false;
    uint32_t emb_n = 0;
    int64_t* d_emb_flow = nullptr;
    uint32_t *d_emb_side = nullptr, *d_emb_idx = nullptr, *d_emb_cnt = nullptr, *d_emb_part = nullptr;
    uint64_t emb_cap = 0;
    hipEvent_t emb_ev[2] = {nullptr, nullptr};  // the end of the token call that borrowed slot [i]'s arrays (BatchSlot.lent)
    hipEvent_t emb_t[4] = {nullptr, nullptr, nullptr, nullptr};  // around the extraction, the token call and the scatter
    bool emb_timed = false;            // ... recorded for the batch in flight (one at a time: no overlap)
    double emb_ms[3] = {0, 0, 0};      // sgx_embedded_ms: their times in the last collected batch that made requests
    uint64_t emb_last[EMB_LAST_WORDS] = {};  // sgx_embedded_last
    // the global inbound node, Constants.ENTRY_NODE (inbound.hip): allocated by the first sg_track_inbound(1); inb_on:
    // batches are counted on it, inb_ever: it exists (readable after tracking was turned off)
    InbNode* d_inb = nullptr;
    InbPart* d_inbpart = nullptr;
    bool inb_on = false, inb_ever = false;
    bool radix_group = false;    // SG_DEBUG_FLAGS & 8192: the all-radix group stage (A/B)
    uint64_t radix_below = 1u << 18;  // SG_RADIX_BELOW: batches of fewer events take the radix group stage (the drop-in's
                                      // 65,536-event batches: 36 vs 30-32 M entries/s on the hot / cold one)
    uint32_t tok_light = 8192;   // SG_TOK_LIGHT: token flows of at most this many requests a call on one-wave workgroups
    uint32_t tok_wide = 1024;    // SG_TOK_WIDE: 1024 or 512 lanes for the other token flows (1024: 7.3 vs 8.0 ms a call)
    bool tiny_on = true;         // SG_TINY=0: synchronous batches of <= 256 events through the batched path too
    // sg_submit_ex: host-side ext / args are staged here (per batch slot, below); origin / context nodes
    AuxNode* d_auxtab = nullptr;
    uint32_t* d_auxcnt = nullptr;
    uint64_t aux_mask = 0;
    // the aux.hip post-pass: partial node results of the pieces of long segments (decide stage: one set)
    AuxAcc* d_auxpool = nullptr;
    uint64_t* d_auxmeta = nullptr;
    uint32_t auxpool_cap = 0;
    uint64_t auxmeta_cap = 0;
    // ContextUtil names: origins (0 = "") and contexts (0 = sentinel_default_context), first-intern order
    std::unordered_map<std::string, uint32_t> origin_ids, context_ids;
    std::unordered_map<std::string, int> rule_names;  // limitApp / CHAIN ref strings the flow rules name
    // AuthorityRuleManager (authority.h): the kept rules, their device table ([max_resources] descriptors, allocated
    // by the first non-empty load) and id lists; auth_on: rules are loaded (the kernels get null pointers otherwise)
    AuthTable auth;
    AuthDesc* d_auth = nullptr;
    uint32_t* d_auth_ids = nullptr;
    size_t auth_ids_cap = 0;
    bool auth_on = false, auth_loaded = false;
    std::vector<std::string> last_auth;
    uint32_t* d_comp = nullptr;  // [res] STRATEGY_RELATE component representative (sort key); null: none
    uint32_t span_cap = 0;
    uint32_t epoch = 0;          // link tag of the batch being grouped
    uint64_t spans_total = 0;    // frozen span slots taken by the cooperative kernels (diagnostics)
    uint64_t cap_n = 0;          // events both slots' arrays hold (ensure_batch)
    uint32_t* d_small = nullptr;  // the engine's small words (dev_types.h SM_*)
    uint32_t* d_sink = nullptr;  // 1024 words, DevState.sink
    int64_t* d_borrow = nullptr;  // [res][2]{ws, pass}: second-window borrow rings (prioritized entries)
    uint64_t* d_keyring = nullptr;  // ENTRY arg keys by global index (exit(count, args)); once param rules exist
    uint32_t dbg_flags = 0;
    int prof_bin = 0;            // SG_PROF_BIN: which cooperative bin (0 J16, 1 J4, 2 J1) fills the SG_DEBUG counters
    unsigned long long* d_dbg = nullptr;  // SG_DEBUG=1: [0..63] counters of the J16 bin
    uint64_t cap_hist = 0;
    uint64_t gbase = 0;
    // decide bins run concurrently: one stream per cooperative bin, the lane bins on the main stream
    // decide streams: J16 on bin_stream[0], J4 then J1 on bin_stream[1] (together shorter than J16), the
    // lane bins on stream; with gstream that is four streams for the four hardware queues a process
    // gets (GPU_MAX_HW_QUEUES): a fifth stream would share a queue and serialise behind another's kernels
    hipStream_t bin_stream[2] = {nullptr, nullptr};
    hipEvent_t fork = nullptr, join[2] = {nullptr, nullptr};
    hipEvent_t fork0 = nullptr;  // XF_MIX batches: the pre passes on bin_stream[1] start here, beside the lane bins
    hipEvent_t grown = nullptr;  // ... and their map-touching part after the maps' growth
    bool pipeline = true;   // the group stage of batch k+1 overlaps the decide stage of batch k (SG_PIPELINE=0: off)
    int j1_stream = -1;     // SG_J1_STREAM=1 / 0: J1 after J16 / J8 on bin_stream[0] / after the lane bins (default:
                            // bin_stream[0] when the short aux nodes take the main stream, else the main stream)
    uint32_t lane_max = 256, j1_max = 4096, j4_max = 65536;
    // k_lite's programs without param rules stay on a lane up to lite_max events (decide.hip k_seg_bin).  A full C4
    // batch with 512 against 256: period 3.46 -> 3.37 ms (group 3.32 -> 3.06, decide 3.11 -> 3.12 ms); with 1,024
    // k_lite's longest lanes are the decide stage's tail (4.42 ms).  512 for k_lane's programs too: C3 6.0 -> 9.0 ms
    // a batch.  DESIGN.md §5 "The lane / J1 boundary".  With pinned bins lane_max holds for every lane bin, unless
    // SG_LITE_MAX pins this one too
    uint32_t lite_max = 512;
    bool lite_pinned = false;
    uint32_t head_min = 0;       // SG_HEAD_MIN: single-rule THREAD / rate-limiter head segments longer than this leave
                                 // the lane bins for the event-driven head owner (0: the lane bins keep up to lane_max;
                                 // C3 A/B: 64 -> 1.15, 128 -> 1.27, 0 -> 1.27 G entries/s)
    bool bins_pinned = false;  // SG_LANE_MAX / SG_J1_MAX / SG_J4_MAX set: no per-batch adaptation
    uint32_t skip_min = 32768;  // frozen stretches shorter than this (x NW/16) are streamed, not skipped
    bool pq_on = true;          // PF_PQ segments to k_pq (SG_PQ=0: the per-lane kernel, as before round 3)
    uint32_t pq_wide = 8192;    // PF_PQ segments longer than this get the 1024-lane k_pq
    bool mix_on = true;         // XF_MIX programs (SG_MIX=0: every param + flow / degrade resource one lane)
    bool mix_pq = false;        // SG_MIX_PQ=1: param-only programs of the XF_MIX shape decided as XF_MIX too
    bool pv_pq = true;          // SG_PV_PQ (default 1): XF_PVPQ programs' long segments through the value-parallel passes
    bool has_mix = false;       // some resource's program is XF_MIX (the batches keep the pre / post pass lists)
    bool has_head = false;      // some resource's program is XF_HEADT / XF_HEADR (head.hip k_head is launched)
    bool pv_on = true;          // SG_PV (default 1): the value-parallel pre pass (pvalue.hip) for the long XF_MIX segments
    PvBuf pvb{};                // its scratch: the pre pass's (launch_pv_a / _b) ...
    PvBuf pvbt{};               // ... and the post pass's (launch_pvt), so that the next batch's extraction and sort
                                // (launch_pv_a, early on bin_stream[1]) can run beside this batch's post pass
    bool has_multi = false;     // some STRATEGY_RELATE component exists (PX_MULTI): launch_pv_a waits for the grants
    uint64_t pv_cap = 0;
    PvSeg* d_pvseg = nullptr;
    PvSeg* d_pvtseg = nullptr;  // the post pass's (pvalue.hip launch_pvt)
    uint32_t* d_pvrest = nullptr;  // the wide segments the passes left to k_pq: pre [0, pvseg_cap], post after
    bool pvt_on = false;        // SG_PVT (default: SG_PV): the value-parallel post pass (thread-count maps)
    uint64_t pvseg_cap = 0;
    uint64_t pvch_cap = 0;      // pvalue.hip's extraction chunk arrays
    uint32_t *d_pvtot = nullptr, *d_pvhist = nullptr, *d_pvpart = nullptr, *d_pvthist = nullptr, *d_pvtpart = nullptr;
    uint32_t pv_last_m = 0;     // listed segments of the last batch that ran it (diagnostics)
    bool skip_pinned = false;   // SG_SKIP_MIN set: no per-batch adaptation
    // token server (cluster.hip): flowId table and ClusterMetric state in HBM, host mirror of the
    // configuration (ClusterFlowRuleManager.FLOW_RULES / ClusterMetricStatistics roles)
    std::vector<CFlow> cflows;                    // host copy of the config part (state lives on the device)
    std::unordered_map<int64_t, uint32_t> cmap;   // flowId -> flow index
    CFlow* d_cflow = nullptr;
    CBkt* d_cbkt = nullptr;
    CSlot* d_ctab = nullptr;
    uint32_t ctab_mask = 0;
    uint64_t ncbkt = 0;
    NsLimiter* d_nslim = nullptr;                 // one RequestLimiter a namespace (SG_MAX_NAMESPACES of them)
    // namespaces (GlobalRequestLimiter / ConnectionManager roles): index 0 = "default", always there
    std::vector<std::string> ns_names;
    std::unordered_map<std::string, uint32_t> ns_of;
    std::vector<double> ns_limit;                 // qpsAllowed (negative: no limiter)
    std::vector<int32_t> ns_conn;                 // connected count a flow of the namespace starts with
    std::unordered_map<int64_t, uint32_t> flow_ns;  // flowId -> namespace index (absent: "default")
    double* d_nslimit = nullptr;                  // ns_limit on the device (the grouped limiter reads it)
    uint32_t* d_nsb = nullptr;                    // per namespace: its bucket range of the call (2 words)
    bool tok_ns = false;                          // SG_TOK_NS=1: the grouped limiter with one namespace too
    sg_token_req* d_treq = nullptr;
    sg_token_result* d_tres = nullptr;
    uint32_t* d_tfidx = nullptr;
    uint32_t* d_tbounds = nullptr;  // the flows' first sorted positions (nflows + 1 words)
    uint64_t tbounds_cap = 0;
    uint64_t tcap = 0;
    // cluster param flows (ClusterParamFlowRuleManager / ClusterParamMetricStatistics roles)
    std::vector<PFlow> pflows;                    // host copy of the config part
    std::unordered_map<int64_t, uint32_t> pmap;   // flowId -> param flow index
    PFlow* d_pflow = nullptr;
    PHot* d_phot = nullptr;
    CSlot* d_pftab = nullptr;
    uint32_t pftab_mask = 0;
    PVal* d_pvtab = nullptr;                      // (flow, value) counts, pv_mask + 1 slots (pvtab.h)
    uint32_t pv_mask = 0;
    uint32_t pv_log2 = 17, pv_max_log2 = 24;      // SG_PV_LOG2, SG_PV_MAX_LOG2: initial and maximum capacity
    uint64_t pv_claimed = 0;                      // claimed_ub: exact after a rehash or a rule load + values listed since
    uint64_t pv_live = 0, pv_rehashes = 0, pv_resizes = 0, pv_last_us = 0;  // (sg_cluster_param_table_stats)
    uint32_t* d_pvcnt = nullptr;                  // the rehash's two result words
    PVal* d_pvspare = nullptr;                    // the table the last same-size rehash left: the next one's target
    uint64_t pv_spare_cap = 0;
    hipEvent_t pv_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    sg_param_token_req* d_preq = nullptr;
    uint64_t* d_pvals = nullptr;
    uint64_t pcap = 0, pvcap = 0;
    // the value-parallel owner (ptok.h): SG_PTOK_VP=0 leaves every flow to k_ptok_flow, SG_PTOK_MIN = the request
    // count below which a call with fewer than PTOK_PER_FLOW requests per loaded flow does (and keeps the one-wave
    // limiter: the parent's launches, measured faster there); d_ptst: [0] listed values and [1] flags of the call (k_ptok_prep), [2..4] the
    // cumulative owner counters (sg_cluster_param_table_stats [7..9]); the per-flow words and the dedup table
    bool ptok_vp = true;
    uint64_t ptok_min = 8192;
    unsigned long long* d_ptst = nullptr;
    uint32_t *d_ptserial = nullptr, *d_ptdedup = nullptr;
    uint64_t ptserial_cap = 0, ptdedup_cap = 0;
    // exact parameter keys (pkeys.h): the value dictionary of sg_param_intern, the entries the loaded param rules'
    // hot items pin, and the sweep's device buffers (keysweep.hip) and statistics (sg_param_keys_stats)
    pk::Dict<pk::StdHash> pkeys;
    std::vector<uint64_t> par_pins;
    uint64_t* d_ks_key = nullptr;
    uint32_t *d_ks_idx = nullptr, *d_ks_marks = nullptr;
    uint64_t ks_cap = 0;                          // slots of d_ks_key / d_ks_idx (and bits of d_ks_marks)
    hipEvent_t ks_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    uint64_t ks_sweeps = 0, ks_last[4] = {0, 0, 0, 0};  // last sweep: candidates, held on the device, dropped, us
    double ks_scan_ms[3] = {0, 0, 0};             // ... and its scans: maps, key ring, token server values
    uint64_t pbm_words = 0;                       // words of d_pbm
    // cluster metrics (cmetrics.hip): nothing of this exists before the first sg_cluster_metrics.  The rows
    // (cluster flows, then param flows, by flow index), the param flows' bucket masks and chunk tables, and, sized by
    // the value table's capacity, the candidate list, its sort pairs and the partial lists
    std::unordered_map<int64_t, std::string> cres, pres;  // flowId -> the rule's resource name
    sg_cluster_metric* d_cm_rows = nullptr;
    uint32_t *d_cm_mask = nullptr, *d_cm_bounds = nullptr, *d_cm_nch = nullptr, *d_cm_coff = nullptr;
    uint64_t cm_flow_cap = 0;                     // flows d_cm_rows .. d_cm_coff are sized for
    uint32_t *d_cm_k0 = nullptr, *d_cm_v0 = nullptr, *d_cm_k1 = nullptr, *d_cm_v1 = nullptr, *d_cm_hist = nullptr,
             *d_cm_part = nullptr, *d_cm_cnt = nullptr;
    int64_t *d_cm_sum = nullptr, *d_cm_psum = nullptr;
    uint64_t *d_cm_key = nullptr, *d_cm_pkey = nullptr;
    uint64_t cm_cand_cap = 0, cm_chunk_cap = 0;
    hipEvent_t cm_ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    double cm_last[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // sgx_cluster_metrics_last
    // snapshot scratch
    uint32_t *d_snap_cnt = nullptr, *d_snap_off = nullptr;
    sg_metric_node* d_snap_out = nullptr;
    uint64_t snap_cap = 0;
};

static int handoff(sg_engine* e);  // (with the batch pipeline, below)

namespace {

constexpr uint64_t SHARD_BATCH = 3ull << 21;  // batches of fewer events take the shard-sized bins and skip threshold

static void free_slot(sg_engine::BatchSlot& B) {
    dfree(B.d_ev); dfree(B.d_out); dfree(B.d_k0); dfree(B.d_v0); dfree(B.d_k1); dfree(B.d_v1);
    dfree(B.d_hist); dfree(B.d_part); dfree(B.d_flag); dfree(B.d_pos); dfree(B.d_order); dfree(B.d_segs);
    dfree(B.d_cand); dfree(B.d_posof); dfree(B.d_dec); dfree(B.d_recs); dfree(B.d_rec_o); dfree(B.d_blkcnt);
    dfree(B.d_prev); dfree(B.d_bsmall); dfree(B.d_ccnt);
    dfree(B.d_link); dfree(B.d_bst); dfree(B.d_pend); dfree(B.d_spans); dfree(B.d_ext); dfree(B.d_args);
    dfree(B.d_ashort); dfree(B.d_apiece); dfree(B.d_amulti); dfree(B.d_along); dfree(B.d_mix);
    B.ext_cap = B.args_cap = B.aux_cap_n = B.mix_cap = 0;
}
int ensure_batch(sg_engine* e, uint64_t n) {
    if (n <= e->cap_n) return SG_OK;
    uint64_t c = std::max<uint64_t>(n, 1u << 20);
    HIPCHK(hipStreamSynchronize(e->stream));  // no batch may use the old buffers
    uint64_t nblocks = (c + radix_tile() - 1) / radix_tile();
    e->cap_hist = nblocks * 256;  // 8-bit digit histograms
    for (auto& B : e->slot) {
        free_slot(B);
        HIPCHK(hipMalloc(&B.d_ev, c * sizeof(sg_event)));
        HIPCHK(hipMalloc(&B.d_out, c * 4));
        HIPCHK(hipMalloc(&B.d_k0, c * 4));
        HIPCHK(hipMalloc(&B.d_v0, c * 4));
        HIPCHK(hipMalloc(&B.d_k1, c * 4));
        HIPCHK(hipMalloc(&B.d_v1, c * 4));
        HIPCHK(hipMalloc(&B.d_hist, e->cap_hist * 4));
        HIPCHK(hipMalloc(&B.d_part, (e->cap_hist / 4096 + c / 4096 + 64) * 4));
        HIPCHK(hipMalloc(&B.d_flag, c * 4));
        HIPCHK(hipMalloc(&B.d_pos, c * 4));
        HIPCHK(hipMalloc(&B.d_order, c * 4));
        HIPCHK(hipMalloc(&B.d_segs, c * sizeof(Seg)));
        HIPCHK(hipMalloc(&B.d_cand, c * 8));
        HIPCHK(hipMalloc(&B.d_posof, c * 4));
        HIPCHK(hipMalloc(&B.d_dec, c * 4));
        HIPCHK(hipMalloc(&B.d_recs, c * sizeof(SEv)));
        // (radix stage only: every batch, or those below radix_below)
        const uint64_t co = (e->radix_group || c >= (1ull << 30)) ? c : std::min<uint64_t>(c, e->radix_below);
        if (co) HIPCHK(hipMalloc(&B.d_rec_o, co * sizeof(SEv)));
        HIPCHK(hipMalloc(&B.d_ccnt, 3 * (nblocks + 64) * 4));
    }
    dfree(e->d_hot_part);
    dfree(e->d_hot_hb);
    dfree(e->d_need);
    dfree(e->d_edges);
    e->need_words = hot_max() + c / 32768 + 2 + hot_max();
    HIPCHK(hipMalloc(&e->d_need, e->need_words * 4));
    HIPCHK(hipMalloc(&e->d_edges, (nblocks + 2) * 4));
    HIPCHK(hipMalloc(&e->d_hot_part, (nblocks / 16 + 2) * hot_max() * 4));  // (HS_TC >= 16 tiles a chunk)
    HIPCHK(hipMalloc(&e->d_hot_hb, 2 * hot_max() * 4));
    for (auto& B : e->slot) {
        HIPCHK(hipMalloc(&B.d_blkcnt, ((c + 255) / 256 + 1) * N_BINS * 4));
        HIPCHK(hipMalloc(&B.d_prev, c * 4));
        HIPCHK(hipMalloc(&B.d_bsmall, BS_WORDS * 4));
        HIPCHK(hipMemset(B.d_bsmall, 0, BS_WORDS * 4));
        HIPCHK(hipMalloc(&B.d_link, c * sizeof(Link)));
        HIPCHK(hipMemset(B.d_link, 0, c * sizeof(Link)));  // tag 0 is never a batch's epoch
        HIPCHK(hipMalloc(&B.d_bst, ((c + 1023) / 1024 + 1) * 4));
        HIPCHK(hipMalloc(&B.d_pend, c * 4));
        HIPCHK(hipMalloc(&B.d_spans, (c / SPAN_CHUNK + 65536) * sizeof(Span)));
    }
    e->span_cap = (uint32_t)(c / SPAN_CHUNK + 65536);
    e->cap_n = c;
    return SG_OK;
}

// What a batch's flags say of it, in two steps.  The group stage's checks: a batch that fails one is rejected before
// any decision.
static int group_verdict(uint32_t bflags) {
    if (bflags & BF_BAD_RES) return fail(SG_EINVAL, "event res_id >= max_resources");
    if (bflags & BF_BAD_REF)
        return fail(SG_EINVAL, "an EXIT/TRACE references an event that is not an earlier ENTRY of the same resource");
    if (bflags & BF_TSPAN) return fail(SG_EINVAL, "a batch must span less than 2^31 ms");
    if (bflags & BF_BACKWARD) return fail(SG_EINVAL, "event timestamps must be non-decreasing (SURVEY Q3)");
    if (bflags & BF_BAD_ARGS)
        return fail(SG_EINVAL, "an sg_event_ext names args outside the table (or more than SG_MAX_ARGS, or a bad kind)");
    return SG_OK;
}
// Flags the decide kernels raise (the group stage's own checks return before the decide stage runs):
// an EXIT/TRACE whose reference names an event that is not an earlier ENTRY of its resource, and a
// batch starting before the last window a resource already holds (the clock went back).
static int decide_verdict(sg_engine* e, uint32_t bflags) {
    if (bflags & BF_BAD_REF)
        return fail(SG_EINVAL, "an EXIT/TRACE references an event that is not an earlier ENTRY of the same resource");
    if (bflags & BF_BACKWARD)
        return fail(SG_EINVAL, "event timestamps must be non-decreasing across batches (SURVEY Q3)");
    if (bflags & BF_AUX_FULL) return fail(SG_ECAPACITY, "origin/context node pool full (raise aux_node_capacity)");
    if (bflags & BF_LITE_STALE)
        return fail(SG_ESTATE, "internal error (SG_LITE_CHECK): k_lite stored a minute bucket without a load that was not stale");
    // A map that could not place a key has already committed its ring bit and live count (a ghost entry), and a
    // failed k_pq invariant leaves its maps in an unknown state: the engine refuses every later batch.
    if (bflags & BF_PQ_INVARIANT)
        e->fatal = "internal error: a k_pq tile's presorted key subset did not match its accesses";
    else if (bflags & BF_POOL_FULL)  // a map that could not grow may have lost a key (a ghost entry, as below)
        e->fatal = "the hot-parameter map pool is used up (raise param_table_log2)";
    else if (bflags & BF_PTAB_FULL)
        e->fatal = "a hot-parameter map table could not place a key (its map holds a ghost entry)";
    if (bflags & (BF_PQ_INVARIANT | BF_PTAB_FULL | BF_POOL_FULL)) return fail(SG_ECAPACITY, e->fatal + " -- engine unusable");
    return SG_OK;
}

// The oldest batch in flight: wait for its decide stage, record its stage times and the idle time of both streams
// before it, and check its device flags (from the pinned mirror its decide stage filled: nothing is enqueued here).
static int collect(sg_engine* e) {
    if (e->inflight.empty()) return SG_OK;
    const sg_engine::InFlight f = e->inflight.front();
    e->inflight.pop_front();
    hipEvent_t* ev = e->evset[f.set];
    HIPCHK(hipEventSynchronize(ev[4]));
    float g = 0, d = 0, p = 0;
    (void)hipEventElapsedTime(&g, ev[0], ev[1]);
    (void)hipEventElapsedTime(&d, ev[2], ev[3]);
    (void)hipEventElapsedTime(&p, ev[3], ev[4]);
    (void)hipGetLastError();
    e->last_ms[0] = g; e->last_ms[1] = d; e->last_ms[2] = p; e->last_ms[3] = (double)g + d + p;
    e->tlog.push_back({(double)g, (double)d, (double)p, (double)g + d + p});
    if (e->tlog.size() > 4096) e->tlog.erase(e->tlog.begin(), e->tlog.begin() + 2048);
    // the gaps: from the end events of the batch handed off before this one (its set is intact: N_SETS); the
    // engine's first batch has none
    float ga = 0, gb = 0;
    const uint64_t collected = e->seq - e->inflight.size() - 1;  // batches handed off before this one
    if (collected > 0) {
        hipEvent_t* pv = e->evset[(f.set + sg_engine::N_SETS - 1) % sg_engine::N_SETS];
        // as measured: a wrong pairing of event sets shows as a negative gap or, where an event was not recorded, NaN
        if (hipEventElapsedTime(&ga, pv[1], ev[0]) != hipSuccess) ga = NAN;
        if (hipEventElapsedTime(&gb, pv[4], ev[2]) != hipSuccess) gb = NAN;
        (void)hipGetLastError();
    }
    e->glog.push_back({(double)ga, (double)gb});
    if (e->glog.size() > 4096) e->glog.erase(e->glog.begin(), e->glog.begin() + 2048);
    const uint32_t* mir = e->h_mirror + (size_t)f.set * BS_MIRROR_WORDS;
    const uint32_t bflags = mir[BS_FLAGS];
    e->spans_total += mir[BS_NSPAN];
    e->hot_marked_last = f.hot_marked;
    e->ublk_last[0] = f.ublk_coop;
    e->ublk_last[1] = f.ublk_lane;
    e->ublk_last[2] = mir[BS_UBLK_WORDS];
    // the embedded token server's read-back: BS_EMB_REQ .. BS_EMB_AHEAD (requests, answers by class, words written ahead)
    for (int i = 0; i < 9; ++i) e->emb_last[i] = mir[BS_EMB_REQ + i];
    e->emb_last[9] = f.emb_coop;
    e->emb_last[10] = f.emb_lane;
    e->emb_last[11] = 0;  // (no late lane pass: rules with cluster_fallback_to_local are refused)
    if (e->emb_timed && mir[BS_EMB_REQ]) {  // (the batch's events are done: its post end was waited for above)
        for (int i = 0; i < 3; ++i) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, e->emb_t[i], e->emb_t[i + 1]);
            e->emb_ms[i] = ms;
        }
        (void)hipGetLastError();
        e->emb_timed = false;
    }
    return decide_verdict(e, bflags);
}
// every batch in flight done (called by the API functions that read or write engine state)
// the authority table the kernels read: null unless authority rules are loaded (the kernels then run as without)
static inline const AuthDesc* dev_auth(const sg_engine* e) { return e->auth_on ? e->d_auth : nullptr; }
static inline const uint32_t* dev_auth_ids(const sg_engine* e) { return e->auth_on ? e->d_auth_ids : nullptr; }

// A batch that is grouped and not handed off yet gets its verdict and its decide stage here first, so every call
// but an async submit leaves no batch behind.  The first error wins; the later batches are still collected.
static int drain(sg_engine* e) {
    int rc = e->held_rc;
    std::string msg = e->held_msg;
    e->held_rc = 0;
    auto note = [&](int r) {
        if (r && !rc) { rc = r; msg = g_err; }
    };
    note(handoff(e));
    while (!e->inflight.empty()) note(collect(e));  // oldest first
    HIPCHK(hipStreamSynchronize(e->stream));
    return rc ? fail(rc, msg) : SG_OK;
}
// drain() for the diagnostics exports, which have no way to return an error: an async batch's verdict met here is
// kept for the next ABI call, not swallowed
static void drain_hold(sg_engine* e) {
    const int rc = drain(e);
    if (rc) { e->held_rc = rc; e->held_msg = g_err; }
}

// what the rule compiler (compile.h) reads of the engine
static CompileEnv compile_env(const sg_engine* e) {
    return CompileEnv{e->names, e->ids, e->origin_ids, e->context_ids, e->tm_base, e->pmap_index, e->psid_of, e->tmaps,
                      e->cfg.max_resources, e->cfg.max_rules, e->cfg.cold_factor,
                      e->mix_on, e->mix_pq, e->pv_on, e->pv_pq, e->emb_on};
}

// Compile the host lists (compile.h) and put the tables on the device.
int upload_rules(sg_engine* e, bool reset_flow_state, bool reset_deg_state, bool reset_par_state) {
    uint32_t R = e->cfg.max_resources;
    // previous rule states to carry over when a kind was not reloaded
    std::vector<RState> old_rst;
    std::vector<Prog> old_prog;
    if ((!reset_flow_state || !reset_deg_state || !reset_par_state) && e->n_dev_rules) {
        old_rst.resize(e->n_dev_rules);
        old_prog.resize(R);
        HIPCHK(hipMemcpy(old_rst.data(), e->d_rstate, e->n_dev_rules * sizeof(RState), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(old_prog.data(), e->d_prog, R * sizeof(Prog), hipMemcpyDeviceToHost));
    }
    Compiled C = compile_rules(RuleLists{e->params, e->res_par, e->flows, e->res_flow, e->degs, e->res_deg}, compile_env(e));
    if (C.err) return fail(C.err, C.msg);
    // carry controller / breaker state of kinds that were not reloaded
    carry_state(old_prog, old_rst, C.prog, C.rst, !reset_par_state, !reset_flow_state, !reset_deg_state);
    const std::vector<DRule>& rules = C.rules;
    const std::vector<DHot>& hot = C.hot;
    const std::vector<uint32_t>& members = C.members;
    if (!C.comp.empty()) {
        // ClusterNode existence of the members from here on: NI_TOUCHED (a chain grant means an ENTRY of
        // the resource was decided in a finished batch: no batch is in flight during a rule load)
        std::vector<NodeInfo> ni(members.size());
        for (size_t k = 0; k < members.size(); ++k)
            HIPCHK(hipMemcpy(&ni[k], e->d_info + members[k], sizeof(NodeInfo), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < members.size(); ++k) {
            if (ni[k].flags & NI_CHAIN) ni[k].flags |= NI_TOUCHED;
            HIPCHK(hipMemcpy(e->d_info + members[k], &ni[k], sizeof(NodeInfo), hipMemcpyHostToDevice));
        }
        // their param maps at full size: a member's events sort under the representative, so the per-segment
        // growth (k_pm_grow) never sees them
        if (e->d_pmap) {
            const std::set<uint32_t> ms(members.begin(), members.end());
            std::vector<uint32_t> ids;
            for (uint32_t i = 0; i < (uint32_t)e->pmap_key.size(); ++i)
                if ((e->pmap_key[i] & TMAP_KEY) && ms.count((uint32_t)(e->pmap_key[i] >> 8))) ids.push_back(i);
            for (const auto& kv : e->psid_of) {
                auto it = e->ids.find(kv.first.substr(0, kv.first.find('\0')));
                auto pi = e->pmap_index.find(kv.second);
                if (it != e->ids.end() && ms.count(it->second) && pi != e->pmap_index.end()) ids.push_back(pi->second);
            }
            if (!ids.empty()) {
                uint32_t* d_ids = nullptr;
                HIPCHK(hipMalloc(&d_ids, ids.size() * 4));
                HIPCHK(hipMemcpy(d_ids, ids.data(), ids.size() * 4, hipMemcpyHostToDevice));
                DevState Sg{};
                std::memset(&Sg, 0, sizeof(Sg));
                Sg.pmap = e->d_pmap; Sg.pbkt = e->d_pbkt; Sg.pdat = e->d_pdat; Sg.pbm = e->d_pbm;
                HIPCHK(hipMemset(e->d_small + SM_FLAGS, 0, 4));
                HIPCHK(launch_pm_grow_ids(d_ids, (uint32_t)ids.size(), Sg, e->d_pool_next, e->pool_nb, e->d_small + SM_FLAGS, e->stream));
                uint32_t fl = 0;
                HIPCHK(hipMemcpyAsync(&fl, e->d_small + SM_FLAGS, 4, hipMemcpyDeviceToHost, e->stream));
                HIPCHK(hipStreamSynchronize(e->stream));
                (void)hipFree(d_ids);
                if (fl & (BF_POOL_FULL | BF_PTAB_FULL))
                    return fail(SG_ECAPACITY, "hot-parameter map pool too small for the maps of STRATEGY_RELATE members "
                                              "(raise param_table_log2)");
            }
        }
    }
    if (rules.size() > e->rules_cap) {
        dfree(e->d_rules); dfree(e->d_rstate);
        e->rules_cap = (uint32_t)std::max<size_t>(rules.size(), 1024);
        HIPCHK(hipMalloc(&e->d_rules, e->rules_cap * sizeof(DRule)));
        HIPCHK(hipMalloc(&e->d_rstate, e->rules_cap * sizeof(RState)));
    }
    if (hot.size() > e->hot_cap) {
        dfree(e->d_hot);
        e->hot_cap = (uint32_t)std::max<size_t>(hot.size(), 1024);
        HIPCHK(hipMalloc(&e->d_hot, e->hot_cap * sizeof(DHot)));
    }
    HIPCHK(hipDeviceSynchronize());
    if (!rules.empty()) {
        HIPCHK(hipMemcpy(e->d_rules, rules.data(), rules.size() * sizeof(DRule), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(e->d_rstate, C.rst.data(), C.rst.size() * sizeof(RState), hipMemcpyHostToDevice));
    }
    if (!hot.empty()) HIPCHK(hipMemcpy(e->d_hot, hot.data(), hot.size() * sizeof(DHot), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->d_prog, C.prog.data(), R * sizeof(Prog), hipMemcpyHostToDevice));
    if (!C.emb_res.empty()) {  // [res] -> flowId, read for XF_EMB resources only
        if (!e->d_emb_flow) HIPCHK(hipMalloc(&e->d_emb_flow, (uint64_t)R * 8));
        std::vector<int64_t> flow_of(R, 0);
        for (const auto& er : C.emb_res) flow_of[er.first] = er.second;
        HIPCHK(hipMemcpy(e->d_emb_flow, flow_of.data(), (uint64_t)R * 8, hipMemcpyHostToDevice));
    }
    e->emb_n = (uint32_t)C.emb_res.size();
    e->n_dev_rules = (uint32_t)rules.size();
    e->has_mix = C.any_mix;
    e->has_head = C.any_head;
    e->has_multi = C.any_multi;
    if (C.comp.empty()) {
        dfree(e->d_comp);
    } else {
        if (!e->d_comp) HIPCHK(hipMalloc(&e->d_comp, (uint64_t)R * 4));
        HIPCHK(hipMemcpy(e->d_comp, C.comp.data(), (uint64_t)R * 4, hipMemcpyHostToDevice));
    }
    return SG_OK;
}

// The size and embedded-shape refusals of compile.h for the lists a loader is about to publish
static int check_rule_limits(const sg_engine* e, const RuleLists& L) {
    std::string msg;
    const int rc = rule_limits(L, compile_env(e), msg);
    return rc ? fail(rc, msg) : SG_OK;
}
static int check_emb_shape(const std::vector<FlowR>& flows, const std::vector<std::vector<int>>& res_flow,
                           const std::vector<std::vector<int>>& res_par) {
    std::string msg;
    const int rc = emb_refuse(flows, res_flow, res_par, msg);
    return rc ? fail(rc, msg) : SG_OK;
}

uint32_t intern(sg_engine* e, const std::string& name) {
    auto it = e->ids.find(name);
    if (it != e->ids.end()) return it->second;
    uint32_t id = (uint32_t)e->names.size();
    e->ids.emplace(name, id);
    e->names.push_back(name);
    return id;
}

template <class V> void resize_lists(sg_engine* e, V& v) {
    if (v.size() < e->names.size()) v.resize(e->names.size());
}

} // namespace

// =====================================================================================
extern "C" {

const char* sg_last_error(void) { return g_err.c_str(); }

void sg_config_default(sg_config* c) {
    std::memset(c, 0, sizeof(*c));
    c->sample_count = 2;
    c->interval_ms = 1000;
    c->statistic_max_rt = 4900;
    c->cold_factor = 3;
    c->occupy_timeout_ms = 500;
    c->max_slot_chain_size = 6000;
    c->switch_on = 1;
    c->device = 0;
    c->max_resources = 1u << 20;
    c->max_rules = 1u << 21;
    c->param_table_log2 = 28;
    c->status_ring_log2 = 28;
    c->max_batch_events = 1u << 25;
    c->cluster_sample_count = 10;
    c->cluster_interval_ms = 1000;
    c->cluster_exceed_count = 1.0;
    c->cluster_max_occupy_ratio = 1.0;
    c->cluster_max_allowed_qps = 30000;
    c->aux_node_capacity = 65536;
}

int sg_engine_create(const sg_config* cfg_in, sg_engine** out) {
    if (!out) return fail(SG_EINVAL, "out is null");
    sg_config cfg;
    if (cfg_in) cfg = *cfg_in;
    else sg_config_default(&cfg);
    if (cfg.sample_count != 2 || cfg.interval_ms != 1000)
        return fail(SG_ENOTSUP, "the device path implements SAMPLE_COUNT=2, INTERVAL=1000 (the reference defaults)");
    if (cfg.cold_factor <= 1) return fail(SG_EINVAL, "cold factor must be > 1");
    if (cfg.max_resources == 0 || cfg.param_table_log2 < 4 || cfg.param_table_log2 > 34 || cfg.status_ring_log2 < 10 ||
        cfg.status_ring_log2 > 36)
        return fail(SG_EINVAL, "bad capacity in sg_config");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(SG_EDEVICE, "no HIP device visible");
    if (cfg.device < 0 || cfg.device >= ndev) return fail(SG_EDEVICE, "device ordinal out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg.device) != hipSuccess) return fail(SG_EDEVICE, "hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(SG_EDEVICE, std::string("this build targets gfx950, found ") + prop.gcnArchName);
    sg_engine* e = new sg_engine();
    e->cfg = cfg;
    e->device = cfg.device;
    auto bad = [&](int rc) { sg_engine_destroy(e); return rc; };
    if (hipSetDevice(e->device) != hipSuccess) return bad(fail(SG_EDEVICE, "hipSetDevice failed"));
    // The group stage (the critical path of the two-slot pipeline) gets the highest stream priority,
    // so that its short bandwidth-bound kernels are dispatched into the CUs the long decide kernels
    // free (C4: 4.53 -> 4.34 ms per batch).  SG_STREAM_PRIO=0: default priorities; =1: decide first.
    int prio_lo = 0, prio_hi = 0;
    const char* sp = std::getenv("SG_STREAM_PRIO");
    if (!(sp && sp[0] == '0')) (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    if (!(sp && sp[0] == '1')) std::swap(prio_lo, prio_hi);
    if (hipStreamCreateWithPriority(&e->stream, hipStreamNonBlocking, prio_hi) != hipSuccess) return bad(fail(SG_EDEVICE, "stream"));
    if (hipStreamCreateWithPriority(&e->gstream, hipStreamNonBlocking, prio_lo) != hipSuccess) {
        return bad(fail(SG_EDEVICE, "stream"));
    }
    for (auto& s : e->evset)
        for (auto& v : s) if (hipEventCreate(&v) != hipSuccess) return bad(fail(SG_EDEVICE, "event"));
    for (auto& B : e->slot) {
        if (hipHostMalloc(&B.h_head, BS_HEAD_WORDS * 4) != hipSuccess) return bad(fail(SG_ENOMEM, "pinned batch head"));
        B.ev = e->evset[0];
    }
    if (hipHostMalloc(&e->h_mirror, sg_engine::N_SETS * BS_MIRROR_WORDS * 4) != hipSuccess)
        return bad(fail(SG_ENOMEM, "pinned batch flags"));
    std::memset(e->h_mirror, 0, sg_engine::N_SETS * BS_MIRROR_WORDS * 4);
    uint64_t R = cfg.max_resources;
    if (hipMalloc(&e->d_sec, R * 2 * sizeof(Bkt)) != hipSuccess || hipMalloc(&e->d_minb, R * 60 * sizeof(Bkt)) != hipSuccess ||
        hipMalloc(&e->d_info, R * sizeof(NodeInfo)) != hipSuccess || hipMalloc(&e->d_prog, R * sizeof(Prog)) != hipSuccess ||
        hipMalloc(&e->d_ring, 1ull << cfg.status_ring_log2) != hipSuccess || hipMalloc(&e->d_small, SM_WORDS * 4) != hipSuccess ||
        hipMalloc(&e->d_sink, 1024 * 4) != hipSuccess || hipMalloc(&e->d_borrow, R * 4 * sizeof(int64_t)) != hipSuccess ||
        hipMalloc(&e->d_prio, R * 4) != hipSuccess || hipMalloc(&e->d_hot_tab, R * 2) != hipSuccess ||
        hipMalloc(&e->d_hot_list, hot_max() * 4) != hipSuccess)
        return bad(fail(SG_ENOMEM, "device allocation of the engine state failed"));
    {   // origin / context node table (open addressing, load <= 2/3 at capacity, power of two)
        const uint64_t cap = std::max<uint32_t>(cfg.aux_node_capacity, 16u);
        uint64_t slots = 32;
        while (2 * slots < 3 * cap) slots <<= 1;
        e->aux_mask = slots - 1;
        e->cfg.aux_node_capacity = (uint32_t)cap;
        if (hipMalloc(&e->d_auxtab, slots * sizeof(AuxNode)) != hipSuccess || hipMalloc(&e->d_auxcnt, 4) != hipSuccess ||
            hipMemsetAsync(e->d_auxtab, 0xFF, slots * sizeof(AuxNode), e->stream) != hipSuccess ||
            hipMemsetAsync(e->d_auxcnt, 0, 4, e->stream) != hipSuccess)
            return bad(fail(SG_ENOMEM, "device allocation of the origin/context node table failed"));
    }
    if (hipMemsetAsync(e->d_prog, 0, R * sizeof(Prog), e->stream) != hipSuccess ||
        hipMemsetAsync(e->d_ring, 0xFF, 1ull << cfg.status_ring_log2, e->stream) != hipSuccess ||
        hipMemsetAsync(e->d_prio, 0, R * 4, e->stream) != hipSuccess ||
        hipMemsetAsync(e->d_hot_tab, 0xFF, R * 2, e->stream) != hipSuccess ||
        launch_init_state(e->d_sec, e->d_minb, e->d_info, e->d_borrow, (uint32_t)R, e->stream) != hipSuccess ||
        hipStreamSynchronize(e->stream) != hipSuccess)
        return bad(fail(SG_EDEVICE, "device initialisation failed"));
    for (auto& s : e->bin_stream)
        if (hipStreamCreateWithPriority(&s, hipStreamNonBlocking, prio_hi) != hipSuccess) return bad(fail(SG_EDEVICE, "stream"));
    if (hipEventCreateWithFlags(&e->fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e->fork0, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e->grown, hipEventDisableTiming) != hipSuccess)
        return bad(fail(SG_EDEVICE, "event"));
    for (auto& v : e->join)
        if (hipEventCreateWithFlags(&v, hipEventDisableTiming) != hipSuccess) return bad(fail(SG_EDEVICE, "event"));
    if (const char* d = std::getenv("SG_DEBUG")) {
        if (d[0] == '1' && hipMalloc(&e->d_dbg, 64 * 8) == hipSuccess) (void)hipMemset(e->d_dbg, 0, 64 * 8);
    }
    if (const char* f = std::getenv("SG_DEBUG_FLAGS")) e->dbg_flags = (uint32_t)std::strtoul(f, nullptr, 0);
    e->radix_group = (e->dbg_flags & 8192) != 0;
    if (const char* f = std::getenv("SG_PROF_BIN")) e->prof_bin = std::atoi(f);  // SG_DEBUG counters of J16/J4/J1
    // decide-bin thresholds (segment lengths); tuning knobs, the defaults are the measured best
    if (const char* v = std::getenv("SG_LANE_MAX")) { e->lane_max = (uint32_t)std::strtoul(v, nullptr, 0); e->bins_pinned = true; }
    if (const char* v = std::getenv("SG_LITE_MAX")) {
        e->lite_max = (uint32_t)std::strtoul(v, nullptr, 0);
        e->lite_pinned = e->bins_pinned = true;
    }
    if (const char* v = std::getenv("SG_J1_MAX")) { e->j1_max = (uint32_t)std::strtoul(v, nullptr, 0); e->bins_pinned = true; }
    if (const char* v = std::getenv("SG_HEAD_MIN")) e->head_min = (uint32_t)std::strtoul(v, nullptr, 0);
    if (const char* v = std::getenv("SG_J4_MAX")) { e->j4_max = (uint32_t)std::strtoul(v, nullptr, 0); e->bins_pinned = true; }
    if (const char* v = std::getenv("SG_PIPELINE")) e->pipeline = v[0] == '1';
    if (const char* v = std::getenv("SG_HANDOFF")) e->handoff_late = v[0] != '0';
    if (const char* v = std::getenv("SG_TINY")) e->tiny_on = v[0] != '0';
    if (const char* v = std::getenv("SG_LITE_CHECK")) { if (v[0] == '1') e->dbg_flags |= LITE_CHECK; }
    // SG_UBLK=0: pre-blocked ENTRYs (SG_F_BLOCKED_UPSTREAM, authority blocks) send their resource to a lane (A/B)
    e->dbg_flags &= ~UBLK_OFF;
    if (const char* v = std::getenv("SG_UBLK")) { if (v[0] == '0') e->dbg_flags |= UBLK_OFF; }
    if (const char* v = std::getenv("SG_RADIX_BELOW")) e->radix_below = std::strtoull(v, nullptr, 0);
    if (const char* v = std::getenv("SG_TOK_WIDE")) e->tok_wide = std::atoi(v) == 512 ? 512u : 1024u;
    if (const char* v = std::getenv("SG_TOK_LIGHT")) e->tok_light = (uint32_t)std::strtoul(v, nullptr, 0);
    if (const char* v = std::getenv("SG_TOK_NS")) e->tok_ns = v[0] == '1';
    // the param value table's capacities (pvtab.h): 2^4 .. 2^24 slots at first, up to 2^26 (18 GB of slots)
    if (const char* v = std::getenv("SG_PV_LOG2")) e->pv_log2 = (uint32_t)std::min(24l, std::max(4l, std::strtol(v, nullptr, 0)));
    if (const char* v = std::getenv("SG_PV_MAX_LOG2")) e->pv_max_log2 = (uint32_t)std::min(26l, std::max(4l, std::strtol(v, nullptr, 0)));
    e->pv_max_log2 = std::max(e->pv_max_log2, e->pv_log2);
    // ServerConstants.DEFAULT_NAMESPACE: the limiter every flowId tries until it is assigned elsewhere
    e->ns_names.push_back("default");
    e->ns_of["default"] = 0;
    e->ns_limit.push_back((double)cfg.cluster_max_allowed_qps);
    e->ns_conn.push_back(0);
    if (const char* v = std::getenv("SG_J1_STREAM")) e->j1_stream = std::atoi(v);
    if (const char* v = std::getenv("SG_PQ")) e->pq_on = v[0] != '0';
    if (const char* v = std::getenv("SG_MIX")) e->mix_on = v[0] != '0';
    if (const char* v = std::getenv("SG_MIX_PQ")) e->mix_pq = v[0] != '0';
    if (const char* v = std::getenv("SG_PTOK_VP")) e->ptok_vp = v[0] != '0';
    if (const char* v = std::getenv("SG_PTOK_MIN")) e->ptok_min = std::strtoull(v, nullptr, 0);
    if (const char* v = std::getenv("SG_PV_PQ")) e->pv_pq = v[0] != '0';
    if (const char* v = std::getenv("SG_PV")) e->pv_on = v[0] != '0';
    e->pvt_on = e->pv_on;
    if (const char* v = std::getenv("SG_PVT")) e->pvt_on = v[0] != '0';
    if (const char* v = std::getenv("SG_PQ_WIDE")) e->pq_wide = (uint32_t)std::strtoul(v, nullptr, 0);
    if (const char* v = std::getenv("SG_SKIP_MIN")) {
        e->skip_min = std::max<uint32_t>(1u, (uint32_t)std::strtoul(v, nullptr, 0));
        e->skip_pinned = true;
    }
    *out = e;
    return SG_OK;
}

// diagnostics export (not part of the ABI): SG_DEBUG=1 counters of the cooperative J16 bin,
// accumulated over batches (see decide.hip k_jac)
// diagnostics export (not part of the ABI): stage times of the batches collected since the last call,
// 4 doubles each ([group, decide, post, total] ms); returns the number of batches written
extern "C" int sgx_timing_log(sg_engine* e, double* out, int cap) {
    if (!e || !out) return 0;
    drain_hold(e);
    int k = 0;
    for (; k < cap && k < (int)e->tlog.size(); ++k)
        for (int j = 0; j < 4; ++j) out[4 * k + j] = e->tlog[k][j];
    e->tlog.clear();
    return k;
}
// diagnostics export (not part of the ABI): for the batches collected since the last call, how long each stream stood
// empty before the batch, 2 doubles each: [group stream: the previous batch's group end to this batch's group start,
// decide stream: the previous batch's post end to this batch's decide start] ms; 0 for the engine's first batch
extern "C" int sgx_gap_log(sg_engine* e, double* out, int cap) {
    if (!e || !out) return 0;
    drain_hold(e);
    int k = 0;
    for (; k < cap && k < (int)e->glog.size(); ++k)
        for (int j = 0; j < 2; ++j) out[2 * k + j] = e->glog[k][j];
    e->glog.clear();
    return k;
}
// diagnostics export (not part of the ABI): frozen span slots recorded by the cooperative kernels so far
extern "C" unsigned long long sgx_spans_total(sg_engine* e) {
    if (!e) return 0;
    drain_hold(e);
    return e->spans_total;
}
// diagnostics export: hot ids whose side tables the last collected batch built (0 on the radix stage and with
// SG_DEBUG_FLAGS & 32768, which build them everywhere)
extern "C" unsigned int sgx_hot_marked(sg_engine* e) {
    if (!e) return 0;
    drain_hold(e);
    return e->hot_marked_last;
}
// diagnostics export: the pre-blocked placement of the last collected batch: [0] segments of PM_UBLK resources in
// cooperative bins (SEG_UBLK), [1] in lane bins, [2] RF_UBLK words k_ublk_words wrote.  Returns the values written.
extern "C" int sgx_preblocked_last(sg_engine* e, unsigned long long* out, int cap) {
    if (!e || !out) return 0;
    drain_hold(e);
    int k = 0;
    for (; k < 3 && k < cap; ++k) out[k] = e->ublk_last[k];
    return k;
}
// diagnostics export: zero the SG_DEBUG counters ([20] is a running minimum)
extern "C" int sgx_debug_reset(sg_engine* e) {
    if (!e || !e->d_dbg) return 0;
    drain_hold(e);
    unsigned long long z[64] = {0};
    z[20] = ~0ull;
    return hipMemcpy(e->d_dbg, z, sizeof(z), hipMemcpyHostToDevice) == hipSuccess ? 1 : 0;
}
extern "C" int sgx_debug_counters(sg_engine* e, unsigned long long* out, int cap) {
    if (!e || !e->d_dbg || !out) return 0;
    int k = cap < 64 ? cap : 64;
    if (hipDeviceSynchronize() != hipSuccess) return 0;
    if (hipMemcpy(out, e->d_dbg, (size_t)k * 8, hipMemcpyDeviceToHost) != hipSuccess) return 0;
    return k;
}

// diagnostics export (not part of the ABI; parity tests): an origin (kind 0) / context (kind 1) node of res.
// out[0..15] = second window buckets {ws, pass, block, exc, succ, rt, occ, minRt} x 2, out[16] = curThreadNum,
// out[17..20] = minute pass history {ws, pass} per second parity; returns 1, 0 if the node does not exist.
extern "C" int sgx_read_aux_node(sg_engine* e, uint32_t res, uint32_t kind, uint32_t id, long long* out) {
    if (!e || !out || drain(e) != SG_OK) return -1;
    const unsigned long long key = ((unsigned long long)res << 32) | ((unsigned long long)kind << 31) | (id & 0x7FFFFFFFu);
    uint64_t h = mix64(key) & e->aux_mask;
    for (uint64_t probe = 0; probe <= e->aux_mask; ++probe) {
        AuxNode a;
        if (hipMemcpy(&a, e->d_auxtab + h, sizeof(a), hipMemcpyDeviceToHost) != hipSuccess) return -1;
        if (a.key == AUX_EMPTY) return 0;
        if (a.key == key) {
            for (int p = 0; p < 2; ++p) {
                const Bkt& b = a.sec[p];
                const int64_t v[8] = {b.ws, b.pass, b.block, b.exc, b.succ, b.rt, b.occ, b.minrt};
                for (int k = 0; k < 8; ++k) out[8 * p + k] = v[k];
            }
            out[16] = a.thread;
            out[17] = a.mws[0]; out[18] = a.mpass[0]; out[19] = a.mws[1]; out[20] = a.mpass[1];
            return 1;
        }
        h = (h + 1) & e->aux_mask;
    }
    return 0;
}
// diagnostics export: the last batch's value-parallel passes (pvalue.hip), out = {pre pass: listed segments it decided,
// accesses, blocked stretches the walk jumped; post pass: segments eligible, ops, segments committed; the pre
// pass's longest walk (steps, when over 256)}
extern "C" int sgx_pv_last(sg_engine* e, unsigned long long* out) {
    if (!e || !out || drain(e) != SG_OK) return -1;
    out[0] = out[1] = out[2] = out[3] = out[4] = out[5] = out[6] = 0;
    if (!e->d_pvseg || !e->d_pvtot || !e->pv_last_m) return 0;
    std::vector<PvSeg> v(e->pv_last_m);
    uint32_t tot[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpy(v.data(), e->d_pvseg, v.size() * sizeof(PvSeg), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (hipMemcpy(tot, e->d_pvtot, 32, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    for (const auto& s : v) out[0] += s.ok ? 1 : 0;
    out[1] = tot[0];
    out[2] = tot[2];
    out[6] = tot[3];
    if (e->pvt_on && e->d_pvtseg) {
        if (hipMemcpy(v.data(), e->d_pvtseg, v.size() * sizeof(PvSeg), hipMemcpyDeviceToHost) != hipSuccess) return -1;
        for (const auto& s : v) out[3] += s.ok ? 1 : 0;
        out[4] = tot[4];
        out[5] = tot[7];
    }
    if (!e->pv_on) out[0] = out[1] = out[2] = out[6] = 0;
    return 0;
}
// diagnostics export: the param map pool, out = {pool buckets, buckets taken, taken at the last compaction,
// compactions between batches, compactions inside a batch (on the device)}
extern "C" int sgx_param_pool(sg_engine* e, unsigned long long* out) {
    if (!e || !out || drain(e) != SG_OK) return -1;
    unsigned long long ctl[PC_WORDS] = {0, 0, 0, 0};
    if (e->d_pool_next && hipMemcpy(ctl, e->d_pool_next, sizeof(ctl), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    out[0] = e->pool_nb; out[1] = ctl[PC_NEXT]; out[2] = ctl[PC_FLOOR]; out[3] = e->n_compact; out[4] = ctl[PC_RESCUES];
    return 0;
}

static int compact_pmaps(sg_engine* e);
// diagnostics export: compact the param map pool now, between batches (tests run the compaction at full size)
extern "C" int sgx_param_compact(sg_engine* e) {
    if (!e || drain(e) != SG_OK) return -1;
    if (!e->pool_nb) return 0;
    if (compact_pmaps(e) != SG_OK) return -1;
    ++e->n_compact;
    return 0;
}

static void free_pv(sg_engine* e);
static void cm_free_flows(sg_engine* e);
static void cm_free_cands(sg_engine* e);

int sg_engine_destroy(sg_engine* e) {
    if (!e) return SG_OK;
    (void)hipSetDevice(e->device);
    // a batch that is grouped and not handed off is dropped: its group stage ends by itself, nothing waits for it
    e->grouped = -1;
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    if (e->gstream) (void)hipStreamSynchronize(e->gstream);
    dfree(e->d_sec); dfree(e->d_minb); dfree(e->d_info); dfree(e->d_prog); dfree(e->d_rules); dfree(e->d_rstate);
    dfree(e->d_hot); dfree(e->d_pmap); dfree(e->d_pbkt); dfree(e->d_pdat); dfree(e->d_pbm); dfree(e->d_ppre); dfree(e->d_tmid); dfree(e->d_ring); dfree(e->d_small); dfree(e->d_sink);
    dfree(e->d_pool_next); dfree(e->d_pmoves); dfree(e->d_pbkt2); dfree(e->d_pdat2); dfree(e->d_pcwork);
    if (e->h_pool_next) (void)hipHostFree(e->h_pool_next);
    free_pv(e);
    dfree(e->d_pvseg); dfree(e->d_pvtseg); dfree(e->d_pvtot); dfree(e->d_pvrest);
    if (e->gstream) (void)hipStreamSynchronize(e->gstream);
    for (auto& B : e->slot) free_slot(B);
    dfree(e->d_auth); dfree(e->d_auth_ids);
    dfree(e->d_prio); dfree(e->d_hot_tab); dfree(e->d_hot_list); dfree(e->d_hot_part); dfree(e->d_hot_hb); dfree(e->d_need); dfree(e->d_edges); dfree(e->d_comp); dfree(e->d_auxtab); dfree(e->d_auxpool); dfree(e->d_auxcnt); dfree(e->d_auxmeta);
    dfree(e->d_pflow); dfree(e->d_phot); dfree(e->d_pftab); dfree(e->d_pvtab); dfree(e->d_preq); dfree(e->d_pvals);
    dfree(e->d_cflow); dfree(e->d_cbkt); dfree(e->d_ctab); dfree(e->d_nslim); dfree(e->d_nslimit); dfree(e->d_nsb); dfree(e->d_borrow); dfree(e->d_keyring);
    dfree(e->d_treq); dfree(e->d_tres); dfree(e->d_tfidx); dfree(e->d_tbounds);
    dfree(e->d_emb_flow); dfree(e->d_emb_side); dfree(e->d_emb_idx); dfree(e->d_emb_cnt); dfree(e->d_emb_part);
    for (auto& x : e->emb_ev)
        if (x) (void)hipEventDestroy(x);
    for (auto& x : e->emb_t)
        if (x) (void)hipEventDestroy(x);
    dfree(e->d_snap_cnt); dfree(e->d_snap_off); dfree(e->d_snap_out); dfree(e->d_dbg);
    dfree(e->d_inb); dfree(e->d_inbpart);
    dfree(e->d_ks_key); dfree(e->d_ks_idx); dfree(e->d_ks_marks);
    for (auto& v : e->ks_ev) if (v) (void)hipEventDestroy(v);
    dfree(e->d_pvcnt); dfree(e->d_pvspare); dfree(e->d_ptst); dfree(e->d_ptserial); dfree(e->d_ptdedup);
    for (auto& v : e->pv_ev) if (v) (void)hipEventDestroy(v);
    cm_free_flows(e);
    cm_free_cands(e);
    dfree(e->d_cm_cnt);
    for (auto& v : e->cm_ev) if (v) (void)hipEventDestroy(v);
    for (auto& s : e->evset)
        for (auto& v : s) if (v) (void)hipEventDestroy(v);
    for (auto& B : e->slot) if (B.h_head) (void)hipHostFree(B.h_head);
    if (e->h_mirror) (void)hipHostFree(e->h_mirror);
    if (e->gstream) (void)hipStreamDestroy(e->gstream);
    for (auto& v : e->join) if (v) (void)hipEventDestroy(v);
    if (e->fork) (void)hipEventDestroy(e->fork);
    if (e->fork0) (void)hipEventDestroy(e->fork0);
    if (e->grown) (void)hipEventDestroy(e->grown);
    for (auto& s : e->bin_stream) if (s) (void)hipStreamDestroy(s);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
    return SG_OK;
}

int sg_register_resources(sg_engine* e, const char* const* names, uint32_t n, uint32_t* out_ids) {
    if (!e || (n && !names)) return fail(SG_EINVAL, "null argument");
    if (int rc = drain(e)) return rc;
    for (uint32_t i = 0; i < n; ++i) {
        if (!names[i]) return fail(SG_EINVAL, "null resource name");
        auto it = e->ids.find(names[i]);
        uint32_t id;
        if (it != e->ids.end()) id = it->second;
        else {
            if (e->names.size() >= e->cfg.max_resources) return fail(SG_ECAPACITY, "max_resources reached");
            id = intern(e, names[i]);
        }
        if (out_ids) out_ids[i] = id;
    }
    return SG_OK;
}

int sg_resource_id(sg_engine* e, const char* name, uint32_t* out_id) {
    if (!e || !name || !out_id) return fail(SG_EINVAL, "null argument");
    auto it = e->ids.find(name);
    if (it == e->ids.end()) return fail(SG_ENOTFOUND, std::string("unknown resource ") + name);
    *out_id = it->second;
    return SG_OK;
}

int sg_param_key(sg_engine* e, const char* value, const char* class_type, uint64_t* out_key) {
    (void)e;
    if (!out_key) return fail(SG_EINVAL, "null out_key");
    *out_key = param_key(value, class_type);
    return SG_OK;
}

static int register_rule_resource(sg_engine* e, const char* name, uint32_t* id) {
    auto it = e->ids.find(name);
    if (it != e->ids.end()) { *id = it->second; return SG_OK; }
    if (e->names.size() >= e->cfg.max_resources) return fail(SG_ECAPACITY, "max_resources reached");
    *id = intern(e, name);
    return SG_OK;
}
// ... as the callback of the list builders (rules.h): false with the reason in rc
static auto rule_resource(sg_engine* e, int& rc) {
    return [e, &rc](const char* name, uint32_t* id) { rc = register_rule_resource(e, name, id); return rc == SG_OK; };
}

// ---- exact parameter keys (pkeys.h, keysweep.hip; the epoch rule is in the header)
int sg_param_intern(sg_engine* e, const char* value, const char* class_type, uint64_t* out_key) {
    if (!e || !out_key) return fail(SG_EINVAL, "null argument");
    *out_key = e->pkeys.intern(value, class_type);
    return SG_OK;
}

int sg_param_intern_batch(sg_engine* e, const char* const* values, const char* const* class_types, uint32_t n,
                          uint64_t* out_keys) {
    if (!e || (n && (!values || !out_keys))) return fail(SG_EINVAL, "null argument");
    for (uint32_t i = 0; i < n; ++i) out_keys[i] = e->pkeys.intern(values[i], class_types ? class_types[i] : nullptr);
    return SG_OK;
}

int sg_param_keys_sweep(sg_engine* e) {
    if (!e) return fail(SG_EINVAL, "null engine");
    HIPCHK(hipSetDevice(e->device));
    if (int rc = drain(e)) return rc;  // every submitted batch: its keys are in the maps and the ring by now
    const auto t_start = std::chrono::steady_clock::now();
    std::vector<uint64_t> cand;
    const uint64_t E = e->pkeys.sweep_begin(cand);
    const uint64_t nc = cand.size();
    std::vector<uint32_t> held((nc + 31) / 32, 0u);
    uint64_t n_held = 0;
    e->ks_scan_ms[0] = e->ks_scan_ms[1] = e->ks_scan_ms[2] = 0;
    const bool dev = (e->d_pmap && !e->pmap_key.empty()) || e->d_keyring || e->d_pvtab;
    if (nc && nc >= (1ull << 30)) return fail(SG_ECAPACITY, "too many sweep candidates for one table");
    if (nc && dev) {
        uint64_t slots = 16;  // a power of two, at most half full
        while (slots < 2 * nc) slots <<= 1;
        if (slots > e->ks_cap) {
            dfree(e->d_ks_key); dfree(e->d_ks_idx); dfree(e->d_ks_marks);
            e->ks_cap = 0;
            HIPCHK(hipMalloc(&e->d_ks_key, slots * 8));
            HIPCHK(hipMalloc(&e->d_ks_idx, slots * 4));
            HIPCHK(hipMalloc(&e->d_ks_marks, ((slots + 31) / 32) * 4));
            e->ks_cap = slots;
        }
        for (auto& v : e->ks_ev)
            if (!v) HIPCHK(hipEventCreate(&v));
        std::vector<uint64_t> tk(slots, PK_EMPTY);
        std::vector<uint32_t> ti(slots, 0u);
        for (uint64_t i = 0; i < nc; ++i) {  // the probe of keysweep.hip ks_mark
            uint64_t h = (uint32_t)mix64(cand[i]) & (slots - 1);
            while (tk[h] != PK_EMPTY) h = (h + 1) & (slots - 1);
            tk[h] = cand[i];
            ti[h] = (uint32_t)i;
        }
        hipStream_t st = e->stream;
        HIPCHK(hipMemcpyAsync(e->d_ks_key, tk.data(), slots * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(e->d_ks_idx, ti.data(), slots * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(e->d_ks_marks, 0, held.size() * 4, st));
        HIPCHK(launch_keysweep(e->pmap_key.empty() ? nullptr : e->d_pmap, (uint32_t)e->pmap_key.size(), e->d_pbkt,
                               e->pool_nb, e->d_pbm, e->pbm_words, e->d_keyring,
                               e->d_keyring ? 1ull << e->cfg.status_ring_log2 : 0, e->d_pvtab,
                               e->d_pvtab ? (uint64_t)e->pv_mask + 1 : 0, e->d_ks_key, e->d_ks_idx,
                               (uint32_t)(slots - 1), e->d_ks_marks, e->ks_ev, st));
        HIPCHK(hipMemcpyAsync(held.data(), e->d_ks_marks, held.size() * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int k = 0; k < 3; ++k) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, e->ks_ev[k], e->ks_ev[k + 1]) == hipSuccess) e->ks_scan_ms[k] = ms;
        }
        (void)hipGetLastError();
        for (uint32_t w : held) n_held += (uint64_t)__builtin_popcount(w);
    }
    // (a failure above leaves the epoch opened and drops nothing: the candidates are candidates again next time)
    const uint64_t dropped = e->pkeys.sweep_finish(E, cand, held.data());
    ++e->ks_sweeps;
    e->ks_last[0] = nc;
    e->ks_last[1] = n_held;
    e->ks_last[2] = dropped;
    e->ks_last[3] = (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_start).count();
    return SG_OK;
}

int sg_param_keys_stats(sg_engine* e, uint64_t* out, int cap) {
    if (!e || !out) return 0;
    const pk::Stats s = e->pkeys.stats();
    const uint64_t v[8] = {s.entries, s.displaced, s.pinned, e->ks_sweeps, e->ks_last[0], e->ks_last[1], e->ks_last[2],
                           e->ks_last[3]};
    int k = 0;
    for (; k < cap && k < 8; ++k) out[k] = v[k];
    return k;
}
int sg_cluster_param_table_stats(sg_engine* e, uint64_t* out, int cap) {
    if (!e || !out) return 0;
    const uint64_t v[7] = {e->d_pvtab ? (uint64_t)e->pv_mask + 1 : 0, e->pv_claimed, e->pv_live, e->pv_rehashes,
                           e->pv_resizes, e->pv_last_us, 1ull << e->pv_max_log2};
    int k = 0;
    for (; k < cap && k < 7; ++k) out[k] = v[k];
    if (cap > 7) {  // the owners' counters live on the device (every call has returned: nothing is in flight)
        unsigned long long c[3] = {0, 0, 0};
        if (e->d_ptst && hipMemcpy(c, e->d_ptst + 2, sizeof(c), hipMemcpyDeviceToHost) != hipSuccess) {
            (void)hipGetLastError();
            return k;
        }
        for (; k < cap && k < 10; ++k) out[k] = c[k - 7];
    }
    return k;
}
// diagnostics export: the last sweep's scans in ms {maps, key ring, token server values}
extern "C" int sgx_keysweep_scans(sg_engine* e, double* out) {
    if (!e || !out) return -1;
    for (int k = 0; k < 3; ++k) out[k] = e->ks_scan_ms[k];
    return 0;
}

// FlowRuleManager.loadRules -> FlowRuleUtil.buildFlowRuleMap (core/slots/block/flow/FlowRuleUtil.java:89-137)
// ClusterFlowRuleManager.applyClusterFlowRule (csrv/flow/rule/ClusterFlowRuleManager.java:323-363): the
// cluster-mode rules of the list, in list order, FlowRuleUtil.isValidRule; a later rule with the same
// flowId replaces an earlier one (ruleMap.put).  ClusterMetricStatistics.putMetricIfAbsent keeps the
// metric (and its window shape) of a flowId that stays; clearAndResetRulesConditional drops the rest.
static uint64_t tab_hash_h(int64_t k) {  // same mix as cluster.hip tab_hash
    uint64_t z = (uint64_t)k + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint32_t ns_index(const sg_engine* e, int64_t fid) {  // the flowId's namespace ("default" unless assigned)
    auto it = e->flow_ns.find(fid);
    return it == e->flow_ns.end() ? 0u : it->second;
}
static int rebuild_cluster(sg_engine* e, const sg_flow_rule* rules, uint32_t n) {
    std::vector<int64_t> order;                       // flowIds in first-appearance order
    std::unordered_map<int64_t, const sg_flow_rule*> rule_of;
    for (uint32_t i = 0; i < n; ++i) {
        const sg_flow_rule& r = rules[i];
        if (!r.cluster_mode || !flow_valid(r)) continue;
        if (!rule_of.count(r.cluster_flow_id)) order.push_back(r.cluster_flow_id);
        rule_of[r.cluster_flow_id] = &r;
    }
    // current device state of the flows that stay
    const uint32_t nold = (uint32_t)e->cflows.size();
    std::vector<CFlow> old_f(nold);
    std::vector<CBkt> old_b(e->ncbkt);
    if (nold) HIPCHK(hipMemcpy(old_f.data(), e->d_cflow, nold * sizeof(CFlow), hipMemcpyDeviceToHost));
    if (e->ncbkt) HIPCHK(hipMemcpy(old_b.data(), e->d_cbkt, e->ncbkt * sizeof(CBkt), hipMemcpyDeviceToHost));
    std::vector<CFlow> nf;
    std::vector<CBkt> nb;
    std::unordered_map<int64_t, uint32_t> nmap;
    for (int64_t fid : order) {
        const sg_flow_rule& r = *rule_of[fid];
        CFlow f;
        std::memset(&f, 0, sizeof(f));
        auto it = e->cmap.find(fid);
        if (it != e->cmap.end()) {  // metric kept, rule replaced
            f = old_f[it->second];
            const uint32_t ob = f.boff;
            f.boff = (uint32_t)nb.size();
            for (int k = 0; k < f.n; ++k) nb.push_back(old_b[ob + k]);
        } else {
            f.flow_id = fid;
            f.n = r.cluster_sample_count;
            f.interval = r.cluster_window_interval_ms;
            f.connected = e->ns_conn[ns_index(e, fid)];  // ConnectionManager.getConnectedCount(namespace)
            f.boff = (uint32_t)nb.size();
            CBkt z;
            std::memset(&z, 0, sizeof(z));
            z.ws = -1;
            for (int k = 0; k < f.n; ++k) nb.push_back(z);
        }
        f.count = r.count;
        f.thr_type = r.cluster_threshold_type;
        nmap[fid] = (uint32_t)nf.size();
        nf.push_back(f);
    }
    e->cres.clear();
    for (int64_t fid : order) e->cres[fid] = sv(rule_of[fid]->resource);
    uint32_t cap = 16;
    while (cap < 2 * nf.size() + 2) cap <<= 1;
    std::vector<CSlot> tab(cap);
    for (auto& t : tab) { t.key = 0; t.idx = 0xFFFFFFFFu; t.pad = 0; }
    for (uint32_t i = 0; i < nf.size(); ++i) {
        uint64_t h = tab_hash_h(nf[i].flow_id) & (cap - 1);
        while (tab[h].idx != 0xFFFFFFFFu) h = (h + 1) & (cap - 1);
        tab[h].key = nf[i].flow_id;
        tab[h].idx = i;
        tab[h].pad = ns_index(e, nf[i].flow_id);
    }
    dfree(e->d_cflow); dfree(e->d_cbkt); dfree(e->d_ctab);
    if (!nf.empty()) {
        HIPCHK(hipMalloc(&e->d_cflow, nf.size() * sizeof(CFlow)));
        HIPCHK(hipMemcpy(e->d_cflow, nf.data(), nf.size() * sizeof(CFlow), hipMemcpyHostToDevice));
        HIPCHK(hipMalloc(&e->d_cbkt, nb.size() * sizeof(CBkt)));
        HIPCHK(hipMemcpy(e->d_cbkt, nb.data(), nb.size() * sizeof(CBkt), hipMemcpyHostToDevice));
    }
    HIPCHK(hipMalloc(&e->d_ctab, cap * sizeof(CSlot)));
    HIPCHK(hipMemcpy(e->d_ctab, tab.data(), cap * sizeof(CSlot), hipMemcpyHostToDevice));
    e->ctab_mask = cap - 1;
    e->cflows = std::move(nf);
    e->ncbkt = nb.size();
    e->cmap = std::move(nmap);
    return SG_OK;
}

int sg_load_flow_rules(sg_engine* e, const sg_flow_rule* rules, uint32_t n, uint32_t* n_loaded) {
    if (!e || (n && !rules)) return fail(SG_EINVAL, "null argument");
    if (int rc = drain(e)) return rc;  // no batch in flight while the rule tables change
    std::vector<std::string> keys = flow_keys(rules, n);
    if (e->flow_loaded && keys == e->last_flow) { // DynamicSentinelProperty.updateValue: equal -> no-op
        if (n_loaded) *n_loaded = (uint32_t)e->flows.size();
        return SG_OK;
    }
    RuleList<FlowR> L;
    int rrc = SG_OK;
    if (!build_flow_list(rules, n, std::move(keys), rule_resource(e, rrc), L)) return rrc;
    if (int rc = check_rule_limits(e, RuleLists{e->params, e->res_par, L.recs, L.per, e->degs, e->res_deg})) return rc;
    if (e->emb_on)
        if (int rc = check_emb_shape(L.recs, L.per, e->res_par)) return rc;
    // publish
    auto old_flows = std::move(e->flows);
    auto old_per = std::move(e->res_flow);
    auto old_names = std::move(e->rule_names);
    e->flows = std::move(L.recs);
    e->res_flow = std::move(L.per);
    resize_lists(e, e->res_flow);
    e->rule_names.clear();  // the origin / context names the flow rules read (sg_intern_* recompiles on first sight)
    for (auto& f : e->flows) {
        e->rule_names["o\x01" + f.la] = 1;
        if (f.r.strategy == SG_STRATEGY_CHAIN) e->rule_names["c\x01" + f.ref] = 1;
    }
    int rc = upload_rules(e, true, false, false);
    if (rc) {  // the old rules go on deciding: their names too (an origin of theirs interned later recompiles them)
        e->flows = std::move(old_flows);
        e->res_flow = std::move(old_per);
        e->rule_names = std::move(old_names);
        return rc;
    }
    e->last_flow = std::move(L.keys);
    e->flow_loaded = true;
    rc = rebuild_cluster(e, rules, n);
    if (rc) return rc;
    if (n_loaded) *n_loaded = (uint32_t)e->flows.size();
    return SG_OK;
}

// AuthorityRuleManager.loadRules (core/slots/block/authority/AuthorityRuleManager.java:105-157); the rules are
// compiled by authority.h.  Origins are not interned here (ids are dense in first-intern order): a listed name
// without an id matches no event until sg_intern_origin gives it one and patches the lists.
static int upload_authority(sg_engine* e) {
    e->auth_on = false;
    if (e->auth.empty()) return SG_OK;
    const size_t R = e->cfg.max_resources;
    if (!e->d_auth && hipMalloc(&e->d_auth, R * sizeof(AuthDesc)) != hipSuccess)
        return fail(SG_ENOMEM, "device allocation of the authority table failed");
    const size_t ni = std::max<size_t>(1, e->auth.ids.size());
    if (ni > e->auth_ids_cap) {
        dfree(e->d_auth_ids);
        e->auth_ids_cap = 0;
        if (hipMalloc(&e->d_auth_ids, 2 * ni * sizeof(uint32_t)) != hipSuccess)
            return fail(SG_ENOMEM, "device allocation of the authority id lists failed");
        e->auth_ids_cap = 2 * ni;
    }
    HIPCHK(hipMemcpy(e->d_auth, e->auth.desc.data(), R * sizeof(AuthDesc), hipMemcpyHostToDevice));
    if (!e->auth.ids.empty())
        HIPCHK(hipMemcpy(e->d_auth_ids, e->auth.ids.data(), e->auth.ids.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    e->auth_on = true;
    return SG_OK;
}

int sg_load_authority_rules(sg_engine* e, const sg_authority_rule* rules, uint32_t n, uint32_t* n_loaded) {
    if (!e || (n && !rules)) return fail(SG_EINVAL, "null argument");
    HIPCHK(hipSetDevice(e->device));
    if (int rc = drain(e)) return rc;  // no batch in flight while the table changes
    std::vector<std::string> keys(n);
    std::vector<AuthIn> in(n);
    for (uint32_t i = 0; i < n; ++i) {
        const sg_authority_rule& r = rules[i];
        keys[i] = std::string(r.resource ? "r" : "R") + (r.resource ? r.resource : "") + '\x01' + (r.limit_app ? "l" : "L") +
                  (r.limit_app ? r.limit_app : "") + '\x01' + std::to_string(r.strategy);
        in[i] = AuthIn{r.resource, r.limit_app, r.strategy};
    }
    if (e->auth_loaded && keys == e->last_auth) {  // DynamicSentinelProperty.updateValue: an equal list is a no-op
        if (n_loaded) *n_loaded = (uint32_t)e->auth.rules.size();
        return SG_OK;
    }
    AuthTable old = e->auth;
    int rrc = SG_OK;
    const bool ok = e->auth.compile(
        in.data(), n, e->cfg.max_resources,
        [&](const char* name, uint32_t* id) { rrc = register_rule_resource(e, name, id); return rrc == SG_OK; },
        [&](const char* name, uint32_t* id) {
            auto it = e->origin_ids.find(name);
            if (it == e->origin_ids.end()) return false;
            *id = it->second;
            return true;
        });
    if (!ok) return rrc;
    if (int rc = upload_authority(e)) {
        e->auth = std::move(old);
        (void)upload_authority(e);
        return rc;
    }
    e->last_auth = keys;
    e->auth_loaded = true;
    if (n_loaded) *n_loaded = (uint32_t)e->auth.rules.size();
    return SG_OK;
}

// DegradeRuleManager.loadRules (core/slots/block/degrade/DegradeRuleManager.java:112-205)
int sg_load_degrade_rules(sg_engine* e, const sg_degrade_rule* rules, uint32_t n, uint32_t* n_loaded) {
    if (!e || (n && !rules)) return fail(SG_EINVAL, "null argument");
    if (int rc = drain(e)) return rc;  // no batch in flight while the rule tables change
    std::vector<std::string> keys = deg_keys(rules, n);
    bool has_nan = false;
    for (uint32_t i = 0; i < n; ++i) has_nan |= rules[i].count != rules[i].count;
    if (e->deg_loaded && !has_nan && keys == e->last_deg) {
        if (n_loaded) *n_loaded = (uint32_t)e->degs.size();
        return SG_OK;
    }
    RuleList<DegR> L;
    int rrc = SG_OK;
    if (!build_degrade_list(rules, n, std::move(keys), rule_resource(e, rrc), L)) return rrc;
    if (int rc = check_rule_limits(e, RuleLists{e->params, e->res_par, e->flows, e->res_flow, L.recs, L.per})) return rc;
    auto od = std::move(e->degs);
    auto op = std::move(e->res_deg);
    e->degs = std::move(L.recs);
    e->res_deg = std::move(L.per);
    resize_lists(e, e->res_deg);
    int rc = upload_rules(e, false, true, false);
    if (rc) { e->degs = std::move(od); e->res_deg = std::move(op); return rc; }
    e->last_deg = std::move(L.keys);
    e->deg_loaded = true;
    if (n_loaded) *n_loaded = (uint32_t)e->degs.size();
    return SG_OK;
}

// ParamFlowRuleManager.loadRules (param/slots/block/flow/param/ParamFlowRuleManager.java:103-166)
// ClusterParamFlowRuleManager.applyClusterParamRules (csrv/flow/rule/ClusterParamFlowRuleManager.java:318-369):
// cluster-mode rules passing ParamFlowRuleUtil.isValidRule, in list order; the last rule of a flowId wins;
// putMetricIfAbsent keeps the metric (window shape and value counts) of a flowId that stays; the metrics of
// the others are dropped (their value slots leave the table, and so do the dead slots of the flows that stay:
// pvtab.h).  The table keeps its capacity.
static int rebuild_cluster_param(sg_engine* e, const sg_param_rule* rules, const std::vector<ParamR>& all, uint32_t n) {
    std::vector<int64_t> order;
    std::unordered_map<int64_t, uint32_t> rule_of;
    for (uint32_t i = 0; i < n; ++i) {
        const sg_param_rule& r = rules[i];
        if (!r.cluster_mode || !param_valid(r)) continue;
        if (r.cluster_sample_count > CP_MAXN)
            return fail(SG_ENOTSUP, "cluster param rules with sampleCount > 16 are not on the device path");
        if (!rule_of.count(r.cluster_flow_id)) order.push_back(r.cluster_flow_id);
        rule_of[r.cluster_flow_id] = i;
    }
    const uint32_t nold = (uint32_t)e->pflows.size();
    std::vector<PFlow> old_f(nold);
    if (nold) HIPCHK(hipMemcpy(old_f.data(), e->d_pflow, nold * sizeof(PFlow), hipMemcpyDeviceToHost));
    std::vector<PFlow> nf;
    std::vector<PHot> nh;
    std::unordered_map<int64_t, uint32_t> nmap;
    std::vector<uint32_t> remap(nold, PV_EMPTY);  // old flow index -> new (value slots that stay)
    for (int64_t fid : order) {
        const uint32_t ri = rule_of[fid];
        const sg_param_rule& r = rules[ri];
        PFlow f;
        std::memset(&f, 0, sizeof(f));
        auto it = e->pmap.find(fid);
        if (it != e->pmap.end()) {
            f = old_f[it->second];
            remap[it->second] = (uint32_t)nf.size();
        } else {
            f.flow_id = fid;
            f.n = r.cluster_sample_count;
            f.interval = r.cluster_window_interval_ms;
            f.connected = e->ns_conn[ns_index(e, fid)];
            for (int k = 0; k < CP_MAXN; ++k) f.fws[k] = -1;
        }
        f.count = r.count;
        f.thr_type = r.cluster_threshold_type;
        f.hoff = (uint32_t)nh.size();
        f.nhot = (uint32_t)all[ri].hot.size();  // ParamFlowRuleUtil.fillExceptionFlowItems
        for (auto& h : all[ri].hot) { PHot x; x.key = h.first; x.count = h.second; x.pad = 0; nh.push_back(x); }
        nmap[fid] = (uint32_t)nf.size();
        nf.push_back(f);
    }
    std::unordered_map<int64_t, std::string> nres;
    for (int64_t fid : order) nres[fid] = sv(rules[rule_of[fid]].resource);
    const uint32_t cap_v = e->d_pvtab ? e->pv_mask + 1 : 1u << e->pv_log2;
    const bool need_v = !nf.empty() || e->d_pvtab;  // no table until a cluster param rule exists
    std::vector<PVal> vt(need_v ? cap_v : 0);
    if (!need_v) {}
    else if (e->d_pvtab) HIPCHK(hipMemcpy(vt.data(), e->d_pvtab, cap_v * sizeof(PVal), hipMemcpyDeviceToHost));
    else for (auto& v : vt) v.flow = PV_EMPTY;
    // re-insert the live value slots of the flows that stay, under their new flow index (same probe as pv_find)
    std::vector<PVal> keep;
    for (auto& v : vt)
        if (v.flow != PV_EMPTY && v.flow < nold && remap[v.flow] != PV_EMPTY && pv_live(old_f[v.flow], v)) {
            keep.push_back(v);
            keep.back().flow = remap[v.flow];
        }
    for (auto& v : vt) { v.flow = PV_EMPTY; v.key = 0; }
    for (auto& v : keep) {  // (at most half of cap_v: there is a free slot)
        const uint64_t h = pv_probe(vt.data(), cap_v, v.flow, v.key);
        if (h >= cap_v) return fail(SG_ECAPACITY, "cluster param value table is full");
        vt[h] = v;
    }
    uint32_t cap = 16;
    while (cap < 2 * nf.size() + 2) cap <<= 1;
    std::vector<CSlot> tab(cap);
    for (auto& t : tab) { t.key = 0; t.idx = 0xFFFFFFFFu; t.pad = 0; }
    for (uint32_t i = 0; i < nf.size(); ++i) {
        uint64_t h = tab_hash_h(nf[i].flow_id) & (cap - 1);
        while (tab[h].idx != 0xFFFFFFFFu) h = (h + 1) & (cap - 1);
        tab[h].key = nf[i].flow_id;
        tab[h].idx = i;
        tab[h].pad = ns_index(e, nf[i].flow_id);
    }
    dfree(e->d_pflow); dfree(e->d_phot); dfree(e->d_pftab);
    if (!nf.empty()) {
        HIPCHK(hipMalloc(&e->d_pflow, nf.size() * sizeof(PFlow)));
        HIPCHK(hipMemcpy(e->d_pflow, nf.data(), nf.size() * sizeof(PFlow), hipMemcpyHostToDevice));
    }
    if (!nh.empty()) {
        HIPCHK(hipMalloc(&e->d_phot, nh.size() * sizeof(PHot)));
        HIPCHK(hipMemcpy(e->d_phot, nh.data(), nh.size() * sizeof(PHot), hipMemcpyHostToDevice));
    }
    if (need_v) {
        if (!e->d_pvtab) HIPCHK(hipMalloc(&e->d_pvtab, cap_v * sizeof(PVal)));
        HIPCHK(hipMemcpy(e->d_pvtab, vt.data(), cap_v * sizeof(PVal), hipMemcpyHostToDevice));
        e->pv_mask = cap_v - 1;
        e->pv_claimed = keep.size();
    }
    HIPCHK(hipMalloc(&e->d_pftab, cap * sizeof(CSlot)));
    HIPCHK(hipMemcpy(e->d_pftab, tab.data(), cap * sizeof(CSlot), hipMemcpyHostToDevice));
    e->pftab_mask = cap - 1;
    e->pflows = std::move(nf);
    e->pmap = std::move(nmap);
    e->pres = std::move(nres);
    return SG_OK;
}

// ---- ParameterMetric maps (dev_types.h PMap)
// A map's cuckoo table: two-choice buckets of PM_BKT slots at <= 50 % load; its live-stamp ring: >= 4 x cap bits
static uint32_t ring_log2(uint32_t cap) {
    uint32_t k = 10;
    while ((1ull << k) < 4ull * cap + 64) ++k;
    return k;
}

// Lay out one region per map in a fresh pool, carrying the entries, stamps, rings and counters of the maps that
// stay (each at its current size; a new map starts at PM_MIN_NB buckets and grows per batch, k_pm_grow).  The pool
// holds 2^param_table_log2 slots, or less when that is more than the maps could ever take (twice their full
// regions: they grow by doubling).  Everything that can fail (the capacity check, the allocations) happens before
// the engine changes: an SG_ECAPACITY leaves the old maps in place.  Called with the current maps it compacts the
// pool (the regions the maps grew out of are dropped).
static int rebuild_pmaps(sg_engine* e, const std::map<uint32_t, uint32_t>& rcap, const std::set<uint64_t>& tmaps) {
    std::vector<PMap> old(e->pmap_key.size());
    if (!old.empty()) HIPCHK(hipMemcpy(old.data(), e->d_pmap, old.size() * sizeof(PMap), hipMemcpyDeviceToHost));
    std::unordered_map<uint64_t, uint32_t> was;
    for (uint32_t i = 0; i < (uint32_t)e->pmap_key.size(); ++i) was[e->pmap_key[i]] = i;
    std::vector<uint64_t> keys;
    std::vector<PMap> hdr;
    uint64_t nbkt = 0, nword = 0, nfull = 0;
    auto add = [&](uint64_t key, uint32_t cap) {
        PMap m;
        std::memset(&m, 0, sizeof(m));
        m.base = nbkt;
        auto it = was.find(key);
        m.nb = it == was.end() ? PM_MIN_NB : old[it->second].nb;
        m.cap = cap;
        m.rb_log2 = ring_log2(cap);
        m.bm = nword;
        keys.push_back(key);
        hdr.push_back(m);
        nbkt += m.nb;
        nfull += 2ull * map_buckets(cap);
        nword += (1ull << m.rb_log2) / 64;
    };
    for (const auto& kv : rcap) add(kv.first, kv.second);
    for (uint64_t t : tmaps) add(TMAP_KEY | t, PM_BASE_CAP);
    const uint64_t total = nbkt * PM_BKT;
    if (total > (1ull << e->cfg.param_table_log2))
        return fail(SG_ECAPACITY, "hot-parameter maps need " + std::to_string(total) + " slots, param_table_log2 = " +
                                      std::to_string(e->cfg.param_table_log2) + " allows " +
                                      std::to_string(1ull << e->cfg.param_table_log2));
    const uint64_t pool_nb = keys.empty() ? 0 : std::max<uint64_t>(nbkt, std::min<uint64_t>((1ull << e->cfg.param_table_log2) / PM_BKT, nfull + nbkt));
    std::vector<uint64_t> tri_b, tri_d, tri_w;  // {source word, destination word, words} per pool
    for (size_t i = 0; i < keys.size(); ++i) {
        auto it = was.find(keys[i]);
        if (it == was.end()) continue;
        const PMap& o = old[it->second];
        if (o.rb_log2 != hdr[i].rb_log2) continue;  // cannot happen: fixed by the map's identity
        hdr[i].clock = o.clock;
        hdr[i].thr = o.thr;
        hdr[i].live = o.live;
        const uint64_t bw = sizeof(PBucket) / 8, dw = PM_BKT * sizeof(PData) / 8;
        tri_b.insert(tri_b.end(), {o.base * bw, hdr[i].base * bw, (uint64_t)o.nb * bw});
        tri_d.insert(tri_d.end(), {o.base * dw, hdr[i].base * dw, (uint64_t)o.nb * dw});
        tri_w.insert(tri_w.end(), {o.bm, hdr[i].bm, (1ull << o.rb_log2) / 64});
    }
    std::vector<uint32_t> tb(e->names.size(), NO_ID), tmid;
    for (size_t i = 0; i < keys.size(); ++i) {
        if (!(keys[i] & TMAP_KEY)) continue;
        const uint32_t r = (uint32_t)(keys[i] >> 8), idx = (uint32_t)(keys[i] & 0xFF);
        if (r >= tb.size()) tb.resize(r + 1, NO_ID);
        if (tb[r] == NO_ID) { tb[r] = (uint32_t)tmid.size(); tmid.resize(tmid.size() + SG_MAX_ARGS, NO_ID); }
        tmid[tb[r] + idx] = (uint32_t)i;
    }
    PBucket* nbk = nullptr;
    PData* ndt = nullptr;
    uint64_t* nbm = nullptr;
    uint32_t* npr = nullptr;
    PMap* nh = nullptr;
    uint32_t* nt = nullptr;
    uint64_t* dtri = nullptr;
    // the compactions' second pool and scratch, allocated with the pool (a compaction that is needed later cannot
    // fail for memory: ADVICE r4)
    PBucket* nbk2 = nullptr;
    PData* ndt2 = nullptr;
    uint32_t* nwork = nullptr;
    const uint64_t mcap = std::max<uint64_t>(e->pmoves_cap, keys.size());
    auto release = [&]() {
        dfree(nbk); dfree(ndt); dfree(nbm); dfree(npr); dfree(nh); dfree(nt); dfree(dtri); dfree(nbk2); dfree(ndt2);
        dfree(nwork);
    };
    const size_t ntri = std::max(tri_b.size(), std::max(tri_d.size(), tri_w.size()));
    if ((nbkt && (hipMalloc(&nbk, pool_nb * sizeof(PBucket)) != hipSuccess ||
                  hipMalloc(&ndt, pool_nb * PM_BKT * sizeof(PData)) != hipSuccess ||
                  hipMalloc(&nbm, nword * 8) != hipSuccess || hipMalloc(&npr, nword * 4) != hipSuccess ||
                  hipMalloc(&nbk2, pool_nb * sizeof(PBucket)) != hipSuccess ||
                  hipMalloc(&ndt2, pool_nb * PM_BKT * sizeof(PData)) != hipSuccess ||
                  hipMalloc(&nwork, (3ull * mcap + 4096) * 4) != hipSuccess)) ||
        (!hdr.empty() && hipMalloc(&nh, hdr.size() * sizeof(PMap)) != hipSuccess) ||
        (!tmid.empty() && hipMalloc(&nt, tmid.size() * 4) != hipSuccess) ||
        (ntri && hipMalloc(&dtri, 3 * ntri * 8) != hipSuccess)) {
        release();
        (void)hipGetLastError();
        return fail(SG_ECAPACITY, "device memory for " + std::to_string(pool_nb * PM_BKT) +
                                      " hot-parameter map slots and their compaction copy (lower param_table_log2)");
    }
    if (!e->d_pool_next) {
        HIPCHK(hipMalloc(&e->d_pool_next, PC_WORDS * 8));
        HIPCHK(hipMemset(e->d_pool_next, 0, PC_WORDS * 8));
        HIPCHK(hipHostMalloc(&e->h_pool_next, PC_WORDS * 8));
        std::memset(e->h_pool_next, 0, PC_WORDS * 8);
    }
    if (nbkt) {
        HIPCHK(hipMemsetAsync(nbk, 0xFF, pool_nb * sizeof(PBucket), e->stream));  // PK_EMPTY keys (regions grow into it)
        HIPCHK(hipMemsetAsync(ndt, 0, total * sizeof(PData), e->stream));
        HIPCHK(hipMemsetAsync(nbm, 0, nword * 8, e->stream));
    }
    if (!hdr.empty()) HIPCHK(hipMemcpyAsync(nh, hdr.data(), hdr.size() * sizeof(PMap), hipMemcpyHostToDevice, e->stream));
    if (!tmid.empty()) HIPCHK(hipMemcpyAsync(nt, tmid.data(), tmid.size() * 4, hipMemcpyHostToDevice, e->stream));
    auto copy = [&](const std::vector<uint64_t>& tri, const void* src, void* dst) -> int {
        if (tri.empty()) return SG_OK;
        HIPCHK(hipMemcpyAsync(dtri, tri.data(), tri.size() * 8, hipMemcpyHostToDevice, e->stream));
        HIPCHK(launch_region_copy(reinterpret_cast<const uint64_t*>(src), reinterpret_cast<uint64_t*>(dst), dtri,
                                  (uint32_t)(tri.size() / 3), e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));  // dtri is reused by the next pool
        return SG_OK;
    };
    if (int rc = copy(tri_b, e->d_pbkt, nbk)) { release(); return rc; }
    if (int rc = copy(tri_d, e->d_pdat, ndt)) { release(); return rc; }
    if (int rc = copy(tri_w, e->d_pbm, nbm)) { release(); return rc; }
    HIPCHK(hipStreamSynchronize(e->stream));
    dfree(dtri);
    dfree(e->d_pbkt); dfree(e->d_pdat); dfree(e->d_pbm); dfree(e->d_ppre); dfree(e->d_pmap); dfree(e->d_tmid);
    dfree(e->d_pbkt2); dfree(e->d_pdat2); dfree(e->d_pcwork);
    e->d_pbkt2 = nbk2;
    e->d_pdat2 = ndt2;
    e->d_pcwork = nwork;
    e->pool2_nb = nbkt ? pool_nb : 0;
    e->d_pbkt = nbk;
    e->d_pdat = ndt;
    e->d_pbm = nbm;
    e->d_ppre = npr;
    e->d_pmap = nh;
    e->d_tmid = nt;
    e->n_pslot = total;
    e->pool_nb = pool_nb;
    e->pbm_words = nbkt ? nword : 0;
    {
        const unsigned long long next[2] = {nbkt, nbkt};  // PC_NEXT, PC_FLOOR
        HIPCHK(hipMemcpy(e->d_pool_next, next, 16, hipMemcpyHostToDevice));
        e->h_pool_next[PC_NEXT] = e->h_pool_next[PC_FLOOR] = nbkt;
    }
    e->pmap_key = keys;
    e->pmap_index.clear();
    for (uint32_t i = 0; i < (uint32_t)keys.size(); ++i)
        if (!(keys[i] & TMAP_KEY)) e->pmap_index[(uint32_t)keys[i]] = i;
    e->tm_base = tb;
    e->rmap_cap = rcap;
    e->tmaps = tmaps;
    if (keys.size() > e->pmoves_cap) {  // (the stream is drained: rebuild_pmaps synchronised it above)
        dfree(e->d_pmoves);
        e->pmoves_cap = keys.size();
        HIPCHK(hipMalloc(&e->d_pmoves, (e->pmoves_cap + 1) * sizeof(uint4)));
    }
    return SG_OK;
}

// The second pool of the compactions and their scratch exist whenever the pool does: laid out with the maps
// (rebuild_pmaps), so a compaction never allocates
static int ensure_pool2(sg_engine* e) {
    if (!e->pool_nb || (e->pool2_nb == e->pool_nb && e->d_pcwork)) return SG_OK;
    return fail(SG_ESTATE, "the hot-parameter map pool has no compaction copy");
}

// The pool's compaction between batches (drained): on the device, every map's region back to back into the
// other pool (kept allocated: a host relayout of ~2M maps took a second), then the pools swap.  Without the memory
// for a second pool, the host relayout (rebuild_pmaps).
static int compact_pmaps(sg_engine* e) {
    const uint32_t nm = (uint32_t)e->pmap_key.size();
    if (!nm) return SG_OK;
    if (int rc = ensure_pool2(e)) return rc;
    hipStream_t st = e->stream;
    HIPCHK(hipMemsetAsync(e->d_pbkt2, 0xFF, e->pool_nb * sizeof(PBucket), st));  // PK_EMPTY: regions grow into it
    HIPCHK(launch_pm_compact(e->d_pmap, nm, e->d_pbkt, e->d_pdat, e->d_pbkt2, e->d_pdat2, e->d_pcwork,
                             e->d_pcwork + e->pmoves_cap, e->d_pcwork + 2 * e->pmoves_cap, e->d_pool_next, st));
    HIPCHK(hipMemcpyAsync(e->h_pool_next, e->d_pool_next, PC_WORDS * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::swap(e->d_pbkt, e->d_pbkt2);
    std::swap(e->d_pdat, e->d_pdat2);
    return SG_OK;
}

int sg_load_param_rules(sg_engine* e, const sg_param_rule* rules, uint32_t n, uint32_t* n_loaded) {
    if (!e || (n && !rules)) return fail(SG_EINVAL, "null argument");
    if (int rc = drain(e)) return rc;  // no batch in flight while the rule tables change
    std::vector<ParamR> all;
    std::vector<std::string> keys;
    // Hot items (local and cluster rules alike) are interned through the dictionary and pinned: the list's pins
    // replace the last list's once the load has succeeded.  A load that fails before anything changed gives its
    // pins back; one that fails later keeps both lists' pins (a pinned entry too many is never a wrong key).
    struct Pins {
        sg_engine* e;
        std::vector<uint64_t> now;
        int end = 0;  // 0: give back, 1: keep beside the old ones, 2: replace the old ones
        ~Pins() {
            if (end == 0) for (uint64_t k : now) e->pkeys.unpin(k);
            else if (end == 1) e->par_pins.insert(e->par_pins.end(), now.begin(), now.end());
            else { for (uint64_t k : e->par_pins) e->pkeys.unpin(k); e->par_pins = std::move(now); }
        }
    } pins{e, {}};
    auto item_key = [&](const char* v, const char* t) {
        bool entry = false;
        const uint64_t k = e->pkeys.intern(v, t, true, &entry);
        if (entry) pins.now.push_back(k);
        return k;
    };
    if (!param_records(rules, n, item_key, all, keys)) return fail(SG_EINVAL, "param rule items pointer is null");
    // a negative paramIdx is rewritten in the loaded rule objects (ParamFlowSlot.applyRealParamIdx), so the
    // property's equality check never matches the list that created them: such a list always reloads
    bool neg = false;
    for (uint32_t i = 0; i < n; ++i) neg |= rules[i].has_param_idx && rules[i].param_idx < 0;
    if (e->par_loaded && keys == e->last_par && !neg) {
        if (n_loaded) *n_loaded = (uint32_t)e->params.size();
        return SG_OK;
    }
    RuleList<ParamR> L;
    int rrc = SG_OK;
    if (!build_param_list(all, std::move(keys), rule_resource(e, rrc), L)) return rrc;
    std::vector<ParamR>& ps = L.recs;
    std::vector<std::vector<int>>& per = L.per;
    // ParameterMetric lifetime: resources that had rules and now have none lose their metric
    // (ParamFlowRuleManager.java:150-159); all metrics are cleared for an empty list.  Work on copies: the maps
    // are rebuilt (and may fail with SG_ECAPACITY) before anything of the engine changes.
    std::vector<bool> now_has(e->names.size(), false);
    for (size_t r = 0; r < per.size(); ++r) now_has[r] = !per[r].empty();
    auto psid_of = e->psid_of;
    auto rcap = e->rmap_cap;
    auto tmaps = e->tmaps;
    uint32_t next_psid = e->next_psid;
    std::vector<uint64_t> clear_flags;
    for (size_t r = 0; r < e->res_par.size(); ++r) {
        bool had = !e->res_par[r].empty();
        if ((had && !now_has[r]) || n == 0) {
            const std::string pre = e->names[r] + std::string("\0", 1);
            for (auto it = psid_of.begin(); it != psid_of.end();) {
                if (it->first.compare(0, pre.size(), pre) == 0) { rcap.erase(it->second); it = psid_of.erase(it); }
                else ++it;
            }
            tmaps.erase(tmaps.lower_bound((uint64_t)r << 8), tmaps.lower_bound((uint64_t)(r + 1) << 8));
            clear_flags.push_back(((uint64_t)(NI_PM | (((1u << SG_MAX_ARGS) - 1) << NI_TM_SHIFT)) << 32) | r);
        }
    }
    for (auto& q : ps) {
        std::string k = q.res + std::string("\0", 1) + q.eqkey;
        if (!psid_of.count(k)) {
            psid_of[k] = next_psid;
            rcap[next_psid++] = rule_map_cap(q.r.duration_in_sec);
        }
    }
    // thread-count maps: ParameterMetric.initialize makes one per paramIdx a rule of the resource resolves to
    // (a negative index resolves per call: any index); a map stays while the resource keeps a metric
    for (size_t r = 0; r < per.size(); ++r)
        for (int i : per[r]) {
            const int32_t idx = ps[i].r.param_idx;
            for (int32_t k = 0; k < SG_MAX_ARGS; ++k)
                if (idx < 0 || idx == k) tmaps.insert(((uint64_t)r << 8) | (uint64_t)k);
        }
    // the checks first: with SG_ENOTSUP / SG_ECAPACITY neither the cluster rules nor the maps change
    if (int rc = check_rule_limits(e, RuleLists{ps, per, e->flows, e->res_flow, e->degs, e->res_deg})) return rc;
    if (e->emb_on)
        if (int rc = check_emb_shape(e->flows, e->res_flow, per)) return rc;
    uint64_t need = (rcap.size() + tmaps.size()) * (uint64_t)PM_MIN_NB * PM_BKT;  // (new maps' first regions)
    if (need > (1ull << e->cfg.param_table_log2))
        return fail(SG_ECAPACITY, "hot-parameter maps need " + std::to_string(need) + " slots, param_table_log2 = " +
                                      std::to_string(e->cfg.param_table_log2) + " allows " +
                                      std::to_string(1ull << e->cfg.param_table_log2));
    if (int rc = rebuild_cluster_param(e, rules, all, n)) return rc;
    pins.end = 1;  // the token server reads the new hot items from here on
    if (int rc = rebuild_pmaps(e, rcap, tmaps)) return rc;
    e->psid_of = std::move(psid_of);
    e->next_psid = next_psid;
    auto op = std::move(e->params);
    auto opr = std::move(e->res_par);
    e->params = std::move(ps);
    e->res_par = std::move(per);
    resize_lists(e, e->res_par);
    int rc = upload_rules(e, false, false, true);
    if (rc) { e->params = std::move(op); e->res_par = std::move(opr); return rc; }
    if (!clear_flags.empty()) {
        uint64_t* d = nullptr;
        HIPCHK(hipMalloc(&d, clear_flags.size() * 8));
        HIPCHK(hipMemcpy(d, clear_flags.data(), clear_flags.size() * 8, hipMemcpyHostToDevice));
        HIPCHK(launch_set_flags(e->d_info, d, (uint32_t)clear_flags.size(), e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        (void)hipFree(d);
    }
    e->last_par = std::move(L.keys);
    e->par_loaded = true;
    pins.end = 2;
    if (!e->params.empty() && !e->d_keyring) {  // thread counts can exist from now on: remember ENTRY keys
        const uint64_t nk = 1ull << e->cfg.status_ring_log2;
        HIPCHK(hipMalloc(&e->d_keyring, nk * sizeof(uint64_t)));
        HIPCHK(hipMemset(e->d_keyring, 0xFF, nk * sizeof(uint64_t)));  // NO_KEY
    }
    if (n_loaded) *n_loaded = (uint32_t)e->params.size();
    return SG_OK;
}

// pvalue.hip's scratch for up to cap accesses of up to m listed segments (the decide stage's: a batch in flight may
// still use the old arrays, so the stream drains first)
static void free_pvbuf(PvBuf& B) {
    dfree(B.key); dfree(B.pos); dfree(B.dt); dfree(B.acq); dfree(B.tc); dfree(B.seg); dfree(B.gid); dfree(B.idx);
    dfree(B.gid2); dfree(B.idx2); dfree(B.prev); dfree(B.w); dfree(B.sprev); dfree(B.sw); dfree(B.fslot); dfree(B.hit);
    dfree(B.keep); dfree(B.flast); dfree(B.ftok); dfree(B.htab); dfree(B.chunk); dfree(B.ccnt); dfree(B.cof);
    dfree(B.gdt); dfree(B.gaw); dfree(B.gpos); dfree(B.range);
    B = PvBuf{};
}
static void free_pv(sg_engine* e) {
    free_pvbuf(e->pvb);
    free_pvbuf(e->pvbt);
    dfree(e->d_pvhist); dfree(e->d_pvpart); dfree(e->d_pvthist); dfree(e->d_pvtpart);
    e->pv_cap = 0;
    e->pvch_cap = 0;
}
// every stream that may still read the scratch: the decide stream and the pre pass's
static hipError_t drain_decide(sg_engine* e) {
    hipError_t r = hipStreamSynchronize(e->stream);
    for (auto s : e->bin_stream)
        if (r == hipSuccess && s) r = hipStreamSynchronize(s);
    return r;
}
// (grown with headroom: a reallocation drains the stream, so it must stay rare)
static int ensure_pv(sg_engine* e, uint64_t cap, uint64_t m) {
    if (m > e->pvseg_cap) {
        HIPCHK(drain_decide(e));
        dfree(e->d_pvseg);
        dfree(e->d_pvtseg);
        e->pvseg_cap = std::max<uint64_t>(m + m / 2, 1024);
        HIPCHK(hipMalloc(&e->d_pvseg, e->pvseg_cap * sizeof(PvSeg)));
        HIPCHK(hipMalloc(&e->d_pvtseg, e->pvseg_cap * sizeof(PvSeg)));
        dfree(e->d_pvrest);
        HIPCHK(hipMalloc(&e->d_pvrest, 2 * (e->pvseg_cap + 1) * 4));
    }
    if (!e->d_pvtot) HIPCHK(hipMalloc(&e->d_pvtot, 64));
    if (cap > e->pv_cap) {
        HIPCHK(drain_decide(e));
        free_pv(e);
        const uint64_t c = std::max<uint64_t>(cap + cap / 4, 1u << 16);
        for (PvBuf* Bp : {&e->pvb, &e->pvbt}) {
            PvBuf& B = *Bp;
            HIPCHK(hipMalloc(&B.key, c * 8)); HIPCHK(hipMalloc(&B.pos, c * 4)); HIPCHK(hipMalloc(&B.dt, c * 4));
            HIPCHK(hipMalloc(&B.acq, c * 4)); HIPCHK(hipMalloc(&B.tc, c * 4)); HIPCHK(hipMalloc(&B.seg, c * 4));
            HIPCHK(hipMalloc(&B.gid, c * 4)); HIPCHK(hipMalloc(&B.idx, c * 4)); HIPCHK(hipMalloc(&B.gid2, c * 4));
            HIPCHK(hipMalloc(&B.idx2, c * 4)); HIPCHK(hipMalloc(&B.prev, c * 4)); HIPCHK(hipMalloc(&B.w, c * 4));
            HIPCHK(hipMalloc(&B.sprev, c * 4)); HIPCHK(hipMalloc(&B.sw, c * 4)); HIPCHK(hipMalloc(&B.fslot, c * 4));
            HIPCHK(hipMalloc(&B.hit, c)); HIPCHK(hipMalloc(&B.keep, c)); HIPCHK(hipMalloc(&B.flast, c * 8));
            HIPCHK(hipMalloc(&B.ftok, c * 4)); HIPCHK(hipMalloc(&B.htab, c * 16));
            HIPCHK(hipMalloc(&B.gdt, c * 4)); HIPCHK(hipMalloc(&B.gaw, c * 4)); HIPCHK(hipMalloc(&B.gpos, c * 4));
            HIPCHK(hipMalloc(&B.range, c * 16));
        }
        const uint64_t nblocks = (c + radix_tile() - 1) / radix_tile();
        HIPCHK(hipMalloc(&e->d_pvhist, nblocks * 256 * 4));
        HIPCHK(hipMalloc(&e->d_pvpart, nblocks * 256 * 4 + 4096));
        HIPCHK(hipMalloc(&e->d_pvthist, nblocks * 256 * 4));
        HIPCHK(hipMalloc(&e->d_pvtpart, nblocks * 256 * 4 + 4096));
        e->pv_cap = c;
    }
    // chunks: cap / PV_CH (4096) + one per segment (launch_pv's grid: pv_cap / 4096 + m + 1)
    const uint64_t nch = e->pv_cap / 4096 + m + 16;
    if (nch > e->pvch_cap) {
        HIPCHK(drain_decide(e));
        e->pvch_cap = nch + nch / 2;
        for (PvBuf* Bp : {&e->pvb, &e->pvbt}) {
            PvBuf& B = *Bp;
            dfree(B.chunk); dfree(B.ccnt); dfree(B.cof);
            HIPCHK(hipMalloc(&B.chunk, e->pvch_cap * 8)); HIPCHK(hipMalloc(&B.ccnt, e->pvch_cap * 4));
            HIPCHK(hipMalloc(&B.cof, e->pvch_cap * 4 + 4));
        }
    }
    return SG_OK;
}

// The XF_MIX segment lists of slot B for up to mb segments (narrow, then wide at mix_cap)
static int ensure_mix(sg_engine::BatchSlot& B, uint64_t mb) {
    if (mb > B.mix_cap) HIPCHK(grow(B.d_mix, B.mix_cap, mb, 1u << 12, 2 * 4));
    return SG_OK;
}

// Lists of the aux.hip post-pass for a batch of n events in slot B, and the engine's partial pool.
#define AUXPOOL_CAP (1u << 20)
static int ensure_aux(sg_engine* e, sg_engine::BatchSlot& B, uint64_t n) {
    const uint64_t npiece = n / AUX_PIECE + n / 257 + 64;  // pieces: every long segment's, <= n/P + n/(AUX_SHORT + 1)
    if (n > B.aux_cap_n) {
        dfree(B.d_ashort); dfree(B.d_apiece); dfree(B.d_amulti); dfree(B.d_along);
        const uint64_t c = std::max<uint64_t>(n, 1u << 16);
        HIPCHK(hipMalloc(&B.d_ashort, c * 4));
        HIPCHK(hipMalloc(&B.d_along, (c / 257 + 64) * 8));
        HIPCHK(hipMalloc(&B.d_apiece, (c / AUX_PIECE + c / 257 + 64) * 8));
        HIPCHK(hipMalloc(&B.d_amulti, (c / AUX_PIECE + 64) * 8));
        B.aux_cap_n = c;
    }
    if (!e->d_auxpool) {
        HIPCHK(hipMalloc(&e->d_auxpool, (uint64_t)AUXPOOL_CAP * sizeof(AuxAcc)));
        e->auxpool_cap = AUXPOOL_CAP;
    }
    if (npiece > e->auxmeta_cap) {
        HIPCHK(hipStreamSynchronize(e->stream));  // no decide stage may use the old buffer
        HIPCHK(grow(e->d_auxmeta, e->auxmeta_cap, npiece, B.aux_cap_n / AUX_PIECE + B.aux_cap_n / 257 + 64));
    }
    return SG_OK;
}

static bool is_device_ptr(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

// sg_submit_ex: the Context and args tables in HBM, staged in slot B on stream st when the caller's are host memory
static int stage_ext_args(sg_engine::BatchSlot& B, const sg_event_ext* ext, uint64_t n, const sg_arg* args,
                          uint64_t n_args, hipStream_t st, const sg_event_ext** dev_ext, const sg_arg** dev_args) {
    *dev_ext = ext;
    *dev_args = n_args ? args : nullptr;
    if (ext && !is_device_ptr(ext)) {
        if (n > B.ext_cap) HIPCHK(grow(B.d_ext, B.ext_cap, n, 1u << 16));
        HIPCHK(hipMemcpyAsync(B.d_ext, ext, n * sizeof(sg_event_ext), hipMemcpyHostToDevice, st));
        *dev_ext = B.d_ext;
    }
    if (n_args && !is_device_ptr(args)) {
        if (n_args > B.args_cap) HIPCHK(grow(B.d_args, B.args_cap, n_args, 1u << 16));
        HIPCHK(hipMemcpyAsync(B.d_args, args, n_args * sizeof(sg_arg), hipMemcpyHostToDevice, st));
        *dev_args = B.d_args;
    }
    return SG_OK;
}

// The DevCfg of a batch and what its DevState holds whichever path decides it from slot B; gbase, epoch, skip_ok and
// skip_min are the caller's to set
static void fill_state(const sg_engine* e, const sg_engine::BatchSlot& B, uint64_t ring_mask, const sg_event_ext* dev_ext,
                       const sg_arg* dev_args, DevCfg& dc, DevState& S) {
    std::memset(&dc, 0, sizeof(dc));
    dc.max_rt = e->cfg.statistic_max_rt;
    dc.occupy_timeout = e->cfg.occupy_timeout_ms;
    dc.max_chain = e->cfg.max_slot_chain_size;
    dc.switch_on = e->cfg.switch_on;
    dc.ring_mask = ring_mask;
    dc.snap_hi = e->snap_hi;
    dc.dbg_flags = e->dbg_flags;
    dc.heads = e->has_head ? 1u : 0u;
    std::memset(&S, 0, sizeof(S));
    S.sec = e->d_sec;
    S.minb = e->d_minb;
    S.info = e->d_info;
    S.prog = e->d_prog;
    S.rules = e->d_rules;
    S.rstate = e->d_rstate;
    S.hot = e->d_hot;
    S.pmap = e->d_pmap;
    S.pbkt = e->d_pbkt;
    S.pdat = e->d_pdat;
    S.pbm = e->d_pbm;
    S.ppre = e->d_ppre;
    S.tmid = e->d_tmid;
    S.ring = e->d_ring;
    S.sink = e->d_sink;
    S.borrow = e->d_borrow;
    S.prio = e->d_prio;
    S.key_ring = e->d_keyring;
    S.link = B.d_link;
    S.bst = B.d_bst;
    S.pend = B.d_pend;
    S.spans = B.d_spans;
    S.nspan = B.d_bsmall + BS_NSPAN;
    S.span_cap = e->span_cap;
    S.ext = dev_ext;
    S.args = dev_args;
    S.aux_tab = e->d_auxtab;
    S.aux_count = e->d_auxcnt;
    S.aux_cap = e->cfg.aux_node_capacity;
    S.aux_mask = e->aux_mask;
    S.max_ctx = SG_MAX_CONTEXTS;
    S.auth = dev_auth(e);
    S.auth_ids = dev_auth_ids(e);
}

static int decide_stage(sg_engine* e, int k);

// The group stage (records, sort, segments, bins) of a batch, enqueued on gstream into slot k; it ends with the copy
// of the batch's head into the slot's pinned buffer and the group-end event.  Its first kernel (k_grp_first /
// k_rs_first) runs long enough for the host to enqueue a whole decide stage behind it: the decide stage of slot
// `prev` (-1: none), whose head the caller has read, is enqueued right after that kernel, so gstream never waits
// for the host to get through those launches.  What the decide stage of this batch needs is left in B.g.
static int group_stage(sg_engine* e, int k, const sg_event* ev, const sg_event_ext* ext, uint64_t n, const sg_arg* args,
                       uint64_t n_args, uint32_t* out, int* prev) {
    auto& B = e->slot[k];
    uint32_t* const sw = B.d_bsmall;  // the batch's small words (BS_*)
    B.ev = e->evset[e->seq % sg_engine::N_SETS];
    hipStream_t gs = e->gstream;
    // the slot's last batch is decided and its decisions are out before anything of the slot is overwritten
    if (B.last_post) HIPCHK(hipStreamWaitEvent(gs, B.last_post, 0));
    if (B.lent) {  // ... and the embedded token call that used the slot's arrays as scratch is through
        HIPCHK(hipStreamWaitEvent(gs, B.lent, 0));
        B.lent = nullptr;
    }
    const sg_event* dev_ev = ev;
    bool host_in = !is_device_ptr(ev);
    bool host_out = !is_device_ptr(out);
    if (host_in) {
        HIPCHK(hipMemcpyAsync(B.d_ev, ev, n * sizeof(sg_event), hipMemcpyHostToDevice, gs));
        dev_ev = B.d_ev;
    }
    uint32_t* dev_out = host_out ? B.d_out : out;
    const sg_event_ext* dev_ext;
    const sg_arg* dev_args;
    if (int src = stage_ext_args(B, ext, n, args, n_args, gs, &dev_ext, &dev_args)) return src;
    const uint64_t ring_mask = (1ull << e->cfg.status_ring_log2) - 1;
    // Overlapping this group stage with the previous batch's decide stage wins once the decide kernels
    // no longer stream frozen stretches through single CUs (C4 on MI355X: 6.45 -> 5.45 ms per batch);
    // SG_PIPELINE=0 runs the stages back to back.
    if (!e->pipeline && e->last >= 0 && e->slot[e->last].last_post)
        HIPCHK(hipStreamWaitEvent(gs, e->slot[e->last].last_post, 0));
    HIPCHK(hipEventRecord(B.ev[0], gs));
    // ---- 1. group: records + stable LSD radix sort on res_id (8-bit digits over the bits of max_resources-1)
    uint32_t R = e->cfg.max_resources;
    int bits = 1;
    while (bits < 32 && (1ull << bits) < R) ++bits;
    // 8-bit digits: measured faster than two 10-bit passes for 1M resources on MI355X (group stage
    // 2.99 vs 3.11 ms standalone; 1024 digit runs per 4096-item tile average 4 items, too short to
    // write coalesced).
    const int db = 8;
    int passes = (bits + db - 1) / db;
    uint32_t nblocks = (uint32_t)((n + radix_tile() - 1) / radix_tile());
    int64_t* d_t0 = reinterpret_cast<int64_t*>(sw + BS_T0);
    uint32_t *kin = B.d_k1, *vin = B.d_v1, *kout = B.d_k0, *vout = B.d_v0;
    if (++e->epoch == 0) e->epoch = 1;
    const uint32_t ublk = (e->dbg_flags & UBLK_OFF) ? 0u : 1u;
    // every event through the radix passes: SG_DEBUG_FLAGS & 8192 (A/B of the group stage), or a batch of 2^30 events
    // or more (the hot / cold stage's words hold a position in 30 bits)
    B.radix = e->radix_group || n >= (1ull << 30) || n < e->radix_below;
    // one launch clears the batch's small words and, for the hot / cold stage, bst[] and the side-table marks: the
    // slot's are free once its last batch is decided (above), d_need since the previous group stage on this stream
    HIPCHK(launch_grp_clear(B.d_bsmall, BS_WORDS, B.d_bst, B.radix ? 0u : (uint32_t)((n + 1023) / 1024), e->d_need,
                            B.radix ? 0u : (uint32_t)e->need_words, gs));
    // bins + bin-ordered dispatch list (per-block counts -> scan -> placement), sized by an upper bound of
    // the segment count so that the group stage needs one host round trip
    const bool force_lane = !e->cfg.switch_on || (e->dbg_flags & 2);
    const uint32_t mb = (uint32_t)std::min<uint64_t>(n, R);
    const uint32_t nblk = (mb + 255) / 256;
    // Bin thresholds by batch size: a full batch (C4: 2^25 events) keeps the decide stage busy with event
    // throughput, and wider owners for shorter segments cost more than they save (measured); in a batch of
    // fewer than SHARD_BATCH (6.3M) events -- one rank's shard of a multi-GPU step -- the longest owner chains bound it
    // instead, so segments get wider owners sooner (tools/shard_rehearsal.sh: 8-way shards of C4, mean
    // rank step 1.70 -> 1.33 ms, slowest 1.85 -> 1.73 ms).
    uint32_t lane_max = e->lane_max, j1_max = e->j1_max, j4_max = e->j4_max;
    // (below SHARD_BATCH events: an 8-way shard of a 2^25-event global batch is ~2^22; a 4-way shard's 2^23 runs
    // faster with the full-batch bins: 4-way rehearsal 2.24 -> 1.79 ms per global batch)
    if (!e->bins_pinned && n < SHARD_BATCH) {
        lane_max = std::min<uint32_t>(lane_max, 128);
        j1_max = std::min<uint32_t>(j1_max, 1024);
        j4_max = std::min<uint32_t>(j4_max, 4096);
    }
    // k_lite's longer limit is a full batch's: a shard-sized batch and pinned bins keep one limit for every lane bin,
    // and so does an engine with THREAD-grade / rate-limiter head programs (C3: the main stream, which the lane bins
    // are on, is close behind its longest chain; 6.01 -> 6.36 ms a batch with the longer limit)
    const uint32_t lite_max = e->lite_pinned ? e->lite_max
                              : (e->bins_pinned || e->has_head || n < SHARD_BATCH) ? lane_max
                                                                                   : std::max(lane_max, e->lite_max);
    // A cooperative owner's lanes sum a stretch's acquire units (<= 65,535 an event) in 32 bits before the 64-bit
    // reduction at the stretch's end, so one owner of 64 * NW lanes takes at most 65,000 events a lane: a pinned limit
    // above that hands the segment to the next wider owner.  (The 512-lane owner ends at J8_MAX = 2^23 events; the
    // 1,024-lane one reaches its 66.5M only in a batch twice the default max_batch_events.)
    j1_max = std::min<uint32_t>(j1_max, 64u * 65000u);
    j4_max = std::min<uint32_t>(j4_max, 256u * 65000u);
    // a shard-sized batch (see the bins above) is bound by its longest owners, whose frozen stretches are
    // cheaper skipped than streamed from 8192 positions on (8-way C4 shards: slowest rank 1.79 -> 1.69 ms)
    const uint32_t skip_min = (!e->skip_pinned && n < SHARD_BATCH) ? std::min<uint32_t>(e->skip_min, 8192) : e->skip_min;
    // need_hot / need_blk (the hot / cold stage; null: the side tables everywhere): the segments whose owner can skip
    // frozen stretches mark their hot id / their cold blocks, and the record kernels, which run after the bins there,
    // build forward links and bst[] for those only.  bmax: per hot id the most events one 500 ms bucket can hold
    // (launch_hot_bmax): an id is marked only where that exceeds its owner's skip threshold.
    auto bins = [&](uint32_t* need_hot, uint32_t* need_blk, const uint32_t* bmax) -> int {
        if (ext) {  // the aux.hip post-pass lists of this slot
            if (int arc = ensure_aux(e, B, n)) return arc;
        }
        if (e->has_mix) {  // the XF_MIX lists of this slot
            if (int mrc = ensure_mix(B, mb)) return mrc;
        }
        HIPCHK(launch_seg_bin(B.d_segs, sw + BS_NSEG, mb, n, e->d_prog, e->d_prio, lane_max, lite_max, j1_max, j4_max,
                              force_lane ? 1 : 0, B.d_blkcnt, e->pq_on ? 1u : 0u, e->pq_wide, ext ? sw + BS_AUX : nullptr,
                              B.d_ashort, B.d_along, B.d_amulti, sw + BS_MIX_N, e->has_mix ? B.d_mix : nullptr,
                              (uint32_t)B.mix_cap, sw + BS_MIX_WIDE, (e->pv_on || e->pvt_on) ? 0u : e->pq_wide,
                              (e->dbg_flags & HEAD_OFF) ? 0u : e->head_min, e->d_hot_tab, e->nhot, sw + BS_HOT_SEGS,
                              need_hot, need_blk, bmax, skip_min, sw + BS_HOT_MARKED, sw + BS_UBLK,
                              e->emb_n ? sw + BS_EMB : nullptr, R, gs));
        HIPCHK(launch_scan(B.d_blkcnt, B.d_blkcnt, (uint64_t)nblk * N_BINS, B.d_part, nullptr, gs));
        HIPCHK(launch_seg_order(B.d_segs, sw + BS_NSEG, mb, B.d_blkcnt, B.d_order, sw + BS_BIN_OFF, gs));
        return SG_OK;
    };
    // the previous batch's decide stage, enqueued while this batch's first kernel runs
    auto decide_prev = [&]() -> int {
        if (*prev < 0) return SG_OK;
        const int pk = *prev;
        *prev = -1;  // (enqueued, or failed for good: the caller does not try again)
        return decide_stage(e, pk);
    };
    if (B.radix) {
        HIPCHK(launch_rs_first(dev_ev, n, R, e->gbase, e->d_ring, ring_mask, e->cfg.statistic_max_rt, B.d_rec_o,
                               B.d_k1, B.d_v1, B.d_hist, nblocks, sw + BS_FLAGS, d_t0, e->d_prio, e->d_keyring,
                               e->d_comp, dev_ext, dev_args, n_args, SG_MAX_CONTEXTS, dev_auth(e), dev_auth_ids(e), ublk, gs));
        if (int drc = decide_prev()) return drc;
        for (int p = 0; p < passes; ++p) {
            if (p > 0) HIPCHK(launch_radix_hist(kin, n, p * db, B.d_hist, nblocks, gs));
            HIPCHK(launch_scan(B.d_hist, B.d_hist, (uint64_t)nblocks << db, B.d_part, nullptr, gs));
            HIPCHK(launch_radix_scatter(kin, vin, n, p * db, B.d_hist, nblocks, kout, vout,
                                        p == passes - 1 ? B.d_posof : nullptr, gs));
            std::swap(kin, kout);
            std::swap(vin, vout);
        }
        HIPCHK(launch_seg(kin, n, B.d_flag, B.d_pos, B.d_segs, gs, B.d_part, sw + BS_NSEG));
        HIPCHK(launch_gather(B.d_rec_o, vin, kin, n, B.d_posof, B.d_recs, B.d_prev, sw + BS_NPREV, B.d_link,
                             B.d_bst, e->epoch, sw + BS_FLAGS, gs));
        if (int brc = bins(nullptr, nullptr, nullptr)) return brc;
    } else {
        // ---- hot / cold group stage (kernels.hip k_grp_*); its own words are BS_GRP .. BS_COLD_SEGS
        const uint32_t nhot = e->nhot;
        B.nhot = nhot;
        uint32_t* words = B.d_flag;    // per event: W_HOT | W_ENT? | hot id << 12 | rank in its tile's run of the id;
                                        // cold: W_ENT? | sorted position (the last cold pass)
        uint32_t* hot_off = B.d_pos;   // [tile][hot id] counts (tile-major, rows of nhot words), scanned in place: the
                                        // runs' sorted positions P (k_grp_records, k_post_w, k_hot_bmax read rows of it)
        uint32_t* ccnt = B.d_ccnt;      // per tile: cold events (compacted at the tile's start in k1 / v1)
        HIPCHK(launch_grp_first(dev_ev, n, R, e->gbase, ring_mask, sw + BS_FLAGS, d_t0, e->d_prio, e->d_keyring,
                                e->d_comp, dev_ext, dev_args, n_args, SG_MAX_CONTEXTS, dev_auth(e), dev_auth_ids(e),
                                e->d_hot_tab, nhot, nblocks,
                                words, hot_off, B.d_k1, B.d_v1, ccnt, B.d_hist, ublk, gs));
        if (int drc = decide_prev()) return drc;
        HIPCHK(launch_hot_scan(hot_off, nblocks, nhot, e->d_hot_part, e->d_hot_hb, sw + BS_GRP, gs));
        HIPCHK(launch_cold_n(n, sw + BS_GRP, sw + BS_COLD_N, gs));
        if (nblocks == 1) {  // one tile: the cold pairs sorted by one workgroup (k_cold_small), into k0 / v0
            HIPCHK(launch_cold_small(kin, vin, ccnt, sw + BS_GRP, kout, vout, words, gs));
            std::swap(kin, kout);
            std::swap(vin, vout);
        }
        for (int p = 0; p < passes && nblocks > 1; ++p) {  // the cold (key, index) pairs
            if (p > 0) HIPCHK(launch_radix_hist_n(kin, n, sw + BS_COLD_N, p * db, B.d_hist, nblocks, gs));
            HIPCHK(launch_scan(B.d_hist, B.d_hist, (uint64_t)nblocks << db, B.d_part, nullptr, gs));
            const bool last = p == passes - 1;
            HIPCHK(launch_radix_scatter_x(kin, vin, n, p ? sw + BS_COLD_N : nullptr, p ? nullptr : ccnt,
                                          last ? sw + BS_GRP : nullptr, p * db, B.d_hist, nblocks, kout, vout,
                                          last ? words : nullptr, gs));
            std::swap(kin, kout);
            std::swap(vin, vout);
        }
        // segments: the hot ids' (in id order), then the cold keys' [hot_total, n)
        HIPCHK(launch_hot_segs(e->d_hot_hb, nhot, e->d_hot_list, B.d_segs, sw + BS_HOT_SEGS, gs));
        const uint64_t sc = nblocks + 64;
        HIPCHK(launch_seg_cold(kin, n, sw + BS_GRP, sw + BS_HOT_SEGS, ccnt + sc, ccnt + 2 * sc, B.d_segs, gs,
                               B.d_part, sw + BS_COLD_SEGS, sw + BS_NSEG));
        // the bins first: they read only the segments, the programs and the marks of k_grp_first, and say which
        // side tables the record kernels must build (SG_DEBUG_FLAGS & 32768: all of them, as the radix stage does)
        uint32_t *need_hot = nullptr, *need_blk = nullptr, *bmax = nullptr;
        if (!(e->dbg_flags & TABLES_ALL)) {
            need_hot = e->d_need;
            need_blk = e->d_need + hot_max();
            bmax = e->d_need + e->need_words - hot_max();
            HIPCHK(launch_hot_bmax(dev_ev, nblocks, hot_off, nhot, e->d_hot_hb, e->d_edges, bmax, gs));
        }
        if (int brc = bins(need_hot, need_blk, bmax)) return brc;
        HIPCHK(launch_grp_records(dev_ev, n, e->gbase, ring_mask, e->cfg.statistic_max_rt, words, hot_off, nhot, nblocks,
                                  e->d_hot_hb, B.d_recs, vin, B.d_prev, sw + BS_NPREV, B.d_bst,
                                  sw + BS_FLAGS, dev_ext, dev_args, SG_MAX_CONTEXTS, B.d_link, e->epoch, need_hot,
                                  need_blk, R, dev_auth(e), dev_auth_ids(e), ublk, gs));
        HIPCHK(launch_block_sums(B.d_recs, n, B.d_bst, B.d_link, e->epoch, sw + BS_FLAGS, kin, sw + BS_GRP,
                                 need_blk, gs));
    }
    // the next batch's hot ids: this batch's resources of >= n / 8192 events (about one per 4096-event tile, so
    // that a tile's run of one hot id is more than a random write), at least 64
    const uint32_t hot_min = (uint32_t)std::max<uint64_t>(64, n / 8192);
    if (!B.radix)
        HIPCHK(launch_hot_build(B.d_segs, sw + BS_NSEG, mb, hot_min, R, e->d_hot_tab, e->d_hot_list, e->nhot,
                                sw + BS_HOT_NEXT, gs));
    HIPCHK(hipMemcpyAsync(B.h_head, B.d_bsmall, BS_HEAD_WORDS * 4, hipMemcpyDeviceToHost, gs));
    HIPCHK(hipEventRecord(B.ev[1], gs));
    auto& G = B.g;
    G.n = n; G.n_args = n_args; G.gbase = e->gbase; G.ring_mask = ring_mask;
    G.dev_ev = dev_ev; G.dev_ext = dev_ext; G.dev_args = dev_args;
    G.out = out; G.dev_out = dev_out; G.vin = vin;
    // (lane_max: the length up to which every segment is a lane one, for the decide stage's aux_early)
    G.epoch = e->epoch; G.skip_min = skip_min; G.lane_max = std::min(lane_max, lite_max); G.mb = mb;
    G.ext = ext != nullptr; G.host_out = host_out; G.force_lane = force_lane;
    G.set = (int)(e->seq % sg_engine::N_SETS);
    e->grouped = k;
    return SG_OK;
}

// The grouped batch's verdict (handoff step 1): wait for its group stage, read its head and run the group stage's
// checks.  A batch that passes is accepted -- gbase, the slot and the event set move on -- and its decide stage is
// the caller's to enqueue; one that fails is dropped as if its submit had returned the error.  Either way no batch is
// left grouped.  drop: the caller gives the batch up; only the hot ids it left for the next group stage are taken.
static int accept_grouped(sg_engine* e, bool drop = false) {
    const int k = e->grouped;
    auto& B = e->slot[k];
    e->grouped = -1;
    HIPCHK(hipEventSynchronize(B.ev[1]));
    const uint32_t* head = B.h_head;
    if (!B.radix) e->nhot = std::min<uint32_t>(head[BS_HOT_NEXT], hot_max());
    if (drop) return SG_OK;
    B.hot_marked = head[BS_HOT_MARKED];
    B.ublk_coop = head[BS_UBLK];
    B.ublk_lane = head[BS_UBLK_LANE];
    B.emb_ub = e->emb_n ? head[BS_EMB] : 0u;
    B.emb_coop = e->emb_n ? head[BS_EMB_COOP] : 0u;
    B.emb_lane = e->emb_n ? head[BS_EMB_LANE] : 0u;
    if (int vrc = group_verdict(head[BS_FLAGS])) return vrc;
    // the decide stage's only allocation (the value-parallel passes' scratch) before the batch is counted: past
    // this point nothing but a device error can keep its decide stage from being enqueued
    if (e->has_mix && head[BS_MIX_NW] && (e->pv_on || e->pvt_on) && head[BS_MIX_WIDE]) {
        if (int prc = ensure_pv(e, head[BS_MIX_WIDE], head[BS_MIX_NW])) return prc;
    }
    e->inflight.push_back({B.g.set, B.hot_marked, B.ublk_coop, B.ublk_lane, B.emb_coop, B.emb_lane});
    ++e->seq;
    e->last = k;
    e->cur = k ^ 1;
    e->gbase += B.g.n;
    return SG_OK;
}

// A grouped batch handed to the decide stage at once (every call but an async submit starts with this: drain()).
static int handoff(sg_engine* e) {
    if (e->grouped < 0) return SG_OK;
    const int k = e->grouped;
    if (int rc = accept_grouped(e)) return rc;
    return decide_stage(e, k);
}

static int decide_enqueue(sg_engine* e, int k);
static int embedded_tokens(sg_engine* e, int k, uint32_t* nreq_out);

// The decide stage of the accepted batch in slot k.  The batch is counted already (accept_grouped), so a decide
// stage that could not be enqueued whole -- a device error -- leaves the engine inconsistent: it refuses every later
// batch, and the batch is not collected (its end events were never recorded).
static int decide_stage(sg_engine* e, int k) {
    const int rc = decide_enqueue(e, k);
    if (rc) {
        const std::string why = g_err;
        if (!e->inflight.empty()) e->inflight.pop_back();
        if (e->fatal.empty()) e->fatal = "the decide stage of an accepted batch could not be enqueued (" + why + ")";
        return fail(rc, why);
    }
    return rc;
}

// The decide stage proper (reference resolution, chain grants, decide kernels, post), enqueued on the decide streams
// behind the previous batch's.
static int decide_enqueue(sg_engine* e, int k) {
    auto& B = e->slot[k];
    uint32_t* const sw = B.d_bsmall;  // the batch's small words (BS_*)
    const auto& G = B.g;
    hipStream_t st = e->stream;
    const uint64_t n = G.n, n_args = G.n_args, ring_mask = G.ring_mask;
    const sg_event* dev_ev = G.dev_ev;
    const sg_event_ext* dev_ext = G.dev_ext;
    const sg_arg* dev_args = G.dev_args;
    uint32_t *out = G.out, *dev_out = G.dev_out, *vin = G.vin;
    const uint32_t skip_min = G.skip_min, lane_max = G.lane_max, mb = G.mb;
    const bool ext = G.ext, host_out = G.host_out, force_lane = G.force_lane;
    (void)n_args;
    const uint32_t* head = B.h_head;  // (the slot's next group stage, which refills it, is enqueued after this returns)
    const uint32_t m = head[BS_NSEG];
    const uint32_t nprev = head[BS_NPREV];
    int64_t t0 = 0;
    std::memcpy(&t0, head + BS_T0, 8);
    const uint32_t bflags = head[BS_FLAGS];
    const uint32_t* off = head + BS_BIN_OFF;
    uint32_t bin_n[N_BINS];
    for (int b = 0; b < N_BINS; ++b) bin_n[b] = off[b + 1] - off[b];
    // ---- 3. decide: cooperative bins on their own streams, lane bins on the main stream (state for every kernel)
    DevCfg dc;
    DevState S;
    fill_state(e, B, ring_mask, dev_ext, dev_args, dc, S);
    S.gbase = G.gbase;
    S.epoch = G.epoch;
    S.skip_ok = !(bflags & (BF_MULTI_LINK | BF_ZERO_CNT)) && !(e->dbg_flags & 4) ? 1u : 0u;
    S.skip_min = skip_min;  // (the bins marked the side tables by it)
    // ---- decide stage, in order after the previous batch's: references into earlier batches first
    HIPCHK(hipStreamWaitEvent(st, B.ev[1], 0));
    const uint32_t n_mix = e->has_mix ? head[BS_MIX_N] : 0u, n_mixw = e->has_mix ? head[BS_MIX_NW] : 0u;
    // SG_DEBUG_FLAGS & 8 (diagnostics): every decide kernel on the main stream, one after the other
    const bool serial_bins = (e->dbg_flags & 8) != 0;
    const bool pre_split = (n_mix || n_mixw) && !serial_bins;
    hipStream_t ps = pre_split ? e->bin_stream[1] : st;
    // the value-parallel pre pass's extraction and sort (launch_pv_a) read only this batch's records and the rules,
    // so with every chain granted (k_pv_prep then knows the grants' outcome) they start as soon as this batch is
    // grouped, on bin_stream[1] beside the previous batch's post pass (their own scratch, pvb; the post pass has pvbt)
    const uint32_t grant_all = (e->cfg.switch_on && e->cfg.max_slot_chain_size <= 0) ? 1u : 0u;
    if (n_mixw && (e->pv_on || e->pvt_on) && head[BS_MIX_WIDE]) {
        if (int prc = ensure_pv(e, head[BS_MIX_WIDE], n_mixw)) return prc;
        e->pv_last_m = n_mixw;
    }
    const bool pv_ran = n_mixw && e->pv_on && head[BS_MIX_WIDE];
    const bool pv_early = pv_ran && pre_split && grant_all && !e->has_multi;
    if (pv_early) {
        HIPCHK(hipStreamWaitEvent(ps, B.ev[1], 0));
        HIPCHK(launch_pv_a(B.d_recs, vin, B.d_segs, B.d_mix + B.mix_cap, n_mixw, S, dc, B.d_dec, e->d_pvseg, e->pvb,
                           head[BS_MIX_WIDE], e->d_pvtot, e->d_pvhist, e->d_pvpart, ps, radix_tile(), e->d_pvrest, grant_all));
    }
    HIPCHK(launch_resolve(B.d_prev, nprev, e->d_ring, B.d_recs, vin, dev_ext, st));
    // ---- chain cap (CtSph.lookProcessChain): grant chains in order of first ENTRY.  First on the decide stream: the
    // pre pass's eligibility reads the chain flags (it ran beside the grants and raced them)
    if (e->cfg.switch_on && (e->cfg.max_slot_chain_size <= 0 || e->n_chains < (uint32_t)e->cfg.max_slot_chain_size)) {
        const bool grant_all = e->cfg.max_slot_chain_size <= 0;
        HIPCHK(launch_chain(B.d_recs, vin, B.d_segs, m, e->d_info, grant_all ? 1 : 0, sw + BS_NCAND, B.d_cand,
                            dev_ev, e->d_prog, dev_ext, SG_MAX_CONTEXTS, st));
        if (!grant_all) {
            uint32_t ncand = 0;
            HIPCHK(hipMemcpyAsync(&ncand, sw + BS_NCAND, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (ncand) {
                std::vector<uint64_t> cand(ncand);
                HIPCHK(hipMemcpy(cand.data(), B.d_cand, ncand * 8ull, hipMemcpyDeviceToHost));
                std::sort(cand.begin(), cand.end());  // by batch index of the first ENTRY
                std::vector<uint64_t> upd;
                std::unordered_map<uint32_t, int> seen;  // RELATE components list every ENTRY
                for (uint32_t i = 0; i < ncand; ++i) {
                    uint32_t res = (uint32_t)cand[i];
                    if (!seen.emplace(res, 1).second) continue;
                    bool grant = e->n_chains < (uint32_t)e->cfg.max_slot_chain_size;
                    if (grant) e->n_chains++;
                    upd.push_back(((uint64_t)(grant ? NI_CHAIN : NI_REJECTED) << 32) | res | (1ull << 63));
                }
                ncand = (uint32_t)upd.size();
                HIPCHK(hipMemcpyAsync(B.d_cand, upd.data(), ncand * 8ull, hipMemcpyHostToDevice, st));
                HIPCHK(launch_set_flags(e->d_info, B.d_cand, ncand, st));
                HIPCHK(hipStreamSynchronize(st));
            }
        }
    }
    // Embedded token server: the batch's token requests, decided by one token call ahead of every owner (after the
    // chain grants, which the request test reads).  Only a batch that holds events of XF_EMB resources comes here
    if (B.emb_ub) {
        uint32_t nreq = 0;
        if (int erc = embedded_tokens(e, k, &nreq)) return erc;
        if (nreq) S.emb = e->d_emb_side;
    }
    // XF_MIX segments of the cooperative bins (and XF_PVPQ ones): their param checks first (the value-parallel pre
    // pass, else k_pq's), the owners then decide the flow / degrade chain on them.  The pre pass runs on
    // bin_stream[1] (whose J4 / J1 wait for it anyway); its extraction and sort touch no map region, so they start
    // after the chain grants, beside the maps' growth on the main stream; the rest waits for the growth.
    if (pre_split) {
        HIPCHK(hipEventRecord(e->fork0, st));
        HIPCHK(hipStreamWaitEvent(ps, e->fork0, 0));
    }
    if (pv_ran && !pv_early)
        HIPCHK(launch_pv_a(B.d_recs, vin, B.d_segs, B.d_mix + B.mix_cap, n_mixw, S, dc, B.d_dec, e->d_pvseg, e->pvb,
                           head[BS_MIX_WIDE], e->d_pvtot, e->d_pvhist, e->d_pvpart, ps, radix_tile(), e->d_pvrest, grant_all));
    // param map regions grown for this batch's segments before anything touches a map; the pool's use, for the
    // compaction check of a later submit
    if (e->pool_nb) {
        DevState Sg{};
        std::memset(&Sg, 0, sizeof(Sg));
        Sg.prog = e->d_prog; Sg.rules = e->d_rules; Sg.tmid = e->d_tmid; Sg.prio = e->d_prio;
        Sg.pmap = e->d_pmap; Sg.pbkt = e->d_pbkt; Sg.pdat = e->d_pdat; Sg.pbm = e->d_pbm;
        const uint32_t nm = (uint32_t)e->pmap_key.size();
        HIPCHK(launch_pm_grow(B.d_segs, sw + BS_NSEG, mb, Sg, e->d_pool_next, e->pool_nb, sw + BS_FLAGS, e->d_pmoves,
                              e->d_pmoves ? reinterpret_cast<uint32_t*>(e->d_pmoves + e->pmoves_cap) : nullptr,
                              (uint32_t)e->pmoves_cap, G.epoch, nm, e->d_pbkt2, e->d_pdat2, e->d_pcwork,
                              e->d_pcwork + e->pmoves_cap, e->d_pcwork + 2 * e->pmoves_cap, st));
        HIPCHK(hipMemcpyAsync(e->h_pool_next, e->d_pool_next, PC_WORDS * 8, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipEventRecord(B.ev[2], st));
    if (pre_split) {  // every map-touching pre-pass kernel after the maps grew (they move)
        HIPCHK(hipEventRecord(e->grown, st));
        HIPCHK(hipStreamWaitEvent(ps, e->grown, 0));
    }
    if (pv_ran) {  // the rest of the value-parallel pre pass
        HIPCHK(launch_pv_b(B.d_recs, B.d_segs, B.d_mix + B.mix_cap, n_mixw, S, t0, B.d_dec, sw + BS_FLAGS,
                           e->d_pvseg, e->pvb, head[BS_MIX_WIDE], e->d_pvtot, e->d_pvpart, (bflags & BF_ZERO_CNT) ? 0u : 1u, ps,
                           e->d_pvrest));
    }
    if (n_mix || n_mixw)
        HIPCHK(launch_pq_mix(0, B.d_recs, dev_ev, vin, B.d_segs, B.d_mix, n_mix, B.mix_cap, n_mixw, S, dc, t0,
                             B.d_dec, sw + BS_FLAGS, ps, pv_ran ? e->d_pvrest + 1 : nullptr, e->d_pvrest));
    // Pre-blocked ENTRYs of the cooperative bins' segments (SEG_UBLK): their words and RF_PBLK after the param pre
    // pass (whose block comes first) and before every owner; launched only in a batch that has such a segment
    // (and the ENTRYs the embedded token call answered BLOCKED, in a batch that made requests)
    if (head[BS_UBLK] || (S.emb && B.emb_coop))
        HIPCHK(launch_ublk_words(B.d_recs, B.d_segs, B.d_order + off[BIN_J16], off[BIN_J8 + 1] - off[BIN_J16], B.d_dec,
                                 sw + BS_UBLK_WORDS, S.emb, sw + BS_EMB_AHEAD, ps));
    HIPCHK(hipEventRecord(e->fork, ps));
    auto lane_bins = [&]() -> int {
        {
            DevState Sl = S;
            Sl.dbg = e->d_dbg;  // SG_KPROF builds: lane-kernel phase cycles in dbg[32..36]
            HIPCHK(launch_decide_bin(BIN_LANE, B.d_recs, dev_ev, vin, B.d_segs, B.d_order + off[BIN_LANE],
                                     off[BIN_LANE + LANE_BINS] - off[BIN_LANE], Sl, dc, t0, B.d_dec, sw + BS_FLAGS, st));
        }
        HIPCHK(launch_decide_bin(BIN_LANE16, B.d_recs, dev_ev, vin, B.d_segs, B.d_order + off[BIN_LANE16],
                                 off[BIN_LANE16 + LANE_BINS] - off[BIN_LANE16], S, dc, t0, B.d_dec, sw + BS_FLAGS, st));
        {
            DevState Sl = S;
            Sl.dbg = e->d_dbg;  // SG_KPROF builds: lane-kernel phase cycles in dbg[32..37]
            HIPCHK(launch_decide_bin(BIN_LITE, B.d_recs, dev_ev, vin, B.d_segs, B.d_order + off[BIN_LITE],
                                     off[BIN_LITE + LANE_BINS] - off[BIN_LITE], Sl, dc, t0, B.d_dec, sw + BS_FLAGS, st));
        }
        return SG_OK;
    };
    if (pre_split) {
        if (int lrc = lane_bins()) return lrc;
        HIPCHK(hipStreamWaitEvent(st, e->fork, 0));  // (J8 / J1 on the main stream read the pre passes' verdicts)
    }
    // J16 and J4 on their own streams; J1 after the lane bins on the main stream (J4 + J1 in series was the
    // longest chain of the decide stage)
    const int coop[2] = {BIN_J16, BIN_J4};
    // J8 (the QPS-DefaultController heads) takes J16's stream when every head is of that kind (C2, C4); beside
    // THREAD-grade / WarmUp heads (C3: J16 is the decide stage's longest chain) it runs first on the main stream
    const bool j8_own = bin_n[BIN_J8] && !bin_n[BIN_J16];
    for (int c = 0; c < 2; ++c) {
        const int b = coop[c];
        if (c == 0 && bin_n[BIN_J8]) {
            DevState Sb = S;
            Sb.dbg = (e->prof_bin == 0 && e->d_dbg) ? e->d_dbg : nullptr;
            hipStream_t bs = (serial_bins || !j8_own) ? st : e->bin_stream[0];
            if (bs != st) HIPCHK(hipStreamWaitEvent(bs, e->fork, 0));
            HIPCHK(launch_decide_bin(BIN_J8, B.d_recs, dev_ev, vin, B.d_segs, B.d_order + off[BIN_J8], bin_n[BIN_J8], Sb, dc,
                                     t0, B.d_dec, sw + BS_FLAGS, bs));
            if (bs != st) HIPCHK(hipEventRecord(e->join[0], bs));
        }
        if (!bin_n[b]) continue;
        DevState Sb = S;
        Sb.dbg = (c == e->prof_bin && e->d_dbg) ? e->d_dbg : nullptr;
        hipStream_t bs = serial_bins ? st : e->bin_stream[c];
        if (!serial_bins) HIPCHK(hipStreamWaitEvent(bs, e->fork, 0));
        HIPCHK(launch_decide_bin(b, B.d_recs, dev_ev, vin, B.d_segs, B.d_order + off[b], bin_n[b], Sb, dc, t0,
                                 B.d_dec, sw + BS_FLAGS, bs));
        HIPCHK(hipEventRecord(e->join[c], bs));
    }
    // hot-parameter owners (k_pq): the wide ones beside J16, the narrow ones beside J4
    for (int c = 0; c < 2; ++c) {
        const int b = c == 0 ? BIN_PQ16 : BIN_PQ4;
        if (!bin_n[b]) continue;
        hipStream_t bs = serial_bins ? st : e->bin_stream[c];
        if (!serial_bins && !bin_n[coop[c]] && !(c == 0 && j8_own)) HIPCHK(hipStreamWaitEvent(bs, e->fork, 0));
        DevState Sp = S;
        Sp.dbg = (c == 0 && e->prof_bin == 3) ? e->d_dbg : nullptr;  // SG_PROF_BIN=3: k_pq<16> phase cycles (kprof builds)
        HIPCHK(launch_pq(c == 0, B.d_recs, dev_ev, vin, B.d_segs, B.d_order + off[b], bin_n[b], Sp, dc, t0, B.d_dec,
                         sw + BS_FLAGS, bs));
        HIPCHK(hipEventRecord(e->join[c], bs));
    }
    if (!pre_split)
        if (int lrc = lane_bins()) return lrc;
    // sg_submit_ex: the short segments' origin / context nodes (aux.hip k_aux_cold) need only the lane bins' verdicts
    // when every short segment (<= AUX_SHORT = 256 events, decide.hip) is a lane one -- lane bins up to 256 events and
    // no k_pq<4> segment -- so they go right after them, beside the owners
    // (a short PF_PQ segment on k_pq<16>, SG_PQ_WIDE below 256, is not a lane one either: ADVICE r5)
    const bool aux_early = ext && !bin_n[BIN_PQ4] && !serial_bins && (force_lane || lane_max >= 256u) &&
                           (!bin_n[BIN_PQ16] || e->pq_wide >= 256u);
    if (aux_early)
        HIPCHK(launch_aux_cold(B.d_recs, B.d_segs, sw + BS_AUX, B.d_ashort, S, dc, t0, B.d_dec, sw + BS_FLAGS, st));
    // J1: after the lane bins on the main stream, or (SG_J1_STREAM=1, and with the short aux nodes on the main stream)
    // after J16 / J8 on bin_stream[0]
    const bool j1_b0 = bin_n[BIN_J1] && !serial_bins && (e->j1_stream == 1 || (e->j1_stream < 0 && aux_early));
    // SG_J1_STREAM=2: the J1 segments halved, one half after J16 / J8 on bin_stream[0], the other after J4 on
    // bin_stream[1] (A/B)
    const bool j1_split = bin_n[BIN_J1] > 1 && !serial_bins && e->j1_stream == 2;
    if (j1_split) {
        const uint32_t h = bin_n[BIN_J1] / 2;
        for (int c = 0; c < 2; ++c) {
            DevState Sj = S;
            Sj.dbg = nullptr;
            hipStream_t bs = e->bin_stream[c];
            const bool ran = c == 0 ? (bin_n[BIN_J16] || bin_n[BIN_J8] || bin_n[BIN_PQ16]) : (bin_n[BIN_J4] || bin_n[BIN_PQ4]);
            if (!ran) HIPCHK(hipStreamWaitEvent(bs, e->fork, 0));
            HIPCHK(launch_decide_bin(BIN_J1, B.d_recs, dev_ev, vin, B.d_segs, B.d_order + off[BIN_J1] + (c ? h : 0),
                                     c ? bin_n[BIN_J1] - h : h, Sj, dc, t0, B.d_dec, sw + BS_FLAGS, bs));
            HIPCHK(hipEventRecord(e->join[c], bs));
        }
    } else if (bin_n[BIN_J1]) {
        DevState Sj = S;
        Sj.dbg = (e->prof_bin == 2 && e->d_dbg) ? e->d_dbg : nullptr;
        hipStream_t bs = j1_b0 ? e->bin_stream[0] : st;
        if (j1_b0 && !(bin_n[BIN_J16] || bin_n[BIN_J8] || bin_n[BIN_PQ16])) HIPCHK(hipStreamWaitEvent(bs, e->fork, 0));
        HIPCHK(launch_decide_bin(BIN_J1, B.d_recs, dev_ev, vin, B.d_segs, B.d_order + off[BIN_J1], bin_n[BIN_J1], Sj, dc,
                                 t0, B.d_dec, sw + BS_FLAGS, bs));
        if (j1_b0) HIPCHK(hipEventRecord(e->join[0], bs));
    }
    for (int c = 0; c < 2; ++c)
        if (bin_n[coop[c]] || bin_n[c == 0 ? BIN_PQ16 : BIN_PQ4] || (c == 0 && (j8_own || j1_b0)) || j1_split)
            HIPCHK(hipStreamWaitEvent(st, e->join[c], 0));
    // verdicts of the frozen spans the cooperative kernels skipped
    if (S.skip_ok && (bin_n[BIN_J16] || bin_n[BIN_J8] || bin_n[BIN_J4]))
        HIPCHK(launch_fill(B.d_spans, S.nspan, e->span_cap, B.d_recs, e->d_prog, e->d_rules, B.d_dec, st));
    // XF_MIX: the thread-count maps and ParameterMetric bits from the final verdicts (the long ones value-parallel
    // where the maps do not overflow, pvalue.hip; the rest by k_pq's post pass)
    if (n_mixw && e->pvt_on && head[BS_MIX_WIDE])
        HIPCHK(launch_pvt(B.d_recs, dev_ev, vin, B.d_segs, B.d_mix + B.mix_cap, n_mixw, S, dc, B.d_dec,
                          sw + BS_FLAGS, e->d_pvtseg, e->pvbt, head[BS_MIX_WIDE], e->d_pvtot + 4, e->d_pvthist, e->d_pvtpart, st,
                          radix_tile(), e->d_pvrest + e->pvseg_cap + 1));
    const bool pvt_ran = n_mixw && e->pvt_on && head[BS_MIX_WIDE];
    uint32_t* prest = e->d_pvrest + e->pvseg_cap + 1;
    if (n_mix || n_mixw)
        HIPCHK(launch_pq_mix(1, B.d_recs, dev_ev, vin, B.d_segs, B.d_mix, n_mix, B.mix_cap, n_mixw, S, dc, t0,
                             B.d_dec, sw + BS_FLAGS, st, pvt_ran ? prest + 1 : nullptr, prest));
    // origin / context nodes of the segments decided off k_lane<16>, from the committed verdicts (aux.hip)
    if (ext)
        HIPCHK(launch_aux(B.d_recs, B.d_segs, sw + BS_AUX, aux_early ? nullptr : B.d_ashort, B.d_along, B.d_apiece,
                          B.d_amulti, S, dc, t0, B.d_dec, e->d_auxpool, e->auxpool_cap, sw + BS_AUX_POOL_N, e->d_auxmeta,
                          sw + BS_FLAGS, st));
    // the global inbound node from the same verdicts (inbound.hip), when it is tracked
    if (e->inb_on)
        HIPCHK(launch_inbound(B.d_recs, B.d_dec, n, dev_ev, vin, S, dc, t0, e->d_inbpart, e->d_inb, st));
    HIPCHK(hipEventRecord(B.ev[3], st));
    // ---- 4. decisions back to submission order + status ring
    if (B.radix) HIPCHK(launch_post(B.d_posof, B.d_dec, n, G.gbase, e->d_ring, ring_mask, dev_out, st));
    else HIPCHK(launch_post_w(B.d_flag, B.d_pos, B.nhot, B.d_dec, n, G.gbase, e->d_ring, ring_mask, dev_out, st));
    if (host_out) HIPCHK(hipMemcpyAsync(out, dev_out, n * 4, hipMemcpyDeviceToHost, st));
    // the flags and the span count for collect(), before the slot's next group stage clears them
    HIPCHK(hipMemcpyAsync(e->h_mirror + (size_t)G.set * BS_MIRROR_WORDS, B.d_bsmall, BS_MIRROR_WORDS * 4, hipMemcpyDeviceToHost,
                          st));
    HIPCHK(hipEventRecord(B.ev[4], st));
    B.last_post = B.ev[4];
    return SG_OK;
}

// Batch pipeline: the group stage of a batch runs on gstream, its decide stage on the decide streams behind the
// previous batch's, so batch k+1's group stage overlaps batch k's decide stage.  The group stage is the longer one,
// so the batch period is its time plus whatever gstream stands empty between two of them.  An async submit therefore
// does not wait for its own group stage: it returns with the batch grouped, and the next submit reads that batch's
// head (which the next group stage needs: the hot ids), queues its own first group kernel, and only then enqueues
// the earlier batch's decide stage.  The earlier batch's verdict is that call's to return.  Buffers must stay valid
// until sg_sync.
static int submit_impl(sg_engine* e, const sg_event* ev, const sg_event_ext* ext, uint64_t n, const sg_arg* args,
                       uint64_t n_args, uint32_t* out) {
    if (!e || (n && (!ev || !out))) return fail(SG_EINVAL, "null argument");
    if (n_args && !args) return fail(SG_EINVAL, "null args table");
    if (!e->fatal.empty()) return fail(SG_ESTATE, e->fatal + " -- engine unusable, recreate it");
    if (n == 0) return SG_OK;
    if (n > e->cfg.max_batch_events || n >= (1ull << 31)) return fail(SG_EINVAL, "batch larger than max_batch_events");
    HIPCHK(hipSetDevice(e->device));
    if (e->held_rc) return drain(e);  // an error a diagnostics export met: returned here, and this batch is not taken
    // SG_PIPELINE=0 and SG_HANDOFF=0 hand every batch off inside its own call; so does a finite chain cap, whose
    // grants the host orders inside the decide stage (two synchronizes, which would stall the group stage between its
    // first kernel and the rest)
    const bool late = e->handoff_late && e->pipeline && e->cfg.max_slot_chain_size <= 0;
    int rc;
    if (n > e->cap_n && (rc = drain(e))) return rc;  // (the buffers grow: no batch may be in them)
    // what can fail without a device error comes before the grouped batch is accepted, so such a failure leaves it
    // grouped for the next call
    if ((rc = ensure_batch(e, n))) return rc;
    if ((rc = ensure_pool2(e))) return rc;
    // 1. the grouped batch's verdict: an error is this call's to return, and this batch is then not taken
    int prev = e->grouped;
    if (prev >= 0 && (rc = accept_grouped(e))) return rc;
    // From here batch `prev` is counted.  Whatever makes this call fail before that batch's decide stage is enqueued
    // enqueues it first: an accepted batch is always decided.
    auto give_up = [&](int why) -> int {
        if (prev >= 0) {
            const std::string msg = g_err;
            const int pk = prev;
            prev = -1;
            if (decide_stage(e, pk) == SG_OK) g_err = msg;
        }
        return why;
    };
    // the param map pool: the regions maps grew out of are dropped by a compaction between batches once the growth
    // since the last one took half of what was free (the counts are a batch or two old); a batch that finds the pool
    // short before that compacts on the device itself (launch_pm_grow)
    const unsigned long long pfloor = e->h_pool_next ? e->h_pool_next[PC_FLOOR] : 0;
    const bool compact = e->pool_nb && e->h_pool_next[PC_NEXT] > pfloor + (e->pool_nb - pfloor) / 2;
    // A grouped batch with events of XF_EMB resources (embedded token server) gives up its overlap: its token call
    // uses the other slot's arrays as scratch and waits on the host, so its decide stage goes first
    const bool emb_prev = prev >= 0 && e->slot[prev].emb_ub != 0;
    if (!late || compact || emb_prev) {  // the earlier order: the batch two back is collected before its slot is taken again
        if (prev >= 0) {
            const int pk = prev;
            prev = -1;
            if ((rc = decide_stage(e, pk))) return rc;
        }
        while (e->inflight.size() > 1)
            if ((rc = collect(e))) return rc;
    }
    if (compact) {
        if (int drc = drain(e)) return drc;
        if (int crc = compact_pmaps(e)) return crc;
        ++e->n_compact;
    }
    // 2.-5. the slot is reused in device order; this batch's first group kernel, the previous batch's decide stage
    // (group_stage clears prev once it has enqueued it), the rest of this group stage
    const int k = e->cur;
    if ((rc = group_stage(e, k, ev, ext, n, args, n_args, out, &prev))) return give_up(rc);
    if (!late) return handoff(e);
    // 6. the batch before the previous one: its times and flags.  The host may wait here: nothing on the device waits
    // for the host any more.  An error drops the batch just grouped, so a call that fails has taken no batch.
    while (e->inflight.size() > 1)
        if ((rc = collect(e))) {
            (void)accept_grouped(e, true);
            return rc;
        }
    return SG_OK;
}

// A synchronous batch of at most tiny_max() events in one kernel (decide.hip k_tiny: every stage in one workgroup):
// the drop-in's small calls.  Returns SG_OK, an error (as the batched path's, at the same points: a malformed batch is
// rejected before any decision), or TINY_FALLBACK when the batch needs the batched path (a chain grant under a finite
// cap, which the host orders; a param pool that must be compacted first) -- nothing was decided then.
constexpr int TINY_FALLBACK = 1;
static int tiny_impl(sg_engine* e, const sg_event* ev, const sg_event_ext* ext, uint64_t n, const sg_arg* args,
                     uint64_t n_args, uint32_t* out) {
    if (!e || !ev || !out) return fail(SG_EINVAL, "null argument");
    if (n_args && !args) return fail(SG_EINVAL, "null args table");
    if (!e->fatal.empty()) return fail(SG_ESTATE, e->fatal + " -- engine unusable, recreate it");
    if (n > e->cfg.max_batch_events) return fail(SG_EINVAL, "batch larger than max_batch_events");
    HIPCHK(hipSetDevice(e->device));
    int rc = ensure_batch(e, n);
    if (rc) return rc;
    if ((rc = drain(e))) return rc;  // every earlier batch decided: the status ring holds their verdicts
    if ((rc = ensure_pool2(e))) return rc;
    const unsigned long long pfloor = e->h_pool_next ? e->h_pool_next[PC_FLOOR] : 0;
    if (e->pool_nb && e->h_pool_next[PC_NEXT] > pfloor + (e->pool_nb - pfloor) / 2) return TINY_FALLBACK;  // compaction due
    auto& B = e->slot[e->cur];
    hipStream_t st = e->stream;
    const sg_event* dev_ev = ev;
    const bool host_out = !is_device_ptr(out);
    if (!is_device_ptr(ev)) {
        HIPCHK(hipMemcpyAsync(B.d_ev, ev, n * sizeof(sg_event), hipMemcpyHostToDevice, st));
        dev_ev = B.d_ev;
    }
    uint32_t* dev_out = host_out ? B.d_out : out;
    const sg_event_ext* dev_ext;
    const sg_arg* dev_args;
    if ((rc = stage_ext_args(B, ext, n, args, n_args, st, &dev_ext, &dev_args))) return rc;
    if (++e->epoch == 0) e->epoch = 1;
    DevCfg dc;
    DevState S;
    fill_state(e, B, (1ull << e->cfg.status_ring_log2) - 1, dev_ext, dev_args, dc, S);
    S.gbase = e->gbase;
    S.epoch = e->epoch;
    S.skip_ok = 0;
    S.skip_min = e->skip_min;
    // the chain grants: every one in place (no cap), none (a cap reached: CtSph.lookProcessChain then returns null),
    // or the host's, in first-ENTRY order (the batched path)
    const int cap = e->cfg.max_slot_chain_size;
    const uint32_t grants = cap <= 0 ? 1u : e->n_chains >= (uint32_t)cap ? 2u : 0u;
    HIPCHK(launch_tiny(dev_ev, (uint32_t)n, S, dc, e->cfg.max_resources, e->d_prio, e->d_comp, n_args, grants,
                       e->d_pool_next, e->pool_nb, e->epoch, B.d_recs, B.d_v0, B.d_dec, B.d_segs, B.d_bsmall + BS_FLAGS,
                       dev_out, st));
    uint32_t bflags = 0;
    HIPCHK(hipMemcpyAsync(&bflags, B.d_bsmall + BS_FLAGS, 4, hipMemcpyDeviceToHost, st));
    if (host_out) HIPCHK(hipMemcpyAsync(out, dev_out, n * 4, hipMemcpyDeviceToHost, st));
    if (e->pool_nb) HIPCHK(hipMemcpyAsync(e->h_pool_next, e->d_pool_next, PC_WORDS * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (bflags & BF_TINY_FALLBACK) return TINY_FALLBACK;
    // rejected before any decision: the group stage's checks, in their order (k_tiny raises the flag with one of them)
    if (bflags & BF_TINY_REJECTED) return group_verdict(bflags);
    e->gbase += n;
    // the global inbound node: the two kernels of the batched path behind a call k_tiny decided (recs, dec and the
    // submission indices are in global memory); the caller's buffers are free again when this returns
    if (e->inb_on) {
        int64_t t0 = 0;
        HIPCHK(hipMemcpy(&t0, &dev_ev[0].ts, 8, hipMemcpyDeviceToHost));
        HIPCHK(launch_inbound(B.d_recs, B.d_dec, n, dev_ev, B.d_v0, S, dc, t0, e->d_inbpart, e->d_inb, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    // the decide stage's own flags, as collect() reads them.  (Its BF_LITE_STALE check cannot fire here: only k_lite
    // raises that flag, and k_tiny decides with lane_seg<16>.)
    return decide_verdict(e, bflags);
}

int sg_submit_async(sg_engine* e, const sg_event* ev, uint64_t n, uint32_t* out) {
    return submit_impl(e, ev, nullptr, n, nullptr, 0, out);
}

int sg_submit_ex_async(sg_engine* e, const sg_event* ev, const sg_event_ext* ext, uint64_t n, const sg_arg* args,
                       uint64_t n_args, uint32_t* out) {
    return submit_impl(e, ev, ext, n, args, n_args, out);
}

int sg_submit_ex(sg_engine* e, const sg_event* ev, const sg_event_ext* ext, uint64_t n, const sg_arg* args,
                 uint64_t n_args, uint32_t* out) {
    if (e && e->tiny_on && !e->emb_n && n && n <= tiny_max() && !e->radix_group) {
        const int trc = tiny_impl(e, ev, ext, n, args, n_args, out);
        if (trc != TINY_FALLBACK) return trc;
    }
    int rc = submit_impl(e, ev, ext, n, args, n_args, out);
    if (rc) {
        if (e) (void)drain(e);
        return rc;
    }
    return sg_sync(e);
}

// ContextUtil.enter(name, origin) names (core/context/ContextUtil.java:118-166).  A flow rule naming an origin
// (limitApp) or a context (STRATEGY_CHAIN refResource) before it was interned was compiled to match nothing;
// the first intern of such a name recompiles the rule programs, keeping every controller / breaker state.
int sg_intern_origin(sg_engine* e, const char* origin, uint32_t* out_id) {
    if (!e || !out_id) return fail(SG_EINVAL, "null argument");
    if (!origin || !*origin) { *out_id = 0; return SG_OK; }
    auto it = e->origin_ids.find(origin);
    if (it != e->origin_ids.end()) { *out_id = it->second; return SG_OK; }
    const uint32_t id = (uint32_t)e->origin_ids.size() + 1;
    if (id >= 0x7FFFFFFFu) return fail(SG_ECAPACITY, "too many origins");
    e->origin_ids.emplace(origin, id);
    *out_id = id;
    if (e->auth.by_name.count(origin)) {  // an authority rule lists the name: its id joins the rules' lists
        if (int rc = drain(e)) return rc;
        e->auth.on_intern(origin, id);
        if (int rc = upload_authority(e)) return rc;
    }
    if (e->rule_names.count(std::string("o\x01") + origin)) {
        if (int rc = drain(e)) return rc;
        return upload_rules(e, false, false, false);
    }
    return SG_OK;
}

int sg_intern_context(sg_engine* e, const char* context, uint32_t* out_id) {
    if (!e || !out_id) return fail(SG_EINVAL, "null argument");
    if (!context || !*context || !std::strcmp(context, "sentinel_default_context")) { *out_id = 0; return SG_OK; }
    auto it = e->context_ids.find(context);
    if (it != e->context_ids.end()) { *out_id = it->second; return SG_OK; }
    const uint32_t id = (uint32_t)e->context_ids.size() + 1;
    e->context_ids.emplace(context, id);
    *out_id = id;
    if (e->rule_names.count(std::string("c\x01") + context)) {
        if (int rc = drain(e)) return rc;
        return upload_rules(e, false, false, false);
    }
    return SG_OK;
}

int sg_sync(sg_engine* e) {
    if (!e) return fail(SG_EINVAL, "null engine");
    HIPCHK(hipSetDevice(e->device));
    return drain(e);
}

int sg_submit(sg_engine* e, const sg_event* ev, uint64_t n, uint32_t* out) {
    if (e && e->tiny_on && !e->emb_n && n && n <= tiny_max() && !e->radix_group) {
        const int trc = tiny_impl(e, ev, nullptr, n, nullptr, 0, out);
        if (trc != TINY_FALLBACK) return trc;
    }
    int rc = sg_submit_async(e, ev, n, out);
    if (rc) {
        if (e) (void)drain(e);
        return rc;
    }
    return sg_sync(e);
}

int sg_last_timings(sg_engine* e, double* ms, int cap) {
    if (!e || !ms) return 0;
    int k = 0;
    for (; k < cap && k < 4; ++k) ms[k] = e->last_ms[k];
    return k;
}

int sg_param_thread_count(sg_engine* e, uint32_t res, int32_t idx, uint64_t key, int64_t* count, int32_t* present) {
    if (!e || !count) return fail(SG_EINVAL, "null argument");
    if (res >= e->cfg.max_resources) return fail(SG_EINVAL, "res_id out of range");
    if (int rc = drain(e)) return rc;
    *count = 0;
    if (present) *present = 0;
    if (idx < 0 || idx >= SG_MAX_ARGS) return SG_OK;
    const uint64_t want = TMAP_KEY | ((uint64_t)res << 8) | (uint64_t)idx;
    uint32_t id = NO_ID;
    for (uint32_t i = 0; i < (uint32_t)e->pmap_key.size(); ++i)
        if (e->pmap_key[i] == want) { id = i; break; }
    if (id == NO_ID) return SG_OK;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    PMap m;
    HIPCHK(hipMemcpy(&m, e->d_pmap + id, sizeof(m), hipMemcpyDeviceToHost));
    uint32_t b[2];
    pm_buckets(m.nb, key, b[0], b[1]);
    for (int h = 0; h < 2; ++h) {
        PBucket bk;
        HIPCHK(hipMemcpy(&bk, e->d_pbkt + m.base + b[h], sizeof(bk), hipMemcpyDeviceToHost));
        for (int j = 0; j < PM_BKT; ++j) {
            if (bk.key[j] != key) continue;
            const int64_t st = bk.stamp[j];
            if (st < m.thr || st >= m.clock) continue;  // a dead slot
            const uint64_t p = (uint64_t)st & ((1ull << m.rb_log2) - 1);
            uint64_t w = 0;
            HIPCHK(hipMemcpy(&w, e->d_pbm + m.bm + (p >> 6), 8, hipMemcpyDeviceToHost));
            if (!((w >> (p & 63)) & 1ull)) continue;
            PData d;
            HIPCHK(hipMemcpy(&d, e->d_pdat + (m.base + b[h]) * PM_BKT + j, sizeof(d), hipMemcpyDeviceToHost));
            *count = d.v0;
            if (present) *present = 1;
            return SG_OK;
        }
    }
    return SG_OK;
}

int sg_read_node(sg_engine* e, uint32_t res, int64_t now_ms, sg_node_state* out) {
    (void)now_ms;
    if (!e || !out) return fail(SG_EINVAL, "null argument");
    if (res >= e->cfg.max_resources) return fail(SG_EINVAL, "res_id out of range");
    if (int rc = drain(e)) return rc;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    Bkt sec[2], mb[60];
    int64_t bor[4];
    NodeInfo ni;
    HIPCHK(hipMemcpy(bor, e->d_borrow + (uint64_t)res * 4, sizeof(bor), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(sec, e->d_sec + (uint64_t)res * 2, sizeof(sec), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(mb, e->d_minb + (uint64_t)res * 60, sizeof(mb), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&ni, e->d_info + res, sizeof(ni), hipMemcpyDeviceToHost));
    std::memset(out, 0, sizeof(*out));
    auto ex = [](const Bkt& b, sg_bucket& o) {
        if (b.ws < 0) { std::memset(&o, 0, sizeof(o)); o.window_start = -1; return; }
        o.window_start = b.ws; o.pass = b.pass; o.block = b.block; o.exception = b.exc; o.success = b.succ;
        o.rt = b.rt; o.occupied_pass = b.occ; o.min_rt = b.minrt;
    };
    for (int i = 0; i < 8; ++i) { out->second[i].window_start = -1; out->borrow[i].window_start = -1; }
    bool chain = (ni.flags & NI_CHAIN) != 0;
    if (chain) {
        ex(sec[0], out->second[0]);
        ex(sec[1], out->second[1]);
        for (int i = 0; i < 60; ++i) ex(mb[i], out->minute[i]);
        for (int i = 0; i < 2; ++i)  // FutureBucketLeapArray buckets: pass only (min_rt as created)
            if (bor[2 * i] >= 0) {
                out->borrow[i].window_start = bor[2 * i];
                out->borrow[i].pass = bor[2 * i + 1];
                out->borrow[i].min_rt = e->cfg.statistic_max_rt;
            }
    } else {
        for (int i = 0; i < 60; ++i) out->minute[i].window_start = -1;
    }
    out->cur_thread_num = chain ? ni.thread : 0;
    out->has_chain = chain ? 1 : 0;
    return SG_OK;
}

// StatisticNode.metrics() of the global inbound node, appended to the *n ClusterNode rows of a snapshot (the pipeline
// is drained): details() creates / resets the bucket of now as k_snap_count does for a ClusterNode, then the buckets
// after the node's own lastFetchTime and before the current second are the rows, in slot order.  One node's 60 buckets:
// host arithmetic on a copy, written back.
static int snapshot_inbound(sg_engine* e, int64_t now_ms, sg_metric_node* out, uint64_t cap, uint64_t* n) {
    InbNode nd;
    HIPCHK(hipMemcpy(&nd, e->d_inb, sizeof(nd), hipMemcpyDeviceToHost));
    const int64_t cur = now_ms - now_ms % 1000;
    if (now_ms >= 0) {
        Bkt& c = nd.minb[(now_ms / 1000) % 60];
        if (c.ws < cur) { std::memset(&c, 0, sizeof(c)); c.ws = cur; c.minrt = e->cfg.statistic_max_rt; }
    }
    std::vector<sg_metric_node> rows;
    int64_t nl = nd.last_fetch;
    for (const Bkt& b : nd.minb) {
        if (b.ws < 0 || now_ms - b.ws > 60000) continue;
        const int64_t rt = b.succ != 0 ? b.rt / b.succ : b.rt;
        if (!(b.ws > nd.last_fetch && b.ws < cur)) continue;
        if (!(b.pass > 0 || b.block > 0 || b.succ > 0 || b.exc > 0 || rt > 0 || b.occ > 0)) continue;
        sg_metric_node m;
        std::memset(&m, 0, sizeof(m));
        m.timestamp = b.ws; m.pass_qps = b.pass; m.block_qps = b.block; m.success_qps = b.succ;
        m.exception_qps = b.exc; m.rt = rt; m.occupied_pass_qps = b.occ; m.res_id = SG_RES_TOTAL_INBOUND;
        rows.push_back(m);
        nl = std::max(nl, b.ws);
    }
    nd.last_fetch = nl;
    HIPCHK(hipMemcpy(e->d_inb, &nd, sizeof(nd), hipMemcpyHostToDevice));
    const uint64_t base = *n;
    if (out && base < cap && !rows.empty()) {
        const uint64_t k = std::min<uint64_t>(rows.size(), cap - base);
        HIPCHK(hipMemcpy(out + base, rows.data(), k * sizeof(sg_metric_node), hipMemcpyDefault));
    }
    *n = base + rows.size();
    return SG_OK;
}

int sg_snapshot_metrics(sg_engine* e, int64_t now_ms, sg_metric_node* out, uint64_t cap, uint64_t* n) {
    if (!e || !n) return fail(SG_EINVAL, "null argument");
    HIPCHK(hipSetDevice(e->device));
    if (int rc = drain(e)) return rc;
    uint32_t R = (uint32_t)std::min<size_t>(e->names.size(), e->cfg.max_resources);
    if (R == 0) {
        *n = 0;
        return e->inb_on ? snapshot_inbound(e, now_ms, out, cap, n) : SG_OK;
    }
    if (!e->d_snap_cnt) {
        HIPCHK(hipMalloc(&e->d_snap_cnt, (uint64_t)e->cfg.max_resources * 4));
        HIPCHK(hipMalloc(&e->d_snap_off, (uint64_t)e->cfg.max_resources * 4));
    }
    // out may be device memory (e.g. the buffer an RCCL all-gather sends from): the kernels write it
    // directly, no staging buffer and no host round trip
    const bool dev_out = out && is_device_ptr(out);
    if (!dev_out && cap > e->snap_cap) HIPCHK(grow(e->d_snap_out, e->snap_cap, cap, 1));
    // the count's scan partials: the d_part of a batch slot (drained: no batch is in it), which an engine that has
    // taken no batch yet does not have
    if (int rc = ensure_batch(e, 1)) return rc;
    auto& scratch = e->slot[e->cur];
    e->snap_hi = std::max(e->snap_hi, now_ms - now_ms % 1000);  // k_snap_count writes the bucket of now (DevCfg.snap_hi)
    HIPCHK(launch_snapshot(e->d_minb, e->d_info, R, now_ms, e->cfg.statistic_max_rt, e->d_snap_cnt, e->d_snap_off,
                           scratch.d_part, e->d_small + SM_SNAP_TOTAL, dev_out ? out : e->d_snap_out, dev_out || out ? cap : 0,
                           e->stream));
    uint32_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, e->d_small + SM_SNAP_TOTAL, 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    uint64_t k = std::min<uint64_t>(total, cap);
    if (k && out && !dev_out)
        HIPCHK(hipMemcpy(out, e->d_snap_out, k * sizeof(sg_metric_node), hipMemcpyDeviceToHost));
    *n = total;
    return e->inb_on ? snapshot_inbound(e, now_ms, out, cap, n) : SG_OK;
}

int sg_track_inbound(sg_engine* e, int32_t on) {
    if (!e) return fail(SG_EINVAL, "null engine");
    HIPCHK(hipSetDevice(e->device));
    if (int rc = drain(e)) return rc;
    if ((on != 0) == e->inb_on) return SG_OK;
    if (!on) { e->inb_on = false; return SG_OK; }  // the node stays readable
    // entries of the batches before this call were never counted: their exits would take threads the node never had
    if (e->gbase != 0) return fail(SG_ESTATE, "sg_track_inbound(1) after the first accepted batch");
    if (!e->d_inb) {
        HIPCHK(hipMalloc(&e->d_inb, sizeof(InbNode)));
        HIPCHK(hipMalloc(&e->d_inbpart, (size_t)INB_MAX_WG * sizeof(InbPart)));
        InbNode z;
        std::memset(&z, 0, sizeof(z));
        for (auto& b : z.sec) b.ws = -1;
        for (auto& b : z.minb) b.ws = -1;
        z.last_fetch = -1;
        HIPCHK(hipMemcpy(e->d_inb, &z, sizeof(z), hipMemcpyHostToDevice));
    }
    e->inb_on = e->inb_ever = true;
    return SG_OK;
}

// the node on the host, every batch counted
static int inbound_fetch(sg_engine* e, InbNode* nd) {
    if (!e->inb_ever) return fail(SG_ESTATE, "the inbound node was never tracked (sg_track_inbound)");
    HIPCHK(hipSetDevice(e->device));
    if (int rc = drain(e)) return rc;
    HIPCHK(hipMemcpy(nd, e->d_inb, sizeof(*nd), hipMemcpyDeviceToHost));
    return SG_OK;
}

int sg_read_inbound_node(sg_engine* e, int64_t now_ms, sg_node_state* out) {
    (void)now_ms;
    if (!e || !out) return fail(SG_EINVAL, "null argument");
    InbNode nd;
    if (int rc = inbound_fetch(e, &nd)) return rc;
    std::memset(out, 0, sizeof(*out));
    auto ex = [](const Bkt& b, sg_bucket& o) {
        if (b.ws < 0) { std::memset(&o, 0, sizeof(o)); o.window_start = -1; return; }
        o.window_start = b.ws; o.pass = b.pass; o.block = b.block; o.exception = b.exc; o.success = b.succ;
        o.rt = b.rt; o.occupied_pass = b.occ; o.min_rt = b.minrt;
    };
    for (int i = 0; i < 8; ++i) { out->second[i].window_start = -1; out->borrow[i].window_start = -1; }
    ex(nd.sec[0], out->second[0]);
    ex(nd.sec[1], out->second[1]);
    for (int i = 0; i < 60; ++i) ex(nd.minb[i], out->minute[i]);
    out->cur_thread_num = nd.thread;
    out->has_chain = 1;
    return SG_OK;
}

// What SystemRuleManager.checkSystem and SystemStatusListener read of ENTRY_NODE (StatisticNode.java:153-260), on a
// copy of its second window: ArrayMetric reads take data.currentWindow() first, so the bucket of now counts as reset
// when it holds an older window -- on the copy only, the node keeps its buckets.
int sg_inbound_metrics(sg_engine* e, int64_t now_ms, double* out, int cap) {
    if (!e || !out) return 0;
    InbNode nd;
    if (inbound_fetch(e, &nd)) return 0;
    const int64_t max_rt = e->cfg.statistic_max_rt;
    if (now_ms >= 0) {
        Bkt& c = nd.sec[(now_ms / 500) & 1];
        const int64_t ws = now_ms - now_ms % 500;
        if (c.ws < ws) { std::memset(&c, 0, sizeof(c)); c.ws = ws; c.minrt = max_rt; }
    }
    int64_t pass = 0, block = 0, succ = 0, exc = 0, rt = 0, min_rt = max_rt, max_succ = 0;
    for (const Bkt& b : nd.sec) {
        if (b.ws < 0 || now_ms - b.ws > 1000) continue;  // LeapArray.isWindowDeprecated
        pass += b.pass; block += b.block; succ += b.succ; exc += b.exc; rt += b.rt;
        min_rt = std::min(min_rt, b.minrt);
        max_succ = std::max(max_succ, b.succ);
    }
    const double v[9] = {(double)pass, (double)block, (double)succ, (double)exc, (double)pass + (double)block,
                         succ ? (double)rt / (double)succ : 0.0, (double)std::max<int64_t>(min_rt, 1),
                         (double)std::max<int64_t>(max_succ, 1) * 2.0, (double)nd.thread};
    int k = 0;
    for (; k < 9 && k < cap; ++k) out[k] = v[k];
    return k;
}

// diagnostics export: the inbound pass of the last collected batch: [0] workgroups that left a partial, [1] records
// visited, [2] updates counted.  Returns the values written.
extern "C" int sgx_inbound_last(sg_engine* e, unsigned long long* out, int cap) {
    if (!e || !out || !e->inb_ever) return 0;
    drain_hold(e);
    InbNode nd;
    if (hipMemcpy(&nd, e->d_inb, sizeof(nd), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    int k = 0;
    for (; k < 3 && k < cap; ++k) out[k] = nd.last[k];
    return k;
}

int sg_cluster_set_connected_count(sg_engine* e, int64_t flow_id, int32_t connected) {
    if (!e) return fail(SG_EINVAL, "null engine");
    if (int rc = drain(e)) return rc;
    // ClusterFlowRuleManager / ClusterParamFlowRuleManager.getConnectedCount: the namespace's count
    auto it = e->cmap.find(flow_id);
    auto pt = e->pmap.find(flow_id);
    if (it == e->cmap.end() && pt == e->pmap.end()) return fail(SG_ENOTFOUND, "no cluster rule with this flowId");
    if (it != e->cmap.end()) {
        e->cflows[it->second].connected = connected;
        HIPCHK(hipMemcpy(&e->d_cflow[it->second].connected, &connected, sizeof(int32_t), hipMemcpyHostToDevice));
    }
    if (pt != e->pmap.end()) {
        e->pflows[pt->second].connected = connected;
        HIPCHK(hipMemcpy(&e->d_pflow[pt->second].connected, &connected, sizeof(int32_t), hipMemcpyHostToDevice));
    }
    return SG_OK;
}

// ---- namespaces: a RequestLimiter and a connected count each (GlobalRequestLimiter, ConnectionManager)
// the limiters (never created), their limits and the grouped limiter's per-namespace words, on first use
static int ensure_ns(sg_engine* e) {
    if (e->d_nslim) return SG_OK;
    std::vector<NsLimiter> z(SG_MAX_NAMESPACES);
    for (auto& l : z)
        for (int k = 0; k < NS_BUCKETS; ++k) { l.ws[k] = -1; l.cnt[k] = 0; }
    std::vector<double> lim(SG_MAX_NAMESPACES, -1.0);
    std::copy(e->ns_limit.begin(), e->ns_limit.end(), lim.begin());
    if (!e->d_nslimit) HIPCHK(hipMalloc(&e->d_nslimit, SG_MAX_NAMESPACES * sizeof(double)));
    if (!e->d_nsb) HIPCHK(hipMalloc(&e->d_nsb, SG_MAX_NAMESPACES * 2 * 4));
    HIPCHK(hipMemcpy(e->d_nslimit, lim.data(), lim.size() * sizeof(double), hipMemcpyHostToDevice));
    NsLimiter* d = nullptr;
    HIPCHK(hipMalloc(&d, z.size() * sizeof(NsLimiter)));
    if (hipMemcpy(d, z.data(), z.size() * sizeof(NsLimiter), hipMemcpyHostToDevice) != hipSuccess) {
        dfree(d);
        return fail(SG_EDEVICE, "limiter initialisation failed");
    }
    e->d_nslim = d;
    return SG_OK;
}
// A token call's stable radix sort of n (key, request) pairs with keys 0..nkeys.  It writes the pair arrays it is
// passed (kin / vin and kout / vout, which swap with every pass: on return kin / vin hold the sorted pairs) and
// scratch.d_hist and scratch.d_part (the digit histograms and the scan's partials) of the borrowed slot.
static int tok_sort(sg_engine* e, sg_engine::BatchSlot& scratch, uint64_t n, uint32_t nkeys, uint32_t*& kin,
                    uint32_t*& vin, uint32_t*& kout, uint32_t*& vout) {
    hipStream_t st = e->stream;
    int bits = 1;
    while (bits < 32 && (1ull << bits) <= nkeys) ++bits;
    const int passes = (bits + 7) / 8;
    const uint32_t nblocks = (uint32_t)((n + radix_tile() - 1) / radix_tile());
    for (int p = 0; p < passes; ++p) {
        HIPCHK(launch_radix_hist(kin, n, p * 8, scratch.d_hist, nblocks, st));
        HIPCHK(launch_scan(scratch.d_hist, scratch.d_hist, (uint64_t)nblocks * 256, scratch.d_part, nullptr, st));
        HIPCHK(launch_radix_scatter(kin, vin, n, p * 8, scratch.d_hist, nblocks, kout, vout, nullptr, st));
        std::swap(kin, kout);
        std::swap(vin, vout);
    }
    return SG_OK;
}
// The limiter step of a token call and the sort of its requests by flow index, for both token calls.  The requests
// are classified (k_tok_classify: e->d_tfidx, and for the grouped limiter the (namespace index, request) pairs in
// scratch.d_k0 / d_v0).  grouped: several limiters -- a stable sort by namespace (nns = tries no limiter), then every
// namespace's limiter over its own run (cluster.hip 2'); else the one limiter, parallel per 100 ms bucket, or with
// one_wave on one wave.  Then, when flows are loaded, the sort by flow index (nflows = not for a flow).  On return
// kin / vin hold the pairs as the flows' kernels read them.
// scratch: the batch slot the call borrows.  It overwrites the slot's d_k0 / d_v0 / d_k1 / d_v1 (the pairs), d_hist
// and d_part (the sorts and scans) and d_flag, d_pos, d_order, d_prev, d_dec, d_posof (the parallel limiters' n-word
// arrays), so no batch may be in the slot: its last batch is decided, and the next group stage into it runs after the
// call (drain() before the call, or BatchSlot::lent).
static int tok_limit_sort(sg_engine* e, sg_engine::BatchSlot& scratch, uint64_t n, uint32_t nflows, bool grouped,
                          bool one_wave, uint32_t*& kin, uint32_t*& vin) {
    hipStream_t st = e->stream;
    auto& X = scratch;
    // GlobalRequestLimiter: a negative qpsAllowed stands for "no limiter registered" (tryPass -> true)
    const double allowed = e->ns_limit[0] < 0 ? 1.0 / 0.0 : e->ns_limit[0];
    uint32_t *kout = X.d_k1, *vout = X.d_v1;
    kin = X.d_k0;
    vin = X.d_v0;
    if (grouped) {
        const uint32_t nns = (uint32_t)e->ns_names.size();
        if (int rc = tok_sort(e, X, n, nns, kin, vin, kout, vout)) return rc;
        HIPCHK(launch_tok_limiter_ns(e->d_treq, n, kin, vin, e->d_tfidx, nflows, e->d_nslim, e->d_nslimit, nns, kout, vout,
                                     e->d_tres, X.d_flag, X.d_pos, X.d_order, X.d_prev, X.d_part, e->d_small + SM_LIMITER,
                                     e->d_nsb, st));
        std::swap(kin, kout);
        std::swap(vin, vout);
    } else if (one_wave)
        HIPCHK(launch_tok_limiter(e->d_treq, n, e->d_tfidx, nflows, e->d_nslim, allowed, X.d_k0, X.d_v0, e->d_tres, st));
    else
        HIPCHK(launch_tok_limiter_par(e->d_treq, n, e->d_tfidx, nflows, e->d_nslim, allowed, X.d_k0, X.d_v0, e->d_tres,
                                      X.d_flag, X.d_pos, X.d_order, X.d_prev, X.d_dec, X.d_posof, X.d_part,
                                      e->d_small + SM_LIMITER, st));
    if (nflows)
        if (int rc = tok_sort(e, X, n, nflows, kin, vin, kout, vout)) return rc;
    return SG_OK;
}
// CSlot.pad of a loaded flowId table := the flowIds' namespace indices
static int upload_ns_pads(sg_engine* e, CSlot* d_tab, uint32_t mask) {
    if (!d_tab) return SG_OK;
    std::vector<CSlot> tab((size_t)mask + 1);
    HIPCHK(hipMemcpy(tab.data(), d_tab, tab.size() * sizeof(CSlot), hipMemcpyDeviceToHost));
    for (auto& t : tab)
        if (t.idx != 0xFFFFFFFFu) t.pad = ns_index(e, t.key);
    HIPCHK(hipMemcpy(d_tab, tab.data(), tab.size() * sizeof(CSlot), hipMemcpyHostToDevice));
    return SG_OK;
}

int sg_cluster_namespace(sg_engine* e, const char* ns, double max_allowed_qps, uint32_t* out_ns_id) {
    if (!e) return fail(SG_EINVAL, "null engine");
    if (!ns || !ns[0]) return fail(SG_EINVAL, "namespace cannot be empty");  // AssertUtil.notEmpty
    if (max_allowed_qps != max_allowed_qps) return fail(SG_EINVAL, "max_allowed_qps is not a number");
    if (int rc = drain(e)) return rc;
    auto it = e->ns_of.find(ns);
    uint32_t id;
    if (it != e->ns_of.end()) id = it->second;
    else {
        if (e->ns_names.size() >= SG_MAX_NAMESPACES) return fail(SG_ECAPACITY, "too many namespaces");
        id = (uint32_t)e->ns_names.size();
        e->ns_names.push_back(ns);
        e->ns_of[ns] = id;
        e->ns_limit.push_back(-1.0);
        e->ns_conn.push_back(0);
    }
    // RequestLimiter.setQpsAllowed: the limit alone, the window stays
    e->ns_limit[id] = max_allowed_qps;
    if (e->d_nslimit)
        HIPCHK(hipMemcpy(e->d_nslimit + id, &max_allowed_qps, sizeof(double), hipMemcpyHostToDevice));
    if (out_ns_id) *out_ns_id = id;
    return SG_OK;
}

int sg_cluster_assign_flows(sg_engine* e, const char* ns, const int64_t* flow_ids, uint32_t n) {
    if (!e || !ns || (n && !flow_ids)) return fail(SG_EINVAL, "null argument");
    auto it = e->ns_of.find(ns);
    if (it == e->ns_of.end()) return fail(SG_ENOTFOUND, "namespace is not registered");
    const uint32_t id = it->second;
    bool changes = false;
    for (uint32_t i = 0; i < n; ++i) {
        if (flow_ids[i] <= 0) return fail(SG_EINVAL, "flowId must be positive");
        auto f = e->flow_ns.find(flow_ids[i]);
        if (f == e->flow_ns.end()) changes = true;
        else if (f->second != id) return fail(SG_ESTATE, "flowId belongs to another namespace");
    }
    if (!changes) return SG_OK;
    if (int rc = drain(e)) return rc;
    for (uint32_t i = 0; i < n; ++i) e->flow_ns[flow_ids[i]] = id;
    if (int rc = upload_ns_pads(e, e->d_ctab, e->ctab_mask)) return rc;
    return upload_ns_pads(e, e->d_pftab, e->pftab_mask);
}

int sg_cluster_set_namespace_connected(sg_engine* e, const char* ns, int32_t connected) {
    if (!e || !ns) return fail(SG_EINVAL, "null argument");
    auto it = e->ns_of.find(ns);
    if (it == e->ns_of.end()) return fail(SG_ENOTFOUND, "namespace is not registered");
    const uint32_t id = it->second;
    if (int rc = drain(e)) return rc;
    e->ns_conn[id] = connected;
    // every loaded flow of the namespace (the metric state lives on the device: read, patch, write back)
    bool any = false;
    for (auto& f : e->cflows) any = any || ns_index(e, f.flow_id) == id;
    if (any) {
        std::vector<CFlow> cur(e->cflows.size());
        HIPCHK(hipMemcpy(cur.data(), e->d_cflow, cur.size() * sizeof(CFlow), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < cur.size(); ++i)
            if (ns_index(e, cur[i].flow_id) == id) { cur[i].connected = connected; e->cflows[i].connected = connected; }
        HIPCHK(hipMemcpy(e->d_cflow, cur.data(), cur.size() * sizeof(CFlow), hipMemcpyHostToDevice));
    }
    any = false;
    for (auto& f : e->pflows) any = any || ns_index(e, f.flow_id) == id;
    if (any) {
        std::vector<PFlow> cur(e->pflows.size());
        HIPCHK(hipMemcpy(cur.data(), e->d_pflow, cur.size() * sizeof(PFlow), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < cur.size(); ++i)
            if (ns_index(e, cur[i].flow_id) == id) { cur[i].connected = connected; e->pflows[i].connected = connected; }
        HIPCHK(hipMemcpy(e->d_pflow, cur.data(), cur.size() * sizeof(PFlow), hipMemcpyHostToDevice));
    }
    return SG_OK;
}

int sg_cluster_namespace_qps(sg_engine* e, const char* ns, int64_t now_ms, double* current_qps,
                             double* max_allowed_qps) {
    if (!e || !ns) return fail(SG_EINVAL, "null argument");
    auto it = e->ns_of.find(ns);
    if (it == e->ns_of.end()) return fail(SG_ENOTFOUND, "namespace is not registered");
    if (now_ms < 0) return fail(SG_EINVAL, "negative time");
    const uint32_t id = it->second;
    if (int rc = drain(e)) return rc;
    int64_t sum = 0;
    if (e->d_nslim) {
        NsLimiter l;
        HIPCHK(hipMemcpy(&l, e->d_nslim + id, sizeof(l), hipMemcpyDeviceToHost));
        // LeapArray.values(now) after currentWindow(now): the slot of now counts only with now's own window
        const int cur = (int)((now_ms / NS_WLEN) % NS_BUCKETS);
        const int64_t wsn = now_ms - now_ms % NS_WLEN;
        for (int k = 0; k < NS_BUCKETS; ++k) {
            if (l.ws[k] < 0 || now_ms - l.ws[k] > NS_INTERVAL) continue;
            if (k == cur && l.ws[k] < wsn) continue;
            sum += l.cnt[k];
        }
    }
    if (current_qps) *current_qps = (double)sum / (NS_INTERVAL / 1000.0);
    if (max_allowed_qps) *max_allowed_qps = e->ns_limit[id];
    return SG_OK;
}

// ---- cluster metrics (cmetrics.hip): ClusterMetricNodeGenerator over every flowId, a read-back
static void cm_free_flows(sg_engine* e) {
    dfree(e->d_cm_rows); dfree(e->d_cm_mask); dfree(e->d_cm_bounds); dfree(e->d_cm_nch); dfree(e->d_cm_coff);
    e->cm_flow_cap = 0;
}
static void cm_free_cands(sg_engine* e) {
    dfree(e->d_cm_k0); dfree(e->d_cm_v0); dfree(e->d_cm_k1); dfree(e->d_cm_v1); dfree(e->d_cm_hist); dfree(e->d_cm_part);
    dfree(e->d_cm_sum); dfree(e->d_cm_key); dfree(e->d_cm_psum); dfree(e->d_cm_pkey);
    e->cm_cand_cap = e->cm_chunk_cap = 0;
}
// The scratch of a call over ncf + npf flows and a value table of `slots` slots (0: no table).  A slot is a
// candidate only if it is claimed, and the capacity policy keeps the claimed slots at half of the table at most
// (pvtab.h); the scan checks the bound all the same.
static int cm_ensure(sg_engine* e, uint64_t nflows, uint64_t npf, uint64_t slots) {
    if (!e->d_cm_cnt) HIPCHK(hipMalloc(&e->d_cm_cnt, 8));
    for (auto& v : e->cm_ev)
        if (!v) HIPCHK(hipEventCreate(&v));
    if (nflows > e->cm_flow_cap) {
        cm_free_flows(e);
        const uint64_t c = std::max<uint64_t>(nflows, 1u << 10);
        HIPCHK(hipMalloc(&e->d_cm_rows, c * sizeof(sg_cluster_metric)));
        HIPCHK(hipMalloc(&e->d_cm_mask, c * 4));
        HIPCHK(hipMalloc(&e->d_cm_bounds, (c + 2) * 4));
        HIPCHK(hipMalloc(&e->d_cm_nch, (c + 2) * 4));
        HIPCHK(hipMalloc(&e->d_cm_coff, (c + 2) * 4));
        e->cm_flow_cap = c;
    }
    const uint64_t cands = slots / 2 + 1;
    const uint64_t chunks = cands / cm_chunk() + e->cm_flow_cap + 1;
    if (slots && (cands > e->cm_cand_cap || chunks > e->cm_chunk_cap)) {
        cm_free_cands(e);
        const uint64_t nblocks = (cands + radix_tile() - 1) / radix_tile();
        HIPCHK(hipMalloc(&e->d_cm_k0, cands * 4));
        HIPCHK(hipMalloc(&e->d_cm_v0, cands * 4));
        HIPCHK(hipMalloc(&e->d_cm_k1, cands * 4));
        HIPCHK(hipMalloc(&e->d_cm_v1, cands * 4));
        HIPCHK(hipMalloc(&e->d_cm_sum, cands * 8));
        HIPCHK(hipMalloc(&e->d_cm_key, cands * 8));
        HIPCHK(hipMalloc(&e->d_cm_hist, nblocks * 256 * 4));
        HIPCHK(hipMalloc(&e->d_cm_part, (nblocks + e->cm_flow_cap + 1024) * 4));  // (a scan's partials: one a tile)
        HIPCHK(hipMalloc(&e->d_cm_psum, chunks * SG_CLUSTER_TOP_MAX * 8));
        HIPCHK(hipMalloc(&e->d_cm_pkey, chunks * SG_CLUSTER_TOP_MAX * 8));
        e->cm_cand_cap = cands;
        e->cm_chunk_cap = chunks;
    }
    (void)npf;
    return SG_OK;
}

int sg_cluster_metrics(sg_engine* e, const char* ns, int64_t now_ms, uint32_t top_n, sg_cluster_metric* out,
                       uint64_t cap, uint64_t* n) {
    if (!e || !n || (cap && !out)) return fail(SG_EINVAL, "null argument");
    if (top_n < 1 || top_n > SG_CLUSTER_TOP_MAX) return fail(SG_EINVAL, "top_n must lie in 1..SG_CLUSTER_TOP_MAX");
    if (now_ms < 0) return fail(SG_EINVAL, "negative time");
    bool all = !ns || !ns[0];
    uint32_t ns_id = 0;
    if (!all) {
        auto it = e->ns_of.find(ns);
        if (it == e->ns_of.end()) return fail(SG_ENOTFOUND, "namespace is not registered");
        ns_id = it->second;
    }
    HIPCHK(hipSetDevice(e->device));
    if (int rc = drain(e)) return rc;
    const auto t_begin = std::chrono::steady_clock::now();
    const uint32_t ncf = (uint32_t)e->cflows.size(), npf = (uint32_t)e->pflows.size();
    for (double& v : e->cm_last) v = 0;
    e->cm_last[2] = cm_chunk();
    *n = 0;
    if (!ncf && !npf) return SG_OK;
    const uint64_t slots = npf && e->d_pvtab ? (uint64_t)e->pv_mask + 1 : 0;
    if (int rc = cm_ensure(e, (uint64_t)ncf + npf, npf, slots)) return rc;
    hipStream_t st = e->stream;
    sg_cluster_metric* prows = e->d_cm_rows + ncf;
    HIPCHK(hipEventRecord(e->cm_ev[0], st));
    HIPCHK(launch_cm_rows(e->d_cflow, ncf, e->d_cbkt, e->d_pflow, npf, now_ms, e->d_cm_mask, e->d_cm_rows, prows, st));
    HIPCHK(hipEventRecord(e->cm_ev[1], st));
    uint32_t ncand = 0;
    if (slots) {
        HIPCHK(launch_cm_scan(e->d_pvtab, slots, e->d_pflow, npf, e->d_cm_mask, e->d_cm_k0, e->d_cm_v0, e->d_cm_sum,
                              e->d_cm_key, (uint32_t)e->cm_cand_cap, e->d_cm_cnt, st));
        HIPCHK(hipMemcpyAsync(&ncand, e->d_cm_cnt, 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipEventRecord(e->cm_ev[2], st));
    HIPCHK(hipStreamSynchronize(st));
    if (ncand > e->cm_cand_cap) return fail(SG_EDEVICE, "cluster metrics: more candidates than half of the value table");
    for (int k = 3; k < 6; ++k) HIPCHK(hipEventRecord(e->cm_ev[k], st));  // (a call without candidates: empty stages)
    if (ncand) {
        uint32_t *kin = e->d_cm_k0, *vin = e->d_cm_v0, *kout = e->d_cm_k1, *vout = e->d_cm_v1;
        int bits = 1;
        while (bits < 32 && (1ull << bits) < npf) ++bits;  // keys 0 .. npf - 1
        const int passes = (bits + 7) / 8;
        const uint32_t nblocks = (uint32_t)(((uint64_t)ncand + radix_tile() - 1) / radix_tile());
        for (int p = 0; p < passes; ++p) {
            HIPCHK(launch_radix_hist(kin, ncand, p * 8, e->d_cm_hist, nblocks, st));
            HIPCHK(launch_scan(e->d_cm_hist, e->d_cm_hist, (uint64_t)nblocks * 256, e->d_cm_part, nullptr, st));
            HIPCHK(launch_radix_scatter(kin, vin, ncand, p * 8, e->d_cm_hist, nblocks, kout, vout, nullptr, st));
            std::swap(kin, kout);
            std::swap(vin, vout);
        }
        HIPCHK(launch_cm_select(kin, vin, ncand, e->d_pflow, npf, e->d_cm_sum, e->d_cm_key, top_n, e->d_cm_bounds,
                                e->d_cm_nch, e->d_cm_coff, e->d_cm_part, e->d_cm_psum, e->d_cm_pkey, prows,
                                e->cm_ev + 3, st));
        HIPCHK(hipEventRecord(e->cm_ev[5], st));
    }
    std::vector<sg_cluster_metric> rows((size_t)ncf + npf);
    uint32_t nchunks = 0;
    if (ncand) HIPCHK(hipMemcpyAsync(&nchunks, e->d_cm_coff + npf, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(rows.data(), e->d_cm_rows, rows.size() * sizeof(sg_cluster_metric), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // the rows in the defined order: flow rules by flowId, then param rules by flowId, of the namespace asked for
    auto emit = [&](const std::unordered_map<int64_t, uint32_t>& idx, const std::unordered_map<int64_t, std::string>& res,
                    uint32_t base) {
        std::vector<int64_t> ids;
        for (auto& kv : idx)
            if (all || ns_index(e, kv.first) == ns_id) ids.push_back(kv.first);
        std::sort(ids.begin(), ids.end());
        for (int64_t fid : ids) {
            sg_cluster_metric r = rows[base + idx.at(fid)];
            auto rn = res.find(fid);
            if (rn != res.end()) {
                auto id = e->ids.find(rn->second);
                if (id != e->ids.end()) r.res_id = id->second;
            }
            if (*n < cap) out[*n] = r;
            ++*n;
        }
    };
    emit(e->cmap, e->cres, 0);
    emit(e->pmap, e->pres, ncf);
    float ms[5] = {0, 0, 0, 0, 0};
    for (int k = 0; k < 5; ++k)
        if (hipEventElapsedTime(&ms[k], e->cm_ev[k], e->cm_ev[k + 1]) != hipSuccess) ms[k] = 0;
    (void)hipGetLastError();
    e->cm_last[0] = ncand;
    e->cm_last[1] = nchunks;
    e->cm_last[3] = (double)slots;
    for (int k = 0; k < 5; ++k) e->cm_last[4 + k] = ms[k];
    e->cm_last[9] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    return SG_OK;
}

// diagnostics export: the last sg_cluster_metrics call: [0] candidates (claimed slots with a sum > 0), [1] chunks the
// select stage cut them into, [2] candidates a chunk holds at most, [3] value table slots scanned, then the device
// times in ms (HIP events) of [4] the rows and masks, [5] the scan, [6] the grouping (sort, bounds, chunk table),
// [7] the select, [8] the merge, and [9] the call's wall time in ms.  Returns the values written.
extern "C" int sgx_cluster_metrics_last(sg_engine* e, double* out, int cap) {
    if (!e || !out) return 0;
    int k = 0;
    for (; k < 10 && k < cap; ++k) out[k] = e->cm_last[k];
    return k;
}

int sg_param_key_value(sg_engine* e, uint64_t key, char* class_type, size_t class_cap, char* value, size_t value_cap) {
    if (!e || !class_type || !value) return fail(SG_EINVAL, "null argument");
    const uint32_t tag = (uint32_t)(key >> 60);
    const uint64_t v = key & pk::KEY_MASK;
    const char* ct = nullptr;
    std::string text;
    char buf[64];
    auto num = [&](const char* fmt, auto x) { std::snprintf(buf, sizeof(buf), fmt, x); text = buf; };
    std::string canon;
    const bool maybe_entry = tag == 1 || tag == 4 || (tag == 3 && (v & pk::LONG_HASHED));
    const bool found = maybe_entry && e->pkeys.value_of(key, canon);
    switch (tag) {
    case 1:
        if (!found) return fail(SG_ENOTFOUND, "no dictionary entry owns this key");
        ct = "java.lang.String";
        text = canon.substr(1);
        break;
    case 2: ct = "int"; num("%d", (int)(int32_t)(uint32_t)v); break;
    case 3: {
        ct = "long";
        long long x;
        if (found && canon.size() == 9) std::memcpy(&x, canon.data() + 1, 8);
        else x = (long long)(v << 4) >> 4;  // the 60-bit two's complement value
        num("%lld", x);
        break;
    }
    case 4: {
        if (!found || canon.size() != 9) return fail(SG_ENOTFOUND, "no dictionary entry owns this key");
        ct = "double";
        double d;
        std::memcpy(&d, canon.data() + 1, 8);
        num("%.17g", d);
        break;
    }
    case 5: {
        ct = "float";
        const uint32_t u = (uint32_t)v;
        float f;
        std::memcpy(&f, &u, 4);
        num("%.9g", (double)f);
        break;
    }
    case 6: ct = "byte"; num("%d", (int)(int8_t)(uint8_t)v); break;
    case 7: ct = "short"; num("%d", (int)(int16_t)(uint16_t)v); break;
    case 8: ct = "boolean"; text = v ? "true" : "false"; break;
    case 9: ct = "char"; text.assign(1, (char)(unsigned char)v); break;
    default: return fail(SG_ENOTFOUND, "not a parameter value key");
    }
    if (std::strlen(ct) + 1 > class_cap || text.size() + 1 > value_cap) return fail(SG_EINVAL, "buffer too small");
    std::memcpy(class_type, ct, std::strlen(ct) + 1);
    std::memcpy(value, text.c_str(), text.size() + 1);
    return (int)text.size();
}

// Batched DefaultTokenService.requestToken (see cluster.hip for the device steps), in two parts so that the decide
// stage can issue a batch's own requests (embedded token server): tok_ensure makes room for n requests and the
// tables a call reads (tab / mask: its flowId table), tok_device decides the n requests already in e->d_treq into
// e->d_tres.
static int tok_ensure(sg_engine* e, uint64_t n, CSlot*& tab, uint32_t& mask) {
    int rc = ensure_batch(e, n);  // radix-sort scratch
    if (rc) return rc;
    if (n > e->tcap) {
        dfree(e->d_treq); dfree(e->d_tres); dfree(e->d_tfidx);
        uint64_t c = std::max<uint64_t>(n, 1u << 16);
        HIPCHK(hipMalloc(&e->d_treq, c * sizeof(sg_token_req)));
        HIPCHK(hipMalloc(&e->d_tres, c * sizeof(sg_token_result)));
        HIPCHK(hipMalloc(&e->d_tfidx, c * 4));
        e->tcap = c;
    }
    if (int rc2 = ensure_ns(e)) return rc2;
    if (!tab) {  // no cluster rule of the call's kind loaded yet: an empty table
        CSlot t[16];
        for (auto& x : t) { x.key = 0; x.idx = 0xFFFFFFFFu; x.pad = 0; }
        HIPCHK(hipMalloc(&tab, sizeof(t)));
        HIPCHK(hipMemcpy(tab, t, sizeof(t), hipMemcpyHostToDevice));
        mask = 15;
    }
    return SG_OK;
}
// The requests are in time order and their tables exist (tok_ensure).  scratch: the batch slot whose arrays the call
// overwrites (tok_limit_sort).  The classification's flag is read back on the host, so every earlier kernel of the
// engine stream is done when this returns; the flows' kernels may still be running.
static int tok_device(sg_engine* e, sg_engine::BatchSlot& scratch, uint64_t n) {
    hipStream_t st = e->stream;
    const uint32_t nflows = (uint32_t)e->cflows.size();
    HIPCHK(hipMemsetAsync(e->d_small + SM_FLAGS, 0, 4, st));
    const uint32_t nns = (uint32_t)e->ns_names.size();
    const bool grouped = nns > 1 || e->tok_ns;  // several limiters: the namespace-grouped limiter step
    HIPCHK(launch_tok_classify(e->d_treq, n, e->d_ctab, e->ctab_mask, e->d_tfidx, e->d_tres, e->d_small + SM_FLAGS,
                               grouped ? scratch.d_k0 : nullptr, grouped ? scratch.d_v0 : nullptr, nns, st));
    uint32_t flags = 0;
    HIPCHK(hipMemcpyAsync(&flags, e->d_small + SM_FLAGS, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (flags & 1) return fail(SG_EINVAL, "token requests must be ordered by ts (the replay clock)");
    uint32_t *kin, *vin;
    if (int rc = tok_limit_sort(e, scratch, n, nflows, grouped, false, kin, vin)) return rc;
    if (nflows) {
        if (nflows + 1 > e->tbounds_cap) HIPCHK(grow(e->d_tbounds, e->tbounds_cap, nflows + 1, 1u << 12));
        // (the other decide streams are idle: every earlier batch is decided, see above)
        HIPCHK(launch_tok_flow(kin, vin, n, e->d_treq, e->d_cflow, nflows, e->d_cbkt, e->cfg.cluster_exceed_count,
                               e->cfg.cluster_max_occupy_ratio, e->d_tres, e->d_tbounds, e->tok_light, e->tok_wide, st,
                               e->bin_stream[0], e->fork, e->join[0]));
    }
    return SG_OK;
}
int sg_cluster_request_tokens(sg_engine* e, const sg_token_req* reqs, uint64_t n, sg_token_result* out) {
    if (!e || (n && (!reqs || !out))) return fail(SG_EINVAL, "null argument");
    if (!n) return SG_OK;
    if (n > 0x7FFFFFFFull) return fail(SG_EINVAL, "too many token requests in one call");
    if (int rc = drain(e)) return rc;
    hipStream_t st = e->stream;
    if (int rc = tok_ensure(e, n, e->d_ctab, e->ctab_mask)) return rc;
    // requests and results may be host or device memory (dist.request_tokens keeps them in HBM under RCCL)
    HIPCHK(hipMemcpyAsync(e->d_treq, reqs, n * sizeof(sg_token_req), hipMemcpyDefault, st));
    if (int rc = tok_device(e, e->slot[e->cur], n)) return rc;  // (drained: no batch is in either slot)
    HIPCHK(hipMemcpyAsync(out, e->d_tres, n * sizeof(sg_token_result), hipMemcpyDefault, st));
    HIPCHK(hipStreamSynchronize(st));
    return SG_OK;
}

// Embedded token server, the decide stage's step for batch slot k (decide_enqueue, after the chain grants): the
// ENTRYs that ask for a token are compacted in submission order into e->d_treq (kernels.hip k_emb_count /
// k_emb_scatter, the test in embedded.h), one token call decides them, and k_emb_answers leaves each answer's side
// word at the ENTRY's sorted position (e->d_emb_side, cleared first) and counts the answers (BS_EMB_ANS ..; BS_EMB_REQ
// the requests).  The token call's scratch is the other slot's arrays: its batch is decided (submit_impl hands a batch
// with XF_EMB events off before the next group stage is enqueued), and the call runs on the engine stream behind it.
// The host waits twice (the request count, the classification's flag): such a batch overlaps with no neighbour.
static int embedded_tokens(sg_engine* e, int k, uint32_t* nreq_out) {
    auto& B = e->slot[k];
    const auto& G = B.g;
    hipStream_t st = e->stream;
    const uint64_t n = G.n;
    if (e->cap_n > e->emb_cap) {
        HIPCHK(hipStreamSynchronize(st));
        dfree(e->d_emb_side); dfree(e->d_emb_idx); dfree(e->d_emb_cnt); dfree(e->d_emb_part);
        const uint64_t c = e->cap_n, nt = c / 1024 + 2;
        HIPCHK(hipMalloc(&e->d_emb_side, c * 4));
        HIPCHK(hipMalloc(&e->d_emb_idx, c * 4));
        HIPCHK(hipMalloc(&e->d_emb_cnt, nt * 4));
        HIPCHK(hipMalloc(&e->d_emb_part, (nt / 4096 + 2) * 4));
        e->emb_cap = c;
    }
    uint32_t* bs = B.d_bsmall;
    for (auto& x : e->emb_t)
        if (!x) HIPCHK(hipEventCreate(&x));
    e->emb_timed = false;
    HIPCHK(hipEventRecord(e->emb_t[0], st));
    HIPCHK(launch_emb_count(G.dev_ev, G.dev_ext, n, e->cfg.max_resources, SG_MAX_CONTEXTS, e->d_prog, e->d_info, dev_auth(e),
                            dev_auth_ids(e), e->cfg.switch_on, e->d_emb_cnt, e->d_emb_part, bs + BS_EMB_REQ, st));
    uint32_t nreq = 0;
    HIPCHK(hipMemcpyAsync(&nreq, bs + BS_EMB_REQ, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *nreq_out = nreq;
    if (!nreq) return SG_OK;
    if (int rc = tok_ensure(e, nreq, e->d_ctab, e->ctab_mask)) return rc;  // (nreq <= n <= cap_n: the batch arrays stay)
    HIPCHK(launch_emb_scatter(G.dev_ev, G.dev_ext, n, e->cfg.max_resources, SG_MAX_CONTEXTS, e->d_prog, e->d_info,
                              dev_auth(e), dev_auth_ids(e), e->cfg.switch_on, e->d_emb_cnt, e->d_emb_flow, nreq, e->d_treq,
                              e->d_emb_idx, st));
    HIPCHK(hipEventRecord(e->emb_t[1], st));
    if (int rc = tok_device(e, e->slot[k ^ 1], nreq)) return rc;
    // the call's last kernels are still in flight: the next group stage into the borrowed slot waits for them
    if (!e->emb_ev[k ^ 1]) HIPCHK(hipEventCreateWithFlags(&e->emb_ev[k ^ 1], hipEventDisableTiming));
    HIPCHK(hipEventRecord(e->emb_ev[k ^ 1], st));
    e->slot[k ^ 1].lent = e->emb_ev[k ^ 1];
    HIPCHK(hipEventRecord(e->emb_t[2], st));
    HIPCHK(hipMemsetAsync(e->d_emb_side, 0, n * 4, st));
    HIPCHK(launch_emb_answers(e->d_tres, e->d_emb_idx, nreq, B.radix ? B.d_posof : nullptr, B.d_flag, B.d_pos, B.nhot, n,
                              e->d_emb_side, bs + BS_EMB_ANS, st));
    HIPCHK(hipEventRecord(e->emb_t[3], st));
    e->emb_timed = true;
    return SG_OK;
}

// diagnostics export, for synchronous batches only (one set of events an engine: with a second embedded batch decided
// before the first is collected the values are stale or 0): device times of the embedded steps in the last collected
// batch that made requests, ms: [0] the
// extraction (both kernels, the scan and the host's wait for the count between them), [1] the token call, [2] the
// side array's clear and the answers' scatter.  Returns the values written.
extern "C" int sgx_embedded_ms(sg_engine* e, double* out, int cap) {
    if (!e || !out) return 0;
    drain_hold(e);
    int k = 0;
    for (; k < 3 && k < cap; ++k) out[k] = e->emb_ms[k];
    return k;
}

// ClusterStateManager's server state (embedded mode, embedded.h): on, the flow rules' cluster rules are decided on the
// decision path by this engine's own token server; off (the default), as in a process without a TokenService.  The
// programs are compiled again; node, breaker and token state stay.  Switching on over a cluster rule outside the
// supported shape is refused (SG_ENOTSUP, sg_last_error names the rule) and changes nothing.
int sg_cluster_embedded(sg_engine* e, int32_t on) {
    if (!e) return fail(SG_EINVAL, "null argument");
    HIPCHK(hipSetDevice(e->device));
    if (int rc = drain(e)) return rc;
    const bool want = on != 0;
    if (want == e->emb_on) return SG_OK;
    if (want)
        if (int rc = check_emb_shape(e->flows, e->res_flow, e->res_par)) return rc;
    e->emb_on = want;
    const int rc = upload_rules(e, false, false, false);
    if (rc) {
        e->emb_on = !want;
        return rc;
    }
    return SG_OK;
}
// diagnostics export: the embedded token server's part of the last collected batch: [0] requests issued, [1..7]
// answers OK, BLOCKED, SHOULD_WAIT, TOO_MANY_REQUEST, BAD_REQUEST, FAIL, NO_RULE_EXISTS, [8] words written ahead of the
// cooperative owners, [9] segments of embedded resources in cooperative bins, [10] in lane bins, [11] in the late
// lane pass (always 0: no fallback rules).  Returns the values written.
extern "C" int sgx_embedded_last(sg_engine* e, unsigned long long* out, int cap) {
    if (!e || !out) return 0;
    drain_hold(e);
    int k = 0;
    for (; k < EMB_LAST_WORDS && k < cap; ++k) out[k] = e->emb_last[k];
    return k;
}

// Room in the value table for a call of V listed values, before any kernel of the call runs (pvtab.h; in the
// spirit of k_pm_grow).  While claimed_ub + V fits half the table this is one comparison.  Otherwise the live
// slots are counted on the device, pv_plan picks the capacity, and k_pv_rehash moves them into a fresh table
// (a rehash that keeps the capacity keeps the old table as the next one's target, so a steady stream allocates
// nothing; a resize frees it; either way two tables exist during the move).  A refusal (SG_ENOMEM: the maximum
// capacity cannot hold the live values and V at half load, or the second table cannot be allocated) leaves the
// table, the limiter and the flows' windows as they were.  Runs on the engine stream after drain.
static int pv_make_room(sg_engine* e, uint64_t V) {
    if (!e->d_pvtab || e->pflows.empty()) return SG_OK;
    const uint64_t cap = (uint64_t)e->pv_mask + 1;
    if (pv_has_room(e->pv_claimed, V, cap)) return SG_OK;
    hipStream_t st = e->stream;
    const uint32_t nflows = (uint32_t)e->pflows.size();
    if (!e->d_pvcnt) HIPCHK(hipMalloc(&e->d_pvcnt, 8));
    for (auto& v : e->pv_ev)
        if (!v) HIPCHK(hipEventCreate(&v));
    uint32_t cnt[2] = {0, 0};
    HIPCHK(hipEventRecord(e->pv_ev[0], st));
    HIPCHK(launch_pv_rehash(e->d_pvtab, cap, e->d_pflow, nflows, nullptr, 0, e->d_pvcnt, st));
    HIPCHK(hipEventRecord(e->pv_ev[1], st));
    HIPCHK(hipMemcpyAsync(cnt, e->d_pvcnt, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const uint64_t live = cnt[0];
    const uint64_t ncap = pv_plan(live, V, 1ull << e->pv_log2, 1ull << e->pv_max_log2);
    if (!ncap)
        return fail(SG_ENOMEM, "cluster param value table: the live values and this call's do not fit half of the "
                               "maximum capacity (SG_PV_MAX_LOG2)");
    PVal* nt = nullptr;
    if (e->d_pvspare && e->pv_spare_cap == ncap) {
        nt = e->d_pvspare;
        e->d_pvspare = nullptr;
    } else {
        dfree(e->d_pvspare);
        if (hipMalloc(&nt, ncap * sizeof(PVal)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(SG_ENOMEM, "cluster param value table: no device memory for the larger table");
        }
    }
    hipError_t rc = hipEventRecord(e->pv_ev[2], st);
    if (rc == hipSuccess) rc = hipMemsetAsync(nt, 0xFF, ncap * sizeof(PVal), st);  // every flow PV_EMPTY
    if (rc == hipSuccess) rc = launch_pv_rehash(e->d_pvtab, cap, e->d_pflow, nflows, nt, (uint32_t)(ncap - 1), e->d_pvcnt, st);
    if (rc == hipSuccess) rc = hipEventRecord(e->pv_ev[3], st);
    if (rc == hipSuccess) rc = hipMemcpyAsync(cnt, e->d_pvcnt, 8, hipMemcpyDeviceToHost, st);
    if (rc == hipSuccess) rc = hipStreamSynchronize(st);
    if (rc != hipSuccess || cnt[1] || cnt[0] != live) {  // (the old table is untouched: it stays)
        (void)hipFree(nt);
        if (rc != hipSuccess) return fail(SG_EDEVICE, std::string("cluster param value table rehash: ") + hipGetErrorString(rc));
        return fail(SG_EDEVICE, "cluster param value table rehash lost a slot");
    }
    float ms0 = 0, ms1 = 0;
    if (hipEventElapsedTime(&ms0, e->pv_ev[0], e->pv_ev[1]) != hipSuccess) ms0 = 0;
    if (hipEventElapsedTime(&ms1, e->pv_ev[2], e->pv_ev[3]) != hipSuccess) ms1 = 0;
    (void)hipGetLastError();
    if (ncap == cap) { e->d_pvspare = e->d_pvtab; e->pv_spare_cap = cap; }
    else (void)hipFree(e->d_pvtab);
    e->d_pvtab = nt;
    e->pv_mask = (uint32_t)(ncap - 1);
    e->pv_claimed = e->pv_live = live;
    e->pv_last_us = (uint64_t)(((double)ms0 + (double)ms1) * 1000.0);
    ++e->pv_rehashes;
    if (ncap != cap) ++e->pv_resizes;
    return SG_OK;
}

// Batched DefaultTokenService.requestParamToken: the flow path's classify and namespace limiter steps on a
// derived sg_token_req view (k_ptok_prep; n_values == 0 -> acquire 0 -> BAD_REQUEST), then per param flow either
// the value-parallel owner (ptok.h, launch_ptok_vp) or k_ptok_flow (k_ptok_elig decides which, on the device).
// reqs, values and out may each be host or device memory: everything is copied into the engine's buffers first.
int sg_cluster_request_param_tokens(sg_engine* e, const sg_param_token_req* reqs, uint64_t n, const uint64_t* values,
                                    uint64_t n_values, sg_token_result* out) {
    if (!e || (n && (!reqs || !out)) || (n_values && !values)) return fail(SG_EINVAL, "null argument");
    if (!n) return SG_OK;
    if (n > 0x7FFFFFFFull) return fail(SG_EINVAL, "too many token requests in one call");
    if (int rc = drain(e)) return rc;
    hipStream_t st = e->stream;
    if (int rc = tok_ensure(e, n, e->d_pftab, e->pftab_mask)) return rc;
    if (n > e->pcap) HIPCHK(grow(e->d_preq, e->pcap, n, 1u << 16));
    if (n_values > e->pvcap) HIPCHK(grow(e->d_pvals, e->pvcap, n_values, 1u << 16));
    if (!e->d_ptst) {
        HIPCHK(hipMalloc(&e->d_ptst, 8 * sizeof(unsigned long long)));
        HIPCHK(hipMemset(e->d_ptst, 0, 8 * sizeof(unsigned long long)));
    }
    const uint32_t nflows = (uint32_t)e->pflows.size();
    if (nflows > e->ptserial_cap) HIPCHK(grow(e->d_ptserial, e->ptserial_cap, nflows, 1u << 12));
    uint64_t dcap = 1u << 12;  // the dedup table: a power of two of at least twice the call's requests
    while (dcap < 2 * n) dcap <<= 1;
    if (dcap > e->ptdedup_cap) HIPCHK(grow(e->d_ptdedup, e->ptdedup_cap, dcap, 0));
    auto& X = e->slot[e->cur];  // the call's scratch (tok_limit_sort; drained: no batch is in either slot)
    uint32_t* d_flags = e->d_small + SM_FLAGS;
    // the request view, the range check and the listed values, on the device, then the classify step (it writes
    // the call's own arrays only); (range flag, listed) and the order flag are read once, before anything moves
    HIPCHK(hipMemcpyAsync(e->d_preq, reqs, n * sizeof(sg_param_token_req), hipMemcpyDefault, st));
    if (n_values) HIPCHK(hipMemcpyAsync(e->d_pvals, values, n_values * sizeof(uint64_t), hipMemcpyDefault, st));
    HIPCHK(hipMemsetAsync(e->d_ptst, 0, 2 * sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(d_flags, 0, 4, st));
    HIPCHK(launch_ptok_prep(e->d_preq, n, n_values, e->d_treq, e->d_ptst, st));
    const uint32_t nns = (uint32_t)e->ns_names.size();
    const bool grouped = nns > 1 || e->tok_ns;
    HIPCHK(launch_tok_classify(e->d_treq, n, e->d_pftab, e->pftab_mask, e->d_tfidx, e->d_tres, d_flags,
                               grouped ? X.d_k0 : nullptr, grouped ? X.d_v0 : nullptr, nns, st));
    unsigned long long pst[2] = {0, 0};
    uint32_t flags = 0;
    HIPCHK(hipMemcpyAsync(pst, e->d_ptst, sizeof(pst), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&flags, d_flags, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (pst[1] & 1) return fail(SG_EINVAL, "param token request values out of range");
    if (flags & 1) return fail(SG_EINVAL, "token requests must be ordered by ts (the replay clock)");
    const uint64_t listed = pst[0];  // the call claims at most that many value slots
    if (int rc2 = pv_make_room(e, listed)) return rc2;  // before the limiter or any window moves
    // A small call spread thinly over many flows (fewer than SG_PTOK_MIN requests and fewer than PTOK_PER_FLOW per
    // loaded flow) keeps the one-wave limiter and k_ptok_flow for every flow: fewer launches than the parallel
    // limiter and the value-parallel owner need, and a lane's walk is short there (measured).
    constexpr uint64_t PTOK_PER_FLOW = 8;
    const bool small = n < e->ptok_min && n < PTOK_PER_FLOW * nflows;
    const bool lane_only = !e->ptok_vp || small;
    uint32_t *kin, *vin;
    if (int rc2 = tok_limit_sort(e, X, n, nflows, grouped, small, kin, vin)) return rc2;
    if (nflows) {
        e->pv_claimed += listed;
        if (lane_only)
            HIPCHK(launch_ptok_flow(kin, vin, n, e->d_preq, e->d_pvals, e->d_pflow, nflows, e->d_phot, e->d_pvtab,
                                    e->pv_mask, e->d_tres, d_flags, nullptr, e->d_ptst + 2, st));
        else {
            // who decides which flow; the two owners then work on disjoint flows (the limiter's scratch arrays are free)
            HIPCHK(launch_ptok_elig(kin, vin, n, e->d_preq, e->d_pflow, nflows, e->d_ptserial, st));
            HIPCHK(launch_ptok_flow(kin, vin, n, e->d_preq, e->d_pvals, e->d_pflow, nflows, e->d_phot, e->d_pvtab,
                                    e->pv_mask, e->d_tres, d_flags, e->d_ptserial, nullptr, st));
            HIPCHK(launch_ptok_vp(kin, vin, n, e->d_preq, e->d_pvals, e->d_pflow, nflows, e->d_phot, e->d_pvtab, e->pv_mask,
                                  e->d_ptserial, e->d_ptdedup, (uint32_t)(dcap - 1), X.d_flag, X.d_pos, X.d_order,
                                  X.d_prev, X.d_dec, X.d_posof, reinterpret_cast<int64_t*>(X.d_cand),
                                  reinterpret_cast<int32_t*>(X.d_out), X.d_hist, X.d_part, radix_tile(), e->d_tres,
                                  d_flags, e->d_ptst + 2, st));
        }
    }
    HIPCHK(hipMemcpyAsync(out, e->d_tres, n * sizeof(sg_token_result), hipMemcpyDefault, st));
    HIPCHK(hipMemcpyAsync(&flags, d_flags, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (flags & 2) return fail(SG_ENOMEM, "cluster param value table is full");
    return SG_OK;
}

} // extern "C"
