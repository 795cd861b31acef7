// dev_types.h -- device-resident state of the MI355X decision engine.
//
// HBM layout (one engine = one GPU = one shard of resources):
//   Bkt     sec[R][2]     rollingCounterInSecond buckets (core/node/StatisticNode.java:102)
//   Bkt     minb[R][60]   rollingCounterInMinute buckets (core/node/StatisticNode.java:111)
//   NodeInfo info[R]      curThreadNum, chain/metric flags, exception running sum
//   Prog    prog[R]       compiled rule program: [param..., flow..., degrade...]
//   DRule   rules[]       compiled rule constants
//   RState  rstate[]      controller / breaker state (one per rule)
//   PMap    pmap[]        ParameterMetric's CacheMaps: one bounded LRU map per (param rule state) and per
//                         (resource, paramIdx) thread-count map, each a private region of
//   PBucket pbkt[]        the cuckoo bucket pool (keys + access stamps), PData pdat[] their values, and
//   uint64  pbm[]         the live-stamp rings (recency order, pmap.h)
//   uint8   ring[2^k]     status of every ENTRY by global event index (EXIT/TRACE references)
// All counters are int64 exactly as the Java LongAdders; RT sums are int64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sentinel_gpu.h"

namespace sg {

struct AuthDesc;  // authority.h

// one LeapArray bucket: MetricBucket (core/slots/statistic/data/MetricBucket.java:28-139)
struct Bkt {
    int64_t ws;      // window start; -1 = never created (WindowWrap absent)
    int64_t pass;
    int64_t block;
    int64_t exc;
    int64_t succ;
    int64_t rt;
    int64_t occ;
    int64_t minrt;
};
static_assert(sizeof(Bkt) == 64, "Bkt must be 64 B");

#define NO_KEY 0xFFFFFFFFFFFFFFFFull  // key-ring value of an ENTRY without an argument

enum : uint32_t {
    NI_CHAIN = 1u,       // CtSph chainMap holds this resource (and its ClusterNode exists)
    NI_REJECTED = 2u,    // lookProcessChain returned null once the cap was reached
    NI_PM = 4u,          // ParamFlowSlot.metricsMap has a ParameterMetric for it
    NI_TOUCHED = 32u,    // ClusterBuilderSlot created its ClusterNode (an ENTRY with a chain was processed);
                         // kept exact for resources in a STRATEGY_RELATE component (ClusterBuilderSlot.getClusterNode)
    NI_TM_SHIFT = 6u     // bit NI_TM_SHIFT + i: ParameterMetric has a thread-count map for paramIdx i (i < SG_MAX_ARGS)
};
__host__ __device__ inline uint32_t ni_tm(uint32_t idx) { return 1u << (NI_TM_SHIFT + idx); }

// sticky per-resource event marks (DevState.prio), set by the group stage: any mark sends the resource's
// segments to the per-lane kernel
enum : uint8_t {
    PM_PRIO = 1,         // a prioritized ENTRY was seen: the second window's borrow ring is live
    PM_LANE = 2,         // an event only k_lane implements was seen: a NullContext, an origin id >= 2^20 (not packable
                         // into the record's node tag); with SG_UBLK=0 also every pre-blocked ENTRY (PM_UBLK)
    PM_AUX = 4,          // an event carried an origin or a named context: the resource keeps its origin
                         // StatisticNodes / context DefaultNodes whatever its rules are.  Rules that read them
                         // (PX_ORIGIN / PX_CHAIN) decide on k_lane<16>; otherwise the segment decides on its usual
                         // owner and aux.hip updates the nodes from the committed verdicts afterwards
    PM_ARGL = 8,         // an event's argument was a Collection / array (per-element checks: not k_pq's; its maps
                         // are grown to full size)
    PM_XARGS = 16,       // an EXIT released thread counts with args of its own (sg_submit_ex)
    PM_UBLK = 32         // a pre-blocked ENTRY was seen: SG_F_BLOCKED_UPSTREAM, or an ENTRY its authority rule blocks.
                         // Its record carries RF_UBLK.  The cooperative owners (k_jac, k_fill) take such a segment
                         // (SEG_UBLK) with the pre-blocked ENTRYs as blocks whose words k_ublk_words writes; what they
                         // do not take -- short segments (k_lite is not taught the class), PF_PQ, PF_SERIAL, RELATE
                         // components, origin / CHAIN rules, prioritized or PM_LANE resources -- keeps the lane bins
};
// SEv.x of an ENTRY (and of an EXIT / TRACE that names no ENTRY of this batch) in an sg_submit_ex batch: the
// origin / context node tag of the event, origin id | context id << 20 (0: no origin, default context)
#define TAG_ORIGIN_BITS 20u
__host__ __device__ inline uint32_t tag_origin(uint32_t tag) { return tag & ((1u << TAG_ORIGIN_BITS) - 1); }
__host__ __device__ inline uint32_t tag_ctx(uint32_t tag) { return tag >> TAG_ORIGIN_BITS; }
// internal SEv.flags bits above the ABI's SG_F_*
#define RF_OWN_ARGS 0x80u  // EXIT of sg_submit_ex with its own args: its args[0] key is in the key ring at its index
#define RF_PBLK 0x40u      // ENTRY of an XF_MIX segment that a param rule blocked (param.hip k_pq pre pass): its dec[]
                           // word is final; the flow / degrade owner counts it as a block and evaluates nothing
#define RF_UBLK 0x20u      // ENTRY blocked before FlowSlot by SystemSlot (with SG_F_BLOCKED_UPSTREAM: status 6) or by its
                           // resource's authority rule (without: status 7), set at intake (a bit the ABI leaves unused
                           // and the intake masks off the caller's flags).  In a SEG_UBLK segment k_ublk_words, after the
                           // param pre pass (a param rule's block comes first and stands), writes its word and raises
                           // RF_PBLK on it: the owner's class.  A lane owner ignores the bit (lane_entry decides)

struct NodeInfo {
    int32_t thread;      // StatisticNode.curThreadNum
    uint32_t flags;      // NI_*
    int64_t exc_sum_sec; // second T for which exc_sum = sum of minute exceptions with ws in [T-59000, T]; -1 unknown
    int64_t exc_sum;
    int64_t last_fetch;  // StatisticNode.lastFetchTime (metrics snapshots)
};
static_assert(sizeof(NodeInfo) == 32, "NodeInfo must be 32 B");

// Prog.pflags: what the decide kernels need to know about a resource's rule program
enum : uint8_t {
    PF_EXC_COUNT = 1,   // has an EXCEPTION_COUNT breaker (minute exception running sum)
    PF_WARM = 2,        // has a WarmUp / WarmUpRateLimiter controller
    PF_PQ = 4,          // only QPS-grade param rules with a fixed paramIdx and maps of capacity <= PQ_MAX_CAP: the
                        // cooperative param owner (param.hip k_pq) decides it in batches it is enabled for
    PF_SERIAL = 8,      // outside the cooperative (Jacobi) kernels' limits: per-lane serial kernel only
    PF_RL = 16,         // has a RateLimiter / WarmUpRateLimiter controller
    PF_RT = 32,         // has an RT breaker
    PF_FROZEN = 64,     // every flow stage is a QPS DefaultController: saturated / cut stretches are pure
                        // reductions (decide.hip k_jac frozen stretch)
    PF_J16 = 128        // fits the 1024-lane kernel's shape: <= 2 flow, <= 2 degrade stages, no rate limiter
};

struct Prog {
    uint32_t rule_off;
    uint8_t n_param, n_flow, n_degrade, pflags;
    uint32_t tm_base;    // thread-count maps of this resource: DevState.tmid[tm_base + paramIdx] (NO_ID: none)
    uint16_t multi;      // PX_* bits
    uint16_t xf;         // XF_* bits
};
enum : uint16_t {
    XF_PTHREAD = 1,      // a THREAD-grade param rule is checked (k_pq resolves an EXIT's release against its ENTRY's
                         // check of the same tile by key: an EXIT with its own args (PM_XARGS) is k_lane's)
    XF_MIX = 2,          // param rules beside flow / degrade rules, cooperatively decided: k_pq's
                         // pre pass decides the QPS param checks per value first (nothing before ParamFlowSlot
                         // blocks), the Jacobi owner the flow / degrade chain with those verdicts as inputs, and
                         // k_pq's post pass the thread-count map from the final verdicts
    XF_PLITE = 4,        // XF_MIX with exactly one (checked) param rule: its short segments take k_lite<true>
    XF_PVPQ = 8,         // PF_PQ with one QPS rule (DefaultController or throttle) on paramIdx 0: its long segments'
                         // checks by pvalue.hip's passes, k_pq then folding the statistics only (SG_PV_PQ)
    XF_HEADT = 16,       // the only rule is one THREAD-grade DefaultController flow rule on the ClusterNode (DIRECT,
                         // limitApp default): its J16 / J4 segments take the event-driven head owner (head.hip)
    XF_HEADR = 32,       // ... one QPS RateLimiter (or WarmUpRateLimiter of count > 0) flow rule likewise
    XF_EMB = 64          // embedded token server (embedded.h): the resource's only flow rule is a cluster rule whose
                         // tokens this engine counts.  The program has no flow stage; the batch's token call decides
                         // the rule ahead of the owners, and an ENTRY it refused is a pre-decided block: the
                         // cooperative owners take the segment as a SEG_UBLK one, a lane reads DevState.emb
};
enum : uint32_t {
    PX_MULTI = 1,        // representative of a STRATEGY_RELATE component (its members share one segment)
    PX_ORIGIN = 2,       // a flow rule reads an origin StatisticNode (limitApp = an origin / "other", DIRECT):
                         // the resource keeps its origin nodes (ClusterNode.getOrCreateOriginNode)
    PX_CHAIN = 4         // a STRATEGY_CHAIN rule reads the DefaultNode of its context: the resource keeps the
                         // DefaultNodes of the contexts its CHAIN rules name (NodeSelectorSlot)
};
static_assert(sizeof(Prog) == 16, "Prog must be 16 B");

enum : uint8_t { RK_PARAM = 0, RK_FLOW = 1, RK_DEGRADE = 2 };

// compiled rule (host: engine.cpp upload_rules)
enum : uint32_t { LA_DEFAULT = 0, LA_ORIGIN = 1, LA_OTHER = 2 };  // FlowRule.limitApp kinds
#define NO_ID 0xFFFFFFFFu
struct DRule {
    uint8_t kind;
    uint8_t grade;       // flow/param: FLOW_GRADE_*; degrade: DEGRADE_GRADE_*
    uint8_t behavior;    // CONTROL_BEHAVIOR_* (flow, param); param: PB_INIT_ONLY = initialised, never checked
    uint8_t slot;        // index in the resource's full compiled list of this kind (decision rule_slot)
    int32_t max_queue;   // maxQueueingTimeMs
    double count;
    double slope;        // WarmUpController.slope
    int32_t warning_token;
    int32_t max_token;
    int32_t count_div_cold; // (int)count / coldFactor (WarmUpController.coolDownTokens)
    int32_t time_window; // degrade seconds
    int32_t burst;       // param burstCount
    int32_t token_count; // param (int)count
    int64_t duration_sec;// param durationInSec
    int64_t token_count_l; // param (long)count (throttle)
    uint32_t hot_off, hot_n;   // hot items
    uint32_t pmap;       // param: its ParameterMetric time/token map (DevState.pmap index; maps are keyed by
                         // rule equality, so an equal rule reloaded keeps its map)
    uint32_t ref;        // flow STRATEGY_RELATE: the resource whose ClusterNode is checked (NO_REF: none)
    int32_t param_idx;   // param: ParamFlowRule.paramIdx as loaded (< 0: resolved on first use, RState.a)
    uint32_t la_kind;    // flow: LA_* of limitApp
    uint32_t la_origin;  // flow: origin id of the limitApp string (NO_ID: never interned)
    uint32_t strategy;   // flow: STRATEGY_*
    uint32_t chain_ctx;  // flow STRATEGY_CHAIN: context id of refResource (NO_ID: never interned)
    uint32_t pad[3];
};
#define NO_REF 0xFFFFFFFFu
#define PB_INIT_ONLY 0xFF
static_assert(sizeof(DRule) == 112, "DRule must be 112 B");

struct DHot {
    uint64_t key;
    int32_t count;
    int32_t pad;
};

// controller / breaker state
struct RState {
    int64_t a;   // WarmUp storedTokens      | degrade cut (0/1)
    int64_t b;   // WarmUp lastFilledTime    | degrade passCount
    int64_t c;   // latestPassedTime (RateLimiter, WarmUpRateLimiter) | degrade cut_until
    int64_t d;
};

// ParameterMetric's CacheMap (ConcurrentLinkedHashMapWrapper, param/.../ParameterMetric.java:37-114): at most
// `cap` entries, least-recently-used evicted on insert.  A rule's ruleTimeCounters and ruleTokenCounter maps
// see the same key sequence (every passDefaultLocalCheck touches both, time first), so they always hold the
// same keys in the same LRU order and share one map here (v0 = time, v1 = tokens).  A map is owned by one
// resource and only its owner (a lane of k_lane, or a k_pq workgroup) touches it.
//
// Representation (pmap.h): recency is a per-map access stamp, not a linked list.  Every access gives the key
// the next stamp (clock++); the live keys are exactly the `live` largest stamps of keys not evicted or erased,
// recorded in a ring bitmap of 2^rb_log2 bits (bit stamp mod 2^rb_log2; every live stamp lies in
// [clock - 2^rb_log2, clock)).  The least recently used key is the lowest set bit at or after `thr`; evicting it
// clears the bit and nothing else (its slot is dead from then on and is reused by inserts).  The recency rank of
// a key -- how many live keys are more recent -- is a popcount over the ring, which is what lets k_pq decide a
// whole tile of accesses at once (LRU residency = fewer than `cap` distinct keys accessed since the key's stamp).
// Keys live in a two-choice bucketed cuckoo table: a bucket is one 128-byte line of 8 keys + their 8 stamps.
#define PM_BKT 8
#define PK_EMPTY 0xFFFFFFFFFFFFFFFFull  // never-used key slot (param keys are type-tagged, never all-ones)
struct PBucket {
    uint64_t key[PM_BKT];
    int64_t stamp[PM_BKT];  // stamp of the key's last access (live iff its ring bit is set, see pmap.h)
};
static_assert(sizeof(PBucket) == 128, "PBucket must be one 128-byte line");
struct PData {
    int64_t v0;      // rule map: last add time / throttle last pass time; thread map: count
    int32_t v1;      // rule map: tokens
    uint32_t pad;
};
static_assert(sizeof(PData) == 16, "PData must be 16 B");
// A map's buckets are a region of one pool: CacheMaps grow with their keys (ConcurrentLinkedHashMap allocates per
// entry), so a region starts at PM_MIN_NB buckets and is moved to a larger one (param.hip k_pm_grow) before a batch
// could put more keys in it than half its slots -- up to map_buckets(cap) (<= 50 % load at capacity).  1M resources
// with a rule each would otherwise reserve 2 x 256 KiB of HBM per resource.
#define PM_MIN_NB 2u
// The pool's control words (engine.cpp d_pool_next, 4 x u64): the next free bucket, the buckets taken at the last
// compaction, the on-device compactions so far, and the epoch of the batch whose growth found the pool short (that
// batch compacts on the device and grows again, param.hip launch_pm_grow)
enum { PC_NEXT = 0, PC_FLOOR = 1, PC_RESCUES = 2, PC_RESCUE = 3, PC_WORDS = 4 };
__host__ __device__ inline uint32_t map_buckets(uint32_t cap) { return (2u * cap + PM_BKT - 1) / PM_BKT > 2u ? (2u * cap + PM_BKT - 1) / PM_BKT : 2u; }
struct PMap {
    uint64_t base;   // first bucket in DevState.pbkt (its slots' data at pdat[base * PM_BKT ...])
    uint64_t bm;     // first word of the live-stamp ring in DevState.pbm (and of the rank scratch in pre)
    int64_t clock;   // next stamp
    int64_t thr;     // <= the lowest live stamp (eviction scans start here)
    uint32_t nb;     // buckets (PM_MIN_NB .. map_buckets(cap))
    uint32_t cap;    // min(4000 * durationInSec, 200000) for rule maps, 4000 for thread-count maps
    uint32_t live;   // keys in the map
    uint32_t rb_log2;// ring bits = 2^rb_log2 >= 4 * cap
    uint32_t pad[4];
};
static_assert(sizeof(PMap) == 64, "PMap must be 64 B");
#define PM_BASE_CAP 4000u      // ParameterMetric.BASE_PARAM_MAX_CAPACITY / THREAD_COUNT_MAX_CAPACITY
#define PM_TOTAL_CAP 200000u   // ParameterMetric.TOTAL_MAX_CAPACITY
#define PQ_MAX_CAP 8176u       // largest map k_pq holds (its live-stamp ring of 2^15 bits in LDS: durationInSec <= 2)

enum : uint8_t { ST_PASS = 0, ST_PASS_WAIT = 1, ST_BLOCK_FLOW = 2, ST_BLOCK_DEGRADE = 3, ST_BLOCK_PARAM = 4,
                 ST_NO_CHECK = 5, ST_BLOCK_UPSTREAM = 6, ST_BLOCK_AUTHORITY = 7, ST_NOT_ENTRY = 0xFF };

#define HEAD_OFF 16384u  // DevCfg.dbg_flags: the cooperative owner decides XF_HEADT / XF_HEADR heads too (A/B)
#define TABLES_ALL 32768u  // SG_DEBUG_FLAGS: the hot / cold group stage builds the side tables for every position (A/B)
#define LITE_CHECK 65536u  // DevCfg.dbg_flags (SG_LITE_CHECK=1): k_lite reads the window start of every minute bucket it
                           // stores without a load and raises BF_LITE_STALE if the bucket was not stale
#define UBLK_OFF 131072u  // DevCfg.dbg_flags (SG_UBLK=0): a pre-blocked ENTRY marks PM_LANE and its record carries no
                          // RF_UBLK: every such resource on a lane, as before the cooperative owners took the class (A/B)
struct DevCfg {
    int32_t max_rt;
    int32_t occupy_timeout;
    int32_t max_chain;
    int32_t switch_on;
    int64_t snap_hi;     // highest second a metrics snapshot created / reset minute buckets at (-1: none): k_snap_count
                         // writes the bucket of its `now` without moving the second window (k_lite's stale rule)
    uint64_t ring_mask;
    uint32_t dbg_flags;  // SG_DEBUG_FLAGS experiment switches (0 in production)
    uint32_t heads;      // some program is XF_HEADT / XF_HEADR: the head owner (head.hip) runs beside the bins
};

// one resource's events inside a batch: sorted positions [start, start+len)
struct Seg {
    uint32_t res;
    uint32_t start;
    uint32_t len;
    uint32_t bin;    // BIN_* (| SEG_AUXP)
};
#define SEG_AUXP 0x80u  // Seg.bin: the segment's origin / context nodes are updated by the aux.hip post-pass
#define SEG_PV 0x40u    // Seg.bin: pvalue.hip decided the segment's param checks (k_pq's pre pass leaves it)
#define SEG_PVT 0x100u  // Seg.bin: pvalue.hip's post pass updated the thread-count map (k_pq's post pass leaves it)
#define SEG_TABS 0x200u  // Seg.bin: the segment's side tables (forward links, bst[]) exist: its owner may skip frozen
                         // stretches (k_seg_bin; bits 0..5 the bin, 6..10 these flags, the rank inside its block above
                         // them until k_seg_order places the segment)
#define SEG_UBLK 0x400u  // Seg.bin: a PM_UBLK resource's segment on a cooperative owner: RF_UBLK ENTRYs are pre-decided
                         // blocks (k_head leaves it to k_jac; bits 6..10 the flags)
#define SEG_RANK_SHIFT 11

// pvalue.hip: the value-parallel pre pass of long XF_MIX segments
// per listed segment (the wide XF_MIX list): what the pre pass found
struct PvSeg {
    uint32_t ok;        // decided here (else k_pq's pre / post pass)
    uint32_t n;         // accesses
    uint32_t off;       // first access in the dense arrays
    uint32_t mid;       // rule map (the post pass: the thread-count map of paramIdx 0)
    uint32_t rk;        // the checked rule's index in the program
    uint32_t ch0;       // first extraction chunk
    uint32_t nch;       // extraction chunks
    uint32_t fbits;     // post pass: ParameterMetric bits of the rules the segment's ENTRYs visited
    uint32_t freach;    // post pass: segment position + 1 of the first ENTRY visiting rule k0 (EXITs release from it)
    int32_t peak;       // post pass: the thread-count map's largest growth over its start size
    uint32_t tm0;       // post pass: EXITs release from position 0 (the node had the bits already)
    uint32_t sub;       // post pass: the segment releases thread counts (else increments only: LRU residency)
};

struct PvBuf {          // dense per-access arrays (capacity >= the listed segments' events)
    uint64_t* key;
    uint32_t* pos;      // segment-relative position
    int32_t* dt;
    uint32_t* acq;      // acquire | (token count of the value) << 16 is not enough: tc in its own array
    int32_t* tc;
    uint32_t* seg;      // listed segment index
    uint32_t* gid;      // sort keys (group = hash slot) -> after the sort: sorted keys
    uint32_t* idx;      // sort values -> after the sort: accesses in (group, order) order
    uint32_t* gid2;
    uint32_t* idx2;
    int32_t* prev;      // previous access of the value (dense index), PV_NONE
    int32_t* w;         // first access of a value: its recency rank at the start (PV_INF: absent); others -1
    int32_t* sprev;     // prev sorted per block
    int32_t* sw;        // w sorted per block
    int32_t* fslot;     // first access: the value's slot in the map (any liveness), -1
    uint8_t* hit;
    uint8_t* keep;      // last access of a value: the value stays in the map
    int64_t* flast;     // last access of a value: its final (lastAddTime, tokens)
    int32_t* ftok;
    unsigned long long* htab;  // 2 slots per access: the per-segment hash tables of values
    // extraction chunks (PV_CH positions of one segment each): (listed segment, first position), accesses, offsets
    uint2* chunk;
    uint32_t* ccnt;
    uint32_t* cof;
    // the walk's inputs in sorted order: time, acquire | hit << 16, record index
    int32_t* gdt;
    uint32_t* gaw;
    uint32_t* gpos;
    uint4* range;       // blocked stretches the walk jumped over: {first, end, decision word}; count in tot[2]
};



// ---- token server (cluster.hip): ClusterMetric per flowId + the namespace GlobalRequestLimiter
enum { CF_PASS = 0, CF_BLOCK, CF_PASS_REQ, CF_BLOCK_REQ, CF_OCC_PASS, CF_OCC_BLOCK, CF_WAITING, CF_N };  // ClusterFlowEvent
struct CBkt {          // ClusterMetricBucket in a LeapArray slot; ws < 0: slot never created
    int64_t ws;
    int64_t c[CF_N];
};
struct CFlow {         // one flowId: rule view + ClusterMetricLeapArray bookkeeping
    int64_t flow_id;
    double count;                  // FlowRule.count
    int32_t thr_type;              // ClusterFlowConfig.thresholdType
    int32_t n, interval;           // sampleCount, windowIntervalMs of the metric (fixed at creation)
    int32_t connected;             // ConnectionManager.getConnectedCount (AVG_LOCAL)
    uint32_t boff;                 // first bucket in the bucket array
    uint32_t has_occ;              // ClusterMetricLeapArray.hasOccupied
    int64_t occ_pass, occ_req;     // occupyCounter[PASS], occupyCounter[PASS_REQUEST]
};
struct CSlot {         // flowId -> flow index (open addressing, idx 0xFFFFFFFF = empty)
    int64_t key;
    uint32_t idx, pad;
};
// token server view of a cluster-mode ParamFlowRule + its ClusterParamMetric
// (csrv/flow/statistic/metric/ClusterParamMetric.java:36-91, ClusterParameterLeapArray.java:30-58)
#define CP_MAXN 16      // sampleCount bound of the device window (SG_ENOTSUP above)
struct PFlow {
    int64_t flow_id;
    double count;                  // ParamFlowRule.count
    int32_t thr_type;              // ParamFlowClusterConfig.thresholdType
    int32_t n, interval;           // sampleCount, windowIntervalMs (fixed at creation)
    int32_t connected;             // connected count of the namespace (AVG_LOCAL)
    uint32_t hoff, nhot;           // parsed hot items: PHot[hoff, hoff + nhot)
    int64_t fws[CP_MAXN];          // bucket window starts; < 0: never created
};
struct PHot {
    uint64_t key;
    int32_t count, pad;
};
#define PV_EMPTY 0xFFFFFFFFu
struct PVal {                      // (flow, value) counts; live in bucket j while ws[j] == PFlow.fws[j]
    uint64_t key;
    uint32_t flow, pad;            // flow == PV_EMPTY: free slot (claimed by CAS)
    int64_t ws[CP_MAXN];
    int64_t cnt[CP_MAXN];
};
#define NS_BUCKETS 10   // RequestLimiter: UnaryLeapArray(10, 1000)
#define NS_WLEN 100
#define NS_INTERVAL 1000
struct NsLimiter {
    int64_t ws[NS_BUCKETS];   // < 0: never created
    int64_t cnt[NS_BUCKETS];
};

// Forward links of one ENTRY (k_gather): (epoch << 32) | sorted position of the EXIT / TRACE of the same
// batch whose reference names it.  A tag from another batch means "no link".
struct Link {
    uint64_t exit_l;
    uint64_t trace_l;
};
// A frozen span [s, e) of sorted positions (<= SPAN_CHUNK of them) whose verdicts k_fill writes: every
// ENTRY blocks on the first flow stage its count exceeds at pass count pint, else on the first degrade
// stage when that breaker was cut (res bit 31).
struct Span {
    uint32_t s, e, res;
    int32_t pint;
};
#define SPAN_CHUNK 8192u
#define BST_STATIC 0x80000000u  // bst[] flag: the block holds an EXIT/TRACE that is effective without a link
#define BST_CNT 0x7FFFFFFFu

// Origin StatisticNodes (ClusterNode.originCountMap) and context DefaultNodes (NodeSelectorSlot): one
// open-addressing table of nodes keyed (resource, kind, id), 256 B a node, claimed by CAS on the key.
//
// What a node keeps is what the path can read of it.  Its second window is a full 2 x 500 ms LeapArray (flow
// rules on an origin / context read passQps, threadNum; StatisticSlot updates it).  Of its minute window the
// only reader is WarmUpController's previousPassQps (LeapArray.getPreviousWindow: the pass of the second before
// now, LeapArray.java:216-234) and addOccupiedPass / addPassRequest only add to it, so the node keeps, per
// second parity, the latest second in which pass was added and that second's pass: the previous second's pass
// is found iff it is the latest pass-second of its parity, as a 60-slot ring would give it (the other minute
// fields of an origin / context node are never read: MetricTimerListener exports ClusterNodes only).
struct AuxNode {
    unsigned long long key;  // res << 32 | kind << 31 | id; AUX_EMPTY = free
    int32_t thread;          // curThreadNum
    uint32_t flags;          // AUXF_*
    int64_t mws[2];          // minute window, per second parity: the latest second with pass added (-1: none)
    int64_t mpass[2];        //   and its pass
    int64_t pad0[2];
    Bkt sec[2];              // rollingCounterInSecond
    int64_t borrow[4];       // FutureBucketLeapArray {ws, pass} x 2 (prioritized entries on this node)
    int64_t pad1[4];
};
static_assert(sizeof(AuxNode) == 256, "AuxNode size");
#define AUXF_BORROW 1u       // the node's borrow ring was written (a reset reads it)
#define AUX_EMPTY 0xFFFFFFFFFFFFFFFFull
enum : uint32_t { AUX_ORIGIN = 0, AUX_CONTEXT = 1 };
// the aux.hip post-pass: one node's updates of a batch (or of a piece of a segment), merged per 500 ms bucket
// parity as LeapArray.currentWindow merges them (a later window replaces, the same window adds)
struct AuxAcc {
    uint32_t key;            // kind << 31 | id
    int32_t thread;          // curThreadNum delta
    int64_t W[2];            // second window: latest window start per 500 ms parity (-1: none)
    uint64_t s[2][4];        //   pass, block, succ, rt added at W[p]
    uint32_t minrt[2];       //   min rt at W[p] (0xFFFFFFFF: none)
    int64_t MW[2];           // minute window: latest second with pass added, per second parity (-1: none)
    uint64_t mpass[2];
};
static_assert(sizeof(AuxAcc) == 128, "AuxAcc size");
#define AUX_PIECE 4096u      // aux.hip: events of a long segment per piece workgroup

// The global inbound node, Constants.ENTRY_NODE (inbound.hip): a ClusterNode without rules that StatisticSlot counts
// every EntryType.IN entry and exit on (StatisticSlot.java:72-76, 89-92, 107-110, 158-161).  One node an engine, in an
// allocation of its own (made by the first sg_track_inbound): both windows in full, as every reader of it wants them
// (MetricTimerListener its minute window, SystemRuleManager / SystemStatusListener its second window and thread count).
#define INB_SLOTS 62         // 2 second-window buckets, then the 60 minute-window buckets
#define INB_TILE 4096u       // records a workgroup folds between two 64-bit folds (4,096 x 65,535 < 2^32)
#define INB_MAX_WG 1024u     // partials a batch can leave (a few workgroups a CU)
struct InbNode {
    Bkt sec[2];              // rollingCounterInSecond (its borrow ring stays empty: nothing occupies on this node)
    Bkt minb[60];            // rollingCounterInMinute
    int32_t thread;          // curThreadNum
    uint32_t last[3];        // of the last batch: workgroups that left a partial, records visited, updates counted
    int64_t last_fetch;      // StatisticNode.lastFetchTime of its metrics()
};
// what one workgroup's tiles add up to: per slot the latest window its events fall in (an index relative to the batch,
// 500 ms units for the second window, seconds for the minute window; -1: none) and the sums of the events in it
struct InbPart {
    int32_t W[64];
    uint64_t s[64][4];       // pass, block, success, rt
    uint32_t minrt[64];      // 0xFFFFFFFF: none
    int32_t thread;
    uint32_t visited, updates, pad;
};

struct DevState {
    Bkt* sec;
    int64_t* borrow;          // [res][2 slots] x {ws, pass}: FutureBucketLeapArray of the second window
    const uint32_t* prio;     // [res] sticky PM_* marks of the group stage (PM_PRIO: the borrow ring is live)
    uint64_t* key_ring;       // arg key of every ENTRY by global event index (ring like the status ring),
                              // NO_KEY if it had none; null until param rules exist
    uint64_t gbase;           // global index of the batch's first event
    Bkt* minb;
    NodeInfo* info;
    const Prog* prog;
    const DRule* rules;
    RState* rstate;
    const DHot* hot;
    PMap* pmap;               // ParameterMetric maps (see PMap)
    PBucket* pbkt;            // their key/stamp buckets
    PData* pdat;              // their values, one per bucket slot
    uint64_t* pbm;            // their live-stamp rings
    uint32_t* ppre;           // per ring word: rank scratch of a lane-side compaction (pmap.h pm_compact)
    const uint32_t* tmid;     // [Prog.tm_base + paramIdx] -> thread-count map (NO_ID: none)
    uint8_t* ring;
    unsigned long long* dbg;  // optional per-batch diagnostics (SG_DEBUG=1), else null
    uint32_t* sink;           // >= 1024 scratch words: target of masked-off unconditional stores
    // frozen-stretch skipping (decide.hip k_jac<..., SKIP>): side tables of the batch built by k_gather
    const Link* link;         // [sorted pos of an ENTRY] -> the EXIT / TRACE of this batch that references it
    const uint32_t* bst;      // [pos >> 10] ENTRY count sum of the 1024-position block | BST_STATIC
    uint32_t* pend;           // [sorted pos] per-segment list of the owner's committed passes (relative positions)
    Span* spans;              // frozen spans whose verdicts k_fill writes after the decide kernels
    uint32_t* nspan;          // span counter (may exceed span_cap: overflow falls back to streaming)
    uint32_t span_cap;
    uint32_t epoch;           // tag of this batch's links
    uint32_t skip_ok;         // 0: no skipping this batch (links not unique / zero-count ENTRYs / SG_DEBUG_FLAGS & 4)
    uint32_t skip_min;        // a stretch is skipped only if it holds more positions than this (SG_SKIP_MIN)
    // sg_submit_ex: per-event context and args (null: none), origin / context nodes
    const sg_event_ext* ext;  // [submission index]
    const sg_arg* args;
    AuxNode* aux_tab;         // origin / context nodes (open addressing, aux_mask + 1 slots)
    uint32_t* aux_count;      // nodes claimed
    uint32_t aux_cap;
    uint32_t max_ctx;         // context ids above this are NullContexts
    uint64_t aux_mask;
    // AuthoritySlot on the device (authority.h): a descriptor per resource and the rules' origin ids; auth is null
    // unless authority rules are loaded
    const AuthDesc* auth;
    const uint32_t* auth_ids;
    // embedded token server: per sorted position the word the token call left for an ENTRY of an XF_EMB resource
    // (embedded.h emb_word: a BLOCKED answer's final word, a SHOULD_WAIT answer's wait, else 0); null unless the
    // batch made a token request
    const uint32_t* emb;
};

enum : uint32_t { BF_PRIORITIZED = 1,
                  BF_PQ_INVARIANT = 2,  // k_pq: a tile's presorted key subset is not what it must be (internal error)
                  BF_PTAB_FULL = 4,     // a param map could not place a key (the map then holds a ghost entry)
                  BF_BAD_RES = 8, BF_BAD_REF = 16,
                  BF_BACKWARD = 32, BF_TSPAN = 64,
                  BF_BAD_ARGS = 512,    // an sg_event_ext names args outside the table, or more than SG_MAX_ARGS
                  BF_AUX_FULL = 1024,   // the origin / context node pool is full
                  BF_POOL_FULL = 2048,  // a param map could not grow: the bucket pool (param_table_log2) is used up
                  BF_MULTI_LINK = 128,  // an ENTRY is referenced by two EXITs (or two TRACEs) of the batch
                  BF_ZERO_CNT = 256,    // an ENTRY acquires 0 (it may pass inside a saturated stretch)
                  BF_TINY_FALLBACK = 4096,  // k_tiny: the batch needs the batched path (nothing decided)
                  BF_TINY_REJECTED = 8192,
                  BF_LITE_STALE = 16384 };  // k_lite under LITE_CHECK: a minute bucket stored without a load held its second or
                                            // a later one (internal error)  // k_tiny: the batch's checks failed before any decision

// One event in resource-sorted order (16 B), built by k_prep from the caller's 24-byte
// sg_event so that every decide kernel streams its segment with coalesced loads.
struct SEv {
    int32_t dt;      // ts - t0 (t0 = ts of the batch's first event)
    uint32_t x;      // EXIT/TRACE with code RC_BATCH: sorted position of the referenced ENTRY
    uint16_t cnt;    // acquire / exit / trace count
    uint16_t rt;     // EXIT: response time clipped to statistic_max_rt (StatisticSlot.exit)
    uint8_t kind;    // SG_EV_*
    uint8_t flags;   // SG_F_*
    uint8_t code;    // EXIT/TRACE: RC_*
    uint8_t pad;
};
static_assert(sizeof(SEv) == 16, "SEv must be 16 B");
// how an EXIT/TRACE's ENTRY reference resolved
enum : uint8_t {
    RC_NONE = 0,    // no reference (or unknown entry): effective iff the resource has a chain
    RC_BATCH = 1,   // ENTRY earlier in this batch, same resource: effective iff it passed
    RC_PASSED = 2,  // ENTRY of an earlier batch that passed
    RC_NOT = 3,     // ENTRY that did not pass (blocked / no chain), or a TRACE of an unknown entry
    RC_PREV = 4     // ENTRY of an earlier batch, status not read yet (x = status-ring index): resolved to
                    // RC_NONE / RC_PASSED / RC_NOT by k_resolve once the earlier batches are decided
};

// decide-kernel bins of a segment (Seg.pad); order[] is laid out bin by bin
enum : uint32_t {
    BIN_J16 = 0,           // one 1024-lane workgroup per segment (Zipf head)
    BIN_J4 = 1,            // one 256-lane workgroup per segment
    BIN_J1 = 2,            // one wavefront per segment
    BIN_PQ16 = 3,          // PF_PQ segments: one 1024-lane k_pq workgroup (long segments)
    BIN_PQ4 = 4,           //                 one 256-lane k_pq workgroup
    BIN_J8 = 5,            // one 512-lane workgroup per segment: the J16 lengths of QPS-DefaultController programs
    BIN_LANE = 6,          // one lane per segment, nr <= 4: bins 6..6+LANE_BINS-1 by descending log2(len)
    LANE_BINS = 19,
    BIN_LANE16 = BIN_LANE + LANE_BINS,  // one lane per segment, nr > 4 (rule state in scratch)
    BIN_LITE = BIN_LANE16 + LANE_BINS,  // one lane per segment, DefaultController flows + breakers only (k_lite)
    N_BINS = BIN_LITE + LANE_BINS       // <= 63: k_bin_offsets runs one 64-lane wave
};

// The words of a batch slot's small block (BatchSlot::d_bsmall, BS_WORDS of them), which the host and the kernels
// share: k_grp_clear zeroes the block at the start of the slot's group stage, the kernels get the address of the
// word they write, and the host reads two prefixes of it from pinned copies -- BS_HEAD_WORDS after the group stage
// (accept_grouped, decide_enqueue), BS_MIRROR_WORDS after the decide stage (collect).
enum : uint32_t {
    BS_FLAGS = 0,        // BF_* of the batch: the group stage's checks, then what the decide kernels raise
    BS_NSEG = 1,         // segments
    BS_NCAND = 2,        // chain candidates (k_chain, under a finite chain cap)
    BS_NPREV = 3,        // references into earlier batches (k_resolve's list)
    BS_T0 = 4,           // [4..5] int64: ts of the batch's first event
    BS_MIX_N = 6,        // XF_MIX segments of the cooperative bins: narrow, [7] wide
    BS_MIX_NW = 7,
    BS_BIN_OFF = 8,      // [8 .. 8 + N_BINS]: the bins' offsets in order[]
    BS_MIX_WIDE = 72,    // events of the wide XF_MIX segments
    BS_HOT_MARKED = 73,  // hot ids k_seg_bin marked for the side tables
    BS_UBLK = 74,        // PM_UBLK segments in cooperative bins (SEG_UBLK), [75] in lane bins
    BS_UBLK_LANE = 75,
    BS_HOT_NEXT = 76,    // the next batch's hot ids
    BS_GRP = 77,         // the hot / cold group stage's own: hot_total (the cold region's start), [78] cold events
    BS_COLD_N = 78,
    BS_HOT_SEGS = 80,    // hot segments, [81] hot_total again, [82] cold segments
    BS_COLD_SEGS = 82,
    BS_EMB = 83,         // events of XF_EMB segments, [84] XF_EMB segments in cooperative bins, [85] in lane bins
    BS_EMB_COOP = 84,
    BS_EMB_LANE = 85,
    BS_HEAD_WORDS = BS_EMB_LANE + 1,    // 86: the last word the host reads after the group stage + 1
    BS_EMB_REQ = 100,    // embedded token server: the batch's requests, [101..107] its answers by class (EMB_A_*)
    BS_EMB_ANS = 101,
    BS_EMB_AHEAD = 108,  // ... and the words written ahead of the cooperative owners
    BS_UBLK_WORDS = 119, // RF_UBLK words written (k_ublk_words)
    BS_NSPAN = 120,      // frozen spans recorded (DevState.nspan)
    BS_MIRROR_WORDS = BS_NSPAN + 1,     // 121: the last word collect() reads + 1
    BS_AUX = 130,        // [130..133] counts of the aux.hip post-pass lists k_seg_bin builds
    BS_AUX_POOL_N = 134, // partials taken from the aux pool
    BS_WORDS = 256
};
static_assert(BS_BIN_OFF + N_BINS + 1 <= BS_MIX_WIDE, "the bin offsets end below the next word");
// The head copy: accept_grouped() reads BS_FLAGS, BS_MIX_NW, BS_MIX_WIDE, BS_HOT_MARKED, BS_UBLK, BS_UBLK_LANE,
// BS_HOT_NEXT and BS_EMB .. BS_EMB_LANE (the highest: BS_HEAD_WORDS is that word + 1); decide_enqueue() reads BS_FLAGS,
// BS_NSEG, BS_NPREV, both words of BS_T0, BS_MIX_N, BS_MIX_NW, the N_BINS + 1 bin offsets, BS_MIX_WIDE and BS_UBLK.
static_assert(BS_T0 + 1 < BS_MIX_N && BS_MIX_NW < BS_BIN_OFF && BS_BIN_OFF + N_BINS < BS_HEAD_WORDS &&
                  BS_MIX_WIDE < BS_HEAD_WORDS && BS_HOT_MARKED < BS_HEAD_WORDS && BS_UBLK_LANE < BS_HEAD_WORDS &&
                  BS_HOT_NEXT < BS_HEAD_WORDS && BS_EMB + 2 == BS_EMB_LANE && BS_HEAD_WORDS == BS_EMB_LANE + 1,
              "accept_grouped() and decide_enqueue() read the head copy only");
// The mirror copy: collect() reads BS_FLAGS, the nine words BS_EMB_REQ .. BS_EMB_AHEAD, BS_UBLK_WORDS and BS_NSPAN
// (the highest: BS_MIRROR_WORDS is that word + 1).
static_assert(BS_EMB_REQ + 1 == BS_EMB_ANS && BS_EMB_REQ + 8 == BS_EMB_AHEAD && BS_EMB_AHEAD < BS_UBLK_WORDS &&
                  BS_UBLK_WORDS < BS_NSPAN && BS_MIRROR_WORDS == BS_NSPAN + 1 && BS_HEAD_WORDS <= BS_MIRROR_WORDS,
              "collect() reads the mirror copy only");
static_assert(BS_AUX_POOL_N < BS_WORDS, "small block size");

// The engine-wide small block (sg_engine::d_small, SM_WORDS of them): scratch words of the calls that run on the
// engine stream outside a batch.
enum : uint32_t {
    SM_FLAGS = 0,        // a call's flag word (token calls: 1 unordered requests, 2 value table full; k_pm_grow_ids: BF_*)
    SM_SNAP_TOTAL = 3,   // sg_snapshot_metrics: rows
    SM_LIMITER = 8,      // the parallel token limiters' words (cluster.hip launch_tok_limiter_par / _ns)
    SM_WORDS = 256
};

} // namespace sg
