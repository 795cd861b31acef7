/*
 * sentinel_gpu.h -- C ABI of the MI355X batched decision engine for Sentinel's
 * statistics-and-rule-check hot path.
 *
 * This header is the drop-in boundary.  Everything the Java
 * side needs crosses it as plain pointers, sizes and POD structs; no C++ or
 * torch type appears here.  Each entry point names the reference interface it
 * replaces (paths relative to /root/reference, prefixes as in SURVEY.md §0.1):
 *
 *   core/  = sentinel-core/src/main/java/com/alibaba/csp/sentinel/
 *   param/ = sentinel-extension/sentinel-parameter-flow-control/src/main/java/com/alibaba/csp/sentinel/
 *   csrv/  = sentinel-cluster/sentinel-cluster-server-default/src/main/java/com/alibaba/csp/sentinel/cluster/
 *
 * Threading: one submitting thread per engine.  Every call returns before its
 * buffers may be reused, except sg_submit_async (completion via sg_sync).
 * Errors are returned as negative status codes; sg_last_error() gives the text.
 * An async batch's errors are reported late: what its group stage finds (a bad
 * res_id, timestamps going back inside the batch, a bad args table) is returned
 * by the next call that touches the engine, which then accepts no batch of its
 * own; what its decide stage finds is returned one call later still, as before.
 * A synchronous call reports every error of its own batch itself.
 * No exception ever crosses the ABI (the Java binding turns status codes into
 * BlockException subclasses, core/CtSph.java:157-166).
 */
#ifndef SENTINEL_GPU_H
#define SENTINEL_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SG_ABI_VERSION 1

/* ---- status codes ------------------------------------------------------ */
enum {
    SG_OK = 0,
    SG_EINVAL = -1,     /* bad argument */
    SG_ENOMEM = -2,     /* device or host allocation failed */
    SG_EDEVICE = -3,    /* HIP runtime error / no gfx950 device */
    SG_ESTATE = -4,     /* call out of order (e.g. submit before rules) */
    SG_ENOTSUP = -5,    /* configuration outside what the device path implements */
    SG_ENOTFOUND = -6,  /* unknown resource / flow id */
    SG_ECAPACITY = -7   /* a fixed-capacity table is full */
};

/* ---- rule constants (core/slots/block/RuleConstant.java:26-55) --------- */
enum {
    SG_FLOW_GRADE_THREAD = 0,
    SG_FLOW_GRADE_QPS = 1,
    SG_DEGRADE_GRADE_RT = 0,
    SG_DEGRADE_GRADE_EXCEPTION_RATIO = 1,
    SG_DEGRADE_GRADE_EXCEPTION_COUNT = 2,
    SG_STRATEGY_DIRECT = 0,
    SG_STRATEGY_RELATE = 1,
    SG_STRATEGY_CHAIN = 2,
    SG_CONTROL_BEHAVIOR_DEFAULT = 0,
    SG_CONTROL_BEHAVIOR_WARM_UP = 1,
    SG_CONTROL_BEHAVIOR_RATE_LIMITER = 2,
    SG_CONTROL_BEHAVIOR_WARM_UP_RATE_LIMITER = 3,
    /* ClusterRuleConstant (sentinel-core .../cluster/ClusterRuleConstant) */
    SG_CLUSTER_THRESHOLD_AVG_LOCAL = 0,
    SG_CLUSTER_THRESHOLD_GLOBAL = 1
};
enum { SG_AUTHORITY_WHITE = 0, SG_AUTHORITY_BLACK = 1 };   /* RuleConstant.AUTHORITY_* */

/* ---- engine configuration ---------------------------------------------- */
typedef struct sg_config {
    int32_t sample_count;        /* SampleCountProperty.SAMPLE_COUNT = 2 (core/node/SampleCountProperty.java:42) */
    int32_t interval_ms;         /* IntervalProperty.INTERVAL = 1000 (core/node/IntervalProperty.java:41) */
    int32_t statistic_max_rt;    /* Constants.TIME_DROP_VALVE = 4900 (core/Constants.java:62) */
    int32_t cold_factor;         /* ColdFactorProperty.coldFactor = 3 */
    int32_t occupy_timeout_ms;   /* OccupyTimeoutProperty = 500 (core/node/OccupyTimeoutProperty.java:40) */
    int32_t max_slot_chain_size; /* Constants.MAX_SLOT_CHAIN_SIZE = 6000 (core/Constants.java:36); 0 = unbounded */
    int32_t switch_on;           /* Constants.ON (core/Constants.java:67) */
    int32_t device;              /* HIP device ordinal this engine owns */
    uint32_t max_resources;      /* capacity of the resource table (dense ids 0..max-1) */
    uint32_t max_rules;          /* capacity of the compiled rule table (all kinds) */
    uint32_t param_table_log2;   /* cap on the hot-parameter map pool: the bucket slots of every ParameterMetric
                                    CacheMap together (~2x each map's LRU capacity, 32 B a slot) <= 2^log2;
                                    rule loads past it fail SG_ECAPACITY.  Default 28 */
    uint32_t status_ring_log2;   /* entry-status ring for EXIT/TRACE references = 2^log2 events */
    uint32_t max_batch_events;   /* largest n accepted by sg_submit */
    /* token server (csrv/server/config/ServerFlowConfig.java:26-31) */
    int32_t cluster_sample_count;     /* 10 */
    int32_t cluster_interval_ms;      /* 1000 */
    double cluster_exceed_count;      /* 1.0 */
    double cluster_max_occupy_ratio;  /* 1.0 */
    int32_t cluster_max_allowed_qps;  /* GlobalRequestLimiter default 30000 */
    uint32_t aux_node_capacity;       /* origin StatisticNodes + context DefaultNodes kept on the device for the
                                         resources whose flow rules read them (origin / "other" / CHAIN rules);
                                         ~4 KB each, default 65536 */
    int32_t reserved[6];
} sg_config;

/* ---- rules ----------------------------------------------------------------
 * Field meaning and defaults follow the Java beans exactly; strings are
 * NUL-terminated UTF-8 (ASCII hashes like java.lang.String.hashCode). */

/* core/slots/block/flow/FlowRule.java:40-90 + ClusterFlowConfig.java */
typedef struct sg_flow_rule {
    const char* resource;
    const char* limit_app;            /* NULL/""/"default" => "default" */
    const char* ref_resource;         /* RELATE / CHAIN */
    double count;
    int32_t grade;                    /* default QPS */
    int32_t strategy;                 /* default DIRECT */
    int32_t control_behavior;         /* default DEFAULT */
    int32_t warm_up_period_sec;       /* default 10 */
    int32_t max_queueing_time_ms;     /* default 500 */
    int32_t cluster_mode;             /* bool */
    int64_t cluster_flow_id;          /* ClusterFlowConfig.flowId (0 = null) */
    int32_t cluster_threshold_type;   /* default AVG_LOCAL */
    int32_t cluster_fallback_to_local;/* default true */
    int32_t cluster_strategy;         /* default 0 (NORMAL) */
    int32_t cluster_sample_count;     /* default 10 */
    int32_t cluster_window_interval_ms; /* default 1000 */
    int32_t reserved;
} sg_flow_rule;

/* core/slots/block/degrade/DegradeRule.java:60-140 */
typedef struct sg_degrade_rule {
    const char* resource;
    const char* limit_app;
    double count;
    int32_t time_window;              /* seconds */
    int32_t grade;                    /* default RT */
} sg_degrade_rule;

/* param/slots/block/flow/param/ParamFlowItem.java:24-40 */
typedef struct sg_param_item {
    const char* object;               /* value as a string */
    const char* class_type;           /* "int", "java.lang.Long", "java.lang.String", ... */
    int32_t count;                    /* item threshold (Integer; <0 = ignored) */
    int32_t has_count;                /* 0 => Integer null => item ignored */
} sg_param_item;

/* param/slots/block/flow/param/ParamFlowRule.java:40-70 + ParamFlowClusterConfig */
typedef struct sg_param_rule {
    const char* resource;
    const char* limit_app;
    double count;
    int64_t duration_in_sec;          /* default 1 */
    int32_t grade;                    /* default QPS */
    int32_t param_idx;                /* Integer paramIdx (has_param_idx=0 => null => invalid) */
    int32_t has_param_idx;
    int32_t control_behavior;         /* DEFAULT or RATE_LIMITER */
    int32_t max_queueing_time_ms;     /* default 0 */
    int32_t burst_count;              /* default 0 */
    int32_t cluster_mode;
    int32_t n_items;
    const sg_param_item* items;
    int64_t cluster_flow_id;
    int32_t cluster_threshold_type;
    int32_t cluster_fallback_to_local;
    int32_t cluster_sample_count;
    int32_t cluster_window_interval_ms;
} sg_param_rule;

/* core/slots/block/authority/AuthorityRule.java */
typedef struct sg_authority_rule {
    const char* resource;
    const char* limit_app;            /* comma-separated origin names, compared verbatim (no trimming) */
    int32_t strategy;                 /* default WHITE; neither WHITE nor BLACK: valid, never blocks */
    int32_t reserved;
} sg_authority_rule;

/* ---- events ----------------------------------------------------------------
 * One 24-byte record per SphU.entry / Entry.exit / Tracer.trace, in
 * non-decreasing ts order (ties keep submission order).  ts is the value
 * TimeUtil.currentTimeMillis() had at the event (core/util/TimeUtil.java:49).
 * One batch spans at most SG_MAX_BATCH_SPAN_MS: its last ts minus its first
 * (the kernels keep an event's time as a 32-bit offset from the batch's first
 * event).  The limit is per batch; any time may pass between two batches. */
#define SG_MAX_BATCH_SPAN_MS 0x7FFFFFFFll /* 2^31 - 1 ms, 24.8 days */
enum {
    SG_EV_ENTRY = 0,  /* SphU.entry(name, type, count, args...)   core/SphU.java:202 */
    SG_EV_EXIT = 1,   /* Entry.exit(count[, args])                core/Entry.java:78-103 */
    SG_EV_TRACE = 2   /* Tracer.trace(t, count)                   core/Tracer.java:47-59 */
};
enum {
    SG_F_PRIORITIZED = 1u << 0, /* SphU.entryWithPriority (ENTRY) */
    SG_F_HAS_ARG = 1u << 1,     /* args = {args[0]}, non-null; aux = its interned 64-bit key (ENTRY; sg_submit_ex
                                   with ext.n_args > 0 takes the args from the table instead) */
    SG_F_EXIT_ARGS = 1u << 2,   /* Entry.exit(count, args): param thread counts are released (EXIT), SURVEY Q14 */
    SG_F_ENTRY_OUT = 1u << 3,   /* EntryType.OUT (ENTRY, and the EXIT of such an ENTRY: an EXIT carries the flag iff its
                                   ENTRY did, the Entry keeps its ResourceWrapper).  No check reads it (SystemSlot is
                                   out of scope); events with the flag are not counted on the global inbound node
                                   (sg_track_inbound) */
    SG_F_BLOCKED_UPSTREAM = 1u << 4 /* ENTRY: the caller's SystemSlot threw (or an AuthoritySlot the caller chose to keep
                                   instead of sg_load_authority_rules).  Those slots sit between ParamFlowSlot and
                                   FlowSlot (param/slots/HotParamSlotChainBuilder.java:39-50), so the param checks still
                                   run (and may block first); otherwise the entry is blocked with SG_BLOCK_UPSTREAM --
                                   before the engine's own authority check, as SystemSlot precedes AuthoritySlot.  The
                                   resource keeps its cooperative owner (the entry is a block whose word is written
                                   ahead of it); only short segments, resources whose rules are param rules alone, read
                                   an origin / context node or name a RELATE resource, and resources that also saw a
                                   prioritized or NullContext entry are decided one lane per resource from then on -- and
                                   StatisticSlot counts the block (StatisticSlot.java:97-117) */
};
/* EXIT/TRACE aux: low 48 bits = global index of the ENTRY event this refers
 * to (SG_REF_NONE = the caller asserts the entry passed); EXIT bits 48..63 =
 * raw response time min(exit_ts - entry_ts, 65535) before the TIME_DROP_VALVE clip. */
#define SG_REF_NONE 0xFFFFFFFFFFFFull
#define SG_AUX_EXIT(ref, rt_raw) (((uint64_t)(rt_raw) << 48) | ((uint64_t)(ref) & SG_REF_NONE))

typedef struct sg_event {
    int64_t ts;
    uint32_t res_id;
    uint16_t count;
    uint8_t kind;
    uint8_t flags;
    uint64_t aux;
} sg_event;

/* ---- per-event extension (sg_submit_ex) ---------------------------------------
 * ProcessorSlot.entry(Context, ResourceWrapper, node, count, prioritized, Object... args)
 * (core/slotchain/ProcessorSlot.java:41-50) carries more than an sg_event: the Context -- its
 * name and origin (core/context/Context.java, ContextUtil.enter(name, origin)) -- and every
 * argument.  sg_submit_ex takes one sg_event_ext per event next to the events, and a flat
 * argument table.  An EXIT/TRACE's ext names the origin and context of its ENTRY (the Entry
 * carries its Context); an EXIT's args are those of Entry.exit(count, args). */
enum {
    SG_ARG_NULL = 0,   /* args[i] == null: param rules on index i pass (ParamFlowChecker.java:59-62) */
    SG_ARG_SCALAR = 1, /* key = the interned value (sg_param_key) */
    SG_ARG_LIST = 2    /* a Collection or an array (ParamFlowChecker.java:75-90): its element keys are
                          args_table[key .. key + len), each an SG_ARG_SCALAR / SG_ARG_NULL entry */
};
#define SG_MAX_ARGS 24        /* args per event (and largest paramIdx with a thread-count map + 1) */
#define SG_MAX_CONTEXTS 2000  /* Constants.MAX_CONTEXT_NAME_SIZE (core/Constants.java:35): context ids above it
                                 are ContextUtil's NullContext -- no checks, no statistics (CtSph.java:120-127) */
typedef struct sg_arg {
    uint64_t key;
    uint32_t kind;     /* SG_ARG_* */
    uint32_t len;      /* SG_ARG_LIST: element count */
} sg_arg;

typedef struct sg_event_ext {
    uint32_t origin_id;  /* sg_intern_origin; 0 = "" (no origin) */
    uint32_t context_id; /* sg_intern_context; 0 = sentinel_default_context */
    uint32_t arg_off;    /* args[i] = args_table[arg_off + i], i < n_args */
    uint32_t n_args;     /* <= SG_MAX_ARGS; ENTRY: 0 with SG_F_HAS_ARG = {aux}, 0 without = an empty array */
} sg_event_ext;

/* ---- decisions --------------------------------------------------------------
 * One uint32 per submitted event: status | rule_slot << 8 | wait_ms << 16.
 * rule_slot is the index of the blocking rule inside the resource's compiled
 * rule list of that kind (flow list sorted by FlowRuleComparator, degrade and
 * param lists in java.util.HashSet iteration order). */
enum {
    SG_PASS = 0,          /* entry passed every slot */
    SG_PASS_WAIT = 1,     /* PriorityWaitException: passed after waiting wait_ms (core/slots/block/flow/PriorityWaitException.java) */
    SG_BLOCK_FLOW = 2,    /* FlowException       core/slots/block/flow/FlowSlot.java:154 */
    SG_BLOCK_DEGRADE = 3, /* DegradeException    core/slots/block/degrade/DegradeRuleManager.java:82 */
    SG_BLOCK_PARAM = 4,   /* ParamFlowException  param/slots/block/flow/param/ParamFlowSlot.java:98 */
    SG_NO_CHECK = 5,      /* no slot chain (MAX_SLOT_CHAIN_SIZE), NullContext, or Constants.ON == false */
    SG_BLOCK_UPSTREAM = 6,/* SG_F_BLOCKED_UPSTREAM: SystemBlockException of the caller's SystemSlot (or the
                             AuthorityException of an AuthoritySlot the caller kept) */
    SG_BLOCK_AUTHORITY = 7,/* AuthorityException: the resource's authority rule (sg_load_authority_rules) rejects the
                             entry's origin (core/slots/block/authority/AuthoritySlot.java:48-65); rule slot 0, wait 0 */
    SG_NOT_ENTRY = 0xFF   /* EXIT / TRACE record */
};
#define SG_DECISION_STATUS(d) ((d) & 0xFFu)
#define SG_DECISION_RULE(d) (((d) >> 8) & 0xFFu)
#define SG_DECISION_WAIT(d) ((d) >> 16)

/* ---- per-second metric snapshot (core/node/metric/MetricNode.java:30-42) */
typedef struct sg_metric_node {
    int64_t timestamp;
    int64_t pass_qps;
    int64_t block_qps;
    int64_t success_qps;
    int64_t exception_qps;
    int64_t rt;               /* rt / success (integer division) or raw rt when success == 0 */
    int64_t occupied_pass_qps;
    uint32_t res_id;
    uint32_t reserved;
} sg_metric_node;

/* ---- node state read-back (parity tests) ------------------------------- */
typedef struct sg_bucket {
    int64_t window_start;     /* -1 = bucket never created */
    int64_t pass, block, exception, success, rt, occupied_pass;
    int64_t min_rt;
} sg_bucket;

typedef struct sg_node_state {
    sg_bucket second[8];      /* rollingCounterInSecond buckets, slot order (sample_count used) */
    sg_bucket minute[60];     /* rollingCounterInMinute buckets, slot order */
    sg_bucket borrow[8];      /* FutureBucketLeapArray of the second window */
    int32_t cur_thread_num;
    int32_t has_chain;        /* CtSph chainMap membership */
    int64_t reserved[3];
} sg_node_state;

/* ---- token server (csrv/flow/ClusterFlowChecker.java:55-112) ---------- */
typedef struct sg_token_req {
    int64_t ts;
    int64_t flow_id;
    int32_t acquire_count;
    int32_t prioritized;
} sg_token_req;

typedef struct sg_param_token_req { /* ParamFlowRequestData (flowId, count, params) */
    int64_t ts;
    int64_t flow_id;
    int32_t acquire_count;
    uint32_t n_values;
    uint64_t value_off;
} sg_param_token_req;

enum { /* TokenResultStatus (sentinel-core .../cluster/TokenResultStatus.java) */
    SG_TOKEN_BAD_REQUEST = -4,
    SG_TOKEN_TOO_MANY_REQUEST = -2,
    SG_TOKEN_FAIL = -1,
    SG_TOKEN_OK = 0,
    SG_TOKEN_BLOCKED = 1,
    SG_TOKEN_SHOULD_WAIT = 2,
    SG_TOKEN_NO_RULE_EXISTS = 3
};

typedef struct sg_token_result {
    int32_t status;
    int32_t remaining;
    int32_t wait_in_ms;
    int32_t reserved;
} sg_token_result;

typedef struct sg_engine sg_engine;

/* ---- entry points ------------------------------------------------------- */

/* Fill *cfg with the reference defaults listed above. */
void sg_config_default(sg_config* cfg);

/* Create an engine on cfg->device.  Replaces the static state owned by
 * CtSph.chainMap (core/CtSph.java:52), ClusterBuilderSlot.clusterNodeMap
 * (core/slots/clusterbuilder/ClusterBuilderSlot.java:60) and the rule managers. */
int sg_engine_create(const sg_config* cfg, sg_engine** out);
int sg_engine_destroy(sg_engine* e);

/* Resource interning: name -> dense id (idempotent).  Replaces the
 * StringResourceWrapper keyed maps (core/slotchain/ResourceWrapper.java:46-60). */
int sg_register_resources(sg_engine* e, const char* const* names, uint32_t n, uint32_t* out_ids);
int sg_resource_id(sg_engine* e, const char* name, uint32_t* out_id);

/* Rule managers.  Same validation, de-duplication and ordering as
 * FlowRuleManager.loadRules (core/slots/block/flow/FlowRuleManager.java:97-99,
 * FlowRuleUtil.java:89-228), DegradeRuleManager.loadRules
 * (core/slots/block/degrade/DegradeRuleManager.java:112-205) and
 * ParamFlowRuleManager.loadRules (param/.../ParamFlowRuleManager.java:56-166).
 * Loading a list equal to the current one is a no-op (DynamicSentinelProperty
 * .updateValue, core/property/DynamicSentinelProperty.java:49-52); any other
 * list replaces the rules with fresh controller/breaker state.  *n_loaded
 * (optional) receives the number of valid rules kept.  A load that is refused
 * for its size (SG_ENOTSUP: a 17th rule on one resource, SG_ECAPACITY: more
 * than cfg.max_rules) leaves the engine as it was, but for the resource names
 * it registered: the old rules of every kind go on deciding on their state. */
int sg_load_flow_rules(sg_engine* e, const sg_flow_rule* rules, uint32_t n, uint32_t* n_loaded);
int sg_load_degrade_rules(sg_engine* e, const sg_degrade_rule* rules, uint32_t n, uint32_t* n_loaded);
int sg_load_param_rules(sg_engine* e, const sg_param_rule* rules, uint32_t n, uint32_t* n_loaded);

/* AuthorityRuleManager.loadRules (core/slots/block/authority/AuthorityRuleManager.java:105-157): a rule is valid
 * iff its resource and its limit_app are not blank and strategy >= 0; the first valid rule of a resource in list
 * order is kept, later ones are ignored; *n_loaded (optional) receives the number kept.  n == 0 (rules may be NULL)
 * clears the rules; an equal list is a no-op; the rules do not count against cfg.max_rules.  The check is
 * AuthorityRuleChecker.passCheck (AuthorityRuleChecker.java:30-65) on the origin of the entry's sg_event_ext: the
 * empty origin passes; otherwise BLACK blocks an origin that equals one of limit_app.split(","), WHITE one that
 * equals none.  It runs where AuthoritySlot sits: after the entry's param rules and after SG_F_BLOCKED_UPSTREAM,
 * before the first flow rule; a blocked entry is SG_BLOCK_AUTHORITY and is counted as any blocked entry.  A resource
 * with blocked entries keeps its cooperative owner, as with SG_F_BLOCKED_UPSTREAM (what stays on a lane: see there;
 * also an origin id >= 2^20).  Loading
 * interns no origin: a listed name takes effect once sg_intern_origin has given it an id. */
int sg_load_authority_rules(sg_engine* e, const sg_authority_rule* rules, uint32_t n, uint32_t* n_loaded);

/* Interns a parameter value exactly as ParamFlowRuleUtil.parseItemValue would
 * type it (param/.../ParamFlowRuleUtil.java:85-121): the key of Integer 1 differs
 * from the key of Long 1 and of String "1".  The Java binding calls this (or an
 * equivalent pure function) for args[0] of every entry. */
int sg_param_key(sg_engine* e, const char* value, const char* class_type, uint64_t* out_key);

/* Exact parameter keys.  sg_param_key is a pure function, and for three kinds of value its 64-bit word is a
 * hash: Strings (and every class turned into text), longs outside +-2^59 and doubles.  Two such values can
 * share a word and then share a token bucket, which ParamFlowChecker's equals()-compared maps never do
 * (param/.../ParameterMetric.java:88-104).  sg_param_intern types the value the same way and gives equal keys
 * only for equal values (String: the bytes; Long: the parsed value; Double: Double.equals -- bit equality,
 * 0.0 != -0.0, one NaN): the engine keeps a dictionary of the hashed values in use.  A value that collides
 * with nothing gets the word sg_param_key gives, so callers of either function interoperate; the other kinds
 * hold their value in the key and are returned as sg_param_key returns them.  A NULL value gives key 0.
 * sg_param_intern(_batch) may be called from any number of threads, also while batches are submitted.
 * sg_load_param_rules interns and pins the hot items of the loaded rules (local and cluster), so two hot items
 * whose words collide keep their own thresholds.  Keys of the intern path belong to the engine that gave them.
 *
 * The dictionary is bounded like the reference's LRU maps: sg_param_keys_sweep drops the entries the device no
 * longer holds.  The epoch rule: the engine has an epoch, starting at 0, and every entry remembers the epoch of
 * its last intern (insert or hit).  A sweep waits for every submitted batch, then sets E = epoch and
 * epoch = E + 1.  Its candidates are the unpinned entries last interned before E.  The device marks the
 * candidates whose key is a live key of a ParameterMetric map (rule maps and thread-count maps), a word of the
 * ENTRY key ring, or the key of a claimed (flow, value) slot of the token server.  The unmarked candidates are
 * dropped, unless an intern hit them while the device was scanning; a dropped value that returns is interned
 * anew (its pure key, if that is free again).
 * Caller contract: a key may be used in events (and token requests) submitted before the start of the second
 * sweep that follows the intern call that returned it.  Sweep at a period far above the time a key spends
 * between its intern and its submit (the Java binding: 60 s by default).  Call sg_param_keys_sweep from the
 * thread that submits.
 *
 * sg_param_keys_stats writes up to cap values and returns how many (as sg_last_timings does): [0] entries,
 * [1] entries whose key is not their pure key, [2] pinned entries, [3] sweeps so far, and of the last sweep
 * [4] candidates, [5] candidates the device held, [6] entries dropped, [7] its duration in microseconds. */
int sg_param_intern(sg_engine* e, const char* value, const char* class_type, uint64_t* out_key);
int sg_param_intern_batch(sg_engine* e, const char* const* values, const char* const* class_types, uint32_t n,
                          uint64_t* out_keys);
int sg_param_keys_sweep(sg_engine* e);
int sg_param_keys_stats(sg_engine* e, uint64_t* out, int cap);

/* Decide a batch: the ProcessorSlot chain Statistic -> ParamFlow -> Flow ->
 * Degrade (param/slots/HotParamSlotChainBuilder.java:38-51) for every ENTRY,
 * StatisticSlot.exit (core/slots/statistic/StatisticSlot.java:136-173) for every
 * EXIT and ClusterNode.trace (core/node/ClusterNode.java:99-106) for every TRACE,
 * in event order per resource.  ev and out may be host or device pointers
 * (device pointers avoid the PCIe copy).  sg_submit is synchronous.
 *
 * A malformed batch returns SG_EINVAL (sg_last_error() says which): a res_id
 * at or above max_resources, a ts below the one before it, a last ts more than
 * SG_MAX_BATCH_SPAN_MS after the first ("a batch must span less than 2^31 ms"),
 * an EXIT / TRACE whose aux names no earlier ENTRY of its resource, an ext row
 * outside the argument table.  Such a batch is refused whole, before any of it
 * is decided, and refusing it is a no-op: no window, rule state, thread count or
 * parameter map moves and it takes no event indices (out holds nothing of
 * use).  The same batch split where the span ends is accepted.
 *
 * sg_submit_async returns once the batch's group stage is queued; the batch is
 * not checked yet.  The next call that touches the engine -- another submit,
 * sg_sync, a read or a rule load -- first reads that batch's verdict.  If the
 * batch is valid, it is handed to the decide stage and the call goes on.  If not,
 * the call returns that batch's error and does nothing else: the invalid batch
 * is not decided and takes no event indices, and a batch passed to that call is
 * not accepted either, so submit it again.  Flags the decide stage raises were
 * already reported late, by the second call after the submit; this is the same
 * rule one stage earlier.  ev and out stay valid until sg_sync returns. */
int sg_submit(sg_engine* e, const sg_event* ev, uint64_t n, uint32_t* out);
int sg_submit_async(sg_engine* e, const sg_event* ev, uint64_t n, uint32_t* out);
int sg_sync(sg_engine* e);

/* sg_submit with the Context and the full argument list of every event (see sg_event_ext):
 * origin-specific and `other` flow rules select the origin's StatisticNode, STRATEGY_CHAIN rules the
 * DefaultNode of the entry's context (FlowRuleChecker.selectNodeByRequesterAndStrategy,
 * core/slots/block/flow/FlowRuleChecker.java:90-124); param rules check args[paramIdx] with negative
 * indices resolved on first use and Collection/array values checked element by element
 * (ParamFlowSlot.java:65-101, ParamFlowChecker.java:48-99).  ext may be NULL (= sg_submit); args may be
 * NULL when no ext names any.  All pointers may be host or device memory; sync as sg_submit. */
int sg_submit_ex(sg_engine* e, const sg_event* ev, const sg_event_ext* ext, uint64_t n, const sg_arg* args,
                 uint64_t n_args, uint32_t* out);
int sg_submit_ex_async(sg_engine* e, const sg_event* ev, const sg_event_ext* ext, uint64_t n, const sg_arg* args,
                       uint64_t n_args, uint32_t* out);

/* Context names and origins (ContextUtil.enter(name, origin), core/context/ContextUtil.java:118-166):
 * dense ids, in first-intern order; the name "" interns to origin 0 and "sentinel_default_context"
 * to context 0.  Context ids above SG_MAX_CONTEXTS are NullContexts.  Idempotent. */
int sg_intern_origin(sg_engine* e, const char* origin, uint32_t* out_id);
int sg_intern_context(sg_engine* e, const char* context, uint32_t* out_id);

/* Per-second MetricNode export: StatisticNode.metrics() of every ClusterNode
 * (core/node/StatisticNode.java:124-151, core/node/metric/MetricTimerListener.java:39-71).
 * Writes up to cap nodes, *n receives the number of rows there are (a cap below it truncates the output only). */
int sg_snapshot_metrics(sg_engine* e, int64_t now_ms, sg_metric_node* out, uint64_t cap, uint64_t* n);

/* The global inbound node, Constants.ENTRY_NODE: StatisticSlot counts every EntryType.IN entry and its exit on it as
 * well as on the resource's ClusterNode (core/slots/statistic/StatisticSlot.java:72-76, 89-92, 107-110, 158-161).
 * MetricTimerListener writes its metrics() as the row Constants.TOTAL_IN_RESOURCE_NAME of the metric log
 * (core/node/metric/MetricTimerListener.java:48); SystemRuleManager.checkSystem and SystemStatusListener read its
 * second window and thread count.  No decision of the engine reads it.
 *
 * sg_track_inbound: tracking is off by default, and an engine on which this is never called does what it did without
 * it.  on = 1 is accepted only before the engine has accepted its first batch (SG_ESTATE afterwards: the entries of
 * later exits would never have been counted); on = 0 at any time: counting stops, the node stays readable.  The same
 * value twice is a no-op.  While tracking is on, the events without SG_F_ENTRY_OUT update the node from their final
 * verdicts: an ENTRY of status SG_PASS adds pass += count and one thread, SG_PASS_WAIT the thread alone
 * (StatisticSlot.java:82-92), a blocked one (status 2, 3, 4, 6, 7) block += count, SG_NO_CHECK nothing; an effective
 * EXIT (the ClusterNode's rule) adds success += count, rt += the clipped rt once, minRt, and takes one thread; a TRACE
 * nothing.  Exception and occupied pass stay 0 and the borrow ring stays empty.  A refused batch leaves the node as
 * it was.
 * sg_read_inbound_node waits for every batch like sg_read_node and fills the same struct (has_chain = 1);
 * SG_ESTATE if tracking was never turned on.
 * sg_inbound_metrics is a read-back (no bucket of the node is created or reset): [0] passQps [1] blockQps
 * [2] successQps [3] exceptionQps [4] totalQps [5] avgRt [6] minRt [7] maxSuccessQps [8] curThreadNum at now_ms
 * (core/node/StatisticNode.java:153-260).  Writes up to cap values and returns how many (0 on an error).
 * With tracking on, sg_snapshot_metrics appends the node's metrics() rows after the ClusterNodes' rows, with
 * res_id = SG_RES_TOTAL_INBOUND; the node has a lastFetchTime of its own. */
#define SG_RES_TOTAL_INBOUND 0xFFFFFFFFu                      /* res_id of the node's sg_metric_node rows */
#define SG_TOTAL_IN_RESOURCE_NAME "__total_inbound_traffic__" /* Constants.TOTAL_IN_RESOURCE_NAME */
int sg_track_inbound(sg_engine* e, int32_t on);
int sg_read_inbound_node(sg_engine* e, int64_t now_ms, sg_node_state* out);
int sg_inbound_metrics(sg_engine* e, int64_t now_ms, double* out, int cap);

/* Batched TokenService.requestToken (core/cluster/TokenService.java:26-35,
 * csrv/flow/DefaultTokenService.java:37-48).  Rules come from the flow rules
 * loaded with cluster_mode=1 (the ClusterFlowRuleManager role).  reqs / out may be host or device
 * memory; the call returns when the results are written. */
int sg_cluster_set_connected_count(sg_engine* e, int64_t flow_id, int32_t connected);
int sg_cluster_request_tokens(sg_engine* e, const sg_token_req* reqs, uint64_t n, sg_token_result* out);

/* Embedded token server: ClusterStateManager's server state (core/cluster/ClusterStateManager.java).  Off (the
 * default), a cluster_mode flow rule is decided as in a process that is neither token client nor token server
 * (FlowRuleChecker.passClusterCheck, core/slots/block/flow/FlowRuleChecker.java:126-143): without
 * cluster_fallback_to_local it limits nothing.  On, this engine is the TokenService of its own decision path
 * (pickClusterService -> EmbeddedClusterTokenServerProvider.getServer(), :155-163): every ENTRY that reaches FlowSlot
 * on a resource whose flow rule is a cluster rule -- it has a chain, Constants.ON is set, it is not in a
 * NullContext, and neither SG_F_BLOCKED_UPSTREAM nor the authority rule blocked it -- issues
 * requestToken(flowId, count, prioritized) at its own ts, and obeys the answer (applyTokenResult, :165-187):
 *   OK            FlowSlot passes, DegradeSlot follows
 *   SHOULD_WAIT   passes after waitInMs: SG_PASS with the wait in bits 16.. (0 if a breaker then blocks); only a
 *                 prioritized entry can get it
 *   BLOCKED       SG_BLOCK_FLOW with the rule's slot; StatisticSlot counts the block
 *   TOO_MANY_REQUEST, BAD_REQUEST (count 0), FAIL, NO_RULE_EXISTS   fallbackToLocalOrPass: the entry passes
 * Tokens are consumed whatever DegradeSlot decides.  The token state is the one sg_cluster_request_tokens serves:
 * calls and batches take effect in call order, a batch's requests in event order; a rejected batch consumes nothing.
 * Supported shape: the cluster rule is the only flow rule of its resource, QPS grade, limitApp "default", strategy
 * DIRECT, without cluster_fallback_to_local, with a flowId no other loaded flow rule uses; the resource has no
 * param rules and is in no STRATEGY_RELATE component; degrade and authority rules are free.  While the mode is on,
 * a flow- or param-rule load that would leave a cluster flow rule outside this shape returns SG_ENOTSUP, and so
 * does switching the mode on over such rules: sg_last_error names the rule and nothing has changed.  Cluster-mode
 * param rules keep their behaviour (no TokenService on the decision path) in either mode.  The call drains the
 * pipeline and compiles the programs again; node, breaker and token state stay.  A batch that holds events of such
 * resources is handed to the decide stage before the next batch is grouped (it gives up the pipeline's overlap),
 * and synchronous batches of at most 256 events take the batched path while such a rule is loaded. */
int sg_cluster_embedded(sg_engine* e, int32_t on);

/* Batched TokenService.requestParamToken (core/cluster/TokenService.java:37-46,
 * csrv/flow/DefaultTokenService.java:50-61 -> csrv/flow/ClusterParamFlowChecker.java:42-88).
 * Rules come from the param rules loaded with cluster_mode=1 (the ClusterParamFlowRuleManager role,
 * csrv/flow/rule/ClusterParamFlowRuleManager.java:318-369).  Request i names its parameter values
 * as values[value_off, value_off + n_values): interned 64-bit keys (sg_param_key).  Requests are
 * time-ordered and share the namespace's GlobalRequestLimiter with sg_cluster_request_tokens.
 * reqs, values and out may each be host or device memory; the call returns when the results are
 * written.  A value range outside values[0, n_values) or unordered ts returns SG_EINVAL, a call whose
 * values cannot fit the value table SG_ENOMEM; either leaves the limiter, the windows and the table
 * as they were.  The flow stage is decided with one lane per (flowId, value) chain across the device;
 * for a call, a flow with a request of more than one value, or whose first request lies before one
 * of its window starts (the clock went back between calls), is decided by one lane in request order
 * instead (SG_PTOK_VP=0: every flow).  The decisions are the same either way. */
int sg_cluster_request_param_tokens(sg_engine* e, const sg_param_token_req* reqs, uint64_t n, const uint64_t* values,
                                    uint64_t n_values, sg_token_result* out);

/* The value table behind sg_cluster_request_param_tokens: one slot per (flowId, value) with a count and a window
 * stamp per bucket.  The reference clears a bucket's value map on every window reset
 * (csrv/flow/statistic/metric/ClusterParameterLeapArray.java:30-58), so ClusterParamMetric.getSum
 * (ClusterParamMetric.java:53-85) sees the values of the last windowIntervalMs only; here a slot is dead, and is
 * dropped by the next rehash or rule load, once none of its stamps equals its flow's stamp of the same bucket
 * (stamps only move forward and a count is read only under an equal stamp, so a dead slot adds 0 to every sum).
 * The table starts at 2^SG_PV_LOG2 slots (default 17) and is rehashed on the device, before a call's first
 * kernel, whenever the slots claimed so far plus the values the call lists would pass half of it: into the
 * smallest power of two that leaves at most a quarter claimed, up to 2^SG_PV_MAX_LOG2 slots (default 24: 4.5 GB of
 * 272-byte slots; the move needs the old and the new table at once, and a rehash that kept the capacity keeps the
 * old table as the next one's target).  A call that cannot fit half of the maximum
 * returns SG_ENOMEM before anything changed: the limiter, the flows' windows and the table are as they were.
 * sg_cluster_param_table_stats writes up to cap values and returns how many (as sg_param_keys_stats does):
 * [0] capacity in slots, [1] upper bound on the claimed slots (exact after a rehash or a rule load, plus the values
 * listed since), [2] live slots kept by the last rehash, [3] rehashes, [4] rehashes that changed the capacity,
 * [5] device time of the last rehash in microseconds (count and move, HIP events), [6] maximum capacity,
 * and, cumulative over the engine's calls (a refused call changes none): [7] flow-stage requests decided by the
 * value-parallel owner, [8] by the one-lane-per-flow owner, [9] flows the latter kept for a call because of a
 * multi-value request or a clock gone back. */
int sg_cluster_param_table_stats(sg_engine* e, uint64_t* out, int cap);

/* Namespaces of the token server (csrv/flow/statistic/limit/GlobalRequestLimiter.java:30-80,
 * csrv/flow/rule/ClusterFlowRuleManager.java:308-317): every namespace has a RequestLimiter of its own and a
 * connected-client count of its own, and a token request tries the limiter of its flowId's namespace only
 * (csrv/flow/ClusterFlowChecker.java:50-53, ClusterParamFlowChecker.java:37-40).  The namespace "default"
 * (ServerConstants.DEFAULT_NAMESPACE) always exists with id 0 and the limit cfg.cluster_max_allowed_qps, and a
 * flowId that was never assigned belongs to it: an engine on which none of these calls is made has one limiter. */
#define SG_MAX_NAMESPACES 1024

/* Register ns (idempotent; *out_ns_id, optional, receives its dense id), or change the limit of a registered
 * namespace, which keeps its window (RequestLimiter.setQpsAllowed).  max_allowed_qps < 0: no limiter, every
 * request passes it.  NULL or "": SG_EINVAL; more than SG_MAX_NAMESPACES namespaces: SG_ECAPACITY. */
int sg_cluster_namespace(sg_engine* e, const char* ns, double max_allowed_qps, uint32_t* out_ns_id);

/* flowIds of ns, for cluster flow rules and cluster param rules alike, loaded now or at any later load.
 * Unregistered ns: SG_ENOTFOUND; a flow_id <= 0: SG_EINVAL; a flowId of another namespace: SG_ESTATE
 * (nothing is assigned then; the same namespace again is a no-op). */
int sg_cluster_assign_flows(sg_engine* e, const char* ns, const int64_t* flow_ids, uint32_t n);

/* ConnectionManager.getConnectedCount(namespace): the count of every loaded flow of ns, and the count a flow
 * of ns loaded later starts with.  A later per-flow call overrides it for that flow (the last call wins). */
int sg_cluster_set_namespace_connected(sg_engine* e, const char* ns, int32_t connected);

/* GlobalRequestLimiter.getCurrentQps / getMaxAllowedQps of ns (GlobalRequestLimiter.java:57-71): the sum of the
 * limiter's buckets valid at now_ms over one second, and the limit (negative: none).  A read-back: no bucket
 * is created or reset.  Either out pointer may be NULL. */
int sg_cluster_namespace_qps(sg_engine* e, const char* ns, int64_t now_ms, double* current_qps,
                             double* max_allowed_qps);

/* Cluster metrics of the token server: what cluster/server/metricList answers, one ClusterMetricNode a flowId
 * (csrv/flow/statistic/ClusterMetricNodeGenerator.java:39-105, metric/ClusterMetric.java:53-72,
 * metric/ClusterParamMetric.java:91-133, csrv/server/command/handler/FetchClusterMetricCommandHandler.java).
 * Rows: the cluster flow rules' flowIds ascending (kind SG_CM_FLOW: pass_qps / block_qps = getAvg(PASS) /
 * getAvg(BLOCK) at now_ms), then the cluster param rules' flowIds ascending (kind SG_CM_PARAM: the top_n values of
 * largest window sum > 0 with top_qps = sum / (windowIntervalMs / 1000.0), ordered by the 64-bit sum descending and
 * among equal sums by the key ascending, unsigned).  A flow without traffic has a row of zeros.  ns NULL or "":
 * every flow; otherwise the flows of that namespace only (an unassigned flowId belongs to "default"; an
 * unregistered ns: SG_ENOTFOUND).  top_n outside 1..SG_CLUSTER_TOP_MAX: SG_EINVAL (the reference asks for 5).
 * out is host memory; up to cap rows are written and *n receives the number of rows there are.
 * A read-back: no bucket is created or reset, no stamp moves and no slot is claimed, so every later request is
 * decided as it would have been without the call.  The reset that the reference's getAvg / getTopValues apply
 * through currentWindow() is applied to a copy: with w = interval / sampleCount, i = (now / w) % sampleCount and
 * ws = now - now % w, bucket i counts as empty if its start is < ws (a FLOW metric's emptied copy of an existing
 * bucket starts with the pending occupy transfer, PASS += the occupied pass count), a bucket never created or with a
 * start >= ws is taken as it is, and then every bucket with now - start > interval is left out.  A value's sum adds
 * its counts of the buckets that survive this and whose stamp equals the flow's.  The reference's cap of 4,000
 * values per bucket map is not applied.  The table scan and the per-flow selection run on the device, on the
 * engine's stream; the first call allocates their scratch, sized by the value table's capacity, and keeps it. */
#define SG_CLUSTER_TOP_MAX 8
enum { SG_CM_FLOW = 0, SG_CM_PARAM = 1 };
typedef struct sg_cluster_metric {      /* ClusterMetricNode */
    int64_t  timestamp;                 /* now_ms */
    int64_t  flow_id;
    uint32_t res_id;                    /* the rule's resource */
    uint32_t kind;                      /* SG_CM_FLOW / SG_CM_PARAM */
    double   pass_qps, block_qps;       /* FLOW: getAvg(PASS), getAvg(BLOCK); PARAM: 0 */
    int64_t  rt;                        /* always 0: the reference never sets it */
    uint32_t n_top, reserved;           /* PARAM: entries used below; FLOW: 0 */
    uint64_t top_key[SG_CLUSTER_TOP_MAX];
    double   top_qps[SG_CLUSTER_TOP_MAX];
} sg_cluster_metric;
int sg_cluster_metrics(sg_engine* e, const char* ns, int64_t now_ms, uint32_t top_n, sg_cluster_metric* out,
                       uint64_t cap, uint64_t* n);

/* The value behind a parameter key, the inverse of sg_param_key / sg_param_intern: class_type receives the class
 * name ("java.lang.String", "int", "long", "double", "float", "byte", "short", "boolean", "char"), value the
 * value's text, both NUL-terminated; returns the text's length (>= 0).  The kinds whose key holds the value (int,
 * long within +-2^59, float, byte, short, boolean, char) are decoded from the key; a hashed kind (String, double,
 * a long outside +-2^59) is looked up in the engine's dictionary (callable from any thread) and returns
 * SG_ENOTFOUND when no entry owns the key, as for a key the pure function made.  A negative long in range and a
 * hashed long share their key space: the dictionary is asked first.  A buffer too small: SG_EINVAL.  The key sweep
 * keeps the keys of claimed (flowId, value) slots, so a key that the metrics call returns resolves. */
int sg_param_key_value(sg_engine* e, uint64_t key, char* class_type, size_t class_cap, char* value,
                       size_t value_cap);

/* Node read-back for parity tests: the ClusterNode of res_id. */
int sg_read_node(sg_engine* e, uint32_t res_id, int64_t now_ms, sg_node_state* out);

/* ParameterMetric.getThreadCount(paramIdx, value) of res_id (param/ParameterMetric.java:233-241): the value's
 * thread count in the resource's thread-count map of paramIdx, 0 when the map or the value is absent; *present
 * (optional) tells the two apart.  A read-back: unlike CacheMap.get it does not move the value in the LRU order. */
int sg_param_thread_count(sg_engine* e, uint32_t res_id, int32_t param_idx, uint64_t key, int64_t* count,
                          int32_t* present);

/* Last error message of the calling thread ("" if none). */
const char* sg_last_error(void);

/* Timing of the most recent sg_submit's device stages (HIP events on the engine
 * stream), in ms: [0] group (sort, segments, records, chain grants), [1] decide
 * (every decide kernel, forked over streams and joined), [2] post (decisions back
 * to submission order), [3] their sum; returns the number of values written. */
int sg_last_timings(sg_engine* e, double* ms, int cap);

#ifdef __cplusplus
}
#endif
#endif /* SENTINEL_GPU_H */
