// compile.h -- the rule compiler: the managers' host lists (rules.h) to the device tables -- one Prog a resource,
// the DRule / RState / DHot arrays and the STRATEGY_RELATE component table -- and with them the owner of every
// resource: the PF_* / XF_* / PX_* bits say which decide kernel implements the resource's rules.
//
// Host only: no HIP call and no engine (tests/rules_host.cpp compiles known programs on the CPU).  The engine's
// upload_rules reads the old state back, calls compile_rules and carry_state, and copies the result to the device.
// What the compiler refuses for its size, and what the embedded token server refuses for its shape, the loaders ask
// beforehand with the same functions (rule_limits, emb_refuse), so that a refused load leaves the engine untouched.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/sentinel_gpu.h"
#include "dev_types.h"
#include "rules.h"

namespace sg {

// The three managers' lists: the kept records and every resource's rules in compiled order.
struct RuleLists {
    const std::vector<ParamR>& params;
    const std::vector<std::vector<int>>& res_par;
    const std::vector<FlowR>& flows;
    const std::vector<std::vector<int>>& res_flow;
    const std::vector<DegR>& degs;
    const std::vector<std::vector<int>>& res_deg;
};

// What the compiler reads of the engine.
struct CompileEnv {
    const std::vector<std::string>& names;                          // resource id -> name
    const std::unordered_map<std::string, uint32_t>& ids;          // resource name -> id
    const std::unordered_map<std::string, uint32_t>& origin_ids;   // interned origins
    const std::unordered_map<std::string, uint32_t>& context_ids;  // interned contexts
    const std::vector<uint32_t>& tm_base;                           // per resource: Prog.tm_base
    const std::unordered_map<uint32_t, uint32_t>& pmap_index;      // param state id -> map index
    const std::map<std::string, uint32_t>& psid_of;                // "res\x00eqkey" -> param state id
    const std::set<uint64_t>& tmaps;                                // thread-count maps: res << 8 | paramIdx
    uint32_t max_resources, max_rules;
    int32_t cold_factor;
    bool mix_on, mix_pq, pv_on, pv_pq, emb_on;
};

struct Compiled {
    int err = SG_OK;  // SG_ENOTSUP / SG_ECAPACITY with msg: a size refusal, nothing else is filled in
    std::string msg;
    std::vector<Prog> prog;    // [max_resources]
    std::vector<DRule> rules;
    std::vector<RState> rst;   // initial states
    std::vector<DHot> hot;
    std::vector<uint32_t> comp;     // [max_resources] STRATEGY_RELATE component representative; empty: no pair
    std::vector<uint32_t> members;  // the resources of the components, sorted
    std::vector<std::pair<uint32_t, int64_t>> emb_res;  // embedded mode: the XF_EMB resources and their flowIds
    bool any_mix = false, any_head = false, any_multi = false;
};

// CacheMap capacity of a rule's time/token maps (ParameterMetric.initialize, ParameterMetric.java:87-104)
inline uint32_t rule_map_cap(int64_t duration_sec) {
    const int64_t c = (int64_t)PM_BASE_CAP * std::max<int64_t>(duration_sec, 1);
    return (uint32_t)std::min<int64_t>(c, PM_TOTAL_CAP);
}

// Embedded token server: the supported shape of a cluster flow rule, in one place for the refusals (emb_refuse) and
// the compile (compile_rules marks XF_EMB exactly where why() finds nothing to object to).  A resource holding a
// cluster-mode flow rule must have that rule as its only flow rule -- QPS grade (flow_valid has dropped a rule without
// a flowId), limitApp "default", strategy DIRECT, a flowId no other loaded flow rule uses -- no param rules, and no
// RELATE rule of another resource may name it: then the batch's requests depend on no verdict the batch still has to
// find.  A rule with cluster_fallback_to_local is outside it too: the local check of a refused request is not built.
struct EmbShape {
    std::unordered_map<long long, int> uses;  // flowId -> cluster flow rules naming it
    std::set<std::string> related;            // resources of a STRATEGY_RELATE pair
    explicit EmbShape(const std::vector<FlowR>& flows) {
        for (const FlowR& f : flows) {
            if (f.r.cluster_mode) ++uses[(long long)f.r.cluster_flow_id];
            if (f.r.strategy == SG_STRATEGY_RELATE && !f.ref.empty() && f.ref != f.res) { related.insert(f.ref); related.insert(f.res); }
        }
    }
    // why the cluster rule f of resource r lies outside the shape (null: it is eligible)
    const char* why(const FlowR& f, size_t r, const std::vector<std::vector<int>>& res_flow,
                    const std::vector<std::vector<int>>& res_par) const {
        if (r >= res_flow.size() || res_flow[r].size() != 1) return "it is not the only flow rule of its resource";
        if (f.r.grade != SG_FLOW_GRADE_QPS) return "it is not QPS grade";
        if (f.la != "default") return "its limitApp is not \"default\"";
        if (f.r.strategy != SG_STRATEGY_DIRECT) return "its strategy is not DIRECT";
        auto it = uses.find((long long)f.r.cluster_flow_id);
        if (it == uses.end() || it->second != 1) return "another flow rule uses its flowId";
        if (r < res_par.size() && !res_par[r].empty()) return "its resource has param rules";
        if (related.count(f.res)) return "its resource is in a STRATEGY_RELATE component";
        if (f.r.cluster_fallback_to_local) return "cluster_fallback_to_local is not decided in embedded mode";
        return nullptr;
    }
};

// What the mode cannot decide, told from the host lists alone, before anything of the engine changes (SG_ENOTSUP, msg
// names the rule; the caller returns it and nothing has changed).
inline int emb_refuse(const std::vector<FlowR>& flows, const std::vector<std::vector<int>>& res_flow,
                      const std::vector<std::vector<int>>& res_par, std::string& msg) {
    const EmbShape shape(flows);
    for (size_t r = 0; r < res_flow.size(); ++r)
        for (int i : res_flow[r]) {
            const FlowR& f = flows[i];
            if (!f.r.cluster_mode) continue;
            if (const char* why = shape.why(f, r, res_flow, res_par)) {
                msg = "embedded token server: cluster flow rule " + std::to_string((long long)f.r.cluster_flow_id) +
                      " on " + f.res + " is outside the supported shape: " + why;
                return SG_ENOTSUP;
            }
        }
    return SG_OK;
}

// A param rule that only initialises its metric: cluster mode + QPS without fallback -- passClusterCheck finds no
// TokenService in this process and passes (ParamFlowSlot.initHotParamMetricsFor still runs)
inline bool param_init_only(const sg_param_rule& q) {
    return q.cluster_mode && q.grade == SG_FLOW_GRADE_QPS && !q.cluster_fallback_to_local;
}
// A cluster flow rule without fallback compiles to no flow stage (no TokenService -> pass)
inline bool flow_cluster_only(const sg_flow_rule& f) { return f.cluster_mode && !f.cluster_fallback_to_local; }

// The DRules resource r compiles to: its param rules, a run of PB_INIT_ONLY rules with fixed indices being one
// pseudo-rule; its flow rules but the cluster-only ones; its degrade rules.  (The compiler joins a rule to the DRule
// before it when that one's behavior byte is PB_INIT_ONLY, which a local rule with control_behavior 255 has too: there
// this count is one above what is emitted, never below.)
inline size_t compiled_rule_count(const RuleLists& L, size_t r) {
    size_t n = r < L.res_deg.size() ? L.res_deg[r].size() : 0;
    bool run = false;  // the last compiled param rule is a PB_INIT_ONLY pseudo-rule with a fixed index
    if (r < L.res_par.size())
        for (int i : L.res_par[r]) {
            const sg_param_rule& q = L.params[i].r;
            const bool init = param_init_only(q);
            if (init && q.param_idx >= 0 && run) continue;  // joins the pseudo-rule before it
            run = init && q.param_idx >= 0;
            ++n;
        }
    if (r < L.res_flow.size())
        for (int i : L.res_flow[r])
            if (!flow_cluster_only(L.flows[i].r)) ++n;
    return n;
}

// What the compiler refuses for its size -- more than 16 compiled rules on one resource, more than max_rules in all.
// compile_rules starts with it; the loaders call it with the lists they are about to publish, before they change
// anything of the engine: a load refused for its size leaves the engine as it was.
inline int rule_limits(const RuleLists& L, const CompileEnv& env, std::string& msg) {
    size_t total = 0;
    const size_t nres = std::min<size_t>(env.names.size(), env.max_resources);
    for (size_t r = 0; r < nres; ++r) {
        const size_t n = compiled_rule_count(L, r);
        if (n > 16) { msg = "more than 16 rules on one resource: " + env.names[r]; return SG_ENOTSUP; }
        total += n;
    }
    if (total > env.max_rules) { msg = "compiled rule table exceeds max_rules"; return SG_ECAPACITY; }
    return SG_OK;
}

// Build the device rule program of every resource from the compiled host lists.  The tables alone, whatever their
// size: compile_rules below refuses first (tests/rules_host.cpp counts here what a refused list would emit).
inline Compiled compile_tables(const RuleLists& L, const CompileEnv& env) {
    Compiled C;
    uint32_t R = env.max_resources;
    C.prog.resize(R);
    std::vector<Prog>& prog = C.prog;
    std::vector<DRule>& rules = C.rules;
    std::vector<RState>& rst = C.rst;
    std::vector<DHot>& hot = C.hot;
    size_t nres = env.names.size();
    const EmbShape emb_shape(L.flows);                  // XF_EMB is told by the shape test the refusals use
    std::vector<std::pair<uint32_t, uint32_t>> relate;  // (resource, referenced resource) of RELATE rules
    for (size_t r = 0; r < nres && r < R; ++r) {
        Prog p;
        std::memset(&p, 0, sizeof(p));
        p.rule_off = (uint32_t)rules.size();
        p.tm_base = r < env.tm_base.size() ? env.tm_base[r] : NO_ID;
        // param rules: HashSet order (ParamFlowSlot.checkFlow iterates them, ParamFlowSlot.java:84-100)
        const auto& pl = r < L.res_par.size() ? L.res_par[r] : std::vector<int>();
        for (size_t i = 0; i < pl.size(); ++i) {
            const ParamR& q = L.params[pl[i]];
            DRule d;
            std::memset(&d, 0, sizeof(d));
            d.kind = RK_PARAM;
            d.grade = (uint8_t)q.r.grade;
            d.behavior = (uint8_t)q.r.control_behavior;
            if (param_init_only(q.r)) {
                d.behavior = PB_INIT_ONLY;
                // a run of such rules with fixed indices is one pseudo-rule: the set of maps it initialises
                if (q.r.param_idx >= 0 && p.n_param && rules.back().behavior == PB_INIT_ONLY &&
                    rules.back().param_idx >= 0) {
                    if (q.r.param_idx < SG_MAX_ARGS) rules.back().burst |= (int32_t)(1u << q.r.param_idx);
                    continue;
                }
            }
            d.slot = (uint8_t)i;
            d.max_queue = q.r.max_queueing_time_ms;
            d.count = q.r.count;
            d.burst = q.r.burst_count;
            if (d.behavior == PB_INIT_ONLY && q.r.param_idx >= 0)  // the pseudo-rule's map set
                d.burst = q.r.param_idx < SG_MAX_ARGS ? (int32_t)(1u << q.r.param_idx) : 0;
            double c = q.r.count;
            d.token_count = (c != c) ? 0 : c >= 2147483647.0 ? INT32_MAX : (int32_t)c;
            d.token_count_l = (c != c) ? 0 : c >= 9.2e18 ? INT64_MAX : (int64_t)c;
            d.duration_sec = q.r.duration_in_sec;
            d.hot_off = (uint32_t)hot.size();
            d.hot_n = (uint32_t)q.hot.size();
            for (auto& h : q.hot) hot.push_back(DHot{h.first, h.second, 0});
            d.pmap = env.pmap_index.at(env.psid_of.at(q.res + std::string("\0", 1) + q.eqkey));
            d.param_idx = q.r.param_idx;
            d.ref = NO_REF;
            rules.push_back(d);
            rst.push_back(RState{0, 0, 0, 0});  // a: paramIdx resolved by applyRealParamIdx + 1 (0 = not yet)
            p.n_param++;
        }
        // flow rules: FlowRuleComparator order; limitApp and strategy pick the node each rule checks
        // (FlowRuleChecker.selectNodeByRequesterAndStrategy, FlowRuleChecker.java:90-124)
        const auto& fl = r < L.res_flow.size() ? L.res_flow[r] : std::vector<int>();
        // FlowRuleManager.isOtherOrigin reads every rule of the resource, the cluster-only ones included
        std::vector<uint32_t> skipped_origins;
        for (size_t i = 0; i < fl.size(); ++i) {
            const FlowR& f = L.flows[fl[i]];
            if (!flow_cluster_only(f.r) || f.la == "default" || f.la == "other") continue;
            auto oi = env.origin_ids.find(f.la);
            if (oi != env.origin_ids.end()) skipped_origins.push_back(oi->second);
        }
        for (size_t i = 0; i < fl.size(); ++i) {
            const FlowR& f = L.flows[fl[i]];
            if (flow_cluster_only(f.r)) continue;
            DRule d;
            std::memset(&d, 0, sizeof(d));
            d.kind = RK_FLOW;
            d.grade = (uint8_t)f.r.grade;
            d.behavior = (uint8_t)(f.r.grade == SG_FLOW_GRADE_QPS ? f.r.control_behavior : SG_CONTROL_BEHAVIOR_DEFAULT);
            if (d.behavior > 3) d.behavior = SG_CONTROL_BEHAVIOR_DEFAULT;
            d.slot = (uint8_t)i;
            d.max_queue = f.r.max_queueing_time_ms;
            d.count = f.r.count;
            d.ref = NO_REF;
            d.la_kind = f.la == "default" ? LA_DEFAULT : f.la == "other" ? LA_OTHER : LA_ORIGIN;
            auto oi = env.origin_ids.find(f.la);
            d.la_origin = oi == env.origin_ids.end() ? NO_ID : oi->second;
            if (d.la_kind == LA_OTHER && !skipped_origins.empty()) {
                d.hot_off = (uint32_t)hot.size();
                d.hot_n = (uint32_t)skipped_origins.size();
                for (uint32_t o : skipped_origins) hot.push_back(DHot{o, 0, 0});
            }
            d.strategy = (uint32_t)f.r.strategy;
            d.chain_ctx = NO_ID;
            if (f.r.strategy == SG_STRATEGY_RELATE) {  // another resource's ClusterNode (same node if itself)
                auto it = env.ids.find(f.ref);
                const uint32_t b = it == env.ids.end() ? NO_REF : it->second;
                if (b != NO_REF && b != (uint32_t)r && b < R) { d.ref = b; relate.emplace_back((uint32_t)r, b); }
            } else if (f.r.strategy == SG_STRATEGY_CHAIN) {  // the DefaultNode of the context named refResource
                if (f.ref == "sentinel_default_context") d.chain_ctx = 0;
                else {
                    auto ci = env.context_ids.find(f.ref);
                    if (ci != env.context_ids.end()) d.chain_ctx = ci->second;
                }
                p.multi |= PX_CHAIN;
            }
            if (d.la_kind != LA_DEFAULT && f.r.strategy == SG_STRATEGY_DIRECT) p.multi |= PX_ORIGIN;
            if (d.la_kind != LA_DEFAULT || f.r.strategy == SG_STRATEGY_CHAIN || f.r.strategy > SG_STRATEGY_CHAIN)
                p.pflags |= PF_SERIAL;  // node selection beyond the ClusterNode: the per-lane kernel
            if (d.behavior == SG_CONTROL_BEHAVIOR_WARM_UP || d.behavior == SG_CONTROL_BEHAVIOR_WARM_UP_RATE_LIMITER) {
                // WarmUpController.construct (WarmUpController.java:100-117)
                int cold = env.cold_factor;
                double c = f.r.count;
                auto d2i = [](double v) -> int32_t {
                    if (v != v) return 0;
                    if (v >= 2147483647.0) return INT32_MAX;
                    if (v <= -2147483648.0) return INT32_MIN;
                    return (int32_t)v;
                };
                int32_t wt = d2i(f.r.warm_up_period_sec * c) / (cold - 1);
                int32_t mt = (int32_t)((uint32_t)wt + (uint32_t)d2i((double)(2 * f.r.warm_up_period_sec) * c / (1.0 + cold)));
                d.warning_token = wt;
                d.max_token = mt;
                d.slope = (cold - 1.0) / c / (double)(mt - wt);
                d.count_div_cold = d2i(c) / cold;
                p.pflags |= PF_WARM;
            }
            rules.push_back(d);
            rst.push_back(RState{0, 0, -1, 0});
            p.n_flow++;
        }
        const auto& dl = r < L.res_deg.size() ? L.res_deg[r] : std::vector<int>();
        for (size_t i = 0; i < dl.size(); ++i) {
            const DegR& g = L.degs[dl[i]];
            DRule d;
            std::memset(&d, 0, sizeof(d));
            d.kind = RK_DEGRADE;
            d.grade = (uint8_t)g.r.grade;
            d.slot = (uint8_t)i;
            d.count = g.r.count;
            d.time_window = g.r.time_window;
            if (g.r.grade == SG_DEGRADE_GRADE_EXCEPTION_COUNT) p.pflags |= PF_EXC_COUNT;
            if (g.r.grade == SG_DEGRADE_GRADE_RT) p.pflags |= PF_RT;
            rules.push_back(d);
            rst.push_back(RState{0, 0, 0, 0});
            p.n_degrade++;
        }
        {  // limits of the cooperative decide kernels (decide.hip JMAX_*); else one lane decides it
            int n_rl = 0;
            for (int i = 0; i < p.n_flow; ++i) {
                uint8_t b = rules[p.rule_off + p.n_param + i].behavior;
                if (b == SG_CONTROL_BEHAVIOR_RATE_LIMITER || b == SG_CONTROL_BEHAVIOR_WARM_UP_RATE_LIMITER) ++n_rl;
            }
            if (n_rl) p.pflags |= PF_RL;
            // param rules beside flow / degrade rules (XF_MIX): QPS DefaultController-style token buckets on
            // paramIdx 0 with LDS-sized maps only -- their verdicts are then a function of earlier checks of the
            // same (rule, value) alone (no THREAD grade: its count moves with full-chain passes; no throttle:
            // its wait would add to the flow stages')
            bool mix = p.n_param >= 1 && p.n_param <= 4 && ((p.n_flow + p.n_degrade) > 0 || env.mix_pq) && !p.multi;
            for (int i = 0; i < p.n_param && mix; ++i) {
                const DRule& d = rules[p.rule_off + i];
                if (d.param_idx < 0) mix = false;
                else if (d.behavior == PB_INIT_ONLY) { if (d.burst & ~1) mix = false; }
                else if (d.param_idx != 0 || d.grade != SG_FLOW_GRADE_QPS ||
                         d.behavior != SG_CONTROL_BEHAVIOR_DEFAULT || rule_map_cap(d.duration_sec) > PQ_MAX_CAP)
                    mix = false;
            }
            if (mix) {  // a thread-count map of another index is k_lane's
                auto it = env.tmaps.lower_bound(((uint64_t)r << 8) | 1);
                if (it != env.tmaps.end() && (*it >> 8) == (uint64_t)r) mix = false;
            }
            if (mix && env.mix_on) { p.xf |= XF_MIX; C.any_mix = true; }
            if ((p.xf & XF_MIX) && p.n_param == 1 && rules[p.rule_off].behavior != PB_INIT_ONLY) p.xf |= XF_PLITE;
            if ((p.n_param && !(p.xf & XF_MIX)) || p.n_flow > 4 || p.n_degrade > 4 || n_rl > 2 || p.multi)
                p.pflags |= PF_SERIAL;
            bool all_default_qps = true;
            for (int i = 0; i < p.n_flow; ++i) {
                const DRule& d = rules[p.rule_off + p.n_param + i];
                if (d.behavior != SG_CONTROL_BEHAVIOR_DEFAULT || d.grade != SG_FLOW_GRADE_QPS) all_default_qps = false;
            }
            if (all_default_qps) p.pflags |= PF_FROZEN;
            // k_pq (param.hip): param rules with a fixed paramIdx and LDS-sized rings, nothing else; QPS-grade
            // rules, and at most one THREAD-grade rule on paramIdx 0 checked last (its check and the entry's
            // thread-count increment are one access of the thread-count map)
            bool pq = p.n_param >= 1 && p.n_param <= 4 && p.n_flow == 0 && p.n_degrade == 0 && !p.multi;
            int last_checked = -1, n_thread = 0, thread_at = -1;
            for (int i = 0; i < p.n_param && pq; ++i) {
                const DRule& d = rules[p.rule_off + i];
                if (d.param_idx < 0) pq = false;
                else if (d.behavior == PB_INIT_ONLY) { if (d.burst & ~1) pq = false; }  // maps on other indices
                else if (d.param_idx != 0) pq = false;  // sg_submit_ex args beyond [0] are k_lane's
                else if (d.grade == SG_FLOW_GRADE_THREAD) { ++n_thread; thread_at = i; last_checked = i; }
                else if (d.grade != SG_FLOW_GRADE_QPS || rule_map_cap(d.duration_sec) > PQ_MAX_CAP) pq = false;
                else last_checked = i;
            }
            if (n_thread > 1 || (n_thread == 1 && thread_at != last_checked)) pq = false;
            if (n_thread) p.xf |= XF_PTHREAD;
            // a thread-count map of another index (an earlier rule set's, kept with the metric) is k_lane's too
            if (pq) {
                auto it = env.tmaps.lower_bound(((uint64_t)r << 8) | 1);
                if (it != env.tmaps.end() && (*it >> 8) == (uint64_t)r) pq = false;
            }
            if (pq && !(p.xf & XF_MIX)) p.pflags |= PF_PQ;
            // one checked QPS rule (DefaultController or throttle), no THREAD grade: the value-parallel passes
            if ((p.pflags & PF_PQ) && env.pv_pq && env.pv_on && p.n_param == 1 && n_thread == 0 &&
                rules[p.rule_off].behavior != PB_INIT_ONLY) {
                p.xf |= XF_PVPQ;
                C.any_mix = true;
            }
            if (p.n_flow <= 2 && p.n_degrade <= 2 && n_rl == 0) p.pflags |= PF_J16;
            // one flow rule and nothing else on the ClusterNode: a THREAD-grade DefaultController or a QPS
            // RateLimiter head is decided by the event-driven head owner (head.hip k_head)
            if (p.n_param == 0 && p.n_flow == 1 && p.n_degrade == 0 && !p.multi && !(p.pflags & PF_SERIAL)) {
                const DRule& d = rules[p.rule_off];
                if (d.strategy == SG_STRATEGY_DIRECT && d.la_kind == LA_DEFAULT) {
                    if (d.grade == SG_FLOW_GRADE_THREAD && d.behavior == SG_CONTROL_BEHAVIOR_DEFAULT) p.xf |= XF_HEADT;
                    else if (d.grade == SG_FLOW_GRADE_QPS && (d.behavior == SG_CONTROL_BEHAVIOR_RATE_LIMITER ||
                                                              (d.behavior == SG_CONTROL_BEHAVIOR_WARM_UP_RATE_LIMITER && d.count > 0)))
                        p.xf |= XF_HEADR;
                }
                if (p.xf & (XF_HEADT | XF_HEADR)) C.any_head = true;
            }
        }
        // Embedded token server: the resource's only flow rule is a cluster rule this engine counts the tokens of
        // (emb_refuse has refused every other shape while the mode is on).  The program is what the rule compiles to
        // without a TokenService -- no flow stage, the breakers as usual -- plus the flag: the batch's token call
        // decides the rule (decide_enqueue)
        if (env.emb_on && fl.size() == 1 && p.n_flow == 0) {
            const FlowR& f = L.flows[fl[0]];
            if (f.r.cluster_mode && !emb_shape.why(f, r, L.res_flow, L.res_par)) {
                p.xf |= XF_EMB;
                C.emb_res.emplace_back((uint32_t)r, (int64_t)f.r.cluster_flow_id);
            }
        }
        prog[r] = p;
    }
    // STRATEGY_RELATE components (co-locate the rule graph's connected components):
    // union-find over the references; every member sorts under the representative, one segment
    std::vector<uint32_t>& comp = C.comp;
    if (!relate.empty()) {
        comp.resize(R);
        for (uint32_t x = 0; x < R; ++x) comp[x] = x;
        std::function<uint32_t(uint32_t)> find = [&](uint32_t x) { return comp[x] == x ? x : comp[x] = find(comp[x]); };
        for (auto& pr : relate) {
            uint32_t a = find(pr.first), b = find(pr.second);
            if (a != b) comp[std::max(a, b)] = std::min(a, b);
        }
        for (uint32_t x = 0; x < R; ++x) comp[x] = find(x);
        std::vector<uint32_t>& members = C.members;
        for (uint32_t x = 0; x < R; ++x)
            if (comp[x] != x) { members.push_back(x); members.push_back(comp[x]); }
        std::sort(members.begin(), members.end());
        members.erase(std::unique(members.begin(), members.end()), members.end());
        for (uint32_t x : members) {
            if (comp[x] == x) { prog[x].multi |= PX_MULTI; prog[x].pflags |= PF_SERIAL; }
        }
        C.any_multi = !members.empty();
    }
    return C;
}
inline Compiled compile_rules(const RuleLists& L, const CompileEnv& env) {
    Compiled C;
    if ((C.err = rule_limits(L, env, C.msg)) != SG_OK) return C;
    return compile_tables(L, env);
}

// Controller / breaker state of the kinds that were not reloaded, carried from the old tables into the new ones:
// a resource keeps a kind's states when it compiles to as many rules of the kind as before (wherever its rule_off
// now lies), and starts from the initial states otherwise.  old_rst empty: nothing to carry.
inline void carry_state(const std::vector<Prog>& old_prog, const std::vector<RState>& old_rst, const std::vector<Prog>& prog,
                        std::vector<RState>& rst, bool keep_par, bool keep_flow, bool keep_deg) {
    if (old_rst.empty()) return;
    for (size_t r = 0; r < prog.size() && r < old_prog.size(); ++r) {
        const Prog& p = prog[r];
        const Prog& op = old_prog[r];
        if (keep_par && op.n_param == p.n_param)
            for (int i = 0; i < p.n_param; ++i) rst[p.rule_off + i] = old_rst[op.rule_off + i];
        if (keep_flow && op.n_flow == p.n_flow)
            for (int i = 0; i < p.n_flow; ++i) rst[p.rule_off + p.n_param + i] = old_rst[op.rule_off + op.n_param + i];
        if (keep_deg && op.n_degrade == p.n_degrade)
            for (int i = 0; i < p.n_degrade; ++i)
                rst[p.rule_off + p.n_param + p.n_flow + i] = old_rst[op.rule_off + op.n_param + op.n_flow + i];
    }
}

}  // namespace sg
