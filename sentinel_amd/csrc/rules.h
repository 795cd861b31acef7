// rules.h -- the flow / degrade / param rule managers: isValidRule, equals / hashCode, java.util.HashSet iteration
// order, the FlowRuleComparator sort and the de-duplication of a loaded list.
//
// Host only: it needs neither HIP nor the engine (tests/rules_host.cpp drives it on the CPU against the oracle's
// rule order).  The engine's loaders (engine.cpp sg_load_*_rules) compare a list's equality keys with the last
// list's, call the list builder of the kind, and publish what it kept; compile.h turns the kept lists into the
// device tables.
//
//   FlowRuleManager.loadRules -> FlowRuleUtil.buildFlowRuleMap (core/slots/block/flow/FlowRuleUtil.java:89-137)
//   DegradeRuleManager.loadRules (core/slots/block/degrade/DegradeRuleManager.java:112-205)
//   ParamFlowRuleManager.loadRules (param/slots/block/flow/param/ParamFlowRuleManager.java:103-166)
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/sentinel_gpu.h"

namespace sg {

// ----------------------------------------------------------------- Java helpers
inline int32_t j_string_hash(const char* s) {
    if (!s) return 0;
    uint32_t h = 0;
    const unsigned char* p = (const unsigned char*)s;
    while (*p) {
        uint32_t cp;
        if (*p < 0x80) cp = *p++;
        else if ((*p & 0xE0) == 0xC0 && p[1]) { cp = ((p[0] & 0x1Fu) << 6) | (p[1] & 0x3Fu); p += 2; }
        else if ((*p & 0xF0) == 0xE0 && p[1] && p[2]) { cp = ((p[0] & 0x0Fu) << 12) | ((p[1] & 0x3Fu) << 6) | (p[2] & 0x3Fu); p += 3; }
        else if (p[1] && p[2] && p[3]) { cp = ((p[0] & 0x07u) << 18) | ((p[1] & 0x3Fu) << 12) | ((p[2] & 0x3Fu) << 6) | (p[3] & 0x3Fu); p += 4; }
        else cp = *p++;
        if (cp >= 0x10000) {
            cp -= 0x10000;
            h = 31u * h + (0xD800u + (cp >> 10));
            h = 31u * h + (0xDC00u + (cp & 0x3FFu));
        } else {
            h = 31u * h + cp;
        }
    }
    return (int32_t)h;
}
inline int32_t h31(int32_t h, int32_t v) { return (int32_t)(31u * (uint32_t)h + (uint32_t)v); }
inline int32_t j_double_hash(double d) {
    uint64_t u;
    std::memcpy(&u, &d, 8);
    if (d != d) u = 0x7ff8000000000000ULL;
    return (int32_t)(uint32_t)(u ^ (u >> 32));
}
inline uint64_t dbl_bits(double d) {
    uint64_t u;
    std::memcpy(&u, &d, 8);
    if (d != d) u = 0x7ff8000000000000ULL;
    return u;
}
inline int32_t long_hash(int64_t v) { return (int32_t)(uint32_t)((uint64_t)v ^ ((uint64_t)v >> 32)); }
inline bool blank(const char* s) {
    if (!s) return true;
    for (; *s; ++s)
        if (*s != ' ' && *s != '\t' && *s != '\n' && *s != '\r' && *s != '\f' && *s != '\v') return false;
    return true;
}
inline std::string sv(const char* s) { return s ? std::string(s) : std::string(); }
// AbstractRule.limitAppEquals normal form: null, "" and "default" are interchangeable
inline std::string la_norm(const char* s) { return (!s || !*s || std::strcmp(s, "default") == 0) ? "default" : std::string(s); }
inline int32_t abstract_hash(const char* res, const char* la) {
    int32_t h = res ? j_string_hash(res) : 0;
    if (!(la == nullptr || !*la || std::strcmp(la, "default") == 0)) h = h31(h, j_string_hash(la));
    return h;
}
inline int32_t cluster_hash(int64_t fid, int thr, int fb, int strat, int sc, int win, bool has_strat) {
    int32_t h = fid ? long_hash(fid) : 0;
    h = h31(h, thr);
    h = h31(h, fb ? 1 : 0);
    if (has_strat) h = h31(h, strat);
    h = h31(h, sc);
    h = h31(h, win);
    return h;
}

// java.util.HashSet iteration order of elements inserted in `order` (see oracle Q11 note):
// bucket index (h ^ h>>>16) & (cap-1) ascending, insertion order inside a bucket.
inline void hashset_order(const std::vector<int32_t>& hashes, std::vector<int>& order) {
    size_t n = order.size();
    if (n <= 1) return;
    int cap = 16;
    for (;;) {
        bool grown = false;
        std::vector<int> bin(cap, 0);
        size_t size = 0;
        for (size_t k = 0; k < n; ++k) {
            uint32_t h = (uint32_t)hashes[order[k]];
            h ^= h >> 16;
            int b = (int)(h & (uint32_t)(cap - 1));
            if (bin[b] >= 8 && cap < 64) { cap *= 2; grown = true; break; }
            bin[b]++;
            if (++size > (size_t)cap * 3 / 4 && k + 1 < n) { cap *= 2; grown = true; break; }
        }
        if (!grown) break;
    }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        uint32_t ha = (uint32_t)hashes[a], hb = (uint32_t)hashes[b];
        ha ^= ha >> 16; hb ^= hb >> 16;
        return (ha & (uint32_t)(cap - 1)) < (hb & (uint32_t)(cap - 1));
    });
}

// ----------------------------------------------------------------- rule records
// (src: the index of the record's rule in the loaded list -- read by tests/rules_host.cpp alone)
struct FlowR {
    sg_flow_rule r;
    std::string res, la, ref;
    int32_t hash;
    std::string eqkey;  // FlowRule.equals
    int src;
};
struct DegR {
    sg_degrade_rule r;
    std::string res, la;
    int32_t hash;
    std::string eqkey;
    int src;
};
struct ParamItemR {
    std::string obj, ct;
    bool has_obj, has_ct;
    int32_t count, has_count;
};
struct ParamR {
    sg_param_rule r;
    std::string res, la;
    std::vector<ParamItemR> items;
    std::vector<std::pair<uint64_t, int32_t>> hot;
    int32_t hash;
    std::string eqkey;
    int src;
};

inline std::string flow_eqkey(const sg_flow_rule& r) {
    char buf[512];
    bool cc = r.cluster_mode || r.cluster_flow_id;
    std::snprintf(buf, sizeof(buf), "%d|%016llx|%d|%d|%d|%d|%d|", r.grade, (unsigned long long)dbl_bits(r.count),
                  r.strategy, r.control_behavior, r.warm_up_period_sec, r.max_queueing_time_ms, r.cluster_mode ? 1 : 0);
    std::string k = std::string(buf) + sv(r.resource) + "\x01" + la_norm(r.limit_app) + "\x01" +
                    (r.ref_resource ? "1" + std::string(r.ref_resource) : "0") + "\x01";
    if (cc) {
        std::snprintf(buf, sizeof(buf), "C%lld|%d|%d|%d|%d|%d", (long long)r.cluster_flow_id, r.cluster_threshold_type,
                      r.cluster_fallback_to_local ? 1 : 0, r.cluster_strategy, r.cluster_sample_count,
                      r.cluster_window_interval_ms);
        k += buf;
    }
    return k;
}
inline int32_t flow_hash(const sg_flow_rule& r) {
    int32_t h = abstract_hash(r.resource, r.limit_app && !blank(r.limit_app) ? r.limit_app : "default");
    h = h31(h, r.grade);
    h = h31(h, j_double_hash(r.count));
    h = h31(h, r.strategy);
    h = h31(h, r.ref_resource ? j_string_hash(r.ref_resource) : 0);
    h = h31(h, r.control_behavior);
    h = h31(h, r.warm_up_period_sec);
    h = h31(h, r.max_queueing_time_ms);
    h = h31(h, r.cluster_mode ? 1 : 0);
    int32_t ch = 0;
    if (r.cluster_mode || r.cluster_flow_id)
        ch = cluster_hash(r.cluster_flow_id, r.cluster_threshold_type, r.cluster_fallback_to_local, r.cluster_strategy,
                          r.cluster_sample_count, r.cluster_window_interval_ms, true);
    return h31(h, ch);
}
inline bool flow_valid(const sg_flow_rule& r) { // FlowRuleUtil.isValidRule (FlowRuleUtil.java:174-228)
    if (blank(r.resource) || !(r.count >= 0) || r.grade < 0 || r.strategy < 0 || r.control_behavior < 0) return false;
    if (r.cluster_mode) {
        if (r.cluster_flow_id <= 0) return false;
        if (!(r.cluster_sample_count > 0 && r.cluster_window_interval_ms > 0 &&
              r.cluster_window_interval_ms % r.cluster_sample_count == 0))
            return false;
        if (r.strategy != 0) return false;
    }
    if ((r.strategy == SG_STRATEGY_RELATE || r.strategy == SG_STRATEGY_CHAIN) && blank(r.ref_resource)) return false;
    switch (r.control_behavior) {
    case SG_CONTROL_BEHAVIOR_WARM_UP: return r.warm_up_period_sec > 0;
    case SG_CONTROL_BEHAVIOR_RATE_LIMITER: return r.max_queueing_time_ms > 0;
    case SG_CONTROL_BEHAVIOR_WARM_UP_RATE_LIMITER: return r.warm_up_period_sec > 0 && r.max_queueing_time_ms > 0;
    default: return true;
    }
}
inline std::string deg_eqkey(const sg_degrade_rule& r, int uniq) {
    char buf[256];
    // DegradeRule.equals compares count with != (NaN never equal): give NaN rules a unique key
    if (r.count != r.count) std::snprintf(buf, sizeof(buf), "NaN#%d|", uniq);
    else std::snprintf(buf, sizeof(buf), "%.17g|%d|%d|", r.count == 0 ? 0.0 : r.count, r.time_window, r.grade);
    return std::string(buf) + sv(r.resource) + "\x01" + la_norm(r.limit_app);
}
inline int32_t deg_hash(const sg_degrade_rule& r) {
    int32_t h = abstract_hash(r.resource, r.limit_app && !blank(r.limit_app) ? r.limit_app : "default");
    h = h31(h, j_double_hash(r.count));
    h = h31(h, r.time_window);
    return h31(h, r.grade);
}
inline bool deg_valid(const sg_degrade_rule& r) {  // DegradeRuleManager.isValidRule
    return !(blank(r.resource) || !(r.count >= 0) || r.time_window <= 0);
}
inline bool param_valid(const sg_param_rule& r) { // ParamFlowRuleUtil.isValidRule (ParamFlowRuleUtil.java:32-55)
    if (blank(r.resource) || !(r.count >= 0) || r.grade < 0 || !r.has_param_idx || r.burst_count < 0 ||
        r.control_behavior < 0 || r.duration_in_sec <= 0 || r.max_queueing_time_ms < 0)
        return false;
    if (r.cluster_mode) {
        if (!(r.cluster_sample_count > 0 && r.cluster_window_interval_ms > 0 &&
              r.cluster_window_interval_ms % r.cluster_sample_count == 0))
            return false;
        if (r.cluster_flow_id <= 0) return false;
    }
    return true;
}
// key: the hot items' keys (the engine's dictionary: two items whose pure keys collide keep their own counts)
inline ParamR make_param(const sg_param_rule& s, const std::function<uint64_t(const char*, const char*)>& key) {
    ParamR p;
    p.r = s;
    p.res = sv(s.resource);
    p.la = la_norm(s.limit_app);
    for (int i = 0; i < s.n_items; ++i) {
        const sg_param_item& it = s.items[i];
        ParamItemR q;
        q.has_obj = it.object != nullptr;
        q.obj = sv(it.object);
        q.has_ct = it.class_type != nullptr;
        q.ct = sv(it.class_type);
        q.count = it.count;
        q.has_count = it.has_count;
        p.items.push_back(q);
        // ParamFlowRuleUtil.parseHotItems (ParamFlowRuleUtil.java:62-83)
        if (!it.object || !it.has_count || it.count < 0) continue;
        uint64_t k = key(it.object, it.class_type);
        bool found = false;
        for (auto& h : p.hot) if (h.first == k) { h.second = it.count; found = true; }
        if (!found) p.hot.push_back({k, it.count});
    }
    // ParamFlowRule.hashCode (ParamFlowRule.java:218-234)
    int32_t h = abstract_hash(s.resource, s.limit_app && !blank(s.limit_app) ? s.limit_app : "default");
    h = h31(h, s.grade);
    h = h31(h, s.has_param_idx ? s.param_idx : 0);
    h = h31(h, j_double_hash(s.count));
    h = h31(h, s.control_behavior);
    h = h31(h, s.max_queueing_time_ms);
    h = h31(h, s.burst_count);
    h = h31(h, long_hash(s.duration_in_sec));
    int32_t lh = 1;
    for (auto& q : p.items) {
        int32_t e = q.has_obj ? j_string_hash(q.obj.c_str()) : 0;
        e = h31(e, q.has_count ? q.count : 0);
        e = h31(e, q.has_ct ? j_string_hash(q.ct.c_str()) : 0);
        lh = h31(lh, e);
    }
    h = h31(h, lh);
    h = h31(h, s.cluster_mode ? 1 : 0);
    int32_t ch = 0;
    if (s.cluster_mode || s.cluster_flow_id)
        ch = cluster_hash(s.cluster_flow_id, s.cluster_threshold_type, s.cluster_fallback_to_local, 0,
                          s.cluster_sample_count, s.cluster_window_interval_ms, false);
    p.hash = h31(h, ch);
    // ParamFlowRule.equals
    char buf[512];
    std::snprintf(buf, sizeof(buf), "%d|%016llx|%d|%d|%d|%lld|%d|%d:%d|", s.grade, (unsigned long long)dbl_bits(s.count),
                  s.control_behavior, s.max_queueing_time_ms, s.burst_count, (long long)s.duration_in_sec,
                  s.cluster_mode ? 1 : 0, s.has_param_idx, s.has_param_idx ? s.param_idx : 0);
    std::string k = std::string(buf) + p.res + "\x01" + p.la + "\x01";
    for (auto& q : p.items) {
        std::snprintf(buf, sizeof(buf), "[%d%d%d:%d]", q.has_obj, q.has_ct, q.has_count, q.has_count ? q.count : 0);
        k += buf + q.obj + "\x02" + q.ct + "\x03";
    }
    if (s.cluster_mode || s.cluster_flow_id) {
        std::snprintf(buf, sizeof(buf), "C%lld|%d|%d|%d|%d", (long long)s.cluster_flow_id, s.cluster_threshold_type,
                      s.cluster_fallback_to_local ? 1 : 0, s.cluster_sample_count, s.cluster_window_interval_ms);
        k += buf;
    }
    p.eqkey = k;
    return p;
}

// ----------------------------------------------------------------- list builders
// What a manager keeps of a loaded list.
template <class Rec> struct RuleList {
    std::vector<Rec> recs;              // the kept rules, list order
    std::vector<std::vector<int>> per;  // [resource id] its rules (indices of recs) in the order they are checked
    std::vector<std::string> keys;      // equality keys of the whole list, kept or not ("equal list = no-op")
};

// The managers' common walk over a list of n rules with equality keys L.keys: the invalid ones skipped, the
// resource of a valid one registered, a rule equal to an earlier one of its resource dropped (HashSet.add), the
// rest kept as make(i); then every resource's rules in HashSet iteration order.  reg(i, &rid) names the resource
// id of rule i (false: the load fails; the caller has the reason).
template <class Rec, class Valid, class Reg, class Make>
bool build_rule_list(uint32_t n, Valid valid, Reg reg, Make make, RuleList<Rec>& L) {
    std::unordered_map<std::string, int> seen;
    for (uint32_t i = 0; i < n; ++i) {
        if (!valid(i)) continue;
        uint32_t rid;
        if (!reg(i, &rid)) return false;
        std::string k = std::to_string(rid) + "#" + L.keys[i];
        if (seen.count(k)) continue; // HashSet.add of an equal rule
        seen[k] = 1;
        L.recs.push_back(make(i));
        L.recs.back().src = (int)i;
        if (L.per.size() <= rid) L.per.resize(rid + 1);
        L.per[rid].push_back((int)L.recs.size() - 1);
    }
    std::vector<int32_t> hs(L.recs.size());
    for (size_t i = 0; i < L.recs.size(); ++i) hs[i] = L.recs[i].hash;
    for (auto& l : L.per) hashset_order(hs, l);
    return true;
}

inline std::vector<std::string> flow_keys(const sg_flow_rule* rules, uint32_t n) {
    std::vector<std::string> keys(n);
    for (uint32_t i = 0; i < n; ++i) keys[i] = flow_eqkey(rules[i]);
    return keys;
}
// reg(name, &id): the id of a resource, registered if new (false: the load fails).  A RELATE rule registers the
// resource it names as well: its ClusterNode is read.
template <class Reg>
bool build_flow_list(const sg_flow_rule* rules, uint32_t n, std::vector<std::string> keys, Reg reg, RuleList<FlowR>& L) {
    L = RuleList<FlowR>();
    L.keys = std::move(keys);
    const bool ok = build_rule_list(
        n, [&](uint32_t i) { return flow_valid(rules[i]); },
        [&](uint32_t i, uint32_t* rid) {
            const sg_flow_rule& r = rules[i];
            if (!reg(r.resource, rid)) return false;
            uint32_t ref;
            return !(r.strategy == SG_STRATEGY_RELATE && r.ref_resource && *r.ref_resource) || reg(r.ref_resource, &ref);
        },
        [&](uint32_t i) {
            const sg_flow_rule& r = rules[i];
            FlowR f;
            f.r = r;
            f.res = r.resource;
            f.la = la_norm(r.limit_app);
            f.ref = sv(r.ref_resource);
            f.hash = flow_hash(r);
            f.eqkey = L.keys[i];
            return f;
        },
        L);
    if (!ok) return false;
    const std::vector<FlowR>& flows = L.recs;
    for (auto& l : L.per) {
        // Collections.sort(rules, FlowRuleComparator) -- stable (FlowRuleComparator.java:30-55)
        std::stable_sort(l.begin(), l.end(), [&](int a, int b) {
            const FlowR &x = flows[a], &y = flows[b];
            auto cmp = [](const FlowR& o1, const FlowR& o2) {
                if (o1.r.cluster_mode && !o2.r.cluster_mode) return 1;
                if (!o1.r.cluster_mode && o2.r.cluster_mode) return -1;
                if (o1.la == o2.la) return 0;
                if (o1.la == "default") return 1;
                if (o2.la == "default") return -1;
                return 0;
            };
            return cmp(x, y) < 0;
        });
    }
    return true;
}

inline std::vector<std::string> deg_keys(const sg_degrade_rule* rules, uint32_t n) {
    std::vector<std::string> keys(n);
    for (uint32_t i = 0; i < n; ++i) keys[i] = deg_eqkey(rules[i], (int)i);
    return keys;
}
template <class Reg>
bool build_degrade_list(const sg_degrade_rule* rules, uint32_t n, std::vector<std::string> keys, Reg reg, RuleList<DegR>& L) {
    L = RuleList<DegR>();
    L.keys = std::move(keys);
    return build_rule_list(
        n, [&](uint32_t i) { return deg_valid(rules[i]); },
        [&](uint32_t i, uint32_t* rid) { return reg(rules[i].resource, rid); },
        [&](uint32_t i) {
            const sg_degrade_rule& r = rules[i];
            DegR d;
            d.r = r;
            d.res = r.resource;
            d.la = la_norm(r.limit_app);
            d.hash = deg_hash(r);
            d.eqkey = L.keys[i];
            return d;
        },
        L);
}

// Param rules in two steps, so that the caller can tell an equal list before any resource is registered: the
// records and keys of the whole list (the invalid rules' too: key interns their hot items as well), then the
// kept ones.  False: a rule names items and has none.
inline bool param_records(const sg_param_rule* rules, uint32_t n, const std::function<uint64_t(const char*, const char*)>& key,
                          std::vector<ParamR>& all, std::vector<std::string>& keys) {
    for (uint32_t i = 0; i < n; ++i) {
        if (rules[i].n_items > 0 && !rules[i].items) return false;
        all.push_back(make_param(rules[i], key));
        all.back().src = (int)i;
        keys.push_back(all.back().eqkey);
    }
    return true;
}
template <class Reg>
bool build_param_list(const std::vector<ParamR>& all, std::vector<std::string> keys, Reg reg, RuleList<ParamR>& L) {
    L = RuleList<ParamR>();
    L.keys = std::move(keys);
    return build_rule_list(
        (uint32_t)all.size(), [&](uint32_t i) { return param_valid(all[i].r); },
        [&](uint32_t i, uint32_t* rid) { return reg(all[i].r.resource, rid); }, [&](uint32_t i) { return all[i]; }, L);
}

}  // namespace sg
