// Host check of the rule managers (sentinel_amd/csrc/rules.h) and the rule compiler (sentinel_amd/csrc/compile.h):
// the list builders the engine loads rules with and the compiler of its device tables, driven on the CPU by a script
// of commands.  Built and run by tests/test_rules_host.py, which compares the compiled order with the oracle's and
// the compiled tables with a hand-written table.  No HIP call is made (dev_types.h needs the runtime header only).
//
// The harness stands in for the engine where the compiler reads it: resources get dense ids at first sight, origins
// and contexts dense ids from 1 at `origin` / `context`, every kept param rule a map of its own (pmap == the rule's
// state id, in first-sight order), and a resource has the thread-count maps its current param rules resolve to.
//
// stdin, one command a line; strings are "-" (NULL) or "=" followed by the hex of their bytes, doubles the hex of
// their bits:
//   env R MAX_RULES COLD MIX_ON MIX_PQ PV_ON PV_PQ EMB_ON     the CompileEnv switches and limits (R: max_resources)
//   origin NAME | context NAME
//   flow N | degrade N | param N    then N rule lines (fields in struct order, see load_*); prints
//        "loaded KIND K" (or "load-error"), "h KIND SRC HASH" a kept rule, "order KIND RES SRC..." a resource
//   compile KEEP_PAR KEEP_FLOW KEEP_DEG     pre-checks, compiles, carries the marked states over and prints the tables;
//                                           "emitted RES N COUNT": the DRules compile_tables builds for RES (no size
//                                           refusal) and what compiled_rule_count says
//   mark                                    gives every current rule state distinct values (a = 1000 + index, ...)
//   forget NAME                             drops NAME from the resource id map (a RELATE reference to an unknown name)
//   why                                     then one flow line: prints EmbShape::why of that rule alone on a resource
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../sentinel_amd/csrc/compile.h"
#include "../sentinel_amd/csrc/rules.h"

using namespace sg;

struct Str {
    bool null = true;
    std::string s;
    const char* c() const { return null ? nullptr : s.c_str(); }
};
static Str unhex(const std::string& t) {
    Str r;
    if (t == "-") return r;
    r.null = false;
    for (size_t i = 1; i + 1 < t.size(); i += 2) r.s.push_back((char)std::stoi(t.substr(i, 2), nullptr, 16));
    return r;
}
static std::string hex(const std::string& s) {
    std::string o = "=";
    char b[3];
    for (unsigned char c : s) { std::snprintf(b, sizeof(b), "%02x", c); o += b; }
    return o;
}
static double dbl(const std::string& t) {
    const uint64_t u = std::strtoull(t.c_str(), nullptr, 16);
    double d;
    std::memcpy(&d, &u, 8);
    return d;
}
static unsigned long long bits(double d) {
    uint64_t u;
    std::memcpy(&u, &d, 8);
    return (unsigned long long)u;
}

// The strings of a loaded list stay alive beside the records that point to them.
struct Strings { std::vector<Str> v; };
static void take(Strings& S, std::istringstream& is) {  // (pointers are taken once the list is read: the vector grows)
    std::string t;
    is >> t;
    S.v.push_back(unhex(t));
}

struct Harness {
    std::vector<std::string> names;
    std::unordered_map<std::string, uint32_t> ids, origin_ids, context_ids;
    std::vector<uint32_t> tm_base;
    std::unordered_map<uint32_t, uint32_t> pmap_index;
    std::map<std::string, uint32_t> psid_of;
    std::set<uint64_t> tmaps;
    uint32_t max_resources = 64, max_rules = 1024;
    int32_t cold_factor = 3;
    bool mix_on = true, mix_pq = false, pv_on = true, pv_pq = true, emb_on = false;
    RuleList<FlowR> flows;
    RuleList<DegR> degs;
    RuleList<ParamR> params;
    Strings fs, ds, ps;
    std::vector<sg_param_item> items;
    std::vector<Prog> prog;  // the tables "on the device"
    std::vector<RState> rst;

    CompileEnv env() const {
        return CompileEnv{names, ids, origin_ids, context_ids, tm_base, pmap_index, psid_of, tmaps,
                          max_resources, max_rules, cold_factor, mix_on, mix_pq, pv_on, pv_pq, emb_on};
    }
    RuleLists lists() const { return RuleLists{params.recs, params.per, flows.recs, flows.per, degs.recs, degs.per}; }
    bool reg(const char* name, uint32_t* id) {
        auto it = ids.find(name);
        if (it == ids.end()) {
            if (names.size() >= max_resources) return false;
            it = ids.emplace(name, (uint32_t)names.size()).first;
            names.push_back(name);
        }
        *id = it->second;
        return true;
    }
    template <class Rec> void print_list(const char* kind, const RuleList<Rec>& L) {
        std::printf("loaded %s %zu\n", kind, L.recs.size());
        for (const Rec& r : L.recs) std::printf("h %s %d %d\n", kind, r.src, (int)r.hash);
        for (size_t r = 0; r < L.per.size(); ++r) {
            if (L.per[r].empty()) continue;
            std::printf("order %s %s", kind, hex(names[r]).c_str());
            for (int i : L.per[r]) std::printf(" %d", L.recs[i].src);
            std::printf("\n");
        }
    }
};

static std::vector<std::string> read_lines(uint32_t n) {
    std::vector<std::string> l(n);
    for (auto& s : l) std::getline(std::cin, s);
    return l;
}

// the rules of n flow lines; their strings live in S
static std::vector<sg_flow_rule> read_flow(const std::vector<std::string>& lines, Strings& S) {
    const uint32_t n = (uint32_t)lines.size();
    std::vector<sg_flow_rule> rules(n);
    for (uint32_t i = 0; i < n; ++i) {
        std::istringstream is(lines[i]);
        sg_flow_rule& r = rules[i];
        std::memset(&r, 0, sizeof(r));
        take(S, is); take(S, is); take(S, is);
        std::string c;
        long long fid;
        is >> c >> r.grade >> r.strategy >> r.control_behavior >> r.warm_up_period_sec >> r.max_queueing_time_ms >>
            r.cluster_mode >> fid >> r.cluster_threshold_type >> r.cluster_fallback_to_local >> r.cluster_strategy >>
            r.cluster_sample_count >> r.cluster_window_interval_ms;
        r.count = dbl(c);
        r.cluster_flow_id = fid;
    }
    for (uint32_t i = 0; i < n; ++i) {
        rules[i].resource = S.v[3 * i].c();
        rules[i].limit_app = S.v[3 * i + 1].c();
        rules[i].ref_resource = S.v[3 * i + 2].c();
    }
    return rules;
}

static void load_flow(Harness& H, uint32_t n) {
    Strings S;
    std::vector<sg_flow_rule> rules = read_flow(read_lines(n), S);
    RuleList<FlowR> L;
    if (!build_flow_list(rules.data(), n, flow_keys(rules.data(), n),
                         [&](const char* nm, uint32_t* id) { return H.reg(nm, id); }, L)) {
        std::printf("load-error\n");
        return;
    }
    H.flows = std::move(L);
    H.fs = std::move(S);
    H.print_list("flow", H.flows);
}

static void load_degrade(Harness& H, uint32_t n) {
    const auto lines = read_lines(n);
    Strings S;
    std::vector<sg_degrade_rule> rules(n);
    for (uint32_t i = 0; i < n; ++i) {
        std::istringstream is(lines[i]);
        sg_degrade_rule& r = rules[i];
        std::memset(&r, 0, sizeof(r));
        take(S, is); take(S, is);
        std::string c;
        is >> c >> r.time_window >> r.grade;
        r.count = dbl(c);
    }
    for (uint32_t i = 0; i < n; ++i) {
        rules[i].resource = S.v[2 * i].c();
        rules[i].limit_app = S.v[2 * i + 1].c();
    }
    RuleList<DegR> L;
    if (!build_degrade_list(rules.data(), n, deg_keys(rules.data(), n),
                            [&](const char* nm, uint32_t* id) { return H.reg(nm, id); }, L)) {
        std::printf("load-error\n");
        return;
    }
    H.degs = std::move(L);
    H.ds = std::move(S);
    H.print_list("degrade", H.degs);
}

static void load_param(Harness& H, uint32_t n) {
    const auto lines = read_lines(n);
    Strings S;
    std::vector<sg_param_rule> rules(n);
    std::vector<sg_param_item> items;
    std::vector<size_t> item_off(n), str_off(n);
    for (uint32_t i = 0; i < n; ++i) {
        std::istringstream is(lines[i]);
        sg_param_rule& r = rules[i];
        std::memset(&r, 0, sizeof(r));
        str_off[i] = S.v.size();
        take(S, is); take(S, is);
        std::string c;
        long long dur, fid;
        is >> c >> dur >> r.grade >> r.param_idx >> r.has_param_idx >> r.control_behavior >> r.max_queueing_time_ms >>
            r.burst_count >> r.cluster_mode >> fid >> r.cluster_threshold_type >> r.cluster_fallback_to_local >>
            r.cluster_sample_count >> r.cluster_window_interval_ms >> r.n_items;
        r.count = dbl(c);
        r.duration_in_sec = dur;
        r.cluster_flow_id = fid;
        item_off[i] = items.size();
        for (int k = 0; k < r.n_items; ++k) {
            sg_param_item it;
            std::memset(&it, 0, sizeof(it));
            take(S, is); take(S, is);
            is >> it.count >> it.has_count;
            items.push_back(it);
        }
    }
    for (uint32_t i = 0; i < n; ++i) {
        rules[i].resource = S.v[str_off[i]].c();
        rules[i].limit_app = S.v[str_off[i] + 1].c();
        rules[i].items = items.data() + item_off[i];
        for (int k = 0; k < rules[i].n_items; ++k) {
            items[item_off[i] + k].object = S.v[str_off[i] + 2 + 2 * k].c();
            items[item_off[i] + k].class_type = S.v[str_off[i] + 3 + 2 * k].c();
        }
    }
    std::vector<ParamR> all;
    std::vector<std::string> keys;
    // an item's key: any function of the value and its type will do here (the engine's dictionary is pkeys.h)
    auto key = [](const char* v, const char* t) {
        return ((uint64_t)(uint32_t)j_string_hash(v) << 32) | (uint32_t)j_string_hash(t);
    };
    RuleList<ParamR> L;
    if (!param_records(rules.data(), n, key, all, keys) ||
        !build_param_list(all, std::move(keys), [&](const char* nm, uint32_t* id) { return H.reg(nm, id); }, L)) {
        std::printf("load-error\n");
        return;
    }
    H.params = std::move(L);
    H.ps = std::move(S);
    H.items = std::move(items);
    // the records point into the harness's copies from here on (rules only lived in this function)
    H.tmaps.clear();
    for (size_t r = 0; r < H.params.per.size(); ++r)
        for (int i : H.params.per[r]) {
            const ParamR& q = H.params.recs[i];
            const std::string k = q.res + std::string("\0", 1) + q.eqkey;
            if (!H.psid_of.count(k)) {
                const uint32_t psid = (uint32_t)H.psid_of.size() + 1;
                H.psid_of[k] = psid;
                H.pmap_index[psid] = psid;
            }
            for (int32_t a = 0; a < SG_MAX_ARGS; ++a)
                if (q.r.param_idx < 0 || q.r.param_idx == a) H.tmaps.insert(((uint64_t)r << 8) | (uint64_t)a);
        }
    H.print_list("param", H.params);
}

static void compile(Harness& H, bool keep_par, bool keep_flow, bool keep_deg) {
    const CompileEnv env = H.env();
    const RuleLists L = H.lists();
    std::string msg;
    int rc = rule_limits(L, env, msg);
    std::printf("limits %d %s\n", rc, hex(msg).c_str());
    msg.clear();
    rc = emb_refuse(H.flows.recs, H.flows.per, H.params.per, msg);
    std::printf("embshape %d %s\n", rc, hex(msg).c_str());
    {  // what the compiler emits with the size refusal left out, beside what the pre-check counts
        const Compiled T = compile_tables(L, env);
        for (size_t r = 0; r < H.names.size() && r < T.prog.size(); ++r)
            std::printf("emitted %s %d %zu\n", hex(H.names[r]).c_str(),
                        (int)T.prog[r].n_param + T.prog[r].n_flow + T.prog[r].n_degrade, compiled_rule_count(L, r));
        std::printf("emitted-total %zu\n", T.rules.size());
    }
    Compiled C = compile_rules(L, env);
    std::printf("compiled %d %s\n", C.err, hex(C.msg).c_str());
    if (C.err) return;
    carry_state(H.prog, H.rst, C.prog, C.rst, keep_par, keep_flow, keep_deg);
    for (size_t r = 0; r < H.names.size() && r < C.prog.size(); ++r) {
        const Prog& p = C.prog[r];
        std::printf("prog %s id=%zu off=%u np=%d nf=%d nd=%d pflags=%u xf=%u multi=%u ncompiled=%zu\n", hex(H.names[r]).c_str(), r,
                    p.rule_off, p.n_param, p.n_flow, p.n_degrade, (unsigned)p.pflags, (unsigned)p.xf, (unsigned)p.multi,
                    compiled_rule_count(L, r));
    }
    for (size_t i = 0; i < C.rules.size(); ++i) {
        const DRule& d = C.rules[i];
        std::printf("rule %zu kind=%d grade=%d behavior=%d slot=%d max_queue=%d count=%016llx slope=%016llx warning_token=%d "
                    "max_token=%d count_div_cold=%d time_window=%d burst=%d token_count=%d duration_sec=%lld token_count_l=%lld "
                    "hot_off=%u hot_n=%u pmap=%u ref=%u param_idx=%d la_kind=%u la_origin=%u strategy=%u chain_ctx=%u\n",
                    i, d.kind, d.grade, d.behavior, d.slot, d.max_queue, bits(d.count), bits(d.slope), d.warning_token,
                    d.max_token, d.count_div_cold, d.time_window, d.burst, d.token_count, (long long)d.duration_sec,
                    (long long)d.token_count_l, d.hot_off, d.hot_n, d.pmap, d.ref, d.param_idx, d.la_kind, d.la_origin,
                    d.strategy, d.chain_ctx);
    }
    for (size_t i = 0; i < C.rst.size(); ++i)
        std::printf("rst %zu %lld %lld %lld %lld\n", i, (long long)C.rst[i].a, (long long)C.rst[i].b, (long long)C.rst[i].c,
                    (long long)C.rst[i].d);
    for (size_t i = 0; i < C.hot.size(); ++i)
        std::printf("hot %zu %llu %d\n", i, (unsigned long long)C.hot[i].key, C.hot[i].count);
    for (size_t r = 0; r < C.comp.size(); ++r)
        if (C.comp[r] != r) std::printf("comp %zu %u\n", r, C.comp[r]);
    std::printf("members");
    for (uint32_t m : C.members) std::printf(" %u", m);
    std::printf("\n");
    for (const auto& er : C.emb_res) std::printf("emb %u %lld\n", er.first, (long long)er.second);
    std::printf("flags any_mix=%d any_head=%d any_multi=%d comp=%zu\n", C.any_mix, C.any_head, C.any_multi, C.comp.size());
    H.prog = std::move(C.prog);
    H.rst = std::move(C.rst);
}

int main() {
    Harness H;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string cmd;
        is >> cmd;
        if (cmd == "env") {
            is >> H.max_resources >> H.max_rules >> H.cold_factor >> H.mix_on >> H.mix_pq >> H.pv_on >> H.pv_pq >> H.emb_on;
        } else if (cmd == "origin" || cmd == "context") {
            std::string t;
            is >> t;
            auto& m = cmd == "origin" ? H.origin_ids : H.context_ids;
            const Str nm = unhex(t);
            if (!m.count(nm.s)) m.emplace(nm.s, (uint32_t)m.size() + 1);
            std::printf("id %u\n", m[nm.s]);
        } else if (cmd == "flow" || cmd == "degrade" || cmd == "param") {
            uint32_t n = 0;
            is >> n;
            if (cmd == "flow") load_flow(H, n);
            else if (cmd == "degrade") load_degrade(H, n);
            else load_param(H, n);
        } else if (cmd == "compile") {
            int kp = 0, kf = 0, kd = 0;
            is >> kp >> kf >> kd;
            compile(H, kp, kf, kd);
        } else if (cmd == "why") {  // EmbShape::why of one flow line's record, alone on resource 0, never validated
            Strings S;
            const sg_flow_rule r = read_flow(read_lines(1), S)[0];
            FlowR f;
            f.r = r;
            f.res = sv(r.resource);
            f.la = la_norm(r.limit_app);
            f.ref = sv(r.ref_resource);
            const char* why = EmbShape({f}).why(f, 0, {{0}}, {});
            std::printf("why %s\n", why ? hex(why).c_str() : "-");
        } else if (cmd == "forget") {  // the name leaves the id map (its id stays taken): a reference to it finds nothing
            std::string t;
            is >> t;
            H.ids.erase(unhex(t).s);
        } else if (cmd == "mark") {
            for (size_t i = 0; i < H.rst.size(); ++i)
                H.rst[i] = RState{1000 + (int64_t)i, 2000 + (int64_t)i, 3000 + (int64_t)i, 4000 + (int64_t)i};
        } else if (!cmd.empty()) {
            std::printf("error\n");
            return 2;
        }
        std::printf("done\n");
    }
    return 0;
}
