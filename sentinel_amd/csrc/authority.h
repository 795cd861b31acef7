// authority.h -- AuthoritySlot's black / white lists: the rule compiler, the device table and the lookup.
//
// The single home of the authority semantics, for the host and the device alike.  It needs neither HIP nor the
// engine (tests/authority_host.cpp drives it on the CPU); under hipcc the lookup is __host__ __device__.
//
//   AuthorityRuleManager.loadAuthorityConf / isValidRule (core/slots/block/authority/AuthorityRuleManager.java:105-157):
//     a rule is valid iff its resource is not blank, its limitApp is not blank and strategy >= 0; the first valid
//     rule of a resource in list order is kept, later ones are ignored.
//   AuthorityRuleChecker.passCheck (core/slots/block/authority/AuthorityRuleChecker.java:30-65):
//     the empty origin passes; contain = the origin equals one of limitApp.split(",") (java.lang.String.split:
//     trailing empty tokens dropped, nothing trimmed; the indexOf pre-test is implied by token equality);
//     AUTHORITY_BLACK blocks when contain, AUTHORITY_WHITE when !contain, any other strategy never blocks.
//
// Device table: one 8-byte AuthDesc per resource (mode, count, offset) into one array of origin ids, each
// resource's ids sorted.  Origins are dense ids in first-intern order, so loading rules interns nothing: a token
// whose name has no id yet matches no event (no event can carry it) and is resolved by on_intern() once the name
// gets its id.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#if defined(__HIPCC__)
#define AUTH_FN __host__ __device__
#else
#define AUTH_FN
#endif

namespace sg {

enum : uint32_t { AUTH_NONE = 0, AUTH_WHITE = 1, AUTH_BLACK = 2 };  // AuthDesc mode (AUTH_NONE: never blocks)

struct AuthDesc {
    uint32_t off;  // first id of the resource's list in the id array
    uint32_t cm;   // mode << 24 | count of ids
};
static_assert(sizeof(AuthDesc) == 8, "AuthDesc must be 8 B");

// AuthorityRuleChecker.passCheck == false for an entry of resource res from origin (an interned id; 0 = "").
// desc holds an AuthDesc for every res the caller may pass; ids is read only inside the resource's list.
AUTH_FN inline bool auth_blocks(const AuthDesc* desc, const uint32_t* ids, uint32_t res, uint32_t origin) {
    if (origin == 0) return false;
    const AuthDesc d = desc[res];
    const uint32_t mode = d.cm >> 24;
    if (mode == AUTH_NONE) return false;
    uint32_t lo = 0, hi = d.cm & 0xFFFFFFu;  // lists hold a handful of names: a short search
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (ids[d.off + mid] < origin) lo = mid + 1;
        else hi = mid;
    }
    const bool contain = lo < (d.cm & 0xFFFFFFu) && ids[d.off + lo] == origin;
    return mode == AUTH_BLACK ? contain : !contain;
}

// ---- host side ---------------------------------------------------------------------------------------------

struct AuthIn {  // one rule as the caller gave it (AuthorityRule.java: resource, limitApp, strategy)
    const char* resource;
    const char* limit_app;
    int32_t strategy;
};

inline bool auth_blank(const char* s) {  // StringUtil.isBlank
    if (!s) return true;
    for (; *s; ++s)
        if (*s != ' ' && *s != '\t' && *s != '\n' && *s != '\r' && *s != '\f' && *s != '\v') return false;
    return true;
}
inline bool auth_valid(const AuthIn& r) { return !auth_blank(r.resource) && r.strategy >= 0 && !auth_blank(r.limit_app); }

// java.lang.String.split(","): every token, then the trailing empty ones removed
inline std::vector<std::string> auth_split(const std::string& s) {
    std::vector<std::string> out;
    size_t a = 0;
    for (;;) {
        const size_t b = s.find(',', a);
        out.push_back(s.substr(a, b == std::string::npos ? std::string::npos : b - a));
        if (b == std::string::npos) break;
        a = b + 1;
    }
    while (!out.empty() && out.back().empty()) out.pop_back();
    return out;
}

struct AuthRule {  // a kept rule
    std::string resource, limit_app;
    int32_t strategy;
    uint32_t res;                     // resource id
    std::vector<std::string> tokens;  // limit_app.split(",")
    std::vector<uint32_t> ids;        // the tokens that are interned origins, sorted, distinct
};

struct AuthTable {
    std::vector<AuthRule> rules;                                    // kept rules, list order
    std::unordered_map<std::string, std::vector<uint32_t>> by_name; // token -> the kept rules listing it
    std::vector<AuthDesc> desc;                                     // [n_res] (empty: no rules)
    std::vector<uint32_t> ids;                                      // the rules' id lists, back to back

    bool empty() const { return rules.empty(); }

    // The first valid rule of every resource, in list order.  res_of(name, &id) names the resource's id (false:
    // the load fails, nothing changes); origin_of(name, &id) the id of an interned origin (false: not interned).
    template <class ResOf, class OriginOf>
    bool compile(const AuthIn* in, uint32_t n, uint32_t n_res, ResOf res_of, OriginOf origin_of) {
        std::vector<AuthRule> kept;
        std::unordered_map<std::string, int> seen;
        for (uint32_t i = 0; i < n; ++i) {
            if (!auth_valid(in[i])) continue;
            if (seen.count(in[i].resource)) continue;
            AuthRule r;
            r.resource = in[i].resource;
            r.limit_app = in[i].limit_app;
            r.strategy = in[i].strategy;
            if (!res_of(in[i].resource, &r.res)) return false;
            seen[r.resource] = 1;
            r.tokens = auth_split(r.limit_app);
            for (const std::string& t : r.tokens) {
                uint32_t id;
                if (!t.empty() && origin_of(t.c_str(), &id)) r.ids.push_back(id);
            }
            std::sort(r.ids.begin(), r.ids.end());
            r.ids.erase(std::unique(r.ids.begin(), r.ids.end()), r.ids.end());
            kept.push_back(std::move(r));
        }
        rules = std::move(kept);
        by_name.clear();
        for (uint32_t k = 0; k < rules.size(); ++k)
            for (const std::string& t : rules[k].tokens) {
                auto& l = by_name[t];
                if (l.empty() || l.back() != k) l.push_back(k);
            }
        flatten(n_res);
        return true;
    }

    // The origin `name` was interned as `id` (a new id: larger than every earlier one).  True if a rule lists it:
    // the tables changed and must be uploaded again.
    bool on_intern(const char* name, uint32_t id) {
        auto it = by_name.find(name);
        if (it == by_name.end()) return false;
        for (uint32_t k : it->second) {
            auto& l = rules[k].ids;
            l.insert(std::lower_bound(l.begin(), l.end(), id), id);
        }
        flatten((uint32_t)desc.size());
        return true;
    }

    void flatten(uint32_t n_res) {
        desc.clear();
        ids.clear();
        if (rules.empty()) return;
        desc.assign(n_res, AuthDesc{0u, 0u});
        for (const AuthRule& r : rules) {
            if (r.res >= n_res) continue;
            const uint32_t mode = r.strategy == 0 ? AUTH_WHITE : r.strategy == 1 ? AUTH_BLACK : AUTH_NONE;
            desc[r.res] = AuthDesc{(uint32_t)ids.size(), (mode << 24) | (uint32_t)(r.ids.size() & 0xFFFFFFu)};
            ids.insert(ids.end(), r.ids.begin(), r.ids.end());
        }
    }
};

}  // namespace sg
