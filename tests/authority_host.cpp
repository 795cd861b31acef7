// Host check of the authority rules (sentinel_amd/csrc/authority.h): the rule compiler the engine loads rules
// with and the exact lookup the kernels run, driven on the CPU by a script of commands.  Built and run by
// tests/test_authority_host.py, which compares the verdicts with a Python restatement of
// AuthorityRuleChecker.passCheck (core/slots/block/authority/AuthorityRuleChecker.java:30-65).
//
// Origins are interned as the engine interns them: "" is id 0, every other name gets the next dense id at its
// first intern, and a new id is handed to AuthTable::on_intern.  Resources get dense ids at first sight.
//
// stdin, one command a line; strings are "-" (NULL) or "=" followed by the hex of their bytes:
//   load N                      then N lines "STRATEGY RESOURCE LIMIT_APP"; prints "loaded K" (K rules kept)
//   intern NAME                 prints "id I"
//   check RESOURCE ORIGIN_ID    prints "v 1" if the entry is blocked, else "v 0"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>

#include "../sentinel_amd/csrc/authority.h"

using namespace sg;

static const uint32_t MAX_RES = 4096;

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

int main() {
    AuthTable tab;
    std::unordered_map<std::string, uint32_t> res_ids, origin_ids;
    auto res_of = [&](const char* name, uint32_t* id) {
        auto it = res_ids.find(name);
        if (it == res_ids.end()) {
            if (res_ids.size() >= MAX_RES) return false;
            it = res_ids.emplace(name, (uint32_t)res_ids.size()).first;
        }
        *id = it->second;
        return true;
    };
    auto origin_of = [&](const char* name, uint32_t* id) {
        auto it = origin_ids.find(name);
        if (it == origin_ids.end()) return false;
        *id = it->second;
        return true;
    };
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string cmd;
        is >> cmd;
        if (cmd == "load") {
            uint32_t n = 0;
            is >> n;
            std::vector<Str> rs(n), ls(n);
            std::vector<AuthIn> in(n);
            for (uint32_t i = 0; i < n; ++i) {
                std::getline(std::cin, line);
                std::istringstream rl(line);
                int strategy;
                std::string r, l;
                rl >> strategy >> r >> l;
                rs[i] = unhex(r);
                ls[i] = unhex(l);
                in[i] = AuthIn{rs[i].c(), ls[i].c(), strategy};
            }
            if (!tab.compile(in.data(), n, MAX_RES, res_of, origin_of)) { std::printf("error\n"); return 2; }
            std::printf("loaded %zu\n", tab.rules.size());
        } else if (cmd == "intern") {
            std::string t;
            is >> t;
            const Str nm = unhex(t);
            uint32_t id = 0;
            if (!nm.null && !nm.s.empty()) {
                auto it = origin_ids.find(nm.s);
                if (it != origin_ids.end()) id = it->second;
                else {
                    id = (uint32_t)origin_ids.size() + 1;
                    origin_ids.emplace(nm.s, id);
                    tab.on_intern(nm.s.c_str(), id);
                }
            }
            std::printf("id %u\n", id);
        } else if (cmd == "check") {
            std::string t;
            uint32_t origin = 0;
            is >> t >> origin;
            const Str nm = unhex(t);
            bool blocked = false;
            auto it = res_ids.find(nm.s);
            // the device reads the table only when rules are loaded (a null pointer otherwise)
            if (!tab.empty() && it != res_ids.end()) blocked = auth_blocks(tab.desc.data(), tab.ids.data(), it->second, origin);
            std::printf("v %d\n", blocked ? 1 : 0);
        } else if (!cmd.empty()) {
            std::printf("error\n");
            return 2;
        }
    }
    return 0;
}
