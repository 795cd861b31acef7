// pkeys_host.cpp -- the parameter key dictionary (sentinel_amd/csrc/pkeys.h) against a std::map reference, on the
// CPU, with a hash of a few bits injected so that pure keys collide all the time.
//
//   pkeys_host <hash bits> <ops> <values> <seed>
//
// Random interns, pins, unpins and sweeps against a fake "device holds these keys" set.  After every operation:
//   * distinct live values have distinct keys; a value keeps its key while its entry lives;
//   * the first owner of a pure key gets the pure key; the tag nibble is the value's; no key is 0 or all-ones;
//   * a sweep's candidates are exactly the unpinned entries last interned before E, and it drops exactly those of
//     them that the device does not hold and that were not hit between sweep_begin and sweep_finish;
//   * a dropped value that returns is interned again (possibly under another key).
// Then eight threads intern overlapping values into one dictionary and must agree on every key.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "../sentinel_amd/csrc/pkeys.h"

using namespace sg::pk;

static unsigned g_bits = 6;
struct Weak {
    static uint64_t text(const char* s) { return StdHash::text(s) & ((1ull << g_bits) - 1); }
    static uint64_t bits(uint64_t u) { return mix64(u) & ((1ull << g_bits) - 1); }
};

struct Rng {
    uint64_t s;
    uint64_t next() { s += 0x9E3779B97F4A7C15ull; return mix64(s); }
    uint64_t below(uint64_t n) { return next() % n; }
};

struct Value {
    std::string text, type;
    uint32_t tag;
};
// value i of the space: Strings, longs outside +-2^59 and doubles in turn
static Value value(uint64_t i) {
    char buf[64];
    switch (i % 3) {
    case 0: std::snprintf(buf, sizeof(buf), "s%" PRIu64, i); return {buf, "java.lang.String", 1};
    case 1: std::snprintf(buf, sizeof(buf), "%lld", (i & 2 ? -1 : 1) * ((1LL << 59) + (long long)i)); return {buf, "long", 3};
    default: std::snprintf(buf, sizeof(buf), "%.17g", 0.25 + 0.5 * (double)i); return {buf, "java.lang.Double", 4};
    }
}

struct Ref {
    uint64_t key, pure, touched;
    uint32_t pins;
};

#define CHECK(c, ...)                                                       \
    do {                                                                    \
        if (!(c)) {                                                         \
            std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c);         \
            std::printf(__VA_ARGS__);                                       \
            std::printf("\n");                                              \
            return 1;                                                       \
        }                                                                   \
    } while (0)

static int churn(uint64_t ops, uint64_t nvalues, uint64_t seed) {
    Dict<Weak> d;
    Rng rng{seed};
    std::map<uint64_t, Ref> ref;          // value index -> entry
    std::map<uint64_t, uint64_t> owner;   // key -> value index
    std::set<uint64_t> held;              // keys the fake device holds
    uint64_t epoch = 0, sweeps = 0, returned = 0, rekeyed = 0;
    std::map<uint64_t, uint64_t> last_key;  // value index -> the key of its last (dropped) entry

    auto intern = [&](uint64_t i, bool pin) -> int {
        const Value v = value(i);
        const uint64_t pure = pure_key<Weak>(v.text.c_str(), v.type.c_str());
        const uint64_t k = d.intern(v.text.c_str(), v.type.c_str(), pin);
        CHECK(k != 0 && k != ~0ull, "value %" PRIu64, i);
        CHECK((k >> 60) == v.tag, "value %" PRIu64 " key %016" PRIx64, i, k);
        if (v.tag == 3) CHECK(k & LONG_HASHED, "hashed long without its bit: %016" PRIx64, k);
        auto it = ref.find(i);
        if (it != ref.end()) {
            CHECK(k == it->second.key, "value %" PRIu64 " changed key while live", i);
            it->second.touched = epoch;
            if (pin) it->second.pins++;
            return 0;
        }
        CHECK(!owner.count(k), "value %" PRIu64 " got the key of live value %" PRIu64, i, owner[k]);
        if (!owner.count(pure)) CHECK(k == pure, "pure key free, yet value %" PRIu64 " was stepped", i);
        if (last_key.count(i)) { ++returned; if (last_key[i] != k) ++rekeyed; }
        ref[i] = Ref{k, pure, epoch, pin ? 1u : 0u};
        owner[k] = i;
        return 0;
    };
    auto stats_match = [&]() -> int {
        uint64_t displaced = 0, pinned = 0;
        for (auto& kv : ref) { displaced += kv.second.key != kv.second.pure; pinned += kv.second.pins > 0; }
        const Stats s = d.stats();
        CHECK(s.entries == ref.size() && s.displaced == displaced && s.pinned == pinned,
              "stats %" PRIu64 "/%" PRIu64 "/%" PRIu64 " vs %zu/%" PRIu64 "/%" PRIu64, s.entries, s.displaced,
              s.pinned, ref.size(), displaced, pinned);
        return 0;
    };

    CHECK(d.intern(nullptr, "java.lang.String") == 0, "NULL value");
    CHECK(d.intern("7", "int") == pure_key<Weak>("7", "int") && d.stats().entries == 0, "exact kinds store nothing");
    for (uint64_t op = 0; op < ops; ++op) {
        const uint64_t what = rng.below(100);
        if (what < 70) {
            if (intern(rng.below(nvalues), false)) return 1;
        } else if (what < 75) {
            if (intern(rng.below(nvalues), true)) return 1;
        } else if (what < 80) {
            if (ref.empty()) continue;
            auto it = ref.lower_bound(rng.below(nvalues));
            if (it == ref.end()) it = ref.begin();
            if (!it->second.pins) continue;
            d.unpin(it->second.key);
            it->second.pins--;
        } else if (what < 92) {  // the device takes up or lets go of a live key
            if (ref.empty()) continue;
            auto it = ref.lower_bound(rng.below(nvalues));
            if (it == ref.end()) it = ref.begin();
            if (!held.erase(it->second.key)) held.insert(it->second.key);
        } else {
            std::vector<uint64_t> cand;
            const uint64_t E = d.sweep_begin(cand);
            CHECK(E == epoch, "epoch %" PRIu64 " vs %" PRIu64, E, epoch);
            epoch = E + 1;
            std::set<uint64_t> want;
            for (auto& kv : ref)
                if (!kv.second.pins && kv.second.touched < E) want.insert(kv.second.key);
            CHECK(std::set<uint64_t>(cand.begin(), cand.end()) == want && cand.size() == want.size(),
                  "sweep %" PRIu64 ": %zu candidates, %zu expected", sweeps, cand.size(), want.size());
            // an intern hits a candidate the device does not hold while the device is scanning
            uint64_t hit = ~0ull;
            for (uint64_t k : cand)
                if (!held.count(k) && rng.below(4) == 0) { hit = owner[k]; break; }
            if (hit != ~0ull && intern(hit, false)) return 1;
            std::vector<uint32_t> marks((cand.size() + 31) / 32, 0u);
            for (size_t i = 0; i < cand.size(); ++i)
                if (held.count(cand[i])) marks[i >> 5] |= 1u << (i & 31);
            const uint64_t dropped = d.sweep_finish(E, cand, marks.data());
            uint64_t expect = 0;
            for (uint64_t k : cand) {
                const uint64_t i = owner[k];
                if (held.count(k) || i == hit) continue;
                last_key[i] = k;
                ref.erase(i);
                owner.erase(k);
                ++expect;
            }
            CHECK(dropped == expect, "sweep %" PRIu64 " dropped %" PRIu64 ", expected %" PRIu64, sweeps, dropped, expect);
            if (sweeps == 0) CHECK(dropped == 0, "the first sweep dropped %" PRIu64, dropped);
            ++sweeps;
            for (auto it = held.begin(); it != held.end();)  // (a held key's entry is never dropped)
                if (!owner.count(*it)) it = held.erase(it); else ++it;
        }
        if ((op & 255) == 0 && stats_match()) return 1;
    }
    if (stats_match()) return 1;
    for (auto& kv : ref) {  // every survivor still interns to its key
        const Value v = value(kv.first);
        CHECK(d.intern(v.text.c_str(), v.type.c_str()) == kv.second.key, "survivor %" PRIu64, kv.first);
    }
    std::printf("churn ok: %" PRIu64 " sweeps, %zu entries, %" PRIu64 " returned (%" PRIu64 " under another key)\n", sweeps,
                ref.size(), returned, rekeyed);
    return 0;
}

static int threads(uint64_t nvalues, uint64_t seed) {
    Dict<Weak> d;
    const int T = 8;
    const uint64_t per = 20000;
    std::vector<std::map<uint64_t, uint64_t>> seen(T);
    std::vector<int> bad(T, 0);
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t)
        th.emplace_back([&, t]() {
            Rng rng{seed + 1000 * (uint64_t)t};
            for (uint64_t n = 0; n < per; ++n) {
                const uint64_t i = rng.below(nvalues);
                const Value v = value(i);
                const uint64_t k = d.intern(v.text.c_str(), v.type.c_str());
                auto it = seen[t].find(i);
                if (it == seen[t].end()) seen[t][i] = k;
                else if (it->second != k) bad[t] = 1;
            }
        });
    for (auto& x : th) x.join();
    std::map<uint64_t, uint64_t> key_of, value_of;
    for (int t = 0; t < T; ++t) {
        CHECK(!bad[t], "thread %d saw a value change key", t);
        for (auto& kv : seen[t]) {
            auto it = key_of.find(kv.first);
            if (it == key_of.end()) {
                CHECK(!value_of.count(kv.second), "two values share key %016" PRIx64, kv.second);
                key_of[kv.first] = kv.second;
                value_of[kv.second] = kv.first;
            } else CHECK(it->second == kv.second, "threads disagree on value %" PRIu64, kv.first);
        }
    }
    CHECK(d.stats().entries == key_of.size(), "entries");
    std::printf("threads ok: %zu values\n", key_of.size());
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 5) { std::printf("usage: pkeys_host <hash bits> <ops> <values> <seed>\n"); return 2; }
    g_bits = (unsigned)std::atoi(argv[1]);
    const uint64_t ops = std::strtoull(argv[2], nullptr, 10), nvalues = std::strtoull(argv[3], nullptr, 10);
    const uint64_t seed = std::strtoull(argv[4], nullptr, 10);
    if (g_bits < 1 || g_bits > 60 || !nvalues) return 2;
    if (churn(ops, nvalues, seed)) return 1;
    if (threads(nvalues, seed)) return 1;
    return 0;
}
