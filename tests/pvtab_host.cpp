// Host check of the token server's value table (sentinel_amd/csrc/pvtab.h): the exact __host__ __device__ hash,
// probe, dead-slot rule and capacity policy the device path uses, driven on the CPU by a random stream of calls
// (value inserts under moving windows) next to a brute-force map that never forgets a (flow, key).  Built and run
// by tests/test_pvtab_host.py.
//
// Per call of V listed values the engine's steps are restated: while claimed_ub + V fits half the table nothing
// happens; otherwise the live slots are counted, pv_plan picks a capacity (or refuses) and the live slots are
// moved by the probe.  Checked: every sum read from the table equals the brute-force map's (so dropping dead
// slots changed no decision input); after every rehash every live (flow, key) is found with equal stamps and
// counts and no dead slot remains; never more than half the slots are claimed; a refusal happens exactly when the
// maximum capacity cannot hold 2 * (live + V).
//
// usage: pvtab_host CAP_INIT CAP_MAX SAMPLE_COUNT SEED CALLS   (exit 0 = every check held)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "../sentinel_amd/csrc/pvtab.h"

using namespace sg;

static uint64_t rng_state;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct Ref {  // what pv_find + k_ptok_flow's add leave in a slot, kept for ever
    int64_t ws[CP_MAXN], cnt[CP_MAXN];
};

static void current(PFlow& F, int64_t now, int& idx) {  // cluster.hip pf_current
    const int64_t wlen = F.interval / F.n;
    idx = (int)((now / wlen) % F.n);
    const int64_t ws = now - now % wlen;
    if (F.fws[idx] < 0 || ws > F.fws[idx]) F.fws[idx] = ws;
}
static bool ref_live(const PFlow& F, const Ref& r) {  // the rule, spelled out apart from pv_live
    for (int j = 0; j < F.n; ++j)
        if (F.fws[j] >= 0 && r.ws[j] == F.fws[j]) return true;
    return false;
}
#define CHECK(c, ...)                              \
    do {                                           \
        if (!(c)) {                                \
            std::printf("FAIL %s: ", #c);          \
            std::printf(__VA_ARGS__);              \
            std::printf("\n");                     \
            return 1;                              \
        }                                          \
    } while (0)

int main(int argc, char** argv) {
    if (argc < 6) { std::printf("usage: pvtab_host CAP_INIT CAP_MAX SAMPLE_COUNT SEED CALLS\n"); return 2; }
    const uint64_t cap_init = std::strtoull(argv[1], nullptr, 0), cap_max = std::strtoull(argv[2], nullptr, 0);
    const int n = std::atoi(argv[3]);
    rng_state = std::strtoull(argv[4], nullptr, 0);
    const uint64_t calls = std::strtoull(argv[5], nullptr, 0);
    const uint32_t NF = cap_max <= 64 ? 2 : 5;  // (a small table is soon full of the flows' last windows)
    std::vector<PFlow> flows(NF);
    for (uint32_t f = 0; f < NF; ++f) {
        std::memset(&flows[f], 0, sizeof(PFlow));
        flows[f].n = f == NF - 1 && n > 1 ? n / 2 : n;  // one flow of another shape
        flows[f].interval = flows[f].n * (f % 2 ? 100 : 50);
        for (int j = 0; j < CP_MAXN; ++j) flows[f].fws[j] = -1;
    }
    uint64_t cap = cap_init, claimed_ub = 0;
    std::vector<PVal> tab(cap);
    for (auto& s : tab) { std::memset(&s, 0, sizeof(s)); s.flow = PV_EMPTY; }
    std::map<std::pair<uint32_t, uint64_t>, Ref> ref;
    int64_t now = 1000;
    uint64_t rehashes = 0, resizes = 0, refusals = 0, next_key = 1;
    // in the third quarter of the stream the live set is pushed towards cap_max / 2, so that refusals happen
    for (uint64_t c = 0; c < calls; ++c) {
        const uint64_t phase = c * 4 / calls;
        const int64_t longest = (int64_t)n * 100;  // the longest interval among the flows
        now += 1 + (int64_t)(rnd() % (uint64_t)(phase == 2 ? longest / 16 + 1 : longest / 2 + 1));
        const uint32_t V = 1 + (uint32_t)(rnd() % (phase == 2 ? cap_max / 4 + 2 : cap_max / 32 + 1));
        std::vector<std::pair<uint32_t, uint64_t>> vals(V);
        for (auto& v : vals) {
            v.first = (uint32_t)(rnd() % NF);
            // mostly never-seen keys, some recent ones again (their moved counts are read)
            v.second = (rnd() % 3) ? next_key++ : 1 + rnd() % next_key;
            // (a small table: mostly a few keys over and over, or the flows' last windows alone fill half of it)
            if (cap_max <= 64 && phase != 2 && rnd() % 8) v.second = 1 + rnd() % (cap_max / 8);
            if (rnd() % 64 == 0) v.second = ~0ull - rnd() % 4;  // keys next to the top of the range
        }
        if (!pv_has_room(claimed_ub, V, cap)) {
            uint64_t live = 0;
            for (auto& s : tab) live += s.flow != PV_EMPTY && pv_live(flows[s.flow], s);
            uint64_t ref_n = 0;
            for (auto& kv : ref) ref_n += ref_live(flows[kv.first.first], kv.second);
            CHECK(live == ref_n, "live count %llu, reference %llu", (unsigned long long)live, (unsigned long long)ref_n);
            const uint64_t ncap = pv_plan(live, V, cap_init, cap_max);
            const bool must_refuse = 2 * (live + V) > cap_max;
            CHECK((ncap == 0) == must_refuse, "plan %llu with live %llu V %u max %llu", (unsigned long long)ncap,
                  (unsigned long long)live, V, (unsigned long long)cap_max);
            if (!ncap) { ++refusals; continue; }  // refused: nothing changed, the call's values are never seen
            CHECK((ncap & (ncap - 1)) == 0 && ncap >= cap_init && ncap <= cap_max, "capacity %llu", (unsigned long long)ncap);
            CHECK((ncap == cap_max || live + V <= ncap / 4) && (ncap == cap_init || live + V > ncap / 8),
                  "capacity %llu is not the smallest with a quarter claimed (live %llu V %u)", (unsigned long long)ncap,
                  (unsigned long long)live, V);
            std::vector<PVal> nt(ncap);
            for (auto& s : nt) { std::memset(&s, 0xFF, sizeof(s)); }
            uint64_t moved = 0;
            for (auto& s : tab) {
                if (s.flow == PV_EMPTY || !pv_live(flows[s.flow], s)) continue;
                const uint64_t h = pv_probe(nt.data(), ncap, s.flow, s.key);
                CHECK(h < ncap && nt[h].flow == PV_EMPTY, "no free slot for a live pair");
                nt[h] = s;
                ++moved;
            }
            CHECK(moved == live, "moved %llu of %llu", (unsigned long long)moved, (unsigned long long)live);
            for (auto& s : tab) {  // a kept slot is carried whole: key, every stamp, every count
                if (s.flow == PV_EMPTY || !pv_live(flows[s.flow], s)) continue;
                const uint64_t h = pv_probe(nt.data(), ncap, s.flow, s.key);
                CHECK(h < ncap && !std::memcmp(&nt[h], &s, sizeof(PVal)), "slot (%u, %llu) changed in the move", s.flow,
                      (unsigned long long)s.key);
            }
            tab.swap(nt);
            if (ncap != cap) ++resizes;
            cap = ncap;
            claimed_ub = live;
            ++rehashes;
            for (auto& kv : ref) {  // every live pair: found, equal; every dead one: gone
                const uint64_t h = pv_probe(tab.data(), cap, kv.first.first, kv.first.second);
                CHECK(h < cap, "probe ran round the table");
                const bool found = tab[h].flow != PV_EMPTY;
                const bool lv = ref_live(flows[kv.first.first], kv.second);
                CHECK(found == lv, "pair (%u, %llu): live %d found %d", kv.first.first, (unsigned long long)kv.first.second,
                      (int)lv, (int)found);
                // (a pair that was dropped once and came back has fresh stamps where the reference has stale
                // ones: equal wherever the flow's stamp can still be met)
                const PFlow& F = flows[kv.first.first];
                for (int j = 0; found && j < F.n; ++j) {
                    const bool a = tab[h].ws[j] == F.fws[j], b = kv.second.ws[j] == F.fws[j];
                    CHECK(F.fws[j] < 0 || (a == b && (!a || tab[h].cnt[j] == kv.second.cnt[j])),
                          "pair (%u, %llu) bucket %d differs from the reference", kv.first.first,
                          (unsigned long long)kv.first.second, j);
                }
            }
            uint64_t claimed = 0;
            for (auto& s : tab) claimed += s.flow != PV_EMPTY;
            CHECK(claimed == live, "claimed %llu after a rehash that kept %llu", (unsigned long long)claimed,
                  (unsigned long long)live);
            CHECK(pv_has_room(claimed_ub, V, cap), "no room after the rehash");
        }
        claimed_ub += V;
        for (auto& v : vals) {  // getSum, then addValue: k_ptok_flow for one value
            PFlow& F = flows[v.first];
            int idx;
            current(F, now, idx);
            int64_t sum = 0, rsum = 0;
            uint64_t h = pv_probe(tab.data(), cap, v.first, v.second);
            CHECK(h < cap, "the table is full");
            auto it = ref.find(v);
            for (int j = 0; j < F.n; ++j) {
                if (F.fws[j] < 0 || now - F.fws[j] > F.interval) continue;
                if (tab[h].flow != PV_EMPTY && tab[h].ws[j] == F.fws[j]) sum += tab[h].cnt[j];
                if (it != ref.end() && it->second.ws[j] == F.fws[j]) rsum += it->second.cnt[j];
            }
            CHECK(sum == rsum, "sum %lld, reference %lld", (long long)sum, (long long)rsum);
            if (tab[h].flow == PV_EMPTY) pv_fresh(tab[h], v.first, v.second);
            if (it == ref.end()) {
                Ref r;
                for (int j = 0; j < CP_MAXN; ++j) { r.ws[j] = -1; r.cnt[j] = 0; }
                it = ref.emplace(v, r).first;
            }
            const int64_t acq = 1 + (int64_t)(rnd() % 3);
            if (tab[h].ws[idx] != F.fws[idx]) { tab[h].ws[idx] = F.fws[idx]; tab[h].cnt[idx] = 0; }
            tab[h].cnt[idx] += acq;
            if (it->second.ws[idx] != F.fws[idx]) { it->second.ws[idx] = F.fws[idx]; it->second.cnt[idx] = 0; }
            it->second.cnt[idx] += acq;
        }
        uint64_t claimed = 0;
        for (auto& s : tab) claimed += s.flow != PV_EMPTY;
        CHECK(claimed <= claimed_ub && claimed_ub <= cap / 2, "claimed %llu, bound %llu, capacity %llu",
              (unsigned long long)claimed, (unsigned long long)claimed_ub, (unsigned long long)cap);
    }
    std::printf("ok: %llu calls, %llu pairs, %llu rehashes (%llu resizes), %llu refusals, capacity %llu\n",
                (unsigned long long)calls, (unsigned long long)ref.size(), (unsigned long long)rehashes,
                (unsigned long long)resizes, (unsigned long long)refusals, (unsigned long long)cap);
    CHECK(rehashes > 0, "the stream never rehashed");
    return 0;
}
