// ptok_host.cpp -- the value-parallel param owner's walk on the CPU (tests/test_ptok_host.py).
//
// Two token servers take the same random calls.  A decides every flow with a literal restatement of k_ptok_flow's
// loop (cluster.hip) over a host PVal table.  B asks ptok.h's eligibility predicate per flow and call; a flow it
// accepts is decided value by value with pt_step (each value's requests alone, in time order, on a private copy of
// the slot) and its stamps are merged with pt_merge; a flow it refuses takes A's loop, as the engine does.
// After every call: equal results, equal flow stamps, equal live pairs with equal stamps and counts.
// The predicate itself is checked against what the generator did: a flow is refused exactly when the call holds a
// multi-value request of it, or its first request lies before the window start of the latest request it ever saw.
//
//   ptok_host <sampleCount> <intervalMs> <seed> <mode>     mode 0: clock never goes back, single values
//                                                          mode 1: some calls start before the last one ended
//                                                          mode 2: some flows get multi-value requests
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>

#include "../sentinel_amd/csrc/ptok.h"
#include "../sentinel_amd/csrc/pvtab.h"

using namespace sg;

struct Req {
    int64_t ts;
    uint32_t flow;
    int32_t acquire;
    std::vector<uint64_t> vals;
};
struct Res {
    int32_t status, remaining;
    bool operator==(const Res& o) const { return status == o.status && remaining == o.remaining; }
};
static int32_t d2i(double d) {  // chain.h j_d2i
    if (d != d) return 0;
    if (d >= 2147483647.0) return INT32_MAX;
    if (d <= -2147483648.0) return INT32_MIN;
    return (int32_t)d;
}

struct Server {
    std::vector<PFlow> flows;
    std::vector<PHot> hot;
    std::vector<PVal> tab;
    Server(const std::vector<PFlow>& f, const std::vector<PHot>& h, size_t cap) : flows(f), hot(h), tab(cap) {
        for (auto& s : tab) { s.flow = PV_EMPTY; s.key = ~0ull; }
    }
    PVal* find(uint32_t f, uint64_t key, bool create) {
        const uint64_t h = pv_probe(tab.data(), tab.size(), f, key);
        if (h >= tab.size()) { std::fprintf(stderr, "host table full\n"); std::exit(2); }
        if (tab[h].flow == PV_EMPTY) {
            if (!create) return nullptr;
            pv_fresh(tab[h], f, key);
        }
        return &tab[h];
    }
    // k_ptok_flow's loop over one flow's requests (idx: their positions in the call)
    void serial(uint32_t f, const std::vector<Req>& call, const std::vector<size_t>& idx, std::vector<Res>& out) {
        PFlow& F = flows[f];
        const double isec = F.interval / 1000.0;
        auto current = [&](int64_t now) {
            const int64_t wlen = F.interval / F.n;
            const int i = (int)((now / wlen) % F.n);
            const int64_t ws = now - now % wlen;
            if (F.fws[i] < 0 || ws > F.fws[i]) F.fws[i] = ws;
            return i;
        };
        for (size_t p : idx) {
            const Req& q = call[p];
            const int64_t now = q.ts;
            double remaining = -1.0;
            bool passed = true;
            for (uint64_t v : q.vals) {
                current(now);
                int64_t sum = 0;
                const PVal* pv = find(f, v, false);
                if (pv)
                    for (int j = 0; j < F.n; ++j) {
                        if (F.fws[j] < 0 || now - F.fws[j] > F.interval) continue;
                        if (pv->ws[j] == F.fws[j]) sum += pv->cnt[j];
                    }
                double raw = F.count;
                for (uint32_t hh = 0; hh < F.nhot; ++hh)
                    if (hot[F.hoff + hh].key == v) { raw = (double)hot[F.hoff + hh].count; break; }
                const double thr = F.thr_type == SG_CLUSTER_THRESHOLD_GLOBAL ? raw : raw * (double)F.connected;
                const double next = thr - (double)sum / isec - (double)q.acquire;
                remaining = next;
                if (next < 0) { passed = false; break; }
            }
            Res o{SG_TOKEN_BLOCKED, 0};
            if (passed) {
                for (uint64_t v : q.vals) {
                    const int i = current(now);
                    PVal* pv = find(f, v, true);
                    if (pv->ws[i] != F.fws[i]) { pv->ws[i] = F.fws[i]; pv->cnt[i] = 0; }
                    pv->cnt[i] += q.acquire;
                }
                if (q.vals.size() > 1) remaining = -1.0;
                o.status = SG_TOKEN_OK;
                o.remaining = d2i(remaining);
            }
            out[p] = o;
        }
    }
    // the value-parallel owner's work on one flow: chains first, every value alone, then the stamp merge
    void by_value(uint32_t f, const std::vector<Req>& call, const std::vector<size_t>& idx, std::vector<Res>& out) {
        PFlow& F = flows[f];
        const double isec = F.interval / 1000.0;
        std::map<uint64_t, std::vector<size_t>> chains;
        for (size_t p : idx) chains[call[p].vals[0]].push_back(p);
        for (auto it = chains.rbegin(); it != chains.rend(); ++it) {  // (any order of the chains)
            PVal* pv = find(f, it->first, true);
            const double thr = pt_threshold(F, hot.data(), it->first);
            PtChain c;
            for (int j = 0; j < CP_MAXN; ++j) { c.ws[j] = j < F.n ? pv->ws[j] : -1; c.cnt[j] = j < F.n ? pv->cnt[j] : 0; }
            for (size_t p : it->second) {
                const double next = pt_step(c, F.n, F.interval, isec, thr, call[p].ts, call[p].acquire);
                Res o{SG_TOKEN_BLOCKED, 0};
                if (!(next < 0)) { o.status = SG_TOKEN_OK; o.remaining = d2i(next); }
                out[p] = o;
            }
            for (int j = 0; j < F.n; ++j) { pv->ws[j] = c.ws[j]; pv->cnt[j] = c.cnt[j]; }
        }
        for (size_t p : idx) pt_merge(F, call[p].ts);
    }
};

#define CHECK(c, ...) do { if (!(c)) { std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); return 1; } } while (0)

int main(int argc, char** argv) {
    if (argc < 5) { std::fprintf(stderr, "usage: ptok_host sampleCount intervalMs seed mode\n"); return 2; }
    const int n = std::atoi(argv[1]), interval = std::atoi(argv[2]), mode = std::atoi(argv[4]);
    std::mt19937_64 rng(std::strtoull(argv[3], nullptr, 0));
    auto rnd = [&](uint64_t m) { return (uint64_t)(rng() % m); };
    const uint32_t NF = 6;
    std::vector<PFlow> flows(NF);
    std::vector<PHot> hot;
    for (uint32_t f = 0; f < NF; ++f) {
        PFlow& F = flows[f];
        F = PFlow();
        F.flow_id = 100 + f;
        F.count = f == 5 ? 0.0 : 2.0 + 3.0 * f;  // (one flow with a threshold of 0)
        F.thr_type = f % 3 == 1 ? SG_CLUSTER_THRESHOLD_AVG_LOCAL : SG_CLUSTER_THRESHOLD_GLOBAL;
        F.n = n;
        F.interval = interval;
        F.connected = 1 + (int32_t)(f % 3);
        F.hoff = (uint32_t)hot.size();
        F.nhot = f % 2 ? 2 : 0;  // hot items with a lower and a higher count than the rule's
        if (F.nhot) { hot.push_back(PHot{1, 1, 0}); hot.push_back(PHot{2, (int32_t)F.count + 9, 0}); }
        for (int j = 0; j < CP_MAXN; ++j) F.fws[j] = -1;
    }
    Server A(flows, hot, 1u << 14), B(flows, hot, 1u << 14);
    const int64_t wlen = interval / n;
    int64_t now = 1000000 + (int64_t)rnd(5000);
    std::vector<int64_t> last_ts(NF, -1);  // the latest request a flow ever saw
    uint64_t n_serial = 0, n_value = 0, n_ok = 0, n_blocked = 0;
    for (int call_no = 0; call_no < 40; ++call_no) {
        if (mode == 1 && call_no && rnd(3) == 0) now -= (int64_t)rnd(2 * (uint64_t)interval) + 1;  // the clock goes back
        else if (rnd(4) == 0) now += (int64_t)(1 + rnd(3)) * interval;                             // idle: whole intervals
        std::vector<Req> call;
        std::vector<bool> multi(NF, false);
        const int len = 1 + (int)rnd(400);
        uint64_t recent = 1;
        uint32_t recent_f = 0;
        while ((int)call.size() < len) {
            const uint64_t kind = rnd(40);
            if (kind == 0) {  // a value returns at w + interval - 1 and at w + interval
                const int64_t w = now - now % wlen;
                for (int64_t t : {w + interval - 1, w + (int64_t)interval}) {
                    now = t;
                    call.push_back(Req{now, recent_f, 1 + (int32_t)rnd(3), {recent}});
                }
                continue;
            }
            if (kind == 1) now += (int64_t)rnd((uint64_t)interval + wlen);
            else now += (int64_t)rnd(3);
            Req q;
            q.ts = now;
            q.flow = (uint32_t)rnd(NF);
            q.acquire = 1 + (int32_t)rnd(3);
            q.vals.push_back(1 + rnd(rnd(2) ? 4 : 60));
            if (mode == 2 && q.flow < 2 && rnd(4) == 0) {
                const int extra = 1 + (int)rnd(2);
                for (int k = 0; k < extra; ++k) q.vals.push_back(rnd(3) ? 1 + rnd(60) : q.vals[0]);
            }
            recent = q.vals[0];
            recent_f = q.flow;
            call.push_back(q);
        }
        std::vector<std::vector<size_t>> of(NF);
        for (size_t p = 0; p < call.size(); ++p) {
            of[call[p].flow].push_back(p);
            if (call[p].vals.size() > 1) multi[call[p].flow] = true;
        }
        std::vector<Res> ra(call.size()), rb(call.size());
        for (uint32_t f = 0; f < NF; ++f) {
            if (of[f].empty()) continue;
            A.serial(f, call, of[f], ra);
            const int64_t first = call[of[f][0]].ts;
            const bool ok = !multi[f] && pt_clock_ok(B.flows[f], first);
            // what the generator knows: the window start of the flow's latest request ever lies after `first`
            const bool back = last_ts[f] >= 0 && last_ts[f] - last_ts[f] % wlen > first;
            CHECK(ok == !(multi[f] || back), "call %d flow %u: predicate %d, multi %d, clock back %d", call_no, f,
                  (int)ok, (int)multi[f], (int)back);
            if (mode == 0) CHECK(ok, "call %d flow %u: refused without a reason", call_no, f);
            if (ok) { B.by_value(f, call, of[f], rb); n_value += of[f].size(); }
            else { B.serial(f, call, of[f], rb); n_serial += of[f].size(); }
            for (size_t p : of[f])
                if (call[p].ts > last_ts[f]) last_ts[f] = call[p].ts;
        }
        for (size_t p = 0; p < call.size(); ++p) {
            CHECK(ra[p] == rb[p], "call %d request %zu (flow %u value %llu ts %lld): serial (%d, %d), by value (%d, %d)",
                  call_no, p, call[p].flow, (unsigned long long)call[p].vals[0], (long long)call[p].ts, ra[p].status,
                  ra[p].remaining, rb[p].status, rb[p].remaining);
            (ra[p].status == SG_TOKEN_OK ? n_ok : n_blocked)++;
        }
        for (uint32_t f = 0; f < NF; ++f)
            for (int j = 0; j < CP_MAXN; ++j)
                CHECK(A.flows[f].fws[j] == B.flows[f].fws[j], "call %d flow %u: stamp %d differs (%lld, %lld)", call_no, f,
                      j, (long long)A.flows[f].fws[j], (long long)B.flows[f].fws[j]);
        for (int dir = 0; dir < 2; ++dir) {  // every live pair of one server is in the other, with equal contents
            Server& X = dir ? B : A;
            Server& Y = dir ? A : B;
            for (const PVal& s : X.tab) {
                if (s.flow == PV_EMPTY || !pv_live(X.flows[s.flow], s)) continue;
                const PVal* o = Y.find(s.flow, s.key, false);
                CHECK(o, "call %d: live pair (%u, %llu) missing on the other side", call_no, s.flow,
                      (unsigned long long)s.key);
                for (int j = 0; j < n; ++j)
                    CHECK(o->ws[j] == s.ws[j] && o->cnt[j] == s.cnt[j], "call %d: pair (%u, %llu) bucket %d differs",
                          call_no, s.flow, (unsigned long long)s.key, j);
            }
        }
    }
    CHECK(n_ok && n_blocked, "the stream decided nothing both ways (%llu ok, %llu blocked)", (unsigned long long)n_ok,
          (unsigned long long)n_blocked);
    CHECK(n_value, "no flow went value by value");
    if (mode) CHECK(n_serial, "mode %d never refused a flow", mode);
    std::printf("ok: %llu ok, %llu blocked, %llu by value, %llu serial\n", (unsigned long long)n_ok,
                (unsigned long long)n_blocked, (unsigned long long)n_value, (unsigned long long)n_serial);
    return 0;
}
