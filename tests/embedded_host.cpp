// embedded_host.cpp -- sentinel_amd/csrc/embedded.h on the CPU (tests/test_embedded_host.py builds and runs it with
// the address and undefined-behaviour sanitizers): the request test against a sequential model of the slot chain
// over random small batches, the ordered compaction the extraction kernels perform with it (tile counts, exclusive
// scan, scatter) against a plain filter, and the answer -> side word mapping.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../sentinel_amd/csrc/embedded.h"

using namespace sg;

namespace {

struct Ev {
    uint32_t kind, flags, res, ctx;
    bool auth_blocked;
};
struct Res {
    bool eligible, chain;
};

// (Not an independent reference: the model restates the same conditions in the order the reference walks them, so it
// catches a dropped term or an inverted sense in emb_requests(), not a misreading of the slot order that both share;
// that order is pinned by the GPU cases of tests/test_gpu_embedded.py against the oracle.  The compaction below is
// checked against a plain filter.)
// The slot chain as CtSph.entryWithPriority and the slots walk it (CtSph.java:117-166,
// HotParamSlotChainBuilder.java:38-51), one step after the other: what happens to the entry before FlowSlot.
bool model_reaches_cluster_rule(const Ev& e, const Res& r, bool on, uint32_t max_ctx) {
    if (e.kind != SG_EV_ENTRY) return false;           // an EXIT or a TRACE enters nothing
    if (e.ctx > max_ctx) return false;                 // NullContext: new CtEntry(resourceWrapper, null, context)
    if (!on) return false;                             // !Constants.ON: the same
    if (!r.chain) return false;                        // lookProcessChain == null
    // StatisticSlot, ParamFlowSlot (no param rule on an eligible resource), then SystemSlot and AuthoritySlot
    if (e.flags & SG_F_BLOCKED_UPSTREAM) return false; // SystemSlot throws
    if (e.auth_blocked) return false;                  // AuthoritySlot throws
    return r.eligible;                                 // FlowSlot: the resource's rule is the embedded cluster rule
}

int fails = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            ++fails;                                                    \
        }                                                               \
    } while (0)

}  // namespace

int main() {
    std::mt19937_64 rng(20240611);
    const uint32_t max_ctx = SG_MAX_CONTEXTS;
    for (int batch = 0; batch < 400; ++batch) {
        const uint32_t nres = 1 + rng() % 9, n = (uint32_t)(rng() % 700);
        const bool on = rng() % 8 != 0;
        std::vector<Res> res(nres);
        for (auto& r : res) { r.eligible = rng() % 2; r.chain = rng() % 4 != 0; }
        std::vector<Ev> ev(n);
        for (auto& e : ev) {
            e.kind = rng() % 5 < 3 ? SG_EV_ENTRY : (rng() % 2 ? SG_EV_EXIT : SG_EV_TRACE);
            e.flags = (uint32_t)(rng() % 32);
            e.res = (uint32_t)(rng() % nres);
            e.ctx = rng() % 6 == 0 ? max_ctx + 1 + (uint32_t)(rng() % 3) : (uint32_t)(rng() % 4);
            e.auth_blocked = rng() % 7 == 0;
        }
        auto pred = [&](uint32_t i) {
            const Ev& e = ev[i];
            const uint32_t xf = (res[e.res].eligible ? EMB_XF : 0u) | (uint32_t)(rng() % 64);  // other Prog.xf bits
            const uint32_t ni = (res[e.res].chain ? EMB_NI_CHAIN : 0u) | (uint32_t)((rng() % 64) << 1);
            return emb_requests(e.kind, e.flags, xf, ni, on ? 1 : 0, e.ctx, max_ctx, e.auth_blocked);
        };
        std::vector<uint32_t> want;
        std::vector<char> q(n);
        for (uint32_t i = 0; i < n; ++i) {
            q[i] = pred(i);
            CHECK(q[i] == (char)model_reaches_cluster_rule(ev[i], res[ev[i].res], on, max_ctx));
            if (q[i]) want.push_back(i);
        }
        // the kernels' compaction: lanes of 4 consecutive events, tiles of 256 lanes (here 8, to cross many tiles)
        const uint32_t items = 4, lanes = 8, tile = items * lanes, nt = (n + tile - 1) / tile;
        std::vector<uint32_t> cnt(nt + 1, 0), got(want.size(), 0xFFFFFFFFu);
        for (uint32_t t = 0; t < nt; ++t)
            for (uint32_t i = t * tile; i < n && i < (t + 1) * tile; ++i) cnt[t] += q[i];
        uint32_t run = 0;
        for (uint32_t t = 0; t <= nt; ++t) { const uint32_t c = cnt[t]; cnt[t] = run; run += c; }
        CHECK(run == want.size());
        for (uint32_t t = 0; t < nt; ++t) {
            uint32_t o = cnt[t];
            for (uint32_t l = 0; l < lanes; ++l)
                for (uint32_t k = 0; k < items; ++k) {
                    const uint32_t i = t * tile + l * items + k;
                    if (i < n && q[i]) got[o++] = i;
                }
            CHECK(o == cnt[t + 1]);
        }
        CHECK(got == want);
    }
    // answers
    CHECK(emb_word(SG_TOKEN_OK, 0, 3) == 0);
    CHECK(emb_word(SG_TOKEN_BLOCKED, 99, 3) == ((uint32_t)SG_BLOCK_FLOW | (3u << 8)));
    CHECK(emb_word_blocks(emb_word(SG_TOKEN_BLOCKED, 0, 0)));
    CHECK(emb_word(SG_TOKEN_SHOULD_WAIT, 250, 3) == (250u << 16));
    CHECK(emb_word(SG_TOKEN_SHOULD_WAIT, 1 << 20, 0) == (0xFFFFu << 16));
    CHECK(emb_word(SG_TOKEN_SHOULD_WAIT, -5, 0) == 0);
    CHECK(!emb_word_blocks(emb_word(SG_TOKEN_SHOULD_WAIT, 250, 0)));
    const int pass[] = {SG_TOKEN_TOO_MANY_REQUEST, SG_TOKEN_BAD_REQUEST, SG_TOKEN_FAIL, SG_TOKEN_NO_RULE_EXISTS, 77};
    for (int s : pass) CHECK(emb_word(s, 123, 1) == 0);  // fallbackToLocalOrPass without a fallback: pass
    bool seen[EMB_A_N] = {};
    const int all[] = {SG_TOKEN_OK, SG_TOKEN_BLOCKED, SG_TOKEN_SHOULD_WAIT, SG_TOKEN_TOO_MANY_REQUEST,
                       SG_TOKEN_BAD_REQUEST, SG_TOKEN_FAIL, SG_TOKEN_NO_RULE_EXISTS};
    for (int s : all) {
        const int c = emb_answer_class(s);
        CHECK(c >= 0 && c < EMB_A_N && !seen[c]);
        seen[c] = true;
    }
    CHECK(emb_answer_class(12345) == EMB_A_FAIL);
    if (fails) return 1;
    std::printf("ok\n");
    return 0;
}
