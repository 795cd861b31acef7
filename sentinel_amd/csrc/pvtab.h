// pvtab.h -- the token server's (flow, value) count table (dev_types.h PVal): slot hash, probe, the dead-slot
// rule and the capacity policy, shared by k_ptok_flow's pv_find and the rehash kernel (cluster.hip), the rule
// load (engine.cpp rebuild_cluster_param) and tests/pvtab_host.cpp.
//
// Reference: a flow's ClusterParameterLeapArray keeps one value map per bucket and clears it on every window
// reset (csrv/flow/statistic/metric/ClusterParameterLeapArray.java:30-58), so ClusterParamMetric.getSum
// (ClusterParamMetric.java:53-85) only ever sees the values of the last windowIntervalMs.  Here a value's counts
// sit in one PVal slot, stamped per bucket with the window start they were added under.
//
// The dead-slot rule.  A slot s of flow F is live iff some j < F.n has F.fws[j] >= 0 && s.ws[j] == F.fws[j].
// A count is read only while its stamp equals the flow's (k_ptok_flow's sum loop), and a flow's fws[j] only moves
// forward (pf_current), so a slot with no equal stamp adds 0 to every sum from now on: dropping it and claiming
// a fresh one later (all stamps -1) decides the same.  The rule looks at stamps only, never at the clock: a
// bucket that matches but is deprecated by time could be read again if the next call's clock lay earlier, and the
// param path checks the order of requests inside one call only.
//
// The capacity policy.  The host keeps claimed_ub, an upper bound on the claimed slots (exact after a rehash or
// a rule load, plus the listed values of every call since: a call claims at most one slot per listed value).
// A call of V listed values runs as it is while claimed_ub + V <= capacity / 2.  Otherwise the live slots are
// counted and moved into the smallest power-of-two capacity in [initial, maximum] that leaves at most a quarter
// claimed counting V (so the next rehash is a table's worth of claims away), or into the maximum while that
// leaves at most half; when even that is out of reach the call is refused before anything changed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_types.h"

#define PV_FN __host__ __device__

namespace sg {

PV_FN inline uint64_t pv_mix(int64_t k) {  // the token server tables' mix (cluster.hip tab_hash)
    uint64_t z = (uint64_t)k + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// home slot of (flow index, value key) before masking; the probe is linear: (h + 1) & mask
PV_FN inline uint64_t pv_hash(uint32_t f, uint64_t key) {
    return pv_mix((int64_t)(key ^ ((uint64_t)f * 0xD6E8FEB86659FD93ull)));
}
PV_FN inline bool pv_live(const PFlow& F, const PVal& s) {
    for (int j = 0; j < F.n && j < CP_MAXN; ++j)
        if (F.fws[j] >= 0 && s.ws[j] == F.fws[j]) return true;
    return false;
}
// One caller at a time (the host, or a lane that owns the flow): the slot of (f, key), else the free slot that
// ends its probe, else (table full of other pairs) cap.
PV_FN inline uint64_t pv_probe(const PVal* tab, uint64_t cap, uint32_t f, uint64_t key) {
    const uint64_t mask = cap - 1;
    uint64_t h = pv_hash(f, key) & mask;
    for (uint64_t probe = 0; probe < cap; ++probe) {
        if (tab[h].flow == PV_EMPTY || (tab[h].flow == f && tab[h].key == key)) return h;
        h = (h + 1) & mask;
    }
    return cap;
}
PV_FN inline void pv_fresh(PVal& s, uint32_t f, uint64_t key) {  // what pv_find writes into a claimed slot
    s.key = key;
    s.flow = f;
    for (int j = 0; j < CP_MAXN; ++j) { s.ws[j] = -1; s.cnt[j] = 0; }
}

PV_FN inline bool pv_has_room(uint64_t claimed_ub, uint64_t V, uint64_t cap) {
    return claimed_ub <= cap / 2 && V <= cap / 2 - claimed_ub;
}
// The capacity to rehash into with `live` slots kept and V values to come; 0: refuse the call.
PV_FN inline uint64_t pv_plan(uint64_t live, uint64_t V, uint64_t cap_init, uint64_t cap_max) {
    if (live > cap_max / 2 || V > cap_max / 2 - live) return 0;
    const uint64_t need = live + V;
    uint64_t cap = cap_init;
    while (cap < cap_max && need > cap / 4) cap <<= 1;
    return cap;
}

}  // namespace sg
