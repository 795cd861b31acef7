// embedded.h -- the embedded token server on the decision path: which ENTRY asks for a cluster token, and what the
// answer means to the entry.
//
// The single home of these two rules, for the host and the device alike.  It needs neither HIP nor the engine
// (tests/embedded_host.cpp drives it on the CPU); under hipcc the functions are __host__ __device__.
//
//   FlowRuleChecker.passClusterCheck (core/slots/block/flow/FlowRuleChecker.java:126-143): a cluster-mode rule asks
//     pickClusterService() (:155-163), which in a process that is the token server (ClusterStateManager.isServer())
//     is EmbeddedClusterTokenServerProvider.getServer(), for requestToken(flowId, acquireCount, prioritized).
//   FlowRuleChecker.applyTokenResult (:165-187): OK passes; SHOULD_WAIT sleeps waitInMs and passes; BLOCKED blocks;
//     NO_RULE_EXISTS, BAD_REQUEST, FAIL, TOO_MANY_REQUEST and everything else go to fallbackToLocalOrPass (:145-153),
//     which without cluster_fallback_to_local passes.
//
// An ENTRY reaches FlowSlot, and so asks, when it has a slot chain (CtSph.lookProcessChain, CtSph.java:206-227),
// Constants.ON is set (CtSph.java:128-131), its context is not a NullContext (CtSph.java:120-127), and neither
// SystemSlot (the caller's SG_F_BLOCKED_UPSTREAM) nor the resource's authority rule blocked it: both slots sit in
// front of FlowSlot (HotParamSlotChainBuilder.java:38-51).  Param rules would sit in front of it too; an eligible
// resource has none.
#pragma once
#include <stdint.h>

#include "../../include/sentinel_gpu.h"

#if defined(__HIPCC__)
#define EMB_FN __host__ __device__
#else
#define EMB_FN
#endif

namespace sg {

#define EMB_XF 64u        // Prog.xf bit of an eligible resource (dev_types.h XF_EMB)
#define EMB_NI_CHAIN 1u   // NodeInfo.flags bit of a resource with a slot chain (dev_types.h NI_CHAIN)

// True iff this event issues requestToken.  xf: the resource's Prog.xf; ni_flags: its NodeInfo.flags after the
// batch's chain grants; context_id: the event's (0 without an sg_event_ext); auth_blocked: its authority rule
// rejects the event's origin.
EMB_FN inline bool emb_requests(uint32_t kind, uint32_t flags, uint32_t xf, uint32_t ni_flags, int32_t switch_on,
                                uint32_t context_id, uint32_t max_ctx, bool auth_blocked) {
    if (kind != SG_EV_ENTRY) return false;
    if (!(xf & EMB_XF)) return false;
    if (!switch_on) return false;                    // Constants.ON == false: no chain is run
    if (context_id > max_ctx) return false;          // NullContext
    if (!(ni_flags & EMB_NI_CHAIN)) return false;    // lookProcessChain returned null
    if (flags & SG_F_BLOCKED_UPSTREAM) return false; // SystemSlot threw
    if (auth_blocked) return false;                  // AuthoritySlot threw
    return true;
}

// The word an answer leaves at the ENTRY's sorted position, in the decision word's layout (status | slot << 8 |
// wait << 16): BLOCKED -> SG_BLOCK_FLOW with the rule's slot, final; SHOULD_WAIT -> SG_PASS with the wait (clipped to
// 16 bits as every wait is), which the owner ORs in if nothing later blocks; everything else -> 0: FlowSlot passes
// (OK), or fallbackToLocalOrPass passes (no fallback rule on this path).
EMB_FN inline uint32_t emb_word(int32_t status, int32_t wait_in_ms, uint32_t slot) {
    if (status == SG_TOKEN_BLOCKED) return (uint32_t)SG_BLOCK_FLOW | ((slot & 0xFFu) << 8);
    if (status == SG_TOKEN_SHOULD_WAIT) {
        const uint32_t w = wait_in_ms < 0 ? 0u : wait_in_ms > 0xFFFF ? 0xFFFFu : (uint32_t)wait_in_ms;
        return (uint32_t)SG_PASS | (w << 16);
    }
    return 0u;
}
// the side word names a block (the low byte is a status; SG_PASS is 0)
EMB_FN inline bool emb_word_blocks(uint32_t w) { return (w & 0xFFu) != 0; }

// Answer classes of the read-back (sgx_embedded_last [1..7]), in this order
enum { EMB_A_OK = 0, EMB_A_BLOCKED, EMB_A_SHOULD_WAIT, EMB_A_TOO_MANY, EMB_A_BAD_REQUEST, EMB_A_FAIL, EMB_A_NO_RULE,
       EMB_A_N };
EMB_FN inline int emb_answer_class(int32_t status) {
    switch (status) {
    case SG_TOKEN_OK: return EMB_A_OK;
    case SG_TOKEN_BLOCKED: return EMB_A_BLOCKED;
    case SG_TOKEN_SHOULD_WAIT: return EMB_A_SHOULD_WAIT;
    case SG_TOKEN_TOO_MANY_REQUEST: return EMB_A_TOO_MANY;
    case SG_TOKEN_BAD_REQUEST: return EMB_A_BAD_REQUEST;
    case SG_TOKEN_NO_RULE_EXISTS: return EMB_A_NO_RULE;
    default: return EMB_A_FAIL;
    }
}

}  // namespace sg
