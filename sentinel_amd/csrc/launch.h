// launch.h -- the host-callable launchers of the .hip files, and the constants of theirs the host sizes buffers by.
// engine.cpp and every .hip that defines or calls one include it, so a launcher has one declaration.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_types.h"

namespace sg {
// ---- kernels.hip
hipError_t launch_rs_first(const sg_event* ev, uint64_t n, uint32_t max_res, uint64_t gbase, const uint8_t* ring,
                           uint64_t ring_mask, int32_t max_rt, SEv* rec_o, uint32_t* keys, uint32_t* vals,
                           uint32_t* ghist, uint32_t nblocks, uint32_t* bflags, int64_t* t0_out, uint32_t* prio,
                           uint64_t* key_ring, const uint32_t* comp, const sg_event_ext* ext, const sg_arg* args,
                           uint64_t n_args, uint32_t max_ctx, const AuthDesc* auth, const uint32_t* auth_ids,
                           uint32_t ublk, hipStream_t st);
hipError_t launch_radix_hist(const uint32_t* keys, uint64_t n, int shift, uint32_t* ghist, uint32_t nblocks,
                             hipStream_t st);
hipError_t launch_radix_hist_n(const uint32_t* keys, uint64_t n, const uint32_t* ndev, int shift, uint32_t* ghist,
                               uint32_t nblocks, hipStream_t st);
hipError_t launch_radix_scatter_n(const uint32_t* kin, const uint32_t* vin, uint64_t n, const uint32_t* ndev, int shift,
                                  const uint32_t* goff, uint32_t nblocks, uint32_t* kout, uint32_t* vout, hipStream_t st);
hipError_t launch_radix_scatter_x(const uint32_t* kin, const uint32_t* vin, uint64_t n, const uint32_t* ndev,
                                  const uint32_t* tcnt, const uint32_t* dbase, int shift, const uint32_t* goff,
                                  uint32_t nblocks, uint32_t* kout, uint32_t* vout, uint32_t* pos_of, hipStream_t st);
hipError_t launch_grp_first(const sg_event* ev, uint64_t n, uint32_t max_res, uint64_t gbase, uint64_t ring_mask,
                            uint32_t* bflags, int64_t* t0_out, uint32_t* prio, uint64_t* key_ring, const uint32_t* comp,
                            const sg_event_ext* ext, const sg_arg* args, uint64_t n_args, uint32_t max_ctx,
                            const AuthDesc* auth, const uint32_t* auth_ids,
                            const uint16_t* hot_tab, uint32_t nhot, uint32_t nblocks, uint32_t* words,
                            uint32_t* hot_hist, uint32_t* ckeys, uint32_t* cvals, uint32_t* ccnt, uint32_t* chist,
                            uint32_t ublk, hipStream_t st);
hipError_t launch_hot_scan(uint32_t* C, uint32_t nblocks, uint32_t nhot, uint32_t* part, uint32_t* hb, uint32_t* total,
                           hipStream_t st);
hipError_t launch_hot_bmax(const sg_event* ev, uint32_t nblocks, const uint32_t* P, uint32_t nhot, const uint32_t* hb,
                           uint32_t* edges, uint32_t* bmax, hipStream_t st);
hipError_t launch_grp_records(const sg_event* ev, uint64_t n, uint64_t gbase, uint64_t ring_mask, int32_t max_rt,
                              const uint32_t* words, const uint32_t* P, uint32_t nhot, uint32_t nblocks,
                              const uint32_t* hb, SEv* recs, uint32_t* svals, uint32_t* prev,
                              uint32_t* nprev, uint32_t* bst, uint32_t* bflags, const sg_event_ext* ext,
                              const sg_arg* args, uint32_t max_ctx, Link* link, uint32_t epoch,
                              const uint32_t* need_hot, const uint32_t* need_blk, uint32_t max_res,
                              const AuthDesc* auth, const uint32_t* auth_ids, uint32_t ublk, hipStream_t st);
hipError_t launch_hot_segs(const uint32_t* hb, uint32_t nhot, const uint32_t* hot_list, Seg* segs, uint32_t* out,
                           hipStream_t st);
hipError_t launch_hot_build(const Seg* segs, const uint32_t* mp, uint32_t mb, uint32_t min_len, uint32_t max_res, uint16_t* hot_tab,
                            uint32_t* hot_list, uint32_t nhot_old, uint32_t* hot_n, hipStream_t st);
hipError_t launch_cold_n(uint64_t n, const uint32_t* hot_total, uint32_t* out, hipStream_t st);
hipError_t launch_cold_small(const uint32_t* kin, const uint32_t* vin, const uint32_t* cnt, const uint32_t* dbase,
                             uint32_t* kout, uint32_t* vout, uint32_t* words, hipStream_t st);
uint32_t hot_max();
hipError_t launch_grp_clear(uint32_t* bsmall, uint32_t nsmall, uint32_t* bst, uint32_t nbst, uint32_t* need,
                            uint32_t nneed, hipStream_t st);
hipError_t launch_radix_scatter(const uint32_t* kin, const uint32_t* vin, uint64_t n, int shift, const uint32_t* goff,
                                uint32_t nblocks, uint32_t* kout, uint32_t* vout, uint32_t* pos_of, hipStream_t st);
uint32_t radix_tile();
hipError_t launch_scan(const uint32_t* in, uint32_t* out, uint64_t n, uint32_t* part, uint32_t* total, hipStream_t st);
// the same over the first min(n, *ndev) elements only (a count known on the device)
hipError_t launch_scan_n(const uint32_t* in, uint32_t* out, uint64_t n, const uint32_t* ndev, uint32_t* part,
                         uint32_t* total, hipStream_t st);
hipError_t launch_snapshot(Bkt*, NodeInfo*, uint32_t, int64_t, int32_t, uint32_t*, uint32_t*, uint32_t*, uint32_t*,
                           sg_metric_node*, uint64_t, hipStream_t);
hipError_t launch_init_state(Bkt* sec, Bkt* minb, NodeInfo* info, int64_t* borrow, uint32_t nres, hipStream_t st);
hipError_t launch_set_flags(NodeInfo* info, const uint64_t* upd, uint32_t n, hipStream_t st);
hipError_t launch_region_copy(const uint64_t* src, uint64_t* dst, const uint64_t* tri, uint32_t n, hipStream_t st);
hipError_t launch_emb_count(const sg_event* ev, const sg_event_ext* ext, uint64_t n, uint32_t max_res, uint32_t max_ctx,
                            const Prog* prog, const NodeInfo* info, const AuthDesc* auth, const uint32_t* auth_ids,
                            int32_t switch_on, uint32_t* cnt, uint32_t* part, uint32_t* total, hipStream_t st);
hipError_t launch_emb_scatter(const sg_event* ev, const sg_event_ext* ext, uint64_t n, uint32_t max_res, uint32_t max_ctx,
                              const Prog* prog, const NodeInfo* info, const AuthDesc* auth, const uint32_t* auth_ids,
                              int32_t switch_on, const uint32_t* off, const int64_t* flow_of, uint32_t cap,
                              sg_token_req* req, uint32_t* idx, hipStream_t st);
hipError_t launch_emb_answers(const sg_token_result* res, const uint32_t* idx, uint32_t nreq, const uint32_t* pos_of,
                              const uint32_t* words, const uint32_t* P, uint32_t nhot, uint64_t n, uint32_t* side,
                              uint32_t* stat, hipStream_t st);
hipError_t launch_post_w(const uint32_t* words, const uint32_t* P, uint32_t nhot, const uint32_t* dec, uint64_t n,
                         uint64_t gbase, uint8_t* ring, uint64_t ring_mask, uint32_t* out, hipStream_t st);
// ---- decide.hip
hipError_t launch_seg_cold(const uint32_t* keys, uint64_t n, const uint32_t* lo, const uint32_t* sbase, uint32_t* flag,
                           uint32_t* pos, Seg* segs, hipStream_t st, uint32_t* part, uint32_t* ccount, uint32_t* nseg);
hipError_t launch_block_sums(const SEv* recs, uint64_t n, uint32_t* bst, Link* link, uint32_t epoch, uint32_t* bflags,
                             const uint32_t* skeys, const uint32_t* lo, const uint32_t* need_blk, hipStream_t st);
hipError_t launch_seg(const uint32_t* keys, uint64_t n, uint32_t* flag, uint32_t* pos, Seg* segs, hipStream_t st,
                      uint32_t* part, uint32_t* nseg);
hipError_t launch_seg_bin(Seg* segs, const uint32_t* mp, uint32_t mb, uint64_t n, const Prog* prog, const uint32_t* prio,
                          uint32_t lane_max, uint32_t lite_max, uint32_t j1_max, uint32_t j4_max, uint32_t force_lane,
                          uint32_t* blkcnt, uint32_t pq_ok, uint32_t pq_wide, uint32_t* aux, uint32_t* ashort, uint64_t* along,
                          uint64_t* amulti, uint32_t* mixc, uint32_t* mix, uint32_t mix_cap, uint32_t* mixlen,
                          uint32_t mix_wide, uint32_t head_min, const uint16_t* hot_tab, uint32_t nhot,
                          const uint32_t* nhotseg, uint32_t* need_hot, uint32_t* need_blk, const uint32_t* bmax,
                          uint32_t skip_min, uint32_t* nmark, uint32_t* ubc, uint32_t* embc, uint32_t max_res,
                          hipStream_t st);
hipError_t launch_seg_order(Seg* segs, const uint32_t* mp, uint32_t mb, const uint32_t* off, uint32_t* order,
                            uint32_t* bin_off, hipStream_t st);
hipError_t launch_gather(const SEv* rec_o, const uint32_t* vals, const uint32_t* skeys, uint64_t n,
                         const uint32_t* pos_of, SEv* recs, uint32_t* prev, uint32_t* nprev, Link* link, uint32_t* bst,
                         uint32_t epoch, uint32_t* bflags, hipStream_t st);
hipError_t launch_fill(const Span* spans, const uint32_t* nspan, uint32_t cap, const SEv* recs, const Prog* prog,
                       const DRule* rules, uint32_t* dec, hipStream_t st);
hipError_t launch_resolve(const uint32_t* prev, uint32_t np, const uint8_t* ring, SEv* recs, const uint32_t* vals,
                          const sg_event_ext* ext, hipStream_t st);
hipError_t launch_ublk_words(SEv* recs, const Seg* segs, const uint32_t* order, uint32_t m, uint32_t* dec,
                             uint32_t* cnt, const uint32_t* emb, uint32_t* ecnt, hipStream_t st);
hipError_t launch_post(const uint32_t* pos_of, const uint32_t* dec, uint64_t n, uint64_t gbase, uint8_t* ring,
                       uint64_t ring_mask, uint32_t* out, hipStream_t st);
hipError_t launch_chain(const SEv* recs, const uint32_t* vals, const Seg* segs, uint32_t m, NodeInfo* info,
                        uint32_t grant_all, uint32_t* ncand, uint64_t* cand, const sg_event* ev, const Prog* prog,
                        const sg_event_ext* ext, uint32_t max_ctx, hipStream_t st);
hipError_t launch_tiny(const sg_event* ev, uint32_t n, const DevState& S, const DevCfg& cfg, uint32_t max_res,
                       uint32_t* prio_w, const uint32_t* comp, uint64_t n_args, uint32_t grant_all,
                       unsigned long long* pool_next, uint64_t pool_nb, uint32_t epoch, SEv* recs, uint32_t* vals,
                       uint32_t* dec, Seg* segs, uint32_t* bflags, uint32_t* out, hipStream_t st);
uint32_t tiny_max();
hipError_t launch_decide_bin(int bin, const SEv* recs, const sg_event* ev, const uint32_t* vals, const Seg* segs,
                             const uint32_t* order, uint32_t m, const DevState& S, const DevCfg& cfg, int64_t t0,
                             uint32_t* dec, uint32_t* bflags, hipStream_t st);
// ---- head.hip
hipError_t launch_head(const SEv* recs, const Seg* segs, const uint32_t* order, uint32_t m, const DevState& S,
                       const DevCfg& cfg, int64_t t0, uint32_t* dec, uint32_t* bflags, hipStream_t st);
// ---- param.hip
hipError_t launch_pq(int wide, const SEv* recs, const sg_event* ev, const uint32_t* vals, const Seg* segs,
                     const uint32_t* order, uint32_t m, const DevState& S, const DevCfg& cfg, int64_t t0, uint32_t* dec,
                     uint32_t* bflags, hipStream_t st);
hipError_t launch_pm_grow(const Seg* segs, const uint32_t* mp, uint32_t mb, const DevState& S, unsigned long long* pool_next,
                          uint64_t pool_nb, uint32_t* bflags, uint4* mv, uint32_t* nmv, uint32_t mcap, uint32_t epoch,
                          uint32_t nm, PBucket* b2, PData* d2, uint32_t* sz, uint32_t* off, uint32_t* part,
                          hipStream_t st);
hipError_t launch_pm_compact(PMap* pm, uint32_t n, const PBucket* ob, const PData* od, PBucket* nbk, PData* nd,
                             uint32_t* sz, uint32_t* off, uint32_t* part, unsigned long long* pool_next,
                             hipStream_t st);
hipError_t launch_pm_grow_ids(const uint32_t* ids, uint32_t n, const DevState& S, unsigned long long* pool_next,
                              uint64_t pool_nb, uint32_t* bflags, hipStream_t st);
hipError_t launch_pq_mix(int post, SEv* recs, const sg_event* ev, const uint32_t* vals, const Seg* segs,
                         const uint32_t* list, uint32_t n_narrow, uint64_t wide_off, uint32_t n_wide, const DevState& S,
                         const DevCfg& cfg, int64_t t0, uint32_t* dec, uint32_t* bflags, hipStream_t st,
                         const uint32_t* rest, const uint32_t* rest_n);
// ---- pvalue.hip
hipError_t launch_pv_a(SEv* recs, const uint32_t* vals, Seg* segs, const uint32_t* list, uint32_t m,
                       const DevState& S, const DevCfg& cfg, uint32_t* dec, PvSeg* pv, PvBuf B, uint32_t cap,
                       uint32_t* tot, uint32_t* hist, uint32_t* part, hipStream_t st, uint32_t tile, uint32_t* rest,
                       uint32_t grant_all);
hipError_t launch_pv_b(SEv* recs, Seg* segs, const uint32_t* list, uint32_t m, const DevState& S, int64_t t0,
                       uint32_t* dec, uint32_t* bflags, PvSeg* pv, PvBuf B, uint32_t cap, uint32_t* tot, uint32_t* part,
                       uint32_t jumps, hipStream_t st, uint32_t* rest);
hipError_t launch_pvt(SEv* recs, const sg_event* ev, const uint32_t* vals, Seg* segs, const uint32_t* list, uint32_t m,
                      const DevState& S, const DevCfg& cfg, uint32_t* dec, uint32_t* bflags, PvSeg* pv, PvBuf B,
                      uint32_t cap, uint32_t* tot, uint32_t* hist, uint32_t* part, hipStream_t st, uint32_t tile,
                      uint32_t* rest);
// ---- aux.hip
hipError_t launch_aux(const SEv* recs, const Seg* segs, const uint32_t* aux, const uint32_t* ashort,
                      const uint64_t* along, uint64_t* apiece, const uint64_t* amulti, const DevState& S, const DevCfg& cfg,
                      int64_t t0, const uint32_t* dec, AuxAcc* pool, uint32_t pool_cap, uint32_t* pool_n, uint64_t* meta,
                      uint32_t* bflags, hipStream_t st);
hipError_t launch_aux_cold(const SEv* recs, const Seg* segs, const uint32_t* aux, const uint32_t* ashort, const DevState& S,
                           const DevCfg& cfg, int64_t t0, const uint32_t* dec, uint32_t* bflags, hipStream_t st);
// ---- inbound.hip
hipError_t launch_inbound(const SEv* recs, const uint32_t* dec, uint64_t n, const sg_event* ev, const uint32_t* vals,
                          const DevState& S, const DevCfg& cfg, int64_t t0, InbPart* part, InbNode* node, hipStream_t st);
// ---- cluster.hip
hipError_t launch_tok_classify(const sg_token_req* req, uint64_t n, const CSlot* tab, uint32_t mask, uint32_t* fidx,
                               sg_token_result* res, uint32_t* flags, uint32_t* nskeys, uint32_t* nsvals, uint32_t nns,
                               hipStream_t st);
hipError_t launch_tok_limiter_ns(const sg_token_req* req, uint64_t n, const uint32_t* sk, const uint32_t* sv,
                                 const uint32_t* fidx, uint32_t nflows, NsLimiter* lims, const double* limits,
                                 uint32_t nns, uint32_t* keys, uint32_t* vals, sg_token_result* res, uint32_t* bflag,
                                 uint32_t* bidx, uint32_t* bstart, uint32_t* kpass, uint32_t* part, uint32_t* small,
                                 uint32_t* nsb, hipStream_t st);
hipError_t launch_tok_limiter_par(const sg_token_req* req, uint64_t n, const uint32_t* fidx, uint32_t nflows,
                                  NsLimiter* lim, double allowed, uint32_t* keys, uint32_t* vals, sg_token_result* res,
                                  uint32_t* bflag, uint32_t* cflag, uint32_t* bidx, uint32_t* cexcl, uint32_t* bstart,
                                  uint32_t* kpass, uint32_t* part, uint32_t* small, hipStream_t st);
hipError_t launch_tok_limiter(const sg_token_req* req, uint64_t n, const uint32_t* fidx, uint32_t nflows,
                              NsLimiter* lim, double allowed, uint32_t* keys, uint32_t* vals, sg_token_result* res,
                              hipStream_t st);
hipError_t launch_tok_flow(const uint32_t* skeys, const uint32_t* svals, uint64_t n, const sg_token_req* req,
                           CFlow* flows, uint32_t nflows, CBkt* bkts, double exceed, double max_occ_ratio,
                           sg_token_result* res, uint32_t* bounds, uint32_t light, uint32_t wide, hipStream_t st,
                           hipStream_t hs, hipEvent_t fork, hipEvent_t join);
hipError_t launch_ptok_flow(const uint32_t* skeys, const uint32_t* svals, uint64_t n, const sg_param_token_req* req,
                            const uint64_t* values, PFlow* flows, uint32_t nflows, const PHot* hot, PVal* tab,
                            uint32_t mask, sg_token_result* res, uint32_t* flags, const uint32_t* serial,
                            unsigned long long* ctr, hipStream_t st);
hipError_t launch_ptok_prep(const sg_param_token_req* preq, uint64_t n, uint64_t n_values, sg_token_req* treq,
                            unsigned long long* st, hipStream_t s);
hipError_t launch_ptok_elig(const uint32_t* skeys, const uint32_t* svals, uint64_t n, const sg_param_token_req* req,
                            const PFlow* flows, uint32_t nflows, uint32_t* serial, hipStream_t st);
hipError_t launch_ptok_vp(const uint32_t* skeys, const uint32_t* svals, uint64_t n, const sg_param_token_req* req,
                          const uint64_t* values, PFlow* flows, uint32_t nflows, const PHot* hot, PVal* tab,
                          uint32_t mask, const uint32_t* serial, uint32_t* dedup, uint32_t dmask, uint32_t* slotof,
                          uint32_t* rep, uint32_t* ka, uint32_t* va, uint32_t* kb, uint32_t* vb, int64_t* dts,
                          int32_t* dacq, uint32_t* hist, uint32_t* part, uint32_t tile, sg_token_result* res,
                          uint32_t* flags, unsigned long long* ctr, hipStream_t st);
hipError_t launch_pv_rehash(const PVal* src, uint64_t n_src, const PFlow* flows, uint32_t nflows, PVal* dst,
                            uint32_t dmask, uint32_t* out, hipStream_t st);
// ---- cmetrics.hip
uint32_t cm_chunk();
hipError_t launch_cm_rows(const CFlow* cflows, uint32_t ncf, const CBkt* bkts, const PFlow* pflows, uint32_t npf,
                          int64_t now, uint32_t* mask, sg_cluster_metric* rows, sg_cluster_metric* prows,
                          hipStream_t st);
hipError_t launch_cm_scan(const PVal* tab, uint64_t n_slots, const PFlow* flows, uint32_t nflows, const uint32_t* mask,
                          uint32_t* cflow, uint32_t* cidx, int64_t* csum, uint64_t* ckey, uint32_t cap, uint32_t* cnt,
                          hipStream_t st);
hipError_t launch_cm_select(const uint32_t* skeys, const uint32_t* svals, uint32_t n, const PFlow* flows, uint32_t nflows,
                            const int64_t* csum, const uint64_t* ckey, uint32_t top_n, uint32_t* bounds, uint32_t* nch,
                            uint32_t* coff, uint32_t* part, int64_t* psum, uint64_t* pkey, sg_cluster_metric* prows,
                            hipEvent_t* ev, hipStream_t st);
// ---- keysweep.hip
hipError_t launch_keysweep(const PMap* pmap, uint32_t nm, const PBucket* pbkt, uint64_t pool_nb, const uint64_t* pbm,
                           uint64_t bm_words, const uint64_t* key_ring, uint64_t ring_n, const PVal* pvtab,
                           uint64_t pv_n, const uint64_t* tkey, const uint32_t* tidx, uint32_t tmask, uint32_t* marks,
                           hipEvent_t* ev, hipStream_t st);
} // namespace sg
