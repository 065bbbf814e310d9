// Kernel choice and launch geometry of the attention family (attn_fwd.hip, attn_decode.hip, attn_bwd.hip), as plain
// C++17: which instantiation a descriptor gets and with what grid, block and LDS size is decided here, without touching
// the device, so that the rule can be compiled and tested by the host compiler alone (tests/test_attn_plan_cpu.py).
// attention.hip validates, plans, launches; the kernels share the grid numbering and the key split below.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/coral_amd.h"

#ifndef CA_PLAN_FN
#if defined(__HIPCC__)
#define CA_PLAN_FN __host__ __device__ __forceinline__
#else
#define CA_PLAN_FN inline
#endif
#endif

// XCD-aware placement.  Workgroups are dealt round-robin over the 8 XCDs by linear id, and each XCD has
// its own L2.  All tiles of one (batch, head) stream the same K/V (or Q/dO) panels, so they are placed
// on ONE XCD: the i-th workgroup of XCD x works on tile (i % ntile) of pair (i / ntile) * 8 + x.  With the
// plain (tile, head, batch) grid every XCD fetched every panel from HBM (6.5x the algorithmic bytes in
// the PMC counters); placement only affects speed.
// (tile, head, clip) of block `L` of attn_grid(ntile, H, B) blocks; false = padding block
CA_PLAN_FN bool attn_tile_of(int L, int ntile, int H, int B, int& tile, int& h, int& b) {
  const int x = L & 7, i = L >> 3;
  const int pair = (i / ntile) * 8 + x;
  tile = i % ntile;
  if (pair >= H * B) return false;
  h = pair % H;
  b = pair / H;
  return true;
}
CA_PLAN_FN unsigned attn_grid(int ntile, int H, int B) { return (unsigned)(((H * B + 7) / 8) * 8 * ntile); }

// Key split of the single-query attention forms (attn_fwd_smallq_kernel and decode.hip's cross-attention phase): the keys
// of (clip, head) item i go to `ns` workgroups for i < tail_start and to `ns_tail` for the others.  Parts of an item are
// consecutive sub-items; sub-items are numbered items-first.
struct CaKeySplit {
  int ns, tail_start, ns_tail;
};
// How many workgroups share one (clip, head)'s keys: CUs / (clips x heads), at most CA_ATTN_SPLIT_MAX (8 clips x 16 heads on
// 256 CUs: 2; 1 clip: 4; 16 x 16: 1).  ONE rule for ca_attn_fwd, ca_decode_attn_qproj and ca_whisper_decode_token
// (decode.hip): the merge order, and so the bits, are the same.  (Round 6, measured and dropped: splitting EVERY item where
// clips x heads exceeds the CUs so that the rounds come out even - whisper-large at 16 clips, 320 items -> 1280
// quarter-items - took the persistent token from 3.04 to 3.17 ms and the launch sequence from 4.5 to 6.3: every part pays
// the prologue, the barriers and the merge.)
// More items than CUs, fewer than two rounds of them (whisper-large at 16 clips: 320 on 256): the items of the second,
// partly filled round - and only they - are split so that their parts fill it: 64 items x 4 parts, a quarter of the keys
// each, beside 256 whole items.  Same box, per token: persistent launch 2.97 -> 2.74 ms, launch sequence 4.48 -> 4.02
// (NOTEBOOK R6.5); tail_on = 0 (CA_ATTN_SPLIT_TAIL=0) keeps whole items.
inline CaKeySplit ca_attn_key_split(int bh, int ncu, int cap, int tail_on) {
  cap = cap > CA_ATTN_SPLIT_MAX ? CA_ATTN_SPLIT_MAX : cap;
  CaKeySplit s;
  s.ns = 1; s.tail_start = bh; s.ns_tail = 1;
  if (bh <= ncu) {
    int ns = ncu / bh;
    ns = ns > cap ? cap : ns;
    s.ns = ns < 2 ? 1 : ns;
  } else if (bh < 2 * ncu && tail_on) {
    const int t = bh - ncu;
    int nt = ncu / t;
    nt = nt > cap ? cap : nt;
    if (nt >= 2) {
      s.tail_start = ncu;
      s.ns_tail = nt;
    }
  }
  return s;
}
CA_PLAN_FN int ca_key_split_parts(const CaKeySplit& s, int bh) {
  return s.tail_start * s.ns + (bh - s.tail_start) * s.ns_tail;
}
// sub-item `it` -> its item, its place among the item's n parts, the item's first sub-item
CA_PLAN_FN void ca_key_split_item(const CaKeySplit& s, int it, int& bh, int& sp, int& n, int& part0) {
  const int head = s.tail_start * s.ns;
  if (it < head) {
    n = s.ns;
    bh = it / n;
    part0 = bh * n;
  } else {
    n = s.ns_tail;
    const int t = (it - head) / n;
    bh = s.tail_start + t;
    part0 = head + t * n;
  }
  sp = it - part0;
}

// ---- tuning values -------------------------------------------------------------------------------------------------
// The environment knobs and the device's CU count, read once (attn_knobs() in attn_decode.hip).
struct AttnKnobs {
  int wide = 1;            // CA_ATTN_WIDE: 0 keeps the 64-query forward / dQ kernels
  int wpe3 = 1;            // CA_ATTN_WPE3: forward, head_dim <= 64 without dropout at three workgroups per CU; 0 keeps two (A/B)
  int dq_wpe3 = 1;         // CA_ATTN_DQ_WPE3: the same for dQ
  int dkv_wide = 1;        // CA_ATTN_DKV_WIDE: 0 keeps the 64-key dK|dV kernel
  int dkv_wpe3 = 0;        // CA_ATTN_DKV_WPE3: 1 holds the 128-key dK|dV kernel to three workgroups per CU
  int smallq_2percu = -1;  // CA_SMALLQ_2PERCU: grid size from which the single-query kernels run rings of two tiles;
                           // unset (-1) = 1.5 x CUs, 0 = never
  int split = CA_ATTN_SPLIT_MAX;  // CA_ATTN_SPLIT: most workgroups that share one (clip, head)'s keys; 1 = off
  int split_tail = 1;      // CA_ATTN_SPLIT_TAIL: 0 = split no partly filled second round
  int device_cus = 256;    // the device's CU count
};

// ---- thresholds ----------------------------------------------------------------------------------------------------
constexpr int ATTN_WIDE_MIN_ROWS = 100;    // 128-query (forward, dQ) / 128-key (dK|dV) workgroups when that side fills them
constexpr int ATTN_SMALLQ_MAX_TQ = 16;     // greedy decoding: the waves split the keys
constexpr int ATTN_SPLIT_MIN_KEYS = 1024;  // the key split needs this many keys to pay for its merge
constexpr int ATTN_HD_NARROW = 64;         // head_dim up to here runs the HDPV = 64 instantiations, beyond it the 128 ones
constexpr int ATTN_KEY_SLOT_MAX_KEYS = 4096;  // key_slot: the row's table of cache rows sits in LDS behind the V rings

// ---- the plan: everything a launch needs ---------------------------------------------------------------------------
enum AttnKernel {
  ATTN_NONE = 0,  // nothing to launch (the backward's prep pass beside the wide dQ kernel)
  ATTN_FWD = 1, ATTN_FWD_WIDE = 2, ATTN_FWD_SMALLQ = 3, ATTN_BWD_PREP = 4, ATTN_BWD_DKV = 5, ATTN_BWD_DKV_WIDE = 6,
  ATTN_BWD_DQ = 7, ATTN_BWD_DQ_WIDE = 8
};
enum AttnPlanError {
  ATTN_PLAN_OK = 0, ATTN_PLAN_KEY_SLOT = 1, ATTN_PLAN_O8 = 2, ATTN_PLAN_SPLIT_WS = 3, ATTN_PLAN_KEY_SLOT_BWD = 4,
  ATTN_PLAN_KSTART = 5
};
struct AttnPlan {
  int error = ATTN_PLAN_OK;
  int kernel = ATTN_NONE;
  // template arguments of the instantiation; 0 where the kernel has no such parameter
  int hdpv = 0;  // 64 / 128: head_dim rounded up to what the kernel's images hold
  int drop = 0;  // dropout on the probabilities
  int wpe = 0;   // wide kernels: workgroups per CU the register budget is held to (2 / 3)
  int dt = 0;    // single-query kernel: tiles in flight per wave (3 / 2)
  int qp = 0;    // ... with the query projection in front (ca_decode_attn_qproj)
  int ks = 0;    // ... with the key_slot table
  int km = 0;    // forward kernels: with a per-row first key (CaAttnDesc.kstart)
  unsigned grid = 0, block = 256;
  size_t lds = 0;  // dynamic LDS bytes
  // single-query kernel, key split: workgroups per (clip, head) at most, the split, byte offset of the partial slabs in
  // split_ws (behind the arrival counters); nsplit 1 = off
  int nsplit = 1;
  CaKeySplit split = {1, 0, 1};
  size_t slab_off = 0;
};
struct AttnBwdPlan {
  int error = ATTN_PLAN_OK;
  AttnPlan prep, dq, dkv;  // prep.kernel == ATTN_NONE: the wide dQ kernel produces D = rowsum(dO * O) itself
};
// one integer per instantiation: what the launchers switch over
// (km sits above the kernel id - hdpv << 8 reaches bit 15, the kernel ids bit 19 - so the numbers without it are the old ones)
constexpr int attn_inst(int kernel, int hdpv, int drop, int wpe = 0, int dt = 0, int qp = 0, int ks = 0, int km = 0) {
  return km << 24 | kernel << 16 | hdpv << 8 | drop << 7 | wpe << 5 | dt << 3 | qp << 1 | ks;
}
inline int attn_inst(const AttnPlan& p) { return attn_inst(p.kernel, p.hdpv, p.drop, p.wpe, p.dt, p.qp, p.ks, p.km); }

// cache rows by table: the single-query decode form only (attn_fwd_smallq_kernel<.., KS>)
inline bool attn_key_slot_ok(const CaAttnDesc& d) {
  return d.key_slot == nullptr ||
         (d.Tq == 1 && d.klen != nullptr && d.hd <= ATTN_HD_NARROW && !d.causal && d.dropout_p == 0.f && d.O8 == nullptr &&
          d.split_ws == nullptr && d.row_off == nullptr && d.Tk <= ATTN_KEY_SLOT_MAX_KEYS);
}
// a per-row first key: the causal tiled forward and the single-query decode form, head_dim <= 64, the plain output only
inline bool attn_kstart_ok(const CaAttnDesc& d) {
  if (d.kstart == nullptr) return true;
  if (d.hd > ATTN_HD_NARROW || d.dropout_p != 0.f || d.O8 || d.row_off || d.split_ws || d.key_slot) return false;
  return d.causal || (d.Tq == 1 && d.klen != nullptr);
}
inline int attn_hdpv(const CaAttnDesc& d) { return d.hd <= ATTN_HD_NARROW ? 64 : 128; }
inline unsigned attn_grid_of(const CaAttnDesc& d, int rows, int rows_per_tile) {
  return attn_grid((rows + rows_per_tile - 1) / rows_per_tile, d.H, d.B);
}

// The kernels that own queries (forward, dQ): 64 queries per workgroup and one image pair, or 128 and a ring of two
inline void attn_plan_query_side(AttnPlan& p, const CaAttnDesc& d, bool wide, int narrow_kernel, int wide_kernel, int wpe3) {
  p.kernel = wide ? wide_kernel : narrow_kernel;
  p.hdpv = attn_hdpv(d);
  p.drop = d.dropout_p > 0.f ? 1 : 0;
  if (wide) p.wpe = wpe3 && d.hd <= ATTN_HD_NARROW && !p.drop ? 3 : 2;
  p.grid = attn_grid_of(d, d.Tq, wide ? 128 : 64);
  p.lds = (size_t)(wide ? 2 : 1) * 2 * 64 * p.hdpv * 2;
}

// dynamic LDS of the single-query kernel: four waves x a ring of dt 8-KiB V images (three: one workgroup per CU; two: two
// workgroups per CU, large batches), + the normalised row and the partial products of the query projection, + the
// key_slot table
inline size_t attn_smallq_lds(int dt, int qp, int table_bytes) {
  return (size_t)4 * dt * 64 * 64 * 2 + (qp ? 4096 + 1024 : 0) + (size_t)table_bytes;
}
// The single-query kernel (ca_attn_fwd at Tq <= 16 and ca_decode_attn_qproj).
// Key split: on when the caller lent a workspace, the keys are many and (clips x heads) leaves at least half of the CUs
// without a workgroup.  Rings of two tiles (two workgroups per CU) from grids of more than 1.5 workgroups per CU.
inline AttnPlan attn_plan_smallq(const CaAttnDesc& d, const AttnKnobs& k, int qp) {
  AttnPlan p;
  p.kernel = ATTN_FWD_SMALLQ;
  p.hdpv = 64;
  p.qp = qp;
  p.ks = d.key_slot ? 1 : 0;
  p.km = d.kstart ? 1 : 0;
  const int bh = d.B * d.H;
  p.grid = (unsigned)bh;
  if (d.split_ws && d.Tk >= ATTN_SPLIT_MIN_KEYS) {
    const CaKeySplit sp = ca_attn_key_split(bh, k.device_cus, k.split, k.split_tail);
    if (sp.ns >= 2 || sp.ns_tail >= 2) {
      if (d.split_ws_bytes < CA_ATTN_SPLIT_WS_BYTES(d.B, d.H) || ((uintptr_t)d.split_ws % 16) != 0) {
        p.error = ATTN_PLAN_SPLIT_WS;
        return p;
      }
      p.nsplit = sp.ns > sp.ns_tail ? sp.ns : sp.ns_tail;
      p.split = sp;
      p.slab_off = ((size_t)bh * 4 + 255) / 256 * 256;
      p.grid = (unsigned)ca_key_split_parts(sp, bh);
    }
  }
  const unsigned two_per_cu = k.smallq_2percu < 0    ? (unsigned)(k.device_cus + k.device_cus / 2)
                              : k.smallq_2percu == 0 ? 0x7fffffffu
                                                     : (unsigned)k.smallq_2percu;
  p.dt = p.grid >= two_per_cu ? 2 : 3;
  p.lds = attn_smallq_lds(p.dt, qp, p.ks ? (d.Tk * 4 + 15) / 16 * 16 : 0);
  return p;
}

inline AttnPlan attn_plan_fwd(const CaAttnDesc& d, const AttnKnobs& k) {
  AttnPlan p;
  // 128-query workgroups when the query side fills them; CA_ATTN_WIDE=0 keeps the 64-query kernel
  const bool wide = k.wide && d.Tq >= ATTN_WIDE_MIN_ROWS;
  if (!attn_key_slot_ok(d)) p.error = ATTN_PLAN_KEY_SLOT;
  else if (!attn_kstart_ok(d)) p.error = ATTN_PLAN_KSTART;
  else if (d.O8 && !(d.o8_scale && wide && (d.ldo % 8) == 0 && ((uintptr_t)d.O8 % 8) == 0)) p.error = ATTN_PLAN_O8;
  if (p.error) return p;
  const bool drop = d.dropout_p > 0.f;
  // training with dropout on the attention probabilities: the general kernels only
  if (!wide && !drop && d.Tq <= ATTN_SMALLQ_MAX_TQ && d.hd <= ATTN_HD_NARROW && !d.causal && !d.row_off)
    return attn_plan_smallq(d, k, 0);
  // head_dim <= 64 without dropout: three workgroups per CU (see the kernel's header)
  attn_plan_query_side(p, d, wide, ATTN_FWD, ATTN_FWD_WIDE, k.wpe3);
  p.km = d.kstart ? 1 : 0;
  return p;
}

// Greedy decoding: LayerNorm + query projection + single-query attention over a K|V cache in one launch per layer
// (ca_decode_attn_qproj checks the descriptor itself: one query per clip, head_dim <= 64, no mask, no dropout).
inline AttnPlan attn_plan_qproj(const CaAttnDesc& d, const AttnKnobs& k) {
  if (d.kstart) {  // the masked decoder self-attention takes its query from the projection GEMM
    AttnPlan p;
    p.error = ATTN_PLAN_KSTART;
    return p;
  }
  return attn_plan_smallq(d, k, 1);
}

inline AttnBwdPlan attn_plan_bwd(const CaAttnDesc& d, const AttnKnobs& k) {
  AttnBwdPlan bp;
  if (!attn_key_slot_ok(d)) bp.error = ATTN_PLAN_KEY_SLOT;
  else if (d.key_slot) bp.error = ATTN_PLAN_KEY_SLOT_BWD;
  else if (d.kstart) bp.error = ATTN_PLAN_KSTART;
  if (bp.error) return bp;
  const int hdpv = attn_hdpv(d), drop = d.dropout_p > 0.f ? 1 : 0;
  const bool narrow = d.hd <= ATTN_HD_NARROW;
  // dQ.  128-query workgroups when the query side fills them: that kernel also produces D = rowsum(dO * O) for the
  // dK/dV kernel behind it.  Otherwise D comes from its own pass first.
  const bool dq_wide = k.wide && d.Tq >= ATTN_WIDE_MIN_ROWS;
  if (!dq_wide) {
    const int64_t groups = (int64_t)d.B * d.H * d.Tq;
    bp.prep.kernel = ATTN_BWD_PREP;
    bp.prep.grid = (unsigned)((groups * 16 + 255) / 256);
  }
  attn_plan_query_side(bp.dq, d, dq_wide, ATTN_BWD_DQ, ATTN_BWD_DQ_WIDE, k.dq_wpe3);
  // dK, dV: 64 keys per workgroup (a 128-key, 8-wave variant with a 4-deep ring measured no faster at T = 499 and 5 %
  // slower at T = 1500: dropped)
  // ... and a wave that owns two key blocks (128 keys per workgroup) halves the LDS fragment reads per MFMA: see
  // attn_bwd_dkv_wide_kernel.  CA_ATTN_DKV_WIDE=0 keeps the 64-key kernel.
  // Measured (tools/archive/exp_dkv.sh, rocprofv3 per-kernel averages): head_dim <= 64 (XLS-R-300M, Whisper) 226 -> 208 us over
  // the models' shapes (XLS-R-300M backward 72.5 -> 63.1 us per layer, whisper-large-turbo encoder 523 -> 494); at
  // head_dim 80 / 120 the doubled accumulators (374 registers) leave one wave per SIMD and it LOSES (73.3 -> 83.7 us):
  // the 64-key kernel stays there.
  AttnPlan& kv = bp.dkv;
  kv.hdpv = hdpv;
  kv.drop = drop;
  kv.lds = (size_t)4 * 32 * hdpv * 2;
  if (k.dkv_wide && d.Tk >= ATTN_WIDE_MIN_ROWS && narrow) {
    kv.kernel = ATTN_BWD_DKV_WIDE;
    kv.wpe = k.dkv_wpe3 && !drop ? 3 : 2;
    kv.grid = attn_grid_of(d, d.Tk, 128);
  } else {
    kv.kernel = ATTN_BWD_DKV;
    kv.grid = attn_grid_of(d, d.Tk, 64);
  }
  return bp;
}
