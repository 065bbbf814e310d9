// Fused attention, C ABI: check the descriptor, plan (attn_plan.h), launch (attn_fwd.hip, attn_decode.hip, attn_bwd.hip).
#include "attn_common.h"

static int attn_check(const CaAttnDesc* d, const char* who) {
  CA_CHECK_ARG(d && d->Q && d->K && d->V, "%s: null pointer", who);
  CA_CHECK_ARG(d->B > 0 && d->H > 0 && d->Tq > 0 && d->Tk > 0, "%s: bad shape", who);
  CA_CHECK_ARG(d->hd >= 8 && d->hd <= 128 && (d->hd % 8) == 0, "%s: head_dim must be a multiple of 8 in [8,128]", who);
  CA_CHECK_ARG((d->ldq % 8) == 0 && (d->ldk % 8) == 0 && (d->ldv % 8) == 0, "%s: strides must be multiples of 8", who);
  CA_CHECK_ARG(d->lse != nullptr && d->Tqp >= d->Tq && (d->Tqp % 32) == 0, "%s: lse needs Tqp %% 32 == 0 rows", who);
  CA_CHECK_ARG(d->dropout_p >= 0.f && d->dropout_p < 1.f, "%s: bad dropout_p", who);
  // packed rows: self-attention over utterances laid end to end, each with its own length as query and key count
  CA_CHECK_ARG(d->row_off == nullptr || (d->Tq == d->Tk && !d->causal && d->klen == nullptr && d->O8 == nullptr &&
                                         d->split_ws == nullptr),
               "%s: row_off needs Tq == Tk and no causal mask, klen, O8 or split_ws", who);
  return CA_OK;
}
// what a planner refused, in the caller's words
static int attn_plan_error(int error, const char* who) {
  CA_CHECK_ARG(error != ATTN_PLAN_KEY_SLOT,
               "%s: key_slot needs Tq == 1, klen, head_dim <= 64, Tk <= 4096 and no causal mask, dropout, O8, split_ws or "
               "row_off", who);
  CA_CHECK_ARG(error != ATTN_PLAN_O8,
               "%s: O8 needs a scale, >= 100 queries per head (the wide kernels) and 8-byte aligned rows", who);
  CA_CHECK_ARG(error != ATTN_PLAN_SPLIT_WS, "attention: split_ws needs CA_ATTN_SPLIT_WS_BYTES(B, H) bytes, 16-byte aligned");
  CA_CHECK_ARG(error != ATTN_PLAN_KEY_SLOT_BWD, "%s: key_slot is a forward (decode) option", who);
  CA_CHECK_ARG(error != ATTN_PLAN_KSTART,
               "%s: kstart needs ca_attn_fwd with a causal mask, or with Tq == 1 and klen; head_dim <= 64 and no dropout, "
               "O8, row_off, split_ws or key_slot", who);
  return CA_OK;
}
static AttnArgs to_args(const CaAttnDesc& d) {
  AttnArgs a;
  a.Q = (const unsigned short*)d.Q; a.K = (const unsigned short*)d.K; a.V = (const unsigned short*)d.V;
  a.ldq = d.ldq; a.ldk = d.ldk; a.ldv = d.ldv; a.sqb = d.sqb; a.skb = d.skb; a.svb = d.svb;
  a.O = (unsigned short*)d.O; a.ldo = d.ldo; a.sob = d.sob;
  a.O8 = (unsigned char*)d.O8; a.o8_scale = d.o8_scale; a.o8_amax = (unsigned int*)d.o8_amax;
  a.row_off = d.row_off; a.Tqd = d.Tq; a.Tkd = d.Tk;
  a.lse = d.lse; a.klen = d.klen; a.key_slot = d.key_slot; a.B = d.B; a.H = d.H; a.Tq = d.Tq; a.Tk = d.Tk; a.hd = d.hd; a.Tqp = d.Tqp;
  a.causal = d.causal; a.scale = d.scale;
  a.dO = (const unsigned short*)d.dO; a.lddo = d.lddo; a.sdob = d.sdob; a.Dq = d.Dq;
  a.dQ = (unsigned short*)d.dQ; a.dK = (unsigned short*)d.dK; a.dV = (unsigned short*)d.dV;
  a.lddq = d.lddq; a.lddk = d.lddk; a.lddv = d.lddv; a.sdqb = d.sdqb; a.sdkb = d.sdkb; a.sdvb = d.sdvb;
  a.drop_p = d.dropout_p; a.drop_seed = d.dropout_seed;
  a.qp_x = nullptr; a.qp_ldx = 0; a.qp_gamma = a.qp_beta = a.qp_bias = nullptr; a.qp_W = nullptr; a.qp_ldw = 0; a.qp_d = 0;
  a.qp_eps = 0.f;
  a.nsplit = 1; a.split_slab = nullptr; a.split_cnt = nullptr;
  a.kstart = d.kstart;
  return a;
}
// the single-query kernel's key split: arrival counters at the front of the caller's workspace, partial slabs behind
static void set_split(AttnArgs& a, const AttnPlan& p, void* split_ws) {
  if (p.nsplit <= 1) return;
  a.nsplit = p.nsplit;
  a.split = p.split;
  a.split_cnt = (unsigned int*)split_ws;
  a.split_slab = (float*)((char*)split_ws + p.slab_off);
}

extern "C" int ca_attn_fwd(const CaAttnDesc* desc, void* stream) {
  const char* who = "ca_attn_fwd";
  if (int rc = attn_check(desc, who)) return rc;
  const AttnPlan p = attn_plan_fwd(*desc, attn_knobs());
  if (p.error == ATTN_PLAN_KEY_SLOT) return attn_plan_error(p.error, who);
  CA_CHECK_ARG(desc->O != nullptr, "ca_attn_fwd: null output");
  if (int rc = attn_plan_error(p.error, who)) return rc;
  AttnArgs a = to_args(*desc);
  if (p.kernel != ATTN_FWD_SMALLQ) return attn_launch_fwd(p, a, (hipStream_t)stream, who);
  set_split(a, p, desc->split_ws);
  return attn_launch_decode(p, a, (hipStream_t)stream, who);
}

// Greedy decoding: LayerNorm + query projection + single-query attention over a K|V cache in one launch per layer.
extern "C" int ca_decode_attn_qproj(const CaAttnDesc* desc, const void* x, int64_t ldx, const float* ln_gamma,
                                    const float* ln_beta, float ln_eps, const void* Wq, int64_t ldw, const float* bq,
                                    int32_t d_model, void* stream) {
  CA_CHECK_ARG(desc && x && ln_gamma && ln_beta && Wq && bq, "ca_decode_attn_qproj: null pointer");
  CA_CHECK_ARG(desc->K && desc->V && desc->O && desc->B > 0 && desc->H > 0 && desc->Tk > 0 && !desc->row_off &&
                   !desc->key_slot,
               "ca_decode_attn_qproj: bad descriptor");
  CA_CHECK_ARG(desc->Tq == 1 && desc->hd <= 64 && (desc->hd % 8) == 0 && !desc->causal && desc->dropout_p == 0.f,
               "ca_decode_attn_qproj: one query per clip, head_dim <= 64, no mask, no dropout");
  CA_CHECK_ARG(d_model >= 64 && d_model <= 2048 && (d_model % 8) == 0 && (ldx % 8) == 0 && (ldw % 8) == 0 &&
                   ((uintptr_t)x % 16) == 0 && ((uintptr_t)Wq % 16) == 0 && ((uintptr_t)ln_gamma % 16) == 0 &&
                   ((uintptr_t)ln_beta % 16) == 0,
               "ca_decode_attn_qproj: d_model in [64, 2048], multiples of 8, 16-byte aligned operands");
  CA_CHECK_ARG((desc->ldk % 8) == 0 && (desc->ldv % 8) == 0, "ca_decode_attn_qproj: ldk / ldv must be multiples of 8");
  const AttnPlan p = attn_plan_qproj(*desc, attn_knobs());
  if (int rc = attn_plan_error(p.error, "ca_decode_attn_qproj")) return rc;
  AttnArgs a = to_args(*desc);
  a.qp_x = (const unsigned short*)x; a.qp_ldx = ldx; a.qp_gamma = ln_gamma; a.qp_beta = ln_beta; a.qp_eps = ln_eps;
  a.qp_W = (const unsigned short*)Wq; a.qp_ldw = ldw; a.qp_bias = bq; a.qp_d = d_model;
  set_split(a, p, desc->split_ws);
  return attn_launch_decode(p, a, (hipStream_t)stream, "ca_decode_attn_qproj");
}

extern "C" int ca_attn_bwd(const CaAttnDesc* desc, void* stream) {
  const char* who = "ca_attn_bwd";
  if (int rc = attn_check(desc, who)) return rc;
  const AttnBwdPlan bp = attn_plan_bwd(*desc, attn_knobs());
  if (bp.error == ATTN_PLAN_KEY_SLOT) return attn_plan_error(bp.error, who);
  CA_CHECK_ARG(desc->dO && desc->O && desc->Dq && desc->dQ && desc->dK && desc->dV, "ca_attn_bwd: null pointer");
  CA_CHECK_ARG((desc->lddo % 8) == 0, "ca_attn_bwd: lddo must be a multiple of 8");
  if (int rc = attn_plan_error(bp.error, who)) return rc;
  const AttnArgs a = to_args(*desc);
  hipStream_t s = (hipStream_t)stream;
  if (bp.prep.kernel != ATTN_NONE)
    if (int rc = attn_launch_bwd(bp.prep, a, s, who)) return rc;
  if (int rc = attn_launch_bwd(bp.dq, a, s, who)) return rc;
  return attn_launch_bwd(bp.dkv, a, s, who);
}
