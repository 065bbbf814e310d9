// Host-only check of the kstart rules of coral_amd/csrc/attn_plan.h (tests/test_attn_kstart_plan_cpu.py builds and runs it).
//   1. kstart == NULL: a sample of descriptors gets, field by field, the plan it gets with the field never looked at
//      (the instantiation number below bit 24 is the old number: km = 0 adds nothing).
//   2. kstart set: the causal 64-query, the causal 128-query and the single-query form get the km instantiations, with the
//      grid, block and LDS size of their unmasked twins.
//   3. every refused combination returns ATTN_PLAN_KSTART.
#include <stdio.h>
#include <string.h>
#include <initializer_list>
#include "../coral_amd/csrc/attn_plan.h"

static int bad = 0;
#define EXPECT(c)                                                  \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #c); \
      bad = 1;                                                     \
    }                                                              \
  } while (0)

alignas(256) static char dummy[4096];

static CaAttnDesc desc(int B, int H, int Tq, int Tk, int hd, int causal, bool klen) {
  CaAttnDesc d;
  memset(&d, 0, sizeof d);
  d.B = B; d.H = H; d.Tq = Tq; d.Tk = Tk; d.hd = hd; d.causal = causal;
  d.Tqp = (Tq + 31) / 32 * 32;
  d.klen = klen ? (const int32_t*)dummy : nullptr;
  d.ldo = (int64_t)H * hd;
  return d;
}
static bool same(const AttnPlan& a, const AttnPlan& b) {
  return a.error == b.error && a.kernel == b.kernel && a.hdpv == b.hdpv && a.drop == b.drop && a.wpe == b.wpe && a.dt == b.dt &&
         a.qp == b.qp && a.ks == b.ks && a.grid == b.grid && a.block == b.block && a.lds == b.lds && a.nsplit == b.nsplit;
}

int main() {
  const AttnKnobs k;
  const int32_t* ks = (const int32_t*)dummy;
  // 1. NULL = today's plan: km 0, and the instantiation number is the seven-argument one
  int n = 0;
  for (int hd : {32, 64, 80, 128})
    for (int Tq : {1, 5, 16, 17, 70, 99, 100, 130, 499})
      for (int causal : {0, 1})
        for (int kl : {0, 1}) {
          const CaAttnDesc d = desc(4, 2, Tq, Tq == 1 ? 200 : Tq, hd, causal, kl);
          const AttnPlan p = attn_plan_fwd(d, k);
          EXPECT(p.error == ATTN_PLAN_OK && p.km == 0);
          EXPECT(attn_inst(p) == attn_inst(p.kernel, p.hdpv, p.drop, p.wpe, p.dt, p.qp, p.ks));
          EXPECT(attn_inst(p) < (1 << 24));
          const AttnBwdPlan bp = attn_plan_bwd(d, k);
          EXPECT(bp.error == ATTN_PLAN_OK && bp.dq.km == 0 && bp.dkv.km == 0 && bp.prep.km == 0);
          ++n;
        }
  {
    const CaAttnDesc d = desc(16, 16, 1, 1500, 64, 0, true);
    EXPECT(attn_plan_qproj(d, k).error == ATTN_PLAN_OK && attn_plan_qproj(d, k).km == 0);
  }
  // 2. the three supported forms
  struct Form { int Tq, Tk, causal, kernel, wpe, dt; };
  for (const Form f : {Form{5, 5, 1, ATTN_FWD, 0, 0}, Form{70, 70, 1, ATTN_FWD, 0, 0}, Form{99, 99, 1, ATTN_FWD, 0, 0},
                       Form{100, 100, 1, ATTN_FWD_WIDE, 3, 0}, Form{130, 130, 1, ATTN_FWD_WIDE, 3, 0},
                       Form{228, 228, 1, ATTN_FWD_WIDE, 3, 0}, Form{1, 200, 0, ATTN_FWD_SMALLQ, 0, 3},
                       Form{1, 448, 0, ATTN_FWD_SMALLQ, 0, 3}})
    for (int hd : {32, 64}) {
      CaAttnDesc d = desc(6, 2, f.Tq, f.Tk, hd, f.causal, true);
      const AttnPlan p0 = attn_plan_fwd(d, k);
      d.kstart = ks;
      const AttnPlan p = attn_plan_fwd(d, k);
      EXPECT(p.error == ATTN_PLAN_OK && p.km == 1 && p.kernel == f.kernel && p.hdpv == 64 && p.wpe == f.wpe && p.dt == f.dt);
      EXPECT(same(p, p0));  // the unmasked twin's launch geometry
      EXPECT(attn_inst(p) == ((1 << 24) | attn_inst(p0)));
      EXPECT(attn_inst(p) == attn_inst(f.kernel, 64, 0, f.wpe, f.dt, 0, 0, 1));
    }
  {  // (two workgroups per CU: the ring of two, also masked)
    CaAttnDesc d = desc(64, 16, 1, 448, 64, 0, true);
    d.kstart = ks;
    const AttnPlan p = attn_plan_fwd(d, k);
    EXPECT(p.error == ATTN_PLAN_OK && p.km == 1 && p.kernel == ATTN_FWD_SMALLQ && p.dt == 2);
    AttnKnobs k2;
    k2.wpe3 = 0;
    CaAttnDesc w = desc(2, 2, 130, 130, 64, 1, false);
    w.kstart = ks;
    const AttnPlan pw = attn_plan_fwd(w, k2);
    EXPECT(pw.error == ATTN_PLAN_OK && pw.km == 1 && pw.kernel == ATTN_FWD_WIDE && pw.wpe == 2);
  }
  // 3. the refused combinations
  auto refused_fwd = [&](CaAttnDesc d) {
    d.kstart = ks;
    return attn_plan_fwd(d, k).error == ATTN_PLAN_KSTART;
  };
  const CaAttnDesc causal = desc(4, 2, 130, 130, 64, 1, true), one = desc(4, 2, 1, 200, 64, 0, true);
  EXPECT(!refused_fwd(causal) && !refused_fwd(one));
  EXPECT(refused_fwd(desc(4, 2, 130, 130, 72, 1, true)));   // head_dim > 64
  EXPECT(refused_fwd(desc(4, 2, 130, 130, 128, 1, true)));
  EXPECT(refused_fwd(desc(4, 2, 1, 200, 128, 0, true)));
  EXPECT(refused_fwd(desc(4, 2, 130, 130, 64, 0, true)));   // neither causal nor the single-query form
  EXPECT(refused_fwd(desc(4, 2, 5, 200, 64, 0, true)));
  EXPECT(refused_fwd(desc(4, 2, 1, 200, 64, 0, false)));    // single query without klen
  for (const CaAttnDesc& base : {causal, one}) {
    CaAttnDesc d = base;
    d.dropout_p = 0.1f;
    EXPECT(refused_fwd(d));
    d = base;
    d.O8 = dummy; d.o8_scale = (const float*)dummy;
    EXPECT(refused_fwd(d));
    d = base;
    d.row_off = (const int32_t*)dummy;
    EXPECT(refused_fwd(d));
    d = base;
    d.split_ws = dummy; d.split_ws_bytes = CA_ATTN_SPLIT_WS_BYTES(d.B, d.H);
    EXPECT(refused_fwd(d));
  }
  {
    CaAttnDesc d = one;  // key_slot alone is fine here; together with kstart it is refused
    d.key_slot = (const int32_t*)dummy;
    EXPECT(attn_plan_fwd(d, k).error == ATTN_PLAN_OK && attn_plan_fwd(d, k).ks == 1);
    EXPECT(refused_fwd(d));
    d = causal;
    d.kstart = ks;
    EXPECT(attn_plan_bwd(d, k).error == ATTN_PLAN_KSTART);
    d = one;
    d.kstart = ks;
    EXPECT(attn_plan_bwd(d, k).error == ATTN_PLAN_KSTART);
    EXPECT(attn_plan_qproj(d, k).error == ATTN_PLAN_KSTART);
  }
  printf("%d unmasked descriptors unchanged; kstart forms and refusals %s\n", n, bad ? "DIFFER" : "ok");
  return bad;
}
