// GEMM family, host side: the C ABI (ca_gemm_bf16, ca_gemm_bf16_group, ca_gemm_fp8; see include/coral_amd.h), argument
// validation, the knobs of the kernel-choice rule (gemm_plan.h), the live profiler and the dispatch to the kernel files'
// launchers (gemm_common.h).  The kernels live in gemm_s.hip (S and M), gemm_l.hip, gemm_x.hip, gemm_skinny.hip and
// gemm_fp8.hip; this file names none of them.
#include "gemm_common.h"
#include <cstdlib>
#include <vector>

// ---- optional per-launch timing (bench.py's live roofline measurement) -----------------------
// When enabled, every ca_gemm_bf16 launch is bracketed by two hipEvents on the launch stream and
// its algorithmic FLOPs (2*M*N*K*batch) are recorded per template variant (index kernel*8 +
// segmented-K*4 + a_layout*2 + b_layout; kernel 0 = S, 1 = L, 2 = X).  ca_prof_end synchronises the events and returns the totals.
struct ProfRec {
  hipEvent_t e0, e1;
  double flops;
  int variant;
};
static bool g_prof_on = false;
static std::vector<ProfRec> g_prof;
hipEvent_t g_gemm_prof_e0 = nullptr, g_gemm_prof_e1 = nullptr;  // events of the launch being profiled (gemm_launch)

extern "C" int ca_prof_begin(void) {
  g_prof.clear();
  g_prof_on = true;
  return CA_OK;
}
extern "C" int ca_prof_end(double* ms, int64_t* count, double* flops) {
  g_prof_on = false;
  for (int v = 0; v < 24; ++v) {
    ms[v] = 0.0;
    count[v] = 0;
    flops[v] = 0.0;
  }
  for (auto& r : g_prof) {
    float t = 0.f;
    if (hipEventSynchronize(r.e1) != hipSuccess || hipEventElapsedTime(&t, r.e0, r.e1) != hipSuccess) {
      ca_set_error("ca_prof_end: event query failed");
      return CA_ERR_LAUNCH;
    }
    ms[r.variant] += t;
    count[r.variant] += 1;
    flops[r.variant] += r.flops;
    hipEventDestroy(r.e0);
    hipEventDestroy(r.e1);
  }
  g_prof.clear();
  return CA_OK;
}

// every kernel file that uses gemm_epilogue has its own copy of the switch (the skinny kernel does not read it)
extern "C" int ca_gemm_debug_general_epilogue(int on) {
  const int v = on ? 1 : 0;
  for (auto set : {gemm_set_epi_general_s, gemm_set_epi_general_l, gemm_set_epi_general_x, gemm_set_epi_general_fp8})
    if (set(v) != hipSuccess) {
      ca_set_error("ca_gemm_debug_general_epilogue: setting the switch failed");
      return CA_ERR_LAUNCH;
    }
  return CA_OK;
}
// CUs the compute kernels may count on (ca_gemm_set_compute_cus): 0 = all of them.  Set by the trainer of an N > 1 run,
// where a collective's kernel holds some CUs for most of the backward: persistent launches are sized to the rest and
// hand out every tile dynamically (CaGemmGroup.dyn_first), and the kernel-choice rule counts rounds on the rest.
static int g_compute_cus = 0;
extern "C" int ca_gemm_set_compute_cus(int n) {
  g_compute_cus = n > 0 ? n : 0;
  return CA_OK;
}
// see include/coral_amd.h: the forward kernel that holds the most registers is kernel X's K-major form
extern "C" int ca_background_update_fits(int32_t* regs) {
  hipFuncAttributes ax, aw;
  const hipError_t e1 = hipFuncGetAttributes(&ax, gemm_x_nt_kernel());
  const hipError_t e2 = hipFuncGetAttributes(&aw, ca_adamw_background_kernel());
  if (e1 != hipSuccess || e2 != hipSuccess) {
    ca_set_error("ca_background_update_fits: hipFuncGetAttributes: %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2));
    return CA_ERR_LAUNCH;
  }
  if (regs) {
    regs[0] = ax.numRegs;
    regs[1] = aw.numRegs;
  }
  const int gx = (ax.numRegs + 7) / 8 * 8, gw = (aw.numRegs + 7) / 8 * 8;
  return 2 * gx + gw <= 512 ? 1 : 0;
}
static unsigned x_device_cus() {
  static const unsigned ncu = [] {
    int dev = 0, n = 256;
    if (hipGetDevice(&dev) == hipSuccess) hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    return (unsigned)(n >= 8 ? (n / 8) * 8 : 8);
  }();
  return ncu;
}
static int g_force_kernel = 0;  // 0 auto, 1 force 128x128, 2 force 256x128, 3 force 256x256, 5 force kernel M (tests / tuning)
extern "C" int ca_gemm_force_kernel(int which) {
  g_force_kernel = which;
  return CA_OK;
}
// The tuning values of the kernel-choice rule (gemm_plan.h): the environment, read once, and the process's settings.
static GemmKnobs gemm_knobs() {
  static const GemmKnobs env = [] {
    GemmKnobs k;
    const auto read = [](const char* name, int& v) { if (const char* e = getenv(name)) v = atoi(e); };
    read("CA_X_PERSIST", k.x_persist);
    read("CA_SKINNY_MB1", k.skinny_mb1);
    read("CA_SKINNY_MB1_ROWS", k.skinny_mb1_rows);
    read("CA_SKINNY_NT", k.skinny_nt);
    read("CA_SKINNY_U", k.skinny_u);
    read("CA_GEMM_PREFER_L", k.prefer_l);
    read("CA_GEMM_L_OVER_X", k.l_over_x);
    read("CA_GEMM_L_MIN", k.l_min);
    read("CA_GEMM_M", k.m_max);
    return k;
  }();
  GemmKnobs k = env;
  k.force_kernel = g_force_kernel;
  k.compute_cus = g_compute_cus;
  k.device_cus = x_device_cus();
  return k;
}
static int ca_gemm_launch(const CaGemmDesc* desc, void* stream);
static int g_last_kind = 0;  // kernel chosen by the last launch: 0 = S, 1 = L, 2 = X

extern "C" int ca_gemm_bf16(const CaGemmDesc* desc, void* stream) {
  if (!g_prof_on || desc == nullptr) return ca_gemm_launch(desc, stream);
  ProfRec r;
  hipEventCreate(&r.e0);
  hipEventCreate(&r.e1);
  r.flops = 2.0 * desc->M * (double)desc->N * desc->K * desc->batch1 * desc->batch2;
  g_gemm_prof_e0 = r.e0;
  g_gemm_prof_e1 = r.e1;
  const int rc = ca_gemm_launch(desc, stream);
  g_gemm_prof_e0 = g_gemm_prof_e1 = nullptr;
  r.variant = g_last_kind * 8 + ((desc->a_kseg > 0 || desc->b_kseg > 0) ? 4 : 0) + (desc->a_layout ? 2 : 0) +
              (desc->b_layout ? 1 : 0);
  g_prof.push_back(r);
  return rc;
}

// ---- host dispatch: validate, plan (gemm_plan.h), launch -------------------------------------------------------------
// Hands the plan to its family's launcher.  grp: the problem list of a grouped launch (kernel X), else null.
static int gemm_launch_plan(const GemmPlan& p, const CaGemmDesc& d, CaGemmGroup* grp, hipStream_t s, const char* who) {
  if (p.fp8) return gemm_launch_fp8(p, d, s, who);
  switch (p.family) {
    case GEMM_SKINNY: return gemm_launch_skinny(p, d, s, who);
    case GEMM_X: {
      CaGemmGroup one;  // a plain launch is a group of one: problem 0, no tile list
      if (!grp) one.d[0] = d, one.count = 0, one.first[0] = 0, one.total = 0;
      return gemm_launch_x(p, grp ? *grp : one, s, who);
    }
    case GEMM_L: return gemm_launch_l(p, d, s, who);
    default: return gemm_launch_s(p, d, s, who);  // GEMM_S, GEMM_M
  }
}

static int gemm_validate_fp8(const CaGemmDesc& d) {
  CA_CHECK_ARG(d.A && d.B && (d.C || d.C2) && d.M > 0 && d.N > 0 && d.K > 0, "ca_gemm_fp8: bad argument");
  CA_CHECK_ARG(d.C8 == nullptr || ((d.epilogue == CA_EPI_GELU || d.epilogue == CA_EPI_DGELU) && d.c8_scale != nullptr && (d.ldc % 8) == 0 &&
                                   ((uintptr_t)d.C8 % 8) == 0),
               "ca_gemm_fp8: C8 needs CA_EPI_GELU / CA_EPI_DGELU, a scale and 8-byte aligned rows");
  CA_CHECK_ARG(d.a_layout == CA_KMAJOR && d.b_layout == CA_KMAJOR && d.batch1 == 1 && d.batch2 == 1 && d.a_kseg == 0 &&
                   d.b_kseg == 0 && !d.a_colsum && !d.c_row_index,
               "ca_gemm_fp8: K-major operands, un-batched, plain rows only");
  CA_CHECK_ARG((d.K % 16) == 0 && (d.lda % 16) == 0 && (d.ldb % 16) == 0 && ((uintptr_t)d.A % 16) == 0 &&
                   ((uintptr_t)d.B % 16) == 0,
               "ca_gemm_fp8: K, lda, ldb must be multiples of 16 bytes and the operands 16-byte aligned");
  return CA_OK;
}
extern "C" int ca_gemm_fp8(const CaGemmDesc* desc, void* stream) {
  CA_CHECK_ARG(desc != nullptr, "ca_gemm_fp8: null descriptor");
  const int rc = gemm_validate_fp8(*desc);
  if (rc != CA_OK) return rc;
  return gemm_launch_plan(gemm_plan_fp8(*desc, gemm_knobs()), *desc, nullptr, (hipStream_t)stream, "ca_gemm_fp8");
}

// Up to eight independent GEMMs of the same operand form in one launch of kernel X (grouped launch): used where
// the problems do not fill the chip one by one (the four weight gradients of a transformer layer: 240 + 240 +
// 184 + 64 tiles on 256 CUs at XLS-R-2B, 64 + 64 + 48 + 16 at d = 1024).  All must be un-batched, un-segmented
// and plain (no epilogue, no bias).
static int gemm_validate_group(const CaGemmDesc* descs, int32_t count) {
  CA_CHECK_ARG(descs && count >= 1 && count <= X_GROUP_MAX, "ca_gemm_bf16_group: 1..8 problems");
  for (int i = 0; i < count; ++i) {
    const CaGemmDesc* p = descs + i;
    CA_CHECK_ARG(p->A && p->B && p->C && p->M > 0 && p->N > 0 && p->K >= 64, "ca_gemm_bf16_group: bad problem %d", i);
    CA_CHECK_ARG(p->batch1 == 1 && p->batch2 == 1 && p->a_kseg == 0 && p->b_kseg == 0 && p->epilogue == CA_EPI_NONE &&
                     p->bias == nullptr && p->dropout_p == 0.f,
                 "ca_gemm_bf16_group: only plain un-batched problems");
    CA_CHECK_ARG((p->lda % 8) == 0 && (p->ldb % 8) == 0 && ((uintptr_t)p->A % 16) == 0 && ((uintptr_t)p->B % 16) == 0,
                 "ca_gemm_bf16_group: alignment");
    CA_CHECK_ARG(p->a_layout == descs->a_layout && p->b_layout == descs->b_layout,
                 "ca_gemm_bf16_group: the problems differ in operand form");
    CA_CHECK_ARG(p->c_sumsq == nullptr || p->epilogue == CA_EPI_NONE, "ca_gemm_bf16_group: c_sumsq needs a plain epilogue");
  }
  return CA_OK;
}
extern "C" int ca_gemm_bf16_group(const CaGemmDesc* descs, int32_t count, void* stream) {
  const int rc = gemm_validate_group(descs, count);
  if (rc != CA_OK) return rc;
  CaGemmGroup g;
  int total = 0;
  for (int i = 0; i < X_GROUP_MAX; ++i) {  // (the unused slots repeat problem 0 and own no tiles)
    g.d[i] = descs[i < count ? i : 0];
    g.first[i] = total;
    if (i < count) total += gemm_x_tiles(descs[i]);
  }
  g.total = total;
  g.count = count > 1 ? count : 0;
  const GemmPlan p = gemm_plan_group(descs, count, gemm_knobs());
  ProfRec r;
  if (g_prof_on) {  // live roofline timing (bench.py): the group counts as one launch of kernel X
    hipEventCreate(&r.e0);
    hipEventCreate(&r.e1);
    r.flops = 0.0;
    for (int i = 0; i < count; ++i) r.flops += 2.0 * descs[i].M * (double)descs[i].N * descs[i].K;
    r.variant = p.kind * 8 + p.lay;
    g_gemm_prof_e0 = r.e0;
    g_gemm_prof_e1 = r.e1;
  }
  const int lrc = gemm_launch_plan(p, descs[0], &g, (hipStream_t)stream, "ca_gemm_bf16_group");
  if (g_prof_on) {
    g_gemm_prof_e0 = g_gemm_prof_e1 = nullptr;
    g_prof.push_back(r);
  }
  return lrc;
}

static int gemm_validate_bf16(const CaGemmDesc& d) {
  CA_CHECK_ARG(d.A && d.B &&
                   (d.C || ((d.epilogue == CA_EPI_GELU || d.epilogue == CA_EPI_GELU_RESIDUAL) && d.C2)),
               "ca_gemm_bf16: null operand");
  CA_CHECK_ARG(d.M > 0 && d.N > 0 && d.K > 0, "ca_gemm_bf16: bad shape %d %d %d", d.M, d.N,
               d.K);
  CA_CHECK_ARG(d.batch1 > 0 && d.batch2 > 0, "ca_gemm_bf16: bad batch");
  CA_CHECK_ARG((d.lda % 8) == 0 && (d.ldb % 8) == 0, "ca_gemm_bf16: lda/ldb must be multiples of 8");
  CA_CHECK_ARG((d.sA1 % 8) == 0 && (d.sA2 % 8) == 0 && (d.sB1 % 8) == 0 && (d.sB2 % 8) == 0,
               "ca_gemm_bf16: batch strides must be multiples of 8");
  CA_CHECK_ARG(((uintptr_t)d.A % 16) == 0 && ((uintptr_t)d.B % 16) == 0,
               "ca_gemm_bf16: A/B must be 16-byte aligned");
  CA_CHECK_ARG(d.a_kseg >= 0 && d.b_kseg >= 0, "ca_gemm_bf16: negative kseg");
  if (d.epilogue == CA_EPI_RESIDUAL || d.epilogue == CA_EPI_DGELU || d.epilogue == CA_EPI_GELU_RESIDUAL)
    CA_CHECK_ARG(d.R != nullptr, "ca_gemm_bf16: epilogue needs R");
  CA_CHECK_ARG(d.dropout_p >= 0.f && d.dropout_p < 1.f, "ca_gemm_bf16: bad dropout_p");
  CA_CHECK_ARG(d.C8 == nullptr || ((d.epilogue == CA_EPI_GELU || d.epilogue == CA_EPI_DGELU) && d.c8_scale != nullptr && d.batch1 == 1 && d.batch2 == 1 &&
                                   (d.ldc % 8) == 0 && ((uintptr_t)d.C8 % 8) == 0 && d.M > 32),
               "ca_gemm_bf16: C8 needs CA_EPI_GELU / CA_EPI_DGELU, a scale, an un-batched problem and 8-byte aligned rows");
  if (d.a_colsum)
    CA_CHECK_ARG(d.a_layout == CA_MNMAJOR && d.b_layout == CA_MNMAJOR && d.batch1 == 1 && d.batch2 == 1 && d.a_kseg == 0,
                 "ca_gemm_bf16: a_colsum needs the un-batched weight-gradient form");
  if (d.c_sumsq)
    CA_CHECK_ARG(d.epilogue == CA_EPI_NONE && d.batch1 == 1 && d.batch2 == 1 && d.c_row_index == nullptr && d.c_split_n == 0,
                 "ca_gemm_bf16: c_sumsq needs an un-batched output with the plain epilogue");
  CA_CHECK_ARG(d.a_layout == CA_KMAJOR || d.a_layout == CA_MNMAJOR, "ca_gemm_bf16: bad a_layout");
  CA_CHECK_ARG(d.b_layout == CA_KMAJOR || d.b_layout == CA_MNMAJOR, "ca_gemm_bf16: bad b_layout");
  return CA_OK;
}
// what the skinny form asks of the features only it has
static int gemm_validate_skinny(const CaGemmDesc& d) {
  CA_CHECK_ARG(d.c_split_n == 0 || (d.C_hi && (d.c_split_n % 16) == 0 && d.c_split_n < d.N && d.epilogue == CA_EPI_NONE),
               "ca_gemm_bf16: c_split_n needs C_hi, a multiple of 16 below N and no epilogue");
  if (d.a_ln_gamma)
    CA_CHECK_ARG(d.a_ln_beta && d.K <= 2048 && ((uintptr_t)d.a_ln_gamma % 16) == 0 && ((uintptr_t)d.a_ln_beta % 16) == 0,
                 "ca_gemm_bf16: a_ln_gamma needs a_ln_beta, K <= 2048 and 16-byte aligned vectors");
  return CA_OK;
}

static int ca_gemm_launch(const CaGemmDesc* desc, void* stream) {
  CA_CHECK_ARG(desc != nullptr, "ca_gemm_bf16: null descriptor");
  const GemmKnobs knobs = gemm_knobs();
  // (a copy: the library, not the caller, owns xcd_balanced - every XCD gets the same number of tiles whenever the
  // host said that the chip is shared with a resident kernel, ca_gemm_set_compute_cus)
  CaGemmDesc d = *desc;
  d.xcd_balanced = knobs.compute_cus > 0 ? 1 : 0;
  int rc = gemm_validate_bf16(d);
  if (rc != CA_OK) return rc;
  const GemmPlan p = gemm_plan_bf16(d, knobs);
  CA_CHECK_ARG(p.error != GEMM_PLAN_LN_NOT_SKINNY,
               "ca_gemm_bf16: a_ln_gamma exists in the skinny form only (M <= 128, K-major operands, un-batched)");
  CA_CHECK_ARG(p.error != GEMM_PLAN_ROWS_NOT_SKINNY,
               "ca_gemm_bf16: c_row_index / c_split_n exist in the skinny form only (M <= 128, K-major operands, un-batched)");
  g_last_kind = p.kind;
  if (p.family == GEMM_SKINNY && (rc = gemm_validate_skinny(d)) != CA_OK) return rc;
  return gemm_launch_plan(p, d, nullptr, (hipStream_t)stream, "ca_gemm_bf16");
}
