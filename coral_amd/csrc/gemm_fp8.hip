// fp8 (OCP e4m3) forward GEMM: C = epilogue(alpha * sa * sb * A B^T), A [M][K], B [N][K] one byte per element.
// See include/coral_amd.h (ca_gemm_fp8).
// BASELINE configs[4] ("fp8 weights, CDNA4 fp8 MFMA").  v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales
// (the per-tensor scales sa, sb are device scalars folded into alpha): 4x the K of the bf16 MFMA at twice its cycles.
// A 128-byte row of the LDS image now holds 128 k, so the tile images, the loaders and the XOR swizzle are the bf16
// kernel's byte for byte; a lane's operand is the 32 consecutive bytes (two 16-B chunks) of its row and lane group,
// for A and B alike - the dot product does not care which k a lane group owns as long as both sides agree.
#include "gemm_common.h"

GEMM_EPILOGUE_KEEP_VISIBLE;  // (no kernel here passes a bias to the epilogue: see gemm_common.h)

// Kernel S structure: 128 x 128 x 128 tile, 4 waves (64 x 64 each), 2 workgroups per CU.
typedef __attribute__((ext_vector_type(8))) int fp8x32_t;
typedef __attribute__((ext_vector_type(4))) int i32x4_t;
__global__ __launch_bounds__(256) void ca_gemm_fp8_kernel(const CaGemmDesc d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  int tm, tn;
  if (!tile_of_block<8, 8>(blockIdx.x, (d.M + BM - 1) / BM, (d.N + BN - 1) / BN, tm, tn)) return;
  const int m0 = tm * BM, n0 = tn * BN;
  KMajorStream<4> la, lb;
  la.init_bytes((const char*)d.A, d.lda, m0, d.M, wave, lane);
  lb.init_bytes((const char*)d.B, d.ldb, n0, d.N, wave, lane);
  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  const int K = d.K;
  constexpr int FBK = 128;  // k per K-step
  const int nk = (K + FBK - 1) / FBK;
  auto burst = [&](int kt) {
    if (kt >= nk) return;
    char* na = smem + (kt & 1) * TILE_BYTES;
    char* nb = na + 2 * TILE_BYTES;
    const bool full = (kt + 1) * FBK <= K;
    if (full) {
#pragma unroll
      for (int part = 0; part < 4; ++part) {
        la.issue_one(na, wave, part);
        lb.issue_one(nb, wave, part);
      }
    } else {
#pragma unroll
      for (int part = 0; part < 4; ++part) {
        la.issue_one_tail(na, wave, K - kt * FBK, part);
        lb.issue_one_tail(nb, wave, K - kt * FBK, part);
      }
    }
    la.advance();
    lb.advance();
  };
  auto zero_tail = [&](int kt) {
    if (kt != nk - 1 || nk * FBK == K) return;
    char* na = smem + (kt & 1) * TILE_BYTES;
    la.zero_fix(na, wave, lane, K - kt * FBK);
    lb.zero_fix(na + 2 * TILE_BYTES, wave, lane, K - kt * FBK);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  };
  const uint32_t lds0 = (uint32_t)(uintptr_t)(lptr_t)smem;
  const int g = lane >> 4;
  uint32_t abase[2], bbase[2];  // the two 16-B chunks of this lane's 32-byte operand
  {
    const int ra = wm * 64 + (lane & 15), rb = wn * 64 + (lane & 15);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      abase[h] = lds0 + ra * 128 + (((2 * g + h) ^ ((ra >> 1) & 7)) * 16);
      bbase[h] = lds0 + 2 * TILE_BYTES + rb * 128 + (((2 * g + h) ^ ((rb >> 1) & 7)) * 16);
    }
  }
  burst(0);
  auto kstep = [&](auto st_c, int kt) {
    constexpr int ST = decltype(st_c)::value;
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // tile kt landed; my reads of kt-1 done
    zero_tail(kt);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    burst(kt + 1);
    bf16x8_t al[4], ah[4], bl[4], bh[4];
#define F8_RD(dst, base, F) dst = lds_read_b128<ST * TILE_BYTES + (F) * 2048>(base)
    F8_RD(al[0], abase[0], 0); F8_RD(ah[0], abase[1], 0); F8_RD(al[1], abase[0], 1); F8_RD(ah[1], abase[1], 1);
    F8_RD(al[2], abase[0], 2); F8_RD(ah[2], abase[1], 2); F8_RD(al[3], abase[0], 3); F8_RD(ah[3], abase[1], 3);
    F8_RD(bl[0], bbase[0], 0); F8_RD(bh[0], bbase[1], 0); F8_RD(bl[1], bbase[0], 1); F8_RD(bh[1], bbase[1], 1);
    F8_RD(bl[2], bbase[0], 2); F8_RD(bh[2], bbase[1], 2); F8_RD(bl[3], bbase[0], 3); F8_RD(bh[3], bbase[1], 3);
#undef F8_RD
    lds_wait(al);
    lds_wait(ah);
    lds_wait(bl);
    lds_wait(bh);
    fp8x32_t af[4], bq[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const i32x4_t a0 = __builtin_bit_cast(i32x4_t, al[i]), a1 = __builtin_bit_cast(i32x4_t, ah[i]);
      const i32x4_t b0 = __builtin_bit_cast(i32x4_t, bl[i]), b1 = __builtin_bit_cast(i32x4_t, bh[i]);
      af[i] = (fp8x32_t){a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
      bq[i] = (fp8x32_t){b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(bq[j], af[i], acc[i][j], 0, 0, 0, 0x7f7f7f7f, 0,
                                                                     0x7f7f7f7f);
  };
  for (int kt = 0; kt < nk; kt += 2) {
    kstep(std::integral_constant<int, 0>{}, kt);
    if (kt + 1 < nk) kstep(std::integral_constant<int, 1>{}, kt + 1);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  CaGemmDesc dd = d;
  dd.alpha = d.alpha * (d.a_scale ? *d.a_scale : 1.f) * (d.b_scale ? *d.b_scale : 1.f);
  if (d.a_row_scale) {  // one dequantisation factor per row of A (ca_layernorm_fwd_fp8): a lane's accumulators of
                        // fragment row i all belong to output row m0 + wm*64 + 16 i + (lane & 15)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + wm * 64 + i * 16 + (lane & 15);
      const float rs = d.a_row_scale[m < d.M ? m : d.M - 1];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] *= rs;
    }
  }
  gemm_epilogue(dd, acc, smem, wave, lane, m0 + wm * 64, n0 + wn * 64, 0, 0, 0);
}

// The same in kernel X's structure: 256 x 256 x 128 tile, 8 waves (2 x 4, 128 x 64 each), one workgroup per CU, LDS
// A0 | A1 | B0 | B1.  Two blocks of 16 MFMAs (K = 128 each) per K-step; block 0 (m-half 0) carries the reads of
// m-half 1, the barrier sits between the blocks, and block 1 runs column by column so that each B fragment can be
// re-loaded for the next tile as soon as its four MFMAs are out (one B buffer: 128 + 3 x 32 operand registers).
__global__ __launch_bounds__(512) void ca_gemm_fp8_kernel_x(const CaGemmDesc d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  int tm, tn;
  if (!tile_of_block<4, 8>(blockIdx.x, (d.M + XBM - 1) / XBM, (d.N + XBN - 1) / XBN, tm, tn)) return;
  const int m0 = tm * XBM, n0 = tn * XBN;
  KMajorStream<4> la, lb;
  la.init_bytes((const char*)d.A, d.lda, m0, d.M, wave, lane);
  lb.init_bytes((const char*)d.B, d.ldb, n0, d.N, wave, lane);
  f32x4_t acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  const int K = d.K;
  constexpr int FBK = 128;
  const int nk = (K + FBK - 1) / FBK;
  auto burst = [&](int kt) {
    if (kt >= nk) return;
    char* na = smem + (kt & 1) * XTILE;
    char* nb = na + 2 * XTILE;
    const bool full = (kt + 1) * FBK <= K;
    if (full) {
#pragma unroll
      for (int part = 0; part < 4; ++part) {
        la.issue_one(na, wave, part);
        lb.issue_one(nb, wave, part);
      }
    } else {
#pragma unroll
      for (int part = 0; part < 4; ++part) {
        la.issue_one_tail(na, wave, K - kt * FBK, part);
        lb.issue_one_tail(nb, wave, K - kt * FBK, part);
      }
    }
    la.advance();
    lb.advance();
  };
  auto zero_tail = [&](int kt) {
    if (kt != nk - 1 || nk * FBK == K) return;
    char* na = smem + (kt & 1) * XTILE;
    la.zero_fix(na, wave, lane, K - kt * FBK);
    lb.zero_fix(na + 2 * XTILE, wave, lane, K - kt * FBK);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  };
  const uint32_t lds0 = (uint32_t)(uintptr_t)(lptr_t)smem;
  const int g = lane >> 4;
  uint32_t abase[2], bbase[2];  // the two 16-B chunks of this lane's 32-byte operand (fragment 0, stage 0)
  {
    const int ra = wm * 128 + (lane & 15), rb = wn * 64 + (lane & 15);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      abase[h] = lds0 + ra * 128 + (((2 * g + h) ^ ((ra >> 1) & 7)) * 16);
      bbase[h] = lds0 + 2 * XTILE + rb * 128 + (((2 * g + h) ^ ((rb >> 1) & 7)) * 16);
    }
  }
  // operand fragments: [fragment][low / high 16 bytes]
  bf16x8_t A0[4][2], A1[4][2], Bq[4][2];
#define F8X_RD_A(ST, F, dst)                                        \
  do {                                                              \
    dst[0] = lds_read_b128<(ST) * XTILE + (F) * 2048>(abase[0]);    \
    dst[1] = lds_read_b128<(ST) * XTILE + (F) * 2048>(abase[1]);    \
  } while (0)
#define F8X_RD_B(ST, F, dst)                                        \
  do {                                                              \
    dst[0] = lds_read_b128<(ST) * XTILE + (F) * 2048>(bbase[0]);    \
    dst[1] = lds_read_b128<(ST) * XTILE + (F) * 2048>(bbase[1]);    \
  } while (0)
#define F8X_SB __builtin_amdgcn_sched_barrier(0)
  auto pack = [&](bf16x8_t (&f)[2]) {
    const i32x4_t lo = __builtin_bit_cast(i32x4_t, f[0]), hi = __builtin_bit_cast(i32x4_t, f[1]);
    return (fp8x32_t){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  };
#define F8X_MM(IH, AF, I, J)                                                                                         \
  do {                                                                                                               \
    acc[(IH) * 4 + (I)][J] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(pack(Bq[J]), pack(AF[I]),              \
                                                                             acc[(IH) * 4 + (I)][J], 0, 0, 0,       \
                                                                             0x7f7f7f7f, 0, 0x7f7f7f7f);             \
    F8X_SB;                                                                                                          \
  } while (0)
  auto wait2 = [&](bf16x8_t (&f)[4][2]) {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(f[0][0]), "+v"(f[0][1]), "+v"(f[1][0]), "+v"(f[1][1]), "+v"(f[2][0]), "+v"(f[2][1]), "+v"(f[3][0]),
                   "+v"(f[3][1]));
  };
  auto kstep = [&](auto st_c, int kt) {
    constexpr int ST = decltype(st_c)::value;
    if (wave >= 4) burst(kt + 1);
    // block 0: A (m-half 0) x B; reads A (m-half 1)
    wait2(A0);
    wait2(Bq);
    F8X_SB;
    __builtin_amdgcn_s_setprio(1);
    F8X_MM(0, A0, 0, 0); F8X_MM(0, A0, 0, 1); F8X_RD_A(ST, 4, A1[0]); F8X_SB;
    F8X_MM(0, A0, 0, 2); F8X_MM(0, A0, 0, 3); F8X_RD_A(ST, 5, A1[1]); F8X_SB;
    F8X_MM(0, A0, 1, 0); F8X_MM(0, A0, 1, 1); F8X_RD_A(ST, 6, A1[2]); F8X_SB;
    F8X_MM(0, A0, 1, 2); F8X_MM(0, A0, 1, 3); F8X_RD_A(ST, 7, A1[3]); F8X_SB;
    F8X_MM(0, A0, 2, 0); F8X_MM(0, A0, 2, 1); F8X_MM(0, A0, 2, 2); F8X_MM(0, A0, 2, 3);
    F8X_MM(0, A0, 3, 0); F8X_MM(0, A0, 3, 1); F8X_MM(0, A0, 3, 2); F8X_MM(0, A0, 3, 3);
    __builtin_amdgcn_s_setprio(0);
    wait2(A1);  // the last fragment reads of tile kt have returned
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    zero_tail(kt + 1);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (wave < 4) burst(kt + 2);
    F8X_SB;
    // block 1: A (m-half 1) x B, one B column at a time; each column's fragment is re-read for tile kt+1 behind its
    // four MFMAs, the m-half-0 fragments of tile kt+1 ride along (harmless stale data after the last tile)
    __builtin_amdgcn_s_setprio(1);
    F8X_MM(1, A1, 0, 0); F8X_MM(1, A1, 1, 0); F8X_RD_A(1 - ST, 0, A0[0]); F8X_SB;
    F8X_MM(1, A1, 2, 0); F8X_MM(1, A1, 3, 0); F8X_RD_B(1 - ST, 0, Bq[0]); F8X_SB;
    F8X_MM(1, A1, 0, 1); F8X_MM(1, A1, 1, 1); F8X_RD_A(1 - ST, 1, A0[1]); F8X_SB;
    F8X_MM(1, A1, 2, 1); F8X_MM(1, A1, 3, 1); F8X_RD_B(1 - ST, 1, Bq[1]); F8X_SB;
    F8X_MM(1, A1, 0, 2); F8X_MM(1, A1, 1, 2); F8X_RD_A(1 - ST, 2, A0[2]); F8X_SB;
    F8X_MM(1, A1, 2, 2); F8X_MM(1, A1, 3, 2); F8X_RD_B(1 - ST, 2, Bq[2]); F8X_SB;
    F8X_MM(1, A1, 0, 3); F8X_MM(1, A1, 1, 3); F8X_RD_A(1 - ST, 3, A0[3]); F8X_SB;
    F8X_MM(1, A1, 2, 3); F8X_MM(1, A1, 3, 3); F8X_RD_B(1 - ST, 3, Bq[3]); F8X_SB;
    __builtin_amdgcn_s_setprio(0);
  };
  burst(0);
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  zero_tail(0);
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  F8X_RD_B(0, 0, Bq[0]); F8X_RD_B(0, 1, Bq[1]); F8X_RD_B(0, 2, Bq[2]); F8X_RD_B(0, 3, Bq[3]);
  F8X_RD_A(0, 0, A0[0]); F8X_RD_A(0, 1, A0[1]); F8X_RD_A(0, 2, A0[2]); F8X_RD_A(0, 3, A0[3]);
  if (wave < 4) burst(1);
  for (int kt = 0; kt < nk; kt += 2) {
    kstep(std::integral_constant<int, 0>{}, kt);
    if (kt + 1 < nk) kstep(std::integral_constant<int, 1>{}, kt + 1);
  }
#undef F8X_RD_A
#undef F8X_RD_B
#undef F8X_MM
#undef F8X_SB
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  CaGemmDesc dd = d;
  dd.alpha = d.alpha * (d.a_scale ? *d.a_scale : 1.f) * (d.b_scale ? *d.b_scale : 1.f);
#pragma unroll
  for (int ih = 0; ih < 2; ++ih) {
    f32x4_t half[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float rs = 1.f;
      if (d.a_row_scale) {
        const int m = m0 + wm * 128 + (ih * 4 + i) * 16 + (lane & 15);
        rs = d.a_row_scale[m < d.M ? m : d.M - 1];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) half[i][j] = acc[ih * 4 + i][j] * rs;
    }
    gemm_epilogue(dd, half, smem, wave, lane, m0 + wm * 128 + ih * 64, n0 + wn * 64, 0, 0, 0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // staging reads done before it is overwritten
  }
}

// ---- launcher ---------------------------------------------------------------------------------------------------------
static const DescKernel k_gemm_fp8[2] = {ca_gemm_fp8_kernel, ca_gemm_fp8_kernel_x};  // 128 x 128, 256 x 256

__global__ void gemm_set_epi_general_fp8_kernel(int on) { g_ca_epi_general = on; }
hipError_t gemm_set_epi_general_fp8(int on) { return gemm_run_epi_general_setter(gemm_set_epi_general_fp8_kernel, on); }

int gemm_launch_fp8(const GemmPlan& p, const CaGemmDesc& d, hipStream_t s, const char* who) {
  static std::atomic<uint64_t> raised[2];  // one family per kernel: their LDS sizes differ
  const int x = p.family == GEMM_X ? 1 : 0;
  if (int rc = gemm_allow_lds(raised[x], &k_gemm_fp8[x], 1, p.lds, who)) return rc;
  return gemm_launch(k_gemm_fp8[x], dim3(p.grid_x, p.grid_y, p.grid_z), p, s, who, d);
}
