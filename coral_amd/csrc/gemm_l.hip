// bf16 GEMM kernel L: 256x128 tile, 8 waves (4x2, 64x64 each), 3 LDS stages, one workgroup per CU.
// For the N = d shapes of the path (out-projection, FFN2 and the data gradients that produce [tokens, d]): 128
// tiles of 256x256 leave half the chip idle, and the 128x128 kernel with its two workgroups per CU runs at the
// per-CU LDS-fill limit (2 x 32 KiB per 64-k step for 2 x 128 x 128 outputs = ~95 GB/s per CU at its in-step rate;
// MI355X_MICROARCH: 66-73 GB/s L2-served).  256x128 tiles give every CU one workgroup (240 tiles at M = 3992,
// N = 1920) at 3/4 of S's fill bytes per FLOP.  Built like kernel X: scalar-base LDS-DMA streams, fragments
// double-buffered in registers with the reads issued BETWEEN the MFMAs of the running block (immediate-offset
// addressing), one barrier per K-step in front of its last block, staggered DMA bursts (waves 0-3 right behind the
// barrier, waves 4-7 one block later).  A K-step has two blocks of 16 MFMAs (k-half 0, k-half 1) per wave.  The 48-KiB
// stages leave room for a ring of three: the LDS-DMA runs TWO tiles ahead behind a counted vmcnt (6 pieces per wave and
// tile), which is what keeps the loop fed when the optimiser's traffic beside the forward stretches the fetch latency.
#include "gemm_common.h"

#define LA_BYTES (LBM * BK * 2)  // 32 KiB
#define LB_BYTES (LBN * BK * 2)  // 16 KiB
#define L_NST 3
static_assert(L_LDS_BYTES == L_NST * (LA_BYTES + LB_BYTES), "147456 >= 8 waves * 64*68*4 (139264) epilogue staging");

template <int AL, int BL>
__global__ __launch_bounds__(512) void ca_gemm_kernel_l(const CaGemmDesc d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;  // 4 x 2 waves, 64x64 each
  int tm, tn;
  if (!tile_of_block<4, 8>(blockIdx.x, (d.M + LBM - 1) / LBM, (d.N + LBN - 1) / LBN, tm, tn, d.xcd_balanced != 0)) return;
  const int m0 = tm * LBM, n0 = tn * LBN;
  const int z = blockIdx.z;
  const int z1 = z / d.batch2, z2 = z % d.batch2;
  const __bf16* A = (const __bf16*)d.A + z1 * d.sA1 + z2 * d.sA2;
  const __bf16* B = (const __bf16*)d.B + z1 * d.sB1 + z2 * d.sB2;
  const int K = d.K;
  const int nk = (K + BK - 1) / BK;

  KMajorStream<4> la_k;
  KMajorStream<2> lb_k;
  MNMajorStream<4, 32> la_f;
  MNMajorStream<2, 16> lb_f;
  if (AL == CA_KMAJOR)
    la_k.init(A, d.lda, m0, d.M, wave, lane);
  else
    la_f.init(A, d.lda, m0, d.M, wave, lane);
  if (BL == CA_KMAJOR)
    lb_k.init(B, d.ldb, n0, d.N, wave, lane);
  else
    lb_f.init(B, d.ldb, n0, d.N, wave, lane);

  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  float lbias[8];  // the lane's bias values, requested a whole main loop ahead of the epilogue
  epi_load_bias(d, lane, n0 + wn * 64, z1, z2, lbias);

  // LDS: A0 | A1 | A2 (32 KiB each) | B0 | B1 | B2 (16 KiB each)
  int bst = 0;  // stage of this wave's next burst (every wave issues its share of every tile, in order)
  auto burst = [&](int kt) {  // this wave's share of tile kt: 4 A pieces + 2 B pieces
    if (kt >= nk) return;
    char* na = smem + bst * LA_BYTES;
    char* nb = smem + L_NST * LA_BYTES + bst * LB_BYTES;
    bst = bst == L_NST - 1 ? 0 : bst + 1;
    const bool full = (kt + 1) * BK <= K;  // wave-uniform
    if (full) {
#pragma unroll
      for (int part = 0; part < 4; ++part) {
        if (AL == CA_KMAJOR)
          la_k.issue_one(na, wave, part);
        else
          la_f.issue_one(na, wave, part);
        if (part < 2) {
          if (BL == CA_KMAJOR)
            lb_k.issue_one(nb, wave, part);
          else
            lb_f.issue_one(nb, wave, part);
        }
      }
    } else {
#pragma unroll
      for (int part = 0; part < 4; ++part) {
        if (AL == CA_KMAJOR)
          la_k.issue_one_tail(na, wave, K - kt * BK, part);
        else
          la_f.issue_one_tail(na, wave, lane, K - kt * BK, part);
        if (part < 2) {
          if (BL == CA_KMAJOR)
            lb_k.issue_one_tail(nb, wave, K - kt * BK, part);
          else
            lb_f.issue_one_tail(nb, wave, lane, K - kt * BK, part);
        }
      }
    }
    if (AL == CA_KMAJOR) la_k.advance(); else la_f.advance();
    if (BL == CA_KMAJOR) lb_k.advance(); else lb_f.advance();
  };
  auto zero_tail = [&](int kt) {
    if (kt != nk - 1 || nk * BK == K) return;
    char* na = smem + (kt % L_NST) * LA_BYTES;
    char* nb = smem + L_NST * LA_BYTES + (kt % L_NST) * LB_BYTES;
    const int krem = K - kt * BK;
    if (AL == CA_KMAJOR) la_k.zero_fix(na, wave, lane, krem); else la_f.zero_fix(na, wave, lane, krem);
    if (BL == CA_KMAJOR) lb_k.zero_fix(nb, wave, lane, krem); else lb_f.zero_fix(nb, wave, lane, krem);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  };
  // per-lane fragment base addresses (stage 0; K-major: one per k-half, fragment = immediate offset;
  // MN-major: one per fragment, k-half = immediate offset)
  const uint32_t lds0 = (uint32_t)(uintptr_t)(lptr_t)smem;
  uint32_t abase[4], bbase[4];
  if (AL == CA_KMAJOR) {
    const int r = wm * 64 + (lane & 15);
#pragma unroll
    for (int sh = 0; sh < 2; ++sh) abase[sh] = lds0 + r * 128 + (((4 * sh + (lane >> 4)) ^ ((r >> 1) & 7)) * 16);
  } else {
    const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
    const int swz = q | ((g & 1) << 2);
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const int c = ((((wm * 64 + f * 16) >> 3) + (pp >> 1)) ^ (swz << 1));
      abase[f] = lds0 + (8 * g + q) * 512 + c * 16 + (pp & 1) * 8;
    }
  }
  if (BL == CA_KMAJOR) {
    const int r = wn * 64 + (lane & 15);
#pragma unroll
    for (int sh = 0; sh < 2; ++sh)
      bbase[sh] = lds0 + L_NST * LA_BYTES + r * 128 + (((4 * sh + (lane >> 4)) ^ ((r >> 1) & 7)) * 16);
  } else {
    const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
    const int swz = q | ((g & 1) << 2);
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const int c = ((((wn * 64 + f * 16) >> 3) + (pp >> 1)) ^ (swz << 1));
      bbase[f] = lds0 + L_NST * LA_BYTES + (8 * g + q) * 256 + c * 16 + (pp & 1) * 8;
    }
  }
  // (DS immediate offsets end at 64 KiB: the third A stage gets base registers of its own)
  uint32_t abase2[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) abase2[f] = abase[f] + 2 * LA_BYTES;
  bf16x8_t A0[4], A1[4], B0[4], B1[4];
#define L_RD_A(ST, SH, F, dst)                                                                      \
  do {                                                                                              \
    if (AL == CA_KMAJOR)                                                                            \
      dst = lds_read_b128<((ST) % 2) * LA_BYTES + (F) * 2048>((ST) == 2 ? abase2[SH] : abase[SH]);  \
    else                                                                                            \
      dst = lds_read_tr<((ST) % 2) * LA_BYTES + (SH) * 16384, 2048>((ST) == 2 ? abase2[F] : abase[F]); \
  } while (0)
#define L_RD_B(ST, SH, F, dst)                                                  \
  do {                                                                          \
    if (BL == CA_KMAJOR)                                                        \
      dst = lds_read_b128<(ST) * LB_BYTES + (F) * 2048>(bbase[SH]);             \
    else                                                                        \
      dst = lds_read_tr<(ST) * LB_BYTES + (SH) * 8192, 1024>(bbase[F]);         \
  } while (0)
#define L_SB __builtin_amdgcn_sched_barrier(0)
#define L_MM2(AF, BF, I, J)                                                                             \
  do {                                                                                                  \
    acc[I][J] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(BF[J], AF[I], acc[I][J], 0, 0, 0);              \
    acc[I][(J) + 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(BF[(J) + 1], AF[I], acc[I][(J) + 1], 0, 0, 0); \
    L_SB;                                                                                               \
  } while (0)
  auto kstep = [&](auto st_c, int kt) {
    constexpr int ST = decltype(st_c)::value;
    constexpr int NS = (ST + 1) % L_NST;  // stage of tile kt + 1
    if (wave >= 4) burst(kt + 2);
    // block 0: k-half 0 of tile kt; reads k-half 1 (same stage)
    lds_wait(B0);
    lds_wait(A0);
    L_SB;
    __builtin_amdgcn_s_setprio(1);
    L_MM2(A0, B0, 0, 0); L_RD_B(ST, 1, 0, B1[0]); L_SB;
    L_MM2(A0, B0, 0, 2); L_RD_B(ST, 1, 1, B1[1]); L_SB;
    L_MM2(A0, B0, 1, 0); L_RD_B(ST, 1, 2, B1[2]); L_SB;
    L_MM2(A0, B0, 1, 2); L_RD_B(ST, 1, 3, B1[3]); L_SB;
    L_MM2(A0, B0, 2, 0); L_RD_A(ST, 1, 0, A1[0]); L_SB;
    L_MM2(A0, B0, 2, 2); L_RD_A(ST, 1, 1, A1[1]); L_SB;
    L_MM2(A0, B0, 3, 0); L_RD_A(ST, 1, 2, A1[2]); L_SB;
    L_MM2(A0, B0, 3, 2); L_RD_A(ST, 1, 3, A1[3]); L_SB;
    __builtin_amdgcn_s_setprio(0);
    lds_wait(B1);
    lds_wait(A1);  // the last fragment reads of tile kt have returned
    // tile kt+1 has landed (this wave's share; the barrier covers the others), tile kt+2 may still be in flight
    if (kt + 2 < nk)
      asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    zero_tail(kt + 1);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (wave < 4) burst(kt + 3);  // into stage ST: every wave has finished reading tile kt
    L_SB;
    // block 1: k-half 1 of tile kt; reads k-half 0 of tile kt+1 (harmless stale data after the last tile)
    __builtin_amdgcn_s_setprio(1);
    L_MM2(A1, B1, 0, 0); L_RD_B(NS, 0, 0, B0[0]); L_SB;
    L_MM2(A1, B1, 0, 2); L_RD_B(NS, 0, 1, B0[1]); L_SB;
    L_MM2(A1, B1, 1, 0); L_RD_B(NS, 0, 2, B0[2]); L_SB;
    L_MM2(A1, B1, 1, 2); L_RD_B(NS, 0, 3, B0[3]); L_SB;
    L_MM2(A1, B1, 2, 0); L_RD_A(NS, 0, 0, A0[0]); L_SB;
    L_MM2(A1, B1, 2, 2); L_RD_A(NS, 0, 1, A0[1]); L_SB;
    L_MM2(A1, B1, 3, 0); L_RD_A(NS, 0, 2, A0[2]); L_SB;
    L_MM2(A1, B1, 3, 2); L_RD_A(NS, 0, 3, A0[3]); L_SB;
    __builtin_amdgcn_s_setprio(0);
  };
  burst(0);
  burst(1);
  if (nk > 1)
    asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)" ::: "memory");
  else
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  zero_tail(0);
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  L_RD_B(0, 0, 0, B0[0]); L_RD_B(0, 0, 1, B0[1]); L_RD_B(0, 0, 2, B0[2]); L_RD_B(0, 0, 3, B0[3]);
  L_RD_A(0, 0, 0, A0[0]); L_RD_A(0, 0, 1, A0[1]); L_RD_A(0, 0, 2, A0[2]); L_RD_A(0, 0, 3, A0[3]);
  if (wave < 4) burst(2);
  for (int kt = 0; kt < nk; kt += 3) {
    kstep(std::integral_constant<int, 0>{}, kt);
    if (kt + 1 < nk) kstep(std::integral_constant<int, 1>{}, kt + 1);
    if (kt + 2 < nk) kstep(std::integral_constant<int, 2>{}, kt + 2);
  }
#undef L_RD_A
#undef L_RD_B
#undef L_MM2
#undef L_SB
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  gemm_epilogue(d, acc, smem, wave, lane, m0 + wm * 64, n0 + wn * 64, z, z1, z2, &lbias);
}

#undef LA_BYTES
#undef LB_BYTES
#undef L_NST

// ---- launcher ---------------------------------------------------------------------------------------------------------
// Layouts indexed a_layout * 2 + b_layout.
static const DescKernel k_gemm_l[4] = {ca_gemm_kernel_l<0, 0>, ca_gemm_kernel_l<0, 1>, ca_gemm_kernel_l<1, 0>, ca_gemm_kernel_l<1, 1>};

__global__ void gemm_set_epi_general_l_kernel(int on) { g_ca_epi_general = on; }
hipError_t gemm_set_epi_general_l(int on) { return gemm_run_epi_general_setter(gemm_set_epi_general_l_kernel, on); }

int gemm_launch_l(const GemmPlan& p, const CaGemmDesc& d, hipStream_t s, const char* who) {
  static std::atomic<uint64_t> raised{0};
  if (int rc = gemm_allow_lds(raised, k_gemm_l, 4, p.lds, who)) return rc;
  return gemm_launch(k_gemm_l[p.lay], dim3(p.grid_x, p.grid_y, p.grid_z), p, s, who, d);
}
