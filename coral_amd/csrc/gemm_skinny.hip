// bf16 GEMM, skinny-M kernel: M <= 32 rows per workgroup (one decoded token per clip), weights streamed from HBM.
// C[m, n] = epilogue(alpha * sum_k A[m, k] W[n, k]): a weight-streaming problem (every weight byte is used once),
// so there is no LDS staging: each wave owns 16 output columns and a quarter of K, loads its W fragment
// (16 rows x 64 B) and the matching A fragment(s) straight from global memory into MFMA operands, eight k-steps
// in flight; the four waves of a workgroup add their partial tiles through LDS and wave 0 runs the epilogue.
// N/16 workgroups: 64 (N = 1024) to 3242 (the 51865-entry vocabulary).  MB = row blocks of 16: a batch of 17..32 clips
// takes a second A fragment and accumulator against the SAME weight fragment (round 3: the launches and the weight
// bytes of a decoded token are shared by twice the clips).
// LN (CaGemmDesc.a_ln_gamma): the A rows are LayerNorm(A rows), formed by every workgroup in its prologue (the
// arithmetic of ln_fwd_kernel, chunk by chunk: a wave per row, the normalised row rounded to bf16 as the LayerNorm
// launch would have stored it) into an LDS image the MFMA operand loads then read - the LayerNorm launch in front of
// the q|k|v and fc1 projections of a decoded token (4.9 us each from dispatch to completion, a quarter of them a
// memory round trip) disappears from the per-token chain; bit-identical to the two launches.  The first eight weight
// fragments of every wave (all of them at K = 1024) are asked for BEFORE the prologue, so the statistics run under
// the weight fetch.
// NCH: 64-lane rounds of 8-element chunks a row takes (K <= 512 NCH), 0 = no LayerNorm prologue
// Round 5: 33 .. 128 rows (an evaluation run decodes more clips per step than 32 - R/config/evaluation.yaml:20,
// R/src/coral/evaluate.py:56-60) run the SAME 32-row kernel on a two-dimensional grid: blockIdx.y picks the block of 32
// rows.  A workgroup then streams 64 KB of A per 1024 k beside its 32 KB of weights, as at 32 rows (four row blocks in one
// workgroup measured 17.7 us per launch at 64 rows against 8 at 32: the A rows, re-read by every workgroup, were 4/5 of
// its bytes); the weight fragment is read by the 2 - 4 workgroups of a column block, once from HBM and then from L2.
// Round 6: NT = output columns per workgroup (16, 8 or 4: MFMA rows NT .. 15 repeat rows 0 .. NT-1 and are dropped), U =
// k-steps a wave asks for at once.  What a launch of this kernel costs is the bytes its BUSIEST CU takes in (~10 B/clk
// per CU from HBM, the weights; ~3x that from L2, the activation rows every workgroup reads): at N = 1024 sixteen-column
// workgroups put the whole weight matrix through 64 CUs (fc2 of a decoded token at 16 clips: 128 KB of weights + 128 KB
// of activations per CU, in four dependent rounds of eight k-steps: 13 us); four-column workgroups on 256 CUs with the
// wave's whole K quarter in flight take 32 KB of weights each.  Per output element the same K split and the same MFMA
// chain: the same bits whatever NT and U.
#include "gemm_common.h"

template <int MB, int NCH = 0, int U = 8, int NT = 16>
__global__ __launch_bounds__(256) void ca_gemm_skinny_kernel(const CaGemmDesc d) {
  constexpr bool LN = NCH > 0;
  static_assert(!LN || U == 8, "the LayerNorm prologue keeps eight weight fragments in flight");
  static_assert(NT == 16 || NT == 8 || NT == 4, "4, 8 or 16 columns per workgroup");
  const int mrow0 = (int)blockIdx.y * 16 * MB;  // first row of this workgroup's row block
  constexpr int NC = LN ? NCH : 1;
  extern __shared__ __attribute__((aligned(16))) char sk_smem[];
  float(*part)[MB * 16 * 16] = (float(*)[MB * 16 * 16]) sk_smem;
  unsigned short* const xs = (unsigned short*)(sk_smem + 4 * MB * 256 * sizeof(float));  // LN only: [16 MB][K + pad]
  const int xpitch = d.K + SKINNY_LN_PAD;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n0 = blockIdx.x * NT;
  const int r = lane & 15, g = lane >> 4;
  const __bf16* A = (const __bf16*)d.A;
  const __bf16* W = (const __bf16*)d.B;
  const int rr = r & (NT - 1);  // (MFMA rows beyond NT: copies, same addresses - one request)
  const int nrow = n0 + rr < d.N ? n0 + rr : d.N - 1;
  const __bf16* wp = W + (int64_t)nrow * d.ldb + 8 * g;
  const __bf16* ap[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int m = mrow0 + 16 * mb + r;
    ap[mb] = A + (int64_t)(m < d.M ? m : d.M - 1) * d.lda + 8 * g;
  }
  const int ksteps = (d.K + 31) / 32;
  const int per = (ksteps + 3) / 4;
  const int ks0 = wave * per, ks1 = (ks0 + per < ksteps) ? ks0 + per : ksteps;
  f32x4_t acc[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) acc[mb] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  const bf16x8_t zero = __builtin_bit_cast(bf16x8_t, (f32x4_t){0.f, 0.f, 0.f, 0.f});
  // The kernel is a short chain of memory round trips behind a ~4 us dependent launch (measured: 4.0 us per launch
  // in a graph at N = K = 1024, +1 us per 24 KB a workgroup streams - the per-CU fill rate - tools/archive/dev_skinny_time.py),
  // so the epilogue's operands (bias, residual, destination row) are asked for up front, beside the first K-steps.
  const int epi = d.epilogue;
  const bool wave0 = wave == 0;
  float e_bias[4] = {0.f, 0.f, 0.f, 0.f}, e_res[MB][4];
  int64_t crow[MB];
  // c_split_n: columns [c_split_n, N) go to a second output (C_hi, ldc_hi; column index n - c_split_n) and only they
  // take the c_row_index rows - q and the cached K|V rows of a decoded token from one launch.  n0 is a multiple of
  // 16 and so is c_split_n: a workgroup is on one side.
  const bool hi = d.c_split_n > 0 && n0 >= d.c_split_n;
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int m = mrow0 + 16 * mb + r;
    crow[mb] = m;
#pragma unroll
    for (int e = 0; e < 4; ++e) e_res[mb][e] = 0.f;
    if (wave0 && m < d.M) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int n = n0 + 4 * g + e;
        if (n < d.N && 4 * g + e < NT) {
          if (mb == 0 && d.bias) e_bias[e] = d.bias[n];
          if (epi == CA_EPI_GELU_RESIDUAL || epi == CA_EPI_RESIDUAL)
            e_res[mb][e] = bf2f(((const unsigned short*)d.R)[(int64_t)m * d.ldr + n]);
        }
      }
      if (d.c_row_index && (d.c_split_n == 0 || hi)) crow[mb] = (int64_t)m * d.c_row_mul + d.c_row_index[m];
    }
  }
  void* const Cdst = hi ? d.C_hi : d.C;
  const int64_t ldcd = hi ? d.ldc_hi : d.ldc;
  const int ncol0 = hi ? d.c_split_n : 0;
  bf16x8_t wf0[8];  // LN: the first iteration's weight fragments, in flight across the prologue
  if constexpr (LN) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = (ks0 + u) * 32 + 8 * g;
      wf0[u] = (ks0 + u < ks1 && k < d.K) ? *(const bf16x8_t*)(wp + (int64_t)(ks0 + u) * 32) : zero;
    }
    // rows wave, wave + 4, ...: all of a wave's rows are asked for before the first statistic (one round trip)
    constexpr int RW = MB * 4;
    const int C = d.K, nchunk = C >> 3;
    const unsigned short* xr = (const unsigned short*)d.A;
    u16x8_t raw[RW][NC];
#pragma unroll
    for (int i = 0; i < RW; ++i) {
      const int row = mrow0 + wave + 4 * i;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int ch = lane + c * 64;
        raw[i][c] = (row < d.M && ch < nchunk) ? *(const u16x8_t*)(xr + (int64_t)row * d.lda + ch * 8)
                                               : (u16x8_t){0, 0, 0, 0, 0, 0, 0, 0};
      }
    }
    f32x4_t gq[NC][2], bq[NC][2];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int ch = lane + c * 64;
      if (ch < nchunk) {
        gq[c][0] = *(const f32x4_t*)(d.a_ln_gamma + ch * 8);
        gq[c][1] = *(const f32x4_t*)(d.a_ln_gamma + ch * 8 + 4);
        bq[c][0] = *(const f32x4_t*)(d.a_ln_beta + ch * 8);
        bq[c][1] = *(const f32x4_t*)(d.a_ln_beta + ch * 8 + 4);
      }
    }
#pragma unroll
    for (int i = 0; i < RW; ++i) {
      const int lrow = wave + 4 * i;  // row of the LDS image; global row mrow0 + lrow
      const int row = mrow0 + lrow;
      if (row >= d.M) break;  // (wave-uniform)
      float sx = 0.f;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if (lane + c * 64 < nchunk) {
#pragma unroll
          for (int e = 0; e < 8; ++e) sx += bf2f(raw[i][c][e]);
        }
      }
      const float mean = wave_sum(sx) / (float)C;
      float s2 = 0.f;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if (lane + c * 64 < nchunk) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float dlt = bf2f(raw[i][c][e]) - mean;
            s2 += dlt * dlt;
          }
        }
      }
      const float rstd = rsqrtf(wave_sum(s2) / (float)C + d.a_ln_eps);
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int ch = lane + c * 64;
        if (ch < nchunk) {
          u16x8_t o8;
#pragma unroll
          for (int e = 0; e < 8; ++e)
            o8[e] = f2bf(ln_apply(bf2f(raw[i][c][e]), mean, rstd, e < 4 ? gq[c][0][e] : gq[c][1][e - 4],
                                  e < 4 ? bq[c][0][e] : bq[c][1][e - 4]));
          *(u16x8_t*)(xs + (int64_t)lrow * xpitch + ch * 8) = o8;
        }
      }
    }
    __syncthreads();
  }
  for (int ks = ks0; ks < ks1; ks += U) {
    bf16x8_t wf[U], af[MB][U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = (ks + u) * 32 + 8 * g;
      const bool ok = ks + u < ks1 && k < d.K;  // K is a multiple of 8 (lda/ldb rule), so a chunk is all-or-nothing
      if constexpr (LN) {
        wf[u] = ks == ks0 ? wf0[u] : (ok ? *(const bf16x8_t*)(wp + (int64_t)(ks + u) * 32) : zero);
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
          af[mb][u] = (ok && mrow0 + 16 * mb + r < d.M) ? *(const bf16x8_t*)(xs + (int64_t)(16 * mb + r) * xpitch + k) : zero;
      } else {
        wf[u] = ok ? *(const bf16x8_t*)(wp + (int64_t)(ks + u) * 32) : zero;
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
          af[mb][u] = (ok && mrow0 + 16 * mb + r < d.M) ? *(const bf16x8_t*)(ap[mb] + (int64_t)(ks + u) * 32) : zero;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[u], af[mb][u], acc[mb], 0, 0, 0);
  }
  // D[n = 4g + e][m = r]: lane holds 4 consecutive n of row m
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int e = 0; e < 4; ++e) part[wave][mb * 256 + r * 16 + 4 * g + e] = acc[mb][e];
  __syncthreads();
  if (!wave0) return;
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    if (mrow0 + 16 * mb + r >= d.M) continue;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int n = n0 + 4 * g + e;
      if (n >= d.N || 4 * g + e >= NT) continue;
      const int i = mb * 256 + r * 16 + 4 * g + e;
      float v = (part[0][i] + part[1][i]) + (part[2][i] + part[3][i]);
      v = v * d.alpha + e_bias[e];
      float v2 = 0.f;
      if (epi == CA_EPI_GELU || epi == CA_EPI_GELU_RESIDUAL) {
        v2 = gelu_erf(v);
        if (epi == CA_EPI_GELU_RESIDUAL) v2 += e_res[mb][e];
      } else if (epi == CA_EPI_RESIDUAL) {
        v += e_res[mb][e];
      }
      const int64_t off = crow[mb] * ldcd + (n - ncol0);
      if (Cdst) {
        if (d.out_f32)
          ((float*)Cdst)[off] = d.accumulate ? ((float*)Cdst)[off] + v : v;
        else
          ((unsigned short*)Cdst)[off] = f2bf(d.accumulate ? bf2f(((unsigned short*)Cdst)[off]) + v : v);
      }
      if ((epi == CA_EPI_GELU || epi == CA_EPI_GELU_RESIDUAL) && d.C2) ((unsigned short*)d.C2)[off] = f2bf(v2);
    }
  }
}

// ---- launcher ---------------------------------------------------------------------------------------------------------
struct SkinnyKernel {
  int mb, nch, u, nt;
  DescKernel fn;
};
#define SK(MB, NCH, U, NT) {MB, NCH, U, NT, ca_gemm_skinny_kernel<MB, NCH, U, NT>}
#define SK_NT(MB, NCH, U) SK(MB, NCH, U, 16), SK(MB, NCH, U, 8), SK(MB, NCH, U, 4)
static const SkinnyKernel k_gemm_skinny[] = {
    SK_NT(1, 0, 8), SK_NT(1, 0, 16), SK_NT(1, 0, 32), SK(2, 0, 8, 16),                                  // plain
    SK_NT(1, 2, 8), SK_NT(1, 3, 8),  SK_NT(1, 4, 8),  SK(2, 2, 8, 16), SK(2, 3, 8, 16), SK(2, 4, 8, 16)  // LayerNorm(A)
};
#undef SK_NT
#undef SK

int gemm_launch_skinny(const GemmPlan& p, const CaGemmDesc& d, hipStream_t s, const char* who) {
  if (p.nch > 0) {  // the LayerNorm prologue's LDS image of the A rows: up to 160 KiB
    static std::atomic<uint64_t> raised{0};
    const int n = (int)(sizeof(k_gemm_skinny) / sizeof(k_gemm_skinny[0]));
    const auto ln_kernel = [](const SkinnyKernel& k) { return k.nch > 0 ? (const void*)k.fn : nullptr; };
    if (int rc = gemm_allow_lds(raised, k_gemm_skinny, n, ln_kernel, 160 * 1024, who)) return rc;
  }
  for (const SkinnyKernel& k : k_gemm_skinny)
    if (k.mb == p.mb && k.nch == p.nch && k.u == p.u && k.nt == p.nt) return gemm_launch(k.fn, dim3(p.grid_x, p.grid_y), p, s, who, d);
  ca_set_error("%s: no skinny kernel <%d, %d, %d, %d>", who, p.mb, p.nch, p.u, p.nt);
  return CA_ERR_UNSUPPORTED;
}
