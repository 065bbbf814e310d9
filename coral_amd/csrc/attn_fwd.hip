// Attention forward: the 64-query kernel and the 128-query (wide) kernel.  See attn_common.h.
#include "attn_common.h"

// ---- forward ----------------------------------------------------------------------------------------
// One pass over the key tiles with a running maximum (online softmax).  Scores are kept in log2 units
// (s * scale * log2 e), so a probability costs one FMA and one v_exp_f32.  The running maximum of a
// query is shared by the four lane groups that hold its keys (two xor-shuffles per tile); the output
// accumulators, whose rows are queries 4g+e, pick up their rescale factor from the lane that owns the
// query (one shuffle per row) and are only touched when some maximum in the wave moved.  Tiles that lie
// fully inside the valid key range take a path without any per-element masking.
// 1024 workgroups at the path's shape (8 query tiles x 128 heads): at 4 waves per SIMD they are all resident at
// once; at 3 (148 VGPRs) a second round runs one third full.
// KM (CaAttnDesc.kstart, causal): the row's keys start at kstart[b] - attn_kstart_shift; qc is the query in shifted indices.
template <int HDPV, bool DROP = false, bool KM = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void attn_fwd_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NKS = HDPV / 32, NNB = HDPV / 16;
  char* Kimg = smem;                  // K-major image of the key tile
  char* Vimg = smem + 64 * HDPV * 2;  // MN-major image of the value tile
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, r = lane & 15;
  int tile, h, b;
  if (!attn_tile_of_block((a.Tq + 63) / 64, a.H, a.B, tile, h, b)) return;
  attn_packed_rows(a, b);
  if (tile * (64) >= a.Tq) return;  // (packed rows: the tile lies past the utterance)
  const int hd = a.hd;
  const unsigned short* Q = a.Q + b * a.sqb + h * hd;
  const unsigned short* K = a.K + b * a.skb + h * hd;
  const unsigned short* V = a.V + b * a.svb + h * hd;
  const int q0 = tile * 64 + wave * 16;
  const int qi = q0 + r;  // this lane's query (column of the transposed score tile)
  const int qrow = qi < a.Tq ? qi : a.Tq - 1;
  int Tk = a.Tk, kl = a.Tk;
  if (a.klen) kl = a.klen[b] < kl ? a.klen[b] : kl;
  int kshift = 0;
  if constexpr (KM) kshift = attn_kstart_shift(a, b, K, V, Tk, kl);
  const int qc = qi - kshift;
  // all HDPV/32 k-steps and HDPV/16 column blocks are computed: dims >= hd are zero in every LDS image
  bf16x8_t qf[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) qf[ks] = load_rowfrag(Q, a.ldq, qrow, ks, lane, hd);
  int ntile = (kl + 63) / 64;
  if constexpr (KM) {
    const int last = tile * 64 + 63 - kshift;  // the tile's last query, shifted: below 0 = no key is allowed
    const int nc = last >= 0 ? last / 64 + 1 : 0;
    ntile = ntile < nc ? ntile : nc;
  } else {
    if (a.causal && ntile > tile + 1) ntile = tile + 1;  // keys beyond the tile's last query are masked
  }
  const float c2 = a.scale * LOG2E;

  float m = NEG_BIG, l = 0.f;  // running max (log2 units, same in the 4 lanes of a query) / this lane's partial sum
  f32x4_t o[NNB];
#pragma unroll
  for (int nb = 0; nb < NNB; ++nb) o[nb] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  KImgFast<64, HDPV> kfast;
  MnImgFast<64, HDPV> vfast;
  kfast.init(a.ldk, wave, lane);
  vfast.init(a.ldv, wave, lane);
  const int nfast = fast_tiles(Tk, 64);
  for (int kt = 0; kt < ntile; ++kt) {
    if (kt < nfast) {
      kfast.issue(Kimg, K + (int64_t)kt * 64 * a.ldk, wave);
      vfast.issue(Vimg, V + (int64_t)kt * 64 * a.ldv, wave);
    } else {
      load_kmajor_image<64, HDPV>(Kimg, K, a.ldk, kt * 64, Tk, hd, wave, lane);
      load_mnmajor_image<64, HDPV>(Vimg, V, a.ldv, kt * 64, Tk, hd, wave, lane);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // transposed scores of the 64 keys: block (s, bb) holds keys 32 s + 8 g + 4 bb + {0..3} of query qi
    f32x4_t sc[4];
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) {
      f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
      const int row = 32 * (blk >> 1) + rowperm(blk & 1, r);
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kimg_frag<64>(Kimg, row, ks, lane), qf[ks], acc, 0, 0, 0);
      sc[blk] = acc;
    }
    const bool full = (kt * 64 + 64 <= kl) && !a.causal;  // uniform: no element of this tile is masked
    if (!full) {
#pragma unroll
      for (int blk = 0; blk < 4; ++blk)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int key = kt * 64 + 32 * (blk >> 1) + 8 * g + 4 * (blk & 1) + e;
          const bool ok = key < kl && (!a.causal || key <= qc);
          sc[blk][e] = ok ? sc[blk][e] : NEG_BIG;
        }
    }
    float tmax = fmaxf(fmaxf(sc[0][0], sc[0][1]), fmaxf(sc[0][2], sc[0][3]));
#pragma unroll
    for (int blk = 1; blk < 4; ++blk)
      tmax = fmaxf(tmax, fmaxf(fmaxf(sc[blk][0], sc[blk][1]), fmaxf(sc[blk][2], sc[blk][3])));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float m_new = fmaxf(m, tmax * c2);
    const float alpha = __builtin_amdgcn_exp2f(m - m_new);
    float p[16];
    float sum = 0.f;
#pragma unroll
    for (int blk = 0; blk < 4; ++blk)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pv = __builtin_amdgcn_exp2f(fmaf(sc[blk][e], c2, -m_new));
        if (!full) pv = sc[blk][e] > 0.5f * NEG_BIG ? pv : 0.f;
        p[4 * blk + e] = pv;
        sum += pv;  // the normaliser is the sum of ALL probabilities: dropout acts on the normalised ones
      }
    if constexpr (DROP) {
      const float ks = 1.f / (1.f - a.drop_p);
#pragma unroll
      for (int blk = 0; blk < 4; ++blk) {
        const int key0 = kt * 64 + 32 * (blk >> 1) + 8 * g + 4 * (blk & 1);
        const unsigned keep = ca_dropout_keep4(a.drop_seed, attn_drop_index(a, b, h, qrow, key0), a.drop_p);
#pragma unroll
        for (int e = 0; e < 4; ++e) p[4 * blk + e] = ((keep >> e) & 1u) ? p[4 * blk + e] * ks : 0.f;
      }
    }
    l = fmaf(l, alpha, sum);
    if (__builtin_amdgcn_ballot_w64(m_new > m) != 0) {  // some query of this wave moved its maximum
      float ar[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) ar[e] = __shfl(alpha, 4 * g + e, 64);
#pragma unroll
      for (int nb = 0; nb < NNB; ++nb)
#pragma unroll
        for (int e = 0; e < 4; ++e) o[nb][e] *= ar[e];
    }
    m = m_new;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float ps[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) ps[e] = p[8 * s + e];
      const bf16x8_t pf = pack8(ps);
#pragma unroll
      for (int nb = 0; nb < NNB; ++nb)
        o[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, timg_frag<HDPV>(Vimg, s, nb, lane), o[nb], 0, 0, 0);
    }
    __syncthreads();
  }
  // total of the four lane groups that share a query; lse in natural-log units for the backward
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  // (KM: a row in front of its first key has attended to nothing by design, and writes nothing that is not finite)
  const float lse = l > 0.f ? (m + __builtin_amdgcn_logf(l)) * 0.69314718055994530942f : (KM ? 0.f : __builtin_inff());
  if (g == 0 && qi < a.Tq && a.lse) a.lse[((int64_t)b * a.H + h) * a.Tqp + qi] = lse;
  const float inv = l > 0.f ? 1.0f / l : 0.f;  // nothing attended -> zero output
  float ir[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) ir[e] = __shfl(inv, 4 * g + e, 64);
  unsigned short* O = a.O + b * a.sob + h * hd;
  // (every loop iteration ended with a workgroup barrier: the images are free)
  store_tile16<HDPV>(smem + wave * (attn_stage_bytes(HDPV) / 4), o, ir, O, a.ldo, q0, a.Tq, hd, lane);
}

// ---- forward, wide workgroups ---------------------------------------------------------------------------------------
// NW waves x 32 queries per workgroup (two 16-query blocks per wave: every K / V fragment read feeds two MFMAs), key /
// value tiles in a ring of NST image pairs with NST - 1 tiles in flight and counted waits (the fast path's LDS-DMA is
// inline asm in a fixed order: DPT instructions per wave and tile).  Tiles fully inside the valid keys run a body
// without any per-element compare / select (written as a run-time `if`, the compiler turns the masks into selects that
// run for every tile: ~190 of ~540 vector instructions per 64 MFMAs); the ragged last tile and causal tiles run the
// masked body in a loop of their own.
// Measured at the XLS-R-2B shape (B 8, H 16, T 499, hd 120; by switching parts of the kernel off): 10 us before the
// first MFMA (launch, the query fragments and the first tile: latency, not bandwidth), 22 us of loop, 5 us of
// output burst.  In the loop the two waves of a SIMD run in lock step behind the per-tile barrier, so per tile and SIMD
// 2 x 64 MFMAs (2048 cycles) and 2 x ~250 vector instructions (~2200 cycles) add up instead of overlapping.  128
// queries x 4 waves x 2 image pairs (two workgroups per CU, which drift apart) runs 9 % faster than the 64-query
// kernel; 256 queries x 8 waves x 4 pairs (one workgroup per CU) measured the same or slower, so only the former is
// instantiated.
template <int N>
using IC = std::integral_constant<int, N>;
// WPE = workgroups (waves per SIMD) the register budget is held to.  Round 4: the kernel is bound by vector-instruction
// issue with both waves of a SIMD stalled ~35 % of the time (LDS fragment reads, the per-tile barrier, MFMA results), and
// a THIRD resident wave hides most of that: the head_dim <= 64 form holds 154 registers (512 / 3 = 170), so it runs three
// workgroups per CU - whisper-medium encoder forward 136 -> 124 us per layer, whisper-large-turbo 166 -> 148
// (tools/archive/exp_attn_env.sh, interleaved).  Measured and dropped on the way: forming the scores of tile kt + 1 under the
// softmax of tile kt inside one wave (a third image pair and a second score set, 230 registers: 5 % SLOWER - the
// co-resident waves already overlap the two pipes, what is short is issue slots), and four waves per SIMD at 128
// registers (27 spilled dwords: 183 us).
// KM (CaAttnDesc.kstart, causal): as in attn_fwd_kernel; qc[] are the queries in shifted indices.
template <int HDPV, bool DROP, int NW, int NST, int WPE = 2, bool KM = false>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void attn_fwd_wide_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NQ = 2, NKS = HDPV / 32, NNB = HDPV / 16;
  constexpr int IMG = 64 * HDPV * 2, PAIR = 2 * IMG;  // a tile = K-major image of the keys + MN-major image of the values
  constexpr int QPB = NW * 16 * NQ;                   // queries per workgroup
  constexpr int DPT = (HDPV / 64) * (64 / 8 / NW) + 64 * HDPV * 2 / 1024 / NW;  // LDS-DMA instructions per wave and tile
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, r = lane & 15;
  int tile, h, b;
  if (!attn_tile_of_block((a.Tq + QPB - 1) / QPB, a.H, a.B, tile, h, b)) return;
  attn_packed_rows(a, b);
  if (tile * (QPB) >= a.Tq) return;  // (packed rows: the tile lies past the utterance)
  const int hd = a.hd;
  const unsigned short* Q = a.Q + b * a.sqb + h * hd;
  const unsigned short* K = a.K + b * a.skb + h * hd;
  const unsigned short* V = a.V + b * a.svb + h * hd;
  const int q0 = tile * QPB + wave * 16 * NQ;
  int qi[NQ], qrow[NQ];  // this lane's queries (columns of the transposed score tiles)
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    qi[j] = q0 + 16 * j + r;
    qrow[j] = qi[j] < a.Tq ? qi[j] : a.Tq - 1;
  }
  int Tk = a.Tk, kl = a.Tk;
  if (a.klen) kl = a.klen[b] < kl ? a.klen[b] : kl;
  int kshift = 0;
  if constexpr (KM) kshift = attn_kstart_shift(a, b, K, V, Tk, kl);
  int qc[NQ];
#pragma unroll
  for (int j = 0; j < NQ; ++j) qc[j] = qi[j] - kshift;
  int ntile = (kl + 63) / 64;
  if constexpr (KM) {
    const int lastq = tile * QPB + QPB - 1 - kshift;  // the workgroup's last query, shifted: below 0 = no key is allowed
    const int last = lastq >= 0 ? lastq / 64 + 1 : 0;
    ntile = ntile < last ? ntile : last;
  } else if (a.causal) {  // keys beyond the workgroup's last query are masked
    const int last = (tile * QPB + QPB - 1) / 64 + 1;
    ntile = ntile < last ? ntile : last;
  }
  KImgFast<64, HDPV, NW> kfast;
  MnImgFast<64, HDPV, NW> vfast;
  kfast.init(a.ldk, wave, lane);
  vfast.init(a.ldv, wave, lane);
  const int nfast = fast_tiles(Tk, 64);
  auto issue = [&](int kt, int stage) __attribute__((always_inline)) {
    char* img = smem + stage * PAIR;
    if (kt < nfast) {
      kfast.issue(img, K + (int64_t)kt * 64 * a.ldk, wave);
      vfast.issue(img + IMG, V + (int64_t)kt * 64 * a.ldv, wave);
    } else {
      load_kmajor_image<64, HDPV, NW>(img, K, a.ldk, kt * 64, Tk, hd, wave, lane);
      load_mnmajor_image<64, HDPV, NW>(img + IMG, V, a.ldv, kt * 64, Tk, hd, wave, lane);
    }
  };
#pragma unroll
  for (int t = 0; t < NST - 1; ++t)
    if (t < ntile) issue(t, t);
  // all HDPV/32 k-steps and HDPV/16 column blocks are computed: dims >= hd are zero in every LDS image
  bf16x8_t qf[NQ][NKS];
#pragma unroll
  for (int j = 0; j < NQ; ++j)
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[j][ks] = load_rowfrag(Q, a.ldq, qrow[j], ks, lane, hd);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the query fragments are younger than the first tiles)
  const float c2 = a.scale * LOG2E;

  float m[NQ], l[NQ];  // running max (log2 units, same in the 4 lanes of a query) / this lane's partial sum
  f32x4_t o[NQ][NNB];
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    m[j] = NEG_BIG;
    l[j] = 0.f;
#pragma unroll
    for (int nb = 0; nb < NNB; ++nb) o[j][nb] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  }
  // LDS address of this lane's value fragments (column block nb, rows 8g + q of half 0) inside value image 0; the
  // half, the +4 rows of the second read and nothing else are immediates
  uint32_t voff[NNB];
  {
    constexpr int PC = HDPV / 8;
    const int q4 = (lane & 15) >> 2, p4 = lane & 3;
#pragma unroll
    for (int nb = 0; nb < NNB; ++nb) {
      const int c = ((2 * nb) + (p4 >> 1)) ^ mnswz<PC>(8 * g + q4);
      voff[nb] = (uint32_t)(uintptr_t)(lptr_t)smem + IMG + (8 * g + q4) * (HDPV * 2) + c * 16 + (p4 & 1) * 8;
    }
  }
  // transposed scores of the 64 keys of the tile in image pair `stage`: block (s, bb) holds keys 32 s + 8 g + 4 bb +
  // {0..3} of query qi
  auto qk_tile = [&](int stage, f32x4_t (&sc)[NQ][4], auto b0_c, auto b1_c) __attribute__((always_inline)) {
    const char* Kimg = smem + stage * PAIR;
#pragma unroll
    for (int blk = decltype(b0_c)::value; blk < decltype(b1_c)::value; ++blk) {
      const int row = 32 * (blk >> 1) + rowperm(blk & 1, r);
#pragma unroll
      for (int j = 0; j < NQ; ++j) sc[j][blk] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        const bf16x8_t kfr = kimg_frag<64>(Kimg, row, ks, lane);
#pragma unroll
        for (int j = 0; j < NQ; ++j) sc[j][blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfr, qf[j][ks], sc[j][blk], 0, 0, 0);
      }
    }
  };
  // softmax of the tile's scores (consumed) and the P V product into o
  // softmax of query block j of the tile's scores (consumed): probabilities as the packed A operands pf[j][0..1]
  auto soft_one = [&](auto full_c, int kt, f32x4_t (&sc)[NQ][4], auto j_c, bf16x8_t (&pf)[NQ][2]) __attribute__((always_inline)) {
    constexpr bool FULL = decltype(full_c)::value;
    constexpr int j = decltype(j_c)::value;
    {
      if constexpr (!FULL) {
#pragma unroll
        for (int blk = 0; blk < 4; ++blk)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int key = kt * 64 + 32 * (blk >> 1) + 8 * g + 4 * (blk & 1) + e;
            const bool ok = key < kl && (!a.causal || key <= qc[j]);
            sc[j][blk][e] = ok ? sc[j][blk][e] : NEG_BIG;
          }
      }
      float p[16];
      float alpha;
      float m_new;
      if constexpr (DROP) {
        // scores in log2 units first: the products are canonical values, so the maximum below compiles to plain
        // v_max3_f32 (fmaxf straight on MFMA outputs makes the compiler canonicalise every operand: v_max x, x), and a
        // probability is one subtraction and one v_exp_f32.  (A hand-written v_max3_f32 on the accumulators is not an
        // option: the hazard recogniser does not see inline asm, and the MFMA -> VALU read then returns stale registers.)
        float t[16];
#pragma unroll
        for (int blk = 0; blk < 4; ++blk)
#pragma unroll
          for (int e = 0; e < 4; ++e) t[4 * blk + e] = sc[j][blk][e] * c2;
        float tmax = fmaxf(fmaxf(t[0], t[1]), t[2]);
#pragma unroll
        for (int i = 3; i < 15; i += 2) tmax = fmaxf(fmaxf(tmax, t[i]), t[i + 1]);
        tmax = fmaxf(tmax, t[15]);
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        m_new = fmaxf(m[j], tmax);
        alpha = __builtin_amdgcn_exp2f(m[j] - m_new);
        float sum = 0.f;
#pragma unroll
        for (int blk = 0; blk < 4; ++blk)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float pv = __builtin_amdgcn_exp2f(t[4 * blk + e] - m_new);
            if constexpr (!FULL) pv = sc[j][blk][e] > 0.5f * NEG_BIG ? pv : 0.f;
            p[4 * blk + e] = pv;
            sum += pv;  // the normaliser is the sum of ALL probabilities: dropout acts on the normalised ones
          }
        const float ks = 1.f / (1.f - a.drop_p);
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) {
          const int key0 = kt * 64 + 32 * (blk >> 1) + 8 * g + 4 * (blk & 1);
          const unsigned keep = ca_dropout_keep4(a.drop_seed, attn_drop_index(a, b, h, qrow[j], key0), a.drop_p);
#pragma unroll
          for (int e = 0; e < 4; ++e) p[4 * blk + e] = ((keep >> e) & 1u) ? p[4 * blk + e] * ks : 0.f;
        }
        l[j] = fmaf(l[j], alpha, sum);
      } else {
        // The kernels are bound by vector-instruction issue (~250 per tile and wave against 32 MFMAs), so
        // the softmax is kept short: the maximum of the RAW scores (median of (x, y, +inf) = max without the
        // canonicalising move the compiler puts in front of fmaxf on MFMA outputs), scale and shift as ONE fma in front
        // of the exponential.  (The row sums as one more column of the P V product - P . 1 on the matrix pipe instead
        // of an addition per probability - were measured too: 4.5 % faster at T = 1500, but sums of bf16-rounded
        // probabilities took the 24-layer logits from 3.7e-2 to 5.2e-2 of the fp32 reference; the fp32 sums stay.)
        const float inf = __builtin_inff();
        float tmax = __builtin_amdgcn_fmed3f(sc[j][0][0], sc[j][0][1], inf);
#pragma unroll
        for (int i = 2; i < 16; ++i) tmax = __builtin_amdgcn_fmed3f(tmax, sc[j][i >> 2][i & 3], inf);
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        m_new = fmaxf(m[j], tmax * c2);
        alpha = __builtin_amdgcn_exp2f(m[j] - m_new);
        const float nm = -m_new;
        float sum = 0.f;
#pragma unroll
        for (int blk = 0; blk < 4; ++blk)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float pv = __builtin_amdgcn_exp2f(fmaf(sc[j][blk][e], c2, nm));
            if constexpr (!FULL) pv = sc[j][blk][e] > 0.5f * NEG_BIG ? pv : 0.f;
            p[4 * blk + e] = pv;
            sum += pv;
          }
        l[j] = fmaf(l[j], alpha, sum);
      }
      if (__builtin_amdgcn_ballot_w64(m_new > m[j]) != 0) {  // some query of this block moved its maximum
        float ar[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) ar[e] = __shfl(alpha, 4 * g + e, 64);
#pragma unroll
        for (int nb = 0; nb < NNB; ++nb)
#pragma unroll
          for (int e = 0; e < 4; ++e) o[j][nb][e] *= ar[e];
      }
      m[j] = m_new;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        float ps[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) ps[e] = p[8 * s + e];
        pf[j][s] = pack8(ps);
      }
    }
  };
  // the P V product of the tile in image pair `stage` into o
  auto pv_tile = [&](int stage, bf16x8_t (&pf)[NQ][2]) __attribute__((always_inline)) {
    // value fragments in batches of four column blocks; the next batch is in flight while the current one is used
    // (inline-asm reads: the builtin would be ordered behind the LDS-DMA of the tiles in flight)
    constexpr int NBATCH = 2 * NNB / 4, PITCH = HDPV * 2;
    const uint32_t sbase = (uint32_t)(stage * PAIR);
    bf16x8_t fa[4], fb[4];
    auto read_batch = [&](auto bt_c, bf16x8_t (&f)[4]) {
      constexpr int BT = decltype(bt_c)::value;
      constexpr int S = BT / (NNB / 4), NB0 = (BT % (NNB / 4)) * 4;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s16x4_t lo, hi;
        const uint32_t ad = voff[NB0 + i] + sbase;
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(lo) : "v"(ad), "n"(S * 32 * PITCH));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(hi) : "v"(ad), "n"(S * 32 * PITCH + 4 * PITCH));
        s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        f[i] = __builtin_bit_cast(bf16x8_t, v);
      }
    };
    auto step = [&](auto bt_c, bf16x8_t (&cur)[4], bf16x8_t (&nxt)[4]) {
      constexpr int BT = decltype(bt_c)::value;
      constexpr int S = BT / (NNB / 4), NB0 = (BT % (NNB / 4)) * 4;
      lds_wait_all();
#pragma unroll
      for (int i = 0; i < 4; ++i) tie(cur[i]);
      if constexpr (BT + 1 < NBATCH) read_batch(std::integral_constant<int, BT + 1>{}, nxt);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NQ; ++j)
          o[j][NB0 + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf[j][S], cur[i], o[j][NB0 + i], 0, 0, 0);
    };
    read_batch(std::integral_constant<int, 0>{}, fa);
    step(std::integral_constant<int, 0>{}, fa, fb);
    step(std::integral_constant<int, 1>{}, fb, fa);
    if constexpr (NBATCH > 2) {
      step(std::integral_constant<int, 2>{}, fa, fb);
      step(std::integral_constant<int, 3>{}, fb, fa);
    }
  };
  auto soft_pv = [&](auto full_c, int kt, int stage, f32x4_t (&sc)[NQ][4]) __attribute__((always_inline)) {
    bf16x8_t pf[NQ][2];
    soft_one(full_c, kt, sc, std::integral_constant<int, 0>{}, pf);
    soft_one(full_c, kt, sc, std::integral_constant<int, 1>{}, pf);
    static_assert(NQ == 2, "two query blocks per wave");
    pv_tile(stage, pf);
  };
  const int nfull = a.causal ? 0 : (kl / 64 < ntile ? kl / 64 : ntile);
  int stage = 0;
  {
    // tile kt lives in image pair kt % NST; tiles kt + 1 .. kt + NST - 2 stay in flight across the wait for tile kt, and
    // the request for tile kt + NST - 1 goes out right after the barrier that frees its pair (one barrier per tile)
    auto run = [&](auto full_c, int kt0, int kt1) __attribute__((always_inline)) {
      for (int kt = kt0; kt < kt1; ++kt) {
        const int ahead = ntile - 1 - kt;
        if (NST >= 4 && ahead >= 2)
          wait_vm<2 * DPT>();
        else if (NST >= 3 && ahead >= 1)
          wait_vm<DPT>();
        else
          wait_vm<0>();
        __syncthreads();
        if (kt + NST - 1 < ntile) issue(kt + NST - 1, stage == 0 ? NST - 1 : stage - 1);
        f32x4_t sc[NQ][4];
        qk_tile(stage, sc, IC<0>{}, IC<4>{});
        soft_pv(full_c, kt, stage, sc);
        stage = stage + 1 == NST ? 0 : stage + 1;
      }
    };
    run(std::true_type{}, 0, nfull);
    run(std::false_type{}, nfull, ntile);
  }
  __syncthreads();  // every wave is done with the images: the LDS becomes output staging
  unsigned short* O = a.O + b * a.sob + h * hd;
  unsigned char* O8 = a.O8 ? a.O8 + b * a.sob + h * hd : nullptr;
  const float s8 = a.O8 ? a.o8_scale[0] : 1.f;
  float amx = 0.f;
  char* st = smem + wave * (16 * (HDPV * 2 + 16));
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    // total of the four lane groups that share a query; lse in natural-log units for the backward
    float lt = l[j];
    lt += __shfl_xor(lt, 16, 64);
    lt += __shfl_xor(lt, 32, 64);
    const float lse = lt > 0.f ? (m[j] + __builtin_amdgcn_logf(lt)) * 0.69314718055994530942f : (KM ? 0.f : __builtin_inff());
    if (g == 0 && qi[j] < a.Tq && a.lse) a.lse[((int64_t)b * a.H + h) * a.Tqp + qi[j]] = lse;
    const float inv = lt > 0.f ? 1.0f / lt : 0.f;  // nothing attended -> zero output
    float ir[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) ir[e] = __shfl(inv, 4 * g + e, 64);
    if (j) __builtin_amdgcn_wave_barrier();
    store_tile16<HDPV>(st, o[j], ir, O, a.ldo, q0 + 16 * j, a.Tq, hd, lane, O8, s8, &amx);
  }
  if (a.O8 && a.o8_amax) {  // (every lane arrives; a maximum does not depend on the order)
    amx = wave_max(amx);
    if (lane == 0 && amx > 0.f) atomicMax(a.o8_amax + (blockIdx.x & (CA_FP8_AMAX_SLOTS - 1)), __float_as_uint(amx));
  }
}

// ---- launcher ---------------------------------------------------------------------------------------------------------
int attn_launch_fwd(const AttnPlan& p, const AttnArgs& a, hipStream_t s, const char* who) {
  switch (attn_inst(p)) {
    case attn_inst(ATTN_FWD, 64, 0): return attn_launch(attn_fwd_kernel<64, false>, p, s, who, a);
    case attn_inst(ATTN_FWD, 64, 1): return attn_launch(attn_fwd_kernel<64, true>, p, s, who, a);
    case attn_inst(ATTN_FWD, 128, 0): return attn_launch(attn_fwd_kernel<128, false>, p, s, who, a);
    case attn_inst(ATTN_FWD, 128, 1): return attn_launch(attn_fwd_kernel<128, true>, p, s, who, a);
    case attn_inst(ATTN_FWD_WIDE, 64, 0, 3): return attn_launch(attn_fwd_wide_kernel<64, false, 4, 2, 3>, p, s, who, a);
    case attn_inst(ATTN_FWD_WIDE, 64, 0, 2): return attn_launch(attn_fwd_wide_kernel<64, false, 4, 2, 2>, p, s, who, a);
    case attn_inst(ATTN_FWD_WIDE, 64, 1, 2): return attn_launch(attn_fwd_wide_kernel<64, true, 4, 2, 2>, p, s, who, a);
    case attn_inst(ATTN_FWD_WIDE, 128, 0, 2): return attn_launch(attn_fwd_wide_kernel<128, false, 4, 2, 2>, p, s, who, a);
    case attn_inst(ATTN_FWD_WIDE, 128, 1, 2): return attn_launch(attn_fwd_wide_kernel<128, true, 4, 2, 2>, p, s, who, a);
    // a per-row first key (CaAttnDesc.kstart): the causal decoder prefill, head_dim <= 64
    case attn_inst(ATTN_FWD, 64, 0, 0, 0, 0, 0, 1): return attn_launch(attn_fwd_kernel<64, false, true>, p, s, who, a);
    case attn_inst(ATTN_FWD_WIDE, 64, 0, 3, 0, 0, 0, 1): return attn_launch(attn_fwd_wide_kernel<64, false, 4, 2, 3, true>, p, s, who, a);
    case attn_inst(ATTN_FWD_WIDE, 64, 0, 2, 0, 0, 0, 1): return attn_launch(attn_fwd_wide_kernel<64, false, 4, 2, 2, true>, p, s, who, a);
  }
  return attn_no_kernel(p, who);
}
