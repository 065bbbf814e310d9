// Attention forward at a handful of queries per head (greedy decoding): the single-query kernel.  See attn_common.h.
#include "attn_common.h"
#include <atomic>
#include <stdlib.h>

// Greedy decoding (Tq <= 16 queries per head, hd <= 64): one workgroup per (clip, head), the four waves split the
// keys in tiles of 64 and merge their (m, l, O) at the end.  The kernel is bound by how many bytes a CU keeps in
// flight (one tile at a time per wave streamed 24 GB/s per CU: 16 us for the 1500 cross-attention keys), so each
// wave keeps THREE tiles in flight: the K fragments go straight from global memory into MFMA operand registers
// (a K row is an A-operand row: no LDS image), the V tile through a wave-private ring of three LDS images
// (LDS-DMA + transposed reads).  All vector-memory operations of the loop are inline asm in a fixed order (16 per
// tile), so the waits are counted by hand: vmcnt(32) leaves the two younger tiles in flight.
__device__ __forceinline__ bf16x8_t gload16_async(const void* p) {
  bf16x8_t v;
  asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(v) : "v"(p) : "memory");
  return v;
}
__device__ __forceinline__ void glds16_async(const void* g, char* lds_wave_base) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off"
               :
               : "v"(g), "s"((uint32_t)(uintptr_t)(lptr_t)lds_wave_base)
               : "memory", "m0");
}
// QP (ca_decode_attn_qproj, one query per clip): the wave-0..3 workgroup of (clip, head) first forms its own query -
// LayerNorm of the clip's residual row (the arithmetic of ln_fwd_kernel, chunk by chunk) and the 64 x d slice of the
// query projection (the arithmetic of ca_gemm_skinny_kernel: the four waves take a quarter of K each, one MFMA chain
// per 16 columns, partials added as (p0 + p1) + (p2 + p3), + bias, rounded to bf16) - so the LayerNorm launch, the
// projection launch and the query's trip through HBM disappear from the per-token chain; bit-identical to them.
#define SPLIT_ROW 66  // floats per query of a partial slab: m, l, 64 output columns
// DT: tiles in flight per wave = slots of its V ring.  3 (96 KiB of LDS: one workgroup per CU) where clips x heads is
// at most about two per CU; 2 (64 KiB: two workgroups per CU) for larger batches (round 5: an evaluation batch of 64
// clips x 16 heads is 1024 workgroups - with one per CU they ran in four rounds, each paying its LayerNorm + query
// projection prologue in front of its K|V stream; with two per CU one workgroup's prologue runs under the other's stream).
// KS (CaAttnDesc.key_slot, beam search): key / value t of query row b comes from cache row key_slot[b, t] instead of row b.
// The row's table is copied into LDS behind the V rings before the first tile is asked for, so the loop's address
// arithmetic gains one LDS read per row and its vector-memory sequence - and the counted waits - stay what they are.
// KM (CaAttnDesc.kstart): the row's keys start at kstart[b] - attn_kstart_shift in the prologue, nothing else changes.
template <int HDPV, bool QP = false, int DT = 3, bool KS = false, bool KM = false>
__global__ __launch_bounds__(256) void attn_fwd_smallq_kernel(const AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NKS = HDPV / 32, NNB = HDPV / 16;
  constexpr int IMG = 64 * HDPV * 2;
  constexpr int D = DT;  // tiles in flight per wave
  static_assert(D == 2 || D == 3, "two or three tiles in flight");
  static_assert(HDPV == 64, "16 vector-memory operations per tile are assumed by the counted waits");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, r = lane & 15;
  // Key split (a.nsplit > 1): nsplit workgroups per (clip, head) - with B x H below the CU count (8 clips x 16 heads on
  // 256 CUs) half the chip would idle while each workgroup streams its 384 KB of cross-attention K|V at what ONE CU takes
  // in.  The tiles are dealt to 4 x nsplit "waves"; each workgroup leaves its (m, l, O) partial in a slab and the last
  // one to arrive (one counter per clip and head; release / acquire at agent scope around it) merges them in slab order.
  int ns = 1, bh = blockIdx.x, sp = 0, part0 = blockIdx.x;
  if (a.nsplit > 1) ca_key_split_item(a.split, blockIdx.x, bh, sp, ns, part0);
  const int h = bh % a.H, b = bh / a.H;
  const int vw = sp * 4 + wave, nvw = 4 * ns;  // this wave's place among the waves that share the keys
  const int hd = a.hd;
  const unsigned short* Q = QP ? nullptr : a.Q + b * a.sqb + h * hd;
  const unsigned short* K = a.K + (KS ? 0 : b * a.skb) + h * hd;
  const unsigned short* V = a.V + (KS ? 0 : b * a.svb) + h * hd;
  char* Vring = smem + wave * D * IMG;
  const int qrow = r < a.Tq ? r : a.Tq - 1;
  int Tk = a.Tk, kl = a.Tk;
  if (a.klen) kl = a.klen[b] < kl ? a.klen[b] : kl;
  if constexpr (KM) attn_kstart_shift(a, b, K, V, Tk, kl);
  const int* slot = (const int*)(smem + 4 * D * IMG);  // KS: [Tk] cache rows of this query row's keys
  if constexpr (KS) {
    int* sw = (int*)(smem + 4 * D * IMG);
    for (int t = threadIdx.x; t < a.Tk; t += 256) {
      int sl = t < kl ? a.key_slot[(int64_t)b * a.Tk + t] : b;  // (keys past klen are loaded clamped and masked: own row)
      sl = sl < 0 ? 0 : (sl >= a.B ? a.B - 1 : sl);           // no table entry can take a load outside the cache
      sw[t] = sl;
    }
    __syncthreads();
  }
  bf16x8_t qf[NKS];
  if constexpr (QP) {
    const int C = a.qp_d, nchunk = C >> 3;
    unsigned short* xs = (unsigned short*)(smem + 4 * D * IMG);  // LayerNorm(x[b]) as bf16 [C <= 2048]
    float* qpart = (float*)(smem + 4 * D * IMG + 4096);          // [4 waves][64] partial dot products
    {  // every wave normalises the row (redundantly: no barrier before the statistics); wave 0 publishes it
      const unsigned short* xr = a.qp_x + (int64_t)b * a.qp_ldx;
      float v[4][8];
      float sx = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int ch = lane + c * 64;
        if (ch < nchunk) {
          const u16x8_t u = *(const u16x8_t*)(xr + ch * 8);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            v[c][e] = bf2f(u[e]);
            sx += v[c][e];
          }
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[c][e] = 0.f;
        }
      }
      const float mean = wave_sum(sx) / (float)C;
      float s2 = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int ch = lane + c * 64;
        if (ch < nchunk) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float dlt = v[c][e] - mean;
            s2 += dlt * dlt;
          }
        }
      }
      const float rstd = rsqrtf(wave_sum(s2) / (float)C + a.qp_eps);
      if (wave == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int ch = lane + c * 64;
          if (ch < nchunk) {
            const f32x4_t g0 = *(const f32x4_t*)(a.qp_gamma + ch * 8), g1 = *(const f32x4_t*)(a.qp_gamma + ch * 8 + 4);
            const f32x4_t b0 = *(const f32x4_t*)(a.qp_beta + ch * 8), b1 = *(const f32x4_t*)(a.qp_beta + ch * 8 + 4);
            u16x8_t o8;
#pragma unroll
            for (int e = 0; e < 8; ++e)
              o8[e] = f2bf(ln_apply(v[c][e], mean, rstd, e < 4 ? g0[e] : g1[e - 4], e < 4 ? b0[e] : b1[e - 4]));
            *(u16x8_t*)(xs + ch * 8) = o8;
          }
        }
      }
    }
    __syncthreads();
    // q[h*hd + n] for n < 64: A operand = the weight rows (16 per block), B operand = the normalised row in every lane
    // row; this wave's quarter of the K-steps, eight at a time, as in the weight-streaming GEMM
    const int ksteps = (C + 31) / 32, per = (ksteps + 3) / 4;
    const int ks0 = wave * per, ks1 = (ks0 + per < ksteps) ? ks0 + per : ksteps;
    const bf16x8_t zero8 = __builtin_bit_cast(bf16x8_t, (f32x4_t){0.f, 0.f, 0.f, 0.f});
    f32x4_t qa[NNB];
#pragma unroll
    for (int nb = 0; nb < NNB; ++nb) qa[nb] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    const unsigned short* wrow[NNB];
#pragma unroll
    for (int nb = 0; nb < NNB; ++nb) {
      const int n = 16 * nb + r;
      wrow[nb] = a.qp_W + (int64_t)(h * hd + (n < hd ? n : hd - 1)) * a.qp_ldw + 8 * g;
    }
    for (int ks = ks0; ks < ks1; ks += 8) {
      bf16x8_t wf[NNB][8], af[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int k = (ks + u) * 32 + 8 * g;
        const bool ok = ks + u < ks1 && k < C;
        af[u] = ok ? *(const bf16x8_t*)(xs + k) : zero8;
#pragma unroll
        for (int nb = 0; nb < NNB; ++nb) wf[nb][u] = ok ? *(const bf16x8_t*)(wrow[nb] + (int64_t)(ks + u) * 32) : zero8;
      }
#pragma unroll
      for (int nb = 0; nb < NNB; ++nb)
#pragma unroll
        for (int u = 0; u < 8; ++u) qa[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nb][u], af[u], qa[nb], 0, 0, 0);
    }
    if (r == 0) {
#pragma unroll
      for (int nb = 0; nb < NNB; ++nb)
#pragma unroll
        for (int e = 0; e < 4; ++e) qpart[wave * 64 + 16 * nb + 4 * g + e] = qa[nb][e];
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      float qv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int n = 32 * ks + 8 * g + j;
        float t = (qpart[n] + qpart[64 + n]) + (qpart[128 + n] + qpart[192 + n]);
        t = t * 1.0f + (n < hd ? a.qp_bias[h * hd + n] : 0.f);
        qv[j] = n < hd ? bf2f(f2bf(t)) : 0.f;  // (the bf16 the projection would have stored)
      }
      qf[ks] = pack8(qv);
    }
  } else {
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[ks] = load_rowfrag(Q, a.ldq, qrow, ks, lane, hd);
  }
  const int ntile = (kl + 63) / 64;
  const int nw = ntile > vw ? (ntile - vw + nvw - 1) / nvw : 0;  // this wave's tiles: kt = vw + nvw j
  const float c2 = a.scale * LOG2E;
  float m = NEG_BIG, l = 0.f;
  f32x4_t o[NNB];
#pragma unroll
  for (int nb = 0; nb < NNB; ++nb) o[nb] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // Q / klen have arrived: from here on the counts are the loop's
  bf16x8_t kf[D][4][NKS];
  // 8 K-fragment loads + 8 LDS-DMA pieces of V for tile j of this wave, into slot S
  auto issue = [&](auto slot_c, int j) {
    constexpr int S = decltype(slot_c)::value;
    const int kt = vw + nvw * j;
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) {
      int key = kt * 64 + 32 * (blk >> 1) + rowperm(blk & 1, r);
      key = key < Tk ? key : Tk - 1;  // clamped rows are masked below (key >= kl)
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        const int dim = 32 * ks + 8 * g;
        kf[S][blk][ks] = gload16_async(K + (KS ? (int64_t)slot[key] * a.skb : (int64_t)0) + (int64_t)key * a.ldk +
                                       (dim < hd ? dim : 0));
      }
    }
    constexpr int PC = HDPV / 8, RPI = 64 / PC;
    char* img = Vring + S * IMG;
#pragma unroll
    for (int i = 0; i < 64 * HDPV * 2 / 1024; ++i) {
      const int kr = i * RPI + lane / PC;
      const int c = (lane % PC) ^ mnswz<PC>(kr);
      const int dim = c * 8;
      const int row = kt * 64 + kr;
      const void* src = (row < Tk && dim < hd)
                            ? (const void*)(V + (KS ? (int64_t)slot[row] * a.svb : (int64_t)0) + (int64_t)row * a.ldv + dim)
                            : (const void*)g_attn_zero_page;
      glds16_async(src, img + i * 1024);
    }
  };
  auto step = [&](auto slot_c, int j) {
    constexpr int S = decltype(slot_c)::value;
    const int kt = vw + nvw * j;
    const int rem = nw - 1 - j;  // younger tiles already issued (at most D - 1)
    if (D > 2 && rem >= 2)
      asm volatile("s_waitcnt vmcnt(32)" ::: "memory");
    else if (rem >= 1)
      asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const char* Vimg = Vring + S * IMG;
    // the V fragments are asked for first: their LDS latency hides under the score MFMAs
    bf16x8_t vf[2][NNB];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int nb = 0; nb < NNB; ++nb) vf[s][nb] = timg_frag_async<HDPV>(Vimg, s, nb, lane);
    f32x4_t sc[4];
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) {
      f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        tie(kf[S][blk][ks]);
        if (32 * ks + 8 * g >= hd) kf[S][blk][ks] = __builtin_bit_cast(bf16x8_t, (f32x4_t){0.f, 0.f, 0.f, 0.f});
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[S][blk][ks], qf[ks], acc, 0, 0, 0);
      }
      sc[blk] = acc;
    }
    // (tiles wholly inside the valid keys: a body of their own without compare / select - a run-time flag inside the
    // element loops becomes control flow per element)
    auto rest = [&](auto full_c) __attribute__((always_inline)) {
    constexpr bool FULL = decltype(full_c)::value;
    if constexpr (!FULL) {
#pragma unroll
      for (int blk = 0; blk < 4; ++blk)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int key = kt * 64 + 32 * (blk >> 1) + 8 * g + 4 * (blk & 1) + e;
          sc[blk][e] = key < kl ? sc[blk][e] : NEG_BIG;
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
        if constexpr (!FULL) pv = sc[blk][e] > 0.5f * NEG_BIG ? pv : 0.f;
        p[4 * blk + e] = pv;
        sum += pv;  // the normaliser is the sum of ALL probabilities: dropout acts on the normalised ones
      }

    l = fmaf(l, alpha, sum);
    float ar[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) ar[e] = __shfl(alpha, 4 * g + e, 64);
#pragma unroll
    for (int nb = 0; nb < NNB; ++nb)
#pragma unroll
      for (int e = 0; e < 4; ++e) o[nb][e] *= ar[e];
    m = m_new;
    lds_wait_all();
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float ps[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) ps[e] = p[8 * s + e];
      const bf16x8_t pf = pack8(ps);
#pragma unroll
      for (int nb = 0; nb < NNB; ++nb) {
        tie(vf[s][nb]);
        o[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, vf[s][nb], o[nb], 0, 0, 0);
      }
    }
    };
    if (kt * 64 + 64 <= kl)
      rest(std::true_type{});
    else
      rest(std::false_type{});
    if (j + D < nw) issue(slot_c, j + D);  // slot S is free again: its registers and its LDS image have been consumed
  };
  if (nw > 0) issue(std::integral_constant<int, 0>{}, 0);
  if (nw > 1) issue(std::integral_constant<int, 1>{}, 1);
  if constexpr (D > 2) {
    if (nw > 2) issue(std::integral_constant<int, 2>{}, 2);
  }
  for (int j = 0; j < nw; j += D) {
    step(std::integral_constant<int, 0>{}, j);
    if (j + 1 < nw) step(std::integral_constant<int, 1>{}, j + 1);
    if constexpr (D > 2) {
      if (j + 2 < nw) step(std::integral_constant<int, 2>{}, j + 2);
    }
  }
  // merge the four waves: (m, l) per query and the output rows, through LDS (the images are dead now)
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  __syncthreads();
  float* cm = (float*)smem;              // [4][16]
  float* cl = cm + 64;                   // [4][16]
  float* co = cl + 64;                   // [4][16][HDPV]
  if (g == 0) {
    cm[wave * 16 + r] = m;
    cl[wave * 16 + r] = l;
  }
#pragma unroll
  for (int nb = 0; nb < NNB; ++nb)
#pragma unroll
    for (int e = 0; e < 4; ++e) co[(wave * 16 + 4 * g + e) * HDPV + 16 * nb + r] = o[nb][e];
  __syncthreads();
  if (wave != 0) return;
  unsigned short* O = a.O + b * a.sob + h * hd;
  if (ns > 1) {
    // this workgroup's partial: per query (m, l) and the unnormalised output row
    float* slab = a.split_slab + ((int64_t)part0 + sp) * (16 * SPLIT_ROW);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int q = 4 * g + e;
      float M = cm[q];
#pragma unroll
      for (int w = 1; w < 4; ++w) M = fmaxf(M, cm[w * 16 + q]);
      float L = 0.f, wgt[4];
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        wgt[w] = __builtin_amdgcn_exp2f(cm[w * 16 + q] - M);
        L = fmaf(cl[w * 16 + q], wgt[w], L);
      }
      if (q < a.Tq) {
        if (r == 0) {
          slab[q * SPLIT_ROW] = M;
          slab[q * SPLIT_ROW + 1] = L;
        }
#pragma unroll
        for (int nb = 0; nb < NNB; ++nb) {
          float v = 0.f;
#pragma unroll
          for (int w = 0; w < 4; ++w) v = fmaf(co[(w * 16 + q) * HDPV + 16 * nb + r], wgt[w], v);
          slab[q * SPLIT_ROW + 2 + 16 * nb + r] = v;
        }
      }
    }
    // publish (plain stores -> drained -> agent-scope release -> ticket); the workgroup that draws the last ticket
    // acquires and merges.  Nobody waits for anybody: no residency assumption.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    unsigned ticket = 0;
    if (lane == 0) ticket = __hip_atomic_fetch_add(a.split_cnt + bh, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ticket = __builtin_amdgcn_readfirstlane(ticket);
    if (ticket != (unsigned)(ns - 1)) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const float* base = a.split_slab + (int64_t)part0 * (16 * SPLIT_ROW);
    // lane = output column; every slab value of a query is asked for before the first is used (one round trip per
    // query - a decoded token has one query per clip - instead of one per slab and value)
    for (int q = 0; q < a.Tq; ++q) {
      float Mt[CA_ATTN_SPLIT_MAX], Lt[CA_ATTN_SPLIT_MAX], ot[CA_ATTN_SPLIT_MAX];
#pragma unroll
      for (int t = 0; t < CA_ATTN_SPLIT_MAX; ++t) {
        const float* row = base + ((t < ns ? t : 0) * 16 + q) * SPLIT_ROW;
        Mt[t] = row[0];
        Lt[t] = row[1];
        ot[t] = row[2 + lane];
      }
      float M = NEG_BIG;
#pragma unroll
      for (int t = 0; t < CA_ATTN_SPLIT_MAX; ++t) M = fmaxf(M, t < ns ? Mt[t] : NEG_BIG);
      float L = 0.f, v = 0.f;
#pragma unroll
      for (int t = 0; t < CA_ATTN_SPLIT_MAX; ++t) {
        const float wt = t < ns ? __builtin_amdgcn_exp2f(Mt[t] - M) : 0.f;
        L = fmaf(Lt[t], wt, L);
        v = fmaf(ot[t], wt, v);
      }
      const float inv = L > 0.f ? 1.0f / L : 0.f;
      if (lane < hd) O[(int64_t)q * a.ldo + lane] = f2bf(v * inv);
      if (lane == 0 && a.lse)
        a.lse[((int64_t)b * a.H + h) * a.Tqp + q] = L > 0.f ? (M + __builtin_amdgcn_logf(L)) * 0.69314718055994530942f
                                                            : __builtin_inff();
    }
    if (lane == 0) __hip_atomic_store(a.split_cnt + bh, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // for the next launch
    return;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int q = 4 * g + e;
    float M = cm[q];
#pragma unroll
    for (int w = 1; w < 4; ++w) M = fmaxf(M, cm[w * 16 + q]);
    float L = 0.f, wgt[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      wgt[w] = __builtin_amdgcn_exp2f(cm[w * 16 + q] - M);
      L = fmaf(cl[w * 16 + q], wgt[w], L);
    }
    const float inv = L > 0.f ? 1.0f / L : 0.f;
    if (q < a.Tq) {
#pragma unroll
      for (int nb = 0; nb < NNB; ++nb) {
        const int n = 16 * nb + r;
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) v = fmaf(co[(w * 16 + q) * HDPV + n], wgt[w], v);
        if (n < hd) O[(int64_t)q * a.ldo + n] = f2bf(v * inv);
      }
      if (r == 0 && a.lse)  // (KM: a row whose first key lies behind its last writes nothing that is not finite)
        a.lse[((int64_t)b * a.H + h) * a.Tqp + q] = L > 0.f ? (M + __builtin_amdgcn_logf(L)) * 0.69314718055994530942f
                                                            : (KM ? 0.f : __builtin_inff());
    }
  }
}

// ---- launcher ---------------------------------------------------------------------------------------------------------
// The rings need more dynamic LDS than a kernel may ask for by default: the limit is raised to the instantiation's
// largest launch (the longest key_slot table) once per device.
template <bool QP, int DT, bool KS, bool KM = false>
static int smallq_launch(const AttnPlan& p, const AttnArgs& a, hipStream_t s, const char* who) {
  static std::atomic<uint64_t> raised{0};  // one bit per device
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  const uint64_t bit = dev < 64 ? uint64_t(1) << dev : 0;  // (devices beyond the mask: every launch)
  if (!(raised.load(std::memory_order_relaxed) & bit)) {
    const hipError_t e = hipFuncSetAttribute((const void*)attn_fwd_smallq_kernel<64, QP, DT, KS, KM>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)attn_smallq_lds(DT, QP, KS ? ATTN_KEY_SLOT_MAX_KEYS * 4 : 0));
    if (e != hipSuccess) {
      ca_set_error("%s: cannot raise the single-query kernel's LDS limit: %s", who, hipGetErrorString(e));
      return CA_ERR_LAUNCH;
    }
    raised.fetch_or(bit, std::memory_order_relaxed);
  }
  return attn_launch(attn_fwd_smallq_kernel<64, QP, DT, KS, KM>, p, s, who, a);
}
int attn_launch_decode(const AttnPlan& p, const AttnArgs& a, hipStream_t s, const char* who) {
  switch (attn_inst(p)) {
    case attn_inst(ATTN_FWD_SMALLQ, 64, 0, 0, 3, 0, 0): return smallq_launch<false, 3, false>(p, a, s, who);
    case attn_inst(ATTN_FWD_SMALLQ, 64, 0, 0, 2, 0, 0): return smallq_launch<false, 2, false>(p, a, s, who);
    case attn_inst(ATTN_FWD_SMALLQ, 64, 0, 0, 3, 0, 1): return smallq_launch<false, 3, true>(p, a, s, who);
    case attn_inst(ATTN_FWD_SMALLQ, 64, 0, 0, 2, 0, 1): return smallq_launch<false, 2, true>(p, a, s, who);
    // (non-temporal loads of the K|V stream measured slower here: 8 491 -> 8 307 audio-s/s at 128 clips, round 5)
    case attn_inst(ATTN_FWD_SMALLQ, 64, 0, 0, 3, 1, 0): return smallq_launch<true, 3, false>(p, a, s, who);
    case attn_inst(ATTN_FWD_SMALLQ, 64, 0, 0, 2, 1, 0): return smallq_launch<true, 2, false>(p, a, s, who);
    // a per-row first key (CaAttnDesc.kstart): the decoder self-attention of a left-padded batch of prompts
    case attn_inst(ATTN_FWD_SMALLQ, 64, 0, 0, 3, 0, 0, 1): return smallq_launch<false, 3, false, true>(p, a, s, who);
    case attn_inst(ATTN_FWD_SMALLQ, 64, 0, 0, 2, 0, 0, 1): return smallq_launch<false, 2, false, true>(p, a, s, who);
  }
  return attn_no_kernel(p, who);
}

// The attention knobs of the environment and the device's CU count, read once (AttnKnobs in attn_plan.h; tools/ENV.md).
const AttnKnobs& attn_knobs() {
  static const AttnKnobs knobs = [] {
    AttnKnobs k;
    auto env = [](const char* name, int dflt) {
      const char* e = getenv(name);
      return e ? atoi(e) : dflt;
    };
    k.wide = env("CA_ATTN_WIDE", k.wide);
    k.wpe3 = env("CA_ATTN_WPE3", k.wpe3);
    k.dq_wpe3 = env("CA_ATTN_DQ_WPE3", k.dq_wpe3);
    k.dkv_wide = env("CA_ATTN_DKV_WIDE", k.dkv_wide);
    k.dkv_wpe3 = env("CA_ATTN_DKV_WPE3", k.dkv_wpe3);
    const int two = env("CA_SMALLQ_2PERCU", 0);
    if (getenv("CA_SMALLQ_2PERCU")) k.smallq_2percu = two > 0 ? two : 0;  // (set to nothing positive: never)
    k.split = env("CA_ATTN_SPLIT", k.split);
    k.split_tail = env("CA_ATTN_SPLIT_TAIL", k.split_tail);
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess) hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    if (n > 0) k.device_cus = n;
    return k;
  }();
  return knobs;
}
