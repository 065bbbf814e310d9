// Attention backward: D = rowsum(dO * O), dK|dV and dQ, each also with wide workgroups.  See attn_common.h.
#include "attn_common.h"

// ---- backward: D = rowsum(dO * O) ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void attn_bwd_prep_kernel(const unsigned short* __restrict__ dO, int64_t lddo,
                                                            int64_t sdob, const unsigned short* __restrict__ O,
                                                            int64_t ldo, int64_t sob, float* __restrict__ Dq, int H,
                                                            int Tq, int Tqp, int hd, int B,
                                                            const int32_t* __restrict__ row_off) {
  // one 16-lane group per (b, h, q)
  const int64_t gid = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
  const int sub = threadIdx.x & 15;
  const int64_t total = (int64_t)B * H * Tq;
  if (gid >= total) return;
  const int q = (int)(gid % Tq);
  const int h = (int)((gid / Tq) % H);
  const int b = (int)(gid / ((int64_t)Tq * H));
  if (row_off) {  // packed rows (attn_packed_rows): utterance b starts at row row_off[b]; Dq stays indexed by (b, h, q)
    const int64_t r0 = row_off[b];
    if (q >= row_off[b + 1] - (int)r0) return;
    dO += r0 * lddo - b * sdob;
    O += r0 * ldo - b * sob;
  }
  const unsigned short* x = dO + b * sdob + (int64_t)q * lddo + h * hd;
  const unsigned short* y = O + b * sob + (int64_t)q * ldo + h * hd;
  float s = 0.f;
  for (int c = sub * 8; c < hd; c += 128) {
    const u16x8_t u = *(const u16x8_t*)(x + c), v = *(const u16x8_t*)(y + c);
#pragma unroll
    for (int e = 0; e < 8; ++e) s += bf2f(u[e]) * bf2f(v[e]);
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (sub == 0) Dq[((int64_t)b * H + h) * Tqp + q] = s;
}

// ---- backward: dK, dV (workgroup = 64 keys, loops over the queries) ------------------------------------
template <int HDPV, bool DROP = false>
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NKS = HDPV / 32, NNB = HDPV / 16;
  constexpr int IMG = 32 * HDPV * 2;
  char* Qk = smem;         // K-major image of the 32-query tile: S = Q K^T, and (read transposed) dK += dS^T Q
  char* dOk = smem + IMG;  // K-major image of dO:                dP = dO V^T, and (read transposed) dV += P^T dO
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, r = lane & 15;
  int tile, h, b;
  if (!attn_tile_of_block((a.Tk + 63) / 64, a.H, a.B, tile, h, b)) return;
  attn_packed_rows(a, b);
  if (tile * (64) >= a.Tk) return;  // (packed rows: the tile lies past the utterance)
  const int hd = a.hd;
  const unsigned short* Q = a.Q + b * a.sqb + h * hd;
  const unsigned short* K = a.K + b * a.skb + h * hd;
  const unsigned short* V = a.V + b * a.svb + h * hd;
  const unsigned short* dO = a.dO + b * a.sdob + h * hd;
  const float* lse = a.lse + ((int64_t)b * a.H + h) * a.Tqp;
  const float* Dq = a.Dq + ((int64_t)b * a.H + h) * a.Tqp;
  const int k0 = tile * 64 + wave * 16;
  const int key = k0 + r;  // this lane's key (column of the score tile)
  const int krow = key < a.Tk ? key : a.Tk - 1;
  int kl = a.Tk;
  if (a.klen) kl = a.klen[b] < kl ? a.klen[b] : kl;
  // all HDPV/32 k-steps and HDPV/16 column blocks are computed: dims >= hd are zero in every LDS image
  bf16x8_t kf[NKS], vf[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    kf[ks] = load_rowfrag(K, a.ldk, krow, ks, lane, hd);
    vf[ks] = load_rowfrag(V, a.ldv, krow, ks, lane, hd);
  }
  f32x4_t dk[NNB], dv[NNB];
#pragma unroll
  for (int nb = 0; nb < NNB; ++nb) dk[nb] = dv[nb] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  const float scale = a.scale;
  const float c2 = scale * LOG2E;
  const bool full_keys = (tile * 64 + 64 <= kl) && !a.causal;
  const int nstep = (a.Tq + 31) / 32;
  const int s0 = a.causal ? (tile * 64) / 32 : 0;  // queries before the tile's first key see none of it
  // Double-buffered: the images and the per-query statistics of step qs+1 are requested right after the barrier
  // of step qs (one barrier per step: every wave has finished reading the other buffer when it arrives).
  KImgFast<32, HDPV> qfast, dofast;
  qfast.init(a.ldq, wave, lane);
  dofast.init(a.lddo, wave, lane);
  const int nfast = fast_tiles(a.Tq, 32);
  auto issue = [&](int qs, int buf) {
    if (qs < nfast) {
      qfast.issue(Qk + buf * 2 * IMG, Q + (int64_t)qs * 32 * a.ldq, wave);
      dofast.issue(dOk + buf * 2 * IMG, dO + (int64_t)qs * 32 * a.lddo, wave);
    } else {
      load_kmajor_image<32, HDPV>(Qk + buf * 2 * IMG, Q, a.ldq, qs * 32, a.Tq, hd, wave, lane);
      load_kmajor_image<32, HDPV>(dOk + buf * 2 * IMG, dO, a.lddo, qs * 32, a.Tq, hd, wave, lane);
    }
  };
  f32x4_t l0, l1, d0, d1;  // statistics of the current step: indices 8g .. 8g+7 are contiguous
  if (s0 < nstep) {
    issue(s0, 0);
    l0 = *(const f32x4_t*)(lse + s0 * 32 + 8 * g);
    l1 = *(const f32x4_t*)(lse + s0 * 32 + 8 * g + 4);
    d0 = *(const f32x4_t*)(Dq + s0 * 32 + 8 * g);
    d1 = *(const f32x4_t*)(Dq + s0 * 32 + 8 * g + 4);
  }
  // One 32-query step; FULL (compile time): nothing in the step is masked - no per-element compare / select.  As a
  // run-time flag inside the element loop the masks became ~30 small basic blocks per step: in-kernel stamps put the
  // softmax / dS section at 1 630 cycles of a 3 430-cycle step (tools/archive/dev_dkv_stamps.py), against 553 + 655 for the 32 MFMAs.
  auto step = [&](auto full_c, int qs) __attribute__((always_inline)) {
    constexpr bool FULL = decltype(full_c)::value;
    const int buf = (qs - s0) & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    f32x4_t nl0 = l0, nl1 = l1, nd0 = d0, nd1 = d1;
    if (qs + 1 < nstep) {
      issue(qs + 1, buf ^ 1);
      nl0 = *(const f32x4_t*)(lse + (qs + 1) * 32 + 8 * g);
      nl1 = *(const f32x4_t*)(lse + (qs + 1) * 32 + 8 * g + 4);
      nd0 = *(const f32x4_t*)(Dq + (qs + 1) * 32 + 8 * g);
      nd1 = *(const f32x4_t*)(Dq + (qs + 1) * 32 + 8 * g + 4);
    }
    const char* Qi = Qk + buf * 2 * IMG;
    const char* dOi = dOk + buf * 2 * IMG;
    f32x4_t sacc[2], pacc[2];
#pragma unroll
    for (int bb = 0; bb < 2; ++bb) {
      sacc[bb] = pacc[bb] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
      const int row = rowperm(bb, r);
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        sacc[bb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kimg_frag<32>(Qi, row, ks, lane), kf[ks], sacc[bb], 0, 0, 0);
        pacc[bb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kimg_frag<32>(dOi, row, ks, lane), vf[ks], pacc[bb], 0, 0, 0);
      }
    }
    // transposed fragments of the first half of the columns fly while the softmax arithmetic runs
    constexpr int HB = NNB / 2;
    bf16x8_t fo[HB], fq[HB];
#pragma unroll
    for (int i = 0; i < HB; ++i) {
      fo[i] = timg_frag_k_async<32>(dOi, 0, i, lane);
      fq[i] = timg_frag_k_async<32>(Qi, 0, i, lane);
    }
    float p[8], ds[8];
#pragma unroll
    for (int bb = 0; bb < 2; ++bb)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float ls2 = (bb == 0 ? l0[e] : l1[e]) * LOG2E;
        const float dq = bb == 0 ? d0[e] : d1[e];
        float pv = __builtin_amdgcn_exp2f(fmaf(sacc[bb][e], c2, -ls2));
        float dpv = pacc[bb][e];  // d/dP of the (dropped) probabilities
        float pdrop = pv;         // the probability as the forward used it against V
        if constexpr (DROP) {
          const int qd = qs * 32 + 8 * g + 4 * bb + e;
          const bool keep = ca_dropout_keep(a.drop_seed, attn_drop_index(a, b, h, qd < a.Tq ? qd : a.Tq - 1, krow), a.drop_p);
          const float ks = 1.f / (1.f - a.drop_p);
          dpv = keep ? dpv * ks : 0.f;
          pdrop = keep ? pv * ks : 0.f;
        }
        float dsv = pv * (dpv - dq);  // (x scale: once, when dK is stored)
        pv = pdrop;
        if constexpr (!FULL) {  // statistics of padded queries are not initialised: select, never multiply by a mask
          const int qi = qs * 32 + 8 * g + 4 * bb + e;
          const bool ok = qi < a.Tq && key < kl && (!a.causal || key <= qi);
          pv = ok ? pv : 0.f;
          dsv = ok ? dsv : 0.f;
        }
        p[4 * bb + e] = pv;
        ds[4 * bb + e] = dsv;
      }
    const bf16x8_t pf = pack8(p), dsf = pack8(ds);
    lds_wait_all();
#pragma unroll
    for (int i = 0; i < HB; ++i) {
      tie(fo[i]);
      tie(fq[i]);
    }
    bf16x8_t go[HB], gq[HB];
#pragma unroll
    for (int i = 0; i < HB; ++i) {
      go[i] = timg_frag_k_async<32>(dOi, 0, HB + i, lane);
      gq[i] = timg_frag_k_async<32>(Qi, 0, HB + i, lane);
    }
#pragma unroll
    for (int i = 0; i < HB; ++i) {
      dv[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, fo[i], dv[i], 0, 0, 0);
      dk[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsf, fq[i], dk[i], 0, 0, 0);
    }
    lds_wait_all();
#pragma unroll
    for (int i = 0; i < HB; ++i) {
      tie(go[i]);
      tie(gq[i]);
    }
#pragma unroll
    for (int i = 0; i < HB; ++i) {
      dv[HB + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, go[i], dv[HB + i], 0, 0, 0);
      dk[HB + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsf, gq[i], dk[HB + i], 0, 0, 0);
    }
    l0 = nl0;
    l1 = nl1;
    d0 = nd0;
    d1 = nd1;
  };
  int nfull = full_keys ? a.Tq / 32 : s0;  // steps [s0, nfull) see whole 32-query blocks of valid queries and keys
  nfull = nfull < s0 ? s0 : nfull;
  for (int qs = s0; qs < nfull; ++qs) step(std::true_type{}, qs);
  for (int qs = nfull; qs < nstep; ++qs) step(std::false_type{}, qs);
  unsigned short* dK = a.dK + b * a.sdkb + h * hd;
  unsigned short* dV = a.dV + b * a.sdvb + h * hd;
  __syncthreads();  // the last step's image reads are done in every wave: the LDS becomes output staging
  const float one[4] = {1.f, 1.f, 1.f, 1.f};
  char* st = smem + wave * (attn_stage_bytes(HDPV) / 4);
  const float sc4[4] = {scale, scale, scale, scale};  // dS was formed without the softmax scale
  store_tile16<HDPV>(st, dk, sc4, dK, a.lddk, k0, a.Tk, hd, lane);
  __builtin_amdgcn_wave_barrier();
  store_tile16<HDPV>(st, dv, one, dV, a.lddv, k0, a.Tk, hd, lane);
}

// ---- backward: dK, dV, wide waves (workgroup = 4 waves x KB key blocks of 16 = 64 * KB keys) --------------------------
// In the kernel above a wave owns 16 keys, so every Q / dO fragment it reads from LDS feeds ONE MFMA: 80 LDS read
// instructions (48 KiB, the transposed ones with a 2-way bank conflict) per 32 MFMAs and 32-query step - at four
// workgroups per CU the LDS, not the matrix pipe, sets the pace (768 LDS cycles against 512 MFMA cycles per step).
// Here a wave owns KB = 2 key blocks: each fragment feeds two MFMAs, a workgroup covers 128 keys, half as many
// workgroups stream the same Q / dO images.
template <int HDPV, bool DROP, int KB, int WPE = 2>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void attn_bwd_dkv_wide_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NKS = HDPV / 32, NNB = HDPV / 16;
  constexpr int IMG = 32 * HDPV * 2;
  char* Qk = smem;         // K-major image of the 32-query tile: S = Q K^T, and (read transposed) dK += dS^T Q
  char* dOk = smem + IMG;  // K-major image of dO:                dP = dO V^T, and (read transposed) dV += P^T dO
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, r = lane & 15;
  int tile, h, b;
  if (!attn_tile_of_block((a.Tk + 64 * KB - 1) / (64 * KB), a.H, a.B, tile, h, b)) return;
  attn_packed_rows(a, b);
  if (tile * (64 * KB) >= a.Tk) return;  // (packed rows: the tile lies past the utterance)
  const int hd = a.hd;
  const unsigned short* Q = a.Q + b * a.sqb + h * hd;
  const unsigned short* K = a.K + b * a.skb + h * hd;
  const unsigned short* V = a.V + b * a.svb + h * hd;
  const unsigned short* dO = a.dO + b * a.sdob + h * hd;
  const float* lse = a.lse + ((int64_t)b * a.H + h) * a.Tqp;
  const float* Dq = a.Dq + ((int64_t)b * a.H + h) * a.Tqp;
  const int k0 = tile * 64 * KB + wave * 16 * KB;  // block kb: keys k0 + 16 kb + r
  int kl = a.Tk;
  if (a.klen) kl = a.klen[b] < kl ? a.klen[b] : kl;
  // all HDPV/32 k-steps and HDPV/16 column blocks are computed: dims >= hd are zero in every LDS image
  bf16x8_t kf[KB][NKS], vf[KB][NKS];
  f32x4_t dk[KB][NNB], dv[KB][NNB];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    const int key = k0 + 16 * kb + r;
    const int krow = key < a.Tk ? key : a.Tk - 1;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      kf[kb][ks] = load_rowfrag(K, a.ldk, krow, ks, lane, hd);
      vf[kb][ks] = load_rowfrag(V, a.ldv, krow, ks, lane, hd);
    }
#pragma unroll
    for (int nb = 0; nb < NNB; ++nb) dk[kb][nb] = dv[kb][nb] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  }
  const float scale = a.scale;
  const float c2 = scale * LOG2E;
  const bool full_keys = (tile * 64 * KB + 64 * KB <= kl) && !a.causal;
  const int nstep = (a.Tq + 31) / 32;
  const int s0 = a.causal ? (tile * 64 * KB) / 32 : 0;  // queries before the tile's first key see none of it
  // Double-buffered: the images and the per-query statistics of step qs+1 are requested right after the barrier
  // of step qs (one barrier per step: every wave has finished reading the other buffer when it arrives).
  KImgFast<32, HDPV> qfast, dofast;
  qfast.init(a.ldq, wave, lane);
  dofast.init(a.lddo, wave, lane);
  const int nfast = fast_tiles(a.Tq, 32);
  auto issue = [&](int qs, int buf) {
    if (qs < nfast) {
      qfast.issue(Qk + buf * 2 * IMG, Q + (int64_t)qs * 32 * a.ldq, wave);
      dofast.issue(dOk + buf * 2 * IMG, dO + (int64_t)qs * 32 * a.lddo, wave);
    } else {
      load_kmajor_image<32, HDPV>(Qk + buf * 2 * IMG, Q, a.ldq, qs * 32, a.Tq, hd, wave, lane);
      load_kmajor_image<32, HDPV>(dOk + buf * 2 * IMG, dO, a.lddo, qs * 32, a.Tq, hd, wave, lane);
    }
  };
  f32x4_t l0, l1, d0, d1;  // statistics of the current step: indices 8g .. 8g+7 are contiguous
  if (s0 < nstep) {
    issue(s0, 0);
    l0 = *(const f32x4_t*)(lse + s0 * 32 + 8 * g);
    l1 = *(const f32x4_t*)(lse + s0 * 32 + 8 * g + 4);
    d0 = *(const f32x4_t*)(Dq + s0 * 32 + 8 * g);
    d1 = *(const f32x4_t*)(Dq + s0 * 32 + 8 * g + 4);
  }
  // One 32-query step; FULL (compile time): nothing in the step is masked - no per-element compare / select.  As a
  // run-time flag inside the element loop the masks became ~30 small basic blocks per step: in-kernel stamps put the
  // softmax / dS section at 1 630 cycles of a 3 430-cycle step (tools/archive/dev_dkv_stamps.py), against 553 + 655 for the 32 MFMAs.
  auto step = [&](auto full_c, int qs) __attribute__((always_inline)) {
    constexpr bool FULL = decltype(full_c)::value;
    const int buf = (qs - s0) & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (qs + 1 < nstep) issue(qs + 1, buf ^ 1);
    // (this step's statistics: asked for here, used behind the S | dP products - no second set of registers for the next step's)
    l0 = *(const f32x4_t*)(lse + qs * 32 + 8 * g);
    l1 = *(const f32x4_t*)(lse + qs * 32 + 8 * g + 4);
    d0 = *(const f32x4_t*)(Dq + qs * 32 + 8 * g);
    d1 = *(const f32x4_t*)(Dq + qs * 32 + 8 * g + 4);
    const char* Qi = Qk + buf * 2 * IMG;
    const char* dOi = dOk + buf * 2 * IMG;
    f32x4_t sacc[KB][2], pacc[KB][2];
#pragma unroll
    for (int bb = 0; bb < 2; ++bb) {
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) sacc[kb][bb] = pacc[kb][bb] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
      const int row = rowperm(bb, r);
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        const bf16x8_t qf = kimg_frag<32>(Qi, row, ks, lane), dof = kimg_frag<32>(dOi, row, ks, lane);
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {  // one fragment read, KB MFMAs
          sacc[kb][bb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf, kf[kb][ks], sacc[kb][bb], 0, 0, 0);
          pacc[kb][bb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dof, vf[kb][ks], pacc[kb][bb], 0, 0, 0);
        }
      }
    }
    // transposed fragments of the first half of the columns fly while the softmax arithmetic runs
    constexpr int HB = NNB / 2;
    bf16x8_t fo[HB], fq[HB];
#pragma unroll
    for (int i = 0; i < HB; ++i) {
      fo[i] = timg_frag_k_async<32>(dOi, 0, i, lane);
      fq[i] = timg_frag_k_async<32>(Qi, 0, i, lane);
    }
    bf16x8_t pf[KB], dsf[KB];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      const int key = k0 + 16 * kb + r;
      const int krow = key < a.Tk ? key : a.Tk - 1;
      float p[8], ds[8];
#pragma unroll
      for (int bb = 0; bb < 2; ++bb)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float ls2 = (bb == 0 ? l0[e] : l1[e]) * LOG2E;
          const float dq = bb == 0 ? d0[e] : d1[e];
          float pv = __builtin_amdgcn_exp2f(fmaf(sacc[kb][bb][e], c2, -ls2));
          float dpv = pacc[kb][bb][e];  // d/dP of the (dropped) probabilities
          float pdrop = pv;             // the probability as the forward used it against V
          if constexpr (DROP) {
            const int qd = qs * 32 + 8 * g + 4 * bb + e;
            const bool keep = ca_dropout_keep(a.drop_seed, attn_drop_index(a, b, h, qd < a.Tq ? qd : a.Tq - 1, krow), a.drop_p);
            const float ks = 1.f / (1.f - a.drop_p);
            dpv = keep ? dpv * ks : 0.f;
            pdrop = keep ? pv * ks : 0.f;
          }
          float dsv = pv * (dpv - dq);  // (x scale: once, when dK is stored)
          pv = pdrop;
          if constexpr (!FULL) {  // statistics of padded queries are not initialised: select, never multiply by a mask
            const int qi = qs * 32 + 8 * g + 4 * bb + e;
            const bool ok = qi < a.Tq && key < kl && (!a.causal || key <= qi);
            pv = ok ? pv : 0.f;
            dsv = ok ? dsv : 0.f;
          }
          p[4 * bb + e] = pv;
          ds[4 * bb + e] = dsv;
        }
      pf[kb] = pack8(p);
      dsf[kb] = pack8(ds);
    }
    lds_wait_all();
#pragma unroll
    for (int i = 0; i < HB; ++i) {
      tie(fo[i]);
      tie(fq[i]);
    }
    bf16x8_t go[HB], gq[HB];
#pragma unroll
    for (int i = 0; i < HB; ++i) {
      go[i] = timg_frag_k_async<32>(dOi, 0, HB + i, lane);
      gq[i] = timg_frag_k_async<32>(Qi, 0, HB + i, lane);
    }
#pragma unroll
    for (int i = 0; i < HB; ++i)
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        dv[kb][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf[kb], fo[i], dv[kb][i], 0, 0, 0);
        dk[kb][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsf[kb], fq[i], dk[kb][i], 0, 0, 0);
      }
    lds_wait_all();
#pragma unroll
    for (int i = 0; i < HB; ++i) {
      tie(go[i]);
      tie(gq[i]);
    }
#pragma unroll
    for (int i = 0; i < HB; ++i)
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        dv[kb][HB + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf[kb], go[i], dv[kb][HB + i], 0, 0, 0);
        dk[kb][HB + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsf[kb], gq[i], dk[kb][HB + i], 0, 0, 0);
      }
  };
  int nfull = full_keys ? a.Tq / 32 : s0;  // steps [s0, nfull) see whole 32-query blocks of valid queries and keys
  nfull = nfull < s0 ? s0 : nfull;
  for (int qs = s0; qs < nfull; ++qs) step(std::true_type{}, qs);
  for (int qs = nfull; qs < nstep; ++qs) step(std::false_type{}, qs);
  unsigned short* dK = a.dK + b * a.sdkb + h * hd;
  unsigned short* dV = a.dV + b * a.sdvb + h * hd;
  __syncthreads();  // the last step's image reads are done in every wave: the LDS becomes output staging
  const float one[4] = {1.f, 1.f, 1.f, 1.f};
  const float sc4[4] = {scale, scale, scale, scale};  // dS was formed without the softmax scale
  char* st = smem + wave * (attn_stage_bytes(HDPV) / 4);
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    store_tile16<HDPV>(st, dk[kb], sc4, dK, a.lddk, k0 + 16 * kb, a.Tk, hd, lane);
    __builtin_amdgcn_wave_barrier();
    store_tile16<HDPV>(st, dv[kb], one, dV, a.lddv, k0 + 16 * kb, a.Tk, hd, lane);
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- backward: dQ (workgroup = 64 queries, loops over the keys) ------------------------------------------
template <int HDPV, bool DROP = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void attn_bwd_dq_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NKS = HDPV / 32, NNB = HDPV / 16;
  constexpr int IMG = 64 * HDPV * 2;
  char* Kk = smem;        // K-major image of the key tile: S^T = K Q^T, and (read transposed) dQ += dS K
  char* Vk = smem + IMG;  // K-major image of V:            dP^T = V dO^T
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
  const unsigned short* dO = a.dO + b * a.sdob + h * hd;
  const int q0 = tile * 64 + wave * 16;
  const int qi = q0 + r;
  const int qrow = qi < a.Tq ? qi : a.Tq - 1;
  int kl = a.Tk;
  if (a.klen) kl = a.klen[b] < kl ? a.klen[b] : kl;
  // all HDPV/32 k-steps and HDPV/16 column blocks are computed: dims >= hd are zero in every LDS image
  bf16x8_t qf[NKS], dof[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    qf[ks] = load_rowfrag(Q, a.ldq, qrow, ks, lane, hd);
    dof[ks] = load_rowfrag(dO, a.lddo, qrow, ks, lane, hd);
  }
  const float lse2 = a.lse[((int64_t)b * a.H + h) * a.Tqp + qrow] * LOG2E;
  const float dq_row = a.Dq[((int64_t)b * a.H + h) * a.Tqp + qrow];
  f32x4_t acc[NNB];
#pragma unroll
  for (int nb = 0; nb < NNB; ++nb) acc[nb] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  const float scale = a.scale;
  const float c2 = scale * LOG2E;
  int ntile = (kl + 63) / 64;
  if (a.causal) {
    const int last = (tile * 64 + 63) / 64 + 1;  // keys beyond the tile's last query are masked
    ntile = ntile < last ? ntile : last;
  }
  KImgFast<64, HDPV> kfast, vfast;
  kfast.init(a.ldk, wave, lane);
  vfast.init(a.ldv, wave, lane);
  const int nfast = fast_tiles(a.Tk, 64);
  for (int kt = 0; kt < ntile; ++kt) {
    if (kt < nfast) {
      kfast.issue(Kk, K + (int64_t)kt * 64 * a.ldk, wave);
      vfast.issue(Vk, V + (int64_t)kt * 64 * a.ldv, wave);
    } else {
      load_kmajor_image<64, HDPV>(Kk, K, a.ldk, kt * 64, a.Tk, hd, wave, lane);
      load_kmajor_image<64, HDPV>(Vk, V, a.ldv, kt * 64, a.Tk, hd, wave, lane);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const bool full = (kt * 64 + 64 <= kl) && !a.causal;  // uniform: no key of this tile is masked
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float ds[8];
#pragma unroll
      for (int bb = 0; bb < 2; ++bb) {
        f32x4_t sacc = {0.f, 0.f, 0.f, 0.f}, pacc = {0.f, 0.f, 0.f, 0.f};
        const int row = 32 * s + rowperm(bb, r);
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
          {
            sacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kimg_frag<64>(Kk, row, ks, lane), qf[ks], sacc, 0, 0, 0);
            pacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kimg_frag<64>(Vk, row, ks, lane), dof[ks], pacc, 0, 0, 0);
          }
        unsigned keep = 0xFu;
        if constexpr (DROP)
          keep = ca_dropout_keep4(a.drop_seed, attn_drop_index(a, b, h, qrow, kt * 64 + 32 * s + 8 * g + 4 * bb), a.drop_p);
        const float kscale = DROP ? 1.f / (1.f - a.drop_p) : 1.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float dpv = DROP ? (((keep >> e) & 1u) ? pacc[e] * kscale : 0.f) : pacc[e];
          float dsv = __builtin_amdgcn_exp2f(fmaf(sacc[e], c2, -lse2)) * (dpv - dq_row);  // (x scale: when dQ is stored)
          if (!full) {
            const int key = kt * 64 + 32 * s + 8 * g + 4 * bb + e;
            const bool ok = key < kl && (!a.causal || key <= qi);
            dsv = ok ? dsv : 0.f;
          }
          ds[4 * bb + e] = dsv;
        }
      }
      const bf16x8_t dsf = pack8(ds);
#pragma unroll
      for (int nb = 0; nb < NNB; ++nb)
        acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsf, timg_frag_k<64>(Kk, s, nb, lane), acc[nb], 0, 0, 0);
    }
    __syncthreads();
  }
  unsigned short* dQ = a.dQ + b * a.sdqb + h * hd;
  const float sc4[4] = {scale, scale, scale, scale};  // dS was formed without the softmax scale
  // (every loop iteration ended with a workgroup barrier: the images are free)
  store_tile16<HDPV>(smem + wave * (attn_stage_bytes(HDPV) / 4), acc, sc4, dQ, a.lddq, q0, a.Tq, hd, lane);
}

// ---- backward: dQ, wide workgroups (same reasoning and ring as attn_fwd_wide_kernel) -----------------------------------
// NW waves x 32 queries; per 64-key tile a K-major image of K (S^T = K Q^T and, read transposed, dQ += dS K) and one of
// V (dP^T = V dO^T): every fragment read feeds the MFMAs of both 16-query blocks of the wave.
template <int HDPV, bool DROP, int NW, int NST, int WPE = 2>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void attn_bwd_dq_wide_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NQ = 2, NKS = HDPV / 32, NNB = HDPV / 16;
  constexpr int IMG = 64 * HDPV * 2, PAIR = 2 * IMG;
  constexpr int QPB = NW * 16 * NQ;
  constexpr int DPT = 2 * (HDPV / 64) * (64 / 8 / NW);  // LDS-DMA instructions per wave and tile
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
  const unsigned short* dO = a.dO + b * a.sdob + h * hd;
  const int q0 = tile * QPB + wave * 16 * NQ;
  int qi[NQ], qrow[NQ];
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    qi[j] = q0 + 16 * j + r;
    qrow[j] = qi[j] < a.Tq ? qi[j] : a.Tq - 1;
  }
  int kl = a.Tk;
  if (a.klen) kl = a.klen[b] < kl ? a.klen[b] : kl;
  int ntile = (kl + 63) / 64;
  if (a.causal) {
    const int last = (tile * QPB + QPB - 1) / 64 + 1;  // keys beyond the workgroup's last query are masked
    ntile = ntile < last ? ntile : last;
  }
  KImgFast<64, HDPV, NW> kfast, vfast;
  kfast.init(a.ldk, wave, lane);
  vfast.init(a.ldv, wave, lane);
  const int nfast = fast_tiles(a.Tk, 64);
  auto issue = [&](int kt, int stage) __attribute__((always_inline)) {
    char* img = smem + stage * PAIR;
    if (kt < nfast) {
      kfast.issue(img, K + (int64_t)kt * 64 * a.ldk, wave);
      vfast.issue(img + IMG, V + (int64_t)kt * 64 * a.ldv, wave);
    } else {
      load_kmajor_image<64, HDPV, NW>(img, K, a.ldk, kt * 64, a.Tk, hd, wave, lane);
      load_kmajor_image<64, HDPV, NW>(img + IMG, V, a.ldv, kt * 64, a.Tk, hd, wave, lane);
    }
  };
#pragma unroll
  for (int t = 0; t < NST - 1; ++t)
    if (t < ntile) issue(t, t);
  // all HDPV/32 k-steps and HDPV/16 column blocks are computed: dims >= hd are zero in every LDS image
  bf16x8_t qf[NQ][NKS], dof[NQ][NKS];
  float lse2[NQ], dq_row[NQ];
  const unsigned short* Oh = a.O + b * a.sob + h * hd;
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    // D = rowsum(dO * O) of the lane's query is taken here, from the dO fragments the kernel holds anyway and the
    // matching O fragments (each lane group has a quarter of the row), and written for the dK/dV kernel, which runs
    // after this one: no separate pass over dO and O (attn_bwd_prep_kernel serves the 64-query path only)
    float dsum = 0.f;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      qf[j][ks] = load_rowfrag(Q, a.ldq, qrow[j], ks, lane, hd);
      dof[j][ks] = load_rowfrag(dO, a.lddo, qrow[j], ks, lane, hd);
      const bf16x8_t of = load_rowfrag(Oh, a.ldo, qrow[j], ks, lane, hd);
      const u16x8_t x = __builtin_bit_cast(u16x8_t, dof[j][ks]), y = __builtin_bit_cast(u16x8_t, of);
#pragma unroll
      for (int e = 0; e < 8; ++e) dsum = fmaf(bf2f(x[e]), bf2f(y[e]), dsum);
    }
    dsum += __shfl_xor(dsum, 16, 64);
    dsum += __shfl_xor(dsum, 32, 64);
    dq_row[j] = dsum;
    if (g == 0 && qi[j] < a.Tq) const_cast<float*>(a.Dq)[((int64_t)b * a.H + h) * a.Tqp + qi[j]] = dsum;
    lse2[j] = a.lse[((int64_t)b * a.H + h) * a.Tqp + qrow[j]] * LOG2E;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (these loads are younger than the first tiles)
  f32x4_t acc[NQ][NNB];
#pragma unroll
  for (int j = 0; j < NQ; ++j)
#pragma unroll
    for (int nb = 0; nb < NNB; ++nb) acc[j][nb] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  const float scale = a.scale;
  const float c2 = scale * LOG2E;
  auto tile_body = [&](auto full_c, int kt, int stage) __attribute__((always_inline)) {
    constexpr bool FULL = decltype(full_c)::value;
    const char* Kk = smem + stage * PAIR;
    const char* Vk = Kk + IMG;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float ds[NQ][8];
#pragma unroll
      for (int bb = 0; bb < 2; ++bb) {
        f32x4_t sacc[NQ], pacc[NQ];
#pragma unroll
        for (int j = 0; j < NQ; ++j) sacc[j] = pacc[j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
        const int row = 32 * s + rowperm(bb, r);
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
          const bf16x8_t kfr = kimg_frag<64>(Kk, row, ks, lane), vfr = kimg_frag<64>(Vk, row, ks, lane);
#pragma unroll
          for (int j = 0; j < NQ; ++j) {
            sacc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfr, qf[j][ks], sacc[j], 0, 0, 0);
            pacc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vfr, dof[j][ks], pacc[j], 0, 0, 0);
          }
        }
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
          unsigned keep = 0xFu;
          if constexpr (DROP)
            keep = ca_dropout_keep4(a.drop_seed, attn_drop_index(a, b, h, qrow[j], kt * 64 + 32 * s + 8 * g + 4 * bb), a.drop_p);
          const float kscale = DROP ? 1.f / (1.f - a.drop_p) : 1.f;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float dpv = DROP ? (((keep >> e) & 1u) ? pacc[j][e] * kscale : 0.f) : pacc[j][e];
            float dsv = __builtin_amdgcn_exp2f(fmaf(sacc[j][e], c2, -lse2[j])) * (dpv - dq_row[j]);  // (x scale: when dQ is stored)
            if constexpr (!FULL) {
              const int key = kt * 64 + 32 * s + 8 * g + 4 * bb + e;
              const bool ok = key < kl && (!a.causal || key <= qi[j]);
              dsv = ok ? dsv : 0.f;
            }
            ds[j][4 * bb + e] = dsv;
          }
        }
      }
      bf16x8_t dsf[NQ];
#pragma unroll
      for (int j = 0; j < NQ; ++j) dsf[j] = pack8(ds[j]);
      // transposed key fragments in batches of four column blocks, the next batch in flight while one is used
      bf16x8_t fa[4], fb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[i] = timg_frag_k_async<64>(Kk, s, i, lane);
#pragma unroll
      for (int bt = 0; bt < NNB / 4; ++bt) {
        lds_wait_all();
#pragma unroll
        for (int i = 0; i < 4; ++i) tie((bt & 1) ? fb[i] : fa[i]);
        if (bt + 1 < NNB / 4) {
#pragma unroll
          for (int i = 0; i < 4; ++i) ((bt & 1) ? fa[i] : fb[i]) = timg_frag_k_async<64>(Kk, s, 4 * (bt + 1) + i, lane);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < NQ; ++j)
            acc[j][4 * bt + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsf[j], (bt & 1) ? fb[i] : fa[i], acc[j][4 * bt + i], 0, 0, 0);
      }
    }
  };
  int stage = 0;
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
      tile_body(full_c, kt, stage);
      stage = stage + 1 == NST ? 0 : stage + 1;
    }
  };
  const int nfull = a.causal ? 0 : (kl / 64 < ntile ? kl / 64 : ntile);
  run(std::true_type{}, 0, nfull);
  run(std::false_type{}, nfull, ntile);
  __syncthreads();  // every wave is done with the images: the LDS becomes output staging
  unsigned short* dQ = a.dQ + b * a.sdqb + h * hd;
  const float sc4[4] = {scale, scale, scale, scale};  // dS was formed without the softmax scale
  char* st = smem + wave * (16 * (HDPV * 2 + 16));
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    if (j) __builtin_amdgcn_wave_barrier();
    store_tile16<HDPV>(st, acc[j], sc4, dQ, a.lddq, q0 + 16 * j, a.Tq, hd, lane);
  }
}

// ---- launcher ---------------------------------------------------------------------------------------------------------
int attn_launch_bwd(const AttnPlan& p, const AttnArgs& a, hipStream_t s, const char* who) {
  switch (attn_inst(p)) {
    case attn_inst(ATTN_BWD_PREP, 0, 0):
      return attn_launch(attn_bwd_prep_kernel, p, s, who, a.dO, a.lddo, a.sdob, (const unsigned short*)a.O, a.ldo, a.sob,
                         (float*)a.Dq, a.H, a.Tq, a.Tqp, a.hd, a.B, a.row_off);
    case attn_inst(ATTN_BWD_DQ, 64, 0): return attn_launch(attn_bwd_dq_kernel<64, false>, p, s, who, a);
    case attn_inst(ATTN_BWD_DQ, 64, 1): return attn_launch(attn_bwd_dq_kernel<64, true>, p, s, who, a);
    case attn_inst(ATTN_BWD_DQ, 128, 0): return attn_launch(attn_bwd_dq_kernel<128, false>, p, s, who, a);
    case attn_inst(ATTN_BWD_DQ, 128, 1): return attn_launch(attn_bwd_dq_kernel<128, true>, p, s, who, a);
    case attn_inst(ATTN_BWD_DQ_WIDE, 64, 0, 3): return attn_launch(attn_bwd_dq_wide_kernel<64, false, 4, 2, 3>, p, s, who, a);
    case attn_inst(ATTN_BWD_DQ_WIDE, 64, 0, 2): return attn_launch(attn_bwd_dq_wide_kernel<64, false, 4, 2, 2>, p, s, who, a);
    case attn_inst(ATTN_BWD_DQ_WIDE, 64, 1, 2): return attn_launch(attn_bwd_dq_wide_kernel<64, true, 4, 2, 2>, p, s, who, a);
    case attn_inst(ATTN_BWD_DQ_WIDE, 128, 0, 2): return attn_launch(attn_bwd_dq_wide_kernel<128, false, 4, 2, 2>, p, s, who, a);
    case attn_inst(ATTN_BWD_DQ_WIDE, 128, 1, 2): return attn_launch(attn_bwd_dq_wide_kernel<128, true, 4, 2, 2>, p, s, who, a);
    case attn_inst(ATTN_BWD_DKV, 64, 0): return attn_launch(attn_bwd_dkv_kernel<64, false>, p, s, who, a);
    case attn_inst(ATTN_BWD_DKV, 64, 1): return attn_launch(attn_bwd_dkv_kernel<64, true>, p, s, who, a);
    case attn_inst(ATTN_BWD_DKV, 128, 0): return attn_launch(attn_bwd_dkv_kernel<128, false>, p, s, who, a);
    case attn_inst(ATTN_BWD_DKV, 128, 1): return attn_launch(attn_bwd_dkv_kernel<128, true>, p, s, who, a);
    // (the 128-key kernel exists for head_dim <= 64 only: attn_plan_bwd)
    case attn_inst(ATTN_BWD_DKV_WIDE, 64, 0, 3): return attn_launch(attn_bwd_dkv_wide_kernel<64, false, 2, 3>, p, s, who, a);
    case attn_inst(ATTN_BWD_DKV_WIDE, 64, 0, 2): return attn_launch(attn_bwd_dkv_wide_kernel<64, false, 2, 2>, p, s, who, a);
    case attn_inst(ATTN_BWD_DKV_WIDE, 64, 1, 2): return attn_launch(attn_bwd_dkv_wide_kernel<64, true, 2, 2>, p, s, who, a);
  }
  return attn_no_kernel(p, who);
}
