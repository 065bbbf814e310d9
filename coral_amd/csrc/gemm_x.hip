// bf16 GEMM kernel X: 256x256 tile, 8 waves (2x4, 128x64 each), 2 LDS stages, one workgroup per CU, persistent over a
// virtual grid where the tiles outnumber the CUs; plain launches and grouped ones (CaGemmGroup, gemm_common.h).
// Half the LDS-fill bytes per FLOP of kernel S (the fill stream is what bounds S);
// used when both output dimensions are large enough to give every CU a tile.
#include "gemm_common.h"

static_assert(X_LDS_BYTES >= 4 * XTILE, "kernel X: the epilogue staging covers the two stages of both operand tiles");

// counter slots for persistent launches: launches that may be in flight together (two streams) use different slots
#define X_CNT_SLOTS 64
__device__ unsigned g_x_cnt[X_CNT_SLOTS][8];
#ifdef X_STAMPS
__device__ long long g_x_stamps[512 * 8 * 8];
extern "C" int ca_gemm_x_stamps(long long* host, int n) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_x_stamps), (size_t)n * sizeof(long long));
}
#endif
template <int AL, int BL, bool KS>
__device__ __forceinline__ void gemm_x_body(const CaGemmGroup& grp) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;  // 2 x 4 waves, 128 (M) x 64 (N) each
  // ---- persistent tile loop ------------------------------------------------------------------------------------
  // One tile per workgroup when the launch covers the virtual grid (vgrid == gridDim.x).  Otherwise the workgroup
  // keeps pulling virtual blocks of its XCD until they run out: a CU that finishes early starts its next tile at once
  // (no round structure: the tiles of a "round" stop finishing together, so their output bursts spread out in time
  // and the next tile's first operand fetch runs under the previous tile's store drain).  Which workgroup computes a
  // tile never changes its result.
  const int vgrid = grp.vgrid;
  const int xcd = (int)blockIdx.x & 7;
  const int npx = ((int)gridDim.x - xcd + 7) >> 3;  // workgroups of this XCD in the launch
  const int nvx = (vgrid - xcd + 7) >> 3;           // virtual blocks of this XCD
  const int ndyn = nvx > npx ? nvx - npx : 0;       // ... handed out dynamically
  // LDS: A0 | A1 | B0 | B1 (the two operand stages, 128 KiB) in the first X_LDS_BYTES, which the epilogue reuses as
  // eight 64 x 64 fp32 staging tiles, one per wave; behind them (X_LAUNCH_LDS = X_LDS_BYTES + 64) the word pair that
  // carries a persistent workgroup's next block index.  Thread 0 writes a word at the start of a tile, every wave
  // reads it behind the main loop - at least one K-step barrier after the write; the two words alternate per
  // iteration, so the write of iteration i + 1 cannot overtake a read of iteration i.
  volatile unsigned* nextw = (volatile unsigned*)(smem + X_LDS_BYTES);
  // K-major operands and plain MN-major ones stream through a scalar base (KMajorStream / MNMajorStream); MN-major
  // operands with segmented rows (KS) keep the per-lane pointer walk.
  KMajorStream<4> la_k, lb_k;
  MNMajorStream<4, 32> la_f, lb_f;
  MNMajorLoader<4, 32, KS> la_m, lb_m;
  int vb = (int)blockIdx.x;
  int dbase = npx, dcount = ndyn;  // dynamic blocks of this XCD: local indices dbase .. dbase + dcount - 1
  if (grp.cnt != nullptr && grp.dyn_first) {
    dbase = 0;
    dcount = nvx;
    if (tid == 0) {
      const unsigned i = __hip_atomic_fetch_add(&grp.cnt[xcd], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (i == (unsigned)(dcount + npx - 1)) __hip_atomic_store(&grp.cnt[xcd], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      nextw[1] = i;  // (the word of odd iterations: rewritten at the start of iteration 1, K-step barriers after this read)
    }
    __syncthreads();
    const unsigned i = (unsigned)__builtin_amdgcn_readfirstlane((int)nextw[1]);
    vb = i < (unsigned)dcount ? xcd + 8 * (int)i : vgrid;
  }
  for (int iter = 0; vb < vgrid; ++iter) {
  int vb_next = vgrid;
  if (grp.cnt != nullptr && tid == 0) {
    // this workgroup's NEXT block (the answer is read after the tile): relaxed device-scope counter
    const unsigned i = __hip_atomic_fetch_add(&grp.cnt[xcd], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (i == (unsigned)(dcount + npx - 1)) __hip_atomic_store(&grp.cnt[xcd], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    nextw[iter & 1] = i;
  }
  bool live = true;
  int which = 0, gt = 0;
  if (grp.count > 1) {
    // grouped launch: the group's tiles form one list (problem after problem, each in run order) and XCD x
    // (= block & 7) takes the x-th run of ceil(total / 8) of them: every XCD gets the same number of tiles
    // whatever the shapes, and a run covers a compact band of one or two problems.
    gt = (vb & 7) * (vgrid >> 3) + (vb >> 3);
    live = gt < grp.total;
    if (live) {
#pragma unroll
      for (int i = 1; i < X_GROUP_MAX; ++i)
        if (grp.count > i && gt >= grp.first[i]) which = i;
    }
  }
  const CaGemmDesc d = grp.d[which];
  int tm = 0, tn = 0;
  if (live) {
    if (grp.count > 1)
      run_tile(gt - grp.first[which], (d.M + XBM - 1) / XBM, (d.N + XBN - 1) / XBN, tm, tn);
    else
      live = tile_of_block_g<4, 8>(vb, vgrid, (d.M + XBM - 1) / XBM, (d.N + XBN - 1) / XBN, tm, tn, d.xcd_balanced != 0);
  }
  if (live) {
  const int m0 = tm * XBM, n0 = tn * XBN;
  const int z = blockIdx.z;
  const int z1 = z / d.batch2, z2 = z % d.batch2;
  const __bf16* A = (const __bf16*)d.A + z1 * d.sA1 + z2 * d.sA2;
  const __bf16* B = (const __bf16*)d.B + z1 * d.sB1 + z2 * d.sB2;

  auto init_loaders = [&](int row0, int col0) {
    if (AL == CA_KMAJOR)
      la_k.init(A, d.lda, row0, d.M, wave, lane);
    else if (KS)
      la_m.init(A, d.lda, d.a_kseg, d.a_kseg_stride, row0, d.M, wave, lane);
    else
      la_f.init(A, d.lda, row0, d.M, wave, lane);
    if (BL == CA_KMAJOR)
      lb_k.init(B, d.ldb, col0, d.N, wave, lane);
    else if (KS)
      lb_m.init(B, d.ldb, d.b_kseg, d.b_kseg_stride, col0, d.N, wave, lane);
    else
      lb_f.init(B, d.ldb, col0, d.N, wave, lane);
  };
  init_loaders(m0, n0);

  f32x4_t acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  float xbias[8];  // the lane's bias values, requested a whole main loop ahead of the epilogue (the segmented-K
                   // instantiations - convolution weight gradients, no bias - have no registers to spare for it)
  if constexpr (!KS) epi_load_bias(d, lane, n0 + wn * 64, z1, z2, xbias);
#ifdef X_STAMPS
  long long stamp_dma = 0, stamp_bar = 0;
#endif
  const int cs_parts = ((d.N + XBN - 1) / XBN) < 8 ? ((d.N + XBN - 1) / XBN) : 8;  // tile columns sharing the column sums
  const bool do_colsum = d.a_colsum != nullptr && tn < cs_parts;
  float csum0 = 0.f, csum1 = 0.f;  // this lane's share of sum_k A[k, m] for m = m0 + wm*128 + (ih*4 + wn)*16 + (lane & 15)

  const int K = d.K;
  const int nk = (K + BK - 1) / BK;

  // Software pipeline over K-steps of 64; LDS holds two stages of each operand tile: A0 | A1 | B0 | B1 (32 KiB each).
  // One barrier per K-step, placed in FRONT of the last of the four MFMA blocks (k-half s x m-half ih, 16 MFMAs
  // each): by then every wave has read all of tile kt and tile kt+1 has landed, so the first fragments of tile kt+1
  // are read behind the barrier and their LDS latency hides under block 3.  Fragments are double-buffered in
  // registers: the reads for block b+1 are issued BETWEEN the MFMAs of block b (one read after every second MFMA,
  // all in the first half of the block) from per-lane base addresses computed once, with the stage / k-half /
  // fragment selected by the instruction's immediate offset - no address arithmetic and no MFMA-free phase between
  // blocks.  A tile's 8 LDS-DMA go out as one burst per wave into the stage the barrier just freed: waves 0-3
  // behind the barrier, waves 4-7 one block later (SIMD partners never issue their bursts together;
  // profiles/r01_gemm_ablation.txt).
  auto burst = [&](int kt) {  // this wave's share of tile kt (called once per tile, in K order)
    if (kt >= nk) return;
    char* na = smem + (kt & 1) * XTILE;
    char* nb = na + 2 * XTILE;
    const bool full = (kt + 1) * BK <= K;  // wave-uniform
    if (full) {
#pragma unroll
      for (int part = 0; part < 4; ++part) {
        if (AL == CA_MNMAJOR && KS)
          la_m.issue_one(na, wave, lane, kt * BK, K, part);
        else if (AL == CA_KMAJOR)
          la_k.issue_one(na, wave, part);
        else
          la_f.issue_one(na, wave, part);
        if (BL == CA_MNMAJOR && KS)
          lb_m.issue_one(nb, wave, lane, kt * BK, K, part);
        else if (BL == CA_KMAJOR)
          lb_k.issue_one(nb, wave, part);
        else
          lb_f.issue_one(nb, wave, part);
      }
    } else {
#pragma unroll
      for (int part = 0; part < 4; ++part) {
        if (AL == CA_MNMAJOR && KS)
          la_m.issue_one(na, wave, lane, kt * BK, K, part);
        else if (AL == CA_KMAJOR)
          la_k.issue_one_tail(na, wave, K - kt * BK, part);
        else
          la_f.issue_one_tail(na, wave, lane, K - kt * BK, part);
        if (BL == CA_MNMAJOR && KS)
          lb_m.issue_one(nb, wave, lane, kt * BK, K, part);
        else if (BL == CA_KMAJOR)
          lb_k.issue_one_tail(nb, wave, K - kt * BK, part);
        else
          lb_f.issue_one_tail(nb, wave, lane, K - kt * BK, part);
      }
    }
    if (AL == CA_KMAJOR) la_k.advance();
    if (AL == CA_MNMAJOR && !KS) la_f.advance();
    if (BL == CA_KMAJOR) lb_k.advance();
    if (BL == CA_MNMAJOR && !KS) lb_f.advance();
  };
  // the partial last K-step (K % 64 != 0): zero what this wave loaded beyond K, once its LDS-DMA has landed
  auto zero_tail = [&](int kt) {
    if (kt != nk - 1 || nk * BK == K) return;
    char* na = smem + (kt & 1) * XTILE;
    char* nb = na + 2 * XTILE;
    const int krem = K - kt * BK;
    if (AL == CA_KMAJOR) la_k.zero_fix(na, wave, lane, krem);
    if (AL == CA_MNMAJOR && !KS) la_f.zero_fix(na, wave, lane, krem);
    if (BL == CA_KMAJOR) lb_k.zero_fix(nb, wave, lane, krem);
    if (BL == CA_MNMAJOR && !KS) lb_f.zero_fix(nb, wave, lane, krem);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  };
  // per-lane fragment base addresses (stage 0, k-half 0, fragment 0 unless noted)
  const uint32_t lds0 = (uint32_t)(uintptr_t)(lptr_t)smem;
  uint32_t abase[8], bbase[4];  // K-major: [0], [1] = k-half 0, 1; MN-major: one per fragment (XOR swizzle)
  if (AL == CA_KMAJOR) {
    const int r = wm * 128 + (lane & 15);
#pragma unroll
    for (int sh = 0; sh < 2; ++sh) abase[sh] = lds0 + r * 128 + (((4 * sh + (lane >> 4)) ^ ((r >> 1) & 7)) * 16);
  } else {
    const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
    const int swz = q | ((g & 1) << 2);
#pragma unroll
    for (int f = 0; f < 8; ++f) {
      const int c = ((((wm * 128 + f * 16) >> 3) + (pp >> 1)) ^ (swz << 1));
      abase[f] = lds0 + (8 * g + q) * 512 + c * 16 + (pp & 1) * 8;
    }
  }
  if (BL == CA_KMAJOR) {
    const int r = wn * 64 + (lane & 15);
#pragma unroll
    for (int sh = 0; sh < 2; ++sh)
      bbase[sh] = lds0 + 2 * XTILE + r * 128 + (((4 * sh + (lane >> 4)) ^ ((r >> 1) & 7)) * 16);
  } else {
    const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
    const int swz = q | ((g & 1) << 2);
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const int c = ((((wn * 64 + f * 16) >> 3) + (pp >> 1)) ^ (swz << 1));
      bbase[f] = lds0 + 2 * XTILE + (8 * g + q) * 512 + c * 16 + (pp & 1) * 8;
    }
  }
  bf16x8_t A0[4], A1[4], B0[4], B1[4];
  // fragment f (0..7 for A, 0..3 for B) of k-half SH from stage ST, all compile-time
#define X_RD_A(ST, SH, F, dst)                                                            \
  do {                                                                                    \
    if (AL == CA_KMAJOR)                                                                  \
      dst = lds_read_b128<(ST) * XTILE + (F) * 2048>(abase[SH]);                          \
    else                                                                                  \
      dst = lds_read_tr<(ST) * XTILE + (SH) * 16384, 2048>(abase[F]);                     \
  } while (0)
#define X_RD_B(ST, SH, F, dst)                                                            \
  do {                                                                                    \
    if (BL == CA_KMAJOR)                                                                  \
      dst = lds_read_b128<(ST) * XTILE + (F) * 2048>(bbase[SH]);                          \
    else                                                                                  \
      dst = lds_read_tr<(ST) * XTILE + (SH) * 16384, 2048>(bbase[F]);                     \
  } while (0)
#define X_SB __builtin_amdgcn_sched_barrier(0)
  // two MFMAs of block (m-half IH, fragments AF x BF): A fragment I against B fragments J and J+1
#define X_MM2(IH, AF, BF, I, J)                                                                                   \
  do {                                                                                                            \
    acc[(IH) * 4 + (I)][J] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(BF[J], AF[I], acc[(IH) * 4 + (I)][J], 0, 0, 0); \
    acc[(IH) * 4 + (I)][(J) + 1] =                                                                                \
        __builtin_amdgcn_mfma_f32_16x16x32_bf16(BF[(J) + 1], AF[I], acc[(IH) * 4 + (I)][(J) + 1], 0, 0, 0);       \
    X_SB;                                                                                                         \
  } while (0)
  // bias gradient from the streaming A tile (a_colsum): the K-steps are dealt round-robin to the first
  // cs_parts tile columns; inside a workgroup the four waves of an m-half share the work, wave wn taking
  // fragment i == wn of every block
  auto colsum_acc = [&](bool cs_step, int ih, bf16x8_t (&af)[4]) {
    if (AL == CA_MNMAJOR && cs_step) {
      // (wn is wave-uniform: a branch per case keeps the fragments in registers - indexing af[] by a run-time
      // value would send the whole array through scratch memory)
      f32x4_t z;
      if (wn == 0)
        z = __builtin_bit_cast(f32x4_t, af[0]);
      else if (wn == 1)
        z = __builtin_bit_cast(f32x4_t, af[1]);
      else if (wn == 2)
        z = __builtin_bit_cast(f32x4_t, af[2]);
      else
        z = __builtin_bit_cast(f32x4_t, af[3]);
      // v_dot2c_f32_bf16 with a vector of ones: two bf16 values added to the fp32 sum per instruction
      typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
      const bf16x2_t ones = __builtin_bit_cast(bf16x2_t, 0x3F803F80u);
      float s = ih == 0 ? csum0 : csum1;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        // through an integer word on purpose: bit-casting element q of the float vector straight to a bf16 pair
        // makes hipcc 7.2 read element 0 four times (seen in the ISA)
        const unsigned int wq = __float_as_uint(z[q]);
        s = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, wq), ones, s, false);
      }
      if (ih == 0)
        csum0 = s;
      else
        csum1 = s;
    }
  };
  // one K-step on stage ST (compile-time); reads of the next tile come from stage 1 - ST
  auto kstep = [&](auto st_c, int kt) {
    constexpr int ST = decltype(st_c)::value;
    const bool cs_step = do_colsum && (kt % cs_parts) == tn;  // this K-step belongs to this tile column
    // waves 4-7 issue their share of tile kt+1 here - or, in the weight-gradient form (both operands MN-major), one
    // MFMA block later, when their SIMD partners' bursts (issued behind the barrier) are over: 2 685 against 2 802
    // cycles per K-step there, but 2 840 against 2 590 for the K-major forms (s_memtime stamps, tools/archive/dev_x_stamps.py)
    constexpr bool LATE_BURST = AL == CA_MNMAJOR && BL == CA_MNMAJOR && !KS;
    if (!LATE_BURST && wave >= 4) burst(kt + 1);
    // block 0: A(s0, m-half 0) x B(s0); reads A(s0, m-half 1)
    lds_wait(B0);
    lds_wait(A0);
    colsum_acc(cs_step, 0, A0);
    X_SB;
    __builtin_amdgcn_s_setprio(1);
    X_MM2(0, A0, B0, 0, 0); X_RD_A(ST, 0, 4, A1[0]); X_SB;
    X_MM2(0, A0, B0, 0, 2); X_RD_A(ST, 0, 5, A1[1]); X_SB;
    X_MM2(0, A0, B0, 1, 0); X_RD_A(ST, 0, 6, A1[2]); X_SB;
    X_MM2(0, A0, B0, 1, 2); X_RD_A(ST, 0, 7, A1[3]); X_SB;
    X_MM2(0, A0, B0, 2, 0);
    X_MM2(0, A0, B0, 2, 2);
    X_MM2(0, A0, B0, 3, 0);
    X_MM2(0, A0, B0, 3, 2);
    __builtin_amdgcn_s_setprio(0);
    if (LATE_BURST && wave >= 4) burst(kt + 1);
    // block 1: A(s0, m-half 1) x B(s0); reads B(s1) and A(s1, m-half 0)
    lds_wait(A1);
    colsum_acc(cs_step, 1, A1);
    X_SB;
    __builtin_amdgcn_s_setprio(1);
    X_MM2(1, A1, B0, 0, 0); X_RD_B(ST, 1, 0, B1[0]); X_SB;
    X_MM2(1, A1, B0, 0, 2); X_RD_B(ST, 1, 1, B1[1]); X_SB;
    X_MM2(1, A1, B0, 1, 0); X_RD_B(ST, 1, 2, B1[2]); X_SB;
    X_MM2(1, A1, B0, 1, 2); X_RD_B(ST, 1, 3, B1[3]); X_SB;
    X_MM2(1, A1, B0, 2, 0); X_RD_A(ST, 1, 0, A0[0]); X_SB;
    X_MM2(1, A1, B0, 2, 2); X_RD_A(ST, 1, 1, A0[1]); X_SB;
    X_MM2(1, A1, B0, 3, 0); X_RD_A(ST, 1, 2, A0[2]); X_SB;
    X_MM2(1, A1, B0, 3, 2); X_RD_A(ST, 1, 3, A0[3]); X_SB;
    __builtin_amdgcn_s_setprio(0);
    // block 2: A(s1, m-half 0) x B(s1); reads A(s1, m-half 1)
    lds_wait(B1);
    lds_wait(A0);
    colsum_acc(cs_step, 0, A0);
    X_SB;
    __builtin_amdgcn_s_setprio(1);
    X_MM2(0, A0, B1, 0, 0); X_RD_A(ST, 1, 4, A1[0]); X_SB;
    X_MM2(0, A0, B1, 0, 2); X_RD_A(ST, 1, 5, A1[1]); X_SB;
    X_MM2(0, A0, B1, 1, 0); X_RD_A(ST, 1, 6, A1[2]); X_SB;
    X_MM2(0, A0, B1, 1, 2); X_RD_A(ST, 1, 7, A1[3]); X_SB;
    X_MM2(0, A0, B1, 2, 0);
    X_MM2(0, A0, B1, 2, 2);
    X_MM2(0, A0, B1, 3, 0);
    X_MM2(0, A0, B1, 3, 2);
    __builtin_amdgcn_s_setprio(0);
    lds_wait(A1);  // the last fragment reads of tile kt have returned
    colsum_acc(cs_step, 1, A1);
    // tile kt+1 has landed (this wave's share; the barrier covers the others) and stage ST is free
#ifdef X_STAMPS
    const long long st0 = __builtin_amdgcn_s_memtime();
#endif
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#ifdef X_STAMPS
    const long long st1 = __builtin_amdgcn_s_memtime();
#endif
    zero_tail(kt + 1);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
#ifdef X_STAMPS
    const long long st2 = __builtin_amdgcn_s_memtime();
    stamp_dma += st1 - st0;
    stamp_bar += st2 - st1;
#endif
    if (wave < 4) burst(kt + 2);
    X_SB;
    // block 3: A(s1, m-half 1) x B(s1); reads B(s0), A(s0, m-half 0) of tile kt+1 (harmless stale data after the
    // last tile)
    __builtin_amdgcn_s_setprio(1);
    X_MM2(1, A1, B1, 0, 0); X_RD_B(1 - ST, 0, 0, B0[0]); X_SB;
    X_MM2(1, A1, B1, 0, 2); X_RD_B(1 - ST, 0, 1, B0[1]); X_SB;
    X_MM2(1, A1, B1, 1, 0); X_RD_B(1 - ST, 0, 2, B0[2]); X_SB;
    X_MM2(1, A1, B1, 1, 2); X_RD_B(1 - ST, 0, 3, B0[3]); X_SB;
    X_MM2(1, A1, B1, 2, 0); X_RD_A(1 - ST, 0, 0, A0[0]); X_SB;
    X_MM2(1, A1, B1, 2, 2); X_RD_A(1 - ST, 0, 1, A0[1]); X_SB;
    X_MM2(1, A1, B1, 3, 0); X_RD_A(1 - ST, 0, 2, A0[2]); X_SB;
    X_MM2(1, A1, B1, 3, 2); X_RD_A(1 - ST, 0, 3, A0[3]); X_SB;
    __builtin_amdgcn_s_setprio(0);
  };
#ifdef X_STAMPS
  const long long stamp_t0 = __builtin_amdgcn_s_memtime();
#endif
  burst(0);
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  zero_tail(0);
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
#ifdef X_STAMPS
  const long long stamp_t1 = __builtin_amdgcn_s_memtime();
  const long long stamp_r1 = __builtin_amdgcn_s_memrealtime();  // 100 MHz: the loop's shader clock = d memtime / d realtime x 100 MHz
  __builtin_amdgcn_s_waitcnt(0xC07F);
#endif
  X_RD_B(0, 0, 0, B0[0]); X_RD_B(0, 0, 1, B0[1]); X_RD_B(0, 0, 2, B0[2]); X_RD_B(0, 0, 3, B0[3]);
  X_RD_A(0, 0, 0, A0[0]); X_RD_A(0, 0, 1, A0[1]); X_RD_A(0, 0, 2, A0[2]); X_RD_A(0, 0, 3, A0[3]);
  if (wave < 4) burst(1);
  for (int kt = 0; kt < nk; kt += 2) {
    kstep(std::integral_constant<int, 0>{}, kt);
    if (kt + 1 < nk) kstep(std::integral_constant<int, 1>{}, kt + 1);
  }
#undef X_RD_A
#undef X_RD_B
#undef X_MM2
#undef X_SB
#ifdef X_STAMPS
  const long long stamp_t2 = __builtin_amdgcn_s_memtime();
  const long long stamp_r2 = __builtin_amdgcn_s_memrealtime();
#endif
  if (AL == CA_MNMAJOR && do_colsum) {
    // a lane's fragment holds k = 8g..8g+7 of a 32-k step: add the four lane groups, then lanes 0-15 own 16 rows
#pragma unroll
    for (int ih = 0; ih < 2; ++ih) {
      float s = ih == 0 ? csum0 : csum1;
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      const int m = m0 + wm * 128 + (ih * 4 + wn) * 16 + (lane & 15);
      if (lane < 16 && m < d.M) d.a_colsum[(int64_t)tn * d.a_colsum_ld + m] = s;  // this tile column's share
    }
  }
  // this workgroup's next block (thread 0 wrote the word at the start of the tile, K-step barriers ago)
  unsigned nxt = 0;
  if (grp.cnt != nullptr) nxt = (unsigned)__builtin_amdgcn_readfirstlane((int)nextw[iter & 1]);  // wave-uniform by construction
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();  // every wave has read the last K-step: the operand stages are free
  asm volatile("" ::: "memory");
  if (grp.cnt != nullptr) vb_next = nxt < (unsigned)dcount ? xcd + 8 * (dbase + (int)nxt) : vgrid;
  // two 64-row halves through the shared epilogue
#pragma unroll
  for (int ih = 0; ih < 2; ++ih) {
    f32x4_t half[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) half[i][j] = acc[ih * 4 + i][j];
    gemm_epilogue(d, half, smem, wave, lane, m0 + wm * 128 + ih * 64, n0 + wn * 64, z, z1, z2, KS ? nullptr : &xbias);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // staging reads done before it is overwritten
  }
  if (grp.cnt != nullptr) __syncthreads();  // every wave is done with the staging area before the next tile lands in it
#ifdef X_STAMPS
  {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const long long stamp_t3 = __builtin_amdgcn_s_memtime();
    if (lane == 0 && iter == 0) {
      long long* o = g_x_stamps + ((size_t)blockIdx.x * 8 + wave) * 8;
      o[0] = stamp_t1 - stamp_t0;  // prologue: first tile
      o[1] = stamp_t2 - stamp_t1;  // main loop
      o[2] = stamp_t3 - stamp_t2;  // epilogue incl. store drain
      o[3] = stamp_dma;
      o[4] = stamp_bar;
      o[5] = nk;
      o[6] = stamp_r2 - stamp_r1;  // main loop in 100-MHz ticks
    }
  }
#endif
  }  // live
  else if (grp.cnt != nullptr) {
    // a padding block of the virtual grid: no K-step barrier separates thread 0's write from the reads
    __syncthreads();
    const unsigned i = (unsigned)__builtin_amdgcn_readfirstlane((int)nextw[iter & 1]);
    vb_next = i < (unsigned)dcount ? xcd + 8 * (dbase + (int)i) : vgrid;
  }
  if (grp.cnt == nullptr) break;
  vb = vb_next;
  }  // persistent tile loop
}

template <int AL, int BL, bool KS>
__global__ __launch_bounds__(512) void ca_gemm_kernel_x(const CaGemmGroup grp) {
  gemm_x_body<AL, BL, KS>(grp);
}
// The NT form (every forward GEMM of the training step) is held to 224 registers per lane: the background AdamW of the
// overlapped optimiser (misc.hip adamw_kernel, 60 -> 64 registers, one workgroup per CU) then fits beside the two waves
// per SIMD of a persistent workgroup (2 x 224 + 64 = 512).  At 225 the allocation granule of 8 makes it 2 x 232: the two
// kernels stop sharing CUs, alternate instead, and the XLS-R-2B step went from 72 to 91 ms (NOTEBOOK.md R5.6).
// (amdgpu_num_vgpr counts one half of gfx950's unified VGPR|AGPR file: 112 = 224 registers; tests/test_build.py checks
// the code object.)
template <>
__global__ __launch_bounds__(512) __attribute__((amdgpu_num_vgpr(112)))
void ca_gemm_kernel_x<CA_KMAJOR, CA_KMAJOR, false>(const CaGemmGroup grp) {
  gemm_x_body<CA_KMAJOR, CA_KMAJOR, false>(grp);
}

// ---- launcher ---------------------------------------------------------------------------------------------------------
// Layouts indexed a_layout * 2 + b_layout (+ 4 with segmented K).  kseg is defined for MN-major operands only
// (include/coral_amd.h, "row(k)"): with two K-major operands KS reaches no loader, and the slot names the <0, 0, false>
// kernel - which also puts that case under the register cap above.
static const GroupKernel k_gemm_x[8] = {ca_gemm_kernel_x<0, 0, false>, ca_gemm_kernel_x<0, 1, false>, ca_gemm_kernel_x<1, 0, false>,
                                        ca_gemm_kernel_x<1, 1, false>, ca_gemm_kernel_x<0, 0, false>, ca_gemm_kernel_x<0, 1, true>,
                                        ca_gemm_kernel_x<1, 0, true>,  ca_gemm_kernel_x<1, 1, true>};

__global__ void gemm_set_epi_general_x_kernel(int on) { g_ca_epi_general = on; }
hipError_t gemm_set_epi_general_x(int on) { return gemm_run_epi_general_setter(gemm_set_epi_general_x_kernel, on); }
const void* gemm_x_nt_kernel() { return (const void*)ca_gemm_kernel_x<0, 0, false>; }

// A persistent launch takes one of the counter slots (launches that may be in flight together use different ones);
// without the counters it falls back to one workgroup per tile.
int gemm_launch_x(const GemmPlan& p, CaGemmGroup& g, hipStream_t s, const char* who) {
  static unsigned seq = 0;
  static std::atomic<uint64_t> raised{0};
  if (int rc = gemm_allow_lds(raised, k_gemm_x, 8, p.lds, who)) return rc;
  g.vgrid = (int)p.vgrid;
  g.cnt = nullptr;
  g.dyn_first = p.dyn_first;
  dim3 grid(p.vgrid, 1, p.grid_z);
  if (p.persistent) {
    unsigned* base = nullptr;
    if (hipGetSymbolAddress((void**)&base, HIP_SYMBOL(g_x_cnt)) == hipSuccess && base) {
      g.cnt = base + (size_t)(seq++ % X_CNT_SLOTS) * 8;
      grid.x = p.grid_x;
    }
  }
  return gemm_launch(k_gemm_x[p.lay + 4 * p.ks], grid, p, s, who, g);
}
#undef X_CNT_SLOTS
