// MFMA GEMM family for gfx950 (CDNA4): what the kernel files share.  See include/coral_amd.h (ca_gemm_bf16).
//
// Common to the tiled kernels (gemm_s.hip: S and M, gemm_l.hip, gemm_x.hip, gemm_fp8.hip):
//   * a wave owns 64x64 output tiles as 4x4 v_mfma_f32_16x16x32_bf16 accumulators (operands swapped so a lane ends up
//     with 4 consecutive n of one m: 8-byte bf16 / 16-byte fp32 stores).
//   * both operand tiles are staged HBM -> LDS with global_load_lds_dwordx4 (no VGPR round trip); the LDS image is
//     lane-linear, bank conflicts are removed by permuting the per-lane SOURCE chunk and applying the same XOR on the
//     fragment read.
//   * KMAJOR operands ([rows][64 k], 128-B rows) are read with ds_read_b128; MNMAJOR operands ([64 k][mn]) with
//     ds_read_b64_tr_b16 (hardware transpose), so NT / NN / TN / TT all run natively without transposed copies.
//   * out-of-range rows are clamped (results discarded), out-of-range k reads a zero page or is zeroed in LDS.
//   * one epilogue (gemm_epilogue), walked per 64x64 wave tile through an LDS staging tile.
// The skinny kernel (gemm_skinny.hip) streams its weights without LDS staging and has its own epilogue.
//
// This header: the LDS-DMA loaders, fragment readers and epilogue, the argument of kernel X (CaGemmGroup), and the
// launchers gemm.hip calls.  Which kernel a descriptor gets is decided in gemm_plan.h.
#pragma once
#include "common.h"
#include "gemm_plan.h"  // tile shapes, LDS sizes, the tile-grid arithmetic and the kernel-choice rule
#include <hip/hip_ext.h>
#include <atomic>
#include <type_traits>

#define TILE_BYTES (BM * BK * 2)  // 16 KiB per operand tile (kernels S and M, fp8 S)
#define XTILE (XBM * BK * 2)      // 32 KiB per operand tile (kernel X, fp8 X)

// (one copy per kernel file - every translation unit is its own code object - and still symbols with external linkage,
// as in attn_common.h)
inline __device__ __attribute__((aligned(16))) uint32_t g_ca_zero_page[4];
// tests: 1 = every wave tile takes the general epilogue walk.  ca_gemm_debug_general_epilogue sets every file's copy
// through that file's gemm_set_epi_general_*(), from the device side: the host's handles of an inline variable are
// merged by the linker, so a hipMemcpyToSymbol would reach one copy only, whichever file it is called from.
inline __device__ int g_ca_epi_general = 0;

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// LDS-DMA, 16 B per lane from a per-lane address to the wave's 1-KiB LDS piece.  Inline asm like the scalar-base
// form below, so that M0 is only ever written inside these statements (the compiler does not track M0 across them).
// The hazard recogniser does not look inside an asm string, so the wait state between the SALU write of M0 and the
// LDS-DMA that reads it is written out (hipcc pads its own LDS-DMA the same way).  The scalar-base form's other
// hazard - a VMEM instruction reading SGPRs that a VALU instruction (v_readfirstlane) wrote needs five states - does
// not arise here: every base below is the result of scalar arithmetic on kernel arguments and tile indices.
__device__ __forceinline__ void glds16(const void* g, char* lds_wave_base) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off"
               :
               : "v"(g), "s"((uint32_t)(uintptr_t)(lptr_t)lds_wave_base)
               : "memory", "m0");
}

// ---- per-lane loader state -------------------------------------------------------------
// NI = LDS-DMA instructions per wave per tile (each moves 1 KiB = 64 lanes x 16 B).
// operand stored [k][mn], mn contiguous; LDS image [64 k][PC*8 mn]; PC = 16-B chunks per row.
// The source pointer of each lane walks down the k rows by plain 64-bit adds (BK rows per step);
// with segmented rows (kseg > 0) it hops by (segstride - kseg*ld) whenever it crosses a segment.
template <int NI, int PC, bool KS = true>
struct MNMajorLoader {
  const char* p[NI];  // current source address of this lane's chunk
  int t[NI];          // row index inside the current segment
  int64_t step, hop;  // bytes per BK rows; extra bytes when crossing a segment boundary
  int kseg;
  static constexpr int RPI = 64 / PC;  // k-rows per LDS-DMA instruction
  __device__ __forceinline__ void init(const __bf16* base, int64_t ld, int kseg_,
                                       int64_t segstride, int col0, int ncols, int wave,
                                       int lane) {
    kseg = kseg_;
    step = (int64_t)BK * ld * 2;
    hop = kseg > 0 ? (segstride - (int64_t)kseg * ld) * 2 : 0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int kr = (wave * NI + i) * RPI + lane / PC;
      const int swz = (kr & 3) | (((kr >> 3) & 1) << 2);
      const int c = (lane % PC) ^ (swz << 1);
      int cc = col0 + c * 8;
      const int nc8 = (ncols + 7) & ~7;  // rows are readable up to ncols rounded up to 8
      cc = cc <= nc8 - 8 ? cc : nc8 - 8;
      int seg = 0, tt = kr;
      if (kseg > 0) {
        seg = kr / kseg;
        tt = kr % kseg;
      }
      t[i] = tt;
      p[i] = (const char*)(base + cc) + ((int64_t)seg * segstride + (int64_t)tt * ld) * 2;
    }
  }
  __device__ __forceinline__ void issue(char* tile, int wave, int lane, int k0, int K) {
#pragma unroll
    for (int i = 0; i < NI; ++i) issue_one(tile, wave, lane, k0, K, i);
  }
  __device__ __forceinline__ void issue_one(char* tile, int wave, int lane, int k0, int K, int i) {
    const int kr = (wave * NI + i) * RPI + lane / PC;
    const void* src = (k0 + kr < K) ? (const void*)p[i] : (const void*)g_ca_zero_page;
    glds16(src, tile + (wave * NI + i) * 1024);
    p[i] += step;
    if (KS && kseg > 0) {
      t[i] += BK;
      while (t[i] >= kseg) {
        t[i] -= kseg;
        p[i] += hop;
      }
    }
  }
};

// LDS-DMA with the scalar-base addressing form: 16 B per lane from base + off (off: 32-bit, zero-extended) to the
// wave's 1-KiB LDS piece at byte address lds_piece (wave-uniform, goes through M0)
__device__ __forceinline__ void glds16_sbase(const char* base, uint32_t off, uint32_t lds_piece) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"
               :
               : "v"(off), "s"(base), "s"(lds_piece)
               : "memory", "m0");
}
// ---- loaders of kernel X: one wave-uniform base per operand tile + a 32-bit offset per lane and piece ----------
// The base walks down K by scalar adds; a full K-step issues its LDS-DMA without any per-lane address arithmetic or
// predicate.  Only the last, partial K-step (K % 64 != 0) selects the zero page per lane.  Rows / columns beyond
// the operand are clamped to its last one (their products are never stored).
template <int NI>
struct KMajorStream {  // operand stored [row][k], k contiguous; LDS image [rows][64 k], 128-B rows
  const char* base;    // wave-uniform: first row of the tile, current k
  uint32_t off[NI];    // byte offset of this lane's 16-B chunk
  int kc[NI];          // element offset of the chunk inside the K-step (tail predicate)
  __device__ __forceinline__ void init(const __bf16* b, int64_t ld, int row0, int nrows, int wave, int lane) {
    base = (const char*)(b + (int64_t)row0 * ld);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int r = (wave * NI + i) * 8 + (lane >> 3);
      const int c = (lane & 7) ^ ((r >> 1) & 7);
      int rr = row0 + r;
      rr = (rr < nrows ? rr : nrows - 1) - row0;
      kc[i] = c * 8;
      off[i] = (uint32_t)(((int64_t)rr * ld + c * 8) * 2);
    }
  }
  // one-byte elements (fp8): the same 128-B rows hold 128 k
  __device__ __forceinline__ void init_bytes(const char* b, int64_t ld, int row0, int nrows, int wave, int lane) {
    base = b + (int64_t)row0 * ld;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int r = (wave * NI + i) * 8 + (lane >> 3);
      const int c = (lane & 7) ^ ((r >> 1) & 7);
      int rr = row0 + r;
      rr = (rr < nrows ? rr : nrows - 1) - row0;
      kc[i] = c * 16;
      off[i] = (uint32_t)((int64_t)rr * ld + c * 16);
    }
  }
  __device__ __forceinline__ void issue_one(char* tile, int wave, int i) {
    glds16_sbase(base, off[i], (uint32_t)(uintptr_t)(lptr_t)(tile + (wave * NI + i) * 1024));
  }
  // partial K-step: chunks beyond K load some valid bytes instead (offset 0) and are zeroed in LDS by zero_fix()
  __device__ __forceinline__ void issue_one_tail(char* tile, int wave, int krem, int i) {
    glds16_sbase(base, kc[i] < krem ? off[i] : 0u, (uint32_t)(uintptr_t)(lptr_t)(tile + (wave * NI + i) * 1024));
  }
  // after this wave's LDS-DMA of the partial K-step has landed, before the barrier that publishes the tile
  __device__ __forceinline__ void zero_fix(char* tile, int wave, int lane, int krem) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
      if (kc[i] >= krem) *(uint4*)(tile + (wave * NI + i) * 1024 + lane * 16) = make_uint4(0, 0, 0, 0);
  }
  __device__ __forceinline__ void advance() { base += BK * 2; }
};
template <int NI, int PC>
struct MNMajorStream {  // operand stored [k][mn], mn contiguous (plain rows, no segments); LDS image [64 k][PC*8 mn]
  const char* base;     // wave-uniform: column col0 of row k0
  uint32_t off[NI];
  int64_t step;
  static constexpr int RPI = 64 / PC;  // k-rows per LDS-DMA instruction
  __device__ __forceinline__ void init(const __bf16* b, int64_t ld, int col0, int ncols, int wave, int lane) {
    base = (const char*)(b + col0);
    step = (int64_t)BK * ld * 2;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int kr = (wave * NI + i) * RPI + lane / PC;
      const int swz = (kr & 3) | (((kr >> 3) & 1) << 2);
      const int c = (lane % PC) ^ (swz << 1);
      int cc = col0 + c * 8;
      const int nc8 = (ncols + 7) & ~7;  // rows are readable up to ncols rounded up to 8
      cc = (cc <= nc8 - 8 ? cc : nc8 - 8) - col0;
      off[i] = (uint32_t)(((int64_t)kr * ld + cc) * 2);
    }
  }
  __device__ __forceinline__ void issue_one(char* tile, int wave, int i) {
    glds16_sbase(base, off[i], (uint32_t)(uintptr_t)(lptr_t)(tile + (wave * NI + i) * 1024));
  }
  __device__ __forceinline__ void issue_one_tail(char* tile, int wave, int lane, int krem, int i) {
    const int kr = (wave * NI + i) * RPI + lane / PC;
    glds16_sbase(base, kr < krem ? off[i] : 0u, (uint32_t)(uintptr_t)(lptr_t)(tile + (wave * NI + i) * 1024));
  }
  __device__ __forceinline__ void zero_fix(char* tile, int wave, int lane, int krem) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int kr = (wave * NI + i) * RPI + lane / PC;
      if (kr >= krem) *(uint4*)(tile + (wave * NI + i) * 1024 + lane * 16) = make_uint4(0, 0, 0, 0);
    }
  }
  __device__ __forceinline__ void advance() { base += step; }
};

// ---- fragment reads ----------------------------------------------------------------------
// KMAJOR tile: 16 rows starting at rb, k-step s (32 k): lane gets row rb+(lane&15),
// k = 32 s + 8 (lane>>4) .. +7.
// Issued as inline asm (completion through lds_wait): lets a kernel order its reads
// against its MFMA blocks by hand
__device__ __forceinline__ bf16x8_t frag_kmajor_async(const char* tile, int rb, int s, int lane) {
  const int r = rb + (lane & 15);
  const int c = (4 * s + (lane >> 4)) ^ ((r >> 1) & 7);
  const uint32_t a = (uint32_t)(uintptr_t)(lptr_t)(tile + r * 128 + c * 16);
  bf16x8_t v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(a));
  return v;
}
// MNMAJOR tile (row pitch PITCH bytes): 16 columns starting at cb (multiple of 16), k-step s:
// two transposed reads (k = 8g..8g+3 and 8g+4..8g+7 of the 32-k step).
// The reads are inline asm on purpose: hipcc treats the ds_read_tr builtin as a memory operation
// that may alias the LDS-DMA of the NEXT tile and puts `s_waitcnt vmcnt(0)` in front of it, which
// serialises the whole prefetch behind every fragment read (seen in the ISA of every MN-major
// variant).  The price: the compiler does not know when the data arrives, so every consumer must
// pass the fragments through lds_wait() first.
template <int PITCH>
__device__ __forceinline__ bf16x8_t frag_mnmajor(const char* tile, int cb, int s, int lane) {
  const int g = lane >> 4;
  const int q = (lane & 15) >> 2;
  const int p = lane & 3;
  const int kr = 32 * s + 8 * g + q;
  const int swz = q | ((g & 1) << 2);
  const int c = ((cb >> 3) + (p >> 1)) ^ (swz << 1);
  const uint32_t a0 = (uint32_t)(uintptr_t)(lptr_t)(tile + kr * PITCH + c * 16 + (p & 1) * 8);
  s16x4_t lo, hi;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(lo) : "v"(a0));
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(hi) : "v"(a0), "n"(4 * PITCH));
  typedef __attribute__((ext_vector_type(8))) short s16x8_t;
  s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, v);
}
// fragment reads with the stage / k-half / fragment folded into the immediate offset (completion through lds_wait)
template <int OFF>
__device__ __forceinline__ bf16x8_t lds_read_b128(uint32_t a) {
  static_assert(OFF >= 0 && OFF < 65536, "DS immediate offset");
  bf16x8_t v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(a), "n"(OFF));
  return v;
}
template <int OFF, int HI>
__device__ __forceinline__ bf16x8_t lds_read_tr(uint32_t a) {
  static_assert(OFF >= 0 && OFF + HI < 65536, "DS immediate offset");
  s16x4_t lo, hi;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(lo) : "v"(a), "n"(OFF));
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(hi) : "v"(a), "n"(OFF + HI));
  typedef __attribute__((ext_vector_type(8))) short s16x8_t;
  s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, v);
}
// all outstanding LDS reads have returned; the "+v" ties make every later use of f wait for it
__device__ __forceinline__ void lds_wait(bf16x8_t (&f)[4]) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]));
}

// XCD-aware tile rasterisation: gemm_plan.h (shared with the host's grid arithmetic).  The tile of block `bid` of this
// launch's own grid:
template <int SBM, int SBN>
__device__ __forceinline__ bool tile_of_block(int bid, int ntm, int ntn, int& tm, int& tn, bool bal = false) {
  return tile_of_block_g<SBM, SBN>(bid, (int)gridDim.x, ntm, ntn, tm, tn, bal);
}

// ---- epilogue --------------------------------------------------------------------------------
// Each wave parks its 64x64 fp32 tile in LDS (row pitch 68 floats: conflict-free b128 writes),
// then walks it 4 rows x 64 columns at a time in a rolled loop so the generic (runtime-selected)
// epilogue is emitted once and every row is stored as one contiguous 128-B (bf16) / 256-B (fp32)
// segment.  mw/nw: global row/column of the wave's tile origin.
// the 8 bias values of a lane's columns (nw: the wave tile's first column); requested early by the kernels that can
// spare the registers, so that the memory round trip is over when the epilogue starts
__device__ __forceinline__ void epi_load_bias(const CaGemmDesc& d, int lane, int nw, int z1, int z2, float (&bias8)[8]) {
  const int nb = nw + 8 * (lane & 7);
  const int nvalid = (d.N - nb) < 8 ? (d.N - nb) : 8;
#pragma unroll
  for (int e = 0; e < 8; ++e) bias8[e] = 0.f;
  if (d.bias && nvalid > 0) {
    const float* bz = d.bias + z1 * d.sBias1 + z2 * d.sBias2 + nb;
    if (nvalid == 8 && (((uintptr_t)bz) & 15) == 0) {
      const f32x4_t b0 = *(const f32x4_t*)bz, b1 = *(const f32x4_t*)(bz + 4);
#pragma unroll
      for (int e = 0; e < 8; ++e) bias8[e] = e < 4 ? b0[e] : b1[e - 4];
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (e < nvalid) bias8[e] = bz[e];
    }
  }
}
// CaGemmDesc.C8: eight consecutive activations as e4m3 with the delayed per-tensor scale; the lane's running max|v|
__device__ __forceinline__ void ca_store_fp8x8(unsigned char* dst, const float (&v)[8], float scale, float& amx) {
  float t[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    amx = fmaxf(amx, fabsf(v[e]));
    t[e] = fminf(fmaxf(v[e] * scale, -448.0f), 448.0f);
  }
  unsigned int w0 = 0, w1 = 0;
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(t[0], t[1], w0, false);
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(t[2], t[3], w0, true);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(t[4], t[5], w1, false);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(t[6], t[7], w1, true);
  *(uint2*)dst = make_uint2(w0, w1);
}

// ---- fast epilogue: a 64 x 64 wave tile that lies wholly inside the output, 16-byte aligned rows -------------------
// The general walk below decides everything per lane and per pass at run time (ragged columns, rows beyond M, which
// epilogue, unaligned dropout groups, both output types): ~400 vector instructions per pass of 8 elements per lane in
// the ISA, against ~130 of arithmetic - on the FFN GEMMs the epilogue's instruction count, not the stores' bytes, is
// what the tile waits for (3.3 VALU per MFMA over the whole kernel).  Interior wave tiles (all but the last row / column
// of tiles) take this form instead: the epilogue kind, the output type and dropout are template parameters, all
// predicates are gone, the flat element index of the dropout hash advances by a constant.  Same arithmetic in the same
// order as the general walk: the results are bit-identical (tests/test_kernels_gpu.py compares ragged and interior tiles
// of one launch against the same reference).
template <int EPI, bool F32, bool DROP>
__device__ __forceinline__ void gemm_epilogue_fast(const CaGemmDesc& d, const float* wt, int lane, int mw, int nb, int z,
                                                   int64_t zoffC, int64_t zoffR, const float (&bias8)[8], float& ssq,
                                                   float& amx) {
  const int M = d.M, N = d.N;
  const float alpha = d.alpha;
  const float keep_scale = DROP ? 1.f / (1.f - d.dropout_p) : 1.f;
  const int r0 = lane >> 3, c0 = 8 * (lane & 7);
  constexpr bool NEEDS_R = EPI == CA_EPI_RESIDUAL || EPI == CA_EPI_DGELU;
  const unsigned short* Rp = NEEDS_R ? (const unsigned short*)d.R + zoffR + nb + (int64_t)(mw + r0) * d.ldr : nullptr;
  const int64_t rstep = 8 * d.ldr;
  int64_t coff = zoffC + (int64_t)(mw + r0) * d.ldc + nb;
  const int64_t cstep = 8 * d.ldc;
  uint64_t idx = ((uint64_t)z * M + (mw + r0)) * (uint64_t)N + nb;  // multiple of 4: N % 8 == 0, nb % 8 == 0
  const uint64_t istep = 8ull * (uint64_t)N;
  u16x8_t r_next = {0, 0, 0, 0, 0, 0, 0, 0};
  if (NEEDS_R) r_next = *(const u16x8_t*)Rp;
  const bool c8_on = (EPI == CA_EPI_GELU || EPI == CA_EPI_DGELU) && d.C8 != nullptr;  // (wave-uniform)
  const float s8 = c8_on ? d.c8_scale[0] : 1.f;
  // dropout: the hash takes the group index (flat element index / 4) as two 32-bit words.  Where the wave tile does
  // not cross a multiple of 2^34 elements (wave-uniform test) the high word is a constant folded into the seed word
  // and the low word advances by a 32-bit add per pass - the same bits as ca_dropout_keep4 on the 64-bit index.
  // (the caller sends a wave tile that does cross such a multiple through the general walk: epi_drop32_ok)
  unsigned int dg = 0, ds_eff = 0, dthr = 0;
  if (DROP) {
    const uint64_t ilo = ((uint64_t)z * M + mw) * (uint64_t)N;
    const unsigned int sd = (unsigned int)d.dropout_seed * 0x9E3779B9u + (unsigned int)(d.dropout_seed >> 32);
    ds_eff = sd ^ ((unsigned int)(ilo >> 34) * 0x85EBCA6Bu);
    dg = (unsigned int)(idx >> 2);
    dthr = ca_dropout_threshold(d.dropout_p);
  }
  const unsigned int dgstep = (unsigned int)(istep >> 2);
#pragma unroll 2
  for (int it = 0; it < 8; ++it) {
    const u16x8_t r_cur = r_next;
    if (NEEDS_R && it < 7) r_next = *(const u16x8_t*)(Rp + (it + 1) * rstep);
    const float* wr = wt + (it * 8 + r0) * EPI_PITCH + c0;
    const f32x4_t a4 = *(const f32x4_t*)wr, b4 = *(const f32x4_t*)(wr + 4);
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (e < 4 ? a4[e] : b4[e - 4]) * alpha + bias8[e];
    unsigned int keep = 0xFFu;
    if (DROP) {
      keep = ca_dropout_keep4_lo(ds_eff, dg, dthr) | (ca_dropout_keep4_lo(ds_eff, dg + 1, dthr) << 4);
      dg += dgstep;
    }
    float v2[8];
    if (EPI == CA_EPI_GELU) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float g = gelu_erf(v[e]);
        if (DROP) g = ((keep >> e) & 1u) ? g * keep_scale : 0.f;
        v2[e] = g + 0.f;  // (the general walk adds the residual slot, zero here: -0 becomes +0 there too)
      }
    } else if (EPI == CA_EPI_RESIDUAL) {
      if (DROP) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = ((keep >> e) & 1u) ? v[e] * keep_scale : 0.f;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += bf2f(r_cur[e]);
    } else if (EPI == CA_EPI_DGELU) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float dg = dgelu_erf(bf2f(r_cur[e]));
        if (DROP) dg = ((keep >> e) & 1u) ? dg * keep_scale : 0.f;
        v[e] *= dg;
      }
    }
    if (F32) {
      float* C = (float*)d.C + coff;
      if (d.accumulate) {
        const f32x4_t c0v = *(const f32x4_t*)C, c1v = *(const f32x4_t*)(C + 4);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += e < 4 ? c0v[e] : c1v[e - 4];
      }
      if (d.c_stream_out) {
        __builtin_nontemporal_store((f32x4_t){v[0], v[1], v[2], v[3]}, (f32x4_t*)C);
        __builtin_nontemporal_store((f32x4_t){v[4], v[5], v[6], v[7]}, (f32x4_t*)(C + 4));
      } else {
        *(f32x4_t*)C = (f32x4_t){v[0], v[1], v[2], v[3]};
        *(f32x4_t*)(C + 4) = (f32x4_t){v[4], v[5], v[6], v[7]};
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) ssq = fmaf(v[e], v[e], ssq);
    } else {
      u16x8_t o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = f2bf(v[e]);
      if (d.c_stream_out)
        __builtin_nontemporal_store(o, (u16x8_t*)((unsigned short*)d.C + coff));
      else
        *(u16x8_t*)((unsigned short*)d.C + coff) = o;
      if (EPI == CA_EPI_NONE && d.c_sumsq != nullptr) {  // (wave-uniform) weight gradients kept in bf16: the norm of what is stored
#pragma unroll
        for (int e = 0; e < 8; ++e) ssq = fmaf(bf2f(o[e]), bf2f(o[e]), ssq);
      }
      if (EPI == CA_EPI_DGELU && c8_on) ca_store_fp8x8((unsigned char*)d.C8 + coff, v, s8, amx);
    }
    if (EPI == CA_EPI_GELU) {
      u16x8_t o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = f2bf(v2[e]);
      *(u16x8_t*)((unsigned short*)d.C2 + coff) = o;
      if (c8_on) ca_store_fp8x8((unsigned char*)d.C8 + coff, v2, s8, amx);
    }
    coff += cstep;
  }
}

// PARKED: the 64 x 64 staging tile `wave` already holds the accumulators (kernel M: two waves fill one tile)
// bias_pre: the lane's bias values where the kernel asked for them ahead of its main loop (epi_load_bias), else null.
// A kernel file whose every call of gemm_epilogue<false> leaves it null has that constant propagated into the body
// BEFORE the body is inlined, and its kernels compile to other code (same registers, other scalar allocation and size)
// than beside a caller that passes a bias (kernels L and X) - the one-file build these kernels were tuned in.  Such a
// file (gemm_s.hip, gemm_fp8.hip) keeps the function visible outside its code object with GEMM_EPILOGUE_KEEP_VISIBLE, at
// the price of one uncalled copy of it, and gets that build's code.
#define GEMM_EPILOGUE_KEEP_VISIBLE                                                                                      \
  template __attribute__((used)) __device__ void gemm_epilogue<false>(const CaGemmDesc&, f32x4_t (&)[4][4], char*, int, \
                                                                      int, int, int, int, int, int, const float (*)[8])
template <bool PARKED = false>
__device__ __forceinline__ void gemm_epilogue(const CaGemmDesc& d, f32x4_t (&acc)[4][4], char* smem,
                                              int wave, int lane, int mw, int nw, int z, int z1,
                                              int z2, const float (*bias_pre)[8] = nullptr) {
  // lane -> 8 consecutive columns of one row; 8 rows per pass, 8 passes; 16-byte bf16 stores
  const int M = d.M, N = d.N;
  const int64_t zoffC = z1 * d.sC1 + z2 * d.sC2;
  const int64_t zoffR = z1 * d.sR1 + z2 * d.sR2;
  const bool vec_ok = ((d.ldc & 7) == 0) && ((zoffC & 7) == 0) && ((d.ldr & 7) == 0) && ((zoffR & 7) == 0);
  const float keep_scale = d.dropout_p > 0.f ? 1.f / (1.f - d.dropout_p) : 1.f;
  const int nb = nw + 8 * (lane & 7);
  const int nvalid = (N - nb) < 8 ? (N - nb) : 8;
  const bool full = nvalid == 8 && vec_ok;
  const int epi = d.epilogue;
  const bool has_gelu = epi == CA_EPI_GELU || epi == CA_EPI_GELU_RESIDUAL;
  const bool needs_r = epi == CA_EPI_RESIDUAL || epi == CA_EPI_DGELU || epi == CA_EPI_GELU_RESIDUAL;
  // Everything the epilogue reads from global memory is requested BEFORE the accumulators go through LDS, and the R
  // row of pass it + 1 before pass it is computed: requested where they were used, the bias (8 dword loads per lane)
  // and each pass's R row put one exposed memory round trip each in front of the stores (+11 us for the bias and
  // +5..10 us for R on a 120-us launch at [3992 x 7680 x 1920]).
  float bias8[8];
  if (bias_pre) {
#pragma unroll
    for (int e = 0; e < 8; ++e) bias8[e] = (*bias_pre)[e];
  } else {
    epi_load_bias(d, lane, nw, z1, z2, bias8);
  }
  const unsigned short* Rbase = (const unsigned short*)d.R + zoffR + nb;
  auto load_r = [&](int it, u16x8_t& u) {  // R row of pass `it` (fast form only; ragged columns load in the pass)
    const int m = mw + it * 8 + (lane >> 3);
    if (needs_r && full && it < 8 && m < M) u = *(const u16x8_t*)(Rbase + (int64_t)m * d.ldr);
  };
  u16x8_t r_next = {0, 0, 0, 0, 0, 0, 0, 0};
  load_r(0, r_next);

  float* wt = (float*)smem + wave * (64 * EPI_PITCH);
  if (!PARKED) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        *(f32x4_t*)(wt + (i * 16 + (lane & 15)) * EPI_PITCH + j * 16 + 4 * (lane >> 4)) = acc[i][j];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // wave-private region: no barrier
  }
  const bool c8_on = d.C8 != nullptr && (epi == CA_EPI_GELU || epi == CA_EPI_DGELU);
  if (nvalid <= 0 && d.c_sumsq == nullptr && !c8_on) return;
  float ssq = 0.f;  // sum of squares of the fp32 values this lane stores (c_sumsq)
  float amx = 0.f;  // max |gelu| this lane stores (C8)
  const float s8 = c8_on ? d.c8_scale[0] : 1.f;
  // interior wave tile (wave-uniform test): the specialised walk above
  const bool drop_on = d.dropout_p > 0.f;
  // (dropout in the specialised walk: the 64 rows' flat element indices share their bits from 34 up)
  const bool drop32_ok = !drop_on || ((((uint64_t)z * M + mw) * (uint64_t)N) >> 34) == ((((uint64_t)z * M + mw + 64) * (uint64_t)N) >> 34);
  const bool interior = g_ca_epi_general == 0 && mw + 64 <= M && nw + 64 <= N && vec_ok && (N & 7) == 0 && d.C != nullptr && drop32_ok &&
                        (d.out_f32 || !d.accumulate) && (!has_gelu || (epi == CA_EPI_GELU && d.C2 != nullptr && !d.out_f32)) &&
                        !(d.out_f32 && epi != CA_EPI_NONE) && !(drop_on && epi == CA_EPI_NONE);
  if (interior) {
#define EPI_FAST(E, F, D) gemm_epilogue_fast<E, F, D>(d, wt, lane, mw, nb, z, zoffC, zoffR, bias8, ssq, amx)
    if (d.out_f32) {
      EPI_FAST(CA_EPI_NONE, true, false);
    } else if (epi == CA_EPI_NONE) {
      EPI_FAST(CA_EPI_NONE, false, false);
    } else if (epi == CA_EPI_GELU) {
      if (drop_on) EPI_FAST(CA_EPI_GELU, false, true); else EPI_FAST(CA_EPI_GELU, false, false);
    } else if (epi == CA_EPI_RESIDUAL) {
      if (drop_on) EPI_FAST(CA_EPI_RESIDUAL, false, true); else EPI_FAST(CA_EPI_RESIDUAL, false, false);
    } else {
      if (drop_on) EPI_FAST(CA_EPI_DGELU, false, true); else EPI_FAST(CA_EPI_DGELU, false, false);
    }
#undef EPI_FAST
  } else {
#pragma unroll 1
  for (int it = 0; it < 8; ++it) {
    const int ml = it * 8 + (lane >> 3);
    const int m = mw + ml;
    const u16x8_t r_cur = r_next;
    load_r(it + 1, r_next);
    if (m >= M || nvalid <= 0) continue;
    const f32x4_t a4 = *(const f32x4_t*)(wt + ml * EPI_PITCH + 8 * (lane & 7));
    const f32x4_t b4 = *(const f32x4_t*)(wt + ml * EPI_PITCH + 8 * (lane & 7) + 4);
    float v[8], v2[8], r[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      v[e] = (e < 4 ? a4[e] : b4[e - 4]) * d.alpha + bias8[e];
      v2[e] = 0.f;
      r[e] = 0.f;
    }
    const int64_t coff = zoffC + (int64_t)m * d.ldc + nb;
    if (needs_r) {
      if (full) {
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = bf2f(r_cur[e]);
      } else {
        const unsigned short* R = Rbase + (int64_t)m * d.ldr;
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (e < nvalid) r[e] = bf2f(R[e]);
      }
    }
    unsigned int keep = 0xFFu;
    if (d.dropout_p > 0.f && (has_gelu || epi == CA_EPI_DGELU || epi == CA_EPI_RESIDUAL)) {
      const uint64_t idx = ((uint64_t)z * M + m) * (uint64_t)N + nb;
      if ((idx & 3) == 0) {  // aligned group: two hashes for the 8 elements
        keep = ca_dropout_keep4(d.dropout_seed, idx, d.dropout_p) |
               (ca_dropout_keep4(d.dropout_seed, idx + 4, d.dropout_p) << 4);
      } else {
        keep = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) keep |= (ca_dropout_keep(d.dropout_seed, idx + e, d.dropout_p) ? 1u : 0u) << e;
      }
    }
    if (has_gelu) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float g = gelu_erf(v[e]);
        if (d.dropout_p > 0.f) g = ((keep >> e) & 1u) ? g * keep_scale : 0.f;
        v2[e] = g + r[e];  // r is zero unless GELU_RESIDUAL
      }
    } else if (epi == CA_EPI_RESIDUAL) {
      // C = R + dropout(alpha A.B + bias): hidden-state dropout on the sub-layer output before the residual add
      if (d.dropout_p > 0.f) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = ((keep >> e) & 1u) ? v[e] * keep_scale : 0.f;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += r[e];
    } else if (epi == CA_EPI_DGELU) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float dg = dgelu_erf(r[e]);
        if (d.dropout_p > 0.f) dg = ((keep >> e) & 1u) ? dg * keep_scale : 0.f;
        v[e] *= dg;
      }
    }
    if (d.out_f32) {
      float* C = (float*)d.C + coff;
      if (full) {
        if (d.accumulate) {
          const f32x4_t c0 = *(const f32x4_t*)C, c1 = *(const f32x4_t*)(C + 4);
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] += e < 4 ? c0[e] : c1[e - 4];
        }
        *(f32x4_t*)C = (f32x4_t){v[0], v[1], v[2], v[3]};
        *(f32x4_t*)(C + 4) = (f32x4_t){v[4], v[5], v[6], v[7]};
#pragma unroll
        for (int e = 0; e < 8; ++e) ssq = fmaf(v[e], v[e], ssq);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (e < nvalid) {
            const float t = d.accumulate ? C[e] + v[e] : v[e];
            C[e] = t;
            ssq = fmaf(t, t, ssq);
          }
      }
    } else if (d.C) {
      unsigned short* C = (unsigned short*)d.C + coff;
      if (full) {
        if (d.accumulate) {
          const u16x8_t c = *(const u16x8_t*)C;
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] += bf2f(c[e]);
        }
        u16x8_t o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = f2bf(v[e]);
        *(u16x8_t*)C = o;
        if (d.c_sumsq != nullptr) {
#pragma unroll
          for (int e = 0; e < 8; ++e) ssq = fmaf(bf2f(o[e]), bf2f(o[e]), ssq);
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (e < nvalid) {
            const unsigned short t = f2bf(d.accumulate ? bf2f(C[e]) + v[e] : v[e]);
            C[e] = t;
            ssq = fmaf(bf2f(t), bf2f(t), ssq);
          }
      }
    }
    if (has_gelu && d.C2) {
      unsigned short* C2 = (unsigned short*)d.C2 + coff;
      if (full) {
        u16x8_t o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = f2bf(v2[e]);
        *(u16x8_t*)C2 = o;
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (e < nvalid) C2[e] = f2bf(v2[e]);
      }
    }
    if (c8_on) {
      unsigned char* C8 = (unsigned char*)d.C8 + coff;
      float w8[8];  // the activation (GELU) or the gradient (GELU') this tile just formed
#pragma unroll
      for (int e = 0; e < 8; ++e) w8[e] = epi == CA_EPI_GELU ? v2[e] : v[e];
      if (full) {
        ca_store_fp8x8(C8, w8, s8, amx);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (e < nvalid) {
            amx = fmaxf(amx, fabsf(w8[e]));
            const float t = fminf(fmaxf(w8[e] * s8, -448.0f), 448.0f);
            C8[e] = (unsigned char)(__builtin_amdgcn_cvt_pk_fp8_f32(t, 0.f, 0u, false) & 0xffu);
          }
      }
    }
  }
  }  // general walk
  if (d.c_sumsq != nullptr) {
    // (every lane of the wave arrives here: fixed butterfly order, the same bits on every run)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ssq += __shfl_xor(ssq, o, 64);
    if (lane == 0 && mw < M && nw < N) d.c_sumsq[(int64_t)(mw >> 6) * ((N + 63) >> 6) + (nw >> 6)] = ssq;
  }
  if (c8_on && d.c8_amax != nullptr) {
    // (every lane of the wave arrives here; a maximum does not depend on the order: the same bits on every run)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amx = fmaxf(amx, __shfl_xor(amx, o, 64));
    // (spread over the accumulator's words: the 15 000 wave tiles of a 12 000 x 5 120 output on one address took 200 us)
    if (lane == 0 && amx > 0.f)
      atomicMax((unsigned int*)d.c8_amax + (((mw >> 6) * 7 + (nw >> 6)) & (CA_FP8_AMAX_SLOTS - 1)), __float_as_uint(amx));
  }
}

// grp.count > 1: a grouped launch of up to X_GROUP_MAX independent problems of the same operand form
// (ca_gemm_bf16_group): block ranges map to problems, each with plain row-major tile numbering.
#define X_GROUP_MAX 8
struct CaGemmGroup {
  CaGemmDesc d[X_GROUP_MAX];
  int first[X_GROUP_MAX];  // first tile of problem i in the group's tile list (first[0] = 0)
  int count;     // number of problems (0 = plain launch of d[0])
  int total;     // tiles in the group
  // Persistent form (vgrid > gridDim.x): the launch has one workgroup per CU; the workgroups of XCD x (blockIdx & 7)
  // take the virtual blocks x, x + 8, x + 16, ... - the first one each statically, the following ones in the order the
  // workgroups become free, through one counter per XCD (cnt[x], zero between launches: the last pull resets it).
  int vgrid;      // blocks of the virtual grid (= gridDim.x in the one-tile-per-workgroup form)
  unsigned* cnt;  // 8 counters, or null
  // Persistent form beside another resident kernel (an RCCL ring kernel during the backward of an N > 1 run): some of the
  // launch's workgroups only start when others have EXITED - i.e. after every dynamic block is taken - and a static
  // first block would then cost one whole tile time at the end of the launch.  dyn_first: every block, the first
  // included, comes from the counter; a workgroup that finds it exhausted exits at once (ca_gemm_set_compute_cus).
  int dyn_first;
};

// ---- launching -------------------------------------------------------------------------------------------------------
// One launcher per kernel file: it holds the family's instantiation table and is the only place that names one.
typedef void (*DescKernel)(const CaGemmDesc);
typedef void (*GroupKernel)(const CaGemmGroup);
int gemm_launch_s(const GemmPlan& p, const CaGemmDesc& d, hipStream_t s, const char* who);       // gemm_s.hip: S and M
int gemm_launch_l(const GemmPlan& p, const CaGemmDesc& d, hipStream_t s, const char* who);       // gemm_l.hip
int gemm_launch_x(const GemmPlan& p, CaGemmGroup& g, hipStream_t s, const char* who);            // gemm_x.hip
int gemm_launch_skinny(const GemmPlan& p, const CaGemmDesc& d, hipStream_t s, const char* who);  // gemm_skinny.hip
int gemm_launch_fp8(const GemmPlan& p, const CaGemmDesc& d, hipStream_t s, const char* who);     // gemm_fp8.hip
// g_ca_epi_general of the file's own code object: each file has a one-thread kernel of its own name that stores it
// (plain functions and kernels on purpose: inline ones in this header would be merged by the linker and reach one copy)
hipError_t gemm_set_epi_general_s(int on);
hipError_t gemm_set_epi_general_l(int on);
hipError_t gemm_set_epi_general_x(int on);
hipError_t gemm_set_epi_general_fp8(int on);
// the setters' common part: complete when it returns, like the hipMemcpyToSymbol of a single copy would be
inline hipError_t gemm_run_epi_general_setter(void (*kernel)(int), int on) {
  hipLaunchKernelGGL(kernel, dim3(1), dim3(1), 0, 0, on);
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? e : hipDeviceSynchronize();
}
// host stub of kernel X's NT form (gemm_x.hip; for hipFuncGetAttributes)
const void* gemm_x_nt_kernel();

// Events of the launch being profiled (gemm.hip, ca_prof_begin), else null.  While profiling, the kernel is launched with
// start/stop events attached to the dispatch itself (hipExtLaunchKernelGGL): they carry the kernel's own begin/end
// timestamps, like rocprofv3's kernel trace, instead of the gaps between stream operations.
extern hipEvent_t g_gemm_prof_e0, g_gemm_prof_e1;
template <class Arg>
int gemm_launch(void (*kernel)(const Arg), dim3 grid, const GemmPlan& p, hipStream_t s, const char* who, const Arg& arg) {
  if (g_gemm_prof_e0)
    hipExtLaunchKernelGGL(kernel, grid, dim3(p.block), p.lds, s, g_gemm_prof_e0, g_gemm_prof_e1, 0, arg);
  else
    hipLaunchKernelGGL(kernel, grid, dim3(p.block), p.lds, s, arg);
  CA_CHECK_LAUNCH(who);
  return CA_OK;
}

// Dynamic LDS beyond the default limit is allowed per kernel: the limit of every kernel of a family is raised at the
// family's first launch on a device.  raised: the family's bit per device; kernel_of: the host stub of a table entry,
// or null for an entry that does not need it.
template <class T, class KernelOf>
int gemm_allow_lds(std::atomic<uint64_t>& raised, const T* table, int n, KernelOf kernel_of, size_t bytes, const char* who) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  const uint64_t bit = dev < 64 ? uint64_t(1) << dev : 0;  // (devices beyond the mask: every launch)
  if (raised.load(std::memory_order_relaxed) & bit) return CA_OK;
  for (int i = 0; i < n; ++i)
    if (const void* k = kernel_of(table[i])) {
      const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
      if (e != hipSuccess) {
        ca_set_error("%s: cannot raise the kernel's LDS limit to %zu bytes: %s", who, bytes, hipGetErrorString(e));
        return CA_ERR_LAUNCH;
      }
    }
  raised.fetch_or(bit, std::memory_order_relaxed);
  return CA_OK;
}
template <class K>
int gemm_allow_lds(std::atomic<uint64_t>& raised, K* const* kernels, int n, size_t bytes, const char* who) {
  return gemm_allow_lds(raised, kernels, n, [](K* k) { return (const void*)k; }, bytes, who);
}
