// Fused (flash-style) multi-head attention for gfx950: forward and backward without ever writing the
// [T, T] score / probability matrices to HBM.  Replaces SDPA at
// $TF/models/wav2vec2/modeling_wav2vec2.py:438-463,529-543 and $TF/models/whisper/modeling_whisper.py:215-238.
//
// Shapes: Q [B, Tq, *] / K, V [B, Tk, *] bf16 with row strides ldq / ldk / ldv and head h at column
// offset h*hd (so q, k, v can live in one fused [B*T, 3d] projection output); head_dim hd is any
// multiple of 8 up to 128 (64, 80 and 120 on this path).
//
// Structure (all three kernels): one 256-thread workgroup = 4 waves x 16 rows (queries or keys); the
// rows of the *other* side stream through LDS in tiles staged by global_load_lds (two images per tile
// where needed: a K-major one read with ds_read_b128 for the Q.K^T / dO.V^T products and an MN-major one
// read with ds_read_b64_tr_b16 for the products that contract over the tile's rows).  Score tiles are
// computed in the orientation whose accumulator registers ARE the next MFMA's A operand (the rows of a
// 32-row step are permuted so that a lane group ends up with 8 consecutive contraction indices), so
// probabilities never leave registers.  The forward is one pass with a running maximum (online softmax);
// the backward kernels recompute probabilities from the saved log-sum-exp.
//
// This header: what the kernel files (attn_fwd.hip, attn_decode.hip, attn_bwd.hip) share - LDS images, fragment
// readers, tile loaders, output staging, the kernel arguments - and the launchers attention.hip calls.  Which kernel a
// descriptor gets is decided in attn_plan.h.
#pragma once
#include "common.h"
#include "attn_plan.h"
#include <type_traits>

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
typedef __attribute__((ext_vector_type(8))) short s16x8_t;

// (one copy per kernel file - every translation unit is its own code object - and still a symbol with external linkage:
// as a `static` the single-query kernels compile to other code)
inline __device__ __attribute__((aligned(16))) uint32_t g_attn_zero_page[4];

__device__ __forceinline__ void glds16a(const void* g, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)lds_wave_base, 16, 0, 0);
}

// ---- LDS images -----------------------------------------------------------------------------------
// K-major image: [HDPV/64 chunks][ROWS][64 dims], 128-B rows, 16-B chunk index XOR ((row>>1)&7).
// NW = number of waves that share the load (4 = the whole workgroup, 1 = a wave-private image)
// Chunk swizzle of the K-major images: the 16-byte chunk c of row r sits at position c ^ kswz(r) of its 128-byte row.
// Two read patterns share an image: operand rows (ds_read_b128 of row 32 s + 8 (r >> 2) + 4 bb + (r & 3), chunk 4 ks + g:
// the instruction's four lane groups are NOT contiguous - {0-3, 12-15, 20-27}, ... (MI355X_MICROARCH.md, LDS) - so one
// group holds 16 rows of two lane groups g) and transposed reads (ds_read_b64_tr_b16 of rows 8 g + q, two 32-lane
// groups, each lane pair a chunk pair).  kswz = (r0, r0 ^ r1, r3) is one of the XOR-linear maps of the row bits for
// which a bank simulation of every read of a step, with the hardware's lane groups, finds no conflict at all
// (tools/archive/dev_lds_swizzle.py); the round-1 map (r >> 1) & 7 cost an extra LDS cycle on every read of either kind
// (SQ_LDS_BANK_CONFLICT = 49 % of SQ_LDS_IDX_ACTIVE in dQ and dK|dV).  LDS-DMA writes are linear and do not care.
// MN-major images ([rows][HDPV dims], read only transposed): XOR value of the chunk index of row kr.  A 32-lane group of
// ds_read_b64_tr_b16 covers rows 8 g + q (q = 0..3, g in {0, 1}) of a 32-row block, each lane pair a chunk PAIR: the
// four even rows need four distinct values of bits 1-2 (and bit 3 where a row has 16 chunks).  With 8 chunks per row
// (head_dim <= 64) the round-1 form (2 q | 8 (g & 1)) & 7 lost the g bit: two-way conflicts on every value-fragment read
// of the forward kernels (SQ_LDS_BANK_CONFLICT 37 % of SQ_LDS_IDX_ACTIVE).
template <int PC>
__device__ __forceinline__ int mnswz(int kr) {
  if (PC == 8) return (((kr >> 1) & 1) << 1) | (((kr >> 3) & 1) << 2);
  return ((((kr & 3) | (((kr >> 3) & 1) << 2))) << 1) & (PC - 1);
}
__device__ __forceinline__ int kswz(int r) { return (r & 1) | (((r ^ (r >> 1)) & 1) << 1) | (((r >> 3) & 1) << 2); }
template <int ROWS, int HDPV, int NW = 4>
__device__ __forceinline__ void load_kmajor_image(char* lds, const unsigned short* base, int64_t ld,
                                                  int row0, int nrows, int hd, int wave, int lane) {
  constexpr int NCH = HDPV / 64;
  constexpr int IPW = ROWS / 8 / NW;  // instructions per wave per chunk (ROWS*128 B / 1 KiB / NW waves)
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int i = 0; i < IPW; ++i) {
      const int inst = wave * IPW + i;
      const int r = inst * 8 + (lane >> 3);
      const int cc = (lane & 7) ^ kswz(r);
      const int dim = c * 64 + cc * 8;
      int row = row0 + r;
      row = row < nrows ? row : nrows - 1;
      const void* src = dim < hd ? (const void*)(base + (int64_t)row * ld + dim) : (const void*)g_attn_zero_page;
      glds16a(src, lds + c * ROWS * 128 + inst * 1024);
    }
}
// MN-major image: [ROWS][HDPV dims], chunk index XOR ((swz(row) << 1) & (PC-1)); rows >= nrows are zero.
template <int ROWS, int HDPV, int NW = 4>
__device__ __forceinline__ void load_mnmajor_image(char* lds, const unsigned short* base, int64_t ld,
                                                   int row0, int nrows, int hd, int wave, int lane) {
  constexpr int PC = HDPV / 8;
  constexpr int RPI = 64 / PC;
  constexpr int IPW = ROWS * HDPV * 2 / 1024 / NW;
#pragma unroll
  for (int i = 0; i < IPW; ++i) {
    const int inst = wave * IPW + i;
    const int kr = inst * RPI + lane / PC;
    const int c = (lane % PC) ^ mnswz<PC>(kr);
    const int dim = c * 8;
    const int row = row0 + kr;
    const void* src = (row < nrows && dim < hd) ? (const void*)(base + (int64_t)row * ld + dim)
                                                : (const void*)g_attn_zero_page;
    glds16a(src, lds + inst * 1024);
  }
}
template <int ROWS>
__device__ __forceinline__ bf16x8_t kimg_frag(const char* img, int row, int ks, int lane) {
  const int cc = (4 * (ks & 1) + (lane >> 4)) ^ kswz(row);
  return *(const bf16x8_t*)(img + (ks >> 1) * ROWS * 128 + row * 128 + cc * 16);
}
// rows 32*s + 8g + {0..7} of the image x 16 columns starting at 16*nb, transposed into a B operand
template <int HDPV>
__device__ __forceinline__ bf16x8_t timg_frag(const char* img, int s, int nb, int lane) {
  constexpr int PC = HDPV / 8;
  constexpr int PITCH = HDPV * 2;
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const int kr = 32 * s + 8 * g + q;
  const int c = ((2 * nb) + (p >> 1)) ^ mnswz<PC>(kr);
  const char* a0 = img + kr * PITCH + c * 16 + (p & 1) * 8;
  s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(lptr_t)a0);
  s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4_t*)(lptr_t)(a0 + 4 * PITCH));
  s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, v);
}
// The same B operand (rows 32*s + 8g + {0..7} x 16 columns starting at 16*nb, transposed) read out of a K-MAJOR
// image, so a tile that is needed in both orientations is staged once.  The K-major swizzle leaves a 2-way bank
// conflict on these reads (rows r and r+2 of a lane group share banks), which costs less than a second image:
// half the LDS-DMA instructions and half the LDS bytes per step.
template <int ROWS>
__device__ __forceinline__ bf16x8_t timg_frag_k(const char* img, int s, int nb, int lane) {
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const int r0 = 32 * s + 8 * g + q, r1 = r0 + 4;
  const int c = 2 * (nb & 3) + (p >> 1);
  const char* base = img + (nb >> 2) * ROWS * 128 + (p & 1) * 8;
  const char* a0 = base + r0 * 128 + ((c ^ kswz(r0)) * 16);
  const char* a1 = base + r1 * 128 + ((c ^ kswz(r1)) * 16);
  s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(lptr_t)a0);
  s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(lptr_t)a1);
  s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, v);
}
// inline-asm variants: hipcc orders the ds_read_tr builtin behind every outstanding LDS-DMA (s_waitcnt vmcnt(0)),
// which would serialise a prefetch of the next tile behind these reads.  The caller must run lds_wait_all() and
// tie() the fragments before using them.
__device__ __forceinline__ bf16x8_t tr_pair_async(const char* a0, const char* a1) {
  s16x4_t lo, hi;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(lo) : "v"((uint32_t)(uintptr_t)(lptr_t)a0));
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(hi) : "v"((uint32_t)(uintptr_t)(lptr_t)a1));
  s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, v);
}
template <int ROWS>
__device__ __forceinline__ bf16x8_t timg_frag_k_async(const char* img, int s, int nb, int lane) {
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const int r0 = 32 * s + 8 * g + q, r1 = r0 + 4;
  const int c = 2 * (nb & 3) + (p >> 1);
  const char* base = img + (nb >> 2) * ROWS * 128 + (p & 1) * 8;
  return tr_pair_async(base + r0 * 128 + ((c ^ kswz(r0)) * 16), base + r1 * 128 + ((c ^ kswz(r1)) * 16));
}
template <int HDPV>
__device__ __forceinline__ bf16x8_t timg_frag_async(const char* img, int s, int nb, int lane) {
  constexpr int PC = HDPV / 8;
  constexpr int PITCH = HDPV * 2;
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const int kr = 32 * s + 8 * g + q;
  const int c = ((2 * nb) + (p >> 1)) ^ mnswz<PC>(kr);
  const char* a0 = img + kr * PITCH + c * 16 + (p & 1) * 8;
  return tr_pair_async(a0, a0 + 4 * PITCH);
}
__device__ __forceinline__ void lds_wait_all() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void tie(bf16x8_t& f) { asm volatile("" : "+v"(f)); }

// ---- fast-path tile loads ---------------------------------------------------------------------------------------
// A tile that lies fully inside its tensor and is not the tensor's last needs no row clamp, and its columns beyond
// head_dim may hold whatever follows in memory (the neighbouring head or the next row: finite activations that only
// ever meet the zero-padded register operand or land in output columns that are never stored).  Its per-lane byte
// offsets relative to the tile's first row are then constants of the kernel and only a wave-uniform base moves from
// tile to tile: one LDS-DMA instruction per 1-KiB piece, no per-lane address arithmetic (the general loaders above
// spend ~20 vector instructions per piece on row clamps, zero-page selects and 64-bit multiplies).  The last tile of
// a tensor always takes the general loader (rows beyond the end, and no read past the allocation).
__device__ __forceinline__ const char* uniform_ptr(const void* p) {  // a wave-uniform pointer the compiler cannot prove uniform
  const uint64_t v = (uint64_t)(uintptr_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  // SGPRs written by a VALU instruction (v_readfirstlane) need five wait states before a VMEM instruction reads them,
  // and the LDS-DMA below is inline asm the hazard recogniser does not see: pass the pair through a scalar move, whose
  // result carries no such hazard
  uint64_t r;
  asm volatile("s_mov_b64 %0, %1" : "=s"(r) : "s"(((uint64_t)hi << 32) | lo));
  return (const char*)(uintptr_t)r;
}
__device__ __forceinline__ void glds16_sb(const char* base, uint32_t off, uint32_t lds_piece) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(off), "s"(base), "s"(lds_piece) : "memory", "m0");
}
template <int ROWS, int HDPV, int NW = 4>
struct KImgFast {
  static constexpr int NCH = HDPV / 64, IPW = ROWS / 8 / NW;
  uint32_t off[NCH * IPW];
  __device__ __forceinline__ void init(int64_t ld, int wave, int lane) {
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int i = 0; i < IPW; ++i) {
        const int r = (wave * IPW + i) * 8 + (lane >> 3);
        const int cc = (lane & 7) ^ kswz(r);
        off[c * IPW + i] = (uint32_t)((r * ld + c * 64 + cc * 8) * 2);
      }
  }
  __device__ __forceinline__ void issue(char* lds, const unsigned short* tile_base, int wave) const {
    const uint32_t l0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lptr_t)lds);
    const char* tb = uniform_ptr(tile_base);
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int i = 0; i < IPW; ++i)
        glds16_sb(tb, off[c * IPW + i], l0 + c * ROWS * 128 + (wave * IPW + i) * 1024);
  }
};
template <int ROWS, int HDPV, int NW = 4>
struct MnImgFast {
  static constexpr int PC = HDPV / 8, RPI = 64 / PC, IPW = ROWS * HDPV * 2 / 1024 / NW;
  uint32_t off[IPW];
  __device__ __forceinline__ void init(int64_t ld, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < IPW; ++i) {
      const int kr = (wave * IPW + i) * RPI + lane / PC;
      const int c = (lane % PC) ^ mnswz<PC>(kr);
      off[i] = (uint32_t)((kr * ld + c * 8) * 2);
    }
  }
  __device__ __forceinline__ void issue(char* lds, const unsigned short* tile_base, int wave) const {
    const uint32_t l0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lptr_t)lds);
    const char* tb = uniform_ptr(tile_base);
#pragma unroll
    for (int i = 0; i < IPW; ++i) glds16_sb(tb, off[i], l0 + (wave * IPW + i) * 1024);
  }
};
// number of leading tiles of `rows_per_tile` rows that are fully inside a tensor of n rows and are not its last tile
__device__ __forceinline__ int fast_tiles(int n, int rows_per_tile) { return (n - 1) / rows_per_tile; }

// ---- wave-private output staging: 16 rows x HDPV columns, accumulator layout -> 16-byte row stores --------------
// o[nb][e] is element (row 4g + e, column 16 nb + r) of the wave's 16-row tile.  Stored straight from the registers
// that is one 2-byte store per lane and element (32 branches + stores per lane for 128 columns, 32-byte segments);
// through LDS the tile goes out as whole 16-byte chunks of rows.
// dst8 (optional): the same rows also as e4m3 bytes of the bf16-rounded values times scale8 (delayed per-tensor scale,
// CaAttnDesc.O8) with the lane's running max |value| in amx.
template <int HDPV>
__device__ __forceinline__ void store_tile16(char* st, const f32x4_t (&o)[HDPV / 16], const float (&rs)[4],
                                             unsigned short* dst, int64_t ld, int row0, int nrows, int hd, int lane,
                                             unsigned char* dst8 = nullptr, float scale8 = 1.f, float* amx = nullptr) {
  constexpr int PITCH = HDPV * 2 + 16;  // bytes: consecutive rows start 4 banks apart
  const int g = lane >> 4, r = lane & 15;
#pragma unroll
  for (int nb = 0; nb < HDPV / 16; ++nb)
#pragma unroll
    for (int e = 0; e < 4; ++e)
      *(unsigned short*)(st + (4 * g + e) * PITCH + (16 * nb + r) * 2) = f2bf(o[nb][e] * rs[e]);
  __builtin_amdgcn_wave_barrier();
  constexpr int CPR = HDPV / 8;  // 16-byte chunks per row
#pragma unroll
  for (int i = 0; i < 16 * CPR / 64; ++i) {
    const int idx = i * 64 + lane;
    const int row = idx / CPR, ch = idx % CPR;
    const int q = row0 + row;
    if (q < nrows && ch * 8 < hd) {
      const u16x8_t v = *(const u16x8_t*)(st + row * PITCH + ch * 16);
      *(u16x8_t*)(dst + (int64_t)q * ld + ch * 8) = v;
      if (dst8) {  // (wave-uniform)
        float t[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float f = bf2f(v[e]);
          *amx = fmaxf(*amx, fabsf(f));
          t[e] = fminf(fmaxf(f * scale8, -448.0f), 448.0f);
        }
        unsigned int w0 = 0, w1 = 0;
        w0 = __builtin_amdgcn_cvt_pk_fp8_f32(t[0], t[1], w0, false);
        w0 = __builtin_amdgcn_cvt_pk_fp8_f32(t[2], t[3], w0, true);
        w1 = __builtin_amdgcn_cvt_pk_fp8_f32(t[4], t[5], w1, false);
        w1 = __builtin_amdgcn_cvt_pk_fp8_f32(t[6], t[7], w1, true);
        *(uint2*)(dst8 + (int64_t)q * ld + ch * 8) = make_uint2(w0, w1);
      }
    }
  }
}
constexpr int attn_stage_bytes(int hdpv) { return 4 * 16 * (hdpv * 2 + 16); }

// row of a 32-row step that lane-row r of block bb must read so that lane group g ends up holding the
// contraction indices 8g .. 8g+7 (bb = 0: +0..3, bb = 1: +4..7)
__device__ __forceinline__ int rowperm(int bb, int r) { return 8 * (r >> 2) + 4 * bb + (r & 3); }

__device__ __forceinline__ bf16x8_t pack8(const float (&v)[8]) {
  s16x8_t o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (short)f2bf(v[e]);
  return __builtin_bit_cast(bf16x8_t, o);
}
__device__ __forceinline__ bf16x8_t load_rowfrag(const unsigned short* base, int64_t ld, int row, int ks,
                                                 int lane, int hd) {
  const int dim = 32 * ks + 8 * (lane >> 4);
  if (dim < hd) return *(const bf16x8_t*)(base + (int64_t)row * ld + dim);
  s16x8_t z = {0, 0, 0, 0, 0, 0, 0, 0};
  return __builtin_bit_cast(bf16x8_t, z);
}

struct AttnArgs {
  const unsigned short *Q, *K, *V;
  int64_t ldq, ldk, ldv, sqb, skb, svb;  // row strides and per-batch strides (elements)
  unsigned short* O;                     // forward output / backward: saved O is not needed (Dq given)
  int64_t ldo, sob;
  unsigned char* O8;                     // forward, wide kernels: the output also as e4m3 (CaAttnDesc.O8) or null
  const float* o8_scale;
  unsigned int* o8_amax;
  float* lse;                            // [B, H, Tqp]
  const int32_t* klen;                   // [B] or null
  const int32_t* key_slot;               // [B, Tk] or null: small-query kernel, the cache row of each key (CaAttnDesc.key_slot)
  const int32_t* row_off;                // [B + 1] or null: packed rows (CaAttnDesc.row_off, attn_packed_rows)
  int B, H, Tq, Tk, hd, Tqp, causal;
  int Tqd, Tkd;                          // strides of the dropout hash: the launch's Tq / Tk (attn_drop_index)
  float scale;
  // backward
  const unsigned short* dO;
  int64_t lddo, sdob;
  const float* Dq;                       // [B, H, Tqp] rowsum(dO * O)
  unsigned short *dQ, *dK, *dV;
  int64_t lddq, lddk, lddv, sdqb, sdkb, sdvb;
  // dropout on the attention probabilities (training): keep decision of (b, h, q, k) from (seed, flat index)
  float drop_p;
  uint64_t drop_seed;
  // small-query kernel only: the keys of one (clip, head) dealt to nsplit workgroups (CaAttnDesc.split_ws): partial
  // (max, normaliser, unnormalised output) slabs + one arrival counter per (clip, head); nsplit <= 1 = off
  int nsplit;
  CaKeySplit split;         // (nsplit > 1: how the grid's workgroups map to (clip, head) and part)
  float* split_slab;        // [B * H][nsplit][16][SPLIT_ROW]
  unsigned int* split_cnt;  // [B * H], zero between launches
  // greedy decoding with the query projection inside the kernel (attn_fwd_smallq_kernel<.., true>, ca_decode_attn_qproj):
  // q[b, h, :] = (LayerNorm(x[b]) Wq[h*hd : (h+1)*hd, :]^T + bq) - one query per clip
  const unsigned short* qp_x;   // [B, qp_d] residual-stream rows
  int64_t qp_ldx;
  const float *qp_gamma, *qp_beta, *qp_bias;
  const unsigned short* qp_W;   // [H*hd, qp_d] row-major
  int64_t qp_ldw;
  int qp_d;
  float qp_eps;
  const int32_t* kstart;        // [B] or null: the KM forward instantiations, first key of each row (CaAttnDesc.kstart)
};
// A per-row first key (CaAttnDesc.kstart) is a shift of the row's keys: the K / V base moves kstart[b] rows on and the key
// counts shrink by as much, so the loops, masks and tile loaders of a kernel stay what they are and run in shifted key
// indices (a causal compare then takes the query index shifted too: attn_kstart_shift's return value).  Keys in front of
// kstart[b] are never loaded; a row left without keys runs no tile and stores zeros.  Workgroup-uniform.
__device__ __forceinline__ int attn_kstart_shift(const AttnArgs& a, int b, const unsigned short*& K, const unsigned short*& V,
                                                 int& Tk, int& kl) {
  int ks = a.kstart[b];
  ks = ks < 0 ? 0 : (ks > kl ? kl : ks);
  K += (int64_t)ks * a.ldk;
  V += (int64_t)ks * a.ldv;
  Tk -= ks;
  kl -= ks;
  return ks;
}
// Flat index of probability (b, h, q, key): rows are padded to a multiple of 4 keys so that 4 consecutive keys from a
// multiple of 4 share one hash (ca_dropout_keep4); the backward kernels regenerate the forward's decisions from it.
__device__ __forceinline__ uint64_t attn_drop_index(const AttnArgs& a, int b, int h, int q, int key) {
  const uint64_t tkp = (uint64_t)((a.Tkd + 3) & ~3);
  return (((uint64_t)b * a.H + h) * (uint64_t)a.Tqd + (uint64_t)q) * tkp + (uint64_t)key;
}
// Packed rows (CaAttnDesc.row_off): the utterances of a batch lie end to end, utterance b at rows row_off[b] ..
// row_off[b + 1] of every tensor.  A workgroup turns its copy of the arguments into those of ITS utterance - base
// pointers moved to its first row, Tq = Tk = its length - so every bound, clamp, tile count, fast-tile count and store
// predicate below is the utterance's: no load and no store touches a neighbour's rows (the general tile loaders clamp
// to the utterance's last row, the fast ones only take tiles that are not its last).  lse / Dq stay [B, H, Tqp] indexed
// by the local query, and the dropout hash keeps the launch's Tq / Tk as strides (Tqd / Tkd): an utterance draws the
// probability mask of the padded run.  All of it is workgroup-uniform (scalar registers).
__device__ __forceinline__ void attn_packed_rows(AttnArgs& a, int b) {
  if (!a.row_off) return;
  const int64_t r0 = a.row_off[b];
  const int len = a.row_off[b + 1] - (int)r0;
  a.Q += r0 * a.ldq; a.K += r0 * a.ldk; a.V += r0 * a.ldv; a.O += r0 * a.ldo;
  a.dO += r0 * a.lddo; a.dQ += r0 * a.lddq; a.dK += r0 * a.lddk; a.dV += r0 * a.lddv;
  a.sqb = a.skb = a.svb = a.sob = a.sdob = a.sdqb = a.sdkb = a.sdvb = 0;
  a.Tq = a.Tk = len;
}

#define NEG_INF (-__builtin_inff())
#define LOG2E 1.44269504088896340736f
#define NEG_BIG (-1.0e30f)
template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// this workgroup's (tile, head, clip) under the XCD-aware placement of attn_plan.h
__device__ __forceinline__ bool attn_tile_of_block(int ntile, int H, int B, int& tile, int& h, int& b) {
  return attn_tile_of(blockIdx.x, ntile, H, B, tile, h, b);
}

// ---- launching -------------------------------------------------------------------------------------------------------
// One launcher per kernel file: a switch over the plan's instantiation, the only place that names one.
int attn_launch_fwd(const AttnPlan& p, const AttnArgs& a, hipStream_t s, const char* who);     // attn_fwd.hip
int attn_launch_decode(const AttnPlan& p, const AttnArgs& a, hipStream_t s, const char* who);  // attn_decode.hip
int attn_launch_bwd(const AttnPlan& p, const AttnArgs& a, hipStream_t s, const char* who);     // attn_bwd.hip

template <class... KArgs, class... Args>
int attn_launch(void (*kernel)(KArgs...), const AttnPlan& p, hipStream_t s, const char* who, const Args&... args) {
  hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.block), p.lds, s, args...);
  CA_CHECK_LAUNCH(who);
  return CA_OK;
}
inline int attn_no_kernel(const AttnPlan& p, const char* who) {
  ca_set_error("%s: no attention kernel for plan (kernel %d, hdpv %d, drop %d, wpe %d, dt %d, qp %d, ks %d)", who, p.kernel,
               p.hdpv, p.drop, p.wpe, p.dt, p.qp, p.ks);
  return CA_ERR_LAUNCH;
}
