// Kernel choice and launch geometry of the GEMM family (gemm.hip and the gemm_*.hip kernel files), as plain C++17: which kernel a descriptor gets and
// with what grid, block and LDS size is decided here, without touching the device, so that the rule can be compiled
// and tested by the host compiler alone (tests/test_gemm_plan_cpu.py).  gemm.hip validates and plans; the launcher of the plan's kernel file launches.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/coral_amd.h"

#if defined(__HIPCC__)
#define CA_PLAN_FN __host__ __device__ __forceinline__
#else
#define CA_PLAN_FN inline
#endif

// tile shapes and dynamic LDS sizes of the kernels (the layouts behind the byte counts are described in each kernel's file)
#define BM 128  // kernels S and M
#define BN 128
#define BK 64
#define LBM 256  // kernel L
#define LBN 128
#define XBM 256  // kernel X
#define XBN 256
#define EPI_PITCH 68  // floats; epilogue staging row pitch (272 B)
#define LDS_BYTES (4 * 64 * EPI_PITCH * 4)    // kernel S: 69632 >= its two operand stages
#define M_LDS_BYTES (2 * 4 * BM * BK * 2)     // kernel M: 131072, four stages of two operand tiles
#define L_LDS_BYTES (3 * (LBM + LBN) * BK * 2)  // kernel L: 147456, three stages
#define X_LDS_BYTES (8 * 64 * EPI_PITCH * 4)  // kernel X: 139264 >= 2 stages * 64 KiB
#define X_LAUNCH_LDS (X_LDS_BYTES + 64)       // bf16 kernel X: + the word pair that carries a persistent workgroup's next block
#define SKINNY_LN_PAD 32  // bf16 elements between LDS rows beyond K: 64 B, lanes r and r + 1 then sit 16 banks apart

// XCD-aware tile rasterisation.  Workgroups are dealt round-robin over the 8 XCDs (blocks b and
// b+8 share an L2), and the tiles that are resident together on one XCD should share operand
// panels: they stream the same K-slices at about the same time, so each slice is pulled across
// the fabric once per XCD and served to the other tiles from that XCD's 4-MiB L2.  The grid is
// cut into super-blocks of SBM x SBN tiles (= the number of tiles one XCD holds at once); the
// i-th workgroup of XCD x works on tile (i % (SBM*SBN)) of super-block (i / (SBM*SBN))*8 + x.
// Placement only affects speed: any dispatch order gives the same result.
// Small / medium grids: the tile grid is cut into exactly 8 rectangular blocks, one per XCD (bm x bn blocks with
// bm * bn = 8, the split that minimises block height + width = the operand bands an XCD has to stream).
// xcd_split returns bm; the block is hb x wb tiles.
CA_PLAN_FN int xcd_split(int ntm, int ntn, int& hb, int& wb) {
  int best = 1, cost = 1 << 30;
#pragma unroll
  for (int bm = 1; bm <= 8; bm *= 2) {
    const int bn = 8 / bm;
    const int c = (ntm + bm - 1) / bm + (ntn + bn - 1) / bn;
    if (c < cost) {
      cost = c;
      best = bm;
    }
  }
  hb = (ntm + best - 1) / best;
  wb = (ntn + 8 / best - 1) / (8 / best);
  return best;
}
// Tile `l` of a grid in run order: the shorter grid dimension runs fastest, so a run of consecutive tiles covers a
// compact band of the grid.
CA_PLAN_FN void run_tile(int l, int ntm, int ntn, int& tm, int& tn) {
  if (ntn <= ntm) {
    tm = l / ntn;
    tn = l % ntn;
  } else {
    tn = l / ntm;
    tm = l % ntm;
  }
}
// The rectangular split leaves XCDs unevenly loaded when the grid does not divide (5 x 5 tiles: 6, 6, 3, 0, 4, 4, 2,
// 0 per XCD): where it would pad by more than a quarter, each XCD takes a run of ceil(T / 8) consecutive tiles.
// bal (CaGemmDesc.xcd_balanced, set by the library beside a resident collective): always runs - every XCD gets
// ceil(T / 8) tiles.  The rectangular split may hand one XCD exactly its 32 CUs' worth of a 240-tile grid (32, 32, ...,
// 24, 24): with two CUs of an XCD held by another kernel that XCD runs a second round and the launch takes twice as long.
CA_PLAN_FN bool xcd_use_runs(int ntm, int ntn, int hb, int wb, bool bal = false) {
  return bal || 8 * hb * wb * 4 > ntm * ntn * 5;
}
CA_PLAN_FN int xcd_grid(int ntm, int ntn, bool bal = false) {
  if (ntm * ntn <= 8) return ntm * ntn;  // a handful of tiles (batched attention-sized problems): plain numbering
  int hb, wb;
  xcd_split(ntm, ntn, hb, wb);
  if (xcd_use_runs(ntm, ntn, hb, wb, bal)) return 8 * ((ntm * ntn + 7) / 8);
  return 8 * hb * wb;
}
// tile of block `bid` under that split (false = padding block)
CA_PLAN_FN bool xcd_tile(int bid, int ntm, int ntn, int& tm, int& tn, bool bal = false) {
  if (ntm * ntn <= 8) {
    tm = bid / ntn;
    tn = bid % ntn;
    return true;
  }
  int hb, wb;
  const int bm = xcd_split(ntm, ntn, hb, wb);
  const int bn = 8 / bm;
  const int x = bid & 7, idx = bid >> 3;
  if (xcd_use_runs(ntm, ntn, hb, wb, bal)) {
    const int l = x * ((ntm * ntn + 7) / 8) + idx;
    run_tile(l, ntm, ntn, tm, tn);
    return l < ntm * ntn;
  }
  const int bi = x / bn, bj = x % bn;
  tm = bi * hb + idx / wb;
  tn = bj * wb + idx % wb;
  return tm < ntm && tn < ntn;
}
// tile of block `bid` of a (virtual) grid of `grid` blocks: persistent workgroups walk a grid larger than the launch
template <int SBM, int SBN>
CA_PLAN_FN bool tile_of_block_g(int bid, int grid, int ntm, int ntn, int& tm, int& tn, bool bal = false) {
  if (grid == xcd_grid(ntm, ntn, bal)) {
    // small problem (fewer than 4 super-blocks per XCD): one rectangular block of tiles per XCD, so an L2 only
    // streams the operand bands of its block.  (Plain round-robin numbering gave each XCD one tile COLUMN: all of
    // A streamed into every L2, 8x the bytes in the PMC counters.)
    return xcd_tile(bid, ntm, ntn, tm, tn, bal);
  }
  const int x = bid & 7, i = bid >> 3;
  const int per = SBM * SBN;
  const int sb = (i / per) * 8 + x, t = i % per;
  const int nsbn = (ntn + SBN - 1) / SBN;
  const int sbm = sb / nsbn, sbn = sb % nsbn;
  tm = sbm * SBM + (t % SBM);
  tn = sbn * SBN + (t / SBM);
  return tm < ntm && tn < ntn;
}
template <int SBM, int SBN>
CA_PLAN_FN unsigned tile_grid(int ntm, int ntn, bool bal = false) {
  if (ntm * ntn < 4 * 8 * SBM * SBN) return (unsigned)xcd_grid(ntm, ntn, bal);  // fewer than 4 super-blocks per XCD
  const int nsb = ((ntm + SBM - 1) / SBM) * ((ntn + SBN - 1) / SBN);
  return (unsigned)(((nsb + 7) / 8) * 8 * SBM * SBN);
}

// ---- tuning values -------------------------------------------------------------------------------------------------
// The environment knobs (read once, gemm_knobs() in gemm.hip) and the per-process settings the rule depends on.
struct GemmKnobs {
  int x_persist = 1;         // CA_X_PERSIST: 0 = one workgroup per tile in kernel X
  int skinny_mb1 = 4;        // CA_SKINNY_MB1: 16-row skinny workgroups up to this many workgroups per CU; 0 = 32-row ones
  int skinny_mb1_rows = 16;  // CA_SKINNY_MB1_ROWS: ... for problems with more rows than this
  int skinny_nt = 0;         // CA_SKINNY_NT: 4 / 8 / 16 pins the columns per skinny workgroup
  int skinny_u = 0;          // CA_SKINNY_U: 8 / 16 / 32 pins the k-steps in flight per skinny wave
  int prefer_l = 3;          // CA_GEMM_PREFER_L: kernel L's tile-count window in rounds; 0 = off
  int l_over_x = 0;          // CA_GEMM_L_OVER_X: 1 / 2 / 3 hand shapes that X fills to L (tuning)
  int l_min = 100;           // CA_GEMM_L_MIN: fewest tiles for kernel L
  int m_max = 256;           // CA_GEMM_M: most tiles for kernel M; 0 = off
  int force_kernel = 0;      // ca_gemm_force_kernel: 0 auto, 1 S, 2 L, 3 X, 5 M (tests / tuning)
  int compute_cus = 0;       // ca_gemm_set_compute_cus: CUs left beside a resident kernel, 0 = all
  unsigned device_cus = 256; // the device's CU count, rounded down to a multiple of 8
};
// CUs the tiled kernels count on (256 on MI355X; fewer beside a resident collective: ca_gemm_set_compute_cus)
inline unsigned gemm_compute_cus(const GemmKnobs& k) {
  if (k.compute_cus <= 0) return k.device_cus;
  const unsigned c = (unsigned)(k.compute_cus >= 8 ? (k.compute_cus / 8) * 8 : 8);
  return c < k.device_cus ? c : k.device_cus;
}

// ---- the plan: everything a launch needs ---------------------------------------------------------------------------
enum GemmFamily { GEMM_SKINNY = 0, GEMM_S = 1, GEMM_M = 2, GEMM_L = 3, GEMM_X = 4 };
enum GemmPlanError { GEMM_PLAN_OK = 0, GEMM_PLAN_LN_NOT_SKINNY = 1, GEMM_PLAN_ROWS_NOT_SKINNY = 2 };
struct GemmPlan {
  int error = GEMM_PLAN_OK;  // form-specific descriptor features asked of a form that does not have them
  int family = GEMM_S;
  int fp8 = 0;  // the fp8 form's kernels (families S and X only)
  int lay = 0;  // a_layout * 2 + b_layout
  int ks = 0;   // segmented-K variant (kernels S and X)
  int mb = 0, nch = 0, u = 0, nt = 0;  // skinny: template arguments MB, NCH, U, NT
  unsigned grid_x = 1, grid_y = 1, grid_z = 1, block = 256;
  size_t lds = 0;  // dynamic LDS bytes
  // kernel X: blocks of the virtual grid, one workgroup per CU pulling them (grid_x < vgrid), every block pulled
  unsigned vgrid = 0;
  int persistent = 0, dyn_first = 0;
  int kind = 0;  // the profiler's kernel index: S, M and skinny 0, L 1, X 2 (-1: the fp8 form is not profiled)
};
inline int gemm_x_tiles(const CaGemmDesc& d) { return ((d.M + XBM - 1) / XBM) * ((d.N + XBN - 1) / XBN); }

// Launch geometry of kernel X.  Default: persistent workgroups (one per CU) with dynamic tile pulls whenever the tile
// grid is larger than the chip and un-batched; CA_X_PERSIST=0 restores one workgroup per tile.
inline void gemm_plan_x_geometry(GemmPlan& p, unsigned vgrid, unsigned nbz, const GemmKnobs& k) {
  const unsigned ncu = gemm_compute_cus(k);
  p.family = GEMM_X;
  p.kind = 2;
  p.vgrid = vgrid;
  p.dyn_first = k.compute_cus > 0 ? 1 : 0;
  p.persistent = (k.x_persist && nbz == 1 && vgrid > ncu) ? 1 : 0;
  p.grid_x = p.persistent ? ncu : vgrid;
  p.grid_z = nbz;
  p.block = 512;
  p.lds = X_LAUNCH_LDS;
}

// Skinny M (greedy decoding: one token per clip): weight streaming without LDS staging.
// (33 .. 128 rows take it when the caller asks for what only this form has - the K|V-cache row scatter of a decoded
// token - or when the problem is too narrow to give the tiled kernels a grid: N < 8192 means <= 64 tiles of 128 x 128)
inline bool gemm_takes_skinny(const CaGemmDesc& d, const GemmKnobs& k) {
  const bool skinny_wide = d.M > 32 && d.M <= 128 && d.C8 == nullptr && d.c_sumsq == nullptr &&
                           (d.a_ln_gamma || d.c_row_index || d.c_split_n > 0 || d.N <= 8192 || d.M <= 64);
  return k.force_kernel == 0 && (d.M <= 32 || skinny_wide) && d.a_layout == CA_KMAJOR && d.b_layout == CA_KMAJOR &&
         d.batch1 == 1 && d.batch2 == 1 && d.a_kseg == 0 && d.b_kseg == 0 && d.dropout_p == 0.f &&
         d.epilogue != CA_EPI_DGELU;
}
inline void gemm_plan_skinny(GemmPlan& p, const CaGemmDesc& d, const GemmKnobs& k) {
  p.family = GEMM_SKINNY;
  p.kind = 0;
  unsigned gy = d.M <= 32 ? 1u : (unsigned)((d.M + 31) / 32);  // row blocks of 32 (blockIdx.y)
  // 17 .. 128 rows: 16-row workgroups over blockIdx.y wherever that leaves the launch at most four workgroups per CU
  // (every projection of a decoder layer; not the vocabulary).  The kernel's pace is set by the requests its waves keep
  // in flight, not by bytes: at 32 clips the 32-row form (one workgroup per column block, two row blocks against the
  // same weight fragment - round 3) gave N = 1024 launches 64 workgroups; 16-row workgroups re-read the weights from
  // L2 but double the waves: 3.06 -> 2.66 ms per token at 32 clips, 4.50 -> 3.90 at 64, 6.96 -> 6.60 at 128 (round 5;
  // 64-row workgroups, the opposite direction, measured 4.40 at 64).  Same K split per output element: same bits.
  // CA_SKINNY_MB1=0 restores 32-row workgroups.
  const bool rows16 = k.skinny_mb1 && d.M > k.skinny_mb1_rows && d.M > 16 &&
                      (unsigned)((d.N + 15) / 16) * gy <= (unsigned)k.skinny_mb1 * k.device_cus;
  if (rows16) gy = (unsigned)((d.M + 15) / 16);
  // columns per workgroup (round 6): the widest of 16 / 8 / 4 that still gives the launch 3/4 of a workgroup per CU
  // (16-row workgroups only; CA_SKINNY_NT=16 restores sixteen everywhere)
  int nt = 16;
  if (d.M <= 16 || rows16) {
    const unsigned want = 3u * k.device_cus / 4u;
    if ((unsigned)((d.N + 15) / 16) * gy < want) nt = (unsigned)((d.N + 7) / 8) * gy >= want ? 8 : 4;
    if (k.skinny_nt == 4 || k.skinny_nt == 8 || k.skinny_nt == 16) nt = k.skinny_nt;
  }
  p.grid_x = (unsigned)((d.N + nt - 1) / nt);
  p.grid_y = gy;
  p.block = 256;
  p.mb = (d.M <= 16 || rows16) ? 1 : 2;  // (33 .. 128 rows: 32- or 16-row blocks over blockIdx.y)
  p.nt = nt;
  p.u = 8;
  if (d.a_ln_gamma) {
    p.nch = (d.K + 511) / 512 <= 2 ? 2 : (d.K + 511) / 512;
    p.lds = (size_t)4 * p.mb * 256 * sizeof(float) + (size_t)16 * p.mb * (d.K + SKINNY_LN_PAD) * 2;
    return;
  }
  p.lds = (size_t)4 * p.mb * 256 * sizeof(float);
  if (p.mb == 1) {
    // k-steps in flight per wave: its whole K quarter up to 32 (K = 4096: one round of loads instead of four;
    // CA_SKINNY_U=8 restores eight)
    const int per = ((d.K + 31) / 32 + 3) / 4;
    p.u = per <= 8 ? 8 : (per <= 16 ? 16 : 32);
    if (k.skinny_u == 8 || k.skinny_u == 16 || k.skinny_u == 32) p.u = k.skinny_u;
  }
}

// Which tiled kernel: the X fill rule, the L window, the tenant cost model and the M gate, in that order.
// The 256x128 pipelined kernel runs one workgroup per CU, so it needs enough tiles to fill the chip; small or heavily
// batched problems use the 128x128 kernel.
inline int gemm_tiled_family(const CaGemmDesc& d, const GemmKnobs& k) {
  const int force = k.force_kernel;
  const int lay = (d.a_layout ? 2 : 0) + (d.b_layout ? 1 : 0);
  const bool ks = d.a_kseg > 0 || d.b_kseg > 0;
  const int64_t nb = (int64_t)d.batch1 * d.batch2;
  const int64_t tiles_l = (int64_t)((d.M + LBM - 1) / LBM) * ((d.N + LBN - 1) / LBN) * nb;
  // Measured on MI355X (profiles/r01_gemm_shapes.txt): at the path's shapes (K = 1920..7680, M = 3992)
  // the 128x128 kernel with two workgroups per CU equals or beats the 256x128 one-per-CU kernel,
  // because its second workgroup hides the epilogue; the L kernel is kept selectable for tuning.
  bool use_l = force == 2 && !ks;
  // Kernel X (256x256): only where it fills the chip -- at least ~0.7 tiles per CU in its last round.
  const int xtm = (d.M + XBM - 1) / XBM, xtn = (d.N + XBN - 1) / XBN;
  const int64_t xt = (int64_t)xtm * xtn * nb;
  const int64_t cus = (int64_t)gemm_compute_cus(k);
  const double xwaves = (double)xt / (double)cus;
  const double xeff = xwaves / (double)((xt + cus - 1) / cus);                         // last-wave occupancy
  const double xfill = ((double)d.M * d.N) / ((double)xtm * XBM * (double)xtn * XBN);  // tile padding waste
  // The MN-major x MN-major (weight-gradient) form gains most from the 256x256 tile (1.0 PFLOP/s against 0.63
  // for S inside the training step), so it switches at a lower fill than the other forms.
  const bool tn = d.a_layout == CA_MNMAJOR && d.b_layout == CA_MNMAJOR;
  // (thresholds from tools/dev_gemm_rule.py on the models' shapes: X wins from ~73 % occupancy of its last round
  // - 188 / 192 / 564 tiles - and loses at 68 % - 368 tiles)
  bool use_x = force == 0 && d.K >= 512 && xt >= 160 && xeff * xfill >= (tn ? 0.60 : 0.70);
  if (force == 3 || d.a_colsum) use_x = true;  // the column sums live in kernel X only
  // Kernel L (256x128, three-stage ring) takes the shapes kernel X does not fill and that give it 160 .. 768 tiles
  // (0.4 .. 3 rounds of one workgroup per CU; CA_GEMM_L_MIN, default 100 tiles: from there it also beats the 128x128
  // kernel on the d = 1024 models, XLS-R-300M step 19.95 -> 19.1 ms): the N = d projections and data gradients and q|k|v at the 2B shape.  Its
  // two-tiles-ahead LDS-DMA keeps it fed under the optimiser's HBM traffic, where the 128x128 kernel (one tile ahead)
  // loses 25 %: XLS-R-2B step 79.2 -> 76.5 ms on one box (tools/archive/exp_l3.sh).  CA_GEMM_PREFER_L=0 turns it off, a larger
  // value widens the tile-count window (x 256).
  const int lox = k.l_over_x;
  if (k.prefer_l && force == 0 && !ks && d.K >= 512 && tiles_l >= k.l_min &&
      (tiles_l <= cus * k.prefer_l || (use_x && lox)) && !d.a_colsum &&
      (!use_x || (lox == 1 && !tn) || lox == 2 || (lox == 3 && lay == 0))) {
    use_l = true;
    use_x = false;
  }
  const int ntm = (d.M + BM - 1) / BM, ntn = (d.N + BN - 1) / BN;
  const int64_t ts = (int64_t)ntm * ntn;
  // Beside a resident kernel that holds some CUs (ca_gemm_set_compute_cus(n), n below the chip's count) the rules above -
  // tuned for exactly 256 CUs - pick single-round tilings that then run TWO rounds (240 tiles on 224 CUs).  There the
  // choice is made by counting rounds on the CUs that are left: cost = rounds x tile work / the shape's efficiency, in
  // units of one 128 x 128 tile's work (kernel S: two tiles per CU at a time; efficiencies from
  // profiles/r05_gemm_shapes.txt, weight-gradient form in brackets): X 4 / 1.0, L 2 / 0.93 [0.85], S 2 / 0.8 [0.6] per
  // pair, M 1 / 0.6.
  if (force == 0 && k.compute_cus > 0 && cus < (int64_t)k.device_cus && nb == 1 && !ks && d.K >= 512 && !d.a_colsum &&
      d.M > 128) {
    auto rounds = [](int64_t tiles, int64_t slots) { return (double)((tiles + slots - 1) / slots); };
    const double cx = rounds(xt, cus) * 4.0, cl = rounds(tiles_l, cus) * 2.0 / (tn ? 0.85 : 0.93),
                 cs = rounds(ts, 2 * cus) * 2.0 / (tn ? 0.6 : 0.8), cm = rounds(ts, cus) * 1.0 / 0.6;
    int family = GEMM_X;
    double best = cx;
    if (cl < best) { best = cl; family = GEMM_L; }
    if (cs < best) { best = cs; family = GEMM_S; }
    if (cm < best) { best = cm; family = GEMM_M; }
    return family;
  }
  if (use_x) return GEMM_X;
  if (use_l) return GEMM_L;
  // at most one tile per CU: kernel M (two waves per SIMD on the same tile; CA_GEMM_M=0 switches it off)
  if (!ks && (force == 5 || (force == 0 && ts * nb <= k.m_max && d.K >= 2 * BK))) return GEMM_M;
  return GEMM_S;
}

inline GemmPlan gemm_plan_bf16(const CaGemmDesc& d, const GemmKnobs& k) {
  GemmPlan p;
  p.lay = (d.a_layout ? 2 : 0) + (d.b_layout ? 1 : 0);
  p.ks = (d.a_kseg > 0 || d.b_kseg > 0) ? 1 : 0;
  if (gemm_takes_skinny(d, k)) {
    gemm_plan_skinny(p, d, k);
    return p;
  }
  if (d.a_ln_gamma) p.error = GEMM_PLAN_LN_NOT_SKINNY;
  else if (d.c_row_index || d.c_split_n != 0) p.error = GEMM_PLAN_ROWS_NOT_SKINNY;
  if (p.error) return p;
  // (xcd_balanced: every XCD gets the same number of tiles whenever the chip is shared with a resident kernel)
  const bool bal = k.compute_cus > 0;
  const unsigned nb = (unsigned)((int64_t)d.batch1 * d.batch2);
  p.family = gemm_tiled_family(d, k);
  p.grid_z = nb;
  switch (p.family) {
    case GEMM_X:
      gemm_plan_x_geometry(p, tile_grid<4, 8>((d.M + XBM - 1) / XBM, (d.N + XBN - 1) / XBN, bal), nb, k);
      break;
    case GEMM_L:
      p.kind = 1;
      p.grid_x = tile_grid<4, 8>((d.M + LBM - 1) / LBM, (d.N + LBN - 1) / LBN, bal);
      p.block = 512;
      p.lds = L_LDS_BYTES;
      break;
    default:  // S and M share the 128 x 128 tile grid
      p.kind = 0;
      p.grid_x = tile_grid<8, 8>((d.M + BM - 1) / BM, (d.N + BN - 1) / BN, bal);
      p.block = p.family == GEMM_M ? 512 : 256;
      p.lds = p.family == GEMM_M ? M_LDS_BYTES : LDS_BYTES;
      break;
  }
  return p;
}

// fp8 form: the 256 x 256 kernel where it fills the chip (the bf16 rule on a fixed 256 CUs), else the 128 x 128 one;
// ca_gemm_force_kernel(1 / 3) pins either for tests
inline GemmPlan gemm_plan_fp8(const CaGemmDesc& d, const GemmKnobs& k) {
  GemmPlan p;
  p.fp8 = 1;
  p.kind = -1;
  const int xtm = (d.M + XBM - 1) / XBM, xtn = (d.N + XBN - 1) / XBN;
  const int64_t xt = (int64_t)xtm * xtn;
  const double xeff = ((double)xt / 256.0) / (double)((xt + 255) / 256);
  const double xfill = ((double)d.M * d.N) / ((double)xtm * XBM * (double)xtn * XBN);
  if (k.force_kernel == 3 || (k.force_kernel == 0 && d.K >= 512 && xt >= 160 && xeff * xfill >= 0.70)) {
    p.family = GEMM_X;
    p.grid_x = tile_grid<4, 8>(xtm, xtn);
    p.block = 512;
    p.lds = X_LDS_BYTES;
  } else {
    p.family = GEMM_S;
    p.grid_x = tile_grid<8, 8>((d.M + BM - 1) / BM, (d.N + BN - 1) / BN);
    p.block = 256;
    p.lds = LDS_BYTES;
  }
  return p;
}

// Grouped launch of kernel X (ca_gemm_bf16_group): XCD x takes the x-th run of ceil(total / 8) tiles of the group's tile
// list, so the grid is the total padded to 8; one problem alone keeps the plain launch's numbering.
inline GemmPlan gemm_plan_group(const CaGemmDesc* descs, int count, const GemmKnobs& k) {
  GemmPlan p;
  p.lay = (descs->a_layout ? 2 : 0) + (descs->b_layout ? 1 : 0);
  int total = 0;
  for (int i = 0; i < count; ++i) total += gemm_x_tiles(descs[i]);
  const unsigned vgrid = count > 1 ? (unsigned)(8 * ((total + 7) / 8))
                                   : tile_grid<4, 8>((descs->M + XBM - 1) / XBM, (descs->N + XBN - 1) / XBN);
  gemm_plan_x_geometry(p, vgrid, 1, k);
  return p;
}
