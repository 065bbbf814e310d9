// Alignment counts of reference / hypothesis token strings (coral_amd/error_rates.py): hits, substitutions, deletions and
// insertions of the minimum-edit-distance alignment with the fewest insertions, for a ragged batch of pairs.
//
// No back-pointers: the rule is a shortest path under the lexicographic order on (distance, insertions),
//   C[0][j] = (j, j),  C[i][0] = (i, 0),
//   C[i][j] = lexmin(C[i-1][j-1] + (r != h, 0),  C[i-1][j] + (1, 0),  C[i][j-1] + (1, 1)),
// and from (d, I) = C[n][m]:  D = I - (m - n),  S = d - I - D,  H = n - S - D.  A key is the one number d * one + I with
// one above every insertion count, so the plain minimum is the lexicographic one (edit_cell below holds the only
// comparison).  Exact integers, no atomics: bit-identical from run to run.
//
// One kernel, one grid for all pairs.  A workgroup has CA_EDIT_WG_WAVES waves and takes the pairs b, b + G, b + 2G, ...
// of the launch order (b its index, G the grid size), so the largest pairs of a largest-first order land on different
// workgroups:
//   wave route       a pair with both sides <= CA_EDIT_WAVE_MAX goes to one wave.  The hypothesis columns are striped over
//                    the 64 lanes, CPL = 1, 2, 4, 8 or 16 columns per lane in registers (the smallest that covers m); lane
//                    l works on row t - l + 1 at step t.  The reference token and the cell left of a lane's stripe come
//                    from lane l - 1 by a DPP wave shift (one VALU move each, no LDS); lane 0 takes the boundary (i, 0) and
//                    the next token, which the wave loads 64 at a time and reads with v_readlane.  32-bit integer keys.
//   workgroup route  any longer pair (or every pair with route = 2) goes to the whole workgroup, one after the other.  The
//                    hypothesis is cut into panels of CA_EDIT_PANEL columns, 8 per thread; inside a panel it is the same
//                    skewed sweep over 256 threads, a wave's last lane handing its cell and token to the next wave through
//                    LDS (double-buffered, one barrier per step).  The panel's right boundary column is kept in the
//                    workspace (two columns of n + 1 keys per pair, written and read alternately; a pair's columns start
//                    behind those of the workgroup-route pairs before it in the launch order).  Keys held as doubles.
// Columns behind m hold the token -1, which no reference token equals, and lie right of column m, so they reach nothing
// that C[n][m] depends on.
#include "common.h"

#define CA_EDIT_WG_WAVES 4
#define CA_EDIT_WG_THREADS (CA_EDIT_WG_WAVES * CA_WAVE)
#define CA_EDIT_CPT (CA_EDIT_PANEL / CA_EDIT_WG_THREADS)
static_assert(CA_EDIT_CPT * CA_EDIT_WG_THREADS == CA_EDIT_PANEL, "a panel is a whole number of columns per thread");
static_assert(CA_EDIT_WAVE_MAX <= 16 * CA_WAVE, "the wave route holds at most 16 columns per lane");
static_assert(2 * CA_EDIT_WAVE_MAX + CA_WAVE < (1 << 15), "32-bit keys: distance and insertions in 16 bits each");
static_assert(CA_EDIT_MAX_TOKENS + CA_EDIT_PANEL < (1 << 22), "double keys: insertions (of padding columns too) below one = 2^22");

// A key is distance * one + insertions in one number.  The wave route's fit 32 bits (one = 2^16).  The workgroup route's
// need 41 bits and are held as doubles (one = 2^22; every value is an integer below 2^44, so the sums are exact): a
// 64-bit integer minimum is a compare and two selects, v_min_f64 is one full-rate instruction.
template <typename K>
struct EditKey;
template <>
struct EditKey<uint32_t> {
  static constexpr uint32_t one = 1u << 16;
  static __device__ __forceinline__ uint32_t make(int d, int ins) { return ((uint32_t)d << 16) | (uint32_t)ins; }
  static __device__ __forceinline__ uint32_t least(uint32_t a, uint32_t b) { return a < b ? a : b; }
};
template <>
struct EditKey<double> {
  static constexpr double one = 4194304.0;
  static __device__ __forceinline__ double make(int d, int ins) { return (double)d * one + (double)ins; }
  static __device__ __forceinline__ double least(double a, double b) { return __builtin_fmin(a, b); }
};

// One cell of the recurrence.  THE TIE RULE: among equal distances the smaller key has the fewest insertions - this
// minimum is the one place to change it.
template <typename K>
__device__ __forceinline__ K edit_cell(K diag, K up, K left, bool differ) {
  const K one = EditKey<K>::one;
  const K sub = diag + (differ ? one : K(0));
  const K del = up + one;
  const K ins = left + (one + K(1));
  return EditKey<K>::least(EditKey<K>::least(sub, del), ins);
}

// lane l takes v of lane l - 1; lane 0 takes `inject` (DPP wave_shr:1, one v_mov)
__device__ __forceinline__ int edit_lane_up(int inject, int v) {
  return __builtin_amdgcn_update_dpp(inject, v, 0x138, 0xf, 0xf, false);
}
__device__ __forceinline__ double edit_lane_up(double inject, double v) {
  const uint64_t a = __builtin_bit_cast(uint64_t, inject), b = __builtin_bit_cast(uint64_t, v);
  const int lo = edit_lane_up((int)(uint32_t)a, (int)(uint32_t)b);
  const int hi = edit_lane_up((int)(uint32_t)(a >> 32), (int)(uint32_t)(b >> 32));
  return __builtin_bit_cast(double, ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
__device__ __forceinline__ double edit_read_lane(double v, int l) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), l);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ void edit_store_counts(int32_t* out, int64_t d, int64_t ins, int n, int m) {
  const int64_t del = ins - ((int64_t)m - n);
  const int64_t sub = d - ins - del;
  out[0] = (int32_t)(n - sub - del);
  out[1] = (int32_t)sub;
  out[2] = (int32_t)del;
  out[3] = (int32_t)ins;
}

// ---- wave route: 1 <= n, m <= CA_EDIT_WAVE_MAX, m <= 64 * CPL ----
template <int CPL>
__device__ __forceinline__ void edit_wave_sweep(const int32_t* __restrict__ ref, int n, const int32_t* __restrict__ hyp,
                                                int m, int lane, int32_t* out) {
  typedef uint32_t K;
  const int j0 = lane * CPL;  // this lane's columns are j0 + 1 .. j0 + CPL
  K prev[CPL];
  int h[CPL];
#pragma unroll
  for (int c = 0; c < CPL; ++c) {
    const int j = j0 + c + 1;
    h[c] = j <= m ? hyp[j - 1] : -1;
    prev[c] = EditKey<K>::make(j, j);
  }
  K diag_left = EditKey<K>::make(j0, j0);  // C[i-1][j0] of the row this lane works on next
  K last = 0;
  int tok = -1, rbuf = -1;
  const int last_lane = (m - 1) / CPL;
  const int nsteps = n + last_lane;
  for (int t = 0; t < nsteps; ++t) {
    if ((t & 63) == 0) rbuf = t + lane < n ? ref[t + lane] : -1;
    tok = edit_lane_up(__builtin_amdgcn_readlane(rbuf, t & 63), tok);
    const K recv = (K)edit_lane_up((int)EditKey<K>::make(t + 1, 0), (int)last);
    if ((unsigned)(t - lane) < (unsigned)n) {  // row i = t - lane + 1
      K diag = diag_left, left = recv;
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        const K up = prev[c];
        left = edit_cell<K>(diag, up, left, tok != h[c]);
        prev[c] = left;
        diag = up;
      }
      diag_left = recv;
      last = left;
    }
  }
  if (lane == last_lane) {
    const int cs = (m - 1) % CPL;
    K res = prev[0];
#pragma unroll
    for (int c = 1; c < CPL; ++c) res = c == cs ? prev[c] : res;
    edit_store_counts(out, res >> 16, res & 0xFFFFu, n, m);
  }
}

// ---- workgroup route: n, m >= 1; col = two boundary columns of at least n + 1 keys each ----
__device__ __forceinline__ void edit_wg_sweep(const int32_t* __restrict__ ref, int n, const int32_t* __restrict__ hyp, int m,
                                              double* col, int64_t col_stride, int32_t* out, double (*lds_key)[CA_EDIT_WG_WAVES],
                                              int (*lds_tok)[CA_EDIT_WG_WAVES]) {
  typedef double K;
  constexpr int CPT = CA_EDIT_CPT;
  const int g = threadIdx.x, lane = g & 63, w = g >> 6;
  const int npanels = (m + CA_EDIT_PANEL - 1) / CA_EDIT_PANEL;
  K prev[CPT];
  for (int p = 0; p < npanels; ++p) {
    const int jbase = p * CA_EDIT_PANEL;
    const K* bin = col + (int64_t)(p & 1) * col_stride;   // C[i][jbase], written by the panel before
    K* bout = col + (int64_t)((p + 1) & 1) * col_stride;  // C[i][jbase + CA_EDIT_PANEL]
    const int width = min(m - jbase, CA_EDIT_PANEL);
    const int nact = (width + CPT - 1) / CPT;  // threads that own a column <= m
    const int j0 = jbase + g * CPT;
    int h[CPT];
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      const int j = j0 + c + 1;
      h[c] = j <= m ? hyp[j - 1] : -1;
      prev[c] = EditKey<K>::make(j, j);
    }
    K diag_left = EditKey<K>::make(j0, j0);
    K last = 0, bbuf = 0;
    int tok = -1, rbuf = -1;
    const int nsteps = n + nact - 1;
    const bool keep = p + 1 < npanels && g == CA_EDIT_WG_THREADS - 1;  // owns the panel's last column, and a panel follows
    for (int t = 0; t < nsteps; ++t) {
      K inj_key;
      int inj_tok;
      if (w == 0) {
        if ((t & 63) == 0) {
          const int i = t + lane + 1;  // the row lane 0 works on at step t + lane
          rbuf = i <= n ? ref[i - 1] : -1;
          bbuf = i <= n ? (p ? bin[i] : EditKey<K>::make(i, 0)) : K(0);
        }
        inj_tok = __builtin_amdgcn_readlane(rbuf, t & 63);
        inj_key = edit_read_lane(bbuf, t & 63);
      } else {  // what the last lane of the wave before left at step t - 1
        inj_key = lds_key[(t + 1) & 1][w - 1];
        inj_tok = lds_tok[(t + 1) & 1][w - 1];
      }
      tok = edit_lane_up(inj_tok, tok);
      const K recv = edit_lane_up(inj_key, last);
      const int i = t - g;  // row i + 1
      if ((unsigned)i < (unsigned)n && g < nact) {
        K diag = diag_left, left = recv;
#pragma unroll
        for (int c = 0; c < CPT; ++c) {
          const K up = prev[c];
          left = edit_cell<K>(diag, up, left, tok != h[c]);
          prev[c] = left;
          diag = up;
        }
        diag_left = recv;
        last = left;
        if (keep) bout[i + 1] = last;
      }
      if (lane == 63) {
        lds_key[t & 1][w] = last;
        lds_tok[t & 1][w] = tok;
      }
      __syncthreads();
    }
  }
  const int mm = (m - 1) % CA_EDIT_PANEL;
  if (g == mm / CPT) {
    const int cs = mm % CPT;
    K res = prev[0];
#pragma unroll
    for (int c = 1; c < CPT; ++c) res = c == cs ? prev[c] : res;
    const int64_t key = (int64_t)res;
    edit_store_counts(out, key >> 22, key & ((1 << 22) - 1), n, m);
  }
}

struct EditPair {
  int n, m, kind;  // kind: 0 nothing to sweep, 1 wave route, 2 workgroup route
  const int32_t *ref, *hyp;
  int32_t* out;
};

// what serves a pair of these lengths: -1 nothing can, 0 an empty side (the result is known), 1 a wave, 2 the workgroup
__device__ __forceinline__ int edit_route(int64_t n, int64_t m, int route) {
  if (n < 0 || m < 0 || n > CA_EDIT_MAX_TOKENS || m > CA_EDIT_MAX_TOKENS) return -1;
  if (n == 0 || m == 0) return 0;
  if (route != 2 && n <= CA_EDIT_WAVE_MAX && m <= CA_EDIT_WAVE_MAX) return 1;
  return route == 1 ? -1 : 2;
}

// The pair at position k of the launch order and its route.  `writer` (one thread per pair) writes the result of a pair
// with an empty side, and -1 into all four counts of a pair that cannot be served (a length outside [0,
// CA_EDIT_MAX_TOKENS], route 1 with a side above CA_EDIT_WAVE_MAX); an `order` entry outside the batch is left alone.
__device__ __forceinline__ EditPair edit_pair(const int32_t* ref, const int64_t* ref_off, const int32_t* hyp,
                                              const int64_t* hyp_off, const int32_t* order, int n_pairs, int32_t* counts,
                                              int route, int64_t k, bool writer) {
  EditPair q;
  q.kind = 0;
  if (k >= n_pairs) return q;
  const int pid = order ? order[k] : (int)k;
  if ((unsigned)pid >= (unsigned)n_pairs) return q;
  const int64_t r0 = ref_off[pid], h0 = hyp_off[pid];
  const int64_t n = ref_off[pid + 1] - r0, m = hyp_off[pid + 1] - h0;
  q.out = counts + 4 * (int64_t)pid;
  q.n = (int)n, q.m = (int)m, q.ref = ref + r0, q.hyp = hyp + h0;
  const int kind = edit_route(n, m, route);
  if (kind == 0 && writer) q.out[0] = 0, q.out[1] = 0, q.out[2] = (int32_t)n, q.out[3] = (int32_t)m;  // (0, 0, n, 0) or (0, 0, 0, m)
  if (kind < 0 && writer) q.out[0] = q.out[1] = q.out[2] = q.out[3] = -1;
  q.kind = kind > 0 ? kind : 0;
  return q;
}

// Where the boundary columns of the workgroup-route pair at launch position k start in the workspace, in keys: every
// such pair before it in the launch order owns 2 (n + 1) keys.  Counted by the whole workgroup (a plain sum: the same
// from run to run); only a workgroup that meets such a pair pays for it.
__device__ __forceinline__ int64_t edit_ws_offset(const int64_t* ref_off, const int64_t* hyp_off, const int32_t* order,
                                                  int n_pairs, int route, int64_t k, int64_t* lds_sum) {
  int64_t s = 0;
  for (int64_t k2 = threadIdx.x; k2 < k; k2 += CA_EDIT_WG_THREADS) {
    const int pid = order ? order[k2] : (int)k2;
    if ((unsigned)pid >= (unsigned)n_pairs) continue;
    const int64_t n = ref_off[pid + 1] - ref_off[pid], m = hyp_off[pid + 1] - hyp_off[pid];
    if (edit_route(n, m, route) == 2) s += 2 * (n + 1);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds_sum[threadIdx.x >> 6] = s;
  __syncthreads();
  s = 0;
#pragma unroll
  for (int v = 0; v < CA_EDIT_WG_WAVES; ++v) s += lds_sum[v];
  return s;
}

__global__ __launch_bounds__(CA_EDIT_WG_THREADS) void edit_counts_kernel(
    const int32_t* __restrict__ ref, const int64_t* __restrict__ ref_off, const int32_t* __restrict__ hyp,
    const int64_t* __restrict__ hyp_off, const int32_t* __restrict__ order, int n_pairs, int32_t* __restrict__ counts,
    int route, double* __restrict__ ws, int64_t ws_keys) {
  __shared__ double lds_key[2][CA_EDIT_WG_WAVES];
  __shared__ int lds_tok[2][CA_EDIT_WG_WAVES];
  __shared__ int64_t lds_sum[CA_EDIT_WG_WAVES];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  {  // wave route: wave w takes the pair at blockIdx.x + w * gridDim.x
    const EditPair q = edit_pair(ref, ref_off, hyp, hyp_off, order, n_pairs, counts, route,
                                 (int64_t)blockIdx.x + (int64_t)w * gridDim.x, lane == 0);
    if (q.kind == 1) {
      if (q.m <= 64) edit_wave_sweep<1>(q.ref, q.n, q.hyp, q.m, lane, q.out);
      else if (q.m <= 128) edit_wave_sweep<2>(q.ref, q.n, q.hyp, q.m, lane, q.out);
      else if (q.m <= 256) edit_wave_sweep<4>(q.ref, q.n, q.hyp, q.m, lane, q.out);
      else if (q.m <= 512) edit_wave_sweep<8>(q.ref, q.n, q.hyp, q.m, lane, q.out);
      else edit_wave_sweep<16>(q.ref, q.n, q.hyp, q.m, lane, q.out);
    }
  }
  // workgroup route: the same pairs again, the long ones by all waves together, one after the other
  for (int v = 0; v < CA_EDIT_WG_WAVES; ++v) {
    const int64_t k = (int64_t)blockIdx.x + (int64_t)v * gridDim.x;
    const EditPair q = edit_pair(ref, ref_off, hyp, hyp_off, order, n_pairs, counts, route, k, false);
    if (q.kind != 2) continue;  // (the same for every thread of the workgroup)
    const int64_t at = edit_ws_offset(ref_off, hyp_off, order, n_pairs, route, k, lds_sum);
    const int64_t col_stride = (int64_t)q.n + 1;
    if (at + 2 * col_stride > ws_keys) {  // the workspace does not hold this pair's columns
      if (threadIdx.x == 0) q.out[0] = q.out[1] = q.out[2] = q.out[3] = -1;
      continue;
    }
    edit_wg_sweep(q.ref, q.n, q.hyp, q.m, ws + at, col_stride, q.out, lds_key, lds_tok);
  }
}

static int64_t edit_groups(int64_t n_pairs) { return (n_pairs + CA_EDIT_WG_WAVES - 1) / CA_EDIT_WG_WAVES; }

extern "C" int64_t ca_edit_counts_workspace_bytes(int32_t n_pairs, int64_t max_ref_len, int64_t max_hyp_len) {
  if (n_pairs <= 0 || max_ref_len < 0 || max_hyp_len < 0) return 0;
  // two boundary columns of n + 1 keys for every pair on the workgroup route (the wave route uses none)
  return (int64_t)n_pairs * 2 * (max_ref_len + 1) * (int64_t)sizeof(uint64_t);
}

extern "C" int ca_edit_counts(const int32_t* ref, const int64_t* ref_off, const int32_t* hyp, const int64_t* hyp_off,
                              const int32_t* order, int32_t n_pairs, int32_t* counts, int32_t route, void* ws,
                              int64_t ws_bytes, void* stream) {
  CA_CHECK_ARG(ref_off && hyp_off && counts, "ca_edit_counts: null pointer");
  CA_CHECK_ARG(ref && hyp, "ca_edit_counts: null pointer (an empty side still needs a valid token pointer)");
  CA_CHECK_ARG(n_pairs > 0, "ca_edit_counts: n_pairs %d must be positive", n_pairs);
  CA_CHECK_ARG(route >= 0 && route <= 2, "ca_edit_counts: route %d is not 0 (by length), 1 (wave) or 2 (workgroup)", route);
  CA_CHECK_ARG(ws_bytes >= 0 && (ws || ws_bytes == 0) && ((uintptr_t)ws & 7) == 0,
               "ca_edit_counts: bad workspace (NULL with ws_bytes > 0, or not 8-byte aligned)");
  hipLaunchKernelGGL(edit_counts_kernel, dim3((unsigned)edit_groups(n_pairs)), dim3(CA_EDIT_WG_THREADS), 0,
                     (hipStream_t)stream, ref, ref_off, hyp, hyp_off, order, n_pairs, counts, route, (double*)ws,
                     ws_bytes / (int64_t)sizeof(double));
  CA_CHECK_LAUNCH("ca_edit_counts");
  return CA_OK;
}
