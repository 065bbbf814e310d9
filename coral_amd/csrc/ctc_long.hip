// Long-form CTC transcription (coral_amd/longform.py): stitching the kept frames of overlapping chunks into one row
// per recording, and a CTC collapse over rows of any length that also reports where every emitted token starts and ends.
//   $TF/pipelines/automatic_speech_recognition.py: postprocess (`items[:, left:right_n]`, concatenate) and
//   $TF/models/wav2vec2/tokenization_wav2vec2.py: convert_tokens_to_string / _compute_offsets (groupby run lengths).
#include "common.h"

// ---- ca_ctc_stitch -----------------------------------------------------------------------------
// One wavefront per kept frame.  A lane holds four consecutive logits (one 16-byte load, one 16-byte store for the
// copy); the per-lane maxima are merged with "larger value, then lower index", which is the first maximum of a scan
// from column 0 - what ctc_greedy_kernel's `x > best` keeps.
#define STITCH_WAVES 4

template <bool VEC>
__global__ __launch_bounds__(STITCH_WAVES * 64) void ctc_stitch_kernel(const float* __restrict__ logits,
                                                                        const int32_t* __restrict__ seg,
                                                                        int32_t* __restrict__ raw_out,
                                                                        float* __restrict__ logits_out, int T, int V,
                                                                        int64_t ldv, int R, int Tout) {
  const int c = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * STITCH_WAVES + (threadIdx.x >> 6);
  const int row = seg[4 * c + 0], off = seg[4 * c + 1], left = seg[4 * c + 2], keep = seg[4 * c + 3];
  // (wave-uniform: a frame outside the chunk, the destination row or the table's own range is not touched)
  if (j >= keep || row < 0 || row >= R || left < 0 || off < 0 || left + j >= T || off + j >= Tout) return;
  const float* src = logits + ((int64_t)c * T + left + j) * ldv;
  float* dst = logits_out ? logits_out + ((int64_t)row * Tout + off + j) * ldv : nullptr;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  if (VEC) {
    for (int v4 = lane; v4 < (int)(ldv >> 2); v4 += 64) {
      const f32x4_t x = *(const f32x4_t*)(src + 4 * v4);
      if (dst) *(f32x4_t*)(dst + 4 * v4) = x;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int v = 4 * v4 + e;
        if (v < V && (x[e] > best || bi == 0x7fffffff)) {
          best = x[e];
          bi = v;
        }
      }
    }
  } else {
    for (int v = lane; v < (int)ldv; v += 64) {
      const float x = src[v];
      if (dst) dst[v] = x;
      if (v < V && (x > best || bi == 0x7fffffff)) {
        best = x;
        bi = v;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (oi != 0x7fffffff && (bi == 0x7fffffff || ov > best || (ov == best && oi < bi))) {
      best = ov;
      bi = oi;
    }
  }
  if (lane == 0) raw_out[(int64_t)row * Tout + off + j] = bi;
}

extern "C" int ca_ctc_stitch(const float* logits, const int32_t* seg, int32_t* raw_out, float* logits_out, int32_t C,
                             int32_t T, int32_t V, int64_t ldv, int32_t R, int32_t Tout, void* stream) {
  CA_CHECK_ARG(logits && seg && raw_out, "ca_ctc_stitch: null pointer");
  CA_CHECK_ARG(C > 0 && C <= 65535 && T > 0 && V > 0 && ldv >= V && R > 0 && Tout > 0,
               "ca_ctc_stitch: bad shape (1 <= C <= 65535, ldv >= V)");
  const bool vec = (ldv % 4 == 0) && ((uintptr_t)logits % 16 == 0) && ((uintptr_t)logits_out % 16 == 0);
  const dim3 grid((unsigned)((T + STITCH_WAVES - 1) / STITCH_WAVES), (unsigned)C);
  if (vec)
    hipLaunchKernelGGL(ctc_stitch_kernel<true>, grid, dim3(STITCH_WAVES * 64), 0, (hipStream_t)stream, logits, seg,
                       raw_out, logits_out, T, V, ldv, R, Tout);
  else
    hipLaunchKernelGGL(ctc_stitch_kernel<false>, grid, dim3(STITCH_WAVES * 64), 0, (hipStream_t)stream, logits, seg,
                       raw_out, logits_out, T, V, ldv, R, Tout);
  CA_CHECK_LAUNCH("ca_ctc_stitch");
  return CA_OK;
}

// ---- ca_ctc_collapse_offsets -------------------------------------------------------------------
// A row is cut into tiles of COLLAPSE_TILE frames, one workgroup per (tile, row), three launches:
//   1. tiles:   per tile, the number of emitted tokens (starts of non-blank runs) and the first run start of any id;
//   2. rows:    per row, the exclusive prefix sum of the tile counts (where a tile's tokens go) and the exclusive suffix
//               minimum of the tiles' first run starts (where a run that is still open at the end of a tile ends);
//   3. scatter: per tile, the same flags again, the rank of every emitted token inside the tile and, by a suffix minimum
//               over the tile, the start of the run that follows it - a token's end offset.  No thread walks along a
//               run, so silence costs what speech costs.
// Nothing waits for another workgroup and every output element has exactly one writer: the result is the same bits on
// every run.
#define COLLAPSE_THREADS 512
#define COLLAPSE_PER 8
#define COLLAPSE_TILE CA_CTC_COLLAPSE_TILE
static_assert(COLLAPSE_THREADS * COLLAPSE_PER == COLLAPSE_TILE, "tile = threads x frames per thread");
#define NO_START 0x7fffffff

__device__ __forceinline__ int clamp_len(const int32_t* in_len, int b, int T) {
  int n = in_len ? in_len[b] : T;
  return n < 0 ? 0 : (n > T ? T : n);
}

// the tile's ids into LDS, sh[0] = the frame in front of the tile (frame 0 is a run start by the t == 0 rule: what
// stands in front of it is not compared)
__device__ __forceinline__ void load_tile(const int32_t* __restrict__ rb, int t0, int T, int* sh) {
  for (int i = threadIdx.x; i <= COLLAPSE_TILE; i += COLLAPSE_THREADS) {
    const int t = t0 + i - 1;
    sh[i] = (t >= 0 && t < T) ? rb[t] : -1;
  }
}

// block-wide inclusive Hillis-Steele scans over one value per thread (buf: 2 x COLLAPSE_THREADS ints)
__device__ __forceinline__ int block_prefix_sum(int v, int* buf) {
  int cur = 0;
  buf[threadIdx.x] = v;
  __syncthreads();
  for (int o = 1; o < COLLAPSE_THREADS; o <<= 1) {
    const int x = buf[cur * COLLAPSE_THREADS + threadIdx.x] +
                  ((int)threadIdx.x >= o ? buf[cur * COLLAPSE_THREADS + threadIdx.x - o] : 0);
    cur ^= 1;
    buf[cur * COLLAPSE_THREADS + threadIdx.x] = x;
    __syncthreads();
  }
  const int r = buf[cur * COLLAPSE_THREADS + threadIdx.x];
  __syncthreads();
  return r;
}
__device__ __forceinline__ int block_suffix_min(int v, int* buf) {
  int cur = 0;
  buf[threadIdx.x] = v;
  __syncthreads();
  for (int o = 1; o < COLLAPSE_THREADS; o <<= 1) {
    const int other = (int)threadIdx.x + o < COLLAPSE_THREADS ? buf[cur * COLLAPSE_THREADS + threadIdx.x + o] : NO_START;
    const int x = min(buf[cur * COLLAPSE_THREADS + threadIdx.x], other);
    cur ^= 1;
    buf[cur * COLLAPSE_THREADS + threadIdx.x] = x;
    __syncthreads();
  }
  const int r = buf[cur * COLLAPSE_THREADS + threadIdx.x];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(COLLAPSE_THREADS) void ctc_collapse_tiles_kernel(const int32_t* __restrict__ raw,
                                                                              const int32_t* __restrict__ in_len,
                                                                              int32_t* __restrict__ tile_cnt,
                                                                              int32_t* __restrict__ tile_first, int T,
                                                                              int ntiles, int blank) {
  __shared__ int sh[COLLAPSE_TILE + 1];
  __shared__ int buf[2 * COLLAPSE_THREADS];
  const int tile = blockIdx.x, b = blockIdx.y;
  const int Tin = clamp_len(in_len, b, T);
  const int t0 = tile * COLLAPSE_TILE;
  load_tile(raw + (int64_t)b * T, t0, T, sh);
  __syncthreads();
  int cnt = 0, first = NO_START;
#pragma unroll
  for (int e = 0; e < COLLAPSE_PER; ++e) {
    const int i = threadIdx.x * COLLAPSE_PER + e, t = t0 + i;
    const int c = sh[i + 1];
    const bool rs = t < Tin && (t == 0 || sh[i] != c);
    if (rs && first == NO_START) first = t;
    cnt += (rs && c != blank) ? 1 : 0;
  }
  const int total = block_prefix_sum(cnt, buf);
  const int fmin = block_suffix_min(first, buf);
  if (threadIdx.x == COLLAPSE_THREADS - 1) tile_cnt[(int64_t)b * ntiles + tile] = total;
  if (threadIdx.x == 0) tile_first[(int64_t)b * ntiles + tile] = fmin;
}

__global__ __launch_bounds__(COLLAPSE_THREADS) void ctc_collapse_rows_kernel(const int32_t* __restrict__ tile_cnt,
                                                                             const int32_t* __restrict__ tile_first,
                                                                             int32_t* __restrict__ tile_off,
                                                                             int32_t* __restrict__ tile_next,
                                                                             int32_t* __restrict__ out_len, int ntiles) {
  __shared__ int buf[2 * COLLAPSE_THREADS];
  __shared__ int last, head;
  const int b = blockIdx.x;
  const int32_t* cnt = tile_cnt + (int64_t)b * ntiles;
  const int32_t* fst = tile_first + (int64_t)b * ntiles;
  int32_t* off = tile_off + (int64_t)b * ntiles;
  int32_t* nxt = tile_next + (int64_t)b * ntiles;
  const int nchunks = (ntiles + COLLAPSE_THREADS - 1) / COLLAPSE_THREADS;
  int carry = 0;
  for (int ch = 0; ch < nchunks; ++ch) {
    const int i = ch * COLLAPSE_THREADS + threadIdx.x;
    const int v = i < ntiles ? cnt[i] : 0;
    const int incl = block_prefix_sum(v, buf);
    if (i < ntiles) off[i] = carry + incl - v;
    if (threadIdx.x == COLLAPSE_THREADS - 1) last = incl;
    __syncthreads();
    carry += last;
    __syncthreads();
  }
  if (threadIdx.x == 0) out_len[b] = carry;
  int cmin = NO_START;
  for (int ch = nchunks - 1; ch >= 0; --ch) {
    const int i = ch * COLLAPSE_THREADS + threadIdx.x;
    // exclusive: tile i looks at the tiles behind it
    const int v = i + 1 < ntiles ? fst[i + 1] : NO_START;
    const int m = block_suffix_min(v, buf);
    if (i < ntiles) nxt[i] = min(m, cmin);
    if (threadIdx.x == 0) head = m;
    __syncthreads();
    cmin = min(cmin, head);
    __syncthreads();
  }
}

__global__ __launch_bounds__(COLLAPSE_THREADS) void ctc_collapse_scatter_kernel(
    const int32_t* __restrict__ raw, const int32_t* __restrict__ in_len, const int32_t* __restrict__ tile_off,
    const int32_t* __restrict__ tile_next, const int32_t* __restrict__ out_len, int32_t* __restrict__ ids,
    int32_t* __restrict__ start, int32_t* __restrict__ end, int T, int ntiles, int blank) {
  __shared__ int sh[COLLAPSE_TILE + 1];
  __shared__ int buf[2 * COLLAPSE_THREADS];
  const int tile = blockIdx.x, b = blockIdx.y;
  const int Tin = clamp_len(in_len, b, T);
  const int t0 = tile * COLLAPSE_TILE;
  const int64_t rowb = (int64_t)b * T;
  load_tile(raw + rowb, t0, T, sh);
  __syncthreads();
  int cnt = 0, first = NO_START;
  unsigned rsm = 0, emm = 0;  // run starts / emitted tokens among this thread's frames
#pragma unroll
  for (int e = 0; e < COLLAPSE_PER; ++e) {
    const int i = threadIdx.x * COLLAPSE_PER + e, t = t0 + i;
    const int c = sh[i + 1];
    const bool rs = t < Tin && (t == 0 || sh[i] != c);
    if (rs) {
      rsm |= 1u << e;
      if (first == NO_START) first = t;
      if (c != blank) {
        emm |= 1u << e;
        ++cnt;
      }
    }
  }
  const int incl = block_prefix_sum(cnt, buf);
  // first run start among the threads behind this one, then behind the tile, then the end of the row
  buf[threadIdx.x] = first;
  __syncthreads();
  const int behind = threadIdx.x + 1 < COLLAPSE_THREADS ? buf[threadIdx.x + 1] : NO_START;
  __syncthreads();
  int nx = block_suffix_min(behind, buf);
  nx = min(min(nx, tile_next[(int64_t)b * ntiles + tile]), Tin);
  int k = tile_off[(int64_t)b * ntiles + tile] + incl;  // one past this thread's last token
#pragma unroll
  for (int e = COLLAPSE_PER - 1; e >= 0; --e) {
    const int i = threadIdx.x * COLLAPSE_PER + e, t = t0 + i;
    if (emm >> e & 1u) {
      --k;
      ids[rowb + k] = sh[i + 1];
      start[rowb + k] = t;
      end[rowb + k] = nx;
    }
    if (rsm >> e & 1u) nx = t;
  }
  // padding behind the row's tokens: the places of this tile's own frame range (tokens land in front of out_len)
  const int total = out_len[b];
  for (int i = threadIdx.x; i < COLLAPSE_TILE; i += COLLAPSE_THREADS) {
    const int p = t0 + i;
    if (p < T && p >= total) {
      ids[rowb + p] = -1;
      start[rowb + p] = -1;
      end[rowb + p] = -1;
    }
  }
}

static inline int64_t collapse_align(int64_t n) { return (n + 255) / 256 * 256; }

extern "C" int64_t ca_ctc_collapse_workspace_bytes(int32_t B, int32_t T) {
  if (B <= 0 || T <= 0) return 0;
  const int64_t ntiles = ((int64_t)T + COLLAPSE_TILE - 1) / COLLAPSE_TILE;
  return 4 * collapse_align((int64_t)B * ntiles * 4);
}

extern "C" int ca_ctc_collapse_offsets(const int32_t* raw, const int32_t* in_len, int32_t* ids, int32_t* start,
                                       int32_t* end, int32_t* out_len, void* ws, int64_t ws_bytes, int32_t B, int32_t T,
                                       int32_t blank, void* stream) {
  CA_CHECK_ARG(raw && ids && start && end && out_len && ws, "ca_ctc_collapse_offsets: null pointer");
  CA_CHECK_ARG(B > 0 && B <= 65535 && T > 0 && T <= 0x7fffffff - COLLAPSE_TILE,
               "ca_ctc_collapse_offsets: bad shape (1 <= B <= 65535, T < 2^31 - %d)", COLLAPSE_TILE);
  CA_CHECK_ARG(ws_bytes >= ca_ctc_collapse_workspace_bytes(B, T), "ca_ctc_collapse_offsets: workspace too small");
  const int ntiles = (int)(((int64_t)T + COLLAPSE_TILE - 1) / COLLAPSE_TILE);
  const int64_t seg = collapse_align((int64_t)B * ntiles * 4);
  char* w = (char*)ws;
  int32_t* tile_cnt = (int32_t*)w;
  int32_t* tile_first = (int32_t*)(w + seg);
  int32_t* tile_off = (int32_t*)(w + 2 * seg);
  int32_t* tile_next = (int32_t*)(w + 3 * seg);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)ntiles, (unsigned)B);
  hipLaunchKernelGGL(ctc_collapse_tiles_kernel, grid, dim3(COLLAPSE_THREADS), 0, s, raw, in_len, tile_cnt, tile_first, T,
                     ntiles, blank);
  hipLaunchKernelGGL(ctc_collapse_rows_kernel, dim3(B), dim3(COLLAPSE_THREADS), 0, s, tile_cnt, tile_first, tile_off,
                     tile_next, out_len, ntiles);
  hipLaunchKernelGGL(ctc_collapse_scatter_kernel, grid, dim3(COLLAPSE_THREADS), 0, s, raw, in_len, tile_off, tile_next,
                     out_len, ids, start, end, T, ntiles, blank);
  CA_CHECK_LAUNCH("ca_ctc_collapse_offsets");
  return CA_OK;
}
