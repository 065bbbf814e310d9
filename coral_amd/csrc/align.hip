// Whisper word timestamps: the cross-attention alignment cost and dynamic time warping
// ($TF/models/whisper/generation_whisper.py: _extract_token_timestamps, _median_filter, _dynamic_time_warping).
//
//   ca_whisper_align_cost   W[b,a,t,:] = softmax_j(scale q[a,b,t,:] . K_a[b,j,:]) over all Te keys, cropped to F_b;
//                           standardised over t per (b,a,j); median-filtered along j; C = -mean_a.       3 launches per
//                           group of clips (the raw weights live in the caller's workspace, clips are grouped to fit it)
//   ca_dtw_token_times      one workgroup per clip sweeps the anti-diagonals of the (Lw+1) x (F_b+1) table, trace codes
//                           to a byte table in global memory, backtrace by one lane.
//
// Built like the rest of the library without fast-math: the DTW's tie and NaN behaviour is that of IEEE comparisons.
#include "common.h"
#include <math.h>

namespace {

struct AlignHeads {
  const unsigned short* k[CA_ALIGN_MAX_HEADS];  // K of alignment head a: the layer's buffer + head * hd
};

__device__ __forceinline__ int clip_frames(const int32_t* frames, int b, int Fmax) {
  const int f = frames[b];
  return f < 1 ? 1 : (f > Fmax ? Fmax : f);
}

// ---- stage 1: softmax rows ----------------------------------------------------------------------------------------------
// One wave per (clip, head, token): a lane owns keys lane, lane + 64, ... (24 x 64 >= 1500), scores by fp32 FMA over the
// head dimension (at most 448 x 1500 x 128 MACs per head: nowhere near a bottleneck), softmax in fp32 over ALL Te keys,
// the first F_b probabilities stored.
#define ALIGN_KEYS_PER_LANE 24
__global__ __launch_bounds__(256) void align_weights_kernel(const unsigned short* __restrict__ q, const AlignHeads hk,
                                                            int64_t ldk, int64_t skb, const int32_t* __restrict__ frames,
                                                            int b0, int B, int A, int Lw, int Te, int hd, int Fmax,
                                                            float scale, float* __restrict__ W) {
  __shared__ float sq[4][CA_ALIGN_MAX_HEAD_DIM];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int a = blockIdx.y, g = blockIdx.z, b = b0 + g;
  const int t_raw = blockIdx.x * 4 + wave;
  const int t = t_raw < Lw ? t_raw : Lw - 1;  // (a wave past the end repeats the last row and stores nothing)
  const unsigned short* qrow = q + (((int64_t)a * B + b) * Lw + t) * hd;
  for (int c = lane; c < hd; c += 64) sq[wave][c] = bf2f(qrow[c]);
  __syncthreads();
  const unsigned short* kb = hk.k[a] + (int64_t)b * skb;
  float s[ALIGN_KEYS_PER_LANE];
  float m = -INFINITY;
#pragma unroll
  for (int u = 0; u < ALIGN_KEYS_PER_LANE; ++u) {
    const int j = u * 64 + lane;
    float acc = -INFINITY;
    if (j < Te) {
      const unsigned short* kr = kb + (int64_t)j * ldk;
      acc = 0.f;
      for (int c = 0; c < hd; c += 8) {
        const u16x8_t v = *(const u16x8_t*)(kr + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = fmaf(sq[wave][c + e], bf2f(v[e]), acc);
      }
      acc *= scale;
      m = fmaxf(m, acc);
    }
    s[u] = acc;
  }
  m = wave_max(m);
  float sum = 0.f;
#pragma unroll
  for (int u = 0; u < ALIGN_KEYS_PER_LANE; ++u) {
    const int j = u * 64 + lane;
    s[u] = j < Te ? expf(s[u] - m) : 0.f;
    sum += s[u];
  }
  sum = wave_sum(sum);
  if (t_raw >= Lw) return;
  const int F = clip_frames(frames, b, Fmax);
  float* wrow = W + (((int64_t)g * A + a) * Lw + t) * Fmax;
#pragma unroll
  for (int u = 0; u < ALIGN_KEYS_PER_LANE; ++u) {
    const int j = u * 64 + lane;
    if (j < F) wrow[j] = s[u] / sum;
  }
}

// ---- stage 2a: mean and population standard deviation over the tokens, per (clip, head, frame) ----------------------------
// In fp64 (Lw <= 447 terms per frame: nothing next to stage 1): the standardised weight (w - mean) / std formed from them
// in stage 2b is then the correctly rounded fp32 of the formula on the stored fp32 weights - at Lw = 2 exactly +-1, where
// an fp32 evaluation is one rounding off or not depending on the operation order.
__global__ __launch_bounds__(256) void align_stats_kernel(const float* __restrict__ W, const int32_t* __restrict__ frames,
                                                          int b0, int A, int Lw, int Fmax, double* __restrict__ stats) {
  const int j = blockIdx.x * 256 + threadIdx.x, a = blockIdx.y, g = blockIdx.z;
  const int F = clip_frames(frames, b0 + g, Fmax);
  if (j >= F) return;
  const float* w = W + ((int64_t)g * A + a) * Lw * Fmax + j;
  double sum = 0.0;
  for (int t = 0; t < Lw; ++t) sum += (double)w[(int64_t)t * Fmax];
  const double mean = sum / (double)Lw;
  double var = 0.0;
  for (int t = 0; t < Lw; ++t) {
    const double dlt = (double)w[(int64_t)t * Fmax] - mean;
    var += dlt * dlt;
  }
  double* st = stats + ((int64_t)g * A + a) * 2 * Fmax;
  st[j] = mean;
  st[Fmax + j] = sqrt(var / (double)Lw);
}

// ---- stage 2b: standardise, median along the frames (reflect padding), mean over the heads, negate ----------------------
// A workgroup owns 256 frames of one (clip, token).  Per head it stages the standardised values of its frames and the
// filter's margin in LDS; a thread then finds the median of its `width` taps by counting ranks (no per-thread array).
// The order is torch.sort's: NaN above every number.
__device__ __forceinline__ bool nan_last_less(float x, float y) { return x < y || (y != y && x == x); }

__global__ __launch_bounds__(256) void align_cost_kernel(const float* __restrict__ W, const double* __restrict__ stats,
                                                         const int32_t* __restrict__ frames, int b0, int A, int Lw,
                                                         int Fmax, int width, float* __restrict__ cost) {
  __shared__ float sv[256 + CA_ALIGN_MAX_FILTER_WIDTH - 1];
  const int tid = threadIdx.x, j0 = blockIdx.x * 256, t = blockIdx.y, g = blockIdx.z, b = b0 + g;
  const int F = clip_frames(frames, b, Fmax);
  const int pad = F > width / 2 ? width / 2 : 0;  // F <= width / 2: the filter is skipped altogether
  const int taps = 2 * pad + 1;
  const int j = j0 + tid;
  double acc = 0.0;  // (the mean over the heads: one rounding, at the end)
  for (int a = 0; a < A; ++a) {
    const float* wrow = W + (((int64_t)g * A + a) * Lw + t) * Fmax;
    const double* st = stats + ((int64_t)g * A + a) * 2 * Fmax;
    __syncthreads();
    for (int x = tid; x < 256 + 2 * pad; x += 256) {
      int jj = j0 - pad + x;
      float v = 0.f;
      if (jj < F + pad) {  // (jj >= -pad always)
        if (jj < 0) jj = -jj;
        if (jj >= F) jj = 2 * (F - 1) - jj;
        v = (float)(((double)wrow[jj] - st[jj]) / st[Fmax + jj]);
      }
      sv[x] = v;
    }
    __syncthreads();
    if (j < F) {
      float med = sv[tid + pad];
      if (pad) {
        for (int k = 0; k < taps; ++k) {
          const float xk = sv[tid + k];
          int below = 0;
          for (int m = 0; m < taps; ++m) {
            const float xm = sv[tid + m];
            below += (nan_last_less(xm, xk) || (!nan_last_less(xk, xm) && m < k)) ? 1 : 0;
          }
          if (below == pad) med = xk;
        }
      }
      acc += (double)med;
    }
  }
  if (j < Fmax) cost[((int64_t)b * Lw + t) * Fmax + j] = j < F ? (float)(-(acc / (double)A)) : 0.f;
}

// ---- dynamic time warping -------------------------------------------------------------------------------------------------
// Thread i - 1 owns row i of the table and walks it left to right, one cell per anti-diagonal k = i + j: cost[i-1, j-1]
// is what it read as cost[i-1, j] one diagonal earlier, cost[i, j-1] its own last result, cost[i-1, j] the neighbour's
// last result, passed through a double-buffered LDS row (one barrier per diagonal).  Every loop bound is Lw + F_b.
__global__ __launch_bounds__(448) void dtw_kernel(const float* __restrict__ cost, const int32_t* __restrict__ frames, int Lw,
                                                  int Fmax, uint8_t* __restrict__ trace, int32_t* __restrict__ jump,
                                                  int32_t* __restrict__ path_text, int32_t* __restrict__ path_time,
                                                  int32_t* __restrict__ path_len) {
  __shared__ float sd[2][CA_ALIGN_MAX_TOKENS + 1];
  const int b = blockIdx.x, tid = threadIdx.x, i = tid + 1;
  const int F = clip_frames(frames, b, Fmax);
  for (int x = tid; x <= Lw; x += blockDim.x) sd[0][x] = sd[1][x] = INFINITY;  // (slot 0 = row 0 of the table: stays +inf)
  __syncthreads();
  const bool row = i <= Lw;
  const int64_t base = ((int64_t)b * Lw + (row ? i - 1 : 0)) * Fmax;
  const float* crow = cost + base;
  uint8_t* trow = trace + base;
  float c0 = i == 1 ? 0.f : INFINITY;  // cost[i-1, 0]
  float c2 = INFINITY;                 // cost[i, 0]
  float cv = row ? crow[0] : 0.f;      // the matrix entry of the next cell of this row
  const int last = Lw + F;
  for (int k = 2; k <= last; ++k) {
    const int j = k - i;
    if (row && j >= 1 && j <= F) {
      const float c1 = sd[(k - 1) & 1][i - 1];
      float c;
      uint8_t tr;
      if (c0 < c1 && c0 < c2) {
        c = c0, tr = 0;
      } else if (c1 < c0 && c1 < c2) {
        c = c1, tr = 1;
      } else {
        c = c2, tr = 2;
      }
      const float cur = cv + c;
      trow[j - 1] = tr;
      sd[k & 1][i] = cur;
      c0 = c1;
      c2 = cur;
      if (j < F) cv = crow[j];
    }
    __syncthreads();
  }
  __threadfence();
  __syncthreads();
  if (tid != 0) return;
  // backtrace from (Lw, F); row 0 reads as trace 2, column 0 as trace 1.  Walking backwards, the last visit of a text
  // index is its first step on the path: its jump frame.
  const uint8_t* tb = trace + (int64_t)b * Lw * Fmax;
  const int64_t pbase = (int64_t)b * (Lw + Fmax);
  int ci = Lw, cj = F, n = 0;
  while ((ci > 0 || cj > 0) && n < last) {
    if (ci >= 1) jump[(int64_t)b * Lw + ci - 1] = cj - 1;
    if (path_text) {
      path_text[pbase + n] = ci - 1;
      path_time[pbase + n] = cj - 1;
    }
    ++n;
    const int tr = ci == 0 ? 2 : (cj == 0 ? 1 : tb[(int64_t)(ci - 1) * Fmax + (cj - 1)]);
    if (tr == 0) {
      --ci, --cj;
    } else if (tr == 1) {
      --ci;
    } else {
      --cj;
    }
  }
  if (path_len) path_len[b] = n;
}

int check_align_limits(const char* what, int A, int Lw, int Fmax, int hd) {
  if (A > CA_ALIGN_MAX_HEADS || Lw > CA_ALIGN_MAX_TOKENS || Fmax > CA_ALIGN_MAX_FRAMES || hd > CA_ALIGN_MAX_HEAD_DIM ||
      (hd & 7) != 0) {
    ca_set_error("%s: at most %d alignment heads, %d tokens, %d frames, head_dim a multiple of 8 up to %d (got %d, %d, %d, %d)",
                 what, CA_ALIGN_MAX_HEADS, CA_ALIGN_MAX_TOKENS, CA_ALIGN_MAX_FRAMES, CA_ALIGN_MAX_HEAD_DIM, A, Lw, Fmax, hd);
    return CA_ERR_UNSUPPORTED;
  }
  return CA_OK;
}

}  // namespace

extern "C" int ca_whisper_align_cost(const void* q, const void* const* cross_k, int32_t n_layers, const int32_t* layer_head,
                                     int32_t A, int32_t B, int32_t Lw, int32_t Te, int32_t H, int32_t hd, int64_t ldk,
                                     int64_t skb, const int32_t* frames, int32_t Fmax, float scale, int32_t filter_width,
                                     float* cost, void* ws, int64_t ws_bytes, void* stream) {
  CA_CHECK_ARG(q && cross_k && layer_head && frames && cost && ws, "ca_whisper_align_cost: null pointer");
  CA_CHECK_ARG(A >= 1 && B >= 1 && Lw >= 1 && Fmax >= 1 && hd >= 1 && H >= 1 && n_layers >= 1,
               "ca_whisper_align_cost: sizes must be positive");
  const int rc = check_align_limits("ca_whisper_align_cost", A, Lw, Fmax, hd);
  if (rc != CA_OK) return rc;
  if (Te > CA_ALIGN_MAX_FRAMES || filter_width > CA_ALIGN_MAX_FILTER_WIDTH) {
    ca_set_error("ca_whisper_align_cost: at most %d encoder positions and a filter of width %d (got %d, %d)",
                 CA_ALIGN_MAX_FRAMES, CA_ALIGN_MAX_FILTER_WIDTH, Te, filter_width);
    return CA_ERR_UNSUPPORTED;
  }
  CA_CHECK_ARG(Fmax <= Te, "ca_whisper_align_cost: Fmax %d exceeds the %d encoder positions", Fmax, Te);
  CA_CHECK_ARG(filter_width >= 1 && (filter_width & 1), "ca_whisper_align_cost: `filter_width` should be an odd number");
  CA_CHECK_ARG(ldk >= (int64_t)H * hd && (ldk & 7) == 0 && skb >= (int64_t)Te * ldk && (skb & 7) == 0,
               "ca_whisper_align_cost: K rows of %lld elements, %lld per clip", (long long)ldk, (long long)skb);
  AlignHeads hk;
  for (int a = 0; a < A; ++a) {
    const int l = layer_head[2 * a], h = layer_head[2 * a + 1];
    CA_CHECK_ARG(l >= 0 && l < n_layers && h >= 0 && h < H && cross_k[l],
                 "ca_whisper_align_cost: alignment head (%d, %d) outside %d layers x %d heads", l, h, n_layers, H);
    hk.k[a] = (const unsigned short*)cross_k[l] + (int64_t)h * hd;
  }
  for (int a = A; a < CA_ALIGN_MAX_HEADS; ++a) hk.k[a] = nullptr;
  const int64_t per_clip = CA_ALIGN_WS_BYTES_PER_CLIP(A, Lw, Fmax);
  int64_t G = ws_bytes / per_clip;
  CA_CHECK_ARG(G >= 1, "ca_whisper_align_cost: the workspace holds %lld bytes, one clip needs %lld", (long long)ws_bytes,
               (long long)per_clip);
  if (G > B) G = B;
  if (G > 65535) G = 65535;
  double* stats = (double*)ws;  // (first: 8-byte aligned whatever the sizes)
  float* W = (float*)(stats + G * A * 2 * (int64_t)Fmax);
  hipStream_t s = (hipStream_t)stream;
  const int ftiles = (Fmax + 255) / 256;
  for (int b0 = 0; b0 < B; b0 += (int)G) {
    const int g = B - b0 < G ? B - b0 : (int)G;
    hipLaunchKernelGGL(align_weights_kernel, dim3((Lw + 3) / 4, A, g), dim3(256), 0, s, (const unsigned short*)q, hk, ldk,
                       skb, frames, b0, B, A, Lw, Te, hd, Fmax, scale, W);
    hipLaunchKernelGGL(align_stats_kernel, dim3(ftiles, A, g), dim3(256), 0, s, W, frames, b0, A, Lw, Fmax, stats);
    hipLaunchKernelGGL(align_cost_kernel, dim3(ftiles, Lw, g), dim3(256), 0, s, W, stats, frames, b0, A, Lw, Fmax,
                       filter_width, cost);
  }
  CA_CHECK_LAUNCH("ca_whisper_align_cost");
  return CA_OK;
}

extern "C" int ca_dtw_token_times(const float* cost, int32_t B, int32_t Lw, const int32_t* frames, int32_t Fmax,
                                  uint8_t* trace, int32_t* jump, int32_t* path_text, int32_t* path_time, int32_t* path_len,
                                  void* stream) {
  CA_CHECK_ARG(cost && frames && trace && jump, "ca_dtw_token_times: null pointer");
  CA_CHECK_ARG(B >= 1 && B <= 65535 && Lw >= 1 && Fmax >= 1, "ca_dtw_token_times: sizes must be positive");
  CA_CHECK_ARG((path_text == nullptr) == (path_time == nullptr) && (path_text == nullptr) == (path_len == nullptr),
               "ca_dtw_token_times: the path takes all three tables");
  const int rc = check_align_limits("ca_dtw_token_times", 1, Lw, Fmax, 8);
  if (rc != CA_OK) return rc;
  const int threads = (Lw + 63) / 64 * 64;
  hipLaunchKernelGGL(dtw_kernel, dim3(B), dim3(threads), 0, (hipStream_t)stream, cost, frames, Lw, Fmax, trace, jump, path_text,
                     path_time, path_len);
  CA_CHECK_LAUNCH("ca_dtw_token_times");
  return CA_OK;
}
