// Sampling-rate conversion in front of ca_pcm_prepare: the device side of the reference's
// `cast_column("audio", Audio(sampling_rate=...))` (R/src/coral/data.py).  The definition (a Hann-windowed sinc at a
// rational ratio, torchaudio's sinc_interp_hann formula) is in include/coral_amd.h; the polyphase table is built on the
// host in float64 (coral_amd/resample.py) and this kernel is deterministic given it:
//   y[j Nw + i] = sum_k taps[i][k] * x[j O + off[i] + k],   x = 0 outside [0, len).
//
// One workgroup = CA_RESAMPLE_CHUNK consecutive outputs of one row, RS_OPT per thread; thread t owns the outputs
// c0 + t + 256 e, so consecutive lanes use consecutive phases.  The input span of the chunk is loaded into LDS once
// (int16 converted, samples outside [0, len) masked to 0 there: padding is never read as a value), and every output
// walks its K taps over that window.  The table comes from LDS (route 1, row stride K | 1: odd, so the 32 lanes of a
// ds_read_b32 group, K floats apart, fall on 32 different banks) or from global memory (route 2: a few hundred KB at
// most, L2-resident).  Both routes run the same chain acc = t0 x0, acc = fmaf(tk, xk, acc), k ascending: the same bits.
// An output whose taps would leave the window (possible only with an `off` that is not the plan's, whose first
// sample j O + off[i] never decreases with the output index) reads its samples from global memory instead, with the
// same mask: nothing is read outside the row either way.
#include "common.h"

#define RS_THREADS 256
#define RS_OPT (CA_RESAMPLE_CHUNK / RS_THREADS)
static_assert(RS_OPT * RS_THREADS == CA_RESAMPLE_CHUNK, "a chunk is a whole number of outputs per thread");

// sample m of a row, 0 outside [0, len)
__device__ __forceinline__ float rs_sample(const void* __restrict__ xrow, bool is_int16, int64_t m, int64_t len) {
  if (m < 0 || m >= len) return 0.f;
  return is_int16 ? (float)((const int16_t*)xrow)[m] * (1.0f / 32768.0f) : ((const float*)xrow)[m];
}

template <bool TAPS_LDS>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(
    const void* __restrict__ pcm, int is_int16, int64_t ld_in, const int32_t* __restrict__ len_in,
    const int32_t* __restrict__ rows, const float* __restrict__ taps, const int32_t* __restrict__ off, int O, int Nw,
    int K, float* __restrict__ y, int64_t ld_out, int32_t* __restrict__ len_out, int64_t chunks, int win_cap) {
  extern __shared__ float rs_lds[];  // window [win_cap], then (route 1) the table [Nw][K | 1]
  float* win = rs_lds;
  const int t = threadIdx.x;
  const int64_t r = (int64_t)blockIdx.x / chunks, chunk = (int64_t)blockIdx.x - r * chunks;
  const int64_t row = rows ? (int64_t)rows[r] : r;
  int64_t len = len_in[row];
  len = len < 0 ? 0 : (len > ld_in ? ld_in : len);
  const int64_t n_out = ((int64_t)Nw * len + O - 1) / O;
  const int64_t lo = n_out < ld_out ? n_out : ld_out;
  if (chunk == 0 && t == 0) len_out[row] = (int32_t)lo;
  const int64_t c0 = chunk * CA_RESAMPLE_CHUNK;
  float* yrow = y + row * ld_out;
  if (c0 >= lo) {  // behind the row's last output: the zero tail
#pragma unroll
    for (int e = 0; e < RS_OPT; ++e) {
      const int64_t n = c0 + t + RS_THREADS * e;
      if (n < ld_out) yrow[n] = 0.f;
    }
    return;
  }
  const char* xrow = (const char*)pcm + row * ld_in * (is_int16 ? 2 : 4);
  const int64_t c1 = (c0 + CA_RESAMPLE_CHUNK < lo ? c0 + CA_RESAMPLE_CHUNK : lo) - 1;  // the chunk's last output
  // the window: from the first sample of output c0 to the last sample of output c1
  const int64_t w0 = (c0 / Nw) * O + off[c0 % Nw];
  int64_t wn = (c1 / Nw) * O + off[c1 % Nw] + K - w0;
  wn = wn < 0 ? 0 : (wn > win_cap ? win_cap : wn);
  for (int i = t; i < (int)wn; i += RS_THREADS) win[i] = rs_sample(xrow, is_int16, w0 + i, len);
  const int ts = K | 1;
  if (TAPS_LDS) {
    float* tl = rs_lds + win_cap;
    const int total = Nw * K;
    for (int i = t; i < total; i += RS_THREADS) {
      const int ph = i / K;
      tl[ph * ts + (i - ph * K)] = taps[i];
    }
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < RS_OPT; ++e) {
    const int64_t n = c0 + t + RS_THREADS * e;
    if (n >= ld_out) continue;
    if (n >= lo) {
      yrow[n] = 0.f;
      continue;
    }
    const int64_t j = n / Nw;
    const int ph = (int)(n - j * Nw);
    const int64_t m0 = j * O + off[ph];
    const int64_t rel = m0 - w0;
    float acc;
    if (rel >= 0 && rel + K <= wn) {
      const float* wp = win + rel;
      if (TAPS_LDS) {
        const float* tp = rs_lds + win_cap + ph * ts;
        acc = tp[0] * wp[0];
        for (int k = 1; k < K; ++k) acc = fmaf(tp[k], wp[k], acc);
      } else {
        const float* tp = taps + (int64_t)ph * K;
        acc = tp[0] * wp[0];
        for (int k = 1; k < K; ++k) acc = fmaf(tp[k], wp[k], acc);
      }
    } else {  // not the plan's `off`: the same chain on samples read (masked) from global memory
      const float* tp = taps + (int64_t)ph * K;
      acc = tp[0] * rs_sample(xrow, is_int16, m0, len);
      for (int k = 1; k < K; ++k) acc = fmaf(tp[k], rs_sample(xrow, is_int16, m0 + k, len), acc);
    }
    yrow[n] = acc;
  }
}

extern "C" int ca_resample(const void* pcm, int32_t is_int16, int64_t ld_in, const int32_t* len_in, const int32_t* rows,
                           int32_t R, const float* taps, const int32_t* off, int32_t O, int32_t Nw, int32_t K, float* y,
                           int64_t ld_out, int32_t* len_out, int32_t route, void* stream) {
  CA_CHECK_ARG(pcm && len_in && taps && off && y && len_out, "ca_resample: null pointer");
  CA_CHECK_ARG(R >= 1 && ld_in >= 1 && ld_out >= 1, "ca_resample: R %d, ld_in %lld and ld_out %lld must be positive", R,
               (long long)ld_in, (long long)ld_out);
  CA_CHECK_ARG(O >= 1 && Nw >= 1 && K >= 1, "ca_resample: O %d, Nw %d and K %d must be positive", O, Nw, K);
  CA_CHECK_ARG(K <= CA_RESAMPLE_MAX_TAPS, "ca_resample: K %d is above CA_RESAMPLE_MAX_TAPS = %d", K, CA_RESAMPLE_MAX_TAPS);
  CA_CHECK_ARG((int64_t)Nw * K <= CA_RESAMPLE_MAX_TABLE, "ca_resample: a table of Nw * K = %lld taps is above %d",
               (long long)Nw * K, CA_RESAMPLE_MAX_TABLE);
  CA_CHECK_ARG(route >= 0 && route <= 2, "ca_resample: route %d is not 0 (by size), 1 (table in LDS) or 2 (table in global memory)",
               route);
  const int64_t win_cap = ((int64_t)CA_RESAMPLE_CHUNK * O + Nw - 1) / Nw + K + 1;
  const int64_t win_bytes = win_cap * 4, table_bytes = (int64_t)Nw * (K | 1) * 4;
  CA_CHECK_ARG(win_bytes <= CA_RESAMPLE_LDS_BYTES,
               "ca_resample: the input window of one chunk (%lld bytes at O / Nw = %d / %d, K = %d) does not fit the %d bytes of LDS",
               (long long)win_bytes, O, Nw, K, CA_RESAMPLE_LDS_BYTES);
  CA_CHECK_ARG(route != 1 || win_bytes + table_bytes <= CA_RESAMPLE_LDS_BYTES,
               "ca_resample: route 1 with a table of %lld bytes beside a window of %lld: more than the %d bytes of LDS",
               (long long)table_bytes, (long long)win_bytes, CA_RESAMPLE_LDS_BYTES);
  const int64_t chunks = (ld_out + CA_RESAMPLE_CHUNK - 1) / CA_RESAMPLE_CHUNK;
  CA_CHECK_ARG(chunks * R <= 0x7fffffffLL, "ca_resample: %lld chunks of %d outputs are more than one launch takes",
               (long long)(chunks * R), CA_RESAMPLE_CHUNK);
  const bool in_lds = route == 1 || (route == 0 && win_bytes + table_bytes <= CA_RESAMPLE_LDS_BYTES);
  const size_t lds = (size_t)(win_bytes + (in_lds ? table_bytes : 0));
  static bool attr = false;
  if (!attr) {
    hipFuncSetAttribute((const void*)resample_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, CA_RESAMPLE_LDS_BYTES);
    hipFuncSetAttribute((const void*)resample_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, CA_RESAMPLE_LDS_BYTES);
    attr = true;
  }
  if (in_lds)
    hipLaunchKernelGGL(resample_kernel<true>, dim3((unsigned)(chunks * R)), dim3(RS_THREADS), lds, (hipStream_t)stream, pcm,
                       is_int16, ld_in, len_in, rows, taps, off, O, Nw, K, y, ld_out, len_out, chunks, (int)win_cap);
  else
    hipLaunchKernelGGL(resample_kernel<false>, dim3((unsigned)(chunks * R)), dim3(RS_THREADS), lds, (hipStream_t)stream, pcm,
                       is_int16, ld_in, len_in, rows, taps, off, O, Nw, K, y, ld_out, len_out, chunks, (int)win_cap);
  CA_CHECK_LAUNCH("ca_resample");
  return CA_OK;
}
