// Softmax over vocabulary rows: cross-entropy (Whisper LM loss) and masked argmax (greedy generation).
// (The attention softmax lives inside the fused attention kernels, attn_fwd.hip / attn_bwd.hip / attn_decode.hip.)
#include "common.h"

#define NEG_INF (-__builtin_inff())

// ---- cross-entropy (Whisper LM loss) ---------------------------------------------------------
// $TF/models/whisper/modeling_whisper.py:1084-1087: CrossEntropyLoss(ignore_index=-100), mean
// taken by the caller (loss_sum / count).  V ~ 51 866.
// One 1024-thread workgroup per row (a wave per row walked 810 dependent loads three times: 0.67 ms for the
// 688 x 51865 logits of a whisper-medium step); 16-byte loads, the row is read from L2 on the second and third sweep.
__global__ __launch_bounds__(1024) void ce_kernel(const float* __restrict__ lg,
                                                  const int32_t* __restrict__ labels,
                                                  float* __restrict__ loss_sum,
                                                  int32_t* __restrict__ count,
                                                  float* __restrict__ grad, int64_t rows, int V,
                                                  int64_t ldv, int ignore) {
  __shared__ float red[16];
  __shared__ float bc;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = blockIdx.x;
  const float* l = lg + row * ldv;
  float* g = grad ? grad + row * ldv : nullptr;
  const int lab = labels[row];
  const int n4 = (int)(ldv >> 2);  // ldv is a multiple of 4 (checked by the launcher)
  if (lab == ignore || lab < 0 || lab >= V) {
    if (g)
      for (int c = threadIdx.x; c < n4; c += 1024) *(f32x4_t*)(g + 4 * c) = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    return;
  }
  float mx = NEG_INF;
  for (int c = threadIdx.x; c < n4; c += 1024) {
    const f32x4_t v = *(const f32x4_t*)(l + 4 * c);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (4 * c + e < V) mx = fmaxf(mx, v[e]);
  }
  mx = wave_max(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    float m = red[0];
    for (int w = 1; w < 16; ++w) m = fmaxf(m, red[w]);
    bc = m;
  }
  __syncthreads();
  mx = bc;
  float sum = 0.f;
  for (int c = threadIdx.x; c < n4; c += 1024) {
    const f32x4_t v = *(const f32x4_t*)(l + 4 * c);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (4 * c + e < V) sum += __expf(v[e] - mx);
  }
  sum = wave_sum(sum);
  __syncthreads();
  if (lane == 0) red[wave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int w = 0; w < 16; ++w) s += red[w];
    // everything stays relative to the row maximum: mx + log(s) rounds to an ulp of |mx|, which a row shifted by 1e4
    // saw as 5e-4 relative on every gradient entry (log_softmax is shift-invariant, the sum mx + log(s) is not)
    const float ls = __logf(s);
    bc = ls;
    atomicAdd(loss_sum, ls - (l[lab] - mx));
    atomicAdd(count, 1);
  }
  __syncthreads();
  const float ls = bc;
  if (g) {
    for (int c = threadIdx.x; c < n4; c += 1024) {
      const f32x4_t v = *(const f32x4_t*)(l + 4 * c);
      f32x4_t o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int col = 4 * c + e;
        o[e] = col < V ? __expf((v[e] - mx) - ls) - (col == lab ? 1.f : 0.f) : 0.f;
      }
      *(f32x4_t*)(g + 4 * c) = o;
    }
  }
}

extern "C" int ca_cross_entropy_fwd_bwd(const float* logits, const int32_t* labels,
                                        float* loss_sum, int32_t* count, float* grad,
                                        int64_t rows, int32_t V, int64_t ldv,
                                        int32_t ignore_index, void* stream) {
  CA_CHECK_ARG(logits && labels && loss_sum && count && rows > 0 && V > 0 && ldv >= V,
               "ca_cross_entropy_fwd_bwd: bad argument");
  CA_CHECK_ARG((ldv % 4) == 0 && ((uintptr_t)logits % 16) == 0 && (!grad || ((uintptr_t)grad % 16) == 0),
               "ca_cross_entropy_fwd_bwd: ldv must be a multiple of 4 and the buffers 16-byte aligned");
  hipLaunchKernelGGL(ce_kernel, dim3((unsigned)rows), dim3(1024), 0, (hipStream_t)stream, logits, labels,
                     loss_sum, count, grad, rows, V, ldv, ignore_index);
  CA_CHECK_LAUNCH("ca_cross_entropy_fwd_bwd");
  return CA_OK;
}

// ---- masked argmax (greedy generation) -------------------------------------------------------
// one 1024-thread workgroup per row (greedy decoding has B rows of ~52 k logits: a wave per row would walk
// 800 dependent loads); ties resolve to the lowest index like torch.argmax.
// adv (ca_argmax_advance): the bookkeeping of a greedy step in the same launch - the row's last thread also records the
// token and moves the row's cursors (eight tiny dependent launches per decoded token otherwise, ~4 us each in a graph)
struct ArgmaxAdvance {
  uint8_t* done;    // [rows] finished flags (a finished row records pad)
  int64_t* ids;     // [rows, ld_ids] generated ids; the token goes to column pos[row] + 1
  int64_t ld_ids;
  int32_t* tok;     // [rows] next input token
  int32_t* pos;     // [rows] position of the token just fed (+1 here)
  int32_t* klen;    // [rows] cached keys (+1 here)
  int32_t pad, eos;
};
__global__ __launch_bounds__(1024) void argmax_kernel(const float* __restrict__ lg,
                                                      const uint8_t* __restrict__ suppress,
                                                      int32_t* __restrict__ out, int64_t rows,
                                                      int V, int64_t ldv, const ArgmaxAdvance adv) {
  __shared__ float sb[16];
  __shared__ int si[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = blockIdx.x;
  const float* l = lg + row * ldv;
  float best = NEG_INF;
  int bi = 0x7fffffff;
  // four logits (and their four suppress bytes) per load where the row is 16-byte aligned; a thread's candidates
  // come in increasing index order, so "strictly greater" keeps the lowest index of equal values
  const bool vec = ((ldv & 3) == 0) && ((((uintptr_t)lg) & 15) == 0) && (!suppress || (((uintptr_t)suppress) & 3) == 0);
  const int V4 = vec ? (V >> 2) : 0;
  for (int q = threadIdx.x; q < V4; q += 1024) {
    const f32x4_t v4 = *(const f32x4_t*)(l + 4 * q);
    const unsigned int sm = suppress ? *(const unsigned int*)(suppress + 4 * q) : 0u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if ((sm >> (8 * e)) & 0xffu) continue;
      if (v4[e] > best) {
        best = v4[e];
        bi = 4 * q + e;
      }
    }
  }
  for (int c = 4 * V4 + threadIdx.x; c < V; c += 1024) {
    if (suppress && suppress[c]) continue;
    const float v = l[c];
    if (v > best || (v == best && c < bi)) {
      best = v;
      bi = c;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ob > best || (ob == best && oi < bi)) {
      best = ob;
      bi = oi;
    }
  }
  if (lane == 0) {
    sb[wave] = best;
    si[wave] = bi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 16; ++w)
      if (sb[w] > best || (sb[w] == best && si[w] < bi)) {
        best = sb[w];
        bi = si[w];
      }
    bi = bi == 0x7fffffff ? 0 : bi;
    out[row] = bi;
    if (adv.ids) {
      const int32_t p = adv.pos[row];
      const int32_t step = adv.done[row] ? adv.pad : bi;
      adv.ids[row * adv.ld_ids + p + 1] = step;
      if (step == adv.eos) adv.done[row] = 1;
      adv.tok[row] = step;
      adv.pos[row] = p + 1;
      adv.klen[row] += 1;
    }
  }
}

extern "C" int ca_argmax_masked(const float* logits, const uint8_t* suppress, int32_t* out,
                                int64_t rows, int32_t V, int64_t ldv, void* stream) {
  CA_CHECK_ARG(logits && out && rows > 0 && V > 0 && ldv >= V, "ca_argmax_masked: bad argument");
  ArgmaxAdvance none = {};
  hipLaunchKernelGGL(argmax_kernel, dim3((unsigned)rows), dim3(1024), 0, (hipStream_t)stream, logits,
                     suppress, out, rows, V, ldv, none);
  CA_CHECK_LAUNCH("ca_argmax_masked");
  return CA_OK;
}
extern "C" int ca_argmax_advance(const float* logits, const uint8_t* suppress, int32_t* out, int64_t rows, int32_t V,
                                 int64_t ldv, uint8_t* done, int64_t* ids, int64_t ld_ids, int32_t* tok, int32_t* pos,
                                 int32_t* klen, int32_t pad_id, int32_t eos_id, void* stream) {
  CA_CHECK_ARG(logits && out && rows > 0 && V > 0 && ldv >= V && done && ids && tok && pos && klen && ld_ids > 0,
               "ca_argmax_advance: bad argument");
  ArgmaxAdvance adv = {done, ids, ld_ids, tok, pos, klen, pad_id, eos_id};
  hipLaunchKernelGGL(argmax_kernel, dim3((unsigned)rows), dim3(1024), 0, (hipStream_t)stream, logits,
                     suppress, out, rows, V, ldv, adv);
  CA_CHECK_LAUNCH("ca_argmax_advance");
  return CA_OK;
}

// ---- timestamp-constrained argmax (greedy generation with return_timestamps) -------------------
// WhisperTimeStampLogitsProcessor ($TF/generation/logits_process.py) + the greedy pick in the launch of argmax_kernel,
// so the per-token graph keeps its shape.  Every rule of the processor masks an index range that is known before the
// row is read, so what is left is two windows - text [tx_lo, tx_hi) inside [0, timestamp_begin) without
// <|notimestamps|>, timestamps [ts_lo, ts_hi) inside [timestamp_begin, V) - and one pass carries the text max/argmax,
// the timestamp max/argmax and the timestamp sum of exp (rescaled online to the running max).  The processor's last
// rule, "the timestamps' total probability beats every text token", is logsumexp(timestamps) > max(text): the
// log-softmax normaliser is on both sides.
// The rules need the row's history since begin_index: was the last token a timestamp, the one before it, and the last
// timestamp.  Every wave finds them itself with a backward scan of the row of `ids` (at most max_target_positions
// int64, L2 hits after the first wave): no per-row state has to stay consistent between launches, and no barrier
// stands in front of the pass.
struct TimestampRules {
  const int64_t* ids;  // [rows, ld_ids] history; the row's generated tokens are ids[row, begin : pos[row] + 1]
  int64_t ld_ids;
  const int32_t* pos;  // [rows] position of the last token of the history
  int32_t begin, ts_begin, eos, cap;  // cap: max_initial_timestamp_index, < 0 = none
};
// (max, sum of exp(x - max)) of two disjoint sets -> of their union; an empty set is (-inf, 0)
__device__ __forceinline__ void lse_merge(float& m, float& s, float om, float os) {
  const float nm = fmaxf(m, om);
  if (nm == NEG_INF) {
    s = 0.f;
    return;
  }
  s = s * expf(m - nm) + os * expf(om - nm);  // expf(-inf) = 0 for the empty side
  m = nm;
}
__global__ __launch_bounds__(1024) void argmax_timestamps_kernel(const float* __restrict__ lg,
                                                                 const uint8_t* __restrict__ suppress,
                                                                 int32_t* __restrict__ out, int64_t rows, int V,
                                                                 int64_t ldv, const TimestampRules ts,
                                                                 const ArgmaxAdvance adv) {
  __shared__ float sb[16], s2b[16], s2s[16];
  __shared__ int si[16], s2i[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = blockIdx.x;
  const float* l = lg + row * ldv;
  // ---- the history: last / penultimate token a timestamp, the last timestamp ----
  const int64_t* seq = ts.ids + row * ts.ld_ids + ts.begin;
  int64_t end = (int64_t)ts.pos[row] + 1;
  end = end < ts.ld_ids ? end : ts.ld_ids;
  const int n = end > ts.begin ? (int)(end - ts.begin) : 0;
  int li = -1;  // index of the last timestamp in seq
  for (int i = n - 1 - lane; i >= 0; i -= 64)
    if (seq[i] >= ts.ts_begin) {
      li = i;
      break;
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int oi = __shfl_xor(li, o, 64);
    li = oi > li ? oi : li;
  }
  const bool last = n >= 1 && li == n - 1;
  const bool penult = n < 2 || seq[n - 2] >= ts.ts_begin;
  // ---- the windows ----
  const int tb = ts.ts_begin;
  int tx_lo = 0, tx_hi = tb, ts_lo = tb, ts_hi = V;
  if (last && penult) ts_hi = tb;       // a closed pair: text (or EOS) next
  if (last && !penult) tx_lo = ts.eos;  // an open segment's end: a timestamp or EOS next
  if (li >= 0) {                        // timestamps do not decrease; a new segment does not start at the same time
    const int64_t t = seq[li] + ((last && !penult) ? 0 : 1);
    ts_lo = t < (int64_t)V ? (int)t : V;
  }
  if (n == 0) {  // the first generated token is a timestamp, at most `cap` steps in
    tx_hi = 0;
    if (ts.cap >= 0 && (int64_t)tb + ts.cap + 1 < (int64_t)ts_hi) ts_hi = tb + ts.cap + 1;
  }
  const int no_ts = tb - 1;  // <|notimestamps|>
  float bt = NEG_INF, bs = NEG_INF, ss = 0.f;
  int bti = 0x7fffffff, bsi = 0x7fffffff;
  // candidates come to a thread in increasing index order: "strictly greater" keeps the lowest index of equal values
#define CA_TS_VISIT(c, v)                                                \
  do {                                                                   \
    if ((c) < tb) {                                                      \
      if ((c) >= tx_lo && (c) < tx_hi && (c) != no_ts && (v) > bt) {     \
        bt = (v);                                                        \
        bti = (c);                                                       \
      }                                                                  \
    } else if ((c) >= ts_lo && (c) < ts_hi && (v) > NEG_INF) {           \
      if ((v) > bs) {                                                    \
        ss = ss * expf(bs - (v)) + 1.f;                                  \
        bs = (v);                                                        \
        bsi = (c);                                                       \
      } else {                                                           \
        ss += expf((v) - bs);                                            \
      }                                                                  \
    }                                                                    \
  } while (0)
  const bool vec = ((ldv & 3) == 0) && ((((uintptr_t)lg) & 15) == 0) && (!suppress || (((uintptr_t)suppress) & 3) == 0);
  const int V4 = vec ? (V >> 2) : 0;
  for (int q = threadIdx.x; q < V4; q += 1024) {
    const f32x4_t v4 = *(const f32x4_t*)(l + 4 * q);
    const unsigned int sm = suppress ? *(const unsigned int*)(suppress + 4 * q) : 0u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if ((sm >> (8 * e)) & 0xffu) continue;
      const int c = 4 * q + e;
      const float v = v4[e];
      CA_TS_VISIT(c, v);
    }
  }
  for (int c = 4 * V4 + threadIdx.x; c < V; c += 1024) {  // (one candidate per thread at most when the row was vectorised)
    if (suppress && suppress[c]) continue;
    const float v = l[c];
    CA_TS_VISIT(c, v);
  }
#undef CA_TS_VISIT
  // the scalar tail visits indices above a thread's vector candidates, so the order above holds for it too; when the
  // row is not vectorised a thread's candidates are c, c + 1024, ..: increasing as well
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(bt, o, 64);
    const int oi = __shfl_xor(bti, o, 64);
    if (ob > bt || (ob == bt && oi < bti)) {
      bt = ob;
      bti = oi;
    }
    const float ob2 = __shfl_xor(bs, o, 64);
    const int oi2 = __shfl_xor(bsi, o, 64);
    const float os2 = __shfl_xor(ss, o, 64);
    if (ob2 > bs || (ob2 == bs && oi2 < bsi)) bsi = oi2;
    lse_merge(bs, ss, ob2, os2);
  }
  if (lane == 0) {
    sb[wave] = bt;
    si[wave] = bti;
    s2b[wave] = bs;
    s2i[wave] = bsi;
    s2s[wave] = ss;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 16; ++w) {
      if (sb[w] > bt || (sb[w] == bt && si[w] < bti)) {
        bt = sb[w];
        bti = si[w];
      }
      if (s2b[w] > bs || (s2b[w] == bs && s2i[w] < bsi)) bsi = s2i[w];
      lse_merge(bs, ss, s2b[w], s2s[w]);
    }
    const float lse = ss > 0.f ? bs + logf(ss) : NEG_INF;
    // timestamps win on their total probability; otherwise the best of both windows, text first on equal values (its
    // indices are the lower ones).  Nothing left at all: index 0, as argmax_kernel.
    int bi = lse > bt ? bsi : bti;  // (lse >= bs: a timestamp above every text token is covered)
    bi = bi == 0x7fffffff ? 0 : bi;
    out[row] = bi;
    if (adv.ids) {
      const int32_t p = adv.pos[row];
      const int32_t step = adv.done[row] ? adv.pad : bi;
      adv.ids[row * adv.ld_ids + p + 1] = step;
      if (step == adv.eos) adv.done[row] = 1;
      adv.tok[row] = step;
      adv.pos[row] = p + 1;
      adv.klen[row] += 1;
    }
  }
}

#define CA_CHECK_TS_ARGS(name)                                                                                        \
  CA_CHECK_ARG(ids && pos && ld_ids > 0 && begin_index >= 0 && timestamp_begin > 0 && timestamp_begin <= V &&         \
                   eos_id >= 0 && eos_id < timestamp_begin,                                                           \
               name ": bad timestamp argument (need 0 <= eos_id < timestamp_begin <= V, begin_index >= 0, a history)")

extern "C" int ca_argmax_timestamps(const float* logits, const uint8_t* suppress, int32_t* out, int64_t rows, int32_t V,
                                    int64_t ldv, const int64_t* ids, int64_t ld_ids, const int32_t* pos,
                                    int32_t begin_index, int32_t timestamp_begin, int32_t eos_id,
                                    int32_t max_initial_timestamp_index, void* stream) {
  CA_CHECK_ARG(logits && out && rows > 0 && V > 0 && ldv >= V, "ca_argmax_timestamps: bad argument");
  CA_CHECK_TS_ARGS("ca_argmax_timestamps");
  ArgmaxAdvance none = {};
  TimestampRules ts = {ids, ld_ids, pos, begin_index, timestamp_begin, eos_id, max_initial_timestamp_index};
  hipLaunchKernelGGL(argmax_timestamps_kernel, dim3((unsigned)rows), dim3(1024), 0, (hipStream_t)stream, logits,
                     suppress, out, rows, V, ldv, ts, none);
  CA_CHECK_LAUNCH("ca_argmax_timestamps");
  return CA_OK;
}
extern "C" int ca_argmax_timestamps_advance(const float* logits, const uint8_t* suppress, int32_t* out, int64_t rows,
                                            int32_t V, int64_t ldv, uint8_t* done, int64_t* ids, int64_t ld_ids,
                                            int32_t* tok, int32_t* pos, int32_t* klen, int32_t pad_id, int32_t eos_id,
                                            int32_t begin_index, int32_t timestamp_begin,
                                            int32_t max_initial_timestamp_index, void* stream) {
  CA_CHECK_ARG(logits && out && rows > 0 && V > 0 && ldv >= V && done && ids && tok && pos && klen && ld_ids > 0,
               "ca_argmax_timestamps_advance: bad argument");
  CA_CHECK_TS_ARGS("ca_argmax_timestamps_advance");
  ArgmaxAdvance adv = {done, ids, ld_ids, tok, pos, klen, pad_id, eos_id};
  TimestampRules ts = {ids, ld_ids, pos, begin_index, timestamp_begin, eos_id, max_initial_timestamp_index};
  hipLaunchKernelGGL(argmax_timestamps_kernel, dim3((unsigned)rows), dim3(1024), 0, (hipStream_t)stream, logits,
                     suppress, out, rows, V, ldv, ts, adv);
  CA_CHECK_LAUNCH("ca_argmax_timestamps_advance");
  return CA_OK;
}
