// From a row of logits to a token (Whisper generation): the greedy picks (masked argmax, with Whisper's timestamp rules,
// with the step's bookkeeping), the scored pick of the temperature fallback (generate_with_fallback,
// $TF/models/whisper/generation_whisper.py: the greedy or sampled token together with its log-probability), and the
// no-speech probability of a prefix row.  Every pick runs the same first pass (pick_first_pass) and keeps the step's
// books with the same function (pick_advance), so the greedy mode of the scored pick gives the greedy launches' bits.
#include "common.h"

#define NEG_INF (-__builtin_inff())

// ---- the timestamp rules ------------------------------------------------------------------------------------------------
// WhisperTimeStampLogitsProcessor ($TF/generation/logits_process.py).  Every rule of the processor masks an index range
// that is known before the row is read, so what is left is two windows - text [tx_lo, tx_hi) inside [0, timestamp_begin)
// without <|notimestamps|>, timestamps [ts_lo, ts_hi) inside [timestamp_begin, V) - and one pass carries the text
// max/argmax, the timestamp max/argmax and the timestamp sum of exp (rescaled online to the running max).  The processor's
// last rule, "the timestamps' total probability beats every text token", is logsumexp(timestamps) > max(text): the
// log-softmax normaliser is on both sides.
// The rules need the row's history since begin_index: was the last token a timestamp, the one before it, and the last
// timestamp.  Every wave finds them itself with a backward scan of the row of `ids` (at most max_target_positions
// int64, L2 hits after the first wave): no per-row state has to stay consistent between launches, and no barrier
// stands in front of the pass.
struct PickRules {
  const int64_t* hist;  // [rows, ld] history; the row's generated tokens are hist[row, begin : pos[row] + 1].  NULL: no rules
  int64_t ld;
  const int32_t* pos;   // [rows] position of the last token of the history
  int32_t begin, ts_begin, eos, cap;  // cap: max_initial_timestamp_index, < 0 = none
};
struct PickWindows {
  int tb, tx_lo, tx_hi, ts_lo, ts_hi, no_ts;  // indices below tb are text, no_ts is <|notimestamps|>
};
// without a history everything is text: the suppress mask alone
__device__ __forceinline__ PickWindows pick_windows(const PickRules& ru, int64_t row, int V) {
  PickWindows w = {V, 0, V, V, V, -1};
  if (!ru.hist) return w;
  const int lane = threadIdx.x & 63;
  // ---- the history: last / penultimate token a timestamp, the last timestamp ----
  const int64_t* seq = ru.hist + row * ru.ld + ru.begin;
  int64_t end = (int64_t)ru.pos[row] + 1;
  end = end < ru.ld ? end : ru.ld;
  const int n = end > ru.begin ? (int)(end - ru.begin) : 0;
  int li = -1;  // index of the last timestamp in seq
  for (int i = n - 1 - lane; i >= 0; i -= 64)
    if (seq[i] >= ru.ts_begin) {
      li = i;
      break;
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int oi = __shfl_xor(li, o, 64);
    li = oi > li ? oi : li;
  }
  const bool last = n >= 1 && li == n - 1;
  const bool penult = n < 2 || seq[n - 2] >= ru.ts_begin;
  // ---- the windows ----
  const int tb = ru.ts_begin;
  w = {tb, 0, tb, tb, V, tb - 1};
  if (last && penult) w.ts_hi = tb;       // a closed pair: text (or EOS) next
  if (last && !penult) w.tx_lo = ru.eos;  // an open segment's end: a timestamp or EOS next
  if (li >= 0) {                          // timestamps do not decrease; a new segment does not start at the same time
    const int64_t t = seq[li] + ((last && !penult) ? 0 : 1);
    w.ts_lo = t < (int64_t)V ? (int)t : V;
  }
  if (n == 0) {  // the first generated token is a timestamp, at most `cap` steps in
    w.tx_hi = 0;
    if (ru.cap >= 0 && (int64_t)tb + ru.cap + 1 < (int64_t)w.ts_hi) w.ts_hi = tb + ru.cap + 1;
  }
  return w;
}
// is index c left by the rules?  forced: the timestamps won on their total probability, which empties the text window
__device__ __forceinline__ bool pick_allowed(const PickWindows& w, int c, bool forced) {
  return c < w.tb ? (!forced && c >= w.tx_lo && c < w.tx_hi && c != w.no_ts) : (c >= w.ts_lo && c < w.ts_hi);
}

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

// ---- the first pass -----------------------------------------------------------------------------------------------------
struct PickFirst {
  float bt;  // the text window's maximum and its first index (0x7fffffff: the window is empty)
  int bti;
  float bs;  // the timestamp window's, with ss = its sum of exp(x - bs)
  int bsi;
  float ss;
};
// RULES = false: no windows, every index is text and only (bt, bti) is carried
template <bool RULES>
__device__ __forceinline__ void pick_visit(const PickWindows& w, int c, float v, PickFirst& f) {
  if (!RULES || c < w.tb) {
    if ((!RULES || pick_allowed(w, c, false)) && v > f.bt) {
      f.bt = v;
      f.bti = c;
    }
  } else if (pick_allowed(w, c, false) && v > NEG_INF) {
    if (v > f.bs) {
      f.ss = f.ss * expf(f.bs - v) + 1.f;
      f.bs = v;
      f.bsi = c;
    } else {
      f.ss += expf(v - f.bs);
    }
  }
}
// four logits (and their four suppress bytes) per load where the row is 16-byte aligned
__device__ __forceinline__ bool pick_vec(const float* lg, int64_t ldv, const uint8_t* suppress) {
  return ((ldv & 3) == 0) && ((((uintptr_t)lg) & 15) == 0) && (!suppress || (((uintptr_t)suppress) & 3) == 0);
}
// One 1024-thread workgroup walks the row l[0 : V) once; the result is complete on thread 0.
template <bool RULES>
__device__ __forceinline__ PickFirst pick_first_pass(const float* __restrict__ l, const uint8_t* __restrict__ suppress,
                                                     bool vec, int V, const PickWindows& w) {
  __shared__ float sb[16], s2b[16], s2s[16];
  __shared__ int si[16], s2i[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  PickFirst f = {NEG_INF, 0x7fffffff, NEG_INF, 0x7fffffff, 0.f};
  // candidates come to a thread in increasing index order: "strictly greater" keeps the lowest index of equal values
  const int V4 = vec ? (V >> 2) : 0;
  for (int q = threadIdx.x; q < V4; q += 1024) {
    const f32x4_t v4 = *(const f32x4_t*)(l + 4 * q);
    const unsigned int sm = suppress ? *(const unsigned int*)(suppress + 4 * q) : 0u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if ((sm >> (8 * e)) & 0xffu) continue;
      pick_visit<RULES>(w, 4 * q + e, v4[e], f);
    }
  }
  for (int c = 4 * V4 + threadIdx.x; c < V; c += 1024) {  // (one candidate per thread at most when the row was vectorised)
    if (suppress && suppress[c]) continue;
    pick_visit<RULES>(w, c, l[c], f);
  }
  // the scalar tail visits indices above a thread's vector candidates, so the order above holds for it too; when the
  // row is not vectorised a thread's candidates are c, c + 1024, ..: increasing as well
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(f.bt, o, 64);
    const int oi = __shfl_xor(f.bti, o, 64);
    if (ob > f.bt || (ob == f.bt && oi < f.bti)) {
      f.bt = ob;
      f.bti = oi;
    }
    if (RULES) {
      const float ob2 = __shfl_xor(f.bs, o, 64);
      const int oi2 = __shfl_xor(f.bsi, o, 64);
      const float os2 = __shfl_xor(f.ss, o, 64);
      if (ob2 > f.bs || (ob2 == f.bs && oi2 < f.bsi)) f.bsi = oi2;
      lse_merge(f.bs, f.ss, ob2, os2);
    }
  }
  if (lane == 0) {
    sb[wave] = f.bt;
    si[wave] = f.bti;
    if (RULES) {
      s2b[wave] = f.bs;
      s2i[wave] = f.bsi;
      s2s[wave] = f.ss;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w_ = 1; w_ < 16; ++w_) {
      if (sb[w_] > f.bt || (sb[w_] == f.bt && si[w_] < f.bti)) {
        f.bt = sb[w_];
        f.bti = si[w_];
      }
      if (RULES) {
        if (s2b[w_] > f.bs || (s2b[w_] == f.bs && s2i[w_] < f.bsi)) f.bsi = s2i[w_];
        lse_merge(f.bs, f.ss, s2b[w_], s2s[w_]);
      }
    }
  }
  return f;
}
// the greedy token of a finished first pass, and whether the timestamps won on their total probability (`forced`);
// otherwise the best of both windows, text first on equal values (its indices are the lower ones).  Nothing left at
// all: index 0.
__device__ __forceinline__ int pick_greedy_token(const PickFirst& f, bool& forced) {
  const float lse = f.ss > 0.f ? f.bs + logf(f.ss) : NEG_INF;
  forced = lse > f.bt;  // (lse >= bs: a timestamp above every text token is covered)
  const int bi = forced ? f.bsi : f.bti;
  return bi == 0x7fffffff ? 0 : bi;
}

// ---- the bookkeeping of a decoding step ---------------------------------------------------------------------------------
// in the launch of the pick: the row's last thread also records the token and moves the row's cursors (eight tiny
// dependent launches per decoded token otherwise, ~4 us each in a graph)
struct PickBooks {
  uint8_t* done;    // [rows] finished flags (a finished row records pad)
  int64_t* ids;     // [rows, ld_ids] generated ids; the token goes to column pos[row] + 1.  NULL: no bookkeeping
  int64_t ld_ids;
  int32_t* tok;     // [rows] next input token
  int32_t* pos;     // [rows] position of the token just fed (+1 here)
  int32_t* klen;    // [rows] cached keys (+1 here)
  int32_t pad, eos;
};
// -> whether the row had finished before this step.  A column outside the row is not stored; the cursors still move.
__device__ __forceinline__ bool pick_advance(const PickBooks& bk, int64_t row, int32_t token) {
  const bool was_done = bk.done[row] != 0;
  const int64_t col = (int64_t)bk.pos[row] + 1;
  const int32_t step = was_done ? bk.pad : token;
  if (col >= 0 && col < bk.ld_ids) bk.ids[row * bk.ld_ids + col] = step;
  if (step == bk.eos) bk.done[row] = 1;
  bk.tok[row] = step;
  bk.pos[row] = (int32_t)col;
  bk.klen[row] += 1;
  return was_done;
}

// ---- the greedy picks ---------------------------------------------------------------------------------------------------
// one 1024-thread workgroup per row (greedy decoding has B rows of ~52 k logits: a wave per row would walk
// 800 dependent loads); ties resolve to the lowest index like torch.argmax.
template <bool RULES>
__global__ __launch_bounds__(1024) void pick_greedy_kernel(const float* __restrict__ lg,
                                                           const uint8_t* __restrict__ suppress,
                                                           int32_t* __restrict__ out, int V, int64_t ldv,
                                                           const PickRules ru, const PickBooks bk) {
  const int64_t row = blockIdx.x;
  const PickWindows w = pick_windows(RULES ? ru : PickRules{}, row, V);
  const PickFirst f = pick_first_pass<RULES>(lg + row * ldv, suppress, pick_vec(lg, ldv, suppress), V, w);
  if (threadIdx.x == 0) {
    bool forced;
    const int bi = pick_greedy_token(f, forced);
    out[row] = bi;
    if (bk.ids) pick_advance(bk, row, bi);
  }
}

static bool pick_ts_args_ok(int32_t V, int32_t begin_index, int32_t timestamp_begin, int32_t eos_id) {
  return begin_index >= 0 && timestamp_begin > 0 && timestamp_begin <= V && eos_id >= 0 && eos_id < timestamp_begin;
}
#define CA_CHECK_TS_ARGS(name)                                                                                        \
  CA_CHECK_ARG(ids && pos && ld_ids > 0 && pick_ts_args_ok(V, begin_index, timestamp_begin, eos_id),                  \
               name ": bad timestamp argument (need 0 <= eos_id < timestamp_begin <= V, begin_index >= 0, a history)")
#define CA_LAUNCH_GREEDY(RULES, ru, bk)                                                                                \
  hipLaunchKernelGGL(pick_greedy_kernel<RULES>, dim3((unsigned)rows), dim3(1024), 0, (hipStream_t)stream, logits,     \
                     suppress, out, V, ldv, ru, bk)

extern "C" int ca_argmax_masked(const float* logits, const uint8_t* suppress, int32_t* out,
                                int64_t rows, int32_t V, int64_t ldv, void* stream) {
  CA_CHECK_ARG(logits && out && rows > 0 && V > 0 && ldv >= V, "ca_argmax_masked: bad argument");
  CA_LAUNCH_GREEDY(false, PickRules{}, PickBooks{});
  CA_CHECK_LAUNCH("ca_argmax_masked");
  return CA_OK;
}
extern "C" int ca_argmax_advance(const float* logits, const uint8_t* suppress, int32_t* out, int64_t rows, int32_t V,
                                 int64_t ldv, uint8_t* done, int64_t* ids, int64_t ld_ids, int32_t* tok, int32_t* pos,
                                 int32_t* klen, int32_t pad_id, int32_t eos_id, void* stream) {
  CA_CHECK_ARG(logits && out && rows > 0 && V > 0 && ldv >= V && done && ids && tok && pos && klen && ld_ids > 0,
               "ca_argmax_advance: bad argument");
  const PickBooks bk = {done, ids, ld_ids, tok, pos, klen, pad_id, eos_id};
  CA_LAUNCH_GREEDY(false, PickRules{}, bk);
  CA_CHECK_LAUNCH("ca_argmax_advance");
  return CA_OK;
}
extern "C" int ca_argmax_timestamps(const float* logits, const uint8_t* suppress, int32_t* out, int64_t rows, int32_t V,
                                    int64_t ldv, const int64_t* ids, int64_t ld_ids, const int32_t* pos,
                                    int32_t begin_index, int32_t timestamp_begin, int32_t eos_id,
                                    int32_t max_initial_timestamp_index, void* stream) {
  CA_CHECK_ARG(logits && out && rows > 0 && V > 0 && ldv >= V, "ca_argmax_timestamps: bad argument");
  CA_CHECK_TS_ARGS("ca_argmax_timestamps");
  const PickRules ru = {ids, ld_ids, pos, begin_index, timestamp_begin, eos_id, max_initial_timestamp_index};
  CA_LAUNCH_GREEDY(true, ru, PickBooks{});
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
  const PickRules ru = {ids, ld_ids, pos, begin_index, timestamp_begin, eos_id, max_initial_timestamp_index};
  const PickBooks bk = {done, ids, ld_ids, tok, pos, klen, pad_id, eos_id};
  CA_LAUNCH_GREEDY(true, ru, bk);
  CA_CHECK_LAUNCH("ca_argmax_timestamps_advance");
  return CA_OK;
}

// ---- ca_pick_scored_advance ---------------------------------------------------------------------------------------------
// One 1024-thread workgroup per row, two passes over the row (the second one reads it from L2: 207 KB at V = 51 866).
//
// Pass 1 is pick_first_pass with the rules, the function ca_argmax_timestamps_advance runs: the decision
// "logsumexp(timestamps) > max(text)" and with it the greedy token are that launch's bits.  Without a history every
// index is "text" and the pass is the masked argmax of ca_argmax_advance (a first maximum does not depend on the order
// it is searched in).
//
// Pass 2 walks the allowed set in index order in segments of 256 (a wave reads one segment per load, four consecutive
// logits per lane), with m = the allowed set's maximum:
//   q_i = exp(x_i - m)             its sum Q gives logsumexp at temperature 1 = m + log Q (the log-probability's base)
//   p_i = exp((x_i - m) * inv_T)   the sampling weights, S = sum p_i
// A segment's totals are 3 additions in the lane and 6 in the wave's butterfly; they go to LDS by segment number.  Wave 0
// scans them: a lane owns ceil(nseg / 64) <= 16 consecutive segments (<= 15 additions), then a 6-step scan over the lanes.
// The segment that holds target = u * S is the first whose inclusive prefix exceeds it; wave 0 reads that segment again
// (the same expressions give the same p_i) and scans its 256 values: 3 additions in the lane, 6 over the lanes, 2 to
// attach the bases.  No prefix value sits behind more than 3 + 6 + 15 + 6 + 3 + 6 + 2 = 41 fp32 additions, the order is
// fixed, and nothing is atomic: a run is reproducible to the bit.
#define PS_SEG 256
#define PS_MAX_SEG 1024  // V <= 262144; a lane of the scanning wave owns at most PS_MAX_SEG / 64 = 16 segments

// inclusive scan over the 64 lanes, lane order (6 additions behind every value)
__device__ __forceinline__ float ps_wave_scan(float v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// sum_logprob [rows] += log-probability of the token of a row that had not finished, n_scored [rows] += 1 for such a row
__global__ __launch_bounds__(1024) void pick_scored_kernel(const float* __restrict__ lg,
                                                           const uint8_t* __restrict__ suppress,
                                                           int32_t* __restrict__ out, int V, int64_t ldv, float inv_t,
                                                           const float* __restrict__ uniforms, int64_t ld_u,
                                                           float* __restrict__ sum_logprob,
                                                           int32_t* __restrict__ n_scored, const PickRules ru,
                                                           const PickBooks bk) {
  __shared__ int slast[16];
  __shared__ float seg_p[PS_MAX_SEG], seg_q[PS_MAX_SEG];
  __shared__ float bc_m;
  __shared__ int bc_forced, bc_greedy;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = blockIdx.x;
  const float* l = lg + row * ldv;
  const int32_t p0 = bk.pos[row];
  const bool vec = pick_vec(lg, ldv, suppress);
  // ---- pass 1 ----
  const PickWindows w = pick_windows(ru, row, V);
  const PickFirst f = pick_first_pass<true>(l, suppress, vec, V, w);
  if (threadIdx.x == 0) {
    bool forced;
    bc_greedy = pick_greedy_token(f, forced);
    bc_forced = forced ? 1 : 0;
    bc_m = forced ? f.bs : fmaxf(f.bt, f.bs);
  }
  __syncthreads();
  const float m = bc_m;
  const bool forced = bc_forced != 0;
  const bool sampled = inv_t > 0.f;
  const bool live = m > NEG_INF;  // something is allowed
  // ---- pass 2: the segments' totals ----
  const int nseg = (V + PS_SEG - 1) / PS_SEG;
  int lastpos = -1;  // the last allowed index with p > 0 this thread saw
  // the four values of this lane in segment s: q[e], p[e] (0 outside the allowed set).  `ok` is formed with & on purpose:
  // with && the predicate became exec-mask branches around each compare, 1.3 us of the launch's 40 at 16 x 51 865
#define CA_PS_LOAD(s, qv, pv)                                                                              \
  do {                                                                                                     \
    const int c0 = (s) * PS_SEG + 4 * lane;                                                                \
    float x[4];                                                                                            \
    unsigned int sm = 0u;                                                                                  \
    if (vec && c0 + 3 < V) {                                                                               \
      const f32x4_t v4 = *(const f32x4_t*)(l + c0);                                                        \
      x[0] = v4[0], x[1] = v4[1], x[2] = v4[2], x[3] = v4[3];                                              \
      if (suppress) sm = *(const unsigned int*)(suppress + c0);                                            \
    } else {                                                                                               \
      _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                      \
        const int c = c0 + e;                                                                              \
        x[e] = c < V ? l[c] : NEG_INF;                                                                     \
        if (c < V && suppress && suppress[c]) sm |= 0xffu << (8 * e);                                      \
      }                                                                                                    \
    }                                                                                                      \
    _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                        \
      const int c = c0 + e;                                                                                \
      const bool ok = (c < V) & !((sm >> (8 * e)) & 0xffu) & (x[e] > NEG_INF) & pick_allowed(w, c, forced); \
      const float a = x[e] - m;                                                                            \
      qv[e] = ok ? expf(a) : 0.f;                                                                          \
      pv[e] = ok ? (sampled ? expf(a * inv_t) : qv[e]) : 0.f;                                              \
    }                                                                                                      \
  } while (0)
  if (live) {
    for (int s = wave; s < nseg; s += 16) {
      float qv[4], pv[4];
      CA_PS_LOAD(s, qv, pv);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (pv[e] > 0.f) lastpos = s * PS_SEG + 4 * lane + e;
      const float tq = wave_sum(((qv[0] + qv[1]) + qv[2]) + qv[3]);
      const float tp = wave_sum(((pv[0] + pv[1]) + pv[2]) + pv[3]);
      if (lane == 0) {
        seg_q[s] = tq;
        seg_p[s] = tp;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int oi = __shfl_xor(lastpos, o, 64);
    lastpos = oi > lastpos ? oi : lastpos;
  }
  if (lane == 0) slast[wave] = lastpos;
  __syncthreads();
  // ---- wave 0: scan the segments, find the one that holds the target, then the token in it ----
  if (wave == 0) {
    int tok = bc_greedy;
    float Q = 0.f;
    if (live) {
      const int per = (nseg + 63) / 64;  // <= 16
      const int s0 = lane * per;
      float lp = 0.f, lq = 0.f;
      for (int k = 0; k < per; ++k)
        if (s0 + k < nseg) {
          lp += seg_p[s0 + k];
          lq += seg_q[s0 + k];
        }
      const float ip = ps_wave_scan(lp, lane), iq = ps_wave_scan(lq, lane);
      const float S = __shfl(ip, 63, 64);
      Q = __shfl(iq, 63, 64);
      if (sampled) {
        int64_t ui = (int64_t)p0 + 1;
        ui = ui < 0 ? 0 : (ui < ld_u ? ui : ld_u - 1);
        const float u = uniforms[row * ld_u + ui];
        const float target = u * S;
        // the first segment whose inclusive prefix exceeds the target, and the prefix in front of it
        const float up = __shfl_up(ip, 1, 64);
        const float ex = lane ? up : 0.f;  // this lane's exclusive prefix
        int fs = 0x7fffffff;
        float fbase = 0.f, run = 0.f;
        for (int k = 0; k < per; ++k)
          if (s0 + k < nseg) {
            const float before = run;
            run += seg_p[s0 + k];
            if (fs == 0x7fffffff && ex + run > target) {
              fs = s0 + k;
              fbase = ex + before;
            }
          }
        int best = fs;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const int ob = __shfl_xor(best, o, 64);
          best = ob < best ? ob : best;
        }
        if (best == 0x7fffffff) {  // rounding left none: the last allowed token with mass
          int lp2 = slast[lane & 15];
#pragma unroll
          for (int o = 8; o > 0; o >>= 1) {
            const int ob = __shfl_xor(lp2, o, 64);
            lp2 = ob > lp2 ? ob : lp2;
          }
          tok = lp2 >= 0 ? lp2 : tok;
        } else {
          const int owner = best / per;
          const float base = __shfl(fbase, owner, 64);
          float qv[4], pv[4];
          CA_PS_LOAD(best, qv, pv);
          const float c1 = pv[0], c2 = c1 + pv[1], c3 = c2 + pv[2], c4 = c3 + pv[3];
          const float up4 = __shfl_up(ps_wave_scan(c4, lane), 1, 64);
          const float lex = base + (lane ? up4 : 0.f);
          const float cs[4] = {c1, c2, c3, c4};
          int hit = 0x7fffffff, lastm = -1;
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (pv[e] > 0.f) {
              const int c = best * PS_SEG + 4 * lane + e;
              lastm = c;
              if (hit == 0x7fffffff && lex + cs[e] > target) hit = c;
            }
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) {
            const int oh = __shfl_xor(hit, o, 64);
            hit = oh < hit ? oh : hit;
            const int ol = __shfl_xor(lastm, o, 64);
            lastm = ol > lastm ? ol : lastm;
          }
          tok = hit != 0x7fffffff ? hit : (lastm >= 0 ? lastm : tok);
        }
      }
    }
    if (lane == 0) {
      out[row] = tok;
      if (!pick_advance(bk, row, tok)) {
        // log softmax of the allowed set at temperature 1 (the temperature undone, as _retrieve_avg_logprobs does)
        if (live) sum_logprob[row] += (l[tok] - m) - logf(Q);
        n_scored[row] += 1;
      }
    }
  }
#undef CA_PS_LOAD
}

extern "C" int ca_pick_scored_advance(const float* logits, const uint8_t* suppress, int32_t* out, int64_t rows, int32_t V,
                                      int64_t ldv, float inv_temperature, const float* uniforms, int64_t ld_u,
                                      float* sum_logprob, int32_t* n_scored, uint8_t* done, int64_t* ids, int64_t ld_ids,
                                      int32_t* tok, int32_t* pos, int32_t* klen, int32_t pad_id, int32_t eos_id,
                                      const int64_t* history, int32_t begin_index, int32_t timestamp_begin,
                                      int32_t max_initial_timestamp_index, void* stream) {
  CA_CHECK_ARG(logits && out && rows > 0 && V > 0 && (ldv >= V || ldv == 0) && done && ids && tok && pos && klen &&
                   ld_ids > 0 && sum_logprob && n_scored,
               "ca_pick_scored_advance: bad argument");
  CA_CHECK_ARG(V <= PS_SEG * PS_MAX_SEG, "ca_pick_scored_advance: V = %d exceeds %d", V, PS_SEG * PS_MAX_SEG);
  CA_CHECK_ARG(inv_temperature >= 0.f && inv_temperature < __builtin_inff(),
               "ca_pick_scored_advance: inv_temperature must be 0 (greedy) or a positive finite number");
  CA_CHECK_ARG(inv_temperature == 0.f || (uniforms && ld_u > 0),
               "ca_pick_scored_advance: sampling needs the uniforms matrix [rows, ld_u]");
  CA_CHECK_ARG(!history || pick_ts_args_ok(V, begin_index, timestamp_begin, eos_id),
               "ca_pick_scored_advance: bad timestamp argument (need 0 <= eos_id < timestamp_begin <= V, begin_index >= 0)");
  const PickRules ru = {history, ld_ids, pos, begin_index, timestamp_begin, eos_id, max_initial_timestamp_index};
  const PickBooks bk = {done, ids, ld_ids, tok, pos, klen, pad_id, eos_id};
  hipLaunchKernelGGL(pick_scored_kernel, dim3((unsigned)rows), dim3(1024), 0, (hipStream_t)stream, logits, suppress, out,
                     V, ldv, inv_temperature, uniforms, ld_u, sum_logprob, n_scored, ru, bk);
  CA_CHECK_LAUNCH("ca_pick_scored_advance");
  return CA_OK;
}

// ---- ca_row_token_prob ----------------------------------------------------------------------------------------------------
// out[r] = softmax(logits[r, :V])[token] over the raw row: WhisperNoSpeechDetection's probability of <|nospeech|> at the
// start-of-transcript position.  One 1024-thread workgroup per row; a thread adds ceil(V / 1024) terms, then 6 + 15.
__global__ __launch_bounds__(1024) void row_token_prob_kernel(const float* __restrict__ lg, float* __restrict__ out, int V,
                                                              int64_t ldv, int token) {
  __shared__ float red[16];
  __shared__ float bc;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* l = lg + (int64_t)blockIdx.x * ldv;
  float mx = NEG_INF;
  for (int c = threadIdx.x; c < V; c += 1024) mx = fmaxf(mx, l[c]);
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
  for (int c = threadIdx.x; c < V; c += 1024) sum += expf(l[c] - mx);
  sum = wave_sum(sum);
  __syncthreads();
  if (lane == 0) red[wave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int w = 0; w < 16; ++w) s += red[w];
    out[blockIdx.x] = expf(l[token] - mx) / s;
  }
}

extern "C" int ca_row_token_prob(const float* logits, float* out, int64_t rows, int32_t V, int64_t ldv, int32_t token,
                                 void* stream) {
  CA_CHECK_ARG(logits && out && rows > 0 && V > 0 && ldv >= V && token >= 0 && token < V, "ca_row_token_prob: bad argument");
  hipLaunchKernelGGL(row_token_prob_kernel, dim3((unsigned)rows), dim3(1024), 0, (hipStream_t)stream, logits, out, V, ldv,
                     token);
  CA_CHECK_LAUNCH("ca_row_token_prob");
  return CA_OK;
}
