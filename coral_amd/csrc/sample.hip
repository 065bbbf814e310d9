// The scored pick of Whisper's temperature fallback (generate_with_fallback, $TF/models/whisper/generation_whisper.py):
// the greedy or sampled token of a decoding step together with its log-probability, in the launch that also keeps the
// step's books, and the no-speech probability of a prefix row.
#include "common.h"

#define NEG_INF (-__builtin_inff())

// ---- ca_pick_scored_advance ---------------------------------------------------------------------------------------------
// One 1024-thread workgroup per row, two passes over the row (the second one reads it from L2: 207 KB at V = 51 866).
//
// Pass 1 is the pass of argmax_timestamps_kernel (softmax.hip), statement for statement: the text and timestamp windows
// from the row's history, the text max / first argmax, the timestamp max / first argmax and the timestamps' sum of exp
// rescaled online, merged in the same order.  So the decision "logsumexp(timestamps) > max(text)" and with it the greedy
// token are the bits ca_argmax_timestamps_advance gives.  Without a history every index is "text" and the pass is the
// masked argmax of ca_argmax_advance (a first maximum does not depend on the order it is searched in).
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

struct PickRules {
  const int64_t* hist;  // [rows, ld_ids] history for the timestamp rules (the `ids` of the books), NULL: suppress mask alone
  int32_t begin, ts_begin, cap;
};
struct PickBooks {
  uint8_t* done;
  int64_t* ids;
  int64_t ld_ids;
  int32_t* tok;
  int32_t* pos;
  int32_t* klen;
  int32_t pad, eos;
  float* sum_logprob;  // [rows] += log-probability of the token of a row that had not finished
  int32_t* n_scored;   // [rows] += 1 for such a row
};

// (max, sum of exp(x - max)) of two disjoint sets -> of their union; an empty set is (-inf, 0)  [as softmax.hip]
__device__ __forceinline__ void ps_lse_merge(float& m, float& s, float om, float os) {
  const float nm = fmaxf(m, om);
  if (nm == NEG_INF) {
    s = 0.f;
    return;
  }
  s = s * expf(m - nm) + os * expf(om - nm);
  m = nm;
}
// inclusive scan over the 64 lanes, lane order (6 additions behind every value)
__device__ __forceinline__ float ps_wave_scan(float v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

__global__ __launch_bounds__(1024) void pick_scored_kernel(const float* __restrict__ lg,
                                                           const uint8_t* __restrict__ suppress,
                                                           int32_t* __restrict__ out, int64_t rows, int V, int64_t ldv,
                                                           float inv_t, const float* __restrict__ uniforms, int64_t ld_u,
                                                           const PickRules ru, const PickBooks bk) {
  __shared__ float sb[16], s2b[16], s2s[16];
  __shared__ int si[16], s2i[16], slast[16];
  __shared__ float seg_p[PS_MAX_SEG], seg_q[PS_MAX_SEG];
  __shared__ float bc_m;
  __shared__ int bc_forced, bc_greedy;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = blockIdx.x;
  const float* l = lg + row * ldv;
  const int32_t p0 = bk.pos[row];
  // ---- the windows (argmax_timestamps_kernel) ----
  int tb = V, tx_lo = 0, tx_hi = V, ts_lo = V, ts_hi = V, no_ts = -1;
  if (ru.hist) {
    const int64_t* seq = ru.hist + row * bk.ld_ids + ru.begin;
    int64_t end = (int64_t)p0 + 1;
    end = end < bk.ld_ids ? end : bk.ld_ids;
    const int n = end > ru.begin ? (int)(end - ru.begin) : 0;
    int li = -1;
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
    tb = ru.ts_begin;
    tx_hi = tb;
    ts_lo = tb;
    if (last && penult) ts_hi = tb;
    if (last && !penult) tx_lo = bk.eos;
    if (li >= 0) {
      const int64_t t = seq[li] + ((last && !penult) ? 0 : 1);
      ts_lo = t < (int64_t)V ? (int)t : V;
    }
    if (n == 0) {
      tx_hi = 0;
      if (ru.cap >= 0 && (int64_t)tb + ru.cap + 1 < (int64_t)ts_hi) ts_hi = tb + ru.cap + 1;
    }
    no_ts = tb - 1;
  }
  // ---- pass 1 ----
  float bt = NEG_INF, bs = NEG_INF, ss = 0.f;
  int bti = 0x7fffffff, bsi = 0x7fffffff;
#define CA_PS_VISIT(c, v)                                                \
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
      CA_PS_VISIT(c, v);
    }
  }
  for (int c = 4 * V4 + threadIdx.x; c < V; c += 1024) {
    if (suppress && suppress[c]) continue;
    const float v = l[c];
    CA_PS_VISIT(c, v);
  }
#undef CA_PS_VISIT
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
    ps_lse_merge(bs, ss, ob2, os2);
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
      ps_lse_merge(bs, ss, s2b[w], s2s[w]);
    }
    const float lse = ss > 0.f ? bs + logf(ss) : NEG_INF;
    const bool forced = lse > bt;  // the timestamps' total probability beats every text token: the text window is empty
    int bi = forced ? bsi : bti;
    bi = bi == 0x7fffffff ? 0 : bi;
    bc_greedy = bi;
    bc_forced = forced ? 1 : 0;
    bc_m = forced ? bs : fmaxf(bt, bs);
  }
  __syncthreads();
  const float m = bc_m;
  const bool forced = bc_forced != 0;
  const bool sampled = inv_t > 0.f;
  const bool live = m > NEG_INF;  // something is allowed
  // ---- pass 2: the segments' totals ----
  const int nseg = (V + PS_SEG - 1) / PS_SEG;
  int lastpos = -1;  // the last allowed index with p > 0 this thread saw
  // the four values of this lane in segment s: q[e], p[e] (0 outside the allowed set)
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
      bool ok = c < V && !((sm >> (8 * e)) & 0xffu) && x[e] > NEG_INF;                                     \
      if (c < tb)                                                                                          \
        ok = ok && !forced && c >= tx_lo && c < tx_hi && c != no_ts;                                       \
      else                                                                                                 \
        ok = ok && c >= ts_lo && c < ts_hi;                                                                \
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
      const bool was_done = bk.done[row] != 0;
      const int32_t step = was_done ? bk.pad : tok;
      if ((int64_t)p0 + 1 >= 0 && (int64_t)p0 + 1 < bk.ld_ids) bk.ids[row * bk.ld_ids + p0 + 1] = step;
      if (step == bk.eos) bk.done[row] = 1;
      bk.tok[row] = step;
      bk.pos[row] = p0 + 1;
      bk.klen[row] += 1;
      if (!was_done) {
        // log softmax of the allowed set at temperature 1 (the temperature undone, as _retrieve_avg_logprobs does)
        if (live) bk.sum_logprob[row] += (l[tok] - m) - logf(Q);
        bk.n_scored[row] += 1;
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
  CA_CHECK_ARG(!history || (begin_index >= 0 && timestamp_begin > 0 && timestamp_begin <= V && eos_id >= 0 &&
                            eos_id < timestamp_begin),
               "ca_pick_scored_advance: bad timestamp argument (need 0 <= eos_id < timestamp_begin <= V, begin_index >= 0)");
  PickRules ru = {history, begin_index, timestamp_begin, max_initial_timestamp_index};
  PickBooks bk = {done, ids, ld_ids, tok, pos, klen, pad_id, eos_id, sum_logprob, n_scored};
  hipLaunchKernelGGL(pick_scored_kernel, dim3((unsigned)rows), dim3(1024), 0, (hipStream_t)stream, logits, suppress, out,
                     rows, V, ldv, inv_temperature, uniforms, ld_u, ru, bk);
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
