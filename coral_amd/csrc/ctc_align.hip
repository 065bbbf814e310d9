// CTC forced alignment: the single most probable alignment of a given label string to the frames (Viterbi over the
// blank-interleaved states), for word / character times of a known transcript - the string the LM beam search
// returned, or one the caller brings.  Contract, tie rule and outputs: include/coral_amd.h.
//
//   lp[t][v] = logit[t][v] - logsumexp_v(logit[t][:V])                                  (fp32)
//   states s = 0 .. 2L, l'_s = blank (s even) | labels[(s - 1) / 2] (s odd)
//   v_0(0) = lp[0][blank], v_0(1) = lp[0][l_0], every other v_0 = -inf
//   v_t(s) = lp[t][l'_s] + max(v_{t-1}(s), v_{t-1}(s-1), v_{t-1}(s-2) if s odd and l'_s != l'_{s-2})
//   ties: the smaller move wins (stay, then s-1, then s-2); at the end a tie between 2L and 2L-1 takes 2L.
//
// Two launches.  The per-frame logsumexp (wave per frame, whole chip) goes to the workspace, so a log-probability is
// one gathered logit minus one broadcast value.  Then one workgroup per utterance walks the T sequential frames,
// which is the latency bound, in one of two regimes chosen by Lmax (as ctc_kernel in ctc.hip):
//   Lmax <= 127: one wave, 4 states per lane.  Lane l owns states 4l .. 4l+3; 4l is a blank state and takes no s-2
//     move, so the only value a lane needs from outside is state 4l-1 of lane l-1: one lane shift (DPP wave_shr) per
//     frame, no exchange through LDS and no barrier inside a step.
//   above: up to 1024 threads, 8 states per thread (8191 states), the same single neighbour value through two LDS
//     rows (ping-pong), one barrier per frame.
// Both keep v in registers and run the same max / add sequence per state, so a row's result does not depend on the
// regime, on its position in the batch or on the run.  The gathers of lp[t][l'_s] stay off the sequential chain's
// global-memory latency: the frames are walked in chunks whose logits and logsumexps sit in LDS, and the loads of the
// next chunk are in flight while the current one is walked (two buffers), so a step gathers with LDS reads only.
// Back-pointers: 2 bits per state and frame (the move 0 / 1 / 2), state s in byte s / 4 at bits 2 (s % 4) of the
// frame's row of the workspace - a lane stores one byte per frame, a thread of the wide regime one 16-bit word.
// The backtrace is sequential over T: wave 0 stages the back-pointer window of 64 frames in LDS (the state falls by
// at most 2 per frame, so 48 bytes per frame cover it: every lane fetches one frame's window with three 16-byte
// loads) and walks it, writing start / end as the path enters and leaves a label state.  tok_score is then one
// sequential fp32 sum per token over its own frames, a thread per token.
#include "common.h"

#define NEG_INF (-__builtin_inff())
#define ALN_WIN 48  // bytes of one frame's back-pointer row staged for the backtrace (3 x 16)

__host__ __device__ static inline int64_t aln_align256(int64_t x) { return (x + 255) & ~(int64_t)255; }
// bytes of one frame's back-pointer row: 4 states per byte, a multiple of 16 and at least one window
__host__ __device__ static inline int64_t aln_row_bytes(int Lmax) {
  const int64_t bytes = ((2 * (int64_t)Lmax + 1 + 3) / 4 + 15) & ~(int64_t)15;
  return bytes < ALN_WIN ? ALN_WIN : bytes;
}

extern "C" int64_t ca_ctc_align_workspace_bytes(int32_t B, int32_t T, int32_t Lmax) {
  if (B <= 0 || T <= 0 || Lmax < 0) return 0;
  return aln_align256((int64_t)B * T * 4) + aln_align256((int64_t)B * T * aln_row_bytes(Lmax));
}

// logsumexp of every frame (wave per frame, the whole chip)
__global__ __launch_bounds__(256) void ctc_align_lse_kernel(const float* __restrict__ logits, float* __restrict__ lse,
                                                            int64_t frames, int V, int64_t ldv) {
  const int lane = threadIdx.x & 63;
  const int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= frames) return;
  const float* l = logits + f * ldv;
  float x[4];  // V <= 256
  float mx = NEG_INF;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int v = lane + 64 * j;
    x[j] = v < V ? l[v] : NEG_INF;
    mx = fmaxf(mx, x[j]);
  }
  mx = wave_max(mx);
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) s += (lane + 64 * j) < V ? expf(x[j] - mx) : 0.f;
  s = wave_sum(s);
  if (lane == 0) lse[f] = mx + logf(s);
}

// lane l takes v of lane l - 1 (DPP wave_shr:1), lane 0 -inf
__device__ __forceinline__ float aln_wave_shr1(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, NEG_INF), __builtin_bit_cast(int, v),
                                                               0x138, 0xf, 0xf, false));
}

// NS states per thread: 4 = one wave per utterance, 8 = one workgroup per utterance
template <int NS>
__global__ __launch_bounds__(NS == 4 ? 64 : 1024) void ctc_align_kernel(
    const float* __restrict__ logits, int64_t ldv, const int32_t* __restrict__ in_len,
    const int32_t* __restrict__ labels, const int32_t* __restrict__ lab_len, const float* __restrict__ lse,
    uint8_t* __restrict__ bp, int64_t rw, int32_t* start, int32_t* end, float* tok_score, float* __restrict__ score,
    int T, int V, int Lmax, int blank) {
  constexpr int NL = NS / 2;  // label states per thread
  constexpr int R = NS == 4 ? 12 : 4;  // staged logits per thread and chunk
  __shared__ float edge[2][NS == 4 ? 1 : 1024];
  __shared__ float tile[2][(NS == 4 ? 64 : 1024) * R];
  __shared__ float lset[2][64];
  __shared__ float fin[2];
  __shared__ uint4 win[64][ALN_WIN / 16];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const float* lg = logits + (int64_t)b * T * ldv;
  const float* lseb = lse + (int64_t)b * T;
  uint8_t* bpb = bp + (int64_t)b * T * rw;
  const int32_t* lab = labels + (int64_t)b * Lmax;
  int32_t* st_out = start + (int64_t)b * Lmax;
  int32_t* en_out = end + (int64_t)b * Lmax;
  float* ts_out = tok_score + (int64_t)b * Lmax;
  int Tin = in_len ? in_len[b] : T;
  Tin = Tin > T ? T : (Tin < 0 ? 0 : Tin);
  int L = lab_len[b];
  L = L > Lmax ? Lmax : (L < 0 ? 0 : L);
  const int S = 2 * L + 1;

  for (int i = L + tid; i < Lmax; i += blockDim.x) {
    st_out[i] = -1;
    en_out[i] = -1;
    ts_out[i] = 0.f;
  }

  const int s0 = NS * tid;
  int c[NL];
  bool skip[NL], valid[NS];
#pragma unroll
  for (int k = 0; k < NL; ++k) {
    const int i = (s0 >> 1) + k;  // token of state s0 + 2k + 1
    const int li = i < L ? lab[i] : blank;
    c[k] = li < 0 ? 0 : (li >= V ? V - 1 : li);  // the caller checks the labels; no gather leaves the row either way
    skip[k] = i < L && i >= 1 && lab[i - 1] != li;
  }
#pragma unroll
  for (int j = 0; j < NS; ++j) valid[j] = s0 + j < S;

  float a[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) a[j] = NEG_INF;
  if (Tin > 0 && tid == 0) {
    const float l0 = lseb[0];
    a[0] = lg[blank] - l0;
    if (valid[1]) a[1] = lg[c[0]] - l0;
  }
  if (NS == 8) edge[0][tid] = a[NS - 1];  // frame 0's row; read behind frame 1's barrier

  // one frame; row = the frame's logits in LDS, lse_t its logsumexp
  auto step = [&](int tt, const float* row, float lse_t) {
    float g[NL];
#pragma unroll
    for (int k = 0; k < NL; ++k) g[k] = row[c[k]] - lse_t;
    const float lpb = row[blank] - lse_t;
    float p1;  // v_{t-1}(s0 - 1), the last state of the thread before
    if (NS == 4) {
      p1 = aln_wave_shr1(a[NS - 1]);
    } else {
      p1 = tid > 0 ? edge[(tt - 1) & 1][tid - 1] : NEG_INF;
    }
    float na[NS];
    unsigned bits = 0;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      float best = a[j];
      unsigned mv = 0;
      const float m1 = j >= 1 ? a[j - 1] : p1;
      if (m1 > best) {
        best = m1;
        mv = 1;
      }
      if (j & 1) {
        const float m2 = j >= 2 ? a[j - 2] : p1;
        if (skip[j >> 1] && m2 > best) {
          best = m2;
          mv = 2;
        }
      }
      na[j] = valid[j] ? best + ((j & 1) ? g[j >> 1] : lpb) : NEG_INF;
      bits |= mv << (2 * j);
    }
#pragma unroll
    for (int j = 0; j < NS; ++j) a[j] = na[j];
    if (valid[0]) {
      if (NS == 4)
        bpb[(int64_t)tt * rw + tid] = (uint8_t)bits;
      else
        *(uint16_t*)(bpb + (int64_t)tt * rw + 2 * tid) = (uint16_t)bits;
    }
    if (NS == 8) edge[tt & 1][tid] = a[NS - 1];
  };

  if (Tin > 1) {
    // Frames 1 .. Tin-1 in chunks of F frames whose logits (F x V floats, at most R per thread) and logsumexps are
    // staged in LDS: the loads of chunk k+1 are issued before chunk k's frames and land in the other buffer behind
    // them, so inside the sequential chain a log-probability costs LDS reads only.  Element e = tid + r * nthr of a
    // chunk is column e % V of its frame e / V; the addresses are clamped to frame Tin-1, not predicated, so every
    // load is unconditional (the clamped ones fill tile slots no frame reads).
    const int nthr = blockDim.x;
    int F = nthr * R / V;
    F = F > 64 ? 64 : F;
    int fr[R], col[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int e = tid + r * nthr;
      fr[r] = e / V;
      col[r] = e - fr[r] * V;
    }
    float reg[R], lreg;
    auto load = [&](int t0) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int t = t0 + fr[r] < Tin ? t0 + fr[r] : Tin - 1;
        reg[r] = lg[(int64_t)t * ldv + col[r]];
      }
      const int t = t0 + (tid & 63) < Tin ? t0 + (tid & 63) : Tin - 1;
      lreg = lseb[t];
    };
    auto store = [&](int buf) {
#pragma unroll
      for (int r = 0; r < R; ++r) tile[buf][tid + r * nthr] = reg[r];
      if (tid < 64) lset[buf][tid] = lreg;
    };
    load(1);
    store(0);
    int buf = 0;
    for (int t0 = 1; t0 < Tin; t0 += F, buf ^= 1) {
      load(t0 + F < Tin ? t0 + F : Tin - 1);
      const int nf = Tin - t0 < F ? Tin - t0 : F;
      for (int f = 0; f < nf; ++f) {
        if (NS == 8) __syncthreads();  // the row of v before, and (first frame) the chunk's tile
        step(t0 + f, &tile[buf][f * V], lset[buf][f]);
      }
      asm volatile("" ::: "memory");
      store(buf ^ 1);
      asm volatile("" ::: "memory");
    }
  }

  // the two final states
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    if (s0 + j == S - 1) fin[0] = a[j];
    if (s0 + j == S - 2) fin[1] = a[j];
  }
  __syncthreads();

  bool feasible = false;
  if (tid < 64) {
    const float vA = Tin > 0 ? fin[0] : NEG_INF;
    const float vB = (Tin > 0 && S >= 2) ? fin[1] : NEG_INF;
    int s = vB > vA ? S - 2 : S - 1;  // a tie takes 2L
    const float best = vB > vA ? vB : vA;
    feasible = best > NEG_INF;
    if (tid == 0) score[b] = feasible ? best : NEG_INF;
    if (feasible) {
      int above = -1;  // the state at frame t + 1
      for (int top = Tin - 1; top >= 0; top -= 64) {
        // window of the next 64 frames: they visit states s - 126 .. s
        int lo = ((s - 126 > 0 ? s - 126 : 0) >> 2) & ~15;
        if (lo > (int)rw - ALN_WIN) lo = (int)rw - ALN_WIN;
        const int tl = top - tid;
        if (tl >= 1) {  // frame 0 has no move
          const uint4* src = (const uint4*)(bpb + (int64_t)tl * rw + lo);
#pragma unroll
          for (int q = 0; q < ALN_WIN / 16; ++q) win[tid][q] = src[q];
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        const int n = top + 1 < 64 ? top + 1 : 64;
        for (int i = 0; i < n; ++i) {
          const int t = top - i;
          const int tok = s >> 1;
          if ((s & 1) && s != above && tid == 0) en_out[tok] = t + 1;
          int mv = 0;
          if (t > 0) {
            int idx = (s >> 2) - lo;
            idx = idx < 0 ? 0 : (idx > ALN_WIN - 1 ? ALN_WIN - 1 : idx);
            const unsigned byte = ((const uint8_t*)win[i])[idx];
            mv = (byte >> (2 * (s & 3))) & 3;
            if (mv > s) mv = s;
          }
          if ((s & 1) && (t == 0 || mv != 0) && tid == 0) st_out[tok] = t;
          above = s;
          s -= mv;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
    }
  }
  __syncthreads();  // start / end of this row are read back below
  feasible = fin[0] > NEG_INF || (S >= 2 && fin[1] > NEG_INF);
  if (Tin <= 0) feasible = false;
  for (int i = tid; i < L; i += blockDim.x) {
    if (!feasible) {
      st_out[i] = -1;
      en_out[i] = -1;
      ts_out[i] = NEG_INF;
      continue;
    }
    const int st = st_out[i], en = en_out[i];
    const int ci = lab[i] < 0 ? 0 : (lab[i] >= V ? V - 1 : lab[i]);
    float sum = 0.f;
    for (int t = st; t < en; ++t) sum += lg[(int64_t)t * ldv + ci] - lseb[t];
    ts_out[i] = sum / (float)(en - st);
  }
}

extern "C" int ca_ctc_align(const float* logits, int64_t ldv, const int32_t* in_len, const int32_t* labels,
                            const int32_t* lab_len, int32_t* start, int32_t* end, float* tok_score, float* score,
                            void* ws, int64_t ws_bytes, int32_t B, int32_t T, int32_t V, int32_t Lmax, int32_t blank,
                            void* stream) {
  CA_CHECK_ARG(logits && lab_len && score && ws, "ca_ctc_align: null pointer");
  CA_CHECK_ARG(B > 0 && T > 0 && V >= 2 && V <= 256 && ldv >= V, "ca_ctc_align: bad shape (2 <= V <= 256)");
  CA_CHECK_ARG(Lmax >= 0 && Lmax <= CA_CTC_ALIGN_MAX_LABELS, "ca_ctc_align: Lmax %d outside [0, %d]", Lmax,
               CA_CTC_ALIGN_MAX_LABELS);
  CA_CHECK_ARG(Lmax == 0 || (labels && start && end && tok_score), "ca_ctc_align: null pointer");
  CA_CHECK_ARG(blank >= 0 && blank < V, "ca_ctc_align: bad blank");
  CA_CHECK_ARG(ws_bytes >= ca_ctc_align_workspace_bytes(B, T, Lmax), "ca_ctc_align: workspace too small (%lld < %lld)",
               (long long)ws_bytes, (long long)ca_ctc_align_workspace_bytes(B, T, Lmax));
  float* lse = (float*)ws;
  uint8_t* bp = (uint8_t*)ws + aln_align256((int64_t)B * T * 4);
  const int64_t rw = aln_row_bytes(Lmax);
  hipStream_t s = (hipStream_t)stream;
  const int64_t frames = (int64_t)B * T;
  hipLaunchKernelGGL(ctc_align_lse_kernel, dim3((unsigned)((frames + 3) / 4)), dim3(256), 0, s, logits, lse, frames, V,
                     ldv);
  if (Lmax <= 127) {
    hipLaunchKernelGGL(ctc_align_kernel<4>, dim3(B), dim3(64), 0, s, logits, ldv, in_len, labels, lab_len, lse, bp, rw,
                       start, end, tok_score, score, T, V, Lmax, blank);
  } else {
    const int threads = (((2 * Lmax + 1 + 7) / 8) + 63) & ~63;
    hipLaunchKernelGGL(ctc_align_kernel<8>, dim3(B), dim3(threads), 0, s, logits, ldv, in_len, labels, lab_len, lse, bp,
                       rw, start, end, tok_score, score, T, V, Lmax, blank);
  }
  CA_CHECK_LAUNCH("ca_ctc_align");
  return CA_OK;
}
