// CTC prefix beam search with n-gram language-model fusion (wav2vec2 evaluation with `no_lm: false`).
//
// This is the project's own decoder with a stated objective, not a restatement of pyctcdecode (parity with it is
// unpinned: neither pyctcdecode nor KenLM can be run beside it).  Objective, for a label string y without blanks, split on
// the word delimiter into words w_1..w_n (empty pieces dropped):
//
//   S(y) = ln P_ctc(y | lp)                                    sum over all alignments, lp = fp32 log_softmax(logits)
//        + alpha ln(10) ( sum_i log10 P_lm(w_i | w_{i-k+1..i-1})  [+ log10 P_lm(</s> | ...) if score_boundary] )
//        + beta n
//        + unk_score_offset #{ w_i that are no LM unigram }
//
// P_lm is the ARPA back-off rule (longest stored n-gram wins, else backoff(context) + P(w | shorter context)); the
// sentence starts in the context <s>.  A word that is no unigram scores as <unk> when the LM has one (and stays <unk> in
// later contexts, as KenLM does), else as log10 P = 0 followed by an empty context.  Without LM tables only beta n is
// added (alpha = beta = 0: plain CTC prefix beam search).  Ids flagged in `forbidden` are never emitted.
//
// Search (per frame t < in_len): a beam is a distinct prefix with (p_blank, p_nonblank) in log space.  Candidates are
// "stay" (blank, or a repeat of the last symbol) and "extend by c" for every c != blank, not forbidden, with
// lp[t, c] >= token_min_logp.  An extension that equals another live beam's prefix is merged into that beam's stay
// (a prefix has one parent, so a probability has at most two contributors and log_add2 is symmetric: no order
// dependence).  Only closed words are LM-scored; the open last word adds a provisional unk_score_offset to the RANKING
// score once it is no prefix of any unigram.  Ranking = ln(p_b + p_nb) + LM/bonus score + provisional offset.
// Candidates below best + beam_prune_logp (or at -inf) are dropped, the best beam_width survive; ties in the ranking
// score break on the lower 64-bit prefix hash.  After the last frame the open word is scored as closed, the boundary
// term is added, and the best S(y) (ties: lower prefix hash) is traced back through (parent, symbol) nodes kept in the
// workspace.
//
// Mapping: one launch per batch, one 256-thread workgroup per utterance, the frame loop inside the kernel; no
// communication between workgroups and no waiting loops - every loop is bounded by T, beam_width * V, the LDS table
// size or log2 of an LM table.  Beams, the frame's candidates, their ranking keys and a 512-slot open-addressing table
// (prefix hash -> live beam) live in LDS; the top beam_width are picked by an 8-bit radix select on the order-preserving
// integer image of the fp32 ranking score (integer LDS atomics only: the counts do not depend on arrival order), so the
// set of survivors, every probability and the returned ids / score are bit-identical from run to run.  The slot a
// survivor lands in may differ between runs; nothing observable depends on it.  LM look-ups are binary searches over
// sorted 64-bit hashes in global memory.
//
// Extended entry (ca_ctc_beam_decode_ex, the EX = true instance of the same kernel; the plain entry is the EX = false
// instance and compiles to what it was): n-best output and hotword boosting.
//
//   S_h(y) = S(y) + hotword_weight #{ w_i that are hotwords }
//
// The hotword table holds the open-word hash (WORD_SEED) of every prefix of every hotword, ascending, with the fraction
// len / len_min (len_min: the shortest hotword with that prefix) and a flag "this prefix is itself a hotword".  A word
// that closes (at a delimiter or after the last frame) adds hotword_weight when it is a hotword - beside, not instead
// of, unk_score_offset when it is no LM unigram.  Ranking only: while the open word is a prefix of a hotword it adds
// hotword_weight * fraction to the ranking score (a complete hotword that is still open: the full weight); the bonus is
// gone once the open word is no hotword prefix, and is replaced by the exact term when the word closes.  A beam carries
// its bonus (b_hot) and a flag bit; a candidate carries the table index in c_wid, which only delimiter candidates use
// otherwise.  After the last frame every live prefix gets its S; a final's rank is the number of finals that beat it
// under (S descending, prefix hash ascending) - counted, not sorted, so nothing depends on arrival order - and thread r
// walks the (parent, symbol) nodes of the rank-r final.  score = logit_score + lm_score exactly: logit_score is
// ln(p_b + p_nb), lm_score everything else, and S is formed as that fp32 sum.  Rank 0 is the plain entry's answer.
//
// Static LDS: 118 816 B for EX = false (as before), 119 840 B (117.0 KiB of the CU's 160 KiB) for EX = true: b_hot adds
// 1 KiB; the final ranking reuses s_pb / s_pnb / merge_s / slot_s.
#include "common.h"

#define NEG_INF (-__builtin_inff())
#define BEAM_MAX 128          // beams per utterance
#define BEAM_CAND_MAX 6144    // new-prefix candidates per frame: beam_width * (V - 1) must fit
#define BEAM_SLOTS 512        // open-addressing table over the live beams
#define BEAM_CTX 4            // LM context words kept (order - 1 <= 4)
#define BEAM_THREADS 256

#define PREFIX_SEED 0x243F6A8885A308D3ull
#define WORD_SEED 0x13198A2E03707344ull
#define NGRAM_SEED 0xA4093822299F31D0ull

// the rolling hash of coral_amd/ngram.py (`mix64`): symbol ids for prefixes and open words, word ids for n-grams
__host__ __device__ __forceinline__ uint64_t beam_mix(uint64_t h, int x) {
  uint64_t z = (h ^ (uint64_t)(int64_t)(x + 1)) * 0x9E3779B97F4A7C15ull;
  z ^= z >> 32;
  z *= 0xD6E8FEB86659FD93ull;
  z ^= z >> 32;
  return z;
}

__device__ __forceinline__ float beam_log_add2(float a, float b) {
  const float m = fmaxf(a, b);
  if (!(m > NEG_INF)) return NEG_INF;
  return m + log1pf(expf(fminf(a, b) - m));
}

// order-preserving integer image of a ranking score; -inf and NaN map to 0 = "dropped"
__device__ __forceinline__ unsigned beam_key(float x) {
  if (!(x > NEG_INF)) return 0u;
  const unsigned u = __builtin_bit_cast(unsigned, x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float beam_unkey(unsigned k) {
  if (k == 0u) return NEG_INF;
  const unsigned u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
  return __builtin_bit_cast(float, u);
}

// index of `key` in the sorted keys[lo, hi), or -1
__device__ __forceinline__ int64_t beam_bsearch(const uint64_t* __restrict__ keys, int64_t lo, int64_t hi, uint64_t key) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    const uint64_t k = keys[mid];
    if (k == key) return mid;
    if (k < key) lo = mid + 1;
    else hi = mid;
  }
  return -1;
}

// open-word hash -> index in the hotword table, or -1 (no prefix of any hotword)
__device__ __forceinline__ int beam_hot_lookup(const CaCtcBeamExt& x, uint64_t h) {
  return (int)beam_bsearch(x.hot_keys, 0, x.n_hot, h);
}

// open-word hash -> word id (>= 0), -1 (proper prefix of a unigram only), -2 (no prefix of any unigram)
__device__ __forceinline__ int beam_word_lookup(const CaCtcBeamDesc& d, uint64_t h) {
  const int64_t i = beam_bsearch(d.pfx_keys, 0, d.n_pfx, h);
  return i < 0 ? -2 : d.pfx_wid[i];
}

// log10 P(w | ctx[0..n)) by the ARPA back-off rule; ctx holds the most recent word last
__device__ float beam_lm_logp(const CaCtcBeamDesc& d, const int* ctx, int n, int w) {
  float bo = 0.f;
  int64_t off[BEAM_CTX + 2];
  off[0] = 0;
#pragma unroll
  for (int k = 0; k <= BEAM_CTX; ++k) off[k + 1] = off[k] + d.ng_count[k];
  for (int k = n; k >= 0; --k) {
    uint64_t h = NGRAM_SEED;
    for (int i = n - k; i < n; ++i) h = beam_mix(h, ctx[i]);
    const uint64_t hc = h;
    h = beam_mix(h, w);
    int64_t idx = beam_bsearch(d.ng_keys, off[k], off[k + 1], h);
    if (idx >= 0) return bo + d.ng_logp[idx];
    if (k > 0) {
      idx = beam_bsearch(d.ng_keys, off[k - 1], off[k], hc);
      if (idx >= 0) bo += d.ng_backoff[idx];
    }
  }
  return bo - 99.f;  // w is always a stored unigram; an inconsistent table scores as impossible
}

// flags word of a beam: bits 0-8 last symbol + 1 (0 = empty prefix), 9 provisional-unk, 10 open word not empty,
// 11-13 LM context length, 14 open word is a prefix of a hotword (EX only)
#define FL_LAST(f) (((f) & 511) - 1)
#define FL_PEN(f) (((f) >> 9) & 1)
#define FL_OPEN(f) (((f) >> 10) & 1)
#define FL_NCTX(f) (((f) >> 11) & 7)
#define FL_HOT(f) (((f) >> 14) & 1)
#define FL_MAKE(last, pen, open, nctx) (((last) + 1) | ((pen) << 9) | ((open) << 10) | ((nctx) << 11))

// score of closing the open word of a beam with context ctx[0..n): returns the addend, the word id that enters the
// context (-1: none, context cleared) in `w`.  EX: `hot` says that the open word is a prefix of a hotword; when it is
// one itself, hotword_weight is added last.
template <bool EX>
__device__ __forceinline__ float beam_close_word(const CaCtcBeamDesc& d, const CaCtcBeamExt& x, bool have_lm, uint64_t ow,
                                                 const int* ctx, int n, float alpha_ln10, bool hot, int& w) {
  float s = d.beta;
  w = -1;
  if (have_lm) {
    const int wid = beam_word_lookup(d, ow);
    if (wid < 0) {
      s += d.unk_score_offset;
      w = d.unk_wid;
    } else {
      w = wid;
    }
    if (w >= 0) s += alpha_ln10 * beam_lm_logp(d, ctx, n, w);
  }
  if constexpr (EX) {
    if (hot) {
      const int hi = beam_hot_lookup(x, ow);
      if (hi >= 0 && x.hot_word[hi]) s += x.hotword_weight;
    }
  }
  return s;
}

__device__ __forceinline__ int beam_push_ctx(int* ctx, int n, int w, int order) {
  if (w < 0) return 0;
  const int cap = order - 1;
  if (cap <= 0) return 0;
  if (n < cap) {
    ctx[n] = w;
    return n + 1;
  }
  for (int i = 0; i + 1 < cap; ++i) ctx[i] = ctx[i + 1];
  ctx[cap - 1] = w;
  return cap;
}

template <bool EX>
__global__ __launch_bounds__(BEAM_THREADS) void ctc_beam_kernel(const CaCtcBeamDesc d, const CaCtcBeamExt x) {
  __shared__ uint64_t b_hash[2][BEAM_MAX], b_ow[2][BEAM_MAX];
  __shared__ float b_pb[2][BEAM_MAX], b_pnb[2][BEAM_MAX], b_lm[2][BEAM_MAX];
  __shared__ int b_flags[2][BEAM_MAX], b_node[2][BEAM_MAX];
  __shared__ int b_ctx[2][BEAM_MAX][BEAM_CTX];
  __shared__ float b_hot[EX ? 2 : 1][EX ? BEAM_MAX : 1];  // provisional hotword bonus of the open word (ranking only)
  __shared__ float s_pb[BEAM_MAX], s_pnb[BEAM_MAX], merge_s[BEAM_MAX];
  __shared__ int c_meta[BEAM_CAND_MAX];   // parent | symbol << 8 | provisional-unk << 16
  __shared__ float c_lm[BEAM_CAND_MAX];   // LM + bonus score of the extended prefix
  __shared__ int c_wid[BEAM_CAND_MAX];    // word id entering the context at a delimiter (-1: none); EX, other symbols:
                                          // index of the open word in the hotword table (-1: no hotword prefix)
  __shared__ unsigned keys[BEAM_MAX + BEAM_CAND_MAX];  // [0, N) stays, [BEAM_MAX, BEAM_MAX + M) new prefixes
  __shared__ float lp_s[256];
  __shared__ int sym_s[256];
  __shared__ int slot_s[BEAM_SLOTS];
  __shared__ int hist_s[256];
  __shared__ int nsym_s, ncand_s, nnew_s, cnt_s, sel_need_s, sel_eq_s;
  __shared__ unsigned best_s, sel_prefix_s;

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = d.T, V = d.V, bw = d.beam_width, order = d.order;
  const bool have_lm = order > 0 && d.n_pfx > 0;
  const float alpha_ln10 = d.alpha * 2.302585092994046f;
  int Tin = d.in_len ? d.in_len[b] : T;
  Tin = Tin > T ? T : (Tin < 0 ? 0 : Tin);
  const float* lg = d.logits + (int64_t)b * T * d.ldv;
  int2* trace = (int2*)d.ws + (int64_t)b * T * bw;  // node t * bw + slot -> (parent node, symbol)
  const bool have_hot = EX && x.n_hot > 0;
  int32_t* ids = EX ? x.ids_n + (int64_t)b * x.n_best * T : d.ids_out + (int64_t)b * T;
  for (int64_t t = tid; t < (int64_t)(EX ? x.n_best : 1) * T; t += BEAM_THREADS) ids[t] = -1;

  int cur = 0, N = 1;
  if (tid == 0) {
    b_hash[0][0] = PREFIX_SEED;
    b_ow[0][0] = WORD_SEED;
    b_pb[0][0] = 0.f;
    b_pnb[0][0] = NEG_INF;
    b_lm[0][0] = 0.f;
    int nctx = 0;
    if (have_lm && d.bos_wid >= 0 && order > 1) {
      b_ctx[0][0][0] = d.bos_wid;
      nctx = 1;
    }
    b_flags[0][0] = FL_MAKE(-1, 0, 0, nctx);
    b_node[0][0] = -1;
    if constexpr (EX) b_hot[0][0] = 0.f;
  }
  __syncthreads();

  for (int t = 0; t < Tin; ++t) {
    // ---- a. log_softmax of the frame and the list of symbols that may extend a prefix (wave 0) ----
    if (wave == 0) {
      const float* l = lg + (int64_t)t * d.ldv;
      float x[4];
      float mx = NEG_INF;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int v = lane + 64 * j;
        x[j] = v < V ? l[v] : NEG_INF;
        mx = fmaxf(mx, x[j]);
      }
      mx = wave_max(mx);
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) sum += (lane + 64 * j) < V ? expf(x[j] - mx) : 0.f;
      sum = wave_sum(sum);
      const float lse = mx + logf(sum);
      int base = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int v = lane + 64 * j;
        const float lpv = x[j] - lse;
        bool pass = false;
        if (v < V) {
          lp_s[v] = lpv;
          pass = v != d.blank && !(d.forbidden && d.forbidden[v]) && lpv >= d.token_min_logp;
        }
        const uint64_t m = __ballot(pass);
        if (pass) sym_s[base + __popcll(m & ((1ull << lane) - 1ull))] = v;
        base += __popcll(m);
      }
      if (lane == 0) {
        nsym_s = base;
        ncand_s = 0;
        nnew_s = 0;
        cnt_s = 0;
        best_s = 0u;
      }
    }
    for (int s = tid; s < BEAM_SLOTS; s += BEAM_THREADS) slot_s[s] = -1;
    if (tid < BEAM_MAX) {
      merge_s[tid] = NEG_INF;
      if (tid >= N) keys[tid] = 0u;
    }
    __syncthreads();
    // ---- b. prefix hash -> live beam ----
    if (tid < N) {
      int s = (int)(b_hash[cur][tid] & (BEAM_SLOTS - 1));
      for (int n = 0; n < BEAM_SLOTS; ++n) {
        if (atomicCAS(&slot_s[s], -1, tid) == -1) break;
        s = (s + 1) & (BEAM_SLOTS - 1);
      }
    }
    __syncthreads();
    // ---- c. extensions: merged into a live beam's stay, or a new prefix ----
    const int nsym = nsym_s;
    for (int e = tid; e < N * nsym; e += BEAM_THREADS) {
      const int i = e / nsym;
      const int c = sym_s[e - i * nsym];
      const int fl = b_flags[cur][i];
      const float pb = b_pb[cur][i], pnb = b_pnb[cur][i];
      const float v = lp_s[c] + (c == FL_LAST(fl) ? pb : beam_log_add2(pb, pnb));
      if (!(v > NEG_INF)) continue;
      const uint64_t h2 = beam_mix(b_hash[cur][i], c);
      int found = -1;
      int s = (int)(h2 & (BEAM_SLOTS - 1));
      for (int n = 0; n < BEAM_SLOTS; ++n) {
        const int j = slot_s[s];
        if (j < 0) break;
        if (b_hash[cur][j] == h2) {
          found = j;
          break;
        }
        s = (s + 1) & (BEAM_SLOTS - 1);
      }
      if (found >= 0) {
        merge_s[found] = v;  // the one extension that can produce this prefix
        continue;
      }
      float lm2 = b_lm[cur][i];
      int pen2 = 0, w = -1;
      if (c == d.delimiter) {
        if (FL_OPEN(fl)) {
          int ctx[BEAM_CTX];
#pragma unroll
          for (int q = 0; q < BEAM_CTX; ++q) ctx[q] = b_ctx[cur][i][q];
          lm2 += beam_close_word<EX>(d, x, have_lm, b_ow[cur][i], ctx, FL_NCTX(fl), alpha_ln10, FL_HOT(fl), w);
        }
      } else {
        pen2 = FL_PEN(fl);
        if (!pen2 && have_lm) pen2 = beam_word_lookup(d, beam_mix(b_ow[cur][i], c)) == -2;
        // a longer word is a hotword prefix only if the word so far is one (or is empty)
        if (have_hot && (!FL_OPEN(fl) || FL_HOT(fl))) w = beam_hot_lookup(x, beam_mix(b_ow[cur][i], c));
      }
      const int idx = atomicAdd(&ncand_s, 1);  // < N * nsym <= beam_width * (V - 1) <= BEAM_CAND_MAX
      c_meta[idx] = i | (c << 8) | (pen2 << 16);
      c_lm[idx] = lm2;
      c_wid[idx] = w;
      float rank = v + lm2 + (pen2 ? d.unk_score_offset : 0.f);
      if constexpr (EX) rank += (c != d.delimiter && w >= 0) ? x.hotword_weight * x.hot_frac[w] : 0.f;
      keys[BEAM_MAX + idx] = beam_key(rank);
    }
    __syncthreads();
    // ---- d. stays ----
    if (tid < N) {
      const int fl = b_flags[cur][tid];
      const float pb = b_pb[cur][tid], pnb = b_pnb[cur][tid];
      const int last = FL_LAST(fl);
      const float npb = beam_log_add2(pb, pnb) + lp_s[d.blank];
      const float npnb = beam_log_add2(last >= 0 ? pnb + lp_s[last] : NEG_INF, merge_s[tid]);
      s_pb[tid] = npb;
      s_pnb[tid] = npnb;
      float rank = beam_log_add2(npb, npnb) + b_lm[cur][tid] + (FL_PEN(fl) ? d.unk_score_offset : 0.f);
      if constexpr (EX) rank += b_hot[cur][tid];
      keys[tid] = beam_key(rank);
    }
    __syncthreads();
    const int K = BEAM_MAX + ncand_s;
    // ---- e. best ranking score, pruning threshold, number of survivors ----
    {
      unsigned m = 0u;
      for (int k = tid; k < K; k += BEAM_THREADS) m = max(m, keys[k]);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
      if (lane == 0) atomicMax(&best_s, m);
    }
    __syncthreads();
    unsigned thr_key = max(beam_key(beam_unkey(best_s) + d.beam_prune_logp), 1u);
    {
      int n = 0;
      for (int k = tid; k < K; k += BEAM_THREADS) n += keys[k] >= thr_key;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
      if (lane == 0) atomicAdd(&cnt_s, n);
    }
    __syncthreads();
    // ---- f. more than beam_width survivors: radix select of the beam_width-th largest key ----
    int tie_need = -1;  // -1: take every key >= thr_key; else: every key > thr_key and `tie_need` of the equal ones
    if (cnt_s > bw) {
      unsigned prefix = 0u, mask = 0u;
      int need = bw, eq = 0;
      for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        hist_s[tid] = 0;
        __syncthreads();
        for (int k = tid; k < K; k += BEAM_THREADS) {
          const unsigned key = keys[k];
          if (key >= thr_key && (key & mask) == prefix) atomicAdd(&hist_s[(key >> shift) & 255u], 1);
        }
        __syncthreads();
        if (wave == 0) {
          // lane l owns the bins 255 - 4 l ... 252 - 4 l (descending); find the bin where the running count reaches need
          int h[4], tot = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            h[j] = hist_s[255 - (4 * lane + j)];
            tot += h[j];
          }
          int incl = tot;
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
          }
          int before = incl - tot;
          if (before < need && need <= incl) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              if (before < need && need <= before + h[j]) {
                sel_prefix_s = prefix | ((unsigned)(255 - (4 * lane + j)) << shift);
                sel_need_s = need - before;
                sel_eq_s = h[j];
              }
              before += h[j];
            }
          }
        }
        __syncthreads();
        prefix = sel_prefix_s;
        need = sel_need_s;
        eq = sel_eq_s;
        mask |= 255u << shift;
      }
      thr_key = prefix;
      if (need < eq) tie_need = need;
    }
    // ---- g. survivors become the next frame's beams ----
    const int nxt = cur ^ 1;
    for (int k = tid; k < K; k += BEAM_THREADS) {
      const unsigned key = keys[k];
      if (key < thr_key || key == 0u) continue;
      const bool is_stay = k < BEAM_MAX;
      if (tie_need >= 0 && key == thr_key) {
        // equal ranking scores at the cut: the lower prefix hashes win
        const int ck = is_stay ? 0 : c_meta[k - BEAM_MAX];
        const uint64_t hk = is_stay ? b_hash[cur][k] : beam_mix(b_hash[cur][ck & 255], (ck >> 8) & 255);
        int lower = 0;
        for (int q = 0; q < K; ++q) {
          if (keys[q] != thr_key || q == k) continue;
          const int cq = q < BEAM_MAX ? 0 : c_meta[q - BEAM_MAX];
          const uint64_t hq = q < BEAM_MAX ? b_hash[cur][q] : beam_mix(b_hash[cur][cq & 255], (cq >> 8) & 255);
          lower += hq < hk;
        }
        if (lower >= tie_need) continue;
      }
      const int slot = atomicAdd(&nnew_s, 1);
      if (is_stay) {
        b_hash[nxt][slot] = b_hash[cur][k];
        b_ow[nxt][slot] = b_ow[cur][k];
        b_pb[nxt][slot] = s_pb[k];
        b_pnb[nxt][slot] = s_pnb[k];
        b_lm[nxt][slot] = b_lm[cur][k];
        b_flags[nxt][slot] = b_flags[cur][k];
        b_node[nxt][slot] = b_node[cur][k];
#pragma unroll
        for (int q = 0; q < BEAM_CTX; ++q) b_ctx[nxt][slot][q] = b_ctx[cur][k][q];
        if constexpr (EX) b_hot[nxt][slot] = b_hot[cur][k];
      } else {
        const int idx = k - BEAM_MAX;
        const int meta = c_meta[idx];
        const int i = meta & 255, c = (meta >> 8) & 255, pen2 = (meta >> 16) & 1;
        const int fl = b_flags[cur][i];
        const float pb = b_pb[cur][i], pnb = b_pnb[cur][i];
        int ctx[BEAM_CTX];
#pragma unroll
        for (int q = 0; q < BEAM_CTX; ++q) ctx[q] = b_ctx[cur][i][q];
        int nctx = FL_NCTX(fl), open = 1;
        uint64_t ow = WORD_SEED;
        if (c == d.delimiter) {
          open = 0;
          if (FL_OPEN(fl) && have_lm) nctx = beam_push_ctx(ctx, nctx, c_wid[idx], order);
        } else {
          ow = beam_mix(b_ow[cur][i], c);
        }
        b_hash[nxt][slot] = beam_mix(b_hash[cur][i], c);
        b_ow[nxt][slot] = ow;
        b_pb[nxt][slot] = NEG_INF;
        b_pnb[nxt][slot] = lp_s[c] + (c == FL_LAST(fl) ? pb : beam_log_add2(pb, pnb));
        b_lm[nxt][slot] = c_lm[idx];
        int flags = FL_MAKE(c, pen2, open, nctx);
        if constexpr (EX) {
          const int hi = open ? c_wid[idx] : -1;
          b_hot[nxt][slot] = hi >= 0 ? x.hotword_weight * x.hot_frac[hi] : 0.f;
          flags |= (hi >= 0) << 14;
        }
        b_flags[nxt][slot] = flags;
#pragma unroll
        for (int q = 0; q < BEAM_CTX; ++q) b_ctx[nxt][slot][q] = ctx[q];
        const int node = t * bw + slot;
        b_node[nxt][slot] = node;
        trace[node] = make_int2(b_node[cur][i], c);
      }
    }
    __syncthreads();
    N = nnew_s;
    cur = nxt;
    __syncthreads();  // wave 0 resets the counters at the top of the next frame
  }

  // ---- the open word closes, the boundary term, the best S(y) ----
  if (tid < N) {
    const int fl = b_flags[cur][tid];
    int ctx[BEAM_CTX];
#pragma unroll
    for (int q = 0; q < BEAM_CTX; ++q) ctx[q] = b_ctx[cur][tid][q];
    int nctx = FL_NCTX(fl);
    float lm = b_lm[cur][tid];
    if (FL_OPEN(fl)) {
      int w;
      lm += beam_close_word<EX>(d, x, have_lm, b_ow[cur][tid], ctx, nctx, alpha_ln10, FL_HOT(fl), w);
      if (have_lm) nctx = beam_push_ctx(ctx, nctx, w, order);
    }
    if (have_lm && d.score_boundary && d.eos_wid >= 0) lm += alpha_ln10 * beam_lm_logp(d, ctx, nctx, d.eos_wid);
    const float logit = beam_log_add2(b_pb[cur][tid], b_pnb[cur][tid]);
    s_pb[tid] = logit + lm;
    if constexpr (EX) {
      s_pnb[tid] = logit;
      merge_s[tid] = lm;
    }
  }
  __syncthreads();  // also orders this workgroup's trace stores before the walk below
  if constexpr (EX) {
    // ---- n-best: rank by counting, one thread per returned hypothesis walks its nodes ----
    const int nb = x.n_best;
    int nfin = 0;
    if (tid < BEAM_MAX) {
      const unsigned mk = tid < N ? beam_key(s_pb[tid]) : 0u;
      const uint64_t mh = tid < N ? b_hash[cur][tid] : 0ull;
      int rank = 0;
      for (int j = 0; j < N; ++j) {
        const unsigned k = beam_key(s_pb[j]);
        nfin += k != 0u;
        rank += k != 0u && (k > mk || (k == mk && b_hash[cur][j] < mh));
      }
      if (mk != 0u && rank < nb) slot_s[rank] = tid;  // live beams have distinct prefix hashes, so ranks are distinct
    }
    __syncthreads();
    if (tid < nb) {
      const int64_t o = (int64_t)b * nb + tid;
      if (tid < nfin) {
        const int i = slot_s[tid];
        int32_t* row = ids + (int64_t)tid * T;
        int len = 0;
        for (int node = b_node[cur][i]; node >= 0 && len < T; node = trace[node].x) ++len;
        int pos = len;
        for (int node = b_node[cur][i]; node >= 0 && pos > 0; node = trace[node].x) row[--pos] = trace[node].y;
        x.len_n[o] = len;
        x.score_n[o] = s_pb[i];
        x.logit_n[o] = s_pnb[i];
        x.lm_n[o] = merge_s[i];
      } else {
        x.len_n[o] = -1;
        x.score_n[o] = NEG_INF;
        x.logit_n[o] = NEG_INF;
        x.lm_n[o] = NEG_INF;
      }
    }
    if (tid == 0) x.n_out[b] = nfin < nb ? nfin : nb;
    return;
  }
  if (tid == 0) {
    int best = -1;
    unsigned bk = 0u;
    for (int i = 0; i < N; ++i) {
      const unsigned k = beam_key(s_pb[i]);
      if (k == 0u) continue;
      if (best < 0 || k > bk || (k == bk && b_hash[cur][i] < b_hash[cur][best])) {
        best = i;
        bk = k;
      }
    }
    int len = 0;
    if (best >= 0) {
      for (int node = b_node[cur][best]; node >= 0 && len < T; node = trace[node].x) ++len;
      int pos = len;
      for (int node = b_node[cur][best]; node >= 0 && pos > 0; node = trace[node].x) ids[--pos] = trace[node].y;
    }
    d.out_len[b] = len;
    d.score_out[b] = best >= 0 ? s_pb[best] : NEG_INF;
  }
}

extern "C" int64_t ca_ctc_beam_workspace_bytes(int32_t B, int32_t T, int32_t V, int32_t beam_width) {
  (void)V;
  if (B <= 0 || T <= 0 || beam_width <= 0) return 0;
  return (((int64_t)B * T * beam_width * (int64_t)sizeof(int2)) + 255) & ~(int64_t)255;
}

// the checks both entries share; `ext` decides which outputs must be there
static int beam_check(const CaCtcBeamDesc* desc, const CaCtcBeamExt* ext) {
  CA_CHECK_ARG(desc, "ca_ctc_beam_decode: null descriptor");
  const CaCtcBeamDesc& d = *desc;
  CA_CHECK_ARG(d.logits && (ext || (d.ids_out && d.out_len && d.score_out)) && d.ws, "ca_ctc_beam_decode: null pointer");
  CA_CHECK_ARG(d.B > 0 && d.T > 0 && d.V >= 2 && d.V <= 256 && d.ldv >= d.V,
               "ca_ctc_beam_decode: bad shape (2 <= V <= 256)");
  CA_CHECK_ARG(d.blank >= 0 && d.blank < d.V && d.delimiter >= -1 && d.delimiter < d.V && d.delimiter != d.blank,
               "ca_ctc_beam_decode: bad blank / delimiter id");
  CA_CHECK_ARG(d.beam_width >= 1 && d.beam_width <= BEAM_MAX, "ca_ctc_beam_decode: beam_width %d outside 1..%d",
               d.beam_width, BEAM_MAX);
  CA_CHECK_ARG((int64_t)d.beam_width * (d.V - 1) <= BEAM_CAND_MAX,
               "ca_ctc_beam_decode: beam_width %d x (V - 1 = %d) candidates per frame exceed the %d the LDS layout holds",
               d.beam_width, d.V - 1, BEAM_CAND_MAX);
  CA_CHECK_ARG((int64_t)d.T * d.beam_width < ((int64_t)1 << 31), "ca_ctc_beam_decode: T x beam_width too large");
  CA_CHECK_ARG(d.order >= 0 && d.order <= BEAM_CTX + 1, "ca_ctc_beam_decode: LM order %d outside 0..%d", d.order,
               BEAM_CTX + 1);
  if (d.order > 0) {
    CA_CHECK_ARG(d.pfx_keys && d.pfx_wid && d.n_pfx > 0 && d.ng_keys && d.ng_logp && d.ng_backoff,
                 "ca_ctc_beam_decode: LM order %d without its tables", d.order);
    for (int k = 0; k <= BEAM_CTX; ++k)
      CA_CHECK_ARG(d.ng_count[k] >= 0 && (k < d.order || d.ng_count[k] == 0),
                   "ca_ctc_beam_decode: bad n-gram count for order %d", k + 1);
    CA_CHECK_ARG(d.ng_count[0] > 0 && d.bos_wid < d.ng_count[0] && d.eos_wid < d.ng_count[0] && d.unk_wid < d.ng_count[0],
                 "ca_ctc_beam_decode: special word id outside the unigram table");
  }
  CA_CHECK_ARG(!(d.token_min_logp != d.token_min_logp) && !(d.beam_prune_logp != d.beam_prune_logp) &&
                   d.beam_prune_logp <= 0.f,
               "ca_ctc_beam_decode: pruning thresholds must be numbers (beam_prune_logp <= 0, -inf = off)");
  CA_CHECK_ARG(d.ws_bytes >= ca_ctc_beam_workspace_bytes(d.B, d.T, d.V, d.beam_width),
               "ca_ctc_beam_decode: workspace too small");
  return CA_OK;
}

extern "C" int ca_ctc_beam_decode(const CaCtcBeamDesc* desc, void* stream) {
  if (const int rc = beam_check(desc, nullptr)) return rc;
  CaCtcBeamExt none = {};
  hipLaunchKernelGGL(ctc_beam_kernel<false>, dim3(desc->B), dim3(BEAM_THREADS), 0, (hipStream_t)stream, *desc, none);
  CA_CHECK_LAUNCH("ca_ctc_beam_decode");
  return CA_OK;
}

extern "C" int ca_ctc_beam_decode_ex(const CaCtcBeamDesc* desc, const CaCtcBeamExt* ext, void* stream) {
  CA_CHECK_ARG(ext, "ca_ctc_beam_decode_ex: null extension");
  if (const int rc = beam_check(desc, ext)) return rc;
  CaCtcBeamExt x = *ext;
  CA_CHECK_ARG(x.n_best >= 1 && x.n_best <= desc->beam_width, "ca_ctc_beam_decode_ex: n_best %d outside 1..beam_width = %d",
               x.n_best, desc->beam_width);
  CA_CHECK_ARG(x.ids_n && x.len_n && x.score_n && x.logit_n && x.lm_n && x.n_out,
               "ca_ctc_beam_decode_ex: null output pointer");
  CA_CHECK_ARG((int64_t)x.n_best * desc->T < ((int64_t)1 << 31), "ca_ctc_beam_decode_ex: n_best x T too large");
  CA_CHECK_ARG(x.n_hot >= 0, "ca_ctc_beam_decode_ex: negative hotword table size");
  CA_CHECK_ARG(x.n_hot > 0 || !(x.hot_keys || x.hot_frac || x.hot_word),
               "ca_ctc_beam_decode_ex: hotword table pointers without a count");
  CA_CHECK_ARG(x.n_hot == 0 || (x.hot_keys && x.hot_frac && x.hot_word),
               "ca_ctc_beam_decode_ex: %lld hotword prefixes without their tables", (long long)x.n_hot);
  CA_CHECK_ARG(x.hotword_weight - x.hotword_weight == 0.f, "ca_ctc_beam_decode_ex: hotword_weight must be a finite number");
  if (x.hotword_weight == 0.f) x.n_hot = 0;  // "no hotwords": the search the plain entry runs
  hipLaunchKernelGGL(ctc_beam_kernel<true>, dim3(desc->B), dim3(BEAM_THREADS), 0, (hipStream_t)stream, *desc, x);
  CA_CHECK_LAUNCH("ca_ctc_beam_decode_ex");
  return CA_OK;
}
