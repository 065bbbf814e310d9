// Whisper beam search on the device: ranking the k x V continuations of every clip (ca_beam_select) and the
// bookkeeping of one search step (ca_beam_advance).  The semantics are those of GenerationMixin._beam_search
// ($TF/generation/utils.py:3208-3508): fp32 log_softmax, the suppress mask as -inf after it, + the running beam's
// score, the top 2k of a clip's k x V candidates; EOS candidates among the first k ranks become finished hypotheses
// scored sum_logprob / generated_length ** length_penalty, the best k others the next running beams.
// Order everywhere: higher score first, then the lower flat index beam * V + token.  Nothing here uses an atomic:
// every list is ranked by counting how many entries beat an entry, so the result does not depend on arrival order.
#include "common.h"

#define NEG_INF (-__builtin_inff())
#define BEAM_CHUNK 2048     // logits of one row per workgroup of the first pass
#define BEAM_K2MAX 32       // 2 x CA_BEAM_MAX_BEAMS
#define BEAM_PART 66        // words of a partial: max, sum of exp, 32 values, 32 tokens
#define BEAM_MAXCHUNKS 64   // the row merge holds chunks x 32 candidates in LDS

// ---- pass 1: one read of the logits ---------------------------------------------------------------------------------
// Workgroup (chunk c, row r): the chunk's maximum and sum of exp(x - max) over ALL tokens (the log-softmax is taken
// before the suppress mask, $TF/generation/utils.py:3388-3389) and its best K2 unsuppressed logits.  Each wave takes
// the best K2 of its 512 values by K2 rounds of a wave-wide argmax (no barrier inside), the four lists are ranked
// together through LDS.  The logits are only compared here, so a row's order is that of its raw values; the score
// is formed in the row merge.  (HBM-bound: rows x V x 4 bytes, read once.)
__global__ __launch_bounds__(256) void beam_partial_kernel(const float* __restrict__ logits, int64_t ldv,
                                                           const uint8_t* __restrict__ suppress, int V, int K2,
                                                           int nchunk, float* __restrict__ part) {
  __shared__ float red[8];
  __shared__ float lv[4 * BEAM_K2MAX];
  __shared__ int li[4 * BEAM_K2MAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = blockIdx.x, row = blockIdx.y;
  const float* l = logits + (int64_t)row * ldv;
  float v[8];
  int id[8];
  bool in[8];
  float mx = NEG_INF;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int base = c * BEAM_CHUNK + (i * 256 + tid) * 4;
    f32x4_t x = {NEG_INF, NEG_INF, NEG_INF, NEG_INF};
    unsigned int sm = 0;
    if (base + 3 < V) {
      x = *(const f32x4_t*)(l + base);
      sm = suppress ? *(const unsigned int*)(suppress + base) : 0u;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (base + e < V) {
          x[e] = l[base + e];
          sm |= (suppress && suppress[base + e]) ? (0xffu << (8 * e)) : 0u;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      in[4 * i + e] = base + e < V;
      id[4 * i + e] = base + e;
      v[4 * i + e] = x[e];
      mx = fmaxf(mx, x[e]);
    }
    // (suppressed tokens stay in the statistics and leave the ranking)
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if ((sm >> (8 * e)) & 0xffu) id[4 * i + e] = -1;
  }
  mx = wave_max(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float sum = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) sum += in[e] ? expf(v[e] - mx) : 0.f;
  sum = wave_sum(sum);
  if (lane == 0) red[4 + wave] = sum;
#pragma unroll
  for (int e = 0; e < 8; ++e)
    if (id[e] < 0) v[e] = NEG_INF;
  // the wave's best K2, best first; equal values: the lower token first
  for (int r = 0; r < K2; ++r) {
    float bv = NEG_INF;
    int bi = 0x7fffffff;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (v[e] > bv || (v[e] == bv && v[e] > NEG_INF && id[e] < bi)) {
        bv = v[e];
        bi = id[e];
      }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (lane == 0) {
      lv[wave * K2 + r] = bv;
      li[wave * K2 + r] = bi;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (id[e] == bi) v[e] = NEG_INF;
  }
  __syncthreads();
  float* p = part + ((int64_t)row * nchunk + c) * BEAM_PART;
  if (tid == 0) {
    p[0] = mx;
    p[1] = (red[4] + red[5]) + (red[6] + red[7]);
  }
  const int n = 4 * K2;
  if (tid < n) {
    const float sv = lv[tid];
    const int si = li[tid];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const float ov = lv[j];
      const int oi = li[j];
      rank += (ov > sv || (ov == sv && (oi < si || (oi == si && j < tid)))) ? 1 : 0;
    }
    if (rank < K2) {
      p[2 + rank] = sv;
      ((int*)p)[2 + BEAM_K2MAX + rank] = sv > NEG_INF ? si : -1;
    }
  }
}

// ---- pass 2: a row's log-sum-exp and its best K2 scores ------------------------------------------------------------
// score = ((logit - max) - log(sum exp(logit - max))) + running score: the order of operations of
// F.log_softmax(logits, -1) + running_beam_scores ($TF/generation/utils.py:3388, 3419).  Ranked by (score, token): two
// logits that round to one score take the order of their tokens.  (Latency-bound: chunks x K2 candidates per row.)
__global__ __launch_bounds__(256) void beam_row_kernel(const float* __restrict__ part, int nchunk, int K2,
                                                       const float* __restrict__ run_score, float* __restrict__ row_score,
                                                       int* __restrict__ row_tok) {
  __shared__ float sv[BEAM_MAXCHUNKS * BEAM_K2MAX];
  __shared__ int st[BEAM_MAXCHUNKS * BEAM_K2MAX];
  __shared__ float stat[2];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* p = part + (int64_t)row * nchunk * BEAM_PART;
  if (tid == 0) {
    float M = NEG_INF;
    for (int c = 0; c < nchunk; ++c) M = fmaxf(M, p[c * BEAM_PART]);
    float S = 0.f;
    for (int c = 0; c < nchunk; ++c) S += p[c * BEAM_PART + 1] * expf(p[c * BEAM_PART] - M);
    stat[0] = M;
    stat[1] = logf(S);
  }
  __syncthreads();
  const float M = stat[0], logZ = stat[1], run = run_score[row];
  const int n = nchunk * K2;
  for (int i = tid; i < n; i += 256) {
    const int c = i / K2, r = i - c * K2;
    const float x = p[c * BEAM_PART + 2 + r];
    const int t = ((const int*)p)[c * BEAM_PART + 2 + BEAM_K2MAX + r];
    sv[i] = t >= 0 ? ((x - M) - logZ) + run : NEG_INF;
    st[i] = t;
  }
  __syncthreads();
  for (int i = tid; i < n; i += 256) {
    const float s = sv[i];
    const int64_t key = st[i] >= 0 ? (int64_t)st[i] : ((int64_t)1 << 40) + i;
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const float o = sv[j];
      const int64_t ok = st[j] >= 0 ? (int64_t)st[j] : ((int64_t)1 << 40) + j;
      rank += (o > s || (o == s && ok < key)) ? 1 : 0;
    }
    if (rank < K2) {
      row_score[row * BEAM_K2MAX + rank] = s;
      row_tok[row * BEAM_K2MAX + rank] = st[i];
    }
  }
}

// ---- pass 3: a clip's best K2 of its k rows' K2 ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void beam_clip_kernel(const float* __restrict__ row_score, const int* __restrict__ row_tok,
                                                        int k, int V, float* __restrict__ cand_score,
                                                        int* __restrict__ cand_parent, int* __restrict__ cand_token) {
  __shared__ float sv[16 * BEAM_K2MAX];
  __shared__ int64_t sk[16 * BEAM_K2MAX];
  __shared__ int st[16 * BEAM_K2MAX];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int K2 = 2 * k, n = k * K2;
  for (int i = tid; i < n; i += 256) {
    const int beam = i / K2, r = i - beam * K2;
    const int t = row_tok[(b * k + beam) * BEAM_K2MAX + r];
    sv[i] = row_score[(b * k + beam) * BEAM_K2MAX + r];
    st[i] = t;
    sk[i] = t >= 0 ? (int64_t)beam * V + t : ((int64_t)1 << 40) + i;  // the flat index of $TF/generation/utils.py:3420
  }
  __syncthreads();
  for (int i = tid; i < n; i += 256) {
    const float s = sv[i];
    const int64_t key = sk[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += (sv[j] > s || (sv[j] == s && sk[j] < key)) ? 1 : 0;
    if (rank < K2) {
      cand_score[b * K2 + rank] = s;
      cand_parent[b * K2 + rank] = i / K2;
      cand_token[b * K2 + rank] = st[i];
    }
  }
}

static int beam_chunks(int V) { return (V + BEAM_CHUNK - 1) / BEAM_CHUNK; }

extern "C" int64_t ca_beam_select_workspace_bytes(int32_t B, int32_t k, int32_t V) {
  if (B <= 0 || k <= 0 || V <= 0) return 0;
  const int64_t rows = (int64_t)B * k;
  return rows * beam_chunks(V) * BEAM_PART * 4 + rows * BEAM_K2MAX * 8;
}

extern "C" int ca_beam_select(const float* logits, int64_t ldv, const uint8_t* suppress, const float* run_score,
                              int32_t B, int32_t k, int32_t V, float* cand_score, int32_t* cand_parent,
                              int32_t* cand_token, void* ws, int64_t ws_bytes, void* stream) {
  CA_CHECK_ARG(logits && run_score && cand_score && cand_parent && cand_token && ws, "ca_beam_select: null pointer");
  CA_CHECK_ARG(B > 0 && k >= 1 && k <= CA_BEAM_MAX_BEAMS && (int64_t)B * k <= CA_BEAM_MAX_ROWS,
               "ca_beam_select: 1 <= num_beams <= %d and clips x num_beams <= %d", CA_BEAM_MAX_BEAMS, CA_BEAM_MAX_ROWS);
  CA_CHECK_ARG(V > 0 && ldv >= V && beam_chunks(V) <= BEAM_MAXCHUNKS, "ca_beam_select: vocabulary of 1 .. %d tokens, ldv >= V",
               BEAM_MAXCHUNKS * BEAM_CHUNK);
  CA_CHECK_ARG((ldv % 4) == 0 && ((uintptr_t)logits % 16) == 0 && ((uintptr_t)suppress % 4) == 0 && ((uintptr_t)ws % 16) == 0,
               "ca_beam_select: ldv must be a multiple of 4, logits / ws 16-byte and suppress 4-byte aligned");
  CA_CHECK_ARG(ws_bytes >= ca_beam_select_workspace_bytes(B, k, V), "ca_beam_select: workspace too small");
  const int rows = B * k, nchunk = beam_chunks(V), K2 = 2 * k;
  float* part = (float*)ws;
  float* row_score = part + (int64_t)rows * nchunk * BEAM_PART;
  int* row_tok = (int*)(row_score + (int64_t)rows * BEAM_K2MAX);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(beam_partial_kernel, dim3(nchunk, rows), dim3(256), 0, s, logits, ldv, suppress, V, K2, nchunk, part);
  hipLaunchKernelGGL(beam_row_kernel, dim3(rows), dim3(256), 0, s, part, nchunk, K2, run_score, row_score, row_tok);
  hipLaunchKernelGGL(beam_clip_kernel, dim3(B), dim3(256), 0, s, row_score, row_tok, k, V, cand_score, cand_parent,
                     cand_token);
  CA_CHECK_LAUNCH("ca_beam_select");
  return CA_OK;
}

// ---- one step of bookkeeping -------------------------------------------------------------------------------------------
// One workgroup per clip.  Thread 0 takes the step's decisions from the 2k ranked candidates (a few hundred scalar
// operations), then all threads copy table rows: the ancestry and id rows of the new running beams out of their
// parents' (anc_out[j, :cur] = anc_in[parent_j, :cur], anc_out[j, cur] = row of j) and the ids of new finished hypotheses.
__global__ __launch_bounds__(256) void beam_advance_kernel(const CaBeamDesc d) {
  __shared__ int s_parent[16], s_token[16];
  __shared__ int f_slot[16], f_parent[16], f_token[16];
  __shared__ int s_nfin, s_cur;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int k = d.k, K2 = 2 * d.k, L = d.max_len, P = d.prompt_len;
  const int r0 = b * k;
  if (tid == 0) {
    const int cur = d.pos[r0] + 1;  // tokens of every running sequence
    s_cur = cur;
    s_nfin = 0;
    if (cur >= 1 && cur < L) {
      const bool last = cur + 1 >= d.max_length;  // the length criterion stops every candidate of the last step
      const float* cs = d.cand_score + b * K2;
      const int* cp = d.cand_parent + b * K2;
      const int* ct = d.cand_token + b * K2;
      float val[BEAM_K2MAX];
      bool hit[BEAM_K2MAX];
      for (int c = 0; c < K2; ++c) {
        hit[c] = last || ct[c] == d.eos_id;
        val[c] = cs[c] + (hit[c] ? -1.0e9f : 0.0f);  // $TF/generation/utils.py:3145
      }
      // the next running beams: best k by (val, rank)
      unsigned int taken = 0;
      float best_run = 0.f;
      for (int j = 0; j < k; ++j) {
        int bc = -1;
        for (int c = 0; c < K2; ++c)
          if (!((taken >> c) & 1u) && (bc < 0 || val[c] > val[bc])) bc = c;
        taken |= 1u << bc;
        int par = cp[bc], tk = ct[bc];
        par = par < 0 ? 0 : (par >= k ? k - 1 : par);
        tk = tk < 0 ? d.eos_id : tk;
        s_parent[j] = par;
        s_token[j] = tk;
        d.run_score[r0 + j] = val[bc];
        d.tok[r0 + j] = tk;
        d.pos[r0 + j] = cur;
        d.klen[r0 + j] = cur + 1;
        if (j == 0) best_run = val[bc];
        if (d.tr_parent) {
          const int64_t o = ((int64_t)(cur - P) * d.B + b) * k + j;
          d.tr_parent[o] = par;
          d.tr_token[o] = tk;
          d.tr_score[o] = val[bc];
        }
      }
      // finished hypotheses: EOS (or the last step's) candidates among the first k ranks, unless the clip is closed
      bool full = true;
      for (int j = 0; j < k; ++j) full = full && d.fin_len[r0 + j] > 0;
      const bool open = d.heur[b] != 0 && !(d.early_stopping && full);
      const float den = d.len_pen[cur + 1 - P];
      int nf = 0;
      if (open) {
        for (int c = 0; c < k; ++c) {
          if (!hit[c] || !(cs[c] > NEG_INF)) continue;
          const float fs = cs[c] / den;  // $TF/generation/utils.py:3182
          int slot = -1;
          for (int j = 0; j < k && slot < 0; ++j)
            if (d.fin_len[r0 + j] == 0) slot = j;
          if (slot < 0) {  // a full table: the worst entry (of equal scores the latest) leaves for a better one
            int w = 0;
            for (int j = 1; j < k; ++j)
              if (d.fin_score[r0 + j] < d.fin_score[r0 + w] ||
                  (d.fin_score[r0 + j] == d.fin_score[r0 + w] && d.fin_seq[r0 + j] > d.fin_seq[r0 + w]))
                w = j;
            if (fs > d.fin_score[r0 + w]) slot = w;
          }
          if (slot < 0) continue;
          d.fin_score[r0 + slot] = fs;
          d.fin_len[r0 + slot] = cur + 1;
          d.fin_seq[r0 + slot] = d.fin_count[b]++;
          int par = cp[c];
          par = par < 0 ? 0 : (par >= k ? k - 1 : par);
          f_slot[nf] = slot;
          f_parent[nf] = par;
          f_token[nf] = ct[c] < 0 ? d.eos_id : ct[c];
          ++nf;
        }
      }
      s_nfin = nf;
      // can a running beam still beat the worst finished one?  ($TF/generation/utils.py:3047-3052, sticky)
      full = true;
      float worst = 0.f;
      for (int j = 0; j < k; ++j) {
        full = full && d.fin_len[r0 + j] > 0;
        worst = j == 0 ? d.fin_score[r0] : fminf(worst, d.fin_score[r0 + j]);
      }
      if (d.heur[b]) d.heur[b] = (best_run / den > (full ? worst : -1.0e9f)) ? 1 : 0;
      d.done[b] = (!d.heur[b] || (d.early_stopping && full) || last) ? 1 : 0;
    } else {
      s_cur = -1;
    }
  }
  __syncthreads();
  const int cur = s_cur;
  if (cur < 0) return;
  for (int j = 0; j < k; ++j) {
    const int64_t src = (int64_t)(r0 + s_parent[j]) * L, dst = (int64_t)(r0 + j) * L;
    for (int t = tid; t < cur; t += 256) {
      d.anc_out[dst + t] = d.anc_in[src + t];
      d.ids_out[dst + t] = d.ids_in[src + t];
    }
    if (tid == 0) {
      d.anc_out[dst + cur] = r0 + j;
      d.ids_out[dst + cur] = s_token[j];
    }
  }
  for (int f = 0; f < s_nfin; ++f) {
    const int64_t src = (int64_t)(r0 + f_parent[f]) * L, dst = (int64_t)(r0 + f_slot[f]) * L;
    for (int t = tid; t < cur; t += 256) d.fin_ids[dst + t] = d.ids_in[src + t];
    if (tid == 0) d.fin_ids[dst + cur] = f_token[f];
  }
}

extern "C" int ca_beam_advance(const CaBeamDesc* desc, void* stream) {
  CA_CHECK_ARG(desc, "ca_beam_advance: null descriptor");
  const CaBeamDesc& d = *desc;
  CA_CHECK_ARG(d.B > 0 && d.k >= 1 && d.k <= CA_BEAM_MAX_BEAMS && (int64_t)d.B * d.k <= CA_BEAM_MAX_ROWS,
               "ca_beam_advance: 1 <= num_beams <= %d and clips x num_beams <= %d", CA_BEAM_MAX_BEAMS, CA_BEAM_MAX_ROWS);
  CA_CHECK_ARG(d.max_len > 0 && d.prompt_len >= 1 && d.max_length > d.prompt_len && d.max_length <= d.max_len,
               "ca_beam_advance: 1 <= prompt_len < max_length <= max_len");
  CA_CHECK_ARG(d.cand_score && d.cand_parent && d.cand_token && d.run_score && d.tok && d.pos && d.klen && d.anc_in &&
                   d.anc_out && d.ids_in && d.ids_out && d.fin_score && d.fin_len && d.fin_seq && d.fin_ids &&
                   d.fin_count && d.heur && d.done && d.len_pen,
               "ca_beam_advance: null pointer");
  CA_CHECK_ARG(d.anc_in != d.anc_out && d.ids_in != d.ids_out, "ca_beam_advance: the tables are double-buffered");
  CA_CHECK_ARG((d.tr_parent == nullptr) == (d.tr_token == nullptr) && (d.tr_parent == nullptr) == (d.tr_score == nullptr),
               "ca_beam_advance: the trace takes all three tables");
  hipLaunchKernelGGL(beam_advance_kernel, dim3(d.B), dim3(256), 0, (hipStream_t)stream, d);
  CA_CHECK_LAUNCH("ca_beam_advance");
  return CA_OK;
}
