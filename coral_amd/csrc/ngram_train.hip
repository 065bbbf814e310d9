// Modified Kneser-Ney n-gram training (coral_amd/ngram_train.py; the estimator is defined in DESIGN.md §8).
//
// Stages, each a few launches on the caller's stream, none allocating or synchronising:
//   tokenise   raw bytes -> (start, length, line, 64-bit hash) per word: a count pass, a scan of the block counts, an emit
//              pass; one workgroup per CA_NGT_TOK_SPAN bytes, 16 bytes per thread.
//   vocabulary an open-addressing table keyed by the word hash.  Bytes are compared on probe, without waiting on another
//              thread: a round is a claim launch (CAS the key, atomicMin of offset << 8 | length: the first occurrence
//              becomes the slot's representative) and a verify launch (compare with the representative's bytes, in the
//              chunk for a slot that is new in this chunk, in the arena for an older one).  A word that differs from the
//              representative of a slot with its hash skips that slot in the next round.  The commit launch copies the
//              bytes of every new word into the arena and lists the new slots for the host, which gives out the ids.
//   count      one thread per word inserts the n-grams of orders 1..N that end at it (and at </s> behind the last word
//              of a line, and the unigram <s> in front of the first); the unigram increments of equal words are summed
//              inside the wave first (measured on 10^8 Zipf tokens: the stage 148 -> 106 ms).  Keys are the NGRAM_SEED hashes of the id tuples;
//              the tuple is stored packed in three 64-bit words that every occurrence CASes from EMPTY to its own value
//              and compares: two different tuples with one hash differ in a word, so one of them sees the mismatch and
//              the run is refused (the decoder's tables are keyed by the same hash and refuse the same collision).
//   adjust     every (n+1)-gram finds its suffix and its prefix in the n-table: distinct left extensions, adjusted counts.
//   statistics count-of-counts per order, Z and N_1..N_3 per context.
//   probs      fp64, order 1 upwards, from the integer statistics and the host's discounts.
//   prune / export keep flags from the raw counts, top order first, and compaction.
// Every cross-thread sum is an integer atomic, so every number is independent of arrival order.  Every probe loop is
// bounded by NGT_MAX_PROBE; a full table sets a bit of status[CA_NGT_ST_OVERFLOW] and the host raises.
#include "common.h"

#define NGT_TOKEN_SEED 0x082EFA98EC4E6C89ull
#define NGT_NGRAM_SEED 0xA4093822299F31D0ull
#define NGT_BLOCK 256
#define NGT_BYTES_PER_THREAD 16
#define NGT_MAX_PROBE 4096
#define NGT_PEEL 4
#define NGT_EMPTY 0xFFFFFFFFFFFFFFFFull
#define NGT_UNK 0
#define NGT_BOS 1
#define NGT_EOS 2

static_assert(NGT_BLOCK * NGT_BYTES_PER_THREAD == CA_NGT_TOK_SPAN, "span");

typedef unsigned long long u64;
typedef unsigned int u32;

__device__ __forceinline__ u64 ngt_mix(u64 h, int x) {  // mix64 of coral_amd/ngram.py
  u64 z = (h ^ (u64)(int64_t)(x + 1)) * 0x9E3779B97F4A7C15ull;
  z ^= z >> 32;
  z *= 0xD6E8FEB86659FD93ull;
  z ^= z >> 32;
  return z;
}
__device__ __forceinline__ bool ngt_ws(unsigned char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n'; }
__device__ __forceinline__ u64 ngt_ld(const void* p) { return __hip_atomic_load((const u64*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void ngt_flag(u64* status, int word, u64 bits) { atomicOr(&status[word], bits); }

// ------------------------------------------------------------------------------------------------ tokeniser
// word-start and line-feed masks of the 16 bytes of one thread (bytes behind n count as whitespace, not as line feeds)
__device__ __forceinline__ void ngt_masks(const uint8_t* text, int64_t n, int64_t i0, u32& starts, u32& lfs) {
  starts = 0;
  lfs = 0;
  if (i0 >= n) return;
  alignas(16) unsigned char b[NGT_BYTES_PER_THREAD];
  if (i0 + NGT_BYTES_PER_THREAD <= n && (((uintptr_t)(text + i0)) & 15) == 0) {
    *(uint4*)b = *(const uint4*)(text + i0);
  } else {
#pragma unroll
    for (int k = 0; k < NGT_BYTES_PER_THREAD; ++k) b[k] = i0 + k < n ? text[i0 + k] : (unsigned char)' ';
  }
  bool prev_ws = i0 == 0 ? true : ngt_ws(text[i0 - 1]);
#pragma unroll
  for (int k = 0; k < NGT_BYTES_PER_THREAD; ++k) {
    const bool w = ngt_ws(b[k]);
    if (!w && prev_ws) starts |= 1u << k;
    if (b[k] == '\n' && i0 + k < n) lfs |= 1u << k;
    prev_ws = w;
  }
}

// exclusive scan of (a, b) over the NGT_BLOCK threads of a workgroup; tot = the workgroup's sums
__device__ __forceinline__ void ngt_block_scan2(int a, int b, int& ea, int& eb, int& ta, int& tb) {
  __shared__ int sa[NGT_BLOCK], sb[NGT_BLOCK];
  const int t = threadIdx.x;
  sa[t] = a;
  sb[t] = b;
  __syncthreads();
  for (int o = 1; o < NGT_BLOCK; o <<= 1) {
    int va = 0, vb = 0;
    if (t >= o) {
      va = sa[t - o];
      vb = sb[t - o];
    }
    __syncthreads();
    sa[t] += va;
    sb[t] += vb;
    __syncthreads();
  }
  ea = sa[t] - a;
  eb = sb[t] - b;
  ta = sa[NGT_BLOCK - 1];
  tb = sb[NGT_BLOCK - 1];
  __syncthreads();
}

__global__ __launch_bounds__(NGT_BLOCK) void ngt_tok_count(const uint8_t* text, int64_t n, int32_t* blk) {
  const int64_t i0 = ((int64_t)blockIdx.x * NGT_BLOCK + threadIdx.x) * NGT_BYTES_PER_THREAD;
  u32 starts, lfs;
  ngt_masks(text, n, i0, starts, lfs);
  int ea, eb, ta, tb;
  ngt_block_scan2(__popc(starts), __popc(lfs), ea, eb, ta, tb);
  if (threadIdx.x == 0) {
    blk[2 * blockIdx.x] = ta;
    blk[2 * blockIdx.x + 1] = tb;
  }
}

// blk[2 i], blk[2 i + 1] -> exclusive prefix sums over the blocks, in place; totals to status (one workgroup)
__global__ __launch_bounds__(1024) void ngt_tok_scan(int32_t* blk, int64_t nblk, u64* status) {
  __shared__ int64_t pa[1024], pb[1024];
  const int t = threadIdx.x;
  const int64_t per = (nblk + 1023) / 1024;
  const int64_t lo = t * per, hi = lo + per < nblk ? lo + per : nblk;
  int64_t a = 0, b = 0;
  for (int64_t i = lo; i < hi; ++i) {
    a += blk[2 * i];
    b += blk[2 * i + 1];
  }
  pa[t] = a;
  pb[t] = b;
  __syncthreads();
  if (t == 0) {
    int64_t ra = 0, rb = 0;
    for (int i = 0; i < 1024; ++i) {
      const int64_t xa = pa[i], xb = pb[i];
      pa[i] = ra;
      pb[i] = rb;
      ra += xa;
      rb += xb;
    }
    status[CA_NGT_ST_WORDS] = (u64)ra;
    status[CA_NGT_ST_LINES] = (u64)rb;
  }
  __syncthreads();
  a = pa[t];
  b = pb[t];
  for (int64_t i = lo; i < hi; ++i) {
    const int xa = blk[2 * i], xb = blk[2 * i + 1];
    blk[2 * i] = (int32_t)a;
    blk[2 * i + 1] = (int32_t)b;
    a += xa;
    b += xb;
  }
}

__global__ __launch_bounds__(NGT_BLOCK) void ngt_tok_emit(const uint8_t* text, int64_t n, int64_t base_off, const int32_t* blk,
                                                          int32_t hash_bits, int32_t* w_start, int32_t* w_len, int32_t* w_line,
                                                          u64* w_hash, int64_t max_words, u64* status) {
  const int64_t i0 = ((int64_t)blockIdx.x * NGT_BLOCK + threadIdx.x) * NGT_BYTES_PER_THREAD;
  u32 starts, lfs;
  ngt_masks(text, n, i0, starts, lfs);
  int ea, eb, ta, tb;
  ngt_block_scan2(__popc(starts), __popc(lfs), ea, eb, ta, tb);
  int64_t wi = (int64_t)blk[2 * blockIdx.x] + ea;
  int line = blk[2 * blockIdx.x + 1] + eb;
  for (int k = 0; k < NGT_BYTES_PER_THREAD; ++k) {
    if (starts >> k & 1u) {
      const int64_t s = i0 + k;
      u64 h = NGT_TOKEN_SEED;
      int len = 0;
      while (s + len < n && len <= CA_NGT_MAX_WORD_BYTES) {
        const unsigned char c = text[s + len];
        if (ngt_ws(c)) break;
        if (len < CA_NGT_MAX_WORD_BYTES) h = ngt_mix(h, (int)c);
        ++len;
      }
      if (len > CA_NGT_MAX_WORD_BYTES) {  // refused by the host, by name; the record keeps the first 255 bytes
        atomicAdd(&status[CA_NGT_ST_LONG], 1ull);
        atomicMin(&status[CA_NGT_ST_LONG_AT], (u64)(base_off + s));
        len = CA_NGT_MAX_WORD_BYTES;
      }
      if (hash_bits < 64) h &= (1ull << hash_bits) - 1ull;
      if (h == 0) h = 1;
      if (wi < max_words) {
        w_start[wi] = (int32_t)s;
        w_len[wi] = len;
        w_line[wi] = line;
        w_hash[wi] = h;
      } else {
        ngt_flag(status, CA_NGT_ST_OVERFLOW, 1ull << 7);
      }
      ++wi;
    }
    if (lfs >> k & 1u) ++line;
  }
}

// ------------------------------------------------------------------------------------------------ vocabulary
struct NgtVocab {
  u64* key;       // [cap] word hash, 0 = empty
  u64* rep;       // [cap] (byte offset in the corpus << 8 | length) of the first occurrence, ~0 before any
  int64_t* arena_at;  // [cap] offset of the word's bytes in the arena, -1 while the slot is new in this chunk
  int64_t cap;
};

__global__ __launch_bounds__(NGT_BLOCK) void ngt_vocab_claim(NgtVocab v, const int32_t* w_start, const int32_t* w_len,
                                                             const u64* w_hash, const int32_t* w_skip, const int32_t* w_slot,
                                                             int32_t* w_cand, int64_t nw, int64_t base_off, u64* status) {
  const int64_t j = (int64_t)blockIdx.x * NGT_BLOCK + threadIdx.x;
  if (j >= nw || w_slot[j] >= 0) return;
  const u64 h = w_hash[j], mask = (u64)v.cap - 1;
  const u64 me = ((u64)(base_off + w_start[j]) << 8) | (u64)w_len[j];
  int skip = w_skip[j];
  const int64_t bound = v.cap < NGT_MAX_PROBE ? v.cap : NGT_MAX_PROBE;
  u64 idx = h & mask;
  int32_t cand = -1;
  for (int64_t p = 0; p < bound; ++p) {
    u64 k = ngt_ld(&v.key[idx]);
    if (k == 0) {
      const u64 old = atomicCAS(&v.key[idx], 0ull, h);
      k = old == 0 ? h : old;
    }
    if (k == h) {
      if (skip == 0) {
        atomicMin(&v.rep[idx], me);
        cand = (int32_t)idx;
        break;
      }
      --skip;
    }
    idx = (idx + 1) & mask;
  }
  if (cand < 0) ngt_flag(status, CA_NGT_ST_OVERFLOW, 1ull);
  w_cand[j] = cand;
}

__global__ __launch_bounds__(NGT_BLOCK) void ngt_vocab_verify(NgtVocab v, const uint8_t* text, const uint8_t* arena,
                                                              const int32_t* w_start, const int32_t* w_len, int32_t* w_skip,
                                                              int32_t* w_slot, const int32_t* w_cand, int64_t nw, int64_t n,
                                                              int64_t base_off, u64* status) {
  const int64_t j = (int64_t)blockIdx.x * NGT_BLOCK + threadIdx.x;
  if (j >= nw || w_slot[j] >= 0) return;
  const int32_t idx = w_cand[j];
  if (idx < 0) return;
  const u64 r = v.rep[idx];
  const int len = w_len[j];
  bool same = (int)(r & 255ull) == len;
  if (same) {
    const int64_t at = v.arena_at[idx];
    const uint8_t* src;
    if (at >= 0) {
      src = arena + at;
    } else {
      const int64_t off = (int64_t)(r >> 8) - base_off;
      if (off < 0 || off + len > n) {  // cannot happen: a slot without arena bytes was claimed in this chunk
        atomicAdd(&status[CA_NGT_ST_MISS], 1ull);
        return;
      }
      src = text + off;
    }
    const uint8_t* mine = text + w_start[j];
    for (int k = 0; k < len; ++k) same &= src[k] == mine[k];
  }
  if (same) {
    w_slot[j] = idx;
  } else {
    w_skip[j] += 1;
    atomicAdd(&status[CA_NGT_ST_PENDING], 1ull);
  }
}

__global__ __launch_bounds__(NGT_BLOCK) void ngt_vocab_commit(NgtVocab v, const uint8_t* text, uint8_t* arena, u64* arena_top,
                                                              int64_t arena_cap, const int32_t* w_start, const int32_t* w_len,
                                                              const int32_t* w_slot, int64_t nw, int64_t base_off,
                                                              int32_t* new_slot, u64* new_count, u64* status) {
  const int64_t j = (int64_t)blockIdx.x * NGT_BLOCK + threadIdx.x;
  if (j >= nw) return;
  const int32_t idx = w_slot[j];
  if (idx < 0 || v.arena_at[idx] >= 0) return;
  const int len = w_len[j];
  const u64 me = ((u64)(base_off + w_start[j]) << 8) | (u64)len;
  if (v.rep[idx] != me) return;  // exactly one occurrence is the slot's first: only it goes on (and only it writes arena_at)
  const u64 at = atomicAdd(arena_top, (u64)len);
  if ((int64_t)(at + len) > arena_cap) {
    ngt_flag(status, CA_NGT_ST_OVERFLOW, 1ull << 6);
    return;
  }
  const uint8_t* mine = text + w_start[j];
  for (int k = 0; k < len; ++k) arena[at + k] = mine[k];
  v.arena_at[idx] = (int64_t)at;
  const u64 k = atomicAdd(new_count, 1ull);
  if ((int64_t)k < nw) new_slot[k] = idx;
}

// ------------------------------------------------------------------------------------------------ n-gram tables
__device__ __forceinline__ u64 ngt_hash(const int* g, int n) {
  u64 h = NGT_NGRAM_SEED;
  for (int i = 0; i < n; ++i) h = ngt_mix(h, g[i]);
  return h == 0 ? 1 : h;
}
__device__ __forceinline__ u64 ngt_pack(const int* g, int n, int w) {
  const u64 lo = 2 * w < n ? (u64)(u32)g[2 * w] : 0ull;
  const u64 hi = 2 * w + 1 < n ? (u64)(u32)g[2 * w + 1] : 0ull;
  return lo | hi << 32;
}
__device__ __forceinline__ void ngt_unpack(const uint64_t* ids, int64_t idx, int n, int* g) {
  for (int w = 0; 2 * w < n; ++w) {
    const u64 x = ids[3 * idx + w];
    g[2 * w] = (int)(u32)x;
    if (2 * w + 1 < n) g[2 * w + 1] = (int)(u32)(x >> 32);
  }
}

// insert g (order n) and add `add` to its raw count -> slot or -1 (table full: the overflow bit of the order is set)
__device__ __forceinline__ int64_t ngt_insert(const CaNgramTables& t, int n, const int* g, u32 add) {
  const int o = n - 1;
  const u64 h = ngt_hash(g, n), mask = (u64)t.cap[o] - 1;
  const int64_t bound = t.cap[o] < NGT_MAX_PROBE ? t.cap[o] : NGT_MAX_PROBE;
  u64 idx = h & mask;
  for (int64_t p = 0; p < bound; ++p) {
    u64 k = ngt_ld(&t.key[o][idx]);
    if (k == 0) {
      const u64 old = atomicCAS((u64*)&t.key[o][idx], 0ull, h);
      k = old == 0 ? h : old;
    }
    if (k == h) {
      for (int w = 0; 2 * w < n; ++w) {
        const u64 mine = ngt_pack(g, n, w);
        u64 cur = ngt_ld(&t.ids[o][3 * idx + w]);
        if (cur == NGT_EMPTY) {
          const u64 old = atomicCAS((u64*)&t.ids[o][3 * idx + w], NGT_EMPTY, mine);
          cur = old == NGT_EMPTY ? mine : old;
        }
        if (cur != mine) atomicAdd((u64*)&t.status[CA_NGT_ST_COLLISION], 1ull);
      }
      if (add) atomicAdd(&t.count[o][idx], add);
      return (int64_t)idx;
    }
    idx = (idx + 1) & mask;
  }
  ngt_flag((u64*)t.status, CA_NGT_ST_OVERFLOW, 1ull << n);
  return -1;
}

// slot of g (order n) or -1 (and a count in status[CA_NGT_ST_MISS]: every gram looked up here was inserted before)
__device__ __forceinline__ int64_t ngt_find(const CaNgramTables& t, int n, const int* g) {
  const int o = n - 1;
  const u64 h = ngt_hash(g, n), mask = (u64)t.cap[o] - 1;
  const int64_t bound = t.cap[o] < NGT_MAX_PROBE ? t.cap[o] : NGT_MAX_PROBE;
  u64 idx = h & mask;
  for (int64_t p = 0; p < bound; ++p) {
    const u64 k = t.key[o][idx];
    if (k == h) {
      for (int w = 0; 2 * w < n; ++w)
        if (t.ids[o][3 * idx + w] != ngt_pack(g, n, w)) atomicAdd((u64*)&t.status[CA_NGT_ST_COLLISION], 1ull);
      return (int64_t)idx;
    }
    if (k == 0) break;
    idx = (idx + 1) & mask;
  }
  atomicAdd((u64*)&t.status[CA_NGT_ST_MISS], 1ull);
  return -1;
}

__device__ __forceinline__ void ngt_insert_suffixes(const CaNgramTables& t, const int* buf, int len) {
  for (int n = 1; n <= len; ++n) ngt_insert(t, n, buf + len - n, 1u);
}

__global__ __launch_bounds__(NGT_BLOCK) void ngt_count(CaNgramTables t, const int32_t* w_slot, const int32_t* slot_id,
                                                       const int32_t* w_line, int64_t nw, int32_t seed_unk) {
  const int64_t j = (int64_t)blockIdx.x * NGT_BLOCK + threadIdx.x;
  const int N = t.order;
  if (j == 0 && seed_unk) {
    const int g = NGT_UNK;
    ngt_insert(t, 1, &g, 0u);
  }
  bool active = j < nw;
  int buf[CA_NGT_MAX_ORDER + 2];
  int len = 0, line = 0;
  bool first = false;
  if (active) {
    line = w_line[j];
    // the last min(N, position + 1) tokens of the padded sentence that end at word j, oldest first
    int back = 0;
    while (back < N - 1 && j - back - 1 >= 0 && w_line[j - back - 1] == line) ++back;
    const bool at_start = back < N - 1 || j - back - 1 < 0 || w_line[j - back - 1] != line;  // <s> stands in front of them
    first = back == 0 && at_start;
    if (at_start && back + 1 < N) buf[len++] = NGT_BOS;
    for (int i = back; i >= 0; --i) {
      const int32_t s = w_slot[j - i];
      const int32_t id = s >= 0 ? slot_id[s] : -1;
      if (id < 3) active = false;  // a word without an id: the vocabulary stage was skipped or failed
      buf[len++] = id;
    }
    if (!active) atomicAdd((u64*)&t.status[CA_NGT_ST_MISS], 1ull);
  }
  // The unigram of the word itself is where a corpus piles up on few addresses.  Up to NGT_PEEL times the first pending
  // lane of the wave takes the increments of every lane with its word (one atomic for all of them); the lanes left over
  // add 1 each.  All 64 lanes run the ballots; the loop bounds are wave-uniform.
  const int id = active ? buf[len - 1] : -1;
  u32 add = 1;
  bool pending = active;
  const int lane = __lane_id();
  for (int r = 0; r < NGT_PEEL; ++r) {
    const u64 m = __ballot(pending);
    if (!m) break;
    const int lead = __ffsll((long long)m) - 1;
    const int key = __shfl(id, lead, 64);
    const u64 same = __ballot(pending && id == key);
    if (pending && id == key) {
      pending = false;
      add = lane == lead ? (u32)__popcll(same) : 0u;
    }
  }
  if (!active) return;
  if (add) ngt_insert(t, 1, buf + len - 1, add);
  for (int n = 2; n <= len; ++n) ngt_insert(t, n, buf + len - n, 1u);
  if (first) {  // first word of its line: the unigram <s>
    const int g = NGT_BOS;
    ngt_insert(t, 1, &g, 1u);
  }
  if (j + 1 >= nw || w_line[j + 1] != line) {  // last word of its line: the grams that end at </s>
    buf[len++] = NGT_EOS;
    const int drop = len > N ? len - N : 0;
    ngt_insert_suffixes(t, buf + drop, len - drop);
  }
}

// (m)-table, m >= 2: suffix and prefix slots in the (m-1)-table, one left extension for the suffix
__global__ __launch_bounds__(NGT_BLOCK) void ngt_adjust(CaNgramTables t, int m) {
  const int64_t idx = (int64_t)blockIdx.x * NGT_BLOCK + threadIdx.x;
  if (idx >= t.cap[m - 1] || t.key[m - 1][idx] == 0) return;
  int g[CA_NGT_MAX_ORDER + 1];
  ngt_unpack(t.ids[m - 1], idx, m, g);
  const int64_t s = ngt_find(t, m - 1, g + 1), c = ngt_find(t, m - 1, g);
  t.suf_slot[m - 1][idx] = (int32_t)s;
  t.ctx_slot[m - 1][idx] = (int32_t)c;
  if (s >= 0) atomicAdd(&t.left[m - 2][s], 1u);
}

__global__ __launch_bounds__(NGT_BLOCK) void ngt_adjusted(CaNgramTables t, int n) {
  const int64_t idx = (int64_t)blockIdx.x * NGT_BLOCK + threadIdx.x;
  if (idx >= t.cap[n - 1] || t.key[n - 1][idx] == 0) return;
  const int first = (int)(u32)t.ids[n - 1][3 * idx];
  u32 a;
  if (n == 1 && (first == NGT_BOS || first == NGT_UNK)) a = 0;
  else if (n == t.order || first == NGT_BOS) a = t.count[n - 1][idx];
  else a = t.left[n - 1][idx];
  t.adj[n - 1][idx] = a;
}

// count-of-counts of order n into gstat[4 (n-1) + k-1]; the sums of each context into cstat of the (n-1)-table, or into
// gstat[20..23] for the empty context.  Integer atomics, summed per workgroup in LDS first where the target is shared.
__global__ __launch_bounds__(NGT_BLOCK) void ngt_stats(CaNgramTables t, int n) {
  __shared__ u32 s_t[4], s_n[4];
  __shared__ u64 s_z;
  if (threadIdx.x < 4) s_t[threadIdx.x] = 0, s_n[threadIdx.x] = 0;
  if (threadIdx.x == 0) s_z = 0;
  __syncthreads();
  const int64_t idx = (int64_t)blockIdx.x * NGT_BLOCK + threadIdx.x;
  if (idx < t.cap[n - 1] && t.key[n - 1][idx] != 0) {
    const u32 a = t.adj[n - 1][idx];
    if (a > 0) {
      if (a <= 4) atomicAdd(&s_t[a - 1], 1u);
      const int kk = a < 3 ? a : 3;
      if (n == 1) {
        atomicAdd(&s_z, (u64)a);
        atomicAdd(&s_n[kk], 1u);
      } else {
        const int32_t c = t.ctx_slot[n - 1][idx];
        if (c >= 0) {
          atomicAdd(&t.cstat[n - 2][4 * (int64_t)c], a);
          atomicAdd(&t.cstat[n - 2][4 * (int64_t)c + kk], 1u);
        }
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < 4 && s_t[threadIdx.x]) atomicAdd((u64*)&t.gstat[4 * (n - 1) + threadIdx.x], (u64)s_t[threadIdx.x]);
  if (n == 1) {
    if (threadIdx.x == 0 && s_z) atomicAdd((u64*)&t.gstat[20], s_z);
    if (threadIdx.x >= 1 && threadIdx.x < 4 && s_n[threadIdx.x]) atomicAdd((u64*)&t.gstat[20 + threadIdx.x], (u64)s_n[threadIdx.x]);
  }
}

__device__ __forceinline__ double ngt_gamma(const double* D, double n1, double n2, double n3, double Z) {
  return (D[1] * n1 + D[2] * n2 + D[3] * n3) / Z;
}

// p_n of every n-gram, from p_{n-1} (launched for n = 1, 2, ..; disc[4 (n-1) + k] = D_n(k), D_n(0) = 0)
__global__ __launch_bounds__(NGT_BLOCK) void ngt_probs(CaNgramTables t, int n, const double* disc, int64_t vocab) {
  const int64_t idx = (int64_t)blockIdx.x * NGT_BLOCK + threadIdx.x;
  if (idx >= t.cap[n - 1] || t.key[n - 1][idx] == 0) return;
  const u32 a = t.adj[n - 1][idx];
  const double* D = disc + 4 * (n - 1);
  const double d = D[a < 3 ? a : 3];
  double p;
  if (n == 1) {
    const double Z = (double)t.gstat[20];
    const double gam = ngt_gamma(D, (double)t.gstat[21], (double)t.gstat[22], (double)t.gstat[23], Z);
    p = ((double)a - d) / Z + gam / (double)(vocab - 1);
  } else {
    const int32_t c = t.ctx_slot[n - 1][idx], s = t.suf_slot[n - 1][idx];
    if (c < 0 || s < 0) return;
    const u32* cs = &t.cstat[n - 2][4 * (int64_t)c];
    const double Z = (double)cs[0];
    const double gam = ngt_gamma(D, (double)cs[1], (double)cs[2], (double)cs[3], Z);
    p = ((double)a - d) / Z + gam * t.prob[n - 2][s];
  }
  t.prob[n - 1][idx] = p;
}

// keep flags of order m (launched for m = N, N-1, .., 1): raw count above the threshold, or the prefix of a kept gram
__global__ __launch_bounds__(NGT_BLOCK) void ngt_prune(CaNgramTables t, int m, u32 tau) {
  const int64_t idx = (int64_t)blockIdx.x * NGT_BLOCK + threadIdx.x;
  if (idx >= t.cap[m - 1]) return;
  bool keep = false;
  if (t.key[m - 1][idx] != 0) keep = m == 1 || t.count[m - 1][idx] > tau || t.ext[m - 1][idx] != 0;
  t.keep[m - 1][idx] = keep ? 1 : 0;
  if (keep && m >= 2) {
    const int32_t c = t.ctx_slot[m - 1][idx];
    if (c >= 0) t.ext[m - 2][c] = 1;
  }
}

__global__ __launch_bounds__(NGT_BLOCK) void ngt_export(CaNgramTables t, int n, const double* disc, int32_t* out_ids,
                                                        u32* out_int, double* out_f, int64_t out_cap, u64* out_n) {
  const int64_t idx = (int64_t)blockIdx.x * NGT_BLOCK + threadIdx.x;
  const bool keep = idx < t.cap[n - 1] && t.keep[n - 1][idx] != 0;
  // one atomic per wave: the kept lanes take consecutive rows behind the wave's base (the host sorts the rows)
  const u64 m = __ballot(keep);
  const int lane = __lane_id();
  u64 base = 0;
  const int leader = m ? __ffsll((long long)m) - 1 : 0;
  if (m && lane == leader) base = atomicAdd(out_n, (u64)__popcll(m));
  base = __shfl(base, leader, 64);
  if (!keep) return;
  const int64_t row = (int64_t)base + __popcll(m & ((1ull << lane) - 1ull));
  if (row >= out_cap) {
    ngt_flag((u64*)t.status, CA_NGT_ST_OVERFLOW, 1ull << 8);
    return;
  }
  int g[CA_NGT_MAX_ORDER + 1];
  ngt_unpack(t.ids[n - 1], idx, n, g);
  for (int i = 0; i < n; ++i) out_ids[row * n + i] = g[i];
  u32 cs[4] = {0, 0, 0, 0};
  if (n < t.order)
    for (int i = 0; i < 4; ++i) cs[i] = t.cstat[n - 1][4 * idx + i];
  out_int[row * 6 + 0] = t.count[n - 1][idx];
  out_int[row * 6 + 1] = t.adj[n - 1][idx];
  for (int i = 0; i < 4; ++i) out_int[row * 6 + 2 + i] = cs[i];
  const double p = t.prob[n - 1][idx];
  out_f[row * 2 + 0] = (n == 1 && g[0] == NGT_BOS) ? 0.0 : log10(p);
  double bo = 0.0;
  if (n < t.order && cs[0] > 0) bo = log10(ngt_gamma(disc + 4 * n, (double)cs[1], (double)cs[2], (double)cs[3], (double)cs[0]));
  out_f[row * 2 + 1] = bo;
}

// ------------------------------------------------------------------------------------------------ C ABI
static inline unsigned ngt_grid(int64_t n) { return (unsigned)((n + NGT_BLOCK - 1) / NGT_BLOCK); }
static inline bool ngt_pow2(int64_t x) { return x >= 2 && (x & (x - 1)) == 0; }

static int ngt_check_tables(const CaNgramTables* t, const char* who) {
  CA_CHECK_ARG(t != nullptr, "%s: null tables", who);
  CA_CHECK_ARG(t->order >= 1 && t->order <= CA_NGT_MAX_ORDER, "%s: order %d outside 1..%d", who, t->order, CA_NGT_MAX_ORDER);
  CA_CHECK_ARG(t->gstat && t->status, "%s: null gstat or status", who);
  for (int o = 0; o < t->order; ++o) {
    CA_CHECK_ARG(ngt_pow2(t->cap[o]) && t->cap[o] <= (1ll << 31), "%s: capacity %lld of order %d is no power of two in [2, 2^31]",
                 who, (long long)t->cap[o], o + 1);
    CA_CHECK_ARG(t->key[o] && t->ids[o] && t->count[o] && t->left[o] && t->adj[o] && t->ctx_slot[o] && t->suf_slot[o] &&
                     t->cstat[o] && t->prob[o] && t->keep[o] && t->ext[o], "%s: null array in the table of order %d", who, o + 1);
  }
  return CA_OK;
}

extern "C" int64_t ca_ngt_tokenize_blocks(int64_t n) { return n <= 0 ? 0 : (n + CA_NGT_TOK_SPAN - 1) / CA_NGT_TOK_SPAN; }

extern "C" int ca_ngt_tokenize(const uint8_t* text, int64_t n, int64_t base_off, int32_t hash_bits, int32_t* blk,
                               int32_t* w_start, int32_t* w_len, int32_t* w_line, uint64_t* w_hash, int64_t max_words,
                               uint64_t* status, void* stream) {
  CA_CHECK_ARG(text && blk && w_start && w_len && w_line && w_hash && status, "ca_ngt_tokenize: null pointer");
  CA_CHECK_ARG(n > 0 && n < (1ll << 31), "ca_ngt_tokenize: chunk of %lld bytes, must lie in [1, 2^31)", (long long)n);
  CA_CHECK_ARG(base_off >= 0 && base_off < (1ll << 55), "ca_ngt_tokenize: base offset %lld", (long long)base_off);
  CA_CHECK_ARG(hash_bits >= 1 && hash_bits <= 64, "ca_ngt_tokenize: hash_bits %d outside 1..64", hash_bits);
  CA_CHECK_ARG(max_words > 0, "ca_ngt_tokenize: max_words %lld", (long long)max_words);
  hipStream_t s = (hipStream_t)stream;
  const int64_t nblk = ca_ngt_tokenize_blocks(n);
  ngt_tok_count<<<(unsigned)nblk, NGT_BLOCK, 0, s>>>(text, n, blk);
  ngt_tok_scan<<<1, 1024, 0, s>>>(blk, nblk, (u64*)status);
  ngt_tok_emit<<<(unsigned)nblk, NGT_BLOCK, 0, s>>>(text, n, base_off, blk, hash_bits, w_start, w_len, w_line, (u64*)w_hash,
                                                    max_words, (u64*)status);
  CA_CHECK_LAUNCH("ca_ngt_tokenize");
  return CA_OK;
}

static int ngt_check_vocab(const char* who, const void* key, const void* rep, const void* arena_at, int64_t cap) {
  CA_CHECK_ARG(key && rep && arena_at, "%s: null vocabulary table", who);
  CA_CHECK_ARG(ngt_pow2(cap) && cap <= (1ll << 31), "%s: vocabulary capacity %lld is no power of two in [2, 2^31]", who,
               (long long)cap);
  return CA_OK;
}

extern "C" int ca_ngt_vocab_round(uint64_t* vkey, uint64_t* vrep, int64_t* varena_at, int64_t cap, const uint8_t* text, int64_t n,
                                  int64_t base_off, const uint8_t* arena, const int32_t* w_start, const int32_t* w_len,
                                  const uint64_t* w_hash, int32_t* w_skip, int32_t* w_slot, int32_t* w_cand, int64_t nw,
                                  uint64_t* status, void* stream) {
  if (int rc = ngt_check_vocab("ca_ngt_vocab_round", vkey, vrep, varena_at, cap)) return rc;
  CA_CHECK_ARG(text && arena && w_start && w_len && w_hash && w_skip && w_slot && w_cand && status, "ca_ngt_vocab_round: null pointer");
  CA_CHECK_ARG(nw > 0 && n > 0, "ca_ngt_vocab_round: nw %lld, n %lld", (long long)nw, (long long)n);
  hipStream_t s = (hipStream_t)stream;
  NgtVocab v{(u64*)vkey, (u64*)vrep, varena_at, cap};
  ngt_vocab_claim<<<ngt_grid(nw), NGT_BLOCK, 0, s>>>(v, w_start, w_len, (const u64*)w_hash, w_skip, w_slot, w_cand, nw, base_off,
                                                     (u64*)status);
  ngt_vocab_verify<<<ngt_grid(nw), NGT_BLOCK, 0, s>>>(v, text, arena, w_start, w_len, w_skip, w_slot, w_cand, nw, n, base_off,
                                                      (u64*)status);
  CA_CHECK_LAUNCH("ca_ngt_vocab_round");
  return CA_OK;
}

extern "C" int ca_ngt_vocab_commit(uint64_t* vkey, uint64_t* vrep, int64_t* varena_at, int64_t cap, const uint8_t* text,
                                   int64_t base_off, uint8_t* arena, uint64_t* arena_top, int64_t arena_cap,
                                   const int32_t* w_start, const int32_t* w_len, const int32_t* w_slot, int64_t nw,
                                   int32_t* new_slot, uint64_t* new_count, uint64_t* status, void* stream) {
  if (int rc = ngt_check_vocab("ca_ngt_vocab_commit", vkey, vrep, varena_at, cap)) return rc;
  CA_CHECK_ARG(text && arena && arena_top && w_start && w_len && w_slot && new_slot && new_count && status,
               "ca_ngt_vocab_commit: null pointer");
  CA_CHECK_ARG(nw > 0 && arena_cap > 0, "ca_ngt_vocab_commit: nw %lld, arena_cap %lld", (long long)nw, (long long)arena_cap);
  NgtVocab v{(u64*)vkey, (u64*)vrep, varena_at, cap};
  ngt_vocab_commit<<<ngt_grid(nw), NGT_BLOCK, 0, (hipStream_t)stream>>>(v, text, arena, (u64*)arena_top, arena_cap, w_start, w_len,
                                                                       w_slot, nw, base_off, new_slot, (u64*)new_count,
                                                                       (u64*)status);
  CA_CHECK_LAUNCH("ca_ngt_vocab_commit");
  return CA_OK;
}

extern "C" int ca_ngt_count(const CaNgramTables* t, const int32_t* w_slot, const int32_t* slot_id, const int32_t* w_line,
                            int64_t nw, int32_t seed_unk, void* stream) {
  if (int rc = ngt_check_tables(t, "ca_ngt_count")) return rc;
  CA_CHECK_ARG(w_slot && slot_id && w_line && nw > 0, "ca_ngt_count: null pointer or no words");
  ngt_count<<<ngt_grid(nw), NGT_BLOCK, 0, (hipStream_t)stream>>>(*t, w_slot, slot_id, w_line, nw, seed_unk);
  CA_CHECK_LAUNCH("ca_ngt_count");
  return CA_OK;
}

extern "C" int ca_ngt_adjust(const CaNgramTables* t, void* stream) {
  if (int rc = ngt_check_tables(t, "ca_ngt_adjust")) return rc;
  hipStream_t s = (hipStream_t)stream;
  for (int m = t->order; m >= 2; --m) ngt_adjust<<<ngt_grid(t->cap[m - 1]), NGT_BLOCK, 0, s>>>(*t, m);
  for (int n = 1; n <= t->order; ++n) ngt_adjusted<<<ngt_grid(t->cap[n - 1]), NGT_BLOCK, 0, s>>>(*t, n);
  CA_CHECK_LAUNCH("ca_ngt_adjust");
  return CA_OK;
}

extern "C" int ca_ngt_stats(const CaNgramTables* t, void* stream) {
  if (int rc = ngt_check_tables(t, "ca_ngt_stats")) return rc;
  for (int n = 1; n <= t->order; ++n) ngt_stats<<<ngt_grid(t->cap[n - 1]), NGT_BLOCK, 0, (hipStream_t)stream>>>(*t, n);
  CA_CHECK_LAUNCH("ca_ngt_stats");
  return CA_OK;
}

extern "C" int ca_ngt_probs(const CaNgramTables* t, const double* disc, int64_t vocab, void* stream) {
  if (int rc = ngt_check_tables(t, "ca_ngt_probs")) return rc;
  CA_CHECK_ARG(disc && vocab >= 3, "ca_ngt_probs: null discounts or a vocabulary of %lld words", (long long)vocab);
  for (int n = 1; n <= t->order; ++n)
    ngt_probs<<<ngt_grid(t->cap[n - 1]), NGT_BLOCK, 0, (hipStream_t)stream>>>(*t, n, disc, vocab);
  CA_CHECK_LAUNCH("ca_ngt_probs");
  return CA_OK;
}

extern "C" int ca_ngt_prune(const CaNgramTables* t, const int32_t* tau, void* stream) {
  if (int rc = ngt_check_tables(t, "ca_ngt_prune")) return rc;
  CA_CHECK_ARG(tau && tau[0] == 0, "ca_ngt_prune: the unigram threshold must be 0");
  for (int m = 0; m < t->order; ++m) CA_CHECK_ARG(tau[m] >= 0, "ca_ngt_prune: negative threshold");
  for (int m = t->order; m >= 1; --m)
    ngt_prune<<<ngt_grid(t->cap[m - 1]), NGT_BLOCK, 0, (hipStream_t)stream>>>(*t, m, (u32)tau[m - 1]);
  CA_CHECK_LAUNCH("ca_ngt_prune");
  return CA_OK;
}

extern "C" int ca_ngt_export(const CaNgramTables* t, int32_t n, const double* disc, int32_t* out_ids, uint32_t* out_int,
                             double* out_f, int64_t out_cap, uint64_t* out_n, void* stream) {
  if (int rc = ngt_check_tables(t, "ca_ngt_export")) return rc;
  CA_CHECK_ARG(n >= 1 && n <= t->order, "ca_ngt_export: order %d outside 1..%d", n, t->order);
  CA_CHECK_ARG(disc && out_ids && out_int && out_f && out_n && out_cap > 0, "ca_ngt_export: null pointer or no room");
  ngt_export<<<ngt_grid(t->cap[n - 1]), NGT_BLOCK, 0, (hipStream_t)stream>>>(*t, n, disc, out_ids, out_int, out_f, out_cap,
                                                                             (u64*)out_n);
  CA_CHECK_LAUNCH("ca_ngt_export");
  return CA_OK;
}
