// Overlap merge of token sequences (ca_overlap_merge, include/coral_amd.h): the chunks of one long Whisper recording
// overlap in audio, so consecutive chunks' token sequences overlap in text; the merge finds where and cuts both sides in
// the middle of the overlap.  The rule is the contract (the header states it; tests/whisper_chunk_ref.py restates it in
// plain Python; it is transformers' `_find_longest_common_sequence`):
//     for i = 1 .. L + R - 1:  matches = #{k : left[max(0, L-i) + k] == right[max(0, i-L) + k]},
//                              score = matches / i + i / 10000.0   (float64: a division, a division, an addition)
//     the winner is the greatest score among the diagonals with matches > 1, the smaller i among equal scores.
//
// One workgroup of 256 lanes per group.  Both sides live in LDS (2 x 1024 int32 = 8 KB); a row is compacted while it is
// loaded (an id whose bit is set in the skip bitmap is dropped: wave ballot + prefix count, the waves' totals through
// LDS).  The boundaries of a group depend on each other (the left side of boundary j is what boundary j-1 left of row
// j), so they are walked in order; inside one boundary the diagonals are dealt round-robin to the lanes - lane t takes
// i = 1 + t, 257 + t, ... - so that neighbouring lanes read neighbouring LDS words of `left` (no bank conflict) and the
// same word of `right` (a broadcast) while i <= L, and the lanes' work (the overlap length of diagonal i) differs by
// one compare.  A lane walks its diagonals in ascending i and replaces its best only on a strictly greater score, the
// wave and the workgroup reductions take the greater score and then the smaller i: together the rule's tie order.
// One fp64 score per diagonal - L + R of them per boundary beside L x R integer compares - so the fp64 rate is not in
// the way.  After the cut, `right[right_mid:]` becomes `left` by moving a pointer, not the tokens.
// Every loop bound is known at loop entry; no atomics, no spinning, nothing between workgroups.
#include "common.h"

#define CA_MERGE_THREADS 256
#define CA_MERGE_WAVES (CA_MERGE_THREADS / CA_WAVE)
#define CA_MERGE_NONE 0x7fffffff  // the diagonal of a lane (wave, workgroup) that accepted none

// (greater score, then smaller i)
__device__ __forceinline__ bool merge_better(double s, int32_t i, double bs, int32_t bi) {
  return s > bs || (s == bs && i < bi);
}

// Row src[0 .. n) -> dst[0 .. count) without the ids the bitmap names; -> count (the same in every lane).
// `parity` alternates the totals' slot, so that one barrier a round is enough.
__device__ __forceinline__ int32_t merge_load_row(const int32_t* __restrict__ src, int32_t n,
                                                  const uint32_t* __restrict__ skip, int32_t skip_bits, int32_t* dst,
                                                  int32_t (*wave_total)[CA_MERGE_WAVES], int32_t& parity) {
  const int32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int32_t count = 0;
  for (int32_t base = 0; base < n; base += CA_MERGE_THREADS) {
    const int32_t k = base + tid;
    int32_t id = 0;
    bool keep = false;
    if (k < n) {
      id = src[k];
      keep = true;
      if (skip != nullptr && (uint32_t)id < (uint32_t)skip_bits) keep = ((skip[(uint32_t)id >> 5] >> (id & 31)) & 1u) == 0;
    }
    const unsigned long long kept = __ballot(keep);
    const int32_t before = __popcll(kept & ((1ull << lane) - 1ull));
    if (lane == 0) wave_total[parity][wave] = __popcll(kept);
    __syncthreads();
    int32_t off = 0, total = 0;
#pragma unroll
    for (int32_t w = 0; w < CA_MERGE_WAVES; ++w) {
      const int32_t t = wave_total[parity][w];
      off += w < wave ? t : 0;
      total += t;
    }
    if (keep) dst[count + off + before] = id;
    count += total;
    parity ^= 1;
  }
  __syncthreads();
  return count;
}

__global__ __launch_bounds__(CA_MERGE_THREADS) void overlap_merge_kernel(
    const int32_t* __restrict__ ids, int64_t ld, const int32_t* __restrict__ row_start,
    const int32_t* __restrict__ row_len, int32_t rows, int32_t max_row_len, const uint32_t* __restrict__ skip,
    int32_t skip_bits, const int32_t* __restrict__ group_off, const int32_t* __restrict__ out_off,
    int32_t* __restrict__ out, int64_t out_cap, int32_t* __restrict__ out_len, int32_t* __restrict__ cuts) {
#pragma clang fp contract(off)
  __shared__ int32_t buf[2][CA_CHUNK_MERGE_MAX_TOKENS];
  __shared__ int32_t wave_total[2][CA_MERGE_WAVES];
  __shared__ double red_score[CA_MERGE_WAVES];
  __shared__ int32_t red_i[CA_MERGE_WAVES];
  const int32_t g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t r0 = group_off[g], r1 = group_off[g + 1];
  const int64_t o0 = out_off[g], o1 = out_off[g + 1];
  // offsets and rows the contract does not allow: the group is marked and nothing is read or written through them
  int32_t bad = !(r0 >= 0 && r1 >= r0 && r1 <= rows && o0 >= 0 && o1 >= o0 && o1 <= out_cap);
  if (!bad) {
    for (int32_t r = r0 + tid; r < r1; r += CA_MERGE_THREADS) {
      const int32_t s = row_start != nullptr ? row_start[r] : 0, n = row_len[r];
      if (s < 0 || n < 0 || n > max_row_len || (int64_t)s + n > ld) bad = 1;
    }
  }
  if (__syncthreads_or(bad)) {
    if (tid == 0) out_len[g] = -1;
    return;
  }
  const int64_t cap = o1 - o0;
  int32_t* __restrict__ dst = out + o0;
  int64_t pos = 0;
  int32_t parity = 0, side = 0, L = 0;
  int32_t* left = buf[0];
  if (r1 > r0) {
    L = merge_load_row(ids + (int64_t)r0 * ld + (row_start != nullptr ? row_start[r0] : 0), row_len[r0], skip, skip_bits,
                       buf[0], wave_total, parity);
    if (cuts != nullptr && tid == 0) cuts[2 * (int64_t)r0] = cuts[2 * (int64_t)r0 + 1] = -1;
  }
  for (int32_t r = r0 + 1; r < r1; ++r) {
    int32_t* right = buf[side ^ 1];  // (the buffer the last cut left dead)
    const int32_t R = merge_load_row(ids + (int64_t)r * ld + (row_start != nullptr ? row_start[r] : 0), row_len[r], skip,
                                     skip_bits, right, wave_total, parity);
    const int32_t last = L + R - 1;
    double best = 0.0;
    int32_t best_i = CA_MERGE_NONE;
    for (int32_t i = 1 + tid; i <= last; i += CA_MERGE_THREADS) {
      const int32_t ls = max(0, L - i), le = min(L, L + R - i), rs = max(0, i - L);
      const int32_t* a = left + ls;
      const int32_t* b = right + rs;
      int32_t matches = 0;
      for (int32_t k = 0; k < le - ls; ++k) matches += a[k] == b[k] ? 1 : 0;
      if (matches > 1) {
        const double ratio = (double)matches / (double)i;
        const double eps = (double)i / 10000.0;
        const double score = ratio + eps;
        if (score > best) {
          best = score;
          best_i = i;
        }
      }
    }
#pragma unroll
    for (int32_t o = 32; o > 0; o >>= 1) {
      const double s = __shfl_xor(best, o, 64);
      const int32_t i = __shfl_xor(best_i, o, 64);
      if (merge_better(s, i, best, best_i)) {
        best = s;
        best_i = i;
      }
    }
    if (lane == 0) {
      red_score[wave] = best;
      red_i[wave] = best_i;
    }
    __syncthreads();
    best = red_score[0];
    best_i = red_i[0];
#pragma unroll
    for (int32_t w = 1; w < CA_MERGE_WAVES; ++w)
      if (merge_better(red_score[w], red_i[w], best, best_i)) {
        best = red_score[w];
        best_i = red_i[w];
      }
    int32_t left_mid = L, right_mid = 0;  // no diagonal accepted: plain concatenation
    if (best_i != CA_MERGE_NONE) {
      const int32_t i = best_i;
      left_mid = (max(0, L - i) + min(L, L + R - i)) >> 1;
      right_mid = (max(0, i - L) + min(R, i)) >> 1;
    }
    for (int32_t k = tid; k < left_mid; k += CA_MERGE_THREADS)
      if (pos + k < cap) dst[pos + k] = left[k];
    pos += left_mid;
    if (cuts != nullptr && tid == 0) {
      cuts[2 * (int64_t)r] = left_mid;
      cuts[2 * (int64_t)r + 1] = right_mid;
    }
    // (the next row is loaded over the old left side: merge_load_row's first barrier stands between these reads and
    // its writes, and between the reads of red_* above and the next boundary's writes)
    side ^= 1;
    left = right + right_mid;
    L = R - right_mid;
  }
  for (int32_t k = tid; k < L; k += CA_MERGE_THREADS)
    if (pos + k < cap) dst[pos + k] = left[k];
  pos += L;
  if (tid == 0) out_len[g] = pos <= cap ? (int32_t)pos : -1;
}

extern "C" int ca_overlap_merge(const int32_t* ids, int64_t ld, const int32_t* row_start, const int32_t* row_len,
                                int32_t rows, int32_t max_row_len, const uint32_t* skip, int32_t skip_bits,
                                const int32_t* group_off, const int32_t* out_off, int32_t G, int32_t* out, int64_t out_cap,
                                int32_t* out_len, int32_t* cuts, void* stream) {
  CA_CHECK_ARG(ids && row_len && group_off && out_off && out && out_len, "ca_overlap_merge: null pointer");
  CA_CHECK_ARG(rows >= 1 && G >= 1 && ld >= 1, "ca_overlap_merge: rows = %d, G = %d and ld = %lld must be positive", rows, G,
               (long long)ld);
  CA_CHECK_ARG(max_row_len >= 0 && max_row_len <= CA_CHUNK_MERGE_MAX_TOKENS,
               "ca_overlap_merge: max_row_len = %d is outside 0 .. %d (CA_CHUNK_MERGE_MAX_TOKENS: both sides of a boundary "
               "live in LDS)", max_row_len, CA_CHUNK_MERGE_MAX_TOKENS);
  CA_CHECK_ARG(skip == nullptr ? skip_bits == 0 : skip_bits >= 1,
               "ca_overlap_merge: skip_bits = %d must be 0 without a bitmap and positive with one", skip_bits);
  CA_CHECK_ARG(out_cap >= 0 && out_cap < (1ll << 31), "ca_overlap_merge: out_cap = %lld is outside [0, 2^31)",
               (long long)out_cap);
  hipLaunchKernelGGL(overlap_merge_kernel, dim3((unsigned)G), dim3(CA_MERGE_THREADS), 0, (hipStream_t)stream, ids, ld,
                     row_start, row_len, rows, max_row_len, skip, skip_bits, group_off, out_off, out, out_cap, out_len,
                     cuts);
  CA_CHECK_LAUNCH("ca_overlap_merge");
  return CA_OK;
}
