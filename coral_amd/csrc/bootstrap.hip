// Bootstrap resampling of per-example counts (ca_bootstrap_sums, include/coral_amd.h): sums[g, r, :] = the column sums of
// n_g rows of `vals` drawn with replacement from group g, for every group and every replicate, in one launch.
//
// The draw rule is the contract (the header states it; tests/bootstrap_ref.py restates it in NumPy):
//     idx = ((uint64)(g * R + r) << 32) | j;   u = ca_hash32(seed, idx);   k = ((uint64)u * n_g) >> 32
// The floor maps the 2^32 values of u onto n_g members, floor(2^32 / n_g) or one more of them each: a member's
// probability differs from 1 / n_g by at most 2^-32, a relative error of at most n_g * 2^-32.  CA_BOOTSTRAP_MAX_GROUP =
// 2^24 keeps that at or below 2^-8 of a member's own weight, far inside the resampling noise of any R the call accepts.
//
// One wave per (group, replicate); w = g * R + r is the wave's index and the high word of idx.  The lanes stride over the
// draws; each draw is a two-step dependent gather (members[goff[g] + k], then that example's row of C int32, 16 bytes at
// a time), and a lane keeps U independent draws in flight (U by the row's width, so that the rows in flight stay within
// 32 registers).  The table is small (16 bytes an example and system) and is re-read by every replicate: it is served
// from L2.  A row can hold 2^21 and a group 2^24 draws, so the accumulators are 64-bit; values are >= 0 by contract and
// are zero-extended.  The wave's 64 partial rows meet in a butterfly and lane 0 stores the row.  No LDS, no barrier, no
// atomics; integer sums do not depend on their order, so any decomposition gives the same bits.
#include "common.h"

typedef __attribute__((ext_vector_type(4))) int i32x4_t;
typedef __attribute__((ext_vector_type(2))) long long i64x2_t;

#define CA_BOOTSTRAP_WG_WAVES 4
#define CA_BOOTSTRAP_MAX_BLOCKS (1 << 20)  // more waves than that stride over the (group, replicate) pairs

// CV = C / 4, the 16-byte pieces of a row
template <int CV>
__global__ __launch_bounds__(CA_BOOTSTRAP_WG_WAVES * CA_WAVE) void bootstrap_sums_kernel(
    const i32x4_t* __restrict__ vals, int32_t N, const int32_t* __restrict__ members, int64_t n_members,
    const int64_t* __restrict__ goff, uint32_t R, uint64_t n_waves, uint64_t seed, int64_t* __restrict__ sums) {
  constexpr int U = CV <= 2 ? 4 : (CV <= 4 ? 2 : 1);
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (uint64_t w = (uint64_t)blockIdx.x * CA_BOOTSTRAP_WG_WAVES + wave; w < n_waves;
       w += (uint64_t)gridDim.x * CA_BOOTSTRAP_WG_WAVES) {
    const uint32_t g = (uint32_t)w / R;
    const int64_t lo = goff[g], hi = goff[g + 1];
    // (wave-uniform) offsets the contract does not allow: the group is marked and nothing is read through them
    const bool served = lo >= 0 && hi > lo && hi <= n_members && hi - lo <= (int64_t)CA_BOOTSTRAP_MAX_GROUP;
    uint64_t acc[4 * CV];
#pragma unroll
    for (int c = 0; c < 4 * CV; ++c) acc[c] = served ? 0ull : ~0ull;
    if (served) {
      const uint32_t n = (uint32_t)(hi - lo);
      const int32_t* __restrict__ mem = members + lo;
      const uint64_t idx_hi = w << 32;
      for (uint32_t j0 = 0; j0 < n; j0 += CA_WAVE * U) {
        int32_t m[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint32_t j = j0 + CA_WAVE * u + lane;
          m[u] = -1;
          if (j < n) m[u] = mem[__umulhi(ca_hash32(seed, idx_hi | j), n)];
        }
        i32x4_t v[U][CV];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const bool in = (uint32_t)m[u] < (uint32_t)N;  // a draw behind the group's end, or a member outside the table
          const i32x4_t* row = vals + (int64_t)(in ? m[u] : 0) * CV;
#pragma unroll
          for (int c = 0; c < CV; ++c) v[u][c] = in ? row[c] : (i32x4_t){0, 0, 0, 0};
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int c = 0; c < CV; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[4 * c + e] += (uint32_t)v[u][c][e];
      }
#pragma unroll
      for (int c = 0; c < 4 * CV; ++c)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[c] += (uint64_t)__shfl_xor((long long)acc[c], o, 64);
    }
    if (lane == 0) {
      i64x2_t* out = (i64x2_t*)(sums + w * (uint64_t)(4 * CV));
#pragma unroll
      for (int c = 0; c < 2 * CV; ++c) out[c] = (i64x2_t){(long long)acc[2 * c], (long long)acc[2 * c + 1]};
    }
  }
}

template <int CV>
static void bootstrap_launch(const int32_t* vals, int32_t N, const int32_t* members, int64_t n_members,
                             const int64_t* goff, uint32_t R, uint64_t n_waves, uint64_t seed, int64_t* sums,
                             hipStream_t stream) {
  uint64_t blocks = (n_waves + CA_BOOTSTRAP_WG_WAVES - 1) / CA_BOOTSTRAP_WG_WAVES;
  if (blocks > CA_BOOTSTRAP_MAX_BLOCKS) blocks = CA_BOOTSTRAP_MAX_BLOCKS;
  hipLaunchKernelGGL(bootstrap_sums_kernel<CV>, dim3((unsigned)blocks), dim3(CA_BOOTSTRAP_WG_WAVES * CA_WAVE), 0, stream,
                     (const i32x4_t*)vals, N, members, n_members, goff, R, n_waves, seed, sums);
}

extern "C" int ca_bootstrap_sums(const int32_t* vals, int32_t N, int32_t C, const int32_t* members, int64_t n_members,
                                 const int64_t* goff, int32_t G, int64_t R, uint64_t seed, int64_t* sums, void* stream) {
  CA_CHECK_ARG(vals && members && goff && sums, "ca_bootstrap_sums: null pointer");
  CA_CHECK_ARG(((uintptr_t)vals & 15) == 0 && ((uintptr_t)sums & 15) == 0,
               "ca_bootstrap_sums: vals and sums must be 16-byte aligned");
  CA_CHECK_ARG(C >= 4 && C <= CA_BOOTSTRAP_MAX_COLUMNS && C % 4 == 0,
               "ca_bootstrap_sums: C = %d is not a multiple of 4 in 4 .. %d (CA_BOOTSTRAP_MAX_COLUMNS)", C,
               CA_BOOTSTRAP_MAX_COLUMNS);
  CA_CHECK_ARG(N >= 1 && n_members >= 1, "ca_bootstrap_sums: N = %d and n_members = %lld must be positive", N,
               (long long)n_members);
  CA_CHECK_ARG(R >= 1, "ca_bootstrap_sums: R = %lld must be at least 1", (long long)R);
  CA_CHECK_ARG(G >= 1, "ca_bootstrap_sums: G = %d must be at least 1", G);
  CA_CHECK_ARG(R < (1ll << 32) && (int64_t)G * R < (1ll << 32),
               "ca_bootstrap_sums: G * R = %d * %lld must stay below 2^32 (the replicate's half of the hash index)", G,
               (long long)R);
  const uint64_t n_waves = (uint64_t)G * (uint64_t)R;
  hipStream_t s = (hipStream_t)stream;
  switch (C / 4) {
    case 1: bootstrap_launch<1>(vals, N, members, n_members, goff, (uint32_t)R, n_waves, seed, sums, s); break;
    case 2: bootstrap_launch<2>(vals, N, members, n_members, goff, (uint32_t)R, n_waves, seed, sums, s); break;
    case 3: bootstrap_launch<3>(vals, N, members, n_members, goff, (uint32_t)R, n_waves, seed, sums, s); break;
    case 4: bootstrap_launch<4>(vals, N, members, n_members, goff, (uint32_t)R, n_waves, seed, sums, s); break;
    case 5: bootstrap_launch<5>(vals, N, members, n_members, goff, (uint32_t)R, n_waves, seed, sums, s); break;
    case 6: bootstrap_launch<6>(vals, N, members, n_members, goff, (uint32_t)R, n_waves, seed, sums, s); break;
    case 7: bootstrap_launch<7>(vals, N, members, n_members, goff, (uint32_t)R, n_waves, seed, sums, s); break;
    default: bootstrap_launch<8>(vals, N, members, n_members, goff, (uint32_t)R, n_waves, seed, sums, s); break;
  }
  CA_CHECK_LAUNCH("ca_bootstrap_sums");
  return CA_OK;
}
