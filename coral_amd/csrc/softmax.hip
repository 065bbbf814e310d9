// Softmax over vocabulary rows: the cross-entropy of the Whisper LM loss.
// (The attention softmax lives inside the fused attention kernels, attn_fwd.hip / attn_bwd.hip / attn_decode.hip; the
// picks of generation - masked argmax, timestamp rules, the scored pick - are in pick.hip.)
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
