// The Lagrange multipliers of the MPO family (V-MPO: jh_vmpo.hip, MPO: jh_mpo.hip): the layout of their caller-owned device block
// (JH_VMPO_BLOCK_FLOATS floats, include/jorldy_hip.h), torch's single-tensor Adam step on one of them followed by its floor, and the
// fixed-order workgroup sums both loss kernels form their means with.  ONE copy: the two kernels step the multipliers with the same bits.
#pragma once
#include "jh_common.h"

namespace {

enum {
  VB_VAL = 0,     // eta, alpha_mu, alpha_sigma
  VB_M = 3,       // exp_avg of the three
  VB_V = 6,       // exp_avg_sq
  VB_FLOOR = 9,   // min_eta, min_alpha_mu, min_alpha_sigma
  VB_EPS = 12,    // eps_eta, eps_alpha_mu, eps_alpha_sigma
  VB_STATE = 15,  // 1: this multiplier has taken an Adam step (has optimizer state).  alpha_sigma of a discrete policy never does.
  VB_GRAD = 18,   // the gradients of the last step
  VB_FLOATS = 24
};
static_assert(VB_FLOATS == JH_VMPO_BLOCK_FLOATS, "the multiplier block of include/jorldy_hip.h");

// N sums over the workgroup: shuffle tree inside a wave, then the waves' partials in wave order.  Every thread returns with the totals.
template <int N>
__device__ __forceinline__ void block_sums(double (&v)[N], double (*red)[8]) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = jh_wave_sum(v[k]);
  __syncthreads();  // `red` may still be read from the previous use
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) red[wid][k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) {
    double r = 0.0;
    for (int w = 0; w < nw; ++w) r += red[w][k];
    v[k] = r;
  }
}

// torch.optim.Adam (single tensor) on one float32 scalar, then max(x, floor) (jh_sac_actor_seed_kernel's arithmetic: lerp of exp_avg, addcmul
// of exp_avg_sq, bias corrections and step size in double, rounded once)
__device__ __forceinline__ float multiplier_step(float* blk, int j, float grad, const float* hyper, float t) {
  const double b1 = *reinterpret_cast<const double*>(hyper + JH_HY_B1D), b2 = *reinterpret_cast<const double*>(hyper + JH_HY_B2D);
  const float m = blk[VB_M + j] + (grad - blk[VB_M + j]) * (float)(1.0 - b1);
  const float v = blk[VB_V + j] * (float)b2 + (float)(1.0 - b2) * grad * grad;
  const float step_size = (float)((double)hyper[JH_HY_LR] / (1.0 - pow(b1, (double)t)));
  const float denom = sqrtf(v) / (float)sqrt(1.0 - pow(b2, (double)t)) + hyper[JH_HY_EPS];
  float x = blk[VB_VAL + j] - step_size * (m / denom);
  const float floor_j = blk[VB_FLOOR + j];
  x = x < floor_j ? floor_j : x;  // a NaN stays a NaN (torch.max), which fmaxf would turn into the floor
  blk[VB_VAL + j] = x;
  blk[VB_M + j] = m;
  blk[VB_V + j] = v;
  blk[VB_STATE + j] = 1.f;
  blk[VB_GRAD + j] = grad;
  return x;
}

}  // namespace
