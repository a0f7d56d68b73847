// The per-row policy mathematics of the policy-loss kernels (V-MPO: jh_vmpo.hip, MPO: jh_mpo.hip, REINFORCE: jh_reinforce.hip), in double
// and rounded once by the caller: the categorical row, the squashed-Gaussian head element (network/policy.py:53-55) and its trust region.
// ONE copy: the library is built with -ffp-contract=off, so the same expression tree inlined from here gives every kernel the same bits.
#pragma once
#include "jh_common.h"

namespace {

// ---- categorical: log-softmax pieces of one row -> the row's log-sum-exp
__device__ __forceinline__ double row_lse(const float* z, int A) {
  float zm = z[0];
  for (int k = 1; k < A; ++k) zm = fmaxf(zm, z[k]);
  double se = 0.0;
  for (int k = 0; k < A; ++k) se += exp((double)z[k] - (double)zm);
  return (double)zm + log(se);
}

// the stored action (a float column) as a logit index, kept inside the row
__device__ __forceinline__ int action_index(float action, int A) {
  const int ak = (int)action;
  return ak < 0 ? 0 : (ak >= A ? A - 1 : ak);
}

// ---- squashed Gaussian, one action dimension: mu = clamp(mu_raw, -5, 5), log std = th = tanh(log_std_raw), var = std^2 = exp(2 th)
constexpr float kAtanhLo = -0.99999988f, kAtanhHi = 0.99999988f;  // (float)(1 - 1e-7): the reference clamps the float32 action tensor
constexpr double kHalfLog2Pi = 0.91893853320467274178;

struct GaussElem {
  double mu, th, var;
  bool inside;  // mu_raw within the clamp, bounds included: torch.clamp passes the gradient on its bounds
};
__device__ __forceinline__ double gauss_mu(float mu_raw) { return fmin(fmax((double)mu_raw, -5.0), 5.0); }
__device__ __forceinline__ GaussElem gauss_elem(float mu_raw, float log_std_raw) {
  const double th = tanh((double)log_std_raw);
  return GaussElem{gauss_mu(mu_raw), th, exp(2.0 * th), mu_raw >= -5.f && mu_raw <= 5.f};
}
// the pre-tanh value of a stored action
__device__ __forceinline__ double gauss_z(float action) { return atanh((double)fminf(fmaxf(action, kAtanhLo), kAtanhHi)); }
// Normal.log_prob at distance dm = z - mu, log(std) = th; _sq takes dm^2, or its mean under weights that sum to 1
__device__ __forceinline__ double gauss_log_prob_sq(double sq, double th, double var) { return -sq / (2.0 * var) - th - kHalfLog2Pi; }
__device__ __forceinline__ double gauss_log_prob(double dm, double th, double var) { return gauss_log_prob_sq(dm * dm, th, var); }
// d/d(mu) -> d/d(mu_raw) through the clamp, d/d(th) -> d/d(log_std_raw) through tanh
__device__ __forceinline__ float gauss_grad_mu_raw(const GaussElem& e, double g_mu) { return e.inside ? (float)g_mu : 0.f; }
__device__ __forceinline__ float gauss_grad_log_std_raw(const GaussElem& e, double g_th) { return (float)(g_th * (1.0 - e.th * e.th)); }

// ---- Gaussian trust region, one dimension of KLD_mu = 1/2 sum_A (mu - mu_old)^2 std_old^2 (times the OLD variance, as vmpo.py:210-213 and
// mpo.py:289-290 write it) and KLD_sigma = 1/2 (sum_A std^2 / std_old^2 - A + log(prod ss / prod ss_old)), ss = 1 / std^2 = exp(-2 th): the
// log of the product ratio is the sum of the logs, 2 sum_A (th_old - th)
struct GaussTrust { double d, var_o, ratio, kl0, kls; };  // kl0, kls: this dimension's terms of the two sums
__device__ __forceinline__ GaussTrust gauss_trust(const GaussElem& e, const GaussElem& old) {
  const double d = e.mu - old.mu, ratio = e.var / old.var;
  return GaussTrust{d, old.var, ratio, d * d * old.var, ratio + 2.0 * (old.th - e.th)};
}
// d(c_mu KLD_mu) / d(mu) and d(c_sg KLD_sigma) / d(th) of this dimension
__device__ __forceinline__ double gauss_trust_grad_mu(const GaussTrust& t, double c_mu) { return c_mu * t.d * t.var_o; }
__device__ __forceinline__ double gauss_trust_grad_th(const GaussTrust& t, double c_sg) { return c_sg * (t.ratio - 1.0); }
// the sums over the A dimensions -> KLD_mu (in place), KLD_sigma
__device__ __forceinline__ void gauss_trust_finish(double& kl0, double& kl1, double kls, int A) {
  kl0 *= 0.5;
  kl1 = 0.5 * (kls - (double)A);
}

// a row's alpha_loss as the agents write it (vmpo.py:214-217, mpo.py:291-309, 381-384): alpha (eps - KL) + alpha KL
__device__ __forceinline__ double alpha_loss_row(float alpha, float eps, double kl) { return (double)alpha * ((double)eps - kl) + (double)alpha * kl; }

}  // namespace
