// The NoisyNet dueling tail's elementwise kernels (network/utils.py:55-107, network/rainbow.py:76-93), shared by the networks that end in
// the four noisy layers a1 | v1 -> a2, v2 and the dueling combine: jh_rbnet (Rainbow, K atoms) and jh_iqnnet's noisy tail (Rainbow-IQN,
// K = 1 over rows x N sampled rows).  Effective weights W = mu + sig * eps for up to three (parameter set, draw) pairs in one launch,
// d(sig) = d(mu) * eps, the combine and its backward.  The GEMMs between them belong to the including file.
#pragma once
#include "jh_netcore.h"

namespace {

// ---------------------------------------------------------------------------------- noisy layers
__device__ __forceinline__ float noise_f(float e) { return copysignf(sqrtf(fabsf(e)), e); }  // utils.py:66-67 (sign(0) = 0 either way)

// Layout of one noise set (standard normal draws, reference draw order utils.py:58-60 per layer a1, v1, a2, v2):
//   [ei_a1 H][ej_a1 H][ei_v1 H][ej_v1 H][ei_a2 H][ej_a2 NA][ei_v2 H][ej_v2 K]
struct NoisyDims {
  int H, NA, K;
  int64_t o_av1, o_bav1, o_a2, o_ba2, o_v2, o_bv2, set_stride;  // inside one effective-weight set
  int64_t p_mu_av1, p_sig_av1, p_mub_av1, p_sigb_av1, p_mu_a2, p_sig_a2, p_mub_a2, p_sigb_a2, p_mu_v2, p_sig_v2, p_mub_v2, p_sigb_v2;
  int64_t noise_len;
  int independent;  // utils.py:73-76: a full eps_w [in][out] + eps_b [out] per layer instead of the outer product
};

// factor pair (f_j of the output unit, f_i of the input unit) for flat index i of the weight part
__device__ __forceinline__ void noisy_locate(const NoisyDims& d, int64_t i, const float* e, int64_t* p_mu, int64_t* p_sig, int64_t* w_off, float* eps) {
  const int H = d.H;
  const int64_t n_av1 = (int64_t)2 * H * H, n_a2 = (int64_t)d.NA * H, n_v2 = (int64_t)d.K * H;
  int64_t n, k;
  const float *ei, *ej;
  // independent noise, one set: [eps_w a1 H x H (in, out)][eps_b a1 H][eps_w v1][eps_b v1][eps_w a2 H x NA][eps_b a2 NA][eps_w v2 H x K][eps_b v2 K]
  const int64_t hh = (int64_t)H * H, i_a1 = 0, i_v1 = hh + H, i_a2 = 2 * (hh + H), i_v2 = i_a2 + (int64_t)H * d.NA + d.NA;
  int64_t ind = 0;  // index of this weight's own draw (independent noise)
  if (i < n_av1) {
    n = i / H; k = i - n * H;
    *p_mu = d.p_mu_av1 + i; *p_sig = d.p_sig_av1 + i; *w_off = d.o_av1 + i;
    if (n < H) { ei = e; ej = e + H; ind = i_a1 + k * H + n; } else { ei = e + 2 * H; ej = e + 3 * H; n -= H; ind = i_v1 + k * H + n; }
  } else if (i < n_av1 + n_a2) {
    i -= n_av1;
    n = i / H; k = i - n * H;
    *p_mu = d.p_mu_a2 + i; *p_sig = d.p_sig_a2 + i; *w_off = d.o_a2 + i;
    ei = e + 4 * H; ej = e + 5 * H;
    ind = i_a2 + k * d.NA + n;
  } else if (i < n_av1 + n_a2 + n_v2) {
    i -= n_av1 + n_a2;
    n = i / H; k = i - n * H;
    *p_mu = d.p_mu_v2 + i; *p_sig = d.p_sig_v2 + i; *w_off = d.o_v2 + i;
    ei = e + 5 * H + d.NA; ej = e + 6 * H + d.NA;
    ind = i_v2 + k * d.K + n;
  } else {  // biases: eps_b = f_j (utils.py:69) / its own draw (utils.py:76)
    i -= n_av1 + n_a2 + n_v2;
    if (i < 2 * H) {
      *p_mu = d.p_mub_av1 + i; *p_sig = d.p_sigb_av1 + i; *w_off = d.o_bav1 + i;
      if (d.independent) *eps = e ? (i < H ? e[i_a1 + hh + i] : e[i_v1 + hh + (i - H)]) : 0.f;
      else *eps = e ? noise_f(i < H ? e[H + i] : e[3 * H + (i - H)]) : 0.f;
    } else if (i < 2 * H + d.NA) {
      i -= 2 * H;
      *p_mu = d.p_mub_a2 + i; *p_sig = d.p_sigb_a2 + i; *w_off = d.o_ba2 + i;
      if (d.independent) *eps = e ? e[i_a2 + (int64_t)H * d.NA + i] : 0.f;
      else *eps = e ? noise_f(e[5 * H + i]) : 0.f;
    } else {
      i -= 2 * H + d.NA;
      *p_mu = d.p_mub_v2 + i; *p_sig = d.p_sigb_v2 + i; *w_off = d.o_bv2 + i;
      if (d.independent) *eps = e ? e[i_v2 + (int64_t)H * d.K + i] : 0.f;
      else *eps = e ? noise_f(e[6 * H + d.NA + i]) : 0.f;
    }
    return;
  }
  if (d.independent) *eps = e ? e[ind] : 0.f;
  else *eps = e ? noise_f(ei[k]) * noise_f(ej[n]) : 0.f;  // torch.outer(f_i, f_j)
}

struct NoiseSets {
  const float* params[3];
  const float* noise[3];  // null: evaluation mode, W = mu (rainbow.py network: is_train False)
  float* weff[3];
  int n_sets;
};

// W_eff = mu + sig * eps for up to three (parameter set, noise draw) pairs in one launch
__global__ void __launch_bounds__(256) jh_rb_noise_kernel(NoisyDims d, NoiseSets s, int64_t n_total) {
  const int set = blockIdx.y;
  const float* P = s.params[set];
  const float* e = s.noise[set];
  float* W = s.weff[set];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_total; i += (int64_t)gridDim.x * 256) {
    int64_t pm, ps, wo;
    float eps;
    noisy_locate(d, i, e, &pm, &ps, &wo, &eps);
    W[wo] = e ? P[pm] + P[ps] * eps : P[pm];
  }
}

// d(sig) = d(W_eff) * eps; d(mu) = d(W_eff) was written in place by the weight-gradient GEMMs
__global__ void __launch_bounds__(256) jh_rb_noisy_grad_kernel(NoisyDims d, const float* __restrict__ e, float* __restrict__ G, int64_t n_total) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_total; i += (int64_t)gridDim.x * 256) {
    int64_t pm, ps, wo;
    float eps;
    noisy_locate(d, i, e, &pm, &ps, &wo, &eps);
    G[ps] = G[pm] * eps;
  }
}

// ---------------------------------------------------------------------------------- dueling combine
struct DuelSets {
  const float* xa[3];
  const float* xv[3];
  float* out[3];
};
// logits[b][a][k] = xa[b][a][k] - mean_a xa[b][.][k] + xv[b][k]   (network/rainbow.py:88-93)
__global__ void __launch_bounds__(256) jh_rb_duel_fwd_kernel(DuelSets s, int B, int A, int K, int ld_a, int ld_v) {
  const int set = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * K) return;
  const int b = i / K, k = i - b * K;
  const float* xa = s.xa[set] + (size_t)b * ld_a;
  float sum = 0.f;
  for (int a = 0; a < A; ++a) sum += xa[a * K + k];
  const float mean = sum / (float)A;
  const float v = s.xv[set][(size_t)b * ld_v + k];
  float* o = s.out[set] + (size_t)b * A * K;
  for (int a = 0; a < A; ++a) o[a * K + k] = (xa[a * K + k] - mean) + v;
}
__global__ void __launch_bounds__(256) jh_rb_duel_bwd_kernel(const float* __restrict__ g, int B, int A, int K, float* __restrict__ dxa, int ld_a,
                                                             float* __restrict__ dxv, int ld_v) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * K) return;
  const int b = i / K, k = i - b * K;
  const float* gb = g + (size_t)b * A * K;
  float sum = 0.f;
  for (int a = 0; a < A; ++a) sum += gb[a * K + k];
  dxv[(size_t)b * ld_v + k] = sum;
  const float mean = sum / (float)A;
  for (int a = 0; a < A; ++a) dxa[(size_t)b * ld_a + a * K + k] = gb[a * K + k] - mean;
}

}  // namespace
