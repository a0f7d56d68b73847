// V-MPO (core/agent/vmpo.py:155-252): everything of one minibatch update between the network's forward and its backward, in ONE launch of
// ONE workgroup (1 <= b <= 1024 rows, one row per thread):
//   top half        adv[idx] -> LDS, the LOWER median (sorted element (b - 1) / 2, torch.median) by rank counting -- float compares only, so
//                   a row is in the top half exactly when torch's `adv > adv.median()` says so (vmpo.py:174), ties at the median fall out
//   psi             exp((adv - max_top) / eta) / sum_top(...)                                   (vmpo.py:177-178)
//   losses          critic = mean (v - (adv + value_old))^2, actor = -sum_top psi logp, eta_loss, alpha_loss (vmpo.py:191-244) and their
//                   gradients with respect to the raw heads, in the layout jh_pponet_backward takes
//   multipliers     one thread: the gradients of eta, alpha_mu, alpha_sigma, torch's single-tensor Adam step on each with the NETWORK's
//                   settings and step count (one optimizer holds them all, vmpo.py:87-91), then the floors (reset_lgr_muls, vmpo.py:271-274)
// The multipliers live in a caller-owned device block of JH_VMPO_BLOCK_FLOATS floats (layout below, include/jorldy_hip.h) that the kernel
// reads and advances itself: minibatch k of a replayed graph sees the multipliers after k - 1 steps.
// Per-row terms are evaluated in double and rounded once (as jh_ppo.hip's continuous head: a row is a handful of elements of a
// latency-bound launch); every sum is a double with a fixed order (shuffle tree, then waves in order): no atomics, same bits every run.
// Departure on purpose: psi and eta_loss are formed around max_top (log-sum-exp), which is the reference's formula wherever the reference's
// float32 exp(adv / eta) is finite, and stays finite where that overflows (adv / eta > ~88).
// Empty top half (b == 1, or no advantage above the median): as the reference -- no actor gradient, eta_loss = log(mean of nothing) = NaN,
// and so is the stepped eta (x < floor ? floor : x keeps a NaN, as torch.max does).
#include "jh_common.h"
#include "jh_mult.h"         // the multiplier block's layout, block_sums, multiplier_step: shared with jh_mpo.hip
#include "jh_policy_head.h"  // the categorical row, the squashed-Gaussian head element, its trust region, alpha_loss_row

namespace {

constexpr int kMaxRows = 1024, kMaxWaves = kMaxRows / 64;
constexpr int kMaxHead = 64;  // action dimensions / logits per row, looped over by the row's thread (jh_pponet: <= 39)

template <bool CONT>
struct VmpoArgs {
  int b, A;
  const float* h0;          // logits | mu_raw       [b][A]
  const float* h1;          // unused | log_std_raw  [b][A]
  const float* value_pred;  // [b]
  const int64_t* idx;       // [b] rows of the rollout-sized arrays, or null (row i)
  const float* action;      // [M] | [M][A]
  const float* adv;         // [M]
  const float* value_old;   // [M]
  const float* h0_old;      // [M][A] raw heads of the pre-pass
  const float* h1_old;      // [M][A] (continuous)
  float* blk;               // the multiplier block
  const float* hyper;       // the network's Adam block (JH_HY_*): lr, betas, eps, step BEFORE this minibatch's step
  float *g0, *g1, *gv;      // d(loss) / d(raw heads), d / d(value_pred)
  float* stats;             // [8] or null
  float* mask;              // [b] or null: 1 where the row is in the top half
};

template <bool CONT>
__global__ void __launch_bounds__(kMaxRows) jh_vmpo_loss_kernel(VmpoArgs<CONT> a) {
  __shared__ __attribute__((aligned(16))) float s_adv[kMaxRows];
  __shared__ double s_red[kMaxWaves][8];
  __shared__ float s_max[kMaxWaves];
  __shared__ float s_med;
  const int i = threadIdx.x, b = a.b, A = a.A;
  const bool on = i < b;
  const float eta = a.blk[VB_VAL + 0], alpha_mu = a.blk[VB_VAL + 1], alpha_sigma = a.blk[VB_VAL + 2];
  const float eps_eta = a.blk[VB_EPS + 0], eps_mu = a.blk[VB_EPS + 1], eps_sigma = a.blk[VB_EPS + 2];

  // ---- adv[idx] -> LDS; the pad up to the block size is NaN: neither below nor equal to anything
  const int64_t r = on ? (a.idx ? a.idx[i] : (int64_t)i) : 0;
  const float adv = on ? a.adv[r] : __builtin_nanf("");
  s_adv[i] = adv;  // blockDim.x = b rounded up to 64 <= kMaxRows
  if (i == 0) s_med = __builtin_nanf("");
  __syncthreads();

  // ---- lower median by rank counting: sorted element k = (b - 1) / 2 is the value with #less <= k < #less + #equal.  Every row holding
  // that value writes it (the same value; +0 and -0 compare equal here and in torch's `>` alike)
  if (on) {
    int less = 0, eq = 0;
    const float4* p = reinterpret_cast<const float4*>(s_adv);
    const int n4 = (int)blockDim.x >> 2;
    for (int j = 0; j < n4; ++j) {  // all lanes read the same 16 bytes: an LDS broadcast
      const float4 q = p[j];
      less += (q.x < adv) + (q.y < adv) + (q.z < adv) + (q.w < adv);
      eq += (q.x == adv) + (q.y == adv) + (q.z == adv) + (q.w == adv);
    }
    const int k = (b - 1) >> 1;
    if (less <= k && k < less + eq) s_med = adv;
  }
  __syncthreads();
  const float med = s_med;
  const bool top = on && adv > med;  // vmpo.py:174, strict
  if (a.mask && on) a.mask[i] = top ? 1.f : 0.f;

  // ---- n_top and max_top
  {
    const float wmx = jh_wave_max(top ? adv : -INFINITY);
    if ((i & 63) == 0) s_max[i >> 6] = wmx;
    double c[1] = {top ? 1.0 : 0.0};
    block_sums<1>(c, s_red);  // its barriers publish s_max too
    const double n_top = c[0];
    float mx = -INFINITY;
    for (int w = 0; w < (((int)blockDim.x + 63) >> 6); ++w) mx = fmaxf(mx, s_max[w]);

    // ---- psi's numerators around max_top, their sum, and sum e (adv - max_top) for eta's gradient
    const double d_eta = (double)eta;
    const double da = top ? (double)adv - (double)mx : 0.0;
    const double e = top ? exp(da / d_eta) : 0.0;
    double s2[2] = {e, e * da};
    block_sums<2>(s2, s_red);
    const double sum_e = s2[0], sum_eda = s2[1];
    const double psi = top ? e / sum_e : 0.0;  // n_top == 0: no row is `top`, sum_e is never divided by

    // ---- per row: critic, log pi(a), the KL terms, head gradients
    double logp = 0.0, kl0 = 0.0, kl1 = 0.0, crit = 0.0;
    if (on) {
      const float ret = adv + a.value_old[r];  // vmpo.py:153: AFTER the standardisation, one float32 add
      const double dv = (double)a.value_pred[i] - (double)ret;
      crit = dv * dv;
      a.gv[i] = (float)(2.0 * dv / (double)b);
      const double inv_b = 1.0 / (double)b;
      if (!CONT) {
        const float* z = a.h0 + (size_t)i * A;
        const float* zo = a.h0_old + (size_t)r * A;
        const double lse = row_lse(z, A), lseo = row_lse(zo, A);
        const int ak = action_index(a.action[r], A);
        logp = (double)z[ak] - lse;
        double s_old = 0.0;
        for (int k = 0; k < A; ++k) {
          const double lpo = (double)zo[k] - lseo, po = exp(lpo);
          kl0 += po * (lpo - ((double)z[k] - lse));  // vmpo.py:237-238
          s_old += po;
        }
        const double c_kl = (double)alpha_mu * inv_b;
        for (int k = 0; k < A; ++k) {
          const double pk = exp((double)z[k] - lse), po = exp((double)zo[k] - lseo);
          a.g0[(size_t)i * A + k] = (float)(-psi * ((k == ak ? 1.0 : 0.0) - pk) + c_kl * (pk * s_old - po));
        }
      } else {
        const double c_mu = (double)alpha_mu * inv_b, c_sg = (double)alpha_sigma * inv_b;
        double kls = 0.0;
        for (int k = 0; k < A; ++k) {
          const GaussElem e = gauss_elem(a.h0[(size_t)i * A + k], a.h1[(size_t)i * A + k]);  // policy_value.py:54
          const GaussTrust tr = gauss_trust(e, gauss_elem(a.h0_old[(size_t)r * A + k], a.h1_old[(size_t)r * A + k]));
          const double dm = gauss_z(a.action[(size_t)r * A + k]) - e.mu;
          logp += gauss_log_prob(dm, e.th, e.var);
          kl0 += tr.kl0;
          kls += tr.kls;
          // d(-psi logp): -psi dm / var to mu, -psi (dm^2 - var) / (var std) to std and so -psi (dm^2 - var) / var to th = log(std)
          const double g_mu = -psi * dm / e.var + gauss_trust_grad_mu(tr, c_mu);
          const double g_th = -psi * ((dm * dm - e.var) / e.var) + gauss_trust_grad_th(tr, c_sg);
          a.g0[(size_t)i * A + k] = gauss_grad_mu_raw(e, g_mu);
          a.g1[(size_t)i * A + k] = gauss_grad_log_std_raw(e, g_th);
        }
        gauss_trust_finish(kl0, kl1, kls, A);  // vmpo.py:220-229
      }
    }
    const double al = on ? alpha_loss_row(alpha_mu, eps_mu, kl0) + (CONT ? alpha_loss_row(alpha_sigma, eps_sigma, kl1) : 0.0) : 0.0;
    double s5[5] = {psi * logp, crit, kl0, kl1, al};
    block_sums<5>(s5, s_red);
    if (i != 0) return;

    // ---- one thread: the scalar losses, the multipliers' gradients and steps, the statistics row
    const double lme = log(sum_e / n_top);  // log(mean_top exp((adv - max_top) / eta)); n_top == 0: log(0 / 0) = NaN
    const double eta_loss = d_eta * (double)eps_eta + d_eta * ((double)mx / d_eta + lme);  // vmpo.py:194-196
    const float g_eta = (float)((double)eps_eta + lme - (sum_eda / sum_e) / d_eta);        // = eps + log mean exp(adv / eta) - sum psi adv / eta
    const float g_mu = (float)((double)eps_mu - s5[2] / (double)b);
    const float g_sg = (float)((double)eps_sigma - s5[3] / (double)b);
    const float t = a.hyper[JH_HY_STEP] + 1.f;  // the step the network's Adam takes for this minibatch (jh_gradnorm_kernel advances it later)
    const float eta_n = multiplier_step(a.blk, 0, g_eta, a.hyper, t);
    const float mu_n = multiplier_step(a.blk, 1, g_mu, a.hyper, t);
    const float sg_n = CONT ? multiplier_step(a.blk, 2, g_sg, a.hyper, t) : alpha_sigma;  // discrete: no gradient, torch's Adam skips it
    if (a.stats) {
      a.stats[0] = (float)(-s5[0]);
      a.stats[1] = (float)(s5[1] / (double)b);
      a.stats[2] = (float)eta_loss;
      a.stats[3] = (float)(s5[4] / (double)b);
      a.stats[4] = eta_n;
      a.stats[5] = mu_n;
      a.stats[6] = sg_n;
      __threadfence_system();  // payload before the arrival mark (mapped host memory, jh_host_wait_marks)
      a.stats[7] = 0.f;
    }
  }
}

template <bool CONT>
static int vmpo_launch(const VmpoArgs<CONT>& a, hipStream_t st) {
  const int threads = ((a.b + 63) / 64) * 64;
  JH_LAUNCH(jh_vmpo_loss_kernel<CONT>, dim3(1), dim3(threads), 0, st, a);
  JH_LAUNCH_CHECK();
  return JH_OK;
}

}  // namespace

JH_EXPORT int jh_vmpo_loss_discrete(jh_ctx* ctx, int32_t B, int32_t A, const float* d_logits, const float* d_value_pred, const int64_t* d_idx,
                                    const float* d_action, const float* d_adv, const float* d_value_old, const float* d_logits_old, float* d_block,
                                    const float* d_hyper, float* d_grad_logits, float* d_grad_value, float* d_stats, float* d_mask, jh_stream stream) {
  JH_ARG(ctx && d_logits && d_value_pred && d_action && d_adv && d_value_old && d_logits_old && d_block && d_hyper && d_grad_logits && d_grad_value);
  JH_ARG(B >= 1 && B <= kMaxRows && A >= 1 && A <= kMaxHead);
  JH_ARG(((uintptr_t)d_hyper & 7) == 0);
  VmpoArgs<false> a{};
  a.b = B; a.A = A; a.h0 = d_logits; a.value_pred = d_value_pred; a.idx = d_idx; a.action = d_action; a.adv = d_adv; a.value_old = d_value_old;
  a.h0_old = d_logits_old; a.blk = d_block; a.hyper = d_hyper; a.g0 = d_grad_logits; a.gv = d_grad_value; a.stats = d_stats; a.mask = d_mask;
  return vmpo_launch<false>(a, jh_s(stream));
}

JH_EXPORT int jh_vmpo_loss_continuous(jh_ctx* ctx, int32_t B, int32_t A, const float* d_mu_raw, const float* d_log_std_raw, const float* d_value_pred,
                                      const int64_t* d_idx, const float* d_action, const float* d_adv, const float* d_value_old, const float* d_mu_raw_old,
                                      const float* d_log_std_raw_old, float* d_block, const float* d_hyper, float* d_grad_mu_raw, float* d_grad_log_std_raw,
                                      float* d_grad_value, float* d_stats, float* d_mask, jh_stream stream) {
  JH_ARG(ctx && d_mu_raw && d_log_std_raw && d_value_pred && d_action && d_adv && d_value_old && d_mu_raw_old && d_log_std_raw_old && d_block && d_hyper);
  JH_ARG(d_grad_mu_raw && d_grad_log_std_raw && d_grad_value);
  JH_ARG(B >= 1 && B <= kMaxRows && A >= 1 && A <= kMaxHead);
  JH_ARG(((uintptr_t)d_hyper & 7) == 0);
  VmpoArgs<true> a{};
  a.b = B; a.A = A; a.h0 = d_mu_raw; a.h1 = d_log_std_raw; a.value_pred = d_value_pred; a.idx = d_idx; a.action = d_action; a.adv = d_adv;
  a.value_old = d_value_old; a.h0_old = d_mu_raw_old; a.h1_old = d_log_std_raw_old; a.blk = d_block; a.hyper = d_hyper; a.g0 = d_grad_mu_raw;
  a.g1 = d_grad_log_std_raw; a.gv = d_grad_value; a.stats = d_stats; a.mask = d_mask;
  return vmpo_launch<true>(a, jh_s(stream));
}
