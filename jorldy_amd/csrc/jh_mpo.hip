// MPO, discrete policy (core/agent/mpo.py:312-386): everything of one learn() between the six network forwards and the two backwards, in
// ONE launch of ONE workgroup (R = B * T <= 1024 rows, row r = b * T + t, one row per thread):
//   policies     log-softmax of the three logit rows: pi = online(s), pi' = online(s'), pi_old = target(s)       (mpo.py:312-313, 321)
//   importance   c = min(pi[a] / (prob_b + 1e-6), 1): the ONLINE policy at the taken action, as the reference     (mpo.py:324-330)
//   target       Qret = reward + gamma sum_a pi' qt_next (1 - done) -> LDS                                        (mpo.py:332-339)
//   Retrace      one lane per trajectory walks t = T - 2 .. 0 out of LDS:
//                Qret[b, t] += gamma c[b, t + 1] (Qret[b, t + 1] - qt[b, t + 1, a]) (1 - done[b, t])              (mpo.py:347-355)
//   losses       critic = mean (q[a] - Qret)^2; V = sum pi_old qt, At = qt - V, w = softmax(At / eta) (a constant); actor = -mean sum_a w log pi;
//                eta_loss = eta eps_eta + eta mean log sum_a pi_old exp(At / eta); KLD = sum pi_old (log pi_old - log pi),
//                alpha_loss = mean[alpha_mu (eps_alpha_mu - KLD) + alpha_mu KLD]                                   (mpo.py:360-384)
//                and their gradients with respect to the actor's logits of s and the critic's q of s
//   multipliers  one thread: the gradients of eta and alpha_mu, torch's single-tensor Adam step on each with the ACTOR's settings and step
//                count (the actor's optimizer holds them, mpo.py:142-146), then the floors (reset_lgr_muls, mpo.py:416-419).  alpha_sigma has no
//                gradient for a discrete policy: torch's Adam skips it, and so does the kernel (as jh_vmpo_loss_discrete).
// The block, its step and the fixed-order sums are jh_mult.h's, shared with jh_vmpo.hip.  Per-row terms are evaluated in double and rounded
// once; every mean is a double sum with a fixed order (shuffle tree, then waves in order), the extrema are exact: no atomics, same bits
// every run.
// Departures on purpose (as V-MPO's): log pi is a log-softmax of the logits where the reference takes log(softmax), finite where float32 pi
// underflows; the log-sum of eta_loss is formed around the row's largest At / eta, which is the reference's formula wherever its float32
// exp(At / eta) is finite, and stays finite where that overflows.
#include "jh_common.h"
#include "jh_mult.h"

namespace {

constexpr int kMaxRows = 1024, kMaxWaves = kMaxRows / 64;
constexpr int kMaxActions = 64;  // logits per row, looped over by the row's thread (the q-network's widest config.mpo head is 18)

struct MpoArgs {
  int R, T, A, retrace;
  const float *la, *la_next, *la_old;  // [R][A]
  const float *q, *qt, *qt_next;       // [R][A]
  const float *action, *reward, *done, *prob_b;  // [R]
  float* blk;          // the multiplier block
  const float* hyper;  // the ACTOR's Adam block (JH_HY_*): lr, betas, eps, step BEFORE this learn's step
  float gamma;
  float *g_la, *g_q;  // [R][A]
  float* stats;       // [11] or null
};

// log-softmax pieces of one row: -> the row's log-sum-exp
__device__ __forceinline__ double row_lse(const float* z, int A) {
  float zm = z[0];
  for (int k = 1; k < A; ++k) zm = fmaxf(zm, z[k]);
  double se = 0.0;
  for (int k = 0; k < A; ++k) se += exp((double)z[k] - (double)zm);
  return (double)zm + log(se);
}

__global__ void __launch_bounds__(kMaxRows) jh_mpo_loss_kernel(MpoArgs a) {
  __shared__ double s_qret[kMaxRows];
  __shared__ float s_c[kMaxRows], s_qta[kMaxRows], s_done[kMaxRows];
  __shared__ double s_red[kMaxWaves][8];
  __shared__ float s_ext[kMaxWaves][4];
  const int i = threadIdx.x, R = a.R, T = a.T, A = a.A;
  const bool on = i < R;
  const float eta = a.blk[VB_VAL + 0], alpha_mu = a.blk[VB_VAL + 1], alpha_sigma = a.blk[VB_VAL + 2];
  const float eps_eta = a.blk[VB_EPS + 0], eps_mu = a.blk[VB_EPS + 1];
  const size_t o = (size_t)i * A;  // only dereferenced when `on`

  // ---- per row: the policies' log-sums, c, the one-step target
  double lse = 0.0, lse_old = 0.0;
  int ak = 0;
  if (on) {
    lse = row_lse(a.la + o, A);
    lse_old = row_lse(a.la_old + o, A);
    const double lse_next = row_lse(a.la_next + o, A);
    ak = (int)a.action[i];
    ak = ak < 0 ? 0 : (ak >= A ? A - 1 : ak);
    const double pa = exp((double)a.la[o + ak] - lse);
    const double ratio = pa / ((double)a.prob_b[i] + 1e-6);
    double ev = 0.0;
    for (int k = 0; k < A; ++k) ev += exp((double)a.la_next[o + k] - lse_next) * (double)a.qt_next[o + k];
    const float dn = a.done[i];
    s_qret[i] = (double)a.reward[i] + (double)a.gamma * ev * (1.0 - (double)dn);
    s_c[i] = (float)(ratio < 1.0 ? ratio : 1.0);  // a NaN ratio stays out of the `<` and gives 1; torch.clip would keep it: the inputs are finite
    s_qta[i] = a.qt[o + ak];
    s_done[i] = dn;
  }
  __syncthreads();

  // ---- Retrace: one lane per trajectory, T - 1 dependent steps out of LDS (i < R / T: every index below stays under R)
  if (a.retrace && T > 1 && i < R / T) {
    const int base = i * T;
    double nxt = s_qret[base + T - 1];
    for (int t = T - 2; t >= 0; --t) {
      const double cur = s_qret[base + t] + (double)a.gamma * (double)s_c[base + t + 1] * (nxt - (double)s_qta[base + t + 1]) * (1.0 - (double)s_done[base + t]);
      s_qret[base + t] = cur;
      nxt = cur;
    }
  }
  __syncthreads();

  // ---- per row: critic, advantage, E-step weights, actor, temperature and trust-region terms, head gradients
  double crit = 0.0, act = 0.0, Lr = 0.0, uAt = 0.0, kld = 0.0;
  float q_lo = INFINITY, q_hi = -INFINITY, at_lo = INFINITY, at_hi = -INFINITY;
  if (on) {
    const double inv_R = 1.0 / (double)R, d_eta = (double)eta;
    const double dq = (double)a.q[o + ak] - s_qret[i];
    crit = dq * dq;
    double V = 0.0;
    for (int k = 0; k < A; ++k) V += exp((double)a.la_old[o + k] - lse_old) * (double)a.qt[o + k];
    double xm = -INFINITY;
    for (int k = 0; k < A; ++k) xm = fmax(xm, ((double)a.qt[o + k] - V) / d_eta);
    double sw = 0.0, su = 0.0;
    for (int k = 0; k < A; ++k) {
      const double e = exp(((double)a.qt[o + k] - V) / d_eta - xm);
      sw += e;
      su += exp((double)a.la_old[o + k] - lse_old) * e;
    }
    Lr = xm + log(su);
    for (int k = 0; k < A; ++k) {
      const float qk = a.q[o + k];
      const double At = (double)a.qt[o + k] - V;
      const double e = exp(At / d_eta - xm);
      const double lp = (double)a.la[o + k] - lse, lpo = (double)a.la_old[o + k] - lse_old;
      const double pk = exp(lp), po = exp(lpo), w = e / sw;
      act += w * lp;
      uAt += (po * e / su) * At;
      kld += po * (lpo - lp);
      a.g_la[o + k] = (float)(((pk - w) + (double)alpha_mu * (pk - po)) * inv_R);
      a.g_q[o + k] = k == ak ? (float)(2.0 * dq * inv_R) : 0.f;
      q_lo = fminf(q_lo, qk); q_hi = fmaxf(q_hi, qk);
      const float Atf = (float)At;
      at_lo = fminf(at_lo, Atf); at_hi = fmaxf(at_hi, Atf);
    }
  }
  const double al = on ? ((double)alpha_mu * ((double)eps_mu - kld) + (double)alpha_mu * kld) : 0.0;  // mpo.py:381-384 as written
  q_lo = jh_wave_min(q_lo); q_hi = jh_wave_max(q_hi); at_lo = jh_wave_min(at_lo); at_hi = jh_wave_max(at_hi);
  if ((i & 63) == 0) {
    s_ext[i >> 6][0] = q_lo; s_ext[i >> 6][1] = q_hi; s_ext[i >> 6][2] = at_lo; s_ext[i >> 6][3] = at_hi;
  }
  double s6[6] = {crit, act, Lr, uAt, kld, al};
  block_sums<6>(s6, s_red);  // its barriers publish s_ext too
  if (i != 0) return;

  // ---- one thread: the scalar losses, the multipliers' gradients and steps, the statistics
  const double n = (double)R, d_eta = (double)eta;
  const double mean_L = s6[2] / n;
  const double eta_loss = d_eta * (double)eps_eta + d_eta * mean_L;                    // mpo.py:370-372
  const float g_eta = (float)((double)eps_eta + mean_L - (s6[3] / n) / d_eta);
  const float g_mu = (float)((double)eps_mu - s6[4] / n);
  const float t = a.hyper[JH_HY_STEP] + 1.f;  // the step the actor's Adam takes for this learn (its optimizer pass advances it later)
  const float eta_n = multiplier_step(a.blk, 0, g_eta, a.hyper, t);
  const float mu_n = multiplier_step(a.blk, 1, g_mu, a.hyper, t);
  if (a.stats) {
    const int nw = ((int)blockDim.x + 63) >> 6;
    for (int w = 1; w < nw; ++w) {
      q_lo = fminf(q_lo, s_ext[w][0]); q_hi = fmaxf(q_hi, s_ext[w][1]); at_lo = fminf(at_lo, s_ext[w][2]); at_hi = fmaxf(at_hi, s_ext[w][3]);
    }
    a.stats[0] = (float)(-s6[1] / n);
    a.stats[1] = (float)(s6[0] / n);
    a.stats[2] = (float)eta_loss;
    a.stats[3] = (float)(s6[5] / n);
    a.stats[4] = eta_n;
    a.stats[5] = mu_n;
    a.stats[6] = alpha_sigma;
    a.stats[7] = q_lo;
    a.stats[8] = q_hi;
    a.stats[9] = at_lo;
    a.stats[10] = at_hi;
  }
}

}  // namespace

JH_EXPORT int jh_mpo_loss_discrete(jh_ctx* ctx, int32_t R, int32_t T, int32_t A, const float* d_la, const float* d_la_next, const float* d_la_old,
                                   const float* d_q, const float* d_qt, const float* d_qt_next, const float* d_action, const float* d_reward,
                                   const float* d_done, const float* d_prob_b, float* d_block, const float* d_hyper, float gamma, int32_t retrace,
                                   float* d_grad_la, float* d_grad_q, float* d_stats, jh_stream stream) {
  JH_ARG(ctx && d_la && d_la_next && d_la_old && d_q && d_qt && d_qt_next && d_action && d_reward && d_done && d_prob_b && d_block && d_hyper);
  JH_ARG(d_grad_la && d_grad_q);
  JH_ARG(R >= 1 && R <= kMaxRows && T >= 1 && R % T == 0 && A >= 2 && A <= kMaxActions);
  JH_ARG(retrace == 0 || retrace == 1);
  JH_ARG(((uintptr_t)d_hyper & 7) == 0);
  MpoArgs a{};
  a.R = R; a.T = T; a.A = A; a.retrace = retrace; a.la = d_la; a.la_next = d_la_next; a.la_old = d_la_old; a.q = d_q; a.qt = d_qt; a.qt_next = d_qt_next;
  a.action = d_action; a.reward = d_reward; a.done = d_done; a.prob_b = d_prob_b; a.blk = d_block; a.hyper = d_hyper; a.gamma = gamma;
  a.g_la = d_grad_la; a.g_q = d_grad_q; a.stats = d_stats;
  const int threads = ((R + 63) / 64) * 64;
  JH_LAUNCH(jh_mpo_loss_kernel, dim3(1), dim3(threads), 0, jh_s(stream), a);
  JH_LAUNCH_CHECK();
  return JH_OK;
}
