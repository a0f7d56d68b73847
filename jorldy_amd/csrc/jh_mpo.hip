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
#include "jh_policy_head.h"  // the categorical row, the squashed-Gaussian head element, its trust region, alpha_loss_row

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

// ---- shared by the two loss kernels.  The multipliers and their thresholds as the launch finds them:
struct Mult { float eta, alpha_mu, alpha_sigma, eps_eta, eps_mu, eps_sigma; };
__device__ __forceinline__ Mult mult_load(const float* b) { return Mult{b[VB_VAL], b[VB_VAL + 1], b[VB_VAL + 2], b[VB_EPS], b[VB_EPS + 1], b[VB_EPS + 2]}; }

// Retrace (mpo.py:347-355, 245-253): one lane per trajectory, T - 1 dependent steps out of LDS (i < R / T: every index below stays under R).
// The caller's barriers stand before and after it.
__device__ __forceinline__ void retrace_scan(double* s_qret, const float* s_c, const float* s_qta, const float* s_done, int retrace, int R, int T, float gamma) {
  const int i = threadIdx.x;
  if (retrace && T > 1 && i < R / T) {
    const int base = i * T;
    double nxt = s_qret[base + T - 1];
    for (int t = T - 2; t >= 0; --t) {
      const double cur = s_qret[base + t] + (double)gamma * (double)s_c[base + t + 1] * (nxt - (double)s_qta[base + t + 1]) * (1.0 - (double)s_done[base + t]);
      s_qret[base + t] = cur;
      nxt = cur;
    }
  }
}

// the exact extrema of q and At: a row's own, then its wave's (published through s_ext), then thread 0's fold over the waves
struct Extrema { float q_lo = INFINITY, q_hi = -INFINITY, at_lo = INFINITY, at_hi = -INFINITY; };
__device__ __forceinline__ void extrema_publish(Extrema& x, float (*s_ext)[4]) {
  const int i = threadIdx.x;
  x.q_lo = jh_wave_min(x.q_lo); x.q_hi = jh_wave_max(x.q_hi); x.at_lo = jh_wave_min(x.at_lo); x.at_hi = jh_wave_max(x.at_hi);
  if ((i & 63) == 0) {
    s_ext[i >> 6][0] = x.q_lo; s_ext[i >> 6][1] = x.q_hi; s_ext[i >> 6][2] = x.at_lo; s_ext[i >> 6][3] = x.at_hi;
  }
}

// Thread 0, after block_sums: the scalar losses, the multipliers' gradients and steps, the statistics in MPO_STATS order.  alpha_sigma
// steps only where it has a gradient (`step_sigma`: the continuous policy); the discrete kernel reports the block's value.  `a`: either
// kernel's arguments (R, blk, hyper, stats); s: the workgroup's sums of the rows' terms.
struct MpoSums { double crit, act, L, wAt, kl_mu, kl_sigma, al; };
template <typename Args>
__device__ __forceinline__ void mpo_finish(const Args& a, const Mult& m, const MpoSums& s, bool step_sigma, Extrema x, const float (*s_ext)[4]) {
  const double n = (double)a.R, d_eta = (double)m.eta;
  const double mean_L = s.L / n;
  const double eta_loss = d_eta * (double)m.eps_eta + d_eta * mean_L;  // mpo.py:276-278, 370-372
  const float g_eta = (float)((double)m.eps_eta + mean_L - (s.wAt / n) / d_eta);
  const float g_mu = (float)((double)m.eps_mu - s.kl_mu / n);
  const float g_sg = (float)((double)m.eps_sigma - s.kl_sigma / n);
  const float t = a.hyper[JH_HY_STEP] + 1.f;  // the step the actor's Adam takes for this learn (its optimizer pass advances it later)
  const float eta_n = multiplier_step(a.blk, 0, g_eta, a.hyper, t);
  const float mu_n = multiplier_step(a.blk, 1, g_mu, a.hyper, t);
  const float sg_n = step_sigma ? multiplier_step(a.blk, 2, g_sg, a.hyper, t) : m.alpha_sigma;
  if (float* stats = a.stats) {
    const int nw = ((int)blockDim.x + 63) >> 6;
    for (int w = 1; w < nw; ++w) {
      x.q_lo = fminf(x.q_lo, s_ext[w][0]); x.q_hi = fmaxf(x.q_hi, s_ext[w][1]); x.at_lo = fminf(x.at_lo, s_ext[w][2]); x.at_hi = fmaxf(x.at_hi, s_ext[w][3]);
    }
    const float out[11] = {(float)(-s.act / n), (float)(s.crit / n), (float)eta_loss, (float)(s.al / n), eta_n, mu_n, sg_n, x.q_lo, x.q_hi, x.at_lo, x.at_hi};
    for (int j = 0; j < 11; ++j) stats[j] = out[j];
  }
}

__global__ void __launch_bounds__(kMaxRows) jh_mpo_loss_kernel(MpoArgs a) {
  __shared__ double s_qret[kMaxRows];
  __shared__ float s_c[kMaxRows], s_qta[kMaxRows], s_done[kMaxRows];
  __shared__ double s_red[kMaxWaves][8];
  __shared__ float s_ext[kMaxWaves][4];
  const int i = threadIdx.x, R = a.R, T = a.T, A = a.A;
  const bool on = i < R;
  const Mult m = mult_load(a.blk);
  const size_t o = (size_t)i * A;  // only dereferenced when `on`

  // ---- per row: the policies' log-sums, c, the one-step target
  double lse = 0.0, lse_old = 0.0;
  int ak = 0;
  if (on) {
    lse = row_lse(a.la + o, A);
    lse_old = row_lse(a.la_old + o, A);
    const double lse_next = row_lse(a.la_next + o, A);
    ak = action_index(a.action[i], A);
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

  retrace_scan(s_qret, s_c, s_qta, s_done, a.retrace, R, T, a.gamma);
  __syncthreads();

  // ---- per row: critic, advantage, E-step weights, actor, temperature and trust-region terms, head gradients
  double crit = 0.0, act = 0.0, Lr = 0.0, uAt = 0.0, kld = 0.0;
  Extrema x;
  if (on) {
    const double inv_R = 1.0 / (double)R, d_eta = (double)m.eta;
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
      a.g_la[o + k] = (float)(((pk - w) + (double)m.alpha_mu * (pk - po)) * inv_R);
      a.g_q[o + k] = k == ak ? (float)(2.0 * dq * inv_R) : 0.f;
      x.q_lo = fminf(x.q_lo, qk); x.q_hi = fmaxf(x.q_hi, qk);
      const float Atf = (float)At;
      x.at_lo = fminf(x.at_lo, Atf); x.at_hi = fmaxf(x.at_hi, Atf);
    }
  }
  const double al = on ? alpha_loss_row(m.alpha_mu, m.eps_mu, kld) : 0.0;
  extrema_publish(x, s_ext);
  double s6[6] = {crit, act, Lr, uAt, kld, al};
  block_sums<6>(s6, s_red);  // its barriers publish s_ext too
  if (i != 0) return;
  mpo_finish(a, m, MpoSums{s6[0], s6[1], s6[2], s6[3], s6[4], 0.0, s6[5]}, false, x, s_ext);
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

// MPO, continuous policy (core/agent/mpo.py:199-309): the Gaussian policy's raw heads are [mu | log_std] rows of 2A floats with
// mu = clamp(raw, -5, 5) and std = exp(tanh(raw)) (network/policy.py:53-55); N = num_sample actions per row come from two policies.
//   jh_mpo_sample            one elementwise launch: zn = mu' + std' eps[0] from online(s'), zt_add = mut + stdt eps[1] from target(s), and their
//                            tanh, each [N][R][A]                                                                    (mpo.py:221-226, 255-258)
//   jh_mpo_loss_continuous   the discrete kernel's sibling, ONE launch of ONE workgroup, one row per thread:
//     importance   z = the pre-tanh value of the stored action (jh_policy_head.h's gauss_z), c = min(exp(sum_A log N(z; mu, std)) / (prob_b + 1e-6), 1)
//                  from the ONLINE policy                                                                            (mpo.py:203-206, 233)
//     target       Qret = reward + gamma mean_n qt_next (1 - done) -> LDS, then the Retrace scan of the discrete kernel   (mpo.py:235-253)
//     E-step       At = qt_add - mean_n qt_add, w = softmax_n(At / eta) (a constant), actor = -mean_r sum_n w log N(zt_add[n]; mu, std);
//                  eta_loss = eta eps_eta + eta mean_r log mean_n exp(At / eta)                                      (mpo.py:265-278)
//     trust region KLD_mu = 1/2 sum_A (mu - mu_old)^2 std_old^2, KLD_sigma = 1/2 (sum_A std^2 / std_old^2 - A + log(prod ss / prod ss_old)),
//                  ss = 1 / std^2, each with its own multiplier and threshold                                        (mpo.py:280-309)
//     gradients    with respect to the RAW heads of online(s) (zero in mu where the raw value lies outside [-5, 5], through 1 - tanh^2 for
//                  log_std) and to q
//     multipliers  eta, alpha_mu AND alpha_sigma step here (all three have a gradient), then the floors.
// The [N][R] tables qt_next / qt_add and zt_add [N][R][A] stay in global memory: thread r reads element (n, r), so a wavefront's loads
// are consecutive floats for every n, every element has exactly one reader and there is nothing for LDS to share; the second pass over
// qt_add (at most 8192 floats in all) comes out of L2.  LDS holds the scan's per-row state only, as in the discrete kernel.
// Departures on purpose: the log-mean of eta_loss is formed around the row's largest At / eta (finite where float32 exp overflows), and
// the log of the product ratio in KLD_sigma is the sum of the logs, 2 sum_A (tanh_old - tanh): finite at any A, equal elsewhere.
namespace {

constexpr int kMaxSampled = 8192;    // N * R rows of the sampled tables
constexpr int kMaxContActions = 8;   // A: the row's thread keeps two accumulators per action dimension in registers

// i over [N][R][A]; blockIdx.y 0: online(s') and eps[0] -> zn, a_next; 1: target(s) and eps[1] -> zt_add, a_add
__global__ void __launch_bounds__(256) jh_mpo_sample_kernel(int n, int R, int A, const float* __restrict__ head_next, const float* __restrict__ head_old,
                                                            const float* __restrict__ eps, float* __restrict__ zn, float* __restrict__ zt_add,
                                                            float* __restrict__ a_next, float* __restrict__ a_add) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= n) return;
  const int which = (int)blockIdx.y;
  const int k = i % A, r = (i / A) % R;
  const float* head = (which ? head_old : head_next) + (size_t)r * 2 * A;
  const float mu = fminf(fmaxf(head[k], -5.f), 5.f);
  const float sd = expf(tanhf(head[A + k]));
  const float z = mu + sd * eps[(size_t)which * n + i];
  (which ? zt_add : zn)[i] = z;
  (which ? a_add : a_next)[i] = tanhf(z);
}

struct MpoContArgs {
  int R, T, N, A, retrace;
  const float *head, *head_old;      // [R][2A]
  const float *q, *qt_a;             // [R]
  const float *qt_next, *qt_add;     // [N][R]
  const float* zt_add;               // [N][R][A]
  const float* action;               // [R][A]
  const float *reward, *done, *prob_b;  // [R]
  float* blk;
  const float* hyper;
  float gamma;
  float *g_head, *g_q;  // [R][2A], [R]
  float* stats;
};

__global__ void __launch_bounds__(kMaxRows) jh_mpo_loss_cont_kernel(MpoContArgs a) {
  __shared__ double s_qret[kMaxRows];
  __shared__ float s_c[kMaxRows], s_qta[kMaxRows], s_done[kMaxRows];
  __shared__ double s_red[kMaxWaves][8];
  __shared__ float s_ext[kMaxWaves][4];
  const int i = threadIdx.x, R = a.R, T = a.T, N = a.N, A = a.A;
  const bool on = i < R;
  const Mult m = mult_load(a.blk);
  const size_t o = (size_t)i * 2 * A;  // only dereferenced when `on`

  // ---- per row: log pi(a) of the stored action, c, the one-step target
  if (on) {
    double logp = 0.0;
    for (int k = 0; k < A; ++k) {
      const GaussElem e = gauss_elem(a.head[o + k], a.head[o + A + k]);
      logp += gauss_log_prob(gauss_z(a.action[(size_t)i * A + k]) - e.mu, e.th, e.var);
    }
    const double ratio = exp(logp) / ((double)a.prob_b[i] + 1e-6);
    double qn = 0.0;
    for (int n = 0; n < N; ++n) qn += (double)a.qt_next[(size_t)n * R + i];
    const float dn = a.done[i];
    s_qret[i] = (double)a.reward[i] + (double)a.gamma * (qn / (double)N) * (1.0 - (double)dn);
    s_c[i] = (float)(ratio < 1.0 ? ratio : 1.0);  // a NaN ratio stays out of the `<` and gives 1; torch.clip would keep it: the inputs are finite
    s_qta[i] = a.qt_a[i];
    s_done[i] = dn;
  }
  __syncthreads();

  retrace_scan(s_qret, s_c, s_qta, s_done, a.retrace, R, T, a.gamma);
  __syncthreads();

  // ---- per row: critic, advantage over the samples, E-step weights, actor, temperature and trust-region terms, head gradients
  double crit = 0.0, act = 0.0, Lr = 0.0, wAt = 0.0, kl0 = 0.0, kl1 = 0.0;
  Extrema x;
  if (on) {
    const double inv_R = 1.0 / (double)R, d_eta = (double)m.eta;
    const float qf = a.q[i];
    const double dq = (double)qf - s_qret[i];
    crit = dq * dq;
    a.g_q[i] = (float)(2.0 * dq * inv_R);
    x.q_lo = qf; x.q_hi = qf;
    double V = 0.0;
    for (int n = 0; n < N; ++n) V += (double)a.qt_add[(size_t)n * R + i];
    V /= (double)N;
    double xm = -INFINITY;
    for (int n = 0; n < N; ++n) {
      const double At = (double)a.qt_add[(size_t)n * R + i] - V;
      xm = fmax(xm, At / d_eta);
      const float Atf = (float)At;
      x.at_lo = fminf(x.at_lo, Atf); x.at_hi = fmaxf(x.at_hi, Atf);
    }
    // sums over the samples of e = exp(At / eta - xm): e, e At, and per action dimension e dm and e dm^2 with dm = zt_add - mu
    double sw = 0.0, s1[kMaxContActions], s2[kMaxContActions], mu[kMaxContActions];
#pragma unroll
    for (int k = 0; k < kMaxContActions; ++k) {
      s1[k] = 0.0; s2[k] = 0.0;
      mu[k] = k < A ? gauss_mu(a.head[o + k]) : 0.0;
    }
    for (int n = 0; n < N; ++n) {
      const double At = (double)a.qt_add[(size_t)n * R + i] - V;
      const double e = exp(At / d_eta - xm);
      sw += e;
      wAt += e * At;
      const float* zt = a.zt_add + ((size_t)n * R + i) * A;
#pragma unroll
      for (int k = 0; k < kMaxContActions; ++k) {
        if (k < A) {
          const double dm = (double)zt[k] - mu[k];
          s1[k] += e * dm;
          s2[k] += e * dm * dm;
        }
      }
    }
    Lr = xm + log(sw / (double)N);
    wAt /= sw;
    const double c_mu = (double)m.alpha_mu * inv_R, c_sg = (double)m.alpha_sigma * inv_R;
    double kls = 0.0;
#pragma unroll
    for (int k = 0; k < kMaxContActions; ++k) {
      if (k < A) {
        GaussElem e = gauss_elem(a.head[o + k], a.head[o + A + k]);
        e.mu = mu[k];  // the same value, already in a register: the clamp is not evaluated a second time
        const GaussTrust tr = gauss_trust(e, gauss_elem(a.head_old[o + k], a.head_old[o + A + k]));
        const double w1 = s1[k] / sw, w2 = s2[k] / sw;  // sum_n w dm, sum_n w dm^2
        act += gauss_log_prob_sq(w2, e.th, e.var);      // sum_n w log N(zt_add[n]; mu, std) of this dimension (sum_n w = 1)
        kl0 += tr.kl0;
        kls += tr.kls;
        // d(-sum_n w logp): -w1 / var to mu, -(w2 / var - 1) to th
        const double g_mu = (-w1 / e.var) * inv_R + gauss_trust_grad_mu(tr, c_mu);
        const double g_th = -(w2 / e.var - 1.0) * inv_R + gauss_trust_grad_th(tr, c_sg);
        a.g_head[o + k] = gauss_grad_mu_raw(e, g_mu);
        a.g_head[o + A + k] = gauss_grad_log_std_raw(e, g_th);
      }
    }
    gauss_trust_finish(kl0, kl1, kls, A);
  }
  const double al = on ? alpha_loss_row(m.alpha_mu, m.eps_mu, kl0) + alpha_loss_row(m.alpha_sigma, m.eps_sigma, kl1) : 0.0;
  extrema_publish(x, s_ext);
  double s7[7] = {crit, act, Lr, wAt, kl0, kl1, al};
  block_sums<7>(s7, s_red);  // its barriers publish s_ext too
  if (i != 0) return;
  mpo_finish(a, m, MpoSums{s7[0], s7[1], s7[2], s7[3], s7[4], s7[5], s7[6]}, true, x, s_ext);
}

inline bool mpo_cont_shape_ok(int R, int N, int A) {
  return R >= 1 && R <= kMaxRows && N >= 1 && (int64_t)N * R <= kMaxSampled && A >= 1 && A <= kMaxContActions;
}

}  // namespace

JH_EXPORT int jh_mpo_sample(jh_ctx* ctx, int32_t R, int32_t N, int32_t A, const float* d_head_next, const float* d_head_old, const float* d_eps, float* d_zn,
                            float* d_zt_add, float* d_a_next, float* d_a_add, jh_stream stream) {
  JH_ARG(ctx && d_head_next && d_head_old && d_eps && d_zn && d_zt_add && d_a_next && d_a_add);
  JH_ARG(mpo_cont_shape_ok(R, N, A));
  const int n = N * R * A;  // <= 8192 * 8
  JH_LAUNCH(jh_mpo_sample_kernel, dim3((unsigned)((n + 255) / 256), 2), dim3(256), 0, jh_s(stream), n, R, A, d_head_next, d_head_old, d_eps, d_zn, d_zt_add,
            d_a_next, d_a_add);
  JH_LAUNCH_CHECK();
  return JH_OK;
}

JH_EXPORT int jh_mpo_loss_continuous(jh_ctx* ctx, int32_t R, int32_t T, int32_t N, int32_t A, const float* d_head, const float* d_head_old, const float* d_q,
                                     const float* d_qt_a, const float* d_qt_next, const float* d_qt_add, const float* d_zt_add, const float* d_action,
                                     const float* d_reward, const float* d_done, const float* d_prob_b, float* d_block, const float* d_hyper, float gamma,
                                     int32_t retrace, float* d_grad_head, float* d_grad_q, float* d_stats, jh_stream stream) {
  JH_ARG(ctx && d_head && d_head_old && d_q && d_qt_a && d_qt_next && d_qt_add && d_zt_add && d_action && d_reward && d_done && d_prob_b && d_block && d_hyper);
  JH_ARG(d_grad_head && d_grad_q);
  JH_ARG(mpo_cont_shape_ok(R, N, A) && T >= 1 && R % T == 0);
  JH_ARG(retrace == 0 || retrace == 1);
  JH_ARG(((uintptr_t)d_hyper & 7) == 0);
  MpoContArgs a{};
  a.R = R; a.T = T; a.N = N; a.A = A; a.retrace = retrace; a.head = d_head; a.head_old = d_head_old; a.q = d_q; a.qt_a = d_qt_a; a.qt_next = d_qt_next;
  a.qt_add = d_qt_add; a.zt_add = d_zt_add; a.action = d_action; a.reward = d_reward; a.done = d_done; a.prob_b = d_prob_b; a.blk = d_block; a.hyper = d_hyper;
  a.gamma = gamma; a.g_head = d_grad_head; a.g_q = d_grad_q; a.stats = d_stats;
  const int threads = ((R + 63) / 64) * 64;
  JH_LAUNCH(jh_mpo_loss_cont_kernel, dim3(1), dim3(threads), 0, jh_s(stream), a);
  JH_LAUNCH_CHECK();
  return JH_OK;
}
