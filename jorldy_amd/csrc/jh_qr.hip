// The quantile family: what QR-DQN (core/agent/qrdqn.py), IQN (core/agent/iqn.py) and M-IQN (core/agent/m_iqn.py) share below the
// network.  One loss and one acting kernel, instantiated for the two layouts of a row block the networks write and, for the loss, the
// two rules that turn the target network's quantiles into theta_target:
//   jh_qr_loss       pairwise quantile-Huber loss, forward and backward to the online quantiles, online net selects / target net
//                    evaluates; [B][A][N], tau [N] shared by the batch                (qrdqn.py:60-95)
//   jh_iqn_loss      the same on [B][N][A] with tau [B][N], the draw of each sample   (iqn.py:89-121)
//   jh_miqn_loss     jh_iqn_loss's pairwise phase under the Munchausen target: log-policy bonus of the online net's second draw at s,
//                    soft bootstrap over the target net's policy at s'                (m_iqn.py:29-95)
//   jh_riqn_loss     jh_iqn_loss under Rainbow's return and replay: the greedy target folded over an n-step window of rewards and
//                    dones, an importance weight per sample, priorities loss_b ^ alpha  (rainbow_iqn.py:158-224)
//   jh_quantile_act  epsilon-greedy acting on the mean of the N quantiles, [R][A][N]  (qrdqn.py:33-47, 112-115)
//   jh_iqn_act       the same on [R][N][A]                                            (iqn.py:60-76, 142-146)
// No floating-point atomics: every sum has a fixed order, so two runs (and a graph replay) give the same bits.
#include "jh_common.h"

namespace {

// Layout of one row block (the A x N values of sample / actor row b).  It decides the address of element (action a, quantile i),
// whether tau is shared or per sample, and the shape of the loop that zeroes the gradient of the actions not taken -- nothing else.
enum QLayout {
  Q_ACTION_MAJOR,  // [A][N], tau [N]     (QR-DQN: the N quantiles of an action are contiguous)
  Q_SAMPLE_MAJOR   // [N][A], tau [B][N]  (IQN: the A values of a sample are contiguous)
};

template <QLayout L>
__device__ __forceinline__ size_t q_at(int b, int A, int N, int a, int i) {
  return L == Q_ACTION_MAJOR ? ((size_t)b * A + a) * N + i : (size_t)b * N * A + (size_t)i * A + a;
}

// The rule that fills the Bellman image T[j] of the target quantiles -- and with it what the second network output means.
enum QTarget {
  Q_TGT_GREEDY,     // next_logit = online(s'): its best mean selects the action the target net evaluates       (qrdqn.py:76-81, iqn.py:106-111)
  Q_TGT_MUNCHAUSEN  // next_logit = online(s) under a second draw: its means are the policy of the log-policy
                    // bonus; the target net's own means at s' are the policy of the soft bootstrap             (m_iqn.py:50-79)
};

// What a sample brings beside its transition -- and with it the shape of reward / done and what leaves the kernel beside the gradient.
enum QReturn {
  Q_RET_1STEP,     // reward, done [B]; every sample weighs 1
  Q_RET_NSTEP_PER  // reward, done [B][n_step], folded from the last step to the first; prio[b] = loss_b ^ alpha; the IS weights enter as their
                   // mean: rainbow_iqn.py:217-219 multiplies weights [B, 1] with loss [B], a [B, B] product whose mean is mean(w) * mean(loss_b)
                   // (the broadcast jh_c51_loss keeps for Rainbow under JH_C51_PER)
};

struct QrArgs {
  int B, A, N;
  const float *logit, *next_logit, *target_logit, *action, *reward, *done, *tau;
  float gamma;
  float alpha, tau_e, l_0;  // Munchausen: scale of the bonus, entropy temperature (the agent's self.tau), lower clip of the log-policy
  float *grad, *stats, *partial;  // partial [B][4] = {sum_j sum_i w * huber, max Q, max logit, min logit} of a sample
  // Q_RET_NSTEP_PER
  int n_step;
  const float* weights;  // [B]
  float prio_alpha;
  float* prio;           // [B]
};

// Mean of the N quantiles of action a of row block b of z on one wave (torch.mean(_logits, dim=-1), qrdqn.py:114; logits2Q,
// iqn.py:142-146): every lane returns it.  rmx / rmn: the largest / smallest of the N entries.
template <QLayout L>
__device__ __forceinline__ float qr_row_mean(const float* __restrict__ z, int b, int A, int N, int a, int lane, float& rmx, float& rmn) {
  float s = 0.f;
  rmx = -3.4e38f;
  rmn = 3.4e38f;
  for (int k = lane; k < N; k += 64) {
    const float v = z[q_at<L>(b, A, N, a, k)];
    s += v;
    rmx = fmaxf(rmx, v);
    rmn = fminf(rmn, v);
  }
  rmx = jh_wave_max(rmx);
  rmn = jh_wave_min(rmn);
  return jh_wave_sum(s) / (float)N;
}

// m_iqn.py:53-79 with agent/utils.py:29-39, for sample b: x = s_pol[A] (means of the online net's second draw at s), x' = s_nxt[A]
// (means of the target net at s'), each with its row maximum subtracted before every exp:
//   lp      = x[act] - (max x + tau_e log sum_k exp((x_k - max x) / tau_e)),  munchausen = alpha * clip(lp, l_0, 0)
//   pi_k    = exp((x'_k - max x') / tau_e - log sum exp(...)),  logpi_k = x'_k - (max x' + tau_e log sum exp(...))
//   T[j]    = (reward + munchausen) + ((1 - done) * gamma) * sum_k pi_k * (target[b][k][j] - logpi_k)
// Every thread walks the same A values in the same order (as the first-maximum walk of the greedy rule does); pi and logpi meet in
// LDS (s_pi, s_lpi [A]).  A = 1: lp = 0, pi = 1.  expf / logf are the accurate ones.
template <QLayout L>
__device__ __forceinline__ void qr_munchausen_target(const QrArgs& a, int b, int act, float r, float dn, const float* s_pol, const float* s_nxt, float* s_pi,
                                                     float* s_lpi, float* s_T, int tid, bool own) {
  const int A = a.A, N = a.N;
  float m = s_pol[0], mn = s_nxt[0];
  for (int k = 1; k < A; ++k) {
    m = fmaxf(m, s_pol[k]);
    mn = fmaxf(mn, s_nxt[k]);
  }
  float se = 0.f, sn = 0.f;
  for (int k = 0; k < A; ++k) {
    se += expf((s_pol[k] - m) / a.tau_e);
    sn += expf((s_nxt[k] - mn) / a.tau_e);
  }
  const float lp = s_pol[act] - (m + a.tau_e * logf(se));
  const float mun = a.alpha * fminf(fmaxf(lp, a.l_0), 0.f);
  const float lsn = logf(sn);
  const float tau_lse = mn + a.tau_e * lsn;
  for (int k = tid; k < A; k += 256) {
    const float x = s_nxt[k];
    s_pi[k] = expf((x - mn) / a.tau_e - lsn);  // exp(log_softmax(y / tau)): the row maximum of y / tau is 0   utils.py:36-39
    s_lpi[k] = x - tau_lse;
  }
  __syncthreads();
  if (own) {
    float soft = 0.f;
    for (int k = 0; k < A; ++k) soft += s_pi[k] * (a.target_logit[q_at<L>(b, A, N, k, tid)] - s_lpi[k]);
    s_T[tid] = (r + mun) + ((1.f - dn) * a.gamma) * soft;  // m_iqn.py:75-79, in torch's order of operations
  }
}

// One workgroup of 256 threads per sample (N <= 256: thread i owns prediction quantile i).
// LDS: [N] Bellman image of the target quantiles, [A] selector means, [4][3] per-wave statistics, [16] reduction; Munchausen: + [3][A]
// (the target net's means at s', pi, logpi).
// Every thread stays to the end: the work of threads i >= N is predicated, not skipped (block reduction at the end).
template <QLayout L, QTarget T, QReturn R>
__global__ void __launch_bounds__(256) jh_qr_block_kernel(QrArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int b = blockIdx.x, A = a.A, N = a.N;
  float* s_T = smem;           // [N]
  float* s_qsel = s_T + N;     // [A]
  float* s_stat = s_qsel + A;  // [4][3]
  float* s_red = s_stat + 12;  // [16]
  float* s_nxt = s_red + 16;   // [A], then s_pi [A], s_lpi [A]   (Munchausen only)
  int act = (int)a.action[b];
  act = act < 0 ? 0 : (act >= A ? A - 1 : act);
  // n-step: the window's rewards and dones are read where the target is folded
  const float r = R == Q_RET_1STEP ? a.reward[b] : 0.f, dn = R == Q_RET_1STEP ? a.done[b] : 0.f;
  // wb: mean of the batch's importance weights, summed in the same fixed order by every workgroup (unit weights: exactly 1)
  float wb = 1.f;
  if constexpr (R == Q_RET_NSTEP_PER) {
    float ws = 0.f;
    for (int k = tid; k < a.B; k += 256) ws += a.weights[k];
    wb = jh_block_reduce(ws, s_red, JhAdd(), 0.f) / (float)a.B;
  }
  // what phase 3 keeps in registers, requested ahead of the reductions of phase 1
  const bool own = tid < N;
  const int ti = own ? tid : N - 1;
  const float P = a.logit[q_at<L>(b, A, N, act, ti)];
  // IQN: the FIRST forward's draw for this sample (iqn.py:90, 96)
  const float tau = a.tau[L == Q_ACTION_MAJOR ? (size_t)ti : (size_t)b * N + ti];
  const float inv_tau = 1.f - tau;  // qrdqn.py:31, iqn.py:120
  // ---- phase 1: quantile means of online(s) (statistics) and online(s') (selector), actions strided over the waves.  Munchausen: the
  // second output is online(s) again; max / min logit are ITS extremes (m_iqn.py:50 reassigns `logit` before lines 94-95 read it),
  // max_Q stays the first output's (m_iqn.py:31, 93); the target net's means at s' are the third set
  float maxq = -3.4e38f, maxl = -3.4e38f, minl = 3.4e38f;
  for (int aa = wid; aa < A; aa += 4) {
    float rmx, rmn, x0, x1;
    const float q = qr_row_mean<L>(a.logit, b, A, N, aa, lane, rmx, rmn);
    maxq = fmaxf(maxq, q);
    const float q2 = qr_row_mean<L>(a.next_logit, b, A, N, aa, lane, x0, x1);
    maxl = fmaxf(maxl, T == Q_TGT_GREEDY ? rmx : x0);
    minl = fminf(minl, T == Q_TGT_GREEDY ? rmn : x1);
    if (lane == 0) s_qsel[aa] = q2;
    if constexpr (T == Q_TGT_MUNCHAUSEN) {
      const float q3 = qr_row_mean<L>(a.target_logit, b, A, N, aa, lane, x0, x1);
      if (lane == 0) s_nxt[aa] = q3;
    }
    if constexpr (L == Q_ACTION_MAJOR) {
      if (aa != act) {  // the rows of the actions not taken: zero gradient (net.backward reads all of it)
        float* g = a.grad + q_at<L>(b, A, N, aa, 0);
        for (int k = lane; k < N; k += 64) g[k] = 0.f;
      }
    }
  }
  if constexpr (L == Q_SAMPLE_MAJOR) {
    // the entries of the actions not taken, interleaved with the taken one: a flat walk, no division on the action-major path
    float* g = a.grad + q_at<L>(b, A, N, 0, 0);
    for (int k = tid; k < N * A; k += 256)
      if (k % A != act) g[k] = 0.f;
  }
  if (lane == 0) { s_stat[wid * 3 + 0] = maxq; s_stat[wid * 3 + 1] = maxl; s_stat[wid * 3 + 2] = minl; }
  __syncthreads();
  if constexpr (T == Q_TGT_GREEDY) {
    // ---- a* = first maximum of the online net's means at s' (qrdqn.py:76, iqn.py:106); every thread walks the same A values
    int best = 0;
    float bq = -3.4e38f;
    for (int aa = 0; aa < A; ++aa) {
      const float q = s_qsel[aa];
      if (q > bq) { bq = q; best = aa; }
    }
    // ---- phase 2: theta_target = reward + (1 - done) * gamma * target(s')[a*]  (qrdqn.py:79-81, iqn.py:109-111, in torch's order of operations)
    if constexpr (R == Q_RET_1STEP) {
      if (own) s_T[tid] = r + ((1.f - dn) * a.gamma) * a.target_logit[q_at<L>(b, A, N, best, tid)];
    } else if (own) {
      // rainbow_iqn.py:192-195: for i in reversed(range(n_step)): T = reward[:, i] + (1 - done[:, i]) * gamma * T, in torch's order of operations
      float t = a.target_logit[q_at<L>(b, A, N, best, tid)];
      const float* rw = a.reward + (size_t)b * a.n_step;
      const float* dw = a.done + (size_t)b * a.n_step;
      for (int i = a.n_step - 1; i >= 0; --i) t = rw[i] + ((1.f - dw[i]) * a.gamma) * t;
      s_T[tid] = t;
    }
  } else {
    // ---- phase 2: theta_target = reward + Munchausen bonus + (1 - done) * gamma * soft value of target(s')   (m_iqn.py:53-79)
    qr_munchausen_target<L>(a, b, act, r, dn, s_qsel, s_nxt, s_nxt + A, s_nxt + 2 * A, s_T, tid, own);
  }
  __syncthreads();
  // ---- phase 3: thread i walks the targets j; e = T[j] - P[i], smooth_l1 (beta 1), weight tau[i] / 1 - tau[i] by the sign of e
  float ls = 0.f, gs = 0.f;
  for (int j = 0; j < N; ++j) {
    const float e = s_T[j] - P;  // the same LDS word for every lane: a broadcast
    const float ae = fabsf(e);
    const float hub = ae < 1.f ? 0.5f * e * e : ae - 0.5f;
    const float w = e < 0.f ? inv_tau : tau;
    ls += w * hub;
    gs += w * fminf(fmaxf(e, -1.f), 1.f);
  }
  // rainbow_iqn.py:219: loss = mean(w) * mean_b(loss_b); unit weights leave the 1-step entries' bits
  if (own) a.grad[q_at<L>(b, A, N, act, tid)] = R == Q_RET_1STEP ? -gs / ((float)a.B * (float)N) : -(wb * gs) / ((float)a.B * (float)N);
  // ---- phase 4: the sample's loss, wave shuffle tree then the waves in order
  const float tot = jh_block_reduce(own ? ls : 0.f, s_red, JhAdd(), 0.f);
  if (tid == 0) {
    float mq = -3.4e38f, ml = -3.4e38f, nl = 3.4e38f;
    const int nw = A < 4 ? A : 4;  // waves that saw at least one action
    for (int w = 0; w < nw; ++w) {
      mq = fmaxf(mq, s_stat[w * 3 + 0]);
      ml = fmaxf(ml, s_stat[w * 3 + 1]);
      nl = fminf(nl, s_stat[w * 3 + 2]);
    }
    float* p = a.partial + 4 * (size_t)b;
    p[0] = R == Q_RET_1STEP ? tot : wb * tot; p[1] = mq; p[2] = ml; p[3] = nl;
    if constexpr (R == Q_RET_NSTEP_PER) a.prio[b] = powf(tot / (float)N, a.prio_alpha);  // rainbow_iqn.py:205, 212: (mean_j sum_i) ^ alpha
  }
}

// Sum of the per-sample partials in a fixed order -> d_stats, payload fenced before the arrival marks (as jh_c51_finish_kernel).
// The partials carry no layout: one kernel for both.
__global__ void __launch_bounds__(256) jh_qr_finish_kernel(QrArgs a) {
  __shared__ float s_red[16];
  float sl = 0.f, mq = -3.4e38f, ml = -3.4e38f, nl = 3.4e38f;
  for (int b = threadIdx.x; b < a.B; b += 256) {
    sl += a.partial[4 * (size_t)b];
    mq = fmaxf(mq, a.partial[4 * (size_t)b + 1]);
    ml = fmaxf(ml, a.partial[4 * (size_t)b + 2]);
    nl = fminf(nl, a.partial[4 * (size_t)b + 3]);
  }
  sl = jh_block_reduce(sl, s_red, JhAdd(), 0.f);
  mq = jh_block_reduce(mq, s_red, JhMax(), -3.4e38f);
  ml = jh_block_reduce(ml, s_red, JhMax(), -3.4e38f);
  nl = jh_block_reduce(nl, s_red, JhMin(), 3.4e38f);
  if (threadIdx.x == 0 && a.stats) {
    a.stats[0] = sl / ((float)a.B * (float)a.N);  // qrdqn.py:91, iqn.py:121: mean over (b, j) of the sum over i
    a.stats[1] = mq;
    a.stats[2] = ml;
    a.stats[3] = nl;
    a.stats[4] = 0.f;
    a.stats[6] = 0.f;
    __threadfence_system();  // payload before the arrival marks [5], [7] (mapped host memory, jh_host_wait_marks)
    a.stats[5] = a.stats[7] = 0.f;
  }
}

// QRDQN.act / IQN.act for R actor rows in one call: one wave per row, Q = mean of the N quantiles, first maximum like torch.argmax,
// epsilon-greedy with the host's draws (jh_value_act's rules), q_taken fenced before the action.
// Every lane of a wave stays through the shuffles: rows beyond R read row R - 1 and write nothing.
template <QLayout L>
__global__ void __launch_bounds__(256) jh_quantile_act_kernel(int R, int A, int N, const float* __restrict__ logits, const float* __restrict__ eps,
                                                              const double* __restrict__ u, const int64_t* __restrict__ rand_action,
                                                              int64_t* __restrict__ action, float* __restrict__ q_taken, float* __restrict__ q_all) {
  const int lane = threadIdx.x & 63;
  const int row0 = blockIdx.x * 4 + (threadIdx.x >> 6);
  const bool live = row0 < R;
  const int row = live ? row0 : R - 1;
  float best = -3.4e38f, q_rand = 0.f;
  int best_a = 0;
  int ra = rand_action ? (int)rand_action[row] : 0;
  ra = ra < 0 ? 0 : (ra >= A ? A - 1 : ra);
  for (int a = 0; a < A; ++a) {
    float rmx, rmn;
    const float q = qr_row_mean<L>(logits, row, A, N, a, lane, rmx, rmn);
    if (q_all && live && lane == 0) q_all[(size_t)row * A + a] = q;
    if (q > best) { best = q; best_a = a; }
    if (a == ra) q_rand = q;
  }
  if (live && lane == 0) {
    const bool explore = eps && u && u[row] < (double)eps[row];
    if (q_taken) {
      q_taken[row] = explore ? q_rand : best;
      __threadfence_system();
    }
    action[row] = explore ? ra : best_a;
  }
}

struct QMunchausen {
  float alpha, tau_e, l_0;
};
struct QPer {
  int n_step;  // columns of reward / done
  const float* weights;
  float alpha;
  float* prio;
};

// The launches keep the names the profile report and DESIGN.md's kernel table know them by, one set per entry point.
template <QLayout L, QTarget T, QReturn R = Q_RET_1STEP>
int qr_loss(jh_ctx* ctx, int32_t B, int32_t A, int32_t N, const float* d_logit, const float* d_next_logit_online, const float* d_target_logit,
            const float* d_action, const float* d_reward, const float* d_done, const float* d_tau, float gamma, float* d_grad_logit, float* d_stats,
            jh_stream stream, QMunchausen mu = {0.f, 1.f, 0.f}, QPer per = {1, nullptr, 0.f, nullptr}) {
  JH_ARG(ctx && d_logit && d_next_logit_online && d_target_logit && d_action && d_reward && d_done && d_tau && d_grad_logit);
  JH_ARG(B >= 1 && A >= 1 && N >= 1 && N <= 256);
  JH_ARG(mu.tau_e > 0.f && mu.l_0 <= 0.f);
  if (R == Q_RET_NSTEP_PER) JH_ARG(per.n_step >= 1 && per.weights && per.prio);
  hipStream_t st = jh_s(stream);
  void* scratch = nullptr;
  int rc = jh_ctx_scratch(ctx, sizeof(float) * 4 * (size_t)B, &scratch);
  if (rc) return rc;
  QrArgs a{};
  a.B = B; a.A = A; a.N = N;
  a.logit = d_logit; a.next_logit = d_next_logit_online; a.target_logit = d_target_logit; a.action = d_action;
  a.reward = d_reward; a.done = d_done; a.tau = d_tau; a.gamma = gamma; a.grad = d_grad_logit; a.stats = d_stats;
  a.alpha = mu.alpha; a.tau_e = mu.tau_e; a.l_0 = mu.l_0;
  a.n_step = per.n_step; a.weights = per.weights; a.prio_alpha = per.alpha; a.prio = per.prio;
  a.partial = (float*)scratch;
  const size_t lds = sizeof(float) * ((size_t)N + (size_t)A * (T == Q_TGT_MUNCHAUSEN ? 4 : 1) + 12 + 16);
  JH_ARG(lds <= 64 * 1024);
  const bool m = T == Q_TGT_MUNCHAUSEN, p = R == Q_RET_NSTEP_PER;
  JH_LAUNCH_NAMED(p ? "jh_riqn_block_kernel" : m ? "jh_miqn_block_kernel" : L == Q_ACTION_MAJOR ? "jh_qr_block_kernel" : "jh_iqn_block_kernel", (jh_qr_block_kernel<L, T, R>),
                  dim3(B), dim3(256), lds, st, a);
  JH_LAUNCH_CHECK();
  JH_LAUNCH_NAMED(p ? "jh_riqn_finish_kernel" : m ? "jh_miqn_finish_kernel" : L == Q_ACTION_MAJOR ? "jh_qr_finish_kernel" : "jh_iqn_finish_kernel", jh_qr_finish_kernel,
                  dim3(1), dim3(256), 0, st, a);
  JH_LAUNCH_CHECK();
  return JH_OK;
}

template <QLayout L>
int qr_act(jh_ctx* ctx, int32_t R, int32_t A, int32_t N, const float* d_logits, const float* h_eps, const double* h_u, const int64_t* h_rand_action,
           int64_t* d_action, float* d_q_taken, float* d_q_all, jh_stream stream) {
  JH_ARG(ctx && d_logits && d_action);
  JH_ARG(R > 0 && A > 0 && N > 0);
  JH_ARG((h_eps == nullptr) == (h_u == nullptr) && (h_eps == nullptr) == (h_rand_action == nullptr));
  hipStream_t st = jh_s(stream);
  jh_draws dr;
  int rc = jh_ctx_stage_draws(ctx, (size_t)R, h_eps, h_u, h_rand_action, &dr);
  if (rc) return rc;
  JH_LAUNCH_NAMED(L == Q_ACTION_MAJOR ? "jh_quantile_act_kernel" : "jh_iqn_act_kernel", jh_quantile_act_kernel<L>, dim3((R + 3) / 4), dim3(256), 0, st, R, A, N,
                  d_logits, dr.eps, dr.u, dr.rand_action, d_action, d_q_taken, d_q_all);
  JH_LAUNCH_CHECK();
  return dr.slab ? jh_ctx_slab_release(ctx, dr.slab, st) : JH_OK;
}

}  // namespace

JH_EXPORT int jh_qr_loss(jh_ctx* ctx, int32_t B, int32_t A, int32_t N, const float* d_logit, const float* d_next_logit_online,
                         const float* d_target_logit, const float* d_action, const float* d_reward, const float* d_done,
                         const float* d_tau, float gamma, float* d_grad_logit, float* d_stats, jh_stream stream) {
  return qr_loss<Q_ACTION_MAJOR, Q_TGT_GREEDY>(ctx, B, A, N, d_logit, d_next_logit_online, d_target_logit, d_action, d_reward, d_done, d_tau, gamma, d_grad_logit, d_stats, stream);
}
JH_EXPORT int jh_iqn_loss(jh_ctx* ctx, int32_t B, int32_t A, int32_t N, const float* d_logit, const float* d_next_logit_online,
                          const float* d_target_logit, const float* d_action, const float* d_reward, const float* d_done,
                          const float* d_tau, float gamma, float* d_grad_logit, float* d_stats, jh_stream stream) {
  return qr_loss<Q_SAMPLE_MAJOR, Q_TGT_GREEDY>(ctx, B, A, N, d_logit, d_next_logit_online, d_target_logit, d_action, d_reward, d_done, d_tau, gamma, d_grad_logit, d_stats, stream);
}
JH_EXPORT int jh_miqn_loss(jh_ctx* ctx, int32_t B, int32_t A, int32_t N, const float* d_logit, const float* d_logit_again, const float* d_target_logit,
                           const float* d_action, const float* d_reward, const float* d_done, const float* d_tau, float gamma, float alpha, float tau_e,
                           float l_0, float* d_grad_logit, float* d_stats, jh_stream stream) {
  return qr_loss<Q_SAMPLE_MAJOR, Q_TGT_MUNCHAUSEN>(ctx, B, A, N, d_logit, d_logit_again, d_target_logit, d_action, d_reward, d_done, d_tau, gamma, d_grad_logit,
                                                   d_stats, stream, QMunchausen{alpha, tau_e, l_0});
}

// n_step as jh_c51_loss takes it: 0 (plain [B] reward / done) or the number of columns of the window
JH_EXPORT int jh_riqn_loss(jh_ctx* ctx, int32_t B, int32_t A, int32_t N, int32_t n_step, const float* d_logit, const float* d_next_logit_online,
                           const float* d_target_logit, const float* d_action, const float* d_reward, const float* d_done, const float* d_weights,
                           const float* d_tau, float gamma, float alpha, float* d_grad_logit, float* d_prio, float* d_stats, jh_stream stream) {
  JH_ARG(n_step >= 0 && d_weights && d_prio);
  return qr_loss<Q_SAMPLE_MAJOR, Q_TGT_GREEDY, Q_RET_NSTEP_PER>(ctx, B, A, N, d_logit, d_next_logit_online, d_target_logit, d_action, d_reward, d_done, d_tau, gamma,
                                                                d_grad_logit, d_stats, stream, QMunchausen{0.f, 1.f, 0.f}, QPer{n_step > 0 ? n_step : 1, d_weights, alpha, d_prio});
}

JH_EXPORT int jh_quantile_act(jh_ctx* ctx, int32_t R, int32_t A, int32_t N, const float* d_logits, const float* h_eps, const double* h_u,
                              const int64_t* h_rand_action, int64_t* d_action, float* d_q_taken, float* d_q_all, jh_stream stream) {
  return qr_act<Q_ACTION_MAJOR>(ctx, R, A, N, d_logits, h_eps, h_u, h_rand_action, d_action, d_q_taken, d_q_all, stream);
}
JH_EXPORT int jh_iqn_act(jh_ctx* ctx, int32_t R, int32_t A, int32_t N, const float* d_logits, const float* h_eps, const double* h_u,
                         const int64_t* h_rand_action, int64_t* d_action, float* d_q_taken, float* d_q_all, jh_stream stream) {
  return qr_act<Q_SAMPLE_MAJOR>(ctx, R, A, N, d_logits, h_eps, h_u, h_rand_action, d_action, d_q_taken, d_q_all, stream);
}
