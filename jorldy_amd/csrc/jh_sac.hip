// Soft actor-critic, continuous actions (core/agent/sac.py:161-269 with the policy of core/network/policy.py:38-55): the elementwise steps
// between the dense layers.
//   jh_sac_sample           mu = clamp(mu_raw, -5, 5), std = exp(tanh(ls_raw)), z = mu + std * eps, a = tanh(z) and
//                           logp = sum_j [Normal(mu, std).log_prob(z)_j - log(1 - a_j^2 + 1e-7)]   (sac.py:161-169)
//   jh_sac_critic_loss      the shared critic loss (jh_acnet.hip) with the entropy term in the target: y = r + (1 - d) gamma (min_i q_i' - alpha logp')
//   jh_sac_actor_seed       actor_loss = -mean(alpha (-logp) + min(q1, q2)), its gradient into q1 / q2, the coefficient alpha / B of logp's
//                           way back, alpha_loss, and the temperature's bookkeeping: alpha <- exp(log_alpha), then Adam on log_alpha
//   jh_sac_sample_backward  d(mu_raw), d(ls_raw) from d(a) and the coefficient of logp
// The temperature lives in a device block of JH_SAC_ALPHA_FLOATS floats (layout below) that the kernels read and advance themselves, so a
// replayed graph sees the current alpha and counts its own Adam steps.
// No floating-point atomics: every sum has a fixed order, so two runs (and a graph replay) give the same bits.
#include "jh_acnet.h"

namespace {

// the alpha block.  IN_USE is the alpha the losses of the CURRENT learn() are formed with (sac.py:250 refreshes it only after the actor
// step, and Adam moves log_alpha after that: the alpha of learn k is exp(log_alpha) after k - 1 steps).
enum {
  SA_LOG_ALPHA = 0, SA_IN_USE = 1, SA_M = 2, SA_V = 3, SA_STEP = 4, SA_LR = 5, SA_EPS = 6, SA_DYNAMIC = 7, SA_TARGET_ENTROPY = 8,
  SA_COEF = 9,    // alpha / B of the actor loss just seeded: what jh_sac_sample_backward multiplies d(logp) with
  SA_B1D = 10,    // beta1 as a double (two floats, 8-byte aligned)
  SA_B2D = 12,    // beta2 as a double
  SA_FLOATS = 16
};

constexpr double kHalfLog2Pi = 0.9189385332046727;

// ---------------------------------------------------------------------------------- sample
// One thread per row, j ascending.  The row is evaluated in double and rounded once: z = mu + std * eps cancels (mu 5, std * eps -5 is an
// ordinary draw), and float32 would then carry the rounding of a ten times larger product into a = tanh(z), where 1 - a^2 is near 1.
// 1 - a^2 is formed as sech^2(z) = 4 t / (1 + t)^2 with t = exp(-2 |z|), which stays exact where 1 - tanh(z)^2 has lost its digits next to
// the 1e-7 of the logarithm.  A row is A elements (a handful): the double rate is not what this launch costs.
// mu_raw / ls_raw: row stride ld (the network object keeps [mu_raw | ls_raw] side by side in one row); eps, a: [B][A].
__global__ void __launch_bounds__(256) jh_sac_sample_kernel(int B, int A, int ld, const float* __restrict__ mu_raw, const float* __restrict__ ls_raw,
                                                            const float* __restrict__ eps, float* __restrict__ a_out, float* __restrict__ logp) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int64_t o = (int64_t)b * A, r = (int64_t)b * ld;
  if (!eps) {
    for (int j = 0; j < A; ++j) a_out[o + j] = tanhf(fminf(fmaxf(mu_raw[r + j], -5.f), 5.f));
    return;
  }
  double s = 0.0;
  for (int j = 0; j < A; ++j) {
    const double mu = (double)fminf(fmaxf(mu_raw[r + j], -5.f), 5.f);
    const double ls = tanh((double)ls_raw[r + j]);
    const double e = (double)eps[o + j];
    const double z = mu + exp(ls) * e;
    a_out[o + j] = (float)tanh(z);
    const double t = exp(-2.0 * fabs(z));
    const double om = 4.0 * t / ((1.0 + t) * (1.0 + t));
    s += (-0.5 * e * e - ls - kHalfLog2Pi) - log(om + 1e-7);
  }
  logp[b] = (float)s;
}

// ---------------------------------------------------------------------------------- actor seed + temperature
// actor_loss = -mean_b(alpha * (-logp_b) + min(q1_b, q2_b)) (sac.py:241-242): d/d(q_i[b]) = -1 / B on the smaller critic, half each on a
// tie (torch.min's backward), d/d(logp_b) = alpha / B -> SA_COEF.  alpha_loss = log_alpha * mean(-logp - target_entropy) (sac.py:248).
// Then thread 0 alone: IN_USE <- exp(log_alpha) (sac.py:250), and, dynamic, one Adam step of log_alpha with the gradient
// mean(-logp - target_entropy) (sac.py:252-255).  The backward of THIS learn reads SA_COEF, formed from the alpha the loss used, so the
// refresh cannot reach it.  stats = {actor_loss, alpha_loss, mean_Q, alpha (the refreshed one), entropy, arrival mark}.
__global__ void __launch_bounds__(256) jh_sac_actor_seed_kernel(int B, int qstride, int gstride, const float* __restrict__ q, const float* __restrict__ logp,
                                                                float* __restrict__ dq, float* blk, float* stats) {
  __shared__ float s_red[16];
  const float alpha = blk[SA_IN_USE], te = blk[SA_TARGET_ENTROPY];
  const float g = -1.f / (float)B;
  float sl = 0.f, sq = 0.f, se = 0.f, sg = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) {
    const float q1 = q[b], q2 = q[qstride + b], ent = -logp[b];
    const float mn = fminf(q1, q2);
    sl += alpha * ent + mn;
    sq += mn;
    se += ent;
    sg += ent - te;
    dq[b] = q1 < q2 ? g : (q1 == q2 ? 0.5f * g : 0.f);
    dq[gstride + b] = q2 < q1 ? g : (q1 == q2 ? 0.5f * g : 0.f);
  }
  const float tl = jh_block_reduce(sl, s_red, JhAdd(), 0.f);
  const float tq = jh_block_reduce(sq, s_red, JhAdd(), 0.f);
  const float tent = jh_block_reduce(se, s_red, JhAdd(), 0.f);
  const float tg = jh_block_reduce(sg, s_red, JhAdd(), 0.f);
  if (threadIdx.x != 0) return;
  const float la = blk[SA_LOG_ALPHA], grad = tg / (float)B;
  const bool dynamic = blk[SA_DYNAMIC] != 0.f;
  const float fresh = dynamic ? expf(la) : alpha;  // a static log_alpha never moves: neither does its alpha
  blk[SA_COEF] = alpha / (float)B;
  if (dynamic) {
    blk[SA_IN_USE] = fresh;
    // torch.optim.Adam on one float32 parameter: lerp of exp_avg, addcmul of exp_avg_sq, the bias corrections and the step size in double
    const double b1 = *reinterpret_cast<const double*>(blk + SA_B1D), b2 = *reinterpret_cast<const double*>(blk + SA_B2D);
    const float t = blk[SA_STEP] + 1.f;  // a float, as the hyper blocks keep it: exact up to 2^24 steps, where it (and the reported step count) would stop advancing
    const float m = blk[SA_M] + (grad - blk[SA_M]) * (float)(1.0 - b1);
    const float v = blk[SA_V] * (float)b2 + (float)(1.0 - b2) * grad * grad;
    const float step_size = (float)((double)blk[SA_LR] / (1.0 - pow(b1, (double)t)));
    const float denom = sqrtf(v) / (float)sqrt(1.0 - pow(b2, (double)t)) + blk[SA_EPS];
    blk[SA_LOG_ALPHA] = la - step_size * (m / denom);
    blk[SA_M] = m;
    blk[SA_V] = v;
    blk[SA_STEP] = t;
  }
  if (stats) {
    stats[0] = -(tl / (float)B);
    stats[1] = la * grad;
    stats[2] = tq / (float)B;
    stats[3] = fresh;
    stats[4] = tent / (float)B;
    __threadfence_system();
    stats[5] = 0.f;
  }
}

// ---------------------------------------------------------------------------------- sample backward
// With z = mu + std * eps the Gaussian part of logp is -eps^2 / 2 - log(std) - log(sqrt(2 pi)): nothing reaches mu through it and
// d/d(log std) = -1.  Through a = tanh(z): d(a)/dz = 1 - a^2 and d(-log(1 - a^2 + 1e-7))/dz = 2 a (1 - a^2) / (1 - a^2 + 1e-7).
//   dz = da (1 - a^2) + c 2 a (1 - a^2) / (1 - a^2 + 1e-7)          c = SA_COEF, da = da1 (+ da2)
//   d(mu_raw) = dz where -5 <= mu_raw <= 5, else 0                  (the clamp passes the gradient on its bounds)
//   d(ls_raw) = (dz std eps - c) (1 - tanh(ls_raw)^2)
// da1, da2, eps, a: [B][A]; mu_raw, ls_raw and the two gradients: row stride ld.
__global__ void __launch_bounds__(256) jh_sac_sample_bwd_kernel(int64_t n, int A, int ld, const float* __restrict__ da1, const float* __restrict__ da2,
                                                                const float* __restrict__ mu_raw, const float* __restrict__ ls_raw,
                                                                const float* __restrict__ eps, const float* __restrict__ a, const float* __restrict__ blk,
                                                                float* __restrict__ dmu, float* __restrict__ dls) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t r = (i / A) * ld + (i % A);
  const float c = blk[SA_COEF];
  const float da = da2 ? da1[i] + da2[i] : da1[i];
  const float v = a[i];
  const float om = 1.f - v * v;
  const float dz = da * om + c * (2.f * v) * (om / (om + 1e-7f));
  const float m = mu_raw[r];
  dmu[r] = (m >= -5.f && m <= 5.f) ? dz : 0.f;
  const float ls = tanhf(ls_raw[r]);
  dls[r] = (dz * expf(ls) * eps[i] - c) * (1.f - ls * ls);
}

// mu = clamp(mu_raw, -5, 5), std = exp(tanh(ls_raw))   (policy.py:38-55): what the policy module returns, for acting
__global__ void __launch_bounds__(256) jh_sac_mu_std_kernel(int64_t n, int A, int ld, const float* __restrict__ raw, float* __restrict__ mu, float* __restrict__ std) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t r = (i / A) * ld + (i % A);
  mu[i] = fminf(fmaxf(raw[r], -5.f), 5.f);
  std[i] = expf(tanhf(raw[r + A]));
}

static int sac_sample(int B, int A, int ld, const float* mu_raw, const float* ls_raw, const float* eps, float* a, float* logp, hipStream_t st) {
  JH_LAUNCH(jh_sac_sample_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, B, A, ld, mu_raw, ls_raw, eps, a, logp);
  JH_LAUNCH_CHECK();
  return JH_OK;
}
static int sac_actor_seed(int B, int qstride, int gstride, const float* q, const float* logp, float* dq, float* blk, float* stats, hipStream_t st) {
  JH_LAUNCH(jh_sac_actor_seed_kernel, dim3(1), dim3(256), 0, st, B, qstride, gstride, q, logp, dq, blk, stats);
  JH_LAUNCH_CHECK();
  return JH_OK;
}
static int sac_sample_bwd(int64_t n, int A, int ld, const float* da1, const float* da2, const float* mu_raw, const float* ls_raw, const float* eps, const float* a,
                          const float* blk, float* dmu, float* dls, hipStream_t st) {
  JH_LAUNCH(jh_sac_sample_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, A, ld, da1, da2, mu_raw, ls_raw, eps, a, blk, dmu, dls);
  JH_LAUNCH_CHECK();
  return JH_OK;
}

static int sac_mu_std(int64_t n, int A, int ld, const float* raw, float* mu, float* std, hipStream_t st) {
  JH_LAUNCH(jh_sac_mu_std_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, A, ld, raw, mu, std);
  JH_LAUNCH_CHECK();
  return JH_OK;
}

}  // namespace

static_assert(SA_FLOATS == JH_SAC_ALPHA_FLOATS, "the alpha block of include/jorldy_hip.h");

// ---------------------------------------------------------------------------------- standalone entries
JH_EXPORT int jh_sac_sample(jh_ctx* ctx, int32_t B, int32_t A, const float* d_mu_raw, const float* d_ls_raw, const float* d_eps, float* d_a, float* d_logp,
                            jh_stream stream) {
  JH_ARG(ctx && d_mu_raw && d_a);
  JH_ARG(d_eps == nullptr || (d_ls_raw && d_logp));
  JH_ARG(B > 0 && A > 0 && (int64_t)B * A < ((int64_t)1 << 31));
  return sac_sample(B, A, A, d_mu_raw, d_ls_raw, d_eps, d_a, d_logp, jh_s(stream));
}
JH_EXPORT int jh_sac_critic_loss(jh_ctx* ctx, int32_t B, const float* d_q, const float* d_q_next, const float* d_logp_next, const float* d_reward, const float* d_done,
                                 float gamma, const float* d_alpha, float* d_y, float* d_grad, float* d_stats, jh_stream stream) {
  JH_ARG(ctx && d_q && d_q_next && d_logp_next && d_reward && d_done && d_alpha && d_grad && d_stats);
  JH_ARG(B > 0 && B <= kMaxLossRows && ((uintptr_t)d_alpha & 7) == 0);
  CriticLossArgs a{d_reward, d_done, gamma, d_y, d_stats, d_logp_next, d_alpha + SA_IN_USE, B, 2, B, d_q, d_q_next, d_grad};
  return ac_critic_loss(a, jh_s(stream));
}
JH_EXPORT int jh_sac_actor_seed(jh_ctx* ctx, int32_t B, const float* d_q, const float* d_logp, float* d_alpha, float* d_grad_q, float* d_stats, jh_stream stream) {
  JH_ARG(ctx && d_q && d_logp && d_alpha && d_grad_q && d_stats);
  JH_ARG(B > 0 && B <= kMaxLossRows && ((uintptr_t)d_alpha & 7) == 0);
  return sac_actor_seed(B, B, B, d_q, d_logp, d_grad_q, d_alpha, d_stats, jh_s(stream));
}
JH_EXPORT int jh_sac_sample_backward(jh_ctx* ctx, int32_t B, int32_t A, const float* d_grad_a, const float* d_grad_a2, const float* d_mu_raw, const float* d_ls_raw,
                                     const float* d_eps, const float* d_a, const float* d_alpha, float* d_grad_mu_raw, float* d_grad_ls_raw, jh_stream stream) {
  JH_ARG(ctx && d_grad_a && d_mu_raw && d_ls_raw && d_eps && d_a && d_alpha && d_grad_mu_raw && d_grad_ls_raw);
  JH_ARG(B > 0 && A > 0 && (int64_t)B * A < ((int64_t)1 << 31));
  return sac_sample_bwd((int64_t)B * A, A, A, d_grad_a, d_grad_a2, d_mu_raw, d_ls_raw, d_eps, d_a, d_alpha, d_grad_mu_raw, d_grad_ls_raw, jh_s(stream));
}

// ---------------------------------------------------------------------------------- the network object
// A Gaussian policy (policy.py:38-55: head.l -> relu(l) -> (mu, log_std)), online only, and two continuous Q networks with their targets
// (sac.py:75-95).  jh_sacnet embeds a jh_acnet (two critics, no target actor, a head of 2A columns) and drives jh_acnet.hip's pieces with it.
// mu and log_std are ONE [2A][H] layer in the actor's bucket -- mu.weight, log_std.weight, then mu.bias, log_std.bias, back to back --, so a
// row of its output is [mu_raw | ls_raw] and the way back into relu(l) is one contraction over 2A; jh_sacnet_segment reports the four
// tensors in the reference's state_dict order.
enum { SAC_A_WMU = 4, SAC_A_BMU, SAC_A_WLS, SAC_A_BLS, SAC_C_FIRST, SAC_SEG_COUNT = SAC_C_FIRST + 8 };

struct jh_sacnet {
  jh_acnet ac;              // at == nullptr; AC_A_WPI / AC_A_BPI are the [2A][H] layer and its [2A] bias; a_z = [mu_raw | ls_raw], dz its gradient
  float* logp = nullptr;    // [maxB]
  float* da2 = nullptr;     // critic 2's d(action) [maxB][A] (critic 1's: ac.da)
  float* alpha = nullptr;   // the temperature block
};

JH_EXPORT int jh_sacnet_param_counts_for(int32_t S, int32_t H, int32_t A, int64_t* actor_floats, int64_t* critic_floats) {
  JH_ARG(actor_floats && critic_floats);
  jh_acnet tmp;
  int rc = ac_layout(&tmp, S, H, A, 2 * A, 2, 1);
  if (rc) return rc;
  *actor_floats = tmp.nA;
  *critic_floats = tmp.nC;
  return JH_OK;
}

static int sac_init(jh_sacnet* s) {
  jh_acnet* n = &s->ac;
  int rc = core_alloc(&n->core, "jh_acnet", (void**)&s->logp, sizeof(float) * n->maxB, true);
  if (!rc) rc = core_alloc(&n->core, "jh_acnet", (void**)&s->da2, sizeof(float) * n->maxB * n->A, true);
  if (!rc) rc = core_alloc(&n->core, "jh_acnet", (void**)&s->alpha, sizeof(float) * SA_FLOATS, true);
  if (rc) return rc;
  float al[SA_FLOATS] = {0.f};
  const double b1 = 0.9, b2 = 0.999;
  al[SA_IN_USE] = 1.f; al[SA_LR] = 3e-4f; al[SA_EPS] = 1e-8f; al[SA_TARGET_ENTROPY] = -(float)n->A;
  memcpy(al + SA_B1D, &b1, 8); memcpy(al + SA_B2D, &b2, 8);
  JH_HIP(hipMemcpy(s->alpha, al, sizeof(al), hipMemcpyHostToDevice));
  JH_HIP(hipDeviceSynchronize());
  return JH_OK;
}

JH_EXPORT int jh_sacnet_create(jh_ctx* ctx, int32_t S, int32_t H, int32_t A, int32_t max_batch, float* d_actor, float* d_actor_grads, float* d_actor_m,
                               float* d_actor_v, float* d_critics, float* d_critics_target, float* d_critics_grads, float* d_critics_m, float* d_critics_v,
                               jh_sacnet** out) {
  JH_ARG(ctx && out && d_actor && d_actor_grads && d_actor_m && d_actor_v);
  JH_ARG(d_critics && d_critics_target && d_critics_grads && d_critics_m && d_critics_v);
  float* const actor[5] = {d_actor, nullptr, d_actor_grads, d_actor_m, d_actor_v};
  float* const critics[5] = {d_critics, d_critics_target, d_critics_grads, d_critics_m, d_critics_v};
  jh_sacnet* s = new jh_sacnet();
  int rc = ac_init(&s->ac, ctx, S, H, A, 2 * A, 2, max_batch, actor, critics);
  if (!rc) rc = sac_init(s);
  if (rc) {
    core_release(&s->ac.core);
    delete s;
    return rc;
  }
  *out = s;
  return JH_OK;
}

JH_EXPORT void jh_sacnet_destroy(jh_sacnet* s) {
  if (!s) return;
  core_release(&s->ac.core);
  delete s;
}

JH_EXPORT int32_t jh_sacnet_segment_count(void) { return SAC_SEG_COUNT; }
// segments 0-7 of the actor bucket in the reference's state_dict order, 8-15 of one critic (offsets relative to that critic)
JH_EXPORT int jh_sacnet_segment(const jh_sacnet* s, int32_t i, int64_t* offset, int32_t* rows, int32_t* cols) {
  JH_ARG(s && i >= 0 && i < SAC_SEG_COUNT && offset && rows && cols);
  const jh_acnet* n = &s->ac;
  const int A = n->A, H = n->H;
  if (i < SAC_A_WMU || i >= SAC_C_FIRST) {
    return seg_query(n, AC_SEG_COUNT, i < SAC_A_WMU ? i : AC_C_W1 + (i - SAC_C_FIRST), offset, rows, cols);
  }
  const bool weight = i == SAC_A_WMU || i == SAC_A_WLS, second = i >= SAC_A_WLS;
  *offset = weight ? n->seg_off[AC_A_WPI] + (second ? (int64_t)A * H : 0) : n->seg_off[AC_A_BPI] + (second ? A : 0);
  *rows = weight ? A : 1;
  *cols = weight ? H : A;
  return JH_OK;
}

// The entries the embedded jh_acnet answers (jh_acnet.hip).  which: 0 the actor's Adam, 1 the critics'; there is no target actor, so the
// target sync and update_target_soft (sac.py:271-275) move the two target critics alone.
JH_EXPORT int jh_sacnet_set_hyper(jh_sacnet* s, int32_t which, double lr, double beta1, double beta2, double eps, int64_t step, jh_stream stream) {
  JH_ARG(s != nullptr);
  return jh_acnet_set_hyper(&s->ac, which, lr, beta1, beta2, eps, step, stream);
}
JH_EXPORT int jh_sacnet_set_lr(jh_sacnet* s, int32_t which, double lr, jh_stream stream) {
  JH_ARG(s != nullptr);
  return jh_acnet_set_lr(&s->ac, which, lr, stream);
}
JH_EXPORT int jh_sacnet_sync_target(jh_sacnet* s, jh_stream stream) {
  JH_ARG(s != nullptr);
  return jh_acnet_sync_target(&s->ac, stream);
}
JH_EXPORT int jh_sacnet_soft_update(jh_sacnet* s, double tau, jh_stream stream) {
  JH_ARG(s != nullptr);
  return jh_acnet_soft_update(&s->ac, tau, stream);
}
// critic_c(x, action) for both critics -> d_q [2][rows]; which 0 online / 1 target
JH_EXPORT int jh_sacnet_critic_forward(jh_sacnet* s, int32_t which, const float* d_x, const float* d_action, int32_t rows, float* d_q, jh_stream stream) {
  JH_ARG(s != nullptr);
  return jh_acnet_critic_forward(&s->ac, which, d_x, d_action, rows, d_q, stream);
}
// The whole temperature block.  Synchronous (checkpoints and construction): not for a captured stream.
JH_EXPORT int jh_sacnet_set_alpha(jh_sacnet* s, double log_alpha, double alpha, double lr, double beta1, double beta2, double eps, int64_t step, double m, double v,
                                  int32_t dynamic, jh_stream stream) {
  JH_ARG(s && alpha > 0.0 && lr >= 0.0 && step >= 0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0);
  float al[SA_FLOATS] = {0.f};
  al[SA_LOG_ALPHA] = (float)log_alpha; al[SA_IN_USE] = (float)alpha; al[SA_M] = (float)m; al[SA_V] = (float)v; al[SA_STEP] = (float)step;
  al[SA_LR] = (float)lr; al[SA_EPS] = (float)eps; al[SA_DYNAMIC] = dynamic ? 1.f : 0.f; al[SA_TARGET_ENTROPY] = -(float)s->ac.A;
  memcpy(al + SA_B1D, &beta1, 8); memcpy(al + SA_B2D, &beta2, 8);
  JH_HIP(hipStreamSynchronize(jh_s(stream)));
  JH_HIP(hipMemcpy(s->alpha, al, sizeof(al), hipMemcpyHostToDevice));
  return JH_OK;
}
// -> h_block: JH_SAC_ALPHA_FLOATS floats of host memory.  Synchronous.
JH_EXPORT int jh_sacnet_get_alpha(jh_sacnet* s, float* h_block, jh_stream stream) {
  JH_ARG(s && h_block);
  JH_HIP(hipStreamSynchronize(jh_s(stream)));
  JH_HIP(hipMemcpy(h_block, s->alpha, sizeof(float) * SA_FLOATS, hipMemcpyDeviceToHost));
  return JH_OK;
}

// actor(x) -> d_mu, d_std [rows][A]   (policy.py:38-55; sac.py:148)
JH_EXPORT int jh_sacnet_actor_forward(jh_sacnet* s, const float* d_x, int32_t rows, float* d_mu, float* d_std, jh_stream stream) {
  JH_ARG(s && d_x && d_mu && d_std);
  jh_acnet* n = &s->ac;
  JH_ARG(rows > 0 && rows <= n->maxB);
  int rc = ac_actor_forward(n, n->ap, d_x, rows, jh_s(stream));
  return rc ? rc : sac_mu_std((int64_t)rows * n->A, n->A, 2 * n->A, n->a_z, d_mu, d_std, jh_s(stream));
}

// The critic update of learn() (sac.py:183-225).  d_x = [state; next_state] (2B rows), d_eps [B][A] standard normals: a', logp' come from the
// ONLINE actor on next_state, which rides in the three grouped levels where TD3's target actor rides.
// -> d_y [B], d_q [2][B], d_a_next [B][A], d_logp_next [B] (all optional), d_stats {loss_1, loss_2, max_Q, mark}; the critics have taken
// their Adam step on return.
// Launches: 3 grouped GEMMs (ac_critic_front, the online actor riding along) + sample + 3 grouped GEMMs, loss, 3 grouped GEMMs of the backward
// and Adam (ac_critic_back) = 12.
JH_EXPORT int jh_sacnet_critic_update(jh_sacnet* s, const float* d_x, const float* d_action, const float* d_reward, const float* d_done, const float* d_eps,
                                      int32_t B, float gamma, float* d_y, float* d_q, float* d_a_next, float* d_logp_next, float* d_stats, jh_stream stream) {
  JH_ARG(s && d_x && d_action && d_reward && d_done && d_eps && d_stats);
  jh_acnet* n = &s->ac;
  JH_ARG(B > 0 && B <= n->maxB);
  hipStream_t st = jh_s(stream);
  const int A = n->A;
  float* a_next = d_a_next ? d_a_next : n->a_out;
  float* lp_next = d_logp_next ? d_logp_next : s->logp;
  int rc;
  if ((rc = ac_critic_front(n, n->ap, d_x, d_action, B, st))) return rc;
  if ((rc = sac_sample(B, A, 2 * A, n->a_z, n->a_z + A, d_eps, a_next, lp_next, st))) return rc;
  CriticLossArgs loss{d_reward, d_done, gamma, d_y, d_stats, lp_next, s->alpha + SA_IN_USE};
  return ac_critic_back(n, d_x, d_action, B, a_next, d_q ? d_q : n->c_q[0], loss, st);
}

// The actor update of learn() (sac.py:229-255): a, logp = sample(actor(state), eps), q_i = critic_i(state, a) with the critics AFTER their step,
// actor_loss = -mean(alpha * (-logp) + min(q_1, q_2)); backward through BOTH critics' action inputs and through logp into the actor; the
// actor's Adam step; the temperature's bookkeeping rides in the seed.  The critics' parameters, gradient bucket and moments are not written.
// -> d_action [B][A], d_logp [B], d_q [2][B] (all optional), d_stats as jh_sac_actor_seed.
// Launches: 3 GEMMs (ac_actor_trunk, both critics' heads in the first) + sample + 3 GEMMs (ac_actor_q) + seed (+ temperature) + 3 GEMMs back
// through the critics (ac_actor_dact) + sample backward + 3 GEMMs of the actor's backward and Adam (ac_actor_backward) = 16.
JH_EXPORT int jh_sacnet_actor_update(jh_sacnet* s, const float* d_x, const float* d_eps, int32_t B, float* d_action, float* d_logp, float* d_q, float* d_stats,
                                     jh_stream stream) {
  JH_ARG(s && d_x && d_eps && d_stats);
  jh_acnet* n = &s->ac;
  JH_ARG(B > 0 && B <= n->maxB);
  hipStream_t st = jh_s(stream);
  const int A = n->A;
  float* a_out = d_action ? d_action : n->a_out;
  float* logp = d_logp ? d_logp : s->logp;
  float* q = d_q ? d_q : n->c_q[0];  // [2][B], packed
  int rc;
  if ((rc = ac_actor_trunk(n, d_x, B, 2, st))) return rc;
  if ((rc = sac_sample(B, A, 2 * A, n->a_z, n->a_z + A, d_eps, a_out, logp, st))) return rc;
  if ((rc = ac_actor_q(n, a_out, B, 2, q, st))) return rc;
  if ((rc = sac_actor_seed(B, B, n->maxB, q, logp, n->dq, s->alpha, d_stats, st))) return rc;
  if ((rc = ac_actor_dact(n, B, 2, s->da2, st))) return rc;
  if ((rc = sac_sample_bwd((int64_t)B * A, A, 2 * A, n->da, s->da2, n->a_z, n->a_z + A, d_eps, a_out, s->alpha, n->dz, n->dz + A, st))) return rc;
  return ac_actor_backward(n, d_x, B, st);
}
