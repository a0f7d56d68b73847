// Deterministic actor-critic (core/agent/td3.py:146-209, core/agent/ddpg.py:117-163) on the device:
//   jh_acnet_*   an actor (network/policy.py:8-20: head.l -> relu(l) -> tanh(pi)) and one or two critics (network/q_network.py:23-39:
//                [head.l(s) | relu(e(a))] -> relu(l) -> q), each with a target copy; the critic update (target pass, online pass, loss,
//                backward, Adam), the actor update (backward through critic 1's ACTION input into the actor, the actor's Adam; critic 1's
//                parameters, gradients and moments are not written), the soft target update and the target sync.
// The object's core, the critic loss, the Polyak average and the pieces of the two updates are jh_acnet.hip's, shared with jh_sac.hip.  The
// kernels of this file are the elementwise steps that are TD3's own: the (noisy, clipped) tanh action, the actor's loss seed, the way back
// through tanh.
// No floating-point atomics: every sum has a fixed order, so two runs (and a graph replay) give the same bits.
#include "jh_acnet.h"

namespace {

// ---------------------------------------------------------------------------------- next action
// a = clamp(tanh(z) + clamp(std * eps, -c, c), -1, 1)   (td3.py:159-162); eps == nullptr: a = tanh(z)   (policy.py:20, ddpg.py:130)
__global__ void __launch_bounds__(256) jh_td3_next_action_kernel(int64_t n, const float* __restrict__ z, const float* __restrict__ eps, float std, float c,
                                                                 float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float a = tanhf(z[i]);
  if (eps) {
    const float nz = fminf(fmaxf(eps[i] * std, -c), c);
    a = fminf(fmaxf(a + nz, -1.f), 1.f);
  }
  out[i] = a;
}

// ---------------------------------------------------------------------------------- actor seed
// actor_loss = -mean_b q1(s, actor(s)) and its constant gradient d(actor_loss)/d(q1[b]) = -1 / B   (td3.py:183, ddpg.py:144).
// stats = {actor_loss, arrival mark}.
__global__ void __launch_bounds__(256) jh_td3_actor_seed_kernel(int B, const float* __restrict__ q, float* __restrict__ dq, float* stats) {
  __shared__ float s_red[16];
  float s = 0.f;
  const float g = -1.f / (float)B;
  for (int b = threadIdx.x; b < B; b += 256) {
    s += q[b];
    dq[b] = g;
  }
  const float t = jh_block_reduce(s, s_red, JhAdd(), 0.f);
  if (threadIdx.x == 0 && stats) {
    stats[0] = -(t / (float)B);
    __threadfence_system();
    stats[1] = 0.f;
  }
}
// the way back through a = tanh(z): dz = da * (1 - a^2)
__global__ void __launch_bounds__(256) jh_td3_tanh_bwd_kernel(int64_t n, const float* __restrict__ da, const float* __restrict__ a, float* __restrict__ dz) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float v = a[i];
  dz[i] = da[i] * (1.f - v * v);
}

static int td3_next_action(int64_t n, const float* z, const float* eps, float std, float c, float* out, hipStream_t st) {
  JH_LAUNCH(jh_td3_next_action_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, z, eps, std, c, out);
  JH_LAUNCH_CHECK();
  return JH_OK;
}
static int td3_actor_seed(int B, const float* q, float* dq, float* stats, hipStream_t st) {
  JH_LAUNCH(jh_td3_actor_seed_kernel, dim3(1), dim3(256), 0, st, B, q, dq, stats);
  JH_LAUNCH_CHECK();
  return JH_OK;
}
static int td3_tanh_bwd(int64_t n, const float* da, const float* a, float* dz, hipStream_t st) {
  JH_LAUNCH(jh_td3_tanh_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, da, a, dz);
  JH_LAUNCH_CHECK();
  return JH_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------- standalone entries
JH_EXPORT int jh_td3_next_action(jh_ctx* ctx, int32_t B, int32_t A, const float* d_z, const float* d_eps, float noise_std, float noise_clip, float* d_out,
                                 jh_stream stream) {
  JH_ARG(ctx && d_z && d_out);
  JH_ARG(B > 0 && A > 0 && (int64_t)B * A < ((int64_t)1 << 31) && noise_clip >= 0.f);
  return td3_next_action((int64_t)B * A, d_z, d_eps, noise_std, noise_clip, d_out, jh_s(stream));
}
JH_EXPORT int jh_td3_critic_loss(jh_ctx* ctx, int32_t B, int32_t n_critics, const float* d_q, const float* d_q_next, const float* d_reward, const float* d_done,
                                 float gamma, float* d_y, float* d_grad, float* d_stats, jh_stream stream) {
  JH_ARG(ctx && d_q && d_q_next && d_reward && d_done && d_grad && d_stats);
  JH_ARG(B > 0 && B <= kMaxLossRows && (n_critics == 1 || n_critics == 2));
  CriticLossArgs a{d_reward, d_done, gamma, d_y, d_stats, nullptr, nullptr, B, n_critics, B, d_q, d_q_next, d_grad};
  return ac_critic_loss(a, jh_s(stream));
}
JH_EXPORT int jh_td3_actor_seed(jh_ctx* ctx, int32_t B, const float* d_q, float* d_grad_q, float* d_stats, jh_stream stream) {
  JH_ARG(ctx && d_q && d_grad_q && d_stats);
  JH_ARG(B > 0 && B <= kMaxLossRows);
  return td3_actor_seed(B, d_q, d_grad_q, d_stats, jh_s(stream));
}
JH_EXPORT int jh_td3_tanh_backward(jh_ctx* ctx, int32_t B, int32_t A, const float* d_grad_a, const float* d_a, float* d_grad_z, jh_stream stream) {
  JH_ARG(ctx && d_grad_a && d_a && d_grad_z);
  JH_ARG(B > 0 && A > 0 && (int64_t)B * A < ((int64_t)1 << 31));
  return td3_tanh_bwd((int64_t)B * A, d_grad_a, d_a, d_grad_z, jh_s(stream));
}
JH_EXPORT int jh_td3_polyak(jh_ctx* ctx, int64_t n, const float* d_params, float* d_target, double tau, jh_stream stream) {
  JH_ARG(ctx && d_params && d_target);
  JH_ARG(n > 0 && n < ((int64_t)1 << 38) && tau >= 0.0 && tau <= 1.0);
  return ac_polyak(n, d_params, d_target, tau, jh_s(stream));
}

// ---------------------------------------------------------------------------------- the network object
// (the object's core and the entries jh_sacnet shares -- set_hyper, set_lr, sync_target, soft_update, critic_forward --: jh_acnet.hip)
JH_EXPORT int jh_acnet_param_counts_for(int32_t S, int32_t H, int32_t A, int64_t* actor_floats, int64_t* critic_floats) {
  JH_ARG(actor_floats && critic_floats);
  jh_acnet tmp;
  int rc = ac_layout(&tmp, S, H, A, A, 1, 1);
  if (rc) return rc;
  *actor_floats = tmp.nA;
  *critic_floats = tmp.nC;
  return JH_OK;
}

JH_EXPORT int jh_acnet_create(jh_ctx* ctx, int32_t S, int32_t H, int32_t A, int32_t n_critics, int32_t max_batch, float* d_actor, float* d_actor_target,
                              float* d_actor_grads, float* d_actor_m, float* d_actor_v, float* d_critics, float* d_critics_target, float* d_critics_grads,
                              float* d_critics_m, float* d_critics_v, jh_acnet** out) {
  JH_ARG(ctx && out && d_actor && d_actor_target && d_actor_grads && d_actor_m && d_actor_v);
  JH_ARG(d_critics && d_critics_target && d_critics_grads && d_critics_m && d_critics_v);
  float* const actor[5] = {d_actor, d_actor_target, d_actor_grads, d_actor_m, d_actor_v};
  float* const critics[5] = {d_critics, d_critics_target, d_critics_grads, d_critics_m, d_critics_v};
  jh_acnet* n = new jh_acnet();
  int rc = ac_init(n, ctx, S, H, A, A, n_critics, max_batch, actor, critics);
  if (rc) {
    core_release(&n->core);
    delete n;
    return rc;
  }
  *out = n;
  return JH_OK;
}

JH_EXPORT void jh_acnet_destroy(jh_acnet* n) {
  if (!n) return;
  core_release(&n->core);
  delete n;
}

JH_EXPORT int32_t jh_acnet_segment_count(void) { return AC_SEG_COUNT; }
JH_EXPORT int jh_acnet_segment(const jh_acnet* n, int32_t i, int64_t* offset, int32_t* rows, int32_t* cols) {
  return seg_query(n, AC_SEG_COUNT, i, offset, rows, cols);
}

// actor(x) -> d_action [rows][A]; which 0 online / 1 target.  This is what acting uses.
JH_EXPORT int jh_acnet_actor_forward(jh_acnet* n, int32_t which, const float* d_x, int32_t rows, float* d_action, jh_stream stream) {
  JH_ARG(n && d_x && d_action);
  JH_ARG(rows > 0 && rows <= n->maxB && (which == 0 || which == 1));
  int rc = ac_actor_forward(n, which == 0 ? n->ap : n->at, d_x, rows, jh_s(stream));
  return rc ? rc : td3_next_action((int64_t)rows * n->A, n->a_z, nullptr, 0.f, 0.f, d_action, jh_s(stream));
}

// The critic update of learn() (td3.py:157-178, ddpg.py:128-140).  d_x = [state; next_state] (2B rows), d_noise [B][A] standard normals or
// NULL (no target noise: DDPG).  -> d_y [B] (optional), d_q [n_critics][B] (optional: the online critics' outputs), d_stats
// {loss_1, loss_2, max_Q, mark}; the critics' parameters have taken their Adam step on return.
// Launches: 3 grouped GEMMs (ac_critic_front, the target actor riding along) + next action + 3 grouped GEMMs, loss, 3 grouped GEMMs of the
// backward and Adam (ac_critic_back) = 12.
JH_EXPORT int jh_acnet_critic_update(jh_acnet* n, const float* d_x, const float* d_action, const float* d_reward, const float* d_done, const float* d_noise,
                                     int32_t B, float gamma, float noise_std, float noise_clip, float* d_y, float* d_q, float* d_stats, jh_stream stream) {
  JH_ARG(n && d_x && d_action && d_reward && d_done && d_stats);
  JH_ARG(B > 0 && B <= n->maxB && noise_clip >= 0.f);
  hipStream_t st = jh_s(stream);
  int rc;
  if ((rc = ac_critic_front(n, n->at, d_x, d_action, B, st))) return rc;
  if ((rc = td3_next_action((int64_t)B * n->A, n->a_z, d_noise, noise_std, noise_clip, n->a_out, st))) return rc;
  CriticLossArgs loss{d_reward, d_done, gamma, d_y, d_stats, nullptr, nullptr};
  return ac_critic_back(n, d_x, d_action, B, n->a_out, d_q ? d_q : n->c_q[0], loss, st);
}

// The actor update of learn() (td3.py:181-188, ddpg.py:143-148): a = actor(s), q = critic_1(s, a), actor_loss = -mean(q), backward through
// critic 1's action input into the actor, the actor's Adam step.  Critic 1's parameters, gradient bucket and moments are not written.
// -> d_action_pred [B][A] (optional), d_stats {actor_loss, mark}.
// Launches: 3 GEMMs (ac_actor_trunk) + tanh + 3 GEMMs (ac_actor_q) + seed + 3 GEMMs back through the critic (ac_actor_dact) + tanh' + 3 GEMMs
// of the actor's backward and Adam (ac_actor_backward) = 16.
JH_EXPORT int jh_acnet_actor_update(jh_acnet* n, const float* d_x, int32_t B, float* d_action_pred, float* d_stats, jh_stream stream) {
  JH_ARG(n && d_x && d_stats);
  JH_ARG(B > 0 && B <= n->maxB);
  hipStream_t st = jh_s(stream);
  float* a_out = d_action_pred ? d_action_pred : n->a_out;
  int rc;
  if ((rc = ac_actor_trunk(n, d_x, B, 1, st))) return rc;
  if ((rc = td3_next_action((int64_t)B * n->A, n->a_z, nullptr, 0.f, 0.f, a_out, st))) return rc;
  if ((rc = ac_actor_q(n, a_out, B, 1, n->c_q[0], st))) return rc;
  if ((rc = td3_actor_seed(B, n->c_q[0], n->dq, d_stats, st))) return rc;
  if ((rc = ac_actor_dact(n, B, 1, nullptr, st))) return rc;
  if ((rc = td3_tanh_bwd((int64_t)B * n->A, n->da, a_out, n->dz, st))) return rc;
  return ac_actor_backward(n, d_x, B, st);
}
