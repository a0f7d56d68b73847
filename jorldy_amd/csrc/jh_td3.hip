// Deterministic actor-critic (core/agent/td3.py:146-209, core/agent/ddpg.py:117-163) on the device:
//   jh_acnet_*   an actor (network/policy.py:8-20: head.l -> relu(l) -> tanh(pi)) and one or two critics (network/q_network.py:23-39:
//                [head.l(s) | relu(e(a))] -> relu(l) -> q), each with a target copy; the critic update (target pass, online pass, loss,
//                backward, Adam), the actor update (backward through critic 1's ACTION input into the actor, the actor's Adam; critic 1's
//                parameters, gradients and moments are not written), the soft target update and the target sync.
// Every dense contraction runs on the tile engine (jh_tgemm.hip) under the call-site name "dense", independent layers sharing a grouped
// launch.  The kernels of this file are the elementwise steps between them: the (noisy, clipped) tanh action, the critic loss with its
// gradient and statistics, the actor's loss seed, the way back through tanh, and the Polyak average.
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

// ---------------------------------------------------------------------------------- critic loss
// y = r + (1 - d) * gamma * min_i q_i'(s', a'), loss_i = mean((y - q_i)^2), d(loss_i)/d(q_i) = 2 (q_i - y) / B, max_Q = max_b y
// (td3.py:163-178, ddpg.py:131-140).  One workgroup: thread t walks b = t, t + 256, ... in ascending order, the block reduction has a
// fixed tree.  stats = {loss_1, loss_2 (0 for one critic), max_Q, arrival mark}.
struct CriticLossArgs {
  int B, n, gstride;                    // grad of critic c starts at c * gstride
  const float *q, *qn, *reward, *done;  // q, qn: [n][B]
  float gamma;
  float *y, *grad, *stats;              // y [B] (optional), grad [n][B]
};
__global__ void __launch_bounds__(256) jh_td3_critic_loss_kernel(CriticLossArgs a) {
  __shared__ float s_red[16];
  float l0 = 0.f, l1 = 0.f, my = -3.4e38f;
  const float inv = 2.f / (float)a.B;
  for (int b = threadIdx.x; b < a.B; b += 256) {
    float mn = a.qn[b];
    if (a.n == 2) mn = fminf(mn, a.qn[a.B + b]);
    const float y = a.reward[b] + (1.f - a.done[b]) * a.gamma * mn;
    if (a.y) a.y[b] = y;
    my = fmaxf(my, y);
    const float d0 = a.q[b] - y;
    l0 += d0 * d0;
    a.grad[b] = d0 * inv;
    if (a.n == 2) {
      const float d1 = a.q[a.B + b] - y;
      l1 += d1 * d1;
      a.grad[a.gstride + b] = d1 * inv;
    }
  }
  const float s0 = jh_block_reduce(l0, s_red, JhAdd(), 0.f);
  const float s1 = jh_block_reduce(l1, s_red, JhAdd(), 0.f);
  const float m = jh_block_reduce(my, s_red, JhMax(), -3.4e38f);
  if (threadIdx.x == 0 && a.stats) {
    a.stats[0] = s0 / (float)a.B;
    a.stats[1] = s1 / (float)a.B;
    a.stats[2] = m;
    __threadfence_system();  // payload before the arrival mark (mapped host memory, jh_host_wait_marks)
    a.stats[3] = 0.f;
  }
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

// ---------------------------------------------------------------------------------- Polyak average
// t <- tau * p + (1 - tau) * t   (td3.py:203-209) as torch evaluates it on float32 tensors: the Python scalars tau and (1 - tau) -- the
// latter formed in DOUBLE -- are rounded to float32, then two float32 products and one float32 sum (the build has -ffp-contract=off).
__global__ void __launch_bounds__(256) jh_td3_polyak_kernel(int64_t n, const float* __restrict__ p, float* __restrict__ t, float tau, float omt) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float a = tau * p[i];
  const float b = omt * t[i];
  t[i] = a + b;
}

static int td3_next_action(int64_t n, const float* z, const float* eps, float std, float c, float* out, hipStream_t st) {
  JH_LAUNCH(jh_td3_next_action_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, z, eps, std, c, out);
  JH_LAUNCH_CHECK();
  return JH_OK;
}
static int td3_critic_loss(const CriticLossArgs& a, hipStream_t st) {
  JH_LAUNCH(jh_td3_critic_loss_kernel, dim3(1), dim3(256), 0, st, a);
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
static int td3_polyak(int64_t n, const float* p, float* t, double tau, hipStream_t st) {
  JH_LAUNCH(jh_td3_polyak_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, p, t, (float)tau, (float)(1.0 - tau));
  JH_LAUNCH_CHECK();
  return JH_OK;
}

constexpr int kMaxLossRows = 1 << 20;

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
  CriticLossArgs a{B, n_critics, B, d_q, d_q_next, d_reward, d_done, gamma, d_y, d_grad, d_stats};
  return td3_critic_loss(a, jh_s(stream));
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
  return td3_polyak(n, d_params, d_target, tau, jh_s(stream));
}

// ---------------------------------------------------------------------------------- the network object
// (the object, its layout, the layer builders and the critics' backward: jh_acnet.h, shared with jh_sac.hip)
JH_EXPORT int jh_acnet_param_counts_for(int32_t S, int32_t H, int32_t A, int64_t* actor_floats, int64_t* critic_floats) {
  JH_ARG(actor_floats && critic_floats);
  jh_acnet tmp;
  int rc = ac_layout(&tmp, S, H, A, 1, 1);
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
  JH_HIP(hipSetDevice(ctx->device));
  jh_acnet* n = new jh_acnet();
  n->ctx = ctx;
  int rc = ac_layout(n, S, H, A, n_critics, max_batch);
  if (rc) {
    delete n;
    return rc;
  }
  n->ap = d_actor; n->at = d_actor_target; n->ag = d_actor_grads; n->am = d_actor_m; n->av = d_actor_v;
  n->cp = d_critics; n->ct = d_critics_target; n->cg = d_critics_grads; n->cm = d_critics_m; n->cv = d_critics_v;
  const size_t B = (size_t)max_batch, NB = (size_t)n_critics * B;
  auto A4 = [&](float** p, size_t floats, bool zero = true) { if (!rc) rc = ac_alloc(n, (void**)p, floats * sizeof(float), zero); };
  A4(&n->hyper_a, JH_HY_FLOATS); A4(&n->hyper_c, JH_HY_FLOATS);
  A4(&n->norm_partial, 256);
  if (!rc) rc = ac_alloc(n, (void**)&n->ticket_a, 2048, true);  // jh_rb_optim_kernel: eight counters 128 bytes apart + the one on top of them
  if (!rc) rc = ac_alloc(n, (void**)&n->ticket_c, 2048, true);
  A4(&n->a_feat, B * H); A4(&n->a_h, B * H); A4(&n->a_z, B * A); A4(&n->a_out, B * A);
  for (int s = 0; s < 2; ++s) {
    A4(&n->c_cat[s], NB * 2 * H); A4(&n->c_h[s], NB * H); A4(&n->c_q[s], NB);
  }
  A4(&n->dq, NB); A4(&n->dh, NB * H); A4(&n->dcat, NB * 2 * H); A4(&n->da, B * A); A4(&n->dz, B * A); A4(&n->dah, B * H); A4(&n->dafeat, B * H);
  n->ws_floats = (size_t)8 << 20;  // 32 MB of split-K partials
  A4(&n->ws, n->ws_floats, false);
  n->cnt_slots = 8192;
  if (!rc) rc = ac_alloc(n, (void**)&n->cnt, sizeof(unsigned) * (size_t)n->cnt_slots * kTgemmCntStride, true);
  if (rc) {
    for (void* p : n->owned) (void)hipFree(p);
    delete n;
    return rc;
  }
  float hy[JH_HY_FLOATS];
  jh_hyper_fill(hy, 1e-3, 0.9, 0.999, 1e-8, 0.0);
  auto init = [&]() -> int {
    JH_HIP(hipMemcpy(n->hyper_a, hy, sizeof(hy), hipMemcpyHostToDevice));
    JH_HIP(hipMemcpy(n->hyper_c, hy, sizeof(hy), hipMemcpyHostToDevice));
    JH_HIP(hipDeviceSynchronize());
    return JH_OK;
  };
  if ((rc = init())) {
    for (void* p : n->owned) (void)hipFree(p);
    delete n;
    return rc;
  }
  *out = n;
  return JH_OK;
}

JH_EXPORT void jh_acnet_destroy(jh_acnet* n) {
  if (!n) return;
  (void)hipSetDevice(n->ctx->device);
  (void)hipDeviceSynchronize();
  for (void* p : n->owned) (void)hipFree(p);
  delete n;
}

JH_EXPORT int32_t jh_acnet_segment_count(void) { return AC_SEG_COUNT; }
JH_EXPORT int jh_acnet_segment(const jh_acnet* n, int32_t i, int64_t* offset, int32_t* rows, int32_t* cols) {
  JH_ARG(n && i >= 0 && i < AC_SEG_COUNT && offset && rows && cols);
  *offset = n->seg_off[i]; *rows = n->seg_rows[i]; *cols = n->seg_cols[i];
  return JH_OK;
}

// which: 0 the actor's optimizer, 1 the critics' (one block for both critics: td3.py:95-112 gives them the same settings)
JH_EXPORT int jh_acnet_set_hyper(jh_acnet* n, int32_t which, double lr, double beta1, double beta2, double eps, int64_t step, jh_stream stream) {
  JH_ARG(n && (which == 0 || which == 1));
  return jh_hyper_upload(n->ctx, which == 0 ? n->hyper_a : n->hyper_c, lr, beta1, beta2, eps, step, 0, jh_s(stream));
}
JH_EXPORT int jh_acnet_set_lr(jh_acnet* n, int32_t which, double lr, jh_stream stream) {
  JH_ARG(n && (which == 0 || which == 1));
  return jh_hyper_upload_lr(n->ctx, which == 0 ? n->hyper_a : n->hyper_c, lr, jh_s(stream));
}
JH_EXPORT int jh_acnet_sync_target(jh_acnet* n, jh_stream stream) {
  JH_ARG(n != nullptr);
  JH_HIP(hipMemcpyAsync(n->at, n->ap, sizeof(float) * (size_t)n->nA, hipMemcpyDeviceToDevice, jh_s(stream)));
  JH_HIP(hipMemcpyAsync(n->ct, n->cp, sizeof(float) * (size_t)n->nC * n->nc, hipMemcpyDeviceToDevice, jh_s(stream)));
  return JH_OK;
}
// update_target_soft (td3.py:203-209, ddpg.py:159-163): the critics' bucket, then the actor's
JH_EXPORT int jh_acnet_soft_update(jh_acnet* n, double tau, jh_stream stream) {
  JH_ARG(n && tau >= 0.0 && tau <= 1.0);
  int rc = td3_polyak(n->nC * n->nc, n->cp, n->ct, tau, jh_s(stream));
  return rc ? rc : td3_polyak(n->nA, n->ap, n->at, tau, jh_s(stream));
}

// actor(x) -> d_action [rows][A]; which 0 online / 1 target.  This is what acting uses.
JH_EXPORT int jh_acnet_actor_forward(jh_acnet* n, int32_t which, const float* d_x, int32_t rows, float* d_action, jh_stream stream) {
  JH_ARG(n && d_x && d_action);
  JH_ARG(rows > 0 && rows <= n->maxB && (which == 0 || which == 1));
  hipStream_t st = jh_s(stream);
  const float* P = which == 0 ? n->ap : n->at;
  TGemm g[1];
  int rc;
  g[0] = ac_head(n, P, AC_A_W1, AC_A_B1, d_x, rows, n->a_feat, n->H);
  if ((rc = ac_tgemm(n, g, 1, st))) return rc;
  g[0] = ac_a_l(n, P, rows);
  if ((rc = ac_tgemm(n, g, 1, st))) return rc;
  g[0] = ac_a_pi(n, P, rows);
  if ((rc = ac_tgemm(n, g, 1, st))) return rc;
  return td3_next_action((int64_t)rows * n->A, n->a_z, nullptr, 0.f, 0.f, d_action, st);
}

// critic_c(x, a) for every critic -> d_q [n_critics][rows]; which 0 online / 1 target
JH_EXPORT int jh_acnet_critic_forward(jh_acnet* n, int32_t which, const float* d_x, const float* d_action, int32_t rows, float* d_q, jh_stream stream) {
  JH_ARG(n && d_x && d_action && d_q);
  JH_ARG(rows > 0 && rows <= n->maxB && (which == 0 || which == 1));
  hipStream_t st = jh_s(stream);
  const float* base = which == 0 ? n->cp : n->ct;
  const int nc = n->nc;
  TGemm g[4];
  int rc;
  for (int c = 0; c < nc; ++c) {
    g[2 * c] = ac_c_head(n, base + c * n->nC, which, c, d_x, rows);
    g[2 * c + 1] = ac_c_embed(n, base + c * n->nC, which, c, d_action, rows);
  }
  if ((rc = ac_tgemm(n, g, 2 * nc, st))) return rc;
  for (int c = 0; c < nc; ++c) g[c] = ac_c_l(n, base + c * n->nC, which, c, rows);
  if ((rc = ac_tgemm(n, g, nc, st))) return rc;
  for (int c = 0; c < nc; ++c) g[c] = ac_c_q(n, base + c * n->nC, which, c, rows, d_q + (size_t)c * rows);
  return ac_tgemm(n, g, nc, st);
}

// The critic update of learn() (td3.py:157-178, ddpg.py:128-140).  d_x = [state; next_state] (2B rows), d_noise [B][A] standard normals or
// NULL (no target noise: DDPG).  -> d_y [B] (optional), d_q [n_critics][B] (optional: the online critics' outputs), d_stats
// {loss_1, loss_2, max_Q, mark}; the critics' parameters have taken their Adam step on return.
// Launches: 6 grouped GEMMs of the two forward passes + next action + loss + 3 grouped GEMMs of the backward + Adam = 12.
JH_EXPORT int jh_acnet_critic_update(jh_acnet* n, const float* d_x, const float* d_action, const float* d_reward, const float* d_done, const float* d_noise,
                                     int32_t B, float gamma, float noise_std, float noise_clip, float* d_y, float* d_q, float* d_stats, jh_stream stream) {
  JH_ARG(n && d_x && d_action && d_reward && d_done && d_stats);
  JH_ARG(B > 0 && B <= n->maxB && noise_clip >= 0.f);
  hipStream_t st = jh_s(stream);
  const int nc = n->nc, S = n->S;
  const float* xs = d_x;
  const float* xn = d_x + (size_t)B * S;
  float* q_on = d_q ? d_q : n->c_q[0];  // [nc][B], packed
  TGemm g[kMaxGroup];
  int k, rc;
  // 1: head.l of the target actor and the target critics on s', of the online critics on s
  k = 0;
  g[k++] = ac_head(n, n->at, AC_A_W1, AC_A_B1, xn, B, n->a_feat, n->H);
  for (int c = 0; c < nc; ++c) g[k++] = ac_c_head(n, n->ct + c * n->nC, 1, c, xn, B);
  for (int c = 0; c < nc; ++c) g[k++] = ac_c_head(n, n->cp + c * n->nC, 0, c, xs, B);
  if ((rc = ac_tgemm(n, g, k, st))) return rc;
  // 2: the target actor's l, the online critics' e(a)
  k = 0;
  g[k++] = ac_a_l(n, n->at, B);
  for (int c = 0; c < nc; ++c) g[k++] = ac_c_embed(n, n->cp + c * n->nC, 0, c, d_action, B);
  if ((rc = ac_tgemm(n, g, k, st))) return rc;
  // 3: the target actor's pi, the online critics' l
  k = 0;
  g[k++] = ac_a_pi(n, n->at, B);
  for (int c = 0; c < nc; ++c) g[k++] = ac_c_l(n, n->cp + c * n->nC, 0, c, B);
  if ((rc = ac_tgemm(n, g, k, st))) return rc;
  if ((rc = td3_next_action((int64_t)B * n->A, n->a_z, d_noise, noise_std, noise_clip, n->a_out, st))) return rc;
  // 4: the target critics' e(a'), the online critics' q
  k = 0;
  for (int c = 0; c < nc; ++c) g[k++] = ac_c_embed(n, n->ct + c * n->nC, 1, c, n->a_out, B);
  for (int c = 0; c < nc; ++c) g[k++] = ac_c_q(n, n->cp + c * n->nC, 0, c, B, q_on + (size_t)c * B);
  if ((rc = ac_tgemm(n, g, k, st))) return rc;
  // 5, 6: the target critics' l and q
  for (int c = 0; c < nc; ++c) g[c] = ac_c_l(n, n->ct + c * n->nC, 1, c, B);
  if ((rc = ac_tgemm(n, g, nc, st))) return rc;
  for (int c = 0; c < nc; ++c) g[c] = ac_c_q(n, n->ct + c * n->nC, 1, c, B, n->c_q[1] + (size_t)c * B);
  if ((rc = ac_tgemm(n, g, nc, st))) return rc;
  // loss: q and q' are packed [nc][B]; the gradient of critic c goes where the backward reads it, at c * maxB
  CriticLossArgs a{B, nc, n->maxB, q_on, n->c_q[1], d_reward, d_done, gamma, d_y, n->dq, d_stats};
  if ((rc = td3_critic_loss(a, st))) return rc;
  if ((rc = ac_critic_backward(n, B, xs, d_action, true, 0, nc, st))) return rc;
  return jh_flat_adam_step(n->nC * nc, n->cp, n->cg, n->cm, n->cv, n->hyper_c, n->ticket_c, n->norm_partial, 0.f, st);
}

// The actor update of learn() (td3.py:181-188, ddpg.py:143-148): a = actor(s), q = critic_1(s, a), actor_loss = -mean(q), backward through
// critic 1's action input into the actor, the actor's Adam step.  Critic 1's parameters, gradient bucket and moments are not written.
// -> d_action_pred [B][A] (optional), d_stats {actor_loss, mark}.
// Launches: 6 grouped GEMMs forward + tanh + seed + 3 GEMMs back through the critic + tanh' + 3 GEMMs of the actor's backward + Adam = 16.
JH_EXPORT int jh_acnet_actor_update(jh_acnet* n, const float* d_x, int32_t B, float* d_action_pred, float* d_stats, jh_stream stream) {
  JH_ARG(n && d_x && d_stats);
  JH_ARG(B > 0 && B <= n->maxB);
  hipStream_t st = jh_s(stream);
  const int H = n->H, S = n->S, A = n->A;
  const float* P = n->ap;
  const float* C1 = n->cp;
  float* G = n->ag;
  float* a_out = d_action_pred ? d_action_pred : n->a_out;
  TGemm g[2];
  int rc;
  g[0] = ac_head(n, P, AC_A_W1, AC_A_B1, d_x, B, n->a_feat, H);
  g[1] = ac_c_head(n, C1, 0, 0, d_x, B);
  if ((rc = ac_tgemm(n, g, 2, st))) return rc;
  g[0] = ac_a_l(n, P, B);
  if ((rc = ac_tgemm(n, g, 1, st))) return rc;
  g[0] = ac_a_pi(n, P, B);
  if ((rc = ac_tgemm(n, g, 1, st))) return rc;
  if ((rc = td3_next_action((int64_t)B * A, n->a_z, nullptr, 0.f, 0.f, a_out, st))) return rc;
  g[0] = ac_c_embed(n, C1, 0, 0, a_out, B);
  if ((rc = ac_tgemm(n, g, 1, st))) return rc;
  g[0] = ac_c_l(n, C1, 0, 0, B);
  if ((rc = ac_tgemm(n, g, 1, st))) return rc;
  g[0] = ac_c_q(n, C1, 0, 0, B, n->c_q[0]);
  if ((rc = ac_tgemm(n, g, 1, st))) return rc;
  if ((rc = td3_actor_seed(B, n->c_q[0], n->dq, d_stats, st))) return rc;
  // back through critic 1 to its action input: d(cat) -> da = d(cat)[:, H:] We
  if ((rc = ac_critic_backward(n, B, d_x, a_out, false, 0, 1, st))) return rc;
  g[0] = mk_gemm(B, A, H, op_dense(OP_KCONT, n->dcat + H, 2 * H), op_dense(OP_XCONT, C1 + n->seg_off[AC_C_WE], A), n->da, A, TEPI_NONE);
  if ((rc = ac_tgemm(n, g, 1, st))) return rc;
  if ((rc = td3_tanh_bwd((int64_t)B * A, n->da, a_out, n->dz, st))) return rc;
  // the actor's backward
  g[0] = mk_gemm(A, H, B, op_dense(OP_XCONT, n->dz, A), op_dense(OP_XCONT, n->a_h, H), G + n->seg_off[AC_A_WPI], H, TEPI_NONE, nullptr, nullptr, 0, G + n->seg_off[AC_A_BPI]);
  g[1] = mk_gemm(B, H, A, op_dense(OP_KCONT, n->dz, A), op_dense(OP_XCONT, P + n->seg_off[AC_A_WPI], H), n->dah, H, TEPI_MASK, nullptr, n->a_h, H);
  if ((rc = ac_tgemm(n, g, 2, st))) return rc;
  g[0] = mk_gemm(H, H, B, op_dense(OP_XCONT, n->dah, H), op_dense(OP_XCONT, n->a_feat, H), G + n->seg_off[AC_A_WL], H, TEPI_NONE, nullptr, nullptr, 0, G + n->seg_off[AC_A_BL]);
  g[1] = mk_gemm(B, H, H, op_dense(OP_KCONT, n->dah, H), op_dense(OP_XCONT, P + n->seg_off[AC_A_WL], H), n->dafeat, H, TEPI_MASK, nullptr, n->a_feat, H);
  if ((rc = ac_tgemm(n, g, 2, st))) return rc;
  g[0] = mk_gemm(H, S, B, op_dense(OP_XCONT, n->dafeat, H), op_dense(OP_XCONT, d_x, S), G + n->seg_off[AC_A_W1], S, TEPI_NONE, nullptr, nullptr, 0, G + n->seg_off[AC_A_B1]);
  if ((rc = ac_tgemm(n, g, 1, st))) return rc;
  return jh_flat_adam_step(n->nA, n->ap, n->ag, n->am, n->av, n->hyper_a, n->ticket_a, n->norm_partial, 0.f, st);
}
