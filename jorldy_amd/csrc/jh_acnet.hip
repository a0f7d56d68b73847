// The one copy of what jh_acnet (TD3, DDPG: jh_td3.hip) and jh_sacnet (SAC: jh_sac.hip) share above the layer builders: the critic loss and the
// Polyak average, the object's core and the entries both objects answer with it, the critics' forward and backward, and the pieces of the critic
// update and of the actor update.  Every dense contraction runs on the tile engine (jh_tgemm.hip) under the call-site name "dense",
// independent layers sharing a grouped launch; a group keeps its problems and their order, which the engine's split decisions depend on.
// No floating-point atomics: every sum has a fixed order, so two runs (and a graph replay) give the same bits.
#include "jh_acnet.h"

namespace {

// ---------------------------------------------------------------------------------- critic loss
// (td3.py:163-178, ddpg.py:131-140; with the entropy term sac.py:186-216).  One workgroup: thread t walks b = t, t + 256, ... in ascending
// order, the block reduction has a fixed tree.  Two critics (TWO) and the entropy term (ENT) are uniform over the launch; the kernel picks
// the loop compiled for its pair, so a row's loads are issued together and not one round trip after another behind each branch.  Without
// ENT the target is gamma * mn as it stands.
template <bool TWO, bool ENT>
__device__ __forceinline__ void ac_critic_loss_rows(const CriticLossArgs& a, float& l0, float& l1, float& my) {
  const float inv = 2.f / (float)a.B;
  const float alpha = ENT ? *a.alpha : 0.f;
  for (int b = threadIdx.x; b < a.B; b += 256) {
    const float q0 = a.q[b], q1 = TWO ? a.q[a.B + b] : 0.f;  // read before the first store: the stores then wait for no load behind them
    float mn = a.qn[b];
    if (TWO) mn = fminf(mn, a.qn[a.B + b]);
    if (ENT) mn = mn + alpha * -a.logp[b];
    const float y = a.reward[b] + (1.f - a.done[b]) * a.gamma * mn;
    if (a.y) a.y[b] = y;
    my = fmaxf(my, y);
    const float d0 = q0 - y;
    l0 += d0 * d0;
    a.grad[b] = d0 * inv;
    if (TWO) {
      const float d1 = q1 - y;
      l1 += d1 * d1;
      a.grad[a.gstride + b] = d1 * inv;
    }
  }
}
__global__ void __launch_bounds__(256) jh_ac_critic_loss_kernel(CriticLossArgs a) {
  __shared__ float s_red[16];
  float l0 = 0.f, l1 = 0.f, my = -3.4e38f;
  if (a.n == 2 && a.logp) ac_critic_loss_rows<true, true>(a, l0, l1, my);
  else if (a.n == 2) ac_critic_loss_rows<true, false>(a, l0, l1, my);
  else if (a.logp) ac_critic_loss_rows<false, true>(a, l0, l1, my);
  else ac_critic_loss_rows<false, false>(a, l0, l1, my);
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

// ---------------------------------------------------------------------------------- Polyak average
// t <- tau * p + (1 - tau) * t   (td3.py:203-209) as torch evaluates it on float32 tensors: the Python scalars tau and (1 - tau) -- the
// latter formed in DOUBLE -- are rounded to float32, then two float32 products and one float32 sum (the build has -ffp-contract=off).
__global__ void __launch_bounds__(256) jh_ac_polyak_kernel(int64_t n, const float* __restrict__ p, float* __restrict__ t, float tau, float omt) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float a = tau * p[i];
  const float b = omt * t[i];
  t[i] = a + b;
}

// ---- the critics' layer builders (network/q_network.py:23-39).  P: the parameter bucket of one critic; set: the activation set; c: the critic.
inline float* ac_cat(const jh_acnet* n, int set, int c) { return n->c_cat[set] + (size_t)c * n->maxB * 2 * n->H; }
inline float* ac_ch(const jh_acnet* n, int set, int c) { return n->c_h[set] + (size_t)c * n->maxB * n->H; }
inline TGemm ac_c_head(const jh_acnet* n, const float* P, int set, int c, const float* x, int rows) {
  return ac_head(n, P, AC_C_W1, AC_C_B1, x, rows, ac_cat(n, set, c), 2 * n->H);
}
inline TGemm ac_c_embed(const jh_acnet* n, const float* P, int set, int c, const float* act, int rows) {
  return mk_gemm(rows, n->H, n->A, op_dense(OP_KCONT, act, n->A), op_dense(OP_KCONT, P + n->seg_off[AC_C_WE], n->A), ac_cat(n, set, c) + n->H, 2 * n->H,
                 TEPI_BIAS_RELU, P + n->seg_off[AC_C_BE]);
}
inline TGemm ac_c_l(const jh_acnet* n, const float* P, int set, int c, int rows) {
  return mk_gemm(rows, n->H, 2 * n->H, op_dense(OP_KCONT, ac_cat(n, set, c), 2 * n->H), op_dense(OP_KCONT, P + n->seg_off[AC_C_WL], 2 * n->H), ac_ch(n, set, c), n->H,
                 TEPI_BIAS_RELU, P + n->seg_off[AC_C_BL]);
}
inline TGemm ac_c_q(const jh_acnet* n, const float* P, int set, int c, int rows, float* out) {
  return mk_gemm(rows, 1, n->H, op_dense(OP_KCONT, ac_ch(n, set, c), n->H), op_dense(OP_KCONT, P + n->seg_off[AC_C_WQ], n->H), out, 1, TEPI_BIAS, P + n->seg_off[AC_C_BQ]);
}

// backward of critics c0 .. c1 - 1's online activations (set 0) from dq [B] down to d(cat) [B][2H]; weights: also the gradient bucket of those
// critics; !weights: only the `e` half d(cat)[:, H:] is computed, the head half keeps whatever it held, and d_x / d_action are not read
int ac_critic_backward(jh_acnet* n, int B, const float* d_x, const float* d_action, bool weights, int c0, int c1, hipStream_t st) {
  const int H = n->H, S = n->S, A = n->A;
  TGemm g[kMaxGroup];
  int k = 0, rc;
  // q: weight gradient (+ bias gradient as the row sum) and data gradient (+ relu' of l)
  for (int c = c0; c < c1; ++c) {
    const float* P = n->cp + c * n->nC;
    float* G = n->cg + c * n->nC;
    const float* dq = n->dq + (size_t)c * n->maxB;
    float* dh = n->dh + (size_t)c * n->maxB * H;
    if (weights)
      g[k++] = mk_gemm(1, H, B, op_dense(OP_XCONT, dq, 1), op_dense(OP_XCONT, ac_ch(n, 0, c), H), G + n->seg_off[AC_C_WQ], H, TEPI_NONE, nullptr, nullptr, 0, G + n->seg_off[AC_C_BQ]);
    g[k++] = mk_gemm(B, H, 1, op_dense(OP_KCONT, dq, 1), op_dense(OP_XCONT, P + n->seg_off[AC_C_WQ], H), dh, H, TEPI_MASK, nullptr, ac_ch(n, 0, c), H);
  }
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, k, st))) return rc;
  k = 0;
  for (int c = c0; c < c1; ++c) {
    const float* P = n->cp + c * n->nC;
    float* G = n->cg + c * n->nC;
    const float* dh = n->dh + (size_t)c * n->maxB * H;
    float* dcat = n->dcat + (size_t)c * n->maxB * 2 * H;
    if (weights)
      g[k++] = mk_gemm(H, 2 * H, B, op_dense(OP_XCONT, dh, H), op_dense(OP_XCONT, ac_cat(n, 0, c), 2 * H), G + n->seg_off[AC_C_WL], 2 * H, TEPI_NONE, nullptr, nullptr, 0,
                       G + n->seg_off[AC_C_BL]);
    // without the weights only d(cat)[:, H:], the `e` half, has a reader (the action input): columns H.. of W_l, of the mask and of d(cat)
    const int o = weights ? 0 : H;
    g[k++] = mk_gemm(B, 2 * H - o, H, op_dense(OP_KCONT, dh, H), op_dense(OP_XCONT, P + n->seg_off[AC_C_WL] + o, 2 * H), dcat + o, 2 * H, TEPI_MASK, nullptr,
                     ac_cat(n, 0, c) + o, 2 * H);
  }
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, k, st))) return rc;
  if (!weights) return JH_OK;
  k = 0;
  for (int c = c0; c < c1; ++c) {
    float* G = n->cg + c * n->nC;
    const float* dcat = n->dcat + (size_t)c * n->maxB * 2 * H;
    g[k++] = mk_gemm(H, S, B, op_dense(OP_XCONT, dcat, 2 * H), op_dense(OP_XCONT, d_x, S), G + n->seg_off[AC_C_W1], S, TEPI_NONE, nullptr, nullptr, 0, G + n->seg_off[AC_C_B1]);
    g[k++] = mk_gemm(H, A, B, op_dense(OP_XCONT, dcat + H, 2 * H), op_dense(OP_XCONT, d_action, A), G + n->seg_off[AC_C_WE], A, TEPI_NONE, nullptr, nullptr, 0,
                     G + n->seg_off[AC_C_BE]);
  }
  return core_tgemm(&n->core, "jh_tgemm_dense", g, k, st);
}

}  // namespace

int ac_critic_loss(const CriticLossArgs& a, hipStream_t st) {
  JH_LAUNCH(jh_ac_critic_loss_kernel, dim3(1), dim3(256), 0, st, a);
  JH_LAUNCH_CHECK();
  return JH_OK;
}
int ac_polyak(int64_t n, const float* p, float* t, double tau, hipStream_t st) {
  JH_LAUNCH(jh_ac_polyak_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, p, t, (float)tau, (float)(1.0 - tau));
  JH_LAUNCH_CHECK();
  return JH_OK;
}

// ---------------------------------------------------------------------------------- the object's core
int ac_layout(jh_acnet* n, int32_t S, int32_t H, int32_t A, int32_t head, int32_t nc, int32_t max_batch) {
  JH_ARG(S > 0 && H > 0 && H % 4 == 0 && A >= 1 && max_batch > 0 && (nc == 1 || nc == 2));
  JH_ARG((int64_t)2 * max_batch * 2 * H < ((int64_t)1 << 31) && (int64_t)max_batch * (S > head ? S : head) < ((int64_t)1 << 31));  // the tile engine indexes in 32 bits
  n->S = S; n->H = H; n->A = A; n->nc = nc; n->maxB = max_batch;
  auto seg = [&](int id, int rows, int cols) { n->seg_rows[id] = rows; n->seg_cols[id] = cols; };
  seg(AC_A_W1, H, S); seg(AC_A_B1, 1, H); seg(AC_A_WL, H, H); seg(AC_A_BL, 1, H); seg(AC_A_WPI, head, H); seg(AC_A_BPI, 1, head);
  seg(AC_C_W1, H, S); seg(AC_C_B1, 1, H); seg(AC_C_WE, H, A); seg(AC_C_BE, 1, H); seg(AC_C_WL, H, 2 * H); seg(AC_C_BL, 1, H);
  seg(AC_C_WQ, 1, H); seg(AC_C_BQ, 1, 1);
  n->nA = seg_pack(n->seg_rows, n->seg_cols, AC_A_W1, AC_C_W1, n->seg_off);
  n->nC = seg_pack(n->seg_rows, n->seg_cols, AC_C_W1, AC_SEG_COUNT, n->seg_off);
  return JH_OK;
}

int ac_init(jh_acnet* n, jh_ctx* ctx, int32_t S, int32_t H, int32_t A, int32_t head, int32_t nc, int32_t max_batch, float* const actor[5], float* const critics[5]) {
  JH_HIP(hipSetDevice(ctx->device));
  n->core.ctx = ctx;
  int rc = ac_layout(n, S, H, A, head, nc, max_batch);
  if (rc) return rc;
  n->ap = actor[0]; n->at = actor[1]; n->ag = actor[2]; n->am = actor[3]; n->av = actor[4];
  n->cp = critics[0]; n->ct = critics[1]; n->cg = critics[2]; n->cm = critics[3]; n->cv = critics[4];
  const size_t B = (size_t)max_batch, NB = (size_t)nc * B;
  auto A4 = [&](float** p, size_t floats) { if (!rc) rc = core_alloc(&n->core, "jh_acnet", (void**)p, floats * sizeof(float), true); };
  rc = optim_init(&n->core, "jh_acnet", &n->opt_a);
  if (!rc) rc = optim_init(&n->core, "jh_acnet", &n->opt_c);
  A4(&n->a_feat, B * H); A4(&n->a_h, B * H); A4(&n->a_z, B * head); A4(&n->a_out, B * A);
  for (int s = 0; s < 2; ++s) {
    A4(&n->c_cat[s], NB * 2 * H); A4(&n->c_h[s], NB * H); A4(&n->c_q[s], NB);
  }
  A4(&n->dq, NB); A4(&n->dh, NB * H); A4(&n->dcat, NB * 2 * H); A4(&n->da, B * A); A4(&n->dz, B * head); A4(&n->dah, B * H); A4(&n->dafeat, B * H);
  if (!rc) rc = core_workspace(&n->core, "jh_acnet", (size_t)8 << 20, 8192);  // 32 MB of split-K partials
  return rc ? rc : core_drain();
}

// ---------------------------------------------------------------------------------- the entries both objects answer with the core
// which: 0 the actor's optimizer, 1 the critics' (one block and one launch for all critics: td3.py:95-112 and sac.py:136-140 give them the same settings)
JH_EXPORT int jh_acnet_set_hyper(jh_acnet* n, int32_t which, double lr, double beta1, double beta2, double eps, int64_t step, jh_stream stream) {
  JH_ARG(n && (which == 0 || which == 1));
  return jh_hyper_upload(n->core.ctx, which == 0 ? n->opt_a.hyper : n->opt_c.hyper, lr, beta1, beta2, eps, step, 0, jh_s(stream));
}
JH_EXPORT int jh_acnet_set_lr(jh_acnet* n, int32_t which, double lr, jh_stream stream) {
  JH_ARG(n && (which == 0 || which == 1));
  return jh_hyper_upload_lr(n->core.ctx, which == 0 ? n->opt_a.hyper : n->opt_c.hyper, lr, jh_s(stream));
}
JH_EXPORT int jh_acnet_sync_target(jh_acnet* n, jh_stream stream) {
  JH_ARG(n != nullptr);
  if (n->at) JH_HIP(hipMemcpyAsync(n->at, n->ap, sizeof(float) * (size_t)n->nA, hipMemcpyDeviceToDevice, jh_s(stream)));
  JH_HIP(hipMemcpyAsync(n->ct, n->cp, sizeof(float) * (size_t)n->nC * n->nc, hipMemcpyDeviceToDevice, jh_s(stream)));
  return JH_OK;
}
// update_target_soft (td3.py:203-209, ddpg.py:159-163, sac.py:271-275): the critics' bucket, then the actor's where it has a target
JH_EXPORT int jh_acnet_soft_update(jh_acnet* n, double tau, jh_stream stream) {
  JH_ARG(n && tau >= 0.0 && tau <= 1.0);
  int rc = ac_polyak(n->nC * n->nc, n->cp, n->ct, tau, jh_s(stream));
  return rc || !n->at ? rc : ac_polyak(n->nA, n->ap, n->at, tau, jh_s(stream));
}

int ac_actor_forward(jh_acnet* n, const float* P, const float* d_x, int rows, hipStream_t st) {
  TGemm g[1];
  int rc;
  g[0] = ac_head(n, P, AC_A_W1, AC_A_B1, d_x, rows, n->a_feat, n->H);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 1, st))) return rc;
  g[0] = ac_a_l(n, P, rows);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 1, st))) return rc;
  g[0] = ac_a_pi(n, P, rows);
  return core_tgemm(&n->core, "jh_tgemm_dense", g, 1, st);
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
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 2 * nc, st))) return rc;
  for (int c = 0; c < nc; ++c) g[c] = ac_c_l(n, base + c * n->nC, which, c, rows);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, nc, st))) return rc;
  for (int c = 0; c < nc; ++c) g[c] = ac_c_q(n, base + c * n->nC, which, c, rows, d_q + (size_t)c * rows);
  return core_tgemm(&n->core, "jh_tgemm_dense", g, nc, st);
}

// ---------------------------------------------------------------------------------- the critic update
// (td3.py:157-178, ddpg.py:128-140, sac.py:183-225).  d_x = [state; next_state] (2B rows)
int ac_critic_front(jh_acnet* n, const float* actor, const float* d_x, const float* d_action, int B, hipStream_t st) {
  const int nc = n->nc;
  const float* xs = d_x;
  const float* xn = d_x + (size_t)B * n->S;
  TGemm g[kMaxGroup];
  int k, rc;
  // 1: head.l of the policy and the target critics on s', of the online critics on s
  k = 0;
  g[k++] = ac_head(n, actor, AC_A_W1, AC_A_B1, xn, B, n->a_feat, n->H);
  for (int c = 0; c < nc; ++c) g[k++] = ac_c_head(n, n->ct + c * n->nC, 1, c, xn, B);
  for (int c = 0; c < nc; ++c) g[k++] = ac_c_head(n, n->cp + c * n->nC, 0, c, xs, B);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, k, st))) return rc;
  // 2: the policy's l, the online critics' e(a)
  k = 0;
  g[k++] = ac_a_l(n, actor, B);
  for (int c = 0; c < nc; ++c) g[k++] = ac_c_embed(n, n->cp + c * n->nC, 0, c, d_action, B);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, k, st))) return rc;
  // 3: the policy's last layer, the online critics' l
  k = 0;
  g[k++] = ac_a_pi(n, actor, B);
  for (int c = 0; c < nc; ++c) g[k++] = ac_c_l(n, n->cp + c * n->nC, 0, c, B);
  return core_tgemm(&n->core, "jh_tgemm_dense", g, k, st);
}

int ac_critic_back(jh_acnet* n, const float* d_x, const float* d_action, int B, const float* a_next, float* q_on, CriticLossArgs loss, hipStream_t st) {
  const int nc = n->nc;
  TGemm g[kMaxGroup];
  int k, rc;
  // 4: the target critics' e(a'), the online critics' q
  k = 0;
  for (int c = 0; c < nc; ++c) g[k++] = ac_c_embed(n, n->ct + c * n->nC, 1, c, a_next, B);
  for (int c = 0; c < nc; ++c) g[k++] = ac_c_q(n, n->cp + c * n->nC, 0, c, B, q_on + (size_t)c * B);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, k, st))) return rc;
  // 5, 6: the target critics' l and q
  for (int c = 0; c < nc; ++c) g[c] = ac_c_l(n, n->ct + c * n->nC, 1, c, B);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, nc, st))) return rc;
  for (int c = 0; c < nc; ++c) g[c] = ac_c_q(n, n->ct + c * n->nC, 1, c, B, n->c_q[1] + (size_t)c * B);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, nc, st))) return rc;
  // loss: q and q' are packed [nc][B]; the gradient of critic c goes where the backward reads it, at c * maxB
  loss.B = B; loss.n = nc; loss.gstride = n->maxB; loss.q = q_on; loss.qn = n->c_q[1]; loss.grad = n->dq;
  if ((rc = ac_critic_loss(loss, st))) return rc;
  if ((rc = ac_critic_backward(n, B, d_x, d_action, true, 0, nc, st))) return rc;
  return jh_flat_adam_step(n->nC * nc, n->cp, n->cg, n->cm, n->cv, n->opt_c.hyper, n->opt_c.ticket, n->core.norm_partial, 0.f, st);
}

// ---------------------------------------------------------------------------------- the actor update
// (td3.py:181-188, ddpg.py:143-148, sac.py:229-255).  The critics' parameters, gradient bucket and moments are not written.
int ac_actor_trunk(jh_acnet* n, const float* d_x, int B, int ncq, hipStream_t st) {
  TGemm g[kMaxGroup];
  int k = 0, rc;
  g[k++] = ac_head(n, n->ap, AC_A_W1, AC_A_B1, d_x, B, n->a_feat, n->H);
  for (int c = 0; c < ncq; ++c) g[k++] = ac_c_head(n, n->cp + c * n->nC, 0, c, d_x, B);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, k, st))) return rc;
  g[0] = ac_a_l(n, n->ap, B);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 1, st))) return rc;
  g[0] = ac_a_pi(n, n->ap, B);
  return core_tgemm(&n->core, "jh_tgemm_dense", g, 1, st);
}

int ac_actor_q(jh_acnet* n, const float* action, int B, int ncq, float* q, hipStream_t st) {
  TGemm g[2];
  int rc;
  for (int c = 0; c < ncq; ++c) g[c] = ac_c_embed(n, n->cp + c * n->nC, 0, c, action, B);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, ncq, st))) return rc;
  for (int c = 0; c < ncq; ++c) g[c] = ac_c_l(n, n->cp + c * n->nC, 0, c, B);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, ncq, st))) return rc;
  for (int c = 0; c < ncq; ++c) g[c] = ac_c_q(n, n->cp + c * n->nC, 0, c, B, q + (size_t)c * B);
  return core_tgemm(&n->core, "jh_tgemm_dense", g, ncq, st);
}

// back through the critics to their action inputs: d(cat) -> da_c = d(cat_c)[:, H:] We_c
int ac_actor_dact(jh_acnet* n, int B, int ncq, float* da2, hipStream_t st) {
  const int H = n->H, A = n->A;
  TGemm g[2];
  int rc;
  if ((rc = ac_critic_backward(n, B, nullptr, nullptr, false, 0, ncq, st))) return rc;
  for (int c = 0; c < ncq; ++c)
    g[c] = mk_gemm(B, A, H, op_dense(OP_KCONT, n->dcat + (size_t)c * n->maxB * 2 * H + H, 2 * H), op_dense(OP_XCONT, n->cp + c * n->nC + n->seg_off[AC_C_WE], A),
                   c == 0 ? n->da : da2, A, TEPI_NONE);
  return core_tgemm(&n->core, "jh_tgemm_dense", g, ncq, st);
}

// the actor's backward from dz [B][head]: the last layer, l, head.l; then its Adam
int ac_actor_backward(jh_acnet* n, const float* d_x, int B, hipStream_t st) {
  const int H = n->H, S = n->S, W = n->seg_rows[AC_A_WPI];
  const float* P = n->ap;
  float* G = n->ag;
  TGemm g[2];
  int rc;
  g[0] = mk_gemm(W, H, B, op_dense(OP_XCONT, n->dz, W), op_dense(OP_XCONT, n->a_h, H), G + n->seg_off[AC_A_WPI], H, TEPI_NONE, nullptr, nullptr, 0, G + n->seg_off[AC_A_BPI]);
  g[1] = mk_gemm(B, H, W, op_dense(OP_KCONT, n->dz, W), op_dense(OP_XCONT, P + n->seg_off[AC_A_WPI], H), n->dah, H, TEPI_MASK, nullptr, n->a_h, H);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 2, st))) return rc;
  g[0] = mk_gemm(H, H, B, op_dense(OP_XCONT, n->dah, H), op_dense(OP_XCONT, n->a_feat, H), G + n->seg_off[AC_A_WL], H, TEPI_NONE, nullptr, nullptr, 0, G + n->seg_off[AC_A_BL]);
  g[1] = mk_gemm(B, H, H, op_dense(OP_KCONT, n->dah, H), op_dense(OP_XCONT, P + n->seg_off[AC_A_WL], H), n->dafeat, H, TEPI_MASK, nullptr, n->a_feat, H);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 2, st))) return rc;
  g[0] = mk_gemm(H, S, B, op_dense(OP_XCONT, n->dafeat, H), op_dense(OP_XCONT, d_x, S), G + n->seg_off[AC_A_W1], S, TEPI_NONE, nullptr, nullptr, 0, G + n->seg_off[AC_A_B1]);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 1, st))) return rc;
  return jh_flat_adam_step(n->nA, n->ap, n->ag, n->am, n->av, n->opt_a.hyper, n->opt_a.ticket, n->core.norm_partial, 0.f, st);
}

// ---------------------------------------------------------------------------------- critic 0 over sampled actions (MPO, mpo.py:219-231, 261-263)
// The reference repeats every state N times in front of the critic.  Here head.l(s) runs ONCE per state row, on R rows; its H outputs are
// then copied into the [head(s) | relu(e(a))] rows of that state's N samples, and only e(a), l and q run over the N * R rows.  A job is one
// critic forward: the R-row ones (online / target of (s, a), in the object's own activation sets, head.l(s) already in place) and the
// sampled ones ride the same grouped launch per layer.
namespace {

struct AcJob {
  const float* P;     // parameter bucket of the critic
  const float* act;   // [rows][A]
  int rows;
  float *cat, *h;     // [rows][2H], [rows][H]
  float* q;           // [rows]
  const float* feat;  // sampled: head.l(s) [R][ldfeat] to copy into cat[:, :H] of every sample's rows; nullptr: already in cat
  int ldfeat;
};

// dst[(n * R + r) * 2H + j] = src[r * ld + j] for j < H, 16 bytes per thread; blockIdx.y picks one of up to two copies
__global__ void __launch_bounds__(256) jh_ac_spread_head_kernel(int rows, int R, int H4, const float* __restrict__ src0, int ld0, float* __restrict__ dst0,
                                                                const float* __restrict__ src1, int ld1, float* __restrict__ dst1) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= rows * H4) return;
  const int row = i / H4, j = (i - row * H4) * 4, r = row % R;
  const float* src = blockIdx.y ? src1 : src0;
  const int ld = blockIdx.y ? ld1 : ld0;
  float* dst = blockIdx.y ? dst1 : dst0;
  *reinterpret_cast<float4*>(dst + (size_t)row * 8 * H4 + j) = *reinterpret_cast<const float4*>(src + (size_t)r * ld + j);
}

// levels 2-5 of `nj` jobs whose head.l(s) the caller has launched: e(a); the copy of head.l(s) into the samples' rows; l; q.  4 launches.
int ac_jobs_run(jh_acnet* n, const AcJob* j, int nj, int R, hipStream_t st) {
  const int H = n->H, A = n->A;
  TGemm g[kMaxGroup];
  int rc;
  const AcJob* s[2] = {nullptr, nullptr};  // the sampled jobs; checked before anything is launched
  int ns = 0;
  for (int i = 0; i < nj; ++i)
    if (j[i].feat) {
      if (ns == 2 || (ns == 1 && j[i].rows != s[0]->rows)) return jh_fail(JH_ERR_ARG, "jh_acnet: at most two sampled jobs of one size");
      s[ns++] = &j[i];
    }
  for (int i = 0; i < nj; ++i)
    g[i] = mk_gemm(j[i].rows, H, A, op_dense(OP_KCONT, j[i].act, A), op_dense(OP_KCONT, j[i].P + n->seg_off[AC_C_WE], A), j[i].cat + H, 2 * H, TEPI_BIAS_RELU,
                   j[i].P + n->seg_off[AC_C_BE]);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, nj, st))) return rc;
  if (ns) {
    const AcJob* s1 = s[ns - 1];
    const int total = s[0]->rows * (H / 4);
    JH_LAUNCH(jh_ac_spread_head_kernel, dim3((unsigned)((total + 255) / 256), ns), dim3(256), 0, st, s[0]->rows, R, H / 4, s[0]->feat, s[0]->ldfeat, s[0]->cat,
              s1->feat, s1->ldfeat, s1->cat);
    JH_LAUNCH_CHECK();
  }
  for (int i = 0; i < nj; ++i)
    g[i] = mk_gemm(j[i].rows, H, 2 * H, op_dense(OP_KCONT, j[i].cat, 2 * H), op_dense(OP_KCONT, j[i].P + n->seg_off[AC_C_WL], 2 * H), j[i].h, H, TEPI_BIAS_RELU,
                   j[i].P + n->seg_off[AC_C_BL]);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, nj, st))) return rc;
  for (int i = 0; i < nj; ++i)
    g[i] = mk_gemm(j[i].rows, 1, H, op_dense(OP_KCONT, j[i].h, H), op_dense(OP_KCONT, j[i].P + n->seg_off[AC_C_WQ], H), j[i].q, 1, TEPI_BIAS, j[i].P + n->seg_off[AC_C_BQ]);
  return core_tgemm(&n->core, "jh_tgemm_dense", g, nj, st);
}

inline float* ac_scat(const jh_acnet* n, int slot) { return n->s_cat + (size_t)slot * n->smax * 2 * n->H; }
inline float* ac_sh(const jh_acnet* n, int slot) { return n->s_h + (size_t)slot * n->smax * n->H; }

}  // namespace

// Room for `rows` = N * R sampled rows in each of the two slots.  Allocates: once, outside any stream capture.
JH_EXPORT int jh_acnet_reserve_sampled(jh_acnet* n, int32_t rows) {
  JH_ARG(n && rows > 0 && (int64_t)rows * 2 * n->H < ((int64_t)1 << 31));  // the tile engine indexes in 32 bits
  if (rows <= n->smax) return JH_OK;
  if (n->smax) return jh_fail(JH_ERR_STATE, "jh_acnet_reserve_sampled: already reserved %d rows", n->smax);
  JH_HIP(hipSetDevice(n->core.ctx->device));
  int rc = core_alloc(&n->core, "jh_acnet", (void**)&n->s_cat, (size_t)2 * rows * 2 * n->H * sizeof(float), true);
  if (!rc) rc = core_alloc(&n->core, "jh_acnet", (void**)&n->s_h, (size_t)2 * rows * n->H * sizeof(float), true);
  if (!rc) rc = core_alloc(&n->core, "jh_acnet", (void**)&n->s_feat, (size_t)n->maxB * n->H * sizeof(float), true);
  if (rc) return rc;
  n->smax = rows;
  return core_drain();
}

// critic 0 (which 0 online / 1 target) of d_x [R][S] over d_actions [N][R][A] -> d_q [N][R]: head.l(s) on R rows, then ac_jobs_run.  5 launches.
JH_EXPORT int jh_acnet_critic_forward_sampled(jh_acnet* n, int32_t which, const float* d_x, const float* d_actions, int32_t R, int32_t N, float* d_q,
                                              jh_stream stream) {
  JH_ARG(n && d_x && d_actions && d_q);
  JH_ARG(R > 0 && R <= n->maxB && N > 0 && (int64_t)N * R <= n->smax && (which == 0 || which == 1));
  hipStream_t st = jh_s(stream);
  const float* P = which == 0 ? n->cp : n->ct;
  TGemm g[1] = {ac_head(n, P, AC_C_W1, AC_C_B1, d_x, R, n->s_feat, n->H)};
  int rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 1, st);
  if (rc) return rc;
  const AcJob j{P, d_actions, N * R, ac_scat(n, 0), ac_sh(n, 0), d_q, n->s_feat, n->H};
  return ac_jobs_run(n, &j, 1, R, st);
}

// Every critic forward of one MPO learn() (mpo.py:201, 219, 228-231, 261-263) in 5 grouped launches.  d_x = [state; next_state] (2R rows),
// d_action [R][A] the stored action, d_a_next / d_a_add [N][R][A] the sampled ones -> d_q = online(s, a) and d_qt_a = target(s, a) [R],
// d_qt_next = target(s', a_next) and d_qt_add = target(s, a_add) [N][R].  The target's head.l(s) serves both target(s, a) and the N samples
// of a_add.  The online activations stay in set 0 for jh_acnet_critic_fit.
JH_EXPORT int jh_acnet_mpo_forward(jh_acnet* n, const float* d_x, const float* d_action, const float* d_a_next, const float* d_a_add, int32_t R, int32_t N,
                                   float* d_q, float* d_qt_a, float* d_qt_next, float* d_qt_add, jh_stream stream) {
  JH_ARG(n && d_x && d_action && d_a_next && d_a_add && d_q && d_qt_a && d_qt_next && d_qt_add);
  JH_ARG(n->nc == 1 && R > 0 && R <= n->maxB && N > 0 && (int64_t)N * R <= n->smax);
  hipStream_t st = jh_s(stream);
  const float* xs = d_x;
  const float* xn = d_x + (size_t)R * n->S;
  TGemm g[3] = {ac_c_head(n, n->cp, 0, 0, xs, R), ac_c_head(n, n->ct, 1, 0, xs, R), ac_head(n, n->ct, AC_C_W1, AC_C_B1, xn, R, n->s_feat, n->H)};
  int rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 3, st);
  if (rc) return rc;
  const AcJob j[4] = {{n->cp, d_action, R, ac_cat(n, 0, 0), ac_ch(n, 0, 0), d_q, nullptr, 0},
                      {n->ct, d_action, R, ac_cat(n, 1, 0), ac_ch(n, 1, 0), d_qt_a, nullptr, 0},
                      {n->ct, d_a_next, N * R, ac_scat(n, 0), ac_sh(n, 0), d_qt_next, n->s_feat, n->H},
                      {n->ct, d_a_add, N * R, ac_scat(n, 1), ac_sh(n, 1), d_qt_add, ac_cat(n, 1, 0), 2 * n->H}};
  return ac_jobs_run(n, j, 4, R, st);
}

// The critic's step from a gradient the caller supplies (MPO's loss kernel writes it): d_dq [R] = d(loss)/d(q) of the online(s, a) that the
// last jh_acnet_mpo_forward left in set 0 -> the critic's backward, clip_grad_norm_(max_norm; <= 0: none) and Adam on the critic's own
// optimizer block.  1 copy + 3 grouped launches + the optimizer's.
JH_EXPORT int jh_acnet_critic_fit(jh_acnet* n, const float* d_x, const float* d_action, const float* d_dq, int32_t R, float max_norm, jh_stream stream) {
  JH_ARG(n && d_x && d_action && d_dq);
  JH_ARG(n->nc == 1 && R > 0 && R <= n->maxB);
  hipStream_t st = jh_s(stream);
  JH_HIP(hipMemcpyAsync(n->dq, d_dq, sizeof(float) * (size_t)R, hipMemcpyDeviceToDevice, st));
  int rc = ac_critic_backward(n, R, d_x, d_action, true, 0, 1, st);
  if (rc) return rc;
  return jh_flat_adam_step(n->nC, n->cp, n->cg, n->cm, n->cv, n->opt_c.hyper, n->opt_c.ticket, n->core.norm_partial, max_norm > 0.f ? max_norm : 0.f, st);
}
