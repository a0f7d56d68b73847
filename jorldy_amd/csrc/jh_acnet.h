// What the actor-critic network objects share (jh_td3.hip: jh_acnet_*, jh_sac.hip: jh_sacnet_*): the object's layout and buffers, the layer
// builders of the policy's trunk (head.l -> relu(l)), and the declarations of what jh_acnet.hip holds once for both: the critic loss and the
// Polyak average, the object's core, the critics' forward, and the pieces the two critic updates and the two actor updates are made of.
// jh_sacnet embeds a jh_acnet and drives these with it.
#pragma once
#include "jh_netcore.h"

enum { AC_A_W1, AC_A_B1, AC_A_WL, AC_A_BL, AC_A_WPI, AC_A_BPI, AC_C_W1, AC_C_B1, AC_C_WE, AC_C_BE, AC_C_WL, AC_C_BL, AC_C_WQ, AC_C_BQ, AC_SEG_COUNT };

struct jh_acnet {
  NetCore core;
  FlatOptim opt_a, opt_c;  // the actor's Adam, the critics' (one block and one launch for all critics)
  int S = 0, H = 0, A = 0, nc = 0, maxB = 0;
  int64_t seg_off[AC_SEG_COUNT] = {0};  // actor segments: offsets in the actor bucket; critic segments: offsets inside ONE critic
  int seg_rows[AC_SEG_COUNT] = {0}, seg_cols[AC_SEG_COUNT] = {0};
  int64_t nA = 0, nC = 0;  // floats of the actor bucket / of one critic (the critic buckets hold nc of them back to back)
  float *ap = nullptr, *at = nullptr, *ag = nullptr, *am = nullptr, *av = nullptr;  // at == nullptr: no target actor
  float *cp = nullptr, *ct = nullptr, *cg = nullptr, *cm = nullptr, *cv = nullptr;
  // actor activations [maxB] rows: feat, h, z (the head's output, `head` columns), a
  float *a_feat = nullptr, *a_h = nullptr, *a_z = nullptr, *a_out = nullptr;
  // critic activations, set 0 = online, 1 = target: cat [nc][maxB][2H] = [head(s) | relu(e(a))], h [nc][maxB][H], q [nc][maxB]
  float *c_cat[2] = {nullptr, nullptr}, *c_h[2] = {nullptr, nullptr}, *c_q[2] = {nullptr, nullptr};
  // backward: dq [nc][maxB], dh [nc][maxB][H], dcat [nc][maxB][2H], da [maxB][A], dz [maxB][head], d(actor h) / d(actor feat) [maxB][H]
  float *dq = nullptr, *dh = nullptr, *dcat = nullptr, *da = nullptr, *dz = nullptr, *dah = nullptr, *dafeat = nullptr;
  // critic 0 over sampled actions (MPO, jh_acnet_reserve_sampled): two slots of smax = N * R rows, cat [2][smax][2H] and h [2][smax][H], and
  // head.l(s) of the slot-0 states [maxB][H], computed on R rows and copied into its samples' rows
  int smax = 0;
  float *s_cat = nullptr, *s_h = nullptr, *s_feat = nullptr;
};

constexpr int kMaxLossRows = 1 << 20;

// ---- the object's core (jh_acnet.hip).  head: the columns of the actor's last layer, A (pi) or 2A ([mu | log_std]).
int ac_layout(jh_acnet* n, int32_t S, int32_t H, int32_t A, int32_t head, int32_t nc, int32_t max_batch);
// layout, the caller's buckets {params, target, grads, m, v}, every buffer above, workspace, counters, both hyper blocks.  On failure the
// caller releases: core_release(&n->core) frees what the object owns (after the device has drained), the object itself stays the caller's.
int ac_init(jh_acnet* n, jh_ctx* ctx, int32_t S, int32_t H, int32_t A, int32_t head, int32_t nc, int32_t max_batch, float* const actor[5], float* const critics[5]);

// ---- layer builders of the actor's trunk.  P: the actor's parameter bucket (online or target)
static inline TGemm ac_head(const jh_acnet* n, const float* P, int w, int b, const float* x, int rows, float* out, int ldc) {
  return mk_gemm(rows, n->H, n->S, op_dense(OP_KCONT, x, n->S), op_dense(OP_KCONT, P + n->seg_off[w], n->S), out, ldc, TEPI_BIAS_RELU, P + n->seg_off[b]);
}
static inline TGemm ac_a_l(const jh_acnet* n, const float* P, int rows) {
  return mk_gemm(rows, n->H, n->H, op_dense(OP_KCONT, n->a_feat, n->H), op_dense(OP_KCONT, P + n->seg_off[AC_A_WL], n->H), n->a_h, n->H, TEPI_BIAS_RELU,
                 P + n->seg_off[AC_A_BL]);
}
// the last layer, seg_rows[AC_A_WPI] columns wide, into a_z
static inline TGemm ac_a_pi(const jh_acnet* n, const float* P, int rows) {
  const int w = n->seg_rows[AC_A_WPI];
  return mk_gemm(rows, w, n->H, op_dense(OP_KCONT, n->a_h, n->H), op_dense(OP_KCONT, P + n->seg_off[AC_A_WPI], n->H), n->a_z, w, TEPI_BIAS, P + n->seg_off[AC_A_BPI]);
}
// actor(x)'s three layers on `rows` rows, one launch each -> a_z
int ac_actor_forward(jh_acnet* n, const float* P, const float* d_x, int rows, hipStream_t st);

// ---- critic loss and Polyak average (the kernels: jh_acnet.hip)
// y = r + (1 - d) * gamma * (min_i q_i' [- alpha * logp']), loss_i = mean((y - q_i)^2), d(loss_i)/d(q_i) = 2 (q_i - y) / B, max_Q = max_b y.
// The first seven members are the caller's; ac_critic_back fills the rest from the object.
struct CriticLossArgs {
  const float *reward, *done;
  float gamma;
  float *y, *stats;          // y [B] (optional); stats = {loss_1, loss_2 (0 for one critic), max_Q, arrival mark}
  const float *logp, *alpha;  // the entropy term: logp' [B] and the alpha in use (ONE float); both null: none (TD3, DDPG)
  int B, n, gstride;          // n critics; grad of critic c starts at c * gstride
  const float *q, *qn;        // [n][B]
  float* grad;                // [n][B]
};
int ac_critic_loss(const CriticLossArgs& a, hipStream_t st);
int ac_polyak(int64_t n, const float* p, float* t, double tau, hipStream_t st);

// ---- the critic update in two halves; the caller launches its action kernel (a_z -> a') in between.
// front, levels 1-3: the policy `actor` (a parameter bucket, online or target) on s' beside the online critics on (s, a)
int ac_critic_front(jh_acnet* n, const float* actor, const float* d_x, const float* d_action, int B, hipStream_t st);
// back, levels 4-6 + loss + the critics' backward + their Adam: the target critics on (s', a_next); q_on [nc][B] takes the online q
int ac_critic_back(jh_acnet* n, const float* d_x, const float* d_action, int B, const float* a_next, float* q_on, CriticLossArgs loss, hipStream_t st);

// ---- the actor update in four pieces; the caller launches its action kernel after the first, its seed after the second, its way back
// through the action kernel after the third.  ncq: how many critics judge the action (critics 0 .. ncq - 1).
int ac_actor_trunk(jh_acnet* n, const float* d_x, int B, int ncq, hipStream_t st);                                   // 3 launches -> a_z; the critics' head.l(s) ride in the first
int ac_actor_q(jh_acnet* n, const float* action, int B, int ncq, float* q, hipStream_t st);                          // 3 launches -> q [ncq][B]
int ac_actor_dact(jh_acnet* n, int B, int ncq, float* da2, hipStream_t st);                                          // 3 launches: dq -> da (critic 0), da2 (critic 1)
int ac_actor_backward(jh_acnet* n, const float* d_x, int B, hipStream_t st);                                         // 4 launches: dz [B][head] -> the actor's gradients, its Adam
