// What the actor-critic network objects share (jh_td3.hip: jh_acnet_*, jh_sac.hip: jh_sacnet_*): the object's layout and buffers, the layer
// builders of the continuous Q network (network/q_network.py:23-39) and of the policy's trunk (head.l -> relu(l)), and the critics' backward.
// One copy: jh_sacnet embeds a jh_acnet and drives these with it.
#pragma once
#include "jh_fused.h"
#include "jh_tgemm.h"

enum { AC_A_W1, AC_A_B1, AC_A_WL, AC_A_BL, AC_A_WPI, AC_A_BPI, AC_C_W1, AC_C_B1, AC_C_WE, AC_C_BE, AC_C_WL, AC_C_BL, AC_C_WQ, AC_C_BQ, AC_SEG_COUNT };

struct jh_acnet {
  jh_ctx* ctx = nullptr;
  int S = 0, H = 0, A = 0, nc = 0, maxB = 0;
  int64_t seg_off[AC_SEG_COUNT] = {0};  // actor segments: offsets in the actor bucket; critic segments: offsets inside ONE critic
  int seg_rows[AC_SEG_COUNT] = {0}, seg_cols[AC_SEG_COUNT] = {0};
  int64_t nA = 0, nC = 0;  // floats of the actor bucket / of one critic (the critic buckets hold nc of them back to back)
  float *ap = nullptr, *at = nullptr, *ag = nullptr, *am = nullptr, *av = nullptr;
  float *cp = nullptr, *ct = nullptr, *cg = nullptr, *cm = nullptr, *cv = nullptr;
  float *hyper_a = nullptr, *hyper_c = nullptr, *norm_partial = nullptr;
  unsigned *ticket_a = nullptr, *ticket_c = nullptr;
  // actor activations [maxB] rows: feat, h, z (pre-tanh), a
  float *a_feat = nullptr, *a_h = nullptr, *a_z = nullptr, *a_out = nullptr;
  // critic activations, set 0 = online, 1 = target: cat [nc][maxB][2H] = [head(s) | relu(e(a))], h [nc][maxB][H], q [nc][maxB]
  float *c_cat[2] = {nullptr, nullptr}, *c_h[2] = {nullptr, nullptr}, *c_q[2] = {nullptr, nullptr};
  // backward: dq [nc][maxB], dh [nc][maxB][H], dcat [nc][maxB][2H], da / dz [maxB][A], d(actor h) / d(actor feat) [maxB][H]
  float *dq = nullptr, *dh = nullptr, *dcat = nullptr, *da = nullptr, *dz = nullptr, *dah = nullptr, *dafeat = nullptr;
  float* ws = nullptr;
  size_t ws_floats = 0;
  unsigned* cnt = nullptr;
  int cnt_slots = 0;
  std::vector<void*> owned;
};

static int ac_layout(jh_acnet* n, int32_t S, int32_t H, int32_t A, int32_t nc, int32_t max_batch) {
  JH_ARG(S > 0 && H > 0 && H % 4 == 0 && A >= 1 && max_batch > 0 && (nc == 1 || nc == 2));
  JH_ARG((int64_t)2 * max_batch * 2 * H < ((int64_t)1 << 31) && (int64_t)max_batch * (S > A ? S : A) < ((int64_t)1 << 31));  // the tile engine indexes in 32 bits
  n->S = S; n->H = H; n->A = A; n->nc = nc; n->maxB = max_batch;
  auto seg = [&](int id, int rows, int cols) { n->seg_rows[id] = rows; n->seg_cols[id] = cols; };
  seg(AC_A_W1, H, S); seg(AC_A_B1, 1, H); seg(AC_A_WL, H, H); seg(AC_A_BL, 1, H); seg(AC_A_WPI, A, H); seg(AC_A_BPI, 1, A);
  seg(AC_C_W1, H, S); seg(AC_C_B1, 1, H); seg(AC_C_WE, H, A); seg(AC_C_BE, 1, H); seg(AC_C_WL, H, 2 * H); seg(AC_C_BL, 1, H);
  seg(AC_C_WQ, 1, H); seg(AC_C_BQ, 1, 1);
  int64_t off = 0;
  for (int i = AC_A_W1; i <= AC_A_BPI; ++i) {
    n->seg_off[i] = off;
    off = (off + (int64_t)n->seg_rows[i] * n->seg_cols[i] + 3) & ~(int64_t)3;
  }
  n->nA = off;
  off = 0;
  for (int i = AC_C_W1; i <= AC_C_BQ; ++i) {
    n->seg_off[i] = off;
    off = (off + (int64_t)n->seg_rows[i] * n->seg_cols[i] + 3) & ~(int64_t)3;
  }
  n->nC = off;
  return JH_OK;
}

static int ac_alloc(jh_acnet* n, void** out, size_t bytes, bool zero) {
  if (bytes == 0) bytes = 16;
  hipError_t e = hipMalloc(out, bytes);
  if (e != hipSuccess) return jh_fail(JH_ERR_NOMEM, "jh_acnet: hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
  n->owned.push_back(*out);
  if (zero) JH_HIP(hipMemset(*out, 0, bytes));
  return JH_OK;
}

static int ac_tgemm(jh_acnet* n, TGemm* probs, int ng, hipStream_t st) {
  TGemmWorkspace w;
  w.ws = n->ws; w.ws_floats = n->ws_floats; w.cnt = n->cnt; w.cnt_slots = n->cnt_slots;
  return jh_tgemm_launch(w, "jh_tgemm_dense", probs, ng, st);
}

// ---- layer builders.  P: the parameter bucket of the actor / of one critic; set: the critic activation set; c: the critic.
static inline TGemm ac_head(const jh_acnet* n, const float* P, int w, int b, const float* x, int rows, float* out, int ldc) {
  return mk_gemm(rows, n->H, n->S, op_dense(OP_KCONT, x, n->S), op_dense(OP_KCONT, P + n->seg_off[w], n->S), out, ldc, TEPI_BIAS_RELU, P + n->seg_off[b]);
}
static inline float* ac_cat(const jh_acnet* n, int set, int c) { return n->c_cat[set] + (size_t)c * n->maxB * 2 * n->H; }
static inline float* ac_ch(const jh_acnet* n, int set, int c) { return n->c_h[set] + (size_t)c * n->maxB * n->H; }
static inline TGemm ac_c_head(const jh_acnet* n, const float* P, int set, int c, const float* x, int rows) {
  return ac_head(n, P, AC_C_W1, AC_C_B1, x, rows, ac_cat(n, set, c), 2 * n->H);
}
static inline TGemm ac_c_embed(const jh_acnet* n, const float* P, int set, int c, const float* act, int rows) {
  return mk_gemm(rows, n->H, n->A, op_dense(OP_KCONT, act, n->A), op_dense(OP_KCONT, P + n->seg_off[AC_C_WE], n->A), ac_cat(n, set, c) + n->H, 2 * n->H,
                 TEPI_BIAS_RELU, P + n->seg_off[AC_C_BE]);
}
static inline TGemm ac_c_l(const jh_acnet* n, const float* P, int set, int c, int rows) {
  return mk_gemm(rows, n->H, 2 * n->H, op_dense(OP_KCONT, ac_cat(n, set, c), 2 * n->H), op_dense(OP_KCONT, P + n->seg_off[AC_C_WL], 2 * n->H), ac_ch(n, set, c), n->H,
                 TEPI_BIAS_RELU, P + n->seg_off[AC_C_BL]);
}
static inline TGemm ac_c_q(const jh_acnet* n, const float* P, int set, int c, int rows, float* out) {
  return mk_gemm(rows, 1, n->H, op_dense(OP_KCONT, ac_ch(n, set, c), n->H), op_dense(OP_KCONT, P + n->seg_off[AC_C_WQ], n->H), out, 1, TEPI_BIAS, P + n->seg_off[AC_C_BQ]);
}
static inline TGemm ac_a_l(const jh_acnet* n, const float* P, int rows) {
  return mk_gemm(rows, n->H, n->H, op_dense(OP_KCONT, n->a_feat, n->H), op_dense(OP_KCONT, P + n->seg_off[AC_A_WL], n->H), n->a_h, n->H, TEPI_BIAS_RELU,
                 P + n->seg_off[AC_A_BL]);
}
static inline TGemm ac_a_pi(const jh_acnet* n, const float* P, int rows) {
  return mk_gemm(rows, n->A, n->H, op_dense(OP_KCONT, n->a_h, n->H), op_dense(OP_KCONT, P + n->seg_off[AC_A_WPI], n->H), n->a_z, n->A, TEPI_BIAS, P + n->seg_off[AC_A_BPI]);
}

// backward of critic c's online activations (set 0) from dq [B] down to d(cat) [B][2H]; weights: also the gradient bucket of that critic;
// !weights: only the `e` half d(cat)[:, H:] is computed, the head half keeps whatever it held
static int ac_critic_backward(jh_acnet* n, int B, const float* d_x, const float* d_action, bool weights, int c0, int c1, hipStream_t st) {
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
  if ((rc = ac_tgemm(n, g, k, st))) return rc;
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
  if ((rc = ac_tgemm(n, g, k, st))) return rc;
  if (!weights) return JH_OK;
  k = 0;
  for (int c = c0; c < c1; ++c) {
    float* G = n->cg + c * n->nC;
    const float* dcat = n->dcat + (size_t)c * n->maxB * 2 * H;
    g[k++] = mk_gemm(H, S, B, op_dense(OP_XCONT, dcat, 2 * H), op_dense(OP_XCONT, d_x, S), G + n->seg_off[AC_C_W1], S, TEPI_NONE, nullptr, nullptr, 0, G + n->seg_off[AC_C_B1]);
    g[k++] = mk_gemm(H, A, B, op_dense(OP_XCONT, dcat + H, 2 * H), op_dense(OP_XCONT, d_action, A), G + n->seg_off[AC_C_WE], A, TEPI_NONE, nullptr, nullptr, 0,
                     G + n->seg_off[AC_C_BE]);
  }
  return ac_tgemm(n, g, k, st);
}
