// Intrinsic curiosity module of ICM-PPO (core/agent/icm_ppo.py:84-218, core/network/icm.py:8-34, 99-218, core/network/utils.py:6-52,
// core/network/rnd.py:9-10) on the device:
//   jh_icmnet_*  the feature trunk fc1 -> bn1 -> ELU -> fc2 -> bn2 -> ELU on s (bn1_next after fc1 and NO batch norm after fc2 on s'), the
//                forward model forward_fc2([relu(forward_fc1([phi | a])) | a]) and the inverse model inverse_fc2(relu(inverse_fc1([phi | phi'])));
//                the running moments of the observations and of the intrinsic reward, the discounted reward filter, the no-grad reward pass
//                over a whole rollout, and one minibatch update (forward, both losses, backward, global-norm clip, Adam).
// Every dense contraction runs on the tile engine (jh_tgemm.hip) under the call-site name "dense", independent layers sharing a grouped
// launch.  Gather + normalise + clip, batch norm under BATCH statistics fused with the activation (the module is never put into eval mode;
// the running statistics are advanced by the same kernel) and its backward, the observation moments and the reward filter are
// jh_curiosity.h's, shared with RND-PPO's module (jh_rnd.hip) and instantiated here with ELU; the kernels of this file are the two-headed
// loss and the raw intrinsic reward.  No atomics and no spinning: every sum has a fixed order, so two runs (and a graph replay) give the
// same bits.
#include "jh_curiosity.h"

namespace {

constexpr int kF = kCurF, kMaxBatch = kCurMaxBatch;

enum { IC_FC1_W, IC_FC1_B, IC_FC2_W, IC_FC2_B, IC_FF1_W, IC_FF1_B, IC_FF2_W, IC_FF2_B, IC_IF1_W, IC_IF1_B, IC_IF2_W, IC_IF2_B,
       IC_BN1_W, IC_BN1_B, IC_BN2_W, IC_BN2_B, IC_BN1N_W, IC_BN1N_B, IC_SEG_MAX };
constexpr int kSegPlain = IC_BN1_W;

}  // namespace

struct jh_icmnet {
  NetCore core;
  FlatOptim opt;
  int S = 0, H = 0, A = 0, cont = 0, W = 0, maxB = 0;
  int ac = 0;    // action columns of the forward model: 1 (the index as a float) | A
  int nout = 0;  // outputs of the inverse model: A
  int ldf = 0, ldf2 = 0;  // row strides of [phi | a] and [relu(forward_fc1) | a], rounded up to 4 floats
  bool obs_norm = false, ri_norm = false, bn = false;
  float eta = 0.f, gamma = 0.f;
  int nseg = 0;
  int64_t seg_off[IC_SEG_MAX] = {0};
  int seg_rows[IC_SEG_MAX] = {0}, seg_cols[IC_SEG_MAX] = {0};
  int64_t n_params = 0;
  float *p = nullptr, *g = nullptr, *m = nullptr, *v = nullptr;  // borrowed flat buckets
  // statistics block: rms_obs mean [S], var [S], count | rms_ri mean, var, count | rewems [W] | running mean, var of bn1 [H], bn2 [256], bn1_next [H]
  float* blk = nullptr;
  int64_t blk_floats = 0;
  int o_obs_mean = 0, o_obs_var = 0, o_obs_cnt = 0, o_ri = 0, o_rew = 0, o_bn1 = 0, o_bn2 = 0, o_bn1n = 0;
  // activations: x [2B][S], z1 / a1 [2B][H], z2 [2B][256], cat [B][512] = [phi | phi'], fin [B][ldf] = [phi | a], fin2 [B][ldf2] = [fh | a]
  float *x = nullptr, *z1 = nullptr, *a1 = nullptr, *z2 = nullptr, *cat = nullptr, *fin = nullptr, *fin2 = nullptr, *ih = nullptr, *xf = nullptr, *xi = nullptr;
  float *dxf = nullptr, *dxi = nullptr, *dfh = nullptr, *dih = nullptr, *dphif = nullptr, *dcat = nullptr, *dz2 = nullptr, *da1 = nullptr, *dz1 = nullptr;
  float* save = nullptr;  // batch mean and 1 / sqrt(var + eps) of bn1 [2][H], bn2 [2][256], bn1_next [2][H]
  float* ri_raw = nullptr;  // [B]
};

namespace {

int icm_layout(jh_icmnet* n, int32_t S, int32_t H, int32_t A, int32_t cont, int32_t bn) {
  JH_ARG(S > 0 && H > 0 && H % 4 == 0 && (cont == 0 || cont == 1));
  JH_ARG(cont ? (A >= 1 && A <= 19) : (A >= 1 && A <= 39));  // the policy-value net's range (jh_pponet_create: <= 40 head outputs)
  n->S = S; n->H = H; n->A = A; n->cont = cont; n->bn = bn != 0;
  n->ac = cont ? A : 1;
  n->nout = A;
  n->ldf = (int)up4(kF + n->ac);
  n->ldf2 = (int)up4(H + n->ac);
  auto seg = [&](int id, int rows, int cols) { n->seg_rows[id] = rows; n->seg_cols[id] = cols; };
  seg(IC_FC1_W, H, S); seg(IC_FC1_B, 1, H); seg(IC_FC2_W, kF, H); seg(IC_FC2_B, 1, kF);
  seg(IC_FF1_W, H, kF + n->ac); seg(IC_FF1_B, 1, H); seg(IC_FF2_W, kF, H + n->ac); seg(IC_FF2_B, 1, kF);
  seg(IC_IF1_W, H, 2 * kF); seg(IC_IF1_B, 1, H); seg(IC_IF2_W, A, H); seg(IC_IF2_B, 1, A);
  seg(IC_BN1_W, 1, H); seg(IC_BN1_B, 1, H); seg(IC_BN2_W, 1, kF); seg(IC_BN2_B, 1, kF); seg(IC_BN1N_W, 1, H); seg(IC_BN1N_B, 1, H);
  n->nseg = n->bn ? IC_SEG_MAX : kSegPlain;
  n->n_params = seg_pack(n->seg_rows, n->seg_cols, 0, n->nseg, n->seg_off);
  return JH_OK;
}

// ---------------------------------------------------------------------------------- the loss with two heads
// l_f = mse(x_forward, phi'.detach()) over b * 256 elements (icm.py:127), l_i = cross entropy against the action index | mse against the
// action (icm.py:137-140); the gradients of beta l_f + (1 - beta) l_i with respect to x_forward and x_inverse (icm_ppo.py:185); the
// statistics row {l_f, l_i, 0, arrival mark}.  One workgroup, fixed order.
struct IcmLossArgs {
  int b, nout, cont, ldf;
  const float *xf, *cat, *xi, *fin;
  double beta;
  float *dxf, *dxi, *stats;
};
__global__ void __launch_bounds__(1024) jh_icm_loss_kernel(IcmLossArgs a) {
  __shared__ double s_red[16];
  const int b = a.b, A = a.nout;
  const int64_t nf = (int64_t)b * kF;
  const float cf = (float)(a.beta * 2.0 / (double)nf);
  double lf = 0.0, li = 0.0;
  for (int64_t i = threadIdx.x; i < nf; i += 1024) {
    const int64_t r = i >> 8;
    const int c = (int)(i & 255);
    const float d = a.xf[i] - a.cat[r * 2 * kF + kF + c];
    lf += (double)d * (double)d;
    a.dxf[i] = cf * d;
  }
  for (int r = threadIdx.x; r < b; r += 1024) {
    const float* z = a.xi + (size_t)r * A;
    float* dz = a.dxi + (size_t)r * A;
    const float* act = a.fin + (size_t)r * a.ldf + kF;
    if (a.cont) {
      const float ci = (float)((1.0 - a.beta) * 2.0 / ((double)b * (double)A));
      for (int k = 0; k < A; ++k) {
        const float d = z[k] - act[k];
        li += (double)d * (double)d;
        dz[k] = ci * d;
      }
    } else {
      const float ci = (float)((1.0 - a.beta) / (double)b);
      int ak = (int)act[0];
      ak = ak < 0 ? 0 : (ak >= A ? A - 1 : ak);
      float zm = z[0];
      for (int k = 1; k < A; ++k) zm = fmaxf(zm, z[k]);
      double se = 0.0;
      for (int k = 0; k < A; ++k) se += exp((double)z[k] - (double)zm);
      const double lse = (double)zm + log(se);
      li += lse - (double)z[ak];
      for (int k = 0; k < A; ++k) dz[k] = ci * (float)(exp((double)z[k] - lse) - (k == ak ? 1.0 : 0.0));
    }
  }
  lf = jh_block_reduce(lf, s_red, JhAdd(), 0.0);
  li = jh_block_reduce(li, s_red, JhAdd(), 0.0);
  if (threadIdx.x == 0 && a.stats) {
    a.stats[0] = (float)(lf / (double)nf);
    a.stats[1] = (float)(li / (a.cont ? (double)b * (double)A : (double)b));
    a.stats[2] = 0.f;
    __threadfence_system();  // payload before the arrival mark (mapped host memory, jh_host_wait_marks)
    a.stats[3] = 0.f;
  }
}

// ---------------------------------------------------------------------------------- intrinsic reward
// r_i = eta / 2 * sum_j |x_forward - phi'| (icm.py:210): a wave per row
__global__ void __launch_bounds__(256) jh_icm_ri_kernel(int rows, const float* __restrict__ xf, const float* __restrict__ cat, float half_eta, float* __restrict__ ri) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  const float4 f = reinterpret_cast<const float4*>(xf + (size_t)r * kF)[lane];
  const float4 p = reinterpret_cast<const float4*>(cat + (size_t)r * 2 * kF + kF)[lane];
  float s = (fabsf(f.x - p.x) + fabsf(f.y - p.y)) + (fabsf(f.z - p.z) + fabsf(f.w - p.w));
  s = jh_wave_sum(s);
  if (lane == 0) ri[r] = half_eta * s;
}

// ---------------------------------------------------------------------------------- host side
inline const float* P(const jh_icmnet* n, int s) { return n->p + n->seg_off[s]; }
inline float* G(const jh_icmnet* n, int s) { return n->g + n->seg_off[s]; }

int icm_prep(jh_icmnet* n, const float* state, const float* next_state, const float* action, const int64_t* idx, int b, int64_t n_rows, hipStream_t st) {
  PrepArgs a{};
  a.b = b; a.S = n->S; a.ac = n->ac; a.halves = 2; a.fcol = kF; a.fcol2 = n->H; a.ldf = n->ldf; a.ldf2 = n->ldf2; a.n_rows = n_rows;
  a.src[0] = state; a.src[1] = next_state; a.action = action; a.idx = idx;
  a.mean = n->obs_norm ? n->blk + n->o_obs_mean : nullptr;
  a.var = n->blk + n->o_obs_var;
  a.x = n->x; a.fin = n->fin; a.fin2 = n->fin2;
  const int64_t total = cur_prep_threads(a);
  JH_LAUNCH_NAMED("jh_icm_prep_kernel", jh_cur_prep_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
  JH_LAUNCH_CHECK();
  return JH_OK;
}

BnHalf icm_bn_half(const jh_icmnet* n, int w_seg, int o_run, int C, float* save, float* out0, int ld0, float* out1, int ld1) {
  BnHalf h{};
  if (n->bn && w_seg >= 0) {
    h.gamma = P(n, w_seg); h.beta = P(n, w_seg + 1);
    h.rmean = n->blk + o_run; h.rvar = n->blk + o_run + C;
    h.smean = save; h.sinv = save + C;
  }
  h.out0 = out0; h.ld0 = ld0; h.out1 = out1; h.ld1 = ld1;
  return h;
}

// x (2b rows, prepared) -> x_forward, x_inverse; every activation the backward needs stays in the object.  6 launches.
int icm_forward(jh_icmnet* n, int b, hipStream_t st) {
  const int H = n->H, S = n->S, ac = n->ac;
  TGemm g[2];
  int rc;
  g[0] = mk_gemm(2 * b, H, S, op_dense(OP_KCONT, n->x, S), op_dense(OP_KCONT, P(n, IC_FC1_W), S), n->z1, H, TEPI_BIAS, P(n, IC_FC1_B));
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 1, st))) return rc;
  {
    BnFwdArgs a{};
    a.z = n->z1; a.b = b; a.C = H;
    a.h[0] = icm_bn_half(n, IC_BN1_W, n->o_bn1, H, n->save, n->a1, H, nullptr, 0);
    a.h[1] = icm_bn_half(n, IC_BN1N_W, n->o_bn1n, H, n->save + 2 * H + 2 * kF, n->a1 + (size_t)b * H, H, nullptr, 0);
    JH_LAUNCH_NAMED("jh_icm_bn_elu_kernel", jh_cur_bn_act_kernel<CUR_ELU>, dim3((unsigned)((H + 15) / 16), 2), dim3(256), 0, st, a);
    JH_LAUNCH_CHECK();
  }
  g[0] = mk_gemm(2 * b, kF, H, op_dense(OP_KCONT, n->a1, H), op_dense(OP_KCONT, P(n, IC_FC2_W), H), n->z2, kF, TEPI_BIAS, P(n, IC_FC2_B));
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 1, st))) return rc;
  {
    BnFwdArgs a{};
    a.z = n->z2; a.b = b; a.C = kF;
    a.h[0] = icm_bn_half(n, IC_BN2_W, n->o_bn2, kF, n->save + 2 * H, n->cat, 2 * kF, n->fin, n->ldf);
    a.h[1] = icm_bn_half(n, -1, 0, kF, nullptr, n->cat + kF, 2 * kF, nullptr, 0);  // no batch norm after fc2 on s' (icm.py:32)
    JH_LAUNCH_NAMED("jh_icm_bn_elu_kernel", jh_cur_bn_act_kernel<CUR_ELU>, dim3(kF / 16, 2), dim3(256), 0, st, a);
    JH_LAUNCH_CHECK();
  }
  g[0] = mk_gemm(b, H, kF + ac, op_dense(OP_KCONT, n->fin, n->ldf), op_dense(OP_KCONT, P(n, IC_FF1_W), kF + ac), n->fin2, n->ldf2, TEPI_BIAS_RELU, P(n, IC_FF1_B));
  g[1] = mk_gemm(b, H, 2 * kF, op_dense(OP_KCONT, n->cat, 2 * kF), op_dense(OP_KCONT, P(n, IC_IF1_W), 2 * kF), n->ih, H, TEPI_BIAS_RELU, P(n, IC_IF1_B));
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 2, st))) return rc;
  g[0] = mk_gemm(b, kF, H + ac, op_dense(OP_KCONT, n->fin2, n->ldf2), op_dense(OP_KCONT, P(n, IC_FF2_W), H + ac), n->xf, kF, TEPI_BIAS, P(n, IC_FF2_B));
  g[1] = mk_gemm(b, n->nout, H, op_dense(OP_KCONT, n->ih, H), op_dense(OP_KCONT, P(n, IC_IF2_W), H), n->xi, n->nout, TEPI_BIAS, P(n, IC_IF2_B));
  return core_tgemm(&n->core, "jh_tgemm_dense", g, 2, st);
}

// d(x_forward), d(x_inverse) -> the gradient bucket.  4 grouped GEMM launches and the two batch-norm backward kernels.
int icm_backward(jh_icmnet* n, int b, hipStream_t st) {
  const int H = n->H, S = n->S, ac = n->ac, A = n->nout;
  TGemm g[4];
  int rc;
  g[0] = mk_gemm(kF, H + ac, b, op_dense(OP_XCONT, n->dxf, kF), op_dense(OP_XCONT, n->fin2, n->ldf2), G(n, IC_FF2_W), H + ac, TEPI_NONE, nullptr, nullptr, 0, G(n, IC_FF2_B));
  g[1] = mk_gemm(b, H, kF, op_dense(OP_KCONT, n->dxf, kF), op_dense(OP_XCONT, P(n, IC_FF2_W), H + ac), n->dfh, H, TEPI_MASK, nullptr, n->fin2, n->ldf2);
  g[2] = mk_gemm(A, H, b, op_dense(OP_XCONT, n->dxi, A), op_dense(OP_XCONT, n->ih, H), G(n, IC_IF2_W), H, TEPI_NONE, nullptr, nullptr, 0, G(n, IC_IF2_B));
  g[3] = mk_gemm(b, H, A, op_dense(OP_KCONT, n->dxi, A), op_dense(OP_XCONT, P(n, IC_IF2_W), H), n->dih, H, TEPI_MASK, nullptr, n->ih, H);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 4, st))) return rc;
  g[0] = mk_gemm(H, kF + ac, b, op_dense(OP_XCONT, n->dfh, H), op_dense(OP_XCONT, n->fin, n->ldf), G(n, IC_FF1_W), kF + ac, TEPI_NONE, nullptr, nullptr, 0, G(n, IC_FF1_B));
  g[1] = mk_gemm(b, kF, H, op_dense(OP_KCONT, n->dfh, H), op_dense(OP_XCONT, P(n, IC_FF1_W), kF + ac), n->dphif, kF, TEPI_NONE);
  g[2] = mk_gemm(H, 2 * kF, b, op_dense(OP_XCONT, n->dih, H), op_dense(OP_XCONT, n->cat, 2 * kF), G(n, IC_IF1_W), 2 * kF, TEPI_NONE, nullptr, nullptr, 0, G(n, IC_IF1_B));
  g[3] = mk_gemm(b, 2 * kF, H, op_dense(OP_KCONT, n->dih, H), op_dense(OP_XCONT, P(n, IC_IF1_W), 2 * kF), n->dcat, 2 * kF, TEPI_NONE);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 4, st))) return rc;
  {
    BnBwdArgs a{};
    a.z = n->z2; a.dz = n->dz2; a.b = b; a.C = kF;
    BnBwdHalf& h0 = a.h[0];
    h0.dy0 = n->dphif; h0.ldd0 = kF; h0.dy1 = n->dcat; h0.ldd1 = 2 * kF; h0.y = n->cat; h0.ldy = 2 * kF;
    if (n->bn) { h0.gamma = P(n, IC_BN2_W); h0.smean = n->save + 2 * H; h0.sinv = n->save + 2 * H + kF; h0.dgamma = G(n, IC_BN2_W); h0.dbeta = G(n, IC_BN2_B); }
    BnBwdHalf& h1 = a.h[1];
    h1.dy0 = n->dcat + kF; h1.ldd0 = 2 * kF; h1.y = n->cat + kF; h1.ldy = 2 * kF;
    JH_LAUNCH_NAMED("jh_icm_bn_elu_bwd_kernel", jh_cur_bn_act_bwd_kernel<CUR_ELU>, dim3(kF / 16, 2), dim3(256), 0, st, a);
    JH_LAUNCH_CHECK();
  }
  g[0] = mk_gemm(kF, H, 2 * b, op_dense(OP_XCONT, n->dz2, kF), op_dense(OP_XCONT, n->a1, H), G(n, IC_FC2_W), H, TEPI_NONE, nullptr, nullptr, 0, G(n, IC_FC2_B));
  g[1] = mk_gemm(2 * b, H, kF, op_dense(OP_KCONT, n->dz2, kF), op_dense(OP_XCONT, P(n, IC_FC2_W), H), n->da1, H, TEPI_NONE);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 2, st))) return rc;
  {
    BnBwdArgs a{};
    a.z = n->z1; a.dz = n->dz1; a.b = b; a.C = H;
    for (int hh = 0; hh < 2; ++hh) {
      BnBwdHalf& h = a.h[hh];
      h.dy0 = n->da1 + (size_t)hh * b * H; h.ldd0 = H; h.y = n->a1 + (size_t)hh * b * H; h.ldy = H;
      if (n->bn) {
        const int w = hh ? IC_BN1N_W : IC_BN1_W;
        float* save = n->save + (hh ? 2 * H + 2 * kF : 0);
        h.gamma = P(n, w); h.smean = save; h.sinv = save + H; h.dgamma = G(n, w); h.dbeta = G(n, w + 1);
      }
    }
    JH_LAUNCH_NAMED("jh_icm_bn_elu_bwd_kernel", jh_cur_bn_act_bwd_kernel<CUR_ELU>, dim3((unsigned)((H + 15) / 16), 2), dim3(256), 0, st, a);
    JH_LAUNCH_CHECK();
  }
  g[0] = mk_gemm(H, S, 2 * b, op_dense(OP_XCONT, n->dz1, H), op_dense(OP_XCONT, n->x, S), G(n, IC_FC1_W), S, TEPI_NONE, nullptr, nullptr, 0, G(n, IC_FC1_B));
  return core_tgemm(&n->core, "jh_tgemm_dense", g, 1, st);
}

int icm_rows_ok(const jh_icmnet* n, int rows) {
  JH_ARG(rows >= 1 && rows <= n->maxB);
  JH_ARG(!n->bn || rows >= 2);  // a training-mode batch norm needs more than one value per channel
  return JH_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------- the object
JH_EXPORT int64_t jh_icmnet_param_count_for(int32_t S, int32_t H, int32_t A, int32_t continuous, int32_t batch_norm) {
  jh_icmnet tmp;
  return icm_layout(&tmp, S, H, A, continuous, batch_norm) ? -1 : tmp.n_params;
}

JH_EXPORT int jh_icmnet_create(jh_ctx* ctx, int32_t S, int32_t H, int32_t A, int32_t continuous, int32_t num_workers, int32_t max_batch, int32_t flags, double eta,
                               double gamma, float* d_params, float* d_grads, float* d_m, float* d_v, jh_icmnet** out) {
  JH_ARG(ctx && out && d_params && d_grads && d_m && d_v);
  JH_ARG(num_workers >= 1 && max_batch >= 1 && max_batch <= kMaxBatch && flags >= 0 && flags < 8);
  jh_icmnet* n = new jh_icmnet();
  n->core.ctx = ctx;
  int rc = icm_layout(n, S, H, A, continuous, (flags & JH_ICM_BATCH_NORM) != 0);
  if (!rc && !((int64_t)2 * max_batch * (n->ldf2 > 2 * kF ? n->ldf2 : 2 * kF) < ((int64_t)1 << 31) && (int64_t)2 * max_batch * S < ((int64_t)1 << 31)))
    rc = jh_fail(JH_ERR_ARG, "jh_icmnet_create: max_batch %d x hidden %d exceeds the tile engine's 32-bit indexing", max_batch, H);
  if (rc) {
    delete n;
    return rc;
  }
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) {
    delete n;
    return jh_fail(JH_ERR_HIP, "jh_icmnet_create: hipSetDevice -> %s", hipGetErrorString(e));
  }
  n->W = num_workers; n->maxB = max_batch;
  n->obs_norm = (flags & JH_ICM_OBS_NORMALIZE) != 0; n->ri_norm = (flags & JH_ICM_RI_NORMALIZE) != 0;
  n->eta = (float)(eta * 0.5); n->gamma = (float)gamma;
  n->p = d_params; n->g = d_grads; n->m = d_m; n->v = d_v;
  int o = 0;
  n->o_obs_mean = o; o += S;
  n->o_obs_var = o; o += S;
  n->o_obs_cnt = o; o += 1;
  n->o_ri = o; o += 3;
  n->o_rew = o; o += num_workers;
  n->o_bn1 = o; o += 2 * H;
  n->o_bn2 = o; o += 2 * kF;
  n->o_bn1n = o; o += 2 * H;
  n->blk_floats = o;
  const size_t B = (size_t)max_batch;
  auto A4 = [&](float** p, size_t floats) { if (!rc) rc = core_alloc(&n->core, "jh_icmnet", (void**)p, floats * sizeof(float), true); };
  rc = optim_init(&n->core, "jh_icmnet", &n->opt);
  A4(&n->blk, (size_t)n->blk_floats);
  A4(&n->x, 2 * B * S); A4(&n->z1, 2 * B * H); A4(&n->a1, 2 * B * H); A4(&n->z2, 2 * B * kF); A4(&n->cat, B * 2 * kF); A4(&n->fin, B * n->ldf);
  A4(&n->fin2, B * n->ldf2); A4(&n->ih, B * H); A4(&n->xf, B * kF); A4(&n->xi, B * n->nout);
  A4(&n->dxf, B * kF); A4(&n->dxi, B * n->nout); A4(&n->dfh, B * H); A4(&n->dih, B * H); A4(&n->dphif, B * kF); A4(&n->dcat, B * 2 * kF);
  A4(&n->dz2, 2 * B * kF); A4(&n->da1, 2 * B * H); A4(&n->dz1, 2 * B * H); A4(&n->save, (size_t)4 * H + 2 * kF); A4(&n->ri_raw, B);
  if (!rc) rc = core_workspace(&n->core, "jh_icmnet", (size_t)8 << 20, 8192);  // 32 MB of split-K partials
  if (!rc) {
    // a fresh module: RunningMeanStd's count 1e-4 (utils.py:19-24), running_var 1 (torch.nn.BatchNorm1d)
    std::vector<float> h((size_t)n->blk_floats, 0.f);
    h[n->o_obs_cnt] = 1e-4f;
    h[n->o_ri + 2] = 1e-4f;
    for (int i = 0; i < H; ++i) h[n->o_bn1 + H + i] = h[n->o_bn1n + H + i] = 1.f;
    for (int i = 0; i < kF; ++i) h[n->o_bn2 + kF + i] = 1.f;
    e = hipMemcpy(n->blk, h.data(), sizeof(float) * h.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = jh_fail(JH_ERR_HIP, "jh_icmnet_create: hipMemcpy -> %s", hipGetErrorString(e));
  }
  if (!rc) rc = core_drain();
  if (rc) {
    core_release(&n->core);
    delete n;
    return rc;
  }
  *out = n;
  return JH_OK;
}

JH_EXPORT void jh_icmnet_destroy(jh_icmnet* n) {
  if (!n) return;
  core_release(&n->core);
  delete n;
}

JH_EXPORT int32_t jh_icmnet_segment_count(const jh_icmnet* n) { return n ? n->nseg : 0; }
JH_EXPORT int jh_icmnet_segment(const jh_icmnet* n, int32_t i, int64_t* offset, int32_t* rows, int32_t* cols) {
  return seg_query(n, n ? n->nseg : 0, i, offset, rows, cols);
}
JH_EXPORT int jh_icmnet_set_hyper(jh_icmnet* n, double lr, double beta1, double beta2, double eps, int64_t step, jh_stream stream) {
  JH_ARG(n != nullptr);
  return jh_hyper_upload(n->core.ctx, n->opt.hyper, lr, beta1, beta2, eps, step, 0, jh_s(stream));
}
JH_EXPORT int jh_icmnet_set_lr(jh_icmnet* n, double lr, jh_stream stream) {
  JH_ARG(n != nullptr);
  return jh_hyper_upload_lr(n->core.ctx, n->opt.hyper, lr, jh_s(stream));
}

JH_EXPORT int64_t jh_icmnet_stats_floats(const jh_icmnet* n) { return n ? n->blk_floats : 0; }
JH_EXPORT int jh_icmnet_stats_get(jh_icmnet* n, float* h_out, jh_stream stream) {
  JH_ARG(n && h_out);
  JH_HIP(hipMemcpyAsync(h_out, n->blk, sizeof(float) * (size_t)n->blk_floats, hipMemcpyDeviceToHost, jh_s(stream)));
  JH_HIP(hipStreamSynchronize(jh_s(stream)));
  return JH_OK;
}
JH_EXPORT int jh_icmnet_stats_set(jh_icmnet* n, const float* h_in, jh_stream stream) {
  JH_ARG(n && h_in);
  JH_HIP(hipMemcpyAsync(n->blk, h_in, sizeof(float) * (size_t)n->blk_floats, hipMemcpyHostToDevice, jh_s(stream)));
  JH_HIP(hipStreamSynchronize(jh_s(stream)));
  return JH_OK;
}

// icm.update_rms_obs(next_state) (icm_ppo.py:98)
JH_EXPORT int jh_icmnet_obs_update(jh_icmnet* n, const float* d_next_state, int32_t rows, jh_stream stream) {
  JH_ARG(n && d_next_state);
  JH_ARG(rows >= 2 && rows <= n->maxB);  // x.std of one row is NaN
  JH_LAUNCH_NAMED("jh_icm_obs_update_kernel", jh_cur_obs_update_kernel, dim3(1), dim3(256), 0, jh_s(stream), rows, n->S, d_next_state, n->blk + n->o_obs_mean, n->blk + n->o_obs_var, n->blk + n->o_obs_cnt);
  JH_LAUNCH_CHECK();
  return JH_OK;
}

// r_i, _, _ = icm(state, action, next_state, update_ri=True); reward = ext * reward + int * r_i (icm_ppo.py:99-102).  9 launches.
JH_EXPORT int jh_icmnet_reward(jh_icmnet* n, const float* d_state, const float* d_next_state, const float* d_action, int32_t rows, float extrinsic_coeff,
                               float intrinsic_coeff, float* d_reward, float* d_ri_mean, float* d_ri_raw, float* d_ri, jh_stream stream) {
  JH_ARG(n && d_state && d_next_state && d_action && d_reward);
  int rc = icm_rows_ok(n, rows);
  if (rc) return rc;
  JH_ARG(rows >= 2 && rows % n->W == 0);  // x.std of one row; r_i.view(num_workers, -1)
  hipStream_t st = jh_s(stream);
  if ((rc = icm_prep(n, d_state, d_next_state, d_action, nullptr, rows, rows, st))) return rc;
  if ((rc = icm_forward(n, rows, st))) return rc;
  float* raw = d_ri_raw ? d_ri_raw : n->ri_raw;
  JH_LAUNCH(jh_icm_ri_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, rows, n->xf, n->cat, n->eta, raw);
  JH_LAUNCH_CHECK();
  RewardArgs a{};
  a.rows = rows; a.W = n->W; a.T = rows / n->W; a.ri_norm = n->ri_norm; a.ri_raw = raw; a.ri_blk = n->blk + n->o_ri; a.rewems = n->blk + n->o_rew;
  a.gamma = n->gamma; a.ext = extrinsic_coeff; a.intr = intrinsic_coeff; a.reward = d_reward; a.ri_out = d_ri; a.ri_mean = d_ri_mean;
  JH_LAUNCH_NAMED("jh_icm_reward_kernel", jh_cur_reward_kernel, dim3(1), dim3(256), 0, st, a);
  JH_LAUNCH_CHECK();
  return JH_OK;
}

// One minibatch (icm_ppo.py:177, 185, 194-199): rows d_idx[0 .. b) of the n_rows-row rollout arrays (NULL: rows 0 .. b - 1).
// Launches: prepare, 6 of the forward, loss, 6 of the backward, gradient norm, Adam = 16.
JH_EXPORT int jh_icmnet_update(jh_icmnet* n, const float* d_state, const float* d_next_state, const float* d_action, const int64_t* d_idx, int32_t b,
                               int64_t n_rows, double beta, float max_norm, float* d_stats, jh_stream stream) {
  JH_ARG(n && d_state && d_next_state && d_action);
  int rc = icm_rows_ok(n, b);
  if (rc) return rc;
  JH_ARG(n_rows >= (d_idx ? 1 : b) && beta >= 0.0 && beta <= 1.0 && max_norm >= 0.f);
  hipStream_t st = jh_s(stream);
  if ((rc = icm_prep(n, d_state, d_next_state, d_action, d_idx, b, n_rows, st))) return rc;
  if ((rc = icm_forward(n, b, st))) return rc;
  IcmLossArgs a{};
  a.b = b; a.nout = n->nout; a.cont = n->cont; a.ldf = n->ldf; a.xf = n->xf; a.cat = n->cat; a.xi = n->xi; a.fin = n->fin; a.beta = beta;
  a.dxf = n->dxf; a.dxi = n->dxi; a.stats = d_stats;
  JH_LAUNCH(jh_icm_loss_kernel, dim3(1), dim3(1024), 0, st, a);
  JH_LAUNCH_CHECK();
  if ((rc = icm_backward(n, b, st))) return rc;
  return jh_flat_adam_step(n->n_params, n->p, n->g, n->m, n->v, n->opt.hyper, n->opt.ticket, n->core.norm_partial, max_norm, st);
}
