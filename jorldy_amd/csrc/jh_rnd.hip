// RND-PPO (core/agent/rnd_ppo.py:14-307, core/network/rnd.py:9-52, 159-225, core/network/utils.py:6-52) on the device:
//   jh_rndnet_*             the distillation module: predictor and frozen target, fc1 [H][S] -> bn1 -> ReLU -> fc2 [256][H] -> bn2 -> ReLU each, the
//                           running moments of the observations and of the intrinsic reward, the discounted reward filter, the no-grad reward
//                           pass over a whole rollout and one minibatch update of the predictor (forward, loss, backward, global-norm clip, Adam)
//   jh_rnd_adv_mix          adv = extrinsic_coeff adv_e + intrinsic_coeff adv_i, standardised per row of n_step; mean(ret), mean(ret_i)
//   jh_rnd_ppo_loss_packed  PPO's clipped surrogate and entropy with TWO clipped critics on heads stacked as (pi | v | v_i) or (mu | log_std | v | v_i)
// Every dense contraction runs on the tile engine (jh_tgemm.hip) under the call-site name "dense"; predictor and target read the same input,
// so each layer is ONE grouped launch of two problems and each batch norm ONE launch over the two halves of [2b][C].  Gather + normalise +
// clip, batch norm + activation forward / backward, the observation moments and the reward filter are jh_curiosity.h's, shared with ICM-PPO's
// module and instantiated here with ReLU and with the normalisation in double (CUR_F64: a minibatch may leave a batch norm two or three rows).  No atomics and no spinning: every sum has a fixed order, so two runs (and a graph replay) give the
// same bits.
#include "jh_curiosity.h"
#include "jh_policy_head.h"  // the categorical row and the squashed-Gaussian head element

namespace {

constexpr int kF = kCurF, kMaxBatch = kCurMaxBatch;

// the predictor's tensors first (the only ones with gradients, moments and Adam steps: one contiguous run of the buckets), the frozen target after
enum { RN_FC1P_W, RN_FC1P_B, RN_FC2P_W, RN_FC2P_B, RN_BN1P_W, RN_BN1P_B, RN_BN2P_W, RN_BN2P_B,
       RN_FC1T_W, RN_FC1T_B, RN_FC2T_W, RN_FC2T_B, RN_BN1T_W, RN_BN1T_B, RN_BN2T_W, RN_BN2T_B, RN_SEG_MAX };

}  // namespace

struct jh_rndnet {
  NetCore core;
  FlatOptim opt;
  int S = 0, H = 0, W = 0, maxB = 0;
  bool obs_norm = false, ri_norm = false, bn = false;
  float gamma = 0.f;
  int64_t seg_off[RN_SEG_MAX] = {0};
  int seg_rows[RN_SEG_MAX] = {0}, seg_cols[RN_SEG_MAX] = {0};
  int64_t n_params = 0, n_train = 0;  // n_train: the floats of the predictor's run
  float *p = nullptr, *g = nullptr, *m = nullptr, *v = nullptr;  // borrowed flat buckets
  // statistics block: jh_curiosity.h's head (rms_obs, rms_ri, rewems [W]) | running mean, var of bn1_predict [H], bn2_predict [256], bn1_target [H], bn2_target [256]
  float* blk = nullptr;
  int64_t blk_floats = 0;
  CurBlock cb;
  int o_bn1p = 0, o_bn2p = 0, o_bn1t = 0, o_bn2t = 0;
  // activations: x [B][S]; z1 / a1 [2][B][H] and z2 / a2 [2][B][256] with the predictor in half 0 and the target in half 1 (the halves are b rows apart)
  float *x = nullptr, *z1 = nullptr, *a1 = nullptr, *z2 = nullptr, *a2 = nullptr;
  float *dp = nullptr, *dz2 = nullptr, *da1 = nullptr, *dz1 = nullptr;
  float* save = nullptr;    // batch mean and 1 / sqrt(var + eps) of bn1_predict [2][H], bn2_predict [2][256], bn1_target [2][H], bn2_target [2][256]
  float* ri_raw = nullptr;  // [B]
};

namespace {

int rnd_layout(jh_rndnet* n, int32_t S, int32_t H, int32_t bn) {
  JH_ARG(S > 0 && H > 0 && H % 4 == 0);
  n->S = S; n->H = H; n->bn = bn != 0;
  const int r = n->bn ? 1 : 0;  // without batch norm its segments are empty
  auto seg = [&](int id, int rows, int cols) { n->seg_rows[id] = rows; n->seg_cols[id] = cols; };
  for (int t = 0; t < 2; ++t) {
    const int o = t * RN_FC1T_W;
    seg(o + RN_FC1P_W, H, S); seg(o + RN_FC1P_B, 1, H); seg(o + RN_FC2P_W, kF, H); seg(o + RN_FC2P_B, 1, kF);
    seg(o + RN_BN1P_W, r, H); seg(o + RN_BN1P_B, r, H); seg(o + RN_BN2P_W, r, kF); seg(o + RN_BN2P_B, r, kF);
  }
  n->n_params = seg_pack(n->seg_rows, n->seg_cols, 0, RN_SEG_MAX, n->seg_off);
  n->n_train = n->seg_off[RN_FC1T_W];
  return JH_OK;
}

// ---------------------------------------------------------------------------------- intrinsic reward
// r_i = mean_j (p - t)^2 over the 256 features (rnd.py:217): a wave per row
__global__ void __launch_bounds__(256) jh_rnd_ri_kernel(int rows, const float* __restrict__ p, const float* __restrict__ t, float* __restrict__ ri) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  const float4 f = reinterpret_cast<const float4*>(p + (size_t)r * kF)[lane];
  const float4 q = reinterpret_cast<const float4*>(t + (size_t)r * kF)[lane];
  const double dx = (double)f.x - (double)q.x, dy = (double)f.y - (double)q.y, dz = (double)f.z - (double)q.z, dw = (double)f.w - (double)q.w;
  double s = (dx * dx + dy * dy) + (dz * dz + dw * dw);
  s = jh_wave_sum(s);
  if (lane == 0) ri[r] = (float)(s / (double)kF);
}

// ---------------------------------------------------------------------------------- the loss of one minibatch
// loss = mean_r (mean_j (p - t)^2 / den), den = sqrt(rms_ri.var) + 1e-7 when ri_normalize (rnd.py:217-225, rnd_ppo.py:251-252);
// d(loss)/dp = 2 (p - t) / (256 b den); the statistics row {loss, 0, 0, arrival mark}.  One workgroup, fixed order.
struct RndLossArgs {
  int b;
  const float *p, *t;
  const float* ri_var;  // nullptr: no normalisation
  float *dp, *stats;
};
__global__ void __launch_bounds__(1024) jh_rnd_loss_kernel(RndLossArgs a) {
  __shared__ double s_red[16];
  const int64_t nf = (int64_t)a.b * kF;
  const float den = a.ri_var ? sqrtf(*a.ri_var) + 1e-7f : 1.f;
  const float cf = (float)(2.0 / ((double)nf * (double)den));
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < nf; i += 1024) {
    const float d = a.p[i] - a.t[i];
    acc += (double)d * (double)d;
    a.dp[i] = cf * d;
  }
  acc = jh_block_reduce(acc, s_red, JhAdd(), 0.0);
  if (threadIdx.x == 0 && a.stats) {
    a.stats[0] = (float)(acc / (double)nf / (double)den);
    a.stats[1] = 0.f;
    a.stats[2] = 0.f;
    __threadfence_system();  // payload before the arrival mark (mapped host memory, jh_host_wait_marks)
    a.stats[3] = 0.f;
  }
}

// ---------------------------------------------------------------------------------- host side
inline const float* P(const jh_rndnet* n, int s) { return n->p + n->seg_off[s]; }
inline float* G(const jh_rndnet* n, int s) { return n->g + n->seg_off[s]; }

int rnd_prep(jh_rndnet* n, const float* next_state, const int64_t* idx, int b, int64_t n_rows, hipStream_t st) {
  PrepArgs a{};
  a.b = b; a.S = n->S; a.ac = 0; a.halves = 1; a.n_rows = n_rows;
  a.src[0] = next_state; a.src[1] = next_state; a.idx = idx;
  a.mean = n->obs_norm ? n->blk + n->cb.o_obs_mean : nullptr;
  a.var = n->blk + n->cb.o_obs_var;
  a.x = n->x;
  JH_LAUNCH_NAMED("jh_rnd_prep_kernel", jh_cur_prep_kernel, dim3((unsigned)((cur_prep_threads(a) + 255) / 256)), dim3(256), 0, st, a);
  JH_LAUNCH_CHECK();
  return JH_OK;
}

BnHalf rnd_bn_half(const jh_rndnet* n, int w_seg, int o_run, int C, float* save, float* out) {
  BnHalf h{};
  if (n->bn) {
    h.gamma = P(n, w_seg); h.beta = P(n, w_seg + 1);
    h.rmean = n->blk + o_run; h.rvar = n->blk + o_run + C;
    h.smean = save; h.sinv = save + C;
  }
  h.out0 = out; h.ld0 = C;
  return h;
}

// x (b rows, prepared) -> a2 = [p; t]; every activation the backward needs stays in the object.  4 launches.
int rnd_forward(jh_rndnet* n, int b, hipStream_t st) {
  const int H = n->H, S = n->S;
  const size_t bH = (size_t)b * H, bF = (size_t)b * kF;
  TGemm g[2];
  int rc;
  g[0] = mk_gemm(b, H, S, op_dense(OP_KCONT, n->x, S), op_dense(OP_KCONT, P(n, RN_FC1P_W), S), n->z1, H, TEPI_BIAS, P(n, RN_FC1P_B));
  g[1] = mk_gemm(b, H, S, op_dense(OP_KCONT, n->x, S), op_dense(OP_KCONT, P(n, RN_FC1T_W), S), n->z1 + bH, H, TEPI_BIAS, P(n, RN_FC1T_B));
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 2, st))) return rc;
  {
    BnFwdArgs a{};
    a.z = n->z1; a.b = b; a.C = H;
    a.h[0] = rnd_bn_half(n, RN_BN1P_W, n->o_bn1p, H, n->save, n->a1);
    a.h[1] = rnd_bn_half(n, RN_BN1T_W, n->o_bn1t, H, n->save + 2 * H + 2 * kF, n->a1 + bH);
    JH_LAUNCH_NAMED("jh_rnd_bn_relu_kernel", jh_cur_bn_act_kernel<CUR_RELU | CUR_F64>, dim3((unsigned)((H + 15) / 16), 2), dim3(256), 0, st, a);
    JH_LAUNCH_CHECK();
  }
  g[0] = mk_gemm(b, kF, H, op_dense(OP_KCONT, n->a1, H), op_dense(OP_KCONT, P(n, RN_FC2P_W), H), n->z2, kF, TEPI_BIAS, P(n, RN_FC2P_B));
  g[1] = mk_gemm(b, kF, H, op_dense(OP_KCONT, n->a1 + bH, H), op_dense(OP_KCONT, P(n, RN_FC2T_W), H), n->z2 + bF, kF, TEPI_BIAS, P(n, RN_FC2T_B));
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 2, st))) return rc;
  {
    BnFwdArgs a{};
    a.z = n->z2; a.b = b; a.C = kF;
    a.h[0] = rnd_bn_half(n, RN_BN2P_W, n->o_bn2p, kF, n->save + 2 * H, n->a2);
    a.h[1] = rnd_bn_half(n, RN_BN2T_W, n->o_bn2t, kF, n->save + 4 * H + 2 * kF, n->a2 + bF);
    JH_LAUNCH_NAMED("jh_rnd_bn_relu_kernel", jh_cur_bn_act_kernel<CUR_RELU | CUR_F64>, dim3(kF / 16, 2), dim3(256), 0, st, a);
    JH_LAUNCH_CHECK();
  }
  return JH_OK;
}

BnBwdHalf rnd_bn_bwd_half(const jh_rndnet* n, const float* dy, const float* y, int C, int w_seg, float* save) {
  BnBwdHalf h{};
  h.dy0 = dy; h.ldd0 = C; h.y = y; h.ldy = C;
  if (n->bn) { h.gamma = P(n, w_seg); h.smean = save; h.sinv = save + C; h.dgamma = G(n, w_seg); h.dbeta = G(n, w_seg + 1); }
  return h;
}

// d(p) -> the predictor's run of the gradient bucket.  The two batch-norm backward kernels (the predictor's half only) and 2 GEMM launches.
int rnd_backward(jh_rndnet* n, int b, hipStream_t st) {
  const int H = n->H, S = n->S;
  TGemm g[2];
  int rc;
  {
    BnBwdArgs a{};
    a.z = n->z2; a.dz = n->dz2; a.b = b; a.C = kF;
    a.h[0] = rnd_bn_bwd_half(n, n->dp, n->a2, kF, RN_BN2P_W, n->save + 2 * H);
    JH_LAUNCH_NAMED("jh_rnd_bn_relu_bwd_kernel", jh_cur_bn_act_bwd_kernel<CUR_RELU | CUR_F64>, dim3(kF / 16, 1), dim3(256), 0, st, a);
    JH_LAUNCH_CHECK();
  }
  g[0] = mk_gemm(kF, H, b, op_dense(OP_XCONT, n->dz2, kF), op_dense(OP_XCONT, n->a1, H), G(n, RN_FC2P_W), H, TEPI_NONE, nullptr, nullptr, 0, G(n, RN_FC2P_B));
  g[1] = mk_gemm(b, H, kF, op_dense(OP_KCONT, n->dz2, kF), op_dense(OP_XCONT, P(n, RN_FC2P_W), H), n->da1, H, TEPI_NONE);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 2, st))) return rc;
  {
    BnBwdArgs a{};
    a.z = n->z1; a.dz = n->dz1; a.b = b; a.C = H;
    a.h[0] = rnd_bn_bwd_half(n, n->da1, n->a1, H, RN_BN1P_W, n->save);
    JH_LAUNCH_NAMED("jh_rnd_bn_relu_bwd_kernel", jh_cur_bn_act_bwd_kernel<CUR_RELU | CUR_F64>, dim3((unsigned)((H + 15) / 16), 1), dim3(256), 0, st, a);
    JH_LAUNCH_CHECK();
  }
  g[0] = mk_gemm(H, S, b, op_dense(OP_XCONT, n->dz1, H), op_dense(OP_XCONT, n->x, S), G(n, RN_FC1P_W), S, TEPI_NONE, nullptr, nullptr, 0, G(n, RN_FC1P_B));
  return core_tgemm(&n->core, "jh_tgemm_dense", g, 1, st);
}

int rnd_rows_ok(const jh_rndnet* n, int rows) {
  JH_ARG(rows >= 1 && rows <= n->maxB);
  JH_ARG(!n->bn || rows >= 2);  // a training-mode batch norm needs more than one value per channel
  return JH_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------- the object
JH_EXPORT int64_t jh_rndnet_param_count_for(int32_t S, int32_t H, int32_t batch_norm) {
  jh_rndnet tmp;
  return rnd_layout(&tmp, S, H, batch_norm) ? -1 : tmp.n_params;
}

JH_EXPORT int jh_rndnet_create(jh_ctx* ctx, int32_t S, int32_t H, int32_t num_workers, int32_t max_batch, int32_t flags, double gamma_i, float* d_params,
                               float* d_grads, float* d_m, float* d_v, jh_rndnet** out) {
  JH_ARG(ctx && out && d_params && d_grads && d_m && d_v);
  JH_ARG(num_workers >= 1 && max_batch >= 1 && max_batch <= kMaxBatch && flags >= 0 && flags < 8);
  jh_rndnet* n = new jh_rndnet();
  n->core.ctx = ctx;
  int rc = rnd_layout(n, S, H, (flags & JH_RND_BATCH_NORM) != 0);
  if (!rc && !((int64_t)2 * max_batch * (H > kF ? H : kF) < ((int64_t)1 << 31) && (int64_t)max_batch * S < ((int64_t)1 << 31)))
    rc = jh_fail(JH_ERR_ARG, "jh_rndnet_create: max_batch %d x hidden %d exceeds the tile engine's 32-bit indexing", max_batch, H);
  if (rc) {
    delete n;
    return rc;
  }
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) {
    delete n;
    return jh_fail(JH_ERR_HIP, "jh_rndnet_create: hipSetDevice -> %s", hipGetErrorString(e));
  }
  n->W = num_workers; n->maxB = max_batch;
  n->obs_norm = (flags & JH_RND_OBS_NORMALIZE) != 0; n->ri_norm = (flags & JH_RND_RI_NORMALIZE) != 0;
  n->gamma = (float)gamma_i;
  n->p = d_params; n->g = d_grads; n->m = d_m; n->v = d_v;
  n->cb = cur_block(S, num_workers);
  int o = n->cb.end;
  n->o_bn1p = o; o += 2 * H;
  n->o_bn2p = o; o += 2 * kF;
  n->o_bn1t = o; o += 2 * H;
  n->o_bn2t = o; o += 2 * kF;
  n->blk_floats = o;
  const size_t B = (size_t)max_batch;
  auto A4 = [&](float** p, size_t floats) { if (!rc) rc = core_alloc(&n->core, "jh_rndnet", (void**)p, floats * sizeof(float), true); };
  rc = optim_init(&n->core, "jh_rndnet", &n->opt);
  A4(&n->blk, (size_t)n->blk_floats);
  A4(&n->x, B * S); A4(&n->z1, 2 * B * H); A4(&n->a1, 2 * B * H); A4(&n->z2, 2 * B * kF); A4(&n->a2, 2 * B * kF);
  A4(&n->dp, B * kF); A4(&n->dz2, B * kF); A4(&n->da1, B * H); A4(&n->dz1, B * H); A4(&n->save, (size_t)4 * H + 4 * kF); A4(&n->ri_raw, B);
  if (!rc) rc = core_workspace(&n->core, "jh_rndnet", (size_t)8 << 20, 8192);  // 32 MB of split-K partials
  if (!rc) {
    // a fresh module: RunningMeanStd's count 1e-4 (utils.py:19-24), running_var 1 (torch.nn.BatchNorm1d)
    std::vector<float> h((size_t)n->blk_floats, 0.f);
    h[n->cb.o_obs_cnt] = 1e-4f;
    h[n->cb.o_ri + 2] = 1e-4f;
    for (int i = 0; i < H; ++i) h[n->o_bn1p + H + i] = h[n->o_bn1t + H + i] = 1.f;
    for (int i = 0; i < kF; ++i) h[n->o_bn2p + kF + i] = h[n->o_bn2t + kF + i] = 1.f;
    e = hipMemcpy(n->blk, h.data(), sizeof(float) * h.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = jh_fail(JH_ERR_HIP, "jh_rndnet_create: hipMemcpy -> %s", hipGetErrorString(e));
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

JH_EXPORT void jh_rndnet_destroy(jh_rndnet* n) {
  if (!n) return;
  core_release(&n->core);
  delete n;
}

JH_EXPORT int32_t jh_rndnet_segment_count(const jh_rndnet* n) { return n ? RN_SEG_MAX : 0; }
JH_EXPORT int jh_rndnet_segment(const jh_rndnet* n, int32_t i, int64_t* offset, int32_t* rows, int32_t* cols) {
  return seg_query(n, n ? RN_SEG_MAX : 0, i, offset, rows, cols);
}
JH_EXPORT int64_t jh_rndnet_trainable_floats(const jh_rndnet* n) { return n ? n->n_train : 0; }
JH_EXPORT int jh_rndnet_set_hyper(jh_rndnet* n, double lr, double beta1, double beta2, double eps, int64_t step, jh_stream stream) {
  JH_ARG(n != nullptr);
  return jh_hyper_upload(n->core.ctx, n->opt.hyper, lr, beta1, beta2, eps, step, 0, jh_s(stream));
}
JH_EXPORT int jh_rndnet_set_lr(jh_rndnet* n, double lr, jh_stream stream) {
  JH_ARG(n != nullptr);
  return jh_hyper_upload_lr(n->core.ctx, n->opt.hyper, lr, jh_s(stream));
}

JH_EXPORT int64_t jh_rndnet_stats_floats(const jh_rndnet* n) { return n ? n->blk_floats : 0; }
JH_EXPORT int jh_rndnet_stats_get(jh_rndnet* n, float* h_out, jh_stream stream) {
  JH_ARG(n && h_out);
  JH_HIP(hipMemcpyAsync(h_out, n->blk, sizeof(float) * (size_t)n->blk_floats, hipMemcpyDeviceToHost, jh_s(stream)));
  JH_HIP(hipStreamSynchronize(jh_s(stream)));
  return JH_OK;
}
JH_EXPORT int jh_rndnet_stats_set(jh_rndnet* n, const float* h_in, jh_stream stream) {
  JH_ARG(n && h_in);
  JH_HIP(hipMemcpyAsync(n->blk, h_in, sizeof(float) * (size_t)n->blk_floats, hipMemcpyHostToDevice, jh_s(stream)));
  JH_HIP(hipStreamSynchronize(jh_s(stream)));
  return JH_OK;
}

// rnd.update_rms_obs(next_state) (rnd_ppo.py:119)
JH_EXPORT int jh_rndnet_obs_update(jh_rndnet* n, const float* d_next_state, int32_t rows, jh_stream stream) {
  JH_ARG(n && d_next_state);
  JH_ARG(rows >= 2 && rows <= n->maxB);  // x.std of one row is NaN
  JH_LAUNCH_NAMED("jh_rnd_obs_update_kernel", jh_cur_obs_update_kernel, dim3(1), dim3(256), 0, jh_s(stream), rows, n->S, d_next_state, n->blk + n->cb.o_obs_mean,
                  n->blk + n->cb.o_obs_var, n->blk + n->cb.o_obs_cnt);
  JH_LAUNCH_CHECK();
  return JH_OK;
}

// r_i = rnd(next_state, update_ri=True) (rnd_ppo.py:120) over a whole rollout, no gradient.  7 launches.
JH_EXPORT int jh_rndnet_reward(jh_rndnet* n, const float* d_next_state, int32_t rows, float* d_ri, float* d_ri_mean, float* d_ri_raw, jh_stream stream) {
  JH_ARG(n && d_next_state && d_ri);
  int rc = rnd_rows_ok(n, rows);
  if (rc) return rc;
  JH_ARG(rows >= 2 && rows % n->W == 0);  // x.std of one row; r_i.view(num_workers, -1)
  hipStream_t st = jh_s(stream);
  if ((rc = rnd_prep(n, d_next_state, nullptr, rows, rows, st))) return rc;
  if ((rc = rnd_forward(n, rows, st))) return rc;
  float* raw = d_ri_raw ? d_ri_raw : n->ri_raw;
  JH_LAUNCH(jh_rnd_ri_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, rows, n->a2, n->a2 + (size_t)rows * kF, raw);
  JH_LAUNCH_CHECK();
  RewardArgs a{};
  a.rows = rows; a.W = n->W; a.T = rows / n->W; a.ri_norm = n->ri_norm; a.ri_raw = raw; a.ri_blk = n->blk + n->cb.o_ri; a.rewems = n->blk + n->cb.o_rew;
  a.gamma = n->gamma; a.ri_out = d_ri; a.ri_mean = d_ri_mean;
  JH_LAUNCH_NAMED("jh_rnd_reward_kernel", jh_cur_reward_kernel, dim3(1), dim3(256), 0, st, a);
  JH_LAUNCH_CHECK();
  return JH_OK;
}

// One minibatch (rnd_ppo.py:251-252, 261-266): rows d_idx[0 .. b) of the n_rows-row next_state array (NULL: rows 0 .. b - 1).
// Launches: prepare, 4 of the forward, loss, 4 of the backward, gradient norm, Adam = 12.
JH_EXPORT int jh_rndnet_update(jh_rndnet* n, const float* d_next_state, const int64_t* d_idx, int32_t b, int64_t n_rows, float max_norm, float* d_stats,
                               jh_stream stream) {
  JH_ARG(n && d_next_state);
  int rc = rnd_rows_ok(n, b);
  if (rc) return rc;
  JH_ARG(n_rows >= (d_idx ? 1 : b) && max_norm >= 0.f);
  hipStream_t st = jh_s(stream);
  if ((rc = rnd_prep(n, d_next_state, d_idx, b, n_rows, st))) return rc;
  if ((rc = rnd_forward(n, b, st))) return rc;
  RndLossArgs a{};
  a.b = b; a.p = n->a2; a.t = n->a2 + (size_t)b * kF; a.ri_var = n->ri_norm ? n->blk + n->cb.o_ri + 1 : nullptr; a.dp = n->dp; a.stats = d_stats;
  JH_LAUNCH(jh_rnd_loss_kernel, dim3(1), dim3(1024), 0, st, a);
  JH_LAUNCH_CHECK();
  if ((rc = rnd_backward(n, b, st))) return rc;
  return jh_flat_adam_step(n->n_train, n->p, n->g, n->m, n->v, n->opt.hyper, n->opt.ticket, n->core.norm_partial, max_norm, st);
}

// ---------------------------------------------------------------------------------- the advantage mix
// rnd_ppo.py:153-166 behind the two jh_gae calls (standardize off): adv[w][t] = ext adv_e + int adv_i, then per row w of T = n_step entries
// (adv - mean) / (std + 1e-7) with the UNBIASED std (torch.std); workgroup W takes mean(ret) and mean(ret_i) over all W T rows -> means[0], [1].
namespace {

__device__ __forceinline__ double mix_block_sum(double v, double* red) {
  v = jh_wave_sum(v);
  __syncthreads();  // `red` may still be read from the previous use
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ void __launch_bounds__(256) jh_rnd_adv_mix_kernel(int W, int T, float ext, float intr, int standardize, const float* __restrict__ adv_e,
                                                             const float* __restrict__ adv_i, const float* __restrict__ ret, const float* __restrict__ ret_i,
                                                             float* __restrict__ adv, float* __restrict__ means) {
  __shared__ double s_red[4];
  if ((int)blockIdx.x == W) {
    const int64_t M = (int64_t)W * T;
    double a = 0.0, b = 0.0;
    for (int64_t i = threadIdx.x; i < M; i += 256) {
      a += (double)ret[i];
      b += (double)ret_i[i];
    }
    a = mix_block_sum(a, s_red);
    b = mix_block_sum(b, s_red);
    if (threadIdx.x == 0) {
      means[0] = (float)(a / (double)M);
      means[1] = (float)(b / (double)M);
    }
    return;
  }
  const size_t o = (size_t)blockIdx.x * T;
  auto mixed = [&](int t) {
    const float e = ext * adv_e[o + t];
    const float f = intr * adv_i[o + t];
    return e + f;
  };
  if (!standardize) {
    for (int t = threadIdx.x; t < T; t += 256) adv[o + t] = mixed(t);
    return;
  }
  double s = 0.0;
  for (int t = threadIdx.x; t < T; t += 256) s += (double)mixed(t);
  const double mu = mix_block_sum(s, s_red) / (double)T;
  double q = 0.0;
  for (int t = threadIdx.x; t < T; t += 256) {
    const double d = (double)mixed(t) - mu;
    q += d * d;
  }
  const double den = sqrt(mix_block_sum(q, s_red) / (double)(T - 1)) + 1e-7;  // T == 1: NaN, as torch.std of one value
  for (int t = threadIdx.x; t < T; t += 256) adv[o + t] = (float)(((double)mixed(t) - mu) / den);
}

}  // namespace

JH_EXPORT int jh_rnd_adv_mix(jh_ctx* ctx, int32_t W, int32_t T, float extrinsic_coeff, float intrinsic_coeff, int32_t standardize, const float* d_adv_e,
                             const float* d_adv_i, const float* d_ret, const float* d_ret_i, float* d_adv, float* d_means, jh_stream stream) {
  JH_ARG(ctx && d_adv_e && d_adv_i && d_ret && d_ret_i && d_adv && d_means);
  JH_ARG(W >= 1 && T >= 1 && (int64_t)W * T <= ((int64_t)1 << 30) && W <= 65535 && (standardize == 0 || standardize == 1));
  JH_LAUNCH(jh_rnd_adv_mix_kernel, dim3((unsigned)W + 1), dim3(256), 0, jh_s(stream), (int)W, (int)T, extrinsic_coeff, intrinsic_coeff, (int)standardize, d_adv_e,
            d_adv_i, d_ret, d_ret_i, d_adv, d_means);
  JH_LAUNCH_CHECK();
  return JH_OK;
}

// ---------------------------------------------------------------------------------- PPO's loss with two critics
// rnd_ppo.py:201-249 on heads [B][ld] = (head0 [A] | head1 [A] (continuous) | v | v_i | padding); the gradient goes back in the same layout
// (padding columns are not written).  Per-row inputs are read at row idx[i] of the rollout arrays (idx NULL: row i).
//   ratio = exp(sum_k (log pi - log pi_old)), actor = -mean min(ratio adv, clamp(ratio, 1 - eps, 1 + eps) adv)
//   critic_e = max(mean (v - ret)^2, mean (v_old + clamp(v - v_old, -eps, eps) - ret)^2), critic_i the same on v_i, ret_i and the stored v_i:
//              each max is over the two MEANS, so which branch carries the gradient is known only after the sums (a tie splits it, as torch.max)
//   entropy = -mean H (over B rows | B A elements), loss = actor + vf (critic_e + critic_i) + ent entropy
//   stats   = {0, actor, critic_e, critic_i, entropy, max ratio, min prob, 0}
// The per-row policy math is jh_policy_head.h's, in double (log pi is a log-softmax of the logits where the reference takes the log of a
// renormalised softmax: a departure on purpose, as jh_mpo_loss_discrete and jh_reinforce_loss_discrete).  One workgroup: pass 1 takes the six
// sums, the maximum and the minimum (shuffle tree, then the waves in order), pass 2 evaluates each row again and writes its gradient.
namespace {

constexpr int kLossThreads = 1024, kLossWaves = kLossThreads / 64;
constexpr int kMaxActionsDiscrete = 64, kMaxActionsContinuous = 32;

struct RndPpoArgs {
  int B, A, ld;
  const float* heads;
  const int64_t* idx;
  const float *action, *adv, *ret, *ret_i, *v_old, *vi_old, *logp_old;
  float eps, vf, ent;
  float *grad, *stats;
};

struct RndRow {
  double ratio, ent, minp;  // ent: the row's entropy (summed over the dimensions of a Gaussian)
  double adv, smin, g_ratio;  // g_ratio: d(min(surr1, surr2)) / d(ratio)
  double v, ret, vclip, vi, ret_i, viclip;
  bool in_v, in_vi;
};

__device__ __forceinline__ void clip_value(double v, double vold, double eps, double& vclip, bool& inside) {
  const double dv = v - vold;
  inside = dv >= -eps && dv <= eps;  // torch.clamp passes the gradient on its bounds
  vclip = vold + fmin(fmax(dv, -eps), eps);
}

template <bool CONT>
__device__ __forceinline__ RndRow rnd_row(const RndPpoArgs& a, int i, int64_t r) {
  const int A = a.A;
  const float* h = a.heads + (size_t)i * a.ld;
  RndRow o;
  double lsum = 0.0;
  if (CONT) {
    o.ent = 0.0;
    o.minp = 1.7e308;
    for (int k = 0; k < A; ++k) {
      const GaussElem e = gauss_elem(h[k], h[A + k]);
      const double lp = gauss_log_prob(gauss_z(a.action[r * A + k]) - e.mu, e.th, e.var);
      lsum += lp - (double)a.logp_old[r * A + k];
      o.ent += 0.5 + kHalfLog2Pi + e.th;  // Normal.entropy = 1/2 + log sqrt(2 pi) + log(std)
      o.minp = fmin(o.minp, exp(lp));
    }
  } else {
    const double lse = row_lse(h, A);
    const int ak = action_index(a.action[r], A);
    double ent = 0.0;
    for (int k = 0; k < A; ++k) {
      const double lg = (double)h[k] - lse;
      ent += exp(lg) * lg;
    }
    const double lp = (double)h[ak] - lse;
    lsum = lp - (double)a.logp_old[r];
    o.ent = -ent;
    o.minp = exp(lp);
  }
  const double eps = (double)a.eps;
  o.ratio = exp(lsum);
  o.adv = (double)a.adv[r];
  const double surr1 = o.ratio * o.adv;
  const bool in_clip = o.ratio >= 1.0 - eps && o.ratio <= 1.0 + eps;
  const double surr2 = fmin(fmax(o.ratio, 1.0 - eps), 1.0 + eps) * o.adv;
  o.smin = fmin(surr1, surr2);
  const double w1 = surr1 < surr2 ? 1.0 : (surr1 == surr2 ? 0.5 : 0.0), w2 = 1.0 - w1;  // torch.min splits a tie
  o.g_ratio = w1 * o.adv + (in_clip ? w2 * o.adv : 0.0);
  const int nv = CONT ? 2 * A : A;
  o.v = (double)h[nv]; o.ret = (double)a.ret[r];
  o.vi = (double)h[nv + 1]; o.ret_i = (double)a.ret_i[r];
  clip_value(o.v, (double)a.v_old[r], eps, o.vclip, o.in_v);
  clip_value(o.vi, (double)a.vi_old[r], eps, o.viclip, o.in_vi);
  return o;
}

__device__ __forceinline__ double sq(double x) { return x * x; }

template <bool CONT>
__global__ void __launch_bounds__(kLossThreads) jh_rnd_ppo_loss_kernel(RndPpoArgs a) {
  __shared__ double s_red[kLossWaves];
  const int B = a.B, A = a.A;
  double smin = 0.0, e1 = 0.0, e2 = 0.0, i1 = 0.0, i2 = 0.0, ent = 0.0, maxr = -1.7e308, minp = 1.7e308;
  for (int i = threadIdx.x; i < B; i += kLossThreads) {
    const RndRow o = rnd_row<CONT>(a, i, a.idx ? a.idx[i] : (int64_t)i);
    smin += o.smin;
    e1 += sq(o.v - o.ret); e2 += sq(o.vclip - o.ret);
    i1 += sq(o.vi - o.ret_i); i2 += sq(o.viclip - o.ret_i);
    ent += o.ent;
    maxr = fmax(maxr, o.ratio);
    minp = fmin(minp, o.minp);
  }
  smin = jh_block_reduce(smin, s_red, JhAdd(), 0.0);
  e1 = jh_block_reduce(e1, s_red, JhAdd(), 0.0);
  e2 = jh_block_reduce(e2, s_red, JhAdd(), 0.0);
  i1 = jh_block_reduce(i1, s_red, JhAdd(), 0.0);
  i2 = jh_block_reduce(i2, s_red, JhAdd(), 0.0);
  ent = jh_block_reduce(ent, s_red, JhAdd(), 0.0);
  maxr = jh_block_reduce(maxr, s_red, JhMax(), -1.7e308);
  minp = jh_block_reduce(minp, s_red, JhMin(), 1.7e308);
  const double invB = 1.0 / (double)B;
  const double we1 = e1 > e2 ? 1.0 : (e1 == e2 ? 0.5 : 0.0), wi1 = i1 > i2 ? 1.0 : (i1 == i2 ? 0.5 : 0.0);
  if (threadIdx.x == 0 && a.stats) {
    a.stats[0] = 0.f;
    a.stats[1] = (float)(-smin * invB);
    a.stats[2] = (float)(fmax(e1, e2) * invB);
    a.stats[3] = (float)(fmax(i1, i2) * invB);
    a.stats[4] = (float)(-ent / (CONT ? (double)B * (double)A : (double)B));
    a.stats[5] = (float)maxr;
    a.stats[6] = (float)minp;
    a.stats[7] = 0.f;
  }
  const int nv = CONT ? 2 * A : A;
  const double vf2 = 2.0 * (double)a.vf * invB;
  for (int i = threadIdx.x; i < B; i += kLossThreads) {
    const int64_t r = a.idx ? a.idx[i] : (int64_t)i;
    const RndRow o = rnd_row<CONT>(a, i, r);
    const float* h = a.heads + (size_t)i * a.ld;
    float* g = a.grad + (size_t)i * a.ld;
    g[nv] = (float)(vf2 * (we1 * (o.v - o.ret) + (o.in_v ? (1.0 - we1) * (o.vclip - o.ret) : 0.0)));
    g[nv + 1] = (float)(vf2 * (wi1 * (o.vi - o.ret_i) + (o.in_vi ? (1.0 - wi1) * (o.viclip - o.ret_i) : 0.0)));
    const double d_logp = -invB * o.g_ratio * o.ratio;  // d(actor) / d(log pi), the same for every dimension of a Gaussian
    if (CONT) {
      const double ce = -(double)a.ent / ((double)B * (double)A);  // d(ent * -mean H) / d(log std)
      for (int k = 0; k < A; ++k) {
        const GaussElem e = gauss_elem(h[k], h[A + k]);
        const double d = gauss_z(a.action[r * A + k]) - e.mu;
        g[k] = gauss_grad_mu_raw(e, d_logp * d / e.var);
        g[A + k] = gauss_grad_log_std_raw(e, d_logp * (d * d / e.var - 1.0) + ce);
      }
    } else {
      const double lse = row_lse(h, A);
      const int ak = action_index(a.action[r], A);
      const double ce = (double)a.ent * invB;  // d(ent * -mean H) / dz_k = ce p_k (log p_k + H)
      for (int k = 0; k < A; ++k) {
        const double lg = (double)h[k] - lse, p = exp(lg);
        g[k] = (float)(d_logp * ((k == ak ? 1.0 : 0.0) - p) + ce * p * (lg + o.ent));
      }
    }
  }
}

}  // namespace

JH_EXPORT int jh_rnd_ppo_loss_packed(jh_ctx* ctx, int32_t continuous, int32_t B, int32_t A, const float* d_heads, int32_t ld, const int64_t* d_idx,
                                     const float* d_action, const float* d_adv, const float* d_ret, const float* d_ret_i, const float* d_value_old,
                                     const float* d_vi_old, const float* d_logp_old, float eps_clip, float vf_coef, float ent_coef, float* d_grad_heads,
                                     float* d_stats, jh_stream stream) {
  JH_ARG(ctx && d_heads && d_action && d_adv && d_ret && d_ret_i && d_value_old && d_vi_old && d_logp_old && d_grad_heads);
  JH_ARG(continuous == 0 || continuous == 1);
  JH_ARG(B >= 1 && B <= (1 << 20) && (continuous ? (A >= 1 && A <= kMaxActionsContinuous) : (A >= 2 && A <= kMaxActionsDiscrete)));
  JH_ARG(ld >= (continuous ? 2 * A + 2 : A + 2) && eps_clip >= 0.f);
  RndPpoArgs a{};
  a.B = B; a.A = A; a.ld = ld; a.heads = d_heads; a.idx = d_idx; a.action = d_action; a.adv = d_adv; a.ret = d_ret; a.ret_i = d_ret_i;
  a.v_old = d_value_old; a.vi_old = d_vi_old; a.logp_old = d_logp_old; a.eps = eps_clip; a.vf = vf_coef; a.ent = ent_coef; a.grad = d_grad_heads; a.stats = d_stats;
  if (continuous)
    JH_LAUNCH_NAMED("jh_rnd_ppo_loss_kernel", jh_rnd_ppo_loss_kernel<true>, dim3(1), dim3(kLossThreads), 0, jh_s(stream), a);
  else
    JH_LAUNCH_NAMED("jh_rnd_ppo_loss_kernel", jh_rnd_ppo_loss_kernel<false>, dim3(1), dim3(kLossThreads), 0, jh_s(stream), a);
  JH_LAUNCH_CHECK();
  return JH_OK;
}
