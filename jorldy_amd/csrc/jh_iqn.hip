// Implicit quantile network (core/network/iqn.py:9-47, core/agent/iqn.py:12-146) on the device:
//   jh_iqnnet_*      the network with an MLP head: x -> relu(head.l) -> psi = relu(state_embed), tau -> cos(tau * i * pi) ->
//                    phi = relu(sample_embed), embed = psi (.) phi, relu(l1), relu(l2), q  -> [rows][N][A]; the three forwards of
//                    learn() in shared launches, the backward of online(s), Adam (jh_rbnet's optimizer kernels on the flat buckets)
//   jh_riqnnet_*     the same object with Rainbow's tail where q stands (core/network/rainbow_iqn.py:9-113): the trunk up to relu(l2) at
//                    the caller's width, then relu(noisy a1) | relu(noisy v1) -> noisy a2, noisy v2 -> x_a - mean_a x_a + x_v over the
//                    rows x N sampled rows.  One trunk (iq_trunk / iq_trunk_backward) serves both tails; the noisy tail's elementwise
//                    kernels are Rainbow's (jh_noisy.h)
// Every dense contraction runs on the tile engine (jh_tgemm.hip) under the call-site name "dense".  The kernels of this file are the
// elementwise steps between them: cosine features, the Hadamard product and its backward.  The loss and acting entries jh_iqn_loss /
// jh_iqn_act are the sample-major instantiations of the quantile family's kernels in jh_qr.hip.
// No floating-point atomics: every sum has a fixed order, so two runs (and a graph replay) give the same bits.
#include "jh_noisy.h"

namespace {

// ---------------------------------------------------------------------------------- cosine features
// out[r][i] = cos(tau[r] * i_pi[i]), i_pi = arange(0, E) * np.pi as a FLOAT32 tensor (iqn.py:14): float(i) * float(pi), rounded, and
// the product with tau rounded to float32 again before the cosine (iqn.py:46; at i = 63 the argument is ~198, one ulp is 1.5e-5).
// cosf is the accurate one (full range reduction), not __cosf.
__global__ void __launch_bounds__(256) jh_iqn_cos_kernel(int64_t rows, int E, const float* __restrict__ tau, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * E) return;
  const int64_t r = i / E;
  const int e = (int)(i - r * E);
  const float i_pi = (float)e * 3.14159274101257324f;
  const float arg = tau[r] * i_pi;
  out[i] = cosf(arg);
}

// ---------------------------------------------------------------------------------- Hadamard product
// embed[(b, n)][h] = psi[b][h] * phi[(b, n)][h]   (iqn.py:34), four h per thread; H % 4 == 0
__global__ void __launch_bounds__(256) jh_iqn_hadamard_kernel(int64_t rows, int N, int H4, const float4* __restrict__ psi, const float4* __restrict__ phi,
                                                              float4* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * H4) return;
  const int64_t r = i / H4;
  const int h = (int)(i - r * H4);
  const float4 p = psi[(r / N) * H4 + h], f = phi[i];
  out[i] = make_float4(p.x * f.x, p.y * f.y, p.z * f.z, p.w * f.w);
}

// d(phi_pre)[(b, n)][h] = d(embed) * psi * (phi > 0);  d(psi_pre)[b][h] = (sum_n d(embed)[(b, n)][h] * phi[(b, n)][h]) * (psi > 0).
// One workgroup per (sample b, slab of 64 float4 of H): wave w walks n = w, w + 4, ... in ascending order, the four partial sums meet
// in LDS and are added in wave order -- a fixed order, no atomics.
__global__ void __launch_bounds__(256) jh_iqn_hadamard_bwd_kernel(int N, int H4, const float4* __restrict__ dem, const float4* __restrict__ psi,
                                                                  const float4* __restrict__ phi, float4* __restrict__ dphi, float4* __restrict__ dpsi) {
  __shared__ float4 s_part[3][64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int b = blockIdx.x, h = blockIdx.y * 64 + lane;
  const bool live = h < H4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) {
    const float4 p = psi[(size_t)b * H4 + h];
    for (int n = wid; n < N; n += 4) {
      const size_t o = ((size_t)b * N + n) * H4 + h;
      const float4 d = dem[o], f = phi[o];
      dphi[o] = make_float4(f.x > 0.f ? d.x * p.x : 0.f, f.y > 0.f ? d.y * p.y : 0.f, f.z > 0.f ? d.z * p.z : 0.f, f.w > 0.f ? d.w * p.w : 0.f);
      acc.x += d.x * f.x; acc.y += d.y * f.y; acc.z += d.z * f.z; acc.w += d.w * f.w;
    }
    if (wid > 0) s_part[wid - 1][lane] = acc;
  }
  __syncthreads();
  if (live && wid == 0) {
    const float4 p = psi[(size_t)b * H4 + h];
#pragma unroll
    for (int w = 0; w < 3; ++w) {
      const float4 q = s_part[w][lane];
      acc.x += q.x; acc.y += q.y; acc.z += q.z; acc.w += q.w;
    }
    dpsi[(size_t)b * H4 + h] = make_float4(p.x > 0.f ? acc.x : 0.f, p.y > 0.f ? acc.y : 0.f, p.z > 0.f ? acc.z : 0.f, p.w > 0.f ? acc.w : 0.f);
  }
}

static int iqn_cos(int64_t rows, int E, const float* tau, float* out, hipStream_t st) {
  const int64_t n = rows * E;
  JH_LAUNCH(jh_iqn_cos_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, rows, E, tau, out);
  JH_LAUNCH_CHECK();
  return JH_OK;
}
static int iqn_hadamard(int64_t rows, int N, int H, const float* psi, const float* phi, float* out, hipStream_t st) {
  const int64_t n = rows * (H / 4);
  JH_LAUNCH(jh_iqn_hadamard_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, rows, N, H / 4, (const float4*)psi, (const float4*)phi, (float4*)out);
  JH_LAUNCH_CHECK();
  return JH_OK;
}
static int iqn_hadamard_bwd(int B, int N, int H, const float* dem, const float* psi, const float* phi, float* dphi, float* dpsi, hipStream_t st) {
  const int H4 = H / 4;
  JH_LAUNCH(jh_iqn_hadamard_bwd_kernel, dim3(B, (H4 + 63) / 64), dim3(256), 0, st, N, H4, (const float4*)dem, (const float4*)psi, (const float4*)phi, (float4*)dphi,
            (float4*)dpsi);
  JH_LAUNCH_CHECK();
  return JH_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------- the network
enum {
  IQ_W1, IQ_B1, IQ_WSE, IQ_BSE, IQ_WSA, IQ_BSA, IQ_WL1, IQ_BL1, IQ_WL2, IQ_BL2, IQ_WQ, IQ_BQ, IQ_SEG_COUNT,
  // the noisy dueling tail (empty under the q tail, as q is under this one): a1 | v1 stacked [2H][H] as jh_rbnet keeps them
  IQ_MU_AV1 = IQ_SEG_COUNT, IQ_SIG_AV1, IQ_MUB_AV1, IQ_SIGB_AV1, IQ_MU_A2, IQ_SIG_A2, IQ_MUB_A2, IQ_SIGB_A2, IQ_MU_V2, IQ_SIG_V2, IQ_MUB_V2, IQ_SIGB_V2, IQ_SEG_ALL
};
enum { IQ_TAIL_Q, IQ_TAIL_NOISY };

struct jh_iqnnet {
  NetCore core;
  FlatOptim opt;
  int S = 0, H = 0, E = 0, N = 0, A = 0, maxB = 0;
  int tail = IQ_TAIL_Q;
  int64_t seg_off[IQ_SEG_ALL] = {0};
  int seg_rows[IQ_SEG_ALL] = {0}, seg_cols[IQ_SEG_ALL] = {0};
  int64_t n_params = 0;
  float *params = nullptr, *target = nullptr, *grads = nullptr, *m = nullptr, *v = nullptr;
  // activations of up to three forwards, rows [online: 2 maxB | target: maxB] (x N for the per-sample ones)
  float *feat = nullptr, *psi = nullptr, *cosf_ = nullptr, *phi = nullptr, *emb = nullptr, *h1 = nullptr, *h2 = nullptr;
  float *dA = nullptr, *dB = nullptr, *dpsi = nullptr, *dfeat = nullptr;  // backward: [maxB * N][H] x 2, [maxB][H] x 2
  // noisy tail: effective weights [3][set_stride]; relu(a1 | v1) [3 maxB N][2H], the streams' outputs [3 maxB N][A4], [.][4]; backward
  // [maxB N][...] of each
  NoisyDims nd{};
  int64_t n_noisy = 0;
  int A4 = 0;
  float *weff = nullptr, *hav = nullptr, *xa = nullptr, *xv = nullptr, *dxa = nullptr, *dxv = nullptr, *dhav = nullptr;
  const float* last_noise = nullptr;  // draw 0 of the last jh_riqnnet_learn_forward: d(sig) = d(mu) * eps
  const float* last_x = nullptr;  // state rows of the last learn_forward (the head's weight gradient reads them again)
  int last_B = 0;
};

static int iq_layout(jh_iqnnet* n, int32_t S, int32_t H, int32_t E, int32_t N, int32_t A, int32_t max_batch, int tail = IQ_TAIL_Q, int independent = 0) {
  JH_ARG(S > 0 && H > 0 && H % 4 == 0 && E > 0 && A > 0 && max_batch > 0);
  JH_ARG(N >= 1 && N <= 256);
  JH_ARG((int64_t)3 * max_batch * N * (int64_t)(H > E ? H : E) < ((int64_t)1 << 31));  // the tile engine indexes rows x columns in 32 bits
  n->S = S; n->H = H; n->E = E; n->N = N; n->A = A; n->maxB = max_batch; n->tail = tail;
  if (tail == IQ_TAIL_NOISY) {
    JH_ARG(S % 4 == 0);
    JH_ARG((int64_t)3 * max_batch * N * (int64_t)(2 * H) < ((int64_t)1 << 31));  // the widest activation: relu(a1 | v1)
  }
  auto seg = [&](int id, int rows, int cols) { n->seg_rows[id] = rows; n->seg_cols[id] = cols; };
  seg(IQ_W1, H, S); seg(IQ_B1, 1, H);
  seg(IQ_WSE, H, H); seg(IQ_BSE, 1, H);
  seg(IQ_WSA, H, E); seg(IQ_BSA, 1, H);
  seg(IQ_WL1, H, H); seg(IQ_BL1, 1, H);
  seg(IQ_WL2, H, H); seg(IQ_BL2, 1, H);
  if (tail == IQ_TAIL_Q) {
    seg(IQ_WQ, A, H); seg(IQ_BQ, 1, A);
    n->n_params = seg_pack(n->seg_rows, n->seg_cols, 0, IQ_SEG_COUNT, n->seg_off);
    return JH_OK;
  }
  seg(IQ_MU_AV1, 2 * H, H); seg(IQ_SIG_AV1, 2 * H, H); seg(IQ_MUB_AV1, 1, 2 * H); seg(IQ_SIGB_AV1, 1, 2 * H);
  seg(IQ_MU_A2, A, H); seg(IQ_SIG_A2, A, H); seg(IQ_MUB_A2, 1, A); seg(IQ_SIGB_A2, 1, A);
  seg(IQ_MU_V2, 1, H); seg(IQ_SIG_V2, 1, H); seg(IQ_MUB_V2, 1, 1); seg(IQ_SIGB_V2, 1, 1);
  n->n_params = seg_pack(n->seg_rows, n->seg_cols, 0, IQ_SEG_ALL, n->seg_off);
  // jh_rbnet's NoisyDims with one support (network/rainbow_iqn.py:26-38: D_out = A, the value stream has one output)
  NoisyDims& d = n->nd;
  d.H = H; d.NA = A; d.K = 1;
  d.o_av1 = 0;
  d.o_bav1 = up4(d.o_av1 + (int64_t)2 * H * H);
  d.o_a2 = up4(d.o_bav1 + 2 * H);
  d.o_ba2 = up4(d.o_a2 + (int64_t)A * H);
  d.o_v2 = up4(d.o_ba2 + A);
  d.o_bv2 = up4(d.o_v2 + (int64_t)H);
  d.set_stride = up4(d.o_bv2 + 1);
  d.p_mu_av1 = n->seg_off[IQ_MU_AV1]; d.p_sig_av1 = n->seg_off[IQ_SIG_AV1]; d.p_mub_av1 = n->seg_off[IQ_MUB_AV1]; d.p_sigb_av1 = n->seg_off[IQ_SIGB_AV1];
  d.p_mu_a2 = n->seg_off[IQ_MU_A2]; d.p_sig_a2 = n->seg_off[IQ_SIG_A2]; d.p_mub_a2 = n->seg_off[IQ_MUB_A2]; d.p_sigb_a2 = n->seg_off[IQ_SIGB_A2];
  d.p_mu_v2 = n->seg_off[IQ_MU_V2]; d.p_sig_v2 = n->seg_off[IQ_SIG_V2]; d.p_mub_v2 = n->seg_off[IQ_MUB_V2]; d.p_sigb_v2 = n->seg_off[IQ_SIGB_V2];
  d.independent = independent;
  d.noise_len = independent ? (int64_t)2 * ((int64_t)H * H + H) + (int64_t)H * A + A + (int64_t)H + 1 : (int64_t)6 * H + A + 1;
  n->n_noisy = (int64_t)2 * H * H + (int64_t)A * H + (int64_t)H + 2 * H + A + 1;
  n->A4 = (int)up4(A);
  return JH_OK;
}

JH_EXPORT int64_t jh_iqnnet_param_count_for(int32_t S, int32_t H, int32_t E, int32_t N, int32_t A) {
  jh_iqnnet tmp;
  if (iq_layout(&tmp, S, H, E, N, A, 1)) return -1;
  return tmp.n_params;
}

static int iq_create(jh_ctx* ctx, int tail, int independent, int32_t S, int32_t H, int32_t E, int32_t N, int32_t A, int32_t max_batch, float* d_params, float* d_target,
                     float* d_grads, float* d_m, float* d_v, jh_iqnnet** out) {
  JH_ARG(ctx && out && d_params && d_target && d_grads && d_m && d_v);
  JH_HIP(hipSetDevice(ctx->device));
  jh_iqnnet* n = new jh_iqnnet();
  n->core.ctx = ctx;
  int rc = iq_layout(n, S, H, E, N, A, max_batch, tail, independent);
  if (rc) {
    delete n;
    return rc;
  }
  n->params = d_params; n->target = d_target; n->grads = d_grads; n->m = d_m; n->v = d_v;
  const size_t R3 = 3 * (size_t)max_batch, RN = R3 * N, BN = (size_t)max_batch * N;
  auto A4 = [&](float** p, size_t floats) { if (!rc) rc = core_alloc(&n->core, "jh_iqnnet", (void**)p, floats * sizeof(float), true); };
  rc = optim_init(&n->core, "jh_iqnnet", &n->opt);
  A4(&n->feat, R3 * H); A4(&n->psi, R3 * H);
  A4(&n->cosf_, RN * E); A4(&n->phi, RN * H); A4(&n->emb, RN * H); A4(&n->h1, RN * H); A4(&n->h2, RN * H);
  A4(&n->dA, BN * H); A4(&n->dB, BN * H); A4(&n->dpsi, (size_t)max_batch * H); A4(&n->dfeat, (size_t)max_batch * H);
  if (tail == IQ_TAIL_NOISY) {
    A4(&n->weff, 3 * (size_t)n->nd.set_stride);
    A4(&n->hav, RN * 2 * H); A4(&n->xa, RN * n->A4); A4(&n->xv, RN * 4);
    A4(&n->dxa, BN * n->A4); A4(&n->dxv, BN * 4); A4(&n->dhav, BN * 2 * H);
  }
  if (!rc) rc = core_workspace(&n->core, "jh_iqnnet", (size_t)8 << 20, 8192);  // 32 MB of split-K partials
  if (!rc) rc = core_drain();
  if (rc) {
    core_release(&n->core);
    delete n;
    return rc;
  }
  *out = n;
  return JH_OK;
}

JH_EXPORT int jh_iqnnet_create(jh_ctx* ctx, int32_t S, int32_t H, int32_t E, int32_t N, int32_t A, int32_t max_batch, float* d_params, float* d_target,
                               float* d_grads, float* d_m, float* d_v, jh_iqnnet** out) {
  return iq_create(ctx, IQ_TAIL_Q, 0, S, H, E, N, A, max_batch, d_params, d_target, d_grads, d_m, d_v, out);
}

JH_EXPORT void jh_iqnnet_destroy(jh_iqnnet* n) {
  if (!n) return;
  core_release(&n->core);
  delete n;
}

JH_EXPORT int32_t jh_iqnnet_segment_count(void) { return IQ_SEG_COUNT; }
JH_EXPORT int jh_iqnnet_segment(const jh_iqnnet* n, int32_t i, int64_t* offset, int32_t* rows, int32_t* cols) {
  return seg_query(n, n && n->tail == IQ_TAIL_NOISY ? IQ_SEG_ALL : IQ_SEG_COUNT, i, offset, rows, cols);
}

JH_EXPORT int jh_iqnnet_set_hyper(jh_iqnnet* n, double lr, double beta1, double beta2, double eps, int64_t step, jh_stream stream) {
  JH_ARG(n != nullptr);
  return jh_hyper_upload(n->core.ctx, n->opt.hyper, lr, beta1, beta2, eps, step, 0, jh_s(stream));
}
JH_EXPORT int jh_iqnnet_set_lr(jh_iqnnet* n, double lr, jh_stream stream) {
  JH_ARG(n != nullptr);
  return jh_hyper_upload_lr(n->core.ctx, n->opt.hyper, lr, jh_s(stream));
}
JH_EXPORT int jh_iqnnet_sync_target(jh_iqnnet* n, jh_stream stream) {
  JH_ARG(n != nullptr);
  JH_HIP(hipMemcpyAsync(n->target, n->params, sizeof(float) * (size_t)n->n_params, hipMemcpyDeviceToDevice, jh_s(stream)));
  return JH_OK;
}

// Up to three (parameter set, input rows) jobs that sit one after the other in the activation buffers: job j's rows start at row0.
// d_tau and d_logits cover the rows of all jobs contiguously, from row 0.  Each layer is ONE grouped launch for all jobs.
struct IqJob {
  const float* P;
  const float* x;  // [rows][S]
  int row0, rows;
};
// The trunk both tails stand on: head.l -> state_embed, cos -> sample_embed, Hadamard, l1, l2 -> n->h2 (iqn.py:28-36, rainbow_iqn.py:43-52)
static int iq_trunk(jh_iqnnet* n, const IqJob* jobs, int nj, const float* d_tau, hipStream_t st) {
  const int S = n->S, H = n->H, E = n->E, N = n->N;
  int total = 0;
  for (int j = 0; j < nj; ++j) total += jobs[j].rows;
  TGemm g[3];
  int rc;
  // head.l and state_embed on the state rows
  for (int j = 0; j < nj; ++j) {
    const IqJob& J = jobs[j];
    g[j] = mk_gemm(J.rows, H, S, op_dense(OP_KCONT, J.x, S), op_dense(OP_KCONT, J.P + n->seg_off[IQ_W1], S), n->feat + (size_t)J.row0 * H, H,
                   TEPI_BIAS_RELU, J.P + n->seg_off[IQ_B1]);
  }
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, nj, st))) return rc;
  for (int j = 0; j < nj; ++j) {
    const IqJob& J = jobs[j];
    g[j] = mk_gemm(J.rows, H, H, op_dense(OP_KCONT, n->feat + (size_t)J.row0 * H, H), op_dense(OP_KCONT, J.P + n->seg_off[IQ_WSE], H), n->psi + (size_t)J.row0 * H, H,
                   TEPI_BIAS_RELU, J.P + n->seg_off[IQ_BSE]);
  }
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, nj, st))) return rc;
  // cosine features of every (row, sample), then sample_embed
  if ((rc = iqn_cos((int64_t)total * N, E, d_tau, n->cosf_, st))) return rc;
  for (int j = 0; j < nj; ++j) {
    const IqJob& J = jobs[j];
    const size_t r0 = (size_t)J.row0 * N;
    g[j] = mk_gemm(J.rows * N, H, E, op_dense(OP_KCONT, n->cosf_ + r0 * E, E), op_dense(OP_KCONT, J.P + n->seg_off[IQ_WSA], E), n->phi + r0 * H, H, TEPI_BIAS_RELU,
                   J.P + n->seg_off[IQ_BSA]);
  }
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, nj, st))) return rc;
  if ((rc = iqn_hadamard((int64_t)total * N, N, H, n->psi, n->phi, n->emb, st))) return rc;
  const float* in[2] = {n->emb, n->h1};
  float* outp[2] = {n->h1, n->h2};
  const int wseg[2] = {IQ_WL1, IQ_WL2}, bseg[2] = {IQ_BL1, IQ_BL2};
  for (int l = 0; l < 2; ++l) {
    for (int j = 0; j < nj; ++j) {
      const IqJob& J = jobs[j];
      const size_t r0 = (size_t)J.row0 * N;
      g[j] = mk_gemm(J.rows * N, H, H, op_dense(OP_KCONT, in[l] + r0 * H, H), op_dense(OP_KCONT, J.P + n->seg_off[wseg[l]], H), outp[l] + r0 * H, H, TEPI_BIAS_RELU,
                     J.P + n->seg_off[bseg[l]]);
    }
    if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, nj, st))) return rc;
  }
  return JH_OK;
}
static int iq_forward(jh_iqnnet* n, const IqJob* jobs, int nj, const float* d_tau, float* d_logits, hipStream_t st) {
  const int H = n->H, N = n->N, A = n->A;
  TGemm g[3];
  int rc = iq_trunk(n, jobs, nj, d_tau, st);
  if (rc) return rc;
  for (int j = 0; j < nj; ++j) {
    const IqJob& J = jobs[j];
    const size_t r0 = (size_t)J.row0 * N;
    g[j] = mk_gemm(J.rows * N, A, H, op_dense(OP_KCONT, n->h2 + r0 * H, H), op_dense(OP_KCONT, J.P + n->seg_off[IQ_WQ], H), d_logits + r0 * A, A, TEPI_BIAS,
                   J.P + n->seg_off[IQ_BQ]);
  }
  return core_tgemm(&n->core, "jh_tgemm_dense", g, nj, st);
}

JH_EXPORT int jh_iqnnet_forward(jh_iqnnet* n, int32_t which, const float* d_x, int32_t rows, const float* d_tau, float* d_logits, jh_stream stream) {
  JH_ARG(n && d_x && d_tau && d_logits);
  JH_ARG(rows > 0 && rows <= n->maxB && (which == 0 || which == 1) && n->tail == IQ_TAIL_Q);
  IqJob j{which == 0 ? n->params : n->target, d_x, 0, rows};
  n->last_x = nullptr;  // the activations of a learn_forward are gone
  return iq_forward(n, &j, 1, d_tau, d_logits, jh_s(stream));
}

JH_EXPORT int jh_iqnnet_learn_forward(jh_iqnnet* n, const float* d_x, int32_t B, const float* d_tau, float* d_logits, jh_stream stream) {
  JH_ARG(n && d_x && d_tau && d_logits);
  JH_ARG(B > 0 && B <= n->maxB && n->tail == IQ_TAIL_Q);
  // rows [0, 2B) of the activation buffers: online on [state; next_state] with the draws 0 and 1; rows [2B, 3B): target on next_state
  // with draw 2
  IqJob jobs[2] = {{n->params, d_x, 0, 2 * B}, {n->target, d_x + (size_t)B * n->S, 2 * B, B}};
  int rc = iq_forward(n, jobs, 2, d_tau, d_logits, jh_s(stream));
  if (rc) return rc;
  n->last_x = d_x;
  n->last_B = B;
  return JH_OK;
}

// The three forwards M-IQN's learn() keeps (m_iqn.py:30, 43, 50; the reference's online(next_state) of line 40 feeds nothing and is
// not run): rows [0, B): online on state with draw 0 -- where jh_iqnnet_backward expects the activations it differentiates --,
// rows [B, 2B): online on state again with draw 1, rows [2B, 3B): target on next_state with draw 2.  The second job runs the state
// trunk (head.l, state_embed) again rather than sharing job 0's: 1 / N of the sampled work, and every job stays a plain row range.
JH_EXPORT int jh_iqnnet_learn_forward_m(jh_iqnnet* n, const float* d_x, int32_t B, const float* d_tau, float* d_logits, jh_stream stream) {
  JH_ARG(n && d_x && d_tau && d_logits);
  JH_ARG(B > 0 && B <= n->maxB && n->tail == IQ_TAIL_Q);
  IqJob jobs[3] = {{n->params, d_x, 0, B}, {n->params, d_x, B, B}, {n->target, d_x + (size_t)B * n->S, 2 * B, B}};
  int rc = iq_forward(n, jobs, 3, d_tau, d_logits, jh_s(stream));
  if (rc) return rc;
  n->last_x = d_x;
  n->last_B = B;
  return JH_OK;
}

// Backward of logits[0] = online(state) of the last jh_iqnnet_learn_forward / _m: d_g = d(loss)/d(logits) [B][N][A]; fills the gradient
// bucket (same layout as the parameters).  The online activations of the state rows are the first B (x N) rows of every buffer.
static int riq_tail_backward(jh_iqnnet* n, const float* d_g, hipStream_t st);
// From dh2 = d(loss)/d(l2's pre-activation) in n->dA down to the head: the trunk's gradients under either tail
static int iq_trunk_backward(jh_iqnnet* n, hipStream_t st) {
  const int B = n->last_B, S = n->S, H = n->H, E = n->E, N = n->N, BN = B * N;
  const float* P = n->params;
  float* G = n->grads;
  float *dh2 = n->dA, *dh1 = n->dB, *dem = n->dA, *dphi = n->dB;
  TGemm g[3];
  int rc;
  g[0] = mk_gemm(H, H, BN, op_dense(OP_XCONT, dh2, H), op_dense(OP_XCONT, n->h1, H), G + n->seg_off[IQ_WL2], H, TEPI_NONE, nullptr, nullptr, 0, G + n->seg_off[IQ_BL2]);
  g[1] = mk_gemm(BN, H, H, op_dense(OP_KCONT, dh2, H), op_dense(OP_XCONT, P + n->seg_off[IQ_WL2], H), dh1, H, TEPI_MASK, nullptr, n->h1, H);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 2, st))) return rc;
  // l1 reads the product itself: no relu between them
  g[0] = mk_gemm(H, H, BN, op_dense(OP_XCONT, dh1, H), op_dense(OP_XCONT, n->emb, H), G + n->seg_off[IQ_WL1], H, TEPI_NONE, nullptr, nullptr, 0, G + n->seg_off[IQ_BL1]);
  g[1] = mk_gemm(BN, H, H, op_dense(OP_KCONT, dh1, H), op_dense(OP_XCONT, P + n->seg_off[IQ_WL1], H), dem, H, TEPI_NONE);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 2, st))) return rc;
  if ((rc = iqn_hadamard_bwd(B, N, H, dem, n->psi, n->phi, dphi, n->dpsi, st))) return rc;
  // sample_embed (its input, the cosine features, has no gradient) and state_embed
  g[0] = mk_gemm(H, E, BN, op_dense(OP_XCONT, dphi, H), op_dense(OP_XCONT, n->cosf_, E), G + n->seg_off[IQ_WSA], E, TEPI_NONE, nullptr, nullptr, 0, G + n->seg_off[IQ_BSA]);
  g[1] = mk_gemm(H, H, B, op_dense(OP_XCONT, n->dpsi, H), op_dense(OP_XCONT, n->feat, H), G + n->seg_off[IQ_WSE], H, TEPI_NONE, nullptr, nullptr, 0, G + n->seg_off[IQ_BSE]);
  g[2] = mk_gemm(B, H, H, op_dense(OP_KCONT, n->dpsi, H), op_dense(OP_XCONT, P + n->seg_off[IQ_WSE], H), n->dfeat, H, TEPI_MASK, nullptr, n->feat, H);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 3, st))) return rc;
  g[0] = mk_gemm(H, S, B, op_dense(OP_XCONT, n->dfeat, H), op_dense(OP_XCONT, n->last_x, S), G + n->seg_off[IQ_W1], S, TEPI_NONE, nullptr, nullptr, 0, G + n->seg_off[IQ_B1]);
  return core_tgemm(&n->core, "jh_tgemm_dense", g, 1, st);
}

JH_EXPORT int jh_iqnnet_backward(jh_iqnnet* n, const float* d_g, jh_stream stream) {
  JH_ARG(n && d_g);
  if (!n->last_x) return jh_fail(JH_ERR_STATE, "jh_iqnnet_backward without a preceding jh_iqnnet_learn_forward");
  hipStream_t st = jh_s(stream);
  if (n->tail == IQ_TAIL_NOISY) return riq_tail_backward(n, d_g, st);
  const int B = n->last_B, H = n->H, N = n->N, A = n->A, BN = B * N;
  const float* P = n->params;
  float* G = n->grads;
  float* dh2 = n->dA;
  TGemm g[2];
  int rc;
  // q: weight gradient (+ bias gradient as row sums) and data gradient (+ relu' of l2)
  g[0] = mk_gemm(A, H, BN, op_dense(OP_XCONT, d_g, A), op_dense(OP_XCONT, n->h2, H), G + n->seg_off[IQ_WQ], H, TEPI_NONE, nullptr, nullptr, 0, G + n->seg_off[IQ_BQ]);
  g[1] = mk_gemm(BN, H, A, op_dense(OP_KCONT, d_g, A), op_dense(OP_XCONT, P + n->seg_off[IQ_WQ], H), dh2, H, TEPI_MASK, nullptr, n->h2, H);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 2, st))) return rc;
  return iq_trunk_backward(n, st);
}

// ---------------------------------------------------------------------------------- the noisy dueling tail (Rainbow-IQN)
// Up to three (parameter set, noise draw, row range) jobs over n->h2 -> d_logits [rows][N][A] (network/rainbow_iqn.py:54-104): one
// effective-weight launch for all jobs, a1 | v1 as one [2H][H] operand per job, a2 and v2, the dueling combine with one support.
// noise null: W = mu (is_train False).
struct RiqTail {
  const float* P;
  const float* noise;
  int row0, rows;  // network rows, each N sampled rows
};
struct RiqW {
  const float *av1, *bav1, *a2, *ba2, *v2, *bv2;
};
static RiqW riq_w(const jh_iqnnet* n, int set) {
  const float* W = n->weff + (size_t)set * n->nd.set_stride;
  const NoisyDims& d = n->nd;
  return RiqW{W + d.o_av1, W + d.o_bav1, W + d.o_a2, W + d.o_ba2, W + d.o_v2, W + d.o_bv2};
}
static int riq_tail(jh_iqnnet* n, const RiqTail* jobs, int nj, float* d_logits, hipStream_t st) {
  const int H = n->H, N = n->N, A = n->A, A4 = n->A4;
  const NoisyDims& d = n->nd;
  NoiseSets ns{};
  ns.n_sets = nj;
  int max_rows = 0;
  for (int j = 0; j < nj; ++j) {
    ns.params[j] = jobs[j].P; ns.noise[j] = jobs[j].noise; ns.weff[j] = n->weff + (size_t)j * d.set_stride;
    if (jobs[j].rows > max_rows) max_rows = jobs[j].rows;
  }
  int64_t blocks = (n->n_noisy + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  JH_LAUNCH(jh_rb_noise_kernel, dim3((unsigned)blocks, nj), dim3(256), 0, st, d, ns, n->n_noisy);
  JH_LAUNCH_CHECK();
  TGemm g[6];
  int rc, ng = 0;
  for (int j = 0; j < nj; ++j) {
    const RiqW w = riq_w(n, j);
    const size_t r0 = (size_t)jobs[j].row0 * N;
    g[j] = mk_gemm(jobs[j].rows * N, 2 * H, H, op_dense(OP_KCONT, n->h2 + r0 * H, H), op_dense(OP_KCONT, w.av1, H), n->hav + r0 * 2 * H, 2 * H, TEPI_BIAS_RELU, w.bav1);
  }
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, nj, st))) return rc;
  for (int j = 0; j < nj; ++j) {
    const RiqW w = riq_w(n, j);
    const size_t r0 = (size_t)jobs[j].row0 * N;
    const float* hav = n->hav + r0 * 2 * H;
    g[ng++] = mk_gemm(jobs[j].rows * N, A, H, op_dense(OP_KCONT, hav, 2 * H), op_dense(OP_KCONT, w.a2, H), n->xa + r0 * A4, A4, TEPI_BIAS, w.ba2);
    g[ng++] = mk_gemm(jobs[j].rows * N, 1, H, op_dense(OP_KCONT, hav + H, 2 * H), op_dense(OP_KCONT, w.v2, H), n->xv + r0 * 4, 4, TEPI_BIAS, w.bv2);
  }
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, ng, st))) return rc;
  // the combine takes one row count for all sets: the jobs of a call have the same number of rows
  for (int j = 0; j < nj; ++j) JH_ARG(jobs[j].rows == max_rows);
  DuelSets ds{};
  for (int j = 0; j < nj; ++j) {
    const size_t r0 = (size_t)jobs[j].row0 * N;
    ds.xa[j] = n->xa + r0 * A4; ds.xv[j] = n->xv + r0 * 4; ds.out[j] = d_logits + r0 * A;
  }
  const int RN = max_rows * N;
  JH_LAUNCH(jh_rb_duel_fwd_kernel, dim3((RN + 255) / 256, nj), dim3(256), 0, st, ds, RN, A, 1, A4, 4);
  JH_LAUNCH_CHECK();
  return JH_OK;
}

// Backward of online(state) through the tail (draw 0's effective weights are set 0): the dueling backward, a2 / v2, then a1 | v1 -- weight
// gradients written in place as d(mu), data gradients through the relu masks, both streams' data gradients into h2 as ONE GEMM --, the
// shared trunk, and d(sig) = d(mu) * eps last.
static int riq_tail_backward(jh_iqnnet* n, const float* d_g, hipStream_t st) {
  const int B = n->last_B, H = n->H, N = n->N, A = n->A, A4 = n->A4, BN = B * N;
  float* G = n->grads;
  const RiqW w0 = riq_w(n, 0);
  JH_LAUNCH(jh_rb_duel_bwd_kernel, dim3((BN + 255) / 256), dim3(256), 0, st, d_g, BN, A, 1, n->dxa, A4, n->dxv, 4);
  JH_LAUNCH_CHECK();
  TGemm g[4];
  int rc;
  g[0] = mk_gemm(A, H, BN, op_dense(OP_XCONT, n->dxa, A4), op_dense(OP_XCONT, n->hav, 2 * H), G + n->seg_off[IQ_MU_A2], H, TEPI_NONE, nullptr, nullptr, 0,
                 G + n->seg_off[IQ_MUB_A2]);
  g[1] = mk_gemm(BN, H, A, op_dense(OP_KCONT, n->dxa, A4), op_dense(OP_XCONT, w0.a2, H), n->dhav, 2 * H, TEPI_MASK, nullptr, n->hav, 2 * H);
  g[2] = mk_gemm(1, H, BN, op_dense(OP_XCONT, n->dxv, 4), op_dense(OP_XCONT, n->hav + H, 2 * H), G + n->seg_off[IQ_MU_V2], H, TEPI_NONE, nullptr, nullptr, 0,
                 G + n->seg_off[IQ_MUB_V2]);
  g[3] = mk_gemm(BN, H, 1, op_dense(OP_KCONT, n->dxv, 4), op_dense(OP_XCONT, w0.v2, H), n->dhav + H, 2 * H, TEPI_MASK, nullptr, n->hav + H, 2 * H);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 4, st))) return rc;
  g[0] = mk_gemm(2 * H, H, BN, op_dense(OP_XCONT, n->dhav, 2 * H), op_dense(OP_XCONT, n->h2, H), G + n->seg_off[IQ_MU_AV1], H, TEPI_NONE, nullptr, nullptr, 0,
                 G + n->seg_off[IQ_MUB_AV1]);
  g[1] = mk_gemm(BN, H, 2 * H, op_dense(OP_KCONT, n->dhav, 2 * H), op_dense(OP_XCONT, w0.av1, H), n->dA, H, TEPI_MASK, nullptr, n->h2, H);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 2, st))) return rc;
  if ((rc = iq_trunk_backward(n, st))) return rc;
  if (!n->last_noise) return jh_fail(JH_ERR_STATE, "jh_iqnnet_backward: the noisy tail's last learn_forward had no noise draw");
  int64_t blocks = (n->n_noisy + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  JH_LAUNCH(jh_rb_noisy_grad_kernel, dim3((unsigned)blocks), dim3(256), 0, st, n->nd, n->last_noise, G, n->n_noisy);
  JH_LAUNCH_CHECK();
  return JH_OK;
}

JH_EXPORT int64_t jh_riqnnet_param_count_for(int32_t S, int32_t H, int32_t E, int32_t N, int32_t A) {
  jh_iqnnet tmp;
  if (iq_layout(&tmp, S, H, E, N, A, 1, IQ_TAIL_NOISY, 0)) return -1;
  return tmp.n_params;
}
JH_EXPORT int jh_riqnnet_create(jh_ctx* ctx, int32_t S, int32_t H, int32_t E, int32_t N, int32_t A, int32_t independent, int32_t max_batch, float* d_params,
                                float* d_target, float* d_grads, float* d_m, float* d_v, jh_iqnnet** out) {
  JH_ARG(independent == 0 || independent == 1);
  return iq_create(ctx, IQ_TAIL_NOISY, independent, S, H, E, N, A, max_batch, d_params, d_target, d_grads, d_m, d_v, out);
}
JH_EXPORT int32_t jh_riqnnet_segment_count(void) { return IQ_SEG_ALL; }
JH_EXPORT int64_t jh_riqnnet_noise_len(const jh_iqnnet* n) { return n && n->tail == IQ_TAIL_NOISY ? n->nd.noise_len : -1; }

JH_EXPORT int jh_riqnnet_forward(jh_iqnnet* n, int32_t which, const float* d_x, int32_t rows, const float* d_tau, const float* d_noise, float* d_logits,
                                 jh_stream stream) {
  JH_ARG(n && d_x && d_tau && d_logits);
  JH_ARG(rows > 0 && rows <= n->maxB && (which == 0 || which == 1) && n->tail == IQ_TAIL_NOISY);
  const float* P = which == 0 ? n->params : n->target;
  IqJob j{P, d_x, 0, rows};
  RiqTail t{P, d_noise, 0, rows};
  n->last_x = nullptr;  // the activations of a learn_forward are gone
  int rc = iq_trunk(n, &j, 1, d_tau, jh_s(stream));
  if (rc) return rc;
  return riq_tail(n, &t, 1, d_logits, jh_s(stream));
}

JH_EXPORT int jh_riqnnet_learn_forward(jh_iqnnet* n, const float* d_x, int32_t B, const float* d_tau, const float* d_noise, float* d_logits, jh_stream stream) {
  JH_ARG(n && d_x && d_tau && d_noise && d_logits);
  JH_ARG(B > 0 && B <= n->maxB && n->tail == IQ_TAIL_NOISY);
  // the trunk as IQN's two jobs; the tail as three, one per (parameter set, noise draw): the target job reads the target bucket's sigmas
  IqJob jobs[2] = {{n->params, d_x, 0, 2 * B}, {n->target, d_x + (size_t)B * n->S, 2 * B, B}};
  const int64_t nl = n->nd.noise_len;
  RiqTail tails[3] = {{n->params, d_noise, 0, B}, {n->params, d_noise + nl, B, B}, {n->target, d_noise + 2 * nl, 2 * B, B}};
  int rc = iq_trunk(n, jobs, 2, d_tau, jh_s(stream));
  if (rc) return rc;
  if ((rc = riq_tail(n, tails, 3, d_logits, jh_s(stream)))) return rc;
  n->last_x = d_x;
  n->last_B = B;
  n->last_noise = d_noise;
  return JH_OK;
}

JH_EXPORT int jh_iqnnet_optim_step(jh_iqnnet* n, float max_norm, jh_stream stream) {
  JH_ARG(n != nullptr);
  return jh_flat_adam_step(n->n_params, n->params, n->grads, n->m, n->v, n->opt.hyper, n->opt.ticket, n->core.norm_partial, max_norm, jh_s(stream));
}

// ---------------------------------------------------------------------------------- standalone entries
JH_EXPORT int jh_iqn_cos_features(jh_ctx* ctx, int64_t rows, int32_t E, const float* d_tau, float* d_out, jh_stream stream) {
  JH_ARG(ctx && d_tau && d_out);
  JH_ARG(rows > 0 && E > 0 && rows * E < ((int64_t)1 << 31));
  return iqn_cos(rows, E, d_tau, d_out, jh_s(stream));
}
JH_EXPORT int jh_iqn_hadamard(jh_ctx* ctx, int32_t B, int32_t N, int32_t H, const float* d_psi, const float* d_phi, float* d_out, jh_stream stream) {
  JH_ARG(ctx && d_psi && d_phi && d_out);
  JH_ARG(B > 0 && N > 0 && H > 0 && H % 4 == 0 && (int64_t)B * N * H < ((int64_t)1 << 31));
  return iqn_hadamard((int64_t)B * N, N, H, d_psi, d_phi, d_out, jh_s(stream));
}
JH_EXPORT int jh_iqn_hadamard_backward(jh_ctx* ctx, int32_t B, int32_t N, int32_t H, const float* d_grad_embed, const float* d_psi, const float* d_phi,
                                       float* d_grad_phi_pre, float* d_grad_psi_pre, jh_stream stream) {
  JH_ARG(ctx && d_grad_embed && d_psi && d_phi && d_grad_phi_pre && d_grad_psi_pre);
  JH_ARG(B > 0 && N > 0 && H > 0 && H % 4 == 0 && (int64_t)B * N * H < ((int64_t)1 << 31));
  return iqn_hadamard_bwd(B, N, H, d_grad_embed, d_psi, d_phi, d_grad_phi_pre, d_grad_psi_pre, jh_s(stream));
}
