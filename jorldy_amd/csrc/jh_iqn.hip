// Implicit quantile network (core/network/iqn.py:9-47, core/agent/iqn.py:12-146) on the device:
//   jh_iqnnet_*      the network with an MLP head: x -> relu(head.l) -> psi = relu(state_embed), tau -> cos(tau * i * pi) ->
//                    phi = relu(sample_embed), embed = psi (.) phi, relu(l1), relu(l2), q  -> [rows][N][A]; the three forwards of
//                    learn() in shared launches, the backward of online(s), Adam (jh_rbnet's optimizer kernels on the flat buckets)
// Every dense contraction runs on the tile engine (jh_tgemm.hip) under the call-site name "dense".  The kernels of this file are the
// elementwise steps between them: cosine features, the Hadamard product and its backward.  The loss and acting entries jh_iqn_loss /
// jh_iqn_act are the sample-major instantiations of the quantile family's kernels in jh_qr.hip.
// No floating-point atomics: every sum has a fixed order, so two runs (and a graph replay) give the same bits.
#include "jh_netcore.h"

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
enum { IQ_W1, IQ_B1, IQ_WSE, IQ_BSE, IQ_WSA, IQ_BSA, IQ_WL1, IQ_BL1, IQ_WL2, IQ_BL2, IQ_WQ, IQ_BQ, IQ_SEG_COUNT };

struct jh_iqnnet {
  NetCore core;
  FlatOptim opt;
  int S = 0, H = 0, E = 0, N = 0, A = 0, maxB = 0;
  int64_t seg_off[IQ_SEG_COUNT] = {0};
  int seg_rows[IQ_SEG_COUNT] = {0}, seg_cols[IQ_SEG_COUNT] = {0};
  int64_t n_params = 0;
  float *params = nullptr, *target = nullptr, *grads = nullptr, *m = nullptr, *v = nullptr;
  // activations of up to three forwards, rows [online: 2 maxB | target: maxB] (x N for the per-sample ones)
  float *feat = nullptr, *psi = nullptr, *cosf_ = nullptr, *phi = nullptr, *emb = nullptr, *h1 = nullptr, *h2 = nullptr;
  float *dA = nullptr, *dB = nullptr, *dpsi = nullptr, *dfeat = nullptr;  // backward: [maxB * N][H] x 2, [maxB][H] x 2
  const float* last_x = nullptr;  // state rows of the last learn_forward (the head's weight gradient reads them again)
  int last_B = 0;
};

static int iq_layout(jh_iqnnet* n, int32_t S, int32_t H, int32_t E, int32_t N, int32_t A, int32_t max_batch) {
  JH_ARG(S > 0 && H > 0 && H % 4 == 0 && E > 0 && A > 0 && max_batch > 0);
  JH_ARG(N >= 1 && N <= 256);
  JH_ARG((int64_t)3 * max_batch * N * (int64_t)(H > E ? H : E) < ((int64_t)1 << 31));  // the tile engine indexes rows x columns in 32 bits
  n->S = S; n->H = H; n->E = E; n->N = N; n->A = A; n->maxB = max_batch;
  auto seg = [&](int id, int rows, int cols) { n->seg_rows[id] = rows; n->seg_cols[id] = cols; };
  seg(IQ_W1, H, S); seg(IQ_B1, 1, H);
  seg(IQ_WSE, H, H); seg(IQ_BSE, 1, H);
  seg(IQ_WSA, H, E); seg(IQ_BSA, 1, H);
  seg(IQ_WL1, H, H); seg(IQ_BL1, 1, H);
  seg(IQ_WL2, H, H); seg(IQ_BL2, 1, H);
  seg(IQ_WQ, A, H); seg(IQ_BQ, 1, A);
  n->n_params = seg_pack(n->seg_rows, n->seg_cols, 0, IQ_SEG_COUNT, n->seg_off);
  return JH_OK;
}

JH_EXPORT int64_t jh_iqnnet_param_count_for(int32_t S, int32_t H, int32_t E, int32_t N, int32_t A) {
  jh_iqnnet tmp;
  if (iq_layout(&tmp, S, H, E, N, A, 1)) return -1;
  return tmp.n_params;
}

JH_EXPORT int jh_iqnnet_create(jh_ctx* ctx, int32_t S, int32_t H, int32_t E, int32_t N, int32_t A, int32_t max_batch, float* d_params, float* d_target,
                               float* d_grads, float* d_m, float* d_v, jh_iqnnet** out) {
  JH_ARG(ctx && out && d_params && d_target && d_grads && d_m && d_v);
  JH_HIP(hipSetDevice(ctx->device));
  jh_iqnnet* n = new jh_iqnnet();
  n->core.ctx = ctx;
  int rc = iq_layout(n, S, H, E, N, A, max_batch);
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

JH_EXPORT void jh_iqnnet_destroy(jh_iqnnet* n) {
  if (!n) return;
  core_release(&n->core);
  delete n;
}

JH_EXPORT int32_t jh_iqnnet_segment_count(void) { return IQ_SEG_COUNT; }
JH_EXPORT int jh_iqnnet_segment(const jh_iqnnet* n, int32_t i, int64_t* offset, int32_t* rows, int32_t* cols) {
  return seg_query(n, IQ_SEG_COUNT, i, offset, rows, cols);
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
static int iq_forward(jh_iqnnet* n, const IqJob* jobs, int nj, const float* d_tau, float* d_logits, hipStream_t st) {
  const int S = n->S, H = n->H, E = n->E, N = n->N, A = n->A;
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
  JH_ARG(rows > 0 && rows <= n->maxB && (which == 0 || which == 1));
  IqJob j{which == 0 ? n->params : n->target, d_x, 0, rows};
  n->last_x = nullptr;  // the activations of a learn_forward are gone
  return iq_forward(n, &j, 1, d_tau, d_logits, jh_s(stream));
}

JH_EXPORT int jh_iqnnet_learn_forward(jh_iqnnet* n, const float* d_x, int32_t B, const float* d_tau, float* d_logits, jh_stream stream) {
  JH_ARG(n && d_x && d_tau && d_logits);
  JH_ARG(B > 0 && B <= n->maxB);
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
  JH_ARG(B > 0 && B <= n->maxB);
  IqJob jobs[3] = {{n->params, d_x, 0, B}, {n->params, d_x, B, B}, {n->target, d_x + (size_t)B * n->S, 2 * B, B}};
  int rc = iq_forward(n, jobs, 3, d_tau, d_logits, jh_s(stream));
  if (rc) return rc;
  n->last_x = d_x;
  n->last_B = B;
  return JH_OK;
}

// Backward of logits[0] = online(state) of the last jh_iqnnet_learn_forward / _m: d_g = d(loss)/d(logits) [B][N][A]; fills the gradient
// bucket (same layout as the parameters).  The online activations of the state rows are the first B (x N) rows of every buffer.
JH_EXPORT int jh_iqnnet_backward(jh_iqnnet* n, const float* d_g, jh_stream stream) {
  JH_ARG(n && d_g);
  if (!n->last_x) return jh_fail(JH_ERR_STATE, "jh_iqnnet_backward without a preceding jh_iqnnet_learn_forward");
  hipStream_t st = jh_s(stream);
  const int B = n->last_B, S = n->S, H = n->H, E = n->E, N = n->N, A = n->A, BN = B * N;
  const float* P = n->params;
  float* G = n->grads;
  float *dh2 = n->dA, *dh1 = n->dB, *dem = n->dA, *dphi = n->dB;
  TGemm g[3];
  int rc;
  // q: weight gradient (+ bias gradient as row sums) and data gradient (+ relu' of l2)
  g[0] = mk_gemm(A, H, BN, op_dense(OP_XCONT, d_g, A), op_dense(OP_XCONT, n->h2, H), G + n->seg_off[IQ_WQ], H, TEPI_NONE, nullptr, nullptr, 0, G + n->seg_off[IQ_BQ]);
  g[1] = mk_gemm(BN, H, A, op_dense(OP_KCONT, d_g, A), op_dense(OP_XCONT, P + n->seg_off[IQ_WQ], H), dh2, H, TEPI_MASK, nullptr, n->h2, H);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 2, st))) return rc;
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
