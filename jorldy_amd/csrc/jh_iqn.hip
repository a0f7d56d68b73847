// Implicit quantile network (core/network/iqn.py:9-47, core/agent/iqn.py:12-146) on the device:
//   jh_iqnnet_*      the network with an MLP head: x -> relu(head.l) -> psi = relu(state_embed), tau -> cos(tau * i * pi) ->
//                    phi = relu(sample_embed), embed = psi (.) phi, relu(l1), relu(l2), q  -> [rows][N][A]; the three forwards of
//                    learn() in shared launches, the backward of online(s), Adam (jh_rbnet's optimizer kernels on the flat buckets)
//   jh_iqn_loss      pairwise quantile-Huber loss with per-sample tau, forward and backward to online(s)   (iqn.py:89-121)
//   jh_iqn_act       epsilon-greedy acting on the mean over the N samples                                  (iqn.py:60-76, 142-146)
// Every dense contraction runs on the tile engine (jh_tgemm.hip) under the call-site name "dense".  The kernels of this file are the
// elementwise / reducing steps between them: cosine features, the Hadamard product and its backward, loss and acting.
// No floating-point atomics: every sum has a fixed order, so two runs (and a graph replay) give the same bits.
#include "jh_fused.h"
#include "jh_tgemm.h"

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

// ---------------------------------------------------------------------------------- loss
struct IqnArgs {
  int B, A, N;
  const float *logit, *next_logit, *target_logit, *action, *reward, *done, *tau;
  float gamma;
  float *grad, *stats, *partial;  // partial [B][4] = {sum_j sum_i w * huber, max Q, max logit, min logit} of a sample
};

// Mean over the N samples of action column a of one row block z [N][A] on one wave (logits2Q, iqn.py:142-146): every lane returns it.
__device__ __forceinline__ float iqn_col_mean(const float* __restrict__ z, int N, int A, int a, int lane, float& cmx, float& cmn) {
  float s = 0.f;
  cmx = -3.4e38f;
  cmn = 3.4e38f;
  for (int k = lane; k < N; k += 64) {
    const float v = z[(size_t)k * A + a];
    s += v;
    cmx = fmaxf(cmx, v);
    cmn = fminf(cmn, v);
  }
  cmx = jh_wave_max(cmx);
  cmn = jh_wave_min(cmn);
  return jh_wave_sum(s) / (float)N;
}

// jh_qr_block_kernel's algorithm on the [B][N][A] layout with tau per sample: one workgroup of 256 threads per sample (N <= 256:
// thread i owns prediction sample i).  LDS: [N] Bellman image of the target samples, [A] selector means, [4][3] per-wave statistics,
// [16] reduction.  Every thread stays to the end: the work of threads i >= N is predicated, not skipped.
__global__ void __launch_bounds__(256) jh_iqn_block_kernel(IqnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int b = blockIdx.x, A = a.A, N = a.N;
  float* s_T = smem;           // [N]
  float* s_qsel = s_T + N;     // [A]
  float* s_stat = s_qsel + A;  // [4][3]
  float* s_red = s_stat + 12;  // [16]
  int act = (int)a.action[b];
  act = act < 0 ? 0 : (act >= A ? A - 1 : act);
  const float r = a.reward[b], dn = a.done[b];
  const size_t base = (size_t)b * N * A;
  const bool own = tid < N;
  const int ti = own ? tid : N - 1;
  const float P = a.logit[base + (size_t)ti * A + act];
  const float tau = a.tau[(size_t)b * N + ti];  // the FIRST forward's draw for this sample (iqn.py:90, 96)
  const float inv_tau = 1.f - tau;              // iqn.py:120
  // ---- phase 1: means over the samples of online(s) (statistics) and online(s') (selector), action columns strided over the waves
  float maxq = -3.4e38f, maxl = -3.4e38f, minl = 3.4e38f;
  for (int aa = wid; aa < A; aa += 4) {
    float cmx, cmn, x0, x1;
    const float q = iqn_col_mean(a.logit + base, N, A, aa, lane, cmx, cmn);
    maxq = fmaxf(maxq, q);
    maxl = fmaxf(maxl, cmx);
    minl = fminf(minl, cmn);
    const float q2 = iqn_col_mean(a.next_logit + base, N, A, aa, lane, x0, x1);
    if (lane == 0) s_qsel[aa] = q2;
  }
  // the entries of the actions not taken: zero gradient (the backward reads all of it)
  for (int k = tid; k < N * A; k += 256)
    if (k % A != act) a.grad[base + k] = 0.f;
  if (lane == 0) { s_stat[wid * 3 + 0] = maxq; s_stat[wid * 3 + 1] = maxl; s_stat[wid * 3 + 2] = minl; }
  __syncthreads();
  // ---- a* = first maximum of the online net's means at s' (iqn.py:106); every thread walks the same A values
  int best = 0;
  float bq = -3.4e38f;
  for (int aa = 0; aa < A; ++aa) {
    const float q = s_qsel[aa];
    if (q > bq) { bq = q; best = aa; }
  }
  // ---- phase 2: theta_target = reward + (1 - done) * gamma * target(s')[a*]  (iqn.py:109-111, in torch's order of operations)
  if (own) s_T[tid] = r + ((1.f - dn) * a.gamma) * a.target_logit[base + (size_t)tid * A + best];
  __syncthreads();
  // ---- phase 3: thread i walks the targets j; e = T[j] - P[i], smooth_l1 (beta 1), weight tau[i] / 1 - tau[i] by the sign of e
  float ls = 0.f, gs = 0.f;
  for (int j = 0; j < N; ++j) {
    const float e = s_T[j] - P;  // the same LDS word for every lane: a broadcast
    const float ae = fabsf(e);
    const float hub = ae < 1.f ? 0.5f * e * e : ae - 0.5f;
    const float w = e < 0.f ? inv_tau : tau;
    ls += w * hub;
    gs += w * fminf(fmaxf(e, -1.f), 1.f);
  }
  if (own) a.grad[base + (size_t)tid * A + act] = -gs / ((float)a.B * (float)N);
  // ---- phase 4: the sample's loss, wave shuffle tree then the waves in order
  const float tot = jh_block_reduce(own ? ls : 0.f, s_red, JhAdd(), 0.f);
  if (tid == 0) {
    float mq = -3.4e38f, ml = -3.4e38f, nl = 3.4e38f;
    const int nw = A < 4 ? A : 4;  // waves that saw at least one action column
    for (int w = 0; w < nw; ++w) {
      mq = fmaxf(mq, s_stat[w * 3 + 0]);
      ml = fmaxf(ml, s_stat[w * 3 + 1]);
      nl = fminf(nl, s_stat[w * 3 + 2]);
    }
    float* p = a.partial + 4 * (size_t)b;
    p[0] = tot; p[1] = mq; p[2] = ml; p[3] = nl;
  }
}

// Sum of the per-sample partials in a fixed order -> d_stats, payload fenced before the arrival marks (as jh_qr_finish_kernel).
__global__ void __launch_bounds__(256) jh_iqn_finish_kernel(IqnArgs a) {
  __shared__ float s_red[16];
  float sl = 0.f, mq = -3.4e38f, ml = -3.4e38f, nl = 3.4e38f;
  for (int b = threadIdx.x; b < a.B; b += 256) {
    sl += a.partial[4 * (size_t)b];
    mq = fmaxf(mq, a.partial[4 * (size_t)b + 1]);
    ml = fmaxf(ml, a.partial[4 * (size_t)b + 2]);
    nl = fminf(nl, a.partial[4 * (size_t)b + 3]);
  }
  sl = jh_block_reduce(sl, s_red, JhAdd(), 0.f);
  mq = jh_block_reduce(mq, s_red, JhMax(), -3.4e38f);
  ml = jh_block_reduce(ml, s_red, JhMax(), -3.4e38f);
  nl = jh_block_reduce(nl, s_red, JhMin(), 3.4e38f);
  if (threadIdx.x == 0 && a.stats) {
    a.stats[0] = sl / ((float)a.B * (float)a.N);  // iqn.py:121: mean over (b, j) of the sum over i
    a.stats[1] = mq;
    a.stats[2] = ml;
    a.stats[3] = nl;
    a.stats[4] = 0.f;
    a.stats[6] = 0.f;
    __threadfence_system();  // payload before the arrival marks [5], [7] (mapped host memory, jh_host_wait_marks)
    a.stats[5] = a.stats[7] = 0.f;
  }
}

// IQN.act for R actor rows in one call: one wave per row, Q = mean over the N samples, first maximum like torch.argmax,
// epsilon-greedy with the host's draws (jh_value_act's rules), q_taken fenced before the action.
// Every lane of a wave stays through the shuffles: rows beyond R read row R - 1 and write nothing.
__global__ void __launch_bounds__(256) jh_iqn_act_kernel(int R, int A, int N, const float* __restrict__ logits, const float* __restrict__ eps,
                                                         const double* __restrict__ u, const int64_t* __restrict__ rand_action,
                                                         int64_t* __restrict__ action, float* __restrict__ q_taken, float* __restrict__ q_all) {
  const int lane = threadIdx.x & 63;
  const int row0 = blockIdx.x * 4 + (threadIdx.x >> 6);
  const bool live = row0 < R;
  const int row = live ? row0 : R - 1;
  float best = -3.4e38f, q_rand = 0.f;
  int best_a = 0;
  int ra = rand_action ? (int)rand_action[row] : 0;
  ra = ra < 0 ? 0 : (ra >= A ? A - 1 : ra);
  for (int a = 0; a < A; ++a) {
    float cmx, cmn;
    const float q = iqn_col_mean(logits + (size_t)row * N * A, N, A, a, lane, cmx, cmn);
    if (q_all && live && lane == 0) q_all[(size_t)row * A + a] = q;
    if (q > best) { best = q; best_a = a; }
    if (a == ra) q_rand = q;
  }
  if (live && lane == 0) {
    const bool explore = eps && u && u[row] < (double)eps[row];
    if (q_taken) {
      q_taken[row] = explore ? q_rand : best;
      __threadfence_system();
    }
    action[row] = explore ? ra : best_a;
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
  jh_ctx* ctx = nullptr;
  int S = 0, H = 0, E = 0, N = 0, A = 0, maxB = 0;
  int64_t seg_off[IQ_SEG_COUNT] = {0};
  int seg_rows[IQ_SEG_COUNT] = {0}, seg_cols[IQ_SEG_COUNT] = {0};
  int64_t n_params = 0;
  float *params = nullptr, *target = nullptr, *grads = nullptr, *m = nullptr, *v = nullptr;
  float* hyper = nullptr;
  float* norm_partial = nullptr;
  unsigned* ticket = nullptr;
  // activations of up to three forwards, rows [online: 2 maxB | target: maxB] (x N for the per-sample ones)
  float *feat = nullptr, *psi = nullptr, *cosf_ = nullptr, *phi = nullptr, *emb = nullptr, *h1 = nullptr, *h2 = nullptr;
  float *dA = nullptr, *dB = nullptr, *dpsi = nullptr, *dfeat = nullptr;  // backward: [maxB * N][H] x 2, [maxB][H] x 2
  float* ws = nullptr;
  size_t ws_floats = 0;
  unsigned* cnt = nullptr;
  int cnt_slots = 0;
  const float* last_x = nullptr;  // state rows of the last learn_forward (the head's weight gradient reads them again)
  int last_B = 0;
  std::vector<void*> owned;
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
  int64_t off = 0;
  for (int i = 0; i < IQ_SEG_COUNT; ++i) {
    n->seg_off[i] = off;
    off = (off + (int64_t)n->seg_rows[i] * n->seg_cols[i] + 3) & ~(int64_t)3;
  }
  n->n_params = off;
  return JH_OK;
}

static int iq_alloc(jh_iqnnet* n, void** out, size_t bytes, bool zero) {
  if (bytes == 0) bytes = 16;
  hipError_t e = hipMalloc(out, bytes);
  if (e != hipSuccess) return jh_fail(JH_ERR_NOMEM, "jh_iqnnet: hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
  n->owned.push_back(*out);
  if (zero) JH_HIP(hipMemset(*out, 0, bytes));
  return JH_OK;
}

static int iq_tgemm(jh_iqnnet* n, TGemm* probs, int ng, hipStream_t st) {
  TGemmWorkspace w;
  w.ws = n->ws; w.ws_floats = n->ws_floats; w.cnt = n->cnt; w.cnt_slots = n->cnt_slots;
  return jh_tgemm_launch(w, "jh_tgemm_dense", probs, ng, st);
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
  n->ctx = ctx;
  int rc = iq_layout(n, S, H, E, N, A, max_batch);
  if (rc) {
    delete n;
    return rc;
  }
  n->params = d_params; n->target = d_target; n->grads = d_grads; n->m = d_m; n->v = d_v;
  const size_t R3 = 3 * (size_t)max_batch, RN = R3 * N, BN = (size_t)max_batch * N;
  auto A4 = [&](float** p, size_t floats, bool zero = true) { if (!rc) rc = iq_alloc(n, (void**)p, floats * sizeof(float), zero); };
  A4(&n->hyper, JH_HY_FLOATS);
  A4(&n->norm_partial, 256);
  if (!rc) rc = iq_alloc(n, (void**)&n->ticket, 2048, true);  // jh_rb_optim_kernel: eight counters 128 bytes apart + the one on top of them
  A4(&n->feat, R3 * H); A4(&n->psi, R3 * H);
  A4(&n->cosf_, RN * E); A4(&n->phi, RN * H); A4(&n->emb, RN * H); A4(&n->h1, RN * H); A4(&n->h2, RN * H);
  A4(&n->dA, BN * H); A4(&n->dB, BN * H); A4(&n->dpsi, (size_t)max_batch * H); A4(&n->dfeat, (size_t)max_batch * H);
  n->ws_floats = (size_t)8 << 20;  // 32 MB of split-K partials
  A4(&n->ws, n->ws_floats, false);
  n->cnt_slots = 8192;
  if (!rc) rc = iq_alloc(n, (void**)&n->cnt, sizeof(unsigned) * (size_t)n->cnt_slots * kTgemmCntStride, true);
  if (rc) {
    for (void* p : n->owned) (void)hipFree(p);
    delete n;
    return rc;
  }
  float hy[JH_HY_FLOATS];
  jh_hyper_fill(hy, 1e-3, 0.9, 0.999, 1e-8, 0.0);
  JH_HIP(hipMemcpy(n->hyper, hy, sizeof(hy), hipMemcpyHostToDevice));
  JH_HIP(hipDeviceSynchronize());
  *out = n;
  return JH_OK;
}

JH_EXPORT void jh_iqnnet_destroy(jh_iqnnet* n) {
  if (!n) return;
  (void)hipSetDevice(n->ctx->device);
  (void)hipDeviceSynchronize();
  for (void* p : n->owned) (void)hipFree(p);
  delete n;
}

JH_EXPORT int32_t jh_iqnnet_segment_count(void) { return IQ_SEG_COUNT; }
JH_EXPORT int jh_iqnnet_segment(const jh_iqnnet* n, int32_t i, int64_t* offset, int32_t* rows, int32_t* cols) {
  JH_ARG(n && i >= 0 && i < IQ_SEG_COUNT && offset && rows && cols);
  *offset = n->seg_off[i]; *rows = n->seg_rows[i]; *cols = n->seg_cols[i];
  return JH_OK;
}

JH_EXPORT int jh_iqnnet_set_hyper(jh_iqnnet* n, double lr, double beta1, double beta2, double eps, int64_t step, jh_stream stream) {
  JH_ARG(n != nullptr);
  jh_pinned_slab* slab = nullptr;
  int rc = jh_ctx_slab(n->ctx, 64, &slab);
  if (rc) return rc;
  jh_hyper_fill((float*)slab->host, lr, beta1, beta2, eps, (double)step);
  JH_HIP(hipMemcpyAsync(n->hyper, slab->dev, JH_HY_FLOATS * sizeof(float), hipMemcpyDeviceToDevice, jh_s(stream)));
  return jh_ctx_slab_release(n->ctx, slab, jh_s(stream));
}
JH_EXPORT int jh_iqnnet_set_lr(jh_iqnnet* n, double lr, jh_stream stream) {
  JH_ARG(n != nullptr);
  jh_pinned_slab* slab = nullptr;
  int rc = jh_ctx_slab(n->ctx, 16, &slab);
  if (rc) return rc;
  *(float*)slab->host = (float)lr;
  JH_HIP(hipMemcpyAsync(n->hyper, slab->dev, sizeof(float), hipMemcpyDeviceToDevice, jh_s(stream)));
  return jh_ctx_slab_release(n->ctx, slab, jh_s(stream));
}
JH_EXPORT int jh_iqnnet_sync_target(jh_iqnnet* n, jh_stream stream) {
  JH_ARG(n != nullptr);
  JH_HIP(hipMemcpyAsync(n->target, n->params, sizeof(float) * (size_t)n->n_params, hipMemcpyDeviceToDevice, jh_s(stream)));
  return JH_OK;
}

// Up to two (parameter set, input rows) jobs that sit one after the other in the activation buffers: job j's rows start at row0.
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
  TGemm g[2];
  int rc;
  // head.l and state_embed on the state rows
  for (int j = 0; j < nj; ++j) {
    const IqJob& J = jobs[j];
    g[j] = mk_gemm(J.rows, H, S, op_dense(OP_KCONT, J.x, S), op_dense(OP_KCONT, J.P + n->seg_off[IQ_W1], S), n->feat + (size_t)J.row0 * H, H,
                   TEPI_BIAS_RELU, J.P + n->seg_off[IQ_B1]);
  }
  if ((rc = iq_tgemm(n, g, nj, st))) return rc;
  for (int j = 0; j < nj; ++j) {
    const IqJob& J = jobs[j];
    g[j] = mk_gemm(J.rows, H, H, op_dense(OP_KCONT, n->feat + (size_t)J.row0 * H, H), op_dense(OP_KCONT, J.P + n->seg_off[IQ_WSE], H), n->psi + (size_t)J.row0 * H, H,
                   TEPI_BIAS_RELU, J.P + n->seg_off[IQ_BSE]);
  }
  if ((rc = iq_tgemm(n, g, nj, st))) return rc;
  // cosine features of every (row, sample), then sample_embed
  if ((rc = iqn_cos((int64_t)total * N, E, d_tau, n->cosf_, st))) return rc;
  for (int j = 0; j < nj; ++j) {
    const IqJob& J = jobs[j];
    const size_t r0 = (size_t)J.row0 * N;
    g[j] = mk_gemm(J.rows * N, H, E, op_dense(OP_KCONT, n->cosf_ + r0 * E, E), op_dense(OP_KCONT, J.P + n->seg_off[IQ_WSA], E), n->phi + r0 * H, H, TEPI_BIAS_RELU,
                   J.P + n->seg_off[IQ_BSA]);
  }
  if ((rc = iq_tgemm(n, g, nj, st))) return rc;
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
    if ((rc = iq_tgemm(n, g, nj, st))) return rc;
  }
  for (int j = 0; j < nj; ++j) {
    const IqJob& J = jobs[j];
    const size_t r0 = (size_t)J.row0 * N;
    g[j] = mk_gemm(J.rows * N, A, H, op_dense(OP_KCONT, n->h2 + r0 * H, H), op_dense(OP_KCONT, J.P + n->seg_off[IQ_WQ], H), d_logits + r0 * A, A, TEPI_BIAS,
                   J.P + n->seg_off[IQ_BQ]);
  }
  return iq_tgemm(n, g, nj, st);
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

// Backward of logits[0] = online(state) of the last jh_iqnnet_learn_forward: d_g = d(loss)/d(logits) [B][N][A]; fills the gradient
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
  if ((rc = iq_tgemm(n, g, 2, st))) return rc;
  g[0] = mk_gemm(H, H, BN, op_dense(OP_XCONT, dh2, H), op_dense(OP_XCONT, n->h1, H), G + n->seg_off[IQ_WL2], H, TEPI_NONE, nullptr, nullptr, 0, G + n->seg_off[IQ_BL2]);
  g[1] = mk_gemm(BN, H, H, op_dense(OP_KCONT, dh2, H), op_dense(OP_XCONT, P + n->seg_off[IQ_WL2], H), dh1, H, TEPI_MASK, nullptr, n->h1, H);
  if ((rc = iq_tgemm(n, g, 2, st))) return rc;
  // l1 reads the product itself: no relu between them
  g[0] = mk_gemm(H, H, BN, op_dense(OP_XCONT, dh1, H), op_dense(OP_XCONT, n->emb, H), G + n->seg_off[IQ_WL1], H, TEPI_NONE, nullptr, nullptr, 0, G + n->seg_off[IQ_BL1]);
  g[1] = mk_gemm(BN, H, H, op_dense(OP_KCONT, dh1, H), op_dense(OP_XCONT, P + n->seg_off[IQ_WL1], H), dem, H, TEPI_NONE);
  if ((rc = iq_tgemm(n, g, 2, st))) return rc;
  if ((rc = iqn_hadamard_bwd(B, N, H, dem, n->psi, n->phi, dphi, n->dpsi, st))) return rc;
  // sample_embed (its input, the cosine features, has no gradient) and state_embed
  g[0] = mk_gemm(H, E, BN, op_dense(OP_XCONT, dphi, H), op_dense(OP_XCONT, n->cosf_, E), G + n->seg_off[IQ_WSA], E, TEPI_NONE, nullptr, nullptr, 0, G + n->seg_off[IQ_BSA]);
  g[1] = mk_gemm(H, H, B, op_dense(OP_XCONT, n->dpsi, H), op_dense(OP_XCONT, n->feat, H), G + n->seg_off[IQ_WSE], H, TEPI_NONE, nullptr, nullptr, 0, G + n->seg_off[IQ_BSE]);
  g[2] = mk_gemm(B, H, H, op_dense(OP_KCONT, n->dpsi, H), op_dense(OP_XCONT, P + n->seg_off[IQ_WSE], H), n->dfeat, H, TEPI_MASK, nullptr, n->feat, H);
  if ((rc = iq_tgemm(n, g, 3, st))) return rc;
  g[0] = mk_gemm(H, S, B, op_dense(OP_XCONT, n->dfeat, H), op_dense(OP_XCONT, n->last_x, S), G + n->seg_off[IQ_W1], S, TEPI_NONE, nullptr, nullptr, 0, G + n->seg_off[IQ_B1]);
  return iq_tgemm(n, g, 1, st);
}

JH_EXPORT int jh_iqnnet_optim_step(jh_iqnnet* n, float max_norm, jh_stream stream) {
  JH_ARG(n != nullptr);
  return jh_flat_adam_step(n->n_params, n->params, n->grads, n->m, n->v, n->hyper, n->ticket, n->norm_partial, max_norm, jh_s(stream));
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

JH_EXPORT int jh_iqn_loss(jh_ctx* ctx, int32_t B, int32_t A, int32_t N, const float* d_logit, const float* d_next_logit_online, const float* d_target_logit,
                          const float* d_action, const float* d_reward, const float* d_done, const float* d_tau, float gamma, float* d_grad_logit, float* d_stats,
                          jh_stream stream) {
  JH_ARG(ctx && d_logit && d_next_logit_online && d_target_logit && d_action && d_reward && d_done && d_tau && d_grad_logit);
  JH_ARG(B >= 1 && A >= 1 && N >= 1 && N <= 256);
  hipStream_t st = jh_s(stream);
  void* scratch = nullptr;
  int rc = jh_ctx_scratch(ctx, sizeof(float) * 4 * (size_t)B, &scratch);
  if (rc) return rc;
  IqnArgs a{};
  a.B = B; a.A = A; a.N = N;
  a.logit = d_logit; a.next_logit = d_next_logit_online; a.target_logit = d_target_logit; a.action = d_action;
  a.reward = d_reward; a.done = d_done; a.tau = d_tau; a.gamma = gamma; a.grad = d_grad_logit; a.stats = d_stats;
  a.partial = (float*)scratch;
  const size_t lds = sizeof(float) * ((size_t)N + (size_t)A + 12 + 16);
  JH_ARG(lds <= 64 * 1024);
  JH_LAUNCH(jh_iqn_block_kernel, dim3(B), dim3(256), lds, st, a);
  JH_LAUNCH_CHECK();
  JH_LAUNCH(jh_iqn_finish_kernel, dim3(1), dim3(256), 0, st, a);
  JH_LAUNCH_CHECK();
  return JH_OK;
}

JH_EXPORT int jh_iqn_act(jh_ctx* ctx, int32_t R, int32_t A, int32_t N, const float* d_logits, const float* h_eps, const double* h_u,
                         const int64_t* h_rand_action, int64_t* d_action, float* d_q_taken, float* d_q_all, jh_stream stream) {
  JH_ARG(ctx && d_logits && d_action);
  JH_ARG(R > 0 && A > 0 && N > 0);
  JH_ARG((h_eps == nullptr) == (h_u == nullptr) && (h_eps == nullptr) == (h_rand_action == nullptr));
  hipStream_t st = jh_s(stream);
  const float* d_eps = nullptr;
  const double* d_u = nullptr;
  const int64_t* d_ra = nullptr;
  jh_pinned_slab* slab = nullptr;
  if (h_eps) {  // the draws ride in a pinned, device-mapped slab the kernel reads in place
    const size_t o_u = ((sizeof(float) * (size_t)R + 255) & ~(size_t)255), o_r = o_u + ((sizeof(double) * (size_t)R + 255) & ~(size_t)255);
    int rc = jh_ctx_slab(ctx, o_r + sizeof(int64_t) * (size_t)R + 256, &slab);
    if (rc) return rc;
    memcpy(slab->host, h_eps, sizeof(float) * (size_t)R);
    memcpy((char*)slab->host + o_u, h_u, sizeof(double) * (size_t)R);
    memcpy((char*)slab->host + o_r, h_rand_action, sizeof(int64_t) * (size_t)R);
    d_eps = (const float*)slab->dev;
    d_u = (const double*)((char*)slab->dev + o_u);
    d_ra = (const int64_t*)((char*)slab->dev + o_r);
  }
  JH_LAUNCH(jh_iqn_act_kernel, dim3((R + 3) / 4), dim3(256), 0, st, R, A, N, d_logits, d_eps, d_u, d_ra, d_action, d_q_taken, d_q_all);
  JH_LAUNCH_CHECK();
  return slab ? jh_ctx_slab_release(ctx, slab, st) : JH_OK;
}
