// Device-resident PPO rollouts: policy-value forward, action sampling, env step with auto-reset, the transition and the acting-time
// capture for T timesteps of W envs in ONE launch, with no host involvement between the timesteps (DESIGN "Device-resident rollouts").
//
// Work split.  One workgroup (4 waves) owns 16 env rows -- one MFMA row tile -- for the whole rollout.  Rows never interact, so there
// is no grid-wide wait, no spin on memory and no communication between workgroups; every loop is bounded by T, H, S or A.  Everything
// a row computes is a function of (weights, env state, sampling seed, counter, env row): the tile a row falls in only decides which
// lane carries it, and every sum below runs in an order fixed by k alone.
//
// Per timestep, in LDS:  es [16][S] float64 env state  ->  h1 [16][H]  ->  h2 [16][H]  ->  heads [16][n_out]  ->  action  ->  es'.
//   layer 1   v_mfma_f32_16x16x4_f32, A = (float)es from LDS, B = W1 from L2 (4-byte loads: S need not be a multiple of 4); wave v owns the
//             column tiles v, v + 4, ... and carries eight of them at once (one A fragment, eight loads in flight)
//   layer 2   the same split of the H output columns: wave v computes column tiles v, v + 4, ... over the WHOLE k range, so no sum crosses
//             a wave and h2 needs no reduction.  W2 (1 MB at H = 512: it cannot live in LDS next to the activations) streams from L2,
//             16 bytes per lane per 16-deep k chunk, in blocks of eight chunks: the next block's eight pieces -- the next column tile's at a
//             tile's end -- are requested before the current block's 32 MFMAs are issued (32 x 32 cycles, about one L2 round trip; with
//             one chunk ahead the step was latency-bound, 46 us at H = 512), and two accumulator chains keep the matrix pipe from
//             waiting on its own result.  The activations are read from LDS with a row stride of H + 4 floats (rows 16 bytes apart in
//             the banks).
//   heads     n_out <= 40 outputs = up to three column tiles; here K is what the waves split (chunk c goes to wave c mod 4), the four
//             partial tiles meet in LDS (in the space of h1, dead by then) and are summed in wave order, bias last.
//   sampling  one thread per env row: jh_sample_discrete_at / jh_sample_continuous_at of jh_common.h, the host collectors' own statements,
//             keyed (seed, counter + t, env row).
//   env       jh_env_dyn.h, the host envs' own statements.  CartPole: the row's thread.  Control: one (row, i) element per thread, then
//             the row's thread for step count, reward, done and reset.
// LDS: 2 x 16 x (H + 4) x 4 bytes of activations + at most 20.5 KB for env state, coupling table, heads and actions; 160 KB per
// workgroup on gfx950 gives H <= 1024 (JH_DEVROLL_MAX_H), 152 KB at S = 64, A = 16.
#include "jh_common.h"
#include "jh_env_dyn.h"
#include "jh_devroll_mlp.h"

namespace {
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kRows = 16, kThreads = 256, kWaves = 4, kHeadLd = 40, kActLd = jh_env::kControlMaxA, kMaxTiles = 3;
constexpr int kPartFloats = kWaves * kMaxTiles * 4 * 64;

struct DevRollArgs {
  int W, T, S, H, A, n_out, cont, training, capture;
  const float *W1, *b1, *W2, *b2, *wh0, *bh0, *wh1, *bh1, *wv, *bv;
  uint64_t seed, ctr;
  double* es; int64_t* et; uint64_t* erng; const double* coupling;
  float* o_state; void* o_action; float* o_reward; float* o_next; uint8_t* o_done;
  float *c_h0, *c_h1, *c_v, *c_nv;
};

struct Lds {
  double *es, *P, *a2;
  int64_t* t;
  uint64_t* rng;
  float *h1, *h2, *heads, *act;
  int* acti;
};
__host__ __device__ inline size_t h1_floats(int H) { return (size_t)kRows * (H + 4) > (size_t)kPartFloats ? (size_t)kRows * (H + 4) : (size_t)kPartFloats; }
__host__ __device__ inline size_t table_doubles(int S, int A) { return ((size_t)S * A + 1) & ~(size_t)1; }  // even: what follows stays 16-byte aligned
__host__ __device__ inline size_t lds_bytes(int S, int A, int H) {
  return 8 * ((size_t)kRows * S + table_doubles(S, A) + 3 * kRows) + 4 * (h1_floats(H) + (size_t)kRows * (H + 4) + kRows * kHeadLd + kRows * kActLd + kRows);
}
__device__ inline Lds carve(char* base, int S, int A, int H) {
  Lds l;
  l.es = reinterpret_cast<double*>(base);
  l.P = l.es + (size_t)kRows * S;
  l.a2 = l.P + table_doubles(S, A);
  l.t = reinterpret_cast<int64_t*>(l.a2 + kRows);
  l.rng = reinterpret_cast<uint64_t*>(l.t + kRows);
  l.h1 = reinterpret_cast<float*>(l.rng + kRows);  // 16-byte aligned: every count above is even
  l.h2 = l.h1 + h1_floats(H);
  l.heads = l.h2 + (size_t)kRows * (H + 4);
  l.act = l.heads + kRows * kHeadLd;
  l.acti = reinterpret_cast<int*>(l.act + kRows * kActLd);
  return l;
}

// es -> h1 -> h2 -> heads, all in LDS; ends behind a workgroup barrier
__device__ void forward(const DevRollArgs& a, const Lds& l) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, kq = lane >> 4;
  const int H = a.H, S = a.S, ld = H + 4, tiles = H / 16;
  // ---- layers 1 and 2 (jh_devroll_mlp.h, shared with the other rollout kernels)
  jh_roll::layer1(a.W1, a.b1, l.es, S, H, l.h1, ld);
  __syncthreads();
  jh_roll::layer2(a.W2, a.b2, l.h1, ld, H, tiles, l.h2, ld);
  __syncthreads();  // h2 complete; h1 is dead from here on: its space takes the heads' partial tiles
  // ---- heads: output o = 16 q + r is a row of pi / mu, of log_std, or the value row; K split over the waves
  const int nt = (a.n_out + 15) / 16;
  float* part = l.h1;  // [wave][q][i][lane]
  {
    const float* wq[kMaxTiles];
#pragma unroll
    for (int q = 0; q < kMaxTiles; ++q) {
      const int o = q * 16 + r;
      wq[q] = o < a.A ? a.wh0 + (size_t)o * H : (a.cont && o < 2 * a.A) ? a.wh1 + (size_t)(o - a.A) * H : o == a.n_out - 1 ? a.wv : nullptr;
    }
    f32x4 acc[kMaxTiles];
#pragma unroll
    for (int q = 0; q < kMaxTiles; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c = wave; c < tiles; c += kWaves) {
      const int k = c * 16 + kq * 4;
      const float4 av = *reinterpret_cast<const float4*>(l.h2 + r * ld + k);
#pragma unroll
      for (int q = 0; q < kMaxTiles; ++q) {
        if (q < nt) {  // (uniform)
          // (4-byte loads: the rows behind a bias vector of A floats are not 16-byte aligned)
          const float4 bv = wq[q] ? make_float4(wq[q][k], wq[q][k + 1], wq[q][k + 2], wq[q][k + 3]) : make_float4(0.f, 0.f, 0.f, 0.f);
          acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc[q], 0, 0, 0);
          acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc[q], 0, 0, 0);
          acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc[q], 0, 0, 0);
          acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc[q], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < kMaxTiles; ++q)
      if (q < nt)
#pragma unroll
        for (int i = 0; i < 4; ++i) part[((wave * kMaxTiles + q) * 4 + i) * 64 + lane] = acc[q][i];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < kRows * a.n_out; e += kThreads) {
    const int row = e / a.n_out, o = e - row * a.n_out, q = o >> 4;
    const int src = (row >> 2) * 16 + (o & 15), i = row & 3;  // the 16x16 C / D map: row 4 kq + i sits in register i of lane 16 kq + column
    auto p = [&](int w) { return part[((w * kMaxTiles + q) * 4 + i) * 64 + src]; };
    const float b = o < a.A ? a.bh0[o] : (a.cont && o < 2 * a.A) ? a.bh1[o - a.A] : a.bv[0];
    l.heads[row * kHeadLd + o] = (((p(0) + p(1)) + p(2)) + p(3)) + b;
  }
  __syncthreads();
}

template <int ENV>  // 0: CartPole (discrete policy), 1: control (continuous policy)
__global__ void __launch_bounds__(kThreads) jh_devroll_kernel(DevRollArgs a) {
  extern __shared__ __attribute__((aligned(16))) char s_dyn[];
  const int S = a.S, A = a.A, T = a.T, tid = threadIdx.x;
  const Lds l = carve(s_dyn, S, A, a.H);
  const int w0 = (int)blockIdx.x * kRows;
  const int rows = a.W - w0 < kRows ? a.W - w0 : kRows;  // >= 1 by the grid
  for (int e = tid; e < kRows * S; e += kThreads) l.es[e] = e < rows * S ? a.es[(size_t)w0 * S + e] : 0.0;
  if (ENV == 1)
    for (int e = tid; e < S * A; e += kThreads) l.P[e] = a.coupling[e];
  if (tid < rows) { l.t[tid] = a.et[w0 + tid]; l.rng[tid] = a.erng[w0 + tid]; }
  __syncthreads();
  const bool mine = tid < rows;  // this thread carries env row w0 + tid through sampling, bookkeeping and reset
  const size_t row0 = (size_t)(w0 + tid) * T;
  const int vcol = a.n_out - 1;
  for (int t = 0; t <= T; ++t) {
    if (t == T && !a.capture) break;
    forward(a, l);
    if (mine && a.capture) {
      const float* z = l.heads + tid * kHeadLd;
      if (t > 0) a.c_nv[row0 + t - 1] = z[vcol];  // V(s_{t+1}); where done_t is set it belongs to the reset state
      if (t < T) {
        a.c_v[row0 + t] = z[vcol];
        for (int k = 0; k < A; ++k) a.c_h0[(row0 + t) * A + k] = z[k];
        if (a.cont)
          for (int k = 0; k < A; ++k) a.c_h1[(row0 + t) * A + k] = z[A + k];
      }
    }
    if (t == T) break;  // the value-only query behind the last step: only V is kept
    // ---- the observation acted on, and the action
    for (int e = tid; e < rows * S; e += kThreads) a.o_state[((size_t)(w0 + e / S) * T + t) * S + e % S] = (float)l.es[e];
    if (mine) {
      const float* z = l.heads + tid * kHeadLd;
      if (ENV == 0) {
        const int64_t act = jh_sample_discrete_at(A, a.seed, a.ctr + (uint64_t)t, z, w0 + tid, a.training);
        l.acti[tid] = (int)act;
        static_cast<int64_t*>(a.o_action)[row0 + t] = act;
      } else {
        float* ac = l.act + tid * kActLd;
        jh_sample_continuous_at(A, a.seed, a.ctr + (uint64_t)t, z, w0 + tid, a.training, ac);
        for (int k = 0; k < A; ++k) static_cast<float*>(a.o_action)[(row0 + t) * A + k] = ac[k];
        l.a2[tid] = jh_env::control_action_cost(ac, A);
      }
    }
    __syncthreads();  // the actions are in LDS, and every thread has read the state it stores
    // ---- the env step
    if (ENV == 0) {
      if (mine) {
        double* s = l.es + tid * 4;
        const bool d = jh_env::cartpole_advance(s, l.t[tid], l.acti[tid]);
        for (int k = 0; k < 4; ++k) a.o_next[(row0 + t) * 4 + k] = (float)s[k];  // the terminal observation where done
        a.o_done[row0 + t] = d ? 1 : 0;
        a.o_reward[row0 + t] = d ? jh_env::kRewardDone : jh_env::kRewardStep;
        if (d) jh_env::reset_row(s, 4, l.rng[tid], l.t[tid]);
      }
    } else {
      constexpr int kPer = kRows * jh_env::kControlMaxS / kThreads;
      double nx[kPer];
#pragma unroll
      for (int u = 0; u < kPer; ++u) {
        const int e = tid + u * kThreads;
        if (e < rows * S) {
          const int row = e / S, i = e - row * S;
          nx[u] = jh_env::control_next(l.es + row * S, l.act + row * kActLd, S, A, i, [&](int i_, int j_) { return l.P[i_ * A + j_]; });
        }
      }
      __syncthreads();  // every element has read the old state
#pragma unroll
      for (int u = 0; u < kPer; ++u) {
        const int e = tid + u * kThreads;
        if (e < rows * S) {
          l.es[e] = nx[u];
          a.o_next[((size_t)(w0 + e / S) * T + t) * S + e % S] = (float)nx[u];
        }
      }
      __syncthreads();
      if (mine) {
        double* s = l.es + tid * S;
        l.t[tid] += 1;
        const bool d = jh_env::control_done(s[0], l.t[tid]);
        a.o_done[row0 + t] = d ? 1 : 0;
        a.o_reward[row0 + t] = jh_env::control_reward(s[0], l.a2[tid]);
        if (d) jh_env::reset_row(s, S, l.rng[tid], l.t[tid]);
      }
    }
    __syncthreads();
  }
  for (int e = tid; e < rows * S; e += kThreads) a.es[(size_t)w0 * S + e] = l.es[e];
  if (mine) { a.et[w0 + tid] = l.t[tid]; a.erng[w0 + tid] = l.rng[tid]; }
}

int upload(void* dst, const void* src, size_t bytes) {
  JH_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  return JH_OK;
}
}  // namespace

// Creation runs the host env's own seeding and reset (jh_cartpole_create / jh_control_create) and uploads: a device env starts
// bit-identical to the host env of the same seed.
JH_EXPORT int jh_devenv_create(jh_ctx* ctx, int32_t kind, int32_t W, int32_t S, int32_t A, uint64_t seed, jh_devenv** out) {
  JH_ARG(ctx && out && W > 0 && (kind == JH_DEVENV_CARTPOLE || kind == JH_DEVENV_CONTROL));
  JH_HIP(hipSetDevice(ctx->device));
  jh_cartpole* cp = nullptr;
  jh_control* cc = nullptr;
  if (kind == JH_DEVENV_CARTPOLE) {
    JH_ARG(S == 4 && A == 2);
    if (int rc = jh_cartpole_create(W, seed, &cp)) return rc;
  } else if (int rc = jh_control_create(W, S, A, seed, &cc)) {
    return rc;
  }
  jh_devenv* e = new jh_devenv();
  e->ctx = ctx; e->kind = kind; e->W = W; e->S = S; e->A = A;
  int rc = JH_OK;
  auto D = [&](auto** p, size_t bytes) {
    if (!rc && hipMalloc((void**)p, bytes) != hipSuccess) rc = jh_fail(JH_ERR_NOMEM, "jh_devenv_create: hipMalloc of %zu bytes failed", bytes);
  };
  D(&e->s, sizeof(double) * (size_t)W * S); D(&e->t, sizeof(int64_t) * (size_t)W); D(&e->rng, sizeof(uint64_t) * (size_t)W);
  if (cc) D(&e->coupling, sizeof(double) * (size_t)S * A);
  if (!rc) rc = upload(e->s, cp ? cp->s.data() : cc->s.data(), sizeof(double) * (size_t)W * S);
  if (!rc) rc = upload(e->t, cp ? cp->t.data() : cc->t.data(), sizeof(int64_t) * (size_t)W);
  if (!rc) rc = upload(e->rng, cp ? cp->rng.data() : cc->rng.data(), sizeof(uint64_t) * (size_t)W);
  if (!rc && cc) {
    std::vector<double> P((size_t)S * A);
    for (int i = 0; i < S; ++i)
      for (int j = 0; j < A; ++j) P[(size_t)i * A + j] = jh_env::control_coupling(i, j);
    rc = upload(e->coupling, P.data(), sizeof(double) * P.size());
  }
  jh_cartpole_destroy(cp);
  jh_control_destroy(cc);
  if (rc) { jh_devenv_destroy(e); return rc; }
  *out = e;
  return JH_OK;
}

JH_EXPORT void jh_devenv_destroy(jh_devenv* e) {
  if (!e) return;
  (void)hipSetDevice(e->ctx->device);
  (void)hipDeviceSynchronize();
  (void)hipFree(e->s); (void)hipFree(e->t); (void)hipFree(e->rng); (void)hipFree(e->coupling); (void)hipFree(e->scratch);
  delete e;
}

// Host copies of the env state (s float64 [W][S], t int64 [W], rng uint64 [W]; any of them NULL: skipped).  Blocking, ordered behind `stream`.
JH_EXPORT int jh_devenv_get_state(jh_devenv* e, double* h_s, int64_t* h_t, uint64_t* h_rng, jh_stream stream) {
  JH_ARG(e != nullptr);
  JH_HIP(hipStreamSynchronize(jh_s(stream)));
  if (h_s) JH_HIP(hipMemcpy(h_s, e->s, sizeof(double) * (size_t)e->W * e->S, hipMemcpyDeviceToHost));
  if (h_t) JH_HIP(hipMemcpy(h_t, e->t, sizeof(int64_t) * (size_t)e->W, hipMemcpyDeviceToHost));
  if (h_rng) JH_HIP(hipMemcpy(h_rng, e->rng, sizeof(uint64_t) * (size_t)e->W, hipMemcpyDeviceToHost));
  return JH_OK;
}

JH_EXPORT int jh_devenv_set_state(jh_devenv* e, const double* h_s, const int64_t* h_t, const uint64_t* h_rng, jh_stream stream) {
  JH_ARG(e != nullptr);
  JH_HIP(hipStreamSynchronize(jh_s(stream)));
  if (h_s) JH_HIP(hipMemcpy(e->s, h_s, sizeof(double) * (size_t)e->W * e->S, hipMemcpyHostToDevice));
  if (h_t) JH_HIP(hipMemcpy(e->t, h_t, sizeof(int64_t) * (size_t)e->W, hipMemcpyHostToDevice));
  if (h_rng) JH_HIP(hipMemcpy(e->rng, h_rng, sizeof(uint64_t) * (size_t)e->W, hipMemcpyHostToDevice));
  return JH_OK;
}

// T timesteps of all W envs in one launch, then the ring append of the W * T rows (worker-major: row = w * T + t) by jh_store_push_device
// -- the store's own append, so its bookkeeping exists once.  cols: the store's column numbers of state, action, reward, next_state, done.
// d_value != NULL: the acting-time capture with the layout and meaning of jh_collector_set_capture, written by the kernel itself.
JH_EXPORT int jh_devroll_run(jh_pponet* n, jh_devenv* e, jh_store* store, const int32_t* cols, int32_t T, int32_t training, float* d_h0, float* d_h1,
                             float* d_value, float* d_next_value, jh_stream stream) {
  JH_ARG(n && e && store && cols && T > 0);
  JH_ARG(n->ctx == e->ctx && n->S == e->S && n->A == e->A && n->cont == (e->kind == JH_DEVENV_CONTROL ? 1 : 0));
  if (n->H > JH_DEVROLL_MAX_H)
    return jh_fail(JH_ERR_ARG, "jh_devroll_run: hidden_size %d: the rollout kernel keeps both activation tiles in LDS and serves hidden_size %% 16 == 0 up to %d", n->H, JH_DEVROLL_MAX_H);
  JH_ARG(!d_value || (d_h0 && d_next_value && (!n->cont || d_h1)));
  const int S = e->S, A = e->A, cont = n->cont;
  const int64_t rows = (int64_t)e->W * T;
  JH_ARG(store->n_cols == 5 && rows <= store->capacity);
  const int dt[5] = {JH_F32, cont ? JH_F32 : JH_I64, JH_F32, JH_F32, JH_U8};
  const int64_t el[5] = {S, cont ? A : 1, 1, S, 1};
  for (int c = 0; c < 5; ++c) {
    JH_ARG(cols[c] >= 0 && cols[c] < 5 && store->cols[cols[c]].dtype == dt[c] && store->cols[cols[c]].elems == el[c]);
    for (int d = 0; d < c; ++d) JH_ARG(cols[d] != cols[c]);
  }
  hipStream_t st = jh_s(stream);
  JH_HIP(hipSetDevice(e->ctx->device));
  size_t off[5], total = 0;
  for (int c = 0; c < 5; ++c) {
    off[c] = total;
    total += (jh_dtype_size(dt[c]) * (size_t)el[c] * (size_t)rows + 255) & ~(size_t)255;
  }
  if (total > e->scratch_bytes) {
    JH_HIP(hipStreamSynchronize(st));  // an earlier run's append may still read the old block
    (void)hipFree(e->scratch);
    e->scratch = nullptr; e->scratch_bytes = 0;
    if (hipMalloc((void**)&e->scratch, total) != hipSuccess) return jh_fail(JH_ERR_NOMEM, "jh_devroll_run: hipMalloc of %zu bytes failed", total);
    e->scratch_bytes = total;
  }
  DevRollArgs a{};
  a.W = e->W; a.T = T; a.S = S; a.H = n->H; a.A = A; a.n_out = n->n_out; a.cont = cont; a.training = training ? 1 : 0; a.capture = d_value ? 1 : 0;
  const float* p = n->params;
  a.W1 = p + n->o_w1; a.b1 = p + n->o_b1; a.W2 = p + n->o_w2; a.b2 = p + n->o_b2; a.wh0 = p + n->o_wh0; a.bh0 = p + n->o_bh0;
  a.wh1 = cont ? p + n->o_wh1 : nullptr; a.bh1 = cont ? p + n->o_bh1 : nullptr; a.wv = p + n->o_wv; a.bv = p + n->o_bv;
  a.seed = n->act_seed; a.ctr = n->act_ctr;
  a.es = e->s; a.et = e->t; a.erng = e->rng; a.coupling = e->coupling;
  a.o_state = (float*)(e->scratch + off[0]); a.o_action = e->scratch + off[1]; a.o_reward = (float*)(e->scratch + off[2]);
  a.o_next = (float*)(e->scratch + off[3]); a.o_done = (uint8_t*)(e->scratch + off[4]);
  a.c_h0 = d_h0; a.c_h1 = cont ? d_h1 : nullptr; a.c_v = d_value; a.c_nv = d_next_value;
  const size_t lds = lds_bytes(S, A, n->H);
  const dim3 grid((unsigned)((e->W + kRows - 1) / kRows));
  static size_t lds_allowed[2] = {64 << 10, 64 << 10};  // beyond 64 KB of dynamic LDS a kernel has to be told once
  if (lds > lds_allowed[cont]) {
    const void* fn = cont ? reinterpret_cast<const void*>(&jh_devroll_kernel<1>) : reinterpret_cast<const void*>(&jh_devroll_kernel<0>);
    JH_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    lds_allowed[cont] = lds;
  }
  if (cont) JH_LAUNCH_NAMED("jh_devroll_kernel<control>", jh_devroll_kernel<1>, grid, dim3(kThreads), lds, st, a);
  else JH_LAUNCH_NAMED("jh_devroll_kernel<cartpole>", jh_devroll_kernel<0>, grid, dim3(kThreads), lds, st, a);
  JH_LAUNCH_CHECK();
  n->act_ctr += (uint64_t)T;
  const void* src[5];
  for (int c = 0; c < 5; ++c) src[cols[c]] = e->scratch + off[c];
  return jh_store_push_device(store, rows, src, stream);
}
