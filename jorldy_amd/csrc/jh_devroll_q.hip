// Device-resident Ape-X actors: Q forward, per-actor epsilon-greedy, CartPole step with auto-reset, the n-step window and the actor-side
// priority |G_n - q| for T timesteps of W envs in ONE launch (DESIGN "Device-resident Ape-X actors").  Env row i of W is actor i.
//
// Work split (the discipline of jh_devroll.hip).  One workgroup (4 waves) owns 16 env rows -- one MFMA row tile -- for the whole run.  Rows
// never interact: no grid-wide wait, no spin on memory, no float atomics; every loop is bounded by T, H, S, A or n_step, and every sum
// runs in an order fixed by k alone, so a row's output is a function of (weights, env state, window, seed, counter, env row, epsilon_i).
//
// Per timestep, in LDS:  es [16][S] float64  ->  x1 [16][H]  ->  x2 [16][N2]  ->  q [16][A]  ->  action, q_t  ->  row + priority  ->  es'.
//   layer 1   head.l, v_mfma_f32_16x16x4_f32: wave v owns the column tiles v, v + 4, ..., eight at a time behind one observation fragment
//   layer 2   kind q: l (H -> H), N2 = H.  kind dueling: l1_a | l1_v stacked (H -> 2H), N2 = 2H.  Wave v computes the output column tiles
//             v, v + 4, ... over the WHOLE k range (no sum crosses a wave); the weights stream from L2 in blocks of eight 16-deep k chunks, the
//             next block in flight during the current block's 32 MFMAs; the activations are read from LDS with a row stride of H + 4 floats
//   tail      kind q: q (H -> A), one column tile.  kind dueling: TWO column tiles that read different halves of x2 -- l2_a over columns
//             [0, H), l2_v (one weight row) over [H, 2H).  The k range is what the waves split (chunk c goes to wave c mod 4); the partial
//             tiles meet in LDS, in the space of x1 (dead by then), and are summed in wave order, bias last.  The row's thread then forms
//             q_k = (v + a_k) - mean(a), the mean summed over k in index order
//   act       the row's thread: greedy = first index of the largest float32 q; u0, u1 = the collectors' counter-based uniforms at keys
//             2 key + 1, 2 key + 2 with key = seed * FNV + (counter + t) * golden + env row; u0 < epsilon_i: action = floor(u1 * A).
//             q_t = q of the action TAKEN
//   window    the last n_step timesteps of (reward, done, q, action) per row live in LDS for the run; their states, n_step x 16 x S floats,
//             in an HBM ring per env (they do not fit beside the dueling activations at large H).  Entry t of the ring sits in slot t mod n_step.
//             At timestep t with t >= n_step (counted over ALL runs: the window is never cleared, not at an episode end either) the slot
//             holds entry t - n_step, which becomes the emitted row -- state, action, reward[n], done[n] of steps t - n .. t - 1, next_state
//             = s_t, priority = | fold(q_t) - q_{t-n} | with fold: x <- r_i + (1 - d_i) gamma x for i = n - 1 .. 0, in double -- and is then
//             overwritten with entry t.  Rows go out time-major: row = (t - t_first) * W + env row
//   env       jh_env_dyn.h, the host env's own statements, by the row's thread
//
// LDS in bytes, S = 4, n_step at its cap 16:   896 (es, t, rng, epsilon)  +  4 x [ max(16 (H + 4), 2048) (x1 | tail partials)
//   + 16 (N2 + 4) (x2)  +  320 (q)  +  1024 (window) ].   kind q: 128 H + 6 784 -> H <= 1216 inside 160 KB;
//   kind dueling: 192 H + 6 784 -> H <= 816 (163 456 of 163 840 bytes).  x1 and x2 are live together during layer 2; the tail's partial tiles
//   alias x1; nothing aliases x2.
#include "jh_common.h"
#include "jh_env_dyn.h"
#include "jh_devroll_mlp.h"

struct jh_devwin {
  jh_ctx* ctx = nullptr;
  int W = 0, S = 0, n = 0;
  int64_t seen = 0;             // timesteps every env has been through since creation
  uint64_t seed = 0, ctr = 0;   // the counter-based exploration stream
  char* block = nullptr;        // ws float [W][n][S] | wq float [W][n] | wr float [W][n] | wa int32 [W][n] | wd int32 [W][n]
  size_t block_bytes = 0;
};

namespace {
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kRows = 16, kThreads = 256, kWaves = 4, kQLd = 20, kVCol = 16, kTailTiles = 2;
constexpr int kPartFloats = kWaves * kTailTiles * 4 * 64;
constexpr size_t kLdsMax = 160u << 10;
constexpr int kHeader = 24;  // seen, seed, counter in front of a saved block

struct QArgs {
  int W, T, S, H, A, N2, dueling, n, t_first;
  int64_t seen;
  const float *W1, *b1, *W2, *b2, *wa, *ba, *wv, *bv;
  uint64_t seed, ctr;
  double gamma;
  const double* eps;
  double* es; int64_t* et; uint64_t* erng;
  float *ws, *wq, *wr; int *wact, *wd;
  float* o_state; int64_t* o_action; float* o_reward; float* o_next; uint8_t* o_done; double* o_prio;
};

struct Lds {
  double *es, *eps;
  int64_t* t;
  uint64_t* rng;
  float *x1, *x2, *q, *wq, *wr;
  int *wact, *wd;
};
__host__ __device__ inline size_t x1_floats(int H) { return (size_t)kRows * (H + 4) > (size_t)kPartFloats ? (size_t)kRows * (H + 4) : (size_t)kPartFloats; }
__host__ __device__ inline size_t lds_bytes(int S, int H, int N2, int n) {
  return 8 * ((size_t)kRows * S + 3 * kRows) + 4 * (x1_floats(H) + (size_t)kRows * (N2 + 4) + kRows * kQLd + 4 * (size_t)kRows * n);
}
__device__ inline Lds carve(char* base, int S, int H, int N2, int n) {
  Lds l;
  l.es = reinterpret_cast<double*>(base);
  l.eps = l.es + (size_t)kRows * S;
  l.t = reinterpret_cast<int64_t*>(l.eps + kRows);
  l.rng = reinterpret_cast<uint64_t*>(l.t + kRows);
  l.x1 = reinterpret_cast<float*>(l.rng + kRows);  // 16-byte aligned: every count above is even
  l.x2 = l.x1 + x1_floats(H);
  l.q = l.x2 + (size_t)kRows * (N2 + 4);
  l.wq = l.q + kRows * kQLd;
  l.wr = l.wq + kRows * n;
  l.wact = reinterpret_cast<int*>(l.wr + kRows * n);
  l.wd = l.wact + kRows * n;
  return l;
}

// es -> x1 -> x2 -> q (dueling: a in columns [0, A), v in column kVCol, uncombined), all in LDS; ends behind a workgroup barrier
__device__ void forward(const QArgs& a, const Lds& l) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, kq = lane >> 4;
  const int H = a.H, S = a.S, ld = H + 4, ld2 = a.N2 + 4, kt = H / 16, ot = a.N2 / 16;
  // ---- layers 1 and 2 (jh_devroll_mlp.h, shared with the other rollout kernels): layer 2 has `ot` output column tiles, H / 16, or 2H / 16
  // for the stacked a | v layer
  jh_roll::layer1(a.W1, a.b1, l.es, S, H, l.x1, ld);
  __syncthreads();
  jh_roll::layer2(a.W2, a.b2, l.x1, ld, H, ot, l.x2, ld2);
  __syncthreads();  // x2 complete; x1 is dead from here on: its space takes the tail's partial tiles
  // ---- tail: column tile 0 = q / l2_a over x2[:, 0 .. H), column tile 1 (dueling) = l2_v over x2[:, H .. 2H); K split over the waves
  const int nt = 1 + a.dueling;
  float* part = l.x1;  // [wave][tile][i][lane]
  {
    const float* wrow[kTailTiles] = {r < a.A ? a.wa + (size_t)r * H : nullptr, (a.dueling && r == 0) ? a.wv : nullptr};
    f32x4 acc[kTailTiles];
#pragma unroll
    for (int q = 0; q < kTailTiles; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c = wave; c < kt; c += kWaves) {
      const int k = c * 16 + kq * 4;
#pragma unroll
      for (int q = 0; q < kTailTiles; ++q) {
        if (q < nt) {  // (uniform)
          const float4 av = *reinterpret_cast<const float4*>(l.x2 + r * ld2 + q * H + k);
          const float4 bv = wrow[q] ? *reinterpret_cast<const float4*>(wrow[q] + k) : make_float4(0.f, 0.f, 0.f, 0.f);  // (segments and rows of H floats: 16-byte aligned)
          acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc[q], 0, 0, 0);
          acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc[q], 0, 0, 0);
          acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc[q], 0, 0, 0);
          acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc[q], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < kTailTiles; ++q)
      if (q < nt)
#pragma unroll
        for (int i = 0; i < 4; ++i) part[((wave * kTailTiles + q) * 4 + i) * 64 + lane] = acc[q][i];
  }
  __syncthreads();
  const int n_out = a.A + a.dueling;
  for (int e = threadIdx.x; e < kRows * n_out; e += kThreads) {
    const int row = e / n_out, o = e - row * n_out, q = o < a.A ? 0 : 1, col = o < a.A ? o : 0;
    const int src = (row >> 2) * 16 + col, i = row & 3;  // the 16x16 C / D map: row 4 kq + i sits in register i of lane 16 kq + column
    auto p = [&](int w) { return part[((w * kTailTiles + q) * 4 + i) * 64 + src]; };
    const float b = q == 0 ? a.ba[o] : a.bv[0];
    l.q[row * kQLd + (q == 0 ? o : kVCol)] = (((p(0) + p(1)) + p(2)) + p(3)) + b;
  }
  __syncthreads();
}

__global__ void __launch_bounds__(kThreads) jh_devroll_q_kernel(QArgs a) {
  extern __shared__ __attribute__((aligned(16))) char s_dyn[];
  const int S = a.S, A = a.A, n = a.n, tid = threadIdx.x;
  const Lds l = carve(s_dyn, S, a.H, a.N2, n);
  const int w0 = (int)blockIdx.x * kRows;
  const int rows = a.W - w0 < kRows ? a.W - w0 : kRows;  // >= 1 by the grid
  for (int e = tid; e < kRows * S; e += kThreads) l.es[e] = e < rows * S ? a.es[(size_t)w0 * S + e] : 0.0;
  for (int e = tid; e < rows * n; e += kThreads) {  // (row, slot) of the carried window: contiguous per env row
    const size_t g = (size_t)w0 * n + e;
    l.wq[e] = a.wq[g]; l.wr[e] = a.wr[g]; l.wact[e] = a.wact[g]; l.wd[e] = a.wd[g];
  }
  if (tid < rows) { l.t[tid] = a.et[w0 + tid]; l.rng[tid] = a.erng[w0 + tid]; l.eps[tid] = a.eps[w0 + tid]; }
  __syncthreads();
  const bool mine = tid < rows;  // this thread carries env row w0 + tid through acting, window, env step and reset
  const int w = w0 + tid;
  for (int t = 0; t < a.T; ++t) {
    const int64_t gt = a.seen + t;
    const int slot = (int)(gt % n);
    const bool emit = t >= a.t_first;  // gt >= n_step
    const size_t rbase = emit ? (size_t)(t - a.t_first) * a.W : 0;
    // ---- the states: the ring's slot holds s_{t-n}; it goes out with s_t as next_state and takes s_t (one thread per element, read then write)
    for (int e = tid; e < rows * S; e += kThreads) {
      const int row = e / S, k = e - row * S;
      float* ring = a.ws + ((size_t)(w0 + row) * n + slot) * S + k;
      const float cur = (float)l.es[e];
      if (emit) {
        a.o_state[(rbase + w0 + row) * S + k] = *ring;
        a.o_next[(rbase + w0 + row) * S + k] = cur;
      }
      *ring = cur;
    }
    forward(a, l);
    if (mine) {
      // ---- q of the row, the greedy action and the draw
      const float* z = l.q + tid * kQLd;
      float mean = 0.f;
      if (a.dueling) {
        for (int k = 0; k < A; ++k) mean += z[k];
        mean = mean / (float)A;
      }
      auto qk = [&](int k) { return a.dueling ? (z[kVCol] + z[k]) - mean : z[k]; };
      int act = 0;
      float best = qk(0);
      for (int k = 1; k < A; ++k) {
        const float v = qk(k);
        if (v > best) { best = v; act = k; }
      }
      float qt = best;
      const uint64_t key = a.seed * 0x100000001B3ull + (a.ctr + (uint64_t)t) * 0x9E3779B97F4A7C15ull + (uint64_t)w;
      if (jh_u01_of(key * 2 + 1) < l.eps[tid]) {
        act = (int)(jh_u01_of(key * 2 + 2) * (double)A);
        act = act < A ? act : A - 1;
        qt = qk(act);
      }
      // ---- the row of entry t - n and its priority
      if (emit) {
        const size_t row = rbase + w;
        a.o_action[row] = l.wact[tid * n + slot];
        double x = (double)qt;
        for (int i = n - 1; i >= 0; --i) {
          const int sl = slot + i < n ? slot + i : slot + i - n;
          const float r = l.wr[tid * n + sl];
          const int d = l.wd[tid * n + sl];
          a.o_reward[row * n + i] = r;
          a.o_done[row * n + i] = (uint8_t)d;
          x = (double)r + ((1.0 - (double)d) * a.gamma) * x;
        }
        a.o_prio[row] = fabs(x - (double)l.wq[tid * n + slot]);
      }
      // ---- the env step; entry t takes the slot
      double* s = l.es + tid * S;
      const bool d = jh_env::cartpole_advance(s, l.t[tid], act);
      if (d) jh_env::reset_row(s, S, l.rng[tid], l.t[tid]);
      l.wq[tid * n + slot] = qt;
      l.wr[tid * n + slot] = d ? jh_env::kRewardDone : jh_env::kRewardStep;
      l.wact[tid * n + slot] = act;
      l.wd[tid * n + slot] = d ? 1 : 0;
    }
    __syncthreads();
  }
  for (int e = tid; e < rows * S; e += kThreads) a.es[(size_t)w0 * S + e] = l.es[e];
  for (int e = tid; e < rows * n; e += kThreads) {
    const size_t g = (size_t)w0 * n + e;
    a.wq[g] = l.wq[e]; a.wr[g] = l.wr[e]; a.wact[g] = l.wact[e]; a.wd[g] = l.wd[e];
  }
  if (mine) { a.et[w] = l.t[tid]; a.erng[w] = l.rng[tid]; }
}

size_t states_bytes(const jh_devwin* w) { return sizeof(float) * (size_t)w->W * w->n * w->S; }
size_t lane_bytes(const jh_devwin* w) { return 4 * (size_t)w->W * w->n; }
}  // namespace

// The window block starts zeroed with no timestep seen: the first n_step timesteps of every env emit nothing.
JH_EXPORT int jh_devwin_create(jh_ctx* ctx, int32_t W, int32_t S, int32_t n_step, uint64_t seed, jh_devwin** out) {
  JH_ARG(ctx && out && W > 0 && S > 0 && n_step >= 1 && n_step <= JH_DEVROLL_Q_MAX_NSTEP);
  JH_HIP(hipSetDevice(ctx->device));
  jh_devwin* w = new jh_devwin();
  w->ctx = ctx; w->W = W; w->S = S; w->n = n_step; w->seed = seed;
  w->block_bytes = states_bytes(w) + 4 * lane_bytes(w);
  if (hipMalloc((void**)&w->block, w->block_bytes) != hipSuccess) {
    const int rc = jh_fail(JH_ERR_NOMEM, "jh_devwin_create: hipMalloc of %zu bytes failed", w->block_bytes);
    delete w;
    return rc;
  }
  if (hipMemset(w->block, 0, w->block_bytes) != hipSuccess) {
    const int rc = jh_fail(JH_ERR_HIP, "jh_devwin_create: hipMemset failed");
    jh_devwin_destroy(w);
    return rc;
  }
  *out = w;
  return JH_OK;
}

JH_EXPORT void jh_devwin_destroy(jh_devwin* w) {
  if (!w) return;
  (void)hipSetDevice(w->ctx->device);
  (void)hipDeviceSynchronize();
  (void)hipFree(w->block);
  delete w;
}

JH_EXPORT int64_t jh_devwin_state_bytes(const jh_devwin* w) { return w ? (int64_t)(kHeader + w->block_bytes) : -1; }

JH_EXPORT int jh_devwin_position(const jh_devwin* w, int64_t* seen, uint64_t* seed, uint64_t* counter) {
  JH_ARG(w != nullptr);
  if (seen) *seen = w->seen;
  if (seed) *seed = w->seed;
  if (counter) *counter = w->ctr;
  return JH_OK;
}

// h_block: jh_devwin_state_bytes bytes = {seen, seed, counter} + the device block.  Blocking, ordered behind `stream`.
JH_EXPORT int jh_devwin_get_state(jh_devwin* w, void* h_block, jh_stream stream) {
  JH_ARG(w && h_block);
  JH_HIP(hipStreamSynchronize(jh_s(stream)));
  char* h = static_cast<char*>(h_block);
  memcpy(h, &w->seen, 8); memcpy(h + 8, &w->seed, 8); memcpy(h + 16, &w->ctr, 8);
  JH_HIP(hipMemcpy(h + kHeader, w->block, w->block_bytes, hipMemcpyDeviceToHost));
  return JH_OK;
}

JH_EXPORT int jh_devwin_set_state(jh_devwin* w, const void* h_block, jh_stream stream) {
  JH_ARG(w && h_block);
  const char* h = static_cast<const char*>(h_block);
  int64_t seen;
  memcpy(&seen, h, 8);
  JH_ARG(seen >= 0);
  JH_HIP(hipStreamSynchronize(jh_s(stream)));
  w->seen = seen;
  memcpy(&w->seed, h + 8, 8); memcpy(&w->ctr, h + 16, 8);
  JH_HIP(hipMemcpy(w->block, h + kHeader, w->block_bytes, hipMemcpyHostToDevice));
  return JH_OK;
}

JH_EXPORT int64_t jh_devroll_q_rows(const jh_devwin* w, int32_t T) {
  if (!w || T <= 0) return -1;
  const int64_t wait = w->n > w->seen ? w->n - w->seen : 0;  // timesteps of this run before the first row
  return (int64_t)w->W * (T > wait ? T - wait : 0);
}

// T timesteps of all W envs in one launch.  The jh_devroll_q_rows(win, T) rows are written time-major into the caller's device columns
// (state f32 [S], action i64, reward f32 [n_step], next_state f32 [S], done u8 [n_step], priority f64); the caller appends them
// (jh_store_push_device + jh_per_push_device), so the ring and tree bookkeeping exists once.  The columns may be NULL when the run emits nothing.
JH_EXPORT int jh_devroll_q_run(jh_rbnet* net, const float* d_params, jh_devenv* e, jh_devwin* win, int32_t T, const double* d_eps, double gamma,
                               float* d_state, int64_t* d_action, float* d_reward, float* d_next_state, uint8_t* d_done, double* d_priority,
                               int64_t out_rows, jh_stream stream) {
  JH_ARG(net && d_params && e && win && d_eps && T > 0);
  JH_ARG(e->kind == JH_DEVENV_CARTPOLE && e->ctx == win->ctx && e->W == win->W && e->S == win->S);
  // the network's shape from its segment table: 0 head.l [H][S], 6 l [H][H] (kind q) | 8 l1_a|l1_v [2H][H] (kind dueling), 12 q / l2_a [A][H], 16 l2_v [1][H]
  int64_t off[20];
  int32_t sr[20], sc[20];
  for (int i = 0; i < 20; ++i)
    if (int rc = jh_rbnet_segment(net, i, &off[i], &sr[i], &sc[i])) return rc;
  const int H = sr[0], A = sr[12];
  const bool dueling = sr[8] > 0, mlp = sr[2] == 0 && sr[4] == 0, plain = sr[9] == 0 && sr[13] == 0 && sr[17] == 0;
  if (!mlp || !plain || sc[0] != e->S || A != e->A || sc[12] != H || (dueling ? (sr[6] != 0 || sr[8] != 2 * H || sc[8] != H || sr[16] != 1) : (sr[6] != H || sc[6] != H || sr[16] != 0)))
    return jh_fail(JH_ERR_ARG, "jh_devroll_q_run: the network must be kind q or dueling on the mlp head, %d -> %d like the env", e->S, e->A);
  const int N2 = dueling ? 2 * H : H, cap = dueling ? JH_DEVROLL_Q_MAX_H_DUELING : JH_DEVROLL_Q_MAX_H;
  const size_t lds = lds_bytes(e->S, H, N2, win->n);
  if (H % 16 != 0 || H > cap || A > 16 || lds > kLdsMax)
    return jh_fail(JH_ERR_ARG, "jh_devroll_q_run: hidden_size %d: the actor kernel keeps the H and the %s activation tile of a 16-row workgroup in LDS and serves "
                   "hidden_size %% 16 == 0 up to %d for this kind", H, dueling ? "2H" : "second H", cap);
  const int64_t rows = jh_devroll_q_rows(win, T);
  JH_ARG(out_rows == rows && (rows == 0 || (d_state && d_action && d_reward && d_next_state && d_done && d_priority)));
  JH_HIP(hipSetDevice(e->ctx->device));
  QArgs a{};
  a.W = e->W; a.T = T; a.S = e->S; a.H = H; a.A = A; a.N2 = N2; a.dueling = dueling ? 1 : 0; a.n = win->n;
  a.t_first = (int)(win->n > win->seen ? win->n - win->seen : 0);
  a.seen = win->seen;
  const int l2 = dueling ? 8 : 6;
  a.W1 = d_params + off[0]; a.b1 = d_params + off[1]; a.W2 = d_params + off[l2]; a.b2 = d_params + off[dueling ? 10 : 7];
  a.wa = d_params + off[12]; a.ba = d_params + off[14]; a.wv = dueling ? d_params + off[16] : nullptr; a.bv = dueling ? d_params + off[18] : nullptr;
  a.seed = win->seed; a.ctr = win->ctr; a.gamma = gamma; a.eps = d_eps;
  a.es = e->s; a.et = e->t; a.erng = e->rng;
  char* b = win->block;
  a.ws = (float*)b; b += states_bytes(win);
  a.wq = (float*)b; b += lane_bytes(win);
  a.wr = (float*)b; b += lane_bytes(win);
  a.wact = (int*)b; b += lane_bytes(win);
  a.wd = (int*)b;
  a.o_state = d_state; a.o_action = d_action; a.o_reward = d_reward; a.o_next = d_next_state; a.o_done = d_done; a.o_prio = d_priority;
  static size_t lds_allowed = 64 << 10;  // beyond 64 KB of dynamic LDS a kernel has to be told once
  if (lds > lds_allowed) {
    JH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&jh_devroll_q_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    lds_allowed = lds;
  }
  const dim3 grid((unsigned)((e->W + kRows - 1) / kRows));
  JH_LAUNCH(jh_devroll_q_kernel, grid, dim3(kThreads), lds, jh_s(stream), a);
  JH_LAUNCH_CHECK();
  win->seen += T;
  win->ctr += (uint64_t)T;
  return JH_OK;
}
