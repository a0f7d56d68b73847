// Device-resident TD3 / SAC actors: actor forward, exploration, control-env step with auto-reset and the replay row for T timesteps of W
// envs in ONE launch (DESIGN "Device-resident TD3 / SAC actors").  The actor is the ONLINE actor of a jh_acnet (TD3: last layer pi, A
// columns) or of the jh_acnet inside a jh_sacnet (SAC: the stacked [mu | log_std] layer, 2A columns), read in place from its parameter
// bucket through the object's segment offsets.
//
// Work split (the discipline of jh_devroll.hip).  One workgroup (4 waves) owns 16 env rows -- one MFMA row tile -- for the whole run.  Rows
// never interact: no grid-wide wait, no spin on memory, no float atomics; every loop is bounded by T, H, S or A, and every sum runs in an
// order fixed by k alone, so a row's output is a function of (actor weights, env state, seed, counter, env row): neither W nor the tile the
// row falls in enters.  The variant that carries TWO row tiles behind each weight fragment (half the L2 traffic per row, H <= ~600) is not
// here: a launch takes the same time at W = 32, 256 and 1024, so up to one workgroup per CU the step is bound by a workgroup's
// own latency chain, not by the L2 traffic of all of them.
//
// Per timestep, in LDS:  es [16][S] float64  ->  h1 [16][H]  ->  h2 [16][H]  ->  z [16][n_out]  ->  action [16][A]  ->  es'.
//   layers    jh_devroll_mlp.h: head.l and l on v_mfma_f32_16x16x4_f32, the column tiles split over the waves, W2 streamed from L2 in blocks of
//             eight k chunks with the next block in flight
//   tail      n_out = A | 2A <= 32 outputs = one or two column tiles of ONE weight matrix [n_out][H] (rows of H floats: 16-byte loads).  K is
//             what the waves split (chunk c goes to wave c mod 4); the partial tiles meet in LDS, in the space of h1 (dead by then), and are
//             summed in wave order, bias last.  There is no value row and no capture: z is the only thing the forward leaves
//   explore   one thread per (env row, action dimension) -- 16 x 16 = the workgroup -- on the collectors' counter-based stream keyed
//             (seed, counter + t, env row, k): jh_u01_pair_at / jh_normal_at / jh_sample_continuous_dim_at of jh_common.h.
//             TD3 (td3.py:132-144, per env row): t < n_random: 2 u2 - 1; training: clamp(tanh(z_k) + action_noise_std n, -1, 1) in double;
//             else tanh(z_k).  The uniform timesteps skip the forward unless the heads are asked for.
//             SAC (sac.py:143-159): tanh(clamp(z_k, -5, 5) + exp(tanh(z_{A+k})) n), or tanh(mu) when not training
//   env       jh_env_dyn.h, the host env's own statements: one (row, i) element per thread, then the row's thread for the action cost,
//             step count, reward, done and reset
//   rows      time-major, row = t W + env row: a tile's 16 rows of one timestep are contiguous in every column, so state, action, heads and
//             next_state go out as one contiguous run each
//
// LDS in bytes:  8 x [ 16 S (es) + S A rounded up to even (coupling) + 32 (t, rng) ]
//              + 4 x [ max(16 (H + 4), 2048) (h1 | tail partials) + 16 (H + 4) (h2) + 16 x 32 (z) + 16 x 16 (action) ]
//   at S = 64, A = 16:  16 640 + 128 H + 512 + 3 072 = 128 H + 20 224  ->  H <= 1120 inside 160 KB (163 584 of 163 840 bytes): JH_DEVROLL_AC_MAX_H.
//   h1 and h2 are live together during layer 2; the tail's partial tiles alias h1; nothing aliases h2.
#include "jh_acnet.h"
#include "jh_env_dyn.h"
#include "jh_devroll_mlp.h"

namespace {
using jh_roll::f32x4;
using jh_roll::kRows;
using jh_roll::kThreads;
using jh_roll::kWaves;

constexpr int kZLd = 32, kActLd = jh_env::kControlMaxA, kTailTiles = 2;
constexpr int kPartFloats = kWaves * kTailTiles * 4 * 64;
constexpr size_t kLdsMax = 160u << 10;
static_assert(kRows * kActLd == kThreads && kTailTiles * 16 == kZLd && 2 * jh_env::kControlMaxA <= kZLd, "one thread per (row, action dimension); two tail tiles hold 2A outputs");

struct AcArgs {
  int W, T, S, H, A, n_out, sac, training, n_random;
  double noise_std;
  const float *W1, *b1, *W2, *b2, *wo, *bo;
  uint64_t seed, ctr;
  double* es; int64_t* et; uint64_t* erng; const double* coupling;
  float *o_state, *o_action, *o_reward, *o_next; uint8_t* o_done; float* o_heads;
};

struct Lds {
  double *es, *P;
  int64_t* t;
  uint64_t* rng;
  float *h1, *h2, *z, *act;
};
__host__ __device__ constexpr size_t h1_floats(int H) { return (size_t)kRows * (H + 4) > (size_t)kPartFloats ? (size_t)kRows * (H + 4) : (size_t)kPartFloats; }
__host__ __device__ constexpr size_t table_doubles(int S, int A) { return ((size_t)S * A + 1) & ~(size_t)1; }  // even: what follows stays 16-byte aligned
__host__ __device__ constexpr size_t lds_bytes(int S, int A, int H) {
  return 8 * ((size_t)kRows * S + table_doubles(S, A) + 2 * kRows) + 4 * (h1_floats(H) + (size_t)kRows * (H + 4) + kRows * kZLd + kRows * kActLd);
}
static_assert(lds_bytes(jh_env::kControlMaxS, jh_env::kControlMaxA, JH_DEVROLL_AC_MAX_H) <= kLdsMax &&
              lds_bytes(jh_env::kControlMaxS, jh_env::kControlMaxA, JH_DEVROLL_AC_MAX_H + 16) > kLdsMax, "JH_DEVROLL_AC_MAX_H is what the carve below leaves");
__device__ inline Lds carve(char* base, int S, int A, int H) {
  Lds l;
  l.es = reinterpret_cast<double*>(base);
  l.P = l.es + (size_t)kRows * S;
  l.t = reinterpret_cast<int64_t*>(l.P + table_doubles(S, A));
  l.rng = reinterpret_cast<uint64_t*>(l.t + kRows);
  l.h1 = reinterpret_cast<float*>(l.rng + kRows);  // 16-byte aligned: every count above is even
  l.h2 = l.h1 + h1_floats(H);
  l.z = l.h2 + (size_t)kRows * (H + 4);
  l.act = l.z + kRows * kZLd;
  return l;
}

// es -> h1 -> h2 -> z, all in LDS; ends behind a workgroup barrier
__device__ void forward(const AcArgs& a, const Lds& l) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, kq = lane >> 4;
  const int H = a.H, ld = H + 4, tiles = H / 16;
  jh_roll::layer1(a.W1, a.b1, l.es, a.S, H, l.h1, ld);
  __syncthreads();
  jh_roll::layer2(a.W2, a.b2, l.h1, ld, H, tiles, l.h2, ld);
  __syncthreads();  // h2 complete; h1 is dead from here on: its space takes the tail's partial tiles
  // ---- tail: output o = 16 q + r is row o of the last layer; K split over the waves
  const int nt = (a.n_out + 15) / 16;
  float* part = l.h1;  // [wave][q][i][lane]
  {
    const float* wrow[kTailTiles];
    f32x4 acc[kTailTiles];
#pragma unroll
    for (int q = 0; q < kTailTiles; ++q) {
      wrow[q] = q * 16 + r < a.n_out ? a.wo + (size_t)(q * 16 + r) * H : nullptr;
      acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int c = wave; c < tiles; c += kWaves) {
      const int k = c * 16 + kq * 4;
      const float4 av = *reinterpret_cast<const float4*>(l.h2 + r * ld + k);
#pragma unroll
      for (int q = 0; q < kTailTiles; ++q) {
        if (q < nt) {  // (uniform)
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
  for (int e = threadIdx.x; e < kRows * a.n_out; e += kThreads) {
    const int row = e / a.n_out, o = e - row * a.n_out, q = o >> 4;
    const int src = (row >> 2) * 16 + (o & 15), i = row & 3;  // the 16x16 C / D map: row 4 kq + i sits in register i of lane 16 kq + column
    auto p = [&](int w) { return part[((w * kTailTiles + q) * 4 + i) * 64 + src]; };
    l.z[row * kZLd + o] = (((p(0) + p(1)) + p(2)) + p(3)) + a.bo[o];
  }
  __syncthreads();
}

// td3.py:132-144 for one (env row, action dimension)
__device__ inline float td3_action(const AcArgs& a, bool uniform, float zk, uint64_t ctr, int w, int k) {
  if (uniform) {
    double u1, u2;
    jh_u01_pair_at(a.seed, ctr, w, k, &u1, &u2);
    return (float)(2.0 * u2 - 1.0);
  }
  const float pi = tanhf(zk);
  if (!a.training) return pi;
  const double v = (double)pi + a.noise_std * jh_normal_at(a.seed, ctr, w, k);
  return (float)fmin(fmax(v, -1.0), 1.0);
}

__global__ void __launch_bounds__(kThreads) jh_devroll_ac_kernel(AcArgs a) {
  extern __shared__ __attribute__((aligned(16))) char s_dyn[];
  const int S = a.S, A = a.A, tid = threadIdx.x;
  const Lds l = carve(s_dyn, S, A, a.H);
  const int w0 = (int)blockIdx.x * kRows;
  const int rows = a.W - w0 < kRows ? a.W - w0 : kRows;  // >= 1 by the grid
  for (int e = tid; e < kRows * S; e += kThreads) l.es[e] = e < rows * S ? a.es[(size_t)w0 * S + e] : 0.0;
  for (int e = tid; e < S * A; e += kThreads) l.P[e] = a.coupling[e];
  if (tid < rows) { l.t[tid] = a.et[w0 + tid]; l.rng[tid] = a.erng[w0 + tid]; }
  __syncthreads();
  const bool mine = tid < rows;  // this thread carries env row w0 + tid through action cost, bookkeeping and reset
  const int arow = tid / A, ak = tid - arow * A;  // ... and action dimension ak of env row w0 + arow, while arow < rows
  for (int t = 0; t < a.T; ++t) {
    const size_t rb = (size_t)t * a.W + w0;  // the tile's first row of this timestep: its `rows` rows are contiguous in every column
    const bool uniform = a.training && t < a.n_random;
    for (int e = tid; e < rows * S; e += kThreads) a.o_state[rb * S + e] = (float)l.es[e];
    if (!uniform || a.o_heads) forward(a, l);  // (uniform over the grid)
    if (a.o_heads)
      for (int e = tid; e < rows * a.n_out; e += kThreads) a.o_heads[rb * a.n_out + e] = l.z[(e / a.n_out) * kZLd + e % a.n_out];
    if (arow < rows) {
      const float* z = l.z + arow * kZLd;
      const uint64_t ctr = a.ctr + (uint64_t)t;
      const float ac = a.sac ? jh_sample_continuous_dim_at(A, a.seed, ctr, z, w0 + arow, ak, a.training) : td3_action(a, uniform, uniform ? 0.f : z[ak], ctr, w0 + arow, ak);
      l.act[arow * kActLd + ak] = ac;
      a.o_action[rb * A + tid] = ac;
    }
    __syncthreads();  // the actions are in LDS, and every thread has read the state it stores
    // ---- the env step
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
    const double a2 = mine ? jh_env::control_action_cost(l.act + tid * kActLd, A) : 0.0;
    __syncthreads();  // every element has read the old state
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int e = tid + u * kThreads;
      if (e < rows * S) {
        l.es[e] = nx[u];
        a.o_next[rb * S + e] = (float)nx[u];  // the terminal observation where done
      }
    }
    __syncthreads();
    if (mine) {
      double* s = l.es + tid * S;
      l.t[tid] += 1;
      const bool d = jh_env::control_done(s[0], l.t[tid]);
      a.o_done[rb + tid] = d ? 1 : 0;
      a.o_reward[rb + tid] = jh_env::control_reward(s[0], a2);
      if (d) jh_env::reset_row(s, S, l.rng[tid], l.t[tid]);
    }
    __syncthreads();
  }
  for (int e = tid; e < rows * S; e += kThreads) a.es[(size_t)w0 * S + e] = l.es[e];
  if (mine) { a.et[w0 + tid] = l.t[tid]; a.erng[w0 + tid] = l.rng[tid]; }
}
}  // namespace

// The launcher behind jh_acnet_devroll_run (jh_td3.hip) and jh_sacnet_devroll_run (jh_sac.hip).  sac: the last layer is [mu | log_std], 2A wide.
int ac_devroll_run(const char* who, jh_acnet* n, int sac, jh_devenv* e, int32_t T, int32_t training, int32_t n_random, double action_noise_std, uint64_t seed,
                   uint64_t counter, float* d_state, float* d_action, float* d_reward, float* d_next_state, uint8_t* d_done, float* d_heads, hipStream_t st) {
  JH_ARG(n && e && T > 0 && n_random >= 0 && d_state && d_action && d_reward && d_next_state && d_done);
  JH_ARG(e->kind == JH_DEVENV_CONTROL && n->core.ctx == e->ctx && n->S == e->S && n->A == e->A);
  JH_ARG(n->ap && n->nc >= 1 && n->seg_rows[AC_A_WPI] == (sac ? 2 * n->A : n->A) && n->seg_cols[AC_A_WPI] == n->H);
  const size_t lds = lds_bytes(e->S, e->A, n->H);
  if (n->H % 16 != 0 || n->H > JH_DEVROLL_AC_MAX_H || lds > kLdsMax)
    return jh_fail(JH_ERR_ARG, "%s: hidden_size %d: the actor kernel keeps both activation tiles of a 16-row workgroup in LDS and serves hidden_size %% 16 == 0 up to %d",
                   who, n->H, JH_DEVROLL_AC_MAX_H);
  JH_HIP(hipSetDevice(e->ctx->device));
  AcArgs a{};
  a.W = e->W; a.T = T; a.S = e->S; a.H = n->H; a.A = e->A; a.n_out = n->seg_rows[AC_A_WPI]; a.sac = sac ? 1 : 0; a.training = training ? 1 : 0;
  a.n_random = sac ? 0 : n_random; a.noise_std = action_noise_std;
  const float* p = n->ap;
  a.W1 = p + n->seg_off[AC_A_W1]; a.b1 = p + n->seg_off[AC_A_B1]; a.W2 = p + n->seg_off[AC_A_WL]; a.b2 = p + n->seg_off[AC_A_BL];
  a.wo = p + n->seg_off[AC_A_WPI]; a.bo = p + n->seg_off[AC_A_BPI];
  a.seed = seed; a.ctr = counter;
  a.es = e->s; a.et = e->t; a.erng = e->rng; a.coupling = e->coupling;
  a.o_state = d_state; a.o_action = d_action; a.o_reward = d_reward; a.o_next = d_next_state; a.o_done = d_done; a.o_heads = d_heads;
  static size_t lds_allowed = 64 << 10;  // beyond 64 KB of dynamic LDS a kernel has to be told once
  if (lds > lds_allowed) {
    JH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&jh_devroll_ac_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    lds_allowed = lds;
  }
  const dim3 grid((unsigned)((e->W + kRows - 1) / kRows));
  JH_LAUNCH(jh_devroll_ac_kernel, grid, dim3(kThreads), lds, st, a);
  JH_LAUNCH_CHECK();
  return JH_OK;
}
