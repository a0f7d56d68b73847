// Device-resident actors of the discrete off-policy agents that fill a plain replay buffer -- the discrete SAC (actor: kind pi) and DQN /
// Double (discrete_q_network: kind q): forward, the decision, CartPole step with auto-reset and the replay row for T timesteps of W envs in
// ONE launch (DESIGN "Device-resident discrete SAC / DQN actors").  The network is a jh_rbnet of kind q on the mlp head,
// head.l (S -> H, relu) -> l (H -> H, relu) -> out (H -> A), read in place from the learner's parameter bucket through the object's
// segment offsets.
//
// Work split (the discipline of jh_devroll.hip).  One workgroup (4 waves) owns 16 env rows -- one MFMA row tile -- for the whole run.  Rows
// never interact: no grid-wide wait, no spin on memory, no float atomics; every loop is bounded by T, H, S or A, and every sum runs in an
// order fixed by k alone, so a row's output is a function of (weights, env state, seed, counter, env row): neither W nor the tile the row
// falls in enters.
//
// Per timestep, in LDS:  es [16][S] float64  ->  h1 [16][H]  ->  h2 [16][H]  ->  logits [16][A]  ->  action  ->  es'.
//   layers    jh_devroll_mlp.h: head.l and l on v_mfma_f32_16x16x4_f32, the column tiles split over the waves
//   tail      A <= 64 outputs = up to FOUR 16-column tiles of out [A][H] (rows of H floats: 16-byte loads).  K is what the waves split (chunk c
//             goes to wave c mod 4): a wave reads its activation fragment once per chunk and feeds every column tile from it, the weight
//             pieces of its NEXT chunk in flight during the MFMAs.  The partial tiles meet in LDS, in the space of h1 (dead by then), and are
//             summed in wave order, bias last
//   decide    a row's logits are owned by a group of G = 2 .. 64 lanes (the power of two that holds A), 256 / G rows at a time.  The first
//             index of the largest float32 logit is a butterfly over (value, index).
//             mode pi (sac.py:151-159), training: p_k = exp(z_k - max) in double, the inclusive prefix a scan over the group, total = its
//             last element; u = the collectors' counter-based uniform at key = seed * FNV + (counter + t) * golden + env row; the action is
//             the first index whose prefix exceeds u * total (a ballot over the group).  Not training: the first largest logit.
//             mode q (dqn.py:100-113, per env row): u1, u2 at keys 2 key + 1, 2 key + 2; u1 < epsilon: floor(u2 * A); else the first largest q
//   env       jh_env_dyn.h, the host env's own statements, by the row's thread
//   rows      time-major, row = t W + env row: a tile's rows of one timestep are contiguous in every column
// The probe (JH_DEVROLL_DISC_PROBE) leaves the env where it is: logits and actions only, for networks wider than the env's action set.
//
// LDS in bytes:  8 x [ 16 S (es) + 32 (t, rng) ]  +  4 x [ max(16 (H + 4), 4096) (h1 | tail partials) + 16 (H + 4) (h2) + 16 x 64 (logits)
//   + 16 (action) ]   at S = 4:  128 H + 5 440  ->  H <= 1232 inside 160 KB (163 136 of 163 840 bytes): JH_DEVROLL_DISC_MAX_H.
//   h1 and h2 are live together during layer 2; the tail's partial tiles alias h1; nothing aliases h2.
#include "jh_common.h"
#include "jh_env_dyn.h"
#include "jh_devroll_mlp.h"

namespace {
using jh_roll::f32x4;
using jh_roll::kRows;
using jh_roll::kThreads;
using jh_roll::kWaves;

constexpr int kMaxA = 64, kZLd = kMaxA, kTailTiles = kMaxA / 16, kCartS = 4;
constexpr int kPartFloats = kWaves * kTailTiles * 4 * 64;
constexpr size_t kLdsMax = 160u << 10;
constexpr int kModePi = 0, kModeQ = 1;

struct DArgs {
  int W, T, S, H, A, G, mode, training, probe;
  double eps;
  const float *W1, *b1, *W2, *b2, *wo, *bo;
  uint64_t seed, ctr;
  double* es; int64_t* et; uint64_t* erng;
  float* o_state; int64_t* o_action; float* o_reward; float* o_next; uint8_t* o_done; float* o_heads;
};

struct Lds {
  double* es;
  int64_t* t;
  uint64_t* rng;
  float *h1, *h2, *z;
  int* act;
};
__host__ __device__ constexpr size_t h1_floats(int H) { return (size_t)kRows * (H + 4) > (size_t)kPartFloats ? (size_t)kRows * (H + 4) : (size_t)kPartFloats; }
__host__ __device__ constexpr size_t lds_bytes(int S, int H) {
  return 8 * ((size_t)kRows * S + 2 * kRows) + 4 * (h1_floats(H) + (size_t)kRows * (H + 4) + kRows * kZLd + kRows);
}
static_assert(lds_bytes(kCartS, JH_DEVROLL_DISC_MAX_H) <= kLdsMax && lds_bytes(kCartS, JH_DEVROLL_DISC_MAX_H + 16) > kLdsMax,
              "JH_DEVROLL_DISC_MAX_H is what the carve below leaves");
__device__ inline Lds carve(char* base, int S, int H) {
  Lds l;
  l.es = reinterpret_cast<double*>(base);
  l.t = reinterpret_cast<int64_t*>(l.es + (size_t)kRows * S);
  l.rng = reinterpret_cast<uint64_t*>(l.t + kRows);
  l.h1 = reinterpret_cast<float*>(l.rng + kRows);  // 16-byte aligned: every count above is even
  l.h2 = l.h1 + h1_floats(H);
  l.z = l.h2 + (size_t)kRows * (H + 4);
  l.act = reinterpret_cast<int*>(l.z + kRows * kZLd);
  return l;
}

// es -> h1 -> h2 -> z, all in LDS; ends behind a workgroup barrier
__device__ void forward(const DArgs& a, const Lds& l) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, kq = lane >> 4;
  const int H = a.H, A = a.A, ld = H + 4, tiles = H / 16;
  jh_roll::layer1(a.W1, a.b1, l.es, a.S, H, l.h1, ld);
  __syncthreads();
  jh_roll::layer2(a.W2, a.b2, l.h1, ld, H, tiles, l.h2, ld);
  __syncthreads();  // h2 complete; h1 is dead from here on: its space takes the tail's partial tiles
  // ---- tail: output o = 16 q + r is row o of the last layer; K split over the waves, every column tile behind one activation fragment
  const int nt = (A + 15) / 16;
  float* part = l.h1;  // [wave][q][i][lane]
  {
    const float* wrow[kTailTiles];
    f32x4 acc[kTailTiles];
    float4 cur[kTailTiles], nxt[kTailTiles];
#pragma unroll
    for (int q = 0; q < kTailTiles; ++q) {
      wrow[q] = q * 16 + r < A ? a.wo + (size_t)(q * 16 + r) * H + kq * 4 : nullptr;
      acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    auto fetch = [&](int c, float4* dst) {  // (segments and rows of H floats: 16-byte aligned)
#pragma unroll
      for (int q = 0; q < kTailTiles; ++q) dst[q] = (wrow[q] && c < tiles) ? *reinterpret_cast<const float4*>(wrow[q] + c * 16) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    fetch(wave, cur);
    for (int c = wave; c < tiles; c += kWaves) {
      fetch(c + kWaves, nxt);
      const float4 av = *reinterpret_cast<const float4*>(l.h2 + r * ld + c * 16 + kq * 4);
#pragma unroll
      for (int q = 0; q < kTailTiles; ++q) {
        if (q < nt) {  // (uniform)
          acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, cur[q].x, acc[q], 0, 0, 0);
          acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, cur[q].y, acc[q], 0, 0, 0);
          acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, cur[q].z, acc[q], 0, 0, 0);
          acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, cur[q].w, acc[q], 0, 0, 0);
        }
        cur[q] = nxt[q];
      }
    }
#pragma unroll
    for (int q = 0; q < kTailTiles; ++q)
      if (q < nt)
#pragma unroll
        for (int i = 0; i < 4; ++i) part[((wave * kTailTiles + q) * 4 + i) * 64 + lane] = acc[q][i];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < kRows * A; e += kThreads) {
    const int row = e / A, o = e - row * A, q = o >> 4;
    const int src = (row >> 2) * 16 + (o & 15), i = row & 3;  // the 16x16 C / D map: row 4 kq + i sits in register i of lane 16 kq + column
    auto p = [&](int w) { return part[((w * kTailTiles + q) * 4 + i) * 64 + src]; };
    l.z[row * kZLd + o] = (((p(0) + p(1)) + p(2)) + p(3)) + a.bo[o];
  }
  __syncthreads();
}

// The decision of every row of the tile at timestep t: lane k of a group of G lanes holds logit k of the group's row.  Every lane of a wave
// takes every cross-lane step (the loops are uniform); only a live row's first lane writes
__device__ void decide(const DArgs& a, const Lds& l, int t, int w0, int rows, size_t rb) {
  const int G = a.G, A = a.A, per = kThreads / G;
  const int g = threadIdx.x / G, k = threadIdx.x - g * G;
  for (int base = 0; base < kRows; base += per) {
    const int row = base + g;
    const bool live = row < kRows && k < A;
    const float z = live ? l.z[row * kZLd + k] : -INFINITY;
    float bz = z;
    int bi = k;
    for (int d = 1; d < G; d <<= 1) {  // the first index of the largest float32 value
      const float oz = __shfl_xor(bz, d, G);
      const int oi = __shfl_xor(bi, d, G);
      if (oz > bz || (oz == bz && oi < bi)) { bz = oz; bi = oi; }
    }
    int act = bi;
    const uint64_t key = a.seed * 0x100000001B3ull + (a.ctr + (uint64_t)t) * 0x9E3779B97F4A7C15ull + (uint64_t)(w0 + row);
    if (a.mode == kModeQ) {
      if (jh_u01_of(key * 2 + 1) < a.eps) act = (int)(jh_u01_of(key * 2 + 2) * (double)A);
    } else if (a.training) {
      double c = live ? exp((double)z - (double)bz) : 0.0;
      for (int d = 1; d < G; d <<= 1) {  // inclusive prefix over the group
        const double up = __shfl_up(c, d, G);
        if (k >= d) c += up;
      }
      const double total = __shfl(c, G - 1, G);
      const unsigned long long over = __ballot(live && c > jh_u01_of(key) * total);
      const unsigned long long mine = (over >> ((threadIdx.x & 63) - k)) & (G == 64 ? ~0ull : (1ull << G) - 1);
      act = mine ? __ffsll((long long)mine) - 1 : A - 1;
    }
    act = act < A ? act : A - 1;
    if (k == 0 && row < rows) {
      l.act[row] = act;
      a.o_action[rb + row] = act;
    }
  }
}

__global__ void __launch_bounds__(kThreads) jh_devroll_disc_kernel(DArgs a) {
  extern __shared__ __attribute__((aligned(16))) char s_dyn[];
  const int S = a.S, A = a.A, tid = threadIdx.x;
  const Lds l = carve(s_dyn, S, a.H);
  const int w0 = (int)blockIdx.x * kRows;
  const int rows = a.W - w0 < kRows ? a.W - w0 : kRows;  // >= 1 by the grid
  for (int e = tid; e < kRows * S; e += kThreads) l.es[e] = e < rows * S ? a.es[(size_t)w0 * S + e] : 0.0;
  if (tid < rows) { l.t[tid] = a.et[w0 + tid]; l.rng[tid] = a.erng[w0 + tid]; }
  __syncthreads();
  const bool mine = tid < rows && !a.probe;  // this thread carries env row w0 + tid through env step and reset
  for (int t = 0; t < a.T; ++t) {
    const size_t rb = (size_t)t * a.W + w0;  // the tile's first row of this timestep: its `rows` rows are contiguous in every column
    if (!a.probe)
      for (int e = tid; e < rows * S; e += kThreads) a.o_state[rb * S + e] = (float)l.es[e];
    forward(a, l);
    if (a.o_heads)
      for (int e = tid; e < rows * A; e += kThreads) a.o_heads[rb * A + e] = l.z[(e / A) * kZLd + e % A];
    decide(a, l, t, w0, rows, rb);
    __syncthreads();  // the actions are in LDS, and every thread has read the state it stores
    if (mine) {
      double* s = l.es + tid * S;
      const bool d = jh_env::cartpole_advance(s, l.t[tid], l.act[tid]);
      for (int k = 0; k < S; ++k) a.o_next[(rb + tid) * S + k] = (float)s[k];  // the terminal observation where done
      a.o_done[rb + tid] = d ? 1 : 0;
      a.o_reward[rb + tid] = d ? jh_env::kRewardDone : jh_env::kRewardStep;
      if (d) jh_env::reset_row(s, S, l.rng[tid], l.t[tid]);
    }
    __syncthreads();
  }
  if (a.probe) return;
  for (int e = tid; e < rows * S; e += kThreads) a.es[(size_t)w0 * S + e] = l.es[e];
  if (mine) { a.et[w0 + tid] = l.t[tid]; a.erng[w0 + tid] = l.rng[tid]; }
}
}  // namespace

// T timesteps of all W envs in one launch; the W * T rows go time-major into the caller's device columns, which the caller appends
// (jh_store_push_device), so the ring's bookkeeping exists once.  seed / counter are the caller's (counter + T for the next run).
JH_EXPORT int jh_devroll_disc_run(jh_rbnet* net, const float* d_params, jh_devenv* e, int32_t T, int32_t mode, int32_t training, double epsilon, uint64_t seed,
                                  uint64_t counter, float* d_state, int64_t* d_action, float* d_reward, float* d_next_state, uint8_t* d_done, float* d_heads,
                                  int32_t flags, jh_stream stream) {
  const bool probe = (flags & JH_DEVROLL_DISC_PROBE) != 0;
  JH_ARG(net && d_params && e && T > 0 && (mode == JH_DEVROLL_DISC_PI || mode == JH_DEVROLL_DISC_Q) && (flags & ~JH_DEVROLL_DISC_PROBE) == 0);
  JH_ARG(d_action && (probe ? d_heads != nullptr : (d_state && d_reward && d_next_state && d_done)));
  JH_ARG(e->kind == JH_DEVENV_CARTPOLE && e->S == kCartS);
  // the network's shape from its segment table: 0 head.l [H][S], 6 l [H][H], 12 out [A][H]; nothing else (no cnn head, no stream layers, no noise)
  int64_t off[20];
  int32_t sr[20], sc[20];
  for (int i = 0; i < 20; ++i)
    if (int rc = jh_rbnet_segment(net, i, &off[i], &sr[i], &sc[i])) return rc;
  const int H = sr[0], A = sr[12];
  const bool mlp = sr[2] == 0 && sr[4] == 0, plain = sr[8] == 0 && sr[9] == 0 && sr[13] == 0 && sr[16] == 0 && sr[17] == 0;
  if (!mlp || !plain || sc[0] != e->S || sr[6] != H || sc[6] != H || sc[12] != H || A < 2 || A > kMaxA || (!probe && A != e->A))
    return jh_fail(JH_ERR_ARG, "jh_devroll_disc_run: bad argument: the network must be head.l -> l -> %d outputs on the mlp head, %d -> %d like the env", A, e->S, e->A);
  const size_t lds = lds_bytes(e->S, H);
  if (H % 16 != 0 || H > JH_DEVROLL_DISC_MAX_H || lds > kLdsMax)
    return jh_fail(JH_ERR_ARG, "jh_devroll_disc_run: bad argument: hidden_size %d: the actor kernel keeps both activation tiles of a 16-row workgroup in LDS and serves "
                   "hidden_size %% 16 == 0 up to %d", H, JH_DEVROLL_DISC_MAX_H);
  JH_HIP(hipSetDevice(e->ctx->device));
  DArgs a{};
  a.W = e->W; a.T = T; a.S = e->S; a.H = H; a.A = A; a.mode = mode == JH_DEVROLL_DISC_Q ? kModeQ : kModePi; a.training = training ? 1 : 0; a.probe = probe ? 1 : 0;
  a.G = 2;
  while (a.G < A) a.G <<= 1;
  a.eps = epsilon;
  a.W1 = d_params + off[0]; a.b1 = d_params + off[1]; a.W2 = d_params + off[6]; a.b2 = d_params + off[7]; a.wo = d_params + off[12]; a.bo = d_params + off[14];
  a.seed = seed; a.ctr = counter;
  a.es = e->s; a.et = e->t; a.erng = e->rng;
  a.o_state = d_state; a.o_action = d_action; a.o_reward = d_reward; a.o_next = d_next_state; a.o_done = d_done; a.o_heads = d_heads;
  static size_t lds_allowed = 64 << 10;  // beyond 64 KB of dynamic LDS a kernel has to be told once
  if (lds > lds_allowed) {
    JH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&jh_devroll_disc_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    lds_allowed = lds;
  }
  const dim3 grid((unsigned)((e->W + kRows - 1) / kRows));
  JH_LAUNCH(jh_devroll_disc_kernel, grid, dim3(kThreads), lds, jh_s(stream), a);
  JH_LAUNCH_CHECK();
  return JH_OK;
}
