// SAC, discrete actions (core/agent/sac.py:192-269, the `else` branches): what one learn() does between the networks' forwards and
// backwards, as two launches.
//   jh_sacd_critic_loss   pi' = softmax(actor(s')), next_q_i = sum_a pi' Q_i'(s'), H' = Categorical(pi').entropy(),
//                         y = r + (1 - d) gamma (min(next_q1, next_q2) + alpha H') -- the minimum of the two EXPECTATIONS --,
//                         both MSE losses, max_Q = max_b y, dQ1 / dQ2 [B][A] (zero except at the taken action)          (sac.py:193-217)
//   jh_sacd_actor_loss    pi = softmax(actor(s)), q_i = sum_a pi Q_i(s) of the critics AFTER their step, H as above,
//                         actor_loss = -mean(alpha H + min(q1, q2)) and its gradient with respect to the RAW logits (through H, through
//                         the smaller expectation -- half each on a tie, torch.min's backward -- and the softmax Jacobian),
//                         alpha_loss = log_alpha mean(H - target_entropy), mean_Q, mean entropy; then the temperature's
//                         bookkeeping: alpha <- exp(log_alpha), and, dynamic, Adam on log_alpha                          (sac.py:235-255)
// Work split: a row of A logits is owned by a GROUP of G lanes, G the smallest power of two >= A (2 .. 64), lane j holding action j; the
// row's maximum, sum-exp, expectations and entropy are butterflies over xor offsets G/2 .. 1, which stay inside the aligned group.  A
// workgroup of 256 lanes takes 256 / G rows and the grid as many workgroups as the batch needs (256 at B = 1024, A = 64).  A lane reads
// its own logit and Q values once, straight from global memory (consecutive lanes, consecutive floats: every element has one reader, LDS
// would only copy it); LDS holds the reductions' wave partials alone.
// Batch sums: lane 0 of a group contributes its row's terms, the workgroup sums them (shuffle tree, then the waves in order: jh_mult.h's
// block_sums) and publishes ONE partial; the last workgroup to arrive (an integer ticket, no floating-point atomics) adds the partials --
// thread t takes partial t, the same tree -- and writes the statistics.  The order of every addition is fixed by the grid alone: an eager
// run, a second run and a hipGraph replay give the same bits.  The ticket returns to zero for the next launch.
// The temperature block is the MPO family's multiplier block (jh_mult.h): slot 0 = log_alpha (floor -inf, VB_EPS = target_entropy) with
// its Adam moments, slot 1's value = the alpha IN USE (sac.py:250 refreshes it after the actor step and Adam moves log_alpha after that:
// the alpha of learn k is exp(log_alpha) after k - 1 steps).  The step is jh_mult.h's multiplier_step with the temperature's OWN hyper
// block (alpha_lr, betas, eps, step count), which this kernel advances.
// Categorical (torch.distributions): log p inside the entropy is log(clamp(p, eps, 1 - eps)) with float32 eps; here that is the
// log-softmax clamped to [log eps, log(1 - eps)] -- the same value wherever float32 p is a normal number, finite where it underflows --
// and its derivative is zero where the clamp binds, as the reference's.  Per-row terms are evaluated in double and rounded once.
#include "jh_common.h"
#include "jh_mult.h"
#include "jh_policy_head.h"  // action_index

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kMaxRows = 1024, kMaxActions = 64;
constexpr int kMaxGrid = kMaxRows / (kThreads / kMaxActions);  // 256 workgroups: one partial per thread of the last one
// the caller's workspace: [0] the ticket, then from float 8 (32 bytes in) kMaxGrid x 4 doubles of partial sums, then kMaxGrid floats of partial maxima
constexpr int kWorkSums = 8, kWorkMax = kWorkSums + kMaxGrid * 4 * 2, kWorkFloats = kWorkMax + kMaxGrid;
static_assert(kWorkFloats <= JH_SACD_WORK_FLOATS, "the workspace of include/jorldy_hip.h");
static_assert(kMaxGrid <= kThreads, "one partial per thread of the last workgroup");

constexpr double kEps = 1.1920928955078125e-07;  // float32 eps = 2^-23: what Categorical clamps its probabilities with

__device__ __forceinline__ int group_lanes(int A) {
  int G = 2;
  while (G < A) G <<= 1;
  return G;
}
__device__ __forceinline__ double group_sum(double v, int G) {
  for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float group_max(float v, int G) {
  for (int o = G >> 1; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// One lane's share of a categorical row: p = softmax(z)[j], lc = clamp(log-softmax, log eps, log(1 - eps)), `free` = the clamp does not
// bind; H = the row's entropy -sum p lc, on every lane of the group.  A padded lane (j >= A) or a lane of a row past the batch holds p = 0.
struct CatLane { double p, lc, H; bool free; };
__device__ __forceinline__ CatLane cat_lane(float z, bool on, int G) {
  const float zm = group_max(on ? z : -INFINITY, G);  // rows past the batch: -inf, never used
  const double e = on ? exp((double)z - (double)zm) : 0.0;
  const double se = group_sum(e, G);
  CatLane c;
  const double kLogEps = log(kEps), kLogOneMinusEps = log1p(-kEps);
  const double lp = on ? ((double)z - (double)zm) - log(se) : 0.0;
  c.p = on ? exp(lp) : 0.0;
  c.free = lp >= kLogEps && lp <= kLogOneMinusEps;
  c.lc = lp < kLogEps ? kLogEps : (lp > kLogOneMinusEps ? kLogOneMinusEps : lp);
  c.H = -group_sum(c.p * c.lc, G);
  return c;
}

// The workgroup's N sums -> its partial; the last workgroup to arrive gets every workgroup's, summed in workgroup order, back in v
// (all threads), the others leave.  mx: a maximum finished the same way (exact).  -> is this the last workgroup
template <int N>
__device__ __forceinline__ bool finish_sums(double (&v)[N], float& mx, float* work, double (*s_red)[8], float* s_redf, int* s_last) {
  static_assert(N <= 4, "four doubles of partial sums per workgroup");
  unsigned* ticket = reinterpret_cast<unsigned*>(work);
  double* part = reinterpret_cast<double*>(work + kWorkSums);
  float* part_mx = work + kWorkMax;
  block_sums<N>(v, s_red);
  mx = jh_block_reduce(mx, s_redf, JhMax(), -INFINITY);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) __hip_atomic_store(part + 4 * blockIdx.x + k, v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(part_mx + blockIdx.x, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *s_last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u;
  }
  __syncthreads();
  if (!*s_last) return false;
  const int t = threadIdx.x;
  const bool has = t < (int)gridDim.x;
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = has ? __hip_atomic_load(part + 4 * t + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
  mx = has ? __hip_atomic_load(part_mx + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : -INFINITY;
  block_sums<N>(v, s_red);
  mx = jh_block_reduce(mx, s_redf, JhMax(), -INFINITY);
  if (t == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}

struct CriticArgs {
  int B, A;
  const float *la_next, *qt1, *qt2, *q1, *q2;  // [B][A]
  const float *action, *reward, *done;         // [B]
  const float* blk;                            // the temperature block: only read here
  float gamma;
  float *g_q1, *g_q2;  // [B][A]
  float* stats;        // [0..3): critic_loss1, critic_loss2, max_Q
  float* work;
};

__global__ void __launch_bounds__(kThreads) jh_sacd_critic_kernel(CriticArgs a) {
  __shared__ double s_red[kWaves][8];
  __shared__ float s_redf[16];
  __shared__ int s_last;
  const int A = a.A, B = a.B, G = group_lanes(A);
  const int j = (int)threadIdx.x & (G - 1), row = (int)blockIdx.x * (kThreads / G) + (int)threadIdx.x / G;
  const bool on = row < B && j < A;
  const size_t o = (size_t)row * A + j;  // only dereferenced when `on`
  const float alpha = a.blk[VB_VAL + 1];

  const CatLane c = cat_lane(on ? a.la_next[o] : 0.f, on, G);
  const double nq1 = group_sum(on ? c.p * (double)a.qt1[o] : 0.0, G);
  const double nq2 = group_sum(on ? c.p * (double)a.qt2[o] : 0.0, G);
  double d1 = 0.0, d2 = 0.0;
  float yf = -INFINITY;
  if (row < B) {  // every lane of the group: the same y, each writes its own gradient entry
    const double mn = nq2 < nq1 ? nq2 : nq1;
    const double y = (double)a.reward[row] + (1.0 - (double)a.done[row]) * (double)a.gamma * (mn + (double)alpha * c.H);
    const int ak = action_index(a.action[row], A);
    if (on) {
      const bool taken = j == ak;
      const double e1 = taken ? (double)a.q1[o] - y : 0.0, e2 = taken ? (double)a.q2[o] - y : 0.0;
      a.g_q1[o] = (float)(2.0 * e1 / (double)B);
      a.g_q2[o] = (float)(2.0 * e2 / (double)B);
      d1 = e1 * e1;  // the taken lane alone is non-zero: the group's contribution sits on one lane
      d2 = e2 * e2;
      if (taken) yf = (float)y;
    }
  }
  double s[2] = {d1, d2};
  if (!finish_sums<2>(s, yf, a.work, s_red, s_redf, &s_last) || threadIdx.x != 0) return;
  a.stats[0] = (float)(s[0] / (double)B);
  a.stats[1] = (float)(s[1] / (double)B);
  a.stats[2] = yf;
}

struct ActorArgs {
  int B, A, dynamic;
  const float *la, *q1, *q2;  // [B][A]
  float* blk;                 // the temperature block
  float* hyper;               // the temperature's own Adam block (JH_HY_*): the step count is advanced here
  float* g_la;                // [B][A]
  float* stats;               // [3..8): actor_loss, alpha_loss, mean_Q, alpha, entropy
  float* work;
};

__global__ void __launch_bounds__(kThreads) jh_sacd_actor_kernel(ActorArgs a) {
  __shared__ double s_red[kWaves][8];
  __shared__ float s_redf[16];
  __shared__ int s_last;
  const int A = a.A, B = a.B, G = group_lanes(A);
  const int j = (int)threadIdx.x & (G - 1), row = (int)blockIdx.x * (kThreads / G) + (int)threadIdx.x / G;
  const bool on = row < B && j < A;
  const size_t o = (size_t)row * A + j;  // only dereferenced when `on`
  const double alpha = (double)a.blk[VB_VAL + 1];  // read before the last workgroup's thread 0 can refresh it: that happens after every ticket

  const CatLane c = cat_lane(on ? a.la[o] : 0.f, on, G);
  const double Q1 = on ? (double)a.q1[o] : 0.0, Q2 = on ? (double)a.q2[o] : 0.0;
  const double e1 = group_sum(c.p * Q1, G), e2 = group_sum(c.p * Q2, G);
  const double w1 = e1 < e2 ? 1.0 : (e2 < e1 ? 0.0 : 0.5);  // torch.min's backward: all to the smaller, half each on a tie
  // d(alpha H + min q)/d(p_j), then through the softmax: dz_j = p_j (g_j - sum_k p_k g_k); the loss is minus the batch mean
  const double g = on ? -alpha * (c.lc + (c.free ? 1.0 : 0.0)) + w1 * Q1 + (1.0 - w1) * Q2 : 0.0;
  const double gbar = group_sum(c.p * g, G);
  if (on) a.g_la[o] = (float)(-(c.p * (g - gbar)) / (double)B);
  const bool lead = row < B && j == 0;
  const double mn = e2 < e1 ? e2 : e1;
  double s[3] = {lead ? alpha * c.H + mn : 0.0, lead ? c.H : 0.0, lead ? mn : 0.0};
  float unused = -INFINITY;
  if (!finish_sums<3>(s, unused, a.work, s_red, s_redf, &s_last) || threadIdx.x != 0) return;
  const double n = (double)B;
  const float la = a.blk[VB_VAL], te = a.blk[VB_EPS];
  const float grad = (float)(s[1] / n - (double)te);  // d(alpha_loss)/d(log_alpha) = mean(H - target_entropy)
  const float fresh = (float)exp((double)la);         // sac.py:250, before log_alpha moves
  a.blk[VB_VAL + 1] = fresh;
  if (a.dynamic) {
    const float t = a.hyper[JH_HY_STEP] + 1.f;
    multiplier_step(a.blk, 0, grad, a.hyper, t);
    a.hyper[JH_HY_STEP] = t;
  }
  a.stats[3] = (float)(-s[0] / n);
  a.stats[4] = (float)((double)la * (s[1] / n - (double)te));
  a.stats[5] = (float)(s[2] / n);
  a.stats[6] = fresh;
  a.stats[7] = (float)(s[1] / n);
}

inline int sacd_grid(int B, int A) {
  int G = 2;
  while (G < A) G <<= 1;
  const int rows = kThreads / G;
  return (B + rows - 1) / rows;
}

}  // namespace

JH_EXPORT int jh_sacd_critic_loss(jh_ctx* ctx, int32_t B, int32_t A, const float* d_la_next, const float* d_qt1_next, const float* d_qt2_next, const float* d_q1,
                                  const float* d_q2, const float* d_action, const float* d_reward, const float* d_done, float gamma, const float* d_block,
                                  float* d_grad_q1, float* d_grad_q2, float* d_stats, float* d_work, jh_stream stream) {
  JH_ARG(ctx && d_la_next && d_qt1_next && d_qt2_next && d_q1 && d_q2 && d_action && d_reward && d_done && d_block && d_grad_q1 && d_grad_q2 && d_stats && d_work);
  JH_ARG(B >= 1 && B <= kMaxRows && A >= 2 && A <= kMaxActions);
  JH_ARG(((uintptr_t)d_work & 7) == 0);
  CriticArgs a{B, A, d_la_next, d_qt1_next, d_qt2_next, d_q1, d_q2, d_action, d_reward, d_done, d_block, gamma, d_grad_q1, d_grad_q2, d_stats, d_work};
  JH_LAUNCH(jh_sacd_critic_kernel, dim3(sacd_grid(B, A)), dim3(kThreads), 0, jh_s(stream), a);
  JH_LAUNCH_CHECK();
  return JH_OK;
}

JH_EXPORT int jh_sacd_actor_loss(jh_ctx* ctx, int32_t B, int32_t A, const float* d_la, const float* d_q1, const float* d_q2, float* d_block, float* d_hyper,
                                 int32_t dynamic, float* d_grad_la, float* d_stats, float* d_work, jh_stream stream) {
  JH_ARG(ctx && d_la && d_q1 && d_q2 && d_block && d_hyper && d_grad_la && d_stats && d_work);
  JH_ARG(B >= 1 && B <= kMaxRows && A >= 2 && A <= kMaxActions);
  JH_ARG(dynamic == 0 || dynamic == 1);
  JH_ARG(((uintptr_t)d_work & 7) == 0 && ((uintptr_t)d_hyper & 7) == 0);
  ActorArgs a{B, A, dynamic, d_la, d_q1, d_q2, d_block, d_hyper, d_grad_la, d_stats, d_work};
  JH_LAUNCH(jh_sacd_actor_kernel, dim3(sacd_grid(B, A)), dim3(kThreads), 0, jh_s(stream), a);
  JH_LAUNCH_CHECK();
  return JH_OK;
}
