// REINFORCE (core/agent/reinforce.py:83-113): what learn() does between the network's forward and its backward.
//   jh_reinforce_returns          ret[t] = r[t] + gamma ret[t + 1] over ALL T rows of the episode (no reset at a done, reinforce.py:90-92), then
//                                 (ret - mean) / (std + 1e-7) with the population std (reinforce.py:93-94); scan, mean and variance in double
//   jh_reinforce_loss_discrete    loss = -mean_t(log pi[t, a_t] ret[t]) with log pi a log-softmax, and d(loss)/d(logits)         (reinforce.py:104-106)
//   jh_reinforce_loss_continuous  the squashed-Gaussian head of jh_policy_head.h (network/policy.py:49-55), z the pre-tanh value of the action,
//                                 loss = -mean over T * A of Normal(mu, std).log_prob(z) ret[t], and d(loss)/d(raw head)          (reinforce.py:98-106)
// T changes with every episode, so nothing here depends on it in its NUMBER of launches: the scan is one workgroup for any T <= 65536, each
// loss is a row pass over at most kLossBlocks workgroups (grid-stride) and a one-workgroup finish.
// The scan is chunked: thread i owns `per` = ceil(T / 1024) consecutive rows.  The recurrence is linear, so a chunk acts on the return that
// follows it as x -> b + a x with a = gamma^len and b its own discounted sum; the chunks' maps are composed right to left by a shuffle scan
// inside a wave and through LDS across the waves, after which every thread knows the return that follows its chunk and walks its rows once
// more from that carry.  Rows are re-read and re-walked per pass (carry, mean, variance, write) instead of being kept: 64 doubles per thread
// would live in scratch memory, and the whole input is at most 256 KB of L2-resident floats.  No atomics anywhere: every sum is a shuffle
// tree followed by the waves' (or workgroups') partials in index order, the same bits every run.
// Departure on purpose (as jh_mpo_loss_discrete): log pi is a log-softmax of the logits where the reference takes log(softmax).
#include "jh_common.h"
#include "jh_policy_head.h"  // the categorical row and the squashed-Gaussian head element, shared with jh_vmpo.hip and jh_mpo.hip

namespace {

constexpr int kScanThreads = 1024, kScanWaves = kScanThreads / 64, kMaxRows = 65536;
constexpr int kLossThreads = 256, kLossBlocks = 64;
constexpr int kMaxActionsDiscrete = 64, kMaxActionsContinuous = 32;

// the affine map x -> b + a x of a run of rows; `then(first, second)` is the map of the run `first` followed (in time) by the run `second`:
// the return in front of `first` is first(second(x))
struct Affine {
  double a, b;
};
__device__ __forceinline__ Affine then(Affine first, Affine second) { return Affine{first.a * second.a, first.b + first.a * second.b}; }

// the workgroup's sum of v, every thread returns with it: shuffle tree, then the waves in order
__device__ __forceinline__ double scan_block_sum(double v, double* red) {
  v = jh_wave_sum(v);
  __syncthreads();  // `red` may still be read from the previous use
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = 0.0;
  const int nw = ((int)blockDim.x + 63) >> 6;
  for (int w = 0; w < nw; ++w) r += red[w];
  return r;
}

__global__ void __launch_bounds__(kScanThreads) jh_reinforce_returns_kernel(const float* __restrict__ reward, float* __restrict__ ret, int T, int per, double gamma,
                                                                            int standardize) {
  __shared__ double s_a[kScanWaves], s_b[kScanWaves], s_carry[kScanWaves], s_red[kScanWaves];
  const int i = threadIdx.x, lane = i & 63, wid = i >> 6, nw = ((int)blockDim.x + 63) >> 6;
  // rows [lo, hi): empty for the threads past the last chunk (lo >= T), whose map is the identity
  const int lo = i * per < T ? i * per : T;
  const int hi = lo + per < T ? lo + per : T;

  // ---- the chunk's own map
  Affine own{1.0, 0.0};
  for (int t = hi - 1; t >= lo; --t) {
    own.b = (double)reward[t] + gamma * own.b;
    own.a *= gamma;
  }
  // ---- inclusive suffix composition inside the wave: after step o, `inc` covers the chunks of lanes [lane, lane + 2 o)
  Affine inc = own;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double oa = __shfl_down(inc.a, o, 64), ob = __shfl_down(inc.b, o, 64);
    if (lane + o < 64) inc = then(inc, Affine{oa, ob});
  }
  if (lane == 0) {
    s_a[wid] = inc.a;
    s_b[wid] = inc.b;
  }
  __syncthreads();
  // ---- across the waves: the return that follows wave w's last row (nw <= 16 steps by one thread)
  if (i == 0) {
    double x = 0.0;
    for (int w = nw - 1; w >= 0; --w) {
      s_carry[w] = x;
      x = s_b[w] + s_a[w] * x;
    }
  }
  __syncthreads();
  // ---- the return that follows this thread's chunk: the wave's carry through the chunks of the lanes after this one
  const double na = __shfl_down(inc.a, 1, 64), nb = __shfl_down(inc.b, 1, 64);
  const double carry = lane == 63 ? s_carry[wid] : nb + na * s_carry[wid];

  if (!standardize) {
    double x = carry;
    for (int t = hi - 1; t >= lo; --t) {
      x = (double)reward[t] + gamma * x;
      ret[t] = (float)x;
    }
    return;
  }
  // ---- mean, population variance around it, then the write: the same walk three times, the same doubles each time
  double x = carry, sum = 0.0;
  for (int t = hi - 1; t >= lo; --t) {
    x = (double)reward[t] + gamma * x;
    sum += x;
  }
  const double mean = scan_block_sum(sum, s_red) / (double)T;
  x = carry;
  double ssq = 0.0;
  for (int t = hi - 1; t >= lo; --t) {
    x = (double)reward[t] + gamma * x;
    ssq += (x - mean) * (x - mean);
  }
  const double sd = sqrt(scan_block_sum(ssq, s_red) / (double)T);
  const double den = sd + 1e-7;
  x = carry;
  for (int t = hi - 1; t >= lo; --t) {
    x = (double)reward[t] + gamma * x;
    ret[t] = (float)((x - mean) / den);
  }
}

// ------------------------------------------------------------------------------------------------ the losses
struct LossArgs {
  int T, A;
  const float *head, *action, *ret;
  float* grad;
  double* partial;  // [gridDim.x]
};

// one workgroup's sum -> partial[blockIdx.x]
__device__ __forceinline__ void loss_block_partial(double acc, double* partial) {
  __shared__ double s_red[kLossThreads / 64];
  acc = jh_wave_sum(acc);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = 0.0;
    for (int w = 0; w < kLossThreads / 64; ++w) r += s_red[w];
    partial[blockIdx.x] = r;
  }
}

__global__ void __launch_bounds__(kLossThreads) jh_reinforce_loss_discrete_kernel(LossArgs a) {
  const int A = a.A;
  const double inv_T = 1.0 / (double)a.T;
  double acc = 0.0;
  for (int t = blockIdx.x * kLossThreads + threadIdx.x; t < a.T; t += gridDim.x * kLossThreads) {
    const float* z = a.head + (size_t)t * A;
    float* g = a.grad + (size_t)t * A;
    const double lse = row_lse(z, A);
    const int ak = action_index(a.action[t], A);
    const double r = (double)a.ret[t];
    acc += ((double)z[ak] - lse) * r;
    const double w = r * inv_T;
    for (int k = 0; k < A; ++k) {
      const double p = exp((double)z[k] - lse);
      g[k] = (float)(w * (p - (k == ak ? 1.0 : 0.0)));
    }
  }
  loss_block_partial(acc, a.partial);
}

__global__ void __launch_bounds__(kLossThreads) jh_reinforce_loss_continuous_kernel(LossArgs a) {
  const int A = a.A;
  const double inv_n = 1.0 / ((double)a.T * (double)A);
  double acc = 0.0;
  for (int t = blockIdx.x * kLossThreads + threadIdx.x; t < a.T; t += gridDim.x * kLossThreads) {
    const float* h = a.head + (size_t)t * 2 * A;
    float* g = a.grad + (size_t)t * 2 * A;
    const double w = (double)a.ret[t] * inv_n;
    double row = 0.0;
    for (int k = 0; k < A; ++k) {
      const float mr = h[k], lr = h[A + k], ac = a.action[(size_t)t * A + k];  // the three loads together, ahead of the arithmetic
      const GaussElem e = gauss_elem(mr, lr);
      const double d = gauss_z(ac) - e.mu;
      row += gauss_log_prob(d, e.th, e.var);
      g[k] = gauss_grad_mu_raw(e, -w * d / e.var);
      g[A + k] = gauss_grad_log_std_raw(e, -w * (d * d / e.var - 1.0));
    }
    acc += row * (double)a.ret[t];
  }
  loss_block_partial(acc, a.partial);
}

// the workgroups' partials in index order -> stats = {loss, rows}
__global__ void jh_reinforce_finish_kernel(const double* __restrict__ partial, int nb, double scale, int T, float* __restrict__ stats) {
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s += partial[b];
  stats[0] = (float)(-s * scale);
  stats[1] = (float)T;
}

template <typename K>
int launch_loss(jh_ctx* ctx, const char* name, K kernel, int T, int A, int head_cols, const float* d_head, const float* d_action, const float* d_ret, float* d_grad, float* d_stats,
                jh_stream stream) {
  const int nb = (T + kLossThreads - 1) / kLossThreads < kLossBlocks ? (T + kLossThreads - 1) / kLossThreads : kLossBlocks;
  void* scratch = nullptr;
  int rc = jh_ctx_scratch(ctx, sizeof(double) * kLossBlocks, &scratch);
  if (rc) return rc;
  LossArgs a{};
  a.T = T; a.A = A; a.head = d_head; a.action = d_action; a.ret = d_ret; a.grad = d_grad; a.partial = (double*)scratch;
  JH_LAUNCH_NAMED(name, kernel, dim3(nb), dim3(kLossThreads), 0, jh_s(stream), a);
  JH_LAUNCH_CHECK();
  JH_LAUNCH(jh_reinforce_finish_kernel, dim3(1), dim3(64), 0, jh_s(stream), (const double*)scratch, nb, 1.0 / ((double)T * (double)(head_cols)), T, d_stats);
  JH_LAUNCH_CHECK();
  return JH_OK;
}

}  // namespace

JH_EXPORT int jh_reinforce_returns(jh_ctx* ctx, int32_t T, const float* d_reward, double gamma, int32_t standardize, float* d_ret, jh_stream stream) {
  JH_ARG(ctx && d_reward && d_ret);
  JH_ARG(T >= 1 && T <= kMaxRows);
  JH_ARG(standardize == 0 || standardize == 1);
  const int per = (T + kScanThreads - 1) / kScanThreads;
  const int chunks = (T + per - 1) / per;
  const int threads = ((chunks + 63) / 64) * 64;
  JH_LAUNCH(jh_reinforce_returns_kernel, dim3(1), dim3(threads), 0, jh_s(stream), d_reward, d_ret, (int)T, per, gamma, (int)standardize);
  JH_LAUNCH_CHECK();
  return JH_OK;
}

JH_EXPORT int jh_reinforce_loss_discrete(jh_ctx* ctx, int32_t T, int32_t A, const float* d_logits, const float* d_action, const float* d_ret, float* d_grad_logits,
                                         float* d_stats, jh_stream stream) {
  JH_ARG(ctx && d_logits && d_action && d_ret && d_grad_logits && d_stats);
  JH_ARG(T >= 1 && T <= kMaxRows && A >= 2 && A <= kMaxActionsDiscrete);
  return launch_loss(ctx, "jh_reinforce_loss_discrete_kernel", jh_reinforce_loss_discrete_kernel, T, A, 1, d_logits, d_action, d_ret, d_grad_logits, d_stats, stream);
}

JH_EXPORT int jh_reinforce_loss_continuous(jh_ctx* ctx, int32_t T, int32_t A, const float* d_head, const float* d_action, const float* d_ret, float* d_grad_head,
                                           float* d_stats, jh_stream stream) {
  JH_ARG(ctx && d_head && d_action && d_ret && d_grad_head && d_stats);
  JH_ARG(T >= 1 && T <= kMaxRows && A >= 1 && A <= kMaxActionsContinuous);
  return launch_loss(ctx, "jh_reinforce_loss_continuous_kernel", jh_reinforce_loss_continuous_kernel, T, A, A, d_head, d_action, d_ret, d_grad_head, d_stats, stream);
}
