// What the two curiosity modules (ICM-PPO: jh_icm.hip, RND-PPO: jh_rnd.hip) share below their architecture, ONE copy: the column-statistics
// helper and the RunningMeanStd merge (core/network/utils.py:18-52), the observation moments, gather + normalise + clip (rnd.py:9-10), batch
// norm under BATCH statistics fused with the activation (ELU: icm.py:20-34 | ReLU: rnd.py:38-52) forward and backward, and the reward filter
// with the moments of the intrinsic reward (icm.py:145-150 = rnd.py:159-164).  The library is built with -ffp-contract=off, so the same
// expression tree inlined from here gives both translation units the same bits.
// A column's statistics are taken by ONE workgroup over all rows (16 columns x 16 row lanes: shuffles inside a wave, then LDS across the four
// waves), the variance about the mean in a second pass, in double.  No atomics and no spinning: every sum has a fixed order, so two runs (and
// a graph replay) give the same bits.
#pragma once
#include "jh_netcore.h"

namespace {

constexpr int kCurF = 256;          // feature size of both modules, whatever hidden_size says (icm.py:181, rnd.py:196)
constexpr int kCurMaxBatch = 8192;  // rows of one call: the tile engine indexes in 32 bits, the loss kernels are one workgroup
constexpr float kBnEps = 1e-5f, kBnMomentum = 0.1f;

enum { CUR_ELU = 0, CUR_RELU = 1 };
// A flag beside the activation in the batch-norm kernels' MODE.  Without it (ICM-PPO) the normalisation runs in float32 on the float32
// roundings of the column's mean and 1 / sqrt(var + eps); with it (RND-PPO) xhat is formed in double from the double statistics, forward and
// backward, and rounded once.  It matters over two or three rows: there xhat = +-1 / sqrt(1 + eps / var), the gradient through the batch
// norm is eps / (var + eps) of its terms, and a mean off by half an ulp of z tilts the two outputs of a column against each other by more
// than that (measured at two rows: gradients 1.8e-4 of their largest entry from float64 without the flag, 5e-6 with it).
enum { CUR_F64 = 2 };

template <int ACT>
__device__ __forceinline__ float cur_act(float u) {
  if (ACT == CUR_ELU) return u > 0.f ? u : expm1f(u);
  return u > 0.f ? u : 0.f;
}
// d(act)/du from the OUTPUT y: ELU 1 (y > 0) | y + 1 = exp(u); ReLU 1 (y > 0) | 0
template <int ACT>
__device__ __forceinline__ float cur_act_grad(float d, float y) {
  if (ACT == CUR_ELU) return y > 0.f ? d : d * (y + 1.f);
  return y > 0.f ? d : 0.f;
}

// sum over the 16 row lanes of a column: lanes c, c + 16, c + 32, c + 48 of each wave by shuffles, then the four waves through LDS in wave order
__device__ __forceinline__ double cur_col_sum(double v, double (*red)[16]) {
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();  // protect `red` from a previous use
  if (lane < 16) red[w][lane] = v;
  __syncthreads();
  const int c = threadIdx.x & 15;
  return ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
}

// RunningMeanStd.update_from_moments (utils.py:31-52) in float32, operation for operation
__device__ __forceinline__ void cur_rms_merge(float& mean, float& var, float count, float bm, float bv, float bc) {
  const float delta = bm - mean;
  const float tot = count + bc;
  const float new_mean = mean + delta * bc / tot;
  const float m_a = var * count;
  const float m_b = bv * bc;
  const float M2 = m_a + m_b + delta * delta * count * bc / (count + bc);
  var = M2 / (count + bc);
  mean = new_mean;
}

// ---------------------------------------------------------------------------------- observation moments and their merge
// update_rms_obs(next_state) (icm_ppo.py:98, rnd_ppo.py:119, utils.py:26-29): per-feature mean and UNBIASED variance over the rows, merged
// into the running mean / var / count.  One workgroup: the count is one word that every feature's merge reads and the last step writes.
__global__ void __launch_bounds__(256) jh_cur_obs_update_kernel(int rows, int S, const float* __restrict__ x, float* mean, float* var, float* count) {
  __shared__ double s_red[4][16];
  const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const float cnt = *count;
  for (int c0 = 0; c0 < S; c0 += 16) {
    const int c = c0 + cl;
    const bool on = c < S;
    double s = 0.0;
    if (on)
      for (int r = rl; r < rows; r += 16) s += (double)x[(size_t)r * S + c];
    s = cur_col_sum(s, s_red);
    const double mu = s / (double)rows;
    double q = 0.0;
    if (on)
      for (int r = rl; r < rows; r += 16) {
        const double d = (double)x[(size_t)r * S + c] - mu;
        q += d * d;
      }
    q = cur_col_sum(q, s_red);
    if (on && rl == 0) {
      float mn = mean[c], vr = var[c];
      cur_rms_merge(mn, vr, cnt, (float)mu, (float)(q / (double)(rows - 1)), (float)rows);
      mean[c] = mn;
      var[c] = vr;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) *count = (float)rows + cnt;
}

// ---------------------------------------------------------------------------------- gather, normalise, clip
// x = [src[0][idx]; src[1][idx]] (halves * b rows), normalize_obs (rnd.py:9-10) when mean != nullptr; with ac > 0 the action columns of
// fin [b][ldf] at column `fcol` and of fin2 [b][ldf2] at column `fcol2` (ICM's [phi | a] and [fh | a])
struct PrepArgs {
  int b, S, ac, halves, fcol, fcol2, ldf, ldf2;
  int64_t n_rows;
  const float* src[2];
  const float* action;
  const int64_t* idx;
  const float *mean, *var;
  float *x, *fin, *fin2;
};
__device__ __forceinline__ int64_t cur_row(const PrepArgs& a, int r) {
  int64_t s = a.idx ? a.idx[r] : (int64_t)r;
  return s < 0 ? 0 : (s >= a.n_rows ? a.n_rows - 1 : s);  // a bad index must not read outside the rollout
}
__global__ void __launch_bounds__(256) jh_cur_prep_kernel(PrepArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t nx = (int64_t)a.halves * a.b * a.S;
  if (i < nx) {
    const int c = (int)(i % a.S);
    const int rr = (int)(i / a.S);
    const int half = rr >= a.b, r = rr - half * a.b;
    float v = a.src[half][cur_row(a, r) * a.S + c];
    if (a.mean) {
      v = (v - a.mean[c]) / (sqrtf(a.var[c]) + 1e-7f);
      v = fminf(fmaxf(v, -5.f), 5.f);
    }
    a.x[i] = v;
  } else if (i < nx + (int64_t)a.b * a.ac) {
    const int64_t j = i - nx;
    const int k = (int)(j % a.ac), r = (int)(j / a.ac);
    const float v = a.action[cur_row(a, r) * a.ac + k];
    a.fin[(size_t)r * a.ldf + a.fcol + k] = v;
    a.fin2[(size_t)r * a.ldf2 + a.fcol2 + k] = v;
  }
}
inline int64_t cur_prep_threads(const PrepArgs& a) { return (int64_t)a.halves * a.b * a.S + (int64_t)a.b * a.ac; }

// ---------------------------------------------------------------------------------- batch norm (batch statistics) + activation
// z [nh * b][C]: half h = rows [h b, h b + b) with its own batch norm (gamma == nullptr: none, the activation only).  y = act((z - mean) /
// sqrt(var + eps) * gamma + beta) with the BIASED batch variance; running_mean / running_var advance with momentum 0.1 and the UNBIASED
// variance (torch.nn.BatchNorm1d in training mode).  grid = (ceil(C / 16), nh).
struct BnHalf {
  const float *gamma, *beta;
  float *rmean, *rvar, *smean, *sinv;
  float* out0;
  int ld0;
  float* out1;  // optional second copy of the output
  int ld1;
};
struct BnFwdArgs {
  const float* z;
  int b, C;
  BnHalf h[2];
};
template <int MODE>
__global__ void __launch_bounds__(256) jh_cur_bn_act_kernel(BnFwdArgs a) {
  constexpr int ACT = MODE & 1;
  constexpr bool F64 = (MODE & CUR_F64) != 0;
  __shared__ double s_red[4][16];
  const BnHalf& h = a.h[blockIdx.y];
  const int c = blockIdx.x * 16 + (threadIdx.x & 15), rl = threadIdx.x >> 4;
  const int b = a.b, C = a.C;
  const bool on = c < C;
  const float* z = a.z + (size_t)blockIdx.y * b * C;
  float mean = 0.f, inv = 1.f, ga = 1.f, be = 0.f;
  double mean_d = 0.0, inv_d = 1.0;
  if (h.gamma) {  // uniform over the workgroup
    double s = 0.0;
    if (on)
      for (int r = rl; r < b; r += 16) s += (double)z[(size_t)r * C + c];
    s = cur_col_sum(s, s_red);
    const double mu = s / (double)b;
    double q = 0.0;
    if (on)
      for (int r = rl; r < b; r += 16) {
        const double d = (double)z[(size_t)r * C + c] - mu;
        q += d * d;
      }
    q = cur_col_sum(q, s_red);
    const double var = q / (double)b;
    mean_d = mu;
    inv_d = 1.0 / sqrt(var + (double)kBnEps);
    mean = (float)mu;
    inv = (float)inv_d;
    if (on) {
      ga = h.gamma[c];
      be = h.beta[c];
      if (rl == 0) {
        h.smean[c] = mean;
        h.sinv[c] = inv;
        const float unb = (float)(q / (double)(b - 1));
        h.rmean[c] = kBnMomentum * mean + (1.f - kBnMomentum) * h.rmean[c];
        h.rvar[c] = kBnMomentum * unb + (1.f - kBnMomentum) * h.rvar[c];
      }
    }
  }
  if (!on) return;
  for (int r = rl; r < b; r += 16) {
    const float u = F64 ? (float)(((double)z[(size_t)r * C + c] - mean_d) * inv_d * (double)ga + (double)be) : (z[(size_t)r * C + c] - mean) * inv * ga + be;
    const float y = cur_act<ACT>(u);
    h.out0[(size_t)r * h.ld0 + c] = y;
    if (h.out1) h.out1[(size_t)r * h.ld1 + c] = y;
  }
}

// backward of the above: g = (dy0 + dy1) * act'(u) from the output y; through the batch statistics
// dz = gamma inv (g - mean_r g - xhat mean_r (g xhat)), d(gamma) = sum_r g xhat, d(beta) = sum_r g; without batch norm dz = g
struct BnBwdHalf {
  const float* dy0;
  int ldd0;
  const float* dy1;  // optional second source of the gradient
  int ldd1;
  const float* y;
  int ldy;
  const float *gamma, *smean, *sinv;
  float *dgamma, *dbeta;
};
struct BnBwdArgs {
  const float* z;
  float* dz;
  int b, C;
  BnBwdHalf h[2];
};
template <int ACT>
__device__ __forceinline__ float cur_bn_g(const BnBwdHalf& h, int r, int c) {
  float d = h.dy0[(size_t)r * h.ldd0 + c];
  if (h.dy1) d += h.dy1[(size_t)r * h.ldd1 + c];
  return cur_act_grad<ACT>(d, h.y[(size_t)r * h.ldy + c]);
}
template <int MODE>
__global__ void __launch_bounds__(256) jh_cur_bn_act_bwd_kernel(BnBwdArgs a) {
  constexpr int ACT = MODE & 1;
  constexpr bool F64 = (MODE & CUR_F64) != 0;
  __shared__ double s_red[4][16];
  const BnBwdHalf& h = a.h[blockIdx.y];
  const int c = blockIdx.x * 16 + (threadIdx.x & 15), rl = threadIdx.x >> 4;
  const int b = a.b, C = a.C;
  const bool on = c < C;
  const float* z = a.z + (size_t)blockIdx.y * b * C;
  float* dz = a.dz + (size_t)blockIdx.y * b * C;
  if (!h.gamma) {
    if (on)
      for (int r = rl; r < b; r += 16) dz[(size_t)r * C + c] = cur_bn_g<ACT>(h, r, c);
    return;
  }
  const float mean = on ? h.smean[c] : 0.f, inv = on ? h.sinv[c] : 1.f, ga = on ? h.gamma[c] : 1.f;
  if (F64) {  // the statistics again from z, in double (the forward saved their float32 roundings)
    double s = 0.0;
    if (on)
      for (int r = rl; r < b; r += 16) s += (double)z[(size_t)r * C + c];
    const double mu = cur_col_sum(s, s_red) / (double)b;
    double q = 0.0;
    if (on)
      for (int r = rl; r < b; r += 16) {
        const double d = (double)z[(size_t)r * C + c] - mu;
        q += d * d;
      }
    const double iv = 1.0 / sqrt(cur_col_sum(q, s_red) / (double)b + (double)kBnEps);
    double tg = 0.0, tgx = 0.0;
    if (on)
      for (int r = rl; r < b; r += 16) {
        const double g = (double)cur_bn_g<ACT>(h, r, c);
        tg += g;
        tgx += g * (((double)z[(size_t)r * C + c] - mu) * iv);
      }
    tg = cur_col_sum(tg, s_red);
    tgx = cur_col_sum(tgx, s_red);
    if (!on) return;
    if (rl == 0) {
      h.dgamma[c] = (float)tgx;
      h.dbeta[c] = (float)tg;
    }
    const double mg = tg / (double)b, mgx = tgx / (double)b;
    for (int r = rl; r < b; r += 16) {
      const double xh = ((double)z[(size_t)r * C + c] - mu) * iv;
      dz[(size_t)r * C + c] = (float)((double)ga * iv * ((double)cur_bn_g<ACT>(h, r, c) - mg - xh * mgx));
    }
    return;
  }
  double sg = 0.0, sgx = 0.0;
  if (on)
    for (int r = rl; r < b; r += 16) {
      const float g = cur_bn_g<ACT>(h, r, c);
      const float xh = (z[(size_t)r * C + c] - mean) * inv;
      sg += (double)g;
      sgx += (double)g * (double)xh;
    }
  sg = cur_col_sum(sg, s_red);
  sgx = cur_col_sum(sgx, s_red);
  if (!on) return;
  if (rl == 0) {
    h.dgamma[c] = (float)sgx;
    h.dbeta[c] = (float)sg;
  }
  const float mg = (float)(sg / (double)b), mgx = (float)(sgx / (double)b);
  for (int r = rl; r < b; r += 16) {
    const float g = cur_bn_g<ACT>(h, r, c);
    const float xh = (z[(size_t)r * C + c] - mean) * inv;
    dz[(size_t)r * C + c] = ga * inv * (g - mg - xh * mgx);
  }
}

// ---------------------------------------------------------------------------------- reward filter, rms_ri, normalisation
// ri_update (icm.py:145-150, rnd.py:159-164) as the reference really behaves, the normalisation and (reward != nullptr: ICM-PPO,
// icm_ppo.py:100-102) the mix.  One workgroup.
//   filter     worker w's rows are w T .. w T + T - 1 (r_i.view(num_workers, -1)): rewems_w <- rewems_w * gamma + r_i[w, t] for t = 0 .. T - 1
//   rms_ri     RewardForwardFilter.update returns the Parameter ITSELF, so the reference's stack is T copies of the FINAL rewems: batch count
//              T W, batch mean mean_w rewems_w, unbiased batch variance T sum_w (rewems_w - mean)^2 / (T W - 1)
//   r_i        /= sqrt(rms_ri.var) + 1e-7 (the var AFTER this update), reward <- ext * reward + int * r_i, *ri_mean = mean(r_i)
struct RewardArgs {
  int rows, W, T, ri_norm;
  const float* ri_raw;
  float *ri_blk, *rewems;  // {mean, var, count}, [W]
  float gamma, ext, intr;
  float *reward, *ri_out, *ri_mean;
};
__global__ void __launch_bounds__(256) jh_cur_reward_kernel(RewardArgs a) {
  __shared__ double s_red[16];
  __shared__ float s_den;
  const int W = a.W, T = a.T;
  for (int w = threadIdx.x; w < W; w += 256) {
    float rew = a.rewems[w];
    for (int t = 0; t < T; ++t) rew = rew * a.gamma + a.ri_raw[(size_t)w * T + t];
    a.rewems[w] = rew;
  }
  __syncthreads();
  double s = 0.0;
  for (int w = threadIdx.x; w < W; w += 256) s += (double)a.rewems[w];
  s = jh_block_reduce(s, s_red, JhAdd(), 0.0);
  const double mu = s / (double)W;
  double q = 0.0;
  for (int w = threadIdx.x; w < W; w += 256) {
    const double d = (double)a.rewems[w] - mu;
    q += d * d;
  }
  q = jh_block_reduce(q, s_red, JhAdd(), 0.0);
  if (threadIdx.x == 0) {
    const double n = (double)T * (double)W;
    float mn = a.ri_blk[0], vr = a.ri_blk[1];
    const float cnt = a.ri_blk[2];
    cur_rms_merge(mn, vr, cnt, (float)mu, (float)((double)T * q / (n - 1.0)), (float)n);
    a.ri_blk[0] = mn;
    a.ri_blk[1] = vr;
    a.ri_blk[2] = (float)n + cnt;
    s_den = a.ri_norm ? sqrtf(vr) + 1e-7f : 1.f;
  }
  __syncthreads();
  const float den = s_den;
  double acc = 0.0;
  for (int i = threadIdx.x; i < a.rows; i += 256) {
    float r = a.ri_raw[i];
    if (a.ri_norm) r = r / den;
    if (a.ri_out) a.ri_out[i] = r;
    if (a.reward) {
      const float e = a.ext * a.reward[i];
      const float f = a.intr * r;
      a.reward[i] = e + f;
    }
    acc += (double)r;
  }
  acc = jh_block_reduce(acc, s_red, JhAdd(), 0.0);
  if (threadIdx.x == 0 && a.ri_mean) *a.ri_mean = (float)(acc / (double)a.rows);
}

// ---------------------------------------------------------------------------------- the statistics block both modules start with
// rms_obs mean [S], var [S], count | rms_ri mean, var, count | rewems [W]; the batch norms' running moments follow, per module
struct CurBlock {
  int o_obs_mean = 0, o_obs_var = 0, o_obs_cnt = 0, o_ri = 0, o_rew = 0, end = 0;
};
inline CurBlock cur_block(int S, int W) {
  CurBlock k;
  int o = 0;
  k.o_obs_mean = o; o += S;
  k.o_obs_var = o; o += S;
  k.o_obs_cnt = o; o += 1;
  k.o_ri = o; o += 3;
  k.o_rew = o; o += W;
  k.end = o;
  return k;
}

}  // namespace
