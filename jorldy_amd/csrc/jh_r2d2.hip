// R2D2 (core/agent/r2d2.py, core/network/r2d2.py): the recurrence of torch.nn.LSTM one time step per launch, forward and backward, and the
// sequence loss of R2D2.learn().  There is no whole-sequence kernel and no grid-wide wait: a step depends on the previous one through (h, c),
// and that dependency is a kernel boundary.
//
//   jh_lstm_step            gates = xproj_t + h_{t-1} W_hh^T on the fp32 MFMA, then the cell, in ONE launch.  A workgroup owns 16 rows x 16
//                           hidden units across all four gates (torch's order i, f, g, o), so the cell update needs nothing from another
//                           workgroup.  Its four waves split the reduction over k; the partial tiles meet in LDS and are summed in wave
//                           order.  Up to four row segments per launch, each with its own weights and buffers (online rows, target rows).
//   jh_lstm_step_backward   the mirror image: dh_t = dh_ext_t + dgates_{t+1} W_hh on the MFMA (the recurrent product belongs to the launch
//                           that CONSUMES it: a workgroup then needs the saved activations of its own 16 units only, where forming
//                           dgates_t first and multiplying afterwards would need all 4H of them per output tile), then dgates_t and
//                           dc_{t-1} of the owned units.
//   jh_r2d2_loss            ONE workgroup, one thread per batch row looping over the trained steps (the shape of jh_mpo_loss_discrete):
//                           double-Q selection, both value rescales, the n-step fold, |td|, the sequence priority, the last step's loss.
// No floating-point atomics anywhere: the same inputs give the same bits, eagerly or replayed in a graph.
#include "jh_common.h"
#include "jh_mult.h"
#include "jh_netcore.h"

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kMaxSeg = JH_LSTM_MAX_SEGS;

struct LstmStepArgs {
  int H, nseg;
  int tile0[kMaxSeg + 1];  // first row tile of every segment in grid.x
  jh_lstm_seg seg[kMaxSeg];
};

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// lane l of a wave holds A[row l & 15][k = 4 (l >> 4) + i] and B[the same k][column l & 15], i = 0 .. 3, of a 16-deep k chunk: four
// 16x16x4 products per chunk, with both operands fetched 16 bytes at a time where k is the contiguous index.  H % 4 == 0 keeps every
// such piece whole: inside the matrix or outside it.
__global__ void __launch_bounds__(256) jh_lstm_step_kernel(LstmStepArgs a) {
  __shared__ float s_part[4][4][4][64];  // [wave][gate][accumulator register][lane]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, H = a.H;
  int s = 0;
  while (s + 1 < a.nseg && (int)blockIdx.x >= a.tile0[s + 1]) ++s;
  const jh_lstm_seg g = a.seg[s];
  const int r0 = ((int)blockIdx.x - a.tile0[s]) * 16, u0 = (int)blockIdx.y * 16;
  {
    const int row = r0 + (lane & 15), unit = u0 + (lane & 15), kq = (lane >> 4) * 4;
    const bool row_ok = row < g.rows, unit_ok = unit < H;
    const float* hp = g.h_prev + (size_t)(row_ok ? row : 0) * H;
    const float* wp = g.w_hh + (size_t)(unit_ok ? unit : 0) * H;
    f32x4 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int chunks = (H + 15) / 16;
    for (int c = wave; c < chunks; c += 4) {
      const int k = c * 16 + kq;
      const bool k_ok = k < H;
      float4 av = make_float4(0.f, 0.f, 0.f, 0.f), bv[4];
      if (row_ok && k_ok) av = *reinterpret_cast<const float4*>(hp + k);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        bv[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (unit_ok && k_ok) bv[q] = *reinterpret_cast<const float4*>(wp + (size_t)q * H * H + k);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv[q].x, acc[q], 0, 0, 0);
        acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv[q].y, acc[q], 0, 0, 0);
        acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv[q].z, acc[q], 0, 0, 0);
        acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv[q].w, acc[q], 0, 0, 0);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j) s_part[wave][q][j][lane] = acc[q][j];
  }
  __syncthreads();
  // thread -> (row r, unit u) of the tile; its sum sits in register r & 3 of lane (r >> 2) * 16 + u (the 16x16 C / D map)
  const int r = threadIdx.x >> 4, u = threadIdx.x & 15;
  const int row = r0 + r, unit = u0 + u;
  if (row >= g.rows || unit >= H) return;
  const int src = (r >> 2) * 16 + u, j = r & 3;
  float pre[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float rec = ((s_part[0][q][j][src] + s_part[1][q][j][src]) + s_part[2][q][j][src]) + s_part[3][q][j][src];
    pre[q] = g.xproj[(size_t)row * g.ld_x + (size_t)q * H + unit] + rec;
  }
  const float gi = sigmoidf_(pre[0]), gf = sigmoidf_(pre[1]), gg = tanhf(pre[2]), go = sigmoidf_(pre[3]);
  const size_t o = (size_t)row * H + unit;
  const float c = gf * g.c_prev[o] + gi * gg;
  g.c_out[o] = c;
  g.h_out[o] = go * tanhf(c);
  if (g.gates_out) {
    float* gp = g.gates_out + (size_t)row * 4 * H + unit;
    gp[0] = gi; gp[H] = gf; gp[2 * (size_t)H] = gg; gp[3 * (size_t)H] = go;
  }
}

struct LstmBwdArgs {
  int R, H;
  const float* dgates_next;  // [R][4H] of step t + 1, or null (the last step)
  const float* w_hh;         // [4H][H]
  const float* dh_ext;       // [R][H] gradient reaching h_t from the layers above, or null
  const float* dc_in;        // [R][H] = dc_t handed down by step t + 1, or null
  const float *gates, *c_prev, *c;
  float *dgates, *dc_prev;
};

__global__ void __launch_bounds__(256) jh_lstm_step_backward_kernel(LstmBwdArgs a) {
  __shared__ float s_part[4][4][64];  // [wave][accumulator register][lane]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, H = a.H, R = a.R;
  const int r0 = (int)blockIdx.x * 16, u0 = (int)blockIdx.y * 16;
  if (a.dgates_next) {  // the same for every thread of the launch
    const int row = r0 + (lane & 15), unit = u0 + (lane & 15), kq = (lane >> 4) * 4;
    const bool row_ok = row < R, unit_ok = unit < H;
    const float* ap = a.dgates_next + (size_t)(row_ok ? row : 0) * 4 * H;
    const float* bp = a.w_hh + (unit_ok ? unit : 0);
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};  // two chains: a dependent 16x16x4 waits 40 cycles, an independent one 32
    const int chunks = H / 4;  // K = 4H in pieces of 16
    for (int c = wave; c < chunks; c += 4) {
      const int k = c * 16 + kq;
      float4 av = make_float4(0.f, 0.f, 0.f, 0.f);
      float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f;
      if (row_ok) av = *reinterpret_cast<const float4*>(ap + k);
      if (unit_ok) {
        b0 = bp[(size_t)k * H]; b1 = bp[(size_t)(k + 1) * H]; b2 = bp[(size_t)(k + 2) * H]; b3 = bp[(size_t)(k + 3) * H];
      }
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, b1, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, b2, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, b3, acc1, 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) s_part[wave][j][lane] = acc0[j] + acc1[j];
    __syncthreads();
  }
  const int r = threadIdx.x >> 4, u = threadIdx.x & 15;
  const int row = r0 + r, unit = u0 + u;
  if (row >= R || unit >= H) return;
  const size_t o = (size_t)row * H + unit;
  float dh = a.dh_ext ? a.dh_ext[o] : 0.f;
  if (a.dgates_next) {
    const int src = (r >> 2) * 16 + u, j = r & 3;
    dh += ((s_part[0][j][src] + s_part[1][j][src]) + s_part[2][j][src]) + s_part[3][j][src];
  }
  const float* gp = a.gates + (size_t)row * 4 * H + unit;
  const float gi = gp[0], gf = gp[H], gg = gp[2 * (size_t)H], go = gp[3 * (size_t)H];
  const float tc = tanhf(a.c[o]);
  float dc = dh * go * (1.f - tc * tc);
  if (a.dc_in) dc += a.dc_in[o];
  float* dg = a.dgates + (size_t)row * 4 * H + unit;
  dg[0] = dc * gg * (gi * (1.f - gi));
  dg[H] = dc * a.c_prev[o] * (gf * (1.f - gf));
  dg[2 * (size_t)H] = dc * gi * (1.f - gg * gg);
  dg[3 * (size_t)H] = dh * tc * (go * (1.f - go));
  a.dc_prev[o] = dc * gf;
}

// ---------------------------------------------------------------------------------------------------------------- the sequence loss
constexpr int kMaxRows = 1024, kMaxWaves = kMaxRows / 64, kMaxSteps = 128, kMaxActions = 64;

struct R2d2LossArgs {
  int B, T, A, burn, n_step, cols;  // T trained steps; cols = seq_len + n_step - 1 entries per row of action / reward / done
  const float *q, *nq, *ntq;        // [T][B][A]: online over state[:, :seq_len], online and target over state[:, n_step:]
  const float *action, *reward, *done;  // [B][cols]
  const float* weights;                 // [B]
  float gamma, eta, alpha, eps;
  float* g_q;     // [T][B][A]
  double* prio;   // [B]
  float* td;      // [B][T] or null
  float* stats;   // [8]
};

// h(x) = sign(x) (sqrt(|x| + 1) - 1) + eps x with sign(x) = x / (|x| + 1e-10) (r2d2.py:304-307), the root taken as |x| / (sqrt(|x| + 1) + 1)
__device__ __forceinline__ double val_rescale(double x, double eps) {
  const double ax = fabs(x);
  return (x / (ax + 1e-10)) * (ax / (sqrt(ax + 1.0) + 1.0)) + eps * x;
}
// h^-1(x) = sign(x) (((sqrt(1 + y) - 1) / (2 eps))^2 - 1), y = 4 eps (|x| + 1 + eps) (r2d2.py:309-313).  sqrt(1 + y) - 1 is formed as
// y / (sqrt(1 + y) + 1), which leaves u = 2 (|x| + 1 + eps) / (sqrt(1 + y) + 1): the float32 expression as written loses up to 2e-4 of the
// largest target there.  u^2 - 1 is taken in double, where its cancellation costs 1e-16.
__device__ __forceinline__ double inv_val_rescale(double x, double eps) {
  const double ax = fabs(x);
  const double y = 4.0 * eps * (ax + 1.0 + eps), sq = sqrt(1.0 + y);
  const double u = 2.0 * (ax + 1.0 + eps) / (sq + 1.0);
  return (x / (ax + 1e-10)) * (u * u - 1.0);
}

__global__ void __launch_bounds__(kMaxRows) jh_r2d2_loss_kernel(R2d2LossArgs a) {
  __shared__ double s_red[kMaxWaves][8];
  __shared__ float s_ext[kMaxWaves];
  const int b = threadIdx.x, B = a.B, T = a.T, A = a.A;
  const bool on = b < B;
  double wl = 0.0;
  float q_hi = -INFINITY;
  if (on) {
    const double gamma = (double)a.gamma, eps = (double)a.eps, eta = (double)a.eta;
    const float* act = a.action + (size_t)b * a.cols + a.burn;
    const float* rew = a.reward + (size_t)b * a.cols + a.burn;
    const float* dn = a.done + (size_t)b * a.cols + a.burn;
    double td_max = 0.0, td_sum = 0.0, d_last = 0.0;
    int ak_last = 0;
    for (int t = 0; t < T; ++t) {
      const size_t o = ((size_t)t * B + b) * A;
      int ak = (int)act[t];
      ak = ak < 0 ? 0 : (ak >= A ? A - 1 : ak);
      const float qa = a.q[o + ak];
      q_hi = fmaxf(q_hi, qa);
      int best = 0;  // first maximum, like torch.argmax (jh_value_act)
      float bq = a.nq[o];
      for (int k = 1; k < A; ++k)
        if (a.nq[o + k] > bq) { bq = a.nq[o + k]; best = k; }
      double tq = inv_val_rescale((double)a.ntq[o + best], eps);
      for (int i = a.n_step - 1; i >= 0; --i) tq = (double)rew[i + t] + (1.0 - (double)dn[i + t]) * gamma * tq;  // r2d2.py:133-139
      tq = val_rescale(tq, eps);
      const double d = (double)qa - tq, ad = fabs(d);
      td_max = fmax(td_max, ad);
      td_sum += ad;
      if (a.td) a.td[(size_t)b * T + t] = (float)ad;
      for (int k = 0; k < A; ++k) a.g_q[o + k] = 0.f;
      d_last = d;
      ak_last = ak;
    }
    const double w = (double)a.weights[b];
    wl = w * d_last * d_last;  // r2d2.py:158-159: the last step only
    a.g_q[((size_t)(T - 1) * B + b) * A + ak_last] = (float)(2.0 * w * d_last / (double)B);
    a.prio[b] = pow(eta * td_max + (1.0 - eta) * (td_sum / (double)T), (double)a.alpha);  // r2d2.py:145-148
  }
  q_hi = jh_wave_max(q_hi);
  if ((b & 63) == 0) s_ext[b >> 6] = q_hi;
  double s1[1] = {wl};
  block_sums<1>(s1, s_red);  // its barriers publish s_ext too
  if (b != 0) return;
  const int nw = ((int)blockDim.x + 63) >> 6;
  for (int w = 1; w < nw; ++w) q_hi = fmaxf(q_hi, s_ext[w]);
  a.stats[0] = (float)(s1[0] / (double)B);
  a.stats[1] = q_hi;
  a.stats[2] = a.stats[3] = a.stats[4] = a.stats[6] = 0.f;
  __threadfence_system();  // payload before the arrival marks [5], [7] (mapped host memory, jh_host_wait_marks)
  a.stats[5] = a.stats[7] = 0.f;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

JH_EXPORT int jh_lstm_step(jh_ctx* ctx, int32_t H, int32_t n_segs, const jh_lstm_seg* segs, jh_stream stream) {
  JH_ARG(ctx && segs && H >= 4 && H % 4 == 0 && H <= 4096 && n_segs >= 1 && n_segs <= kMaxSeg);
  LstmStepArgs a{};
  a.H = H;
  int tiles = 0;
  for (int s = 0; s < n_segs; ++s) {
    const jh_lstm_seg& g = segs[s];
    JH_ARG(g.rows >= 0 && g.rows <= (1 << 20));
    if (g.rows == 0) continue;  // an empty segment takes no part in the launch
    JH_ARG(g.xproj && g.w_hh && g.h_prev && g.c_prev && g.h_out && g.c_out && g.ld_x >= 4 * H);
    JH_ARG(aligned16(g.w_hh) && aligned16(g.h_prev));
    a.tile0[a.nseg] = tiles;
    a.seg[a.nseg++] = g;
    tiles += (g.rows + 15) / 16;
  }
  if (!a.nseg) return JH_OK;
  for (int s = a.nseg; s <= kMaxSeg; ++s) a.tile0[s] = tiles;
  JH_LAUNCH(jh_lstm_step_kernel, dim3(tiles, (H + 15) / 16), dim3(256), 0, jh_s(stream), a);
  JH_LAUNCH_CHECK();
  return JH_OK;
}

JH_EXPORT int jh_lstm_step_backward(jh_ctx* ctx, int32_t R, int32_t H, const float* d_dgates_next, const float* d_w_hh, const float* d_dh_ext,
                                    const float* d_dc_in, const float* d_gates, const float* d_c_prev, const float* d_c, float* d_dgates,
                                    float* d_dc_prev, jh_stream stream) {
  JH_ARG(ctx && d_w_hh && d_gates && d_c_prev && d_c && d_dgates && d_dc_prev);
  JH_ARG(R >= 1 && R <= (1 << 20) && H >= 4 && H % 4 == 0 && H <= 4096);
  JH_ARG(aligned16(d_dgates_next));
  LstmBwdArgs a{};
  a.R = R; a.H = H; a.dgates_next = d_dgates_next; a.w_hh = d_w_hh; a.dh_ext = d_dh_ext; a.dc_in = d_dc_in; a.gates = d_gates; a.c_prev = d_c_prev;
  a.c = d_c; a.dgates = d_dgates; a.dc_prev = d_dc_prev;
  JH_LAUNCH(jh_lstm_step_backward_kernel, dim3((R + 15) / 16, (H + 15) / 16), dim3(256), 0, jh_s(stream), a);
  JH_LAUNCH_CHECK();
  return JH_OK;
}

JH_EXPORT int jh_r2d2_loss(jh_ctx* ctx, int32_t B, int32_t T, int32_t A, int32_t n_burn_in, int32_t n_step, const float* d_q, const float* d_next_q,
                           const float* d_next_target_q, const float* d_action, const float* d_reward, const float* d_done, const float* d_weights,
                           float gamma, float eta, float alpha, float eps, float* d_grad_q, double* d_prio, float* d_td, float* d_stats,
                           jh_stream stream) {
  JH_ARG(ctx && d_q && d_next_q && d_next_target_q && d_action && d_reward && d_done && d_weights && d_grad_q && d_prio && d_stats);
  JH_ARG(B >= 1 && B <= kMaxRows && T >= 1 && n_burn_in >= 0 && T + n_burn_in <= kMaxSteps && A >= 2 && A <= kMaxActions);
  JH_ARG(n_step >= 1 && n_step <= kMaxSteps);
  R2d2LossArgs a{};
  a.B = B; a.T = T; a.A = A; a.burn = n_burn_in; a.n_step = n_step; a.cols = T + n_burn_in + n_step - 1;
  a.q = d_q; a.nq = d_next_q; a.ntq = d_next_target_q; a.action = d_action; a.reward = d_reward; a.done = d_done; a.weights = d_weights;
  a.gamma = gamma; a.eta = eta; a.alpha = alpha; a.eps = eps; a.g_q = d_grad_q; a.prio = d_prio; a.td = d_td; a.stats = d_stats;
  JH_LAUNCH(jh_r2d2_loss_kernel, dim3(1), dim3(((B + 63) / 64) * 64), 0, jh_s(stream), a);
  JH_LAUNCH_CHECK();
  return JH_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the network object
// core/network/r2d2.py:8-53 over flat fp32 buckets: head.l (S -> H, relu), cat[x, prev_action_onehot], the LSTM (H + A -> H), l (relu), the
// dueling streams.  Everything is TIME-MAJOR inside (row t * B + b): a time step's rows are then contiguous, the trained steps of a pass are
// one contiguous row range for the layers above the LSTM, and the products over all trained steps (dW_hh, dW_ih, dx) are plain GEMMs.
// l1_a | l1_v are kept as ONE [2H][H] layer with ONE [2H] bias (their segments sit next to each other): one product forward, one backward.
namespace {

enum { R2_W1, R2_B1, R2_WIH, R2_WHH, R2_BIH, R2_BHH, R2_WL, R2_BL, R2_WA1, R2_WV1, R2_BA1, R2_BV1, R2_WA2, R2_BA2, R2_WV2, R2_BV2, R2_SEG_COUNT };

struct PrepArgs {
  int B, L, S, A, H, T;  // L = seq_len + n_step stored steps, T = seq_len
  const float *state, *onehot;                  // [B][L][S], [B][L][A]
  const float *hid[4];                          // hidden_h, hidden_c, next_hidden_h, next_hidden_c [B][H]
  const float *bih[2], *bhh[2];                 // online, target
  float *x_tm, *xin[2], *bsum[2], *hseq, *cseq; // [L B][S], [L B][H + A], [4H], [3][T + 1][B][H]
};

// what the passes need before their first product: the time-major copies, b_ih + b_hh, the stored states in slot 0 of every pass
__global__ void __launch_bounds__(256) jh_r2d2_prep_kernel(PrepArgs a) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
  const int B = a.B, L = a.L, S = a.S, A = a.A, H = a.H;
  for (int64_t i = tid; i < (int64_t)L * B * S; i += nth) {
    const int k = (int)(i % S), b = (int)((i / S) % B), t = (int)(i / ((int64_t)S * B));
    a.x_tm[i] = a.state[((int64_t)b * L + t) * S + k];
  }
  for (int64_t i = tid; i < (int64_t)L * B * A; i += nth) {
    const int k = (int)(i % A), b = (int)((i / A) % B), t = (int)(i / ((int64_t)A * B));
    const float v = a.onehot[((int64_t)b * L + t) * A + k];
    const int64_t o = ((int64_t)t * B + b) * (H + A) + H + k;
    a.xin[0][o] = v;
    a.xin[1][o] = v;
  }
  for (int64_t i = tid; i < 8 * (int64_t)H; i += nth) {
    const int w = (int)(i / (4 * H)), k = (int)(i % (4 * H));
    a.bsum[w][k] = a.bih[w][k] + a.bhh[w][k];
  }
  if (!a.hseq) return;  // (acting: the caller holds the carried state)
  const int64_t slab = (int64_t)(a.T + 1) * B * H;
  for (int64_t i = tid; i < (int64_t)B * H; i += nth) {
    a.hseq[i] = a.hid[0][i];
    a.cseq[i] = a.hid[1][i];
    a.hseq[slab + i] = a.hseq[2 * slab + i] = a.hid[2][i];
    a.cseq[slab + i] = a.cseq[2 * slab + i] = a.hid[3][i];
  }
}

// q = adv - mean_a adv + val (r2d2.py:46-52) for `rows` rows
__global__ void __launch_bounds__(256) jh_r2d2_duel_kernel(int64_t rows, int A, const float* adv, const float* val, float* q) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  float s = 0.f;
  for (int k = 0; k < A; ++k) s += adv[r * A + k];
  const float m = s / (float)A, v = val[r];
  for (int k = 0; k < A; ++k) q[r * A + k] = (adv[r * A + k] - m) + v;
}
// ... and its gradient: dadv = g - mean_a g, dval = sum_a g
__global__ void __launch_bounds__(256) jh_r2d2_duel_bwd_kernel(int64_t rows, int A, const float* g, float* dadv, float* dval) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  float s = 0.f;
  for (int k = 0; k < A; ++k) s += g[r * A + k];
  const float m = s / (float)A;
  for (int k = 0; k < A; ++k) dadv[r * A + k] = g[r * A + k] - m;
  dval[r] = s;
}

}  // namespace

struct jh_r2d2net {
  NetCore core;
  FlatOptim opt;
  int S = 0, H = 0, A = 0, maxB = 0, T = 0, burn = 0, n_step = 0;
  int64_t seg_off[R2_SEG_COUNT] = {0};
  int seg_rows[R2_SEG_COUNT] = {0}, seg_cols[R2_SEG_COUNT] = {0};
  int64_t n_params = 0;
  float *params = nullptr, *target = nullptr, *grads = nullptr, *m = nullptr, *v = nullptr;
  float *x_tm = nullptr, *xin[2] = {nullptr, nullptr}, *bsum[2] = {nullptr, nullptr}, *xp[2] = {nullptr, nullptr};
  float *hseq = nullptr, *cseq = nullptr, *gates = nullptr;      // [3][T + 1][maxB][H] x 2, [T'][maxB][4H]
  float *hl = nullptr, *hav = nullptr, *adv = nullptr, *val = nullptr;  // [3 T' maxB] rows of H, 2H, A, 1
  // acting has buffers of its own ([maxB] rows): an act_step between a learn_forward and its backward leaves the latter's activations alone
  float *a_xin = nullptr, *a_bsum = nullptr, *a_xp = nullptr, *a_hl = nullptr, *a_hav = nullptr, *a_adv = nullptr, *a_val = nullptr;
  float *dadv = nullptr, *dval = nullptr, *dhav = nullptr, *dhl = nullptr, *dh = nullptr, *dgates = nullptr, *dc[2] = {nullptr, nullptr}, *dx = nullptr;
  int last_B = 0;
};

static int r2_layout(jh_r2d2net* n, int32_t S, int32_t H, int32_t A, int32_t max_batch, int32_t seq_len, int32_t n_burn_in, int32_t n_step) {
  JH_ARG(S > 0 && H >= 4 && H % 4 == 0 && H <= 4096 && A >= 2 && A <= kMaxActions);
  JH_ARG(max_batch >= 1 && max_batch <= kMaxRows && seq_len >= 2 && seq_len <= kMaxSteps && n_burn_in >= 1 && n_burn_in < seq_len && n_step >= 1 && n_step <= kMaxSteps);
  JH_ARG((int64_t)(seq_len + n_step) * max_batch * 4 * H < ((int64_t)1 << 31));  // the tile engine indexes rows x columns in 32 bits
  n->S = S; n->H = H; n->A = A; n->maxB = max_batch; n->T = seq_len; n->burn = n_burn_in; n->n_step = n_step;
  auto seg = [&](int id, int rows, int cols) { n->seg_rows[id] = rows; n->seg_cols[id] = cols; };
  seg(R2_W1, H, S); seg(R2_B1, 1, H);
  seg(R2_WIH, 4 * H, H + A); seg(R2_WHH, 4 * H, H); seg(R2_BIH, 1, 4 * H); seg(R2_BHH, 1, 4 * H);
  seg(R2_WL, H, H); seg(R2_BL, 1, H);
  seg(R2_WA1, H, H); seg(R2_WV1, H, H); seg(R2_BA1, 1, H); seg(R2_BV1, 1, H);
  seg(R2_WA2, A, H); seg(R2_BA2, 1, A); seg(R2_WV2, 1, H); seg(R2_BV2, 1, 1);
  n->n_params = seg_pack(n->seg_rows, n->seg_cols, 0, R2_SEG_COUNT, n->seg_off);
  return JH_OK;
}

JH_EXPORT int64_t jh_r2d2net_param_count_for(int32_t S, int32_t H, int32_t A) {
  jh_r2d2net tmp;
  if (r2_layout(&tmp, S, H, A, 1, 2, 1, 1)) return -1;
  return tmp.n_params;
}

JH_EXPORT int jh_r2d2net_create(jh_ctx* ctx, int32_t S, int32_t H, int32_t A, int32_t max_batch, int32_t seq_len, int32_t n_burn_in, int32_t n_step,
                                float* d_params, float* d_target, float* d_grads, float* d_m, float* d_v, jh_r2d2net** out) {
  JH_ARG(ctx && out && d_params && d_target && d_grads && d_m && d_v);
  JH_ARG(aligned16(d_params) && aligned16(d_target));
  JH_HIP(hipSetDevice(ctx->device));
  jh_r2d2net* n = new jh_r2d2net();
  n->core.ctx = ctx;
  int rc = r2_layout(n, S, H, A, max_batch, seq_len, n_burn_in, n_step);
  if (rc) {
    delete n;
    return rc;
  }
  n->params = d_params; n->target = d_target; n->grads = d_grads; n->m = d_m; n->v = d_v;
  const size_t B = max_batch, L = seq_len + n_step, T = seq_len, Tt = seq_len - n_burn_in, LB = L * B, R = Tt * B;
  auto A4 = [&](float** p, size_t floats) { if (!rc) rc = core_alloc(&n->core, "jh_r2d2net", (void**)p, floats * sizeof(float), true); };
  rc = optim_init(&n->core, "jh_r2d2net", &n->opt);
  A4(&n->x_tm, LB * S);
  for (int w = 0; w < 2; ++w) { A4(&n->xin[w], LB * (H + A)); A4(&n->bsum[w], 4 * (size_t)H); A4(&n->xp[w], LB * 4 * H); }
  A4(&n->hseq, 3 * (T + 1) * B * H); A4(&n->cseq, 3 * (T + 1) * B * H); A4(&n->gates, R * 4 * H);
  A4(&n->hl, 3 * R * H); A4(&n->hav, 3 * R * 2 * H); A4(&n->adv, 3 * R * A); A4(&n->val, 3 * R);
  A4(&n->dadv, R * A); A4(&n->dval, R); A4(&n->dhav, R * 2 * H); A4(&n->dhl, R * H); A4(&n->dh, R * H); A4(&n->dgates, R * 4 * H);
  A4(&n->dc[0], B * H); A4(&n->dc[1], B * H); A4(&n->dx, R * H);
  A4(&n->a_xin, B * (H + A)); A4(&n->a_bsum, 4 * (size_t)H); A4(&n->a_xp, B * 4 * H); A4(&n->a_hl, B * H); A4(&n->a_hav, B * 2 * H); A4(&n->a_adv, B * A);
  A4(&n->a_val, B);
  if (!rc) rc = core_workspace(&n->core, "jh_r2d2net", (size_t)8 << 20, 8192);
  if (!rc) rc = core_drain();
  if (rc) {
    core_release(&n->core);
    delete n;
    return rc;
  }
  *out = n;
  return JH_OK;
}

JH_EXPORT void jh_r2d2net_destroy(jh_r2d2net* n) {
  if (!n) return;
  core_release(&n->core);
  delete n;
}
JH_EXPORT int32_t jh_r2d2net_segment_count(void) { return R2_SEG_COUNT; }
JH_EXPORT int jh_r2d2net_segment(const jh_r2d2net* n, int32_t i, int64_t* offset, int32_t* rows, int32_t* cols) {
  return seg_query(n, R2_SEG_COUNT, i, offset, rows, cols);
}
JH_EXPORT int jh_r2d2net_set_hyper(jh_r2d2net* n, double lr, double beta1, double beta2, double eps, int64_t step, jh_stream stream) {
  JH_ARG(n != nullptr);
  return jh_hyper_upload(n->core.ctx, n->opt.hyper, lr, beta1, beta2, eps, step, 0, jh_s(stream));
}
JH_EXPORT int jh_r2d2net_set_lr(jh_r2d2net* n, double lr, jh_stream stream) {
  JH_ARG(n != nullptr);
  return jh_hyper_upload_lr(n->core.ctx, n->opt.hyper, lr, jh_s(stream));
}
JH_EXPORT int jh_r2d2net_sync_target(jh_r2d2net* n, jh_stream stream) {
  JH_ARG(n != nullptr);
  JH_HIP(hipMemcpyAsync(n->target, n->params, sizeof(float) * (size_t)n->n_params, hipMemcpyDeviceToDevice, jh_s(stream)));
  return JH_OK;
}

// The layers above the LSTM for `np` row ranges (parameter set P[j], LSTM outputs h[j], `rows` rows each) whose activations sit one after
// the other in hl / hav / adv / val from row 0: l, l1_a | l1_v, l2_a and l2_v as one grouped launch each, then the dueling combine -> q.
static int r2_heads(jh_r2d2net* n, int np, const float* const* P, const float* const* h, int rows, float* q, hipStream_t st, bool acting = false) {
  const int H = n->H, A = n->A;
  float *b_hl = acting ? n->a_hl : n->hl, *b_hav = acting ? n->a_hav : n->hav, *b_adv = acting ? n->a_adv : n->adv, *b_val = acting ? n->a_val : n->val;
  TGemm g[6];
  int rc;
  for (int j = 0; j < np; ++j)
    g[j] = mk_gemm(rows, H, H, op_dense(OP_KCONT, h[j], H), op_dense(OP_KCONT, P[j] + n->seg_off[R2_WL], H), b_hl + (size_t)j * rows * H, H, TEPI_BIAS_RELU,
                   P[j] + n->seg_off[R2_BL]);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, np, st))) return rc;
  for (int j = 0; j < np; ++j)
    g[j] = mk_gemm(rows, 2 * H, H, op_dense(OP_KCONT, b_hl + (size_t)j * rows * H, H), op_dense(OP_KCONT, P[j] + n->seg_off[R2_WA1], H),
                   b_hav + (size_t)j * rows * 2 * H, 2 * H, TEPI_BIAS_RELU, P[j] + n->seg_off[R2_BA1]);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, np, st))) return rc;
  for (int j = 0; j < np; ++j) {
    const float* hav = b_hav + (size_t)j * rows * 2 * H;
    g[2 * j] = mk_gemm(rows, A, H, op_dense(OP_KCONT, hav, 2 * H), op_dense(OP_KCONT, P[j] + n->seg_off[R2_WA2], H), b_adv + (size_t)j * rows * A, A, TEPI_BIAS,
                       P[j] + n->seg_off[R2_BA2]);
    g[2 * j + 1] = mk_gemm(rows, 1, H, op_dense(OP_KCONT, hav + H, 2 * H), op_dense(OP_KCONT, P[j] + n->seg_off[R2_WV2], H), b_val + (size_t)j * rows, 1, TEPI_BIAS,
                           P[j] + n->seg_off[R2_BV2]);
  }
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 2 * np, st))) return rc;
  const int64_t total = (int64_t)np * rows;
  JH_LAUNCH(jh_r2d2_duel_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, total, A, b_adv, b_val, q);
  JH_LAUNCH_CHECK();
  return JH_OK;
}

// The three sequence passes of R2D2.learn() (r2d2.py:117-129, get_q r2d2.py:289-302) in lockstep, seq_len step launches of three row
// segments: online over steps [0, seq_len) from `hidden`, online and target over steps [n_step, n_step + seq_len) from `next_hidden`.  The
// head and the input projection of the online network run ONCE over all seq_len + n_step stored steps: the second pass reads the first
// one's projection n_step rows further on.  d_q [3][T'][B][A] time-major over the T' = seq_len - n_burn_in trained steps.
JH_EXPORT int jh_r2d2net_learn_forward(jh_r2d2net* n, const float* d_state, const float* d_onehot, const float* d_hidden_h, const float* d_hidden_c,
                                       const float* d_next_hidden_h, const float* d_next_hidden_c, int32_t B, float* d_q, jh_stream stream) {
  JH_ARG(n && d_state && d_onehot && d_hidden_h && d_hidden_c && d_next_hidden_h && d_next_hidden_c && d_q);
  JH_ARG(B >= 1 && B <= n->maxB);
  hipStream_t st = jh_s(stream);
  const int S = n->S, H = n->H, A = n->A, T = n->T, burn = n->burn, ns = n->n_step, L = T + ns, Tt = T - burn, X = H + A;
  const float* P[2] = {n->params, n->target};
  n->last_B = 0;
  PrepArgs pa{};
  pa.B = B; pa.L = L; pa.S = S; pa.A = A; pa.H = H; pa.T = T; pa.state = d_state; pa.onehot = d_onehot;
  pa.hid[0] = d_hidden_h; pa.hid[1] = d_hidden_c; pa.hid[2] = d_next_hidden_h; pa.hid[3] = d_next_hidden_c;
  for (int w = 0; w < 2; ++w) {
    pa.bih[w] = P[w] + n->seg_off[R2_BIH]; pa.bhh[w] = P[w] + n->seg_off[R2_BHH]; pa.xin[w] = n->xin[w]; pa.bsum[w] = n->bsum[w];
  }
  pa.x_tm = n->x_tm; pa.hseq = n->hseq; pa.cseq = n->cseq;
  const int64_t work = (int64_t)L * B * (S > A ? S : A);
  JH_LAUNCH(jh_r2d2_prep_kernel, dim3((unsigned)((work + 255) / 256 < 1024 ? (work + 255) / 256 : 1024)), dim3(256), 0, st, pa);
  JH_LAUNCH_CHECK();
  TGemm g[2];
  int rc;
  // the target network only ever sees the steps from n_step on
  const size_t r0[2] = {0, (size_t)ns * B};
  const int rows[2] = {L * B, T * B};
  for (int w = 0; w < 2; ++w)
    g[w] = mk_gemm(rows[w], H, S, op_dense(OP_KCONT, n->x_tm + r0[w] * S, S), op_dense(OP_KCONT, P[w] + n->seg_off[R2_W1], S), n->xin[w] + r0[w] * X, X, TEPI_BIAS_RELU,
                   P[w] + n->seg_off[R2_B1]);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 2, st))) return rc;
  for (int w = 0; w < 2; ++w)
    g[w] = mk_gemm(rows[w], 4 * H, X, op_dense(OP_KCONT, n->xin[w] + r0[w] * X, X), op_dense(OP_KCONT, P[w] + n->seg_off[R2_WIH], X), n->xp[w] + r0[w] * 4 * H, 4 * H,
                   TEPI_BIAS, n->bsum[w]);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 2, st))) return rc;
  const size_t slab = (size_t)(T + 1) * B * H, BH = (size_t)B * H;
  for (int t = 0; t < T; ++t) {
    jh_lstm_seg seg[3];
    for (int p = 0; p < 3; ++p) {
      const int w = p == 2, tx = p == 0 ? t : t + ns;
      seg[p].rows = B; seg[p].ld_x = 4 * H;
      seg[p].xproj = n->xp[w] + (size_t)tx * B * 4 * H;
      seg[p].w_hh = P[w] + n->seg_off[R2_WHH];
      seg[p].h_prev = n->hseq + p * slab + t * BH; seg[p].c_prev = n->cseq + p * slab + t * BH;
      seg[p].h_out = n->hseq + p * slab + (t + 1) * BH; seg[p].c_out = n->cseq + p * slab + (t + 1) * BH;
      seg[p].gates_out = (p == 0 && t >= burn) ? n->gates + (size_t)(t - burn) * B * 4 * H : nullptr;
    }
    if ((rc = jh_lstm_step(n->core.ctx, H, 3, seg, stream))) return rc;
  }
  const float* Ph[3] = {n->params, n->params, n->target};
  const float* hh[3];
  for (int p = 0; p < 3; ++p) hh[p] = n->hseq + p * slab + (size_t)(burn + 1) * BH;
  if ((rc = r2_heads(n, 3, Ph, hh, Tt * B, d_q, st))) return rc;
  n->last_B = B;
  return JH_OK;
}

// Backward of q[0] (the online pass over state[:, :seq_len]) of the last jh_r2d2net_learn_forward: d_g = d(loss)/dq [T'][B][A]; fills the
// gradient bucket.  The burn-in steps hand over (h, c) without gradient (r2d2.py:290-295): the walk stops at step n_burn_in.
JH_EXPORT int jh_r2d2net_backward(jh_r2d2net* n, const float* d_g, jh_stream stream) {
  JH_ARG(n && d_g);
  if (!n->last_B) return jh_fail(JH_ERR_STATE, "jh_r2d2net_backward without a preceding jh_r2d2net_learn_forward");
  hipStream_t st = jh_s(stream);
  const int B = n->last_B, S = n->S, H = n->H, A = n->A, T = n->T, burn = n->burn, Tt = T - burn, R = Tt * B, X = H + A;
  const float* P = n->params;
  float* G = n->grads;
  const size_t BH = (size_t)B * H;
  const float* hav = n->hav;  // pass 0's activations are the first R rows of every buffer
  TGemm g[4];
  int rc;
  JH_LAUNCH(jh_r2d2_duel_bwd_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, (int64_t)R, A, d_g, n->dadv, n->dval);
  JH_LAUNCH_CHECK();
  // l2_a, l2_v: weight gradients (bias gradients as row sums), data gradients through relu' of l1_a | l1_v into the two halves of dhav
  g[0] = mk_gemm(A, H, R, op_dense(OP_XCONT, n->dadv, A), op_dense(OP_XCONT, hav, 2 * H), G + n->seg_off[R2_WA2], H, TEPI_NONE, nullptr, nullptr, 0, G + n->seg_off[R2_BA2]);
  g[1] = mk_gemm(1, H, R, op_dense(OP_XCONT, n->dval, 1), op_dense(OP_XCONT, hav + H, 2 * H), G + n->seg_off[R2_WV2], H, TEPI_NONE, nullptr, nullptr, 0, G + n->seg_off[R2_BV2]);
  g[2] = mk_gemm(R, H, A, op_dense(OP_KCONT, n->dadv, A), op_dense(OP_XCONT, P + n->seg_off[R2_WA2], H), n->dhav, 2 * H, TEPI_MASK, nullptr, hav, 2 * H);
  g[3] = mk_gemm(R, H, 1, op_dense(OP_KCONT, n->dval, 1), op_dense(OP_XCONT, P + n->seg_off[R2_WV2], H), n->dhav + H, 2 * H, TEPI_MASK, nullptr, hav + H, 2 * H);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 4, st))) return rc;
  g[0] = mk_gemm(2 * H, H, R, op_dense(OP_XCONT, n->dhav, 2 * H), op_dense(OP_XCONT, n->hl, H), G + n->seg_off[R2_WA1], H, TEPI_NONE, nullptr, nullptr, 0, G + n->seg_off[R2_BA1]);
  g[1] = mk_gemm(R, H, 2 * H, op_dense(OP_KCONT, n->dhav, 2 * H), op_dense(OP_XCONT, P + n->seg_off[R2_WA1], H), n->dhl, H, TEPI_MASK, nullptr, n->hl, H);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 2, st))) return rc;
  const float* h_tr = n->hseq + (size_t)(burn + 1) * BH;  // h_t of the trained steps
  g[0] = mk_gemm(H, H, R, op_dense(OP_XCONT, n->dhl, H), op_dense(OP_XCONT, h_tr, H), G + n->seg_off[R2_WL], H, TEPI_NONE, nullptr, nullptr, 0, G + n->seg_off[R2_BL]);
  g[1] = mk_gemm(R, H, H, op_dense(OP_KCONT, n->dhl, H), op_dense(OP_XCONT, P + n->seg_off[R2_WL], H), n->dh, H, TEPI_NONE);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 2, st))) return rc;
  // backpropagation through time: one launch per trained step
  for (int t = T - 1; t >= burn; --t) {
    const int k = t - burn;
    const bool last = t == T - 1;
    if ((rc = jh_lstm_step_backward(n->core.ctx, B, H, last ? nullptr : n->dgates + (size_t)(k + 1) * B * 4 * H, P + n->seg_off[R2_WHH], n->dh + (size_t)k * BH,
                                    last ? nullptr : n->dc[(k + 1) & 1], n->gates + (size_t)k * B * 4 * H, n->cseq + (size_t)t * BH, n->cseq + (size_t)(t + 1) * BH,
                                    n->dgates + (size_t)k * B * 4 * H, n->dc[k & 1], stream)))
      return rc;
  }
  // over all trained steps at once: dW_hh (+ db_ih), dW_ih, dx through relu' of the head
  const float* xin_tr = n->xin[0] + (size_t)burn * B * X;
  g[0] = mk_gemm(4 * H, H, R, op_dense(OP_XCONT, n->dgates, 4 * H), op_dense(OP_XCONT, n->hseq + (size_t)burn * BH, H), G + n->seg_off[R2_WHH], H, TEPI_NONE, nullptr, nullptr,
                 0, G + n->seg_off[R2_BIH]);
  g[1] = mk_gemm(4 * H, X, R, op_dense(OP_XCONT, n->dgates, 4 * H), op_dense(OP_XCONT, xin_tr, X), G + n->seg_off[R2_WIH], X, TEPI_NONE);
  g[2] = mk_gemm(R, H, 4 * H, op_dense(OP_KCONT, n->dgates, 4 * H), op_dense(OP_XCONT, P + n->seg_off[R2_WIH], X), n->dx, H, TEPI_MASK, nullptr, xin_tr, X);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 3, st))) return rc;
  // bias_ih_l0 and bias_hh_l0 are two parameters with one gradient
  JH_HIP(hipMemcpyAsync(G + n->seg_off[R2_BHH], G + n->seg_off[R2_BIH], sizeof(float) * 4 * (size_t)H, hipMemcpyDeviceToDevice, st));
  g[0] = mk_gemm(H, S, R, op_dense(OP_XCONT, n->dx, H), op_dense(OP_XCONT, n->x_tm + (size_t)burn * B * S, S), G + n->seg_off[R2_W1], S, TEPI_NONE, nullptr, nullptr, 0,
                 G + n->seg_off[R2_B1]);
  return core_tgemm(&n->core, "jh_tgemm_dense", g, 1, st);
}

JH_EXPORT int jh_r2d2net_optim_step(jh_r2d2net* n, float max_norm, jh_stream stream) {
  JH_ARG(n != nullptr);
  return jh_flat_adam_step(n->n_params, n->params, n->grads, n->m, n->v, n->opt.hyper, n->opt.ticket, n->core.norm_partial, max_norm, jh_s(stream));
}

// R2D2.act (r2d2.py:62-66): ONE step of the online network for N <= max_batch actor rows.  d_x [N][S], d_prev_onehot [N][A] (zeros at an
// episode start), the carried state d_h_in / d_c_in [N][H] -> d_q [N][A] and the state going out, all on the device.  Its buffers
// are its own: it may run between a learn_forward and its backward.
JH_EXPORT int jh_r2d2net_act_step(jh_r2d2net* n, const float* d_x, const float* d_prev_onehot, const float* d_h_in, const float* d_c_in, int32_t N,
                                  float* d_q, float* d_h_out, float* d_c_out, jh_stream stream) {
  JH_ARG(n && d_x && d_prev_onehot && d_h_in && d_c_in && d_q && d_h_out && d_c_out);
  JH_ARG(N >= 1 && N <= n->maxB && aligned16(d_h_in));
  hipStream_t st = jh_s(stream);
  const int S = n->S, H = n->H, A = n->A, X = H + A;
  const float* P = n->params;
  PrepArgs pa{};  // one stored step of N rows: the one-hot columns and b_ih + b_hh; no hidden state to place
  pa.B = N; pa.L = 1; pa.S = 0; pa.A = A; pa.H = H; pa.T = 0; pa.onehot = d_prev_onehot;
  for (int w = 0; w < 2; ++w) { pa.bih[w] = P + n->seg_off[R2_BIH]; pa.bhh[w] = P + n->seg_off[R2_BHH]; pa.xin[w] = n->a_xin; pa.bsum[w] = n->a_bsum; }
  JH_LAUNCH(jh_r2d2_prep_kernel, dim3(16), dim3(256), 0, st, pa);
  JH_LAUNCH_CHECK();
  TGemm g[1];
  int rc;
  g[0] = mk_gemm(N, H, S, op_dense(OP_KCONT, d_x, S), op_dense(OP_KCONT, P + n->seg_off[R2_W1], S), n->a_xin, X, TEPI_BIAS_RELU, P + n->seg_off[R2_B1]);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 1, st))) return rc;
  g[0] = mk_gemm(N, 4 * H, X, op_dense(OP_KCONT, n->a_xin, X), op_dense(OP_KCONT, P + n->seg_off[R2_WIH], X), n->a_xp, 4 * H, TEPI_BIAS, n->a_bsum);
  if ((rc = core_tgemm(&n->core, "jh_tgemm_dense", g, 1, st))) return rc;
  jh_lstm_seg seg{};
  seg.rows = N; seg.ld_x = 4 * H; seg.xproj = n->a_xp; seg.w_hh = P + n->seg_off[R2_WHH]; seg.h_prev = d_h_in; seg.c_prev = d_c_in;
  seg.h_out = d_h_out; seg.c_out = d_c_out; seg.gates_out = nullptr;
  if ((rc = jh_lstm_step(n->core.ctx, H, 1, &seg, stream))) return rc;
  const float* hh[1] = {d_h_out};
  return r2_heads(n, 1, &P, hh, N, d_q, st, true);
}
