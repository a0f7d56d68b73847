// Batched recurrent actors for R2D2: the epilogue of an acting tick and interact_callback (core/agent/r2d2.py:179-287) for N lockstep actors,
// with the carried LSTM state, the previous action's one-hot, the per-actor sequence windows and the actor-side priorities kept in HBM.
//
// Reference: every actor is a process; per env step R2D2.act() returns q, hidden_h, hidden_c and the action to the host, interact_callback
// appends them to a deque(maxlen = n_step + seq_len), and every store_period steps (and at once after an episode start) stacks the deque
// into one stored row -- zero-padded at the front while the window is short -- and folds the actor-side priority from the stacked q.
//
// Here, per tick and for all N actors:
//   jh_r2d2net_act_step      (csrc/jh_r2d2.hip) reads h / c slot p and the fed one-hot, writes q and h / c slot 1 - p (p = tick & 1): the
//                            carried state ping-pongs between two slots, so "carry h and c" is no copy at all
//   jh_r2d2_actors_act       one lane per actor decides (first-maximum argmax, epsilon-greedy with the host's draws, jh_value_act's rules) and
//                            publishes q then the action to device-mapped host memory; then 16 lanes per actor copy the tick's record
//                            (observation, fed one-hot, h_in, c_in, q taken, action) into the actor's window ring, float4 where aligned
//   jh_r2d2_actors_emit      one workgroup per actor: append (reward, done), test the emit condition, assemble the stored row straight from
//                            the ring, fold the priority in double, truncate after an episode end, zero the carried state after `done`
// Only the N actions, the N q values and one row count cross PCIe downwards; the N rewards and done flags come up.
//
// Ring layout: PER-ACTOR CONTIGUOUS, one ring per field ([N][L][S] observations, [N][L][A] one-hots, [N][L][H] h, [N][L][H] c, [N][L][4]
// {q, action, reward, done}; L = n_step + seq_len).  The emit kernel reads ALL ticks of ONE actor: with this layout a window is at most two
// contiguous runs (the ring's wrap) of L * S floats that map one to one onto the contiguous output row, so consecutive lanes read and write
// consecutive float4s.  The act kernel writes ONE tick of ALL actors; a tick-major layout would put those N records next to each other, but
// each record is written by its own lane group as a run of S / A / H floats either way -- the runs are as long in both layouts and the act
// kernel gains nothing from their being adjacent, while the emit kernel would pay a stride of N * S floats between the ticks of its window.
//
// Compaction: emitted rows are stored in ascending actor order at cursor + (number of emitters among the actors below).  Whether an actor
// emits at this tick depends on its state block only ({len, head, store_start, stamp} BEFORE the tick), never on the tick's reward or done.
// The state blocks and the row cursor are double-buffered by tick parity (read p, write 1 - p), so every workgroup can evaluate the flags of
// the actors below it from the read side while their owners write the other side: the prefix is a first phase of the SAME launch (wave 0,
// 64 flags per ballot, popcount), no grid barrier and no second launch (a launch costs more than the <= 16 ballots it would save).
// The workgroup of the last actor writes the new cursor and the row count to mapped host memory: it arrives with the next tick's actions.
//
// One thread drives an object: act and emit of a tick, and save / load, must come from the same host thread (nothing here is locked).
// No floating-point atomics; the max and the mean of |td| are taken by one thread over LDS in index order.  Plain vector stores only.
#include "jh_common.h"

namespace {
constexpr int kMaxWindow = 160;   // seq_len + n_step: the learner's seq_len <= 128 plus headroom for n_step
constexpr int kMaxActors = 1024;
constexpr int kMaxActions = 64;
constexpr int kActGroup = 16;     // actors per workgroup of the act kernel: 16 lanes copy one actor's record
enum { ST_LEN = 0, ST_HEAD = 1, ST_START = 2, ST_STAMP = 3, ST_INTS = 4 };
enum { SC_Q = 0, SC_ACTION = 1, SC_REWARD = 2, SC_DONE = 3, SC_FLOATS = 4 };

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the rescales of jh_r2d2_loss (csrc/jh_r2d2.hip), in double and without their cancellations
__device__ __forceinline__ double val_rescale(double x, double eps) {
  const double ax = fabs(x);
  return (x / (ax + 1e-10)) * (ax / (sqrt(ax + 1.0) + 1.0)) + eps * x;
}
__device__ __forceinline__ double inv_val_rescale(double x, double eps) {
  const double ax = fabs(x);
  const double y = 4.0 * eps * (ax + 1.0 + eps), sq = sqrt(1.0 + y);
  const double u = 2.0 * (ax + 1.0 + eps) / (sq + 1.0);
  return (x / (ax + 1e-10)) * (u * u - 1.0);
}

// n floats by `nt` cooperating lanes (lane `t` of them); vec: n % 4 == 0 and both rows 16-byte aligned
__device__ __forceinline__ void copy_row(float* __restrict__ dst, const float* __restrict__ src, int n, bool vec, int t, int nt) {
  if (vec) {
    for (int i = t; i < (n >> 2); i += nt) reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[i];
  } else {
    for (int i = t; i < n; i += nt) dst[i] = src[i];
  }
}

struct ActArgs {
  int N, S, A, H, L;
  int obs_vec;
  const int32_t* st;  // [N][4], this tick's side
  const float *q, *obs, *h_in, *c_in;
  float* onehot;      // [N][A]: in the one-hot fed this tick, out the next tick's
  float *r_obs, *r_oh, *r_h, *r_c, *r_sc;
  const float* eps;
  const double* u;
  const int64_t* rand_action;
  int64_t* action;    // [N] device-mapped host memory
  float* q_taken;     // [N] device-mapped host memory
};

__global__ void __launch_bounds__(256) jh_r2d2_actors_act_kernel(ActArgs g) {
  __shared__ int s_slot[kActGroup];
  const int tid = threadIdx.x, a0 = blockIdx.x * kActGroup;
  const int A = g.A, L = g.L;
  if (tid < kActGroup) {  // one lane per actor
    const int a = a0 + tid;
    int slot = -1;
    if (a < g.N) {
      const int len = g.st[a * ST_INTS + ST_LEN], head = g.st[a * ST_INTS + ST_HEAD];
      slot = len < L ? (head + len) % L : head;  // a full deque drops its oldest entry: the new one takes its place
      const float* q = g.q + (size_t)a * A;
      float best = q[0];
      int act = 0;
      for (int k = 1; k < A; ++k)
        if (q[k] > best) { best = q[k]; act = k; }  // first maximum, like torch.argmax
      float qt = best;
      if (g.eps && g.u[a] < (double)g.eps[a]) {
        int ra = (int)g.rand_action[a];
        ra = ra < 0 ? 0 : (ra >= A ? A - 1 : ra);
        act = ra;
        qt = q[ra];
      }
      g.q_taken[a] = qt;
      __threadfence_system();  // payload before the arrival mark (mapped host memory, jh_host_wait_words)
      g.action[a] = act;
      float* oh = g.onehot + (size_t)a * A;
      float* roh = g.r_oh + ((size_t)a * L + slot) * A;
      for (int k = 0; k < A; ++k) {
        roh[k] = oh[k];
        oh[k] = k == act ? 1.f : 0.f;
      }
      float* sc = g.r_sc + ((size_t)a * L + slot) * SC_FLOATS;
      sc[SC_Q] = qt;
      sc[SC_ACTION] = (float)act;
    }
    s_slot[tid] = slot;
  }
  __syncthreads();
  const int i = tid >> 4, t = tid & 15, a = a0 + i, slot = s_slot[i];
  if (slot < 0) return;
  const size_t rec = (size_t)a * L + slot;
  copy_row(g.r_obs + rec * g.S, g.obs + (size_t)a * g.S, g.S, g.obs_vec != 0, t, 16);
  copy_row(g.r_h + rec * g.H, g.h_in + (size_t)a * g.H, g.H, true, t, 16);
  copy_row(g.r_c + rec * g.H, g.c_in + (size_t)a * g.H, g.H, true, t, 16);
}

struct EmitArgs {
  int N, S, A, H, L, seq, burn, n, period, pad, restart;
  double gamma, eta, eps;
  const int32_t* st_in;
  int32_t* st_out;
  const int64_t* cur_in;
  int64_t* cur_out;
  int64_t cap;
  const float *h_rew, *h_done;  // [N] device-visible pinned memory
  const float *r_obs, *r_oh, *r_h, *r_c;
  float* r_sc;
  float *onehot, *h_next, *c_next;  // the carried state the next tick reads
  float *o_state, *o_oh, *o_action, *o_reward, *o_done, *o_hh, *o_hc, *o_nhh, *o_nhc;
  double* o_prio;
  int64_t* count;  // device-mapped host memory
};

__device__ __forceinline__ bool emits(const EmitArgs& g, int b) {
  const int32_t* s = g.st_in + (size_t)b * ST_INTS;
  const int len1 = s[ST_LEN] < g.L ? s[ST_LEN] + 1 : g.L;
  const bool due = s[ST_START] != 0 || s[ST_STAMP] == g.period;
  return due && (g.pad ? len1 >= g.n + 1 : len1 == g.L);
}

// ring [L][W] of one actor -> row [L][W]: `lack` zero ticks in front, then the window from `head`; lanes over (tick, feature)
__device__ __forceinline__ void copy_window(float* __restrict__ dst, const float* __restrict__ ring, int W, int L, int head, int lack, bool vec,
                                            int tid, int nt) {
  if (vec) {
    const int W4 = W >> 2;
    for (int e = tid; e < L * W4; e += nt) {
      const int j = e / W4, f = e - j * W4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (j >= lack) v = reinterpret_cast<const float4*>(ring + (size_t)((head + j - lack) % L) * W)[f];
      reinterpret_cast<float4*>(dst)[e] = v;
    }
  } else {
    for (int e = tid; e < L * W; e += nt) {
      const int j = e / W, f = e - j * W;
      dst[e] = j >= lack ? ring[(size_t)((head + j - lack) % L) * W + f] : 0.f;
    }
  }
}

__global__ void __launch_bounds__(256) jh_r2d2_actors_emit_kernel(EmitArgs g) {
  __shared__ int s_i[4];  // len, head (after the append), emit, emitters below
  __shared__ float s_q[kMaxWindow], s_r[kMaxWindow], s_d[kMaxWindow];
  __shared__ double s_td[kMaxWindow];
  const int tid = threadIdx.x, a = blockIdx.x, L = g.L, n = g.n;
  // ---- phase 1: how many of the actors below emit at this tick (wave 0; the flags come from the read side of the state blocks)
  if (tid < 64) {
    int below = 0;
    for (int b0 = 0; b0 < a; b0 += 64) {
      const int b = b0 + tid;
      below += __popcll(__ballot(b < a && emits(g, b)));
    }
    if (tid == 0) {
      const int32_t* s = g.st_in + (size_t)a * ST_INTS;
      int len = s[ST_LEN], head = s[ST_HEAD];
      const int w = len < L ? (head + len) % L : head;  // where the act kernel put this tick's record
      float* sc = g.r_sc + ((size_t)a * L + w) * SC_FLOATS;
      sc[SC_REWARD] = g.h_rew[a];
      sc[SC_DONE] = g.h_done[a];
      if (len < L) ++len; else head = (head + 1) % L;
      s_i[0] = len; s_i[1] = head; s_i[2] = emits(g, a) ? 1 : 0; s_i[3] = below;
    }
  }
  __syncthreads();
  int len = s_i[0], head = s_i[1];
  const bool emit = s_i[2] != 0;
  const int64_t base = g.restart ? 0 : g.cur_in[0];
  const int64_t row = base + s_i[3];
  if (a == g.N - 1 && tid == 0) {
    const int64_t total = row + (emit ? 1 : 0);
    g.cur_out[0] = total;
    g.count[0] = total;  // over `capacity`: the rows beyond it were not written, the host reports it
  }
  if (emit && row < g.cap) {  // a row beyond the capacity is never written; the count above tells the host
    // ---- phase 2: the stored row, straight from the ring
    const int lack = L - len;
    const size_t ar = (size_t)a * L;
    copy_window(g.o_state + (size_t)row * L * g.S, g.r_obs + ar * g.S, g.S, L, head, lack, (g.S & 3) == 0, tid, 256);
    copy_window(g.o_oh + (size_t)row * L * g.A, g.r_oh + ar * g.A, g.A, L, head, lack, (g.A & 3) == 0, tid, 256);
    for (int j = tid; j < L; j += 256) {
      float4 sc = make_float4(0.f, 0.f, 0.f, 0.f);
      if (j >= lack) sc = reinterpret_cast<const float4*>(g.r_sc)[ar + (head + j - lack) % L];
      s_q[j] = sc.x; s_r[j] = sc.z; s_d[j] = sc.w;
      if (j < L - 1) {
        const size_t o = (size_t)row * (L - 1) + j;
        g.o_action[o] = sc.y; g.o_reward[o] = sc.z; g.o_done[o] = sc.w;
      }
    }
    const int k = lack > n ? 0 : n - lack;  // r2d2.py:229-232; n when the window is full
    const size_t first = (ar + head) * g.H, next = (ar + (head + k) % L) * g.H, o = (size_t)row * g.H;
    copy_row(g.o_hh + o, g.r_h + first, g.H, true, tid, 256);
    copy_row(g.o_hc + o, g.r_c + first, g.H, true, tid, 256);
    copy_row(g.o_nhh + o, g.r_h + next, g.H, true, tid, 256);
    copy_row(g.o_nhc + o, g.r_c + next, g.H, true, tid, 256);
    __syncthreads();
    // ---- the actor-side priority (r2d2.py:234-262) over the trained steps, one lane per step
    const int T = g.seq - g.burn;
    if (tid < T) {
      double tq = inv_val_rescale((double)s_q[g.burn + n + tid], g.eps);
      for (int i = n - 1; i >= 0; --i) tq = (double)s_r[i + g.burn + tid] + (1.0 - (double)s_d[i + g.burn + tid]) * g.gamma * tq;
      s_td[tid] = fabs(val_rescale(tq, g.eps) - (double)s_q[g.burn + tid]);
    }
    __syncthreads();
    if (tid == 0) {
      double mx = 0.0, sum = 0.0;
      for (int t = 0; t < T; ++t) { mx = fmax(mx, s_td[t]); sum += s_td[t]; }
      g.o_prio[row] = g.eta * mx + (1.0 - g.eta) * (sum / (double)T);
    }
  }
  // ---- the rest of the state machine (r2d2.py:264-275)
  if (tid == 0) {
    const int32_t* s = g.st_in + (size_t)a * ST_INTS;
    int start = s[ST_START], stamp = s[ST_STAMP];
    if (emit) { start = 0; stamp -= g.period; }
    if (len > n && g.r_sc[((size_t)a * L + (head + len - n - 1) % L) * SC_FLOATS + SC_DONE] != 0.f) {
      start = 1;
      head = (head + len - n) % L;
      len = n;
    }
    int32_t* so = g.st_out + (size_t)a * ST_INTS;
    so[ST_LEN] = len; so[ST_HEAD] = head; so[ST_START] = start; so[ST_STAMP] = stamp + 1;
  }
  if (g.h_done[a] != 0.f) {  // the next tick starts an episode: no carried state, no previous action
    for (int i = tid; i < g.H; i += 256) g.h_next[(size_t)a * g.H + i] = g.c_next[(size_t)a * g.H + i] = 0.f;
    for (int i = tid; i < g.A; i += 256) g.onehot[(size_t)a * g.A + i] = 0.f;
  }
}
}  // namespace

struct jh_r2d2_actors {
  jh_ctx* ctx = nullptr;
  int N = 0, S = 0, A = 0, H = 0, L = 0, seq = 0, burn = 0, n = 0, period = 0, pad = 0;
  double gamma = 0.0, eta = 0.0, eps = 1e-3;
  int64_t tick = 0;
  bool acted = false;  // this tick's record is in (jh_r2d2_actors_act), jh_r2d2_actors_emit closes the tick
  void* block = nullptr;
  size_t block_bytes = 0;
  int32_t* st = nullptr;                    // [2][N][4]
  int64_t* cur = nullptr;                   // [2]
  float *onehot = nullptr, *h = nullptr, *c = nullptr;  // h, c: [2][N][H]
  float *r_obs = nullptr, *r_oh = nullptr, *r_h = nullptr, *r_c = nullptr, *r_sc = nullptr;
};

JH_EXPORT int jh_r2d2_actors_create(jh_ctx* ctx, int32_t n_actors, int32_t S, int32_t A, int32_t H, int32_t seq_len, int32_t n_burn_in, int32_t n_step,
                                    int32_t store_period, int32_t zero_padding, double gamma, double eta, jh_r2d2_actors** out) {
  JH_ARG(ctx && out);
  if (n_actors < 1 || n_actors > kMaxActors) return jh_fail(JH_ERR_ARG, "jh_r2d2_actors_create: n_actors = %d is outside 1..%d", n_actors, kMaxActors);
  if (A < 2 || A > kMaxActions) return jh_fail(JH_ERR_ARG, "jh_r2d2_actors_create: action_size = %d is outside 2..%d", A, kMaxActions);
  if (seq_len < 1 || n_step < 1 || seq_len + n_step > kMaxWindow)
    return jh_fail(JH_ERR_ARG, "jh_r2d2_actors_create: seq_len + n_step = %d + %d is over %d (or one of them is below 1)", seq_len, n_step, kMaxWindow);
  JH_ARG(S >= 1 && H >= 4 && H % 4 == 0 && H <= 4096 && n_burn_in >= 0 && n_burn_in < seq_len && store_period >= 0);
  jh_r2d2_actors* f = new jh_r2d2_actors();
  f->ctx = ctx; f->N = n_actors; f->S = S; f->A = A; f->H = H; f->L = seq_len + n_step; f->seq = seq_len; f->burn = n_burn_in; f->n = n_step;
  f->period = store_period; f->pad = zero_padding != 0; f->gamma = gamma; f->eta = eta;
  const size_t N = n_actors, L = f->L;
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t b_st = up(sizeof(int32_t) * 2 * N * ST_INTS), b_cur = 256, b_oh = up(sizeof(float) * N * A), b_hc = up(sizeof(float) * 2 * N * H),
               b_ro = up(sizeof(float) * N * L * S), b_ra = up(sizeof(float) * N * L * A), b_rh = up(sizeof(float) * N * L * H),
               b_rs = up(sizeof(float) * N * L * SC_FLOATS);
  const size_t total = b_st + b_cur + b_oh + 2 * b_hc + b_ro + b_ra + 2 * b_rh + b_rs;
  f->block_bytes = total;
  hipError_t e = hipMalloc(&f->block, total);
  if (e == hipSuccess) e = hipMemset(f->block, 0, total);
  std::vector<int32_t> st0(2 * N * ST_INTS, 0);
  for (size_t i = 0; i < 2 * N; ++i) st0[i * ST_INTS + ST_START] = 1;  // r2d2.py:44: store_start = True
  if (e == hipSuccess) e = hipMemcpy(f->block, st0.data(), sizeof(int32_t) * st0.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (f->block) (void)hipFree(f->block);
    delete f;
    return jh_fail(JH_ERR_HIP, "jh_r2d2_actors_create: %zu bytes of device memory -> %s", total, hipGetErrorString(e));
  }
  char* p = static_cast<char*>(f->block);
  f->st = reinterpret_cast<int32_t*>(p); p += b_st;
  f->cur = reinterpret_cast<int64_t*>(p); p += b_cur;
  f->onehot = reinterpret_cast<float*>(p); p += b_oh;
  f->h = reinterpret_cast<float*>(p); p += b_hc;
  f->c = reinterpret_cast<float*>(p); p += b_hc;
  f->r_obs = reinterpret_cast<float*>(p); p += b_ro;
  f->r_oh = reinterpret_cast<float*>(p); p += b_ra;
  f->r_h = reinterpret_cast<float*>(p); p += b_rh;
  f->r_c = reinterpret_cast<float*>(p); p += b_rh;
  f->r_sc = reinterpret_cast<float*>(p);
  *out = f;
  return JH_OK;
}

JH_EXPORT void jh_r2d2_actors_destroy(jh_r2d2_actors* f) {
  if (!f) return;
  if (f->block) (void)hipFree(f->block);
  delete f;
}

// The carried state of the tick that is about to act: jh_r2d2net_act_step reads h_in / c_in / onehot and writes h_out / c_out.
JH_EXPORT int jh_r2d2_actors_carried(jh_r2d2_actors* f, float** h_in, float** c_in, float** h_out, float** c_out, float** onehot) {
  JH_ARG(f && h_in && c_in && h_out && c_out && onehot);
  const size_t p = (size_t)(f->tick & 1), NH = (size_t)f->N * f->H;
  *h_in = f->h + p * NH; *c_in = f->c + p * NH; *h_out = f->h + (1 - p) * NH; *c_out = f->c + (1 - p) * NH; *onehot = f->onehot;
  return JH_OK;
}

JH_EXPORT int jh_r2d2_actors_act(jh_r2d2_actors* f, const float* d_q, const float* d_obs, const float* d_h_in, const float* d_c_in, const float* h_eps,
                                 const double* h_u, const int64_t* h_rand_action, int64_t* d_action, float* d_q_taken, jh_stream stream) {
  JH_ARG(f && d_q && d_obs && d_h_in && d_c_in && d_action && d_q_taken);
  JH_ARG((h_eps == nullptr) == (h_u == nullptr) && (h_eps == nullptr) == (h_rand_action == nullptr));
  JH_ARG(aligned16(d_h_in) && aligned16(d_c_in));
  if (f->acted) return jh_fail(JH_ERR_STATE, "jh_r2d2_actors_act twice in one tick: jh_r2d2_actors_emit closes the tick");
  hipStream_t st = jh_s(stream);
  jh_draws dr;
  int rc = jh_ctx_stage_draws(f->ctx, (size_t)f->N, h_eps, h_u, h_rand_action, &dr);
  if (rc) return rc;
  ActArgs g{};
  g.N = f->N; g.S = f->S; g.A = f->A; g.H = f->H; g.L = f->L;
  g.obs_vec = (f->S % 4 == 0) && aligned16(d_obs);
  g.st = f->st + (size_t)(f->tick & 1) * f->N * ST_INTS;
  g.q = d_q; g.obs = d_obs; g.h_in = d_h_in; g.c_in = d_c_in; g.onehot = f->onehot;
  g.r_obs = f->r_obs; g.r_oh = f->r_oh; g.r_h = f->r_h; g.r_c = f->r_c; g.r_sc = f->r_sc;
  g.eps = dr.eps; g.u = dr.u; g.rand_action = dr.rand_action; g.action = d_action; g.q_taken = d_q_taken;
  JH_LAUNCH(jh_r2d2_actors_act_kernel, dim3((f->N + kActGroup - 1) / kActGroup), dim3(256), 0, st, g);
  JH_LAUNCH_CHECK();
  f->acted = true;
  return dr.slab ? jh_ctx_slab_release(f->ctx, dr.slab, st) : JH_OK;
}

JH_EXPORT int jh_r2d2_actors_emit(jh_r2d2_actors* f, const float* h_reward, const float* h_done, const jh_r2d2_rows* out, int64_t capacity,
                                  int32_t restart, int64_t* d_count, jh_stream stream) {
  JH_ARG(f && h_reward && h_done && out && d_count);
  if (capacity < f->N) return jh_fail(JH_ERR_ARG, "jh_r2d2_actors_emit: capacity = %lld rows is below n_actors = %d (a tick can emit a row per actor)", (long long)capacity, f->N);
  JH_ARG(out->state && out->prev_action_onehot && out->action && out->reward && out->done && out->hidden_h && out->hidden_c && out->next_hidden_h &&
         out->next_hidden_c && out->priority);
  JH_ARG(aligned16(out->state) && aligned16(out->prev_action_onehot) && aligned16(out->hidden_h) && aligned16(out->hidden_c) &&
         aligned16(out->next_hidden_h) && aligned16(out->next_hidden_c));
  if (!f->acted) return jh_fail(JH_ERR_STATE, "jh_r2d2_actors_emit without this tick's jh_r2d2_actors_act");
  hipStream_t st = jh_s(stream);
  const int N = f->N;
  const int64_t t = f->tick;
  const size_t p = (size_t)(t & 1), NH = (size_t)N * f->H;
  jh_pinned_slab* slab = nullptr;
  int rc = jh_ctx_slab(f->ctx, sizeof(float) * 2 * (size_t)N, &slab);
  if (rc) return rc;
  memcpy(slab->host, h_reward, sizeof(float) * (size_t)N);
  memcpy(static_cast<float*>(slab->host) + N, h_done, sizeof(float) * (size_t)N);
  EmitArgs g{};
  g.N = N; g.S = f->S; g.A = f->A; g.H = f->H; g.L = f->L; g.seq = f->seq; g.burn = f->burn; g.n = f->n; g.period = f->period; g.pad = f->pad;
  g.restart = restart != 0; g.gamma = f->gamma; g.eta = f->eta; g.eps = f->eps;
  g.st_in = f->st + p * N * ST_INTS; g.st_out = f->st + (1 - p) * N * ST_INTS; g.cur_in = f->cur + p; g.cur_out = f->cur + (1 - p);
  g.cap = capacity;
  g.h_rew = static_cast<const float*>(slab->dev); g.h_done = static_cast<const float*>(slab->dev) + N;
  g.r_obs = f->r_obs; g.r_oh = f->r_oh; g.r_h = f->r_h; g.r_c = f->r_c; g.r_sc = f->r_sc;
  g.onehot = f->onehot; g.h_next = f->h + (1 - p) * NH; g.c_next = f->c + (1 - p) * NH;
  g.o_state = out->state; g.o_oh = out->prev_action_onehot; g.o_action = out->action; g.o_reward = out->reward; g.o_done = out->done;
  g.o_hh = out->hidden_h; g.o_hc = out->hidden_c; g.o_nhh = out->next_hidden_h; g.o_nhc = out->next_hidden_c; g.o_prio = out->priority;
  g.count = d_count;
  JH_LAUNCH(jh_r2d2_actors_emit_kernel, dim3(N), dim3(256), 0, st, g);
  JH_LAUNCH_CHECK();
  rc = jh_ctx_slab_release(f->ctx, slab, st);
  if (rc) return rc;
  f->tick = t + 1;
  f->acted = false;
  return JH_OK;
}

// Checkpoint: the device block (state blocks, cursor, carried state, window rings) + the tick.  Both calls synchronise `stream`.
JH_EXPORT int64_t jh_r2d2_actors_state_bytes(const jh_r2d2_actors* f) { return f ? (int64_t)f->block_bytes + 16 : 0; }

JH_EXPORT int jh_r2d2_actors_save(jh_r2d2_actors* f, void* h_out, int64_t bytes, jh_stream stream) {
  JH_ARG(f && h_out && bytes == jh_r2d2_actors_state_bytes(f));
  if (f->acted) return jh_fail(JH_ERR_STATE, "jh_r2d2_actors_save between the two halves of a tick");
  int64_t head[2] = {f->tick, (int64_t)f->block_bytes};
  memcpy(h_out, head, 16);
  JH_HIP(hipMemcpyAsync((char*)h_out + 16, f->block, f->block_bytes, hipMemcpyDeviceToHost, jh_s(stream)));
  JH_HIP(hipStreamSynchronize(jh_s(stream)));
  return JH_OK;
}

JH_EXPORT int jh_r2d2_actors_load(jh_r2d2_actors* f, const void* h_in, int64_t bytes, jh_stream stream) {
  JH_ARG(f && h_in && bytes == jh_r2d2_actors_state_bytes(f));
  int64_t head[2];
  memcpy(head, h_in, 16);
  if (head[1] != (int64_t)f->block_bytes)
    return jh_fail(JH_ERR_ARG, "jh_r2d2_actors_load: the saved actors have another geometry (%lld vs %zu state bytes)", (long long)head[1], f->block_bytes);
  JH_HIP(hipMemcpyAsync(f->block, (const char*)h_in + 16, f->block_bytes, hipMemcpyHostToDevice, jh_s(stream)));
  JH_HIP(hipStreamSynchronize(jh_s(stream)));
  f->tick = head[0];
  f->acted = false;
  return JH_OK;
}
