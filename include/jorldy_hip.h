/*
 * jorldy_hip.h -- C ABI of libjorldy_hip.so, the MI355X (gfx950) native RL hot path
 * that sits behind JORLDY's core/agent + core/buffer API.
 *
 * The reference (kakaoenterprise/JORLDY, all paths below relative to
 * /root/reference/jorldy/) has NO native code and NO FFI: every function here
 * replaces a piece of pure-Python/numpy/torch-CPU code.  Each entry point cites
 * the reference file:line it stands in for.  INTEGRATION.md shows the ctypes
 * binding a JORLDY maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, a negative jh_status otherwise;
 *     jh_last_error() returns a thread-local, human readable message.
 *   - `d_*` parameters are DEVICE pointers (e.g. torch `tensor.data_ptr()`),
 *     borrowed for the duration of the enqueued work; `h_*` are HOST pointers,
 *     consumed before the call returns (copied into the library's pinned staging).
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  All
 *     work is enqueued on it; no call synchronises unless its comment says so.
 *   - one jh_ctx per GPU; a ctx (and objects created from it) is not thread-safe.
 *   - plain C types only; no torch / C++ types cross this boundary.
 */
#ifndef JORLDY_HIP_H
#define JORLDY_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JH_ABI_VERSION 2

typedef enum {
  JH_OK = 0,
  JH_ERR_HIP = -1,      /* a HIP runtime call failed (message has hipGetErrorString) */
  JH_ERR_ARG = -2,      /* invalid argument */
  JH_ERR_STATE = -3,    /* object in the wrong state (e.g. sampling an empty tree) */
  JH_ERR_NOMEM = -4,
  JH_ERR_NODEVICE = -5  /* no usable gfx950 device */
} jh_status;

typedef enum { JH_U8 = 0, JH_F32 = 1, JH_I64 = 2, JH_F64 = 3, JH_I32 = 4 } jh_dtype;

typedef struct jh_ctx jh_ctx;
typedef struct jh_store jh_store;
typedef struct jh_per jh_per;
typedef struct jh_cartpole jh_cartpole;
typedef void* jh_stream;

/* ------------------------------------------------------------------ library / context */
int jh_abi_version(void);
/* End a stream capture that was invalidated and abandoned by its owner (hipStreamEndCapture + destroy whatever graph comes back) and clear
 * the sticky error: 1 = there was a capture to end, 0 = the stream was not capturing.  The host side calls it when torch.cuda.graph raises
 * out of capture_end(), which leaves the capture stream current and still capturing.                                                  */
int jh_stream_abort_capture(jh_stream stream);
const char* jh_last_error(void);
int jh_device_count(void);                       /* 0 when no GPU is visible (never an error) */
int jh_ctx_create(int device, jh_ctx** out);     /* binds the device, allocates pinned staging */
void jh_ctx_destroy(jh_ctx* ctx);
/* Host cores local to this context's GPU (sysfs local_cpulist of its PCI function, e.g. "64-127,192-255"): the
 * collector thread (Actor.run's replacement, manager/distributed_manager.py:76-92) should run there -- acting crosses
 * PCIe twice per timestep and the far socket adds ~1.8 us per crossing.                                   */
int jh_ctx_local_cpulist(jh_ctx* ctx, char* out, int64_t len);
int jh_ctx_sync(jh_ctx* ctx, jh_stream stream);  /* hipStreamSynchronize */
/* Pinned host memory mapped into the device address space (the pinned staging of the collector:
 * observations written by the host are read in place by the acting kernels, actions come back
 * the same way).  *dev_out is the address kernels must use.                                 */
/* Host-side wait for results that kernels write into device-mapped pinned memory (the learn() statistics: the
 * reference reads them with .item() syncs, core/agent/ppo.py:171-184, rainbow.py:241-253): returns 0 once none of
 * base[idx[i]], i < n, equals `sentinel` any more, 1 after timeout_s seconds.  Pure host spin, no HIP call.          */
int jh_host_wait_marks(const float* base, const int32_t* idx, int32_t n, float sentinel, double timeout_s);
/* The same on 32-bit words (e.g. the low words of int64 actions preset to -1 by the host). */
int jh_host_wait_words(const uint32_t* base, const int32_t* idx, int32_t n, uint32_t sentinel, double timeout_s);
/* The epoch shuffles of PPO.learn (core/agent/ppo.py:116-118: idxs = np.arange(M); np.random.shuffle(idxs) per epoch, cumulative)
 * drawn IN PLACE from numpy's global MT19937 with numpy's algorithm (RandomState._shuffle_raw + random_interval), through the
 * state address / next_uint32 / next_uint64 function pointers of BitGenerator.ctypes: h_perm_out [epochs][n] = the index list of
 * every epoch, bit-identical to the Python calls (3 us instead of 12 us per 1024 indices).  Pure host code.                    */
int jh_np_legacy_shuffles(void* bitgen_state, void* next_uint32_fn, void* next_uint64_fn, int64_t n, int32_t epochs,
                          int64_t* h_perm_out);
int jh_pinned_alloc(jh_ctx* ctx, int64_t bytes, void** host_out, void** dev_out);
void jh_pinned_free(void* host);

/* Per-kernel timing with HIP events recorded on the launch stream around every kernel of this
 * library (measurement only; off by default).  jh_prof_report synchronises the device and writes
 * "<kernel>\t<launches>\t<total_ms>\n" lines into buf.                                          */
int jh_prof_enable(int32_t on);
int jh_prof_report(char* buf, int64_t cap);
int jh_prof_calibrate(int32_t n, jh_stream stream); /* n empty event pairs -> "__event_pair_overhead" */
/* Measurement aid: a streaming read of exactly `bytes` device bytes with `width` (4 / 8 / 16) bytes per lane and access -- the
 * known byte count the rocprofv3 HBM counters are calibrated against per access width (tools/pmc_calibrate.sh).              */
int jh_calib_stream(jh_ctx* ctx, const void* d_src, int64_t bytes, int32_t width, float* d_out, jh_stream stream);

/* ------------------------------------------------------------------ transition store
 * GPU-resident struct-of-arrays ring that replaces the list-of-dicts storage of
 *   ReplayBuffer   core/buffer/replay_buffer.py:8-35   (ring + uniform gather)
 *   RolloutBuffer  core/buffer/rollout_buffer.py:6-24  (append, take all, clear)
 * and BaseBuffer.stack_transition core/buffer/base.py:42-56 (AoS->SoA, done once at
 * push time on the host side instead of at every sample).
 * Column c is a device array [capacity][elems[c]] of dtype[c].                      */
typedef struct {
  int32_t dtype;  /* jh_dtype of the stored column */
  int64_t elems;  /* elements per transition */
} jh_col_desc;

int jh_store_create(jh_ctx* ctx, int64_t capacity, int32_t n_cols, const jh_col_desc* cols, jh_store** out);
void jh_store_destroy(jh_store* s);
/* Append n transitions (ring write at buffer_index, wraps; replay_buffer.py:16-23).
 * h_cols[c] points at n*elems[c] contiguous elements of dtype[c].  The data is copied into
 * pinned staging before returning, then moved with hipMemcpyAsync on `stream`.          */
int jh_store_push(jh_store* s, int64_t n, const void* const* h_cols, jh_stream stream);
/* Zero-copy variant for native collectors: get pinned slab pointers for n rows, fill them,
 * then commit (enqueues the async H2D copies).  begin/commit must alternate.             */
int jh_store_stage_begin(jh_store* s, int64_t n, void** h_cols_out);
int jh_store_stage_commit(jh_store* s, jh_stream stream);
/* Same ring append from DEVICE-resident rows already in the stored dtypes (on-device collectors,
 * growing a rollout store): d_cols[c] -> n*elems[c] elements, device-to-device async copies.   */
int jh_store_push_device(jh_store* s, int64_t n, const void* const* d_cols, jh_stream stream);
/* out[c][b][:] = convert(col[c][idx[b] - idx_offset][:]) for the selected columns
 * (replay_buffer.py:25-31 + base.py:42-56 + the fp32 cast of BaseAgent.as_tensor,
 * core/agent/base.py:61-73).  out_dtype[c] is JH_F32 (as_tensor semantics) or the stored
 * dtype (keeps uint8 frames 4x smaller).  d_idx: int64[B]; idx_offset lets PER pass
 * tree-space indices (leaf = idx - (N-1), per_buffer.py:95).                             */
/* Positional writes: row i of the host columns lands in slot h_slots[i] (0 <= slot < capacity); index / counter
 * of the ring are not touched.  Used for the frame pool of the de-duplicated image replay (SURVEY.md §8f rank 2:
 * single 84x84 frames + per-transition frame indices instead of two 4-frame stacks per transition).       */
int jh_store_write_rows(jh_store* s, int64_t n, const int64_t* h_slots, const void* const* h_cols, jh_stream stream);
int jh_store_gather(jh_store* s, int64_t B, const int64_t* d_idx, int64_t idx_offset, int32_t n_sel,
                    const int32_t* sel_cols, void* const* d_out, const int32_t* out_dtype, jh_stream stream);
void* jh_store_col_ptr(jh_store* s, int32_t col);  /* device base of a column (rollout "sample" is a view) */
int64_t jh_store_size(const jh_store* s);          /* buffer_counter */
int64_t jh_store_index(const jh_store* s);         /* buffer_index   */
int64_t jh_store_capacity(const jh_store* s);
void jh_store_clear(jh_store* s);                  /* rollout_buffer.py:19 */
int jh_store_set_position(jh_store* s, int64_t index, int64_t counter); /* checkpoint restore */

/* ------------------------------------------------------------------ prioritized replay
 * Device-resident float64 sum tree, array-heap layout identical to
 * core/buffer/per_buffer.py:7-105: 2N-1 nodes, leaves at [N-1, 2N-2].  All updates
 * are the reference's incremental `+= delta` climbs applied in batch order per node,
 * so the tree stays BIT-IDENTICAL to the reference's numpy tree.                        */
int jh_per_create(jh_ctx* ctx, int64_t capacity, double uniform_sample_prob, jh_per** out);
void jh_per_destroy(jh_per* p);
/* per_buffer.py:19-40: n x add_tree_data at tree_index (wraps independently).
 * h_prio == NULL -> every new leaf gets the current max_priority (per_buffer.py:27-31). */
int jh_per_push(jh_per* p, int64_t n, const double* h_prio, jh_stream stream);
/* The same append with priorities that already live in HBM (float64 [n], device): jh_feed_tick's actor-side priorities. */
int jh_per_push_device(jh_per* p, int64_t n, const double* d_prio, jh_stream stream);
/* per_buffer.py:42-54 applied for b = 0..B-1 in order: d_idx int64[B] TREE-space indices,
 * d_prio float32[B] (prio_dtype JH_F32: the `.item()` of an fp32 tensor, per.py:68-70,
 * rainbow.py:230-231) or float64[B].  Duplicated indices behave sequentially.          */
int jh_per_update(jh_per* p, int64_t B, const int64_t* d_idx, const void* d_prio, int32_t prio_dtype, jh_stream stream);
/* per_buffer.py:70-101.  The three numpy global-RNG draws stay on the host so indices are
 * bit-exact: n_uniform = sum(uniform(B) < usp); h_uniform_slot = randint(counter, n_uniform);
 * h_u = uniform(B - n_uniform) (NOT yet multiplied by the root).  Outputs (device):
 * d_idx int64[B] tree-space, uniform first; d_w64 float64[B] and/or d_w32 float32[B]
 * (either may be NULL) = ((1/counter)/P)^beta / max; d_stats float64[4] =
 * {sampled_p, mean_p, root, max_w_unnormalised}.                                        */
int jh_per_sample(jh_per* p, int64_t B, double beta, int64_t n_uniform, const int64_t* h_uniform_slot,
                  const double* h_u, int64_t* d_idx, double* d_w64, float* d_w32, double* d_stats, jh_stream stream);
/* Blocking read-back of the scalar state (synchronises `stream`). */
/* Sharded PER for data-parallel learners: every rank samples from its own shard with jh_per_sample;
 * jh_per_shard_stats writes {root, count, min priority of that sample} (3 float64) for an all-gather over the ranks,
 * jh_per_weights_sharded recomputes the IS weights of the last sample against the LOGICAL buffer (sum of roots /
 * counts, maximum weight over the global batch = weight of the smallest gathered priority): per_buffer.py:88-94 for
 * one tree holding all shards.  d_all3 float64[n_shards][3] in rank order.                                          */
int jh_per_shard_stats(jh_per* p, int64_t B, double* d_out3, jh_stream stream);
int jh_per_weights_sharded(jh_per* p, int64_t B, double beta, const double* d_all3, int32_t n_shards, double* d_w64,
                           float* d_w32, jh_stream stream);
int jh_per_state(jh_per* p, double* max_priority, double* root, int64_t* tree_index, int64_t* counter, jh_stream stream);
double* jh_per_tree_ptr(jh_per* p);  /* device float64[2N-1] */
int64_t jh_per_tree_size(const jh_per* p);
/* Checkpoint / restore of the whole tree state (blocking; the reference cannot resume its buffer,
 * SURVEY.md §5 -- this is what a complete checkpoint needs).  h_tree: float64[2N-1].   */
int jh_per_load(jh_per* p, const double* h_tree, double max_priority, int64_t tree_index, int64_t counter);
int jh_per_dump(jh_per* p, double* h_tree, jh_stream stream);

/* ------------------------------------------------------------------ PPO math
 * jh_gae: core/agent/ppo.py:95-110.  Inputs float32[W*T], worker-major (row w = one
 * worker's T steps).  delta = r + (1-d)*gamma*V' - V; reverse scan per row that does not
 * bootstrap across the row end; ret = adv + V; if standardize: per-row
 * (adv-mean)/(std_unbiased+1e-7).  One wave per row, wave-shuffle segmented scan.       */
int jh_gae(jh_ctx* ctx, int32_t W, int32_t T, float gamma, float lambda, const float* d_reward, const float* d_done,
           const float* d_value, const float* d_next_value, float* d_adv, float* d_ret, int32_t standardize,
           jh_stream stream);
/* ppo.py:118-125 gathers state[idx], action[idx], adv[idx], ret[idx], value[idx], log_prob_old[idx] inside the
 * minibatch loop; the index lists of all epochs exist before the loop, so the rows are gathered ONCE per learn():
 * row i of d_dst[c] ([n][elems[c]] float32) = row d_idx[i] of d_src[c].  n_cols <= 8.  The minibatch kernels then
 * read consecutive rows (jh_pponet_ppo_update with d_idx = NULL).                                                   */
int jh_ppo_minibatch_rows(jh_ctx* ctx, int64_t n, const int64_t* d_idx, int32_t n_cols, const int32_t* elems,
                          const float* const* d_src, float* const* d_dst, jh_stream stream);
/* ppo.py:112 `ret.mean()`: *d_out = mean of n floats, one workgroup, fixed summation order.                          */
int jh_mean_f32(jh_ctx* ctx, int64_t n, const float* d_x, float* d_out, jh_stream stream);
/* log pi_old(a|s): ppo.py:90-92 `pi.gather(1, action).log()` with pi = exp(log_softmax(logits)). */
int jh_logp_discrete(jh_ctx* ctx, int64_t M, int32_t A, const float* d_logits, const float* d_action, float* d_logp,
                     jh_stream stream);
/* ppo.py:85-88 continuous: per-dimension Normal log-prob of atanh(clamp(a)); takes RAW heads
 * (mu before clamp(+-5), log_std before tanh; core/network/policy_value.py:52-56).      */
int jh_logp_continuous(jh_ctx* ctx, int64_t M, int32_t A, const float* d_mu_raw, const float* d_log_std_raw,
                       const float* d_action, float* d_logp, jh_stream stream);
/* Clipped surrogate + clipped value + entropy, forward AND backward to the head outputs
 * (ppo.py:131-165).  Row i of the minibatch reads the rollout-sized arrays at
 * r = d_idx ? d_idx[i] : i  (the `x[idx]` gathers of ppo.py:122-125 are fused away);
 * d_logits / d_value_pred are minibatch-sized [B][A] / [B].
 * d_stats float32[8] = {loss, actor_loss, critic_loss, entropy_loss, max_ratio, min_prob, c1, c2}. */
int jh_ppo_loss_discrete(jh_ctx* ctx, int32_t B, int32_t A, const float* d_logits, const float* d_value_pred,
                         const int64_t* d_idx, const float* d_action, const float* d_adv, const float* d_ret,
                         const float* d_value_old, const float* d_logp_old, float eps_clip, float vf_coef,
                         float ent_coef, float* d_grad_logits, float* d_grad_value, float* d_stats,
                         jh_stream stream);
int jh_ppo_loss_continuous(jh_ctx* ctx, int32_t B, int32_t A, const float* d_mu_raw, const float* d_log_std_raw,
                           const float* d_value_pred, const int64_t* d_idx, const float* d_action, const float* d_adv,
                           const float* d_ret, const float* d_value_old, const float* d_logp_old, float eps_clip,
                           float vf_coef, float ent_coef, float* d_grad_mu_raw, float* d_grad_log_std_raw,
                           float* d_grad_value, float* d_stats, jh_stream stream);
/* The same loss for DATA-PARALLEL learners with the critic of ppo.py:147-154 exact over the global minibatch (see
 * jh_pponet_ppo_update_dp_begin): both critic branches' value gradients are kept (d_grad_value | d_dv2 float32[B]), d_critic_sums
 * float32[2] <- this rank's {sum e1, sum e2}, d_stats_local float32[8] <- this rank's statistics.  After the caller's all-reduce (MEAN
 * over the ranks) of d_critic_sums, jh_ppo_critic_select_rows mixes d_grad_value in place with the global branch weights and writes
 * d_stats (actor / entropy terms of this rank, critic terms of the global minibatch).                                            */
int jh_ppo_loss_deferred(jh_ctx* ctx, int32_t continuous, int32_t B, int32_t A, const float* d_head0, const float* d_head1,
                         const float* d_value_pred, const int64_t* d_idx, const float* d_action, const float* d_adv, const float* d_ret,
                         const float* d_value_old, const float* d_logp_old, float eps_clip, float vf_coef, float ent_coef,
                         float* d_grad_head0, float* d_grad_head1, float* d_grad_value, float* d_dv2, float* d_critic_sums,
                         float* d_stats_local, jh_stream stream);
int jh_ppo_critic_select_rows(jh_ctx* ctx, int32_t B, const float* d_critic_sums, float vf_coef, float ent_coef, float* d_grad_value,
                              const float* d_dv2, const float* d_stats_local, float* d_stats, jh_stream stream);

/* The same losses for a network whose LAST LAYER stacks the heads (the policy-value net on the CNN head as jh_rbnet runs it: policy_value.py:8-22 with
 * head.py:21-61 under it; rows of the last layer = pi [A] | v, or mu [A] | log_std [A] | v): d_heads float32[B][ld] = (head0 [A] | head1 [A] (continuous) |
 * value | padding), gradient back in the same layout (d_grad_heads float32[B][ld], padding columns untouched).  d_dv2 float32[B] + d_critic_sums float32[2]
 * both non-NULL: the deferred critic of jh_ppo_loss_deferred (d_stats is then the LOCAL row; finish with jh_ppo_critic_select_strided on the value column,
 * ldv = ld).  Replaces ppo.py:122-165 for config.ppo.atari / ppo.procgen.                                                                               */
int jh_ppo_loss_packed(jh_ctx* ctx, int32_t continuous, int32_t B, int32_t A, const float* d_heads, int32_t ld, const int64_t* d_idx, const float* d_action,
                       const float* d_adv, const float* d_ret, const float* d_value_old, const float* d_logp_old, float eps_clip, float vf_coef,
                       float ent_coef, float* d_grad_heads, float* d_dv2, float* d_critic_sums, float* d_stats, jh_stream stream);
int jh_ppo_critic_select_strided(jh_ctx* ctx, int32_t B, const float* d_critic_sums, float vf_coef, float ent_coef, float* d_grad_value, int32_t ldv,
                                 const float* d_dv2, const float* d_stats_local, float* d_stats, jh_stream stream);
/* d_packed float32[rows][ld] -> d_h0 [rows][A], d_h1 [rows][A] (NULL: one head), d_value [rows]: what jh_logp_* / jh_gae read (ppo.py:83-94, once per learn()) */
int jh_heads_unpack(jh_ctx* ctx, int64_t rows, int32_t A, const float* d_packed, int32_t ld, float* d_h0, float* d_h1, float* d_value, jh_stream stream);
/* PPO.act, discrete policy, heads already on the device (ppo.py:63-69): action[w] = Categorical(softmax(d_heads[w][0..A))).sample() by inverse CDF on the
 * counter-based stream (seed, counter = timestep, w) -- the stream of jh_pponet_act_discrete's host-side sampler --, or the first maximum when !training.
 * d_action int64[W]: device or device-mapped host memory.                                                                                                */
int jh_policy_act_discrete(jh_ctx* ctx, int32_t W, int32_t A, const float* d_heads, int32_t ld, uint64_t seed, uint64_t counter, int32_t training,
                           int64_t* d_action, jh_stream stream);

/* ------------------------------------------------------------------ TD losses (DQN family)
 * One kernel for dqn.py:128-141, double.py:28-39, multistep.py:41-50, per.py:54-74,
 * ape_x.py:96-116.  flags: */
#define JH_TD_DOUBLE 1   /* a* = argmax Q_online(s'); bootstrap Q_target(s')[a*]           */
#define JH_TD_PER 2      /* loss = mean(w*td^2), priorities td^alpha; else Huber (beta=1)  */
/* d_q [B][A] online Q(s); d_q_next_online [B][A] (DOUBLE only); d_q_next_target [B][A];
 * d_action float32[B]; d_reward/d_done float32 [B][n] (n = max(n_step,1); n_step==0 is the
 * 1-step form); d_weights float32[B] (PER only).  Outputs: d_grad_q [B][A] (d loss/d Q(s)),
 * d_prio float32[B] (= td^alpha, or |td| when not PER; may be NULL),
 * d_stats float32[4] = {loss, max_Q, mean_td, 0}.                                        */
int jh_td_loss(jh_ctx* ctx, int32_t B, int32_t A, int32_t n_step, int32_t flags, const float* d_q,
               const float* d_q_next_online, const float* d_q_next_target, const float* d_action,
               const float* d_reward, const float* d_done, const float* d_weights, float gamma, float alpha,
               float* d_grad_q, float* d_prio, float* d_stats, jh_stream stream);

/* ------------------------------------------------------------------ Munchausen DQN
 * core/agent/m_dqn.py:29-59 with agent/utils.py:29-39, forward and backward to Q(s).  d_q / d_q_target / d_q_next_target
 * float32 [B][A] = online(s), target(s), target(s'); d_action / d_reward / d_done float32 [B] (actions clamped into [0, A)).
 * Per row, with the row maximum subtracted before every exp:
 *   log-policy  lp = d_q_target[a] - (max + tau * log(sum_k exp((d_q_target[k] - max) / tau)))
 *   soft value  V  = sum_k pi_k * (x_k - tau * log pi_k),  x = d_q_next_target, pi = softmax((x - max) / tau)
 *   target      y  = reward + alpha * clamp(lp, l_0, 0) + (1 - done) * gamma * V
 *   loss = mean_b smooth_l1(d_q[b][a] - y, beta 1)
 * Outputs: d_grad_q [B][A] = d loss / d d_q, every entry written (clamp(q - y, -1, 1) / B at the taken action, zero elsewhere);
 * d_stats float32[4] = {loss, max over b of the TAKEN q, mean of alpha * clamp(lp, l_0, 0), mark}: the payload is fenced before
 * the arrival mark [3] (0.f), as jh_td_loss leaves it.  tau > 0, l_0 <= 0; A == 1 is legal (lp is exactly 0, V is x itself).
 * At most two launches, no floating-point atomics: the same inputs give the same bits, eagerly or replayed in a graph.        */
int jh_mdqn_loss(jh_ctx* ctx, int32_t B, int32_t A, const float* d_q, const float* d_q_target, const float* d_q_next_target,
                 const float* d_action, const float* d_reward, const float* d_done, float gamma, float alpha, float tau, float l_0,
                 float* d_grad_q, float* d_stats, jh_stream stream);

/* ------------------------------------------------------------------ C51 / Rainbow
 * Categorical n-step projection + cross-entropy, forward and backward to the online
 * logits (rainbow.py:167-239, c51.py:68-109, logits2Q rainbow.py:285-292).  flags: */
#define JH_C51_DOUBLE 1     /* rainbow: action from argmax Q_online(s'); else target net's own */
#define JH_C51_PER 2        /* rainbow: prio = KL^alpha, loss = mean(w)*mean(KL) (shape-broadcast quirk) */
#define JH_C51_SHIFT_MAX 4  /* c51.py:126-128 subtracts the row max before log_softmax        */
/* d_logit / d_next_logit_online / d_target_logit: [B][A][K]; d_reward/d_done [B][n];
 * outputs d_grad_logit [B][A][K], d_prio float32[B] (NULL ok), d_kl float32[B] (NULL ok),
 * d_stats float32[8] = {loss, max_Q, max_logit, min_logit, mean_kl, 0,0,0}.              */
int jh_c51_loss(jh_ctx* ctx, int32_t B, int32_t A, int32_t K, int32_t n_step, int32_t flags, const float* d_logit,
                const float* d_next_logit_online, const float* d_target_logit, const float* d_action,
                const float* d_reward, const float* d_done, const float* d_weights, float v_min, float v_max,
                float gamma, float alpha, float* d_grad_logit, float* d_prio, float* d_kl, float* d_stats,
                jh_stream stream);

/* Batched acting of the value-net agents: DQN.act / ApeX.act / C51.act / Rainbow.act (core/agent/dqn.py:76-92,
 * ape_x.py:64-77, c51.py:50-66, rainbow.py:140-152) for N actors in one call.  d_logits [N][A][K] are the network's
 * outputs (K = 1: Q values; K > 1: atom logits, Q = expectation under softmax over the support linspace(v_min,
 * v_max, K), rainbow.py:285-292).  Epsilon-greedy per actor with the HOST's draws (h_eps float32[N], h_u float64[N]
 * = np.random.random(), h_rand_action int64[N] = np.random.randint(A); all three NULL: greedy).  Outputs (device):
 * d_action int64[N] (first maximum, like torch.argmax), d_q_taken float32[N] (Q of the action taken; NULL ok),
 * d_q_all float32[N][A] (NULL ok).                                                                                */
int jh_value_act(jh_ctx* ctx, int32_t N, int32_t A, int32_t K, const float* d_logits, float v_min, float v_max,
                 const float* h_eps, const double* h_u, const int64_t* h_rand_action, int64_t* d_action,
                 float* d_q_taken, float* d_q_all, jh_stream stream);

/* ------------------------------------------------------------------ QR-DQN
 * Pairwise quantile-Huber loss, forward and backward to the online quantiles (core/agent/qrdqn.py:60-95, logits2Q
 * qrdqn.py:112-115).  d_logit / d_next_logit_online / d_target_logit float32 [B][A][N] = online(s), online(s'), target(s');
 * d_action / d_reward / d_done float32 [B] (actions clamped into [0, A)); d_tau float32 [N], the quantile midpoints as the
 * host's torch.arange gives them (qrdqn.py:26-31; 1 - tau is formed in fp32 as the reference forms inv_tau).  With
 * P[i] = logit[b][action[b]][i], a* = first maximum over a of mean_i next_logit_online[b][a][i] (the online net selects, the
 * target net evaluates; there is no other form) and T[j] = reward + (1 - done) * gamma * target_logit[b][a*][j]:
 * e = T[j] - P[i], loss = 1 / (B N) * sum_b sum_j sum_i (e < 0 ? 1 - tau[i] : tau[i]) * smooth_l1(e, beta 1).
 * Outputs: d_grad_logit float32 [B][A][N] = d loss / d logit, every entry written (zero outside the taken action's row);
 * d_stats float32[8] = {loss, max_Q, max_logit, min_logit, 0, mark, 0, mark}: max_Q over the quantile means of d_logit, max / min
 * over d_logit itself, the payload fenced before the arrival marks [5], [7] (0.f) as jh_c51_loss leaves them.
 * 1 <= N <= 256.  Two launches, no floating-point atomics: the same inputs give the same bits, eagerly or replayed in a graph.      */
int jh_qr_loss(jh_ctx* ctx, int32_t B, int32_t A, int32_t N, const float* d_logit, const float* d_next_logit_online,
               const float* d_target_logit, const float* d_action, const float* d_reward, const float* d_done,
               const float* d_tau, float gamma, float* d_grad_logit, float* d_stats, jh_stream stream);

/* QRDQN.act (core/agent/qrdqn.py:33-47) for R actor rows in one call: jh_value_act with Q = mean of the N quantiles
 * (qrdqn.py:112-115) in place of the expectation over a support.  d_logits float32 [R][A][N]; the host's epsilon draws as in
 * jh_value_act (all three NULL: greedy); d_action int64[R] (first maximum), d_q_taken float32[R] (NULL ok; written and fenced
 * before the action, so a host that waits on device-mapped actions finds it in place), d_q_all float32[R][A] (NULL ok).    */
int jh_quantile_act(jh_ctx* ctx, int32_t R, int32_t A, int32_t N, const float* d_logits, const float* h_eps, const double* h_u,
                    const int64_t* h_rand_action, int64_t* d_action, float* d_q_taken, float* d_q_all, jh_stream stream);

/* ------------------------------------------------------------------ IQN
 * The implicit quantile network with an MLP head (core/network/iqn.py:9-47) and what IQN.learn() / act() do around it
 * (core/agent/iqn.py:60-146).  With S inputs, width H (H % 4 == 0), E cosine features, N samples per row (1 <= N <= 256), A actions:
 *   feat = relu(head.l(x)) [rows][H], psi = relu(state_embed(feat)) [rows][H]                         (iqn.py:28-29)
 *   cos_term[r][n][i] = cos(tau[r][n] * i_pi[i]), i_pi = arange(0, E) * pi as FLOAT32; the product is rounded to float32 before
 *   the cosine (iqn.py:14, 40-47), phi = relu(sample_embed(cos_term)) [rows][N][H], embed = psi[:, None, :] * phi,
 *   relu(l1), relu(l2), q -> [rows][N][A]                                                              (iqn.py:31-38)
 * tau is the CALLER's draw (uniform in [tau_min, tau_max], iqn.py:41-45).  Parameters live in caller-owned flat fp32 buckets as
 * jh_rbnet's do; jh_iqnnet_segment describes the layout (rows x cols, row-major [out][in] = the reference's own, 16-byte aligned):
 *   0 head.l.weight [H][S]  1 head.l.bias   2 state_embed.weight [H][H]  3 bias   4 sample_embed.weight [H][E]  5 bias
 *   6 l1.weight [H][H]  7 bias   8 l2.weight [H][H]  9 bias   10 q.weight [A][H]  11 q.bias
 * Every dense contraction is a launch of the tile engine (jh_tgemm_dense's kernel).                                           */
typedef struct jh_iqnnet jh_iqnnet;
int64_t jh_iqnnet_param_count_for(int32_t state_size, int32_t hidden, int32_t embedding_dim, int32_t num_sample, int32_t action_size);
int jh_iqnnet_create(jh_ctx* ctx, int32_t state_size, int32_t hidden, int32_t embedding_dim, int32_t num_sample, int32_t action_size,
                     int32_t max_batch, float* d_params, float* d_target, float* d_grads, float* d_m, float* d_v, jh_iqnnet** out);
void jh_iqnnet_destroy(jh_iqnnet* n);
int32_t jh_iqnnet_segment_count(void);
int jh_iqnnet_segment(const jh_iqnnet* n, int32_t i, int64_t* offset, int32_t* rows, int32_t* cols);
/* torch.optim.Adam's (lr, beta1, beta2, eps) and step counter; every config.iqn.* uses Adam */
int jh_iqnnet_set_hyper(jh_iqnnet* n, double lr, double beta1, double beta2, double eps, int64_t step, jh_stream stream);
int jh_iqnnet_set_lr(jh_iqnnet* n, double lr, jh_stream stream);
int jh_iqnnet_sync_target(jh_iqnnet* n, jh_stream stream);
/* network(x) with the draws d_tau [rows][N]: rows <= max_batch, which 0 online / 1 target -> d_logits [rows][N][A]            */
int jh_iqnnet_forward(jh_iqnnet* n, int32_t which, const float* d_x, int32_t rows, const float* d_tau, float* d_logits, jh_stream stream);
/* The three forwards of IQN.learn() (iqn.py:90, 100, 103), each with its own draw: d_x = [state; next_state] (2B rows),
 * d_tau [3][B][N] -> d_logits [3][B][N][A] = online(state), online(next_state), target(next_state); every layer is one grouped
 * launch for the online rows and the target rows.  The activations of online(state) stay in place for jh_iqnnet_backward.     */
int jh_iqnnet_learn_forward(jh_iqnnet* n, const float* d_x, int32_t B, const float* d_tau, float* d_logits, jh_stream stream);
/* The forwards of M_IQN.learn() (m_iqn.py:30, 43, 50) in jh_iqnnet_learn_forward's launches: d_x = [state; next_state] (2B rows),
 * d_tau [3][B][N] -> d_logits [3][B][N][A] = online(state) with draw 0 (the one jh_iqnnet_backward differentiates), online(state)
 * with draw 1, target(next_state) with draw 2.  The reference's online(next_state) (m_iqn.py:40-41, 46-47) feeds nothing and is
 * not computed: 3 B N sampled rows, as IQN's learn().                                                                          */
int jh_iqnnet_learn_forward_m(jh_iqnnet* n, const float* d_x, int32_t B, const float* d_tau, float* d_logits, jh_stream stream);
/* loss.backward() (iqn.py:128) given d(loss)/d(online(state) output) [B][N][A] (from jh_iqn_loss); fills d_grads              */
int jh_iqnnet_backward(jh_iqnnet* n, const float* d_g, jh_stream stream);
/* [clip_grad_norm_(max_norm) when max_norm > 0,] torch.optim.Adam's step (iqn.py:129); advances the step counter              */
int jh_iqnnet_optim_step(jh_iqnnet* n, float max_norm, jh_stream stream);
/* The network's elementwise steps on their own (tests): the cosine features d_out [rows][E] of d_tau [rows] (iqn.py:46); the
 * Hadamard product d_out [B][N][H] = d_psi [B][H] * d_phi [B][N][H] (iqn.py:34) and its backward through both relus (iqn.py:29, 32):
 * d_grad_phi_pre = d_grad_embed * psi * (phi > 0), d_grad_psi_pre [B][H] = (sum over n, in a fixed order, of d_grad_embed * phi) * (psi > 0). */
int jh_iqn_cos_features(jh_ctx* ctx, int64_t rows, int32_t E, const float* d_tau, float* d_out, jh_stream stream);
int jh_iqn_hadamard(jh_ctx* ctx, int32_t B, int32_t N, int32_t H, const float* d_psi, const float* d_phi, float* d_out, jh_stream stream);
int jh_iqn_hadamard_backward(jh_ctx* ctx, int32_t B, int32_t N, int32_t H, const float* d_grad_embed, const float* d_psi, const float* d_phi,
                             float* d_grad_phi_pre, float* d_grad_psi_pre, jh_stream stream);
/* jh_qr_loss on the network's [B][N][A] layout with tau per sample (iqn.py:89-121): d_logit / d_next_logit_online / d_target_logit
 * float32 [B][N][A]; d_tau float32 [B][N], the draw of the FIRST forward (1 - tau formed in fp32 as iqn.py:120 does).  With
 * P[i] = logit[b][i][action[b]], a* = first maximum over a of mean_n next_logit_online[b][n][a] (iqn.py:106, 142-146) and
 * T[j] = reward + (1 - done) * gamma * target_logit[b][j][a*]: e = T[j] - P[i],
 * loss = 1 / (B N) * sum_b sum_j sum_i (e < 0 ? 1 - tau[b][i] : tau[b][i]) * smooth_l1(e, beta 1).
 * d_grad_logit float32 [B][N][A], every entry written (zero for the actions not taken); d_stats float32[8] as jh_qr_loss leaves
 * them.  1 <= N <= 256.  Two launches, no floating-point atomics: the same inputs give the same bits, eagerly or replayed.      */
int jh_iqn_loss(jh_ctx* ctx, int32_t B, int32_t A, int32_t N, const float* d_logit, const float* d_next_logit_online,
                const float* d_target_logit, const float* d_action, const float* d_reward, const float* d_done, const float* d_tau,
                float gamma, float* d_grad_logit, float* d_stats, jh_stream stream);
/* jh_iqn_loss's pairwise loss under the Munchausen target (m_iqn.py:29-95, agent/utils.py:29-39).  d_logit = online(state) under
 * the first draw d_tau [B][N], d_logit_again = online(state) under a second draw, d_target_logit = target(next_state), each
 * float32 [B][N][A].  With x = mean_n logit_again, x' = mean_n target_logit, tau_e the entropy temperature (the agent's self.tau):
 *   lp = x[action] - (max x + tau_e log sum exp((x - max x) / tau_e)),  pi = softmax(x' / tau_e),  logpi = x' - (max x' + tau_e log sum exp(...)),
 *   T[j] = (reward + alpha * clip(lp, l_0, 0)) + ((1 - done) * gamma) * sum_a pi[a] * (target_logit[b][j][a] - logpi[a]);
 * loss and d_grad_logit as jh_iqn_loss.  d_stats float32[8] in jh_iqn_loss's slots: loss, max_Q (the largest mean of d_logit),
 * max / min over d_logit_again (m_iqn.py:50 reassigns `logit` before lines 94-95 read it), marks at [5] and [7].
 * tau_e > 0, l_0 <= 0, 1 <= N <= 256.  Two launches, no floating-point atomics: the same bits eagerly or replayed.               */
int jh_miqn_loss(jh_ctx* ctx, int32_t B, int32_t A, int32_t N, const float* d_logit, const float* d_logit_again, const float* d_target_logit,
                 const float* d_action, const float* d_reward, const float* d_done, const float* d_tau, float gamma, float alpha, float tau_e,
                 float l_0, float* d_grad_logit, float* d_stats, jh_stream stream);
/* IQN.act (iqn.py:60-76) for R actor rows: jh_quantile_act's rules on d_logits float32 [R][N][A] (Q = mean over the N samples). */
int jh_iqn_act(jh_ctx* ctx, int32_t R, int32_t A, int32_t N, const float* d_logits, const float* h_eps, const double* h_u,
               const int64_t* h_rand_action, int64_t* d_action, float* d_q_taken, float* d_q_all, jh_stream stream);

/* ------------------------------------------------------------------ Rainbow-IQN: the noisy dueling tail on the implicit quantile trunk
 * core/network/rainbow_iqn.py:9-113 on jh_iqnnet's object: the trunk above up to relu(l2) at the CALLER's width (rainbow_iqn.py:85-94
 * passes hidden_size; IQN's agent does not), then Rainbow's four NoisyNet layers (network/utils.py:55-107) with one support over the
 * rows x N sampled rows:  x_a = relu(noisy a1), x_v = relu(noisy v1) (H -> H each, stacked as one [2H][H] operand as jh_rbnet keeps
 * them), noisy a2 (H -> A), noisy v2 (H -> 1), out = x_a - mean_a x_a + x_v -> [rows][N][A]        (rainbow_iqn.py:54-104)
 * jh_riqnnet_create gives a jh_iqnnet whose segment table (jh_iqnnet_segment, jh_riqnnet_segment_count entries) is the trunk's ten
 * segments, q's two left empty, then -- [out][in], the reference keeps noisy weights [in][out] --
 *   12 mu a1|v1 [2H][H]  13 sig  14 mu_b [2H]  15 sig_b   16 mu a2 [A][H]  17 sig  18 mu_b  19 sig_b   20 mu v2 [1][H]  21 sig  22 mu_b  23 sig_b
 * One noise set (jh_riqnnet_noise_len floats of N(0, 1), the draw order of a forward: a1, v1, a2, v2; utils.py:58-60, 75-76):
 *   factorized   [ei_a1 H][ej_a1 H][ei_v1 H][ej_v1 H][ei_a2 H][ej_a2 A][ei_v2 H][ej_v2 1]  eps_w = outer(f(ei), f(ej)), eps_b = f(ej)
 *   independent  [eps_w a1 H x H (in, out)][eps_b a1 H][eps_w v1][eps_b v1][eps_w a2 H x A][eps_b a2 A][eps_w v2 H][eps_b v2 1]
 * state_size % 4 == 0, H % 4 == 0, 1 <= N <= 256, 3 * max_batch * N * 2H < 2^31.  jh_iqnnet_destroy / _segment / _set_hyper / _set_lr /
 * _sync_target / _backward / _optim_step serve this object as they serve IQN's; jh_iqnnet_forward / _learn_forward / _learn_forward_m
 * refuse it, as the entries below refuse IQN's.                                                                                   */
int64_t jh_riqnnet_param_count_for(int32_t state_size, int32_t hidden, int32_t embedding_dim, int32_t num_sample, int32_t action_size);
int jh_riqnnet_create(jh_ctx* ctx, int32_t state_size, int32_t hidden, int32_t embedding_dim, int32_t num_sample, int32_t action_size,
                      int32_t independent_noise, int32_t max_batch, float* d_params, float* d_target, float* d_grads, float* d_m, float* d_v,
                      jh_iqnnet** out);
int32_t jh_riqnnet_segment_count(void);
int64_t jh_riqnnet_noise_len(const jh_iqnnet* n);
/* network(x, is_train) with the draws d_tau [rows][N] (rainbow_iqn.py:42-104): d_noise one noise set, or NULL for is_train False
 * (W = mu); which 0 online / 1 target (its own sigmas) -> d_logits [rows][N][A]                                                    */
int jh_riqnnet_forward(jh_iqnnet* n, int32_t which, const float* d_x, int32_t rows, const float* d_tau, const float* d_noise, float* d_logits,
                       jh_stream stream);
/* The three forwards of RainbowIQN.learn() (agent/rainbow_iqn.py:172, 182, 185): d_x = [state; next_state] (2B rows), d_tau [3][B][N],
 * d_noise [3][noise_len] -> d_logits [3][B][N][A] = online(state), online(next_state), target(next_state), forward i under draw i of
 * both.  The trunk runs as jh_iqnnet_learn_forward's two jobs; the tail as three: one effective-weight launch for the three
 * (parameter set, draw) pairs, grouped GEMMs, one dueling launch.  jh_iqnnet_backward then differentiates online(state): dueling
 * backward, a2 / v2, a1 | v1 (d(mu) in place, both streams' data gradients into the trunk as one GEMM), the trunk,
 * d(sig) = d(mu) * eps under draw 0 (rainbow_iqn.py:221-223).  No floating-point atomics; a replay gives the eager call's bits.      */
int jh_riqnnet_learn_forward(jh_iqnnet* n, const float* d_x, int32_t B, const float* d_tau, const float* d_noise, float* d_logits,
                             jh_stream stream);
/* jh_iqn_loss under Rainbow's return and replay (agent/rainbow_iqn.py:158-224): d_reward / d_done float32 [B][n_step] (n_step 0: [B],
 * as jh_c51_loss takes it), T[j] = target_logit[b][j][a*] folded as T = reward[b][i] + (1 - done[b][i]) * gamma * T for
 * i = n_step - 1 .. 0 in torch's order of operations (rainbow_iqn.py:192-195); d_weights float32 [B], the importance weights.
 * With loss_b = 1 / N * sum_j sum_i (e < 0 ? 1 - tau[b][i] : tau[b][i]) * smooth_l1(e):  d_prio[b] = powf(loss_b, alpha)
 * (rainbow_iqn.py:212).  The reference multiplies weights [B, 1] with loss [B] (rainbow_iqn.py:217-219): the mean of that [B, B]
 * product is loss = mean(w) * mean_b(loss_b) -- the broadcast jh_c51_loss keeps under JH_C51_PER -- so with w = mean(w), summed in a
 * fixed order:  d_grad_logit[b][i][action[b]] = -w * sum_j (...) clip(e, -1, 1) / (B N), zeros elsewhere, and
 * d_stats float32[8] in jh_iqn_loss's slots with d_stats[0] = w * mean_b(loss_b).  With n_step <= 1 and unit
 * weights the gradient and the statistics are jh_iqn_loss's bits.  1 <= N <= 256, n_step >= 0.  Two launches, no atomics.           */
int jh_riqn_loss(jh_ctx* ctx, int32_t B, int32_t A, int32_t N, int32_t n_step, const float* d_logit, const float* d_next_logit_online,
                 const float* d_target_logit, const float* d_action, const float* d_reward, const float* d_done, const float* d_weights,
                 const float* d_tau, float gamma, float alpha, float* d_grad_logit, float* d_prio, float* d_stats, jh_stream stream);

/* ------------------------------------------------------------------ deterministic actor-critic (TD3, DDPG)
 * The elementwise steps of td3.py:146-209 / ddpg.py:117-163 (float32, fixed summation order, capturable, no host sync):
 *   jh_td3_next_action    a = clamp(tanh(z) + clamp(noise_std * eps, -noise_clip, noise_clip), -1, 1) on [B][A] (td3.py:159-162);
 *                         d_eps NULL: a = tanh(z) (policy.py:20; ddpg.py:130, acting, the actor update)
 *   jh_td3_critic_loss    d_q, d_q_next [n_critics][B]: y = r + (1 - d) * gamma * min_i q_next_i (td3.py:163-166, ddpg.py:131-132),
 *                         loss_i = mean((y - q_i)^2), d_grad [n_critics][B] = 2 (q_i - y) / B, d_y [B] (optional);
 *                         d_stats float32[4] = {loss_1, loss_2 (0 for one critic), max_b y (td3.py:178), arrival mark}.
 *                         1 <= B <= 2^20, n_critics 1 or 2.
 *   jh_td3_actor_seed     actor_loss = -mean(q) (td3.py:183, ddpg.py:144), d_grad_q [B] = -1 / B; d_stats float32[2] = {actor_loss, mark}
 *   jh_td3_tanh_backward  d_grad_z = d_grad_a * (1 - a^2): the way back through a = tanh(z)
 *   jh_td3_polyak         target <- tau * params + (1 - tau) * target (td3.py:203-209) bit for bit as torch evaluates it on float32 CPU
 *                         tensors: tau and (1 - tau) -- formed in double -- rounded to float32, two products, one sum.  0 <= tau <= 1.  */
int jh_td3_next_action(jh_ctx* ctx, int32_t B, int32_t A, const float* d_z, const float* d_eps, float noise_std, float noise_clip, float* d_out,
                       jh_stream stream);
int jh_td3_critic_loss(jh_ctx* ctx, int32_t B, int32_t n_critics, const float* d_q, const float* d_q_next, const float* d_reward,
                       const float* d_done, float gamma, float* d_y, float* d_grad, float* d_stats, jh_stream stream);
int jh_td3_actor_seed(jh_ctx* ctx, int32_t B, const float* d_q, float* d_grad_q, float* d_stats, jh_stream stream);
int jh_td3_tanh_backward(jh_ctx* ctx, int32_t B, int32_t A, const float* d_grad_a, const float* d_a, float* d_grad_z, jh_stream stream);
int jh_td3_polyak(jh_ctx* ctx, int64_t n, const float* d_params, float* d_target, double tau, jh_stream stream);
/* The networks: a deterministic policy (network/policy.py:8-20: head.l -> relu(l) -> tanh(pi)) and n_critics = 1 (DDPG) or 2 (TD3)
 * continuous Q networks (network/q_network.py:23-39: [head.l(s) | relu(e(a))] -> relu(l) -> q), each with a target copy.  MLP head,
 * scalar S, H % 4 == 0, A >= 1.  Caller-owned flat fp32 buckets: five of actor_floats (online, target, gradients, exp_avg, exp_avg_sq)
 * and five of n_critics * critic_floats, critic c at c * critic_floats (jh_acnet_param_counts_for).  The critics share one optimizer
 * block and one Adam launch: td3.py:95-112 gives both the same settings.  jh_acnet_segment: segments 0-5 of the actor bucket
 * (head.l.weight [H][S], head.l.bias, l.weight [H][H], l.bias, pi.weight [A][H], pi.bias) and 6-13 of one critic (head.l.weight [H][S],
 * head.l.bias, e.weight [H][A], e.bias, l.weight [H][2H], l.bias, q.weight [1][H], q.bias), offsets relative to that critic.        */
typedef struct jh_acnet jh_acnet;
int jh_acnet_param_counts_for(int32_t S, int32_t H, int32_t A, int64_t* actor_floats, int64_t* critic_floats);
int jh_acnet_create(jh_ctx* ctx, int32_t S, int32_t H, int32_t A, int32_t n_critics, int32_t max_batch, float* d_actor,
                    float* d_actor_target, float* d_actor_grads, float* d_actor_m, float* d_actor_v, float* d_critics,
                    float* d_critics_target, float* d_critics_grads, float* d_critics_m, float* d_critics_v, jh_acnet** out);
void jh_acnet_destroy(jh_acnet* n);
int32_t jh_acnet_segment_count(void);
int jh_acnet_segment(const jh_acnet* n, int32_t i, int64_t* offset, int32_t* rows, int32_t* cols);
/* which: 0 the actor's Adam, 1 the critics'                                                                      */
int jh_acnet_set_hyper(jh_acnet* n, int32_t which, double lr, double beta1, double beta2, double eps, int64_t step, jh_stream stream);
int jh_acnet_set_lr(jh_acnet* n, int32_t which, double lr, jh_stream stream);
/* every target <- its online network; update_target_soft (td3.py:203-209, ddpg.py:159-163) as jh_td3_polyak on both buckets */
int jh_acnet_sync_target(jh_acnet* n, jh_stream stream);
int jh_acnet_soft_update(jh_acnet* n, double tau, jh_stream stream);
/* actor(x) -> d_action [rows][A] (td3.py:139, ddpg.py:112), critic_c(x, action) -> d_q [n_critics][rows]; rows <= max_batch,
 * which 0 online / 1 target                                                                                      */
int jh_acnet_actor_forward(jh_acnet* n, int32_t which, const float* d_x, int32_t rows, float* d_action, jh_stream stream);
int jh_acnet_critic_forward(jh_acnet* n, int32_t which, const float* d_x, const float* d_action, int32_t rows, float* d_q, jh_stream stream);
/* The critic update (td3.py:157-176, ddpg.py:128-138): d_x = [state; next_state] (2B rows); d_noise [B][A] standard normals, or NULL
 * for no target noise (DDPG).  Target pass and online pass share grouped launches; loss; backward; one Adam step of the critics.
 * -> d_y [B], d_q [n_critics][B] (both optional), d_stats as jh_td3_critic_loss.  12 launches.                      */
int jh_acnet_critic_update(jh_acnet* n, const float* d_x, const float* d_action, const float* d_reward, const float* d_done,
                           const float* d_noise, int32_t B, float gamma, float noise_std, float noise_clip, float* d_y, float* d_q,
                           float* d_stats, jh_stream stream);
/* The actor update (td3.py:181-188, ddpg.py:143-148): a = actor(state), -mean(critic_1(state, a)), backward through critic 1's action
 * input into the actor, the actor's Adam step.  Critic 1's parameters, gradient bucket and moments are not written.
 * -> d_action_pred [B][A] (optional), d_stats as jh_td3_actor_seed.  16 launches.                                   */
int jh_acnet_actor_update(jh_acnet* n, const float* d_x, int32_t B, float* d_action_pred, float* d_stats, jh_stream stream);
/* Critic 0 over SAMPLED actions (continuous MPO, mpo.py:219-231, 261-263; objects with n_critics = 1 for the last two entries).  The
 * reference repeats every state N times in front of the critic; here head.l(s) runs once per state row, on R rows, its outputs are copied
 * into the rows of that state's N samples, and only e(a), l and q run over the N * R rows, on the tile engine.
 *   jh_acnet_reserve_sampled         room for rows = N * R sampled rows in each of two slots; allocates, so: once, outside any stream capture
 *   jh_acnet_critic_forward_sampled  critic 0 (which 0 online / 1 target) of d_x [R][S] over d_actions [N][R][A] -> d_q [N][R].  5 launches.
 *   jh_acnet_mpo_forward             every critic forward of one learn(): d_x = [state; next_state] (2R rows), d_action [R][A] the stored
 *                                    action, d_a_next / d_a_add [N][R][A] -> d_q = online(s, a), d_qt_a = target(s, a) [R], d_qt_next =
 *                                    target(s', a_next), d_qt_add = target(s, a_add) [N][R]; one grouped launch per layer for the four, the
 *                                    target's head.l(s) shared by target(s, a) and the samples of a_add.  5 launches (a group of a heavy and
 *                                    a light problem may go as two).  The online activations stay for jh_acnet_critic_fit.
 *   jh_acnet_critic_fit              d_dq [R] = d(loss)/d(online q) of the last jh_acnet_mpo_forward -> the critic's backward,
 *                                    clip_grad_norm_(max_norm; <= 0: none) and Adam on the critic's own optimizer block.  The actor's
 *                                    buckets are not touched.
 * JH_ERR_ARG: R > max_batch, N * R over the reserved rows, N < 1.                                                                     */
int jh_acnet_reserve_sampled(jh_acnet* n, int32_t rows);
int jh_acnet_critic_forward_sampled(jh_acnet* n, int32_t which, const float* d_x, const float* d_actions, int32_t R, int32_t N, float* d_q,
                                    jh_stream stream);
int jh_acnet_mpo_forward(jh_acnet* n, const float* d_x, const float* d_action, const float* d_a_next, const float* d_a_add, int32_t R, int32_t N,
                         float* d_q, float* d_qt_a, float* d_qt_next, float* d_qt_add, jh_stream stream);
int jh_acnet_critic_fit(jh_acnet* n, const float* d_x, const float* d_action, const float* d_dq, int32_t R, float max_norm, jh_stream stream);

/* ------------------------------------------------------------------ soft actor-critic, continuous actions (SAC)
 * The elementwise steps of sac.py:161-269 on the Gaussian policy of policy.py:38-55 (float32, fixed summation order, capturable, no
 * host sync).  The temperature lives in a caller-owned, 8-byte aligned device block of JH_SAC_ALPHA_FLOATS floats that the kernels read
 * and advance themselves, so that a replayed graph sees the current alpha and counts its own Adam steps:
 *   [0] log_alpha   [1] alpha in use: what the losses of the current learn() are formed with (sac.py:250 refreshes it only after the
 *   actor step, before Adam moves log_alpha: the alpha of learn k is exp(log_alpha) after k - 1 steps)   [2] exp_avg   [3] exp_avg_sq
 *   [4] Adam's step count   [5] alpha_lr   [6] Adam's eps   [7] dynamic (0: static log_alpha, the block is only read, but for [9])
 *   [8] target_entropy = -action_size (sac.py:109)   [9] alpha / B of the actor loss just seeded (written by jh_sac_actor_seed, read
 *   by jh_sac_sample_backward)   [10-11] beta1 and [12-13] beta2 as doubles   [14-15] unused
 *   jh_sac_sample           mu = clamp(mu_raw, -5, 5), std = exp(tanh(ls_raw)) (policy.py:38-55), z = mu + std * eps, d_a = tanh(z) and
 *                           d_logp [B] = sum_j [Normal(mu, std).log_prob(z)_j - log(1 - a_j^2 + 1e-7)], j ascending (sac.py:161-169).
 *                           d_eps NULL: the evaluation action tanh(mu) (sac.py:149-150), d_ls_raw and d_logp unused.
 *   jh_sac_critic_loss      d_q, d_q_next [2][B]: y = r + (1 - d) * gamma * (min_i q_next_i - alpha * logp_next) (sac.py:186-211), alpha
 *                           from the block; loss_i = mean((y - q_i)^2), d_grad [2][B] = 2 (q_i - y) / B, d_y [B] (optional);
 *                           d_stats float32[4] = {loss_1, loss_2, max_b y (sac.py:213), arrival mark}.  1 <= B <= 2^20.
 *   jh_sac_actor_seed       d_q [2][B] = q_i(s, a), d_logp [B]: actor_loss = -mean(alpha * (-logp) + min(q_1, q_2)) (sac.py:241-242);
 *                           d_grad_q [2][B] = -1 / B on the smaller critic, half each on a tie (torch.min's backward); block[9] = alpha / B;
 *                           alpha_loss = log_alpha * mean(-logp - target_entropy) (sac.py:248); then, dynamic, alpha in use <-
 *                           exp(log_alpha) and ONE Adam step of log_alpha (sac.py:250-255).  d_stats float32[6] = {actor_loss,
 *                           alpha_loss, mean_Q = mean(min(q_1, q_2)), alpha (the refreshed one), entropy = mean(-logp), arrival mark}.
 *   jh_sac_sample_backward  d_grad_a (+ d_grad_a2 when not NULL: the two critics' action gradients) and block[9] -> d(mu_raw), d(ls_raw):
 *                           dz = da (1 - a^2) + c 2 a (1 - a^2) / (1 - a^2 + 1e-7); d(mu_raw) = dz where -5 <= mu_raw <= 5;
 *                           d(ls_raw) = (dz std eps - c) (1 - tanh(ls_raw)^2).                                                    */
#define JH_SAC_ALPHA_FLOATS 16
int jh_sac_sample(jh_ctx* ctx, int32_t B, int32_t A, const float* d_mu_raw, const float* d_ls_raw, const float* d_eps, float* d_a,
                  float* d_logp, jh_stream stream);
int jh_sac_critic_loss(jh_ctx* ctx, int32_t B, const float* d_q, const float* d_q_next, const float* d_logp_next, const float* d_reward,
                       const float* d_done, float gamma, const float* d_alpha, float* d_y, float* d_grad, float* d_stats, jh_stream stream);
int jh_sac_actor_seed(jh_ctx* ctx, int32_t B, const float* d_q, const float* d_logp, float* d_alpha, float* d_grad_q, float* d_stats,
                      jh_stream stream);
int jh_sac_sample_backward(jh_ctx* ctx, int32_t B, int32_t A, const float* d_grad_a, const float* d_grad_a2, const float* d_mu_raw,
                           const float* d_ls_raw, const float* d_eps, const float* d_a, const float* d_alpha, float* d_grad_mu_raw,
                           float* d_grad_ls_raw, jh_stream stream);
/* The networks (sac.py:75-95): a Gaussian policy, ONLINE ONLY (network/policy.py:38-55: head.l -> relu(l) -> mu, log_std; the module returns
 * clamp(mu, -5, 5) and exp(tanh(log_std))), and two continuous Q networks (network/q_network.py:23-39) with their targets.  MLP head,
 * scalar S, H % 4 == 0, A >= 1.  Caller-owned flat fp32 buckets: four of actor_floats (online, gradients, exp_avg, exp_avg_sq) and five of
 * 2 * critic_floats (online, target, gradients, exp_avg, exp_avg_sq), critic c at c * critic_floats (jh_sacnet_param_counts_for, which
 * needs no GPU).  jh_sacnet_segment: segments 0-7 of the actor bucket in the reference's state_dict order (head.l.weight [H][S],
 * head.l.bias, l.weight [H][H], l.bias, mu.weight [A][H], mu.bias, log_std.weight [A][H], log_std.bias; inside the bucket mu.weight and
 * log_std.weight are stored back to back, as are the two biases: one [2A][H] layer) and 8-15 of one critic as jh_acnet_segment's 6-13.
 * The critics share one optimizer block and one Adam launch (sac.py:136-140 gives both the same settings); the temperature block of the
 * jh_sac_* kernels lives inside the object.                                                                         */
typedef struct jh_sacnet jh_sacnet;
int jh_sacnet_param_counts_for(int32_t S, int32_t H, int32_t A, int64_t* actor_floats, int64_t* critic_floats);
int jh_sacnet_create(jh_ctx* ctx, int32_t S, int32_t H, int32_t A, int32_t max_batch, float* d_actor, float* d_actor_grads, float* d_actor_m,
                     float* d_actor_v, float* d_critics, float* d_critics_target, float* d_critics_grads, float* d_critics_m,
                     float* d_critics_v, jh_sacnet** out);
void jh_sacnet_destroy(jh_sacnet* n);
int32_t jh_sacnet_segment_count(void);
int jh_sacnet_segment(const jh_sacnet* n, int32_t i, int64_t* offset, int32_t* rows, int32_t* cols);
/* which: 0 the actor's Adam, 1 the critics'                                                                      */
int jh_sacnet_set_hyper(jh_sacnet* n, int32_t which, double lr, double beta1, double beta2, double eps, int64_t step, jh_stream stream);
int jh_sacnet_set_lr(jh_sacnet* n, int32_t which, double lr, jh_stream stream);
/* The temperature block as a whole (sac.py:97-109; target_entropy = -A is the object's own): log_alpha, the alpha in use, alpha_lr
 * (never decayed: sac.py:292-300), Adam's betas, eps, step count and moments, dynamic (use_dynamic_alpha).  jh_sacnet_get_alpha copies
 * the JH_SAC_ALPHA_FLOATS floats to host memory.  Both synchronise the stream: not for a capture.                  */
int jh_sacnet_set_alpha(jh_sacnet* n, double log_alpha, double alpha, double lr, double beta1, double beta2, double eps, int64_t step,
                        double m, double v, int32_t dynamic, jh_stream stream);
int jh_sacnet_get_alpha(jh_sacnet* n, float* h_block, jh_stream stream);
/* target critics <- online critics; update_target_soft (sac.py:271-275) as jh_td3_polyak on the critics' bucket     */
int jh_sacnet_sync_target(jh_sacnet* n, jh_stream stream);
int jh_sacnet_soft_update(jh_sacnet* n, double tau, jh_stream stream);
/* actor(x) -> d_mu, d_std [rows][A] (sac.py:148); critic_c(x, action) -> d_q [2][rows], which 0 online / 1 target; rows <= max_batch */
int jh_sacnet_actor_forward(jh_sacnet* n, const float* d_x, int32_t rows, float* d_mu, float* d_std, jh_stream stream);
int jh_sacnet_critic_forward(jh_sacnet* n, int32_t which, const float* d_x, const float* d_action, int32_t rows, float* d_q, jh_stream stream);
/* The critic update (sac.py:183-225): d_x = [state; next_state] (2B rows), d_eps [B][A] standard normals; a', logp' from the ONLINE actor
 * on next_state, y with the alpha in use; loss; backward; one Adam step of the critics.
 * -> d_y [B], d_q [2][B], d_a_next [B][A], d_logp_next [B] (all optional), d_stats as jh_sac_critic_loss.  12 launches. */
int jh_sacnet_critic_update(jh_sacnet* n, const float* d_x, const float* d_action, const float* d_reward, const float* d_done,
                            const float* d_eps, int32_t B, float gamma, float* d_y, float* d_q, float* d_a_next, float* d_logp_next,
                            float* d_stats, jh_stream stream);
/* The actor update and the temperature (sac.py:229-255): a, logp = sample(actor(state), d_eps), both critics AFTER their step, backward
 * through both critics' action inputs and through logp, the actor's Adam step; the seed advances the temperature block.  The critics'
 * parameters, gradient bucket and moments are not written.
 * -> d_action [B][A], d_logp [B], d_q [2][B] (all optional), d_stats as jh_sac_actor_seed.  16 launches.           */
int jh_sacnet_actor_update(jh_sacnet* n, const float* d_x, const float* d_eps, int32_t B, float* d_action, float* d_logp, float* d_q,
                           float* d_stats, jh_stream stream);

/* ------------------------------------------------------------------ V-MPO (vmpo.py:155-252)
 * Everything of one minibatch update between the policy-value net's forward and its backward, in ONE launch of ONE workgroup:
 * 1 <= B <= 1024 rows, 1 <= A <= 64; anything else is JH_ERR_ARG.  d_idx (int64 [B], or NULL for rows 0 .. B-1) selects the minibatch's
 * rows of the rollout-sized d_action, d_adv, d_value_old and OLD raw heads (the pre-pass of vmpo.py:122-153); the new raw heads and
 * d_value_pred are the minibatch's own [B][A] / [B].
 *   top half   the LOWER median of adv[idx] (sorted element (B - 1) / 2, torch.median) by rank counting; a row belongs to the top half
 *              exactly when adv > median (vmpo.py:174): ties at the median fall out, B == 1 or all-equal advantages leave it empty
 *   psi        exp((adv - max_top) / eta) / sum_top(...); eta_loss = eta eps_eta + eta (max_top / eta + log mean_top exp((adv - max_top) / eta)):
 *              the reference's formulas (vmpo.py:177-178, 194-196) wherever its float32 exp(adv / eta) is finite, and finite beyond
 *   losses     ret = adv + value_old as one float32 add (vmpo.py:153: AFTER the standardisation), critic = mean (v - ret)^2;
 *              actor = -sum_top psi logp; discrete: KL = sum_a pi_old (log pi_old - log pi), alpha_loss = mean[alpha_mu (eps_alpha_mu - KL) +
 *              alpha_mu KL]; continuous (mu = clamp(mu_raw, -5, 5), std = exp(tanh(log_std_raw)), policy_value.py:51-57):
 *              KLD_mu = 1/2 sum_a (mu - mu_old)^2 std_old^2 (vmpo.py:210-213 as written), KLD_sigma = 1/2 (sum_a std^2 / std_old^2 - A +
 *              log(prod ss / prod ss_old)), ss = 1 / std^2, each with its own multiplier and threshold.  Per-row terms in double, every sum a
 *              double with a fixed order: same bits every run.  Gradients with respect to the raw heads and d_value_pred.
 *   d_block    the Lagrange multipliers, a caller-owned device block of JH_VMPO_BLOCK_FLOATS floats the kernel reads and advances:
 *              [0-2] eta, alpha_mu, alpha_sigma   [3-5] exp_avg   [6-8] exp_avg_sq   [9-11] floors (min_eta, ..)   [12-14] thresholds
 *              (eps_eta, ..)   [15-17] 1 once the multiplier has taken an Adam step   [18-20] the gradients of the last step   [21-23] unused.
 *              After the sums one thread takes torch's single-tensor Adam step on each multiplier that has a gradient (a discrete policy
 *              leaves alpha_sigma, its moments and its flag untouched) with d_hyper's lr, betas (the doubles), eps and t = step + 1 -- the
 *              step the net's own Adam takes for this minibatch --, then x = max(x, floor) with NaN kept (reset_lgr_muls, vmpo.py:271-274).
 *   d_hyper    an 8-byte aligned optimizer block of 16 floats as jh_pponet_hyper_ptr returns it; only read.
 *   d_stats    optional float32[8] = {actor_loss, critic_loss, eta_loss, alpha_loss, eta', alpha_mu', alpha_sigma' (after the step and the
 *              floor), arrival mark 0}, the mark written last behind a system-scope fence (device-mapped host memory may receive it).
 *   d_mask     optional float32[B]: 1 where the row is in the top half.
 * Empty top half: no actor gradient, eta_loss and the stepped eta are NaN, as in the reference.                         */
#define JH_VMPO_BLOCK_FLOATS 24
int jh_vmpo_loss_discrete(jh_ctx* ctx, int32_t B, int32_t A, const float* d_logits, const float* d_value_pred, const int64_t* d_idx,
                          const float* d_action, const float* d_adv, const float* d_value_old, const float* d_logits_old, float* d_block,
                          const float* d_hyper, float* d_grad_logits, float* d_grad_value, float* d_stats, float* d_mask, jh_stream stream);
int jh_vmpo_loss_continuous(jh_ctx* ctx, int32_t B, int32_t A, const float* d_mu_raw, const float* d_log_std_raw, const float* d_value_pred,
                            const int64_t* d_idx, const float* d_action, const float* d_adv, const float* d_value_old, const float* d_mu_raw_old,
                            const float* d_log_std_raw_old, float* d_block, const float* d_hyper, float* d_grad_mu_raw,
                            float* d_grad_log_std_raw, float* d_grad_value, float* d_stats, float* d_mask, jh_stream stream);

/* ------------------------------------------------------------------ MPO, discrete policy
 * core/agent/mpo.py:312-386 between the six forwards and the two backwards, ONE launch of ONE workgroup.  R = batch_size * T rows, row
 * r = b * T + t (T = n_step with Retrace, 1 for 1step_TD).  float32 [R][A]: d_la / d_la_next / d_la_old = actor logits online(s),
 * online(s'), target(s); d_q / d_qt / d_qt_next = critic online(s), target(s), target(s').  float32 [R]: d_action (clamped into [0, A)),
 * d_reward, d_done, d_prob_b (the behaviour policy's probability of the taken action).  With pi = softmax(d_la), pi' = softmax(d_la_next),
 * pi_old = softmax(d_la_old), every log pi a log-softmax:
 *   c        = min(pi[a] / (prob_b + 1e-6), 1)                      the ONLINE policy, as the reference (mpo.py:324-330)
 *   Qret     = reward + gamma sum_a pi' qt_next (1 - done)          (mpo.py:332-339)
 *   retrace  for t = T - 2 .. 0: Qret[b,t] += gamma c[b,t+1] (Qret[b,t+1] - qt[b,t+1,a[b,t+1]]) (1 - done[b,t])   (mpo.py:347-355), one lane
 *            per trajectory out of LDS; retrace == 0: skipped
 *   critic   mean_r (q[r,a] - Qret)^2; d_grad_q[r][a] = 2 (q[r,a] - Qret) / R, zero elsewhere (every entry written)   (mpo.py:360)
 *   V = sum pi_old qt, At = qt - V, w = softmax(At / eta) taken as a constant; actor = -mean_r sum_a w log pi      (mpo.py:363-368)
 *   eta_loss = eta eps_eta + eta mean_r L_r, L_r = log sum_a pi_old exp(At / eta) formed around the row's largest At / eta: the reference's
 *            formula (mpo.py:370-372) wherever its float32 exp is finite, and finite beyond
 *   KLD = sum pi_old (log pi_old - log pi); alpha_loss = mean[alpha_mu (eps_alpha_mu - KLD) + alpha_mu KLD]          (mpo.py:379-384)
 *   d_grad_la = ((pi - w) + alpha_mu (pi - pi_old)) / R
 *   d eta = eps_eta + mean L_r - (1 / eta) mean sum_a u At, u = pi_old exp(At / eta) normalised; d alpha_mu = eps_alpha_mu - mean KLD
 * d_block is V-MPO's multiplier block (JH_VMPO_BLOCK_FLOATS, layout above) and d_hyper the ACTOR's optimizer block (jh_rbnet_hyper_ptr,
 * 8-byte aligned, only read): eta and alpha_mu take torch's single-tensor Adam step with its lr, betas, eps and t = step + 1, then their
 * floors (reset_lgr_muls, mpo.py:416-419), by the code jh_vmpo_loss_* use; alpha_sigma has no gradient for a discrete policy and is left alone.
 * d_stats optional float32[11] = {actor_loss, critic_loss, eta_loss, alpha_loss, eta', alpha_mu', alpha_sigma (after the step and the
 * floors), min q, max q, min At, max At over all [R][A] entries}.  Per-row terms in double, every mean a double sum in a fixed order: the
 * same bits every run.  JH_ERR_ARG, nothing launched: R < 1 or > 1024, T < 1, R % T != 0, A < 2 or A > 64.                         */
int jh_mpo_loss_discrete(jh_ctx* ctx, int32_t R, int32_t T, int32_t A, const float* d_la, const float* d_la_next, const float* d_la_old,
                         const float* d_q, const float* d_qt, const float* d_qt_next, const float* d_action, const float* d_reward,
                         const float* d_done, const float* d_prob_b, float* d_block, const float* d_hyper, float gamma, int32_t retrace,
                         float* d_grad_la, float* d_grad_q, float* d_stats, jh_stream stream);

/* ------------------------------------------------------------------ MPO, continuous policy
 * core/agent/mpo.py:199-309.  R and T as above, N = num_sample, A = action_size.  A Gaussian policy's RAW head is a float32 row [mu | log_std]
 * of 2A floats (jh_rbnet kind "gauss"); mu = clamp(raw, -5, 5), std = exp(tanh(raw)) (network/policy.py:53-55).  Both entries take
 * 1 <= R <= 1024, 1 <= N, N * R <= 8192 and 1 <= A <= 8; anything else is JH_ERR_ARG with nothing launched.
 *
 * jh_mpo_sample: ONE elementwise launch.  d_head_next = online(s'), d_head_old = target(s), each [R][2A]; d_eps [2][N][R][A] standard normals.
 *   d_zn = mu' + std' eps[0], d_a_next = tanh(d_zn)               (mpo.py:221-226)
 *   d_zt_add = mu_old + std_old eps[1], d_a_add = tanh(d_zt_add)  (mpo.py:255-258)          each [N][R][A], float32 arithmetic
 *
 * jh_mpo_loss_continuous: between the forwards and the two backwards, ONE launch of ONE workgroup, one row per thread.  d_head = online(s)
 * and d_head_old = target(s) [R][2A]; d_q = online critic(s, a), d_qt_a = target critic(s, a) [R]; d_qt_next = target critic(s', a_next),
 * d_qt_add = target critic(s, a_add) [N][R]; d_zt_add [N][R][A]; d_action [R][A] the stored (tanh-squashed) action; d_reward, d_done,
 * d_prob_b [R].
 *   z        = atanh(clamp(a, -(1 - 1e-7), 1 - 1e-7)), the bound as float32 rounds it; log_prob = sum_A log N(z; mu, std)
 *   c        = min(exp(log_prob) / (prob_b + 1e-6), 1)             the ONLINE policy, as the reference (mpo.py:203-206, 233)
 *   Qret     = reward + gamma mean_n qt_next (1 - done), then the Retrace scan of jh_mpo_loss_discrete with qt_a  (mpo.py:235-253)
 *   critic   mean_r (q - Qret)^2; d_grad_q[r] = 2 (q - Qret) / R
 *   At = qt_add - mean_n qt_add, w = softmax_n(At / eta) taken as a constant; actor = -mean_r sum_n w log N(zt_add[n]; mu, std)
 *   eta_loss = eta eps_eta + eta mean_r log mean_n exp(At / eta), the log-mean formed around the row's largest At / eta: the reference's
 *            formula (mpo.py:276-278) wherever its float32 exp is finite, and finite beyond
 *   KLD_mu = 1/2 sum_A (mu - mu_old)^2 std_old^2; KLD_sigma = 1/2 (sum_A std^2 / std_old^2 - A + log(prod ss / prod ss_old)), ss = 1 / std^2,
 *            the log of the product ratio formed as the sum of the logs (finite at any A, equal elsewhere); alpha_loss = mean[alpha_mu
 *            (eps_alpha_mu - KLD_mu) + alpha_mu KLD_mu] + mean[alpha_sigma (eps_alpha_sigma - KLD_sigma) + alpha_sigma KLD_sigma]  (mpo.py:280-309)
 *   d_grad_head [R][2A]: d(actor + alpha_mu KLD_mu + alpha_sigma KLD_sigma)/d(raw head of online(s)), the multipliers as constants: zero in mu
 *            where the raw value lies outside [-5, 5], through 1 - tanh^2 for log_std
 *   d eta = eps_eta + mean L_r - (1 / eta) mean_r sum_n w At; d alpha_mu = eps_alpha_mu - mean KLD_mu; d alpha_sigma = eps_alpha_sigma - mean KLD_sigma
 * d_block and d_hyper as jh_mpo_loss_discrete; ALL THREE multipliers take their Adam step and then their floors.
 * d_stats optional float32[11] as jh_mpo_loss_discrete; min / max q over d_q [R], min / max At over all [N][R] entries.  Per-row terms in
 * double, every mean a double sum in a fixed order, no atomics: the same bits every run.  The [N][R] tables are read from global memory
 * (one reader per element, consecutive across a wavefront); LDS holds the scan's per-row state.
 * JH_ERR_ARG besides the shape rule above: T < 1, R % T != 0.                                                                       */
int jh_mpo_sample(jh_ctx* ctx, int32_t R, int32_t N, int32_t A, const float* d_head_next, const float* d_head_old, const float* d_eps, float* d_zn,
                  float* d_zt_add, float* d_a_next, float* d_a_add, jh_stream stream);
int jh_mpo_loss_continuous(jh_ctx* ctx, int32_t R, int32_t T, int32_t N, int32_t A, const float* d_head, const float* d_head_old, const float* d_q,
                           const float* d_qt_a, const float* d_qt_next, const float* d_qt_add, const float* d_zt_add, const float* d_action,
                           const float* d_reward, const float* d_done, const float* d_prob_b, float* d_block, const float* d_hyper, float gamma,
                           int32_t retrace, float* d_grad_head, float* d_grad_q, float* d_stats, jh_stream stream);

/* ------------------------------------------------------------------ REINFORCE: the return scan and the policy-gradient losses
 * core/agent/reinforce.py:83-113 between the network's forward and its backward, over the T rows of ONE episode (T differs from learn to
 * learn; 1 <= T <= 65536).  The number of launches of each entry does not depend on T.
 * jh_reinforce_returns: d_ret[t] = d_reward[t] + gamma d_ret[t + 1] over ALL T rows (no reset at a done and no done column: the reference
 * scans whatever its buffer holds, reinforce.py:90-92); standardize != 0: then (ret - mean) / (std + 1e-7) with the population standard
 * deviation, numpy's ret.std() (reinforce.py:93-94).  Scan, mean and variance in double (gamma is a double: numpy multiplies by the Python
 * float), rounded once into float32 d_ret [T].  ONE workgroup: a chunked scan, per-thread local scans whose carries are combined with
 * gamma^len by shuffles and through LDS; no float atomics, the same bits every run.  T = 1 with standardize gives exactly 0.
 * jh_reinforce_loss_discrete: d_logits [T][A], d_action [T] as float (clamped into [0, A)), d_ret [T]:
 *   loss = -mean_t(logp[t][a_t] ret[t]), logp a log-softmax (the reference takes log(softmax): finite where its float32 pi underflows)
 *   d_grad_logits[t][k] = ret[t] (pi[t][k] - [k == a_t]) / T                                                     2 <= A <= 64
 * jh_reinforce_loss_continuous: d_head [T][2A] = [mu_raw | log_std_raw], d_action [T][A], d_ret [T]:
 *   mu = clamp(mu_raw, -5, 5), std = exp(tanh(log_std_raw)) (network/policy.py:49-55), z = atanh(clamp(action, -1 + 1e-7, 1 - 1e-7)) with the
 *   bounds as float32 values, loss = -mean over T * A of (Normal(mu, std).log_prob(z) ret[t])
 *   d_grad_head [T][2A] with respect to the raw head: zero where mu_raw is clamped, through tanh and exp for the std half  1 <= A <= 32
 * Both losses: per-row terms in double; the mean is a two-stage sum in a fixed order (workgroup partials in the context's scratch, then one
 * thread over them in index order); d_stats float32[JH_REINFORCE_STATS_FLOATS] = {loss, T} is written by the second stage, so nothing is
 * read back by the call.  JH_ERR_ARG, nothing launched: T < 1 or T > 65536, A outside its range, a null pointer.                      */
#define JH_REINFORCE_STATS_FLOATS 2
#define JH_REINFORCE_MAX_ROWS 65536
int jh_reinforce_returns(jh_ctx* ctx, int32_t T, const float* d_reward, double gamma, int32_t standardize, float* d_ret, jh_stream stream);
int jh_reinforce_loss_discrete(jh_ctx* ctx, int32_t T, int32_t A, const float* d_logits, const float* d_action, const float* d_ret,
                               float* d_grad_logits, float* d_stats, jh_stream stream);
int jh_reinforce_loss_continuous(jh_ctx* ctx, int32_t T, int32_t A, const float* d_head, const float* d_action, const float* d_ret,
                                 float* d_grad_head, float* d_stats, jh_stream stream);

/* ------------------------------------------------------------------ R2D2: the LSTM recurrence and the sequence loss
 * torch.nn.LSTM(H + A -> H, one layer) as core/network/r2d2.py:13-15, 38 runs it, one time step per launch.  Gate order i, f, g, o.
 * jh_lstm_step, for every segment s < n_segs (up to JH_LSTM_MAX_SEGS row groups in ONE launch, each with weights and buffers of its own:
 * the online rows and the target rows of R2D2.learn(), r2d2.py:117-129; a segment of 0 rows is skipped):
 *   gates = xproj + h_prev W_hh^T      xproj [rows] rows of 4H floats, ld_x floats apart: the input projection x_t W_ih^T + b_ih + b_hh,
 *                                      which does not depend on the recurrence; w_hh [4H][H]; h_prev, c_prev [rows][H]
 *   i, f, o = sigmoid, g = tanh;  c_out = f c_prev + i g;  h_out = o tanh(c_out)            [rows][H]
 *   gates_out [rows][4H] (NULL ok) = the ACTIVATED gates, what the backward needs
 * A workgroup owns 16 rows x 16 hidden units across all four gates: the product runs on the fp32 MFMA, the cell in the same launch.
 * H % 4 == 0, 4 <= H <= 4096; w_hh and h_prev 16-byte aligned.                                                                   */
#define JH_LSTM_MAX_SEGS 4
typedef struct {
  int32_t rows, ld_x;
  const float *xproj, *w_hh, *h_prev, *c_prev;
  float *h_out, *c_out, *gates_out;
} jh_lstm_seg;
int jh_lstm_step(jh_ctx* ctx, int32_t H, int32_t n_segs, const jh_lstm_seg* segs, jh_stream stream);
/* One step of backpropagation through time, t descending, one launch per trained step:
 *   dh_t = d_dh_ext (gradient reaching h_t from the layers above; NULL: 0) + d_dgates_next W_hh (d_dgates_next [R][4H] = this function's
 *          d_dgates of step t + 1; NULL at the last step)
 *   dc_t = d_dc_in (this function's d_dc_prev of step t + 1; NULL: 0) + dh_t o (1 - tanh(c_t)^2)
 *   d_dgates [R][4H] = the gradient of the PRE-activation gates of step t; d_dc_prev [R][H] = dc_t f
 * with d_gates [R][4H] the activated gates of step t, d_c_prev = c_{t-1}, d_c = c_t [R][H].  The recurrent product sits in the launch
 * that consumes it, so that a workgroup needs the saved activations of its own 16 units only.  dW_hh, dW_ih, the bias gradients and dx
 * are products over ALL trained steps' d_dgates at once (the tile engine), not this function's.                                  */
int jh_lstm_step_backward(jh_ctx* ctx, int32_t R, int32_t H, const float* d_dgates_next, const float* d_w_hh, const float* d_dh_ext,
                          const float* d_dc_in, const float* d_gates, const float* d_c_prev, const float* d_c, float* d_dgates,
                          float* d_dc_prev, jh_stream stream);
/* R2D2.learn() between the three sequence passes and the backward (r2d2.py:113-159), T = seq_len - n_burn_in trained steps:
 * d_q / d_next_q / d_next_target_q float32 [T][B][A] (time-major) = online over state[:, :seq_len], online and target over
 * state[:, n_step:]; d_action / d_reward / d_done float32 [B][seq_len + n_step - 1] as the replay row holds them (actions clamped into
 * [0, A)); d_weights float32 [B].  Per row b and step t: a* = first maximum of next_q, y = h(fold(h^-1(next_target_q[a*]))) with the
 * n-step fold over reward / done [i + n_burn_in + t], i = n_step - 1 .. 0, and the value rescale h(x) = sign(x)(sqrt(|x| + 1) - 1) +
 * eps x (r2d2.py:304-313); td = |y - q[action]|.  Outputs: d_prio float64 [B] = (eta max_t td + (1 - eta) mean_t td)^alpha;
 * d_grad_q [T][B][A], every entry written, non-zero only at the LAST step's taken action: 2 w_b (q - y) / B, the gradient of
 * loss = mean_b w_b td[b, T - 1]^2; d_td [B][T] (NULL ok); d_stats float32[8] = {loss, max_Q over all taken q, 0, 0, 0, mark, 0, mark}, the
 * payload fenced before the arrival marks as jh_qr_loss leaves them.  Per-row terms in double, rounded once.  A departure on purpose:
 * sqrt(1 + y) - 1 inside h^-1 (and sqrt(|x| + 1) - 1 inside h) is formed without its cancellation; the float32 expression as written is
 * off by up to 2e-4 of the largest target at |Q| = 0.05.  One workgroup, no atomics: the same bits every run.
 * JH_ERR_ARG, nothing launched: B < 1 or > 1024, T < 1, seq_len > 128, A < 2 or > 64, n_step < 1.                                  */
int jh_r2d2_loss(jh_ctx* ctx, int32_t B, int32_t T, int32_t A, int32_t n_burn_in, int32_t n_step, const float* d_q, const float* d_next_q,
                 const float* d_next_target_q, const float* d_action, const float* d_reward, const float* d_done, const float* d_weights,
                 float gamma, float eta, float alpha, float eps, float* d_grad_q, double* d_prio, float* d_td, float* d_stats,
                 jh_stream stream);

/* The recurrent dueling network of R2D2 (core/network/r2d2.py:8-53) with an MLP head over caller-owned flat fp32 buckets (online and target
 * parameters, gradients, exp_avg, exp_avg_sq) of jh_r2d2net_param_count_for floats (needs no GPU; -1 for bad sizes), every segment 16-byte
 * aligned, in the library's own order (jh_r2d2net_segment_count / _segment):
 *   head.l.weight [H][S], head.l.bias [H], lstm.weight_ih_l0 [4H][H + A], lstm.weight_hh_l0 [4H][H], lstm.bias_ih_l0 [4H], lstm.bias_hh_l0 [4H],
 *   l.weight [H][H], l.bias [H], l1_a.weight, l1_v.weight [H][H], l1_a.bias, l1_v.bias [H], l2_a.weight [A][H], l2_a.bias [A], l2_v.weight [1][H],
 *   l2_v.bias [1]     (l1_a | l1_v next to each other: one [2H][H] layer to the kernels)
 * H % 4 == 0, 2 <= A <= 64, max_batch <= 1024, 2 <= seq_len <= 128, 1 <= n_burn_in < seq_len, n_step >= 1.  Every buffer is allocated at
 * create; nothing is allocated afterwards, so learn_forward / backward / optim_step may be captured into a graph.                     */
typedef struct jh_r2d2net jh_r2d2net;
int64_t jh_r2d2net_param_count_for(int32_t S, int32_t H, int32_t A);
int jh_r2d2net_create(jh_ctx* ctx, int32_t S, int32_t H, int32_t A, int32_t max_batch, int32_t seq_len, int32_t n_burn_in, int32_t n_step,
                      float* d_params, float* d_target, float* d_grads, float* d_m, float* d_v, jh_r2d2net** out);
void jh_r2d2net_destroy(jh_r2d2net* n);
int32_t jh_r2d2net_segment_count(void);
int jh_r2d2net_segment(const jh_r2d2net* n, int32_t i, int64_t* offset, int32_t* rows, int32_t* cols);
int jh_r2d2net_set_hyper(jh_r2d2net* n, double lr, double beta1, double beta2, double eps, int64_t step, jh_stream stream);
int jh_r2d2net_set_lr(jh_r2d2net* n, double lr, jh_stream stream);
int jh_r2d2net_sync_target(jh_r2d2net* n, jh_stream stream);
/* The three sequence passes of R2D2.learn() (r2d2.py:117-129 through get_q, r2d2.py:289-302), seq_len steps each, run in lockstep: the
 * online network over steps [0, seq_len) from (d_hidden_h, d_hidden_c), the online and the target network over steps [n_step, n_step +
 * seq_len) from (d_next_hidden_h, d_next_hidden_c).  d_state [B][seq_len + n_step][S], d_onehot [B][seq_len + n_step][A] (the previous
 * action's one-hot), the stored states [B][H].  The head and the input projection run once per network over all stored steps (the
 * second online pass is the first one's input n_step steps on), then one jh_lstm_step launch of three row segments per time step, then
 * the layers above the LSTM over the seq_len - n_burn_in trained steps of all three passes.
 * -> d_q [3][seq_len - n_burn_in][B][A], time-major: what jh_r2d2_loss takes.  seq_len + 7 launches.                                  */
int jh_r2d2net_learn_forward(jh_r2d2net* n, const float* d_state, const float* d_onehot, const float* d_hidden_h, const float* d_hidden_c,
                             const float* d_next_hidden_h, const float* d_next_hidden_c, int32_t B, float* d_q, jh_stream stream);
/* Backward of d_q[0] of the last jh_r2d2net_learn_forward: d_g [seq_len - n_burn_in][B][A] -> the gradient bucket, every segment written.
 * One jh_lstm_step_backward launch per trained step, t descending; the burn-in steps take no gradient (r2d2.py:290-295).  dW_hh, dW_ih, the
 * bias gradients (bias_hh_l0's is a copy of bias_ih_l0's) and the head's are products over all trained steps at once.                 */
int jh_r2d2net_backward(jh_r2d2net* n, const float* d_g, jh_stream stream);
/* [clip_grad_norm_(max_norm) over the bucket (0: none),] torch.optim.Adam's step, the step counter advanced on the device.            */
int jh_r2d2net_optim_step(jh_r2d2net* n, float max_norm, jh_stream stream);
/* R2D2.act's network call (r2d2.py:62-66) for N <= max_batch actor rows, one time step: d_x [N][S], d_prev_onehot [N][A] (zeros at an episode
 * start), the carried state d_h_in / d_c_in [N][H] (16-byte aligned) -> d_q [N][A], d_h_out / d_c_out [N][H]; all on the device.  Its
 * buffers are its own: it may run between a learn_forward and its backward.                                                          */
int jh_r2d2net_act_step(jh_r2d2net* n, const float* d_x, const float* d_prev_onehot, const float* d_h_in, const float* d_c_in, int32_t N, float* d_q,
                        float* d_h_out, float* d_c_out, jh_stream stream);

/* ------------------------------------------------------------------ ICM-PPO's curiosity module
 * core/network/icm.py:153-218 (ICM_MLP) with its helpers icm.py:8-34 (the feature trunk: fc1 -> bn1 -> ELU -> fc2 -> bn2 -> ELU on s; the
 * SAME fc1 and fc2 on s' with bn1_next after fc1 and no batch norm after fc2), icm.py:99-142 (forward and inverse model), icm.py:145-150
 * (ri_update), core/network/utils.py:6-52 (RewardForwardFilter, RunningMeanStd) and core/network/rnd.py:9-10 (normalize_obs), as
 * icm_ppo.py:96-102 and icm_ppo.py:177-199 use them.  The feature size is 256.  Every batch norm uses BATCH statistics (the module is
 * never put into eval mode): biased variance, eps 1e-5; the running statistics advance with momentum 0.1 and the unbiased variance.
 * Caller-owned flat fp32 buckets (params, gradients, exp_avg, exp_avg_sq) of jh_icmnet_param_count_for floats (needs no GPU; -1 for bad
 * sizes) hold the trainable tensors in the reference's registration order, weight then bias, every segment 16-byte aligned:
 *   fc1 [H][S], fc2 [256][H], forward_fc1 [H][256 + a], forward_fc2 [256][H + a], inverse_fc1 [H][512], inverse_fc2 [A][H]
 *   and, with JH_ICM_BATCH_NORM, bn1 [H], bn2 [256], bn1_next [H]         (a = 1, the action index as a float | A action columns)
 * = 12 or 18 segments (jh_icmnet_segment_count / _segment).  continuous 0: 1 <= A <= 39, 1: 1 <= A <= 19; H % 4 == 0;
 * max_batch <= 8192 rows per call.  The statistics block (device, jh_icmnet_stats_floats floats, _stats_get / _stats_set copy it whole and
 * synchronise the stream): rms_obs mean [S], var [S], count | rms_ri mean, var, count | rewems [W] | running mean [C], var [C] of bn1
 * (C = H), bn2 (256), bn1_next (H).  A fresh object holds a fresh module's values (counts 1e-4, running variances 1).              */
typedef struct jh_icmnet jh_icmnet;
#define JH_ICM_OBS_NORMALIZE 1
#define JH_ICM_RI_NORMALIZE 2
#define JH_ICM_BATCH_NORM 4
int64_t jh_icmnet_param_count_for(int32_t S, int32_t H, int32_t A, int32_t continuous, int32_t batch_norm);
int jh_icmnet_create(jh_ctx* ctx, int32_t S, int32_t H, int32_t A, int32_t continuous, int32_t num_workers, int32_t max_batch, int32_t flags,
                     double eta, double gamma, float* d_params, float* d_grads, float* d_m, float* d_v, jh_icmnet** out);
void jh_icmnet_destroy(jh_icmnet* n);
int32_t jh_icmnet_segment_count(const jh_icmnet* n);
int jh_icmnet_segment(const jh_icmnet* n, int32_t i, int64_t* offset, int32_t* rows, int32_t* cols);
/* the module's own Adam (icm_ppo.py:76); learning_rate_decay never reaches it (base.py:103-104)                     */
int jh_icmnet_set_hyper(jh_icmnet* n, double lr, double beta1, double beta2, double eps, int64_t step, jh_stream stream);
int jh_icmnet_set_lr(jh_icmnet* n, double lr, jh_stream stream);
int64_t jh_icmnet_stats_floats(const jh_icmnet* n);
int jh_icmnet_stats_get(jh_icmnet* n, float* h_out, jh_stream stream);
int jh_icmnet_stats_set(jh_icmnet* n, const float* h_in, jh_stream stream);
/* icm.update_rms_obs(next_state) (icm_ppo.py:98): the per-feature mean and UNBIASED variance of d_next_state [rows][S] merged into
 * rms_obs in float32, operation for operation (utils.py:31-52).  2 <= rows <= max_batch.  One launch.                  */
int jh_icmnet_obs_update(jh_icmnet* n, const float* d_next_state, int32_t rows, jh_stream stream);
/* r_i, _, _ = icm(state, action, next_state, update_ri=True) and the mix (icm_ppo.py:99-102) over a whole rollout, no gradient:
 *   r_i = eta / 2 sum_j |x_forward - phi'|; the filter per worker w over its rows w T .. w T + T - 1 (T = rows / W); rms_ri merged with what
 *   the reference's stack really holds -- RewardForwardFilter.update returns the Parameter itself, so T copies of the FINAL rewems:
 *   batch count T W, mean mean_w rewems_w, unbiased variance over the T W entries --; with JH_ICM_RI_NORMALIZE r_i /= sqrt(rms_ri.var) +
 *   1e-7 (the variance AFTER this update); d_reward [rows] <- extrinsic_coeff * d_reward + intrinsic_coeff * r_i in place.
 * d_action [rows] (the index as a float) | [rows][A].  Optional outputs: d_ri_mean [1] = mean(r_i) as mixed, d_ri_raw [rows] before and
 * d_ri [rows] after the normalisation.  The batch norms' running statistics advance once.  JH_ERR_ARG, nothing launched: rows < 2,
 * rows > max_batch, rows % W != 0.  9 launches.                                                                         */
int jh_icmnet_reward(jh_icmnet* n, const float* d_state, const float* d_next_state, const float* d_action, int32_t rows, float extrinsic_coeff,
                     float intrinsic_coeff, float* d_reward, float* d_ri_mean, float* d_ri_raw, float* d_ri, jh_stream stream);
/* One minibatch (icm_ppo.py:177, 185, 194-199) on rows d_idx[0 .. b) of the n_rows-row rollout arrays (NULL: rows 0 .. b - 1; an index is
 * clamped into the rollout): forward, l_f = mse(x_forward, phi'.detach()), l_i = cross entropy against the action index | mse against the
 * action, backward of beta l_f + (1 - beta) l_i, clip_grad_norm_(max_norm) over the trainable bucket (0: none), Adam.  d_stats optional
 * float32[4] = {l_f, l_i, 0, arrival mark 0}, the mark written last behind a system-scope fence (device-mapped host memory may receive
 * it).  JH_ERR_ARG, nothing launched: b < 1, b < 2 under batch norm, b > max_batch.  16 launches.                       */
int jh_icmnet_update(jh_icmnet* n, const float* d_state, const float* d_next_state, const float* d_action, const int64_t* d_idx, int32_t b,
                     int64_t n_rows, double beta, float max_norm, float* d_stats, jh_stream stream);

/* ------------------------------------------------------------------ RND-PPO's distillation module and its PPO kernels
 * core/network/rnd.py:173-225 (RND_MLP) with rnd.py:9-52 (normalize_obs; predictor and frozen target, each fc1 [H][S] -> bn1 -> ReLU ->
 * fc2 [256][H] -> bn2 -> ReLU), rnd.py:159-164 (the reward filter) and utils.py:6-52, as rnd_ppo.py:119-120 and rnd_ppo.py:251-266 use
 * them.  All four batch norms use BATCH statistics and advance their running statistics on every forward, the target's included (the
 * module is never put into eval mode).  Caller-owned flat fp32 buckets of jh_rndnet_param_count_for floats (needs no GPU; -1 for bad
 * sizes) in 16 segments, every offset a multiple of 4 floats: fc1_predict [H][S], [H], fc2_predict [256][H], [256], bn1_predict [H], [H],
 * bn2_predict [256], [256], then the same eight of the target; without JH_RND_BATCH_NORM the batch norms' segments have 0 rows.  Only
 * the first jh_rndnet_trainable_floats floats (the predictor's eight) get gradients, moments and Adam steps, and clip_grad_norm_ runs
 * over exactly those.  H % 4 == 0; max_batch <= 8192 rows per call.  The statistics block (device, jh_rndnet_stats_floats floats):
 *   rms_obs mean [S], var [S], count | rms_ri mean, var, count | rff.rewems [W] | running mean, var of bn1_predict [H], bn2_predict
 *   [256], bn1_target [H], bn2_target [256]                                                                                            */
typedef struct jh_rndnet jh_rndnet;
#define JH_RND_OBS_NORMALIZE 1
#define JH_RND_RI_NORMALIZE 2
#define JH_RND_BATCH_NORM 4
int64_t jh_rndnet_param_count_for(int32_t S, int32_t H, int32_t batch_norm);
int jh_rndnet_create(jh_ctx* ctx, int32_t S, int32_t H, int32_t num_workers, int32_t max_batch, int32_t flags, double gamma_i, float* d_params,
                     float* d_grads, float* d_m, float* d_v, jh_rndnet** out);
void jh_rndnet_destroy(jh_rndnet* n);
int32_t jh_rndnet_segment_count(const jh_rndnet* n);
int jh_rndnet_segment(const jh_rndnet* n, int32_t i, int64_t* offset, int32_t* rows, int32_t* cols);
int64_t jh_rndnet_trainable_floats(const jh_rndnet* n);
/* the module's own Adam (rnd_ppo.py:83); learning_rate_decay never reaches it (base.py:103-104)                     */
int jh_rndnet_set_hyper(jh_rndnet* n, double lr, double beta1, double beta2, double eps, int64_t step, jh_stream stream);
int jh_rndnet_set_lr(jh_rndnet* n, double lr, jh_stream stream);
int64_t jh_rndnet_stats_floats(const jh_rndnet* n);
int jh_rndnet_stats_get(jh_rndnet* n, float* h_out, jh_stream stream);
int jh_rndnet_stats_set(jh_rndnet* n, const float* h_in, jh_stream stream);
/* rnd.update_rms_obs(next_state) (rnd_ppo.py:119), as jh_icmnet_obs_update.  JH_ERR_ARG, nothing launched: rows < 2, rows > max_batch. */
int jh_rndnet_obs_update(jh_rndnet* n, const float* d_next_state, int32_t rows, jh_stream stream);
/* r_i = rnd(next_state, update_ri=True) (rnd_ppo.py:120) over a whole rollout of rows = W T rows, no gradient: r_i = mean_f (p - t)^2,
 * the reward filter and rms_ri exactly as jh_icmnet_reward documents them (T copies of the FINAL rewems), then with JH_RND_RI_NORMALIZE
 * r_i /= sqrt(rms_ri.var) + 1e-7.  Writes d_ri [rows]; optional d_ri_mean [1] = mean(r_i), d_ri_raw [rows] = r_i before the
 * normalisation.  JH_ERR_ARG, nothing launched: rows < 2, rows > max_batch, rows % num_workers != 0.  7 launches.      */
int jh_rndnet_reward(jh_rndnet* n, const float* d_next_state, int32_t rows, float* d_ri, float* d_ri_mean, float* d_ri_raw, jh_stream stream);
/* One minibatch (rnd_ppo.py:251-252, 261-266) on rows d_idx[0 .. b) of the n_rows-row next_state array (NULL: rows 0 .. b - 1; an index
 * is clamped into the rollout): forward of both networks, loss = mean of the normalised r_i, backward through the predictor,
 * clip_grad_norm_(max_norm) over the predictor's tensors (0: none), Adam.  d_stats optional float32[4] = {r_i mean, 0, 0, arrival mark
 * 0}, the mark written last behind a system-scope fence.  JH_ERR_ARG, nothing launched: b < 1, b < 2 under batch norm, b > max_batch.
 * 12 launches.                                                                                                                       */
int jh_rndnet_update(jh_rndnet* n, const float* d_next_state, const int64_t* d_idx, int32_t b, int64_t n_rows, float max_norm, float* d_stats,
                     jh_stream stream);
/* rnd_ppo.py:153-166 behind two jh_gae calls with standardize off: d_adv [W T] = extrinsic_coeff d_adv_e + intrinsic_coeff d_adv_i, with
 * standardize (adv - mean) / (std + 1e-7) per row of T = n_step entries (UNBIASED std); d_means[0] = mean(d_ret), [1] = mean(d_ret_i).   */
int jh_rnd_adv_mix(jh_ctx* ctx, int32_t W, int32_t T, float extrinsic_coeff, float intrinsic_coeff, int32_t standardize, const float* d_adv_e,
                   const float* d_adv_i, const float* d_ret, const float* d_ret_i, float* d_adv, float* d_means, jh_stream stream);
/* jh_ppo_loss_packed with the second critic (rnd_ppo.py:201-249): d_heads [B][ld] = (head0 [A] | head1 [A] (continuous) | v | v_i |
 * padding), the gradient of actor + vf_coef (critic_e + critic_i) + ent_coef entropy goes back in the same layout (padding columns are not
 * written); each critic is the max of the MEANS of its plain and its clipped squared error.  d_stats optional float32[8] = {0, actor,
 * critic_e, critic_i, entropy, max ratio, min prob, 0}.  Discrete 2 <= A <= 64, continuous 1 <= A <= 32.  One launch.                 */
int jh_rnd_ppo_loss_packed(jh_ctx* ctx, int32_t continuous, int32_t B, int32_t A, const float* d_heads, int32_t ld, const int64_t* d_idx,
                           const float* d_action, const float* d_adv, const float* d_ret, const float* d_ret_i, const float* d_value_old,
                           const float* d_vi_old, const float* d_logp_old, float eps_clip, float vf_coef, float ent_coef, float* d_grad_heads,
                           float* d_stats, jh_stream stream);

/* ------------------------------------------------------------------ native policy-value MLP
 * The encoder of the PPO configs (core/network/head.py:6-18 MLP head + policy_value.py:8-57):
 * S -> H relu -> H relu -> {A logits | A mu, A log_std} + value, as hand-written kernels
 * (fp32-input MFMA for the H x H contractions).  Parameters, gradients and Adam moments are FLAT
 * fp32 device buckets borrowed from the caller, laid out in the reference's state_dict order:
 *   head.l.weight [H][S], head.l.bias [H], l.weight [H][H], l.bias [H],
 *   pi.weight [A][H], pi.bias [A]                              (discrete)
 *   mu.weight, mu.bias, log_std.weight [A][H], log_std.bias    (continuous)
 *   v.weight [1][H], v.bias [1]
 * so one RCCL all-reduce covers the whole gradient and torch views give state_dict()/ckpt compat. */
typedef struct jh_pponet jh_pponet;
int64_t jh_pponet_param_count(int32_t S, int32_t H, int32_t A, int32_t continuous);
int jh_pponet_create(jh_ctx* ctx, int32_t S, int32_t H, int32_t A, int32_t continuous, int32_t max_rows,
                     float* d_params, float* d_grads, float* d_m, float* d_v, uint64_t seed, jh_pponet** out);
void jh_pponet_destroy(jh_pponet* n);
/* Adam hyper-parameters live in device memory (a captured graph can be replayed while the host
 * anneals lr, core/agent/base.py:93-111).  step >= 0 sets Adam's step counter (checkpoint restore),
 * step < 0 keeps it.  Hyper-parameters are DOUBLES: torch.optim derives (1 - beta) and the bias
 * corrections 1 - beta^t in Python double arithmetic before its fp32 kernels see them, and so does this
 * library ((1.f - 0.999f) would be off by 1.3e-5 relative, visible in exp_avg_sq).                */
int jh_pponet_set_hyper(jh_pponet* n, double lr, double beta1, double beta2, double eps, double step, jh_stream stream);
int jh_pponet_set_lr(jh_pponet* n, double lr, jh_stream stream);
/* Forward of B rows of d_x [*, S] (gathered through d_idx int64[B] when non-NULL: the `state[idx]`
 * of ppo.py:122).  Writes the RAW heads: d_head0 = logits | mu_raw [B][A], d_head1 = log_std_raw
 * (continuous only), d_value [B].  Activations stay in the net for a following backward.     */
int jh_pponet_forward(jh_pponet* n, int32_t B, const float* d_x, const int64_t* d_idx, float* d_head0,
                      float* d_head1, float* d_value, jh_stream stream);
/* Backward of the last forward given d(loss)/d(raw heads); OVERWRITES the flat gradient bucket
 * (== optimizer.zero_grad + loss.backward, ppo.py:164-165).                                    */
int jh_pponet_backward(jh_pponet* n, int32_t B, const float* d_x, const int64_t* d_idx, const float* d_g_head0,
                       const float* d_g_head1, const float* d_g_value, jh_stream stream);
/* torch.nn.utils.clip_grad_norm_(max_norm) (skipped if max_norm <= 0) + torch.optim.Adam.step
 * on the flat buckets (ppo.py:166-169).  d_norm_out: optional device float, pre-clip norm.      */
int jh_pponet_adam_step(jh_pponet* n, float max_norm, float* d_norm_out, jh_stream stream);
/* One whole PPO minibatch update (ppo.py:122-169: forward of `state[idx]`, clipped loss forward +
 * backward, encoder backward, clip_grad_norm_, Adam) in 4-5 launches (csrc/jh_ppo_mb.hip): layer 1 is
 * generated in the operand fetch, the heads never exist as tensors (per-column-tile partials are summed
 * by the loss kernel), d(loss)/d(h2) is generated in the operand fetch of its two consumers, and ONE
 * backward grid produces every gradient (dh1 only as the per-row-tile partial sums of dW1 / db1).
 * B <= 1024, hidden_size % 32 == 0.  d_idx may be NULL (rows already gathered: jh_ppo_minibatch_rows).
 * do_adam == 0 stops after the backward with a complete gradient bucket (data-parallel: all-reduce, then
 * jh_pponet_adam_step).  d_stats float32[8] as in jh_ppo_loss_*.                                    */
int jh_pponet_ppo_update(jh_pponet* n, int32_t B, const float* d_x, const int64_t* d_idx, const float* d_action,
                         const float* d_adv, const float* d_ret, const float* d_value_old, const float* d_logp_old,
                         float eps_clip, float vf_coef, float ent_coef, float max_norm, int32_t do_adam, float* d_stats,
                         jh_stream stream);
/* The minibatch update of ppo.py:122-169 for ANY number of rows up to max_rows (config.ppo.mujoco: 2048-row minibatches) in one call: forward, the loss --
 * forward and backward in ONE launch whatever B (both critic branches' value gradients are kept per row, the last workgroup to arrive reduces the
 * partials and leaves the branch weights; the backward's first kernel forms the value gradient) --, backward, [clip_grad_norm_ + Adam unless
 * do_adam == 0].  Bit-identical to jh_pponet_forward -> jh_ppo_loss_discrete / _continuous -> jh_pponet_backward -> jh_pponet_adam_step, one launch less. */
int jh_pponet_ppo_update_rows(jh_pponet* n, int32_t B, const float* d_x, const int64_t* d_idx, const float* d_action, const float* d_adv, const float* d_ret,
                              const float* d_value_old, const float* d_logp_old, float eps_clip, float vf_coef, float ent_coef, float max_norm,
                              int32_t do_adam, float* d_stats, jh_stream stream);
/* jh_pponet_ppo_update for DATA-PARALLEL learners with the reference's critic exactly: core/agent/ppo.py:147-154 takes
 * max(mean(e1), mean(e2)) over the WHOLE minibatch -- a max of two means, so with the minibatch sharded over ranks the branch is
 * only known after {sum e1, sum e2} have been reduced.  _begin: forward + loss of this rank's B rows; d_critic_sums float32[2] <- this
 * rank's sums.  The caller all-reduces d_critic_sums (MEAN over ranks; every rank holds B rows).  _end: branch weights from the
 * reduced sums, value gradients, backward -> a complete gradient bucket (then: all-reduce MEAN of the bucket, jh_pponet_adam_step).
 * d_stats float32[8] as in jh_ppo_loss_*: actor / entropy terms of this rank's rows, critic terms of the global minibatch.       */
int jh_pponet_ppo_update_dp_begin(jh_pponet* n, int32_t B, const float* d_x, const int64_t* d_idx, const float* d_action, const float* d_adv,
                                  const float* d_ret, const float* d_value_old, const float* d_logp_old, float eps_clip, float vf_coef,
                                  float ent_coef, float* d_critic_sums, jh_stream stream);
int jh_pponet_ppo_update_dp_end(jh_pponet* n, int32_t B, const float* d_x, const int64_t* d_idx, const float* d_critic_sums, float vf_coef,
                                float ent_coef, float* d_stats, jh_stream stream);
/* jh_pponet_ppo_update_dp_end with the ranks' exchange of the critic sums folded into its first launch (jh_peer_*, B <= 256 rows per rank):
 * d_critic_sums = this rank's sums on entry, the ranks' mean on exit.  Declared behind jh_peer below (forward declaration here).  */
struct jh_peer;
int jh_pponet_ppo_update_dp_end_peer(jh_pponet* n, struct jh_peer* peer, int32_t B, const float* d_x, const int64_t* d_idx, float* d_critic_sums,
                                     float vf_coef, float ent_coef, float* d_stats, jh_stream stream);
/* Device address of the optimizer's hyper block (float[8]: lr, beta1, beta2, eps, step, ...), e.g. as the destination of a
 * jh_collector_set_ride_along copy that delivers the next decayed learning rate (base.py:93-111) without a copy of its own. */
void* jh_pponet_hyper_ptr(jh_pponet* n);
/* Sampling stream of the acting calls and the collectors (counter-based: the action of env row w at acting step c is a function
 * of (seed, c, w); the reference samples with torch.multinomial / torch.normal, ppo.py:55-69): read, or with set != 0 restore,
 * {seed, counter} -- what a resumed run needs to continue the same action stream.                                     */
int jh_pponet_act_rng(jh_pponet* n, uint64_t* seed, uint64_t* counter, int32_t set);
/* PPO.act for W envs in one shot (ppo.py:55-69, discrete): ONE kernel launch computes the fused MLP
 * forward and writes per-column-tile partial head outputs + sequence words into device-mapped
 * pinned memory; the host polls them, sums the partials, and does softmax + multinomial (argmax
 * when training == 0).  h_obs [W][S] / h_action [W] / h_logits_out [W][A] / h_value_out [W] are
 * ordinary HOST pointers; BLOCKING: returns when the actions are available.                     */
int jh_pponet_act_discrete(jh_pponet* n, int32_t W, const float* h_obs, int64_t* h_action, float* h_logits_out,
                           float* h_value_out, int32_t training, jh_stream stream);
/* The continuous policy (ppo.py:55-63): h_action [W][A] = tanh(Normal(clamp(mu_raw, -5, 5), exp(tanh(log_std_raw)))
 * .sample()), tanh(mu) when training == 0; h_mu_raw_out / h_log_std_raw_out [W][A] and h_value_out [W] optional.   */
int jh_pponet_act_continuous(jh_pponet* n, int32_t W, const float* h_obs, float* h_action, float* h_mu_raw_out,
                             float* h_log_std_raw_out, float* h_value_out, int32_t training, jh_stream stream);

/* ------------------------------------------------------------------ vectorised host collector
 * Synthetic CartPole-v1 (gym is not installable in the build image): W envs stepped in one
 * call on the host, float64 dynamics, reward shaping of core/env/gym_env.py:78, auto-reset
 * like Actor.run (manager/distributed_manager.py:76-92).  Pure host code.               */
int jh_cartpole_create(int32_t W, uint64_t seed, jh_cartpole** out);
void jh_cartpole_destroy(jh_cartpole* e);
int jh_cartpole_obs(const jh_cartpole* e, float* h_obs /* [W][4] */);
int jh_cartpole_step(jh_cartpole* e, const int64_t* h_action /* [W] */, float* h_next_obs /* [W][4] */,
                     float* h_reward /* [W] */, uint8_t* h_done /* [W] */);

/* Synthetic continuous-control env at config.ppo.mujoco shapes (MuJoCo is not installable in the build image; Hopper-v3
 * is S = 11, A = 3, actions in [-1, 1]): deterministic float64 dynamics (csrc/jh_env.hip), float32 observations,
 * auto-reset like Actor.run (manager/distributed_manager.py:91); mirrored bit for bit by oracle ControlOracle.  */
typedef struct jh_control jh_control;
int jh_control_create(int32_t W, int32_t S, int32_t A, uint64_t seed, jh_control** out);
void jh_control_destroy(jh_control* e);
int jh_control_obs(const jh_control* e, float* h_obs /* [W][S] */);
int jh_control_step(jh_control* e, const float* h_action /* [W][A] */, float* h_next_obs /* [W][S] */,
                    float* h_reward /* [W] */, uint8_t* h_done /* [W] */);

/* ------------------------------------------------------------------ native sync collector
 * DistributedManager.run + Actor.run (manager/distributed_manager.py:26-31,76-92) for every worker
 * and T steps in one call: batched on-GPU acting through device-mapped pinned memory, host env
 * stepping, transitions written worker-major into the rollout store's pinned staging and moved with
 * one hipMemcpyAsync per column.  cols = store column indices of {state, action, reward,
 * next_state, done} (f32[4], i64[1], f32[1], f32[4], u8[1]).                                       */
typedef struct jh_collector jh_collector;

/* The host envs behind the collector as a table of functions (round 5): what `Actor.run` needs from an env
 * (manager/distributed_manager.py:76-92: the current observations, one step with auto-reset) plus, OPTIONALLY, the ability to be
 * copied on the host.  The two built-in envs above are two such tables (jh_collector_create / _create_control build them);
 * jh_collector_create_env plugs any other host simulator -- a C user's, or Python callbacks through ctypes (tests).
 *   obs   rows r0 .. r1-1 of the CURRENT observations (the reset observation where the last step ended an episode) -> h_obs [r1-r0][S]
 *   step  rows r0 .. r1-1 take h_action (int64 [n] for a discrete policy, float [n][A] in [-1, 1] for a continuous one):
 *         h_next_obs [n][S] (the terminal observation where done), h_reward [n], h_done [n]; finished rows reset themselves
 *   both return 0 or a negative JH_ERR_* (the run stops, what was collected is still committed).
 *   fork_alloc / fork_free / copy_row (all three or none): a scratch env of `rows` rows, its release, and "row di of dst becomes an
 *   exact copy of row si of src" including the row's RNG stream.  An env that offers them and has two discrete actions gets TWO
 *   timesteps per acting exchange (the collector steps copies one to three steps ahead while the GPU evaluates the policy; rollouts
 *   are bit-identical to one timestep per exchange); one that does not runs one timestep per exchange.
 * The collector calls obs / step with r0 = 0, r1 = W on the env itself and with arbitrary row ranges on scratch envs only.          */
typedef struct jh_env_vtbl {
  int32_t W, S, A, continuous;
  int (*obs)(void* env, int32_t r0, int32_t r1, float* h_obs);
  int (*step)(void* env, int32_t r0, int32_t r1, const void* h_action, float* h_next_obs, float* h_reward, uint8_t* h_done);
  void* (*fork_alloc)(void* env, int32_t rows);
  void (*fork_free)(void* scratch);
  void (*copy_row)(void* dst, int32_t di, const void* src, int32_t si);
} jh_env_vtbl;
int jh_collector_create_env(jh_ctx* ctx, jh_pponet* net, const jh_env_vtbl* vt, void* env, jh_store* store, const int32_t* cols,
                            jh_collector** out);

int jh_collector_create(jh_ctx* ctx, jh_pponet* net, jh_cartpole* env, jh_store* store, const int32_t* cols,
                        jh_collector** out);
/* The same for a CONTINUOUS policy (PPO.act, ppo.py:55-63: tanh(Normal(mu, std).sample())) on jh_control: the
 * persistent acting kernel returns mu / log_std partials, the host samples; action column f32[A], state f32[S].   */
int jh_collector_create_control(jh_ctx* ctx, jh_pponet* net, jh_control* env, jh_store* store, const int32_t* cols,
                                jh_collector** out);
void jh_collector_destroy(jh_collector* c);
int jh_collector_run(jh_collector* c, int32_t T, int32_t training, jh_stream stream);
/* Acting-time capture: PPO.learn opens with two no-grad passes of the network over the rollout (core/agent/ppo.py:83-94:
 * pi, value = network(state); next_value = network(next_state)[-1]); in sync mode the actors' weights ARE the learner's, so
 * these numbers existed when the actions were sampled.  After jh_collector_set_capture every jh_collector_run of rows = W * T
 * transitions also delivers, in the launch that commits the rows (worker-major like the store): d_h0 [rows][A] raw policy head
 * (logits | mu_raw), d_h1 [rows][A] log_std_raw (continuous; NULL otherwise), d_value [rows] = V(state_t), d_next_value [rows]
 * = V(state_{t+1}) (one extra value-only query after the last step; where done_t is set the entry belongs to the reset state
 * and is multiplied by (1 - done_t) = 0 in GAE, ppo.py:96).  d_value == NULL switches capture off.                         */
int jh_collector_set_capture(jh_collector* c, float* d_h0, float* d_h1, float* d_value, float* d_next_value, int64_t rows);
/* jh_collector_run in two halves, the commit launch enqueued AHEAD of the host loop:
 *   jh_collector_begin  staging, the acting kernel (unless prelaunched), then the commit launch (rows + captured block + ride-along
 *                       copies) -- gated: its workgroups wait, bounded, for a flag word in device-mapped pinned memory.  The store's
 *                       row count advances here: the caller may enqueue the rollout's consumer (the learner's launches) on `stream` now.
 *   jh_collector_loop   the T-step host loop (Actor.run, manager/distributed_manager.py:76-92); its last act releases the flag.
 * The consumer then starts the instant the rollout ends instead of after the host has returned and launched it.  Needs the persistent
 * acting kernel (W <= 32, W * S <= 512) and a one-launch commit (<= 512 KB of rows), else the pair behaves exactly like jh_collector_run.
 * A stalled environment (no observations for ~0.2 s) is an ERROR in this form (work is queued behind the acting kernel, the per-step
 * fallback of jh_collector_run cannot run); the flag is released regardless so that the stream drains.                              */
int jh_collector_begin(jh_collector* c, int32_t T, jh_stream stream);
int jh_collector_loop(jh_collector* c, int32_t training, jh_stream stream);
/* Two more copies (slot 0 / 1; bytes == 0 clears the slot) for the commit launch of every following run: device-visible source
 * (device-mapped pinned memory, jh_pinned_alloc) -> device buffer, read when that launch executes (the end of the run).  For the
 * learner's inputs that change between learn() calls and are known before the rollout ends: the coming epochs' minibatch index
 * lists (ppo.py:116-118, drawn ahead) and the decayed learning rate (base.py:93-111).                                    */
int jh_collector_set_ride_along(jh_collector* c, int32_t slot, const void* d_src_mapped, void* d_dst, int64_t bytes);
/* Enqueue the persistent acting kernel of the NEXT jh_collector_run(T) now, e.g. right behind the learner's last launch: it
 * starts when the stream reaches it, reads the then-current weights and waits (bounded, ~0.2 s) for the first observations.
 * Nothing else may be enqueued on `stream` before that run.  A kernel that timed out is replaced by the run itself.      */
int jh_collector_prelaunch(jh_collector* c, int32_t T, jh_stream stream);
/* Host-side timing of the collection loop (microseconds per timestep): launching + waiting for the
 * actions, and stepping the envs + writing the transitions.                                        */
int jh_collector_stats(jh_collector* c, double* act_us_per_step, double* env_us_per_step, int32_t reset);
/* out6 = {first step's action wait per run (acting kernel start-up), value-only query per run, commit launch per run,
 * steady-state action wait per timestep (both excluded), runs, timesteps}, microseconds; call before a resetting jh_collector_stats. */
int jh_collector_stats_detail(jh_collector* c, double* out6);
/* out4 = {1 if a persistent acting kernel exists else 0, lookahead (1|2), split (0|1),
 *         runs since creation that were finished by per-step launches after the kernel gave up} */
int jh_collector_mode(const jh_collector* c, int64_t* out4);

/* N(0,1) draws on the device for NoisyNet layers (core/network/utils.py:58-60 draws torch.randn per forward):
 * counter-based (element i of call c = Box-Muller on splitmix64(seed, c, i)); d_state uint64[4] = {seed, call counter,
 * 0, 0} in DEVICE memory, advanced by the kernel itself, so a replayed hipGraph draws fresh noise every time.        */
int jh_normal_fill(jh_ctx* ctx, int64_t n, float* d_out, uint64_t* d_state, jh_stream stream);

/* ------------------------------------------------------------------ native value networks
 * The encoders of the DQN / Rainbow / Ape-X family with their learn()-side network work:
 *   kind 0  rainbow  core/network/rainbow.py:8-94: head -> l -> noisy a1|v1 -> noisy a2, v2 -> dueling over K atoms
 *                    (utils.py:55-107 factorised noisy linear)
 *   kind 3  rainbow with independent Gaussian noise (utils.py:72-79): one draw per weight instead of the outer product
 *   kind 1  dueling  core/network/dueling.py:8-35: head -> l1_a|l1_v -> l2_a, l2_v -> dueling combine  (K = 1)
 *   kind 2  q        core/network/q_network.py:8-20: head -> l -> q                                    (K = 1)
 *   kind 4  noisy    core/network/noisy.py:8-50: head -> relu(noisy(F -> H)) -> noisy(H -> A), factorised noise   (K = 1)
 *   kind 5  noisy with independent Gaussian noise (utils.py:72-79)
 * on core/network/head.py:6-61 (MLP or Nature-CNN head), plus the three forwards / backward / optimizer step
 * of the agents' learn() (rainbow.py:160-186,236-238; dqn.py:128-147; ape_x.py:96-131).  Convolutions are
 * implicit GEMMs on the fp32 MFMA; uint8 NCHW frames are read straight from the replay store (divide by 255
 * inside the operand fetch, head.py:46).  Parameters live in flat fp32 buckets with a private layout;
 * jh_rbnet_segment describes it (rows x cols, row-major, 16-byte aligned offsets, rows = 0: absent):
 *   0 conv1.weight [32][(c,ky,kx)] | head.l.weight [H][S] (mlp)     1 its bias
 *   2 conv2.weight [64][(ky,kx,c)]   3 bias    4 conv3.weight [64][(ky,kx,c)]   5 bias   (cnn only)
 *   6 l.weight [H][F] (cnn: F ordered (y,x,c))   7 l.bias                         (kinds 0, 2)
 *   8 first stream layer, a|v stacked [2H][in] (in = H, or F for kind 1; rainbow: mu_w^T)   9 sig_w   10 bias [2H]   11 sig_b
 *   12-15 a2 / l2_a / q: weight [A*K][H], sig_w, bias, sig_b        16-19 v2 / l2_v: weight [K][H], sig_w, bias, sig_b
 * (sig_* only for kinds 0, 3, 4, 5).
 * Kinds 4 / 5 (network/noisy.py:15-20, utils.py:55-107) have no segment 6 / 7 and no 16-19; their two noisy layers use the slots
 *   8 mu_w1^T [H][F] (F = H for the mlp head, 64 * P3 ordered (y,x,c) for the cnn head)   9 sig_w1^T   10 mu_b1 [H]   11 sig_b1
 *   12 mu_w2^T [A][H]   13 sig_w2^T   14 mu_b2 [A]   15 sig_b2
 * each padded up to 4 floats like every segment; jh_rbnet_param_count_for(4 | 5, ...) is the padded sum.               */
typedef struct jh_rbnet jh_rbnet;
int64_t jh_rbnet_param_count_for(int32_t kind, int32_t head_cnn, int32_t channels_or_state_size, int32_t height, int32_t width,
                                 int32_t hidden, int32_t action_size, int32_t num_support);
/* d_params (online), d_target, d_grads, d_m, d_v: caller-owned flat fp32 device buckets of
 * jh_rbnet_param_count_for(...) floats each (16-byte aligned), borrowed for the net's lifetime.
 * d_m / d_v: Adam exp_avg / exp_avg_sq, or RMSprop grad_avg / square_avg.                               */
int jh_rbnet_create(jh_ctx* ctx, int32_t kind, int32_t head_cnn, int32_t channels_or_state_size, int32_t height, int32_t width,
                    int32_t hidden, int32_t action_size, int32_t num_support, int32_t max_batch, float* d_params,
                    float* d_target, float* d_grads, float* d_m, float* d_v, jh_rbnet** out);
void jh_rbnet_destroy(jh_rbnet* n);
int64_t jh_rbnet_param_count(const jh_rbnet* n);
int32_t jh_rbnet_segment_count(void);
int jh_rbnet_segment(const jh_rbnet* n, int32_t i, int64_t* offset, int32_t* rows, int32_t* cols);
/* Length of one noise set (kind 0): N(0,1) draws in the reference's draw order (utils.py:58-60, layers a1, v1,
 * a2, v2): [e_in a1 H][e_out a1 H][e_in v1 H][e_out v1 H][e_in a2 H][e_out a2 A*K][e_in v2 H][e_out v2 K];
 * kind 3: per layer [eps_w (in x out, row-major like the reference's mu_w)][eps_b (out)]
 * kind 4: [eps_i1 F][eps_j1 H][eps_i2 H][eps_j2 A];   kind 5: [eps_w1 F x H (in, out)][eps_b1 H][eps_w2 H x A][eps_b2 A].
 *   eps_i1[k] and the rows of eps_w1 are indexed by the REFERENCE's feature index k (cnn head: (c, y, x), head.py:58), not by the stored
 *   column (y, x, c): the kernels apply the permutation the weights' columns get on import.                              */
int64_t jh_rbnet_noise_len(const jh_rbnet* n);
/* Adam: (lr, beta1, beta2, eps).  RMSprop: (lr, alpha, unused, eps) + centered.  step = optimizer step counter. */
int jh_rbnet_set_hyper(jh_rbnet* n, double lr, double beta1_or_alpha, double beta2, double eps, int64_t step, int32_t centered,
                       jh_stream stream);
int jh_rbnet_set_lr(jh_rbnet* n, double lr, jh_stream stream);
/* update_target (dqn.py:162-163, rainbow.py:270-271): target <- online                                  */
int jh_rbnet_sync_target(jh_rbnet* n, jh_stream stream);
/* network(x[, is_train]): rows <= max_batch observations (JH_U8 or JH_F32; NCHW images or [rows][S]),
 * which 0 online / 1 target, d_noise one noise set or NULL (kind 0: is_train = False) -> logits [rows][A][K] */
int jh_rbnet_forward(jh_rbnet* n, int32_t which, const void* d_x, int32_t x_dtype, int32_t rows, const float* d_noise,
                     float* d_logits, jh_stream stream);
/* An on-policy learner's forward (ppo.py:127-135 on the CNN head): network(x) of the online parameters for B <= max_batch rows, activations kept for
 * jh_rbnet_backward (which then takes d(loss)/d(outputs) [B][A][K] of these rows).  Kinds 1 and 2 (no noise).                                  */
int jh_rbnet_forward_keep(jh_rbnet* n, const void* d_x, int32_t x_dtype, int32_t B, float* d_logits, jh_stream stream);
/* The three forwards of learn(): d_x = [state; next_state] (2B rows), d_noise three noise sets (kind 0, else
 * NULL) -> d_logits [3][B][A][K] = online(state), online(next_state), target(next_state)                */
int jh_rbnet_learn_forward(jh_rbnet* n, const void* d_x, int32_t x_dtype, int32_t B, const float* d_noise, float* d_logits,
                           jh_stream stream);
/* The three forwards of Munchausen DQN's learn() (m_dqn.py:31-38): d_x as above -> d_logits [3][B][A][K] = online(state),
 * target(state), target(next_state).  The online trunk runs over B rows and the target trunk over 2B, in as many launches as
 * jh_rbnet_learn_forward; jh_rbnet_backward continues from it in the same way.  Kinds 1 and 2 (a noisy network: JH_ERR_ARG); d_noise
 * is ignored.  The target network's activation buffers hold max_batch rows unless jh_rbnet_reserve_target_rows(n, rows) grew them
 * (rows <= 2 * max_batch; allocates, so: once, outside any stream capture); without room for 2B rows: JH_ERR_STATE.            */
int jh_rbnet_reserve_target_rows(jh_rbnet* n, int32_t rows);
int jh_rbnet_learn_forward_m(jh_rbnet* n, const void* d_x, int32_t x_dtype, int32_t B, const float* d_noise, float* d_logits,
                             jh_stream stream);
/* The three forwards of MPO's discrete actor (mpo.py:312-313, 321): d_x as above -> d_logits [3][B][A][K] = online(state),
 * online(next_state), target(state): jh_rbnet_learn_forward with the target trunk on the FIRST half of the batch, in as many launches;
 * jh_rbnet_backward continues from it in the same way.  Kinds 1 and 2 (a noisy network: JH_ERR_ARG); d_noise is ignored.          */
int jh_rbnet_learn_forward_p(jh_rbnet* n, const void* d_x, int32_t x_dtype, int32_t B, const float* d_noise, float* d_logits,
                             jh_stream stream);
/* The two forwards of Noisy.learn() (agent/noisy.py:83-105), kinds 4 / 5 only: d_x as above, d_noise [2][noise_len] -> d_logits [2][B][A] =
 * online(state; noise 0), target(next_state; noise 1).  The online trunk runs over the first B rows only and the target trunk over the last
 * B rows only, in shared launches; jh_rbnet_backward[_deferred] continues from it.  jh_rbnet_learn_forward, _m, _p, jh_rbnet_learn_trunk /
 * _heads, jh_rbnet_prepare_noise and jh_rbnet_c51_step answer JH_ERR_ARG for these kinds.                                            */
int jh_rbnet_learn_forward_n(jh_rbnet* n, const void* d_x, int32_t x_dtype, int32_t B, const float* d_noise, float* d_logits,
                             jh_stream stream);
/* Noisy.get_sig_w_mean (network/noisy.py:46-50) of the online parameters, kinds 4 / 5: d_out2 = {mean |sig_w1|, mean |sig_w2|} (device or
 * device-mapped memory) in one launch whose summation order is fixed (a graph replay returns the bits of the eager call).           */
int jh_rbnet_sig_abs_mean(jh_rbnet* n, float* d_out2, jh_stream stream);
/* Device address of the optimizer's hyper block (16 floats: lr, beta1, beta2, eps, steps taken, ..., the betas as doubles at [10:14]),
 * as jh_pponet_hyper_ptr: what jh_mpo_loss_discrete reads to step the multipliers that sit in the actor's optimizer (mpo.py:142-146). */
void* jh_rbnet_hyper_ptr(jh_rbnet* n);
/* jh_rbnet_learn_forward in two halves + the part that does not depend on the batch (rainbow.py:160-186: the three forwards of learn()):
 *   jh_rbnet_prepare_noise  W = mu + sig * eps of the three noisy weight sets (network/utils.py:55-86) for the draw d_noise [3][noise_len]
 *                           -- may run on another stream while the trunk runs (a 12-us launch off the critical path)
 *   jh_rbnet_learn_trunk    head + l of [state; next_state] (online) and next_state (target)
 *   jh_rbnet_learn_heads    the noisy dueling heads of the three forwards -> d_logits [3][B][A][K]; uses the prepared sets when
 *                           jh_rbnet_prepare_noise ran for the same d_noise, else materialises them itself                          */
int jh_rbnet_prepare_noise(jh_rbnet* n, const float* d_noise, jh_stream stream);
int jh_rbnet_learn_trunk(jh_rbnet* n, const void* d_x, int32_t x_dtype, int32_t B, jh_stream stream);
int jh_rbnet_learn_heads(jh_rbnet* n, int32_t B, const float* d_noise, float* d_logits, jh_stream stream);
/* loss.backward() given d(loss)/d(online(state) output) [B][A][K] (from jh_c51_loss / jh_td_loss; NULL after jh_rbnet_c51_step); fills d_grads */
int jh_rbnet_backward(jh_rbnet* n, const float* d_g, jh_stream stream);
/* Rainbow.learn()'s loss step on the network's own stream outputs (rainbow.py:160-235), three launches where the separate calls
 * (jh_rbnet_learn_heads' combine, jh_c51_loss x 2, jh_per_update x 2, jh_rbnet_backward's first kernel) take six:
 *   jh_rbnet_learn_heads_raw  = jh_rbnet_learn_heads up to the advantage / value streams (network/rainbow.py:76-87); no logits yet
 *   jh_rbnet_c51_step         launch 1: dueling combine of the three forwards (rainbow.py:88-93 -> d_logits [3][B][A][K], bit-identical
 *                             to jh_rbnet_learn_heads) + double-Q action + n-step projection + KL + priorities KL^alpha (-> d_prio, d_kl)
 *                             + the gradient pulled back through the combine (kept in the network);
 *                             launch 2: batch statistics (d_stats as jh_c51_loss) + priorities into the leaves d_tree_idx of `per`
 *                             (per_buffer.py:42-54); launch 3: the climb.  per NULL: no write-back.  flags: JH_C51_DOUBLE required.
 *   jh_rbnet_backward(n, NULL, ..) continues from the gradient jh_rbnet_c51_step left.                                               */
int jh_rbnet_learn_heads_raw(jh_rbnet* n, int32_t B, const float* d_noise, jh_stream stream);
int jh_rbnet_c51_step(jh_rbnet* n, jh_per* per, int32_t B, int32_t n_step, int32_t flags, const float* d_action, const float* d_reward,
                      const float* d_done, const float* d_weights, const int64_t* d_tree_idx, float v_min, float v_max, float gamma,
                      float alpha, float* d_logits, float* d_prio, float* d_kl, float* d_stats, jh_stream stream);
/* (kinds 4 / 5: the tail left undone is d(sigma) = d(mu) * eps of the two noisy layers, one launch in jh_rbnet_flush_grads / jh_rbnet_optim_step.)
 * jh_rbnet_backward that leaves two elementwise tails undone -- d(sigma) = d(mu) * eps of the noisy layers (network/utils.py:60-70) and
 * the sum of conv1's weight-gradient partials -- for jh_rbnet_optim_step to do inside the optimizer's own pass (no clipping) or as the
 * launches they were (clipping).  jh_rbnet_flush_grads completes the gradient bucket for anybody who reads it before the optimizer step
 * (a data-parallel all-reduce).                                                                                                       */
int jh_rbnet_backward_deferred(jh_rbnet* n, const float* d_g, jh_stream stream);
int jh_rbnet_flush_grads(jh_rbnet* n, jh_stream stream);
/* [clip_grad_norm_(max_norm) when max_norm > 0 (ape_x.py:128),] optimizer.step(): optimizer 0 torch.optim.Adam,
 * 1 torch.optim.RMSprop (momentum 0, centered per set_hyper); advances the step counter                 */
int jh_rbnet_optim_step(jh_rbnet* n, int32_t optimizer, float max_norm, jh_stream stream);
int jh_rbnet_adam_step(jh_rbnet* n, jh_stream stream);

/* The dense form of the grouped LDS-tiled fp32 MFMA GEMM every value-network layer runs on (nn.Linear forward /
 * data gradient / weight gradient of the core/network modules): C[M][N] = sum_k A(m,k) B(k,n) with a fused epilogue.
 *   a_kcont != 0: A stored [M][K] (lda), else [K][M];   b_kcont != 0: B stored [N][K] (ldb), else [K][N]
 *   epi 0 none | 1 + bias[n] | 2 relu(. + bias[n]) | 3 zero where aux[m][n] <= 0;  d_rowsum (optional) [M] = sum_k A(m,k) */
int jh_tgemm_dense(jh_ctx* ctx, int32_t M, int32_t N, int32_t K, const float* d_a, int32_t lda, int32_t a_kcont, const float* d_b,
                   int32_t ldb, int32_t b_kcont, float* d_c, int32_t ldc, int32_t epi, const float* d_bias, const float* d_aux,
                   int32_t ldaux, float* d_rowsum, jh_stream stream);
/* Test entry: n (<= 6) independent problems C_j [M][N] = A_j [M][K] B_j [N][K]^T as ONE grouped launch (the shape of the value
 * networks' forward launches: online and target trunks side by side); d_a / d_b / d_c are host arrays of n device pointers.  */
int jh_tgemm_dense_group(jh_ctx* ctx, int32_t n, int32_t M, int32_t N, int32_t K, const float* const* d_a, const float* const* d_b,
                         float* const* d_c, jh_stream stream);

/* Measurement / test hook of the tile engine: per-call-site overrides of the workgroup tile, the K split and the XCD order,
 * "<site id | *>:<TM>x<TN>[:s<splits>][:x<0|1>],..." (TM x TN in 16 x 16 fragments per wave: 2x2 = 64 x 64, 4x2 = 128 x 64, 2x4 = 64 x 128);
 * the same grammar as the environment variable JH_TGEMM_CFG; "" or NULL restores the defaults.  No reference counterpart.  */
int jh_tgemm_set_cfg(const char* cfg);

/* ------------------------------------------------------------------ asynchronous actor -> learner staging
 * Replaces the async path's transport (run_mode.py:212-363 async_distributed_train: Ray actors -> manager
 * process -> multiprocessing trans_queue -> `gather_thread` spinning on flags, process.py:7-31,82-97) for
 * many-actor / one-learner agents (Ape-X, ape_x.py:174-199 actor-side priorities): one bounded lock-free
 * multi-producer / single-consumer ring of transitions in pinned host memory with the replay store's column
 * layout.  Actor threads produce rows (+ priorities); the learner thread drains what is published with
 * hipMemcpyAsync straight from the ring's pinned slots into the device store (+ the sum-tree leaves).
 * ctx may be NULL for a host-only ring (pageable memory, jh_ring_consume_host only).                      */
typedef struct jh_ring jh_ring;
int jh_ring_create(jh_ctx* ctx, int64_t slots, int32_t n_cols, const jh_col_desc* cols, int32_t with_priority, jh_ring** out);
void jh_ring_destroy(jh_ring* r);
/* Any thread.  n <= slots rows, h_cols[c] = n rows of column c, h_prio[n] when the ring carries priorities.
 * Blocks while the ring is full; timeout_ms >= 0 bounds that wait (JH_ERR_STATE, nothing written), < 0 forever. */
int jh_ring_produce(jh_ring* r, int64_t n, const void* const* h_cols, const double* h_prio, int32_t timeout_ms);
/* The consumer thread.  Appends every published row (<= max_rows; <= 0: as many as the store holds) to the device
 * store and, with per != NULL, pushes the leaves (actor priorities, or max_priority for a ring without).
 * Asynchronous on `stream`; slots are recycled when the copies have executed.  *n_out = rows taken.        */
int jh_ring_drain(jh_ring* r, jh_store* s, jh_per* per, int64_t max_rows, jh_stream stream, int64_t* n_out);
/* Consumer thread: recycle the slots of drains whose copies have executed (wait != 0: wait for all of them).  */
int jh_ring_reclaim(jh_ring* r, int32_t wait);
/* Host-side consumer (tests / CPU plumbing): rows are copied to h_out_cols and their slots recycled at once. */
int jh_ring_consume_host(jh_ring* r, int64_t max_rows, void* const* h_out_cols, double* h_prio_out, int64_t* n_out);
int jh_ring_stats(jh_ring* r, int64_t* produced, int64_t* drained, double* producer_wait_ms);

/* ------------------------------------------------------------------ device-resident actor -> replay feed
 * For N lockstep actors whose frame stacks are already in HBM (they were uploaded for the batched acting forward):
 * replaces, per tick, the env wrapper's stack bookkeeping as seen by the replay (core/env/atari.py:145-149: consecutive
 * stacks share C - 1 frames), Ape-X's per-actor n-step deque with actor-side priorities (core/agent/ape_x.py:174-199)
 * and the transfer of both full stacks of every transition to the learner (process.py:82-97, run_mode.py:300-330).
 * Planes go into a caller-owned plane pool [n_actors * planes_per_actor][plane_bytes] (each actor owns a private ring of
 * planes_per_actor slots); a stack is C slot numbers.  A stack that is not its predecessor shifted by one frame (reset,
 * frame skip glitch, ...) simply appends all C planes: the comparison is bytewise, so the stored content is always exact.
 * window_ticks: for how many ticks a plane must survive (buffer rows / n_actors + n_step + C + in-flight ticks); when an
 * actor allocates more than planes_per_actor planes inside that window, bit 0 of the flags word is set (jh_feed_state).
 * jh_feed_tick: d_obs uint8 [N][C][plane_bytes] = the stacks acted on this tick, d_prev_obs = those of the previous tick
 * (NULL on the first), d_action int64 [N] / d_q float [N] = action taken and its Q (jh_value_act), h_reward / h_done
 * float [N] (host) = the env's answer.  From tick n_step on (*emitted = N, else 0) the outputs hold one n-step
 * transition per actor: slot numbers of state_t and state_{t+n} int64 [N][C], action_t int64 [N], reward float [N][n],
 * done uint8 [N][n], priority float64 [N] = |G_n - q_t| + prio_eps, all on the device, enqueued on `stream`.          */
typedef struct jh_feed jh_feed;
int jh_feed_create(jh_ctx* ctx, int32_t n_actors, int32_t C, int64_t plane_bytes, int32_t n_step, float gamma,
                   int64_t planes_per_actor, int64_t window_ticks, jh_feed** out);
void jh_feed_destroy(jh_feed* f);
int jh_feed_tick(jh_feed* f, const uint8_t* d_obs, const uint8_t* d_prev_obs, uint8_t* d_pool, const int64_t* d_action,
                 const float* d_q, const float* h_reward, const float* h_done, double prio_eps, int64_t* d_state_ids,
                 int64_t* d_next_ids, int64_t* d_action_out, float* d_reward_out, uint8_t* d_done_out, double* d_prio_out,
                 int32_t* emitted, jh_stream stream);
/* jh_feed_tick in two halves (the acting forward runs between them):
 *   jh_feed_push_stacks  stack mode: the stacks as they were uploaded for the forward (what jh_feed_tick does first)
 *   jh_feed_push_frames  frame mode: the env hands over only the NEWEST plane of every actor, d_frames uint8 [N][plane_bytes]
 *                        (device), and h_reset uint8 [N] (host; 1 = the env was reset: the stack is that frame C times,
 *                        core/env/atari.py:112); the stacks [N][C][plane_bytes] for the forward are rebuilt into d_stack_out
 *                        by gather from the plane pool.  7 KB instead of 28 KB per env step over PCIe at Atari shapes,
 *                        and the wrapper's np.concatenate of atari.py:147 has no counterpart at all.
 *   jh_feed_emit         the second half: action / Q / reward / done -> n-step rows + priorities
 * A feed uses ONE of the two push modes for its whole life.                                                              */
int jh_feed_push_stacks(jh_feed* f, const uint8_t* d_obs, const uint8_t* d_prev_obs, uint8_t* d_pool, jh_stream stream);
int jh_feed_push_frames(jh_feed* f, const uint8_t* d_frames, const uint8_t* h_reset, uint8_t* d_pool, uint8_t* d_stack_out,
                        jh_stream stream);
int jh_feed_emit(jh_feed* f, const int64_t* d_action, const float* d_q, const float* h_reward, const float* h_done,
                 double prio_eps, int64_t* d_state_ids, int64_t* d_next_ids, int64_t* d_action_out, float* d_reward_out,
                 uint8_t* d_done_out, double* d_prio_out, int32_t* emitted, jh_stream stream);
/* Blocking read of the flags word (bit 0: plane ring overrun) and the number of planes written so far. */
int jh_feed_state(jh_feed* f, int32_t* h_flags, int64_t* h_planes_written, jh_stream stream);
/* Checkpoint of the feed itself (the reference cannot resume a replay at all, core/agent/dqn.py:184-199): rolling stacks' slot
 * numbers, plane cursors + history, rolling action / reward / done / q windows, flags, tick.  Together with the plane pool, the
 * store's rows and the sum tree, a feed of the SAME geometry continues exactly where the saved one stood.  h buffers hold
 * jh_feed_state_bytes(f) bytes; both calls synchronise `stream` and must not race a tick.                               */
int64_t jh_feed_state_bytes(const jh_feed* f);
int jh_feed_save(jh_feed* f, void* h_out, int64_t bytes, jh_stream stream);
int jh_feed_load(jh_feed* f, const void* h_in, int64_t bytes, jh_stream stream);

/* ------------------------------------------------------------------ data-parallel learners: the collective
 * The reference has ONE learner and no collective (its "distributed" mode is Ray actors feeding that learner,
 * manager/distributed_manager.py, process.py); BASELINE.json's north star re-expresses Ape-X's many-actor / one-learner
 * layout as one learner per GPU that averages gradients between backward and clip_grad_norm_ / optimizer.step()
 * (core/agent/ppo.py:164-169, ape_x.py:118-122, rainbow.py:236-238).  This is that step: one RCCL communicator per
 * process (one rank per GPU, xGMI inside a node), bound at run time (dlopen of librccl.so.1: single-GPU users need no RCCL).
 *   jh_comm_unique_id   rank 0 creates the 128-byte id; the caller ships it to the other ranks (any side channel:
 *                       a file, MPI, torch.distributed's store).
 *   jh_comm_create      collective over all ranks (ncclCommInitRank on ctx's device).
 *   jh_comm_allreduce_mean_f32   in place, d_bucket[i] <- mean over ranks (ncclAvg), enqueued on `stream`: the flat
 *                       gradient bucket of jh_pponet_* / jh_rbnet_* between their backward and their optimizer step.
 *                       Capturable into a hipGraph (every rank must then replay in the same order).
 *   jh_comm_broadcast   bytes from `root` to all (identical initial weights / optimizer moments).
 *   jh_comm_allgather_f64   n doubles per rank -> [nranks][n] (sharded PER: {root, count, min sampled priority},
 *                       core/buffer/per_buffer.py:88-94 evaluated for the logical buffer over all shards).          */
#define JH_COMM_ID_BYTES 128
typedef struct jh_comm jh_comm;
int jh_comm_unique_id(void* h_id128);
int jh_comm_create(jh_ctx* ctx, int32_t nranks, int32_t rank, const void* h_id128, jh_comm** out);
void jh_comm_destroy(jh_comm* m);
int jh_comm_info(const jh_comm* m, int32_t* nranks, int32_t* rank);
int jh_comm_allreduce_mean_f32(jh_comm* m, float* d_bucket, int64_t n, jh_stream stream);
int jh_comm_broadcast(jh_comm* m, void* d_buf, int64_t bytes, int32_t root, jh_stream stream);
int jh_comm_allgather_f64(jh_comm* m, const double* d_in, double* d_out, int64_t n, jh_stream stream);

/* ---- the same collectives through peer pointers (round 6): every rank of ONE node maps its peers' arenas (hipIpc) and the gradient
 * bucket's all-reduce is two one-hop exchanges -- reduce-scatter by reading slice `rank` of every peer's bucket, all-gather by reading the
 * peers' reduced slices -- inside two launches of this library, no collective library's launch and no ring (csrc/jh_peer.hip).  Chosen with
 * JH_DP_COLLECTIVE=peer; RCCL (jh_comm_*) stays the default.  No reference counterpart.
 *   jh_peer_create   this rank's arena for buckets of up to max_floats floats
 *   jh_peer_handle   its 64-byte hipIpcMemHandle_t; the caller ships all ranks' handles to every rank (any side channel)
 *   jh_peer_connect  h_handles: nranks x 64 bytes in rank order (the own entry is ignored)
 *   jh_peer_allreduce_mean_f32   in place, d_bucket[i] <- mean over ranks; every slice is summed in rank order by ONE rank: identical bits on
 *                    all ranks.  Capturable (sequence numbers advance on the device).  d_bucket 16-byte aligned.
 *   jh_peer_allreduce_small_f32  <= 16 floats, sum (mean != 0: mean) over ranks in rank order, one single-workgroup launch
 *   jh_peer_status   bounded waits (~2 s) that gave up since creation, completed all-reduces                                        */
#define JH_PEER_HANDLE_BYTES 64
typedef struct jh_peer jh_peer;
int jh_peer_create(jh_ctx* ctx, int32_t nranks, int32_t rank, int64_t max_floats, jh_peer** out);
int jh_peer_handle(jh_peer* p, void* h_handle64);
int jh_peer_connect(jh_peer* p, const void* h_handles);
int jh_peer_allreduce_mean_f32(jh_peer* p, float* d_bucket, int64_t n, jh_stream stream);
int jh_peer_allreduce_small_f32(jh_peer* p, float* d_vals, int32_t n, int32_t mean, jh_stream stream);
int jh_peer_status(jh_peer* p, int32_t* timeouts, int64_t* completed);
void jh_peer_destroy(jh_peer* p);


#ifdef __cplusplus
}
#endif
#endif /* JORLDY_HIP_H */
