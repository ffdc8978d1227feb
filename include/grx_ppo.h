/* grx_ppo.h -- C ABI of libgrx_ppo.so: the PPO minibatch loss, forward and gradients in one pass (gfx950).
 *
 * Replaces, for the training loop that sits on top of the env step, the ~100 element-wise kernels that
 * rsl_rl/algorithms/ppo.py:215-245 (log-prob, ratio, clipped surrogate, clipped value loss, entropy, KL) and
 * their autograd backward expand to.  Plain device pointers and sizes, no torch types; everything is fp32.
 * Deterministic: per-block partial sums are combined in block order by a second kernel.
 * Also here: the column sum behind every bias gradient of the two MLPs (grx_ppo_colsum).
 */
#ifndef GRX_PPO_H
#define GRX_PPO_H
#ifdef __cplusplus
extern "C" {
#endif

/* number of floats the caller must provide in `partials` (8-byte aligned scratch) for a batch of `batch` samples */
int grx_ppo_loss_partials_size(int batch);

/* One minibatch.
 *   mu [batch][num_actions], std [num_actions], value [batch]: the networks' outputs (row-major, contiguous)
 *   actions, old_mu, old_sigma [batch][num_actions]; old_logp, advantages, returns, target_values [batch]
 *   out[4]      = { surrogate loss, value loss, total loss, mean KL(old || new) }
 *   d_mu [batch][num_actions], d_std [num_actions], d_value [batch] = d(total loss)/d(.)
 *   total loss = surrogate + value_loss_coef * value_loss - entropy_coef * mean entropy   (ppo.py:243)
 * Where inputs leave the finite range (a sigma that underflows, is 0, negative, inf or NaN; a ratio that overflows; infinite
 * advantages, returns or values) the loss and the mean KL are finite exactly where the fp32 torch spelling's are, and a gradient entry
 * is non-finite exactly where torch.autograd's is -- including the NaN that `sigma = mean * 0.0 + std` hands every d_mu entry whose
 * d sigma is not finite.  A finite loss never hides a non-finite gradient; grx_ppo_step_tail skips the step on either.
 * `stream` is a hipStream_t (0 = the null stream).  Returns 0, or a negative number for invalid arguments
 * (num_actions outside 1..32, batch < 1) -- nothing is launched then.
 */
int grx_ppo_loss(int batch, int num_actions, const float* mu, const float* std, const float* value,
                 const float* actions, const float* old_logp, const float* old_mu, const float* old_sigma,
                 const float* advantages, const float* returns, const float* target_values,
                 float clip_param, float value_loss_coef, float entropy_coef, int use_clipped_value_loss,
                 float* out, float* d_mu, float* d_std, float* d_value, float* partials, void* stream);

/* Column sums of a row-major fp32 matrix x [rows][cols] -> out [cols] (the bias gradient of a linear layer: the sum of
 * dY over the batch), deterministic (256-row slabs added in order).  `partials`: scratch of
 * grx_ppo_colsum_partials_size(rows, cols) floats.  Returns 0, negative for rows < 1 or cols < 1. */
int grx_ppo_colsum_partials_size(int rows, int cols);
int grx_ppo_colsum(int rows, int cols, const float* x, float* out, float* partials, void* stream);

/* Backward of a hidden layer's ELU(alpha 1) fused with that layer's bias gradient: dz [rows][cols] = dy * (y > 0 ? 1 : y + 1)
 * from the layer's OUTPUT y (torch's elu_backward on the result), out [cols] = column sums of dz (as grx_ppo_colsum:
 * deterministic, same slab order).  `partials`: grx_ppo_colsum_partials_size(rows, cols) floats. */
int grx_ppo_elu_backward_colsum(int rows, int cols, const float* dy, const float* y, float* dz, float* out, float* partials, void* stream);

/* One rollout step's bookkeeping in ONE launch (rsl_rl: PPO.process_env_step ppo.py:184-197 + RolloutStorage.add_transitions
 * rollout_storage.py:23-59 + the runner's running episode reward / length, on_policy_runner.py:170-181 -- ~25 small torch
 * kernels per env step otherwise).  All pointers are device pointers; N envs.
 *   in : obs (N, num_obs), pri (N, num_pri) or NULL, actions / mu / sigma (N, num_actions), values / logp / rewards (N),
 *        dones / time_outs (N) uint8 (time_outs may be NULL), gamma
 *   out: the storage rows of this step, each contiguous: st_obs (N, num_obs), st_pri (N, num_pri) or NULL, st_actions / st_mu /
 *        st_sigma (N, num_actions), st_values / st_logp / st_rewards (N), st_dones (N) uint8.
 *        st_rewards = rewards + gamma * values * time_outs  (bootstrap on time-outs, ppo.py:190-191)
 *   logging (all four may be NULL): cur_rew / cur_len (N) running sums, updated in place and zeroed where done; done_rew /
 *        done_len (N): the finished episode's totals where done (left untouched elsewhere).
 * Returns 0, negative for invalid sizes. */
int grx_ppo_store_transition(int N, int num_obs, int num_pri, int num_actions,
                             const float* obs, const float* pri, const float* actions, const float* mu, const float* sigma,
                             const float* values, const float* logp, const float* rewards, const unsigned char* dones,
                             const unsigned char* time_outs, float gamma,
                             float* st_obs, float* st_pri, float* st_actions, float* st_mu, float* st_sigma, float* st_values,
                             float* st_logp, float* st_rewards, unsigned char* st_dones,
                             float* cur_rew, float* cur_len, float* done_rew, float* done_len, void* stream);

/* One layer of an MLP at inference: Y [M][N] = act(X [M][K] . W^T + bias), W [N][K] row-major as torch.nn.Linear.weight,
 * bias [N] or NULL, act = ELU(alpha 1) when `elu` != 0 -- the rollout's policy / value forward (rsl_rl modules/mlp.py:7-42,
 * actor_critic_mlp.py act() / evaluate()) as one launch per layer: f32-input MFMA (v_mfma_f32_32x32x2_f32, exact f32:
 * every output is a k-ordered fmaf chain), bias and activation in the epilogue.  Any M, K, N >= 1; layers narrower than 32
 * outputs (action means, value) take a lane-per-row path.  Contiguous row-major fp32 everywhere.  Returns 0, negative for
 * invalid arguments / a failed launch. */
/* The minibatch of one PPO step in one launch: dst[t][r][:] = src[t][idx[r]][:] for t < n_tensors (<= GRX_PPO_GATHER_MAX), r < mb;
 * src[t] row-major fp32 with widths[t] columns, idx int64 on the device (RolloutStorage.mini_batch_generator's permutation
 * slice, rollout_storage.py:82-112).  src / dst / widths are HOST arrays of device pointers / ints. */
/* The TAIL of one PPO minibatch step in two launches: everything rsl_rl/algorithms/ppo.py:264-311 does between loss.backward() and the
 * next minibatch -- the adaptive learning rate from the minibatch KL (ppo.py:205-213), the NaN-skip (ppo.py:297-299),
 * nn.utils.clip_grad_norm_ and Adam.step() -- which PyTorch runs as ~20 small kernels (comparisons, clamps, wheres, a foreach norm, a
 * foreach multiply, the fused-Adam kernel's 42 us multi-tensor launch, statistics adds): 145 us of a 790 us captured step at the GR1T1
 * train shape, all of it on the step's critical path (profiles/r06_ppo_update_kernel_stats.txt).
 *   launch 1: per-chunk sums of squares of the gradients -> partials (deterministic order); block 0: lr <- adaptive rule(kl);
 *             the chunk-0 block of every tensor: its Adam step counter += 1 unless the loss is not finite
 *   launch 2: every block adds the partials in a fixed order -> per-tensor norms -> total norm -> clip coefficient (clip_grad_norm_'s
 *             formulas); unless the loss is not finite: Adam on its chunk with the CLIPPED gradient -- the arithmetic of ATen's
 *             fused_adam_utils.cuh adam_math (double constants, float state), bias corrections from the step counter; block 0: the
 *             update's running statistics sums[0] += value_loss, sums[1] += surrogate_loss (finite steps only), sums[2] = kl.
 * A step is SKIPPED when the loss is not finite, when *bad_flag != 0, or when the gradients' total norm as launch 2 computes it in fp32 is
 * not finite: a NaN or +-inf gradient element, or finite elements whose fp32 sum of squares overflows.  A skipped step leaves parameters,
 * both moments and the step counters bit-identical (launch 1 has counted the step before the norm is known; launch 2's block of each
 * tensor's first elements takes that back, exact below 2^24 steps), adds nothing to sums[0] / sums[1], and still writes sums[2] = kl and
 * the learning rate.  This is the rule of PPO's multi-rank paths (a non-finite gradient bucket skips).  It departs from torch on purpose:
 * clip_grad_norm_ + fused Adam with found_inf = !isfinite(loss) poisons every parameter on a NaN norm and, on an infinite one (clip
 * coefficient 0), takes an Adam step on zero gradients; PPO's torch tails fold !isfinite(total norm) into found_inf to agree with this.
 * weight_decay = 0, no amsgrad, no maximize (the reference's optimizer).  Tensor pointers travel BY VALUE in the launch arguments: a captured
 * graph keeps the addresses of its capture (PyTorch's graph pool keeps gradient buffers where they were).  All pointers: device memory. */
#define GRX_PPO_TAIL_MAX 24
typedef struct grx_ppo_tail_tensors {
    int n, pad;
    float* param[GRX_PPO_TAIL_MAX]; const float* grad[GRX_PPO_TAIL_MAX]; float* exp_avg[GRX_PPO_TAIL_MAX]; float* exp_avg_sq[GRX_PPO_TAIL_MAX];
    float* step[GRX_PPO_TAIL_MAX];          /* the optimizer's per-parameter step counter (a float scalar on the device, torch's capturable Adam) */
    long long numel[GRX_PPO_TAIL_MAX];
} grx_ppo_tail_tensors;
typedef struct grx_ppo_tail_args {
    const float* loss;                      /* total loss of the minibatch: a non-finite one skips the step (so does a non-finite gradient norm) */
    const float* bad_flag;                  /* optional: != 0 skips the step too (the multi-rank path's collective decision) */
    const float* kl;                        /* minibatch mean KL */
    float* lr;                              /* learning rate, in / out */
    const float *value_loss, *surrogate_loss;
    float* sums;                            /* [3] running statistics of the update (may be NULL) */
    float* partials;                        /* scratch: grx_ppo_step_tail_blocks(tensors) floats */
    int adaptive, pad;
    float desired_kl, lr_min, lr_max, max_grad_norm;
    double beta1, beta2, eps;
} grx_ppo_tail_args;
int grx_ppo_step_tail_blocks(const grx_ppo_tail_tensors* t);
int grx_ppo_step_tail(const grx_ppo_tail_tensors* t, const grx_ppo_tail_args* a, void* stream);

#define GRX_PPO_GATHER_MAX 12
int grx_ppo_gather_rows(int n_tensors, const float* const* src, float* const* dst, const int* widths, const long long* idx, int mb, void* stream);

int grx_mlp_layer(int M, int K, int N, const float* X, const float* W, const float* bias, float* Y, int elu, void* stream);

/* The bf16 matrix path of a hidden layer (PPO(precision="bf16")): the three products of a Linear layer with bf16 operands and fp32
 * accumulation on v_mfma_f32_32x32x16_bf16.  Operands stay fp32 in memory and are rounded to bf16 (round-to-nearest-even, NaN kept)
 * as they are loaded; outputs are fp32.  Each output's summation order is fixed by the shape (a row's result does not depend on the
 * rows beside it), and the weight gradient adds its batch slabs in a fixed order: the results are deterministic.  Contiguous
 * row-major fp32 everywhere; any size >= 1.  Return 0, or negative for invalid arguments (nothing is launched) / a failed launch.
 *   grx_mlp_layer_bf16:       Y [M][N] = act(bf16(X [M][K]) . bf16(W [N][K])^T + bias), act = ELU(alpha 1) when `elu` != 0
 *                             (grx_mlp_layer's signature and epilogue)
 *   grx_mlp_input_grad_bf16:  dX [M][K] = bf16(dZ [M][N]) . bf16(W [N][K])
 *   grx_mlp_weight_grad_bf16: dW [N][K] = bf16(dZ [M][N])^T . bf16(X [M][K]), summed over the M batch rows in slabs of rows;
 *                             `partials`: scratch of grx_mlp_weight_grad_bf16_partials_size(M, N, K) floats (0: invalid sizes) */
int grx_mlp_layer_bf16(int M, int K, int N, const float* X, const float* W, const float* bias, float* Y, int elu, void* stream);
int grx_mlp_input_grad_bf16(int M, int N, int K, const float* dZ, const float* W, float* dX, void* stream);
int grx_mlp_weight_grad_bf16_partials_size(int M, int N, int K);
int grx_mlp_weight_grad_bf16(int M, int N, int K, const float* dZ, const float* X, float* dW, float* partials, void* stream);

/* The actor's output layer fused with the rollout's sampling and log-probability (actor_critic_mlp.py act() /
 * get_actions_log_prob() -> torch.distributions.Normal): mu = X . W^T + bias, actions = mu + std * eps,
 * logp = sum_k -(a - mu)^2 / (2 std^2) - log(std) - log(sqrt(2 pi)); sigma = std broadcast to (M, A).
 * X [M][K], W [A][K], std [A], eps [M][A] standard-normal draws supplied by the caller.  1 <= A <= 32. */
int grx_mlp_policy_head(int M, int K, int A, const float* X, const float* W, const float* bias, const float* std,
                        const float* eps, float* actions, float* logp, float* mu, float* sigma, void* stream);

/* Empirical observation normalisation (rsl_rl 2.x `empirical_normalization`; rl/normalizer.py): the running mean and
 * variance of every column of an observation tensor x [rows][cols], and y = (x - mean) / (std + eps).  State per tensor, all on the
 * device: count (ONE int64: a float count stops being exact after 2^24 samples), mean / var / std [cols] fp32.  A training step is three
 * launches -- moments, merge, apply --, an evaluation step the third alone.  Deterministic: no atomics, every sum's order is a function
 * of (rows, cols) / of n_partials.  The state is written by the merge launch only (one block), never while another launch reads it.
 *   grx_obs_norm_moments: per slab of rows (the slab geometry is a function of (rows, cols) only) one CENTRED triple per column,
 *                         partials [slab][3][cols] = { n, mean, M2 = sum (x - mean)^2 }: the slab's mean is formed before its squares
 *                         are summed (never E[x^2] - mean^2).  `partials`: grx_obs_norm_partials_size(rows, cols) floats (0: invalid).
 *   grx_obs_norm_merge:   merges n_partials triples in index order (Chan et al.: n = na + nb, d = mb - ma, m = ma + d nb / n,
 *                         M2 = M2a + M2b + d^2 na nb / n), then the running update in place, with n, m, v = M2 / n of the merged batch:
 *                           count += n; rate = n / count; delta = m - mean; mean += rate * delta;
 *                           var += rate * (v - var + delta * (m - mean_new)); std = sqrt(var)
 *                         Triple p starts at partials + p * stride floats (stride 0: packed, 3 * cols): the same kernel consumes the
 *                         slab partials of one rank and the all_gathered triples of several ranks packed beside another tensor's.
 *   grx_obs_norm_combine: the same merge without a state: out [3][cols] = the one triple of all n_partials (a rank's contribution)
 *   grx_obs_norm_apply:   y [rows][cols] = (x - mean) / (std + eps); reads the state, writes y only (y may be x)
 *   grx_obs_norm_step:    moments, merge (packed partials) and apply of one training step behind one call: the same three launches
 * rows <= 2^24 per call (a triple carries n as a float).  Return 0, or negative for invalid sizes / NULL pointers (nothing is
 * launched) / a failed launch. */
int grx_obs_norm_partials_size(int rows, int cols);
int grx_obs_norm_moments(int rows, int cols, const float* x, float* partials, void* stream);
int grx_obs_norm_merge(int n_partials, int cols, int stride, const float* partials, long long* count, float* mean, float* var, float* std,
                       void* stream);
int grx_obs_norm_combine(int n_partials, int cols, const float* partials, float* out, void* stream);
int grx_obs_norm_apply(int rows, int cols, const float* x, const float* mean, const float* std, float eps, float* y, void* stream);
int grx_obs_norm_step(int rows, int cols, const float* x, float* partials, long long* count, float* mean, float* var, float* std, float eps,
                      float* y, void* stream);

/* Observation history (humanoid-gym `frame_stack`, Isaac Lab / rsl_rl 2.x `history_length`; rl/history.py): the policy
 * sees the last H frames of an observation of width D.  The stacked row of env n is H frames, oldest first, newest last:
 *   dones[n] == 0:  dst[n] = concat(src[n][D:], obs[n])       (shift by one frame, append the new one)
 *   dones[n] != 0:  dst[n] = obs[n] repeated H times          (obs[n] is already the first frame of the new episode)
 * dst [N][H*D] from src [N][H*D] and the new frame obs [N][D]; dones [N] uint8 or NULL; fill_all != 0 or dones == NULL: every row
 * filled (src is not read and may be NULL).  H == 1: dst = obs.  Out of place: src and dst are two buffers that the caller alternates.
 * One launch, pure copies (exact), no atomics.  Return 0, or negative with nothing launched for N, D, H < 1, N*H*D >= 2^31, NULL obs
 * or dst, NULL src when a row may shift, src == dst or overlapping src / dst or obs / dst ranges; negative for a failed launch. */
int grx_obs_history_push(int N, int D, int H, const float* obs, const unsigned char* dones, int fill_all, const float* src, float* dst,
                         void* stream);

/* Teacher-student policy distillation (rsl_rl 2.x `Distillation` / `StudentTeacher`; rl/distillation.py).
 *   grx_distill_loss: the behaviour loss of one minibatch and its gradient.  student_mu, teacher_mu [batch][A] contiguous; d = student -
 *                     teacher; huber == 0: e = d^2 (torch mse_loss), huber != 0: e = |d| <= 1 ? d^2 / 2 : |d| - 1 / 2 (torch huber_loss,
 *                     delta 1); out[0] = the mean of e over all batch * A elements, d_mu [batch][A] = d out[0] / d student_mu =
 *                     d * fl(2 / n), or clamp(d, -1, 1) * fl(1 / n).  Two launches: per-block partial sums (double), then one block that
 *                     adds them in block order; no atomics, the order of every sum is a function of batch * A alone.  A NaN in either
 *                     input gives a NaN out[0].  `partials`: 8-byte aligned scratch of grx_distill_loss_partials_size(batch, A) floats
 *                     (0: invalid sizes).  Any batch >= 1, A >= 1 with batch * A < 2^31.
 *   grx_distill_store: one rollout step in ONE launch: st_obs (N, D) = obs, st_labels (N, A) = labels, st_dones (N) uint8 = dones != 0,
 *                     each the contiguous storage row of this step, copied by dword; logging (all four may be NULL, `rewards` (N) may
 *                     then be NULL too): cur_rew += rewards, cur_len += 1, done_rew / done_len = the totals where done, cur_* zeroed
 *                     there -- grx_ppo_store_transition's arithmetic.
 * Return 0, or negative for invalid sizes / NULL pointers (nothing is launched, nothing written) / a failed launch. */
int grx_distill_loss_partials_size(int batch, int A);
int grx_distill_loss(int batch, int A, const float* student_mu, const float* teacher_mu, int huber, float* out, float* d_mu, float* partials,
                     void* stream);
int grx_distill_store(int N, int D, int A, const float* obs, const float* labels, const float* rewards, const unsigned char* dones,
                      float* st_obs, float* st_labels, unsigned char* st_dones,
                      float* cur_rew, float* cur_len, float* done_rew, float* done_len, void* stream);

/* The LSTM cell of the recurrent actor-critic (legged_gym `ActorCriticRecurrent`, rsl_rl `Memory`; rl/recurrent.py).
 * torch.nn.LSTM's formulas, gate order and weight layout, one layer:
 *     G = x W_ih^T + h' W_hh^T + b_ih + b_hh        G = [i | f | g | o], each H wide
 *     i, f, o = sigmoid(.)   g = tanh(.)            c = f c' + i g       h = o tanh(c)
 * (h', c') = (h_prev, c_prev) of the row, or zero where the row's `reset` byte is non-zero: the rollout's done-reset is part of the
 * next cell launch, there is no zeroing launch.
 *   grx_lstm_cell: ONE launch.  x [M][D]; h_prev, c_prev, h, c [M][H]; reset [M] uint8 or NULL (no row is reset); W_ih [4H][D],
 *                  W_hh [4H][H], b_ih, b_hh [4H]; acts [M][5H] or NULL: the four activated gates and tanh(c), [i | f | g | o | tanh c],
 *                  what grx_lstm_cell_backward reads.  Out of place: h / c must not overlap h_prev / c_prev (the caller alternates two
 *                  buffers, as with grx_obs_history_push).  Both products run on the f32 MFMA: every pre-activation is ONE fmaf chain
 *                  from zero over x's columns in index order, then over h_prev's, then + b_ih, then + b_hh.  A row's result depends
 *                  on that row's inputs alone: not on M, not on its neighbours.  No atomics.
 *   grx_lstm_cell_preact: the test hook: the same reduction, G [M][4H] (biases added) written instead of h, c and acts.
 *   grx_lstm_cell_backward: the element-wise half of the backward, one launch: from dh [M][H] (the gradient at h), dc_in [M][H] (the
 *                  gradient arriving at c from the step after; NULL: zero), acts, c_prev and reset:
 *                      do = dh tanh(c)     dc = dc_in + dh o (1 - tanh(c)^2)     di = dc g     dg = dc i     df = dc c'
 *                      dG [M][4H] = [ di i (1 - i) | df f (1 - f) | dg (1 - g^2) | do o (1 - o) ]      dc_prev [M][H] = dc f
 *                  with c' = 0 and dc_prev = 0 for a reset row (the caller zeroes those rows of dh_prev = dG W_hh likewise).
 * Return 0, or negative with nothing launched and nothing written for M, D < 1, H no multiple of 32 in 32..1024, M * 5H >= 2^31, a NULL
 * required pointer, or h / c overlapping h_prev / c_prev; negative for a failed launch. */
int grx_lstm_cell(int M, int D, int H, const float* x, const float* h_prev, const float* c_prev, const unsigned char* reset,
                  const float* W_ih, const float* W_hh, const float* b_ih, const float* b_hh, float* h, float* c, float* acts, void* stream);
int grx_lstm_cell_preact(int M, int D, int H, const float* x, const float* h_prev, const unsigned char* reset, const float* W_ih,
                         const float* W_hh, const float* b_ih, const float* b_hh, float* G, void* stream);
int grx_lstm_cell_backward(int M, int H, const float* dh, const float* dc_in, const float* acts, const float* c_prev,
                           const unsigned char* reset, float* dG, float* dc_prev, void* stream);

/* The minibatch of one PPO step WITH its mirror image (rsl_rl 2.x `symmetry_cfg`; rl/symmetry.py): grx_ppo_gather_rows's
 * contract -- host arrays of device pointers, at most GRX_PPO_GATHER_MAX tensors, idx int64 on the device -- with a second half.  For
 * every tensor t and r < mb, with s = idx[r] (idx == NULL: s = r, the stand-alone "mirror these rows" call):
 *     dst[t][r][:]      = src[t][s][:]
 *     dst[t][mb + r][j] = modes[t] == 2:  fmaf(scale[t][j], src[t][s][perm[t][j]], offset[t][j])   (offset[t] or offset NULL: a plain product)
 *                         modes[t] == 1:  src[t][s][j]                                              (values, advantages, returns, old_logp)
 *                         modes[t] == 0:  not written: dst[t] has mb rows only
 * modes / perm / scale / offset are HOST arrays of n_tensors entries; perm[t] int32 [widths[t]], scale[t] / offset[t] fp32 [widths[t]] on
 * the device, read by mode 2 only (perm, scale, offset and their entries may be NULL where no tensor needs them).  src[t] and dst[t] must
 * not overlap.  ONE launch: a block stages its tensor's map and four source rows in LDS, (3 + 4) * 4 bytes per column of the widest tensor,
 * so a width is at most GRX_SYM_MAX_WIDTH = 2048 (56 KiB): 12 stacked privileged frames of 168 columns.  Pure copies and one fmaf per
 * element, no atomics: deterministic, and a row's result does not depend on mb.  The kernel trusts the maps: a perm entry outside
 * 0..widths[t]-1 is refused where the maps are built (rl/symmetry.py).
 * Returns 0, or negative with nothing launched and nothing written for mb < 1, n_tensors outside 1..GRX_PPO_GATHER_MAX, a width outside
 * 1..GRX_SYM_MAX_WIDTH, a mode outside 0..2, mode 2 without perm[t] / scale[t], a NULL src / dst / widths / modes or entry of src / dst;
 * negative for a failed launch. */
#define GRX_SYM_MAX_WIDTH 2048
int grx_sym_gather_rows(int n_tensors, const float* const* src, float* const* dst, const int* widths, const int* modes,
                        const int* const* perm, const float* const* scale, const float* const* offset, const long long* idx, int mb,
                        void* stream);

/* The intrinsic reward of random network distillation for one rollout step (rsl_rl 2.x `rnd_cfg`; rl/rnd.py): the error of
 * the trained predictor against the fixed random target, divided by the running spread of its own discounted return, added to the env's
 * reward.  pred, targ: [N][E] contiguous fp32.  ret [N]: in/out, the per-env discounted return of r.  count (int64) / mean / var / std:
 * single-element device state of the return's normaliser, EmpiricalNormalization's for one column.  rewards [N]: in/out (the rollout
 * storage's row of this step).  intrinsic [N]: out.  raw [N]: out, or NULL.  Three launches in stream order:
 *     1. r[n] = sqrt(sum_e (targ[n][e] - pred[n][e])^2);  ret[n] = fmaf(gamma, ret[n], r[n]);  raw[n] = r[n];  per slab of 128 rows the
 *        centred triple {n, mean, M2} of the new ret -> partials (the slab's mean is formed before its squares are summed)
 *     2. grx_obs_norm_merge(slabs, cols = 1): the triples merged in index order, then count += n; rate = n / count; delta = m - mean;
 *        mean += rate * delta; var += rate * (v - var + delta * (m - mean_new)); std = sqrt(var).  One block; the only writer of the state
 *     3. x = weight * r[n] / (std + eps) with the std just written;  intrinsic[n] = x;  rewards[n] += x
 * The power of two >= E (at most 64) lanes share a row: a lane adds the squares of its elements j, j + G, ... in index order, the lanes add
 * in an xor butterfly -- the order of a row's sum is a function of E alone, so r[n] depends neither on N nor on the other rows; the slab
 * geometry is a function of N alone.  No atomics: the same inputs give the same bytes.  Between the first and the third launch `intrinsic`
 * holds r.  rewards, intrinsic, raw, ret must not overlap.  `partials`: 8-byte aligned scratch of grx_rnd_reward_partials_size(N) floats
 * (0: invalid N).
 * Returns 0, or negative with nothing launched and nothing written for N < 1, N > 2^24 (a triple carries its n as a float), E outside
 * 1..256, N * E >= 2^31, a NULL pointer other than raw or a misaligned `partials`; negative for a failed launch. */
int grx_rnd_reward_partials_size(int N);
int grx_rnd_reward(int N, int E, const float* pred, const float* targ, float gamma, float weight, float eps, float* ret, long long* count,
                   float* mean, float* var, float* std, float* rewards, float* intrinsic, float* raw, float* partials, void* stream);

#ifdef __cplusplus
}
#endif

/* ... and a state-dependent action noise: the loss and the policy head for an actor whose output layer is [mean | s],
 * csrc/grx_ppo_noise.hip in the same library */
#include "grx_ppo_noise.h"
/* ... and the action-smoothness regulariser: the minibatch with its successor and perturbed rows, and the two smoothness
 * losses, csrc/grx_ppo_smooth.hip in the same library */
#include "grx_ppo_smooth.h"
/* ... and the concurrent state estimator: its rollout forward -- copy, every layer, column select -- in one launch,
 * csrc/grx_ppo_est.hip in the same library */
#include "grx_ppo_est.h"
/* ... and value normalisation: the GAE scan, the advantages' normalisation and the returns' running statistics in three
 * launches, csrc/grx_ppo_gae.hip in the same library */
#include "grx_ppo_gae.h"
/* ... and the Lipschitz gradient penalty: the element-wise passes of the penalty and of its second-order backward,
 * csrc/grx_ppo_gp.hip in the same library */
#include "grx_ppo_gp.h"
/* ... and layer normalisation in the hidden layers: LayerNorm + ELU behind a layer's product, forward and backward,
 * csrc/grx_ppo_ln.hip in the same library */
#include "grx_ppo_ln.h"
/* ... and multi-critic PPO: a value head, a GAE pass and a value loss per group of reward terms,
 * csrc/grx_ppo_mc.hip in the same library */
#include "grx_ppo_mc.h"
/* ... and a Beta action distribution: the loss, the parameter map and the rollout's sample for an actor whose output
 * layer is [p | q], csrc/grx_ppo_beta.hip in the same library */
#include "grx_ppo_beta.h"
/* ... and the context-aided estimator network: the rollout's head behind the encoder, the reparameterisation with its
 * backward, and the estimation + reconstruction + KL loss, csrc/grx_ppo_cenet.hip in the same library */
#include "grx_ppo_cenet.h"
/* ... and constraints as terminations: the per-step violations, running maxima and termination probabilities with the
 * reward row's edit, and the GAE pass that discounts by them, csrc/grx_ppo_cat.hip in the same library */
#include "grx_ppo_cat.h"
/* ... and the recurrent distillation student: one step of the LSTM's backward through time -- dG_next W_hh, the sum with
 * the loss's gradient and the cell's element-wise backward -- in one launch, csrc/grx_ppo_bptt.hip in the same library */
#include "grx_ppo_bptt.h"
#endif
