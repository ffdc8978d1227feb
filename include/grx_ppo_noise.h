/* grx_ppo_noise.h -- libgrx_ppo.so's entry points for a state-dependent action noise (csrc/grx_ppo_noise.hip).
 * Included at the end of grx_ppo.h, whose conventions hold: contiguous fp32 device pointers, `stream` a hipStream_t, 0 on success. */
#ifndef GRX_PPO_NOISE_H
#define GRX_PPO_NOISE_H
#ifdef __cplusplus
extern "C" {
#endif

/* A state-dependent action noise (rl/modules.py `state_dependent_std`): the actor's output layer has 2A outputs,
 * raw[i] = [mean (A) | s (A)], and sigma[i][k] = s (log_std == 0, `scalar`) or expf(s) (log_std != 0, `log`).
 *
 * grx_ppo_loss_sd: grx_ppo_loss for such a policy.  raw, d_raw: [batch][2A]; every other argument as in grx_ppo_loss, `out` included.
 * grx_ppo_loss's arithmetic term by term with m = raw[i][k], s = raw[i][A + k] (the same NaN propagation through max / clamp, the same
 * tie and clamp gradient rules, batch sums in double, block partials added in block order by a finalize launch).  The entropy is a fourth
 * batch sum: the mean over rows of sum_k (1/2 + 1/2 log 2 pi + log sigma_ik), where log sigma is s itself under `log` (where expf(s)
 * saturates to inf or 0 it is logf of that, +-inf as torch's: a finite loss must not stand over such a row).  The gradient of
 * the total loss lands on the raw output:
 *     d_raw[i][k]     = g_logp df / sigma^2                                    (grx_ppo_loss's d_mu expression)
 *     d sigma         = g_logp (df^2 / sigma^3 - 1 / sigma) - entropy_coef / (batch sigma)
 *     d_raw[i][A + k] = d sigma (`scalar`),  d sigma * sigma (`log`)
 * With `scalar` a non-positive s gives a NaN (or infinite) total loss, as a non-positive std does in grx_ppo_loss.  Two launches, no
 * atomics: the same inputs give the same bytes.  `partials`: 8-byte aligned scratch of grx_ppo_loss_sd_partials_size(batch) floats (0:
 * invalid batch).  Returns 0, or negative with nothing launched and nothing written for batch < 1, A outside 1..32, a misaligned
 * `partials` or a NULL pointer (target_values may be NULL when use_clipped_value_loss == 0); negative for a failed launch. */
int grx_ppo_loss_sd_partials_size(int batch);
int grx_ppo_loss_sd(int batch, int A, const float* raw /*[batch][2A]*/, int log_std, const float* value,
                    const float* actions, const float* old_logp, const float* old_mu, const float* old_sigma,
                    const float* advantages, const float* returns, const float* target_values,
                    float clip_param, float value_loss_coef, float entropy_coef, int use_clipped_value_loss,
                    float* out /*[4]*/, float* d_raw /*[batch][2A]*/, float* d_value, float* partials, void* stream);

/* grx_mlp_policy_head_sd: grx_mlp_policy_head for the 2A-wide output layer, W [2A][K] and bias [2A] (or NULL) = [mean rows | s rows]:
 *     mu = X Wm^T + bm;  s = X Ws^T + bs;  sigma = s or expf(s);  actions = mu + sigma * eps;
 *     logp[i] = sum_k -(a - mu)^2 / (2 sigma^2) - log sigma - log sqrt(2 pi)          (log sigma = s under `log`)
 * eps, actions, mu, sigma: [M][A]; logp [M].  One launch.  Products on v_mfma_f32_32x32x2_f32, every output one k-ordered fmaf chain from
 * zero, then + bias: mu and the raw s equal grx_mlp_layer(X, that half of W, that half of bias, elu = 0) bit for bit, and a row's result
 * depends on that row alone.  Deterministic, no atomics.  Returns 0, or negative with nothing launched for M < 1, K < 1, A outside 1..32
 * or a NULL pointer other than bias; negative for a failed launch. */
int grx_mlp_policy_head_sd(int M, int K, int A, const float* X, const float* W /*[2A][K]*/, const float* bias /*[2A]*/,
                           int log_std, const float* eps /*[M][A]*/, float* actions, float* logp, float* mu, float* sigma, void* stream);

#ifdef __cplusplus
}
#endif
#endif
