/* grx_ppo_beta.h -- libgrx_ppo.so's entry points for a Beta action distribution (csrc/grx_ppo_beta.hip).
 * Included at the end of grx_ppo.h, whose conventions hold: contiguous fp32 device pointers, `stream` a hipStream_t, 0 on success. */
#ifndef GRX_PPO_BETA_H
#define GRX_PPO_BETA_H
#ifdef __cplusplus
extern "C" {
#endif

/* A Beta policy (rl/beta.py, rl/modules.py `action_dist="beta"`): the actor's output layer has 2A outputs, raw[i] = [p (A) | q (A)],
 * alpha = 1 + softplus(p) and beta = 1 + softplus(q) in fp32 (torch.nn.functional.softplus, threshold 20), both >= 1.  The action lives in
 * unit-box coordinates, x in [2^-24, 1 - 2^-24]; the env receives lo + span x.  The constant sum_k log span_k of the density in action
 * units cancels in PPO's ratio and is left out of every log-probability and entropy here.
 *
 * Every lgamma, digamma and trigamma is evaluated in double on an argument >= 1 (below 1: NaN): digamma and trigamma by the upward
 * recurrence to an argument >= 10 and the asymptotic series, the products and differences around them in double too; results are rounded
 * to fp32 once.
 *
 * grx_ppo_loss_beta: grx_ppo_loss_sd for such a policy.  raw, d_raw: [batch][2A]; x, old_alpha, old_beta: [batch][A]; every other
 * argument as in grx_ppo_loss_sd, `out` = [surrogate, value loss, total, mean KL] included.  Per row
 *     logp = sum_k (a - 1) ln x + (b - 1) ln(1 - x) - lnB(a, b),            lnB = lgG(a) + lgG(b) - lgG(a + b)
 *     H    = sum_k lnB - (a - 1) psi(a) - (b - 1) psi(b) + (a + b - 2) psi(a + b)
 *     KL   = sum_k lnB(a, b) - lnB(a0, b0) + (a0 - a) psi(a0) + (b0 - b) psi(b0) + (a - a0 + b - b0) psi(a0 + b0)     (old || new)
 * summed over k in double and rounded once; the ratio, the clip, the surrogate, the value loss, the tie and clamp gradient rules and the
 * NaN propagation through max / clamp are grx_ppo_loss_sd's term for term.  The gradient of the total loss lands on the raw output:
 *     d_raw[i][k]     = (g_logp (ln x - psi(a) + psi(a + b)) - entropy_coef / batch (-(a - 1) psi1(a) + (a + b - 2) psi1(a + b))) sigmoid(p)
 *     d_raw[i][A + k] = the same with b, q and ln(1 - x)
 * (sigmoid as torch's softplus backward: z / (z + 1), z = exp(p); 1 above the threshold).  An x outside (0, 1) gives a NaN total loss.
 * Batch sums in double, block partials added in block order by a finalize launch: two launches, no atomics, the same inputs give the
 * same bytes.  `partials`: 8-byte aligned scratch of grx_ppo_loss_beta_partials_size(batch) floats (0: invalid batch).  Returns 0, or
 * negative with nothing launched and nothing written for batch < 1, A outside 1..32, a misaligned `partials` or a NULL pointer
 * (target_values may be NULL when use_clipped_value_loss == 0); negative for a failed launch. */
int grx_ppo_loss_beta_partials_size(int batch);
int grx_ppo_loss_beta(int batch, int A, const float* raw /*[batch][2A]*/, const float* value, const float* x,
                      const float* old_logp, const float* old_alpha, const float* old_beta,
                      const float* advantages, const float* returns, const float* target_values,
                      float clip_param, float value_loss_coef, float entropy_coef, int use_clipped_value_loss,
                      float* out /*[4]*/, float* d_raw /*[batch][2A]*/, float* d_value, float* partials, void* stream);

/* grx_beta_params: alpha[i][k] = 1 + softplus(raw[i][k]), beta[i][k] = 1 + softplus(raw[i][A + k]); raw [M][2A], alpha, beta [M][A].
 * The function grx_ppo_loss_beta applies to its raw input: the same raw gives the same bits.  One launch.  Returns 0, or negative with
 * nothing launched for M < 1, A outside 1..32 or a NULL pointer. */
int grx_beta_params(int M, int A, const float* raw /*[M][2A]*/, float* alpha, float* beta, void* stream);

/* grx_beta_sample: the rollout's sample from two gamma draws g1 ~ Gamma(alpha, 1), g2 ~ Gamma(beta, 1) (all [M][A]; lo, span [A]):
 *     x = min(max(g1 / (g1 + g2), 2^-24), 1 - 2^-24);   actions = fmaf(span, x, lo);   logp[i] = sum_k the loss's term at (alpha, beta, x)
 * logp [M].  The log-probability goes through the device functions and the summation order of grx_ppo_loss_beta: for the same
 * (alpha, beta, x) the two agree bit for bit, so a batch evaluated with the parameters it was sampled with has ratio 1 exactly.  A row's
 * result depends on that row alone.  One launch.  Returns 0, or negative with nothing launched for M < 1, A outside 1..32 or a NULL
 * pointer. */
int grx_beta_sample(int M, int A, const float* alpha, const float* beta, const float* g1, const float* g2,
                    const float* lo /*[A]*/, const float* span /*[A]*/, float* x, float* actions, float* logp /*[M]*/, void* stream);

/* grx_beta_functions: lgamma, digamma and trigamma of t[i] (>= 1; below: NaN) as the kernels above evaluate them, rounded to fp32 -- the
 * test hook.  t and the three outputs: [n].  Returns 0, or negative with nothing launched for n < 1 or a NULL pointer. */
int grx_beta_functions(int n, const float* t, float* lgamma_out, float* digamma_out, float* trigamma_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
