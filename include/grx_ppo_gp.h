/* grx_ppo_gp.h -- the element-wise passes of the Lipschitz gradient penalty (Chen et al., "Learning Smooth Humanoid Locomotion through
 * Lipschitz-Constrained Policies", 2024; rl/grad_penalty.py):  P = (1/B) sum_r || d logp_r / d x_r ||^2  of a
 * Linear -> ELU -> ... -> Linear actor with a Normal(mu, sigma) head, and the second-order pass that gives P's gradient.  Part of
 * libgrx_ppo.so (csrc/grx_ppo_gp.hip); included by grx_ppo.h.  The matrix products of the pass are not here: rl/grad_penalty.py runs them
 * through grx_mlp_layer and torch.
 *
 * Everything is fp32, row-major and contiguous; [B][n] is B rows of n columns.  With y the saved OUTPUT of a hidden layer,
 *     e1(y) = y > 0 ? 1 : y + 1          (ELU'(z) from the output, as grx_ppo_elu_backward_colsum)
 *     e2(y) = y < 0 ? y + 1 : 0          (ELU''(z) from the output; 0 at y == 0, where ELU'' jumps: torch's double backward takes that side)
 * Every product and sum below is rounded on its own (no contraction), in the order written, so an element equals its torch spelling bit
 * for bit.  An element of an element-wise output depends on its own row alone, not on B or on its neighbours.  A column sum is taken as
 * grx_ppo_colsum takes it: slabs of 256 rows into `partials` [slab][col], four interleaved accumulators per wave, then the slabs in order;
 * it depends on B through that slab order only.  No atomics anywhere: two calls give the same bits.
 *
 *   grx_gp_seed:            u[r][j]  = (a[r][j] - mu[r][j]) / (sigma[j] * sigma[j])                                    = d logp_r / d mu_rj
 *   grx_gp_gate:            h[r][k]  = g[r][k] * e1(y[r][k])
 *   grx_gp_sqnorm:          P[0]     = (float)((sum_i (double)g0[i]^2) / B),   i over all B * n elements.  Two launches: per block of 2048
 *                           elements the sum in double into `partials`, then one block adds the blocks in order.  `partials`: 8-byte aligned
 *                           scratch of grx_gp_sqnorm_partials_size(B, n) floats (0: invalid sizes).
 *   grx_gp_gate_backward:   one pass over a hidden layer [B][n] on the way down.  It reads hbar (the gradient arriving at h), g, y and dY
 *                           (the gradient arriving at the layer's output from the layer above) and writes
 *                               gbar[r][k] = hbar[r][k] * e1(y[r][k])                                   (only when gbar is not NULL)
 *                               dz[r][k]   = dY[r][k] * e1(y[r][k]) + (hbar[r][k] * g[r][k]) * e2(y[r][k])
 *                               db[k]      = sum_r dz[r][k]
 *                           `partials`: grx_ppo_colsum_partials_size(B, n) floats.  With hbar = 0 it is grx_ppo_elu_backward_colsum, whose
 *                           launch it replaces.  (gbar is what the sweep upwards needs BEFORE dY exists -- dY depends on it through every
 *                           layer above --, so rl/grad_penalty.py takes it from grx_gp_gate(hbar, y) there and passes NULL here.)
 *   grx_gp_seed_backward:   ubar [B][A] is the gradient arriving at u, dmu [B][A] the one arriving at mu from the rest of the loss:
 *                               dmu_out[r][j] = dmu[r][j] - ubar[r][j] / (sigma[j] * sigma[j])
 *                               dsigma[j]     = sum_r ubar[r][j] * ((-2 * (a[r][j] - mu[r][j])) / (sigma[j] * sigma[j] * sigma[j]))
 *                           dmu_out may be dmu itself.  `partials`: grx_ppo_colsum_partials_size(B, A) floats.
 *
 * Element-wise loads and stores are dwordx4 where the element count is a multiple of four and every pointer is 16-byte aligned, dwords
 * otherwise; the column-sum passes read a dword per lane, 64 consecutive columns of a row per wave.  No LDS beyond the 1 KiB the slab sums
 * and the 32 bytes the block sums use, no scratch.
 * Every entry point returns 0, or negative with nothing launched and nothing written for a NULL required pointer, B < 1, a width < 1 or
 * B * width >= 2^31 (grx_gp_sqnorm also: a misaligned partials; the two column-sum passes also: more than 65535 slabs); negative for a
 * failed launch.  `stream` is a hipStream_t (NULL: the default stream). */
#ifndef GRX_PPO_GP_H
#define GRX_PPO_GP_H
#ifdef __cplusplus
extern "C" {
#endif

int grx_gp_seed(int B, int A, const float* a, const float* mu, const float* sigma, float* u, void* stream);
int grx_gp_gate(int B, int n, const float* g, const float* y, float* h, void* stream);
int grx_gp_sqnorm_partials_size(int B, int n);
int grx_gp_sqnorm(int B, int n, const float* g0, float* P, float* partials, void* stream);
int grx_gp_gate_backward(int B, int n, const float* hbar, const float* g, const float* y, const float* dY, float* gbar, float* dz,
                         float* db, float* partials, void* stream);
int grx_gp_seed_backward(int B, int A, const float* ubar, const float* a, const float* mu, const float* sigma, const float* dmu,
                         float* dmu_out, float* dsigma, float* partials, void* stream);

#ifdef __cplusplus
}
#endif
#endif
