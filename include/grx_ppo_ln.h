/* grx_ppo_ln.h -- a hidden layer with layer normalisation (Ba et al., 2016): Linear -> LayerNorm -> ELU, the part behind the matrix product
 * (rl/modules.py _TrainLinearLNELU, rl/fused_loss.py).  Part of libgrx_ppo.so (csrc/grx_ppo_ln.hip); included by
 * grx_ppo.h.  The product z = x W^T + b itself is grx_mlp_layer with elu = 0.
 *
 * Everything is fp32, row-major and contiguous; [rows][cols] with 1 <= cols <= 1024 and rows >= 1 (rows * cols < 2^31).  Every product and
 * sum is rounded on its own (no contraction), in the order written.
 *
 *   grx_ln_elu_forward:   per row r, with C = cols,
 *                             m    = (sum_j z[r][j]) / C,  then once  m = m + (sum_j (z[r][j] - m)) / C     (the residuals' mean: the fp32 sum of
 *                                    a row with a large common offset is off by ulps of the SUM; this brings m to the nearest fp32 number)
 *                             v    = (sum_j (z[r][j] - m)^2) / C          passes over the row held in registers, not E[z^2] - m^2
 *                             s    = 1 / sqrtf(v + eps)
 *                             xhat = (z[r][j] - m) * s
 *                             a    = gamma[j] * xhat + beta[j]
 *                             y[r][j] = a > 0 ? a : expm1f(a)
 *                         mean[r] = m and rstd[r] = s are written when both pointers are given; both NULL (inference): y alone, the same
 *                         bits.  One launch: a wave per row, lane l holds columns l, l + 64, ... (at most 16 of them); a row sum is the
 *                         lane's own values in that order, then a fixed xor butterfly over the 64 lanes (32, 16, ..., 1).  A row does not
 *                         depend on `rows` or on its neighbours.
 *   grx_ln_elu_backward:  dy [rows][cols] is the gradient arriving at y; y, z, mean, rstd as the forward call left them.
 *                             g    = dy * (y > 0 ? 1 : y + 1)             ELU' from the output, as grx_ppo_elu_backward_colsum
 *                             xhat = (z - mean[r]) * rstd[r]
 *                             q    = g * gamma[j]
 *                             c1   = (sum_j q) / C,   c2 = (sum_j q * xhat) / C          (row sums as in the forward call)
 *                             dz[r][j] = rstd[r] * ((q - c1) - xhat * c2)                the gradient arriving at z
 *                         The difference q - c1 cancels in every column whose q is close to the row's mean, so it is formed with what fp32
 *                         dropped: ql, the rounding errors of the two products of q = (dy e1) gamma (two fma), and r = mean_j ((q - c1) + ql),
 *                         the residuals' mean, kept apart from c1:  dz = rstd * ((((q - c1) - r) + ql) - xhat * c2).  The same value to
 *                         first order; a column where q - c1 is small keeps its leading digits.
 *                             dbeta[j]  = sum_r g,   dgamma[j] = sum_r g * xhat,   dbias[j] = sum_r dz[r][j]
 *                         Three launches: the row pass that writes dz; a column pass in grx_ppo_colsum's shape that recomputes g and xhat
 *                         and reads dz back -- slabs of 256 rows into `partials`, four interleaved accumulators per wave --; one pass that
 *                         adds the slabs of the 3 * cols columns in grx_ppo_colsum's order.  The three column sums therefore equal
 *                         grx_ppo_colsum applied to the matrices g, g * xhat and dz bit for bit.  No atomics: two calls give the same
 *                         bits.  `partials`: scratch of grx_ln_elu_backward_partials_size(rows, cols) floats (0: invalid sizes).
 *                         dbias is the gradient of the bias of the Linear in front (dz is what arrives at its output).
 *
 * LDS: the column pass holds 3 KiB of slab sums; the row kernels use none.  No scratch.
 * Every entry point returns 0, or negative with nothing launched and nothing written: rows < 1, cols < 1, cols > 1024,
 * rows * cols >= 2^31, a NULL required pointer, exactly one of mean / rstd NULL in the forward call, more than 65535 slabs in the backward
 * call; negative for a failed launch.  `stream` is a hipStream_t (NULL: the default stream). */
#ifndef GRX_PPO_LN_H
#define GRX_PPO_LN_H
#ifdef __cplusplus
extern "C" {
#endif

#define GRX_LN_MAX_COLS 1024

int grx_ln_elu_forward(int rows, int cols, const float* z, const float* gamma, const float* beta, float eps, float* y, float* mean,
                       float* rstd, void* stream);
int grx_ln_elu_backward_partials_size(int rows, int cols);
int grx_ln_elu_backward(int rows, int cols, const float* dy, const float* y, const float* z, const float* mean, const float* rstd,
                        const float* gamma, float* dz, float* dgamma, float* dbeta, float* dbias, float* partials, void* stream);

#ifdef __cplusplus
}
#endif
#endif
