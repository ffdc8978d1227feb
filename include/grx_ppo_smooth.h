/* grx_ppo_smooth.h -- action-smoothness regularisation of the policy (CAPS: Mysore et al., "Regularizing Action Policies for Smooth
 * Control", ICRA 2021; rl/smooth.py): the minibatch with its successor rows and its perturbed rows behind it, and the two
 * smoothness losses with their gradient.  Part of libgrx_ppo.so (csrc/grx_ppo_smooth.hip); included by grx_ppo.h.
 *
 * Storage rows are s = t * N + e (T rollout steps, N envs).  Minibatch row r has the source row s = idx[r], t = s / N, and
 *     valid[r] = (t < T - 1) && dones[s] == 0
 * -- the row s + N is the same env one step later, unless the episode ended at s (the stored next row is a reset observation then) or s is
 * the rollout's last step (nothing is stored behind it).
 *
 *   grx_smooth_gather_rows: grx_ppo_gather_rows's contract -- HOST arrays of device pointers and widths, at most GRX_PPO_GATHER_MAX tensors,
 *       idx int64 [mb] on the device, every entry in 0 .. T * N - 1 (trusted, as grx_ppo_gather_rows trusts it) -- with extra row blocks
 *       behind tensor 0, in this order, W = widths[0]:
 *           dst[0][r][:]                         = src[0][s][:]
 *           want_succ:  dst[0][mb + r][:]        = src[0][valid[r] ? s + N : s][:]          (an invalid pair repeats its own row: finite data)
 *           want_pert:  dst[0][P * mb + r][j]    = fmaf(sigma, eps[r][j], src[0][s][j])     (P = 1 + (want_succ != 0); eps [mb][W])
 *       dst[0] has (1 + (want_succ != 0) + (want_pert != 0)) * mb rows; tensors 1 .. n-1 are the plain gather, mb rows.  valid [mb] uint8
 *       is written when want_succ; dones [T * N] uint8 is read when want_succ only.  ONE launch: pure copies and one fmaf per perturbed
 *       element, no atomics; a row's result depends on idx[r] and eps[r] alone, not on mb.  A tensor whose width is a multiple of four and
 *       whose pointers are 16-byte aligned moves as dwordx4, every other one dword by dword.
 *       Returns 0, or negative with nothing launched and nothing written for mb, N, T < 1, n_tensors outside 1..GRX_PPO_GATHER_MAX, a width
 *       < 1, a NULL src / dst / widths / idx or entry of src / dst, want_pert with a NULL eps, want_succ with a NULL dones or valid, a
 *       sigma that is negative or not finite, dst[0]'s rows overlapping src[0]'s T * N rows; negative for a failed launch.
 *
 *   grx_smooth_loss: mu [R * mb][A] = the actor's means on grx_smooth_gather_rows's tensor 0 (R = 1 + has_succ + has_pert, the same block
 *       order), valid [mb] uint8 (required iff has_succ), n_v = the number of valid rows:
 *           L_T = sum_{r valid} sum_a (mu[r][a] - mu[mb + r][a])^2 / (A * max(n_v, 1))           (0 without has_succ)
 *           L_S = sum_r sum_a (mu[r][a] - mu[P * mb + r][a])^2 / (A * mb)                        (0 without has_pert)
 *           out[4] = { L_T, L_S, coef_t * L_T + coef_s * L_S, n_v }
 *           d_mu [R * mb][A] = d out[2] / d mu: both sides of each difference, every row block written
 *       The mask is a select: an invalid row adds exactly 0 to L_T and its temporal gradient is exactly +0, whatever its successor block
 *       holds (a NaN there included); a NaN in a row that counts reaches out.  n_v = 0: L_T = 0 and a zero temporal gradient.
 *       Squares (not the paper's norm, which has no gradient at a zero difference -- what a masked row holds).  Three launches: per block
 *       of 2048 elements the two sums of squares and the valid count, double, into `partials`; one block that adds them in block order and
 *       writes out; the gradient, scaled by 2 coef / (A * max(n_v, 1)) and 2 coef / (A * mb) as fp32 constants.  No atomics: the order of
 *       every sum is a function of (mb, A) alone.  `partials`: 8-byte aligned scratch of grx_smooth_loss_partials_size(mb, A) floats (0:
 *       invalid sizes).
 *       Returns 0, or negative with nothing launched and nothing written for A outside 1..256, mb < 1 or >= 2^24, R * mb * A >= 2^31,
 *       neither has_succ nor has_pert, a NULL mu / out / d_mu / partials, has_succ with a NULL valid, a misaligned partials; negative for a
 *       failed launch. */
#ifndef GRX_PPO_SMOOTH_H
#define GRX_PPO_SMOOTH_H
#ifdef __cplusplus
extern "C" {
#endif

int grx_smooth_gather_rows(int n_tensors, const float* const* src, float* const* dst, const int* widths, const long long* idx, int mb,
                           int N, int T, const unsigned char* dones, int want_succ, int want_pert, const float* eps, float sigma,
                           unsigned char* valid, void* stream);

int grx_smooth_loss_partials_size(int mb, int A);
int grx_smooth_loss(int mb, int A, const float* mu, int has_succ, int has_pert, const unsigned char* valid, float coef_t, float coef_s,
                    float* out, float* d_mu, float* partials, void* stream);

#ifdef __cplusplus
}
#endif
#endif
