/* grx_ppo_cenet.h -- the context-aided estimator network (CENet: Nahrendra, Yu & Myung, "DreamWaQ: Learning Robust Quadrupedal Locomotion
 * With Implicit Terrain Imagination via Deep Reinforcement Learning", ICRA 2023; rl/cenet.py): the rollout's head behind
 * the encoder's layers, the update's reparameterisation with its backward, and the three-part loss with its gradient.  Part of
 * libgrx_ppo.so (csrc/grx_ppo_cenet.hip); included by grx_ppo.h.
 *
 * The encoder's output row is enc_out[n] = [v_hat (E) | mu (Z) | raw (Z)], and
 *     lv = clamp(raw, -10, 2),  sigma = exp(lv / 2),  z = fma(sigma, eps, mu)
 * sigma is the fp32 rounding of a double exp, z one fmaf: ONE device function for the head and the reparameterisation, so the same
 * (mu, raw, eps) give the same z bits in both.  The clamp's gradient is torch.clamp's: 1 for -10 <= raw <= 2, else 0 (a NaN: 0).
 *
 *   grx_cenet_head: ONE launch, a wave per row:
 *           out[n][0 .. D)              = x[n][:]                        an exact copy
 *           out[n][D .. D + E)          = enc_out[n][0 .. E)             an exact copy
 *           out[n][D + E .. D + E + Z)  = z(enc_out[n], eps[n])
 *           targets[n][e]               = pri[n][target_cols[e]]         an exact copy; pri or targets NULL: not written
 *       x [N][D], enc_out [N][E + 2Z], eps [N][Z], pri [N][P], out [N][D + E + Z], targets [N][E] row-major fp32 on the device;
 *       target_cols is a HOST array of E ints.  x moves as dwordx4 where D and D + E + Z are multiples of four and x and out are 16-byte
 *       aligned, dword by dword otherwise.  A row's result depends on that row alone, not on N.  No LDS, no atomics.
 *       Returns 0, or negative with nothing launched and nothing written for a NULL x / enc_out / eps / out, N or D < 1, D > 2048, E outside
 *       1..GRX_CENET_MAX_TARGETS, Z outside 1..GRX_CENET_MAX_LATENT, N * (D + E + Z) >= 2^31, out overlapping x, enc_out or eps, and -- when
 *       pri and targets are given -- P < 1, a NULL target_cols or an entry of it outside 0..P-1; negative for a failed launch.
 *
 *   grx_cenet_reparam: dec_in[r] = [v_hat | z] [mb][E + Z] from enc_out [mb][E + 2Z] and eps [mb][Z]; ONE launch, element-wise.
 *   grx_cenet_reparam_backward: d_enc_out [mb][E + 2Z] from d_dec_in [mb][E + Z]:
 *           d v_hat = d_dec_in[:, :E],   d mu = dz,   d raw = ((dz * eps) * sigma) * 0.5 where -10 <= raw <= 2, else +0
 *       Both return 0, or negative with nothing launched and nothing written for mb < 1, E / Z outside their ranges, mb * (E + 2Z) >= 2^31
 *       or a NULL pointer; negative for a failed launch.
 *
 *   grx_cenet_loss: enc_out [mb][E + 2Z], targets [mb][E], dec [mb][F], valid [mb] uint8; the decoder's target of row r is
 *       next[r * next_ld + next_off + f], f < F -- read in place from the gathered successor block, and only where valid[r] != 0.
 *       n_v = the number of valid rows:
 *           L_est = sum_r sum_e (v_hat - v)^2 / (mb E)
 *           L_rec = sum_{r valid} sum_f (dec - next)^2 / (F max(n_v, 1))
 *           L_kl  = sum_r sum_j (mu^2 + exp(lv) - lv - 1) / 2 / mb
 *           out[5] = { L_est, L_rec, L_kl, L = L_est + L_rec + beta L_kl, n_v }
 *           d_enc_out [mb][E + 2Z] = d L / d enc_out (the estimation and the KL part; raw's is 0 where the clamp saturates)
 *           d_dec [mb][F]          = d L / d dec
 *       The mask is a select: an invalid row adds exactly 0 to L_rec and its d_dec is exactly +0, whatever its successor block holds (a NaN
 *       there included); n_v = 0: L_rec = 0 and a zero d_dec.  Three launches: per block of 2048 elements of the [mb][E + Z + F] index
 *       space the three sums and the valid count, double, into `partials`; one wave that adds them in block order and writes out; the
 *       gradient, each element ONE rounding of a double expression.  No atomics: the order of every sum is a function of (mb, E, Z, F)
 *       alone.  `partials`: 8-byte aligned scratch of grx_cenet_loss_partials_size(mb, E, Z, F) floats (0: invalid sizes).
 *       Returns 0, or negative with nothing launched and nothing written for mb < 1 or >= 2^24, E / Z outside their ranges, F outside
 *       1..2048, mb * (E + 2Z + F) >= 2^31, next_off < 0, next_ld < next_off + F, mb * next_ld >= 2^31, a beta that is negative or not
 *       finite, a NULL pointer, a misaligned partials; negative for a failed launch. */
#ifndef GRX_PPO_CENET_H
#define GRX_PPO_CENET_H

#define GRX_CENET_MAX_TARGETS 8
#define GRX_CENET_MAX_LATENT 64
#define GRX_CENET_MAX_INPUT 2048
#define GRX_CENET_MAX_FRAME 2048

#ifdef __cplusplus
extern "C" {
#endif

int grx_cenet_head(int N, int D, int E, int Z, const float* x, const float* enc_out, const float* eps, int P, const float* pri,
                   const int* target_cols, float* out, float* targets, void* stream);

int grx_cenet_reparam(int mb, int E, int Z, const float* enc_out, const float* eps, float* dec_in, void* stream);
int grx_cenet_reparam_backward(int mb, int E, int Z, const float* enc_out, const float* eps, const float* d_dec_in, float* d_enc_out,
                               void* stream);

int grx_cenet_loss_partials_size(int mb, int E, int Z, int F);
int grx_cenet_loss(int mb, int E, int Z, int F, const float* enc_out, const float* targets, const float* dec, const float* next,
                   int next_ld, int next_off, const unsigned char* valid, float beta, float* out, float* d_enc_out, float* d_dec,
                   float* partials, void* stream);

#ifdef __cplusplus
}
#endif
#endif
