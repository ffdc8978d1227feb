/* grx_ppo_gae.h -- the rollout's returns: the GAE scan, the advantages' normalisation and, with a state, value normalisation (running
 * statistics of the returns; rl/value_norm.py).  Part of libgrx_ppo.so (csrc/grx_ppo_gae.hip); included by grx_ppo.h.
 *
 *   grx_gae_returns: THREE launches in stream order, for a rollout of T steps of N envs ([T][N] contiguous fp32, dones bytes):
 *     scan  : one lane per env, t = T-1 .. 0, the next value and the running advantage in registers, every access coalesced over n:
 *                 alive = 1 - done;  delta = r + (alive gamma) next - v;  adv = delta + ((alive gamma) lam) adv;
 *                 returns = adv + v;  a = returns - v                         each operation rounded to fp32 on its own (no contraction):
 *             `returns` equals RolloutStorage.compute_returns' torch loop bit for bit, and an env's column depends on that column alone.
 *             Each lane carries one Welford triple (n, mean, M2) of its a and one of its returns, the block's 64 lanes merge theirs by
 *             Chan's formula in a fixed order: one pair of triples per block in `partials`, no re-read.  The triples are kept in float64.
 *     merge : ONE block merges the blocks' triples in index order.  stats[0..3] = mean(a), the unbiased std(a) = sqrt(M2 / (n - 1)) (NaN for
 *             T N = 1, as torch.std), the batch mean m and the population variance v of the raw returns.  With a state, the running update
 *             of the observation normaliser on one column, in fp32:
 *                 count += n;  rate = n / count;  delta = m - mean;  mean += rate delta;  var += rate (v - var + delta (m - mean_new));
 *                 std = sqrt(var);  scale = std + eps                              -- this launch is the only writer of the state
 *     apply : advantages = (a - stats[0]) / (stats[1] + 1e-8); with a state also values_out = (values - mean) / scale and
 *             returns = (returns - mean) / scale under the statistics just written.  Without one, returns stay raw and values_out is not
 *             written: the call is RolloutStorage.compute_returns.
 *   The state is five one-element device tensors, count (int64) and mean / var / std / scale (fp32): all given or all NULL.
 *   values_out may be values itself.  No atomics, no scratch memory: the same inputs give the same bytes.  T N <= 2^24 (a triple's n is
 *   read back as a float).
 *   Returns 0, or negative with nothing launched and nothing written for T < 1, N < 1, T N > 2^24, a NULL rewards / values / dones /
 *   last_values / returns / advantages / values_out / stats / partials, a state of which only a part is given, a partials that is not
 *   8-byte aligned, and an output that overlaps an input (other than values_out == values) or another output; negative for a failed
 *   launch.
 *   grx_gae_partials_size: the number of floats `partials` must hold for (T, N), a function of N alone; 0 for a shape that is refused. */
#ifndef GRX_PPO_GAE_H
#define GRX_PPO_GAE_H
#ifdef __cplusplus
extern "C" {
#endif

int grx_gae_partials_size(int T, int N);

int grx_gae_returns(int T, int N, const float* rewards, const float* values, const unsigned char* dones, const float* last_values,
                    float gamma, float lam, float eps,
                    long long* count, float* mean, float* var, float* std, float* scale,   /* all NULL: no value normalisation */
                    float* returns, float* advantages, float* values_out, float* stats, float* partials, void* stream);

#ifdef __cplusplus
}
#endif
#endif
