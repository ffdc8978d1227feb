/* grx_ppo_mc.h -- multi-critic PPO (rl/multi_critic.py): the critic has one value head per GROUP of reward terms, GAE runs
 * per group, every group's advantage is normalised on its own and the policy sees their weighted sum.  Part of libgrx_ppo.so
 * (csrc/grx_ppo_mc.hip); included by grx_ppo.h.  K groups, 1 <= K <= GRX_MC_MAX_GROUPS.  Contiguous row-major fp32 on one device, plain
 * device pointers unless said otherwise; no atomics, no scratch memory: the same inputs give the same bytes.  Every entry returns 0, or
 * negative with nothing launched and nothing written for the invalid arguments it lists; negative for a failed launch.
 *
 *   grx_mc_store: ONE launch per rollout step.  terms [NT][N] and base_terms [NB][N] (NULL: one table) are the step kernel's per-term
 *     reward tables (GRX_T_REWARD_TERMS, GRX_T_BASE_REWARD_TERMS), term_group [NT + NB] (int32, on the device; [NT] without the second
 *     table) the group each term feeds, -1 for a term that feeds none (its row is not read).  Per env n and group k:
 *         r = 0;  r = r + terms[t][n] for the t of group k in table order, the main table first        -- one fp32 chain, uncontracted
 *         st_values[n][k] = values[n][k];   st_rewards[n][k] = r + (time_outs[n] ? gamma values[n][k] : 0)
 *     the time-out bootstrap of grx_ppo_store_transition per head (time_outs: bytes, NULL for none).  One lane per (n, k): the two rows are
 *     written as one contiguous run, a term's row is read coalesced over n, and an env's results depend on that env alone.
 *     Refused: N < 1, K outside 1..GRX_MC_MAX_GROUPS, NT < 1, NB < 0, a base_terms with NB < 1, NT + NB > 256, a NULL terms / term_group /
 *     values / st_values / st_rewards, an output that overlaps an input or the other output.  A map entry outside -1..K-1 is visible to the
 *     device alone: the launch then writes nothing (the call still returns 0).  A caller validates the map where it builds it, on the
 *     host: rl.multi_critic.MultiCritic does, once, before the map is uploaded.
 *
 *   grx_mc_returns: THREE launches in stream order, the shape of grx_gae_returns, for a rollout of T steps of N envs: rewards / values /
 *     returns [T][N][K], dones [T][N] bytes, last_values [N][K], advantages [T][N], stats [K][2].  weights [K] is a HOST array, each
 *     entry finite and > 0.
 *       scan  : one lane per (env, group); a block is 64 envs x K groups and reads a step's [64][K] slab as 64 K consecutive floats.  Per
 *               column the recursion of grx_gae_returns, operation for operation with every operation rounded to fp32 on its own:
 *                   alive = 1 - done;  delta = r + (alive gamma) next - v;  adv = delta + ((alive gamma) lam) adv;
 *                   returns = adv + v;  a = returns - v
 *               so column k of `returns` is grx_gae_returns' on that column alone, bit for bit.  Each lane carries the Welford triple
 *               (n, mean, M2; float64) of its a; wave k of the block merges group k's 64 triples by Chan's formula down grx_gae_returns'
 *               tree: one triple per block and group in `partials`.
 *       merge : ONE block, thread k merges group k's triples in block-index order: stats[k] = (mean(a_k), sqrt(M2 / (n - 1))), the unbiased
 *               std (NaN for T N = 1, as torch.std).
 *       apply : advantages[t][n] = sum_k weights[k] ((a_k - stats[k][0]) / (stats[k][1] + 1e-8)), added in group order from zero, a_k
 *               recomputed as returns - values.  With K = 1 and weights = {1} the call is grx_gae_returns without a state
 *               (RolloutStorage.compute_returns): returns and advantages byte for byte.
 *     T N <= 2^24.  Refused: T < 1, N < 1, T N > 2^24, K outside 1..GRX_MC_MAX_GROUPS, a NULL pointer, a weight that is not finite and > 0,
 *     a partials that is not 8-byte aligned, an output that overlaps an input or another output.
 *   grx_mc_partials_size: the number of floats `partials` must hold for (T, N, K); 0 for a shape that is refused.
 *
 *   grx_mc_loss: grx_ppo_loss with K value heads.  value / returns / target_values / d_value are [batch][K]; the value loss is
 *     sum_k L_k, L_k the clipped (or plain) value loss of head k -- the same clip_param and value_loss_coef for every head:
 *         out[0..3] = surrogate, sum_k L_k, surrogate + value_loss_coef sum_k L_k - entropy_coef entropy, mean KL;   out[4 + k] = L_k
 *         d_mu [batch][A], d_std [A], d_value [batch][K]: the gradients of out[2]
 *     Two launches; per-block partials in float64, added in block order.  The non-finite-input contract is grx_ppo_loss's: finite where
 *     torch's spelling is finite, non-finite gradients exactly where autograd's are.  With K = 1 out[0..3], d_mu, d_std and d_value are
 *     grx_ppo_loss's byte for byte.
 *     Refused: batch < 1, num_actions outside 1..32, K outside 1..GRX_MC_MAX_GROUPS, a NULL pointer (target_values may be NULL without
 *     use_clipped_value_loss), a partials that is not 8-byte aligned, an output that overlaps an input or another output.
 *   grx_mc_loss_partials_size: the number of floats `partials` must hold; 0 for batch < 1. */
#ifndef GRX_PPO_MC_H
#define GRX_PPO_MC_H
#ifdef __cplusplus
extern "C" {
#endif

#define GRX_MC_MAX_GROUPS 8

int grx_mc_store(int N, int K, int NT, int NB, const float* terms, const float* base_terms, const int* term_group,
                 const float* values, const unsigned char* time_outs, float gamma, float* st_values, float* st_rewards, void* stream);

int grx_mc_partials_size(int T, int N, int K);

int grx_mc_returns(int T, int N, int K, const float* rewards, const float* values, const unsigned char* dones, const float* last_values,
                   const float* weights /* host */, float gamma, float lam, float* returns, float* advantages, float* stats,
                   float* partials, void* stream);

int grx_mc_loss_partials_size(int batch);

int grx_mc_loss(int batch, int num_actions, int K, const float* mu, const float* std, const float* value, const float* actions,
                const float* old_logp, const float* old_mu, const float* old_sigma, const float* advantages, const float* returns,
                const float* target_values, float clip_param, float value_loss_coef, float entropy_coef, int use_clipped_value_loss,
                float* out /* [4 + K] */, float* d_mu, float* d_std, float* d_value, float* partials, void* stream);

#ifdef __cplusplus
}
#endif
#endif
