/* grx_ppo_cat.h -- constraints as terminations (CaT, Chane-Sane et al., IROS 2024; rl/constraints.py): a constraint violation
 * becomes a probability delta of ending the episode at that step, which scales the reward and the discount inside GAE.  Part of
 * libgrx_ppo.so (csrc/grx_ppo_cat.hip); included by grx_ppo.h.
 *
 *   A spec expands into C columns, 1 <= C <= 256, of F families, 1 <= F <= 8.  A column is one row of a device table:
 *     col_kind    GRX_CAT_TORQUE   c = |torques[n][src]| - hi            hi = soft_torque_limit * torque_limits[src], formed by the caller
 *                 GRX_CAT_DOF_VEL  c = |dof_vel[n][src]| - hi            likewise
 *                 GRX_CAT_DOF_POS  c = max(lo - dof_pos[n][src], dof_pos[n][src] - hi)
 *                 GRX_CAT_ACTION_RATE  c = |actions[n][src] - prev[n][src]| - hi
 *                 GRX_CAT_UPRIGHT  c = sqrt(g_x g_x + g_y g_y) - hi      on gravity[n][0..2]
 *     col_src     the source's column (a DOF or an action; ignored for UPRIGHT); a src outside the source's width yields c = 0
 *     col_family  the column's family 0 .. F-1, for the counters
 *     col_lo / col_hi / col_prob   fp32; col_prob is the family's maximum termination probability at this iteration
 *   c+ = c > 0 ? c : 0; a row whose dones byte is set has c+ = 0 in every column.
 *
 *   grx_cat_step: ONE call per rollout step, THREE launches in stream order:
 *     violations : one lane per (env, column), a block per 16 envs: the block's slab of c+ goes to the [N][C] scratch `cplus` as one
 *                  contiguous run, and through LDS to the block's column maxima (part_max [nb][C]) and its per-family counts of rows
 *                  with any c+ > 0 (part_count [nb][F], integers).  Element (n, j) of a source is read at p[n env_stride + j col_stride]:
 *                  the env publishes its state as (N, k) views with strides (1, N) over SoA storage, a test hands over contiguous rows
 *     merge      : ONE block: m = max over the blocks, c_max <- tau c_max + one_minus_tau m (two products, one sum, each rounded on its
 *                  own); counts <- (reset_counts ? 0 : counts) + the blocks' sum.  The only writer of c_max and counts
 *     apply      : one lane per env: delta = max over columns of col_prob clip(c+ / c_max, 0, 1), a column with c_max = 0 contributing 0;
 *                  term_prob_row[n] = delta; reward_row[n] = (1 - delta) r with r = reward_row[n] (clip_zero: r < 0 ? 0 : r), in place;
 *                  then the block writes prev[n][:] = dones[n] ? 0 : actions[n][:] for its envs (prev != NULL)
 *   max and integer sums are exact in any order; everything else is a single correctly rounded fp32 operation (no contraction): the results
 *   equal rl/constraints.py's torch spelling bit for bit.  No launch reads what another block of the same launch writes.  No atomics, no
 *   scratch memory.  `kinds` is the bit mask (1 << kind) of the kinds the table holds.
 *   Returns 0, or negative with nothing launched and nothing written for N < 1, N > 2^24, C < 1, C > 256, F < 1, F > 8, a NULL table /
 *   dones / c_max / counts / cplus / part_max / part_count / term_prob_row / reward_row, a kind in `kinds` whose source (or width D / A) is
 *   missing (ACTION_RATE needs actions and prev), a negative stride, bits in `kinds` beyond the five kinds or none, and an output that overlaps an input or
 *   another output; negative for a failed launch.
 *   grx_cat_step_blocks: nb, the number of rows part_max / part_count must hold for N envs; 0 for an N that is refused.
 *
 *   grx_cat_returns: grx_gae_returns without a value-normalisation state and with one more operand, term_prob [T][N]:
 *                 alive = (1 - done) (1 - term_prob)                           otherwise the same three launches, operation for operation
 *   With term_prob == 0 its returns, advantages and stats are byte-equal to grx_gae_returns with a NULL state; for any term_prob the
 *   returns equal the torch loop bit for bit.  stats[0..3] as grx_gae_returns'.  partials: grx_cat_partials_size(T, N) floats, 8-byte aligned.
 *   Returns 0, or negative with nothing launched and nothing written for T < 1, N < 1, T N > 2^24, a NULL pointer, a misaligned partials,
 *   an output that overlaps an input or another output; negative for a failed launch. */
#ifndef GRX_PPO_CAT_H
#define GRX_PPO_CAT_H
#ifdef __cplusplus
extern "C" {
#endif

#define GRX_CAT_MAX_COLUMNS 256
#define GRX_CAT_MAX_FAMILIES 8
#define GRX_CAT_TORQUE 0
#define GRX_CAT_DOF_VEL 1
#define GRX_CAT_DOF_POS 2
#define GRX_CAT_ACTION_RATE 3
#define GRX_CAT_UPRIGHT 4
#define GRX_CAT_NUM_KINDS 5

int grx_cat_step_blocks(int N);

int grx_cat_step(int N, int C, int F, int D, int A, int kinds,
                 const int* col_kind, const int* col_src, const int* col_family, const float* col_lo, const float* col_hi,
                 const float* col_prob,                                                    /* the column table, [C] each */
                 const float* torques, const float* dof_vel, const float* dof_pos,         /* [N][D]; NULL for a kind that is absent */
                 const float* actions,                                                     /* [N][A] */
                 const float* gravity,                                                     /* [N][3] */
                 const long long* src_strides,   /* host, [5][2]: the element strides (env, column) of the five sources in this order; NULL: contiguous rows */
                 const unsigned char* dones,                                               /* [N] */
                 float tau, float one_minus_tau, int clip_zero, int reset_counts,
                 float* prev,                                                              /* [N][A]; NULL without ACTION_RATE */
                 float* c_max, int* counts,                                                /* [C], [F]: the state */
                 float* cplus, float* part_max, int* part_count,                           /* [N][C], [nb][C], [nb][F]: scratch */
                 float* term_prob_row, float* reward_row,                                  /* [N], [N] (in place) */
                 void* stream);

int grx_cat_partials_size(int T, int N);

int grx_cat_returns(int T, int N, const float* rewards, const float* values, const unsigned char* dones, const float* term_prob,
                    const float* last_values, float gamma, float lam,
                    float* returns, float* advantages, float* stats, float* partials, void* stream);

#ifdef __cplusplus
}
#endif
#endif
