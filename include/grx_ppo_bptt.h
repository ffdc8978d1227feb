/* grx_ppo_bptt.h -- one step of an LSTM's backward through time in one launch (the recurrent distillation student, rl/distillation.py
 * StudentTeacherRecurrent / rl/recurrent.py LSTMSequenceBPTT).  Part of libgrx_ppo.so (csrc/grx_ppo_bptt.hip); included by
 * grx_ppo.h.
 *
 *   grx_lstm_bptt_step: ONE launch for what LSTMSequence.backward spells as a matrix product, an addcmul and grx_lstm_cell_backward.
 *     Per (row r, unit j):
 *       s  = ONE k-ordered fmaf chain from +0 over k = 0 .. 4H-1 of dG_next[r][k] W_hh[k][j]; +0 when dG_next is NULL (the sequence's
 *            last step) and +0 for a row whose reset_next byte is set, whatever dG_next holds there (the row is never read)
 *       dh = dh_out + s
 *       then exactly grx_lstm_cell_backward's formulas on dh, dc_in, acts [M][5H], c_prev and reset (grx_ppo.h), c' = 0 and dc_prev = 0
 *       for a row whose `reset` byte is set: dG [M][4H] and dc_prev [M][H].
 *     The product runs on v_mfma_f32_32x32x2_f32 (exact f32); a row's result depends on that row alone, not on M.  No atomics, no scratch
 *     memory.  reset_next, dc_in and reset may be NULL.
 *   grx_lstm_bptt_dh: the test hook: the same reduction, dh [M][H] = dh_out + s written and nothing else.
 *   grx_lstm_bptt_step_tile: the measurement hook: grx_lstm_bptt_step with the block's width in hidden units chosen by the caller
 *     (32, 64 or 128; 0: what grx_lstm_bptt_step takes).  Every width gives the same bytes.
 *   All return 0, or negative with nothing launched and nothing written for M < 1, H not a multiple of 32 in 32..1024, M * 5H >= 2^31, a
 *   NULL dh_out / acts / c_prev / dG / dc_prev (the hook: dh_out / dh), a NULL W_hh beside a dG_next, a dG (the hook: dh) that overlaps
 *   dG_next, a width other than those; negative for a failed launch. */
#ifndef GRX_PPO_BPTT_H
#define GRX_PPO_BPTT_H
#ifdef __cplusplus
extern "C" {
#endif

int grx_lstm_bptt_step(int M, int H,
                       const float* dG_next,               /* [M][4H], or NULL: the sequence's last step */
                       const float* W_hh,                  /* [4H][H] */
                       const unsigned char* reset_next,    /* [M] or NULL: rows whose NEXT step started from zero */
                       const float* dh_out,                /* [M][H]: the gradient arriving at h_t from the loss */
                       const float* dc_in,                 /* [M][H] or NULL */
                       const float* acts, const float* c_prev, const unsigned char* reset,   /* step t's, as grx_lstm_cell_backward takes them */
                       float* dG, float* dc_prev, void* stream);

int grx_lstm_bptt_dh(int M, int H, const float* dG_next, const float* W_hh, const unsigned char* reset_next, const float* dh_out,
                     float* dh, void* stream);

int grx_lstm_bptt_step_tile(int tile_units, int M, int H, const float* dG_next, const float* W_hh, const unsigned char* reset_next,
                            const float* dh_out, const float* dc_in, const float* acts, const float* c_prev, const unsigned char* reset,
                            float* dG, float* dc_prev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
