/* grx_ppo_est.h -- the concurrent state estimator's rollout forward (Ji et al., "Concurrent Training of a Control Policy and a State
 * Estimator", RA-L 2022; rl/estimator.py).  Part of libgrx_ppo.so (csrc/grx_ppo_est.hip); included by grx_ppo.h.
 *
 * The estimator is an MLP of n_layers Linear layers (2..4: one to three hidden layers and the output layer), Linear -> ELU(1) -> ... ->
 * Linear.  Layer l multiplies by W[l], [widths[l]][in] row-major with in = D for l = 0 and widths[l - 1] otherwise, and adds bias[l]
 * ([widths[l]], NULL: no bias).  E = widths[n_layers - 1] is the number of estimated columns.
 *
 *   grx_est_forward: ONE launch, a block per slab of 64 rows:
 *           out[n][0 .. D)      = x[n][:]                               an exact copy, dword by dword
 *           out[n][D .. D + E)  = est(x[n])                             hidden layers ELU(h W^T + b), the output layer linear
 *           targets[n][e]       = pri[n][target_cols[e]]                an exact copy; pri or targets NULL: not written
 *       Every layer's output stays in LDS as the next layer's operand ([k][row] tiles of row stride 65, two buffers of 256 columns);
 *       weights stream from L2 through a double-buffered 64 x 32 tile.  Each output is the chain grx_mlp_layer forms for it:
 *       v_mfma_f32_32x32x2_f32 from a zero accumulator with k ascending, then + bias, then the same ELU -- est(x) equals one grx_mlp_layer
 *       call per layer bit for bit, and a row's result does not depend on N or on the rows beside it.  No atomics, no scratch.
 *       x [N][D], pri [N][P], out [N][D + E], targets [N][E] row-major fp32 on the device; net's pointers are device pointers;
 *       target_cols is a HOST array of E ints.
 *       Returns 0, or negative with nothing launched and nothing written for a NULL net / x / out / W[l], N, D or E < 1, D > 2048,
 *       E > GRX_EST_MAX_TARGETS, a hidden width outside 1..GRX_EST_MAX_WIDTH, n_layers outside 2..GRX_EST_MAX_LAYERS, N * (D + E) >= 2^31,
 *       out overlapping x, and -- when pri and targets are given -- P < 1, a NULL target_cols or an entry of it outside 0..P-1; negative
 *       for a failed launch. */
#ifndef GRX_PPO_EST_H
#define GRX_PPO_EST_H

#define GRX_EST_MAX_LAYERS 4
#define GRX_EST_MAX_WIDTH 256
#define GRX_EST_MAX_TARGETS 8
#define GRX_EST_MAX_INPUT 2048

typedef struct grx_est_net {
    int n_layers;                             /* 2..GRX_EST_MAX_LAYERS */
    int widths[GRX_EST_MAX_LAYERS];           /* output width of each layer; widths[n_layers - 1] = E */
    const float* W[GRX_EST_MAX_LAYERS];       /* device, [widths[l]][in] row-major */
    const float* bias[GRX_EST_MAX_LAYERS];    /* device, [widths[l]], or NULL */
} grx_est_net;

#ifdef __cplusplus
extern "C" {
#endif

int grx_est_forward(const grx_est_net* net, int N, int D, const float* x, int P, const float* pri, const int* target_cols, float* out,
                    float* targets, void* stream);

#ifdef __cplusplus
}
#endif
#endif
