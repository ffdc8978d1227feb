// grx_ppo_ln.hip -- LayerNorm + ELU behind a hidden layer's matrix product, forward and backward (include/grx_ppo_ln.h, rl/modules.py
// _TrainLinearLNELU).  The header states every element's expression; the kernels below compute exactly that, every operation
// rounded on its own (contraction off).  Memory-bound, no MFMA, no atomics:
//   row kernels          a wave per row, four rows per block; lane l holds columns l, l + 64, ... in registers (NV of them, NV a template
//                        parameter in {1, 2, 4, 8, 16}: every register index is static, nothing spills); a row sum is the lane's own values in
//                        order, then an xor butterfly over the wave, which leaves the same bits in every lane
//   column pass          grx_ppo_colsum's scheme for three sums at once: a wave reads 64 consecutive columns of a row, the four waves of a block
//                        interleave the 256 rows of a slab with four accumulators each; partials [slab][3 * cols]; one wave per column adds
//                        the slabs in order
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grx_ppo.h"

namespace {
constexpr int NTHR = 256;
constexpr int CS_ROWS = 256;     // rows per column-sum slab (grx_ppo_colsum's)

__device__ inline float wave_sum_all(float v) {
#pragma clang fp contract(off) reassociate(off)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- forward: y = ELU(gamma * xhat + beta), mean, rstd ------------------------------------------------------------------------------------
template <int NV>
__global__ __launch_bounds__(NTHR) void ln_elu_fwd_kernel(int rows, int cols, const float* __restrict__ z, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float eps, float* __restrict__ y,
                                                          float* __restrict__ mean, float* __restrict__ rstd) {
#pragma clang fp contract(off) reassociate(off)
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * (NTHR / 64) + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* zr = z + (size_t)r * cols;
    float v[NV];
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int c = lane + 64 * k;
        v[k] = c < cols ? zr[c] : 0.f;
        acc += v[k];
    }
    const float C = (float)cols;
    const float m0 = wave_sum_all(acc) / C;
    acc = 0.f;   // the residuals' mean on top: a row with a large common offset (1e4 + noise) gets the fp32 number nearest to its mean
#pragma unroll
    for (int k = 0; k < NV; ++k) acc += (lane + 64 * k < cols) ? v[k] - m0 : 0.f;
    const float m = m0 + wave_sum_all(acc) / C;
    acc = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int c = lane + 64 * k;
        v[k] = c < cols ? v[k] - m : 0.f;
        acc += v[k] * v[k];
    }
    const float s = 1.0f / sqrtf(wave_sum_all(acc) / C + eps);
    float* yr = y + (size_t)r * cols;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int c = lane + 64 * k;
        if (c < cols) {
            const float a = gamma[c] * (v[k] * s) + beta[c];
            yr[c] = a > 0.f ? a : expm1f(a);
        }
    }
    if (mean && lane == 0) { mean[r] = m; rstd[r] = s; }
}

// ---- backward, the row pass: dz ------------------------------------------------------------------------------------------------------------
template <int NV>
__global__ __launch_bounds__(NTHR) void ln_elu_bwd_row_kernel(int rows, int cols, const float* __restrict__ dy, const float* __restrict__ y,
                                                              const float* __restrict__ z, const float* __restrict__ mean,
                                                              const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                              float* __restrict__ dz) {
#pragma clang fp contract(off) reassociate(off)
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * (NTHR / 64) + (threadIdx.x >> 6);
    if (r >= rows) return;
    const size_t base = (size_t)r * cols;
    const float m = mean[r], s = rstd[r];
    float q[NV], ql[NV], xh[NV];
    float a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int c = lane + 64 * k;
        q[k] = 0.f; ql[k] = 0.f; xh[k] = 0.f;
        if (c < cols) {
            const float yy = y[base + c], d = dy[base + c], gm = gamma[c];
            const float e1 = yy > 0.f ? 1.0f : yy + 1.0f;
            const float g = d * e1;
            xh[k] = (z[base + c] - m) * s;
            q[k] = g * gm;
            ql[k] = fmaf(g, gm, -q[k]) + fmaf(d, e1, -g) * gm;   // what the two roundings of q = (dy e1) gamma dropped
        }
        a1 += q[k];
        a2 += q[k] * xh[k];
    }
    const float C = (float)cols;
    const float c1 = wave_sum_all(a1) / C, c2 = wave_sum_all(a2) / C;
    // q - c1 cancels wherever a column's q is close to the row's mean, and dz there is all rounding unless the difference is formed with
    // what the roundings dropped: q's low part, and the mean rm of the residuals (q - c1) + ql, kept apart from c1 instead of rounded into it
    a1 = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) a1 += (lane + 64 * k < cols) ? (q[k] - c1) + ql[k] : 0.f;
    const float rm = wave_sum_all(a1) / C;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int c = lane + 64 * k;
        if (c < cols) dz[base + c] = s * ((((q[k] - c1) - rm) + ql[k]) - xh[k] * c2);
    }
}

// ---- backward, the column pass: slab sums of g, g * xhat and dz ------------------------------------------------------------------------------
__global__ __launch_bounds__(NTHR) void ln_elu_bwd_col_partial(int rows, int cols, const float* __restrict__ dy, const float* __restrict__ y,
                                                               const float* __restrict__ z, const float* __restrict__ mean,
                                                               const float* __restrict__ rstd, const float* __restrict__ dz,
                                                               float* __restrict__ partials) {
#pragma clang fp contract(off) reassociate(off)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + lane;
    const int r0 = blockIdx.y * CS_ROWS, r1 = min(rows, r0 + CS_ROWS);
    float sb = 0.f, sg = 0.f, sd = 0.f;
    if (col < cols) {
        float b[4] = {0.f, 0.f, 0.f, 0.f}, g[4] = {0.f, 0.f, 0.f, 0.f}, d[4] = {0.f, 0.f, 0.f, 0.f};   // (grx_ppo_colsum's four interleaved accumulators, three times)
        auto one = [&](const int r, float& ab, float& ag, float& ad) {
            const size_t o = (size_t)r * cols + col;
            const float yy = y[o];
            const float gg = dy[o] * (yy > 0.f ? 1.0f : yy + 1.0f);
            const float xh = (z[o] - mean[r]) * rstd[r];
            ab += gg;
            ag += gg * xh;
            ad += dz[o];
        };
        int r = r0 + wv;
        for (; r + 12 < r1; r += 16) {
            one(r, b[0], g[0], d[0]); one(r + 4, b[1], g[1], d[1]); one(r + 8, b[2], g[2], d[2]); one(r + 12, b[3], g[3], d[3]);
        }
        for (; r < r1; r += 4) one(r, b[0], g[0], d[0]);
        sb = (b[0] + b[1]) + (b[2] + b[3]);
        sg = (g[0] + g[1]) + (g[2] + g[3]);
        sd = (d[0] + d[1]) + (d[2] + d[3]);
    }
    __shared__ float s_acc[3][4][64];
    s_acc[0][wv][lane] = sb; s_acc[1][wv][lane] = sg; s_acc[2][wv][lane] = sd;
    __syncthreads();
    if (wv < 3 && col < cols)   // wave w writes sum w: [slab][dbeta | dgamma | dbias]
        partials[(size_t)blockIdx.y * 3 * cols + (size_t)wv * cols + col] =
            (s_acc[wv][0][lane] + s_acc[wv][1][lane]) + (s_acc[wv][2][lane] + s_acc[wv][3][lane]);
}
// one wave per column of the 3 * cols: lane l adds slabs l, l + 64, ... (in order), then grx_ppo_colsum's shuffle tree
__global__ __launch_bounds__(NTHR) void ln_elu_bwd_col_final(int cols, int nslab, const float* __restrict__ partials, float* __restrict__ dbeta,
                                                             float* __restrict__ dgamma, float* __restrict__ dbias) {
    const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= 3 * cols) return;
    float t = 0.f;
    for (int b = lane; b < nslab; b += 64) t += partials[(size_t)b * 3 * cols + j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o);
    if (lane == 0) {
        const int which = j / cols, col = j - which * cols;
        (which == 0 ? dbeta : which == 1 ? dgamma : dbias)[col] = t;
    }
}

inline bool bad_size(int rows, int cols) {
    return rows < 1 || cols < 1 || cols > GRX_LN_MAX_COLS || (long long)rows * cols >= (1LL << 31);
}
inline int nslabs(int rows) { return (rows + CS_ROWS - 1) / CS_ROWS; }
}   // namespace

#define GRX_LN_DISPATCH(KERNEL, ...)                                                                                              \
    do {                                                                                                                          \
        const int nv = (cols + 63) / 64;                                                                                          \
        const dim3 grid((unsigned)((rows + NTHR / 64 - 1) / (NTHR / 64))), block(NTHR);                                           \
        if (nv <= 1) hipLaunchKernelGGL((KERNEL<1>), grid, block, 0, st, __VA_ARGS__);                                            \
        else if (nv <= 2) hipLaunchKernelGGL((KERNEL<2>), grid, block, 0, st, __VA_ARGS__);                                       \
        else if (nv <= 4) hipLaunchKernelGGL((KERNEL<4>), grid, block, 0, st, __VA_ARGS__);                                       \
        else if (nv <= 8) hipLaunchKernelGGL((KERNEL<8>), grid, block, 0, st, __VA_ARGS__);                                       \
        else hipLaunchKernelGGL((KERNEL<16>), grid, block, 0, st, __VA_ARGS__);                                                   \
    } while (0)

extern "C" int grx_ln_elu_forward(int rows, int cols, const float* z, const float* gamma, const float* beta, float eps, float* y, float* mean,
                                  float* rstd, void* stream) {
    if (bad_size(rows, cols) || !z || !gamma || !beta || !y || ((mean == nullptr) != (rstd == nullptr))) return -1;
    hipStream_t st = (hipStream_t)stream;
    GRX_LN_DISPATCH(ln_elu_fwd_kernel, rows, cols, z, gamma, beta, eps, y, mean, rstd);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int grx_ln_elu_backward_partials_size(int rows, int cols) {
    if (bad_size(rows, cols) || nslabs(rows) > 65535) return 0;
    const long long n = 3LL * nslabs(rows) * cols;
    return n >= (1LL << 31) ? 0 : (int)n;
}

extern "C" int grx_ln_elu_backward(int rows, int cols, const float* dy, const float* y, const float* z, const float* mean, const float* rstd,
                                   const float* gamma, float* dz, float* dgamma, float* dbeta, float* dbias, float* partials, void* stream) {
    if (bad_size(rows, cols) || nslabs(rows) > 65535) return -1;   // (the slabs are the grid's y dimension)
    if (!dy || !y || !z || !mean || !rstd || !gamma || !dz || !dgamma || !dbeta || !dbias || !partials) return -1;
    hipStream_t st = (hipStream_t)stream;
    GRX_LN_DISPATCH(ln_elu_bwd_row_kernel, rows, cols, dy, y, z, mean, rstd, gamma, dz);
    const int nslab = nslabs(rows);
    hipLaunchKernelGGL(ln_elu_bwd_col_partial, dim3((cols + 63) / 64, nslab), dim3(NTHR), 0, st, rows, cols, dy, y, z, mean, rstd,
                       (const float*)dz, partials);
    hipLaunchKernelGGL(ln_elu_bwd_col_final, dim3((3 * cols + 3) / 4), dim3(NTHR), 0, st, cols, nslab, (const float*)partials, dbeta, dgamma,
                       dbias);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
#undef GRX_LN_DISPATCH
