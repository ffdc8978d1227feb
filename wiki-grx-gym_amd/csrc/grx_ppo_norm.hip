// grx_ppo_norm.hip -- empirical observation normalisation for the PPO rollout (include/grx_ppo.h, grx_obs_norm_*).
// Running mean / variance of every observation column and y = (x - mean) / (std + eps), as three launches per tensor per env step:
//   moments: per slab of ON_ROWS rows and per column a CENTRED triple (n, mean, M2 = sum (x - mean)^2)
//   merge  : ONE block merges the triples in index order (Chan et al.) and applies the running update to the state in place
//   apply  : y from the state
// The state is written by the merge launch only, which no other launch overlaps on the stream: no block reads a half-updated
// mean.  No atomics anywhere; the order of every sum is a function of (rows, cols): the same inputs give the same bits.
// Strict IEEE arithmetic (the library's flags): divisions and square roots are correctly rounded, as in the torch spelling.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grx_ppo.h"

namespace {

constexpr int ON_ROWS = 128;           // rows per slab
constexpr int ON_WAVES = 4;            // waves per block: wave w reads rows w, w + 4, ... of the slab
constexpr int ON_RPW = ON_ROWS / ON_WAVES;
constexpr int ON_MAX_ROWS = 1 << 24;   // a triple carries its n as a float: exact up to here

// One block: 64 columns x one slab.  Lane = column, so a wave reads 64 consecutive floats of one row (256 B, coalesced along the
// row whatever the width).  The slab's 32 rows per wave stay in registers between the two passes: x is read once, the mean is
// formed before the squares are summed.
__global__ __launch_bounds__(64 * ON_WAVES) void obs_norm_moments_kernel(int rows, int cols, const float* __restrict__ x, float* __restrict__ partials) {
    __shared__ float red[ON_WAVES][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const int r0 = blockIdx.y * ON_ROWS;
    const int nr = min(ON_ROWS, rows - r0);
    const bool live = c < cols;
    const float* xp = x + (size_t)r0 * cols + c;
    float v[ON_RPW];
#pragma unroll
    for (int k = 0; k < ON_RPW; ++k) {
        const int r = w + ON_WAVES * k;
        v[k] = (live && r < nr) ? xp[(size_t)r * cols] : 0.f;
    }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < ON_RPW; ++k) s += v[k];
    red[w][lane] = s;
    __syncthreads();
    const float mean = ((red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane])) / (float)nr;
    __syncthreads();
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < ON_RPW; ++k) {
        const float d = v[k] - mean;
        q += (w + ON_WAVES * k < nr) ? d * d : 0.f;
    }
    red[w][lane] = q;
    __syncthreads();
    if (w == 0 && live) {
        float* p = partials + (size_t)blockIdx.y * 3 * cols;
        p[c] = (float)nr;
        p[cols + c] = mean;
        p[2 * cols + c] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
    }
}

// (n, mean, M2) of column c over triples 0 .. np-1, merged in index order
__device__ __forceinline__ void chan_merge(int np, int cols, int stride, const float* __restrict__ partials, int c, float& n, float& m, float& M2) {
    n = partials[c]; m = partials[cols + c]; M2 = partials[2 * cols + c];
    for (int p = 1; p < np; ++p) {
        const float* q = partials + (size_t)p * stride;
        const float nb = q[c], mb = q[cols + c], Mb = q[2 * cols + c];
        const float nab = n + nb, d = mb - m;
        m += d * (nb / nab);
        M2 += Mb + d * d * (n * nb / nab);
        n = nab;
    }
}

// ONE block.  Every thread reads the old count before the barrier, thread 0 writes the new one after it; each column's state is
// read and written by one thread only.
__global__ __launch_bounds__(256) void obs_norm_merge_kernel(int np, int cols, int stride, const float* __restrict__ partials, long long* count,
                                                             float* mean, float* var, float* std_) {
    const long long old_count = *count;
    __syncthreads();
    long long n_total = 0;
    for (int c = threadIdx.x; c < cols; c += 256) {
        float n, m, M2;
        chan_merge(np, cols, stride, partials, c, n, m, M2);
        n_total = (long long)n;
        const float rate = (float)((double)n_total / (double)(old_count + n_total));
        const float var_x = M2 / n;
        const float mean_old = mean[c], var_old = var[c];
        const float delta = m - mean_old;
        const float mean_new = mean_old + rate * delta;
        const float var_new = var_old + rate * (var_x - var_old + delta * (m - mean_new));
        mean[c] = mean_new;
        var[c] = var_new;
        std_[c] = sqrtf(var_new);
    }
    if (threadIdx.x == 0) *count = old_count + n_total;   // (cols >= 1: thread 0 has merged column 0)
}

// the same merge without a state: one triple out (what a rank contributes to the all_gather)
__global__ __launch_bounds__(256) void obs_norm_combine_kernel(int np, int cols, const float* __restrict__ partials, float* __restrict__ out) {
    for (int c = threadIdx.x; c < cols; c += 256) {
        float n, m, M2;
        chan_merge(np, cols, 3 * cols, partials, c, n, m, M2);
        out[c] = n; out[cols + c] = m; out[2 * cols + c] = M2;
    }
}

__global__ __launch_bounds__(256) void obs_norm_apply_kernel(long long total, int cols, const float* __restrict__ x, const float* __restrict__ mean,
                                                             const float* __restrict__ std_, float eps, float* __restrict__ y) {
    const long long step = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
        const int c = (int)(i % cols);
        y[i] = (x[i] - mean[c]) / (std_[c] + eps);
    }
}

inline int nslabs(int rows) { return (rows + ON_ROWS - 1) / ON_ROWS; }
inline bool bad_shape(int rows, int cols) { return rows < 1 || cols < 1 || rows > ON_MAX_ROWS; }

}  // namespace

extern "C" int grx_obs_norm_partials_size(int rows, int cols) { return bad_shape(rows, cols) ? 0 : nslabs(rows) * 3 * cols; }

extern "C" int grx_obs_norm_moments(int rows, int cols, const float* x, float* partials, void* stream) {
    if (bad_shape(rows, cols) || !x || !partials) return -1;
    hipLaunchKernelGGL(obs_norm_moments_kernel, dim3((cols + 63) / 64, nslabs(rows)), dim3(64 * ON_WAVES), 0, (hipStream_t)stream, rows, cols, x, partials);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int grx_obs_norm_merge(int n_partials, int cols, int stride, const float* partials, long long* count, float* mean, float* var, float* std,
                                  void* stream) {
    if (n_partials < 1 || cols < 1 || (stride != 0 && stride < 3 * cols) || !partials || !count || !mean || !var || !std) return -1;
    hipLaunchKernelGGL(obs_norm_merge_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, n_partials, cols, stride ? stride : 3 * cols, partials, count,
                       mean, var, std);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// a training step's three launches behind one call (the rollout is bound by what the host enqueues)
extern "C" int grx_obs_norm_step(int rows, int cols, const float* x, float* partials, long long* count, float* mean, float* var, float* std, float eps,
                                 float* y, void* stream) {
    if (bad_shape(rows, cols) || !x || !partials || !count || !mean || !var || !std || !y) return -1;
    int rc = grx_obs_norm_moments(rows, cols, x, partials, stream);
    if (rc == 0) rc = grx_obs_norm_merge(nslabs(rows), cols, 0, partials, count, mean, var, std, stream);
    if (rc == 0) rc = grx_obs_norm_apply(rows, cols, x, mean, std, eps, y, stream);
    return rc;
}

extern "C" int grx_obs_norm_combine(int n_partials, int cols, const float* partials, float* out, void* stream) {
    if (n_partials < 1 || cols < 1 || !partials || !out) return -1;
    hipLaunchKernelGGL(obs_norm_combine_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, n_partials, cols, partials, out);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int grx_obs_norm_apply(int rows, int cols, const float* x, const float* mean, const float* std, float eps, float* y, void* stream) {
    if (bad_shape(rows, cols) || !x || !mean || !std || !y) return -1;
    const long long total = (long long)rows * cols;
    const int blocks = (int)((total + 1023) / 1024 < 2048 ? (total + 1023) / 1024 : 2048);   // ~4 elements per thread, grid-stride above 2 M
    hipLaunchKernelGGL(obs_norm_apply_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, total, cols, x, mean, std, eps, y);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
