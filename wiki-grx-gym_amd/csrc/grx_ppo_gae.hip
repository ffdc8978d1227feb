// grx_ppo_gae.hip -- the rollout's returns and value normalisation (include/grx_ppo_gae.h, grx_gae_returns; rl/value_norm.py).
// Three launches in stream order:
//   scan  : lane = env, t = T-1 .. 0; the arithmetic of RolloutStorage.compute_returns' loop operation for operation, uncontracted, so
//           `returns` is that loop's bit for bit.  A wave's load of one step covers 64 consecutive floats (dones: 64 bytes).  The next
//           value and the running advantage stay in registers, and so do two Welford triples (n, mean, M2), of a = returns - v and of
//           returns; the block's 64 lanes merge theirs by Chan's formula down a shuffle tree: one pair of triples per block, no re-read.
//   merge : ONE block, two threads: thread 0 merges the blocks' triples of a in index order, thread 1 those of the returns and, with a
//           state, applies grx_obs_norm_merge's running update to it (the only writer of the state)
//   apply : element-wise over T N
// A block is ONE wave of 64 envs: the geometry is a function of N alone, an env's results do not depend on its neighbours, and the tree's
// order is a function of nothing.  Triples are float64 (the returns are of order 10 with a spread of order 1: their fp32 Welford mean
// would carry the rounding of every step); the running update is fp32, as the observation normaliser's.  No atomics, no scratch, no LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grx_ppo.h"

namespace {

constexpr int GAE_ENVS = 64;                  // envs per block = lanes of its one wave
constexpr long long GAE_MAX_ROWS = 1ll << 24;   // a triple's n is read back as a float: exact up to here (grx_obs_norm's limit)

struct Triple {
    double n, m, M2;
};

__device__ inline void push(Triple& t, double inv_n, float x) {   // Welford; inv_n = 1 / (t.n + 1), the same for every lane
    const double d = (double)x - t.m;
    t.n += 1.0;
    t.m += d * inv_n;
    t.M2 += d * ((double)x - t.m);
}

__device__ inline void chan(Triple& a, const Triple& b) {   // a <- a merged with b; an empty b (a lane past N) changes nothing
    const double nab = a.n + b.n;
    if (b.n > 0.0) {
        const double d = b.m - a.m;
        a.m += d * (b.n / nab);
        a.M2 += b.M2 + d * d * (a.n * b.n / nab);
        a.n = nab;
    }
}

__device__ inline Triple wave_merge(Triple t) {   // lane 0 holds the 64 lanes' triple; the order is the tree's, a function of nothing
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Triple b;
        b.n = __shfl_down(t.n, o);
        b.m = __shfl_down(t.m, o);
        b.M2 = __shfl_down(t.M2, o);
        chan(t, b);
    }
    return t;
}

__global__ __launch_bounds__(GAE_ENVS) void gae_scan_kernel(int T, int N, const float* __restrict__ rewards, const float* __restrict__ values,
                                                            const unsigned char* __restrict__ dones, const float* __restrict__ last_values,
                                                            float gamma, float lam, float* __restrict__ returns, float* __restrict__ raw_adv,
                                                            double* __restrict__ partials) {
#pragma clang fp contract(off) reassociate(off)
    const int n = blockIdx.x * GAE_ENVS + threadIdx.x;
    const bool live = n < N;
    Triple ta = {0.0, 0.0, 0.0}, tr = {0.0, 0.0, 0.0};
    if (live) {
        float next = last_values[n], adv = 0.f;
        double k = 0.0;
#pragma unroll 4
        for (int t = T - 1; t >= 0; --t) {
            const size_t i = (size_t)t * N + n;
            const float r = rewards[i], v = values[i];
            const float alive = 1.0f - (float)dones[i];
            const float ag = alive * gamma;
            const float delta = (r + ag * next) - v;
            adv = delta + (ag * lam) * adv;
            const float ret = adv + v;
            const float a = ret - v;
            returns[i] = ret;
            raw_adv[i] = a;
            next = v;
            k += 1.0;
            const double inv = 1.0 / k;
            push(ta, inv, a);
            push(tr, inv, ret);
        }
    }
    ta = wave_merge(ta);
    tr = wave_merge(tr);
    if (threadIdx.x == 0) {   // (lane 0 of every block is live: the grid has ceil(N / 64) blocks)
        double* p = partials + (size_t)blockIdx.x * 6;
        p[0] = ta.n; p[1] = ta.m; p[2] = ta.M2;
        p[3] = tr.n; p[4] = tr.m; p[5] = tr.M2;
    }
}

// ONE block.  Thread 0: the advantages' moments.  Thread 1: the returns' batch moments and the running update (state == NULL: none).
__global__ __launch_bounds__(64) void gae_merge_kernel(int nb, const double* __restrict__ partials, float eps, long long* count, float* mean,
                                                       float* var, float* std_, float* scale, float* __restrict__ stats) {
#pragma clang fp contract(off) reassociate(off)
    const int w = threadIdx.x;
    if (w > 1) return;
    const double* p = partials + 3 * w;
    Triple t = {p[0], p[1], p[2]};
    for (int b = 1; b < nb; ++b) {
        const double* q = p + (size_t)b * 6;
        const Triple o = {q[0], q[1], q[2]};
        chan(t, o);
    }
    if (w == 0) {
        stats[0] = (float)t.m;
        stats[1] = (float)sqrt(t.M2 / (t.n - 1.0));   // (T N = 1: 0 / 0, NaN as torch.std)
        return;
    }
    const float m = (float)t.m, v = (float)(t.M2 / t.n);
    stats[2] = m;
    stats[3] = v;
    if (count) {   // grx_obs_norm_merge's update on one column
        const long long old_count = *count, n_total = (long long)t.n;
        const float rate = (float)((double)n_total / (double)(old_count + n_total));
        const float mean_old = *mean, var_old = *var;
        const float delta = m - mean_old;
        const float mean_new = mean_old + rate * delta;
        const float var_new = var_old + rate * (v - var_old + delta * (m - mean_new));
        const float s = sqrtf(var_new);
        *count = old_count + n_total;
        *mean = mean_new;
        *var = var_new;
        *std_ = s;
        *scale = s + eps;
    }
}

// (values_out may be values: every element is read and written by one thread; no __restrict__ on the two)
__global__ __launch_bounds__(256) void gae_apply_kernel(int total, const float* __restrict__ stats, const float* __restrict__ mean,
                                                        const float* __restrict__ scale, const float* values, float* values_out,
                                                        float* __restrict__ returns, float* __restrict__ advantages) {
#pragma clang fp contract(off) reassociate(off)
    const float ma = stats[0], sa = stats[1] + 1e-8f;
    const bool norm = mean != nullptr;
    const float mu = norm ? mean[0] : 0.f, sc = norm ? scale[0] : 1.f;
    const int step = gridDim.x * 256;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
        advantages[i] = (advantages[i] - ma) / sa;
        if (norm) {
            values_out[i] = (values[i] - mu) / sc;
            returns[i] = (returns[i] - mu) / sc;
        }
    }
}

inline int nblocks(int N) { return (N + GAE_ENVS - 1) / GAE_ENVS; }
inline bool bad_shape(int T, int N) { return T < 1 || N < 1 || (long long)T * N > GAE_MAX_ROWS; }
inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

}  // namespace

extern "C" int grx_gae_partials_size(int T, int N) { return bad_shape(T, N) ? 0 : nblocks(N) * 12; }   // two triples of three doubles per block

extern "C" int grx_gae_returns(int T, int N, const float* rewards, const float* values, const unsigned char* dones, const float* last_values,
                               float gamma, float lam, float eps, long long* count, float* mean, float* var, float* std, float* scale,
                               float* returns, float* advantages, float* values_out, float* stats, float* partials, void* stream) {
    if (bad_shape(T, N)) return -1;
    if (!rewards || !values || !dones || !last_values || !returns || !advantages || !values_out || !stats || !partials) return -1;
    const int given = (count != nullptr) + (mean != nullptr) + (var != nullptr) + (std != nullptr) + (scale != nullptr);
    if (given != 0 && given != 5) return -1;
    if ((uintptr_t)partials & 7) return -1;
    const size_t total = (size_t)T * N, fb = total * sizeof(float);
    struct Span {
        const void* p;
        size_t bytes;
    };
    const Span in[4] = {{rewards, fb}, {values, fb}, {dones, total}, {last_values, (size_t)N * sizeof(float)}};
    Span out[10] = {{returns, fb}, {advantages, fb}, {values_out, fb}, {stats, 4 * sizeof(float)},
                    {partials, (size_t)nblocks(N) * 12 * sizeof(float)}};
    int n_out = 5;
    if (given) {
        out[n_out++] = {count, sizeof(long long)};
        out[n_out++] = {mean, sizeof(float)};
        out[n_out++] = {var, sizeof(float)};
        out[n_out++] = {std, sizeof(float)};
        out[n_out++] = {scale, sizeof(float)};
    }
    for (int o = 0; o < n_out; ++o) {
        for (int i = 0; i < 4; ++i) {
            if (o == 2 && i == 1 && values_out == values) continue;   // the one allowed alias
            if (overlap(out[o].p, out[o].bytes, in[i].p, in[i].bytes)) return -1;
        }
        for (int q = o + 1; q < n_out; ++q)
            if (overlap(out[o].p, out[o].bytes, out[q].p, out[q].bytes)) return -1;
    }
    hipStream_t st = (hipStream_t)stream;
    const int nb = nblocks(N);
    hipLaunchKernelGGL(gae_scan_kernel, dim3(nb), dim3(GAE_ENVS), 0, st, T, N, rewards, values, dones, last_values, gamma, lam, returns, advantages,
                       (double*)partials);
    if (hipGetLastError() != hipSuccess) return -2;
    hipLaunchKernelGGL(gae_merge_kernel, dim3(1), dim3(64), 0, st, nb, (const double*)partials, eps, count, mean, var, std, scale, stats);
    if (hipGetLastError() != hipSuccess) return -3;
    const int blocks = (int)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024);
    hipLaunchKernelGGL(gae_apply_kernel, dim3(blocks), dim3(256), 0, st, (int)total, (const float*)stats, (const float*)mean, (const float*)scale,
                       values, values_out, returns, advantages);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}
