// grx_ppo_smooth.hip -- action-smoothness regularisation of the policy (include/grx_ppo_smooth.h; rl/smooth.py).
//
// grx_smooth_gather_rows: grx_ppo_gather_rows with up to two more row blocks behind tensor 0 -- the successor row s + N of every minibatch
// row s = idx[r] (the row itself again where the pair is no trajectory step: a done at s, or s in the rollout's last step), and the row
// perturbed by sigma * eps.  ONE launch.  A block works on rows of ONE tensor (blockIdx.y), one WAVE per row, four rows per pass; a wave
// reads idx[r] (and, tensor 0, dones[s]) as wave-uniform values, then walks the row: lane l elements l, l + 64, ... -- every load and store
// of a wave covers 64 consecutive units.  A unit is a float4 (global_load_dwordx4) when the host found the tensor's width a multiple of
// four and all its pointers 16-byte aligned, so that every row of it starts on a 16-byte boundary; a dword otherwise (widths such as 39
// leave rows mutually misaligned).  Pure copies and one fmaf per perturbed element; no LDS, no atomics, no barrier: a row's bytes depend
// on idx[r] and eps[r] alone.
//
// grx_smooth_loss: the two losses and their gradient in three launches.  mu's row blocks are contiguous [mb][A] matrices, walked as flat
// arrays of n = mb * A elements: block b owns elements [b * SL_CHUNK, (b + 1) * SL_CHUNK), thread t of it t, t + 256, ... (coalesced
// whatever A is); element i belongs to row i / A.  Launch 1: per element the squared differences in double (the fp32 difference is exact
// in double), selected -- not multiplied -- by the row's valid byte; a row's first element counts the row.  A thread adds its eight
// elements in index order, a wave its lanes in a shuffle tree, thread 0 the four waves in wave order -> partials[b] = {sum_T, sum_S, n_v}.
// Launch 2 (one wave): lane l adds the partials l, l + 64, ... in order, then the same tree -> out[4].  Launch 3: the gradient, each
// element ONE rounding of a double expression (so the sum of the temporal and the spatial part on the unextended rows is rounded once,
// however the two cancel); masked rows get +0 in the temporal part by a select.  The order of every sum is a function of (mb, A) alone.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/grx_ppo.h"

namespace {

// ---- the gather ---------------------------------------------------------------------------------------------------------------------
constexpr int SMG_WAVES = 4;   // rows per pass of a block

struct SmoothGatherArgs {
    const float* src[GRX_PPO_GATHER_MAX]; float* dst[GRX_PPO_GATHER_MAX];
    int width[GRX_PPO_GATHER_MAX], vec[GRX_PPO_GATHER_MAX];
    const long long* idx; const unsigned char* dones; const float* eps; unsigned char* valid;
    int mb, N, T, want_succ, want_pert;
    float sigma;
};

__global__ __launch_bounds__(64 * SMG_WAVES) void smooth_gather_kernel(SmoothGatherArgs a) {
    const int t = blockIdx.y, w = a.width[t];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool succ = t == 0 && a.want_succ, pert = t == 0 && a.want_pert;
    const float* __restrict__ src = a.src[t];
    float* __restrict__ dst = a.dst[t];
    const size_t mb = (size_t)a.mb;
    const size_t pert_block = a.want_succ ? 2 * mb : mb;
    const float sigma = a.sigma;
    for (size_t r = (size_t)blockIdx.x * SMG_WAVES + wave; r < mb; r += (size_t)gridDim.x * SMG_WAVES) {
        const long long s = a.idx[r];
        bool v = false;
        if (succ) {
            v = (s / a.N < (long long)(a.T - 1)) && a.dones[s] == 0;
            if (lane == 0) a.valid[r] = v ? 1 : 0;
        }
        const float* x = src + (size_t)s * w;
        const float* xs = src + (size_t)(v ? s + a.N : s) * w;
        const float* e = pert ? a.eps + r * w : nullptr;
        float* out = dst + r * w;
        float* outs = dst + (mb + r) * w;
        float* outp = dst + (pert_block + r) * w;
        if (a.vec[t]) {
            const int w4 = w >> 2;
            for (int j = lane; j < w4; j += 64) {
                const float4 q = ((const float4*)x)[j];
                ((float4*)out)[j] = q;
                if (succ) ((float4*)outs)[j] = ((const float4*)xs)[j];
                if (pert) {
                    const float4 n = ((const float4*)e)[j];
                    float4 p;
                    p.x = fmaf(sigma, n.x, q.x); p.y = fmaf(sigma, n.y, q.y); p.z = fmaf(sigma, n.z, q.z); p.w = fmaf(sigma, n.w, q.w);
                    ((float4*)outp)[j] = p;
                }
            }
        } else {
            for (int j = lane; j < w; j += 64) {
                const float q = x[j];
                out[j] = q;
                if (succ) outs[j] = xs[j];
                if (pert) outp[j] = fmaf(sigma, e[j], q);
            }
        }
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---- the loss -------------------------------------------------------------------------------------------------------------------------
constexpr int SL_THR = 256;              // threads per block
constexpr int SL_PER = 8;                // elements per thread
constexpr int SL_CHUNK = SL_THR * SL_PER;

__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;   // lane 0 holds the sum
}

__global__ __launch_bounds__(SL_THR) void smooth_loss_partials_kernel(int n, int A, const float* __restrict__ mu, int has_succ, int has_pert,
                                                                      const unsigned char* __restrict__ valid, double* __restrict__ partials) {
    __shared__ double waves[3][SL_THR / 64];
    const float* __restrict__ mu_s = mu + (size_t)n;
    const float* __restrict__ mu_p = mu + (size_t)(has_succ ? 2 : 1) * n;
    const long long base = (long long)blockIdx.x * SL_CHUNK + threadIdx.x;
    double acc_t = 0.0, acc_s = 0.0, cnt = 0.0;
#pragma unroll
    for (int k = 0; k < SL_PER; ++k) {
        const long long i = base + (long long)k * SL_THR;
        if (i < n) {
            const double m0 = (double)mu[i];
            if (has_succ) {
                const int r = (int)(i / A);
                if (valid[r] != 0) {   // a select: a masked row's successor is not even looked at
                    const double d = m0 - (double)mu_s[i];   // exact
                    acc_t += d * d;
                    if (i - (long long)r * A == 0) cnt += 1.0;
                }
            }
            if (has_pert) {
                const double d = m0 - (double)mu_p[i];
                acc_s += d * d;
            }
        }
    }
    acc_t = wave_sum(acc_t); acc_s = wave_sum(acc_s); cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0) { waves[0][threadIdx.x >> 6] = acc_t; waves[1][threadIdx.x >> 6] = acc_s; waves[2][threadIdx.x >> 6] = cnt; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const double* wv = waves[threadIdx.x];
        partials[(size_t)blockIdx.x * 3 + threadIdx.x] = ((wv[0] + wv[1]) + wv[2]) + wv[3];
    }
}

__global__ __launch_bounds__(64) void smooth_loss_finalize_kernel(int mb, int A, int nblk, int has_succ, int has_pert, float coef_t, float coef_s,
                                                                  const double* __restrict__ partials, float* __restrict__ out) {
    double sum_t = 0.0, sum_s = 0.0, cnt = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 64) {
        sum_t += partials[(size_t)b * 3];
        sum_s += partials[(size_t)b * 3 + 1];
        cnt += partials[(size_t)b * 3 + 2];
    }
    sum_t = wave_sum(sum_t); sum_s = wave_sum(sum_s); cnt = wave_sum(cnt);
    if (threadIdx.x == 0) {
        const double lt = has_succ ? sum_t / ((double)A * (cnt > 1.0 ? cnt : 1.0)) : 0.0;
        const double ls = has_pert ? sum_s / ((double)A * (double)mb) : 0.0;
        double total = 0.0;
        if (has_succ) total += (double)coef_t * lt;
        if (has_pert) total += (double)coef_s * ls;
        out[0] = (float)lt; out[1] = (float)ls; out[2] = (float)total; out[3] = (float)cnt;   // (cnt < 2^24: exact)
    }
}

__global__ __launch_bounds__(SL_THR) void smooth_loss_grad_kernel(int n, int mb, int A, const float* __restrict__ mu, int has_succ, int has_pert,
                                                                  const unsigned char* __restrict__ valid, float coef_t, float coef_s,
                                                                  const float* __restrict__ out, float* __restrict__ d_mu) {
    const float* __restrict__ mu_s = mu + (size_t)n;
    const float* __restrict__ mu_p = mu + (size_t)(has_succ ? 2 : 1) * n;
    float* __restrict__ d_s = d_mu + (size_t)n;
    float* __restrict__ d_p = d_mu + (size_t)(has_succ ? 2 : 1) * n;
    const double nv = (double)out[3];
    const double g_t = 2.0 * (double)coef_t / ((double)A * (nv > 1.0 ? nv : 1.0));
    const double g_s = 2.0 * (double)coef_s / ((double)A * (double)mb);
    const long long base = (long long)blockIdx.x * SL_CHUNK + threadIdx.x;
#pragma unroll
    for (int k = 0; k < SL_PER; ++k) {
        const long long i = base + (long long)k * SL_THR;
        if (i < n) {
            const double m0 = (double)mu[i];
            double own = 0.0;
            if (has_succ) {
                double gt = 0.0;
                if (valid[(int)(i / A)] != 0) gt = g_t * (m0 - (double)mu_s[i]);
                own += gt;
                d_s[i] = (float)(0.0 - gt);   // (masked: +0, not -0)
            }
            if (has_pert) {
                const double gs = g_s * (m0 - (double)mu_p[i]);
                own += gs;
                d_p[i] = (float)(-gs);
            }
            d_mu[i] = (float)own;
        }
    }
}

inline long long smooth_elements(int mb, int A) {
    if (mb < 1 || mb >= (1 << 24) || A < 1 || A > 256) return 0;
    const long long n = (long long)mb * A;
    return n < (1ll << 31) ? n : 0;
}

}  // namespace

extern "C" int grx_smooth_gather_rows(int n_tensors, const float* const* src, float* const* dst, const int* widths, const long long* idx, int mb,
                                      int N, int T, const unsigned char* dones, int want_succ, int want_pert, const float* eps, float sigma,
                                      unsigned char* valid, void* stream) {
    if (n_tensors < 1 || n_tensors > GRX_PPO_GATHER_MAX || mb < 1 || N < 1 || T < 1 || !src || !dst || !widths || !idx) return -1;
    if (want_pert && !eps) return -1;
    if (want_succ && (!dones || !valid)) return -1;
    if (!(sigma >= 0.0f) || !isfinite(sigma)) return -1;
    for (int t = 0; t < n_tensors; ++t)
        if (!src[t] || !dst[t] || widths[t] < 1) return -1;
    const int R = 1 + (want_succ ? 1 : 0) + (want_pert ? 1 : 0);
    {   // dst[0]'s R * mb rows against src[0]'s T * N rows
        const uintptr_t s0 = (uintptr_t)src[0], s1 = s0 + (size_t)T * N * widths[0] * sizeof(float);
        const uintptr_t d0 = (uintptr_t)dst[0], d1 = d0 + (size_t)R * mb * widths[0] * sizeof(float);
        if (d0 < s1 && s0 < d1) return -1;
    }
    SmoothGatherArgs a;
    for (int t = 0; t < GRX_PPO_GATHER_MAX; ++t) {
        const int u = t < n_tensors ? t : 0;
        a.src[t] = src[u]; a.dst[t] = dst[u]; a.width[t] = widths[u];
        a.vec[t] = (widths[u] % 4 == 0 && aligned16(src[u]) && aligned16(dst[u]) && (u != 0 || !want_pert || aligned16(eps))) ? 1 : 0;
    }
    a.idx = idx; a.dones = dones; a.eps = eps; a.valid = valid;
    a.mb = mb; a.N = N; a.T = T; a.want_succ = want_succ ? 1 : 0; a.want_pert = want_pert ? 1 : 0; a.sigma = sigma;
    const int passes = (mb + SMG_WAVES - 1) / SMG_WAVES;
    const int bx = passes < 1024 ? passes : 1024;
    hipLaunchKernelGGL(smooth_gather_kernel, dim3(bx, n_tensors), dim3(64 * SMG_WAVES), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int grx_smooth_loss_partials_size(int mb, int A) {
    const long long n = smooth_elements(mb, A);
    return n ? (int)((n + SL_CHUNK - 1) / SL_CHUNK) * 6 : 0;   // three doubles per block
}

extern "C" int grx_smooth_loss(int mb, int A, const float* mu, int has_succ, int has_pert, const unsigned char* valid, float coef_t, float coef_s,
                               float* out, float* d_mu, float* partials, void* stream) {
    const long long n = smooth_elements(mb, A);
    has_succ = has_succ ? 1 : 0; has_pert = has_pert ? 1 : 0;
    if (!n || (1 + has_succ + has_pert) * n >= (1ll << 31)) return -1;
    if (!has_succ && !has_pert) return -1;   // (no second row block: there is no loss)
    if (!mu || !out || !d_mu || !partials || ((uintptr_t)partials & 7) || (has_succ && !valid)) return -1;
    const int nblk = (int)((n + SL_CHUNK - 1) / SL_CHUNK);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(smooth_loss_partials_kernel, dim3(nblk), dim3(SL_THR), 0, st, (int)n, A, mu, has_succ, has_pert, valid, (double*)partials);
    hipLaunchKernelGGL(smooth_loss_finalize_kernel, dim3(1), dim3(64), 0, st, mb, A, nblk, has_succ, has_pert, coef_t, coef_s,
                       (const double*)partials, out);
    hipLaunchKernelGGL(smooth_loss_grad_kernel, dim3(nblk), dim3(SL_THR), 0, st, (int)n, mb, A, mu, has_succ, has_pert, valid, coef_t, coef_s,
                       (const float*)out, d_mu);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
