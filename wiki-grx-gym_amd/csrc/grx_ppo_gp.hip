// grx_ppo_gp.hip -- the element-wise passes of the Lipschitz gradient penalty and of its second-order backward (include/grx_ppo_gp.h,
// rl/grad_penalty.py).  The header states every element's expression; the kernels below compute exactly that, every
// operation rounded on its own (contraction off), so an element equals its torch spelling bit for bit.  Memory-bound, no MFMA, no atomics:
//   seed, gate           flat element-wise kernels, dwordx4 where count and alignment allow
//   sqnorm               2048 elements per block summed in double (wave shuffle tree, four wave sums through LDS), then one block over the
//                        partials in order
//   gate_backward,       grx_ppo_colsum's scheme: a wave reads 64 consecutive columns of a row, the four waves of a block interleave the
//   seed_backward        256 rows of a slab with four accumulators each; partials [slab][col]; one wave per column adds the slabs in order
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grx_ppo.h"

namespace {
constexpr int NTHR = 256;
constexpr int CS_ROWS = 256;     // rows per column-sum slab (grx_ppo_colsum's)
constexpr int SQ_PER = 2048;     // elements per block of grx_gp_sqnorm

__device__ inline float e1(float y) { return y > 0.f ? 1.0f : y + 1.0f; }
__device__ inline float e2(float y) { return y < 0.f ? y + 1.0f : 0.0f; }   // (0 at y == 0: torch's double backward of ELU)

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- seed: u = (a - mu) / sigma^2 ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NTHR) void gp_seed_kernel(long long n, int A, const float* __restrict__ a, const float* __restrict__ mu,
                                                       const float* __restrict__ sigma, float* __restrict__ u, int vec) {
#pragma clang fp contract(off) reassociate(off)
    const long long t = (long long)blockIdx.x * NTHR + threadIdx.x;
    if (vec) {
        const long long i = t * 4;
        if (i >= n) return;
        const float4 av = *reinterpret_cast<const float4*>(a + i), mv = *reinterpret_cast<const float4*>(mu + i);
        const float aa[4] = {av.x, av.y, av.z, av.w}, mm[4] = {mv.x, mv.y, mv.z, mv.w};
        float o[4];
        int j = (int)(i % A);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float s = sigma[j];
            o[k] = (aa[k] - mm[k]) / (s * s);
            j = j + 1 == A ? 0 : j + 1;
        }
        *reinterpret_cast<float4*>(u + i) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
        if (t >= n) return;
        const float s = sigma[(int)(t % A)];
        u[t] = (a[t] - mu[t]) / (s * s);
    }
}

// ---- gate: h = g * e1(y) ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NTHR) void gp_gate_kernel(long long n, const float* __restrict__ g, const float* __restrict__ y,
                                                       float* __restrict__ h, int vec) {
#pragma clang fp contract(off) reassociate(off)
    const long long t = (long long)blockIdx.x * NTHR + threadIdx.x;
    if (vec) {
        const long long i = t * 4;
        if (i >= n) return;
        const float4 gv = *reinterpret_cast<const float4*>(g + i), yv = *reinterpret_cast<const float4*>(y + i);
        *reinterpret_cast<float4*>(h + i) = make_float4(gv.x * e1(yv.x), gv.y * e1(yv.y), gv.z * e1(yv.z), gv.w * e1(yv.w));
    } else {
        if (t >= n) return;
        h[t] = g[t] * e1(y[t]);
    }
}

// ---- sqnorm: P = (sum g0^2) / B --------------------------------------------------------------------------------------------------------
__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}
// the block's 256 values -> their sum in thread 0 (a fixed tree: shuffle within the wave, the four wave sums in order)
__device__ inline double block_sum(double v, double* s_w) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    return (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}
__global__ __launch_bounds__(NTHR) void gp_sqnorm_partial(long long n, const float* __restrict__ g0, double* __restrict__ partials) {
    __shared__ double s_w[4];
    const long long base = (long long)blockIdx.x * SQ_PER;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < SQ_PER / NTHR; ++k) {
        const long long i = base + k * NTHR + threadIdx.x;
        if (i < n) { const double v = (double)g0[i]; acc += v * v; }
    }
    const double t = block_sum(acc, s_w);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}
__global__ __launch_bounds__(NTHR) void gp_sqnorm_final(int nblk, int B, const double* __restrict__ partials, float* __restrict__ P) {
    __shared__ double s_w[4];
    double acc = 0.0;
    for (int b = threadIdx.x; b < nblk; b += NTHR) acc += partials[b];
    const double t = block_sum(acc, s_w);
    if (threadIdx.x == 0) P[0] = (float)(t / (double)B);
}

// ---- the column-sum passes ---------------------------------------------------------------------------------------------------------------
// F::one(o, col) writes what the pass writes at element o = r * cols + col and returns the value whose column sum is wanted
template <class F>
__global__ __launch_bounds__(NTHR) void gp_colsum_partial(int rows, int cols, F f, float* __restrict__ partials) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + lane;
    const int r0 = blockIdx.y * CS_ROWS, r1 = min(rows, r0 + CS_ROWS);
    float acc = 0.f;
    if (col < cols) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;   // (the same four interleaved accumulators as grx_ppo_colsum)
        int r = r0 + wv;
        for (; r + 12 < r1; r += 16) {
            a0 += f.one((size_t)r * cols + col, col); a1 += f.one((size_t)(r + 4) * cols + col, col);
            a2 += f.one((size_t)(r + 8) * cols + col, col); a3 += f.one((size_t)(r + 12) * cols + col, col);
        }
        for (; r < r1; r += 4) a0 += f.one((size_t)r * cols + col, col);
        acc = (a0 + a1) + (a2 + a3);
    }
    __shared__ float s_acc[4][64];
    s_acc[wv][lane] = acc;
    __syncthreads();
    if (wv == 0 && col < cols) partials[(size_t)blockIdx.y * cols + col] = (s_acc[0][lane] + s_acc[1][lane]) + (s_acc[2][lane] + s_acc[3][lane]);
}
// one wave per column: lane l adds slabs l, l + 64, ... (in order), then a fixed shuffle tree
__global__ __launch_bounds__(NTHR) void gp_colsum_final(int cols, int nslab, const float* __restrict__ partials, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, col = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (col >= cols) return;
    float t = 0.f;
    for (int b = lane; b < nslab; b += 64) t += partials[(size_t)b * cols + col];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o);
    if (lane == 0) out[col] = t;
}

struct GateBackward {
    const float* hbar; const float* g; const float* y; const float* dY; float* gbar; float* dz;
    __device__ inline float one(size_t o, int) const {
#pragma clang fp contract(off) reassociate(off)
        const float yy = y[o], hb = hbar[o];
        const float d1 = e1(yy);
        if (gbar) gbar[o] = hb * d1;
        const float v = dY[o] * d1 + (hb * g[o]) * e2(yy);
        dz[o] = v;
        return v;
    }
};

struct SeedBackward {
    const float* ubar; const float* a; const float* mu; const float* sigma; const float* dmu; float* dmu_out;
    __device__ inline float one(size_t o, int col) const {
#pragma clang fp contract(off) reassociate(off)
        const float s = sigma[col], ub = ubar[o];
        dmu_out[o] = dmu[o] - ub / (s * s);
        return ub * ((-2.0f * (a[o] - mu[o])) / (s * s * s));
    }
};

inline bool bad_size(int B, int n) { return B < 1 || n < 1 || (long long)B * n >= (1LL << 31); }
inline bool bad_slabs(int B) { return (B + CS_ROWS - 1) / CS_ROWS > 65535; }   // (the slabs are the grid's y dimension)

template <class F>
int colsum_pass(int rows, int cols, const F& f, float* out, float* partials, hipStream_t st) {
    const int nslab = (rows + CS_ROWS - 1) / CS_ROWS;
    hipLaunchKernelGGL(gp_colsum_partial<F>, dim3((cols + 63) / 64, nslab), dim3(NTHR), 0, st, rows, cols, f, partials);
    hipLaunchKernelGGL(gp_colsum_final, dim3((cols + 3) / 4), dim3(NTHR), 0, st, cols, nslab, partials, out);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
}   // namespace

extern "C" int grx_gp_seed(int B, int A, const float* a, const float* mu, const float* sigma, float* u, void* stream) {
    if (bad_size(B, A) || !a || !mu || !sigma || !u) return -1;
    const long long n = (long long)B * A;
    const int vec = (n % 4 == 0 && aligned16(a) && aligned16(mu) && aligned16(u)) ? 1 : 0;
    const long long thr = vec ? n / 4 : n;
    hipLaunchKernelGGL(gp_seed_kernel, dim3((unsigned)((thr + NTHR - 1) / NTHR)), dim3(NTHR), 0, (hipStream_t)stream, n, A, a, mu, sigma, u, vec);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int grx_gp_gate(int B, int n_, const float* g, const float* y, float* h, void* stream) {
    if (bad_size(B, n_) || !g || !y || !h) return -1;
    const long long n = (long long)B * n_;
    const int vec = (n % 4 == 0 && aligned16(g) && aligned16(y) && aligned16(h)) ? 1 : 0;
    const long long thr = vec ? n / 4 : n;
    hipLaunchKernelGGL(gp_gate_kernel, dim3((unsigned)((thr + NTHR - 1) / NTHR)), dim3(NTHR), 0, (hipStream_t)stream, n, g, y, h, vec);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// in floats (the buffer holds doubles: 2 floats each; the caller's allocation must be 8-byte aligned)
extern "C" int grx_gp_sqnorm_partials_size(int B, int n) {
    return bad_size(B, n) ? 0 : (int)(((long long)B * n + SQ_PER - 1) / SQ_PER) * 2;
}

extern "C" int grx_gp_sqnorm(int B, int n_, const float* g0, float* P, float* partials, void* stream) {
    if (bad_size(B, n_) || !g0 || !P || !partials || (reinterpret_cast<uintptr_t>(partials) & 7)) return -1;
    const long long n = (long long)B * n_;
    const int nblk = (int)((n + SQ_PER - 1) / SQ_PER);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gp_sqnorm_partial, dim3(nblk), dim3(NTHR), 0, st, n, g0, reinterpret_cast<double*>(partials));
    hipLaunchKernelGGL(gp_sqnorm_final, dim3(1), dim3(NTHR), 0, st, nblk, B, reinterpret_cast<const double*>(partials), P);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int grx_gp_gate_backward(int B, int n, const float* hbar, const float* g, const float* y, const float* dY, float* gbar, float* dz,
                                    float* db, float* partials, void* stream) {
    if (bad_size(B, n) || bad_slabs(B) || !hbar || !g || !y || !dY || !dz || !db || !partials) return -1;
    return colsum_pass(B, n, GateBackward{hbar, g, y, dY, gbar, dz}, db, partials, (hipStream_t)stream);
}

extern "C" int grx_gp_seed_backward(int B, int A, const float* ubar, const float* a, const float* mu, const float* sigma, const float* dmu,
                                    float* dmu_out, float* dsigma, float* partials, void* stream) {
    if (bad_size(B, A) || bad_slabs(B) || !ubar || !a || !mu || !sigma || !dmu || !dmu_out || !dsigma || !partials) return -1;
    return colsum_pass(B, A, SeedBackward{ubar, a, mu, sigma, dmu, dmu_out}, dsigma, partials, (hipStream_t)stream);
}
