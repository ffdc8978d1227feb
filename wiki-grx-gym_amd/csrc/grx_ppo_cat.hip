// grx_ppo_cat.hip -- constraints as terminations (include/grx_ppo_cat.h, grx_cat_step and grx_cat_returns; rl/constraints.py).
// grx_cat_step, three launches in stream order:
//   violations : a block of 256 lanes owns CAT_ENVS = 16 consecutive envs, i.e. one contiguous run of 16 C floats of the [N][C] scratch.  A
//                lane walks that run with stride 256: neighbouring lanes hold neighbouring columns of one env, and the scratch is written as
//                one contiguous run whatever C is.  A source is read through its own (env, column) strides: row-major rows come in as one
//                contiguous piece per env, the env's SoA views (strides (1, N)) as one 64-byte piece per column.  The same values go to an
//                LDS slab [16][C]; behind one barrier lane c folds column c over the 16 envs (the block's column maximum) and lane
//                (e, f) ORs family f's columns of env e into one flag; behind a second one lane f adds the 16 flags.
//   merge      : ONE block: lane c folds the blocks' maxima of column c and applies the running update, lane f adds the blocks' counts.
//   apply      : a block is ONE wave of 64 envs.  Lane = env: the row's C ratios against c_max (read by every lane at the same address),
//                delta, the reward in place.  Then the wave copies its envs' action rows to prev as one contiguous run, zero where done.
// max over fp32 and integer sums are exact in any order; every other step is one correctly rounded fp32 operation, uncontracted.
// No atomics, no scratch.  LDS: violations 16 C floats + 16 F ints (static, at most 16.5 KB); merge and apply none.
// grx_cat_returns is grx_ppo_gae.hip's three launches without a state and with alive = (1 - done)(1 - term_prob): the same operations in
// the same order, so that term_prob == 0 gives grx_gae_returns' bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grx_ppo.h"

namespace {

constexpr int CAT_ENVS = 16;                    // envs per block of the violations launch
constexpr int CAT_THREADS = 256;                // its lanes; >= GRX_CAT_MAX_COLUMNS and >= CAT_ENVS * GRX_CAT_MAX_FAMILIES
constexpr int CAT_APPLY = 64;                   // envs per block of the apply launch = lanes of its one wave
constexpr long long CAT_MAX_ROWS = 1ll << 24;
static_assert(CAT_THREADS >= GRX_CAT_MAX_COLUMNS && CAT_THREADS >= CAT_ENVS * GRX_CAT_MAX_FAMILIES, "one lane per column, one per (env, family)");

struct Strided {   // a source [N][W] as the caller holds it: element (n, j) at p[n * env + j * col]
    const float* p;
    long long env, col;
    __device__ inline float at(size_t n, int j) const { return p[n * (size_t)env + (size_t)j * (size_t)col]; }
};

struct Sources {
    Strided torques, dof_vel, dof_pos, actions, gravity;
    const float* prev;   // [N][A] contiguous
};

__global__ __launch_bounds__(CAT_THREADS) void cat_violations_kernel(int N, int C, int F, int D, int A, const int* __restrict__ col_kind,
                                                                     const int* __restrict__ col_src, const int* __restrict__ col_family,
                                                                     const float* __restrict__ col_lo, const float* __restrict__ col_hi,
                                                                     Sources s, const unsigned char* __restrict__ dones,
                                                                     float* __restrict__ cplus, float* __restrict__ part_max,
                                                                     int* __restrict__ part_count) {
#pragma clang fp contract(off) reassociate(off)
    __shared__ float slab[CAT_ENVS * GRX_CAT_MAX_COLUMNS];
    __shared__ int flags[CAT_ENVS * GRX_CAT_MAX_FAMILIES];
    const int n0 = blockIdx.x * CAT_ENVS;
    const int envs = N - n0 < CAT_ENVS ? N - n0 : CAT_ENVS;   // (>= 1: the grid has ceil(N / 16) blocks)
    const int run = envs * C;
    for (int i = threadIdx.x; i < run; i += CAT_THREADS) {
        const int e = i / C, c = i - e * C;
        const size_t n = (size_t)(n0 + e);
        const int kind = col_kind[c], j = col_src[c];
        const float lo = col_lo[c], hi = col_hi[c];
        float v = 0.f;
        if (kind == GRX_CAT_TORQUE) {
            if (j >= 0 && j < D) v = fabsf(s.torques.at(n, j)) - hi;
        } else if (kind == GRX_CAT_DOF_VEL) {
            if (j >= 0 && j < D) v = fabsf(s.dof_vel.at(n, j)) - hi;
        } else if (kind == GRX_CAT_DOF_POS) {
            if (j >= 0 && j < D) {
                const float q = s.dof_pos.at(n, j);
                const float below = lo - q, above = q - hi;
                v = below > above ? below : above;   // (torch.maximum of two finite numbers; a NaN compares false and ends as c+ = 0 below)
            }
        } else if (kind == GRX_CAT_ACTION_RATE) {
            if (j >= 0 && j < A) v = fabsf(s.actions.at(n, j) - s.prev[n * A + j]) - hi;
        } else if (kind == GRX_CAT_UPRIGHT) {
            const float gx = s.gravity.at(n, 0), gy = s.gravity.at(n, 1);
            const float xx = gx * gx, yy = gy * gy;
            v = sqrtf(xx + yy) - hi;
        }
        float p = v > 0.f ? v : 0.f;
        if (dones[n]) p = 0.f;
        cplus[(size_t)n0 * C + i] = p;
        slab[i] = p;
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < C) {
        float m = 0.f;   // (c+ >= 0)
        for (int e = 0; e < envs; ++e) {
            const float x = slab[e * C + t];
            m = x > m ? x : m;
        }
        part_max[(size_t)blockIdx.x * C + t] = m;
    }
    if (t < CAT_ENVS * F) {
        const int e = t / F, f = t - e * F;
        int any = 0;
        if (e < envs)
            for (int c = 0; c < C; ++c) any |= (col_family[c] == f && slab[e * C + c] > 0.f) ? 1 : 0;
        flags[t] = any;
    }
    __syncthreads();
    if (t < F) {
        int k = 0;
        for (int e = 0; e < CAT_ENVS; ++e) k += flags[e * F + t];
        part_count[(size_t)blockIdx.x * F + t] = k;
    }
}

// ONE block.  The only writer of c_max and counts.
__global__ __launch_bounds__(CAT_THREADS) void cat_merge_kernel(int nb, int C, int F, const float* __restrict__ part_max,
                                                                const int* __restrict__ part_count, float tau, float one_minus_tau,
                                                                int reset_counts, float* __restrict__ c_max, int* __restrict__ counts) {
#pragma clang fp contract(off) reassociate(off)
    const int t = threadIdx.x;
    if (t < C) {
        float m = 0.f;
        for (int b = 0; b < nb; ++b) {
            const float x = part_max[(size_t)b * C + t];
            m = x > m ? x : m;
        }
        const float keep = tau * c_max[t], add = one_minus_tau * m;
        c_max[t] = keep + add;
    }
    if (t < F) {
        int k = reset_counts ? 0 : counts[t];
        for (int b = 0; b < nb; ++b) k += part_count[(size_t)b * F + t];
        counts[t] = k;
    }
}

__global__ __launch_bounds__(CAT_APPLY) void cat_apply_kernel(int N, int C, int A, const float* __restrict__ cplus, const float* __restrict__ c_max,
                                                              const float* __restrict__ col_prob, const unsigned char* __restrict__ dones,
                                                              Strided actions, int clip_zero, float* __restrict__ prev,
                                                              float* __restrict__ term_prob_row, float* __restrict__ reward_row) {
#pragma clang fp contract(off) reassociate(off)
    const int n0 = blockIdx.x * CAT_APPLY;
    const int n = n0 + threadIdx.x;
    if (n < N) {
        const float* row = cplus + (size_t)n * C;
        float delta = 0.f;
        for (int c = 0; c < C; ++c) {
            const float cm = c_max[c];
            if (cm > 0.f) {   // (c_max = 0: the column was never violated and contributes 0 -- no division)
                float r = row[c] / cm;
                r = r > 1.f ? 1.f : r;   // (c+ >= 0 and c_max > 0: the ratio is in [0, inf])
                const float term = col_prob[c] * r;
                delta = term > delta ? term : delta;
            }
        }
        term_prob_row[n] = delta;
        float r = reward_row[n];
        if (clip_zero) r = r < 0.f ? 0.f : r;
        reward_row[n] = (1.0f - delta) * r;
    }
    if (prev != nullptr) {   // the wave's envs' action rows as one contiguous run
        const int envs = N - n0 < CAT_APPLY ? N - n0 : CAT_APPLY;
        const size_t base = (size_t)n0 * A;
        for (int i = threadIdx.x; i < envs * A; i += CAT_APPLY) {
            const int e = i / A;
            prev[base + i] = dones[n0 + e] ? 0.f : actions.at((size_t)(n0 + e), i - e * A);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- the returns
// (grx_ppo_gae.hip's triples, operation for operation: its anonymous namespace is not visible here)
constexpr int GAE_ENVS = 64;

struct Triple {
    double n, m, M2;
};

__device__ inline void push(Triple& t, double inv_n, float x) {
    const double d = (double)x - t.m;
    t.n += 1.0;
    t.m += d * inv_n;
    t.M2 += d * ((double)x - t.m);
}

__device__ inline void chan(Triple& a, const Triple& b) {
    const double nab = a.n + b.n;
    if (b.n > 0.0) {
        const double d = b.m - a.m;
        a.m += d * (b.n / nab);
        a.M2 += b.M2 + d * d * (a.n * b.n / nab);
        a.n = nab;
    }
}

__device__ inline Triple wave_merge(Triple t) {
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

__global__ __launch_bounds__(GAE_ENVS) void cat_scan_kernel(int T, int N, const float* __restrict__ rewards, const float* __restrict__ values,
                                                            const unsigned char* __restrict__ dones, const float* __restrict__ term_prob,
                                                            const float* __restrict__ last_values, float gamma, float lam,
                                                            float* __restrict__ returns, float* __restrict__ raw_adv, double* __restrict__ partials) {
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
            const float not_done = 1.0f - (float)dones[i], survives = 1.0f - term_prob[i];
            const float alive = not_done * survives;
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
    if (threadIdx.x == 0) {
        double* p = partials + (size_t)blockIdx.x * 6;
        p[0] = ta.n; p[1] = ta.m; p[2] = ta.M2;
        p[3] = tr.n; p[4] = tr.m; p[5] = tr.M2;
    }
}

// ONE block, two threads: thread 0 the advantages' moments, thread 1 the returns'
__global__ __launch_bounds__(64) void cat_moments_kernel(int nb, const double* __restrict__ partials, float* __restrict__ stats) {
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
    stats[2] = (float)t.m;
    stats[3] = (float)(t.M2 / t.n);
}

__global__ __launch_bounds__(256) void cat_normalise_kernel(int total, const float* __restrict__ stats, float* __restrict__ advantages) {
#pragma clang fp contract(off) reassociate(off)
    const float ma = stats[0], sa = stats[1] + 1e-8f;
    const int step = gridDim.x * 256;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += step) advantages[i] = (advantages[i] - ma) / sa;
}

struct Span {
    const void* p;
    size_t bytes;
};

inline bool overlap(const Span& a, const Span& b) {
    if (!a.p || !b.p || !a.bytes || !b.bytes) return false;
    const uintptr_t x = (uintptr_t)a.p, y = (uintptr_t)b.p;
    return x < y + b.bytes && y < x + a.bytes;
}

inline bool clash(const Span* in, int n_in, const Span* out, int n_out) {   // an output on an input or on another output
    for (int o = 0; o < n_out; ++o) {
        for (int i = 0; i < n_in; ++i)
            if (overlap(out[o], in[i])) return true;
        for (int q = o + 1; q < n_out; ++q)
            if (overlap(out[o], out[q])) return true;
    }
    return false;
}

inline int step_blocks(int N) { return (N + CAT_ENVS - 1) / CAT_ENVS; }
inline int gae_blocks(int N) { return (N + GAE_ENVS - 1) / GAE_ENVS; }
inline bool bad_rollout(int T, int N) { return T < 1 || N < 1 || (long long)T * N > CAT_MAX_ROWS; }

}  // namespace

extern "C" int grx_cat_step_blocks(int N) { return (N < 1 || N > CAT_MAX_ROWS) ? 0 : step_blocks(N); }

extern "C" int grx_cat_step(int N, int C, int F, int D, int A, int kinds, const int* col_kind, const int* col_src, const int* col_family,
                            const float* col_lo, const float* col_hi, const float* col_prob, const float* torques, const float* dof_vel,
                            const float* dof_pos, const float* actions, const float* gravity, const long long* src_strides,
                            const unsigned char* dones, float tau,
                            float one_minus_tau, int clip_zero, int reset_counts, float* prev, float* c_max, int* counts, float* cplus,
                            float* part_max, int* part_count, float* term_prob_row, float* reward_row, void* stream) {
    if (N < 1 || N > CAT_MAX_ROWS || C < 1 || C > GRX_CAT_MAX_COLUMNS || F < 1 || F > GRX_CAT_MAX_FAMILIES) return -1;
    if (!col_kind || !col_src || !col_family || !col_lo || !col_hi || !col_prob || !dones || !c_max || !counts || !cplus || !part_max ||
        !part_count || !term_prob_row || !reward_row)
        return -1;
    if (kinds <= 0 || kinds >= (1 << GRX_CAT_NUM_KINDS)) return -1;
    const bool dof = kinds & ((1 << GRX_CAT_TORQUE) | (1 << GRX_CAT_DOF_VEL) | (1 << GRX_CAT_DOF_POS));
    const bool rate = kinds & (1 << GRX_CAT_ACTION_RATE);
    if (dof && D < 1) return -1;
    if ((kinds & (1 << GRX_CAT_TORQUE)) && !torques) return -1;
    if ((kinds & (1 << GRX_CAT_DOF_VEL)) && !dof_vel) return -1;
    if ((kinds & (1 << GRX_CAT_DOF_POS)) && !dof_pos) return -1;
    if (rate && (A < 1 || !actions || !prev)) return -1;
    if (!rate && prev && (A < 1 || !actions)) return -1;
    if ((kinds & (1 << GRX_CAT_UPRIGHT)) && !gravity) return -1;
    const int nb = step_blocks(N);
    const int widths[5] = {D, D, D, A, 3};
    long long sd[5][2];   // element strides (env, column): the caller's, or those of contiguous rows
    size_t span[5];       // bytes from a source's first element to behind its last
    for (int k = 0; k < 5; ++k) {
        sd[k][0] = src_strides ? src_strides[2 * k] : widths[k];
        sd[k][1] = src_strides ? src_strides[2 * k + 1] : 1;
        if ((kinds & (1 << k)) && (sd[k][0] < 0 || sd[k][1] < 0 || sd[k][0] > (1ll << 40) || sd[k][1] > (1ll << 40))) return -1;
        span[k] = widths[k] > 0 ? ((size_t)(N - 1) * (size_t)sd[k][0] + (size_t)(widths[k] - 1) * (size_t)sd[k][1] + 1) * sizeof(float) : 0;
    }
    const size_t cf = (size_t)C * sizeof(float), na = (size_t)N * (A > 0 ? A : 0) * sizeof(float);
    const Span in[12] = {{col_kind, (size_t)C * sizeof(int)}, {col_src, (size_t)C * sizeof(int)}, {col_family, (size_t)C * sizeof(int)},
                         {col_lo, cf}, {col_hi, cf}, {col_prob, cf}, {torques, span[0]}, {dof_vel, span[1]}, {dof_pos, span[2]},
                         {actions, span[3]}, {gravity, span[4]}, {dones, (size_t)N}};
    const Span out[8] = {{prev, na}, {c_max, cf}, {counts, (size_t)F * sizeof(int)}, {cplus, (size_t)N * cf}, {part_max, (size_t)nb * cf},
                         {part_count, (size_t)nb * F * sizeof(int)}, {term_prob_row, (size_t)N * sizeof(float)},
                         {reward_row, (size_t)N * sizeof(float)}};
    if (clash(in, 12, out, 8)) return -1;
    hipStream_t st = (hipStream_t)stream;
    const Sources s = {{torques, sd[0][0], sd[0][1]}, {dof_vel, sd[1][0], sd[1][1]}, {dof_pos, sd[2][0], sd[2][1]},
                       {actions, sd[3][0], sd[3][1]}, {gravity, sd[4][0], sd[4][1]}, prev};
    hipLaunchKernelGGL(cat_violations_kernel, dim3(nb), dim3(CAT_THREADS), 0, st, N, C, F, D, A, col_kind, col_src, col_family, col_lo, col_hi, s,
                       dones, cplus, part_max, part_count);
    if (hipGetLastError() != hipSuccess) return -2;
    hipLaunchKernelGGL(cat_merge_kernel, dim3(1), dim3(CAT_THREADS), 0, st, nb, C, F, (const float*)part_max, (const int*)part_count, tau,
                       one_minus_tau, reset_counts, c_max, counts);
    if (hipGetLastError() != hipSuccess) return -3;
    hipLaunchKernelGGL(cat_apply_kernel, dim3((N + CAT_APPLY - 1) / CAT_APPLY), dim3(CAT_APPLY), 0, st, N, C, A, (const float*)cplus,
                       (const float*)c_max, col_prob, dones, s.actions, clip_zero, prev, term_prob_row, reward_row);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

extern "C" int grx_cat_partials_size(int T, int N) { return bad_rollout(T, N) ? 0 : gae_blocks(N) * 12; }

extern "C" int grx_cat_returns(int T, int N, const float* rewards, const float* values, const unsigned char* dones, const float* term_prob,
                               const float* last_values, float gamma, float lam, float* returns, float* advantages, float* stats,
                               float* partials, void* stream) {
    if (bad_rollout(T, N)) return -1;
    if (!rewards || !values || !dones || !term_prob || !last_values || !returns || !advantages || !stats || !partials) return -1;
    if ((uintptr_t)partials & 7) return -1;
    const size_t total = (size_t)T * N, fb = total * sizeof(float);
    const int nb = gae_blocks(N);
    const Span in[5] = {{rewards, fb}, {values, fb}, {dones, total}, {term_prob, fb}, {last_values, (size_t)N * sizeof(float)}};
    const Span out[4] = {{returns, fb}, {advantages, fb}, {stats, 4 * sizeof(float)}, {partials, (size_t)nb * 12 * sizeof(float)}};
    if (clash(in, 5, out, 4)) return -1;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cat_scan_kernel, dim3(nb), dim3(GAE_ENVS), 0, st, T, N, rewards, values, dones, term_prob, last_values, gamma, lam,
                       returns, advantages, (double*)partials);
    if (hipGetLastError() != hipSuccess) return -2;
    hipLaunchKernelGGL(cat_moments_kernel, dim3(1), dim3(64), 0, st, nb, (const double*)partials, stats);
    if (hipGetLastError() != hipSuccess) return -3;
    const int blocks = (int)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024);
    hipLaunchKernelGGL(cat_normalise_kernel, dim3(blocks), dim3(256), 0, st, (int)total, (const float*)stats, advantages);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}
