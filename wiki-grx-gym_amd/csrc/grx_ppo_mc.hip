// grx_ppo_mc.hip -- multi-critic PPO: a value head, a GAE pass and a value loss per group of reward terms (include/grx_ppo_mc.h,
// rl/multi_critic.py).  Nothing here is shared with grx_ppo.hip / grx_ppo_gae.hip: what is needed of them is restated, so
// their code objects are what they were.
//   grx_mc_store   : ONE launch per rollout step, one lane per (env, group): the lane adds the terms of its group in table order (a wave
//                    reads 64 / K consecutive floats of a term's row, every lane of an env the same one), bootstraps its head on a
//                    time-out and writes the two storage rows [N][K] as one contiguous run.
//   grx_mc_returns : THREE launches, the shape of grx_gae_returns.  scan: a block is 64 envs x K groups = K waves, thread j = env j / K,
//                    group j % K, so a step's [64][K] slab is read as 64 K consecutive floats; each lane keeps grx_gae_returns' recursion
//                    and Welford triple (float64) of ITS column; the triples go through LDS once ([K][64]), wave k then merges group k's
//                    64 down grx_gae_returns' shuffle tree -- with K = 1 the block IS that kernel's block, bit for bit.  merge: one block,
//                    thread k merges group k's per-block triples in block order.  apply: element-wise over T N.
//   grx_mc_loss    : grx_ppo_loss with K value columns; per-block partials in float64, added in block order.
// No atomics, no scratch memory; the scan uses 12 KB of LDS, the loss 1.3 KB + 32 KB in its one-block finalize.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/grx_ppo.h"

namespace {

constexpr int MC_MAXK = GRX_MC_MAX_GROUPS;
constexpr int MC_ENVS = 64;                      // envs per scan block
constexpr long long MC_MAX_ROWS = 1ll << 24;     // as grx_gae_returns: a triple's n is exact as a float up to here
constexpr int MC_MAX_TERMS = 256;                // NT + NB of a store call

struct Triple {
    double n, m, M2;
};

__device__ inline void push(Triple& t, double inv_n, float x) {   // Welford; inv_n = 1 / (t.n + 1)
    const double d = (double)x - t.m;
    t.n += 1.0;
    t.m += d * inv_n;
    t.M2 += d * ((double)x - t.m);
}

__device__ inline void chan(Triple& a, const Triple& b) {   // a <- a merged with b; an empty b changes nothing
    const double nab = a.n + b.n;
    if (b.n > 0.0) {
        const double d = b.m - a.m;
        a.m += d * (b.n / nab);
        a.M2 += b.M2 + d * d * (a.n * b.n / nab);
        a.n = nab;
    }
}

__device__ inline Triple wave_merge(Triple t) {   // lane 0 holds the 64 lanes' triple
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

// ---- grx_mc_store --------------------------------------------------------------------------------------------------------------------
// (a map entry outside -1 .. K-1 is seen by the device alone: every thread reads the whole map first and the launch writes nothing)
__global__ __launch_bounds__(256) void mc_store_kernel(int N, int K, int NT, int NB, const float* __restrict__ terms,
                                                        const float* __restrict__ base_terms, const int* __restrict__ map,
                                                        const float* __restrict__ values, const unsigned char* __restrict__ time_outs,
                                                        float gamma, float* __restrict__ st_values, float* __restrict__ st_rewards) {
#pragma clang fp contract(off) reassociate(off)
    const int nmap = NT + (base_terms ? NB : 0);
    bool ok = true;
    for (int t = 0; t < nmap; ++t) ok = ok && map[t] >= -1 && map[t] < K;
    if (!ok) return;
    const int total = N * K, step = gridDim.x * 256;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
        const int n = i / K, k = i - n * K;
        float r = 0.f;
        for (int t = 0; t < NT; ++t) {
            if (map[t] < 0) continue;   // (uniform: an inactive term's row is not read)
            const float x = terms[(size_t)t * N + n];
            if (map[t] == k) r = r + x;
        }
        if (base_terms)
            for (int t = 0; t < NB; ++t) {
                if (map[NT + t] < 0) continue;
                const float x = base_terms[(size_t)t * N + n];
                if (map[NT + t] == k) r = r + x;
            }
        const float v = values[i];
        const bool to = time_outs && time_outs[n] != 0;
        st_values[i] = v;
        st_rewards[i] = r + (to ? gamma * v : 0.0f);   // rewards + gamma * values * time_outs, per head
    }
}

// ---- grx_mc_returns ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MC_ENVS * MC_MAXK) void mc_scan_kernel(int T, int N, int K, const float* __restrict__ rewards,
                                                                     const float* __restrict__ values, const unsigned char* __restrict__ dones,
                                                                     const float* __restrict__ last_values, float gamma, float lam,
                                                                     float* __restrict__ returns, double* __restrict__ partials) {
#pragma clang fp contract(off) reassociate(off)
    __shared__ double s_t[MC_MAXK][MC_ENVS][3];
    const int j = threadIdx.x;             // < 64 K
    const int e = j / K, k = j - e * K;
    const int n = blockIdx.x * MC_ENVS + e;
    Triple ta = {0.0, 0.0, 0.0};
    if (n < N) {
        const size_t col = (size_t)n * K + k, row = (size_t)N * K;
        float next = last_values[col], adv = 0.f;
        double cnt = 0.0;
#pragma unroll 4
        for (int t = T - 1; t >= 0; --t) {
            const size_t i = (size_t)t * row + col;
            const float r = rewards[i], v = values[i];
            const float alive = 1.0f - (float)dones[(size_t)t * N + n];
            const float ag = alive * gamma;
            const float delta = (r + ag * next) - v;
            adv = delta + (ag * lam) * adv;
            const float ret = adv + v;
            const float a = ret - v;
            returns[i] = ret;
            next = v;
            cnt += 1.0;
            push(ta, 1.0 / cnt, a);
        }
    }
    s_t[k][e][0] = ta.n; s_t[k][e][1] = ta.m; s_t[k][e][2] = ta.M2;
    __syncthreads();
    const int w = j >> 6, lane = j & 63;   // wave w merges group w's 64 envs
    Triple tm = {s_t[w][lane][0], s_t[w][lane][1], s_t[w][lane][2]};
    tm = wave_merge(tm);
    if (lane == 0) {
        double* p = partials + ((size_t)blockIdx.x * K + w) * 3;
        p[0] = tm.n; p[1] = tm.m; p[2] = tm.M2;
    }
}

__global__ __launch_bounds__(64) void mc_merge_kernel(int nb, int K, const double* __restrict__ partials, float* __restrict__ stats) {
#pragma clang fp contract(off) reassociate(off)
    const int k = threadIdx.x;
    if (k >= K) return;
    const double* p = partials + (size_t)k * 3;
    Triple t = {p[0], p[1], p[2]};
    for (int b = 1; b < nb; ++b) {
        const double* q = p + (size_t)b * K * 3;
        const Triple o = {q[0], q[1], q[2]};
        chan(t, o);
    }
    stats[2 * k] = (float)t.m;
    stats[2 * k + 1] = (float)sqrt(t.M2 / (t.n - 1.0));   // (T N = 1: 0 / 0, NaN as torch.std)
}

struct McWeights {
    float w[MC_MAXK];
};

__global__ __launch_bounds__(256) void mc_apply_kernel(int total, int K, const float* __restrict__ stats, McWeights wts,
                                                        const float* __restrict__ values, const float* __restrict__ returns,
                                                        float* __restrict__ advantages) {
#pragma clang fp contract(off) reassociate(off)
    float ma[MC_MAXK], sa[MC_MAXK];
#pragma unroll
    for (int k = 0; k < MC_MAXK; ++k) {
        ma[k] = k < K ? stats[2 * k] : 0.f;
        sa[k] = k < K ? stats[2 * k + 1] + 1e-8f : 1.f;
    }
    const int step = gridDim.x * 256;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
        float adv = 0.f;
#pragma unroll
        for (int k = 0; k < MC_MAXK; ++k)
            if (k < K) {
                const size_t c = (size_t)i * K + k;
                const float a = returns[c] - values[c];   // (the scan's a = ret - v again: the same operation on the same floats)
                adv = adv + wts.w[k] * ((a - ma[k]) / sa[k]);
            }
        advantages[i] = adv;
    }
}

// ---- grx_mc_loss ---------------------------------------------------------------------------------------------------------------------
constexpr int MAXA = 32;
constexpr int NTHR = 256;
constexpr int MC_NRED = 2 + MC_MAXK + MAXA;   // surrogate, KL, value loss[MC_MAXK], d_std[MAXA]

// (grx_ppo.hip: torch.max / torch.clamp PROPAGATE NaN, fmaxf / fminf drop it)
__device__ inline float nmax(float a, float b) { return (a > b || a != a) ? a : b; }
__device__ inline float nmin(float a, float b) { return (a < b || a != a) ? a : b; }

__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

template <int A>
__global__ __launch_bounds__(NTHR) void mc_loss_kernel(int B, int K, const float* __restrict__ mu, const float* __restrict__ stdp,
                                                        const float* __restrict__ value, const float* __restrict__ actions,
                                                        const float* __restrict__ old_logp, const float* __restrict__ old_mu,
                                                        const float* __restrict__ old_sigma, const float* __restrict__ adv_,
                                                        const float* __restrict__ ret_, const float* __restrict__ tv_,
                                                        float clip, float vcoef, int use_clipped,
                                                        float* __restrict__ d_mu, float* __restrict__ d_value, double* __restrict__ partials) {
    const int i = blockIdx.x * NTHR + threadIdx.x;
    float red[2 + A], redv[MC_MAXK];
#pragma unroll
    for (int k = 0; k < 2 + A; ++k) red[k] = 0.f;
#pragma unroll
    for (int k = 0; k < MC_MAXK; ++k) redv[k] = 0.f;
    if (i < B) {
        const float invB = 1.0f / (float)B;
        float sg[A], df[A];
        float logp = 0.f, kl = 0.f;
#pragma unroll
        for (int k = 0; k < A; ++k) {
            const float s = stdp[k], m = mu[(size_t)i * A + k];
            sg[k] = s;
            df[k] = actions[(size_t)i * A + k] - m;
            logp += -(df[k] * df[k]) / (2.0f * s * s) - logf(s) - 0.9189385332046727f;
            const float os = old_sigma[(size_t)i * A + k], dm = old_mu[(size_t)i * A + k] - m;
            kl += logf(s / os + 1.e-5f) + (os * os + dm * dm) / (2.0f * s * s) - 0.5f;
        }
        const float adv = adv_[i];
        const float ratio = expf(logp - old_logp[i]);
        const float lo = 1.0f - clip, hi = 1.0f + clip;
        const float rc = nmin(nmax(ratio, lo), hi);
        const float s1 = -adv * ratio, s2 = -adv * rc;
        const float surr = nmax(s1, s2);
        const float w1 = s1 > s2 ? 1.f : (s1 == s2 ? 0.5f : 0.f), w2 = 1.f - w1;
        const float in_range = (ratio >= lo && ratio <= hi) ? 1.f : 0.f;
        const float g_ratio = -adv * (w1 + w2 * in_range);
        const float g_logp = g_ratio * ratio * invB;
#pragma unroll
        for (int k = 0; k < A; ++k) {
            const float s = sg[k], inv2 = 1.0f / (s * s);
            // (grx_ppo.hip: `np` is torch's chain to sigma times 0 -- +-0 where it is finite, NaN where it is not)
            const float half = 0.5f * inv2;
            const float np = 0.f * (g_logp * (((df[k] * df[k] * half) * half) * 2.0f * (2.0f * s)) - g_logp / s);
            d_mu[(size_t)i * A + k] = g_logp * df[k] * inv2 + np;
            red[2 + k] = g_logp * (df[k] * df[k] * inv2 / s - 1.0f / s) + np;
        }
#pragma unroll
        for (int h = 0; h < MC_MAXK; ++h)
            if (h < K) {
                const size_t c = (size_t)i * K + h;
                const float v = value[c], ret = ret_[c];
                float vl, gv;
                if (use_clipped) {
                    const float tv = tv_[c];
                    const float dv = v - tv;
                    const float vc = tv + nmin(nmax(dv, -clip), clip);
                    const float l1 = (v - ret) * (v - ret), l2 = (vc - ret) * (vc - ret);
                    vl = nmax(l1, l2);
                    const float u1 = l1 > l2 ? 1.f : (l1 == l2 ? 0.5f : 0.f), u2 = 1.f - u1;
                    const float vin = (dv >= -clip && dv <= clip) ? 1.f : 0.f;
                    gv = u1 * 2.0f * (v - ret) + (vin != 0.f ? u2 * 2.0f * (vc - ret) : 0.f);
                } else {
                    vl = (ret - v) * (ret - v);
                    gv = -2.0f * (ret - v);
                }
                d_value[c] = vcoef * gv * invB;
                redv[h] = vl;
            }
        red[0] = surr; red[1] = kl;
    }
    __shared__ double s_red[NTHR / 64][MC_NRED];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double t = wave_sum((double)red[k]);
        if (lane == 0) s_red[wv][k] = t;
    }
#pragma unroll
    for (int k = 0; k < MC_MAXK; ++k) {
        const double t = wave_sum((double)redv[k]);
        if (lane == 0) s_red[wv][2 + k] = t;
    }
#pragma unroll
    for (int k = 0; k < A; ++k) {
        const double t = wave_sum((double)red[2 + k]);
        if (lane == 0) s_red[wv][2 + MC_MAXK + k] = t;
    }
    __syncthreads();
    if (threadIdx.x < 2 + MC_MAXK + A) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < NTHR / 64; ++w) t += s_red[w][threadIdx.x];
        partials[(size_t)blockIdx.x * MC_NRED + threadIdx.x] = t;
    }
}

__global__ __launch_bounds__(64) void mc_loss_finalize(int B, int A, int K, int nblk, const double* __restrict__ partials,
                                                        const float* __restrict__ stdp, float vcoef, float ecoef,
                                                        float* __restrict__ out, float* __restrict__ d_std) {
    const int k = threadIdx.x;
    double t = 0.0;
    constexpr int STAGE = 4096;   // doubles: fetched in parallel, added from LDS in the SAME (block) order
    __shared__ double s_p[STAGE];
    const bool staged = nblk * MC_NRED <= STAGE;
    if (staged) {
        for (int i = k; i < nblk * MC_NRED; i += 64) s_p[i] = partials[i];
        __syncthreads();
    }
    if (k < 2 + MC_MAXK + A)
        for (int b = 0; b < nblk; ++b) t += staged ? s_p[b * MC_NRED + k] : partials[(size_t)b * MC_NRED + k];
    __shared__ double s_t[64];
    s_t[k] = t;   // MC_NRED <= 64
    __syncthreads();
    if (k >= 2 + MC_MAXK && k < 2 + MC_MAXK + A) d_std[k - 2 - MC_MAXK] = (float)t - ecoef / stdp[k - 2 - MC_MAXK];
    if (k >= 2 && k < 2 + K) out[4 + (k - 2)] = (float)(t / (double)B);   // the heads' own value losses
    if (k == 0) {
        double vsum = 0.0;   // the value loss is the sum over the heads, in head order
        for (int h = 0; h < K; ++h) vsum += s_t[2 + h];
        const float surr = (float)(s_t[0] / (double)B), vl = (float)(vsum / (double)B), klm = (float)(s_t[1] / (double)B);
        float ent = 0.f;
        for (int a = 0; a < A; ++a) ent += 1.4189385332046727f + logf(stdp[a]);
        out[0] = surr; out[1] = vl; out[2] = surr + vcoef * vl - ecoef * ent; out[3] = klm;
    }
}

template <int A>
void launch_loss(int nblk, hipStream_t st, int B, int K, const float* mu, const float* stdp, const float* value, const float* actions,
                 const float* old_logp, const float* old_mu, const float* old_sigma, const float* adv, const float* ret, const float* tv,
                 float clip, float vcoef, int use_clipped, float* d_mu, float* d_value, double* partials) {
    hipLaunchKernelGGL(mc_loss_kernel<A>, dim3(nblk), dim3(NTHR), 0, st, B, K, mu, stdp, value, actions, old_logp, old_mu, old_sigma,
                       adv, ret, tv, clip, vcoef, use_clipped, d_mu, d_value, partials);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
struct Span {
    const void* p;
    size_t bytes;
};
inline bool overlap(const Span& a, const Span& b) {
    const uintptr_t x = (uintptr_t)a.p, y = (uintptr_t)b.p;
    return a.p && b.p && x < y + b.bytes && y < x + a.bytes;
}
// true when an output overlaps an input or another output
inline bool clash(const Span* in, int n_in, const Span* out, int n_out) {
    for (int o = 0; o < n_out; ++o) {
        for (int i = 0; i < n_in; ++i)
            if (overlap(out[o], in[i])) return true;
        for (int q = o + 1; q < n_out; ++q)
            if (overlap(out[o], out[q])) return true;
    }
    return false;
}
inline int scan_blocks(int N) { return (N + MC_ENVS - 1) / MC_ENVS; }
inline bool bad_groups(int K) { return K < 1 || K > MC_MAXK; }
inline bool bad_shape(int T, int N, int K) { return T < 1 || N < 1 || bad_groups(K) || (long long)T * N > MC_MAX_ROWS; }

}  // namespace

extern "C" int grx_mc_store(int N, int K, int NT, int NB, const float* terms, const float* base_terms, const int* term_group,
                            const float* values, const unsigned char* time_outs, float gamma, float* st_values, float* st_rewards,
                            void* stream) {
    if (N < 1 || bad_groups(K) || NT < 1 || NB < 0 || (base_terms && NB < 1) || NT + NB > MC_MAX_TERMS) return -1;
    if ((long long)N * K > (1ll << 30)) return -1;
    if (!terms || !term_group || !values || !st_values || !st_rewards) return -1;
    const size_t nk = (size_t)N * K * sizeof(float);
    const Span in[5] = {{terms, (size_t)NT * N * sizeof(float)}, {base_terms, (size_t)NB * N * sizeof(float)},
                        {term_group, (size_t)(NT + (base_terms ? NB : 0)) * sizeof(int)}, {values, nk}, {time_outs, (size_t)N}};
    const Span out[2] = {{st_values, nk}, {st_rewards, nk}};
    if (clash(in, 5, out, 2)) return -1;
    int blocks = (int)(((size_t)N * K + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(mc_store_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, N, K, NT, NB, terms, base_terms, term_group, values,
                       time_outs, gamma, st_values, st_rewards);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// in floats (the buffer holds doubles: one triple per block and group; the caller's allocation must be 8-byte aligned)
extern "C" int grx_mc_partials_size(int T, int N, int K) { return bad_shape(T, N, K) ? 0 : scan_blocks(N) * K * 6; }

extern "C" int grx_mc_returns(int T, int N, int K, const float* rewards, const float* values, const unsigned char* dones,
                              const float* last_values, const float* weights, float gamma, float lam, float* returns, float* advantages,
                              float* stats, float* partials, void* stream) {
    if (bad_shape(T, N, K)) return -1;
    if (!rewards || !values || !dones || !last_values || !weights || !returns || !advantages || !stats || !partials) return -1;
    if ((uintptr_t)partials & 7) return -1;
    McWeights wts;
    for (int k = 0; k < MC_MAXK; ++k) {
        wts.w[k] = k < K ? weights[k] : 0.f;
        if (k < K && !(isfinite(weights[k]) && weights[k] > 0.f)) return -1;
    }
    const size_t total = (size_t)T * N, fb = total * K * sizeof(float);
    const int nb = scan_blocks(N);
    const Span in[4] = {{rewards, fb}, {values, fb}, {dones, total}, {last_values, (size_t)N * K * sizeof(float)}};
    const Span out[4] = {{returns, fb}, {advantages, total * sizeof(float)}, {stats, (size_t)K * 2 * sizeof(float)},
                         {partials, (size_t)nb * K * 6 * sizeof(float)}};
    if (clash(in, 4, out, 4)) return -1;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mc_scan_kernel, dim3(nb), dim3(MC_ENVS * K), 0, st, T, N, K, rewards, values, dones, last_values, gamma, lam, returns,
                       (double*)partials);
    if (hipGetLastError() != hipSuccess) return -2;
    hipLaunchKernelGGL(mc_merge_kernel, dim3(1), dim3(64), 0, st, nb, K, (const double*)partials, stats);
    if (hipGetLastError() != hipSuccess) return -3;
    const int blocks = (int)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024);
    hipLaunchKernelGGL(mc_apply_kernel, dim3(blocks), dim3(256), 0, st, (int)total, K, (const float*)stats, wts, values, (const float*)returns,
                       advantages);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

extern "C" int grx_mc_loss_partials_size(int batch) { return batch < 1 ? 0 : ((batch + NTHR - 1) / NTHR) * MC_NRED * 2; }

extern "C" int grx_mc_loss(int batch, int num_actions, int K, const float* mu, const float* std, const float* value, const float* actions,
                           const float* old_logp, const float* old_mu, const float* old_sigma, const float* advantages, const float* returns,
                           const float* target_values, float clip_param, float value_loss_coef, float entropy_coef,
                           int use_clipped_value_loss, float* out, float* d_mu, float* d_std, float* d_value, float* partials, void* stream) {
    if (batch < 1 || num_actions < 1 || num_actions > MAXA || bad_groups(K)) return -1;
    if (!mu || !std || !value || !actions || !old_logp || !old_mu || !old_sigma || !advantages || !returns || !out || !d_mu || !d_std ||
        !d_value || !partials)
        return -1;
    if (use_clipped_value_loss && !target_values) return -1;
    if ((uintptr_t)partials & 7) return -1;
    const int nblk = (batch + NTHR - 1) / NTHR;
    const size_t f = sizeof(float), ba = (size_t)batch * num_actions * f, bk = (size_t)batch * K * f, b1 = (size_t)batch * f;
    const Span in[10] = {{mu, ba}, {std, (size_t)num_actions * f}, {value, bk}, {actions, ba}, {old_logp, b1}, {old_mu, ba}, {old_sigma, ba},
                         {advantages, b1}, {returns, bk}, {target_values, bk}};
    const Span outs[5] = {{out, (size_t)(4 + K) * f}, {d_mu, ba}, {d_std, (size_t)num_actions * f}, {d_value, bk},
                          {partials, (size_t)nblk * MC_NRED * 2 * f}};
    if (clash(in, 10, outs, 5)) return -1;
    hipStream_t st = (hipStream_t)stream;
#define GRX_MC_CASE(A) case A: launch_loss<A>(nblk, st, batch, K, mu, std, value, actions, old_logp, old_mu, old_sigma, advantages, returns, \
                                              target_values, clip_param, value_loss_coef, use_clipped_value_loss, d_mu, d_value, (double*)partials); break;
    switch (num_actions) {
        GRX_MC_CASE(1) GRX_MC_CASE(2) GRX_MC_CASE(3) GRX_MC_CASE(4) GRX_MC_CASE(5) GRX_MC_CASE(6) GRX_MC_CASE(7) GRX_MC_CASE(8)
        GRX_MC_CASE(9) GRX_MC_CASE(10) GRX_MC_CASE(11) GRX_MC_CASE(12) GRX_MC_CASE(13) GRX_MC_CASE(14) GRX_MC_CASE(15) GRX_MC_CASE(16)
        GRX_MC_CASE(17) GRX_MC_CASE(18) GRX_MC_CASE(19) GRX_MC_CASE(20) GRX_MC_CASE(21) GRX_MC_CASE(22) GRX_MC_CASE(23) GRX_MC_CASE(24)
        GRX_MC_CASE(25) GRX_MC_CASE(26) GRX_MC_CASE(27) GRX_MC_CASE(28) GRX_MC_CASE(29) GRX_MC_CASE(30) GRX_MC_CASE(31) GRX_MC_CASE(32)
    }
#undef GRX_MC_CASE
    if (hipGetLastError() != hipSuccess) return -2;
    hipLaunchKernelGGL(mc_loss_finalize, dim3(1), dim3(64), 0, st, batch, num_actions, K, nblk, (const double*)partials, std, value_loss_coef,
                       entropy_coef, out, d_std);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}
