// grx_ppo_beta.hip -- PPO with a Beta action distribution (include/grx_ppo_beta.h, rl/beta.py): the actor's output layer has
// 2A outputs, raw[i] = [p (A) | q (A)], alpha = 1 + softplus(p), beta = 1 + softplus(q), and the action in unit-box coordinates is x ~ Beta.
//   grx_ppo_loss_beta     the minibatch loss of grx_ppo_noise.hip's ppo_loss_sd_kernel term by term with the Beta's log-probability, entropy
//                         and KL in the Gaussian's places, the gradient written straight onto the raw output
//   grx_beta_params       raw -> (alpha, beta)
//   grx_beta_sample       two gamma draws -> x (clamped), the env's action lo + span x, and log p(x)
//   grx_beta_functions    lgamma, digamma and trigamma as the kernels evaluate them (the test hook)
// Every special function is evaluated in double and takes arguments >= 1 only: lnB = lgG(a) + lgG(b) - lgG(a + b) cancels to 1e-6 of its
// terms once a + b reaches the thousands, and so do the psi differences of the gradient; at batch x A ~ 1e5 elements the cost does not
// show.  A translation unit of its own: the other kernels' code objects are what they were.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grx_ppo.h"

#pragma clang fp contract(off)   // strict IEEE: a product and a sum stay two roundings, the one fmaf below is spelled out

namespace {
constexpr int MAXA = 32;
constexpr int NTHR = 256;
constexpr int ROWS = 64;  // rows per block of the loss kernel, whatever A: the partials' count depends on the batch alone
constexpr int NRED = 4;   // surrogate, value loss, KL, entropy
constexpr float X_MIN = 5.9604644775390625e-08f;         // 2^-24
constexpr float X_MAX = 0.999999940395355224609375f;     // 1 - 2^-24

// (grx_ppo.hip: torch.max / torch.clamp PROPAGATE NaN, fmaxf / fminf drop it -- a NaN ratio or value must reach the loss, so that
//  the update's NaN-skip fires)
__device__ inline float nmax(float a, float b) { return (a > b || a != a) ? a : b; }
__device__ inline float nmin(float a, float b) { return (a < b || a != a) ? a : b; }

__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

// the sum over the LPR lanes of a row (LPR a power of two, the group aligned in the wave): a butterfly, so that every lane of the group
// holds the same bits.  Both kernels that sum a row's log-probability go through here
template <int LPR>
__device__ inline double group_sum(double v) {
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// digamma for y >= 1: the upward recurrence psi(y) = psi(y + 1) - 1 / y to an argument >= 10, then the asymptotic series to y^-12
// (the next term, 1 / (12 y^14), is below 1e-15 there)
__device__ inline double digamma_d(double y) {
    if (!(y >= 1.0)) return (double)NAN;   // (also what bounds the recurrence: at most 9 steps)
    double r = 0.0;
    for (int n = 0; n < 9 && y < 10.0; ++n) { r -= 1.0 / y; y += 1.0; }
    const double i = 1.0 / y, i2 = i * i;
    const double ser = i2 * (1.0 / 12.0 - i2 * (1.0 / 120.0 - i2 * (1.0 / 252.0 - i2 * (1.0 / 240.0 - i2 * (1.0 / 132.0 - i2 * (691.0 / 32760.0))))));
    return r + (log(y) - 0.5 * i - ser);
}

// trigamma for y >= 1: psi1(y) = psi1(y + 1) + 1 / y^2 to an argument >= 10, then the asymptotic series to y^-13
__device__ inline double trigamma_d(double y) {
    if (!(y >= 1.0)) return (double)NAN;
    double r = 0.0;
    for (int n = 0; n < 9 && y < 10.0; ++n) { r += 1.0 / (y * y); y += 1.0; }
    const double i = 1.0 / y, i2 = i * i;
    const double ser = i * i2 * (1.0 / 6.0 - i2 * (1.0 / 30.0 - i2 * (1.0 / 42.0 - i2 * (1.0 / 30.0 - i2 * (5.0 / 66.0 - i2 * (691.0 / 2730.0))))));
    return r + (i + 0.5 * i2 + ser);
}

__device__ inline double lgamma_d(double y) { return y >= 1.0 ? lgamma(y) : (double)NAN; }

__device__ inline double lnbeta_d(double a, double b) { return lgamma_d(a) + lgamma_d(b) - lgamma_d(a + b); }

// alpha (or beta) of a raw output: 1 + softplus(p), torch.nn.functional.softplus with its threshold of 20, in fp32 -- what the storage
// holds and what the loss recomputes: the same function, so that the update's first epoch sees KL = 0 exactly
__device__ inline float beta_param(float p) { return 1.0f + (p > 20.0f ? p : log1pf(expf(p))); }
// d softplus / d p as torch's softplus_backward spells it: z / (z + 1) with z = exp(p), 1 above the threshold
__device__ inline float beta_dparam(float p) {
    if (p > 20.0f) return 1.0f;
    const float z = expf(p);
    return z / (z + 1.0f);
}

// an action's term of log p(x): (a - 1) ln x + (b - 1) ln(1 - x) - lnB(a, b).  1 - x is exact in double for an fp32 x >= 2^-24.  An x
// outside (0, 1) gives NaN: -inf there would make the ratio 0 and leave a finite loss over an infinite gradient
__device__ inline double beta_logp_term(double a, double b, double x, double* lx_, double* l1x_) {
    const bool inside = x > 0.0 && x < 1.0;
    const double lx = inside ? log(x) : (double)NAN, l1x = inside ? log(1.0 - x) : (double)NAN;
    *lx_ = lx; *l1x_ = l1x;
    return (a - 1.0) * lx + (b - 1.0) * l1x - lnbeta_d(a, b);
}

template <int LPR>
__global__ __launch_bounds__(NTHR) void ppo_loss_beta_kernel(int B, int A, const float* __restrict__ raw, const float* __restrict__ value,
                                                              const float* __restrict__ x_, const float* __restrict__ old_logp,
                                                              const float* __restrict__ old_alpha, const float* __restrict__ old_beta,
                                                              const float* __restrict__ adv_, const float* __restrict__ ret_,
                                                              const float* __restrict__ tv_, float clip, float vcoef, float ecoef, int use_clipped,
                                                              float* __restrict__ d_raw, float* __restrict__ d_value, double* __restrict__ partials) {
    double red[NRED];
#pragma unroll
    for (int k = 0; k < NRED; ++k) red[k] = 0.0;
    const float invB = 1.0f / (float)B;
    // LPR lanes per row, one action each; a block covers ROWS rows in ROWS * LPR / NTHR passes (the bound is a multiple of 64: a wave
    // is inside or outside as a whole, and so is a row's group)
    for (int e = threadIdx.x; e < ROWS * LPR; e += NTHR) {
        const int i = blockIdx.x * ROWS + e / LPR, k = e % LPR;
        const bool row_live = i < B, live = row_live && k < A;
        double lp = 0.0, kl = 0.0, ent = 0.0;
        float dla = 0.f, dlb = 0.f, dha = 0.f, dhb = 0.f, sp = 0.f, sq = 0.f;
        if (live) {
            const float p = raw[(size_t)i * (2 * A) + k], q = raw[(size_t)i * (2 * A) + A + k];
            const double a = (double)beta_param(p), b = (double)beta_param(q), s = a + b;
            sp = beta_dparam(p); sq = beta_dparam(q);
            double lx, l1x;
            lp = beta_logp_term(a, b, (double)x_[(size_t)i * A + k], &lx, &l1x);
            const double lnB = lnbeta_d(a, b);
            const double pa = digamma_d(a), pb = digamma_d(b), ps = digamma_d(s);
            const double ta = trigamma_d(a), tb = trigamma_d(b), ts = trigamma_d(s);
            dla = (float)(lx - pa + ps);
            dlb = (float)(l1x - pb + ps);
            ent = lnB - (a - 1.0) * pa - (b - 1.0) * pb + (s - 2.0) * ps;
            dha = (float)(-(a - 1.0) * ta + (s - 2.0) * ts);
            dhb = (float)(-(b - 1.0) * tb + (s - 2.0) * ts);
            // KL(old || new) of two Betas
            const double a0 = (double)old_alpha[(size_t)i * A + k], b0 = (double)old_beta[(size_t)i * A + k];
            kl = lnB - lnbeta_d(a0, b0) + (a0 - a) * digamma_d(a0) + (b0 - b) * digamma_d(b0) + ((a - a0) + (b - b0)) * digamma_d(a0 + b0);
        }
        lp = group_sum<LPR>(lp);
        kl = group_sum<LPR>(kl);
        ent = group_sum<LPR>(ent);
        if (row_live) {
        // the row's scalars, in every lane of its group (ppo_loss_sd_kernel's expressions)
        const float logp = (float)lp;
        const float adv = adv_[i];
        const float ratio = expf(logp - old_logp[i]);
        const float lo = 1.0f - clip, hi = 1.0f + clip;
        const float rc = nmin(nmax(ratio, lo), hi);
        const float s1 = -adv * ratio, s2 = -adv * rc;
        const float surr = nmax(s1, s2);
        // d max(s1, s2): the larger one takes the gradient, a tie splits it; d clamp = 1 on [lo, hi]
        const float w1 = s1 > s2 ? 1.f : (s1 == s2 ? 0.5f : 0.f), w2 = 1.f - w1;
        const float in_range = (ratio >= lo && ratio <= hi) ? 1.f : 0.f;
        const float g_ratio = -adv * (w1 + w2 * in_range);
        const float g_logp = g_ratio * ratio * invB;
        const float g_ent = ecoef * invB;   // the entropy bonus: -ecoef * mean_b H_b
        if (live) {
            d_raw[(size_t)i * (2 * A) + k] = (g_logp * dla - g_ent * dha) * sp;
            d_raw[(size_t)i * (2 * A) + A + k] = (g_logp * dlb - g_ent * dhb) * sq;
        }
        if (k == 0) {
        const float v = value[i], ret = ret_[i];
        float vl, gv;
        if (use_clipped) {
            const float tv = tv_[i];
            const float dv = v - tv;
            const float vc = tv + nmin(nmax(dv, -clip), clip);
            const float l1 = (v - ret) * (v - ret), l2 = (vc - ret) * (vc - ret);
            vl = nmax(l1, l2);
            const float u1 = l1 > l2 ? 1.f : (l1 == l2 ? 0.5f : 0.f), u2 = 1.f - u1;
            const float vin = (dv >= -clip && dv <= clip) ? 1.f : 0.f;
            // (clamp's backward SELECTS: outside the interval the gradient is 0 even where (vc - ret) is infinite -- a target value of inf)
            gv = u1 * 2.0f * (v - ret) + (vin != 0.f ? u2 * 2.0f * (vc - ret) : 0.f);
        } else {
            vl = (ret - v) * (ret - v);
            gv = -2.0f * (ret - v);
        }
        d_value[i] = vcoef * gv * invB;
        red[0] += (double)surr; red[1] += (double)vl; red[2] += kl; red[3] += ent;
        }
        }
    }
    __shared__ double s_red[NTHR / 64][NRED];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NRED; ++k) {
        const double t = wave_sum(red[k]);   // the batch sums run in double (grx_ppo.hip: the surrogate cancels to ~1e-3 of its terms)
        if (lane == 0) s_red[wv][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < NRED) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < NTHR / 64; ++w) t += s_red[w][threadIdx.x];
        partials[(size_t)blockIdx.x * NRED + threadIdx.x] = t;
    }
}

// the block partials added in block order; fetched in parallel into LDS while they fit (1024 blocks: 65536 rows), added from there in
// the SAME order (ppo_loss_sd_finalize)
__global__ __launch_bounds__(64) void ppo_loss_beta_finalize(int B, int nblk, const double* __restrict__ partials, float vcoef, float ecoef,
                                                              float* __restrict__ out) {
    const int k = threadIdx.x;
    constexpr int STAGE = 4096;
    __shared__ double s_p[STAGE];
    const bool staged = nblk * NRED <= STAGE;
    if (staged) {
        for (int i = k; i < nblk * NRED; i += 64) s_p[i] = partials[i];
        __syncthreads();
    }
    double t = 0.0;
    if (k < NRED)
        for (int b = 0; b < nblk; ++b) t += staged ? s_p[b * NRED + k] : partials[(size_t)b * NRED + k];
    __shared__ double s_t[NRED];
    if (k < NRED) s_t[k] = t;
    __syncthreads();
    if (k == 0) {
        const float surr = (float)(s_t[0] / (double)B), vl = (float)(s_t[1] / (double)B), klm = (float)(s_t[2] / (double)B);
        const float ent = (float)(s_t[3] / (double)B);
        out[0] = surr; out[1] = vl; out[2] = surr + vcoef * vl - ecoef * ent; out[3] = klm;
    }
}

__global__ __launch_bounds__(NTHR) void beta_params_kernel(int M, int A, const float* __restrict__ raw, float* __restrict__ alpha,
                                                            float* __restrict__ beta) {
    const size_t n = (size_t)M * A;
    for (size_t e = (size_t)blockIdx.x * NTHR + threadIdx.x; e < n; e += (size_t)gridDim.x * NTHR) {
        const size_t i = e / A, k = e % A;
        alpha[e] = beta_param(raw[i * (2 * A) + k]);
        beta[e] = beta_param(raw[i * (2 * A) + A + k]);
    }
}

// LPR lanes per row as in the loss kernel; a block covers NTHR / LPR rows
template <int LPR>
__global__ __launch_bounds__(NTHR) void beta_sample_kernel(int M, int A, const float* __restrict__ alpha, const float* __restrict__ beta,
                                                            const float* __restrict__ g1, const float* __restrict__ g2,
                                                            const float* __restrict__ lo, const float* __restrict__ span,
                                                            float* __restrict__ x_, float* __restrict__ actions, float* __restrict__ logp) {
    const int e = threadIdx.x;
    const int i = blockIdx.x * (NTHR / LPR) + e / LPR, k = e % LPR;
    const bool live = i < M && k < A;
    double lp = 0.0;
    if (live) {
        const size_t o = (size_t)i * A + k;
        const float ga = g1[o], gb = g2[o];
        const float x = fminf(fmaxf(ga / (ga + gb), X_MIN), X_MAX);   // (a 0 / 0 of two underflowed draws lands on the lower end)
        x_[o] = x;
        actions[o] = fmaf(span[k], x, lo[k]);
        double lx, l1x;
        lp = beta_logp_term((double)alpha[o], (double)beta[o], (double)x, &lx, &l1x);
    }
    lp = group_sum<LPR>(lp);
    if (live && k == 0) logp[i] = (float)lp;
}

__global__ __launch_bounds__(NTHR) void beta_functions_kernel(int n, const float* __restrict__ t, float* __restrict__ lg, float* __restrict__ dg,
                                                               float* __restrict__ tg) {
    const int i = blockIdx.x * NTHR + threadIdx.x;
    if (i >= n) return;
    const double y = (double)t[i];
    lg[i] = (float)lgamma_d(y); dg[i] = (float)digamma_d(y); tg[i] = (float)trigamma_d(y);
}

inline int lanes_per_row(int A) { int l = 1; while (l < A) l <<= 1; return l; }
}  // namespace

// in floats (the buffer holds doubles: 2 floats each; the caller's allocation must be 8-byte aligned)
extern "C" int grx_ppo_loss_beta_partials_size(int batch) { return batch < 1 ? 0 : ((batch + ROWS - 1) / ROWS) * NRED * 2; }

extern "C" int grx_ppo_loss_beta(int batch, int A, const float* raw, const float* value, const float* x, const float* old_logp,
                                 const float* old_alpha, const float* old_beta, const float* advantages, const float* returns,
                                 const float* target_values, float clip_param, float value_loss_coef, float entropy_coef,
                                 int use_clipped_value_loss, float* out, float* d_raw, float* d_value, float* partials, void* stream) {
    if (batch < 1 || A < 1 || A > MAXA) return -1;
    if (!raw || !value || !x || !old_logp || !old_alpha || !old_beta || !advantages || !returns || !out || !d_raw || !d_value || !partials)
        return -1;
    if (use_clipped_value_loss && !target_values) return -1;
    if ((uintptr_t)partials % 8 != 0) return -1;
    hipStream_t st = (hipStream_t)stream;
    const int nblk = (batch + ROWS - 1) / ROWS;
#define GRX_BETA_CASE(N) case N: hipLaunchKernelGGL(ppo_loss_beta_kernel<N>, dim3(nblk), dim3(NTHR), 0, st, batch, A, raw, value, x, old_logp, \
                                                    old_alpha, old_beta, advantages, returns, target_values, clip_param, value_loss_coef, \
                                                    entropy_coef, use_clipped_value_loss, d_raw, d_value, (double*)partials); break;
    switch (lanes_per_row(A)) { GRX_BETA_CASE(1) GRX_BETA_CASE(2) GRX_BETA_CASE(4) GRX_BETA_CASE(8) GRX_BETA_CASE(16) GRX_BETA_CASE(32) }
#undef GRX_BETA_CASE
    hipLaunchKernelGGL(ppo_loss_beta_finalize, dim3(1), dim3(64), 0, st, batch, nblk, (const double*)partials, value_loss_coef, entropy_coef, out);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int grx_beta_params(int M, int A, const float* raw, float* alpha, float* beta, void* stream) {
    if (M < 1 || A < 1 || A > MAXA || !raw || !alpha || !beta) return -1;
    const size_t n = (size_t)M * A;
    const int nblk = (int)((n + NTHR - 1) / NTHR < 65535 ? (n + NTHR - 1) / NTHR : 65535);
    hipLaunchKernelGGL(beta_params_kernel, dim3(nblk), dim3(NTHR), 0, (hipStream_t)stream, M, A, raw, alpha, beta);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int grx_beta_sample(int M, int A, const float* alpha, const float* beta, const float* g1, const float* g2, const float* lo,
                               const float* span, float* x, float* actions, float* logp, void* stream) {
    if (M < 1 || A < 1 || A > MAXA || !alpha || !beta || !g1 || !g2 || !lo || !span || !x || !actions || !logp) return -1;
    hipStream_t st = (hipStream_t)stream;
    const int lpr = lanes_per_row(A);
    const int nblk = (M + NTHR / lpr - 1) / (NTHR / lpr);
#define GRX_BETA_CASE(N) case N: hipLaunchKernelGGL(beta_sample_kernel<N>, dim3(nblk), dim3(NTHR), 0, st, M, A, alpha, beta, g1, g2, lo, span, x, \
                                                    actions, logp); break;
    switch (lpr) { GRX_BETA_CASE(1) GRX_BETA_CASE(2) GRX_BETA_CASE(4) GRX_BETA_CASE(8) GRX_BETA_CASE(16) GRX_BETA_CASE(32) }
#undef GRX_BETA_CASE
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int grx_beta_functions(int n, const float* t, float* lgamma_out, float* digamma_out, float* trigamma_out, void* stream) {
    if (n < 1 || !t || !lgamma_out || !digamma_out || !trigamma_out) return -1;
    hipLaunchKernelGGL(beta_functions_kernel, dim3((n + NTHR - 1) / NTHR), dim3(NTHR), 0, (hipStream_t)stream, n, t, lgamma_out, digamma_out,
                       trigamma_out);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
