// grx_ppo_noise.hip -- PPO with a state-dependent action noise (include/grx_ppo_noise.h, rl/modules.py `state_dependent_std`): the actor's
// output layer has 2A outputs, raw[i] = [mean (A) | s (A)], and sigma = s (`scalar`) or exp(s) (`log`) per row.
//   grx_ppo_loss_sd          the minibatch loss of grx_ppo.hip's ppo_loss_kernel term by term with a sigma per row, the entropy a fourth
//                            batch sum, the gradient written straight onto the raw output
//   grx_mlp_policy_head_sd   the rollout's fused policy head for the 2A-wide layer: both halves on the matrix cores, sampling and
//                            log-probability in the epilogue, one launch
// A translation unit of its own: the other kernels' code objects are what they were.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grx_ppo.h"

namespace {
constexpr int MAXA = 32;
constexpr int NTHR = 256;
constexpr int NRED = 4;   // surrogate, value loss, KL, entropy

// (grx_ppo.hip: torch.max / torch.clamp PROPAGATE NaN, fmaxf / fminf drop it -- a NaN ratio or value must reach the loss, so that
//  the update's NaN-skip fires.  With `scalar` a non-positive s gives logf(s) = NaN or -inf on that row: the same way out)
__device__ inline float nmax(float a, float b) { return (a > b || a != a) ? a : b; }
__device__ inline float nmin(float a, float b) { return (a < b || a != a) ? a : b; }

__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

// One thread per row, as ppo_loss_kernel.  The expressions shared with it are spelled the same way, so that the mean half of d_raw
// equals its d_mu bit for bit where every row carries the same sigma (tests/test_noise_std_gpu.py).
template <int A>
__global__ __launch_bounds__(NTHR) void ppo_loss_sd_kernel(int B, const float* __restrict__ raw, int log_std,
                                                            const float* __restrict__ value, const float* __restrict__ actions,
                                                            const float* __restrict__ old_logp, const float* __restrict__ old_mu,
                                                            const float* __restrict__ old_sigma, const float* __restrict__ adv_,
                                                            const float* __restrict__ ret_, const float* __restrict__ tv_,
                                                            float clip, float vcoef, float ecoef, int use_clipped,
                                                            float* __restrict__ d_raw, float* __restrict__ d_value, double* __restrict__ partials) {
    const int i = blockIdx.x * NTHR + threadIdx.x;
    float red[NRED];
#pragma unroll
    for (int k = 0; k < NRED; ++k) red[k] = 0.f;
    if (i < B) {
        const float invB = 1.0f / (float)B;
        float sg[A], df[A];
        float logp = 0.f, kl = 0.f, ent = 0.f;
#pragma unroll
        for (int k = 0; k < A; ++k) {
            const float rs = raw[(size_t)i * (2 * A) + A + k], m = raw[(size_t)i * (2 * A) + k];
            const float s = log_std ? expf(rs) : rs;
            // (log: log sigma is s itself, not logf(expf(s)) -- unless expf saturated: torch's log of a sigma of inf or 0 is +-inf, and a
            //  finite s = 100 there left the loss finite over gradients that are not)
            const float ls = log_std ? ((s == INFINITY || s == 0.f) ? logf(s) : rs) : logf(s);
            sg[k] = s;
            df[k] = actions[(size_t)i * A + k] - m;
            // Normal.log_prob: -((x - loc)^2) / (2 var) - log(scale) - log(sqrt(2 pi))
            logp += -(df[k] * df[k]) / (2.0f * s * s) - ls - 0.9189385332046727f;
            const float os = old_sigma[(size_t)i * A + k], dm = old_mu[(size_t)i * A + k] - m;
            kl += logf(s / os + 1.e-5f) + (os * os + dm * dm) / (2.0f * s * s) - 0.5f;
            ent += 1.4189385332046727f + ls;   // Normal.entropy: 0.5 + 0.5 log(2 pi) + log(scale)
        }
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
        const float g_ent = ecoef * invB;   // the entropy bonus: -ecoef * mean_b sum_k log(sigma_bk) -> -ecoef / (B sigma)
#pragma unroll
        for (int k = 0; k < A; ++k) {
            const float s = sg[k], inv2 = 1.0f / (s * s);
            d_raw[(size_t)i * (2 * A) + k] = g_logp * df[k] * inv2;
            // (np: torch's chain to d sigma through var = sigma^2, times 0 -- +-0 where it is finite, NaN where it is not: grx_ppo.hip)
            const float half = 0.5f * inv2;
            const float np = 0.f * (g_logp * (((df[k] * df[k] * half) * half) * 2.0f * (2.0f * s)) - g_logp / s);
            const float ds = g_logp * (df[k] * df[k] * inv2 / s - 1.0f / s) - g_ent / s + np;
            d_raw[(size_t)i * (2 * A) + A + k] = log_std ? ds * s : ds;   // (log: d sigma / d s = sigma)
        }
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
        red[0] = surr; red[1] = vl; red[2] = kl; red[3] = ent;
    }
    __shared__ double s_red[NTHR / 64][NRED];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NRED; ++k) {
        const double t = wave_sum((double)red[k]);   // the batch sums run in double (grx_ppo.hip: the surrogate cancels to ~1e-3 of its terms)
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

// the block partials added in block order; fetched in parallel into LDS while they fit (1024 blocks: 262144 rows), added from there in
// the SAME order
__global__ __launch_bounds__(64) void ppo_loss_sd_finalize(int B, int nblk, const double* __restrict__ partials, float vcoef, float ecoef,
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

// ---------------------------------------------------------------------------------------------------------------------
// The policy head.  grx_ppo.hip's mlp_layer_kernel blocking (64 rows per 256-thread block, K in chunks of 64 through double-buffered
// LDS tiles [k][row] of row stride 65, v_mfma_f32_32x32x2_f32) with the 64-column tile holding BOTH halves of the layer: tile columns
// 0..31 are the mean rows of W (rows 0..A-1, zero beyond), tile columns 32..63 the s rows (A..2A-1).  Wave (wy, wx) multiplies rows
// 32 wy.. by tile columns 32 wx.. exactly as a wave of grx_mlp_layer does for the same half of W on its own -- one k-ordered fmaf chain
// from zero per output, then + bias -- so mu and the raw s equal grx_mlp_layer's bit for bit.  The mean wave (wx = 0) and the s wave
// (wx = 1) of the same 32 rows hold an action's mean and s in the same lane and accumulator register: the s wave hands its 16
// registers over through LDS ([register][lane], conflict free), and the mean wave samples and reduces the log-probability over its
// half wave as mlp_layer_kernel<HEAD> does.  (Two accumulators in one wave would need no hand-over, but leave two of the four waves of
// a block without matrix work: this way the head's time is that of the [A]-sigma head, whose wx = 1 waves multiply zeros.)
// Operand maps (cdna_hip_programming.md): A: lane l holds A[i = l & 31][k = l >> 5]; B: B[k = l >> 5][j = l & 31];
// D: col = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int ML_BM = 64, ML_KC = 64, ML_LD = 65;

// 64 tile rows x 64 k of a row-major matrix -> registers (4 x float4 per thread: thread t, pass p -> tile row 16 p + t / 16, k 4 (t % 16)),
// zero beyond the matrix.  Tile row j is matrix row r0 + j (HALVES = false: X) or, for W, j < 32 ? j : A + j - 32, live while (j & 31) < A.
template <bool VEC, bool HALVES>
__device__ inline void hd_fetch(const float* __restrict__ G, int rows, int ld, int r0, int A, int k0, int tid, float4 v[4]) {
    const int kq = k0 + 4 * (tid & 15);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int j = 16 * p + (tid >> 4);
        const int r = HALVES ? ((j & 31) < A ? (j < 32 ? j : A + j - 32) : rows) : r0 + j;
        const float* g = G + (size_t)min(r, rows - 1) * ld + kq;
        float4 x = {0.f, 0.f, 0.f, 0.f};
        if (r < rows) {
            if (VEC) { if (kq < ld) x = *reinterpret_cast<const float4*>(g); }   // (ld % 4 == 0: a quad is inside or outside as a whole)
            else { if (kq < ld) x.x = g[0]; if (kq + 1 < ld) x.y = g[1]; if (kq + 2 < ld) x.z = g[2]; if (kq + 3 < ld) x.w = g[3]; }
        }
        v[p] = x;
    }
}
__device__ inline void hd_stash(float* __restrict__ S, int tid, const float4 v[4]) {
    const int kq = 4 * (tid & 15);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        float* s = S + kq * ML_LD + 16 * p + (tid >> 4);
        s[0] = v[p].x; s[ML_LD] = v[p].y; s[2 * ML_LD] = v[p].z; s[3 * ML_LD] = v[p].w;
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void policy_head_sd_kernel(int M, int K, int A, const float* __restrict__ X, const float* __restrict__ W,
                                                              const float* __restrict__ bias, int log_std, const float* __restrict__ eps,
                                                              float* __restrict__ actions, float* __restrict__ logp,
                                                              float* __restrict__ mu, float* __restrict__ sigma) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "policy_head_sd_kernel keeps 65 KB of static LDS: gfx950 (160 KB per CU) only -- this library is built for MI355X, see the Makefile"
#endif
    __shared__ float Xs[2][ML_KC * ML_LD], Ws[2][ML_KC * ML_LD];   // double-buffered: chunk c + 1 lands while chunk c multiplies
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wy = wv >> 1, wx = wv & 1;
    const int m0 = blockIdx.x * ML_BM;
    float4 xr[4], wr[4];
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    hd_fetch<VEC, false>(X, M, K, m0, A, 0, tid, xr);
    hd_fetch<VEC, true>(W, 2 * A, K, 0, A, 0, tid, wr);
    hd_stash(Xs[0], tid, xr); hd_stash(Ws[0], tid, wr);
    __syncthreads();
    int buf = 0;
    for (int k0 = 0; k0 < K; k0 += ML_KC, buf ^= 1) {
        const bool more = k0 + ML_KC < K;
        if (more) { hd_fetch<VEC, false>(X, M, K, m0, A, k0 + ML_KC, tid, xr); hd_fetch<VEC, true>(W, 2 * A, K, 0, A, k0 + ML_KC, tid, wr); }
        const float* xa = Xs[buf] + (lane >> 5) * ML_LD + 32 * wy + (lane & 31);
        const float* wb = Ws[buf] + (lane >> 5) * ML_LD + 32 * wx + (lane & 31);
        const int nk = min(ML_KC, K - k0);
        if (nk == ML_KC) {
            float av[ML_KC / 2], bv[ML_KC / 2];   // the chunk's operands first, then 32 MFMAs back to back (mlp_layer_kernel)
#pragma unroll
            for (int kk = 0; kk < ML_KC / 2; ++kk) { av[kk] = xa[2 * kk * ML_LD]; bv[kk] = wb[2 * kk * ML_LD]; }
#pragma unroll
            for (int kk = 0; kk < ML_KC / 2; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[kk], bv[kk], acc, 0, 0, 0);
        } else {
            for (int kk = 0; kk < (nk + 1) / 2; ++kk)   // (the tile is zero beyond K)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[2 * kk * ML_LD], wb[2 * kk * ML_LD], acc, 0, 0, 0);
        }
        if (more) { hd_stash(Xs[buf ^ 1], tid, xr); hd_stash(Ws[buf ^ 1], tid, wr); }
        __syncthreads();
    }
    // (every wave is past its last LDS read: Xs[0] carries the s waves' registers over, [wy][register][lane])
    const int col = lane & 31;
    const bool live = col < A;
    float* hand = Xs[0] + wy * (16 * 64);
    if (wx == 1) {
        const float b = (live && bias) ? bias[A + col] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) hand[r * 64 + lane] = acc[r] + b;
    }
    __syncthreads();
    if (wx != 0) return;
    const float b = (live && bias) ? bias[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + 32 * wy + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const bool ok = live && row < M;
        const float m = acc[r] + b;
        float term = 0.f;
        if (ok) {
            const float rs = hand[r * 64 + lane];
            const float sd = log_std ? expf(rs) : rs;
            const float lsd = log_std ? rs : logf(sd), inv2 = 1.0f / (2.0f * sd * sd);
            const size_t o = (size_t)row * A + col;
            const float a = m + sd * eps[o];
            const float d = a - m;
            term = -(d * d) * inv2 - lsd - 0.9189385332046727f;
            actions[o] = a; mu[o] = m; sigma[o] = sd;
        }
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) term += __shfl_xor(term, off);   // over the 32 lanes (actions) of this row
        if (col == 0 && row < M) logp[row] = term;
    }
}

template <int A>
void launch_loss(int nblk, hipStream_t st, int B, const float* raw, int log_std, const float* value, const float* actions,
                 const float* old_logp, const float* old_mu, const float* old_sigma, const float* adv, const float* ret, const float* tv,
                 float clip, float vcoef, float ecoef, int use_clipped, float* d_raw, float* d_value, double* partials) {
    hipLaunchKernelGGL(ppo_loss_sd_kernel<A>, dim3(nblk), dim3(NTHR), 0, st, B, raw, log_std, value, actions, old_logp, old_mu, old_sigma,
                       adv, ret, tv, clip, vcoef, ecoef, use_clipped, d_raw, d_value, partials);
}
}  // namespace

// in floats (the buffer holds doubles: 2 floats each; the caller's allocation must be 8-byte aligned)
extern "C" int grx_ppo_loss_sd_partials_size(int batch) { return batch < 1 ? 0 : ((batch + NTHR - 1) / NTHR) * NRED * 2; }

extern "C" int grx_ppo_loss_sd(int batch, int A, const float* raw, int log_std, const float* value, const float* actions,
                               const float* old_logp, const float* old_mu, const float* old_sigma, const float* advantages,
                               const float* returns, const float* target_values, float clip_param, float value_loss_coef,
                               float entropy_coef, int use_clipped_value_loss, float* out, float* d_raw, float* d_value, float* partials,
                               void* stream) {
    if (batch < 1 || A < 1 || A > MAXA) return -1;
    if (!raw || !value || !actions || !old_logp || !old_mu || !old_sigma || !advantages || !returns || !out || !d_raw || !d_value || !partials)
        return -1;
    if (use_clipped_value_loss && !target_values) return -1;
    if ((uintptr_t)partials % 8 != 0) return -1;
    hipStream_t st = (hipStream_t)stream;
    const int nblk = (batch + NTHR - 1) / NTHR;
    const int lg = log_std ? 1 : 0;
#define GRX_SD_CASE(N) case N: launch_loss<N>(nblk, st, batch, raw, lg, value, actions, old_logp, old_mu, old_sigma, advantages, returns, \
                                              target_values, clip_param, value_loss_coef, entropy_coef, use_clipped_value_loss, d_raw, d_value, \
                                              (double*)partials); break;
    switch (A) {
        GRX_SD_CASE(1) GRX_SD_CASE(2) GRX_SD_CASE(3) GRX_SD_CASE(4) GRX_SD_CASE(5) GRX_SD_CASE(6) GRX_SD_CASE(7) GRX_SD_CASE(8)
        GRX_SD_CASE(9) GRX_SD_CASE(10) GRX_SD_CASE(11) GRX_SD_CASE(12) GRX_SD_CASE(13) GRX_SD_CASE(14) GRX_SD_CASE(15) GRX_SD_CASE(16)
        GRX_SD_CASE(17) GRX_SD_CASE(18) GRX_SD_CASE(19) GRX_SD_CASE(20) GRX_SD_CASE(21) GRX_SD_CASE(22) GRX_SD_CASE(23) GRX_SD_CASE(24)
        GRX_SD_CASE(25) GRX_SD_CASE(26) GRX_SD_CASE(27) GRX_SD_CASE(28) GRX_SD_CASE(29) GRX_SD_CASE(30) GRX_SD_CASE(31) GRX_SD_CASE(32)
    }
#undef GRX_SD_CASE
    hipLaunchKernelGGL(ppo_loss_sd_finalize, dim3(1), dim3(64), 0, st, batch, nblk, (const double*)partials, value_loss_coef, entropy_coef, out);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int grx_mlp_policy_head_sd(int M, int K, int A, const float* X, const float* W, const float* bias, int log_std, const float* eps,
                                      float* actions, float* logp, float* mu, float* sigma, void* stream) {
    if (M < 1 || K < 1 || A < 1 || A > 32 || !X || !W || !eps || !actions || !logp || !mu || !sigma) return -1;
    const bool vec = K % 4 == 0 && ((uintptr_t)X % 16 == 0) && ((uintptr_t)W % 16 == 0);
    const dim3 grid((M + ML_BM - 1) / ML_BM);
    const int lg = log_std ? 1 : 0;
    if (vec) hipLaunchKernelGGL(policy_head_sd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, M, K, A, X, W, bias, lg, eps, actions, logp, mu, sigma);
    else hipLaunchKernelGGL(policy_head_sd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, M, K, A, X, W, bias, lg, eps, actions, logp, mu, sigma);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
