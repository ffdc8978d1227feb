// grx_ppo_cenet.hip -- the context-aided estimator network (include/grx_ppo_cenet.h; rl/cenet.py).
//
// grx_cenet_head: what stands behind the encoder's layers in a rollout step, ONE launch.  One WAVE per row, four rows per pass of a block
// (grx_smooth_gather_rows' shape): the wave walks x's row -- lane l elements l, l + 64, ... as float4 where the host found every row of x
// and of out on a 16-byte boundary, as dwords otherwise --, then lanes 0 .. E + Z - 1 write v_hat and z (E + Z <= 72: two passes at most)
// and lanes 0 .. E - 1 select the privileged columns.  No LDS, no barrier, no atomics: a row's bytes depend on that row alone.
//
// cenet_z is the ONE place z is formed: sigma is the fp32 rounding of exp in double (so its error is the final rounding's alone), z one
// fmaf.  The head and grx_cenet_reparam call it with the same operands in the same order: the same bits.
//
// grx_cenet_loss has grx_smooth_loss's shape.  The index space is [mb][W], W = E + Z + F: column c < E is an estimation term, c < E + Z a
// KL term, the rest reconstruction terms, selected -- not multiplied -- by the row's valid byte; column 0 counts the row.  Block b owns
// elements [b * 2048, (b + 1) * 2048), thread t of it t, t + 256, ...; a thread adds its eight elements in index order, a wave its lanes in
// a shuffle tree, thread 0..3 the four waves in wave order -> partials[b] = {sum_est, sum_rec, sum_kl, n_v}, double.  Launch 2 (one wave):
// lane l adds the partials l, l + 64, ... in order, then the same tree -> out[5].  Launch 3: the gradients over [mb][E + 2Z + F], each
// element one rounding of a double expression.  The order of every sum is a function of (mb, E, Z, F) alone.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/grx_ppo.h"

#pragma clang fp contract(off)

namespace {

constexpr float CN_LV_MIN = -10.f, CN_LV_MAX = 2.f;

__device__ inline bool cenet_unsaturated(float raw) { return raw >= CN_LV_MIN && raw <= CN_LV_MAX; }   // (a NaN: false, as torch.clamp's gradient)
__device__ inline float cenet_lv(float raw) { return raw < CN_LV_MIN ? CN_LV_MIN : (raw > CN_LV_MAX ? CN_LV_MAX : raw); }   // (a NaN passes, as torch.clamp)
__device__ inline float cenet_sigma(float raw) { return (float)exp(0.5 * (double)cenet_lv(raw)); }
__device__ inline float cenet_z(float mu, float raw, float eps) { return fmaf(cenet_sigma(raw), eps, mu); }

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + na, b0 = (uintptr_t)b, b1 = b0 + nb;
    return a0 < b1 && b0 < a1;
}
inline bool sizes_ok(int E, int Z) { return E >= 1 && E <= GRX_CENET_MAX_TARGETS && Z >= 1 && Z <= GRX_CENET_MAX_LATENT; }

// ---- the head -------------------------------------------------------------------------------------------------------------------------
constexpr int CH_WAVES = 4;

struct HeadArgs {
    const float* x; const float* enc; const float* eps; const float* pri; float* out; float* targets;
    int N, D, E, Z, P, vec;
    int cols[GRX_CENET_MAX_TARGETS];
};

__global__ __launch_bounds__(64 * CH_WAVES) void cenet_head_kernel(const HeadArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int D = a.D, E = a.E, Z = a.Z, OW = D + E + Z, EW = E + 2 * Z;
    for (size_t n = (size_t)blockIdx.x * CH_WAVES + wave; n < (size_t)a.N; n += (size_t)gridDim.x * CH_WAVES) {
        const float* __restrict__ x = a.x + n * D;
        const float* __restrict__ enc = a.enc + n * EW;
        float* __restrict__ out = a.out + n * OW;
        if (a.vec) {
            for (int j = lane; j < (D >> 2); j += 64) ((float4*)out)[j] = ((const float4*)x)[j];
        } else {
            for (int j = lane; j < D; j += 64) out[j] = x[j];
        }
        for (int c = lane; c < E + Z; c += 64) {
            float v;
            if (c < E) v = enc[c];
            else v = cenet_z(enc[c], enc[c + Z], a.eps[n * Z + (c - E)]);
            out[D + c] = v;
        }
        if (a.targets != nullptr && lane < E) a.targets[n * E + lane] = a.pri[n * a.P + a.cols[lane]];
    }
}

// ---- the reparameterisation -------------------------------------------------------------------------------------------------------------
constexpr int CR_THR = 256;

__global__ __launch_bounds__(CR_THR) void cenet_reparam_kernel(long long n, int E, int Z, const float* __restrict__ enc,
                                                               const float* __restrict__ eps, float* __restrict__ dec_in) {
    const long long i = (long long)blockIdx.x * CR_THR + threadIdx.x;
    if (i >= n) return;
    const int W = E + Z, EW = E + 2 * Z;
    const long long r = i / W;
    const int c = (int)(i - r * W);
    const float* e = enc + r * EW;
    dec_in[i] = c < E ? e[c] : cenet_z(e[c], e[c + Z], eps[r * Z + (c - E)]);
}

__global__ __launch_bounds__(CR_THR) void cenet_reparam_backward_kernel(long long n, int E, int Z, const float* __restrict__ enc,
                                                                        const float* __restrict__ eps, const float* __restrict__ d_in,
                                                                        float* __restrict__ d_enc) {
    const long long i = (long long)blockIdx.x * CR_THR + threadIdx.x;
    if (i >= n) return;
    const int W = E + Z, EW = E + 2 * Z;
    const long long r = i / EW;
    const int c = (int)(i - r * EW);
    const float* d = d_in + r * W;
    float g;
    if (c < E + Z) g = d[c];                  // d v_hat, d mu = dz
    else {
        const int j = c - E - Z;
        const float raw = enc[i];
        g = 0.f;
        if (cenet_unsaturated(raw)) g = ((d[E + j] * eps[r * Z + j]) * cenet_sigma(raw)) * 0.5f;
    }
    d_enc[i] = g;
}

// ---- the loss -------------------------------------------------------------------------------------------------------------------------
constexpr int CL_THR = 256;
constexpr int CL_PER = 8;
constexpr int CL_CHUNK = CL_THR * CL_PER;

__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;   // lane 0 holds the sum
}

struct LossArgs {
    const float* enc; const float* targets; const float* dec; const float* next; const unsigned char* valid;
    int mb, E, Z, F, next_ld, next_off;
    float beta;
};

__global__ __launch_bounds__(CL_THR) void cenet_loss_partials_kernel(const LossArgs a, long long n, double* __restrict__ partials) {
    __shared__ double waves[4][CL_THR / 64];
    const int E = a.E, Z = a.Z, F = a.F, W = E + Z + F, EW = E + 2 * Z;
    const long long base = (long long)blockIdx.x * CL_CHUNK + threadIdx.x;
    double s_est = 0.0, s_rec = 0.0, s_kl = 0.0, cnt = 0.0;
#pragma unroll
    for (int k = 0; k < CL_PER; ++k) {
        const long long i = base + (long long)k * CL_THR;
        if (i < n) {
            const long long r = i / W;
            const int c = (int)(i - r * W);
            if (c == 0 && a.valid[r] != 0) cnt += 1.0;
            if (c < E) {
                const double d = (double)a.enc[r * EW + c] - (double)a.targets[r * E + c];   // exact
                s_est += d * d;
            } else if (c < E + Z) {
                const double mu = (double)a.enc[r * EW + c];
                const double lv = (double)cenet_lv(a.enc[r * EW + c + Z]);
                s_kl += 0.5 * (((mu * mu + exp(lv)) - lv) - 1.0);
            } else if (a.valid[r] != 0) {   // a select: a masked row's successor is not even looked at
                const int f = c - E - Z;
                const double d = (double)a.dec[r * F + f] - (double)a.next[r * a.next_ld + a.next_off + f];
                s_rec += d * d;
            }
        }
    }
    s_est = wave_sum(s_est); s_rec = wave_sum(s_rec); s_kl = wave_sum(s_kl); cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        waves[0][w] = s_est; waves[1][w] = s_rec; waves[2][w] = s_kl; waves[3][w] = cnt;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const double* wv = waves[threadIdx.x];
        partials[(size_t)blockIdx.x * 4 + threadIdx.x] = ((wv[0] + wv[1]) + wv[2]) + wv[3];
    }
}

__global__ __launch_bounds__(64) void cenet_loss_finalize_kernel(int mb, int E, int F, int nblk, float beta, const double* __restrict__ partials,
                                                                 float* __restrict__ out) {
    double s_est = 0.0, s_rec = 0.0, s_kl = 0.0, cnt = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 64) {
        s_est += partials[(size_t)b * 4];
        s_rec += partials[(size_t)b * 4 + 1];
        s_kl += partials[(size_t)b * 4 + 2];
        cnt += partials[(size_t)b * 4 + 3];
    }
    s_est = wave_sum(s_est); s_rec = wave_sum(s_rec); s_kl = wave_sum(s_kl); cnt = wave_sum(cnt);
    if (threadIdx.x == 0) {
        const double l_est = s_est / ((double)mb * (double)E);
        const double l_rec = s_rec / ((double)F * (cnt > 1.0 ? cnt : 1.0));
        const double l_kl = s_kl / (double)mb;
        out[0] = (float)l_est; out[1] = (float)l_rec; out[2] = (float)l_kl;
        out[3] = (float)((l_est + l_rec) + (double)beta * l_kl);
        out[4] = (float)cnt;   // (< 2^24: exact)
    }
}

__global__ __launch_bounds__(CL_THR) void cenet_loss_grad_kernel(const LossArgs a, long long n, const float* __restrict__ out,
                                                                 float* __restrict__ d_enc, float* __restrict__ d_dec) {
    const int E = a.E, Z = a.Z, F = a.F, EW = E + 2 * Z, W2 = EW + F;
    const double nv = (double)out[4];
    const double g_est = 2.0 / ((double)a.mb * (double)E);
    const double g_rec = 2.0 / ((double)F * (nv > 1.0 ? nv : 1.0));
    const double g_kl = (double)a.beta / (double)a.mb;
    const long long base = (long long)blockIdx.x * CL_CHUNK + threadIdx.x;
#pragma unroll
    for (int k = 0; k < CL_PER; ++k) {
        const long long i = base + (long long)k * CL_THR;
        if (i < n) {
            const long long r = i / W2;
            const int c = (int)(i - r * W2);
            if (c < E) {
                d_enc[r * EW + c] = (float)(g_est * ((double)a.enc[r * EW + c] - (double)a.targets[r * E + c]));
            } else if (c < E + Z) {
                d_enc[r * EW + c] = (float)(g_kl * (double)a.enc[r * EW + c]);
            } else if (c < EW) {
                const float raw = a.enc[r * EW + c];
                double g = 0.0;
                if (cenet_unsaturated(raw)) g = g_kl * (0.5 * (exp((double)raw) - 1.0));
                d_enc[r * EW + c] = (float)g;
            } else {
                const int f = c - EW;
                double g = 0.0;
                if (a.valid[r] != 0) g = g_rec * ((double)a.dec[r * F + f] - (double)a.next[r * a.next_ld + a.next_off + f]);
                d_dec[r * F + f] = (float)g;   // (masked: +0)
            }
        }
    }
}

inline long long loss_elements(int mb, int E, int Z, int F) {
    if (mb < 1 || mb >= (1 << 24) || !sizes_ok(E, Z) || F < 1 || F > GRX_CENET_MAX_FRAME) return 0;
    const long long n = (long long)mb * (E + 2 * Z + F);
    return n < (1ll << 31) ? n : 0;
}

}  // namespace

extern "C" int grx_cenet_head(int N, int D, int E, int Z, const float* x, const float* enc_out, const float* eps, int P, const float* pri,
                              const int* target_cols, float* out, float* targets, void* stream) {
    if (!x || !enc_out || !eps || !out || N < 1 || D < 1 || D > GRX_CENET_MAX_INPUT || !sizes_ok(E, Z)) return -1;
    const int OW = D + E + Z;
    if ((long long)N * OW >= (1ll << 31)) return -1;
    const size_t ob = (size_t)N * OW * sizeof(float);
    if (overlap(out, ob, x, (size_t)N * D * sizeof(float)) || overlap(out, ob, enc_out, (size_t)N * (E + 2 * Z) * sizeof(float))
        || overlap(out, ob, eps, (size_t)N * Z * sizeof(float))) return -1;
    HeadArgs a;
    const bool want_targets = pri != nullptr && targets != nullptr;
    for (int e = 0; e < GRX_CENET_MAX_TARGETS; ++e) a.cols[e] = 0;
    if (want_targets) {
        if (P < 1 || !target_cols) return -1;
        for (int e = 0; e < E; ++e) {
            if (target_cols[e] < 0 || target_cols[e] >= P) return -1;
            a.cols[e] = target_cols[e];
        }
    }
    a.x = x; a.enc = enc_out; a.eps = eps; a.pri = want_targets ? pri : nullptr; a.out = out; a.targets = want_targets ? targets : nullptr;
    a.N = N; a.D = D; a.E = E; a.Z = Z; a.P = want_targets ? P : 0;
    a.vec = (D % 4 == 0 && OW % 4 == 0 && aligned16(x) && aligned16(out)) ? 1 : 0;
    const int passes = (N + CH_WAVES - 1) / CH_WAVES;
    hipLaunchKernelGGL(cenet_head_kernel, dim3(passes < 1024 ? passes : 1024), dim3(64 * CH_WAVES), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int grx_cenet_reparam(int mb, int E, int Z, const float* enc_out, const float* eps, float* dec_in, void* stream) {
    if (mb < 1 || !sizes_ok(E, Z) || !enc_out || !eps || !dec_in || (long long)mb * (E + 2 * Z) >= (1ll << 31)) return -1;
    const long long n = (long long)mb * (E + Z);
    hipLaunchKernelGGL(cenet_reparam_kernel, dim3((unsigned)((n + CR_THR - 1) / CR_THR)), dim3(CR_THR), 0, (hipStream_t)stream, n, E, Z,
                       enc_out, eps, dec_in);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int grx_cenet_reparam_backward(int mb, int E, int Z, const float* enc_out, const float* eps, const float* d_dec_in,
                                          float* d_enc_out, void* stream) {
    if (mb < 1 || !sizes_ok(E, Z) || !enc_out || !eps || !d_dec_in || !d_enc_out || (long long)mb * (E + 2 * Z) >= (1ll << 31)) return -1;
    const long long n = (long long)mb * (E + 2 * Z);
    hipLaunchKernelGGL(cenet_reparam_backward_kernel, dim3((unsigned)((n + CR_THR - 1) / CR_THR)), dim3(CR_THR), 0, (hipStream_t)stream, n, E,
                       Z, enc_out, eps, d_dec_in, d_enc_out);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int grx_cenet_loss_partials_size(int mb, int E, int Z, int F) {
    if (!loss_elements(mb, E, Z, F)) return 0;
    const long long n = (long long)mb * (E + Z + F);
    return (int)((n + CL_CHUNK - 1) / CL_CHUNK) * 8;   // four doubles per block
}

extern "C" int grx_cenet_loss(int mb, int E, int Z, int F, const float* enc_out, const float* targets, const float* dec, const float* next,
                              int next_ld, int next_off, const unsigned char* valid, float beta, float* out, float* d_enc_out, float* d_dec,
                              float* partials, void* stream) {
    const long long n2 = loss_elements(mb, E, Z, F);
    if (!n2) return -1;
    if (next_off < 0 || next_ld < 1 || (long long)next_off + F > (long long)next_ld || (long long)mb * next_ld >= (1ll << 31)) return -1;
    if (!(beta >= 0.0f) || !isfinite(beta)) return -1;
    if (!enc_out || !targets || !dec || !next || !valid || !out || !d_enc_out || !d_dec || !partials || ((uintptr_t)partials & 7)) return -1;
    LossArgs a;
    a.enc = enc_out; a.targets = targets; a.dec = dec; a.next = next; a.valid = valid;
    a.mb = mb; a.E = E; a.Z = Z; a.F = F; a.next_ld = next_ld; a.next_off = next_off; a.beta = beta;
    const long long n1 = (long long)mb * (E + Z + F);
    const int nblk = (int)((n1 + CL_CHUNK - 1) / CL_CHUNK), nblk2 = (int)((n2 + CL_CHUNK - 1) / CL_CHUNK);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cenet_loss_partials_kernel, dim3(nblk), dim3(CL_THR), 0, st, a, n1, (double*)partials);
    hipLaunchKernelGGL(cenet_loss_finalize_kernel, dim3(1), dim3(64), 0, st, mb, E, F, nblk, beta, (const double*)partials, out);
    hipLaunchKernelGGL(cenet_loss_grad_kernel, dim3(nblk2), dim3(CL_THR), 0, st, a, n2, (const float*)out, d_enc_out, d_dec);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
