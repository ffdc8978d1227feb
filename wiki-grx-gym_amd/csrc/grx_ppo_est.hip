// grx_ppo_est.hip -- the concurrent state estimator's rollout forward (include/grx_ppo_est.h; rl/estimator.py).
//
// One launch per rollout step instead of a launch per layer plus a concatenation and a column select: a 256-thread block owns a slab of
// 64 rows, copies them into the wide output row, runs EVERY layer of the estimator on them with the activations in LDS, writes the E
// estimated columns behind the copy and selects the target columns of the privileged frame.
//
// LDS (160 KiB per CU on gfx950, 149,760 B used, one block per CU): two activation buffers of 256 columns x 64 rows, [k][row] with row
// stride 65 -- the layout grx_ppo.hip's mlp_layer_kernel stages its X tile in, so a layer's epilogue writes the next layer's A operand in
// place -- and a double-buffered 32 x 64 tile of W, [k][col].  Layer 0 reads x from global memory through a double-buffered tile of its own
// that lives in the second activation buffer (nothing is in it until layer 1 writes its output there).  Layer l writes buffer l & 1.
//
// The same bits as grx_mlp_layer: wave (wy, wx) of the block multiplies rows 32 wy.. by columns n0 + 32 wx.. with
// v_mfma_f32_32x32x2_f32 from a zero accumulator, k ascending two at a time, ceil(K / 2) instructions with zeros beyond K, then + bias, then
// elu1 -- exactly the chain a wave of mlp_layer_kernel forms for the same output (its K chunk is 64 instead of 32: the order of k is the
// same).  A column beyond a layer's width is written as zero, so an odd K multiplies 0 x 0 in its last instruction, as there.
// Operand maps (cdna_hip_programming.md): A: lane l holds A[i = l & 31][k = l >> 5]; B: B[k = l >> 5][j = l & 31];
// D: col = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grx_ppo.h"

namespace {
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int ES_BM = 64, ES_BN = 64, ES_KC = 32, ES_LD = 65;
constexpr int ES_ACT = GRX_EST_MAX_WIDTH * ES_LD;   // floats of one activation buffer
constexpr int ES_TILE = ES_KC * ES_LD;              // floats of one operand tile

__device__ inline float elu1(float x) { return x > 0.f ? x : expm1f(x); }   // torch.nn.ELU(alpha = 1), as grx_ppo.hip spells it

struct EstArgs {
    grx_est_net net;
    int vec[GRX_EST_MAX_LAYERS];     // bit 0: W[l]'s rows load as float4; bit 1 (layer 0): x's rows do
    int cols[GRX_EST_MAX_TARGETS];   // target_cols
};

// 64 rows x 32 k of a row-major matrix -> registers (2 x float4 per thread: thread t, pass p -> row 32 p + t / 8, k 4 (t % 8)), zero
// beyond the matrix; vec: rows are 16-byte aligned (ld % 4 == 0: a quad is inside or outside as a whole)
__device__ inline void es_fetch(const float* __restrict__ G, int rows, int ld, int r0, int k0, int tid, bool vec, float4 v[2]) {
    const int kq = k0 + 4 * (tid & 7);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int r = r0 + 32 * p + (tid >> 3);
        float4 x = {0.f, 0.f, 0.f, 0.f};
        if (r < rows && kq < ld) {
            const float* g = G + (size_t)r * ld + kq;
            if (vec) x = *reinterpret_cast<const float4*>(g);
            else { x.x = g[0]; if (kq + 1 < ld) x.y = g[1]; if (kq + 2 < ld) x.z = g[2]; if (kq + 3 < ld) x.w = g[3]; }
        }
        v[p] = x;
    }
}
__device__ inline void es_stash(float* __restrict__ S, int tid, const float4 v[2]) {
    const int kq = 4 * (tid & 7);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        float* s = S + kq * ES_LD + 32 * p + (tid >> 3);
        s[0] = v[p].x; s[ES_LD] = v[p].y; s[2 * ES_LD] = v[p].z; s[3 * ES_LD] = v[p].w;
    }
}

__global__ __launch_bounds__(256) void est_forward_kernel(const EstArgs a, int N, int D, const float* __restrict__ x, int P,
                                                           const float* __restrict__ pri, float* __restrict__ out,
                                                           float* __restrict__ targets) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "est_forward_kernel keeps 146 KB of static LDS: gfx950 (160 KB per CU) only -- this library is built for MI355X, see the Makefile"
#endif
    __shared__ float lds[2 * ES_ACT + 2 * ES_TILE];
    float* const Ws = lds + 2 * ES_ACT;
    float* const Xs = lds + ES_ACT;   // layer 0's x tiles: inside activation buffer 1, which layer 1 is the first to write
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wy = wv >> 1, wx = wv & 1;
    const int m0 = blockIdx.x * ES_BM;
    const int rows = min(ES_BM, N - m0);
    const int nl = a.net.n_layers, E = a.net.widths[nl - 1], OW = D + E;

    // the copy and the column select: the slab's rows are contiguous in x
    {
        const float* xs = x + (size_t)m0 * D;
        for (int i = tid; i < rows * D; i += 256) {
            const int r = i / D, c = i - r * D;
            out[(size_t)(m0 + r) * OW + c] = xs[i];
        }
        if (pri != nullptr && targets != nullptr) {
            for (int i = tid; i < rows * E; i += 256) {
                const int r = i / E, e = i - r * E;
                targets[(size_t)(m0 + r) * E + e] = pri[(size_t)(m0 + r) * P + a.cols[e]];
            }
        }
    }

    int K = D;
#pragma unroll
    for (int l = 0; l < GRX_EST_MAX_LAYERS; ++l) {
        if (l < nl) {
            const int Nout = a.net.widths[l];
            const float* __restrict__ W = a.net.W[l];
            const float* __restrict__ bias = a.net.bias[l];
            const bool first = l == 0, last = l == nl - 1;
            const bool vw = (a.vec[l] & 1) != 0, vx = (a.vec[l] & 2) != 0;
            const float* Ain = lds + ((l + 1) & 1) * ES_ACT;   // what layer l - 1 wrote
            float* Aout = lds + (l & 1) * ES_ACT;
            for (int n0 = 0; n0 < Nout; n0 += ES_BN) {
                const bool live = n0 + 32 * wx < Nout;   // (a wave whose 32 columns lie beyond the layer only stages)
                f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
                float4 wr[2], xr[2];
                es_fetch(W, Nout, K, n0, 0, tid, vw, wr);
                es_stash(Ws, tid, wr);
                if (first) { es_fetch(x, N, D, m0, 0, tid, vx, xr); es_stash(Xs, tid, xr); }
                __syncthreads();   // (also: the previous layer's output is complete)
                int buf = 0;
                for (int k0 = 0; k0 < K; k0 += ES_KC, buf ^= 1) {
                    const bool more = k0 + ES_KC < K;
                    if (more) {   // in flight during the MFMAs
                        es_fetch(W, Nout, K, n0, k0 + ES_KC, tid, vw, wr);
                        if (first) es_fetch(x, N, D, m0, k0 + ES_KC, tid, vx, xr);
                    }
                    const float* xa = (first ? Xs + buf * ES_TILE : Ain + k0 * ES_LD) + (lane >> 5) * ES_LD + 32 * wy + (lane & 31);
                    const float* wb = Ws + buf * ES_TILE + (lane >> 5) * ES_LD + 32 * wx + (lane & 31);
                    const int nk = min(ES_KC, K - k0);
                    if (live) {
                        if (nk == ES_KC) {   // the chunk's operands into registers first, then the MFMAs back to back
                            float av[ES_KC / 2], bv[ES_KC / 2];
#pragma unroll
                            for (int kk = 0; kk < ES_KC / 2; ++kk) { av[kk] = xa[2 * kk * ES_LD]; bv[kk] = wb[2 * kk * ES_LD]; }
#pragma unroll
                            for (int kk = 0; kk < ES_KC / 2; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[kk], bv[kk], acc, 0, 0, 0);
                        } else {
                            for (int kk = 0; kk < (nk + 1) / 2; ++kk)   // (both tiles are zero beyond K)
                                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[2 * kk * ES_LD], wb[2 * kk * ES_LD], acc, 0, 0, 0);
                        }
                    }
                    if (more) {
                        es_stash(Ws + (buf ^ 1) * ES_TILE, tid, wr);
                        if (first) es_stash(Xs + (buf ^ 1) * ES_TILE, tid, xr);
                    }
                    __syncthreads();
                }
                if (live) {
                    const int col = n0 + 32 * wx + (lane & 31);   // < 256
                    const bool in = col < Nout;
                    const float b = (in && bias != nullptr) ? bias[col] : 0.f;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = 32 * wy + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                        const float y = acc[r] + b;
                        if (last) {
                            if (in && m0 + row < N) out[(size_t)(m0 + row) * OW + D + col] = y;
                        } else {
                            Aout[col * ES_LD + row] = in ? elu1(y) : 0.f;   // (zero beyond the layer: the next layer's k = K of an odd K)
                        }
                    }
                }
            }
            K = Nout;
        }
    }
}
}  // namespace

extern "C" int grx_est_forward(const grx_est_net* net, int N, int D, const float* x, int P, const float* pri, const int* target_cols,
                               float* out, float* targets, void* stream) {
    if (!net || !x || !out || N < 1 || D < 1 || D > GRX_EST_MAX_INPUT) return -1;
    if (net->n_layers < 2 || net->n_layers > GRX_EST_MAX_LAYERS) return -1;
    const int nl = net->n_layers, E = net->widths[nl - 1];
    if (E < 1 || E > GRX_EST_MAX_TARGETS) return -1;
    for (int l = 0; l < nl; ++l)
        if (!net->W[l] || net->widths[l] < 1 || net->widths[l] > GRX_EST_MAX_WIDTH) return -1;
    if ((long long)N * (D + E) >= (1ll << 31)) return -1;
    const uintptr_t xb = (uintptr_t)x, xe = xb + (size_t)N * D * sizeof(float);
    const uintptr_t ob = (uintptr_t)out, oe = ob + (size_t)N * (D + E) * sizeof(float);
    if (xb < oe && ob < xe) return -1;
    EstArgs a;
    a.net = *net;
    const bool want_targets = pri != nullptr && targets != nullptr;
    for (int e = 0; e < GRX_EST_MAX_TARGETS; ++e) a.cols[e] = 0;
    if (want_targets) {
        if (P < 1 || !target_cols) return -1;
        for (int e = 0; e < E; ++e) {
            if (target_cols[e] < 0 || target_cols[e] >= P) return -1;
            a.cols[e] = target_cols[e];
        }
    }
    int K = D;
    for (int l = 0; l < GRX_EST_MAX_LAYERS; ++l) {
        a.vec[l] = 0;
        if (l >= nl) { a.net.widths[l] = 0; a.net.W[l] = nullptr; a.net.bias[l] = nullptr; continue; }
        if (K % 4 == 0 && (uintptr_t)net->W[l] % 16 == 0) a.vec[l] |= 1;
        if (l == 0 && D % 4 == 0 && (uintptr_t)x % 16 == 0) a.vec[l] |= 2;
        K = net->widths[l];
    }
    hipLaunchKernelGGL(est_forward_kernel, dim3((N + ES_BM - 1) / ES_BM), dim3(256), 0, (hipStream_t)stream, a, N, D, x, P,
                       want_targets ? pri : (const float*)nullptr, out, want_targets ? targets : (float*)nullptr);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
