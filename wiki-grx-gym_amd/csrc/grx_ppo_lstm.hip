// grx_ppo_lstm.hip -- the LSTM cell of the recurrent actor-critic (include/grx_ppo.h grx_lstm_cell / grx_lstm_cell_backward).
// torch.nn.LSTM's formulas and gate order, one layer:
//     G = x W_ih^T + h' W_hh^T + b_ih + b_hh       G = [i | f | g | o], each H wide
//     i, f, o = sigmoid(.)   g = tanh(.)           c = f c' + i g      h = o tanh(c)
// with (h', c') the previous state, taken as ZERO for a row whose `reset` byte is set: the done-reset of the rollout rides on the cell.
//
// grx_lstm_cell is ONE launch.  A 256-thread block owns 128 rows x 32 hidden units; each of its four waves owns 32 of those rows and keeps
// FOUR 32 x 32 accumulators -- the i, f, g and o tiles of its rows and the block's units -- on v_mfma_f32_32x32x2_f32 (exact f32: a
// k-ordered fmaf chain per output).  The reduction runs over x (k = 0 .. D-1) and then over h' (k = 0 .. H-1), 32 k at a time through
// LDS: a [32 k][128 rows] tile of x or h' and a [32 k][4 gates x 32 units] tile of W_ih or W_hh, the next chunk's global loads in flight
// during the current chunk's 64 MFMAs.  Rows beyond M, k beyond D and the h' of a reset row are loaded as zero (x * 0 added to an
// accumulator leaves it as it is).  Bias, activations and the state update are the epilogue: all four gates of an output sit in the same
// lane and register of the four accumulators, so nothing is exchanged.  A row's result depends on that row's inputs only -- not on M,
// not on the rows beside it.  No atomics, no scratch; 33 KB of static LDS (mlp_layer_kernel of grx_ppo.hip keeps 65 KB).
// Operand maps as in grx_ppo.hip: A: lane l holds A[i = l & 31][k = l >> 5]; B: B[k = l >> 5][j = l & 31];
// D: col = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grx_ppo.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int LS_BM = 128, LS_BJ = 32, LS_KC = 32, LS_LD = 129;   // LDS tiles are [k][row], row stride 129

__device__ inline float sigmoid1(float x) { return 1.0f / (1.0f + expf(-x)); }

// 128 tile rows x 32 k of a row-major matrix -> registers: thread t, pass p -> tile row 32 p + t / 8, k = k0 + 4 (t % 8) .. + 3.
// The tile row's global row is grow[p]; a negative grow[p] loads zeros (a row beyond the matrix, a reset row).  Zero beyond ld.
// VEC: rows are 16-byte aligned (ld % 4 == 0, base pointer aligned)
template <bool VEC>
__device__ inline void ls_fetch(const float* __restrict__ G, int ld, const int grow[4], int k0, int tid, float4 v[4]) {
    const int kq = k0 + 4 * (tid & 7);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        float4 x = {0.f, 0.f, 0.f, 0.f};
        if (grow[p] >= 0) {
            const float* g = G + (size_t)grow[p] * ld + kq;
            if (VEC) { if (kq < ld) x = *reinterpret_cast<const float4*>(g); }   // (ld % 4 == 0: a quad is inside or outside as a whole)
            else { if (kq < ld) x.x = g[0]; if (kq + 1 < ld) x.y = g[1]; if (kq + 2 < ld) x.z = g[2]; if (kq + 3 < ld) x.w = g[3]; }
        }
        v[p] = x;
    }
}
__device__ inline void ls_stash(float* __restrict__ S, int tid, const float4 v[4]) {
    const int kq = 4 * (tid & 7);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        float* s = S + kq * LS_LD + 32 * p + (tid >> 3);
        s[0] = v[p].x; s[LS_LD] = v[p].y; s[2 * LS_LD] = v[p].z; s[3 * LS_LD] = v[p].w;
    }
}

// PRE: the test hook grx_lstm_cell_preact -- the same reduction, the epilogue writes G (biases added) to `pre` [M][4H] and nothing else
template <bool VEC, bool PRE>
__global__ __launch_bounds__(256) void lstm_cell_kernel(int M, int D, int H, const float* __restrict__ X, const float* __restrict__ Hp,
                                                         const float* __restrict__ Cp, const unsigned char* __restrict__ reset,
                                                         const float* __restrict__ Wih, const float* __restrict__ Whh,
                                                         const float* __restrict__ bih, const float* __restrict__ bhh,
                                                         float* __restrict__ Hn, float* __restrict__ Cn, float* __restrict__ acts,
                                                         float* __restrict__ pre) {
    __shared__ float Xs[LS_KC * LS_LD], Ws[LS_KC * LS_LD];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int m0 = blockIdx.x * LS_BM, j0 = blockIdx.y * LS_BJ;
    // the global rows behind this thread's four tile rows: of x, of h' (none where the row is reset) and of W (pass p = gate p)
    int xrow[4], hrow[4], wrow[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int r = m0 + 32 * p + (tid >> 3);
        xrow[p] = r < M ? r : -1;
        hrow[p] = (r < M && !(reset && reset[r] != 0)) ? r : -1;
        wrow[p] = p * H + j0 + (tid >> 3);   // (H % 32 == 0: always inside the 4H rows)
    }
    f32x16 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[g][r] = 0.f;
    const int nx = (D + LS_KC - 1) / LS_KC, nchunk = nx + H / LS_KC;   // x's chunks first, then h's
    float4 xr[4], wr[4];
    ls_fetch<VEC>(X, D, xrow, 0, tid, xr);
    ls_fetch<VEC>(Wih, D, wrow, 0, tid, wr);
    const float* xa = Xs + (lane >> 5) * LS_LD + 32 * wv + (lane & 31);
    const float* wb = Ws + (lane >> 5) * LS_LD + (lane & 31);
    for (int c = 0; c < nchunk; ++c) {
        ls_stash(Xs, tid, xr); ls_stash(Ws, tid, wr);
        __syncthreads();
        const int n = c + 1;
        if (n < nchunk) {   // in flight during the MFMAs
            if (n < nx) { ls_fetch<VEC>(X, D, xrow, n * LS_KC, tid, xr); ls_fetch<VEC>(Wih, D, wrow, n * LS_KC, tid, wr); }
            else { ls_fetch<VEC>(Hp, H, hrow, (n - nx) * LS_KC, tid, xr); ls_fetch<VEC>(Whh, H, wrow, (n - nx) * LS_KC, tid, wr); }
        }
#pragma unroll
        for (int kk = 0; kk < LS_KC / 2; ++kk) {   // (the tiles are zero beyond D)
            const float a = xa[2 * kk * LS_LD];
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wb[2 * kk * LS_LD + 32 * g], acc[g], 0, 0, 0);
        }
        __syncthreads();   // every wave is done with the tiles before the next chunk overwrites them
    }
    const int j = j0 + (lane & 31);
    float b[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) b[g] = bih[g * H + j] + bhh[g * H + j];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + 32 * wv + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row >= M) continue;
        const float gi = acc[0][r] + b[0], gf = acc[1][r] + b[1], gg = acc[2][r] + b[2], go = acc[3][r] + b[3];
        if (PRE) {
            float* o = pre + (size_t)row * 4 * H + j;
            o[0] = gi; o[H] = gf; o[2 * H] = gg; o[3 * H] = go;
            continue;
        }
        const size_t e = (size_t)row * H + j;
        const float cp = (reset && reset[row] != 0) ? 0.f : Cp[e];
        const float i = sigmoid1(gi), f = sigmoid1(gf), g = tanhf(gg), o = sigmoid1(go);
        const float c = f * cp + i * g;
        const float tc = tanhf(c);
        Cn[e] = c;
        Hn[e] = o * tc;
        if (acts) {
            float* a = acts + (size_t)row * 5 * H + j;
            a[0] = i; a[H] = f; a[2 * H] = g; a[3 * H] = o; a[4 * H] = tc;
        }
    }
}

// The element-wise half of the backward, one thread per (row, unit): from dh, the incoming dc, the saved activations and c',
//     do = dh tanh(c)      dc = dc_in + dh o (1 - tanh(c)^2)      di = dc g      dg = dc i      df = dc c'      dc' = dc f
//     dG = [ di i (1 - i) | df f (1 - f) | dg (1 - g^2) | do o (1 - o) ]
// with c' = 0 and dc' = 0 for a reset row.
__global__ __launch_bounds__(256) void lstm_cell_backward_kernel(int M, int H, const float* __restrict__ dh, const float* __restrict__ dc_in,
                                                                  const float* __restrict__ acts, const float* __restrict__ Cp,
                                                                  const unsigned char* __restrict__ reset, float* __restrict__ dG,
                                                                  float* __restrict__ dCp) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)M * H) return;
    const int row = (int)(e / H), j = (int)(e - (long long)row * H);
    const bool rs = reset && reset[row] != 0;
    const float* a = acts + (size_t)row * 5 * H + j;
    const float i = a[0], f = a[H], g = a[2 * H], o = a[3 * H], tc = a[4 * H];
    const float cp = rs ? 0.f : Cp[e];
    const float d_h = dh[e];
    const float d_o = d_h * tc;
    const float d_c = (dc_in ? dc_in[e] : 0.f) + d_h * o * (1.0f - tc * tc);
    float* q = dG + (size_t)row * 4 * H + j;
    q[0] = d_c * g * (i * (1.0f - i));
    q[H] = d_c * cp * (f * (1.0f - f));
    q[2 * H] = d_c * i * (1.0f - g * g);
    q[3 * H] = d_o * (o * (1.0f - o));
    dCp[e] = rs ? 0.f : d_c * f;
}

inline bool overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + bytes && pb < pa + bytes;
}

inline bool bad_sizes(int M, int D, int H) { return M < 1 || D < 1 || H < 32 || H > 1024 || H % 32 != 0 || (long long)M * 5 * H >= (1ll << 31); }

template <bool PRE>
int launch_cell(int M, int D, int H, const float* x, const float* h_prev, const float* c_prev, const unsigned char* reset, const float* W_ih,
                const float* W_hh, const float* b_ih, const float* b_hh, float* h, float* c, float* acts, float* pre, void* stream) {
    const bool vec = D % 4 == 0 && (((uintptr_t)x | (uintptr_t)h_prev | (uintptr_t)W_ih | (uintptr_t)W_hh) % 16 == 0);
    const dim3 grid((M + LS_BM - 1) / LS_BM, H / LS_BJ);
    if (vec) hipLaunchKernelGGL((lstm_cell_kernel<true, PRE>), grid, dim3(256), 0, (hipStream_t)stream, M, D, H, x, h_prev, c_prev, reset, W_ih, W_hh,
                                b_ih, b_hh, h, c, acts, pre);
    else hipLaunchKernelGGL((lstm_cell_kernel<false, PRE>), grid, dim3(256), 0, (hipStream_t)stream, M, D, H, x, h_prev, c_prev, reset, W_ih, W_hh,
                            b_ih, b_hh, h, c, acts, pre);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace

extern "C" int grx_lstm_cell(int M, int D, int H, const float* x, const float* h_prev, const float* c_prev, const unsigned char* reset,
                             const float* W_ih, const float* W_hh, const float* b_ih, const float* b_hh, float* h, float* c, float* acts,
                             void* stream) {
    if (bad_sizes(M, D, H) || !x || !h_prev || !c_prev || !W_ih || !W_hh || !b_ih || !b_hh || !h || !c) return -1;
    const size_t bytes = (size_t)M * H * sizeof(float);
    if (overlap(h, h_prev, bytes) || overlap(c, c_prev, bytes)) return -1;
    return launch_cell<false>(M, D, H, x, h_prev, c_prev, reset, W_ih, W_hh, b_ih, b_hh, h, c, acts, nullptr, stream);
}

extern "C" int grx_lstm_cell_preact(int M, int D, int H, const float* x, const float* h_prev, const unsigned char* reset, const float* W_ih,
                                    const float* W_hh, const float* b_ih, const float* b_hh, float* G, void* stream) {
    if (bad_sizes(M, D, H) || !x || !h_prev || !W_ih || !W_hh || !b_ih || !b_hh || !G) return -1;
    return launch_cell<true>(M, D, H, x, h_prev, nullptr, reset, W_ih, W_hh, b_ih, b_hh, nullptr, nullptr, nullptr, G, stream);
}

extern "C" int grx_lstm_cell_backward(int M, int H, const float* dh, const float* dc_in, const float* acts, const float* c_prev,
                                      const unsigned char* reset, float* dG, float* dc_prev, void* stream) {
    if (bad_sizes(M, 1, H) || !dh || !acts || !c_prev || !dG || !dc_prev) return -1;
    const long long n = (long long)M * H;
    hipLaunchKernelGGL(lstm_cell_backward_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, M, H, dh, dc_in, acts, c_prev,
                       reset, dG, dc_prev);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
