// grx_ppo_bptt.hip -- one step of the LSTM's backward through time in ONE launch (include/grx_ppo_bptt.h grx_lstm_bptt_step):
//     s[r][j]  = sum over k = 0 .. 4H-1 of dG_next[r][k] W_hh[k][j]       one k-ordered fmaf chain from +0; +0 for a row whose NEXT step was reset
//     dh       = dh_out + s
//     (dG, dc') = grx_lstm_cell_backward's formulas on dh (csrc/grx_ppo_lstm.hip), c' = 0 and dc' = 0 for a row whose own step was reset
// which LSTMSequence.backward spells as a rocBLAS product, an addcmul and the element-wise launch.
//
// A 256-thread block owns 128 rows x 32 NJ hidden units; each of its four waves owns 32 of those rows and keeps NJ 32 x 32 accumulators on
// v_mfma_f32_32x32x2_f32 (exact f32: a k-ordered fmaf chain per output).  The reduction runs over the 4H gate columns, 32 k at a time
// through LDS: a [32 k][128 rows] tile of dG_next (row-major, k contiguous: the cell kernel's fetch with ld = 4H) and a [32 k][32 NJ units]
// tile of W_hh, whose row index already is k (a straight copy); the next chunk's global loads are in flight during the current chunk's
// 16 NJ MFMAs.  Rows beyond M and the rows of a reset_next row are loaded as zero, so their chain is +0 whatever dG_next holds there.
// The element-wise backward is the epilogue on the accumulator: an output's dh sits in one lane and register, nothing is exchanged.
// A row's result depends on that row's inputs only.  No atomics, no scratch; at most 33 KB of static LDS.
// Operand maps as in grx_ppo_lstm.hip: A: lane l holds A[i = l & 31][k = l >> 5]; B: B[k = l >> 5][j = l & 31];
// D: col = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grx_ppo.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int BP_BM = 128, BP_KC = 32, BP_LD = 129;   // the dG_next tile is [k][row], row stride 129

// 128 tile rows x 32 k of dG_next -> registers: thread t, pass p -> tile row 32 p + t / 8, k = k0 + 4 (t % 8) .. + 3 (always inside:
// 4H % 32 == 0).  A negative grow[p] loads zeros (a row beyond M, a row whose next step was reset).  VEC: 16-byte aligned rows
template <bool VEC>
__device__ inline void bp_fetch_a(const float* __restrict__ G, int ld, const int grow[4], int k0, int tid, float4 v[4]) {
    const int kq = k0 + 4 * (tid & 7);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        float4 x = {0.f, 0.f, 0.f, 0.f};
        if (grow[p] >= 0) {
            const float* g = G + (size_t)grow[p] * ld + kq;
            if (VEC) x = *reinterpret_cast<const float4*>(g);
            else { x.x = g[0]; x.y = g[1]; x.z = g[2]; x.w = g[3]; }
        }
        v[p] = x;
    }
}
__device__ inline void bp_stash_a(float* __restrict__ S, int tid, const float4 v[4]) {
    const int kq = 4 * (tid & 7);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        float* s = S + kq * BP_LD + 32 * p + (tid >> 3);
        s[0] = v[p].x; s[BP_LD] = v[p].y; s[2 * BP_LD] = v[p].z; s[3 * BP_LD] = v[p].w;
    }
}
// 32 k x 32 NJ units of W_hh [4H][H] -> registers: quad q = t + 256 p -> k = k0 + q / (8 NJ), units j0 + 4 (q % (8 NJ)) .. + 3; zero beyond H
// (H % 32 == 0: a quad is inside or outside as a whole)
template <int NJ, bool VEC>
__device__ inline void bp_fetch_w(const float* __restrict__ W, int H, int j0, int k0, int tid, float4 v[NJ]) {
#pragma unroll
    for (int p = 0; p < NJ; ++p) {
        const int q = tid + 256 * p, k = k0 + q / (8 * NJ), j = j0 + 4 * (q % (8 * NJ));
        float4 x = {0.f, 0.f, 0.f, 0.f};
        if (j < H) {
            const float* g = W + (size_t)k * H + j;
            if (VEC) x = *reinterpret_cast<const float4*>(g);
            else { x.x = g[0]; x.y = g[1]; x.z = g[2]; x.w = g[3]; }
        }
        v[p] = x;
    }
}
template <int NJ>
__device__ inline void bp_stash_w(float* __restrict__ S, int tid, const float4 v[NJ]) {
#pragma unroll
    for (int p = 0; p < NJ; ++p) {
        const int q = tid + 256 * p;
        float* s = S + (q / (8 * NJ)) * (32 * NJ + 1) + 4 * (q % (8 * NJ));
        s[0] = v[p].x; s[1] = v[p].y; s[2] = v[p].z; s[3] = v[p].w;
    }
}

// DH: the test hook grx_lstm_bptt_dh -- the same reduction, the epilogue writes dh = dh_out + s to `dh` [M][H] and nothing else
template <int NJ, bool VEC, bool DH>
__global__ __launch_bounds__(256) void lstm_bptt_kernel(int M, int H, const float* __restrict__ dGn, const float* __restrict__ Whh,
                                                         const unsigned char* __restrict__ reset_next, const float* __restrict__ dh_out,
                                                         const float* __restrict__ dc_in, const float* __restrict__ acts,
                                                         const float* __restrict__ Cp, const unsigned char* __restrict__ reset,
                                                         float* __restrict__ dG, float* __restrict__ dCp, float* __restrict__ dh) {
    constexpr int WLD = 32 * NJ + 1;
    __shared__ float As[BP_KC * BP_LD], Ws[BP_KC * WLD];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int m0 = blockIdx.x * BP_BM, j0 = blockIdx.y * 32 * NJ;
    f32x16 acc[NJ];
#pragma unroll
    for (int g = 0; g < NJ; ++g)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[g][r] = 0.f;
    if (dGn) {   // (NULL: the sequence's last step, s = +0)
        int arow[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int r = m0 + 32 * p + (tid >> 3);
            arow[p] = (r < M && !(reset_next && reset_next[r] != 0)) ? r : -1;
        }
        const int K = 4 * H, nchunk = K / BP_KC;
        float4 ar[4], wr[NJ];
        bp_fetch_a<VEC>(dGn, K, arow, 0, tid, ar);
        bp_fetch_w<NJ, VEC>(Whh, H, j0, 0, tid, wr);
        const float* xa = As + (lane >> 5) * BP_LD + 32 * wv + (lane & 31);
        const float* wb = Ws + (lane >> 5) * WLD + (lane & 31);
        for (int c = 0; c < nchunk; ++c) {
            bp_stash_a(As, tid, ar); bp_stash_w<NJ>(Ws, tid, wr);
            __syncthreads();
            if (c + 1 < nchunk) {   // in flight during the MFMAs
                bp_fetch_a<VEC>(dGn, K, arow, (c + 1) * BP_KC, tid, ar);
                bp_fetch_w<NJ, VEC>(Whh, H, j0, (c + 1) * BP_KC, tid, wr);
            }
#pragma unroll
            for (int kk = 0; kk < BP_KC / 2; ++kk) {
                const float a = xa[2 * kk * BP_LD];
#pragma unroll
                for (int g = 0; g < NJ; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wb[2 * kk * WLD + 32 * g], acc[g], 0, 0, 0);
            }
            __syncthreads();   // every wave is done with the tiles before the next chunk overwrites them
        }
    }
#pragma unroll
    for (int g = 0; g < NJ; ++g) {
        const int j = j0 + 32 * g + (lane & 31);
        if (j >= H) continue;   // (wave-uniform: H % 32 == 0)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = m0 + 32 * wv + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (row >= M) continue;
            const size_t e = (size_t)row * H + j;
            const float d_h = dh_out[e] + acc[g][r];
            if (DH) { dh[e] = d_h; continue; }
            // grx_lstm_cell_backward's element, operation for operation
            const bool rs = reset && reset[row] != 0;
            const float* a = acts + (size_t)row * 5 * H + j;
            const float i = a[0], f = a[H], gt = a[2 * H], o = a[3 * H], tc = a[4 * H];
            const float cp = rs ? 0.f : Cp[e];
            const float d_o = d_h * tc;
            const float d_c = (dc_in ? dc_in[e] : 0.f) + d_h * o * (1.0f - tc * tc);
            float* q = dG + (size_t)row * 4 * H + j;
            q[0] = d_c * gt * (i * (1.0f - i));
            q[H] = d_c * cp * (f * (1.0f - f));
            q[2 * H] = d_c * i * (1.0f - gt * gt);
            q[3 * H] = d_o * (o * (1.0f - o));
            dCp[e] = rs ? 0.f : d_c * f;
        }
    }
}

inline bool overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + bytes && pb < pa + bytes;
}

inline bool bad_sizes(int M, int H) { return M < 1 || H < 32 || H > 1024 || H % 32 != 0 || (long long)M * 5 * H >= (1ll << 31); }

template <int NJ, bool DH>
int launch_nj(int M, int H, const float* dG_next, const float* W_hh, const unsigned char* reset_next, const float* dh_out, const float* dc_in,
              const float* acts, const float* c_prev, const unsigned char* reset, float* dG, float* dc_prev, float* dh, void* stream) {
    const bool vec = (((uintptr_t)dG_next | (uintptr_t)W_hh) % 16 == 0);
    const dim3 grid((M + BP_BM - 1) / BP_BM, (H + 32 * NJ - 1) / (32 * NJ));
    if (vec) hipLaunchKernelGGL((lstm_bptt_kernel<NJ, true, DH>), grid, dim3(256), 0, (hipStream_t)stream, M, H, dG_next, W_hh, reset_next, dh_out,
                                dc_in, acts, c_prev, reset, dG, dc_prev, dh);
    else hipLaunchKernelGGL((lstm_bptt_kernel<NJ, false, DH>), grid, dim3(256), 0, (hipStream_t)stream, M, H, dG_next, W_hh, reset_next, dh_out,
                            dc_in, acts, c_prev, reset, dG, dc_prev, dh);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// the block's width in hidden units, measured: 32 everywhere -- 128 x 32 blocks are the most blocks, and one accumulator
// per wave already meets the 32x32x2 issue rate
inline int default_tile(int, int) { return 32; }

}  // namespace

extern "C" int grx_lstm_bptt_step_tile(int tile_units, int M, int H, const float* dG_next, const float* W_hh, const unsigned char* reset_next,
                                       const float* dh_out, const float* dc_in, const float* acts, const float* c_prev,
                                       const unsigned char* reset, float* dG, float* dc_prev, void* stream) {
    if (bad_sizes(M, H) || !dh_out || !acts || !c_prev || !dG || !dc_prev || (dG_next && !W_hh)) return -1;
    if (dG_next && overlap(dG, dG_next, (size_t)M * 4 * H * sizeof(float))) return -1;
    if (tile_units == 0) tile_units = default_tile(M, H);
    switch (tile_units) {
    case 32: return launch_nj<1, false>(M, H, dG_next, W_hh, reset_next, dh_out, dc_in, acts, c_prev, reset, dG, dc_prev, nullptr, stream);
    case 64: return launch_nj<2, false>(M, H, dG_next, W_hh, reset_next, dh_out, dc_in, acts, c_prev, reset, dG, dc_prev, nullptr, stream);
    case 128: return launch_nj<4, false>(M, H, dG_next, W_hh, reset_next, dh_out, dc_in, acts, c_prev, reset, dG, dc_prev, nullptr, stream);
    }
    return -1;
}

extern "C" int grx_lstm_bptt_step(int M, int H, const float* dG_next, const float* W_hh, const unsigned char* reset_next, const float* dh_out,
                                  const float* dc_in, const float* acts, const float* c_prev, const unsigned char* reset, float* dG,
                                  float* dc_prev, void* stream) {
    return grx_lstm_bptt_step_tile(0, M, H, dG_next, W_hh, reset_next, dh_out, dc_in, acts, c_prev, reset, dG, dc_prev, stream);
}

extern "C" int grx_lstm_bptt_dh(int M, int H, const float* dG_next, const float* W_hh, const unsigned char* reset_next, const float* dh_out,
                                float* dh, void* stream) {
    if (bad_sizes(M, H) || !dh_out || !dh || (dG_next && !W_hh)) return -1;
    if (dG_next && overlap(dh, dG_next, (size_t)M * 4 * H * sizeof(float))) return -1;
    switch (default_tile(M, H)) {
    case 64: return launch_nj<2, true>(M, H, dG_next, W_hh, reset_next, dh_out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, dh, stream);
    case 128: return launch_nj<4, true>(M, H, dG_next, W_hh, reset_next, dh_out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, dh, stream);
    }
    return launch_nj<1, true>(M, H, dG_next, W_hh, reset_next, dh_out, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, dh, stream);
}
