// grx_ppo_rnd.hip -- the intrinsic reward of random network distillation (include/grx_ppo.h, grx_rnd_reward; rl/rnd.py).
// One rollout step, three launches in stream order:
//   rows  : r[n] = sqrt(sum_e (targ[n][e] - pred[n][e])^2);  ret[n] = fmaf(gamma, ret[n], r[n]);  per slab of RR_ROWS rows one CENTRED
//           triple (n, mean, M2) of the new ret (the slab's mean is formed before its squares are summed, as grx_obs_norm_moments does)
//   merge : grx_obs_norm_merge with one column -- ONE block merges the triples in index order and applies the running update in place
//   apply : x = weight * r[n] / (std + eps) with the std just written;  intrinsic[n] = x;  rewards[n] += x
// Row-to-lane map of `rows`: G = the power of two >= E (at most 64) consecutive lanes share a row, lane j of them takes the elements
// j, j + G, ... -- with E <= 64 one element per lane, so a wave's load covers 64 / G consecutive rows, which are (E == G) or nearly are
// 64 consecutive dwords, whatever E's alignment.  A lane adds its (at most four) squares in index order, the G lanes add in an xor
// butterfly: the order is a function of E alone, a row's r depends neither on N nor on its neighbours.  r travels from the first to
// the third launch in `intrinsic`.  No atomics, no scratch; LDS: the slab's RR_ROWS norms and two partial sums.
// Strict IEEE arithmetic (the library's flags): the square root and the division are correctly rounded, as in the torch spelling.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grx_ppo.h"

namespace {

constexpr int RR_ROWS = 128;           // rows per slab = per block: a function of nothing, so the slab geometry is one of N only
constexpr int RR_THR = 256;            // threads per block
constexpr int RR_MAX_E = 256;
constexpr int RR_MAX_ROWS = 1 << 24;   // a triple carries its n as a float: exact up to here (grx_obs_norm's limit)

__device__ inline float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;   // lane 0 holds the sum
}

template <int G>
__global__ __launch_bounds__(RR_THR) void rnd_rows_kernel(int N, int E, const float* __restrict__ pred, const float* __restrict__ targ, float gamma,
                                                          float* __restrict__ ret, float* __restrict__ r_out, float* __restrict__ raw,
                                                          float* __restrict__ partials) {
    __shared__ float rs[RR_ROWS];
    __shared__ float red[2];
    constexpr int RPP = RR_THR / G;                              // rows per pass
    constexpr int PASSES = RPP >= RR_ROWS ? 1 : RR_ROWS / RPP;
    constexpr int KMAX = G == 64 ? RR_MAX_E / 64 : 1;            // elements per lane: E <= G below 64 lanes
    const int tid = threadIdx.x, sub = tid % G, rloc = tid / G;
    const int r0 = blockIdx.x * RR_ROWS;
    const int nr = min(RR_ROWS, N - r0);
#pragma unroll 4
    for (int p = 0; p < PASSES; ++p) {
        const int rl = p * RPP + rloc;
        float acc = 0.f;
        if (rl < nr) {
            const size_t base = (size_t)(r0 + rl) * E;
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                const int e = sub + G * k;
                if (e < E) {
                    const float d = targ[base + e] - pred[base + e];
                    acc = fmaf(d, d, acc);
                }
            }
        }
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (sub == 0 && rl < nr) rs[rl] = sqrtf(acc);
    }
    __syncthreads();
    const int lane = tid & 63, w = tid >> 6;
    const bool live = tid < nr;   // (nr <= RR_ROWS: waves 0 and 1)
    float v = 0.f;
    if (live) {
        const int n = r0 + tid;
        const float r = rs[tid];
        v = fmaf(gamma, ret[n], r);
        ret[n] = v;
        r_out[n] = r;
        if (raw) raw[n] = r;
    }
    if (w < 2) {
        const float s = wave_sum(v);
        if (lane == 0) red[w] = s;
    }
    __syncthreads();
    const float mean = (red[0] + red[1]) / (float)nr;
    __syncthreads();
    if (w < 2) {
        const float d = v - mean;
        const float q = wave_sum(live ? d * d : 0.f);
        if (lane == 0) red[w] = q;
    }
    __syncthreads();
    if (tid == 0) {
        float* p = partials + (size_t)blockIdx.x * 3;
        p[0] = (float)nr;
        p[1] = mean;
        p[2] = red[0] + red[1];
    }
}

__global__ __launch_bounds__(256) void rnd_apply_kernel(int N, float weight, float eps, const float* __restrict__ std_, float* __restrict__ intrinsic,
                                                        float* __restrict__ rewards) {
    const float scale = std_[0] + eps;
    const int step = gridDim.x * 256;
    for (int n = blockIdx.x * 256 + threadIdx.x; n < N; n += step) {
        const float x = weight * intrinsic[n] / scale;   // (intrinsic holds r since the first launch)
        intrinsic[n] = x;
        rewards[n] += x;
    }
}

inline int nslabs(int N) { return (N + RR_ROWS - 1) / RR_ROWS; }
inline bool bad_rows(int N) { return N < 1 || N > RR_MAX_ROWS; }

template <int G>
inline void launch_rows(int N, int E, const float* pred, const float* targ, float gamma, float* ret, float* r_out, float* raw, float* partials,
                        hipStream_t st) {
    hipLaunchKernelGGL(rnd_rows_kernel<G>, dim3(nslabs(N)), dim3(RR_THR), 0, st, N, E, pred, targ, gamma, ret, r_out, raw, partials);
}

}  // namespace

extern "C" int grx_rnd_reward_partials_size(int N) { return bad_rows(N) ? 0 : nslabs(N) * 3; }

extern "C" int grx_rnd_reward(int N, int E, const float* pred, const float* targ, float gamma, float weight, float eps, float* ret,
                              long long* count, float* mean, float* var, float* std, float* rewards, float* intrinsic, float* raw,
                              float* partials, void* stream) {
    if (bad_rows(N) || E < 1 || E > RR_MAX_E || (long long)N * E >= (1ll << 31)) return -1;
    if (!pred || !targ || !ret || !count || !mean || !var || !std || !rewards || !intrinsic || !partials || ((uintptr_t)partials & 7)) return -1;
    hipStream_t st = (hipStream_t)stream;
    if (E <= 1) launch_rows<1>(N, E, pred, targ, gamma, ret, intrinsic, raw, partials, st);
    else if (E <= 2) launch_rows<2>(N, E, pred, targ, gamma, ret, intrinsic, raw, partials, st);
    else if (E <= 4) launch_rows<4>(N, E, pred, targ, gamma, ret, intrinsic, raw, partials, st);
    else if (E <= 8) launch_rows<8>(N, E, pred, targ, gamma, ret, intrinsic, raw, partials, st);
    else if (E <= 16) launch_rows<16>(N, E, pred, targ, gamma, ret, intrinsic, raw, partials, st);
    else if (E <= 32) launch_rows<32>(N, E, pred, targ, gamma, ret, intrinsic, raw, partials, st);
    else launch_rows<64>(N, E, pred, targ, gamma, ret, intrinsic, raw, partials, st);
    if (hipGetLastError() != hipSuccess) return -2;
    const int rc = grx_obs_norm_merge(nslabs(N), 1, 3, partials, count, mean, var, std, stream);
    if (rc) return rc < 0 ? rc - 1 : -3;
    const int blocks = (N + 255) / 256 < 1024 ? (N + 255) / 256 : 1024;
    hipLaunchKernelGGL(rnd_apply_kernel, dim3(blocks), dim3(256), 0, st, N, weight, eps, (const float*)std, intrinsic, rewards);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}
