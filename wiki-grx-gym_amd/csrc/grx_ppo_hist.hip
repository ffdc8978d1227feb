// grx_ppo_hist.hip -- observation history for the PPO rollout (include/grx_ppo.h, grx_obs_history_push).
// The stacked row of env n is H frames of width D, oldest first: dst[n] = concat(src[n][D:], obs[n]), or obs[n] repeated H times where
// the env's episode just ended (or for every row: the first frame).  ONE launch, pure copies: the same inputs give the same bytes.
//
// One WAVE per row, four rows per block: the row index and the row's `dones` byte are wave-uniform, so no element needs an integer
// division to find its row, and the byte is read once per row.  Lane l handles elements l, l + 64, ... of the row: every load and
// store instruction of a wave covers 64 consecutive dwords (256 B), whatever the alignment of the row -- D = 39 makes source and
// destination rows mutually misaligned, so nothing wider than a dword is assumed.  A refilled row needs (element index) mod D: lane l
// starts at l mod D (one division per lane, none per element) and advances by 64 mod D with a conditional subtract.
// No atomics, no LDS, no scratch; src and dst never alias (the entry point refuses that), obs and dst neither.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grx_ppo.h"

namespace {

constexpr int OH_WAVES = 4;   // rows per block

__global__ __launch_bounds__(64 * OH_WAVES) void obs_history_push_kernel(int N, int D, int W, const float* __restrict__ obs,
                                                                         const unsigned char* __restrict__ dones, int fill_all,
                                                                         const float* __restrict__ src, float* __restrict__ dst) {
    const int lane = threadIdx.x & 63;
    const int n = __builtin_amdgcn_readfirstlane((int)blockIdx.x * OH_WAVES + (int)(threadIdx.x >> 6));   // wave-uniform
    if (n >= N) return;
    const float* x = obs + (size_t)n * D;
    float* out = dst + (size_t)n * W;
    const bool fill = fill_all || dones[n] != 0;   // (fill_all != 0 whenever dones is NULL: grx_obs_history_push)
    if (fill) {
        const int step = 64 % D;
        int c = lane % D;
        for (int j = lane; j < W; j += 64) {
            out[j] = x[c];
            c += step;
            c = c >= D ? c - D : c;
        }
    } else {
        const int keep = W - D;            // the H - 1 newest frames of the old row move one frame down
        const float* old = src + (size_t)n * W + D;
#pragma unroll 4
        for (int j = lane; j < W; j += 64) out[j] = j < keep ? old[j] : x[j - keep];
    }
}

inline bool overlap(const void* a, const void* b, size_t bytes_a, size_t bytes_b) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + bytes_b && pb < pa + bytes_a;
}

}  // namespace

extern "C" int grx_obs_history_push(int N, int D, int H, const float* obs, const unsigned char* dones, int fill_all, const float* src,
                                    float* dst, void* stream) {
    if (N < 1 || D < 1 || H < 1 || (long long)N * H * D >= (1ll << 31) || !obs || !dst) return -1;
    const int fill = (fill_all != 0 || !dones) ? 1 : 0;
    const bool shift = !fill && H > 1;     // some row may read src
    const size_t row_bytes = (size_t)N * H * D * sizeof(float);
    if (shift && !src) return -1;
    if (src && (src == dst || overlap(src, dst, row_bytes, row_bytes))) return -1;
    if (overlap(obs, dst, (size_t)N * D * sizeof(float), row_bytes)) return -1;
    hipLaunchKernelGGL(obs_history_push_kernel, dim3((N + OH_WAVES - 1) / OH_WAVES), dim3(64 * OH_WAVES), 0, (hipStream_t)stream, N, D, H * D, obs, dones,
                       fill, src, dst);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
