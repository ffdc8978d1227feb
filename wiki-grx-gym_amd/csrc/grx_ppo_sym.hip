// grx_ppo_sym.hip -- the mirrored minibatch of PPO's left-right symmetry (include/grx_ppo.h, grx_sym_gather_rows).
// grx_ppo_gather_rows's contract with a second half: dst[t][r] = src[t][idx[r]], and dst[t][mb + r] the same row again -- copied
// (mode 1) or mapped (mode 2): dst[t][mb + r][j] = fmaf(scale[t][j], src[t][idx[r]][perm[t][j]], offset[t][j]).  ONE launch for every
// tensor and both halves; pure copies and one fmaf per element: the same inputs give the same bytes, whatever mb is.
//
// A block works on rows of ONE tensor (blockIdx.y), one WAVE per row, four rows per pass.  It stages the tensor's perm / scale / offset
// in LDS once, then walks its rows: a wave reads its source row from HBM ONCE, lane l elements l, l + 64, ... (every load of a wave
// covers 64 consecutive dwords, whatever the row's alignment -- widths such as 39 leave rows mutually misaligned, so nothing wider than
// a dword is assumed), writes the first half straight from the registers, parks the row in its LDS slot, and after the barrier forms the
// second half from LDS: the permuted read never goes to HBM, and both output rows are written coalesced.
// LDS layout: the row slot is linear.  ds_read_b32 banks are (dword address) mod 32 per 32-lane half: 32 consecutive j read
// row[perm[j]], and a mirror map permutes within short windows (two leg blocks of 5 joints, a scan line of 11 samples, one frame of a
// history), so the 32 addresses of a half lie in a window barely wider than 32 dwords: conflict-free but for the few entries that
// straddle the window's edge (2-way at worst).  An arbitrary permutation is still correct, only slower.  perm / scale / offset are read
// at j itself: conflict-free.  No atomics, no scratch; the entry point refuses what the staging cannot hold.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grx_ppo.h"

namespace {

constexpr int SG_WAVES = 4;   // rows per pass of a block

struct SymGatherArgs {
    const float* src[GRX_PPO_GATHER_MAX]; float* dst[GRX_PPO_GATHER_MAX];
    const int* perm[GRX_PPO_GATHER_MAX]; const float* scale[GRX_PPO_GATHER_MAX]; const float* offset[GRX_PPO_GATHER_MAX];
    int width[GRX_PPO_GATHER_MAX], mode[GRX_PPO_GATHER_MAX];
};

__global__ __launch_bounds__(64 * SG_WAVES) void sym_gather_rows_kernel(SymGatherArgs a, const long long* __restrict__ idx, int mb, int wmax) {
    extern __shared__ float lds[];   // [scale wmax | offset wmax | perm wmax | SG_WAVES row slots of wmax]
    const int t = blockIdx.y, w = a.width[t], mode = a.mode[t];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* s_scale = lds;
    float* s_offset = lds + wmax;
    int* s_perm = (int*)(lds + 2 * wmax);
    float* s_row = lds + (3 + wave) * wmax;
    const float* __restrict__ src = a.src[t];
    float* __restrict__ dst = a.dst[t];
    if (mode == 2) {
        const int* perm = a.perm[t];
        const float *scale = a.scale[t], *offset = a.offset[t];
        for (int j = threadIdx.x; j < w; j += 64 * SG_WAVES) {
            s_perm[j] = perm[j];
            s_scale[j] = scale[j];
            s_offset[j] = offset ? offset[j] : 0.0f;
        }
    }
    const bool affine = mode == 2 && a.offset[t] != nullptr;
    // (the trip count is the same for every wave of the block: the barriers below are reached by all of them)
    for (int base = blockIdx.x * SG_WAVES; base < mb; base += gridDim.x * SG_WAVES) {
        const int r = base + wave;
        const bool live = r < mb;
        if (live) {
            const long long srow = idx ? idx[r] : (long long)r;
            const float* x = src + (size_t)srow * w;
            float* out = dst + (size_t)r * w;
            float* out2 = dst + ((size_t)mb + r) * w;
            for (int j = lane; j < w; j += 64) {
                const float v = x[j];
                out[j] = v;
                if (mode == 1) out2[j] = v;
                else if (mode == 2) s_row[j] = v;
            }
        }
        __syncthreads();   // the row slots (and, first pass, the map) are complete
        if (live && mode == 2) {
            float* out2 = dst + ((size_t)mb + r) * w;
            if (affine) for (int j = lane; j < w; j += 64) out2[j] = fmaf(s_scale[j], s_row[s_perm[j]], s_offset[j]);
            else for (int j = lane; j < w; j += 64) out2[j] = s_scale[j] * s_row[s_perm[j]];
        }
        __syncthreads();   // every slot has been read before the next pass overwrites it
    }
}

}  // namespace

extern "C" int grx_sym_gather_rows(int n_tensors, const float* const* src, float* const* dst, const int* widths, const int* modes,
                                   const int* const* perm, const float* const* scale, const float* const* offset, const long long* idx,
                                   int mb, void* stream) {
    if (n_tensors < 1 || n_tensors > GRX_PPO_GATHER_MAX || mb < 1 || !src || !dst || !widths || !modes) return -1;
    SymGatherArgs a;
    int wmax = 1;
    for (int t = 0; t < GRX_PPO_GATHER_MAX; ++t) {
        const int u = t < n_tensors ? t : 0;
        if (!src[u] || !dst[u] || widths[u] < 1 || widths[u] > GRX_SYM_MAX_WIDTH || modes[u] < 0 || modes[u] > 2) return -1;
        if (modes[u] == 2 && (!perm || !scale || !perm[u] || !scale[u])) return -1;
        a.src[t] = src[u]; a.dst[t] = dst[u]; a.width[t] = widths[u]; a.mode[t] = modes[u];
        a.perm[t] = modes[u] == 2 ? perm[u] : nullptr;
        a.scale[t] = modes[u] == 2 ? scale[u] : nullptr;
        a.offset[t] = (modes[u] == 2 && offset) ? offset[u] : nullptr;
        if (widths[u] > wmax) wmax = widths[u];
    }
    const int passes = (mb + SG_WAVES - 1) / SG_WAVES;
    const int bx = passes < 1024 ? passes : 1024;
    const size_t lds_bytes = (size_t)(3 + SG_WAVES) * wmax * sizeof(float);   // <= 56 KiB at GRX_SYM_MAX_WIDTH
    hipLaunchKernelGGL(sym_gather_rows_kernel, dim3(bx, n_tensors), dim3(64 * SG_WAVES), lds_bytes, (hipStream_t)stream, a, idx, mb, wmax);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
