// grx_ppo_distill.hip -- teacher-student policy distillation (include/grx_ppo.h, grx_distill_*; rl/distillation.py).
//
// grx_distill_loss: the behaviour loss between the student's and the teacher's mean actions, mean over all batch * A elements, and its
// gradient with respect to the student's, in two launches.  mse: e = d^2, de = 2 d; huber (delta 1): e = |d| <= 1 ? d^2 / 2 : |d| - 1/2,
// de = clamp(d, -1, 1); d = student - teacher.  The two matrices are contiguous, so the kernel walks them as one flat array of
// n = batch * A dwords: block b owns elements [b * DL_CHUNK, (b + 1) * DL_CHUNK), thread t of it elements t, t + 256, ... -- every load
// and store instruction of a wave covers 64 consecutive dwords, whatever A is.  The gradient is fp32: one subtraction and one product with
// the rounded constant 2 / n (1 / n).  The element's loss and every sum are double: a thread adds its DL_PER elements in index order, a
// wave its 64 lanes in a shuffle tree, thread 0 the block's four waves in wave order -> partials[b]; the second launch (one wave) gives
// lane l the partials l, l + 64, ... in order, then the same tree.  The order of every sum is a function of n alone: the same inputs
// give the same bytes.  A NaN anywhere reaches out[0].  No atomics, no scratch; LDS: four doubles.
//
// grx_distill_store: one rollout step of a distillation run in ONE launch -- the student's input row, the label row and the dones bytes
// into the storage rows of this step, and the runner's running episode reward / length (the arithmetic of grx_ppo_store_transition).
// Pure dword copies over the flat (N, D) and (N, A) blocks: with D = 39 the storage row of a step starts on a 4-byte boundary only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grx_ppo.h"

namespace {

constexpr int DL_THR = 256;              // threads per block
constexpr int DL_PER = 8;                // elements per thread
constexpr int DL_CHUNK = DL_THR * DL_PER;

__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;   // lane 0 holds the sum
}

template <bool HUBER>
__global__ __launch_bounds__(DL_THR) void distill_loss_kernel(int n, float coef, const float* __restrict__ s, const float* __restrict__ t,
                                                              float* __restrict__ d_mu, double* __restrict__ partials) {
    __shared__ double waves[DL_THR / 64];
    const long long base = (long long)blockIdx.x * DL_CHUNK + threadIdx.x;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < DL_PER; ++k) {
        const long long i = base + (long long)k * DL_THR;
        if (i < n) {
            const float sv = s[i], tv = t[i];
            const float d = sv - tv;
            const double dd = (double)sv - (double)tv;   // exact
            if (HUBER) {
                const double ad = fabs(dd);
                acc += ad <= 1.0 ? 0.5 * dd * dd : ad - 0.5;                       // (a NaN takes the second branch and stays one)
                d_mu[i] = d < -1.0f ? -coef : (d > 1.0f ? coef : coef * d);
            } else {
                acc += dd * dd;
                d_mu[i] = coef * d;
            }
        }
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = ((waves[0] + waves[1]) + waves[2]) + waves[3];
}

__global__ __launch_bounds__(64) void distill_loss_finalize(int n, int nblk, const double* __restrict__ partials, float* __restrict__ out) {
    double acc = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 64) acc += partials[b];
    acc = wave_sum(acc);
    if (threadIdx.x == 0) out[0] = (float)(acc / (double)n);
}

struct DistillStoreArgs {
    int N, D, A;
    const float *obs, *labels, *rewards;
    const unsigned char* dones;
    float *st_obs, *st_labels;
    unsigned char* st_dones;
    float *cur_rew, *cur_len, *done_rew, *done_len;
};

__global__ __launch_bounds__(256) void distill_store_kernel(DistillStoreArgs a) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t n_obs = (size_t)a.N * a.D, n_lab = (size_t)a.N * a.A;
    for (size_t i = tid; i < n_obs; i += stride) a.st_obs[i] = a.obs[i];
    for (size_t i = tid; i < n_lab; i += stride) a.st_labels[i] = a.labels[i];
    for (size_t i = tid; i < (size_t)a.N; i += stride) {
        const bool done = a.dones[i] != 0;
        a.st_dones[i] = done ? 1 : 0;
        if (a.cur_rew) {   // grx_ppo_store_transition's episode bookkeeping
            const float cr = a.cur_rew[i] + a.rewards[i], cl = a.cur_len[i] + 1.0f;
            if (done) { a.done_rew[i] = cr; a.done_len[i] = cl; }
            a.cur_rew[i] = done ? 0.0f : cr;
            a.cur_len[i] = done ? 0.0f : cl;
        }
    }
}

inline long long loss_elements(int batch, int A) {
    if (batch < 1 || A < 1) return 0;
    const long long n = (long long)batch * A;
    return n < (1ll << 31) ? n : 0;
}

}  // namespace

extern "C" int grx_distill_loss_partials_size(int batch, int A) {
    const long long n = loss_elements(batch, A);
    return n ? (int)((n + DL_CHUNK - 1) / DL_CHUNK) * 2 : 0;   // one double per block
}

extern "C" int grx_distill_loss(int batch, int A, const float* student_mu, const float* teacher_mu, int huber, float* out, float* d_mu,
                                float* partials, void* stream) {
    const long long n = loss_elements(batch, A);
    if (!n || !student_mu || !teacher_mu || !out || !d_mu || !partials || ((uintptr_t)partials & 7)) return -1;
    const int nblk = (int)((n + DL_CHUNK - 1) / DL_CHUNK);
    hipStream_t st = (hipStream_t)stream;
    if (huber) {
        hipLaunchKernelGGL(distill_loss_kernel<true>, dim3(nblk), dim3(DL_THR), 0, st, (int)n, (float)(1.0 / (double)n), student_mu, teacher_mu, d_mu,
                           (double*)partials);
    } else {
        hipLaunchKernelGGL(distill_loss_kernel<false>, dim3(nblk), dim3(DL_THR), 0, st, (int)n, (float)(2.0 / (double)n), student_mu, teacher_mu, d_mu,
                           (double*)partials);
    }
    hipLaunchKernelGGL(distill_loss_finalize, dim3(1), dim3(64), 0, st, (int)n, nblk, (const double*)partials, out);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int grx_distill_store(int N, int D, int A, const float* obs, const float* labels, const float* rewards, const unsigned char* dones,
                                 float* st_obs, float* st_labels, unsigned char* st_dones,
                                 float* cur_rew, float* cur_len, float* done_rew, float* done_len, void* stream) {
    if (N < 1 || D < 1 || A < 1 || (long long)N * D >= (1ll << 31) || (long long)N * A >= (1ll << 31)) return -1;
    if (!obs || !labels || !dones || !st_obs || !st_labels || !st_dones) return -1;
    if ((cur_rew != nullptr) != (cur_len != nullptr) || (cur_rew != nullptr) != (done_rew != nullptr) || (cur_rew != nullptr) != (done_len != nullptr)) return -1;
    if (cur_rew && !rewards) return -1;
    DistillStoreArgs a = {N, D, A, obs, labels, rewards, dones, st_obs, st_labels, st_dones, cur_rew, cur_len, done_rew, done_len};
    const size_t work = (size_t)N * (size_t)(D > A ? D : A);
    int blocks = (int)((work + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(distill_store_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
