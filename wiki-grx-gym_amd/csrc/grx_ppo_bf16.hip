// grx_ppo_bf16.hip -- the bf16 matrix path of the PPO hidden layers (include/grx_ppo.h: grx_mlp_layer_bf16,
// grx_mlp_input_grad_bf16, grx_mlp_weight_grad_bf16).
//
// Every operand is read as fp32 and rounded to bf16 (round-to-nearest-even, NaN kept: v_cvt_pk_bf16_f32, which the compiler
// emits for __builtin_convertvector float -> __bf16) on its way from registers into LDS; nothing bf16 is stored in memory.
// Products accumulate in fp32 on v_mfma_f32_32x32x16_bf16 (K = 16 per instruction, where the f32 form takes K = 2).
//
// One kernel serves the three products.  It computes D[r][c] = sum_k A(r, k) B(c, k) over a range of k, where each operand is
// either K-CONTIGUOUS (element (r, k) at G[r * ld + k]) or ROW-CONTIGUOUS (element (r, k) at G[k * ld + r]):
//   forward  Y  [M][N] = X [M][K] . W^T   A = X  (K-contiguous), B = W  (K-contiguous), bias + ELU in the epilogue
//   input    dX [M][K] = dZ[M][N] . W     A = dZ (K-contiguous), B = W  (row-contiguous: B(c = k, n) = W[n][k])
//   weight   dW [N][K] = dZ^T . X         A = dZ (row-contiguous), B = X (row-contiguous), summed over the batch in slabs
// Block: 256 threads, a 128 x 64 output tile; the four waves sit 2 x 2 and each owns 64 x 32 (two 32 x 32 accumulators that share
// the B fragment: three ds_read_b128 per two MFMAs).  The contraction runs in chunks of 64 through two LDS buffers; the next chunk's
// global loads are in flight while the current chunk multiplies.  LDS rows are [row][k] with 72 bf16 (144 B = 36 dwords) per row:
// a 16-lane group of fragment reads hits 16 rows that differ mod 16, and 36 / 4 is odd, so the reads are free of bank conflicts.
// The k order of every output is fixed by the chunking alone: a row's result does not depend on the batch it sits in, and the
// weight gradient's slabs are added in slab order (deterministic: a captured replay equals the eager call bit for bit).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grx_ppo.h"

namespace {
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 128, BN = 64, KC = 64, LDK = KC + 8, NT = 256;
constexpr int WS_MIN_SLAB = 256, WS_TARGET_BLOCKS = 512;   // weight gradient: batch slabs of >= 256 rows, ~2 blocks per CU

__device__ inline float elu1(float x) { return x > 0.f ? x : expm1f(x); }   // torch.nn.ELU(alpha = 1)
__device__ inline bf16x4 to_bf16(f32x4 v) { return __builtin_convertvector(v, bf16x4); }   // v_cvt_pk_bf16_f32 x 2 (RNE, NaN kept)

// R rows x KC contraction values of one operand, global -> registers (fp32) -> LDS (bf16), zero outside rows x [k0, k1).
// K-contiguous: thread t, pass p covers row 16 p + t / 16, k quad 4 (t % 16).  Row-contiguous: a 4-row x 4-k block per thread and
// pass (consecutive threads walk consecutive row quads: coalesced along the rows), transposed in registers, so that both kinds of
// operand land as [row][k] in LDS with 8-byte stores.  VEC: 16-byte aligned base and ld % 4 == 0.
template <int R, bool KCONTIG, bool VEC>
struct Tile {
    static constexpr int NV = R * KC / 4 / NT;
    f32x4 v[NV];
    __device__ inline void fetch(const float* __restrict__ G, int ld, int rows, int r0, int k0, int k1, int tid) {
        if (KCONTIG) {
#pragma unroll
            for (int p = 0; p < NV; ++p) {
                const int r = r0 + 16 * p + (tid >> 4), k = k0 + 4 * (tid & 15);
                f32x4 x = {0.f, 0.f, 0.f, 0.f};
                if (r < rows) {
                    const float* g = G + (size_t)r * ld + k;
                    if (VEC && k + 3 < k1) x = *reinterpret_cast<const f32x4*>(g);
                    else { if (k < k1) x[0] = g[0]; if (k + 1 < k1) x[1] = g[1]; if (k + 2 < k1) x[2] = g[2]; if (k + 3 < k1) x[3] = g[3]; }
                }
                v[p] = x;
            }
        } else {
#pragma unroll
            for (int p = 0; p < NV / 4; ++p) {
                const int b = p * NT + tid, r = r0 + 4 * (b % (R / 4)), k = k0 + 4 * (b / (R / 4));
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    f32x4 x = {0.f, 0.f, 0.f, 0.f};
                    if (k + i < k1) {
                        const float* g = G + (size_t)(k + i) * ld + r;
                        if (VEC && r + 3 < rows) x = *reinterpret_cast<const f32x4*>(g);
                        else { if (r < rows) x[0] = g[0]; if (r + 1 < rows) x[1] = g[1]; if (r + 2 < rows) x[2] = g[2]; if (r + 3 < rows) x[3] = g[3]; }
                    }
                    v[4 * p + i] = x;   // v[4p + i][j]: row r + j, k + i
                }
            }
        }
    }
    __device__ inline void stash(__bf16* __restrict__ S, int tid) const {
        if (KCONTIG) {
#pragma unroll
            for (int p = 0; p < NV; ++p)
                *reinterpret_cast<bf16x4*>(S + (16 * p + (tid >> 4)) * LDK + 4 * (tid & 15)) = to_bf16(v[p]);
        } else {
#pragma unroll
            for (int p = 0; p < NV / 4; ++p) {
                const int b = p * NT + tid, r = 4 * (b % (R / 4)), k = 4 * (b / (R / 4));
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x4 t = {v[4 * p][j], v[4 * p + 1][j], v[4 * p + 2][j], v[4 * p + 3][j]};
                    *reinterpret_cast<bf16x4*>(S + (r + j) * LDK + k) = to_bf16(t);
                }
            }
        }
    }
};

// D[z][r][c] (r < MA, c < NB, row stride ldd) = sum over k in slab z of [0, KT) of bf16(A(r, k)) bf16(B(c, k)) [+ bias[c], ELU]
template <bool AK, bool BK, bool VEC, bool ELU>
__global__ __launch_bounds__(NT) void bf16_gemm_kernel(int MA, int NB, int KT, int kslab, const float* __restrict__ A, int lda,
                                                       const float* __restrict__ B, int ldb, const float* __restrict__ bias,
                                                       float* __restrict__ D, int ldd) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "bf16_gemm_kernel uses v_mfma_f32_32x32x16_bf16: gfx950 only -- this library is built for MI355X, see the Makefile"
#endif
    __shared__ __bf16 As[2][BM * LDK], Bs[2][BN * LDK];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wy = wv >> 1, wx = wv & 1;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int kb = blockIdx.z * kslab, ke = min(KT, kb + kslab);
    D += (size_t)blockIdx.z * MA * ldd;
    Tile<BM, AK, VEC> ta;
    Tile<BN, BK, VEC> tb;
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    ta.fetch(A, lda, MA, m0, kb, ke, tid);
    tb.fetch(B, ldb, NB, n0, kb, ke, tid);
    ta.stash(As[0], tid); tb.stash(Bs[0], tid);
    __syncthreads();
    // fragment reads (cdna_hip_programming.md section 3): lane l holds A[row l & 31][k = 8 (l >> 5) + j], B[k = 8 (l >> 5) + j][col l & 31]
    const int fo = (lane & 31) * LDK + 8 * (lane >> 5);
    int buf = 0;
    for (int k0 = kb; k0 < ke; k0 += KC, buf ^= 1) {
        const bool more = k0 + KC < ke;
        if (more) { ta.fetch(A, lda, MA, m0, k0 + KC, ke, tid); tb.fetch(B, ldb, NB, n0, k0 + KC, ke, tid); }   // in flight during the MFMAs
        const __bf16* xa = As[buf] + 64 * wy * LDK + fo;
        const __bf16* xb = Bs[buf] + 32 * wx * LDK + fo;
        bf16x8 a0[KC / 16], a1[KC / 16], b[KC / 16];
#pragma unroll
        for (int s = 0; s < KC / 16; ++s) {
            a0[s] = *reinterpret_cast<const bf16x8*>(xa + 16 * s);
            a1[s] = *reinterpret_cast<const bf16x8*>(xa + 32 * LDK + 16 * s);
            b[s] = *reinterpret_cast<const bf16x8*>(xb + 16 * s);
        }
#pragma unroll
        for (int s = 0; s < KC / 16; ++s) {   // (a chunk beyond the range is zero in LDS: adds +0)
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[s], b[s], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[s], b[s], acc[1], 0, 0, 0);
        }
        if (more) { ta.stash(As[buf ^ 1], tid); tb.stash(Bs[buf ^ 1], tid); }
        __syncthreads();
    }
    // D layout: col = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5)
    const int col = n0 + 32 * wx + (lane & 31);
    if (col >= NB) return;
    const float bv = bias ? bias[col] : 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = m0 + 64 * wy + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (row < MA) { const float y = acc[t][r] + bv; D[(size_t)row * ldd + col] = ELU ? elu1(y) : y; }
        }
}

// out[i] = partials[0][i] + partials[1][i] + ... in slab order
__global__ __launch_bounds__(256) void slab_sum_kernel(long long n, int nslab, const float* __restrict__ partials, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float t = 0.f;
    for (int s = 0; s < nslab; ++s) t += partials[(size_t)s * n + i];
    out[i] = t;
}

template <bool AK, bool BK, bool ELU>
int launch_gemm(dim3 grid, hipStream_t st, bool vec, int MA, int NB, int KT, int kslab, const float* A, int lda, const float* B,
                int ldb, const float* bias, float* D, int ldd) {
    if (vec) hipLaunchKernelGGL((bf16_gemm_kernel<AK, BK, true, ELU>), grid, dim3(NT), 0, st, MA, NB, KT, kslab, A, lda, B, ldb, bias, D, ldd);
    else hipLaunchKernelGGL((bf16_gemm_kernel<AK, BK, false, ELU>), grid, dim3(NT), 0, st, MA, NB, KT, kslab, A, lda, B, ldb, bias, D, ldd);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// rows of batch per slab of the weight gradient: a function of the shape alone
inline int ws_slab(int M, int N, int K) {
    const long long tiles = (long long)((N + BM - 1) / BM) * ((K + BN - 1) / BN);
    const long long want = (WS_TARGET_BLOCKS + tiles - 1) / tiles;                // slabs wanted for ~WS_TARGET_BLOCKS blocks
    long long slab = (M + want - 1) / want;
    slab = (slab + KC - 1) / KC * KC;
    return (int)(slab < WS_MIN_SLAB ? WS_MIN_SLAB : slab);
}
}  // namespace

extern "C" int grx_mlp_layer_bf16(int M, int K, int N, const float* X, const float* W, const float* bias, float* Y, int elu, void* stream) {
    if (M < 1 || K < 1 || N < 1 || !X || !W || !Y) return -1;
    const bool vec = K % 4 == 0 && al16(X) && al16(W);
    const dim3 grid((M + BM - 1) / BM, (N + BN - 1) / BN, 1);
    hipStream_t st = (hipStream_t)stream;
    return elu ? launch_gemm<true, true, true>(grid, st, vec, M, N, K, K, X, K, W, K, bias, Y, N)
               : launch_gemm<true, true, false>(grid, st, vec, M, N, K, K, X, K, W, K, bias, Y, N);
}

extern "C" int grx_mlp_input_grad_bf16(int M, int N, int K, const float* dZ, const float* W, float* dX, void* stream) {
    if (M < 1 || N < 1 || K < 1 || !dZ || !W || !dX) return -1;
    const bool vec = N % 4 == 0 && K % 4 == 0 && al16(dZ) && al16(W);
    const dim3 grid((M + BM - 1) / BM, (K + BN - 1) / BN, 1);
    return launch_gemm<true, false, false>(grid, (hipStream_t)stream, vec, M, K, N, N, dZ, N, W, K, nullptr, dX, K);
}

extern "C" int grx_mlp_weight_grad_bf16_partials_size(int M, int N, int K) {
    if (M < 1 || N < 1 || K < 1) return 0;
    const int slab = ws_slab(M, N, K);
    const long long n = (long long)((M + slab - 1) / slab) * N * K;
    return n > 0x7fffffffLL ? 0 : (int)n;
}

extern "C" int grx_mlp_weight_grad_bf16(int M, int N, int K, const float* dZ, const float* X, float* dW, float* partials, void* stream) {
    if (M < 1 || N < 1 || K < 1 || !dZ || !X || !dW || !partials || grx_mlp_weight_grad_bf16_partials_size(M, N, K) < 1) return -1;
    const int slab = ws_slab(M, N, K), nslab = (M + slab - 1) / slab;
    const bool vec = N % 4 == 0 && K % 4 == 0 && al16(dZ) && al16(X);
    const dim3 grid((N + BM - 1) / BM, (K + BN - 1) / BN, nslab);
    hipStream_t st = (hipStream_t)stream;
    const int rc = launch_gemm<false, false, false>(grid, st, vec, N, K, M, slab, dZ, N, X, K, nullptr, partials, K);
    if (rc) return rc;
    const long long n = (long long)N * K;
    hipLaunchKernelGGL(slab_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, nslab, (const float*)partials, dW);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
