// hip_host_stub.cpp -- host-memory stand-in for the HIP runtime calls libgrx_hip.so makes while it BUILDS a handle (grx_create, grx_layout, grx_tensor,
// grx_state_bytes, grx_save_state, grx_destroy): device memory is host memory, nothing is launched.  tools/host_create_digest.py loads it ahead of
// the library.  Every host-to-device copy is logged as (bytes, hash), the words that point into an allocation replaced by (allocation size, offset).
#include <hip/hip_runtime_api.h>
#include <map>
#include <vector>
#include <cstring>
#include <cstdlib>
#include <cstdint>
static std::map<uintptr_t, size_t> g_allocs;
static std::vector<std::pair<uint64_t, uint64_t>> g_log;
static uint64_t fnv(const void* p, size_t n) { uint64_t h = 0xcbf29ce484222325ull; auto b = (const unsigned char*)p; for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 0x100000001b3ull; } return h; }
extern "C" {
hipError_t hipGetDeviceCount(int* n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipMalloc(void** p, size_t n) { *p = malloc(n); g_allocs[(uintptr_t)*p] = n; return hipSuccess; }
hipError_t hipFree(void* p) { g_allocs.erase((uintptr_t)p); free(p); return hipSuccess; }
hipError_t hipMemset(void* p, int v, size_t n) { memset(p, v, n); return hipSuccess; }
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind k) {
    memcpy(d, s, n);
    if (k == hipMemcpyHostToDevice) {
        std::vector<unsigned char> c((const unsigned char*)s, (const unsigned char*)s + n);
        for (size_t o = 0; o + 8 <= n; o += 8) {
            uint64_t w; memcpy(&w, &c[o], 8);
            auto it = g_allocs.upper_bound((uintptr_t)w);
            if (it != g_allocs.begin()) { --it; if (w >= it->first && w < it->first + it->second) { uint64_t r = 0xA110C00000000000ull + it->second * 4096 + (w - it->first); memcpy(&c[o], &r, 8); } }
        }
        g_log.push_back({n, fnv(c.data(), n)});
    }
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) { memcpy(d, s, n); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamIsCapturing(hipStream_t, hipStreamCaptureStatus* s) { *s = hipStreamCaptureStatusNone; return hipSuccess; }
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_tR0600* p, int) { memset(p, 0, sizeof *p); p->multiProcessorCount = 256; return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t n, unsigned) { *p = calloc(1, n); return hipSuccess; }
hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned) { *d = h; return hipSuccess; }
hipError_t hipHostFree(void* p) { free(p); return hipSuccess; }
hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipSuccess; }
hipError_t hipGetLastError() { return hipSuccess; }
hipError_t hipPeekAtLastError() { return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "hip_host_stub"; }
void stub_reset() { g_log.clear(); }
int stub_log(uint64_t* out, int max) { int n = 0; for (auto& e : g_log) { if (n + 2 > max) break; out[n++] = e.first; out[n++] = e.second; } return n; }
}
