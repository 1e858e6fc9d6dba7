// Dispatch-trace stub: forced into every GEMM translation unit with -include.  Launches print instead of running.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "insv2v_hip.h"
static inline void stub_arg(const insv2v_gemm_desc& d) {
    std::printf(" desc[M=%d N=%d K=%d ldc=%lld fp32=%d act=%d split_k=%d tile=%d c=%llx rs=%llx sp=%d bias=%d rb=%d res=%d cs=%d so=%d]", d.M, d.N, d.K, (long long)d.ldc, d.c_fp32,
                d.act, d.split_k > 1 ? d.split_k : 1, d.tile, (unsigned long long)(uintptr_t)d.c, (unsigned long long)(uintptr_t)d.row_stats, d.stats_parts, d.bias != nullptr, d.row_bias != nullptr,
                d.residual != nullptr, d.col_sum != nullptr, d.stats_out != nullptr);
}
static inline void stub_arg(int v) { std::printf(" %d", v); }
static inline void stub_arg(unsigned v) { std::printf(" %u", v); }
static inline void stub_arg(long v) { std::printf(" %ld", v); }
static inline void stub_arg(long long v) { std::printf(" %lld", v); }
static inline void stub_arg(float v) { std::printf(" %g", v); }
static inline void stub_arg(double v) { std::printf(" %g", v); }
static inline void stub_arg(const void* v) { std::printf(" %llx", (unsigned long long)(uintptr_t)v); }
template <class... A> static inline void stub_args(const A&... a) { (stub_arg(a), ...); }
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, grid, block, lds, stream, ...)                                                                        \
    do {                                                                                                                            \
        const dim3 g_ = (grid), b_ = (block);                                                                                       \
        std::printf("LAUNCH %s | %s | grid %u %u %u block %u lds %zu |", std::strstr(__PRETTY_FUNCTION__, "launch_") ? __PRETTY_FUNCTION__ : "-", #k, g_.x, g_.y, g_.z, b_.x, (size_t)(lds)); \
        stub_args(__VA_ARGS__);                                                                                                     \
        std::printf("\n");                                                                                                          \
    } while (0)
#define hipFuncSetAttribute(...) hipSuccess
static inline int stub_cus() { const char* e = std::getenv("HARNESS_CUS"); return e ? std::atoi(e) : 256; }
static inline hipError_t stub_props(hipDeviceProp_t* p, int) { p->multiProcessorCount = stub_cus(); return hipSuccess; }
#undef hipGetDeviceProperties
#define hipGetDeviceProperties(p, d) stub_props(p, d)
#define hipGetDevice(p) (*(p) = 0, hipSuccess)
#define hipGetLastError() hipSuccess
