// cf2sim_timing.h -- phase stamps of -DCF2_TIMING builds (tools/timeline.py)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cf2 {

// ---- phase timeline instrumentation (tools/timeline.py; -DCF2_TIMING builds only) ----
#ifdef CF2_TIMING
__device__ uint64_t* g_cf2_timing;   // [waves][16]: 0 hw id, 1 realtime start, 2 realtime end, 3.. memtime stamps
__device__ __forceinline__ uint64_t* timing_row() {
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    return g_cf2_timing ? g_cf2_timing + (size_t)wave * 16 : nullptr;
}
#define TSTAMP(k)                                                                              \
    do {                                                                                       \
        const uint64_t t_ = __builtin_amdgcn_s_memtime();                                      \
        uint64_t* r_ = timing_row();                                                           \
        const int first_ = __ffsll((unsigned long long)__builtin_amdgcn_read_exec()) - 1;      \
        if (r_ && (int)(threadIdx.x & 63) == first_) r_[3 + (k)] = t_;                         \
    } while (0)
#define TREADY(...) asm volatile("" ::__VA_ARGS__)
// a kernel's entry: the wave's hardware id, realtime start and stamp 0
__device__ __forceinline__ void timing_begin() {
    if (uint64_t* r = timing_row()) {
        if ((threadIdx.x & 63) == 0) {
            const uint32_t hw = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4);    // HW_ID
            const uint32_t xcc = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20);   // XCC_ID
            r[0] = ((uint64_t)xcc << 32) | hw;
            r[1] = __builtin_amdgcn_s_memrealtime();
            r[3] = __builtin_amdgcn_s_memtime();
        }
    }
}
// a kernel's exit: stamp 5 and the realtime end
__device__ __forceinline__ void timing_end() {
    TSTAMP(5);
    if (uint64_t* r = timing_row())
        if ((threadIdx.x & 63) == 0) r[2] = __builtin_amdgcn_s_memrealtime();
}
#else
#define TSTAMP(k) do { } while (0)
#define TREADY(...) do { } while (0)
__device__ __forceinline__ void timing_begin() {}
__device__ __forceinline__ void timing_end() {}
#endif

}  // namespace cf2
