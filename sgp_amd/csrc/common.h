// Shared host-side helpers for libsgp_amd.so (gfx950 only; no other target is supported).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <atomic>
#include "../../include/sgp_amd.h"

namespace sgp {

char* err_buf();                       // thread-local, 512 bytes
int fail(int code, const char* fmt, ...);

inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail((int)e, "%s: %s", what, hipGetErrorString(e));
    return 0;
}

// A launch with more than 48 KB of dynamic LDS needs the kernel's limit raised first; callers enter this only above
// 48 KB, with `cap` the largest size they ever ask of the kernel.  Done once per kernel and device (the attribute
// belongs to the device's copy of the function): the state hangs on the kernel itself, a template VALUE, so two
// instantiations of one signature never share it.  A refusal is reported here, under the caller's name, instead of
// at the launch that would follow.
template <auto Kernel>
int raise_lds_limit(int cap, const char* who) {
    static std::atomic<bool> done[64];
    int dev = 0;
    const bool known = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64;    // (an unknown device: set every time)
    if (known && done[dev].load(std::memory_order_relaxed)) return 0;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, cap);
    if (e != hipSuccess) return fail((int)e, "%s: %d bytes of LDS refused: %s", who, cap, hipGetErrorString(e));
    if (known) done[dev].store(true, std::memory_order_relaxed);
    return 0;
}

// SGP_TUNE="key=value,key=value": the one debug / tuning hook (keys: sgp_amd/tune.py); default when absent
long tune(const char* key, long dflt);

// A zeroed 256-byte device word block for ONE launch's cross-workgroup counters (arrival counts, pacing):
// slots come from a per-device ring of 64, cleared on the launch stream, so launches in flight on different
// streams never share a counter.  nullptr when the allocation fails (callers then run unpaced).
unsigned* sync_slot(hipStream_t s);
// A second lane beside the caller's stream (per host thread and device, created on first use): work forked onto
// `stream` after fork(main) runs concurrently with what the caller enqueues on `main` next; join(main) makes `main`
// wait for it.  Both are event edges (legal under stream capture).  nullptr when the lane cannot be created.
struct SideLane {
    hipStream_t stream;
    hipEvent_t forked, done;
    bool fork(hipStream_t main) { return hipEventRecord(forked, main) == hipSuccess && hipStreamWaitEvent(stream, forked, 0) == hipSuccess; }
    bool join(hipStream_t main) { return hipEventRecord(done, stream) == hipSuccess && hipStreamWaitEvent(main, done, 0) == hipSuccess; }
};
SideLane* side_lane();


// Launch predicate (the trailing `pred, run_if` pair of the hop entries, include/sgp_amd.h): the launch runs only if
// *flag == want when the kernel starts (device-side choice between the split-fp16 hop and the exact kernels, no host
// round trip); flag == nullptr: unconditional.
struct Predicate { const int* flag; int want; };

__host__ __device__ inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// The operand block every hop entry takes (include/sgp_amd.h), in the ABI's order; strides in floats.
struct HopOperands {
    const float* X;  int64_t xrs, xbs;                    // owned source rows
    const float* Xh; int64_t xhrs, xhbs; int32_t n_own;   // halo rows (columns >= n_own), or nullptr: every column is in X
    float* Y;        int64_t yrs, ybs;
    int32_t n_rows, n_cols, batch, feat;
    const int32_t* pred; int32_t run_if; sgp_stream_t stream;
    bool empty() const { return n_rows == 0 || batch == 0 || feat == 0; }
    bool aligned() const {                                // 16-byte bases, strides in whole float4s
        return aligned16(X) && aligned16(Y) && xrs % 4 == 0 && xbs % 4 == 0 && yrs % 4 == 0 && ybs % 4 == 0 &&
               (!Xh || (aligned16(Xh) && xhrs % 4 == 0 && xhbs % 4 == 0));
    }
};
// What a hop kernel asks of the block beyond the common rules (DESIGN.md 4.5 has the table and the reason for every value)
struct HopLimits {
    int64_t own_floats, far_floats, y_floats;   // rows x row stride of X | X_halo | Y stays below this; 0: no bound
    bool aligned16;                             // HopOperands::aligned() required
    int feat_multiple, feat_code;               // feat % feat_multiple != 0 fails with feat_code
    bool own_needs_halo;                        // without a halo n_own must cover n_cols (else it is ignored)
};
// The one judge of a hop operand block: 0, or sgp::fail(...) with a message that starts with `entry`.  Null pointers,
// sizes, n_own and row offsets are judged always; feat and alignment only where there is work (!o.empty()).
int check_hop_operands(const char* entry, const HopOperands& o, const HopLimits& lim);

typedef float f32x4 __attribute__((ext_vector_type(4)));

}  // namespace sgp

#define SGP_STR_(x) #x
#define SGP_STR(x) SGP_STR_(x)        // the spelling of a macro's expansion (entry names built by SGP_SPLIT_NAME)
#define SGP_REQUIRE(cond, ...) \
    do { if (!(cond)) return sgp::fail(SGP_EINVAL, __VA_ARGS__); } while (0)
