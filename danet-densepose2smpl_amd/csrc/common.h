// Shared helpers of libdanet_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include "danet_hip.h"

namespace danet {

char* last_error_buf();
constexpr int kErrLen = 512;

inline int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error_buf(), kErrLen, fmt, ap);
    va_end(ap);
    return code;
}

#define DANET_CHECK_ARG(cond, ...) \
    do { if (!(cond)) return ::danet::fail(DANET_ERR_ARG, __VA_ARGS__); } while (0)

// An offsets table on the host (the row starts of a CSR: tracks, groups, a person's views): off[0] = 0, off[n] = total, and no entry
// below the one before it.  `op` and `name` open the message ("track_smooth: track_start ...").
inline int check_offsets(const char* op, const char* name, const int32_t* off, int n, long total) {
    DANET_CHECK_ARG(off[0] == 0 && off[n] == total, "%s: %s must run from 0 to N=%ld, got %d..%d", op, name, total, off[0], off[n]);
    for (int i = 0; i < n; ++i) DANET_CHECK_ARG(off[i + 1] >= off[i], "%s: %s descends at entry %d", op, name, i);
    return DANET_OK;
}

#define DANET_CHECK_OFFSETS(op, name, off, n, total) \
    do { const int e_ = ::danet::check_offsets(op, name, off, n, total); if (e_ != DANET_OK) return e_; } while (0)

// first statement of every enqueueing entry point: drop any sticky error left by an earlier,
// unrelated HIP call so that DANET_CHECK_LAUNCH reports only our own launch failures
#define DANET_ENTER() (void)hipGetLastError()

#define DANET_CHECK_LAUNCH(name) \
    do { hipError_t e_ = hipGetLastError(); \
         if (e_ != hipSuccess) return ::danet::fail(DANET_ERR_HIP, "%s: %s", name, hipGetErrorString(e_)); } while (0)

// An internal launcher answers 0 (launched), DANET_ERR_HIP (a HIP call failed; its message stands) or -1 (no instantiation: this message)
#define DANET_CHECK_LAUNCHER(call, ...) \
    do { const int e_ = (call); if (e_ == DANET_ERR_HIP) return e_; if (e_ != 0) return ::danet::fail(DANET_ERR_ARG, __VA_ARGS__); } while (0)

inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// Zero `bytes` (a multiple of 4) at p (4-byte aligned) with a KERNEL on `stream` (capi.hip).  The library never enqueues
// hipMemsetAsync: captured into a hipGraph it becomes a memset NODE, and on this stack (ROCm 7.0 runtime under torch 2.10)
// a memset node followed by a kernel that accumulates into the same buffer was observed to race -- round 5 found one head
// bias gradient in two turning into inf after a few replays of the captured train step (tools/replay_probe.py; the bias
// gradients of danet_channel_sum were the step's only memset nodes), never in eager execution.
hipError_t zero_async(void* p, size_t bytes, hipStream_t stream);

// The opt-in for more than 64 KB of dynamic LDS (capi.hip).  The limit is an attribute of a kernel ON A DEVICE: a launch site calls
// raise_dynamic_lds<&kernel>(bytes, "kernel") before it launches; the attribute is raised the first time each current device is seen, and
// afterwards the call costs hipGetDevice and one atomic load.  Returns DANET_OK, or DANET_ERR_HIP with the kernel, the byte count and
// the HIP error in danet_last_error: do not launch.
struct LdsOptIn { std::atomic<unsigned long long> devices{0}; };     // one bit per device ordinal; ordinals past 63 raise at every call
int raise_dynamic_lds(LdsOptIn& st, const void* kernel, size_t bytes, const char* name);
template <auto Kernel> int raise_dynamic_lds(size_t bytes, const char* name) {     // (one LdsOptIn per kernel instantiation)
    static LdsOptIn st;
    return raise_dynamic_lds(st, reinterpret_cast<const void*>(Kernel), bytes, name);
}

// Compute units of the current device, asked once per device (256 where the runtime will not say).
int compute_units();

}  // namespace danet
