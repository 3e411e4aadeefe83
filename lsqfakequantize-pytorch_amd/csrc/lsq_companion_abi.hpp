// lsq_companion_abi.hpp -- what the C ABI of every companion library of liblsq_hip.so (group, pack, qlinear, qlinear_a8)
// needs besides its own checks: the calling thread's last error message, the two ways a status is made, and the sizes
// and alignments of the dtype codes of include/lsq_hip.h.  Host code only.
//
// Everything is in an ANONYMOUS namespace: each library is one translation unit with a C ABI, includes this once and so
// keeps an error buffer of its own; its `*_last_error()` returns g_last_error.  (liblsq_hip.so has its own plumbing in
// lsq_capi.hip.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/lsq_hip.h"

namespace {

thread_local char g_last_error[512] = "";

// the message for `*_last_error()`; returns `code`
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_error, sizeof(g_last_error), fmt, ap);
    va_end(ap);
    return code;
}

int hip_status(hipError_t e, const char* what) {
    if (e == hipSuccess) return LSQ_OK;
    return fail(static_cast<int>(e), "%s: %s (%s)", what, hipGetErrorName(e), hipGetErrorString(e));
}

int io_vec(int dtype) { return dtype == LSQ_F32 ? 4 : dtype == LSQ_F64 ? 2 : 8; }      // elements of a 16-byte packet
uintptr_t elem_bytes(int dtype) { return dtype == LSQ_F64 ? 8 : (dtype == LSQ_F32 ? 4 : 2); }
uintptr_t param_bytes(int dtype) { return dtype == LSQ_F64 ? 8 : 4; }                   // scale / shift: the arithmetic type
bool aligned_to(const void* a, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(a) & (bytes - 1)) == 0; }

}  // namespace
