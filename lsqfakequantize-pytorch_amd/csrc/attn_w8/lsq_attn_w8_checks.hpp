// lsq_attn_w8_checks.hpp -- the host-side checks that the C ABIs of liblsq_hip_attn_w8.so and liblsq_hip_attn_fused_w8.so share:
// level and floating dtype codes, strided extents and overlaps, the grid limit and the output side (include/lsq_hip_attn_w8.h
// lists the refusals).  Host code only, in the anonymous namespace of the including translation unit: include it after
// lsq_companion_abi.hpp (fail, aligned_to, elem_bytes) and lsq_attn_w8_dev.hpp (lsq::AttnOut).
#pragma once
#include <algorithm>

#include "../lsq_companion_abi.hpp"
#include "../lsq_w8_out_side_host.hpp"
#include "../../../include/lsq_hip_attn_w8.h"
#include "lsq_attn_w8_dev.hpp"

namespace {

bool level_dtype(int64_t code) { return code == LSQ_ATTN_W8_U8 || code == LSQ_ATTN_W8_I8; }

// elements from the first to one past the last of a [B0, B1, rows, cols] tensor
int64_t span_of(const lsq_attn_w8_strides& s, int64_t B0, int64_t B1, int64_t rows, int64_t cols) {
    return (B0 - 1) * s.s0 + (B1 - 1) * s.s1 + (rows - 1) * s.ld + cols;
}

int check_strides(const char* what, const char* name, const lsq_attn_w8_strides& s, int64_t cols) {
    if (s.ld < cols) return fail(LSQ_EINVAL, "%s: %s's row stride %lld is smaller than its row of %lld", what, name, static_cast<ll>(s.ld), static_cast<ll>(cols));
    if (s.s0 < 0 || s.s1 < 0)
        return fail(LSQ_EINVAL, "%s: %s's batch strides (%lld, %lld) must not be negative", what, name, static_cast<ll>(s.s0), static_cast<ll>(s.s1));
    return LSQ_OK;
}

// y's rows and batches must not overlap each other: the strides sorted, each must clear the span of those below it
bool self_overlap(const lsq_attn_w8_strides& s, int64_t B0, int64_t B1, int64_t rows, int64_t cols) {
    int64_t st[3] = {s.s0, s.s1, s.ld}, ex[3] = {B0, B1, rows};
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j)
            if (st[j] < st[i]) {
                std::swap(st[i], st[j]);
                std::swap(ex[i], ex[j]);
            }
    int64_t span = cols;
    for (int i = 0; i < 3; ++i) {
        if (ex[i] == 1) continue;
        if (st[i] < span) return true;
        span += (ex[i] - 1) * st[i];
    }
    return false;
}

constexpr int64_t kMaxGrid = (int64_t{1} << 24) - 1;

int check_grid(const char* what, int64_t grid) {
    // 256 threads a workgroup: the whole launch stays below 2^32 threads, which every HIP runtime accepts
    if (grid > kMaxGrid) return fail(LSQ_EINVAL, "%s: %lld workgroups are beyond 2^24 - 1", what, static_cast<ll>(grid));
    return LSQ_OK;
}

// the output side; the bytes of one element of y into `y_elem`
int check_out(const char* what, const lsq_attn_w8_out* c, lsq::AttnOut& arg, int64_t& y_elem) {
    if (!c) return fail(LSQ_EINVAL, "%s: NULL output description", what);
    return check_out_side(what, *c, arg, y_elem);
}

}  // namespace
