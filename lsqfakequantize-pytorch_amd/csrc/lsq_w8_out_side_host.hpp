// lsq_w8_out_side_host.hpp -- the host side of lsq_w8_out_side.hpp: what the C ABIs of the W8 libraries say the same way.  The
// check of the output side of the level ops (pool_w8, dwconv_w8, eltwise_w8, norm_w8, attn_w8, attn_fused_w8), the byte range of
// a quantizer (the tile-kernel libraries' checks take it from here too) and four small helpers.  Host code only, and like
// lsq_companion_abi.hpp everything is in an ANONYMOUS namespace: each library is one translation unit and reports into an error
// buffer of its own.
#pragma once
#include <algorithm>

#include "lsq_companion_abi.hpp"

namespace {

typedef long long ll;

int64_t ceil_div(int64_t a, int64_t b) { return a / b + (a % b ? 1 : 0); }

bool float_dtype(int64_t code) { return code == LSQ_F32 || code == LSQ_BF16 || code == LSQ_F16; }

bool overlap(const void* p, int64_t p_bytes, const void* r, int64_t r_bytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(r);
    return a < b + static_cast<uintptr_t>(r_bytes) && b < a + static_cast<uintptr_t>(p_bytes);
}

// a quantizer's levels fit a byte; `whose`: "" or the quantizer's name with a trailing blank ("the output's ")
int check_byte_range(const char* what, const char* whose, int64_t quant_min, int64_t quant_max, int64_t type_min, int64_t type_max) {
    const ll lo = std::min(quant_min, type_min), hi = std::max(quant_max, type_max);
    if (quant_min > quant_max || type_min > type_max || !((lo >= 0 && hi <= 255) || (lo >= -128 && hi <= 127)))
        return fail(LSQ_EINVAL, "%s: %s[quant_min, quant_max] = [%lld, %lld] and [type_min, type_max] = [%lld, %lld] must lie within "
                    "0..255 or within -128..127", what, whose, static_cast<ll>(quant_min), static_cast<ll>(quant_max),
                    static_cast<ll>(type_min), static_cast<ll>(type_max));
    return LSQ_OK;
}

// The output side of a level op.  `c` is the public struct that describes it (mid_dtype, out_scale and out_shift -- both NULL: a
// floating y --, quant_min .. type_max), `arg` the kernel argument (scale, shift, qmin .. tmax, mid), which is filled; the bytes
// of one element of y into `y_elem`.
template <typename C, typename Arg>
int check_out_side(const char* what, const C& c, Arg& arg, int64_t& y_elem) {
    if (!float_dtype(c.mid_dtype))
        return fail(LSQ_EINVAL, "%s: mid_dtype must be LSQ_F32, LSQ_BF16 or LSQ_F16, got code %lld", what, static_cast<ll>(c.mid_dtype));
    if ((c.out_scale == nullptr) != (c.out_shift == nullptr))
        return fail(LSQ_EINVAL, "%s: NULL out_scale or out_shift: they come together", what);
    if (c.out_scale) {
        if (!aligned_to(c.out_scale, 4) || !aligned_to(c.out_shift, 4))
            return fail(LSQ_EINVAL, "%s: out_scale and out_shift must be element-aligned", what);
        if (int rc = check_byte_range(what, "the output's ", c.quant_min, c.quant_max, c.type_min, c.type_max)) return rc;
    }
    y_elem = c.out_scale ? 1 : static_cast<int64_t>(elem_bytes(static_cast<int>(c.mid_dtype)));
    arg.scale = static_cast<const float*>(c.out_scale);
    arg.shift = static_cast<const float*>(c.out_shift);
    arg.qmin = static_cast<float>(c.quant_min);
    arg.qmax = static_cast<float>(c.quant_max);
    arg.tmin = static_cast<float>(c.type_min);
    arg.tmax = static_cast<float>(c.type_max);
    arg.mid = static_cast<int>(c.mid_dtype);
    return LSQ_OK;
}

}  // namespace
