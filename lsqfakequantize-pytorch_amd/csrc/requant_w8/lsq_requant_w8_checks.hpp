// lsq_requant_w8_checks.hpp -- the check of the output quantizer of include/lsq_hip_requant_w8.h, for the C ABIs of
// csrc/requant_w8/ and csrc/resadd_w8/.  Host code only, in an ANONYMOUS namespace as csrc/qconv_w8/lsq_w8_host_checks.hpp: an
// error buffer per library.
#pragma once
#include "lsq_requant_w8_tiles.hpp"
#include "../qconv_w8/lsq_w8_host_checks.hpp"
#include "../../../include/lsq_hip_requant_w8.h"

static_assert(LSQ_REQUANT_W8_U8 == LSQ_QCONV_W8_U8 && LSQ_REQUANT_W8_I8 == LSQ_QCONV_W8_I8, "the shared checks read these codes");

namespace {

const char* const kCodes = "LSQ_REQUANT_W8";    // both libraries name lsq_hip_requant_w8.h's level type codes

// the output quantizer's checks; the mid dtype (which takes the place of y's dtype in the other checks) into `mid`
int check_out(const char* what, const lsq_requant_w8_out* o, int& mid, lsq::W8OutArg& arg) {
    if (!o) return fail(LSQ_EINVAL, "%s: NULL output quantizer", what);
    if (o->mid_dtype != LSQ_F32 && o->mid_dtype != LSQ_BF16 && o->mid_dtype != LSQ_F16)
        return fail(LSQ_EINVAL, "%s: mid_dtype must be LSQ_F32, LSQ_BF16 or LSQ_F16, got code %lld", what, static_cast<ll>(o->mid_dtype));
    if (!o->out_scale || !o->out_shift) return fail(LSQ_EINVAL, "%s: NULL out_scale or out_shift", what);
    if (!aligned_to(o->out_scale, 4) || !aligned_to(o->out_shift, 4))
        return fail(LSQ_EINVAL, "%s: out_scale and out_shift must be element-aligned", what);
    if (int rc = check_byte_range(what, "the output's ", o->quant_min, o->quant_max, o->type_min, o->type_max)) return rc;
    mid = static_cast<int>(o->mid_dtype);
    arg = lsq::W8OutArg{static_cast<const float*>(o->out_scale), static_cast<const float*>(o->out_shift),
                        static_cast<float>(o->quant_min), static_cast<float>(o->quant_max), static_cast<float>(o->type_min),
                        static_cast<float>(o->type_max), o->relu ? 1 : 0, mid, 0};
    return LSQ_OK;
}

}  // namespace
