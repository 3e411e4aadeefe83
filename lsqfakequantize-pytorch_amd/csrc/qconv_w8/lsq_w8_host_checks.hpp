// lsq_w8_host_checks.hpp -- the argument checks and kernel arguments that the C ABIs of csrc/qconv_w8/, csrc/requant_w8/ and
// csrc/resadd_w8/ share; check_byte_range is ../lsq_w8_out_side_host.hpp's, which the level ops' libraries include too.  Host code only,
// and like lsq_companion_abi.hpp everything is in an ANONYMOUS namespace: each library is one translation unit, includes this once
// and so reports into an error buffer of its own.
//
// `codes` is the prefix of the including library's level type codes in a message ("LSQ_REQUANT_W8": LSQ_REQUANT_W8_U8 / _I8);
// the codes of every W8A8 header have the values of LSQ_QCONV_W8_U8 / _I8.
#pragma once
#include "lsq_w8_conv_src.hpp"
#include "../lsq_w8_out_side_host.hpp"
#include "../../../include/lsq_hip_qconv_w8.h"

namespace {

int check_dtype(const char* what, int dtype) {
    if (dtype == LSQ_F64) return fail(LSQ_EINVAL, "%s: float64 is not supported (the kernel computes in integers and float32)", what);
    if (dtype != LSQ_F32 && dtype != LSQ_BF16 && dtype != LSQ_F16) return fail(LSQ_EINVAL, "%s: unknown dtype code %d", what, dtype);
    return LSQ_OK;
}

int check_linear_shape(const char* what, int64_t M, int64_t N, int64_t K) {
    const ll m = M, n = N, k = K;
    if (N < 0 || K < 0) return fail(LSQ_EINVAL, "%s: negative weight shape [%lld, %lld]", what, n, k);
    if (M < 1) return fail(LSQ_EINVAL, "%s: M = %lld rows of x, at least 1 is needed", what, m);
    if (M > INT64_MAX / std::max<int64_t>(1, std::max(N, K)) / 4 || N > INT64_MAX / std::max<int64_t>(1, K))
        return fail(LSQ_EINVAL, "%s: M = %lld rows of x on a [%lld, %lld] weight are beyond 64-bit offsets", what, m, n, k);
    return LSQ_OK;
}

// the geometry's checks; fills `s`
int check_conv_geom(const char* what, const lsq_qconv_w8_geom* g, lsq::W8ConvShape& s) {
    if (!g) return fail(LSQ_EINVAL, "%s: NULL geometry", what);
    if (g->B < 1 || g->Cin < 1 || g->H < 1 || g->W < 1)
        return fail(LSQ_EINVAL, "%s: x is [B, H, W, Cin] = [%lld, %lld, %lld, %lld], every extent must be at least 1", what,
                    static_cast<ll>(g->B), static_cast<ll>(g->H), static_cast<ll>(g->W), static_cast<ll>(g->Cin));
    if (g->Cout < 0) return fail(LSQ_EINVAL, "%s: negative Cout = %lld", what, static_cast<ll>(g->Cout));
    if (g->kh < 1 || g->kw < 1)
        return fail(LSQ_EINVAL, "%s: the kernel is %lld x %lld, both must be positive", what, static_cast<ll>(g->kh), static_cast<ll>(g->kw));
    if (g->sh < 1 || g->sw < 1)
        return fail(LSQ_EINVAL, "%s: the stride is (%lld, %lld), both must be positive", what, static_cast<ll>(g->sh), static_cast<ll>(g->sw));
    if (g->dh < 1 || g->dw < 1)
        return fail(LSQ_EINVAL, "%s: the dilation is (%lld, %lld), both must be positive", what, static_cast<ll>(g->dh), static_cast<ll>(g->dw));
    if (g->ph < 0 || g->pw < 0)
        return fail(LSQ_EINVAL, "%s: the padding is (%lld, %lld), negative padding is not supported", what, static_cast<ll>(g->ph),
                    static_cast<ll>(g->pw));
    const int64_t lim = INT32_MAX;
    if (g->H > lim || g->W > lim || g->ph > lim || g->pw > lim || g->H + 2 * g->ph > lim || g->W + 2 * g->pw > lim || g->sh > lim ||
        g->sw > lim || g->dh > lim || g->dw > lim)
        return fail(LSQ_EINVAL, "%s: a padded extent (H + 2 ph, W + 2 pw), stride or dilation is beyond 31 bits", what);
    const int64_t eh = g->H + 2 * g->ph - 1, ew = g->W + 2 * g->pw - 1;           // the last padded coordinate
    if (g->kh - 1 > eh / g->dh || g->kw - 1 > ew / g->dw)
        return fail(LSQ_EINVAL, "%s: an empty output: the dilated %lld x %lld kernel does not fit the padded [%lld, %lld] image", what,
                    static_cast<ll>(g->kh), static_cast<ll>(g->kw), static_cast<ll>(eh + 1), static_cast<ll>(ew + 1));
    s.OH = (eh - g->dh * (g->kh - 1)) / g->sh + 1;
    s.OW = (ew - g->dw * (g->kw - 1)) / g->sw + 1;
    const int64_t taps = g->kh * g->kw;                                             // both below 2^31
    const int64_t pix = s.OH * s.OW, img = g->H * g->W;                             // likewise
    if (g->Cin > INT64_MAX / taps || g->B > INT64_MAX / pix || g->Cin > INT64_MAX / 4 / img || g->B > INT64_MAX / 4 / (img * g->Cin))
        return fail(LSQ_EINVAL, "%s: the shapes are beyond 64-bit offsets", what);
    s.M = g->B * pix;
    s.N = g->Cout;
    s.K = taps * g->Cin;
    s.x_elems = g->B * img * g->Cin;
    if (s.M > INT64_MAX / std::max<int64_t>(1, std::max(s.N, s.K)) / 4 || s.N > INT64_MAX / s.K)
        return fail(LSQ_EINVAL, "%s: %lld output pixels on a [%lld, %lld] weight are beyond 64-bit offsets", what, static_cast<ll>(s.M),
                    static_cast<ll>(s.N), static_cast<ll>(s.K));
    s.cg = lsq::W8ConvGeom{g->Cin, s.OH, s.OW, img * g->Cin, static_cast<int>(g->H), static_cast<int>(g->W), static_cast<int>(g->kw),
                           static_cast<int>(g->sh), static_cast<int>(g->sw), static_cast<int>(g->ph), static_cast<int>(g->pw),
                           static_cast<int>(g->dh), static_cast<int>(g->dw)};
    return LSQ_OK;
}

int check_level_dtype(const char* what, const char* codes, const char* name, int code) {
    if (code != LSQ_QCONV_W8_U8 && code != LSQ_QCONV_W8_I8)
        return fail(LSQ_EINVAL, "%s: %s must be %s_U8 (0) or %s_I8 (1), got %d", what, name, codes, codes, code);
    return LSQ_OK;
}

// the weight's checks of a layer with an 8-bit output; `mid`: the dtype of the unfused op's y
int check_weights(const char* what, const char* codes, int mid, int w_level_dtype, const void* w_levels, const void* w_scale,
                  const void* w_zero, const void* bias, int bias_dtype, const void* y) {
    if (int rc = check_level_dtype(what, codes, "w_level_dtype", w_level_dtype)) return rc;
    if (!w_levels || !w_scale || !w_zero || !y) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (bias && bias_dtype != LSQ_F32 && bias_dtype != mid)
        return fail(LSQ_EINVAL, "%s: the bias must be float32 or of mid_dtype, got dtype code %d", what, bias_dtype);
    if (!aligned_to(w_scale, 4) || !aligned_to(w_zero, 4) || (bias && !aligned_to(bias, elem_bytes(bias_dtype))))
        return fail(LSQ_EINVAL, "%s: w_scale, w_zero and bias must be element-aligned", what);
    return LSQ_OK;
}

int check_levels_in(const char* what, const char* codes, int level_dtype, const void* x_levels, const void* s_x, const void* zx) {
    if (int rc = check_level_dtype(what, codes, "level_dtype", level_dtype)) return rc;
    if (!x_levels || !s_x || !zx) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (!aligned_to(s_x, 4) || !aligned_to(zx, 4)) return fail(LSQ_EINVAL, "%s: s_x and zx must be element-aligned", what);
    return LSQ_OK;
}

int check_grid(const char* what, int64_t grid, int64_t M, int64_t N) {
    if (grid > INT32_MAX)
        return fail(LSQ_EINVAL, "%s: %lld rows by %lld output columns are beyond a 31-bit grid", what, static_cast<ll>(M), static_cast<ll>(N));
    return LSQ_OK;
}

lsq::W8Act levels_act(int level_dtype, const void* x_levels, const void* s_x, const void* zx) {
    lsq::W8Act act{};
    act.a = static_cast<const uint8_t*>(x_levels);
    act.scale = static_cast<const float*>(s_x);
    act.zx = static_cast<const int32_t*>(zx);
    act.off = level_dtype == LSQ_QCONV_W8_U8 ? 128 : 0;
    act.fused = 0;
    act.aligned = aligned_to(x_levels, 16) ? 1 : 0;
    return act;
}

lsq::W8Act fused_act(const void* levels_ws, const void* scale, const void* shift, int64_t quant_min, int64_t quant_max,
                     int64_t type_min, int64_t type_max) {
    lsq::W8Act act{};
    act.a = static_cast<const uint8_t*>(levels_ws);
    act.scale = static_cast<const float*>(scale);
    act.shift = static_cast<const float*>(shift);
    act.qmin = static_cast<float>(quant_min);
    act.qmax = static_cast<float>(quant_max);
    act.tmin = static_cast<float>(type_min);
    act.tmax = static_cast<float>(type_max);
    act.off = std::max(quant_max, type_max) > 127 ? 128 : 0;
    act.fused = 1;
    act.aligned = 1;
    return act;
}

lsq::W8Weight weight_arg(int w_level_dtype, const void* w_levels, const void* w_scale, const void* w_zero, const void* bias, int bias_dtype) {
    return lsq::W8Weight{static_cast<const uint8_t*>(w_levels), static_cast<const float*>(w_scale), static_cast<const int32_t*>(w_zero),
                         bias, bias_dtype, w_level_dtype == LSQ_QCONV_W8_U8 ? 128 : 0};
}

// the eight entries that every plan table begins with
template <typename Plan>
void write_plan(const Plan& pl, int32_t* out8) {
    out8[0] = pl.form;
    out8[1] = pl.shape;
    out8[2] = static_cast<int32_t>(pl.grid);
    out8[3] = pl.block;
    out8[4] = pl.rows;
    out8[5] = pl.cols;
    out8[6] = pl.lds;
    out8[7] = pl.ksplit;
}

}  // namespace
