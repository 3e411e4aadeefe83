// lsq_qconv_w8.hip -- 2-D convolution of 8-bit activation levels with 8-bit weight levels, one (scale, zero point) per output
// channel, on gfx950 (include/lsq_hip_qconv_w8.h, which states the contract): the kernels and the C ABI of
// liblsq_hip_qconv_w8.so.
//
//     I[b, n, oh, ow] = sum_{i, j, c} (lx[b, oh sh - ph + i dh, ow sw - pw + j dw, c] - zx) * (lw[n, i, j, c] - zw[n])
//     y = ((s_w[n] * float(I)) * s_x) + bias[n]
//
// With channels-last operands this is the W8A8 linear's GEMM (csrc/qlinear_w8/) with M = B OH OW, N = Cout and
// K = kh kw Cin: the weight [Cout, kh, kw, Cin] is the row-major [N, K] byte matrix, y [B, OH, OW, Cout] the row-major [M, N]
// output, and only the A operand differs -- row m = (b, oh, ow) of the IMPLICIT matrix holds, at k = (i kw + j) Cin + c, the
// byte operand of x[b, oh sh - ph + i dh, ow sw - pw + j dw, c], or that of the LEVEL zx (the real value 0) where the tap
// lies in the padding: the byte zx - off, so that sum a w, sum_k a and w8_exact's corrections need no special case.
//
//  * MATRIX-CORE form (Cin % 16 == 0, K <= 65536, lw and the levels 16-byte aligned): lsq_qconv_w8_tiles.hpp's tile body,
//    the linear's TILES kernel step for step, on W8ConvSrc.  Every 16-byte packet of a row lies inside one tap: one aligned
//    load of x or one padding packet.  A thread's staging rows are fixed over all steps, so m -> (b, oh, ow) -> (offset of image b, ih0, iw0) is
//    taken apart once before the K loop, in 64 bits; per step one k -> (i, j, c) (two 32-bit divisions, shared by the
//    thread's rows), advanced packet by packet, and per packet one bounds test and one address.  M <= 16 takes the 32-row
//    tile: a convolution has no decode shape worth a kernel.
//  * GENERIC form (every other legal call: Cin = 3 stems, Cin % 16 != 0, K > 65536, misaligned buffers): one wave per output
//    channel and four output pixels, 64-bit integer multiply-adds of (lx - zx)(lw - zw) over the in-bounds taps only, a
//    butterfly over the wave.  Correct for every legal input; not tuned.
//  * The fused entry form runs the linear's flat pre-pass (w8_levels_body) over the B H W Cin elements of channels-last x.
#include "lsq_qconv_w8_tiles.hpp"
#include "lsq_w8_host_checks.hpp"

namespace lsq {

// ------------------------------------------------------------------------------------------------
// matrix-core form: lsq_qconv_w8_tiles.hpp's body on the implicit matrix
// ------------------------------------------------------------------------------------------------
template <int SUBS, bool SPLITK>
__global__ __launch_bounds__(kW8TileWaves * 64, 2) void qconv_w8_tiles_kernel(W8Act act, W8Weight wt, W8Geom geo, W8ConvGeom cg,
                                                                             void* __restrict__ y, int y_dtype) {
    const W8Const ac = w8_constants(act);
    w8_tiles_body<SUBS, SPLITK>(w8_conv_src(act, ac, cg), ac, wt, geo, y, y_dtype);
}

// ------------------------------------------------------------------------------------------------
// generic form
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void qconv_w8_generic_kernel(W8Act act, W8Weight wt, W8Geom geo, W8ConvGeom cg,
                                                                 void* __restrict__ y, int y_dtype) {
    constexpr int R = kQGenericRowsAtOnce;
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int64_t wave = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
    const int64_t waves = static_cast<int64_t>(gridDim.x) * (kBlock / 64);
    const int64_t M = geo.M, N = geo.N, K = geo.K;
    const int64_t items = (M + R - 1) / R * N;              // (four output pixels, output channel)
    const W8Const ac = w8_constants(act);
    const uint8_t flipx = static_cast<uint8_t>(ac.flip & 0xffu), flipw = static_cast<uint8_t>(wt.off);
    for (int64_t item = wave; item < items; item += waves) {
        const int64_t mb = item / N, n = item - mb * N, m0 = mb * R;
        const uint8_t* __restrict__ wrow = wt.w + n * K;
        const int z_w = wt.zero[n] - wt.off;
        W8ConvRow r[R];
        int64_t I[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            r[i] = w8_conv_row(m0 + i, cg.OH, cg.OW, cg.image, cg.sh, cg.sw, cg.ph, cg.pw);
            I[i] = 0;
        }
        for (int64_t k = lane; k < K; k += 64) {
            const int64_t tap = k / cg.Cin, c = k - tap * cg.Cin;
            const int64_t ti = tap / cg.kw, tj = tap - ti * cg.kw;
            const unsigned idh = static_cast<unsigned>(ti * cg.dh), jdw = static_cast<unsigned>(tj * cg.dw);
            const int64_t wz = static_cast<int>(static_cast<int8_t>(wrow[k] ^ flipw)) - z_w;
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const unsigned ih = static_cast<unsigned>(r[i].ih0) + idh, iw = static_cast<unsigned>(r[i].iw0) + jdw;
                if (m0 + i < M && ih < static_cast<unsigned>(cg.H) && iw < static_cast<unsigned>(cg.W)) {
                    const int64_t at = r[i].base + (static_cast<int64_t>(ih) * cg.W + iw) * cg.Cin + c;
                    I[i] += (static_cast<int>(static_cast<int8_t>(act.a[at] ^ flipx)) - ac.z) * wz;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < R; ++i) {
            for (int s = 32; s >= 1; s >>= 1) I[i] += w8_shfl_xor_i64(I[i], s);        // integers: any order
            if (lane == 0 && m0 + i < M) w8_store(I[i], wt, ac.s_x, n, y, y_dtype, (m0 + i) * N + n);
        }
    }
}

// the fused form's pre-pass (the body: lsq_qconv_w8_tiles.hpp): on channels-last data the linear's flat pass
template <typename IO>
__global__ __launch_bounds__(kBlock) void qconv_w8_levels_kernel(const void* __restrict__ x, int64_t n, const float* __restrict__ scale,
                                                                const float* __restrict__ shift, float qmin, float qmax, float tmin,
                                                                float tmax, int off, uint8_t* __restrict__ ws) {
    w8_levels_body<IO>(x, n, scale, shift, qmin, qmax, tmin, tmax, off, ws);
}

// ------------------------------------------------------------------------------------------------
// host side: the plan and the launchers
// ------------------------------------------------------------------------------------------------
struct W8ConvPlan {
    int form, shape, block, lds, rows, cols, ksplit, subs;
    int64_t grid, row_tiles, col_tiles;
};

inline W8ConvPlan plan_conv_w8(const W8ConvShape& s, bool aligned) {
    W8ConvPlan pl = {};
    const int64_t cus = device_info().cu_count;
    const int64_t M = s.M, N = s.N, K = s.K;
    if (!(aligned && s.cg.Cin % 16 == 0 && K <= kW8MaxK)) {
        pl.form = 0;
        pl.shape = LSQ_QCONV_W8_SHAPE_GENERIC;
        pl.block = kBlock;
        pl.rows = kQGenericRowsAtOnce;
        pl.cols = 1;
        pl.ksplit = 1;
        const int64_t per_block = kBlock / 64, blocks = (M + pl.rows - 1) / pl.rows;
        const int64_t items = blocks <= INT64_MAX / std::max<int64_t>(1, N) ? blocks * N : INT64_MAX;
        pl.grid = std::min(std::max<int64_t>(1, items / per_block + (items % per_block ? 1 : 0)), cus * 8);
        return pl;
    }
    pl.form = 1;
    pl.subs = M <= 32 ? 2 : (M <= 64 ? 4 : kW8MaxSubs);
    pl.rows = pl.subs * 16;
    pl.row_tiles = (M + pl.rows - 1) / pl.rows;
    const int64_t wide = (N + 16 * kW8TileWaves - 1) / (16 * kW8TileWaves);
    // 64-column tiles once they give every compute unit a tile; below that 16-column tiles, four times as many, K split over the waves
    const bool split = wide <= INT64_MAX / pl.row_tiles && pl.row_tiles * wide < cus;
    pl.shape = split ? LSQ_QCONV_W8_SHAPE_TILES_SPLIT_K : LSQ_QCONV_W8_SHAPE_TILES;
    pl.cols = split ? kW8Tile : 16 * kW8TileWaves;
    pl.ksplit = split ? kW8TileWaves : 1;
    pl.col_tiles = (N + pl.cols - 1) / pl.cols;
    pl.grid = pl.col_tiles <= INT64_MAX / pl.row_tiles ? pl.row_tiles * pl.col_tiles : INT64_MAX;
    pl.block = kW8TileWaves * 64;
    pl.lds = w8_tiles_lds(pl.subs);
    return pl;
}

template <int SUBS, bool SPLITK>
static hipError_t conv_w8_launch_tiles(const W8ConvPlan& pl, const W8Act& act, const W8Weight& wt, const W8Geom& geo, const W8ConvGeom& cg,
                                       void* y, int y_dtype, hipStream_t stream) {
    static_assert(w8_tiles_lds(SUBS) <= 64 * 1024, "the tile fits the LDS a kernel gets unasked");
    static_assert(kW8TileWaves * SUBS * 64 * 16 <= SUBS * 16 * kW8TileStride, "the split-K tiles fit the staging area");
    hipLaunchKernelGGL((qconv_w8_tiles_kernel<SUBS, SPLITK>), dim3(static_cast<unsigned>(pl.grid)), dim3(kW8TileWaves * 64), pl.lds,
                       stream, act, wt, geo, cg, y, y_dtype);
    return hipGetLastError();
}

template <bool SPLITK>
static hipError_t conv_w8_subs(const W8ConvPlan& pl, const W8Act& act, const W8Weight& wt, const W8Geom& geo, const W8ConvGeom& cg, void* y,
                               int y_dtype, hipStream_t s) {
    if (pl.subs == 2) return conv_w8_launch_tiles<2, SPLITK>(pl, act, wt, geo, cg, y, y_dtype, s);
    if (pl.subs == 4) return conv_w8_launch_tiles<4, SPLITK>(pl, act, wt, geo, cg, y, y_dtype, s);
    return conv_w8_launch_tiles<kW8MaxSubs, SPLITK>(pl, act, wt, geo, cg, y, y_dtype, s);
}

static hipError_t conv_w8_launch(const W8ConvPlan& pl, const W8Act& act, const W8Weight& wt, const W8ConvShape& s, void* y, int y_dtype,
                                 hipStream_t stream) {
    const W8Geom geo{s.M, s.N, s.K, pl.row_tiles};
    if (pl.shape == LSQ_QCONV_W8_SHAPE_GENERIC) {
        hipLaunchKernelGGL(qconv_w8_generic_kernel, dim3(static_cast<unsigned>(pl.grid)), dim3(kBlock), 0, stream, act, wt, geo, s.cg, y,
                           y_dtype);
        return hipGetLastError();
    }
    return pl.shape == LSQ_QCONV_W8_SHAPE_TILES_SPLIT_K ? conv_w8_subs<true>(pl, act, wt, geo, s.cg, y, y_dtype, stream)
                                                        : conv_w8_subs<false>(pl, act, wt, geo, s.cg, y, y_dtype, stream);
}

template <typename IO>
static hipError_t conv_w8_levels(const void* x, int64_t n, const W8Act& act, void* ws, hipStream_t stream) {
    const int64_t cus = device_info().cu_count;
    const int64_t turns = (n + 15) / 16;
    const int grid = static_cast<int>(std::min(std::max<int64_t>(1, (turns + kBlock - 1) / kBlock), cus * 8));
    hipLaunchKernelGGL((qconv_w8_levels_kernel<IO>), dim3(grid), dim3(kBlock), 0, stream, x, n, act.scale, act.shift, act.qmin, act.qmax,
                       act.tmin, act.tmax, act.off, static_cast<uint8_t*>(ws));
    return hipGetLastError();
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_qconv_w8.h: validation, dtype dispatch, error bookkeeping
// ------------------------------------------------------------------------------------------------
namespace {

const char* const kCodes = "LSQ_QCONV_W8";

// (not lsq_w8_host_checks.hpp's check_weights: the bias is held to y's type in other words, and y's alignment is checked here)
int check_conv_weights(const char* what, int y_dtype, int w_level_dtype, const void* w_levels, const void* w_scale, const void* w_zero,
                       const void* bias, int bias_dtype, const void* y) {
    if (int rc = check_level_dtype(what, kCodes, "w_level_dtype", w_level_dtype)) return rc;
    if (!w_levels || !w_scale || !w_zero || !y) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (bias && bias_dtype != LSQ_F32 && bias_dtype != y_dtype)
        return fail(LSQ_EINVAL, "%s: the bias must be float32 or of y's type, got dtype code %d", what, bias_dtype);
    if (!aligned_to(y, elem_bytes(y_dtype))) return fail(LSQ_EINVAL, "%s: x and y must be element-aligned", what);
    if (!aligned_to(w_scale, 4) || !aligned_to(w_zero, 4) || (bias && !aligned_to(bias, elem_bytes(bias_dtype))))
        return fail(LSQ_EINVAL, "%s: w_scale, w_zero and bias must be element-aligned", what);
    return LSQ_OK;
}

int checked_conv_plan(const char* what, lsq::W8ConvPlan& pl, const lsq::W8ConvShape& s, bool aligned) {
    pl = lsq::plan_conv_w8(s, aligned);
    if (pl.grid > INT32_MAX)
        return fail(LSQ_EINVAL, "%s: %lld output pixels by %lld output channels are beyond a 31-bit grid", what,
                    static_cast<long long>(s.M), static_cast<long long>(s.N));
    return LSQ_OK;
}

}  // namespace

extern "C" {

int lsq_qconv_w8_abi_version(void) { return LSQ_QCONV_W8_ABI_VERSION; }

const char* lsq_qconv_w8_last_error(void) { return g_last_error; }

int lsq_qconv_w8_forward_levels(int level_dtype, const void* x_levels, const void* s_x, const void* zx, const lsq_qconv_w8_geom* geom,
                                int w_level_dtype, const void* w_levels, const void* w_scale, const void* w_zero, const void* bias,
                                int bias_dtype, void* y, int y_dtype, void* stream) {
    const char* what = "lsq_qconv_w8_forward_levels";
    lsq::W8ConvShape s;
    if (int rc = check_dtype(what, y_dtype)) return rc;
    if (int rc = check_conv_geom(what, geom, s)) return rc;
    if (int rc = check_level_dtype(what, kCodes, "level_dtype", level_dtype)) return rc;
    if (!x_levels || !s_x || !zx) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (int rc = check_conv_weights(what, y_dtype, w_level_dtype, w_levels, w_scale, w_zero, bias, bias_dtype, y)) return rc;
    if (!aligned_to(s_x, 4) || !aligned_to(zx, 4)) return fail(LSQ_EINVAL, "%s: s_x and zx must be element-aligned", what);
    lsq::W8ConvPlan pl;
    if (int rc = checked_conv_plan(what, pl, s, aligned_to(w_levels, 16) && aligned_to(x_levels, 16))) return rc;
    if (s.N == 0) return LSQ_OK;
    lsq::W8Act act{};
    act.a = static_cast<const uint8_t*>(x_levels);
    act.scale = static_cast<const float*>(s_x);
    act.zx = static_cast<const int32_t*>(zx);
    act.off = level_dtype == LSQ_QCONV_W8_U8 ? 128 : 0;
    act.fused = 0;
    const lsq::W8Weight wt = weight_arg(w_level_dtype, w_levels, w_scale, w_zero, bias, bias_dtype);
    return hip_status(lsq::conv_w8_launch(pl, act, wt, s, y, y_dtype, static_cast<hipStream_t>(stream)), what);
}

int lsq_qconv_w8_forward(int dtype, const void* x, const void* scale, const void* shift, int64_t quant_min, int64_t quant_max,
                         int64_t type_min, int64_t type_max, const lsq_qconv_w8_geom* geom, int w_level_dtype, const void* w_levels,
                         const void* w_scale, const void* w_zero, const void* bias, int bias_dtype, void* y, void* levels_ws,
                         void* stream) {
    const char* what = "lsq_qconv_w8_forward";
    lsq::W8ConvShape s;
    if (int rc = check_dtype(what, dtype)) return rc;
    if (int rc = check_conv_geom(what, geom, s)) return rc;
    if (int rc = check_byte_range(what, "", quant_min, quant_max, type_min, type_max)) return rc;
    if (!x || !scale || !shift) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (int rc = check_conv_weights(what, dtype, w_level_dtype, w_levels, w_scale, w_zero, bias, bias_dtype, y)) return rc;
    if (!aligned_to(x, elem_bytes(dtype))) return fail(LSQ_EINVAL, "%s: x and y must be element-aligned", what);
    if (!aligned_to(scale, 4) || !aligned_to(shift, 4))
        return fail(LSQ_EINVAL, "%s: scale and shift must be element-aligned", what);
    lsq::W8ConvPlan pl;
    if (int rc = checked_conv_plan(what, pl, s, aligned_to(w_levels, 16))) return rc;
    if (!levels_ws || !aligned_to(levels_ws, 16))
        return fail(LSQ_EINVAL, "%s: levels_ws must be a 16-byte aligned device buffer of B * H * W * Cin bytes", what);
    if (s.N == 0) return LSQ_OK;
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
    const lsq::W8Weight wt = weight_arg(w_level_dtype, w_levels, w_scale, w_zero, bias, bias_dtype);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e = hipSuccess;
    switch (dtype) {
        case LSQ_BF16: e = lsq::conv_w8_levels<lsq::io_bf16>(x, s.x_elems, act, levels_ws, st); break;
        case LSQ_F16: e = lsq::conv_w8_levels<lsq::io_f16>(x, s.x_elems, act, levels_ws, st); break;
        default: e = lsq::conv_w8_levels<lsq::io_f32>(x, s.x_elems, act, levels_ws, st); break;
    }
    if (e != hipSuccess) return hip_status(e, what);
    return hip_status(lsq::conv_w8_launch(pl, act, wt, s, y, dtype, st), what);
}

int lsq_qconv_w8_plan(const lsq_qconv_w8_geom* geom, int aligned, int32_t* out8) {
    const char* what = "lsq_qconv_w8_plan";
    lsq::W8ConvShape s;
    if (int rc = check_conv_geom(what, geom, s)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    lsq::W8ConvPlan pl;
    if (int rc = checked_conv_plan(what, pl, s, aligned != 0)) return rc;
    write_plan(pl, out8);
    return LSQ_OK;
}

}  // extern "C"
