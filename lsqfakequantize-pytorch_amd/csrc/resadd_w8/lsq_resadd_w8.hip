// lsq_resadd_w8.hip -- the W8A8 linear and conv2d that close a residual block on gfx950 (include/lsq_hip_resadd_w8.h, which
// states the contract): the kernels and the C ABI of liblsq_hip_resadd_w8.so.
//
//     v = ((s_w[n] * float(I)) * s_x) + bias[n],  u = float(round_to(mid, v)),  p = pre ? fake-quantize(u; pre) in mid : u,
//     d = float(round_to(mid, (float(l_r) - float(z_r)) * s_r)),  t = float(round_to(mid, p + d)),  r = relu ? (t < 0 ? 0 : t) : t,
//     y = level(r) of the OUTPUT quantizer, one byte
//
// with I the exact integer of csrc/qlinear_w8/ (rows of a dense [M, K] byte matrix) or csrc/qconv_w8/ (the implicit matrix of
// a channels-last convolution) and l_r the residual's level at the same (m, n).
//
//  * MATRIX-CORE form: lsq_resadd_w8_tiles.hpp's tile body on W8LinSrc (linear: K % 16 == 0, K <= 65536, lw and the levels
//    16-byte aligned) or W8ConvSrc (conv2d: Cin % 16 == 0, K <= 65536, the same alignment), SUBS 2 / 4 / 8, wide and split K.
//    M <= 16 takes the 32-row tile, as in csrc/requant_w8/.
//  * GENERIC form (every other legal call): the generic kernels' integer sum (one wave per output column and four rows),
//    the same epilogue function, one byte of the residual loaded per output, byte stores.  Correct, not tuned.
// W8ConvGeom, W8ConvSrc and w8_conv_row are csrc/qconv_w8/lsq_w8_conv_src.hpp's, the checks that are not the residual's or
// the pre-quantizer's csrc/qconv_w8/lsq_w8_host_checks.hpp's and csrc/requant_w8/lsq_requant_w8_checks.hpp's (check_out).  The
// plan is csrc/requant_w8/lsq_requant_w8.hip's, which is a translation unit and not a header: a fix there belongs here too.
#include "lsq_resadd_w8_tiles.hpp"
#include "../requant_w8/lsq_requant_w8_checks.hpp"
#include "../../../include/lsq_hip_resadd_w8.h"

namespace lsq {

// ------------------------------------------------------------------------------------------------
// matrix-core form
// ------------------------------------------------------------------------------------------------
template <int SUBS, bool SPLITK>
__global__ __launch_bounds__(kW8TileWaves * 64, 2) void resadd_w8_linear_tiles_kernel(W8Act act, W8Weight wt, W8Geom geo, W8OutArg out,
                                                                                     W8ResArg res, W8PreArg pre, uint8_t* __restrict__ y) {
    const W8Const ac = w8_constants(act);
    const W8LinSrc src{act.a, ac.flip, geo.K};
    w8r_tiles_body<SUBS, SPLITK>(src, ac, wt, geo, out, res, pre, y);
}

template <int SUBS, bool SPLITK>
__global__ __launch_bounds__(kW8TileWaves * 64, 2) void resadd_w8_conv_tiles_kernel(W8Act act, W8Weight wt, W8Geom geo, W8ConvGeom cg,
                                                                                   W8OutArg out, W8ResArg res, W8PreArg pre,
                                                                                   uint8_t* __restrict__ y) {
    const W8Const ac = w8_constants(act);
    w8r_tiles_body<SUBS, SPLITK>(w8_conv_src(act, ac, cg), ac, wt, geo, out, res, pre, y);
}

// ------------------------------------------------------------------------------------------------
// generic form: the integer sums of qlinear_w8_generic_kernel / qconv_w8_generic_kernel
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void resadd_w8_linear_generic_kernel(W8Act act, int64_t M, W8Weight wt, int64_t N, int64_t K,
                                                                         W8OutArg out, W8ResArg res, W8PreArg pre,
                                                                         uint8_t* __restrict__ y) {
    constexpr int R = kQGenericRowsAtOnce;
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int64_t wave = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
    const int64_t waves = static_cast<int64_t>(gridDim.x) * (kBlock / 64);
    const W8Const ac = w8_constants(act);
    const W8OutQ oq = w8q_constants(out);
    const W8PreQ pq = w8r_pre_constants(pre);
    const W8ResQ rq = w8r_res_constants(res);
    const uint8_t flipx = static_cast<uint8_t>(ac.flip & 0xffu), flipw = static_cast<uint8_t>(wt.off);
    for (int64_t n = wave; n < N; n += waves) {
        const uint8_t* __restrict__ wrow = wt.w + n * K;
        const int z_w = wt.zero[n] - wt.off;
        for (int64_t m0 = 0; m0 < M; m0 += R) {
            int64_t I[R];
#pragma unroll
            for (int i = 0; i < R; ++i) I[i] = 0;
            for (int64_t k = lane; k < K; k += 64) {
                const int64_t wz = static_cast<int>(static_cast<int8_t>(wrow[k] ^ flipw)) - z_w;
#pragma unroll
                for (int i = 0; i < R; ++i)
                    if (m0 + i < M) I[i] += (static_cast<int>(static_cast<int8_t>(act.a[(m0 + i) * K + k] ^ flipx)) - ac.z) * wz;
            }
#pragma unroll
            for (int i = 0; i < R; ++i) {
                for (int s = 32; s >= 1; s >>= 1) I[i] += w8_shfl_xor_i64(I[i], s);        // integers: any order
                if (lane == 0 && m0 + i < M) {
                    const int64_t at = (m0 + i) * N + n;
                    y[at] = w8r_byte(I[i], wt, ac.s_x, n, oq, pq, rq, res.l[at]);
                }
            }
        }
    }
}

__global__ __launch_bounds__(kBlock) void resadd_w8_conv_generic_kernel(W8Act act, W8Weight wt, W8Geom geo, W8ConvGeom cg, W8OutArg out,
                                                                       W8ResArg res, W8PreArg pre, uint8_t* __restrict__ y) {
    constexpr int R = kQGenericRowsAtOnce;
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int64_t wave = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
    const int64_t waves = static_cast<int64_t>(gridDim.x) * (kBlock / 64);
    const int64_t M = geo.M, N = geo.N, K = geo.K;
    const int64_t items = (M + R - 1) / R * N;              // (four output pixels, output channel)
    const W8Const ac = w8_constants(act);
    const W8OutQ oq = w8q_constants(out);
    const W8PreQ pq = w8r_pre_constants(pre);
    const W8ResQ rq = w8r_res_constants(res);
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
            if (lane == 0 && m0 + i < M) {
                const int64_t at = (m0 + i) * N + n;
                y[at] = w8r_byte(I[i], wt, ac.s_x, n, oq, pq, rq, res.l[at]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side: the plan and the launchers
// ------------------------------------------------------------------------------------------------
struct W8RPlan {
    int form, shape, block, lds, rows, cols, ksplit, subs, store, res_load;
    int64_t grid, row_tiles, col_tiles;
};

// the plan of lsq_hip_requant_w8.h on (M, N, K); `mfma`: the form's preconditions hold; `generic_grid`: form 0's grid
inline W8RPlan plan_resadd_w8(int64_t M, int64_t N, int64_t K, bool mfma, int generic_cols, int64_t generic_blocks, bool y_aligned,
                              bool res_aligned) {
    W8RPlan pl = {};
    const int64_t cus = device_info().cu_count;
    pl.store = LSQ_REQUANT_W8_STORE_BYTES;
    pl.res_load = LSQ_RESADD_W8_LOAD_BYTES;
    if (!mfma) {
        pl.form = 0;
        pl.shape = LSQ_REQUANT_W8_SHAPE_GENERIC;
        pl.block = kBlock;
        pl.rows = kQGenericRowsAtOnce;
        pl.cols = generic_cols;
        pl.ksplit = 1;
        pl.grid = generic_blocks;
        return pl;
    }
    pl.form = 1;
    pl.subs = M <= 32 ? 2 : (M <= 64 ? 4 : kW8MaxSubs);
    pl.rows = pl.subs * 16;
    pl.row_tiles = (M + pl.rows - 1) / pl.rows;
    const int64_t wide = (N + 16 * kW8TileWaves - 1) / (16 * kW8TileWaves);
    // 64-column tiles once they give every compute unit a tile; below that 16-column tiles, four times as many, K split over the waves
    const bool split = wide <= INT64_MAX / pl.row_tiles && pl.row_tiles * wide < cus;
    pl.shape = split ? LSQ_REQUANT_W8_SHAPE_TILES_SPLIT_K : LSQ_REQUANT_W8_SHAPE_TILES;
    pl.cols = split ? kW8Tile : 16 * kW8TileWaves;
    pl.ksplit = split ? kW8TileWaves : 1;
    pl.col_tiles = (N + pl.cols - 1) / pl.cols;
    pl.grid = pl.col_tiles <= INT64_MAX / pl.row_tiles ? pl.row_tiles * pl.col_tiles : INT64_MAX;
    pl.block = kW8TileWaves * 64;
    pl.lds = w8_tiles_lds(pl.subs);
    pl.store = (N % 16 == 0 && y_aligned) ? LSQ_REQUANT_W8_STORE_PACKETS : LSQ_REQUANT_W8_STORE_BYTES;
    pl.res_load = (N % 16 == 0 && res_aligned) ? LSQ_RESADD_W8_LOAD_PACKETS : LSQ_RESADD_W8_LOAD_BYTES;
    return pl;
}

inline W8RPlan plan_resadd_linear(int64_t M, int64_t N, int64_t K, bool aligned, bool y_aligned, bool res_aligned) {
    const int64_t cus = device_info().cu_count;
    return plan_resadd_w8(M, N, K, aligned && K > 0 && K % 16 == 0 && K <= kW8MaxK, kBlock / 64, generic_grid(N, cus), y_aligned,
                          res_aligned);
}

inline W8RPlan plan_resadd_conv(const W8ConvShape& s, bool aligned, bool y_aligned, bool res_aligned) {
    const int64_t cus = device_info().cu_count;
    const int64_t per_block = kBlock / 64, blocks = (s.M + kQGenericRowsAtOnce - 1) / kQGenericRowsAtOnce;
    const int64_t items = blocks <= INT64_MAX / std::max<int64_t>(1, s.N) ? blocks * s.N : INT64_MAX;
    const int64_t grid = std::min(std::max<int64_t>(1, items / per_block + (items % per_block ? 1 : 0)), cus * 8);
    return plan_resadd_w8(s.M, s.N, s.K, aligned && s.cg.Cin % 16 == 0 && s.K <= kW8MaxK, 1, grid, y_aligned, res_aligned);
}

template <int SUBS, bool SPLITK>
static hipError_t resadd_launch_tiles(const W8RPlan& pl, const W8Act& act, const W8Weight& wt, const W8Geom& geo, const W8ConvGeom* cg,
                                      const W8OutArg& out, const W8ResArg& res, const W8PreArg& pre, uint8_t* y, hipStream_t stream) {
    static_assert(w8_tiles_lds(SUBS) <= 64 * 1024, "the tile fits the LDS a kernel gets unasked");
    static_assert(kW8TileWaves * SUBS * 64 * 16 <= SUBS * 16 * kW8TileStride, "the split-K tiles fit the staging area");
    const dim3 grid(static_cast<unsigned>(pl.grid)), block(kW8TileWaves * 64);
    if (cg) hipLaunchKernelGGL((resadd_w8_conv_tiles_kernel<SUBS, SPLITK>), grid, block, pl.lds, stream, act, wt, geo, *cg, out, res, pre,
                               y);
    else hipLaunchKernelGGL((resadd_w8_linear_tiles_kernel<SUBS, SPLITK>), grid, block, pl.lds, stream, act, wt, geo, out, res, pre, y);
    return hipGetLastError();
}

template <bool SPLITK>
static hipError_t resadd_subs(const W8RPlan& pl, const W8Act& act, const W8Weight& wt, const W8Geom& geo, const W8ConvGeom* cg,
                              const W8OutArg& out, const W8ResArg& res, const W8PreArg& pre, uint8_t* y, hipStream_t s) {
    if (pl.subs == 2) return resadd_launch_tiles<2, SPLITK>(pl, act, wt, geo, cg, out, res, pre, y, s);
    if (pl.subs == 4) return resadd_launch_tiles<4, SPLITK>(pl, act, wt, geo, cg, out, res, pre, y, s);
    return resadd_launch_tiles<kW8MaxSubs, SPLITK>(pl, act, wt, geo, cg, out, res, pre, y, s);
}

// `cg`: the convolution's geometry, NULL for a linear layer
static hipError_t resadd_launch(const W8RPlan& pl, const W8Act& act, const W8Weight& wt, int64_t M, int64_t N, int64_t K,
                                const W8ConvGeom* cg, W8OutArg out, W8ResArg res, const W8PreArg& pre, uint8_t* y, hipStream_t stream) {
    const W8Geom geo{M, N, K, pl.row_tiles};
    out.packets = pl.store == LSQ_REQUANT_W8_STORE_PACKETS ? 1 : 0;
    res.packets = pl.res_load == LSQ_RESADD_W8_LOAD_PACKETS ? 1 : 0;
    if (pl.shape == LSQ_REQUANT_W8_SHAPE_GENERIC) {
        const dim3 grid(static_cast<unsigned>(pl.grid)), block(kBlock);
        if (cg) hipLaunchKernelGGL(resadd_w8_conv_generic_kernel, grid, block, 0, stream, act, wt, geo, *cg, out, res, pre, y);
        else hipLaunchKernelGGL(resadd_w8_linear_generic_kernel, grid, block, 0, stream, act, M, wt, N, K, out, res, pre, y);
        return hipGetLastError();
    }
    return pl.shape == LSQ_REQUANT_W8_SHAPE_TILES_SPLIT_K ? resadd_subs<true>(pl, act, wt, geo, cg, out, res, pre, y, stream)
                                                          : resadd_subs<false>(pl, act, wt, geo, cg, out, res, pre, y, stream);
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_resadd_w8.h: validation, dtype dispatch, error bookkeeping
// ------------------------------------------------------------------------------------------------
namespace {

// the residual's and the pre-quantizer's checks; `MN`: the bytes of y and of the residual
int check_res(const char* what, const lsq_resadd_w8_res* r, const void* y, int64_t MN, lsq::W8ResArg& arg) {
    if (!r) return fail(LSQ_EINVAL, "%s: NULL residual (without one the op is lsq_hip_requant_w8.h's)", what);
    if (r->level_dtype != LSQ_REQUANT_W8_U8 && r->level_dtype != LSQ_REQUANT_W8_I8)
        return fail(LSQ_EINVAL, "%s: the residual's level_dtype must be LSQ_REQUANT_W8_U8 (0) or LSQ_REQUANT_W8_I8 (1), got %lld", what,
                    static_cast<ll>(r->level_dtype));
    if (!r->levels || !r->scale || !r->zero_point) return fail(LSQ_EINVAL, "%s: NULL residual levels, scale or zero_point", what);
    if (!aligned_to(r->scale, 4) || !aligned_to(r->zero_point, 4))
        return fail(LSQ_EINVAL, "%s: the residual's scale and zero_point must be element-aligned", what);
    const uintptr_t a = reinterpret_cast<uintptr_t>(r->levels), b = reinterpret_cast<uintptr_t>(y), n = static_cast<uintptr_t>(MN);
    if (a < b + n && b < a + n)
        return fail(LSQ_EINVAL, "%s: the residual's %lld bytes overlap y's: an in-place add is not served", what, static_cast<ll>(MN));
    arg = lsq::W8ResArg{static_cast<const uint8_t*>(r->levels), static_cast<const float*>(r->scale),
                        static_cast<const int32_t*>(r->zero_point), r->level_dtype == LSQ_REQUANT_W8_I8 ? 1 : 0, 0};
    return LSQ_OK;
}

int check_pre(const char* what, const lsq_resadd_w8_pre* p, lsq::W8PreArg& arg) {
    arg = lsq::W8PreArg{nullptr, nullptr, 0.0f, 0.0f, 0.0f, 0.0f};
    if (!p) return LSQ_OK;
    if (!p->scale || !p->shift) return fail(LSQ_EINVAL, "%s: NULL scale or shift of the pre-quantizer", what);
    if (!aligned_to(p->scale, 4) || !aligned_to(p->shift, 4))
        return fail(LSQ_EINVAL, "%s: the pre-quantizer's scale and shift must be element-aligned", what);
    if (int rc = check_byte_range(what, "the pre-quantizer's ", p->quant_min, p->quant_max, p->type_min, p->type_max)) return rc;
    arg = lsq::W8PreArg{static_cast<const float*>(p->scale), static_cast<const float*>(p->shift), static_cast<float>(p->quant_min),
                        static_cast<float>(p->quant_max), static_cast<float>(p->type_min), static_cast<float>(p->type_max)};
    return LSQ_OK;
}

}  // namespace

extern "C" {

int lsq_resadd_w8_abi_version(void) { return LSQ_RESADD_W8_ABI_VERSION; }

const char* lsq_resadd_w8_last_error(void) { return g_last_error; }

int lsq_resadd_w8_linear_levels(int level_dtype, const void* x_levels, int64_t M, const void* s_x, const void* zx, int w_level_dtype,
                                const void* w_levels, int64_t N, int64_t K, const void* w_scale, const void* w_zero, const void* bias,
                                int bias_dtype, const lsq_requant_w8_out* out, const lsq_resadd_w8_res* res, const lsq_resadd_w8_pre* pre,
                                void* y, void* stream) {
    const char* what = "lsq_resadd_w8_linear_levels";
    int mid = 0;
    lsq::W8OutArg oa{};
    lsq::W8ResArg ra{};
    lsq::W8PreArg pa{};
    if (int rc = check_out(what, out, mid, oa)) return rc;
    if (int rc = check_linear_shape(what, M, N, K)) return rc;
    if (int rc = check_levels_in(what, kCodes, level_dtype, x_levels, s_x, zx)) return rc;
    if (int rc = check_weights(what, kCodes, mid, w_level_dtype, w_levels, w_scale, w_zero, bias, bias_dtype, y)) return rc;
    if (int rc = check_res(what, res, y, M * N, ra)) return rc;
    if (int rc = check_pre(what, pre, pa)) return rc;
    const lsq::W8RPlan pl = lsq::plan_resadd_linear(M, N, K, aligned_to(w_levels, 16) && aligned_to(x_levels, 16), aligned_to(y, 16),
                                                    aligned_to(res->levels, 16));
    if (int rc = check_grid(what, pl.grid, M, N)) return rc;
    if (N == 0) return LSQ_OK;
    return hip_status(lsq::resadd_launch(pl, levels_act(level_dtype, x_levels, s_x, zx),
                                         weight_arg(w_level_dtype, w_levels, w_scale, w_zero, bias, bias_dtype), M, N, K, nullptr, oa, ra,
                                         pa, static_cast<uint8_t*>(y), static_cast<hipStream_t>(stream)), what);
}

int lsq_resadd_w8_conv_levels(int level_dtype, const void* x_levels, const void* s_x, const void* zx, const lsq_qconv_w8_geom* geom,
                              int w_level_dtype, const void* w_levels, const void* w_scale, const void* w_zero, const void* bias,
                              int bias_dtype, const lsq_requant_w8_out* out, const lsq_resadd_w8_res* res, const lsq_resadd_w8_pre* pre,
                              void* y, void* stream) {
    const char* what = "lsq_resadd_w8_conv_levels";
    int mid = 0;
    lsq::W8OutArg oa{};
    lsq::W8ResArg ra{};
    lsq::W8PreArg pa{};
    lsq::W8ConvShape s;
    if (int rc = check_out(what, out, mid, oa)) return rc;
    if (int rc = check_conv_geom(what, geom, s)) return rc;
    if (int rc = check_levels_in(what, kCodes, level_dtype, x_levels, s_x, zx)) return rc;
    if (int rc = check_weights(what, kCodes, mid, w_level_dtype, w_levels, w_scale, w_zero, bias, bias_dtype, y)) return rc;
    if (int rc = check_res(what, res, y, s.M * s.N, ra)) return rc;
    if (int rc = check_pre(what, pre, pa)) return rc;
    const lsq::W8RPlan pl = lsq::plan_resadd_conv(s, aligned_to(w_levels, 16) && aligned_to(x_levels, 16), aligned_to(y, 16),
                                                  aligned_to(res->levels, 16));
    if (int rc = check_grid(what, pl.grid, s.M, s.N)) return rc;
    if (s.N == 0) return LSQ_OK;
    return hip_status(lsq::resadd_launch(pl, levels_act(level_dtype, x_levels, s_x, zx),
                                         weight_arg(w_level_dtype, w_levels, w_scale, w_zero, bias, bias_dtype), s.M, s.N, s.K, &s.cg, oa,
                                         ra, pa, static_cast<uint8_t*>(y), static_cast<hipStream_t>(stream)), what);
}

int lsq_resadd_w8_plan_linear(int64_t M, int64_t N, int64_t K, int aligned, int y_aligned, int res_aligned, int32_t* out10) {
    const char* what = "lsq_resadd_w8_plan_linear";
    if (int rc = check_linear_shape(what, M, N, K)) return rc;
    if (!out10) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::W8RPlan pl = lsq::plan_resadd_linear(M, N, K, aligned != 0, y_aligned != 0, res_aligned != 0);
    if (int rc = check_grid(what, pl.grid, M, N)) return rc;
    write_plan(pl, out10);
    out10[8] = pl.store;
    out10[9] = pl.res_load;
    return LSQ_OK;
}

int lsq_resadd_w8_plan_conv(const lsq_qconv_w8_geom* geom, int aligned, int y_aligned, int res_aligned, int32_t* out10) {
    const char* what = "lsq_resadd_w8_plan_conv";
    lsq::W8ConvShape s;
    if (int rc = check_conv_geom(what, geom, s)) return rc;
    if (!out10) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::W8RPlan pl = lsq::plan_resadd_conv(s, aligned != 0, y_aligned != 0, res_aligned != 0);
    if (int rc = check_grid(what, pl.grid, s.M, s.N)) return rc;
    write_plan(pl, out10);
    out10[8] = pl.store;
    out10[9] = pl.res_load;
    return LSQ_OK;
}

}  // extern "C"
