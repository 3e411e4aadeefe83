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
// W8ConvGeom, W8ConvSrc, w8_conv_row, the geometry's checks and the plan are csrc/qconv_w8/lsq_qconv_w8.hip's and
// csrc/requant_w8/lsq_requant_w8.hip's, which are translation units and not headers: a fix there belongs here too.
#include "lsq_resadd_w8_tiles.hpp"
#include "../../../include/lsq_hip_resadd_w8.h"

namespace lsq {

struct W8ConvGeom {         // kernel argument; the host has checked that the coordinates fit 32 bits
    int64_t Cin, OH, OW, image;     // image = H W Cin, the bytes of one image of x
    int H, W, kw, sh, sw, ph, pw, dh, dw;
};

struct W8ConvRow {          // output pixel m = (b, oh, ow): where its receptive field starts
    int64_t base;           // b * image
    int ih0, iw0;           // oh sh - ph, ow sw - pw
};

__device__ __forceinline__ W8ConvRow w8_conv_row(int64_t m, int64_t OH, int64_t OW, int64_t image, int sh, int sw, int ph, int pw) {
    const int64_t t = m / OW, ow = m - t * OW;
    const int64_t b = t / OH, oh = t - b * OH;
    W8ConvRow r;
    r.base = b * image;
    r.ih0 = static_cast<int>(oh * sh - ph);
    r.iw0 = static_cast<int>(ow * sw - pw);
    return r;
}

// the implicit [B OH OW, kh kw Cin] matrix of byte operands, Cin % 16 == 0 and K <= 65536 (scalars only)
struct W8ConvSrc {
    const uint8_t* a;
    uint32_t flip;          // of a loaded packet
    uint32_t pad;           // four times the byte zx - off: a tap in the padding
    int64_t OH, OW, image;
    unsigned H, W, Cin, kw, dh, dw;
    int sh, sw, ph, pw;
    typedef W8ConvRow Row;
    struct Col {            // k = (i kw + j) Cin + c
        unsigned idh, jdw;  // i dh, j dw
        unsigned j, c;
    };
    __device__ __forceinline__ Row row(int64_t m) const { return w8_conv_row(m, OH, OW, image, sh, sw, ph, pw); }
    __device__ __forceinline__ Col col(int64_t k) const {
        const unsigned kk = static_cast<unsigned>(k);
        const unsigned tap = kk / Cin, i = tap / kw, j = tap - i * kw;
        return Col{i * dh, j * dw, j, kk - tap * Cin};
    }
    __device__ __forceinline__ void advance(Col& p) const {     // 16 bytes further: Cin % 16 == 0, so c reaches Cin exactly
        p.c += 16u;
        if (p.c >= Cin) {
            p.c = 0u;
            p.j += 1u;
            p.jdw += dw;
            if (p.j == kw) {
                p.j = 0u;
                p.jdw = 0u;
                p.idh += dh;
            }
        }
    }
    __device__ __forceinline__ u32x4 packet(const Row& r, const Col& p) const {
        const unsigned ih = static_cast<unsigned>(r.ih0) + p.idh, iw = static_cast<unsigned>(r.iw0) + p.jdw;   // negative: huge
        u32x4 v = {pad, pad, pad, pad};
        if (ih < H && iw < W) {
            const int64_t at = r.base + (static_cast<int64_t>(ih) * W + iw) * Cin + p.c;
            v = *reinterpret_cast<const u32x4*>(a + at) ^ flip;
        }
        return v;
    }
};

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
    const uint32_t pad = static_cast<uint32_t>(ac.z & 0xff) * 0x01010101u;
    const W8ConvSrc src{act.a, ac.flip, pad, cg.OH, cg.OW, cg.image, static_cast<unsigned>(cg.H), static_cast<unsigned>(cg.W),
                        static_cast<unsigned>(cg.Cin), static_cast<unsigned>(cg.kw), static_cast<unsigned>(cg.dh),
                        static_cast<unsigned>(cg.dw), cg.sh, cg.sw, cg.ph, cg.pw};
    w8r_tiles_body<SUBS, SPLITK>(src, ac, wt, geo, out, res, pre, y);
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
struct W8ConvShape {        // a checked geometry
    int64_t M, N, K, OH, OW, x_elems;
    W8ConvGeom cg;
};

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

typedef long long ll;

// the output quantizer's checks; the mid dtype (which takes the place of y's dtype in the other checks) into `mid`
int check_out(const char* what, const lsq_requant_w8_out* o, int& mid, lsq::W8OutArg& arg) {
    if (!o) return fail(LSQ_EINVAL, "%s: NULL output quantizer", what);
    if (o->mid_dtype != LSQ_F32 && o->mid_dtype != LSQ_BF16 && o->mid_dtype != LSQ_F16)
        return fail(LSQ_EINVAL, "%s: mid_dtype must be LSQ_F32, LSQ_BF16 or LSQ_F16, got code %lld", what, static_cast<ll>(o->mid_dtype));
    if (!o->out_scale || !o->out_shift) return fail(LSQ_EINVAL, "%s: NULL out_scale or out_shift", what);
    if (!aligned_to(o->out_scale, 4) || !aligned_to(o->out_shift, 4))
        return fail(LSQ_EINVAL, "%s: out_scale and out_shift must be element-aligned", what);
    const ll lo = std::min(o->quant_min, o->type_min), hi = std::max(o->quant_max, o->type_max);
    if (o->quant_min > o->quant_max || o->type_min > o->type_max || !((lo >= 0 && hi <= 255) || (lo >= -128 && hi <= 127)))
        return fail(LSQ_EINVAL, "%s: the output's [quant_min, quant_max] = [%lld, %lld] and [type_min, type_max] = [%lld, %lld] must "
                    "lie within 0..255 or within -128..127", what, static_cast<ll>(o->quant_min), static_cast<ll>(o->quant_max),
                    static_cast<ll>(o->type_min), static_cast<ll>(o->type_max));
    mid = static_cast<int>(o->mid_dtype);
    arg = lsq::W8OutArg{static_cast<const float*>(o->out_scale), static_cast<const float*>(o->out_shift),
                        static_cast<float>(o->quant_min), static_cast<float>(o->quant_max), static_cast<float>(o->type_min),
                        static_cast<float>(o->type_max), o->relu ? 1 : 0, mid, 0};
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

// the geometry's checks (check_conv_geom of csrc/qconv_w8/lsq_qconv_w8.hip); fills `s`
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

int check_level_dtype(const char* what, const char* name, int code) {
    if (code != LSQ_REQUANT_W8_U8 && code != LSQ_REQUANT_W8_I8)
        return fail(LSQ_EINVAL, "%s: %s must be LSQ_REQUANT_W8_U8 (0) or LSQ_REQUANT_W8_I8 (1), got %d", what, name, code);
    return LSQ_OK;
}

// `mid`: the dtype of the unfused op's y
int check_weights(const char* what, int mid, int w_level_dtype, const void* w_levels, const void* w_scale, const void* w_zero,
                  const void* bias, int bias_dtype, const void* y) {
    if (int rc = check_level_dtype(what, "w_level_dtype", w_level_dtype)) return rc;
    if (!w_levels || !w_scale || !w_zero || !y) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (bias && bias_dtype != LSQ_F32 && bias_dtype != mid)
        return fail(LSQ_EINVAL, "%s: the bias must be float32 or of mid_dtype, got dtype code %d", what, bias_dtype);
    if (!aligned_to(w_scale, 4) || !aligned_to(w_zero, 4) || (bias && !aligned_to(bias, elem_bytes(bias_dtype))))
        return fail(LSQ_EINVAL, "%s: w_scale, w_zero and bias must be element-aligned", what);
    return LSQ_OK;
}

int check_levels_in(const char* what, int level_dtype, const void* x_levels, const void* s_x, const void* zx) {
    if (int rc = check_level_dtype(what, "level_dtype", level_dtype)) return rc;
    if (!x_levels || !s_x || !zx) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (!aligned_to(s_x, 4) || !aligned_to(zx, 4)) return fail(LSQ_EINVAL, "%s: s_x and zx must be element-aligned", what);
    return LSQ_OK;
}

int check_grid(const char* what, const lsq::W8RPlan& pl, int64_t M, int64_t N) {
    if (pl.grid > INT32_MAX)
        return fail(LSQ_EINVAL, "%s: %lld rows by %lld output columns are beyond a 31-bit grid", what, static_cast<ll>(M), static_cast<ll>(N));
    return LSQ_OK;
}

lsq::W8Act levels_act(int level_dtype, const void* x_levels, const void* s_x, const void* zx) {
    lsq::W8Act act{};
    act.a = static_cast<const uint8_t*>(x_levels);
    act.scale = static_cast<const float*>(s_x);
    act.zx = static_cast<const int32_t*>(zx);
    act.off = level_dtype == LSQ_REQUANT_W8_U8 ? 128 : 0;
    act.fused = 0;
    act.aligned = aligned_to(x_levels, 16) ? 1 : 0;
    return act;
}

lsq::W8Weight weight_arg(int w_level_dtype, const void* w_levels, const void* w_scale, const void* w_zero, const void* bias, int bias_dtype) {
    return lsq::W8Weight{static_cast<const uint8_t*>(w_levels), static_cast<const float*>(w_scale), static_cast<const int32_t*>(w_zero),
                         bias, bias_dtype, w_level_dtype == LSQ_REQUANT_W8_U8 ? 128 : 0};
}

void write_plan(const lsq::W8RPlan& pl, int32_t* out10) {
    out10[0] = pl.form;
    out10[1] = pl.shape;
    out10[2] = static_cast<int32_t>(pl.grid);
    out10[3] = pl.block;
    out10[4] = pl.rows;
    out10[5] = pl.cols;
    out10[6] = pl.lds;
    out10[7] = pl.ksplit;
    out10[8] = pl.store;
    out10[9] = pl.res_load;
}

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
    const ll lo = std::min(p->quant_min, p->type_min), hi = std::max(p->quant_max, p->type_max);
    if (p->quant_min > p->quant_max || p->type_min > p->type_max || !((lo >= 0 && hi <= 255) || (lo >= -128 && hi <= 127)))
        return fail(LSQ_EINVAL, "%s: the pre-quantizer's [quant_min, quant_max] = [%lld, %lld] and [type_min, type_max] = [%lld, %lld] "
                    "must lie within 0..255 or within -128..127", what, static_cast<ll>(p->quant_min), static_cast<ll>(p->quant_max),
                    static_cast<ll>(p->type_min), static_cast<ll>(p->type_max));
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
    if (int rc = check_levels_in(what, level_dtype, x_levels, s_x, zx)) return rc;
    if (int rc = check_weights(what, mid, w_level_dtype, w_levels, w_scale, w_zero, bias, bias_dtype, y)) return rc;
    if (int rc = check_res(what, res, y, M * N, ra)) return rc;
    if (int rc = check_pre(what, pre, pa)) return rc;
    const lsq::W8RPlan pl = lsq::plan_resadd_linear(M, N, K, aligned_to(w_levels, 16) && aligned_to(x_levels, 16), aligned_to(y, 16),
                                                    aligned_to(res->levels, 16));
    if (int rc = check_grid(what, pl, M, N)) return rc;
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
    if (int rc = check_levels_in(what, level_dtype, x_levels, s_x, zx)) return rc;
    if (int rc = check_weights(what, mid, w_level_dtype, w_levels, w_scale, w_zero, bias, bias_dtype, y)) return rc;
    if (int rc = check_res(what, res, y, s.M * s.N, ra)) return rc;
    if (int rc = check_pre(what, pre, pa)) return rc;
    const lsq::W8RPlan pl = lsq::plan_resadd_conv(s, aligned_to(w_levels, 16) && aligned_to(x_levels, 16), aligned_to(y, 16),
                                                  aligned_to(res->levels, 16));
    if (int rc = check_grid(what, pl, s.M, s.N)) return rc;
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
    if (int rc = check_grid(what, pl, M, N)) return rc;
    write_plan(pl, out10);
    return LSQ_OK;
}

int lsq_resadd_w8_plan_conv(const lsq_qconv_w8_geom* geom, int aligned, int y_aligned, int res_aligned, int32_t* out10) {
    const char* what = "lsq_resadd_w8_plan_conv";
    lsq::W8ConvShape s;
    if (int rc = check_conv_geom(what, geom, s)) return rc;
    if (!out10) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::W8RPlan pl = lsq::plan_resadd_conv(s, aligned != 0, y_aligned != 0, res_aligned != 0);
    if (int rc = check_grid(what, pl, s.M, s.N)) return rc;
    write_plan(pl, out10);
    return LSQ_OK;
}

}  // extern "C"
