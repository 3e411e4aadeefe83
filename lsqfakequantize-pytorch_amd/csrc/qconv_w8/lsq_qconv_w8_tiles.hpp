// lsq_qconv_w8_tiles.hpp -- the W8A8 TILES kernel with a float output on a packet source (lsq_w8_tiles_loop.hpp's body with
// the linear's store per output), and the fused form's pre-pass.
#pragma once
#include "lsq_w8_tiles_loop.hpp"

namespace lsq {

template <int SUBS, bool SPLITK, typename Src>
__device__ __forceinline__ void w8_tiles_body(const Src src, const W8Const ac, const W8Weight& wt, const W8Geom& geo,
                                              void* __restrict__ y, int y_dtype) {
    const W8TileAt at = w8_tile_at<SUBS, SPLITK>(geo);
    w8_tiles_run<SUBS, SPLITK>(src, ac, wt, geo, [] {}, [] {}, [&] {
        return [&](int64_t I, int m, int, int64_t n) { w8_store(I, wt, ac.s_x, n, y, y_dtype, (at.m0 + m) * geo.N + n); };
    });
}

// the fused form's pre-pass: ws[i] = level(x[i]) - off as a byte, 16 elements per thread and turn, then the tail
template <typename IO>
__device__ __forceinline__ void w8_levels_body(const void* __restrict__ x, int64_t n, const float* __restrict__ scale,
                                               const float* __restrict__ shift, float qmin, float qmax, float tmin, float tmax, int off,
                                               uint8_t* __restrict__ ws) {
    const Range<float> r = Range<float>{qmin, qmax, tmin, tmax};
    const QParams<float> qp = make_qparams<float>(sanitize_scale_per_tensor<float>(scale[0]), shift[0], r);
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock, n16 = n / 16;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    for (int64_t i = first; i < n16; i += stride) {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int a = static_cast<int>(level<float>(IO::load1(x, i * 16 + j), qp, r)) - off;
            w[j >> 2] |= static_cast<uint32_t>(a & 0xff) << ((j & 3) * 8);
        }
        *reinterpret_cast<u32x4*>(ws + i * 16) = u32x4{w[0], w[1], w[2], w[3]};
    }
    for (int64_t i = n16 * 16 + first; i < n; i += stride)
        ws[i] = static_cast<uint8_t>((static_cast<int>(level<float>(IO::load1(x, i), qp, r)) - off) & 0xff);
}

}  // namespace lsq
