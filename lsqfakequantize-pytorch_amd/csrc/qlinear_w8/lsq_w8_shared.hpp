// lsq_w8_shared.hpp -- what the W8A8 kernels on 8-bit levels share (csrc/qlinear_w8/, csrc/qconv_w8/): the kernel arguments,
// the constants of the byte operands, the 16-byte load of the A operand, and the fp32 steps of the contract on the exact
// integer (include/lsq_hip_qlinear_w8.h states the arithmetic).  Scalar pieces only: moved here they leave every kernel of
// liblsq_hip_qlinear_w8.so instruction for instruction as it was (profiles/r16_qconv_w8_isa_diff.txt); the TILES kernel's
// body as a shared function template does not (same file), so the linear keeps its own and the convolution's is
// csrc/qconv_w8/lsq_qconv_w8_tiles.hpp.
#pragma once
#include "../qlinear/lsq_qdecode.hpp"

#include <climits>

namespace lsq {

constexpr int kW8Tile = 16;                         // output columns of one MFMA tile
constexpr int kW8Step = 256;                        // elements of K per wave and chunk (decode), per step (tiles)
constexpr int kW8RowPad = 16;                       // bytes between rows of x in LDS beyond their data
constexpr int kW8MaxK = 65536;                      // |a w| <= 2^14: the raw sum fits 32 bits up to here
constexpr int kW8MaxSubs = 8;                       // tiles: most 16-row sub-tiles per workgroup
constexpr int kW8TileWaves = 4;
constexpr int kW8TileStride = kW8Step + kW8RowPad;

struct W8Act {              // kernel argument: where the byte operand a and its constants come from
    const uint8_t* a;       // levels form: the levels; fused form: the workspace, a = level(x) - off already
    const float* scale;     // levels form: s_x; fused form: the quantizer's scale
    const float* shift;     // fused form
    const int32_t* zx;      // levels form
    float qmin, qmax, tmin, tmax;   // fused form
    int off;                // 128: levels in 0..255; 0: levels in -128..127
    int fused;
    int aligned;            // `a` is 16-byte aligned
};

struct W8Const {
    int z;                  // zx - off
    float s_x;
    uint32_t flip;          // byte ^ 0x80 read as int8 is byte - 128
};

struct W8Weight {           // kernel argument
    const uint8_t* w;       // lw [N, K]
    const float* scale;     // s_w [N]
    const int32_t* zero;    // zw [N]
    const void* bias;
    int bias_dtype;
    int off;                // 128: uint8 levels; 0: int8
};

struct W8Geom {             // kernel argument
    int64_t M, N, K, row_tiles;
};

__device__ __forceinline__ W8Const w8_constants(const W8Act& a) {
    W8Const c;
    if (a.fused) {
        const Range<float> r = Range<float>{a.qmin, a.qmax, a.tmin, a.tmax};
        const QParams<float> q = make_qparams<float>(sanitize_scale_per_tensor<float>(a.scale[0]), a.shift[0], r);
        c.z = static_cast<int>(q.zp) - a.off;
        c.s_x = q.s;
        c.flip = 0u;
    } else {
        c.z = a.zx[0] - a.off;
        c.s_x = a.scale[0];
        c.flip = a.off ? 0x80808080u : 0u;
    }
    return c;
}

// 16 byte operands of x from element `at` on
__device__ __forceinline__ u32x4 w8_load16(const W8Act& act, uint32_t flip, int64_t at) {
    const uint8_t* src = act.a + at;
    u32x4 v;
    if (act.aligned) {
        v = *reinterpret_cast<const u32x4*>(src);
    } else {
        uint32_t d[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 16; ++j) d[j >> 2] |= static_cast<uint32_t>(src[j]) << ((j & 3) * 8);
        v = u32x4{d[0], d[1], d[2], d[3]};
    }
    return v ^ flip;
}

__device__ __forceinline__ int w8_sum_bytes(uint32_t w) {
    return static_cast<int>(static_cast<int8_t>(w)) + static_cast<int>(static_cast<int8_t>(w >> 8)) +
           static_cast<int>(static_cast<int8_t>(w >> 16)) + (static_cast<int>(w) >> 24);
}

__device__ __forceinline__ float w8_bias_at(const void* bias, int bias_dtype, int64_t n) {
    switch (bias_dtype) {
        case LSQ_BF16: return io_bf16::load1(bias, n);
        case LSQ_F16: return io_f16::load1(bias, n);
        default: return static_cast<const float*>(bias)[n];
    }
}

// the fp32 steps of the contract on the exact integer, and the one rounding to y
__device__ __forceinline__ void w8_store(int64_t I, const W8Weight& wt, float s_x, int64_t n, void* y, int y_dtype, int64_t at) {
    float v = __fmul_rn(__fmul_rn(wt.scale[n], static_cast<float>(I)), s_x);
    if (wt.bias) v = __fadd_rn(v, w8_bias_at(wt.bias, wt.bias_dtype, n));
    if (y_dtype == LSQ_BF16) store_out<io_bf16, false>(y, at, v);
    else if (y_dtype == LSQ_F16) store_out<io_f16, false>(y, at, v);
    else store_out<io_f32, false>(y, at, v);
}

// I from the raw sums: P = sum a w, C = sum_k w, S = sum_k a
__device__ __forceinline__ int64_t w8_exact(int64_t P, int64_t C, int64_t S, int64_t K, int z_a, int z_w) {
    return P - static_cast<int64_t>(z_a) * C - static_cast<int64_t>(z_w) * S + K * z_a * static_cast<int64_t>(z_w);
}

__device__ __forceinline__ i32x4 w8_as_i32(u32x4 v) {
    return i32x4{static_cast<int>(v.x), static_cast<int>(v.y), static_cast<int>(v.z), static_cast<int>(v.w)};
}

__device__ __forceinline__ int64_t w8_shfl_xor_i64(int64_t v, int mask) {
    int lo = static_cast<int>(static_cast<uint64_t>(v) & 0xffffffffu), hi = static_cast<int>(static_cast<uint64_t>(v) >> 32);
    lo = __shfl_xor(lo, mask, 64);
    hi = __shfl_xor(hi, mask, 64);
    return static_cast<int64_t>((static_cast<uint64_t>(static_cast<uint32_t>(hi)) << 32) | static_cast<uint32_t>(lo));
}

constexpr int w8_tiles_lds(int subs) { return subs * 16 * kW8TileStride + subs * 16 * 4 * 4 + kW8TileWaves * 16 * 4; }

}  // namespace lsq
