// lsq_w8_out_side.hpp -- the output side of the level ops (pool_w8, dwconv_w8, eltwise_w8, norm_w8, attn_w8, attn_fused_w8), once:
// a float32 value is rounded to mid_dtype and leaves either as one level byte of a per-tensor output quantizer or as itself,
// stored as mid_dtype.  Device code.  (The tile kernels' levels-only output is W8OutArg of requant_w8/lsq_requant_w8_tiles.hpp.)
//
// A library's kernel argument names the fields `scale` (NULL: a floating y), `shift`, `qmin`, `qmax`, `tmin`, `tmax`, `mid`; its
// per-thread constants struct inherits W8OutSide and w8o_constants() fills that part.  The helpers are templates over the
// constants struct and read only its `qp`, `r`, `levels_out` and `mid`: norm_w8 keeps a struct and an order of its own
// (DESIGN.md 9.17).
#pragma once
#include "lsq_kernels.hpp"

namespace lsq {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;     // the same type as qlinear/lsq_qdecode.hpp's, which may come too

struct W8OutSide {          // the constants of the output side, read once per thread
    QParams<float> qp;
    Range<float> r;
    int levels_out, mid;
};

template <typename Arg>
__device__ __forceinline__ void w8o_constants(W8OutSide& q, const Arg& a) {
    q.r = Range<float>{a.qmin, a.qmax, a.tmin, a.tmax};
    q.levels_out = a.scale != nullptr;
    if (q.levels_out) q.qp = make_qparams<float>(sanitize_scale_per_tensor<float>(a.scale[0]), a.shift[0], q.r);
    else q.qp = QParams<float>{1.0f, 1.0f, 0.0f};
    q.mid = a.mid;
}

// both roundings are formed and one is selected: no branch stands between a packet's loads and its arithmetic
__device__ __forceinline__ float w8o_round_mid(float v, int mid) {
    const float b = static_cast<float>(io_bf16::to_elem(v)), h = static_cast<float>(io_f16::to_elem(v));
    return mid == LSQ_BF16 ? b : (mid == LSQ_F16 ? h : v);
}

template <typename Q>
__device__ __forceinline__ uint32_t w8o_byte(float u, const Q& q) {
    return static_cast<uint32_t>(static_cast<int>(level<float>(u, q.qp, q.r)) & 0xff);
}

// u (a value of mid) as element `at` of a floating y
__device__ __forceinline__ void w8o_store_float(void* y, int64_t at, float u, int mid) {
    if (mid == LSQ_F32) static_cast<float*>(y)[at] = u;
    else if (mid == LSQ_BF16) static_cast<__bf16*>(y)[at] = io_bf16::passthrough(u);
    else static_cast<_Float16*>(y)[at] = static_cast<_Float16>(u);        // u is a float16 value: exact
}

// one output element: `at` in elements of y
template <typename Q>
__device__ __forceinline__ void w8o_store1(void* y, int64_t at, float u, const Q& q) {
    if (q.levels_out) static_cast<uint8_t*>(y)[at] = static_cast<uint8_t>(w8o_byte(u, q));
    else w8o_store_float(y, at, u, q.mid);
}

// a packet of 16 outputs: `at` in elements of y, y 16-byte aligned
template <typename Q>
__device__ __forceinline__ void w8o_store16(void* y, int64_t at, const float (&u)[16], const Q& q) {
    if (q.levels_out) {
        uint32_t w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            w[i] = w8o_byte(u[4 * i], q) | w8o_byte(u[4 * i + 1], q) << 8 | w8o_byte(u[4 * i + 2], q) << 16 | w8o_byte(u[4 * i + 3], q) << 24;
        *reinterpret_cast<u32x4*>(static_cast<uint8_t*>(y) + at) = u32x4{w[0], w[1], w[2], w[3]};
    } else if (q.mid == LSQ_F32) {
        u32x4* out = reinterpret_cast<u32x4*>(static_cast<float*>(y) + at);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            out[i] = u32x4{__float_as_uint(u[4 * i]), __float_as_uint(u[4 * i + 1]), __float_as_uint(u[4 * i + 2]),
                           __float_as_uint(u[4 * i + 3])};
    } else {
        uint32_t w[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const _Float16 a = static_cast<_Float16>(u[2 * i]), b = static_cast<_Float16>(u[2 * i + 1]);
            unsigned short ha, hb;
            __builtin_memcpy(&ha, &a, 2);
            __builtin_memcpy(&hb, &b, 2);
            // u is a value of mid: a bfloat16 is its high half, a float16 converts exactly.  A select, not a branch: the form
            // that leaves eltwise_w8's and norm_w8's kernels as they were
            const uint32_t lo = q.mid == LSQ_BF16 ? __float_as_uint(u[2 * i]) >> 16 : static_cast<uint32_t>(ha);
            const uint32_t hi = q.mid == LSQ_BF16 ? __float_as_uint(u[2 * i + 1]) >> 16 : static_cast<uint32_t>(hb);
            w[i] = lo | hi << 16;
        }
        u32x4* out = reinterpret_cast<u32x4*>(static_cast<uint8_t*>(y) + at * 2);
        out[0] = u32x4{w[0], w[1], w[2], w[3]};
        out[1] = u32x4{w[4], w[5], w[6], w[7]};
    }
}

}  // namespace lsq
