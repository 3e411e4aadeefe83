// lsq_glu_w8_dev.hpp -- the arithmetic of the gated product act(gate) * up on 8-bit levels (include/lsq_hip_glu_w8.h states it), once:
// the kernel argument with the constants, the per-thread constants, up's dequantization and the one rounded product.  Device code,
// scalar pieces only.  csrc/glu_w8/ (the product as a launch of its own) and csrc/linglu_w8/ (the product in the epilogue of the
// decode-shape gate and up linears) compile these same functions.
#pragma once
#include "../lsq_kernels.hpp"
#include "../lsq_w8_out_side.hpp"

namespace lsq {

struct GluArg {             // kernel argument: the constants
    const float* s_u;
    const int32_t* z_u;
    const float* scale;     // the output quantizer; NULL: a floating y
    const float* shift;
    float qmin, qmax, tmin, tmax;
    int mid;                // LSQ_F32 / LSQ_BF16 / LSQ_F16
    uint32_t flip_u;        // 0x80808080 for int8 levels of up (biased by 128 on load), 0 for uint8
};

struct GluQ : W8OutSide {   // the constants, read once per thread
    float s_u, z_u, off_u;  // off_u: 128.0f for int8 levels, what the flipped byte carries too much; 0.0f for uint8
};

__device__ __forceinline__ GluQ glu_constants(const GluArg& a) {
    GluQ q;
    w8o_constants(q, a);
    q.s_u = a.s_u[0];
    q.z_u = static_cast<float>(a.z_u[0]);
    q.off_u = a.flip_u ? 128.0f : 0.0f;
    return q;
}

// LevelsTensor.dequantize(mid) of byte `I` of a packet's word `w` of up, which was flipped by 0x80 per byte for int8 levels so
// that it holds level + off as an unsigned byte: float(level) = float(byte) - off exactly, then (float(level) - float(zero)) *
// scale, rounded to mid
template <int I>
__device__ __forceinline__ float glu_dequant(uint32_t w, const GluQ& q) {
    const float l = __fsub_rn(static_cast<float>((w >> (8 * I)) & 0xffu), q.off_u);
    return w8o_round_mid(__fmul_rn(__fsub_rn(l, q.z_u), q.s_u), q.mid);
}

// t of the contract: one rounded fp32 multiply (never an fma), one rounding to mid
__device__ __forceinline__ float glu_product(float a, float d, int mid) { return w8o_round_mid(__fmul_rn(a, d), mid); }

}  // namespace lsq
