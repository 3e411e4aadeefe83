// lsq_attn_w8_dev.hpp -- the device-side arithmetic of the attention core on 8-bit levels, one definition of each step for the
// kernels of liblsq_hip_attn_w8.so (lsq_attn_w8.hip: three launches) and of liblsq_hip_attn_fused_w8.so
// (../attn_fused_w8/lsq_attn_fused_w8.hip: one): the output side and its constants, the rounding to mid, the level byte, the
// tail mask of a packet, the fp32 steps of the matmul on the exact integer, the 4 x 4 byte transposition and the softmax's value.
// Moved here they leave every kernel of liblsq_hip_attn_w8.so instruction for instruction as it was
// (profiles/r24_attn_w8_shared_isa_diff.txt).
#pragma once
#include "../lsq_kernels.hpp"
#include "../lsq_w8_out_side.hpp"
#include "../qlinear_w8/lsq_w8_shared.hpp"

namespace lsq {

struct AttnOut {            // kernel argument: the output side
    const float* scale;     // NULL: a floating y
    const float* shift;
    float qmin, qmax, tmin, tmax;
    int mid;
};

typedef W8OutSide AttnQ;     // the output side alone: the rounding, the byte and the stores are lsq_w8_out_side.hpp's

__device__ __forceinline__ AttnQ attn_constants(const AttnOut& o) {
    AttnQ q;
    w8o_constants(q, o);
    return q;
}

// the packet's bytes from `valid` on become 0 (valid >= 16: none)
__device__ __forceinline__ u32x4 attn_mask_tail(u32x4 v, int valid) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = min(max(valid - 4 * i, 0), 4);
        v[i] &= n >= 4 ? 0xffffffffu : ((1u << (8 * n)) - 1u);
    }
    return v;
}

// the fp32 steps of the contract on the exact integer, and the rounding to mid
__device__ __forceinline__ float bmm_value(float fI, float s_a, float s_b, int mid) {
    return w8o_round_mid(__fmul_rn(__fmul_rn(s_b, fI), s_a), mid);
}

__device__ __forceinline__ float bmm_value(int64_t I, float s_a, float s_b, int mid) { return bmm_value(static_cast<float>(I), s_a, s_b, mid); }

// I from the raw sums, P = sum a b, C = sum_k b, S = sum_k a, as w8_exact forms it -- but with 64-bit zero points and in wrapping
// unsigned arithmetic: exact wherever I fits 64 bits (every zero point within -32768..32767), no signed overflow anywhere
__device__ __forceinline__ int64_t bmm_exact(int64_t P, int64_t C, int64_t S, int64_t K, int64_t z_a, int64_t z_b) {
    const uint64_t za = static_cast<uint64_t>(z_a), zb = static_cast<uint64_t>(z_b);
    return static_cast<int64_t>(static_cast<uint64_t>(P) - za * static_cast<uint64_t>(C) - zb * static_cast<uint64_t>(S) +
                                static_cast<uint64_t>(K) * za * zb);
}

// The constants of one matmul's exact integer I = P - z_a C - z_b S + K z_a z_b.  |I| <= K max|la - za| max|lb - zb|: where that
// stays below 2^31 (every K up to 32768 with zero points inside the level ranges) the four terms are summed in 32 wrapping bits
// and converted with one instruction (`narrow`); elsewhere bmm_exact's 64 bits.  The value is the same integer.  For the fused
// kernel; bmm_w8_mfma_kernel keeps the same selection inline, because calling these changes its machine code (see there).
struct BmmInt {
    int64_t z_a, z_b;       // the zero points less the operands' offsets (128 for uint8 levels)
    int K;
    uint32_t kzz;
    bool narrow;
};

__device__ __forceinline__ BmmInt bmm_int_constants(int64_t z_a, int64_t z_b, int K) {
    BmmInt e;
    e.z_a = z_a;
    e.z_b = z_b;
    e.K = K;
    const int64_t reach_a = max(z_a + 128, 127 - z_a), reach_b = max(z_b + 128, 127 - z_b);        // max |a - z| over a in -128..127
    e.narrow = reach_a < 65536 && reach_b < 65536 && K * reach_a * reach_b < (int64_t{1} << 31);
    e.kzz = static_cast<uint32_t>(K) * static_cast<uint32_t>(z_a) * static_cast<uint32_t>(z_b);
    return e;
}

// float(I) from the raw sums of the matrix core: P = sum a b, C = sum_k b, S = sum_k a
__device__ __forceinline__ float bmm_int_float(const BmmInt& e, int P, int C, int S) {
    if (e.narrow) {
        const uint32_t I32 = static_cast<uint32_t>(P) - static_cast<uint32_t>(e.z_a) * static_cast<uint32_t>(C) -
                             static_cast<uint32_t>(e.z_b) * static_cast<uint32_t>(S) + e.kzz;
        return static_cast<float>(static_cast<int32_t>(I32));
    }
    return static_cast<float>(bmm_exact(P, C, S, e.K, e.z_a, e.z_b));
}

// the 4 x 4 block of bytes of four words transposed: c[k] = byte k of each word, in their order
__device__ __forceinline__ void attn_transpose4(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3, uint32_t (&c)[4]) {
    // __builtin_amdgcn_perm(hi, lo, sel): selector bytes 0..3 take lo's bytes, 4..7 hi's
    const uint32_t lo01 = __builtin_amdgcn_perm(x1, x0, 0x05010400u), hi01 = __builtin_amdgcn_perm(x1, x0, 0x07030602u);
    const uint32_t lo23 = __builtin_amdgcn_perm(x3, x2, 0x05010400u), hi23 = __builtin_amdgcn_perm(x3, x2, 0x07030602u);
    c[0] = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u);
    c[1] = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
    c[2] = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u);
    c[3] = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
}

__device__ __forceinline__ uint64_t smx_shfl_xor_u64(uint64_t v, int mask) {
    return static_cast<uint64_t>(w8_shfl_xor_i64(static_cast<int64_t>(v), mask));
}

// p of the contract rounded to mid: float(E) is exact (E <= 2^24)
__device__ __forceinline__ float smx_value(int E, float r, int mid) { return w8o_round_mid(__fmul_rn(static_cast<float>(E), r), mid); }

}  // namespace lsq
