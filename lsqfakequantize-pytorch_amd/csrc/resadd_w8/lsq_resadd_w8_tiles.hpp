// lsq_resadd_w8_tiles.hpp -- the W8A8 TILES kernel that closes a residual block: csrc/requant_w8/lsq_requant_w8_tiles.hpp's
// kernel with a residual LEVEL per output in the epilogue.  The residual tile is loaded as 16-byte packets along n during the
// LAST K step (behind its MFMAs), written into the LDS region of the output byte tile after the loop's last barrier, and read
// from there by the lane that forms the output byte, which then overwrites it.
#pragma once
#include "../requant_w8/lsq_requant_w8_tiles.hpp"

namespace lsq {

struct W8ResArg {           // kernel argument: the residual levels, dense [M, N] bytes in y's layout
    const uint8_t* l;
    const float* scale;     // one value each, read in the kernel as they are
    const int32_t* zero;
    int is_signed;          // int8 levels
    int packets;            // tiles: N % 16 == 0 and `l` 16-byte aligned
};

struct W8PreArg {           // kernel argument: the layer's own output fake-quantizer
    const float* scale;     // NULL: none
    const float* shift;
    float qmin, qmax, tmin, tmax;
};

struct W8ResQ {
    float s, z;
    int is_signed;
};

struct W8PreQ {
    QParams<float> qp;
    Range<float> r;
    int on;
};

__device__ __forceinline__ W8ResQ w8r_res_constants(const W8ResArg& a) {
    return W8ResQ{a.scale[0], static_cast<float>(a.zero[0]), a.is_signed};
}

__device__ __forceinline__ W8PreQ w8r_pre_constants(const W8PreArg& a) {
    W8PreQ p;
    p.on = a.scale != nullptr;
    p.r = Range<float>{a.qmin, a.qmax, a.tmin, a.tmax};
    p.qp = QParams<float>{1.0f, 1.0f, 0.0f};
    if (p.on) p.qp = make_qparams<float>(sanitize_scale_per_tensor<float>(a.scale[0]), a.shift[0], p.r);
    return p;
}

__device__ __forceinline__ float w8r_round(float v, int mid) {
    if (mid == LSQ_BF16) return static_cast<float>(io_bf16::to_elem(v));
    if (mid == LSQ_F16) return static_cast<float>(io_f16::to_elem(v));
    return v;
}

// w8q_byte with the contract's p, d and t between the rounding to mid_dtype and the select.  Every step is rounded once: the
// product d and the sum p + d are NOT one fused multiply-add (for mid_dtype float32 the rounding between them is the identity).
__device__ __forceinline__ uint8_t w8r_byte(int64_t I, const W8Weight& wt, float s_x, int64_t n, const W8OutQ& oq, const W8PreQ& pq,
                                            const W8ResQ& rq, uint8_t lr) {
    float v = __fmul_rn(__fmul_rn(wt.scale[n], static_cast<float>(I)), s_x);
    if (wt.bias) v = __fadd_rn(v, w8_bias_at(wt.bias, wt.bias_dtype, n));
    const float u = w8r_round(v, oq.mid);
    float p = u;
    if (pq.on) p = w8r_round(dequant<float>(level<float>(u, pq.qp, pq.r), pq.qp), oq.mid);
    const float lf = rq.is_signed ? static_cast<float>(static_cast<int8_t>(lr)) : static_cast<float>(lr);
    const float d = w8r_round(__fmul_rn(__fsub_rn(lf, rq.z), rq.s), oq.mid);
    float t = w8r_round(__fadd_rn(p, d), oq.mid);
    if (oq.relu) t = (t < 0.0f) ? 0.0f : t;         // a select: a NaN stays a NaN and goes to quant_min below
    return static_cast<uint8_t>(static_cast<int>(level<float>(t, oq.qp, oq.r)) & 0xff);
}

template <int SUBS, bool SPLITK, typename Src>
__device__ __forceinline__ void w8r_tiles_body(const Src src, const W8Const ac, const W8Weight& wt, const W8Geom& geo,
                                               const W8OutArg& out, const W8ResArg& res, const W8PreArg& pre,
                                               uint8_t* __restrict__ y) {
    typedef W8TileShape<SUBS, SPLITK> T;
    constexpr int kRows = T::kRows, kCols = T::kCols, kThreads = T::kThreads;
    constexpr int kPackets = kCols / 16;            // 16-byte packets of a row of the byte tile
    constexpr int kResItems = (kRows * kPackets + kThreads - 1) / kThreads;    // residual packets per thread: at most 2
    static_assert(kResItems <= 2, "the residual tile costs a thread at most eight registers");
    unsigned char* outb = w8q_tile_bytes<SUBS, SPLITK>();                       // residual in, y out
    const W8TileAt at = w8_tile_at<SUBS, SPLITK>(geo);
    const int tid = static_cast<int>(threadIdx.x);
    const int64_t N = geo.N;

    u32x4 rp[kResItems];                            // this thread's packets of the residual tile
#pragma unroll
    for (int j = 0; j < kResItems; ++j) rp[j] = u32x4{0u, 0u, 0u, 0u};

    w8_tiles_run<SUBS, SPLITK>(
        src, ac, wt, geo,
        [&] {                                       // N % 16 == 0: a packet that starts inside N lies inside N
            if (!res.packets) return;
#pragma unroll
            for (int j = 0; j < kResItems; ++j) {
                const int it = tid + j * kThreads;
                const int m = it / kPackets, p = it - m * kPackets;
                const int64_t n = at.nt0 + p * 16;
                if (it < kRows * kPackets && m < at.rows && n < N) rp[j] = *reinterpret_cast<const u32x4*>(res.l + (at.m0 + m) * N + n);
            }
        },
        [&] {
            // the residual tile into the byte tile (no byte of it overlaps the row sums or the split-K partials).  Bytes of
            // columns n >= N and of rows m >= rows are not written here, not read in the epilogue and not stored.
            if (res.packets) {
#pragma unroll
                for (int j = 0; j < kResItems; ++j) {
                    const int it = tid + j * kThreads;
                    if (it < kRows * kPackets) *reinterpret_cast<u32x4*>(outb + it * 16) = rp[j];
                }
            } else {                                // byte by byte along n: consecutive lanes on consecutive bytes
                for (int it = tid; it < kRows * kCols; it += kThreads) {
                    const int m = it / kCols, c = it - m * kCols;
                    const int64_t n = at.nt0 + c;
                    if (m < at.rows && n < N) outb[it] = res.l[(at.m0 + m) * N + n];
                }
            }
        },
        [&] {
            const W8OutQ oq = w8q_constants(out);
            const W8PreQ pq = w8r_pre_constants(pre);
            const W8ResQ rq = w8r_res_constants(res);
            // the lane reads the residual byte at (m, c) and writes the output byte to the same place: no other lane touches it
            return [=, &wt](int64_t I, int m, int c, int64_t n) {
                unsigned char* at_b = outb + m * kCols + c;
                *at_b = w8r_byte(I, wt, ac.s_x, n, oq, pq, rq, *at_b);
            };
        });
    __syncthreads();
    w8q_store_tile<SUBS, SPLITK>(at, N, out.packets, y);
}

}  // namespace lsq
