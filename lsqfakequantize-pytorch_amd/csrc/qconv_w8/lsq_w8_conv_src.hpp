// lsq_w8_conv_src.hpp -- the A operand of a W8A8 conv2d on channels-last levels as the tile body's packet source
// (lsq_w8_tiles_loop.hpp): the geometry as a kernel argument, an output pixel's receptive field, the implicit
// [B OH OW, kh kw Cin] matrix, and the checked geometry of the host side.  For csrc/qconv_w8/, csrc/requant_w8/ and
// csrc/resadd_w8/.
#pragma once
#include "../qlinear_w8/lsq_w8_shared.hpp"

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

// the implicit [B OH OW, kh kw Cin] matrix of byte operands, Cin % 16 == 0 and K <= 65536 (scalars only: a nested W8ConvGeom
// sends the struct through scratch memory)
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

// the source of a tile kernel: a tap in the padding holds the level zx, the byte zx - off
__device__ __forceinline__ W8ConvSrc w8_conv_src(const W8Act& act, const W8Const& ac, const W8ConvGeom& cg) {
    const uint32_t pad = static_cast<uint32_t>(ac.z & 0xff) * 0x01010101u;
    return W8ConvSrc{act.a, ac.flip, pad, cg.OH, cg.OW, cg.image, static_cast<unsigned>(cg.H), static_cast<unsigned>(cg.W),
                     static_cast<unsigned>(cg.Cin), static_cast<unsigned>(cg.kw), static_cast<unsigned>(cg.dh),
                     static_cast<unsigned>(cg.dw), cg.sh, cg.sw, cg.ph, cg.pw};
}

struct W8ConvShape {        // a checked geometry (host side)
    int64_t M, N, K, OH, OW, x_elems;
    W8ConvGeom cg;
};

}  // namespace lsq
