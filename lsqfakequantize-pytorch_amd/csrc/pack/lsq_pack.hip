// lsq_pack.hip -- group-wise LSQ weights as packed 4- / 2-bit codes on gfx950, and back (include/lsq_hip_pack.h, which
// defines the format): the kernels and the C ABI of liblsq_hip_pack.so.
//
// All three ops are flat streams in the idiom of group/lsq_per_group.hip: a persistent grid in whole rounds of the chip,
// 16-byte packets on the wide side moved with one global_load / global_store_dwordx4 each, kGrpUnroll independent packets
// per lane in flight, non-temporal hints on the streams, 64-bit indexing, the group index by shift or by DivU64.
//  * QUANTIZE (x -> codes, qscale, qzero).  PACKET form (G % E == 0, E = elements per lane = max(VEC, 8 / bits)): a lane
//    loads one packet of x (two adjacent ones for fp64 at 2 bits, where one packet is half a byte), derives its group's
//    constants once, and stores the E * bits / 8 bytes of its own codes -- 1, 2 or 4 bytes -- with one narrow store; the
//    64 lanes of a wave write one contiguous run of 64 to 256 bytes per instruction, whole cache lines, so the stores
//    coalesce like the dword-per-lane level bytes of the group forward.  (Handing four lanes' codes to one lane with DPP moves
//    for a four times wider store was measured and is 0-2 % slower: DESIGN.md section 9.2.)  The lane that holds the first packet
//    of a group also writes qscale / qzero.  BYTE form (any other G, or a codes pointer that is not aligned to the
//    lane's store): one code byte per lane from 8 / bits elements, which lie in one group because G % (8 / bits) == 0.
//  * DEQUANTIZE (codes -> y): the mirror image.  PACKET form (G % VEC == 0): a lane loads the VEC * bits / 8 bytes of
//    codes of one packet of y (the shared byte for fp64 at 2 bits) and stores the packet; ELEMENT form otherwise.
//  * UNPACK (codes -> one byte per element): 16 elements per lane, an 8- or 4-byte load and a 16-byte store; the ragged
//    end and misaligned buffers go one code byte per lane.
// The arithmetic is lsq_math.hpp's: level() for the codes, make_qparams for the constants, and (c - qzero) * qscale rounded
// by out_elem like the forward's dequant() -- compiled with -ffp-contract=off like everything else.
#include "../group/lsq_grp_body.hpp"
#include "../lsq_companion_abi.hpp"
#include "../../../include/lsq_hip_pack.h"

namespace lsq {

template <int BYTES> struct CodeWord;
template <> struct CodeWord<1> { typedef uint8_t type; };
template <> struct CodeWord<2> { typedef uint16_t type; };
template <> struct CodeWord<4> { typedef uint32_t type; };

// what one lane of a form handles, per (storage type, bits)
template <typename IO, int BITS>
struct PackGeom {
    static constexpr int kPerByte = 8 / BITS;                                        // elements per code byte
    static constexpr int kQPackets = IO::VEC >= kPerByte ? 1 : kPerByte / IO::VEC;   // packets of x per quantize lane
    static constexpr int kQElems = IO::VEC * kQPackets;                              // E
    static constexpr int kQBytes = kQElems * BITS / 8;                               // code bytes a quantize lane stores
    static constexpr int kDBits = IO::VEC * BITS;                                    // code bits of one packet of y
    static constexpr int kDBytes = kDBits >= 8 ? kDBits / 8 : 1;                     // code bytes a dequantize lane loads
};

template <typename T>
__device__ __forceinline__ uint32_t code_of(T x, const QParams<T>& q, const Range<T>& r) {
    return static_cast<uint32_t>(static_cast<int>(level<T>(x, q, r) - r.qmin));     // exact: both are small integers
}

template <typename T>
__device__ __forceinline__ void store_group_constants(T* __restrict__ qscale, int32_t* __restrict__ qzero, int64_t g,
                                                      const QParams<T>& q, int quant_min) {
    qscale[g] = q.s;
    qzero[g] = static_cast<int32_t>(q.zp) - quant_min;
}

// ------------------------------------------------------------------------------------------------
// quantize
// ------------------------------------------------------------------------------------------------
// per_group: division by the lanes (packet form) resp. code bytes (byte form) of one group
template <typename IO, int BITS, bool PACKET>
__global__ __launch_bounds__(kBlock) void pack_quantize_kernel(const void* __restrict__ x, uint8_t* __restrict__ codes,
                                                               typename IO::arith* __restrict__ qscale,
                                                               int32_t* __restrict__ qzero, int64_t n, int pg_shift,
                                                               DivU64 per_group,
                                                               const typename IO::arith* __restrict__ scale,
                                                               const typename IO::arith* __restrict__ shift,
                                                               Range<typename IO::arith> r, int quant_min) {
    using T = typename IO::arith;
    using GEO = PackGeom<IO, BITS>;
    constexpr int VEC = IO::VEC;
    const int64_t block = static_cast<int64_t>(blockIdx.x), grid = static_cast<int64_t>(gridDim.x);
    if constexpr (!PACKET) {
        constexpr int PB = GEO::kPerByte;
        const int64_t n_bytes = n / PB;
        for (int64_t b = block * kBlock + threadIdx.x; b < n_bytes; b += grid * kBlock) {
            const int64_t g = per_group.div(b);
            const QParams<T> q = group_qparams<T>(scale, shift, g, r);
            if (b - g * static_cast<int64_t>(per_group.d) == 0) store_group_constants<T>(qscale, qzero, g, q, quant_min);
            uint32_t w = 0;
#pragma unroll
            for (int j = 0; j < PB; ++j) w |= code_of<T>(IO::load1(x, b * PB + j), q, r) << (j * BITS);
            codes[b] = static_cast<uint8_t>(w);
        }
    } else {
        constexpr int QP = GEO::kQPackets, E = GEO::kQElems;
        using Word = typename CodeWord<GEO::kQBytes>::type;
        Word* __restrict__ out = reinterpret_cast<Word*>(codes);
        const int64_t n_lanes = n / E;              // exact: n % G == 0 and G % E == 0
        constexpr int64_t kTile = static_cast<int64_t>(kBlock) * kGrpUnroll;
        const int64_t n_full = n_lanes / kTile;
        auto emit = [&](const Packet<IO>* in, int64_t l) {
            const int64_t g = pg_shift >= 0 ? (l >> pg_shift) : per_group.div(l);
            const QParams<T> q = group_qparams<T>(scale, shift, g, r);
            const bool first = pg_shift >= 0 ? (l & ((int64_t{1} << pg_shift) - 1)) == 0
                                             : l - g * static_cast<int64_t>(per_group.d) == 0;
            if (first) store_group_constants<T>(qscale, qzero, g, q, quant_min);
            uint32_t w = 0;
#pragma unroll
            for (int k = 0; k < QP; ++k)
#pragma unroll
                for (int j = 0; j < VEC; ++j) w |= code_of<T>(static_cast<T>(in[k].v[j]), q, r) << ((k * VEC + j) * BITS);
            __builtin_nontemporal_store(static_cast<Word>(w), out + l);
        };
        for (int64_t tile = block; tile < n_full; tile += grid) {
            const int64_t l0 = tile * kTile + threadIdx.x;
            Packet<IO> in[kGrpUnroll][QP];
#pragma unroll
            for (int u = 0; u < kGrpUnroll; ++u)
#pragma unroll
                for (int k = 0; k < QP; ++k)
                    in[u][k] = load_packet_nt<IO>(x, ((l0 + static_cast<int64_t>(u) * kBlock) * QP + k) * VEC);
#pragma unroll
            for (int u = 0; u < kGrpUnroll; ++u) emit(in[u], l0 + static_cast<int64_t>(u) * kBlock);
        }
        if (block == n_full % grid) {               // the one partial tile
            for (int64_t l = n_full * kTile + threadIdx.x; l < n_lanes; l += kBlock) {
                Packet<IO> in[QP];
#pragma unroll
                for (int k = 0; k < QP; ++k) in[k] = load_packet<IO>(x, (l * QP + k) * VEC);
                emit(in, l);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// dequantize
// ------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T dequant_code(uint32_t c, T qz, T qs) {
    return (static_cast<T>(static_cast<int>(c)) - qz) * qs;
}

// per_group: division by the packets (packet form) resp. elements (element form) of one group
template <typename IO, int BITS, bool PACKET>
__global__ __launch_bounds__(kBlock) void pack_dequantize_kernel(const uint8_t* __restrict__ codes, void* __restrict__ y,
                                                                 int64_t n, int pg_shift, DivU64 per_group,
                                                                 const typename IO::arith* __restrict__ qscale,
                                                                 const int32_t* __restrict__ qzero) {
    using T = typename IO::arith;
    using GEO = PackGeom<IO, BITS>;
    constexpr int VEC = IO::VEC;
    constexpr uint32_t kMask = (1u << BITS) - 1u;
    const int64_t block = static_cast<int64_t>(blockIdx.x), grid = static_cast<int64_t>(gridDim.x);
    if constexpr (!PACKET) {
        constexpr int PB = GEO::kPerByte;
        for (int64_t i = block * kBlock + threadIdx.x; i < n; i += grid * kBlock) {
            const int64_t g = per_group.div(i);
            const uint32_t c = (static_cast<uint32_t>(codes[i / PB]) >> (static_cast<int>(i % PB) * BITS)) & kMask;
            store_out<IO, false>(y, i, dequant_code<T>(c, static_cast<T>(qzero[g]), qscale[g]));
        }
    } else {
        using Word = typename CodeWord<GEO::kDBytes>::type;
        const Word* __restrict__ in_codes = reinterpret_cast<const Word*>(codes);
        const int64_t n_packets = n / VEC;          // exact: n % G == 0 and G % VEC == 0
        constexpr int64_t kTile = static_cast<int64_t>(kBlock) * kGrpUnroll;
        const int64_t n_full = n_packets / kTile;
        // the code word of packet p: its own VEC * BITS / 8 bytes, or -- fp64 at 2 bits -- the byte it shares with a neighbour
        auto word_index = [](int64_t p) { return GEO::kDBits >= 8 ? p : (p * GEO::kDBits) >> 3; };
        auto emit = [&](uint32_t w, int64_t p) {
            if constexpr (GEO::kDBits < 8) w >>= static_cast<int>((p * GEO::kDBits) & 7);
            const int64_t g = pg_shift >= 0 ? (p >> pg_shift) : per_group.div(p);
            const T qs = qscale[g], qz = static_cast<T>(qzero[g]);
            Packet<IO> out;
#pragma unroll
            for (int j = 0; j < VEC; ++j) out.v[j] = out_elem<IO, false>(dequant_code<T>((w >> (j * BITS)) & kMask, qz, qs));
            store_packet_nt<IO>(y, p * VEC, out);
        };
        for (int64_t tile = block; tile < n_full; tile += grid) {
            const int64_t p0 = tile * kTile + threadIdx.x;
            uint32_t w[kGrpUnroll];
#pragma unroll
            for (int u = 0; u < kGrpUnroll; ++u)
                w[u] = __builtin_nontemporal_load(in_codes + word_index(p0 + static_cast<int64_t>(u) * kBlock));
#pragma unroll
            for (int u = 0; u < kGrpUnroll; ++u) emit(w[u], p0 + static_cast<int64_t>(u) * kBlock);
        }
        if (block == n_full % grid) {               // the one partial tile
            for (int64_t p = n_full * kTile + threadIdx.x; p < n_packets; p += kBlock) emit(in_codes[word_index(p)], p);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// unpack
// ------------------------------------------------------------------------------------------------
// WIDE: n16 lanes of 16 elements each come first (codes and levels aligned for them), the rest goes one code byte per lane
template <int BITS, bool WIDE>
__global__ __launch_bounds__(kBlock) void pack_unpack_kernel(const uint8_t* __restrict__ codes, uint8_t* __restrict__ levels,
                                                             int64_t n, int offset) {
    constexpr int PB = 8 / BITS;
    constexpr uint32_t kMask = (1u << BITS) - 1u;
    using V4 = __attribute__((ext_vector_type(4))) unsigned int;
    const int64_t gid = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
    const int64_t n16 = WIDE ? n / 16 : 0;
    if constexpr (WIDE) {
        for (int64_t l = gid; l < n16; l += stride) {
            uint64_t w;
            if constexpr (BITS == 4) w = __builtin_nontemporal_load(reinterpret_cast<const uint64_t*>(codes) + l);
            else w = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(codes) + l);
            V4 out;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                uint32_t word = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t c = static_cast<uint32_t>(w >> ((d * 4 + j) * BITS)) & kMask;
                    word |= ((c + static_cast<uint32_t>(offset)) & 0xffu) << (8 * j);
                }
                out[d] = word;
            }
            __builtin_nontemporal_store(out, reinterpret_cast<V4*>(levels) + l);
        }
    }
    const int64_t n_bytes = n / PB;
    for (int64_t b = n16 * 16 / PB + gid; b < n_bytes; b += stride) {
        const uint32_t w = codes[b];
#pragma unroll
        for (int j = 0; j < PB; ++j)
            levels[b * PB + j] = static_cast<uint8_t>(((w >> (j * BITS)) & kMask) + static_cast<uint32_t>(offset));
    }
}

// ------------------------------------------------------------------------------------------------
// host side: the plan and the launchers
// ------------------------------------------------------------------------------------------------
struct PackPlan {
    bool q_packet, d_packet;
    int q_grid, d_grid, u_grid;
    int q_elems, d_elems;           // elements per lane of the packet forms
    int64_t q_per_group, d_per_group;
};

// whole rounds of the chip: at most kGrpFwdBlocksPerCU workgroups per compute unit, fewer when the work is smaller
inline int pack_grid(int64_t lanes, int per_lane_unroll) {
    const int64_t round = static_cast<int64_t>(device_info().cu_count) * kGrpFwdBlocksPerCU;
    const int64_t tile = static_cast<int64_t>(kBlock) * per_lane_unroll;
    return static_cast<int>(std::min(std::max<int64_t>(1, (lanes + tile - 1) / tile), round));
}

inline int unpack_grid(int64_t n) { return pack_grid((n + 15) / 16, 1); }   // 16 elements per lane

inline PackPlan plan_pack(int vec, int64_t n, int64_t G, int bits) {
    PackPlan pl;
    const int per_byte = 8 / bits;
    pl.q_elems = std::max(vec, per_byte);
    pl.d_elems = vec;
    pl.q_packet = G % pl.q_elems == 0;
    pl.d_packet = G % vec == 0;
    pl.q_per_group = pl.q_packet ? G / pl.q_elems : G / per_byte;
    pl.d_per_group = pl.d_packet ? G / vec : G;
    pl.q_grid = pl.q_packet ? pack_grid(n / pl.q_elems, kGrpUnroll) : pack_grid(n / per_byte, 1);
    pl.d_grid = pl.d_packet ? pack_grid(n / vec, kGrpUnroll) : pack_grid(n, 1);
    pl.u_grid = unpack_grid(n);
    return pl;
}

template <typename IO, int BITS>
static hipError_t quantize_packed(const void* x, int64_t n, int64_t G, const void* scale, const void* shift, const lsq_params& p,
                                  void* codes, void* qscale, void* qzero, hipStream_t stream) {
    using T = typename IO::arith;
    using GEO = PackGeom<IO, BITS>;
    PackPlan pl = plan_pack(IO::VEC, n, G, BITS);
    if (pl.q_packet && !aligned_to(codes, GEO::kQBytes)) {      // the lane's narrow store needs its own alignment
        pl.q_packet = false;
        pl.q_per_group = G / GEO::kPerByte;
        pl.q_grid = pack_grid(n / GEO::kPerByte, 1);
    }
    const Range<T> r = make_range<T>(p);
    const DivU64 per_group = make_div(pl.q_per_group);
#define LSQ_LAUNCH_PACK_Q(P)                                                                                              \
    hipLaunchKernelGGL((pack_quantize_kernel<IO, BITS, P>), dim3(pl.q_grid), dim3(kBlock), 0, stream, x,                    \
                       static_cast<uint8_t*>(codes), static_cast<T*>(qscale), static_cast<int32_t*>(qzero), n,             \
                       P ? log2_exact(pl.q_per_group) : -1, per_group, static_cast<const T*>(scale),                       \
                       static_cast<const T*>(shift), r, static_cast<int>(p.quant_min))
    if (pl.q_packet) LSQ_LAUNCH_PACK_Q(true);
    else LSQ_LAUNCH_PACK_Q(false);
#undef LSQ_LAUNCH_PACK_Q
    return hipGetLastError();
}

template <typename IO, int BITS>
static hipError_t dequantize_packed(const void* codes, int64_t n, int64_t G, const void* qscale, const void* qzero, void* y,
                                    hipStream_t stream) {
    using T = typename IO::arith;
    using GEO = PackGeom<IO, BITS>;
    PackPlan pl = plan_pack(IO::VEC, n, G, BITS);
    if (pl.d_packet && !aligned_to(codes, GEO::kDBytes)) {      // a misaligned view of the codes: the element form
        pl.d_packet = false;
        pl.d_per_group = G;
        pl.d_grid = pack_grid(n, 1);
    }
    const DivU64 per_group = make_div(pl.d_per_group);
#define LSQ_LAUNCH_PACK_D(P)                                                                                              \
    hipLaunchKernelGGL((pack_dequantize_kernel<IO, BITS, P>), dim3(pl.d_grid), dim3(kBlock), 0, stream,                     \
                       static_cast<const uint8_t*>(codes), y, n, P ? log2_exact(pl.d_per_group) : -1, per_group,           \
                       static_cast<const T*>(qscale), static_cast<const int32_t*>(qzero))
    if (pl.d_packet) LSQ_LAUNCH_PACK_D(true);
    else LSQ_LAUNCH_PACK_D(false);
#undef LSQ_LAUNCH_PACK_D
    return hipGetLastError();
}

template <int BITS>
static hipError_t unpack_packed(const void* codes, int64_t n, int offset, void* levels, hipStream_t stream) {
    const int grid = unpack_grid(n);
    const uint8_t* c = static_cast<const uint8_t*>(codes);
    uint8_t* lv = static_cast<uint8_t*>(levels);
    if (aligned_to(codes, 8) && aligned_to(levels, 16))
        hipLaunchKernelGGL((pack_unpack_kernel<BITS, true>), dim3(grid), dim3(kBlock), 0, stream, c, lv, n, offset);
    else
        hipLaunchKernelGGL((pack_unpack_kernel<BITS, false>), dim3(grid), dim3(kBlock), 0, stream, c, lv, n, offset);
    return hipGetLastError();
}

}  // namespace lsq

// ------------------------------------------------------------------------------------------------
// the C ABI of include/lsq_hip_pack.h: validation, dtype dispatch, error bookkeeping
// ------------------------------------------------------------------------------------------------
namespace {

constexpr int32_t kTypeLimit = 1 << 23;

int check_bits(int bits, const char* what) {
    if (bits != 4 && bits != 2) return fail(LSQ_EINVAL, "%s: bits must be 4 or 2, got %d", what, bits);
    return LSQ_OK;
}

int check_layout(int dtype, int64_t n, int64_t G, int bits, const char* what) {
    if (dtype < LSQ_F32 || dtype > LSQ_F16) return fail(LSQ_EINVAL, "%s: unknown dtype code %d", what, dtype);
    if (int rc = check_bits(bits, what)) return rc;
    const long long nn = n, g = G;
    if (G <= 0) return fail(LSQ_EINVAL, "%s: group_size must be positive, got %lld", what, g);
    if (n < 0) return fail(LSQ_EINVAL, "%s: negative element count %lld", what, nn);
    if (n % G != 0) return fail(LSQ_EINVAL, "%s: element count %lld is not a multiple of group_size %lld", what, nn, g);
    if (G % (8 / bits) != 0)
        return fail(LSQ_EINVAL, "%s: group_size %lld is not a multiple of %d, the elements of one byte of %d-bit codes (a group "
                    "must start on a byte boundary)", what, g, 8 / bits, bits);
    return LSQ_OK;
}

}  // namespace

#define LSQ_PACK_DISPATCH(dtype, bits, CALL)                                                  \
    switch (dtype) {                                                                          \
        case LSQ_F32: { using IO = lsq::io_f32; if (bits == 4) { constexpr int B = 4; CALL; } else { constexpr int B = 2; CALL; } } break;  \
        case LSQ_F64: { using IO = lsq::io_f64; if (bits == 4) { constexpr int B = 4; CALL; } else { constexpr int B = 2; CALL; } } break;  \
        case LSQ_BF16: { using IO = lsq::io_bf16; if (bits == 4) { constexpr int B = 4; CALL; } else { constexpr int B = 2; CALL; } } break; \
        default: { using IO = lsq::io_f16; if (bits == 4) { constexpr int B = 4; CALL; } else { constexpr int B = 2; CALL; } } break;       \
    }

extern "C" {

int lsq_pack_abi_version(void) { return LSQ_PACK_ABI_VERSION; }

const char* lsq_pack_last_error(void) { return g_last_error; }

int lsq_pack_quantize(int dtype, const void* x, int64_t n, int64_t group_size, const void* scale, const void* shift,
                      const lsq_params* p, int bits, void* codes, void* qscale, void* qzero, void* stream) {
    const char* what = "lsq_pack_quantize";
    if (int rc = check_layout(dtype, n, group_size, bits, what)) return rc;
    if (!p) return fail(LSQ_EINVAL, "%s: lsq_params pointer is NULL", what);
    if (p->quant_min > p->quant_max) return fail(LSQ_EINVAL, "%s: quant_min %d > quant_max %d", what, p->quant_min, p->quant_max);
    if (p->type_min > p->type_max) return fail(LSQ_EINVAL, "%s: type_min %d > type_max %d", what, p->type_min, p->type_max);
    // (code - qzero) and (level - zp) are the same exact integer only while every operand is exact in fp32
    if (p->type_min < -kTypeLimit || p->type_max > kTypeLimit || p->quant_min < -kTypeLimit || p->quant_max > kTypeLimit)
        return fail(LSQ_EINVAL, "%s: quant_min, quant_max, type_min and type_max must lie within +-2^23 (got [%d, %d] in [%d, %d])",
                    what, p->quant_min, p->quant_max, p->type_min, p->type_max);
    if (static_cast<int64_t>(p->quant_max) - p->quant_min > (1 << bits) - 1)
        return fail(LSQ_EINVAL, "%s: the range [%d, %d] has more than the %d levels of %d-bit codes", what, p->quant_min,
                    p->quant_max, 1 << bits, bits);
    if (p->numel_for_scaler != 0)
        return fail(LSQ_EINVAL, "%s: numel_for_scaler must be 0 (there is no sharded group op), got %lld", what,
                    static_cast<long long>(p->numel_for_scaler));
    if (!x || !scale || !shift || !codes || !qscale || !qzero) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (!aligned_to(x, elem_bytes(dtype))) return fail(LSQ_EINVAL, "%s: x must be element-aligned", what);
    if (!aligned_to(scale, param_bytes(dtype)) || !aligned_to(shift, param_bytes(dtype)) ||
        !aligned_to(qscale, param_bytes(dtype)) || !aligned_to(qzero, 4))
        return fail(LSQ_EINVAL, "%s: scale, shift, qscale and qzero must be element-aligned", what);
    if (n == 0) return LSQ_OK;
    hipError_t e = hipSuccess;
    LSQ_PACK_DISPATCH(dtype, bits, (e = lsq::quantize_packed<IO, B>(x, n, group_size, scale, shift, *p, codes, qscale, qzero,
                                                                     static_cast<hipStream_t>(stream))));
    return hip_status(e, what);
}

int lsq_pack_dequantize(int dtype, const void* codes, int64_t n, int64_t group_size, int bits, const void* qscale,
                        const void* qzero, void* y, void* stream) {
    const char* what = "lsq_pack_dequantize";
    if (int rc = check_layout(dtype, n, group_size, bits, what)) return rc;
    if (!codes || !qscale || !qzero || !y) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (!aligned_to(y, elem_bytes(dtype))) return fail(LSQ_EINVAL, "%s: y must be element-aligned", what);
    if (!aligned_to(qscale, param_bytes(dtype)) || !aligned_to(qzero, 4))
        return fail(LSQ_EINVAL, "%s: qscale and qzero must be element-aligned", what);
    if (n == 0) return LSQ_OK;
    hipError_t e = hipSuccess;
    LSQ_PACK_DISPATCH(dtype, bits, (e = lsq::dequantize_packed<IO, B>(codes, n, group_size, qscale, qzero, y,
                                                                       static_cast<hipStream_t>(stream))));
    return hip_status(e, what);
}

int lsq_pack_unpack(const void* codes, int64_t n, int bits, int quant_min, int level_bias, void* levels, void* stream) {
    const char* what = "lsq_pack_unpack";
    if (int rc = check_bits(bits, what)) return rc;
    if (n < 0) return fail(LSQ_EINVAL, "%s: negative element count %lld", what, static_cast<long long>(n));
    if (n % (8 / bits) != 0)
        return fail(LSQ_EINVAL, "%s: element count %lld is not a multiple of %d, the elements of one byte of %d-bit codes", what,
                    static_cast<long long>(n), 8 / bits, bits);
    const long long lo = static_cast<long long>(quant_min) - level_bias, hi = lo + (1 << bits) - 1;
    if (!((lo >= -128 && hi <= 127) || (lo >= 0 && hi <= 255)))
        return fail(LSQ_EINVAL, "%s: levels: [quant_min, quant_min + %d] - level_bias = [%lld, %lld] fits neither int8 nor uint8",
                    what, (1 << bits) - 1, lo, hi);
    if (!codes || !levels) return fail(LSQ_EINVAL, "%s: NULL buffer", what);
    if (n == 0) return LSQ_OK;
    hipError_t e = hipSuccess;
    if (bits == 4) e = lsq::unpack_packed<4>(codes, n, static_cast<int>(lo), levels, static_cast<hipStream_t>(stream));
    else e = lsq::unpack_packed<2>(codes, n, static_cast<int>(lo), levels, static_cast<hipStream_t>(stream));
    return hip_status(e, what);
}

int lsq_pack_plan(int dtype, int64_t n, int64_t group_size, int bits, int32_t* out8) {
    const char* what = "lsq_pack_plan";
    if (int rc = check_layout(dtype, n, group_size, bits, what)) return rc;
    if (!out8) return fail(LSQ_EINVAL, "%s: NULL output", what);
    const lsq::PackPlan pl = lsq::plan_pack(io_vec(dtype), n, group_size, bits);
    out8[0] = pl.q_grid;
    out8[1] = pl.d_grid;
    out8[2] = pl.u_grid;
    out8[3] = lsq::kBlock;
    out8[4] = pl.q_packet ? 1 : 0;
    out8[5] = pl.d_packet ? 1 : 0;
    out8[6] = pl.q_elems;
    out8[7] = pl.d_elems;
    return LSQ_OK;
}

}  // extern "C"
