// lsq_qdecode.hpp -- the decode linear on packed 4- / 2-bit group-wise weight codes, the part that does not depend on what
// the activation is: shared by qlinear/lsq_qlinear.hip (float x, mfma_f32_16x16x32) and qlinear_a8/lsq_qlinear_a8.hip
// (8-bit levels, mfma_i32_16x16x64_i8).  The two libraries stay separate; each compiles these pieces into its own kernels.
//
// The op is a stream over the codes -- N * K * bits / 8 bytes, the only large traffic -- with x (at most 16 x K) kept close.
//  * MATRIX-CORE form.
//    TILE OWNERSHIP.  A workgroup of kQWaves = 16 waves owns a tile of kQTile = 16 output columns (rows of w) and walks the
//    tiles in a persistent grid (mfma_grid: one workgroup per compute unit).  Lane (n = lane & 15, q = lane >> 4) reads
//    row tile * 16 + n of w, clamped to N - 1: a clamped row computes a value nobody stores.
//    K SPLIT BY WAVE.  A LOAD STEP is 4 packets of 16 bytes = 4 * BE consecutive k (BE = 128 / bits) of each of the 16
//    rows; the lane loads packet p0 + q of its row with one non-temporal global_load_dwordx4 (load_code_packet) and the
//    step's four qscale / qzero (load_packet_scale).  Which steps a wave takes is fixed by (K, G, bits) alone: step s of
//    a chunk belongs to wave s % 16 (float x), span s -- lcm(G, 4 BE) elements -- to wave s % 16 (8-bit levels).  Never
//    by M.
//    x is staged in LDS behind the reduction buffer in chunks of at most kQChunk = 4096 k, rows kQRowPad = 16 bytes
//    further apart than their data against bank conflicts; it STAYS there across tiles when one chunk holds all of K.
//    TRANSPOSE.  Four v_permlane{32,16}_swap transpose the 4 x 4 dwords of the lanes (n, 0..3) (transpose_over_rows):
//    afterwards dword t of lane (n, q) is dword q of packet p0 + t, so the k of one MFMA lie in ONE packet and with it in
//    one group, and the B operand is made from one register.
//    REDUCTION ORDER.  Each wave keeps one fp32 x 4 accumulator per lane -- the MFMA's D layout: column = lane & 15, row =
//    4 * (lane >> 4) + register -- over its steps in ascending k.  At the end of a tile every wave writes it to
//    red[(wave * 64 + lane) * 4 ..], the kQRedBytes at the start of LDS, and after a barrier thread tid < 256 sums register
//    tid >> 6 of lane tid & 63 over the waves in wave order 0, 1, ..., 15: one thread per output, no atomics.  So the
//    order of the fp32 sum depends on (K, G, bits, the form) alone, never on M or the data: row m of an M-row call is the
//    1-row call bit for bit, and repeated launches are bit-identical.  The kernel then finishes the sum its own way (+ bias; * s_x + bias) and rounds
//    once.
//  * GENERIC form: one wave per output column (generic_grid), kQGenericRowsAtOnce = 4 rows of x at a time, a butterfly
//    over the wave.  Correct for every legal format; not tuned.  The two kernels share no frame beyond these constants and
//    bias_at: their inner loops and their butterflies (all lanes; the lanes of a group, then the groups) differ.
//
// Host side: what both plans and both C ABIs say the same way -- the grids, the one-time LDS opt-in, the shape check and
// the out8[] of `*_plan`.
#pragma once
#include "../group/lsq_grp_body.hpp"
#include "../lsq_companion_abi.hpp"
#include "../../../include/lsq_hip_qlinear.h"
#include "../../../include/lsq_hip_qlinear_a8.h"

static_assert(LSQ_QLINEAR_MAX_ROWS == LSQ_QLINEAR_A8_MAX_ROWS && LSQ_QLINEAR_MAX_ROWS == 16,
              "both kernels hold the rows of x in the 16 rows of one MFMA tile");

namespace lsq {

constexpr int kQWaves = 16;                         // waves that share one output tile (matrix-core form)
constexpr int kQBlock = kQWaves * 64;
constexpr int kQTile = 16;                          // output columns per tile
constexpr int kQChunk = 4096;                       // most elements of K per LDS chunk of x
constexpr int kQRowPad = 16;                        // bytes between rows of x in LDS beyond their data: 4 banks further per row
constexpr int kQRedBytes = kQWaves * 64 * 16;       // one fp32 x 4 accumulator per lane and wave
constexpr int kQGenericRowsAtOnce = 4;

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// the 4 x 4 transpose of r[t] over the lanes (n, q = 0..3) = lane n + 16 q: afterwards r[t] of lane q is what r[q] of lane t was
__device__ __forceinline__ void transpose_over_rows(uint32_t (&r)[4]) {
    u32x2 p;
    p = __builtin_amdgcn_permlane32_swap(r[0], r[2], false, false); r[0] = p.x; r[2] = p.y;    // lanes 32..63 of r[0] <-> 0..31 of r[2]
    p = __builtin_amdgcn_permlane32_swap(r[1], r[3], false, false); r[1] = p.x; r[3] = p.y;
    p = __builtin_amdgcn_permlane16_swap(r[0], r[1], false, false); r[0] = p.x; r[1] = p.y;    // odd rows of r[0] <-> even rows of r[1]
    p = __builtin_amdgcn_permlane16_swap(r[2], r[3], false, false); r[2] = p.x; r[3] = p.y;
}

template <typename IO>
__device__ __forceinline__ float bias_at(const void* bias, int bias_f32, int64_t n) {
    if (!bias) return 0.0f;
    return bias_f32 ? static_cast<const float*>(bias)[n] : IO::load1(bias, n);
}

// Packet p of the row of codes `wrow`: one non-temporal global_load_dwordx4 -- the codes are read once.
__device__ __forceinline__ u32x4 load_code_packet(const uint8_t* wrow, int64_t p) {
    return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wrow + p * 16));
}

// qscale and qzero of packet p of a row (0 past the row's n_packets).  ppg: 16-byte packets per group -- the shift when a
// power of two (ppg_shift >= 0), else the division.
__device__ __forceinline__ void load_packet_scale(const float* qs_row, const int32_t* qz_row, int64_t p, int64_t n_packets,
                                                  int ppg_shift, DivU64 ppg, float& qs, int32_t& qz) {
    qs = 0.0f;
    qz = 0;
    if (p < n_packets) {
        const int64_t g = ppg_shift >= 0 ? (p >> ppg_shift) : ppg.div(p);
        qs = qs_row[g];
        qz = qz_row[g];
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// one workgroup of 16 waves per compute unit
inline int mfma_grid(int64_t N, int64_t cus) {
    return static_cast<int>(std::min(std::max<int64_t>(1, (N + kQTile - 1) / kQTile), cus));
}

inline int generic_grid(int64_t N, int64_t cus) {
    const int64_t per_block = kBlock / 64;
    return static_cast<int>(std::min(std::max<int64_t>(1, (N + per_block - 1) / per_block), cus * 8));
}

// A matrix-core kernel may use more LDS than the 64 KiB a kernel gets unasked: said once per kernel and device.  The
// launcher of each instantiation owns one LdsOnce (a function-local static).
struct LdsOnce {
    std::atomic<int> ready[64];
};

inline hipError_t allow_lds(LdsOnce& once, const void* kernel, int bytes) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (once.ready[dev].load(std::memory_order_acquire)) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) once.ready[dev].store(1, std::memory_order_release);
    return e;
}

// out8[] of lsq_qlinear_plan and lsq_qlinear_a8_plan
inline void write_plan8(int32_t* out8, bool mfma, int grid, int block, int lds, int chunk, int waves, int cols) {
    out8[0] = mfma ? 1 : 0;
    out8[1] = grid;
    out8[2] = block;
    out8[3] = LSQ_QLINEAR_MAX_ROWS;
    out8[4] = lds;
    out8[5] = chunk;
    out8[6] = waves;
    out8[7] = cols;
}

}  // namespace lsq

namespace {

// the shape of a call on a packed weight.  no_f64: why the library has no float64; beyond: what to do with more rows
int check_shape(int dtype, int64_t M, int64_t N, int64_t K, int64_t G, int bits, const char* what, const char* no_f64,
                const char* beyond) {
    if (dtype == LSQ_F64) return fail(LSQ_EINVAL, "%s: float64 is not supported (%s)", what, no_f64);
    if (dtype != LSQ_F32 && dtype != LSQ_BF16 && dtype != LSQ_F16) return fail(LSQ_EINVAL, "%s: unknown dtype code %d", what, dtype);
    if (bits != 4 && bits != 2) return fail(LSQ_EINVAL, "%s: bits must be 4 or 2, got %d", what, bits);
    const long long m = M, n = N, k = K, g = G;
    if (G <= 0) return fail(LSQ_EINVAL, "%s: group_size must be positive, got %lld", what, g);
    if (N < 0 || K < 0) return fail(LSQ_EINVAL, "%s: negative weight shape [%lld, %lld]", what, n, k);
    if (K % G != 0) return fail(LSQ_EINVAL, "%s: K = %lld is not a multiple of group_size %lld", what, k, g);
    if (G % (8 / bits) != 0)
        return fail(LSQ_EINVAL, "%s: group_size %lld is not a multiple of %d, the elements of one byte of %d-bit codes", what, g,
                    8 / bits, bits);
    if (M < 1 || M > LSQ_QLINEAR_MAX_ROWS)
        return fail(LSQ_EINVAL, "%s: M = %lld rows of x, the kernel serves 1 to %d (%s)", what, m, LSQ_QLINEAR_MAX_ROWS, beyond);
    return LSQ_OK;
}

}  // namespace
