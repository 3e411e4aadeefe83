// lsq_pc_plan.hpp -- host side of the per-channel ops, no device code: the policy constants with their measurement
// notes, the plan structs and plan_forward / plan_bwd_pc / plan_backward, which decide a launch in
// full (kernel instantiation, geometry, grid, LDS, finalize) before anything is enqueued.  The launchers that run a plan
// are in lsq_per_channel.hip.
#pragma once
#include <optional>

#include "lsq_pc_bwd.hpp"
#include "lsq_pc_finalize.hpp"
#include "lsq_pc_fwd.hpp"
#include "lsq_pc_seg.hpp"

namespace lsq {

// =================================================================================================
// policy constants
// =================================================================================================
// Elements per lane per row in the window-mode backward.  Half packets (4 elements, 8 bytes per lane) for 16-bit
// storage were measured: 103 instead of 156 VGPRs, but no faster at BASELINE config 5 (best 35.0 us vs 36.3 us, within
// the run-to-run spread: the dx-only kernel shows the access pattern itself tops out near 5.3 TB/s there), so every
// storage type moves full packets; load_elems / store_elems keep the 8-byte path.
template <typename IO>
constexpr int kWindowBwdVec = IO::VEC;
constexpr int kLastAxisBwdBlocksPerCU = 2;
// (tools-build knobs consulted below, all 0 in the production library -- lsq_kernels.hpp `knob`: kWwMinRows = rows a
// row-group-window workgroup walks at least, 0 = kWwMinRows<IO>; kWwSplit64 = rows of 128 / 192 / 256 lanes as 64-lane windows;
// kRingNt = streaming hint on the ring's copies, 0 = policy, 1 = on, 2 = off; kWwBig = 768/1024-lane workgroups, 0 = policy,
// 1 = always, 2 = never)
// Policy: on for the BACKWARD of tensors of more than 32 MB -- the x a backward reads was saved by a forward long ago and
// is not in the 256 MB Infinity Cache any more, whatever the gradient is, and nt copies still hit the lines a producer left
// there.  256-lane windows, cold (profiles/r02_ring_nt_ab.txt): config 5 fp32 64.9 -> 59.8 us, bf16 (51 MB) 37.1 -> 34.3 us.
// Row-group windows with the gradient fresh from a producer kernel and x cold (profiles/r02_ww_nt_ab.txt): [8192,4096] fp32
// 78 -> 68 us, [256,197,768] fp32 91 -> 80 us, [65536,1024] bf16 82 -> 76 us; never slower, cold included.  (An earlier A/B that
// found the hint harmful for row groups and for the forward re-read one set of buffers: the hint kept them out of the cache.)
static inline int ring_nt_for(int64_t tensor_bytes, bool backward) {
    const int k = knob::get(knob::kRingNt);
    if (k != 0) return k == 1 ? 1 : 0;
    return backward && tensor_bytes > (int64_t{32} << 20) ? 1 : 0;
}
// (16-bit storage: 768 lanes -- its kernel needs ~140 registers, 1024 lanes would cap it at 128 and spill)
template <int ELEM_BYTES>
constexpr int kBigBlockOf = ELEM_BYTES < 4 ? 768 : 1024;
// Owner windows (plan_own): launch bound of their kernels (the workgroup is R x lanes-per-row threads, at most this: eight
// waves, so the 16-bit kernel keeps its ~120 registers without spilling) and the tensor size up to which the policy takes
// them.  Measured with one owner per CU (plan_own's fattest channel group; profiles/r04_owner_windows_ab2.txt, backward op,
// cold): they win where the finalize launch is a large share of the op -- [64,2048,7,7] bf16 15.6 -> 11.9 us, fp32 22.9 ->
// 18.5; [16,1024,14,14] fp32 17.2 -> 9.9 -- stay ahead in 16-bit storage up to 19 M elements ([192,2048,7,7] 28.2 -> 27.2,
// [96,1024,14,14] 28.7 -> 26.8) and in fp32 up to 12.8 M ([128,2048,7,7] 33.4 -> 32.9, [32,512,28,28] 33.9 -> 31.2), and are
// behind from there: fp32 16 M +2 %, 19 M +5 %, BASELINE config 5 (25.7 M) bf16 33.8 -> 35.6 us, fp32 59.8 -> 65.7 -- every owner
// walks the same rows at the same time and the access pattern tops out at 5.4 TB/s (profiles/r04_owner_pattern_probe.txt),
// where the row slabs of the 256-lane windows spread the chip over the whole tensor.
// Short runs (channel rows of a few positions: 1-D feature maps, 3x3 ... 10x10) are fine -- [128,2048,4,4] fp32 17.9 -> 11.9 us,
// [512,2048,8] 26.2 -> 23.1, [128,2048,5,5] 25.5 -> 19.4, bf16 [512,2048,8] 18.3 -> 13.7 -- unless they are under 512 bytes AND
// not whole 128-byte lines: every row of every owner then shares a partial line with its neighbours ([rows,2048,7] fp32, eight
// channels = 224 bytes: 384 rows 21.2 -> 20.4 us, 512 rows 24.9 -> 25.5, 768 rows 32.2 -> 39.3); those only up to 5 * 2^20
// elements ([256,2048,7] 17.0 -> 11.8 us, [292,2048,7] 18.2 -> 13.8, [192,2048,3,3] 15.5 -> 11.1).  profiles/r04_owner_short_runs.txt, r04_owner_min_run.txt.
constexpr int kOwnBlock = 512;
constexpr size_t kLdsBytesPerWorkgroup = 160 * 1024;      // gfx950: LDS a workgroup may allocate (the Makefile builds for gfx950 only)
template <int ELEM_BYTES>
constexpr int64_t kOwnMaxElemsOf = ELEM_BYTES < 4 ? int64_t{20} << 20 : (ELEM_BYTES == 4 ? int64_t{13} << 20 : int64_t{1} << 23);
constexpr int64_t kOwnMaxElemsShortRun = int64_t{5} << 20;
constexpr int kOwnShortRunBytes = 512;
constexpr int kWwBwdBlocksPerCU = 4;     // row-group windows: one full round for every storage type (3-4 resident per CU)
// Rows a forward workgroup walks at least, per unit of its per-workgroup overhead (make_geom): that overhead is only
// the channel-table build -- VEC channels per lane when the quantized axis is the last one, so twice as heavy per
// streamed byte for 16-bit storage.  ([64,197,768] fp32 forward 17.8 -> 13.7 us, bf16 13.8 -> 11.4 us against the
// backward's bound of 27.)  A variant without the table (every lane computing its own channels' constants, no LDS,
// no barrier) was measured too and is slower: its scale/shift loads are strided by VEC across the lanes.
template <typename IO>
constexpr int kFwdPerSlotRows = sizeof(typename IO::elem) < 4 ? 12 : 4;
// Packets in flight per lane in the segment kernels (profiles/r01_segment_sweep.txt, typical weight shapes): 4 for
// 4/8-byte storage; 16-bit storage (twice the arithmetic and registers per packet, half the packets per channel --
// [4096, 4096] in bf16 is two packets per lane) runs best at 1: [32000, 4096] bf16 backward 125 us vs 143 us at 4.
template <typename IO>
constexpr int kSegUnroll = sizeof(typename IO::elem) < 4 ? 1 : 4;
static inline int pick_cpl(int vec, int64_t inner) {
    if (vec == 1 || inner % vec == 0) return 1;
    return inner >= vec ? 2 : vec;
}

// LDS-DMA ring in the window-mode kernels by default, with the grid it likes: fewer, longer workgroups than the register
// loops (it needs rows to keep its ring full).  A/B on one box, profiles/r02_dma_ab.txt: 8-16 % faster on every large shape
// in both directions when the tensors are cache-resident; on cold buffers (profiles/r02_cold_buffers_pc.txt) it keeps that
// lead for 16-bit storage only, hence the size rules further down (plan_forward, ring_nt_for).
template <typename IO>
constexpr bool kDmaDefault = true;
template <typename IO>
constexpr int kDmaBwdBlocksPerCU = sizeof(typename IO::elem) < 4 ? 4 : 8;
template <typename IO>
constexpr int kDmaFwdBlocksPerCU = sizeof(typename IO::elem) < 4 ? 4 : 8;
constexpr int kFwdDmaDepth = 8;      // one 1 KiB stage per row and wave in the forward (x only); the backward rings are 4 deep

// ---- plans ----------------------------------------------------------------------------------------
// A per-channel launch is decided in full before anything is enqueued.  plan_forward / plan_backward hold the whole launch
// policy: they pick the kernel instantiation, the geometry, the grid and the finalize, and call nothing of HIP but the
// cached queries (device_info, registers_of, resident_blocks_per_cu).  forward_per_channel / backward_per_channel launch
// what the plan says; lsq_hip_plan_backward_per_channel and the workspace size read the plan and launch nothing.
template <typename T>
using FwdPcKernel = void (*)(const void*, void*, int8_t*, int, int, PcGeom, const T*, const T*, Range<T>);
template <typename T>
using FwdSegKernel = void (*)(const void*, void*, int8_t*, int, int, SegGeom, const T*, const T*, Range<T>);
template <typename T>
using BwdPcKernel = void (*)(const void*, const void*, void*, PcGeom, const T*, const T*, Range<T>, T, double2*, PcDirect<T>);
template <typename T>
using BwdSegKernel = void (*)(const void*, const void*, void*, SegGeom, const T*, const T*, Range<T>, T, double2*, SegDirect<T>);
template <typename T, typename G>
using FinalizeKernel = void (*)(const double2*, G, int, int, int, T, T*, T*, double*);

// Exactly one of `win` (window kernels over g) and `seg` (segment walk over sg) is set.
template <typename T>
struct FwdPcPlan {
    FwdPcKernel<T> win = nullptr;
    FwdSegKernel<T> seg = nullptr;
    PcGeom g{};
    SegGeom sg{};
    dim3 grid;
    size_t lds = 0;
    LaunchNote note{};
};

template <typename T>
struct BwdPcPlan {
    BwdPcKernel<T> win = nullptr;
    BwdSegKernel<T> seg = nullptr;
    // the finalize that folds the partials (null for both: the kernel stores d_scale / d_shift itself -- owner windows, and
    // the segment walk with one workgroup per channel)
    FinalizeKernel<T, PcGeom> fin_win = nullptr;
    FinalizeKernel<T, SegGeom> fin_seg = nullptr;
    PcGeom g{};
    SegGeom sg{};
    dim3 grid, fin_grid;
    int fin_ch = 0;
    size_t lds = 0;
    size_t workspace = 0;    // bytes of partials the launch writes
    LaunchNote note{};
};

// One window-kernel candidate committed to the plan: what every family (256-lane, row-group, owner windows) fills alike.
template <typename T>
static void commit_window(BwdPcPlan<T>& pl, BwdPcKernel<T> kern, const PcGeom& g, size_t lds, int per_cu, int vgprs_hint, int family,
                          int dma_depth) {
    pl.win = kern;
    pl.g = g;
    pl.grid = dim3(static_cast<unsigned>(g.n_windows), static_cast<unsigned>(g.splits));
    pl.lds = lds;
    pl.note = LaunchNote{static_cast<int>(g.n_windows), g.splits, per_cu, vgprs_hint, family, dma_depth, g.block_threads, g.ring_nt};
}

// Run-time mode flags -> template arguments: f is called with std::true_type / std::false_type per flag.
template <typename F>
static hipError_t with_flags(bool a, F&& f) {
    return a ? f(std::true_type{}) : f(std::false_type{});
}
template <typename F>
static hipError_t with_flags(bool a, bool b, F&& f) {
    return with_flags(a, [&](auto A) { return with_flags(b, [&](auto B) { return f(A, B); }); });
}
// the backward's (sym, init, eval): eval mode computes no sums, so it has no symmetric form
template <typename F>
static hipError_t with_bwd_modes(const lsq_params& p, F&& f) {
    if (p.eval_mode) return with_flags(p.init_mode != 0, [&](auto I) { return f(std::false_type{}, I, std::true_type{}); });
    return with_flags(p.sym != 0, p.init_mode != 0, [&](auto S, auto I) { return f(S, I, std::false_type{}); });
}

// ---- forward --------------------------------------------------------------------------------------
template <typename IO, int V, int CPL, bool INIT, bool LEVELS>
static hipError_t pick_fwd_pc(FwdPcPlan<typename IO::arith>& pl, const Variant& v) {
    // LDS-DMA ring (16-byte packets): plan_forward decided (v.dma == 2) and sized the grid and the LDS for it
    if constexpr (V * sizeof(typename IO::elem) == 16) {
        if (v.dma == 2) {
            pl.win = fwd_pc_kernel<IO, V, CPL, INIT, LEVELS, 1, true, true, kFwdDmaDepth>;
            return hipSuccess;
        }
    }
#define LSQ_PICK(U, NTLF, NTSF) pl.win = fwd_pc_kernel<IO, V, CPL, INIT, LEVELS, U, NTLF, NTSF>
    [[maybe_unused]] constexpr bool kFull = !INIT && !LEVELS && V > 1 && !std::is_same<IO, io_f64>::value &&
                                            !std::is_same<IO, io_f16>::value;
    LSQ_DISPATCH_VARIANT(kFull, 4, v, LSQ_PICK);
#undef LSQ_PICK
    return hipSuccess;
}

template <typename IO, bool INIT, bool LEVELS>
static hipError_t pick_fwd_seg(FwdPcPlan<typename IO::arith>& pl, bool short_walk, const Variant& v) {
#define LSQ_PICK(U, NTLF, NTSF)                                                         \
    do {                                                                                \
        if (short_walk) pl.seg = fwd_seg_kernel<IO, IO::VEC, INIT, LEVELS, U, NTLF, NTSF, 1>; \
        else pl.seg = fwd_seg_kernel<IO, IO::VEC, INIT, LEVELS, U, NTLF, NTSF, 2>;      \
    } while (0)
    [[maybe_unused]] constexpr bool kFull = !INIT && !LEVELS && (std::is_same<IO, io_f32>::value || std::is_same<IO, io_bf16>::value);
    LSQ_DISPATCH_VARIANT(kFull, kSegUnroll<IO>, v, LSQ_PICK);
#undef LSQ_PICK
    return hipSuccess;
}

template <typename IO, int V, int CPL>
static hipError_t fwd_pc_modes(FwdPcPlan<typename IO::arith>& pl, bool init, bool levels, const Variant& v) {
    return with_flags(init, levels, [&](auto I, auto L) { return pick_fwd_pc<IO, V, CPL, decltype(I)::value, decltype(L)::value>(pl, v); });
}

// packets_ok: every buffer is aligned for packets (forward_per_channel); ring_ok: x and y are 16-byte aligned
template <typename IO>
static hipError_t plan_forward(int64_t outer, int64_t channels, int64_t inner, bool init, bool levels, bool packets_ok,
                               bool ring_ok, int variant, FwdPcPlan<typename IO::arith>& pl) {
    using T = typename IO::arith;
    const DeviceInfo& dev = device_info();
    const int vec = pick_vec(IO::VEC, channels * inner, packets_ok);
    const bool seg = pick_segment_mode(vec, outer, channels, inner, dev.cu_count);
    const Variant v = decode_variant(variant, seg ? (sizeof(typename IO::elem) >= 4 ? kDefaultPcSegVariant : kDefaultPcSegNarrowVariant)
                                                  : kDefaultPcFwdVariant);
    const int target = dev.cu_count * v.blocks_per_cu;
    if (seg) {
        const SegGeom sg = make_seg_geom(outer, channels, inner, vec, target);
        if (!grid_fits(sg)) return hipErrorInvalidConfiguration;
        pl.sg = sg;
        pl.grid = dim3(static_cast<unsigned>(sg.C * sg.segs), static_cast<unsigned>(sg.osplits));
        pl.note = LaunchNote{static_cast<int>(sg.C * sg.segs), sg.osplits, 0, 0, 3, 0, kBlock, 0};
        // the most iterations a workgroup walks: short walks (a weight's channel) and long ones are two kernels (seg_forward)
        // (not for a big grid whose iterations are rows 16 MB apart instead of neighbouring sub-rows: [4,8,1048576] bf16 forward
        // 23.7 us with the loop, 26.4 us with the group -- profiles/r03_seg_up_front_ab.txt)
        const bool short_walk = sg.sub_per_seg * sg.o_per_split <= kSegUpFront && knob::get(knob::kSegNoUpFront) == 0 &&
                                (sg.o_per_split == 1 || sg.C * sg.segs * sg.osplits <= 8 * static_cast<int64_t>(dev.cu_count));
        return with_flags(init, levels, [&](auto I, auto L) { return pick_fwd_seg<IO, decltype(I)::value, decltype(L)::value>(pl, short_walk, v); });
    }
    const int cpl = pick_cpl(vec, inner);
    PcGeom g = make_geom(outer, channels, inner, vec, target, kFwdPerSlotRows<IO>);
    auto ring_lds = [](const PcGeom& gg) {      // the channel table, then one 1 KiB stage per row and wave
        return ((static_cast<size_t>(gg.k_slots) * sizeof(QSlot<T>) + 1023) & ~size_t(1023)) +
               static_cast<size_t>(kBlock / 64) * kFwdDmaDepth * 1024;
    };
    // The forward's LDS-DMA ring is NOT a default any more: it wins only when the same buffers are read again and again
    // (profiles/r02_dma_ab.txt: config 5 fp32 35.2 -> 32.2 us).  On input the previous kernel has just written
    // (profiles/r02_producer_consumer.txt: config 5 bf16 14.2 us with the register loops at 16 workgroups per CU, 17.5 us on
    // the ring; [32,256,56,56] bf16 14.3 vs 18.3 us) and on cold input (profiles/r02_cold_buffers_pc.txt: 6-14 % behind for
    // every storage type) the register loops are faster.  Variant bits 12-13 = 2 still select it (A/B runs, tests).
    // What stays from its tuning is the grid for one case: a 16-bit last-axis window has 2048 channels, a 32 KiB table, and
    // building half as many tables pays -- those shapes take the ring's grid (4 workgroups per CU) with the register loop
    // ([8192,4096] bf16 28.8 us against 34.3 us on the usual grid, cold 29.3 vs 35.3 us, after a producer 21.8 vs 24.7 us;
    // profiles/r02_fwd_lastaxis_grid.txt).
    Variant vv = v;
    vv.dma = 1;
    // A lane whose components are different channels (cpl == vec: the quantized axis is the last or nearly the last one)
    // reads its own scale / shift: no LDS table (fwd_pc_kernel, LaneChannels::load_direct) -- profiles/r03_fwd_direct_ab.txt,
    // cold: [12608,768] bf16 11.9 -> 9.5 us, [8192,4096] bf16 29.6 -> 26.8 us, [65536,1024] bf16 51.4 -> 46.6 us, [3152,768]
    // fp32 8.8 -> 7.1 us, the big fp32 tensors -1 .. -4 %.
    // tools builds, lsq_hip_debug_set_fwd_direct: 1 = direct on the usual grid, 2 = the table, 3 = the policy
    const int direct_knob = knob::get(knob::kFwdDirect);
    // tools knob 4: also the lanes of one or two channels (cpl < vec) -- A/B
    const bool direct = direct_knob == 4 || (vec > 2 && cpl == vec && direct_knob != 2);
    g.direct = direct ? 1 : 0;
    // (the grid rule that was found for the 32 KiB table stays on the direct path: [8192,4096] bf16 26.8 us against 27.5 us on
    // the usual grid, [16384,8192] 97.0 vs 99.5 us -- profiles/r03_fwd_direct_ab.txt)
    const bool table_grid_rule = direct_knob != 1;
    if (vec > 1 && vec * sizeof(typename IO::elem) == 16 && v.dma != 1 && (table_grid_rule || v.dma == 2)) {
        const int tgt = variant == 0 ? dev.cu_count * kDmaFwdBlocksPerCU<IO> : target;
        const PcGeom gd = make_geom(outer, channels, inner, vec, tgt, kFwdPerSlotRows<IO>);
        const int64_t tiles_each = gd.n_tiles / std::max(1, gd.splits);
        const bool table_big = ring_lds(gd) > 64 * 1024;
        // (tiles_each >= 8 on the ring's grid with a 2048-slot table already implies >= 2^24 elements: no separate size rule)
        if (v.dma == 2 || (table_big && tiles_each >= kFwdDmaDepth && tiles_each <= 64)) {
            g = gd;
            vv.dma = (table_big || !ring_ok) ? 1 : 2;
            g.direct = (direct && vv.dma == 1) ? 1 : 0;
            g.ring_nt = ring_nt_for(outer * channels * inner * static_cast<int64_t>(sizeof(typename IO::elem)), false);
        }
    }
    if (!grid_fits(g)) return hipErrorInvalidConfiguration;
    pl.g = g;
    pl.grid = dim3(static_cast<unsigned>(g.n_windows), static_cast<unsigned>(g.splits));
    // the ring's stages, else the channel table (direct: none, every lane reads its own channels)
    pl.lds = vv.dma == 2 ? ring_lds(g) : g.direct ? 0 : static_cast<size_t>(g.k_slots) * sizeof(QSlot<T>);
    pl.note = LaunchNote{static_cast<int>(g.n_windows), g.splits, 0, 0, 1, vv.dma == 2 ? kFwdDmaDepth : 0, kBlock, g.ring_nt};
    if (vec == 1) return fwd_pc_modes<IO, 1, 1>(pl, init, levels, vv);
    if (cpl == 1) return fwd_pc_modes<IO, IO::VEC, 1>(pl, init, levels, vv);
    if (cpl == 2) return fwd_pc_modes<IO, IO::VEC, 2>(pl, init, levels, vv);
    return fwd_pc_modes<IO, IO::VEC, IO::VEC>(pl, init, levels, vv);
}

// ---- backward -------------------------------------------------------------------------------------
// Everything a window-mode backward plan needs besides the kernel's template arguments.
struct BwdPcCall {
    int64_t outer, C, inner;
    int target_blocks;     // requested workgroups (CUs x workgroups per CU)
    bool default_variant;  // the caller passed variant 0: the plan may pick the grid of the code path it chooses
    bool whole_rounds;     // size the grid in whole rounds of what the chip holds at once (make_geom)
    bool ring_ok;          // grad / x / dx are 16-byte aligned: the LDS-DMA ring (and the owner windows built on it) may be used
    Variant v;
};

// rows a row-group-window workgroup walks at least.  4- and 8-byte storage: enough to keep its 16-byte-per-slot partial
// row under ~5 % of what it streams.  16-bit storage: 16 -- the tensors this floor binds on (fewer rows than workgroups
// wanted x floor) are latency-bound, every row a wave walks is another ~0.6 us on its serial chain, and the extra partial
// bytes cost less than that ([3152,768] bf16 21 -> 13.5 us, [4096,1024] 22 -> 14.6 us, profiles/r02_ww_rows_per_workgroup.txt)
template <typename IO>
constexpr int kWwMinRows = sizeof(typename IO::elem) < 4
                               ? 16
                               : (107 + static_cast<int>(sizeof(typename IO::elem)) - 1) / static_cast<int>(sizeof(typename IO::elem));
template <typename IO>
static inline int ww_min_rows() {
    const int o = knob::get(knob::kWwMinRows);
    return o > 0 ? o : kWwMinRows<IO>;
}

template <typename IO, int V, int CPL, bool SYM, bool INIT, bool EVAL, bool WW = false>
static hipError_t plan_bwd_pc(const BwdPcCall& c, BwdPcPlan<typename IO::arith>& pl) {
    using T = typename IO::arith;
    // (tuning builds also compile the variant table of the dx-only EVAL kernel: the streaming rate of the access pattern)
    [[maybe_unused]] constexpr bool kFull = !SYM && !INIT && V > 1 && !std::is_same<IO, io_f64>::value &&
                                            !std::is_same<IO, io_f16>::value;
    // 16-bit storage: unroll 1 + the software-pipelined loop (profiles/r01_pc_pipeline_sweep.txt: 36.3 us against
    // 38.5 us for the best plain variant at BASELINE config 5); 4/8-byte storage gains nothing from it (55.6 vs 55.9 us)
    // and keeps the plain loop at unroll 4.
    // CPL == V (inner < V: the quantized axis is the last or nearly the last one -- [tokens, features], NHWC): 16-bit
    // storage runs the pipelined loop at unroll 2 there (profiles/r01_lastaxis_sweep.txt).
    constexpr bool kNarrow = sizeof(typename IO::elem) < 4;
    constexpr int kDefU = kNarrow ? ((CPL == V && V > 1 && !WW) ? 2 : 1) : 4;
    // One candidate: 256-lane or row-group windows with `kern`.  The geometry depends on how many workgroups of the chosen
    // instantiation fit on the chip at once, so it is built here, where the kernel is known, together with the finalize.
    // No value (nothing planned, the next candidate's turn) when there is no room for the ring or a workgroup would walk
    // fewer row tiles than `min_tiles`.
    auto window = [&](BwdPcKernel<T> kern, int dma_depth, int target_blocks, int64_t min_tiles,
                      int block = kBlock) -> std::optional<hipError_t> {
        const DeviceInfo& dev = device_info();
        auto geom = [&](int resident) {
            // rows of 128 / 192 / 256 lanes: 4- and 8-byte storage cuts them into 64-lane windows of four row groups
            // ([65536,1024] fp32 backward 157 -> 140 us, profiles/r02_ww_split64_ab.txt); 16-bit storage gains nothing
            const bool split64 = sizeof(typename IO::elem) >= 4 ? knob::get(knob::kWwSplit64) != 2 : knob::get(knob::kWwSplit64) == 1;
            return WW ? make_geom_ww(c.outer, c.C, V, target_blocks, ww_min_rows<IO>(), resident, split64, block)
                      : make_geom(c.outer, c.C, c.inner, V, target_blocks, 27, resident);
        };
        // the LDS a workgroup needs does not depend on the split count: size it first, then the residency, then the grid
        const PcGeom g0 = geom(0);
        // row groups: every group parks its sums ([R][k_slots] double2); narrow windows add one row per walk of a slot
        size_t lds = WW ? (static_cast<size_t>(g0.R) * g0.k_slots + (g0.k_slots < g0.block_threads ? g0.block_threads : 0)) * sizeof(double2)
                        : static_cast<size_t>(g0.k_slots) * (sizeof(QSlot<T>) + 2 * sizeof(double));
        if (dma_depth > 0) {
            const size_t ring = bwd_lds_front_bytes(g0, sizeof(QSlot<T>)) +
                                static_cast<size_t>(g0.block_threads / 64) * dma_depth * kDmaStageBytes;
            lds = WW ? std::max(lds, ring) : ring;      // row groups: the combine buffer reuses the ring's LDS
        }
        // no room for the ring next to a very wide channel table: register loop (a 1024-lane workgroup has the CU to itself)
        if (dma_depth > 0 && lds > (block > kBlock ? 160 : 64) * 1024) return std::nullopt;
        if (lds > 160 * 1024) return hipErrorInvalidConfiguration;   // (gfx950: 160 KiB of LDS per workgroup)
        int per_cu = c.whole_rounds ? resident_blocks_per_cu(reinterpret_cast<const void*>(kern), lds) : 0;
        if (block > kBlock && per_cu > 0) {      // the register bound counts four-wave workgroups: convert it
            const int by_regs = resident_blocks_by_registers(reinterpret_cast<const void*>(kern)) * 4 / std::max(1, g0.block_threads / 64);
            per_cu = std::max(1, std::min(per_cu, by_regs));
        }
        PcGeom g = geom(per_cu * dev.cu_count);
        g.ring_nt = ring_nt_for(c.outer * c.C * c.inner * static_cast<int64_t>(sizeof(typename IO::elem)), true);
        const int64_t tiles_each = g.n_tiles / std::max<int64_t>(1, g.splits);
        if (tiles_each < min_tiles) return std::nullopt;
        if (!grid_fits(g)) return hipErrorInvalidConfiguration;
        commit_window<T>(pl, kern, g, lds, per_cu, registers_of(reinterpret_cast<const void*>(kern)), WW ? 2 : 1, dma_depth);
        pl.workspace = EVAL ? 0 : static_cast<size_t>(g.splits) * g.n_windows * g.k_slots * sizeof(double2);
        pl.fin_ch = fin_channels(c.C);
        pl.fin_win = WW ? finalize_ww_kernel<T> : finalize_pc_kernel<T>;
        pl.fin_grid = dim3(static_cast<unsigned>(((WW ? g.n_windows * g.k_slots : c.C) + pl.fin_ch - 1) / pl.fin_ch));
        return hipSuccess;
    };
    // LDS-DMA ring instead of register buffers (16-byte packets only): the default whenever a workgroup walks at least
    // as many row tiles as the ring is deep -- with the grid the ring likes, kDmaBwdBlocksPerCU workgroups per CU;
    // variant bits 12-13 force either path for A/B runs (1 = registers, 2 = ring).
    constexpr bool kDmaAble = V * sizeof(typename IO::elem) == 16;
#ifndef LSQ_BWD_DMA_DEPTH
#define LSQ_BWD_DMA_DEPTH 4
#endif
    constexpr int kDmaDepth = LSQ_BWD_DMA_DEPTH;
    // OWNER windows first (lsq_pc_geom.hpp, plan_own): activations whose channel rows are short (NCHW with small H x W) and
    // whose tensor is small enough for the finalize launch to matter -- one launch, no workspace.
    if constexpr (kDmaAble && !WW && !EVAL && V > 1 && CPL <= 2) {
        const int own_knob = knob::get(knob::kOwn);     // tools builds: 1 = wherever the shape allows, 2 = never, 3 = 1 without the priority turns
        const int own = own_knob == 3 ? 1 : own_knob;
        const int64_t elems = c.outer * c.C * c.inner;
        if (c.ring_ok && own != 2 && (own == 1 || (c.default_variant && elems <= kOwnMaxElemsOf<static_cast<int>(sizeof(typename IO::elem))>))) {
            const int min_run = knob::get(knob::kOwnMinRun);           // tools builds: bytes, 0 = kOwnMinRunBytes
            const int fat = knob::get(knob::kOwnFat);                  // tools builds: 1 = smallest channel group, 2 = fattest
            const OwnPlan op = plan_own(c.outer, c.C, c.inner, V, static_cast<int>(sizeof(typename IO::elem)), kDmaDepth,
                                        device_info().cu_count, kOwnBlock, min_run > 0 ? min_run : kOwnMinRunBytes,
                                        fat ? fat - 1 : kOwnFatDefault);
            const bool short_run_out = own != 1 && op.run_bytes < kOwnShortRunBytes && op.run_bytes % 128 != 0 && elems > kOwnMaxElemsShortRun;
            if (op.k != 0 && !short_run_out) {
                PcGeom g = make_geom_own(c.outer, c.C, c.inner, V, op);
                g.ring_nt = ring_nt_for(elems * static_cast<int64_t>(sizeof(typename IO::elem)), true);
                g.own_prio = own_knob == 3 ? 0 : 1;
                const size_t lds = bwd_lds_front_bytes(g, sizeof(QSlot<T>)) +
                                   static_cast<size_t>(g.block_threads / 64) * kDmaDepth * kDmaStageBytes;
                // (cannot fail with plan_own's sizing on gfx950: the other families otherwise)
                if (lds <= kLdsBytesPerWorkgroup) {
                    commit_window<T>(pl, bwd_pc_kernel<IO, V, CPL, SYM, INIT, EVAL, 1, true, true, false, false, kDmaDepth, kOwnBlock>, g,
                                     lds, op.per_cu, 0, 4, kDmaDepth);      // (make_geom_own: one split; no finalize, no workspace)
                    return hipSuccess;
                }
            }
        }
    }
    if constexpr (kDmaAble) {
        // (4- and 8-byte storage with one channel per lane, CPL == 1, keeps its register loop: it already has eight loads
        // in flight per lane and few registers, the ring only adds its LDS round trip -- measured 3-6 % slower)
        constexpr bool kDefaultHere = kDmaDefault<IO> && (sizeof(typename IO::elem) < 4 || CPL >= 2);
        if (c.ring_ok && (c.v.dma == 2 || (c.v.dma == 0 && kDefaultHere))) {
            const int target = c.default_variant ? device_info().cu_count * kDmaBwdBlocksPerCU<IO> : c.target_blocks;
            // (row-group windows of 4- and 8-byte storage: only tensors up to 160 MB -- [8192,4096] 78 -> 69 us,
            // [64,197,768] 33 -> 28 us; on the bigger ones, four elements a row, the ring's per-row bookkeeping costs more
            // than its loads in flight gain: NHWC [64,56,56,256] 119 -> 127 us, [65536,1024] 157 -> 172 us,
            // profiles/r02_ww_min_rows_sweep.txt)
            const bool big_wide = WW && sizeof(typename IO::elem) >= 4 &&
                                  c.outer * c.C * static_cast<int64_t>(sizeof(typename IO::elem)) > (int64_t{160} << 20);
            // ... and not below 2^24 elements either: register loops are level or ahead there on every row width -- 1 M elements
            // -8 .. -12 % ([1024,1024] 10.1 -> 8.9 us), 2-4 M 0 .. -6 %, 8.4 M -3 .. -11 %, 12.6 M -3 .. -6 %; from 16.8 M on the
            // ring leads ([16384,1024] 51.3 -> 44.7 us).  profiles/r04_rowgroup_ring_small.txt, r04_rowgroup_mid.txt
            const bool small_wide = WW && sizeof(typename IO::elem) >= 4 && c.outer * c.C < (int64_t{1} << 24);
            if constexpr (WW && !EVAL) {
                // Mid-sized tensors whose rows fit one window (8 M .. 80 M elements: [64,197,768], [256,197,768], NHWC
                // [16,56,56,256]): ONE 768/1024-lane workgroup per CU instead of three or four 3-4-wave ones -- the same
                // waves in flight, evenly over the four SIMDs (3-wave workgroups load them 3:2:2:2), a third of the partial
                // rows, constants and epilogues.  6-12 % faster there, slower below (a [16,197,768] wants many short
                // workgroups) and no gain above (profiles/r02_ww_big_ab.txt; upper end, cold buffers:
                // profiles/r03_ww_big_upper_ab.txt -- 16-bit storage -7 % at 48 M elements, -1 .. -4 % at 64 M, +1 .. +5 % at 96 M).
                const int big = knob::get(knob::kWwBig);
                const int64_t elems = c.outer * c.C;
                // (round 2 kept 4- and 8-byte storage up to 64 MB: [256,197,768] fp32 cold 91.5 vs 102.7 us for the usual
                // workgroups, profiles/r02_cold_buffers_pc.txt)
                // Round 4, another box (profiles/r04_rowgroup_mid.txt): 16-bit storage only -- in fp32 the fat workgroup never
                // led (8.4 M: 26.3-29.4 us against 24.1-26.1 for register loops; 12.6 M: level with the usual ring) -- and
                // only for rows of at least 64 lanes: [rows,64] bf16 loses 11-16 % with it (12.6 M elements 33.5 -> 28.0 us),
                // [rows,128] 5-7 %, [rows,256] 2-3 %; from [rows,512] on it is level or ahead up to 67 M elements.  At the lower
                // end, 8.4-11 M elements, it is -1 .. -8 % on nine shapes of twelve and +9 / +14 % on two with power-of-two row
                // counts ([8192,1024], [4096,2048]), with a third of the partial rows (profiles/r04_ww_big_low_end.txt): the
                // lower end stays at 2^23.
                // Round 5, after the epilogue's combine went over all lanes (the fat workgroup's own cost): BELOW 2^23 elements it
                // now leads wherever a row is at most 96 lanes -- every shape of [rows, 128 .. 768] bf16 from 3 M elements on
                // (+4 .. +19 %: [8192,384] 14.2 -> 12.5 us, [10000,768] 20.6 -> 16.8, [12608,256] +8 %), and from 0.8 M on where
                // the row does not tile a 256-lane workgroup (48, 80, 96 lanes: [2048,384] +8 %, [4096,640] +12 %, [3152,768]
                // +14 %; rows of 16 / 32 / 64 lanes are -10 .. +2 % there and keep their four-wave workgroups); rows of 128+ lanes
                // stay as they were ([4096,1024], [2048,2048] -5 %).  One row tile per workgroup is enough down there.
                // profiles/r05_ww_big_small_tensors.txt
                const bool fits = sizeof(typename IO::elem) < 4;
                const int64_t w_lanes = c.C / V;
                const bool low = elems < (int64_t{1} << 23);
                // (floors: what the round-5 sweep covered -- 16 lanes below 2^23 elements, 8 lanes inside the band; narrower rows
                //  mean hundreds of row groups per workgroup and a ~100 KB combine buffer nobody measured: they keep the usual
                //  four-wave workgroups)
                const bool low_ok = w_lanes >= 16 && w_lanes <= 96 && (elems >= (int64_t{3} << 20) ||
                                                      (elems >= (int64_t{3} << 18) && kBlock % static_cast<int>(w_lanes) != 0));
                // ... and INSIDE the band the narrow rows changed sides with it: [rows, 64 / 128 / 256] +4 .. +9 % at 9-17 M
                // elements (round 4: -11 .. -16 % for [rows,64]), -3 % at 25 M, level above; [rows,384] +1 .. +13 % through the
                // whole band (same file, second table)
                const bool band_ok = w_lanes >= 8 && elems < (int64_t{5} << 24) &&
                                     (w_lanes >= 64 || kBlock % static_cast<int>(w_lanes) != 0 || elems < (int64_t{5} << 22));
                const bool use_big = big == 1 || (big == 0 && c.default_variant && w_lanes <= kBlock && fits && (low ? low_ok : band_ok));
                constexpr int kBigBlock = kBigBlockOf<sizeof(typename IO::elem)>;
                if (use_big) {
                    if (auto e = window(bwd_pc_kernel<IO, V, CPL, SYM, INIT, EVAL, 1, true, true, false, WW, kDmaDepth, kBigBlock>,
                                        kDmaDepth, device_info().cu_count, (big == 1 || low) ? 0 : 2, kBigBlock))
                        return *e;
                }
            }
            // The tiles-per-workgroup floor of the ring (as many as it is deep) does not hold for 16-bit row groups: there the
            // ring is ahead with ONE tile per workgroup too -- [1568,512] bf16 13.1 -> 11.0 us, [16384,128] 21.0 -> 15.8,
            // [1365,384] 11.9 -> 10.2, nothing behind by more than 2.5 % (profiles/r04_rowgroup_ring_small.txt)
            const int64_t floor_tiles = (WW && sizeof(typename IO::elem) < 4) ? 1 : kDmaDepth;
            if (!((big_wide || small_wide) && c.v.dma != 2)) {
                if (auto e = window(bwd_pc_kernel<IO, V, CPL, SYM, INIT, EVAL, 1, true, true, false, WW, kDmaDepth>, kDmaDepth, target,
                                    c.v.dma == 2 ? 0 : floor_tiles))
                    return *e;
            }
        }
    }
    // register loops
    BwdPcKernel<T> kern = nullptr;
#define LSQ_PICK_P(U, NTLF, NTSF, PIPEF) kern = bwd_pc_kernel<IO, V, CPL, SYM, INIT, EVAL, U, NTLF, NTSF, PIPEF, WW>
#ifdef LSQ_TUNING
    // tuning builds compile both loops for the swept kernels; the switch is the variant's `chunked` bit (unused here)
    const bool pipe = kFull ? c.v.chunked : kNarrow;
#define LSQ_PICK(U, NTLF, NTSF)                                     \
    do {                                                            \
        if constexpr (kFull) {                                      \
            if (pipe) LSQ_PICK_P(U, NTLF, NTSF, true);              \
            else LSQ_PICK_P(U, NTLF, NTSF, false);                  \
        } else {                                                    \
            LSQ_PICK_P(U, NTLF, NTSF, kNarrow);                     \
        }                                                           \
    } while (0)
#else
#define LSQ_PICK(U, NTLF, NTSF) LSQ_PICK_P(U, NTLF, NTSF, kNarrow)
#endif
    LSQ_DISPATCH_VARIANT(kFull, kDefU, c.v, LSQ_PICK);
#undef LSQ_PICK
#undef LSQ_PICK_P
    return *window(kern, 0, c.target_blocks, 0);     // (no ring, no tile floor: always an answer)
}

template <typename IO, bool SYM, bool INIT, bool EVAL>
static hipError_t pick_bwd_seg(BwdPcPlan<typename IO::arith>& pl, bool short_walk, const Variant& v) {
#define LSQ_PICK(U, NTLF, NTSF)                                                                \
    do {                                                                                       \
        if (short_walk) pl.seg = bwd_seg_kernel<IO, IO::VEC, SYM, INIT, EVAL, U, NTLF, NTSF, 1>; \
        else pl.seg = bwd_seg_kernel<IO, IO::VEC, SYM, INIT, EVAL, U, NTLF, NTSF, 2>;          \
    } while (0)
    [[maybe_unused]] constexpr bool kFull = !INIT && !EVAL && (std::is_same<IO, io_f32>::value || std::is_same<IO, io_bf16>::value);
    LSQ_DISPATCH_VARIANT(kFull, kSegUnroll<IO>, v, LSQ_PICK);
#undef LSQ_PICK
    return hipSuccess;
}

template <typename IO, int V, int CPL, bool WW = false>
static hipError_t bwd_pc_modes(const BwdPcCall& c, const lsq_params& p, BwdPcPlan<typename IO::arith>& pl) {
    return with_bwd_modes(p, [&](auto S, auto I, auto E) {
        return plan_bwd_pc<IO, V, CPL, decltype(S)::value, decltype(I)::value, decltype(E)::value, WW>(c, pl);
    });
}

// Last-axis tensors under 512 MB take row-group windows in the backward; from there on the 256-lane windows, which read
// 4 KiB contiguous per row and workgroup instead of 1 KiB from each of four rows, are level or ahead
// (profiles/r03_ww_max_ab.txt, cold buffers: bf16 row groups -2 .. -12 % at 256 MB, -4 .. +7 % at 512 MB, level at 1 GB;
// fp32 -3 .. -9 % at 512 MB for rows up to 2048 features, +6 .. +22 % for wider rows -- those decide the 4-byte bound).
template <typename IO>
inline int64_t ww_max_elems() {
    const int k = knob::get(knob::kWwMaxLog2);      // tools builds: lsq_hip_debug_set_ww_max_log2
    return k > 0 ? int64_t{1} << k : (int64_t{512} << 20) / static_cast<int64_t>(sizeof(typename IO::elem));
}

// ring_ok: grad, x and dx are 16-byte aligned (they are element-aligned in any case, lsq_capi.hip)
template <typename IO>
static hipError_t plan_backward(int64_t outer, int64_t channels, int64_t inner, const lsq_params& p, bool ring_ok, int variant,
                                BwdPcPlan<typename IO::arith>& pl) {
    using T = typename IO::arith;
    const DeviceInfo& dev = device_info();
    // (plan_forward: packets on any element-aligned view; the ring and the owner windows built on it want 16 bytes)
    const int vec = pick_vec(IO::VEC, channels * inner, true);
    const bool seg = pick_segment_mode(vec, outer, channels, inner, dev.cu_count);
    const Variant v = decode_variant(variant, seg ? (sizeof(typename IO::elem) >= 4 ? kDefaultPcSegVariant : kDefaultPcSegNarrowVariant)
                                                  : (sizeof(typename IO::elem) >= 4 ? kDefaultPcBwdWideVariant
                                                                                    : kDefaultPcBwdNarrowVariant));
    const int target = dev.cu_count * v.blocks_per_cu;

    if (seg) {
        const SegGeom sg = make_seg_geom(outer, channels, inner, vec, target);
        if (!grid_fits(sg)) return hipErrorInvalidConfiguration;
        pl.sg = sg;
        pl.grid = dim3(static_cast<unsigned>(sg.C * sg.segs), static_cast<unsigned>(sg.osplits));
        pl.workspace = p.eval_mode ? 0 : static_cast<size_t>(channels) * sg.segs * sg.osplits * sizeof(double2);
        if (sg.segs != 1 || sg.osplits != 1) {      // (one workgroup per channel: it stores the sums itself, lsq_seg_body.hpp)
            pl.fin_seg = finalize_seg_kernel<T>;
            pl.fin_ch = fin_channels(channels);
            pl.fin_grid = dim3(static_cast<unsigned>((channels + pl.fin_ch - 1) / pl.fin_ch));
        }
        pl.note = LaunchNote{static_cast<int>(sg.C * sg.segs), sg.osplits, 0, 0, 3, 0, kBlock, 0};
        const bool short_walk = sg.sub_per_seg * sg.o_per_split <= kSegUpFrontBwd<IO> && knob::get(knob::kSegNoUpFront) == 0 &&
                                (sg.o_per_split == 1 || sg.C * sg.segs * sg.osplits <= 8 * static_cast<int64_t>(dev.cu_count));
        return with_bwd_modes(p, [&](auto S, auto I, auto E) {
            return pick_bwd_seg<IO, decltype(S)::value, decltype(I)::value, decltype(E)::value>(pl, short_walk, v);
        });
    }

    constexpr int VB = kWindowBwdVec<IO>;
    const int vecw = pick_vec(VB, channels * inner, true);
    const int cpl = pick_cpl(vecw, inner);
    // One channel per packet component (inner < V): a window spans 256 x V channels, so every workgroup ends with a
    // long epilogue and a 16-byte partial per slot, and the finalize has `splits` of them to fold per channel.  Fewer,
    // fatter workgroups win there in every shape swept (profiles/r01_lastaxis_sweep.txt: 2 per CU; [8192, 4096] fp32
    // 82 us against 100 us at 16 per CU, [200704, 256] 133 against 205).
    const bool last_axis = vecw > 1 && cpl == vecw;
    // (under 512 MB only, ww_max_elems; variant bit 11 (tools) forces the 256-lane windows, for A/B runs)
    if (last_axis && inner == 1 && !(variant & (1 << 11)) && (variant != 0 || outer * channels < ww_max_elems<IO>())) {
        // the quantized axis is the last one ([tokens, features], channels-last): row-group windows, one round of what
        // the chip holds (variant: workgroups per CU requested, rounded to whole rounds)
        const BwdPcCall call{outer, channels, inner, variant == 0 ? dev.cu_count * kWwBwdBlocksPerCU : target,
                             /*default_variant=*/variant == 0, /*whole_rounds=*/true, ring_ok, v};
        return bwd_pc_modes<IO, VB, VB, true>(call, p, pl);
    }
    const int target_w = (variant == 0 && last_axis) ? dev.cu_count * kLastAxisBwdBlocksPerCU : target;
    const BwdPcCall call{outer, channels, inner, target_w, /*default_variant=*/variant == 0, /*whole_rounds=*/!last_axis, ring_ok, v};
    if (vecw == 1) return bwd_pc_modes<IO, 1, 1>(call, p, pl);
    if (cpl == 1) return bwd_pc_modes<IO, VB, 1>(call, p, pl);
    if (cpl == 2) return bwd_pc_modes<IO, VB, 2>(call, p, pl);
    return bwd_pc_modes<IO, VB, VB>(call, p, pl);
}

}  // namespace lsq
