// lsq_per_channel.hip -- K3 (forward) and K4 (fused backward + per-channel reduction) on gfx950.
//
// Replaces the reference's per-channel CUDA backend (/root/reference/torchlsq/csrc/ops/cuda/lsq_cuda.cu:147-297):
// TensorIterator-broadcast scale/shift with a division per element (lsq_kernel.h:157-158), three
// elementwise backward kernels, three N-sized temporaries and two `sum(axes != axis)`.
//
// Data view: dense memory as [outer][C][inner]; a "row" is the L = C*inner elements of one outer
// index, position p of a row belongs to channel p / inner.
//
// CDNA4 design: CHANNEL-STATIONARY LANES.  A lane keeps the same channel(s) for its whole life, so
// the per-channel constants {s, 1/s, zp} sit in registers, no per-element index arithmetic or
// division is left in the loop (the reference divides per element), and every wave instruction still
// moves 1 KiB of contiguous HBM.  Two work decompositions, chosen on the host:
//
//  * WINDOW mode (many rows: activations, [batch, features], channels-last).  A workgroup owns a
//    window of W = 256 lanes x V positions of the row and walks down a slab of rows; short rows
//    (L < W) fold R = W/L rows into one tile.  The window's channel table is computed ONCE per
//    workgroup into LDS and fanned out to the lanes (1 lane = 1, 2 or V channels, template CPL).
//    d_scale/d_shift: fp64 lane accumulators -> segmented wave64 shuffle reduction keyed by runs of
//    equal channel -> LDS fp64 atomics (ds_add_f64) on the window's channel slots -> one partial per
//    (workgroup, slot) -> fixed-order finalize.
//  * SEGMENT mode (few rows, long channels: conv/linear weights on axis 0).  A workgroup owns a
//    segment of ONE channel row (sub-rows of W positions) for a range of outer indices: one channel
//    per workgroup, its constants computed in registers, reduction = wave64 butterfly + 4 partials
//    through LDS -> one partial per workgroup -> fixed-order finalize.
//
// Loads are never predicated (a predicated version serialised them behind s_waitcnt) and no slot of a load group
// is padding: a walk of n rows is cut into groups of UNROLL, then UNROLL/2, ..., 1 rows.  Only the software-pipelined
// loop of the 16-bit backward, whose prefetch can run past the end, re-reads the last row (clamped address, served
// by L2) and masks its effects.  No global atomics, no zero-initialised buffers.
//
// This file is the translation unit (compiled once per storage type, -DLSQ_PC_IO): the launchers, the workspace sizing and
// the instantiations.  The rest by subject: lsq_pc_window.hpp (channel table, LaneChannels, segmented wave reduce),
// lsq_pc_fwd.hpp (K3), lsq_pc_bwd.hpp (K4), lsq_pc_finalize.hpp (finalizers), lsq_pc_seg.hpp (segment kernels),
// lsq_pc_plan.hpp (policy constants, plans), lsq_pc_geom.hpp (geometry), lsq_seg_body.hpp (the segment walk).
#include "lsq_pc_plan.hpp"

namespace lsq {

template <typename IO>
hipError_t forward_per_channel(const void* x, void* y, int64_t outer, int64_t channels, int64_t inner,
                               const void* scale, const void* shift, const lsq_params& p,
                               const lsq_fwd_extras* ex, int variant, hipStream_t stream) {
    using T = typename IO::arith;
    int8_t* levels = ex ? static_cast<int8_t*>(ex->levels) : nullptr;
    const int bias = ex ? ex->level_bias : 0;
    const int aux_kind = ex ? ex->aux_kind : 0;
    // Packets need ELEMENT alignment only (lsq_math.hpp, PacketWord), which x and y have (lsq_capi.hip): a sliced view runs
    // the packet kernels' register loops.  What wants 16-byte sources is the LDS-DMA ring (ring_ok); the level bytes of a
    // packet are stored as one word.
    const bool packets_ok = !levels || (reinterpret_cast<uintptr_t>(levels) & 7u) == 0;
    FwdPcPlan<T> pl;
    if (hipError_t e = plan_forward<IO>(outer, channels, inner, p.init_mode != 0, levels != nullptr, packets_ok,
                                        is_aligned16(x) && is_aligned16(y), variant, pl))
        return e;
#ifdef LSQ_TOOLS
    last_launch_note() = pl.note;
#endif
    const Range<T> r = make_range<T>(p);
    const T* sc = static_cast<const T*>(scale);
    const T* sh = static_cast<const T*>(shift);
    if (pl.seg) {
        LSQ_NOTE_LAUNCH(pl.seg);
        hipLaunchKernelGGL(pl.seg, pl.grid, dim3(kBlock), 0, stream, x, y, levels, bias, aux_kind, pl.sg, sc, sh, r);
    } else {
        LSQ_NOTE_LAUNCH(pl.win);
        hipLaunchKernelGGL(pl.win, pl.grid, dim3(kBlock), pl.lds, stream, x, y, levels, bias, aux_kind, pl.g, sc, sh, r);
    }
    return hipGetLastError();
}

template <typename IO>
hipError_t backward_per_channel(const void* grad, const void* x, void* dx, void* ds, void* db, double* wide,
                                int64_t outer, int64_t channels, int64_t inner, const void* scale,
                                const void* shift, const lsq_params& p, void* workspace, size_t workspace_bytes,
                                int variant, hipStream_t stream) {
    using T = typename IO::arith;
    BwdPcPlan<T> pl;
    if (hipError_t e = plan_backward<IO>(outer, channels, inner, p, is_aligned16(grad) && is_aligned16(x) && is_aligned16(dx),
                                         variant, pl))
        return e;
    if (workspace_bytes < pl.workspace) return hipErrorInvalidValue;
#ifdef LSQ_TOOLS
    last_launch_note() = pl.note;
    if (pl.win) last_launch_note().vgprs_hint = registers_of(reinterpret_cast<const void*>(pl.win));   // (owner windows too)
#ifdef LSQ_TIMELINE
    pl.g.timeline = knob::timeline_buffer().load();
#endif
#endif
    const int64_t n4s = p.numel_for_scaler > 0 ? p.numel_for_scaler : outer * channels * inner;
    const T gs = grad_scaler_per_channel<T>(n4s, p.quant_max, channels, p.use_grad_scaling != 0, p.grad_scaler);
    const T sym_term = static_cast<T>(0) * gs;
    const Range<T> r = make_range<T>(p);
    const T* sc = static_cast<const T*>(scale);
    const T* sh = static_cast<const T*>(shift);
    T* const dsT = static_cast<T*>(ds);
    T* const dbT = static_cast<T*>(db);
    double2* const partials = static_cast<double2*>(workspace);
    const bool direct = !pl.fin_win && !pl.fin_seg;     // no finalize follows: the kernel stores d_scale / d_shift
    if (pl.seg) {
        const SegDirect<T> sd{direct ? dsT : nullptr, dbT, wide, sym_term};
        LSQ_NOTE_LAUNCH(pl.seg);
        hipLaunchKernelGGL(pl.seg, pl.grid, dim3(kBlock), 0, stream, grad, x, dx, pl.sg, sc, sh, r, gs, partials, sd);
    } else {
        const PcDirect<T> pd = direct ? PcDirect<T>{dsT, dbT, wide, sym_term, p.sym ? 1 : 0} : PcDirect<T>{nullptr, nullptr, nullptr, sym_term, 0};
        LSQ_NOTE_LAUNCH(pl.win);
        hipLaunchKernelGGL(pl.win, pl.grid, dim3(pl.g.block_threads), pl.lds, stream, grad, x, dx, pl.g, sc, sh, r, gs, partials, pd);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || direct) return e;
    const int eval = p.eval_mode ? 1 : 0, sym = p.sym ? 1 : 0;
    if (pl.seg) {
        LSQ_NOTE_LAUNCH(pl.fin_seg);
        hipLaunchKernelGGL(pl.fin_seg, pl.fin_grid, dim3(kBlock), 0, stream, partials, pl.sg, pl.fin_ch, eval, sym, sym_term, dsT, dbT, wide);
    } else {
        LSQ_NOTE_LAUNCH(pl.fin_win);
        hipLaunchKernelGGL(pl.fin_win, pl.fin_grid, dim3(kBlock), 0, stream, partials, pl.g, pl.fin_ch, eval, sym, sym_term, dsT, dbT, wide);
    }
    return hipGetLastError();
}

// lsq_hip_plan_backward_per_channel: what a backward over such buffers would launch
template <typename IO>
hipError_t plan_backward_per_channel(int64_t outer, int64_t channels, int64_t inner, const lsq_params& p, bool aligned16,
                                     LaunchNote& note) {
    BwdPcPlan<typename IO::arith> pl;
    const hipError_t e = plan_backward<IO>(outer, channels, inner, p, aligned16, 0, pl);
    note = pl.note;
    return e;
}

#ifdef LSQ_TOOLS
// Tools build: a caller may force any launch variant or knob, so the size is the maximum over every geometry the tuning
// range allows (tens of milliseconds of host time; lsq_capi.hip memoises it).
template <typename IO>
static size_t bwd_pc_workspace_bytes_any(int64_t outer, int64_t channels, int64_t inner) {
    const DeviceInfo& dev = device_info();
    size_t need = 0;
    const int vecs[3] = {IO::VEC, 1, 4};   // full packets, single elements, half packets (16-bit window backward)
    for (int vi = 0; vi < 3; ++vi) {
        for (int bpc = 1; bpc <= 2 * kMaxBlocksPerCU; ++bpc) {   // pick_splits may go up to twice the requested count
            for (int res = 0; res <= 8; ++res) {   // residency of the instantiation that will run: 0 (not used) .. 8 per CU
                const PcGeom g = make_geom(outer, channels, inner, vecs[vi], dev.cu_count * bpc, 27, dev.cu_count * res);
                need = std::max(need, static_cast<size_t>(g.splits) * g.n_windows * g.k_slots * sizeof(double2));
            }
            if (vi == 0 && inner == 1 && IO::VEC > 1 && channels % IO::VEC == 0) {
                for (int res = 0; res <= 8; ++res) {
                    for (int s64 = 0; s64 < 3; ++s64) {     // whole rows, 64-lane windows, 1024-lane workgroups
                        const PcGeom g = make_geom_ww(outer, channels, IO::VEC, dev.cu_count * bpc, ww_min_rows<IO>(), dev.cu_count * res,
                                                      s64 == 1, s64 == 2 ? kBigBlockOf<sizeof(typename IO::elem)> : kBlock);
                        need = std::max(need, static_cast<size_t>(g.splits) * g.n_windows * g.k_slots * sizeof(double2));
                    }
                }
            }
            if (vi < 2 && pick_segment_mode(vecs[vi], outer, channels, inner, dev.cu_count)) {
                const SegGeom sgm = make_seg_geom(outer, channels, inner, vecs[vi], dev.cu_count * bpc);
                need = std::max(need, static_cast<size_t>(channels) * sgm.segs * sgm.osplits * sizeof(double2));
            }
        }
    }
    return need + 256;
}
#endif

// Scratch bytes of the backward: the most any plan_backward (the library's own launch policy) asks for over the argument
// properties the size does not take: symmetric or not, init mode or not, 16-byte-aligned buffers or not (the launch
// takes element-aligned buffers only, lsq_capi.hip); eval mode needs none.  A few microseconds of host time (eight plans).
template <typename IO>
size_t bwd_pc_workspace_bytes(int64_t outer, int64_t channels, int64_t inner) {
    size_t need = 0;
#ifdef LSQ_TOOLS
    need = bwd_pc_workspace_bytes_any<IO>(outer, channels, inner);
#else
    lsq_params p{};
    for (int mode = 0; mode < 8; ++mode) {
        p.sym = mode & 1;
        p.init_mode = (mode >> 1) & 1;
        BwdPcPlan<typename IO::arith> pl;
        if (plan_backward<IO>(outer, channels, inner, p, (mode >> 2) != 0, 0, pl) == hipSuccess) need = std::max(need, pl.workspace);
    }
#endif
    return need + 256;
}

#define LSQ_INSTANTIATE(IO)                                                                                          \
    template hipError_t forward_per_channel<IO>(const void*, void*, int64_t, int64_t, int64_t, const void*,          \
                                                const void*, const lsq_params&, const lsq_fwd_extras*, int,          \
                                                hipStream_t);                                                        \
    template hipError_t backward_per_channel<IO>(const void*, const void*, void*, void*, void*, double*, int64_t,    \
                                                 int64_t, int64_t, const void*, const void*, const lsq_params&,      \
                                                 void*, size_t, int, hipStream_t);                                   \
    template hipError_t plan_backward_per_channel<IO>(int64_t, int64_t, int64_t, const lsq_params&, bool, LaunchNote&); \
    template size_t bwd_pc_workspace_bytes<IO>(int64_t, int64_t, int64_t);
// One translation unit per storage type (the Makefile compiles this file four times with -DLSQ_PC_IO=io_f32 ... in
// parallel: the window kernels' template space takes minutes in one piece); without the macro, all four.
#ifdef LSQ_PC_IO
LSQ_INSTANTIATE(LSQ_PC_IO)
#else
LSQ_INSTANTIATE(io_f32)
LSQ_INSTANTIATE(io_f64)
LSQ_INSTANTIATE(io_bf16)
LSQ_INSTANTIATE(io_f16)
#endif
#undef LSQ_INSTANTIATE

}  // namespace lsq
