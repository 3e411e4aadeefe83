// lsq_pc_seg.hpp -- SEGMENT mode of the single-tensor per-channel ops: the two kernels, entry points over the walk of
// lsq_seg_body.hpp (which lsq_multi.hip runs for many tensors at once).
#pragma once
#include "lsq_seg_body.hpp"

namespace lsq {

// =================================================================================================
// SEGMENT mode: one channel per workgroup
// =================================================================================================
template <typename IO, int V, bool INIT, bool LEVELS, int UNROLL, bool NTL, bool NTS, int WALK>
__global__ __launch_bounds__(kBlock) void fwd_seg_kernel(const void* __restrict__ x, void* __restrict__ y,
                                                         int8_t* __restrict__ levels, int level_bias, int aux_kind, SegGeom g,
                                                         const typename IO::arith* __restrict__ scale,
                                                         const typename IO::arith* __restrict__ shift,
                                                         Range<typename IO::arith> r) {
    seg_forward<IO, V, INIT, LEVELS, UNROLL, NTL, NTS, WALK>(x, y, levels, level_bias, aux_kind, g, SegWalk(g), scale, shift, r);
}

// (SegDirect, seg_forward, seg_backward: lsq_seg_body.hpp)
template <typename IO, int V, bool SYM, bool INIT, bool EVAL, int UNROLL, bool NTL, bool NTS, int WALK>
__global__ __launch_bounds__(kBlock) void bwd_seg_kernel(const void* __restrict__ grad, const void* __restrict__ x,
                                                         void* __restrict__ dx, SegGeom g,
                                                         const typename IO::arith* __restrict__ scale,
                                                         const typename IO::arith* __restrict__ shift,
                                                         Range<typename IO::arith> r, typename IO::arith grad_scaler,
                                                         double2* __restrict__ partials,
                                                         SegDirect<typename IO::arith> direct) {
    seg_backward<IO, V, SYM, INIT, EVAL, UNROLL, NTL, NTS, WALK>(grad, x, dx, g, SegWalk(g), scale, shift, r, grad_scaler, partials,
                                                           static_cast<int64_t>(blockIdx.y) * gridDim.x + blockIdx.x, direct);
}

}  // namespace lsq
