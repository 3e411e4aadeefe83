// lsq_pc_finalize.hpp -- the fixed-order finalize kernels of the per-channel backward: they fold the partials of the
// window kernels (finalize_pc_kernel), the row-group windows (finalize_ww_kernel) and the segment kernels
// (finalize_seg_kernel) into d_scale / d_shift; fin_channels picks the channels per finalize workgroup (host).
#pragma once
#include "lsq_kernels.hpp"
#include "lsq_pc_geom.hpp"

namespace lsq {

// Finalize (window mode): folds, in a fixed order, every (split, window) partial that can hold a piece
// of a channel (the reference's `ds_buffer.sum(axes != axis)`, lsq_cpu.cpp:287-292).  A workgroup
// handles fin_ch channels x (256 / fin_ch) interleaved slices of a channel's partials, so each lane issues only
// a few INDEPENDENT loads (a one-lane-per-channel loop serialised `splits` dependent HBM latencies); the
// slices are then combined through LDS by a fixed-order tree.
constexpr int kFinCh = 32;   // channels per finalize workgroup when there are at least that many

// Channels per finalize workgroup: a power of two, at most 32, chosen so that the finalize grid still has ~256
// workgroups when the channel count allows it: with few channels (RGB inputs; 768 features x 512 row slabs) the
// lanes of a workgroup share a channel's partials -- there can be thousands -- instead of 24 workgroups walking
// them one lane per channel.
static inline int fin_channels(int64_t C) {
    const int o = knob::get(knob::kFinCh);        // tools build only: a power of two <= kFinCh
    if (o > 0) return o > kFinCh ? kFinCh : (o & (o - 1)) ? 1 : o;
    int ch = 1;
    while (ch < kFinCh && static_cast<int64_t>(ch) * 2 * 256 <= C) ch <<= 1;
    // ... but at least 8 channels (128 contiguous bytes of partials per split) where there are that many: better
    // coalescing beats the extra workgroups (profiles/r02_finalize_channels_sweep.txt: 1-2 us on every shape)
    while (ch < 8 && static_cast<int64_t>(ch) * 2 <= C) ch <<= 1;
    return ch;
}

// Fixed-order combination of the kBlock / fin_ch slices of every channel (fin_ch a power of two <= 32, thread t holds
// channel t % fin_ch): a wave64 butterfly over the lane bits above the channel bits, then the four wave results
// through LDS -- one barrier.  Threads 0 .. fin_ch-1 return their channel's total.
__device__ __forceinline__ double2 combine_parts(double2* wave_part, int fin_ch, double s, double b) {
    for (int m = 32; m >= fin_ch; m >>= 1) {
        s += shfl_xor_f64(s, m);
        b += shfl_xor_f64(b, m);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < fin_ch) wave_part[wave * kFinCh + lane] = make_double2(s, b);
    __syncthreads();
    double2 t = make_double2(0.0, 0.0);
    if (threadIdx.x < fin_ch) {
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) {
            t.x += wave_part[w * kFinCh + threadIdx.x].x;
            t.y += wave_part[w * kFinCh + threadIdx.x].y;
        }
    }
    return t;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void finalize_pc_kernel(const double2* __restrict__ partials, PcGeom g, int fin_ch,
                                                             int eval_mode, int sym, T sym_term, T* __restrict__ ds,
                                                             T* __restrict__ db, double* __restrict__ wide) {
    __shared__ double2 wave_part[(kBlock / 64) * kFinCh];
    const int parts = kBlock / fin_ch;
    const int lane_c = threadIdx.x % fin_ch, part = threadIdx.x / fin_ch;
    const int64_t c = static_cast<int64_t>(blockIdx.x) * fin_ch + lane_c;
    double s = 0.0, b = 0.0;
    if (!eval_mode && c < g.C) {
        const bool f32 = g.fits32 != 0;      // row positions fit 32 bits: every division below is a 32-bit one
        int64_t w_lo = 0, w_hi = 0;
        if (g.R == 1) {
            w_lo = udiv(c * g.inner, g.wpos, f32);
            w_hi = udiv((c + 1) * g.inner - 1, g.wpos, f32);
        }
        // the (window, split) pairs holding a piece of channel c, flattened and dealt out to the `parts` lanes of c
        const int64_t total = (w_hi - w_lo + 1) * g.splits;
        const int64_t stride = g.n_windows * g.k_slots;
        const bool idx32 = total < 0x7fffffffLL;
#pragma unroll 4
        for (int64_t idx = part; idx < total; idx += parts) {
            const int64_t wi = udiv(idx, g.splits, idx32);
            const int64_t w = w_lo + wi;
            const int64_t sy = idx - wi * g.splits;
            const int64_t c_lo = (g.R == 1) ? udiv(w * g.wpos, g.inner, f32) : 0;
            const double2 v = partials[sy * stride + w * g.k_slots + (c - c_lo)];
            s += v.x;
            b += v.y;
        }
    }
    const double2 t = combine_parts(wave_part, fin_ch, s, b);
    if (part == 0 && c < g.C) {
        double ts = t.x, tb = t.y;
        if (!eval_mode && sym) tb = 0.0 + static_cast<double>(sym_term);
        ds[c] = static_cast<T>(ts);
        db[c] = static_cast<T>(tb);
        if (wide) {
            wide[c] = ts;
            wide[g.C + c] = tb;
        }
    }
}

// Finalize (row-group windows): the partials are [splits][n_windows * w V] in slot order (slot = component * w + lane
// inside a window), so consecutive threads read consecutive 16-byte partials; thread -> slot -> channel
// c = window * w V + lane * V + component.  fin_ch slots x (256 / fin_ch) interleaved slices of the splits per
// workgroup, fixed-order combination as in finalize_pc_kernel.
template <typename T>
__global__ __launch_bounds__(kBlock) void finalize_ww_kernel(const double2* __restrict__ partials, PcGeom g, int fin_ch,
                                                             int eval_mode, int sym, T sym_term, T* __restrict__ ds,
                                                             T* __restrict__ db, double* __restrict__ wide) {
    __shared__ double2 wave_part[(kBlock / 64) * kFinCh];
    const int parts = kBlock / fin_ch;
    const int lane_c = threadIdx.x % fin_ch, part = threadIdx.x / fin_ch;
    const uint32_t k_slots = static_cast<uint32_t>(g.k_slots), w = static_cast<uint32_t>(g.ww_lanes);
    const uint32_t total_slots = static_cast<uint32_t>(g.n_windows) * k_slots;     // ~ the channel count: fits 32 bits
    const uint32_t gslot = blockIdx.x * static_cast<uint32_t>(fin_ch) + lane_c;
    const uint32_t win = gslot / k_slots, k = gslot - win * k_slots;
    const uint32_t comp = k / w, lane = k - comp * w;
    const int64_t c = static_cast<int64_t>(win) * k_slots + static_cast<int64_t>(lane) * g.vec + comp;
    const bool valid = gslot < total_slots && c < g.C;
    double s = 0.0, b = 0.0;
    if (!eval_mode && valid) {
        const double2* col = partials + gslot;
#pragma unroll 4
        for (int sy = part; sy < g.splits; sy += parts) {
            const double2 v = col[static_cast<int64_t>(sy) * total_slots];
            s += v.x;
            b += v.y;
        }
    }
    const double2 t = combine_parts(wave_part, fin_ch, s, b);
    if (part == 0 && valid) {
        double ts = t.x, tb = t.y;
        if (!eval_mode && sym) tb = 0.0 + static_cast<double>(sym_term);
        ds[c] = static_cast<T>(ts);
        db[c] = static_cast<T>(tb);
        if (wide) {
            wide[c] = ts;
            wide[g.C + c] = tb;
        }
    }
}

// Finalize (segment mode): fin_ch channels x (256 / fin_ch) interleaved slices of the (osplit, seg) partials.
template <typename T>
__global__ __launch_bounds__(kBlock) void finalize_seg_kernel(const double2* __restrict__ partials, SegGeom g, int fin_ch,
                                                              int eval_mode, int sym, T sym_term, T* __restrict__ ds,
                                                              T* __restrict__ db, double* __restrict__ wide) {
    __shared__ double2 wave_part[(kBlock / 64) * kFinCh];
    const int parts = kBlock / fin_ch;
    const int lane_c = threadIdx.x % fin_ch, part = threadIdx.x / fin_ch;
    const int64_t c = static_cast<int64_t>(blockIdx.x) * fin_ch + lane_c;
    double s = 0.0, b = 0.0;
    if (!eval_mode && c < g.C) {
        const int64_t gx = g.C * g.segs;
        const int32_t total = g.osplits * g.segs;
#pragma unroll 4
        for (int32_t sl = part; sl < total; sl += parts) {
            const int32_t oy = sl / g.segs, sg = sl - oy * g.segs;
            const double2 v = partials[static_cast<int64_t>(oy) * gx + c * g.segs + sg];
            s += v.x;
            b += v.y;
        }
    }
    const double2 t = combine_parts(wave_part, fin_ch, s, b);
    if (part == 0 && c < g.C) {
        double ts = t.x, tb = t.y;
        if (!eval_mode && sym) tb = 0.0 + static_cast<double>(sym_term);
        ds[c] = static_cast<T>(ts);
        db[c] = static_cast<T>(tb);
        if (wide) {
            wide[c] = ts;
            wide[g.C + c] = tb;
        }
    }
}

}  // namespace lsq
