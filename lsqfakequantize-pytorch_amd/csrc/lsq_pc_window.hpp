// lsq_pc_window.hpp -- WINDOW mode of the per-channel kernels, the pieces both directions share (lsq_pc_fwd.hpp,
// lsq_pc_bwd.hpp): the LDS image of a channel's constants (QSlot), the window's channel table in one step or in an
// "issue the loads" + "finish" pair, the channels of a lane (LaneChannels: from the table or straight from global memory),
// where an owner window stores its sums (PcDirect) and the segmented wave64 reduction keyed by runs of equal channel.
// The geometry (which lane sits where, which rows it walks) is lsq_pc_geom.hpp.
#pragma once
#include "lsq_kernels.hpp"
#include "lsq_pc_geom.hpp"

namespace lsq {

// =================================================================================================
// shared pieces
// =================================================================================================
template <typename T>
struct alignas(16) QSlot {  // LDS image of one channel's constants
    T s, inv_s, zp, pad;
};

// =================================================================================================
// WINDOW mode
// =================================================================================================
// One channel's slot from its raw scale / shift (lsq_kernel.h:157-158 + :12), and the slot of a window position past the
// last channel (no live lane reads it).  (build_channel_table / finish_channel_table below spell the same formula out:
// routing them through these two renames registers inside a loop of two forward kernels, so they stay as they are.)
template <typename T>
__device__ __forceinline__ QSlot<T> make_qslot(T scale, T shift, const Range<T>& r) {
    const QParams<T> q = make_qparams<T>(sanitize_scale_per_channel<T>(scale), shift, r);
    QSlot<T> e;
    e.s = q.s; e.inv_s = q.inv_s; e.zp = q.zp; e.pad = static_cast<T>(0);
    return e;
}
template <typename T>
__device__ __forceinline__ QSlot<T> idle_qslot() {
    QSlot<T> e;
    e.s = static_cast<T>(1); e.inv_s = static_cast<T>(1); e.zp = static_cast<T>(0); e.pad = static_cast<T>(0);
    return e;
}

// Build the window's channel table in LDS (lsq_kernel.h:157-158 + :12, once per channel).
template <typename T>
__device__ __forceinline__ void build_channel_table(QSlot<T>* table, int k_count, int64_t c_lo, int64_t C,
                                                    const T* __restrict__ scale, const T* __restrict__ shift,
                                                    const Range<T>& r) {
    for (int k = threadIdx.x; k < k_count; k += kBlock) {
        const int64_t c = c_lo + k;
        QSlot<T> e;
        if (c < C) {
            const QParams<T> q = make_qparams<T>(sanitize_scale_per_channel<T>(scale[c]), shift[c], r);
            e.s = q.s; e.inv_s = q.inv_s; e.zp = q.zp; e.pad = static_cast<T>(0);
        } else {
            e.s = static_cast<T>(1); e.inv_s = static_cast<T>(1); e.zp = static_cast<T>(0); e.pad = static_cast<T>(0);
        }
        table[k] = e;
    }
}

// The same in two steps, for kernels that put their first rows in flight before the table exists: the scale / shift loads
// are ISSUED first (vector-memory operations retire in issue order: a wait for a load behind the rows' loads would be a wait
// for the rows), the row loads follow, and the table is finished when its raw values are needed.  Up to kRawSlots table
// slots per thread travel in registers; wider windows (last-axis windows of more than 512 channels) use build_channel_table.
constexpr int kRawSlots = 2;
template <typename T>
struct ChannelRaw {
    T s[kRawSlots], b[kRawSlots];
};
template <typename T>
__device__ __forceinline__ ChannelRaw<T> load_channel_raw(int k_count, int64_t c_lo, int64_t C, const T* __restrict__ scale,
                                                          const T* __restrict__ shift) {
    ChannelRaw<T> raw;
#pragma unroll
    for (int i = 0; i < kRawSlots; ++i) {
        const int k = threadIdx.x + i * kBlock;
        int64_t c = c_lo + k;
        c = (k < k_count && c < C) ? c : (C - 1);        // (a valid address for the lanes without a slot: the value is unused)
        raw.s[i] = scale[c];
        raw.b[i] = shift[c];
    }
    return raw;
}
template <typename T>
__device__ __forceinline__ void finish_channel_table(QSlot<T>* table, int k_count, int64_t c_lo, int64_t C, const ChannelRaw<T>& raw,
                                                     const Range<T>& r) {
#pragma unroll
    for (int i = 0; i < kRawSlots; ++i) {
        const int k = threadIdx.x + i * kBlock;
        if (k < k_count) {
            QSlot<T> e;
            if (c_lo + k < C) {
                const QParams<T> q = make_qparams<T>(sanitize_scale_per_channel<T>(raw.s[i]), raw.b[i], r);
                e.s = q.s; e.inv_s = q.inv_s; e.zp = q.zp; e.pad = static_cast<T>(0);
            } else {
                e.s = static_cast<T>(1); e.inv_s = static_cast<T>(1); e.zp = static_cast<T>(0); e.pad = static_cast<T>(0);
            }
            table[k] = e;
        }
    }
}
// first channel of workgroup blockIdx.x's window (LaneSite::c_lo without the per-lane part)
__device__ __forceinline__ int64_t window_first_channel(const PcGeom& g) {
    if (g.own) return own_window(g) * g.k_slots;
    return g.R == 1 ? udiv(static_cast<int64_t>(blockIdx.x) * g.wpos, g.inner, g.fits32 != 0) : 0;
}

// Where an OWNER-window backward stores its channels' finished sums (d_scale / d_shift, rounded once; wide: un-rounded).
template <typename T>
struct PcDirect {
    T* ds;
    T* db;
    double* wide;
    T sym_term;         // the constant per-element d_shift term of the symmetric case, 0 * grad_scaler (lsq_kernel.h:118,122)
    int32_t sym;
};

// CPL = channels a lane can touch: 1 (inner % V == 0), 2 (inner >= V), V (anything).
template <typename T, int V, int CPL>
struct LaneChannels {
    static constexpr int N = (CPL == 1) ? 1 : (CPL == 2 ? 2 : V);
    QParams<T> q[N];
    int32_t key[N];   // slot index in the window table
    int32_t split;    // CPL == 2: components j >= split belong to q[1]
    __device__ __forceinline__ void init(const QSlot<T>* table, const LaneSite& s, const PcGeom& g) {
        // dead lanes (past the row end / beyond the tile rows) point at slot 0 and never accumulate.
        // Everything is computed into scalars first so the struct stays in registers.
        const bool f32 = g.fits32 != 0;
        const int64_t p0 = s.live ? s.p0 : s.c_lo * g.inner;
        const int64_t c0 = udiv(p0, g.inner, f32);
        int32_t sp = V;
        if (CPL == 2) {
            const int64_t left = (c0 + 1) * g.inner - p0;  // elements of channel c0 from p0 on
            sp = (s.live && left < V) ? static_cast<int32_t>(left) : V;
        }
        split = sp;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            int32_t k;
            if (N == 1 || j == 0) k = static_cast<int32_t>(c0 - s.c_lo);
            else if (CPL == 2) k = static_cast<int32_t>(c0 - s.c_lo) + (sp < V ? 1 : 0);
            else k = s.live ? static_cast<int32_t>(udiv(p0 + j, g.inner, f32) - s.c_lo) : 0;
            key[j] = k;
            const QSlot<T> e = table[k];
            q[j].s = e.s; q[j].inv_s = e.inv_s; q[j].zp = e.zp;
        }
    }
    // CPL == V without a table: a lane whose V components are V (mostly) different channels -- the quantized axis is the last
    // or nearly the last one -- reads ITS channels' scale / shift itself.  A 256-lane window then shares nothing through the
    // table (2048 channels, 2048 lanes' worth of slots), so building one is pure latency: global loads -> divisions -> LDS
    // writes -> barrier -> LDS reads.  Two steps, like load_channel_raw / finish_channel_table: the loads are issued before
    // the first rows' loads, the divisions happen when the rows are in flight.
    __device__ __forceinline__ void load_direct(const T* __restrict__ scale, const T* __restrict__ shift, const LaneSite& s,
                                                const PcGeom& g, T (&rs)[N], T (&rb)[N]) {
        const bool f32 = g.fits32 != 0;
        const int64_t p0 = s.live ? s.p0 : s.c_lo * g.inner;
        if constexpr (CPL == V && V > 2) {
            split = V;
            const bool wide = g.inner == 1 && p0 + V <= g.C &&
                              ((reinterpret_cast<uintptr_t>(scale) | reinterpret_cast<uintptr_t>(shift)) & 15u) == 0;
            if (wide) {      // V consecutive channels from a multiple of V on: 16-byte loads
                struct alignas(16) Pack { T v[N]; };
                const Pack a = *reinterpret_cast<const Pack*>(scale + p0);
                const Pack b = *reinterpret_cast<const Pack*>(shift + p0);
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    key[j] = static_cast<int32_t>(p0 + j - s.c_lo);
                    rs[j] = a.v[j];
                    rb[j] = b.v[j];
                }
                return;
            }
#pragma unroll
            for (int j = 0; j < N; ++j) {
                int64_t c = udiv(p0 + j, g.inner, f32);
                c = c < g.C ? c : g.C - 1;
                key[j] = static_cast<int32_t>(c - s.c_lo);
                rs[j] = scale[c];
                rb[j] = shift[c];
            }
        } else {
            // one channel, or two with a split point (init() above, from global memory instead of the table)
            const int64_t c0 = udiv(p0, g.inner, f32);
            int32_t sp = V;
            if (CPL == 2) {
                const int64_t left = (c0 + 1) * g.inner - p0;
                sp = (s.live && left < V) ? static_cast<int32_t>(left) : V;
            }
            split = sp;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                int64_t c = c0 + ((j > 0 && sp < V) ? 1 : 0);
                c = c < g.C ? c : g.C - 1;
                key[j] = static_cast<int32_t>(c - s.c_lo);
                rs[j] = scale[c];
                rb[j] = shift[c];
            }
        }
    }
    __device__ __forceinline__ void finish_direct(const T (&rs)[N], const T (&rb)[N], const Range<T>& r) {
#pragma unroll
        for (int j = 0; j < N; ++j) q[j] = make_qparams<T>(sanitize_scale_per_channel<T>(rs[j]), rb[j], r);
    }
    // constants of component j, by select (never a runtime-indexed register array -> no scratch)
    __device__ __forceinline__ QParams<T> params(int j) const {
        if (N == 1) return q[0];
        if (CPL == 2) {
            const bool hi = j >= split;
            QParams<T> o;
            o.s = hi ? q[N - 1].s : q[0].s;
            o.inv_s = hi ? q[N - 1].inv_s : q[0].inv_s;
            o.zp = hi ? q[N - 1].zp : q[0].zp;
            return o;
        }
        return q[j < N ? j : 0];
    }
    // constants of the component pair (2 pr, 2 pr + 1), fp32 arithmetic: what backward_pair / forward_pair take.  Built
    // field by field from scalars (selects for the two-channel form) -- once, before the row loop.
    __device__ __forceinline__ QPair pair(int pr) const {
        static_assert(std::is_same<T, float>::value || N == 0, "pairs are an fp32 construct");
        QPair o;
        if (N == 1) {
            o.s = f2{q[0].s, q[0].s}; o.inv_s = f2{q[0].inv_s, q[0].inv_s}; o.zp = f2{q[0].zp, q[0].zp};
        } else if (CPL == 2) {
            const bool h0 = 2 * pr >= split, h1 = 2 * pr + 1 >= split;
            o.s = f2{h0 ? q[N - 1].s : q[0].s, h1 ? q[N - 1].s : q[0].s};
            o.inv_s = f2{h0 ? q[N - 1].inv_s : q[0].inv_s, h1 ? q[N - 1].inv_s : q[0].inv_s};
            o.zp = f2{h0 ? q[N - 1].zp : q[0].zp, h1 ? q[N - 1].zp : q[0].zp};
        } else {
            const int a = 2 * pr < N ? 2 * pr : 0, b = 2 * pr + 1 < N ? 2 * pr + 1 : 0;
            o.s = f2{q[a].s, q[b].s}; o.inv_s = f2{q[a].inv_s, q[b].inv_s}; o.zp = f2{q[a].zp, q[b].zp};
        }
        return o;
    }
};

// Segmented wave64 reduction: lanes hold (key, s, b).  A RUN is a maximal group of ADJACENT lanes
// with the same key (equal keys may re-appear further away -- folded rows, inner < V -- so runs are
// numbered with a ballot + popcount and the scan is keyed by run id, not by channel).  After
// log2(64) shuffle steps the first lane of every run owns the run total and adds it to the
// window's LDS slot with an LDS fp64 atomic (ds_add_f64).
// The two halves are separate so that the shuffles of all waves run side by side while the ADDS can be made in wave order
// (bwd_pc_kernel's epilogue): segmented_wave_reduce leaves the run total in (s, b) of the run's first lane and says whether
// this lane is one that adds; segmented_wave_commit adds.
template <bool SYM>
__device__ __forceinline__ bool segmented_wave_reduce(int key, double& s, double& b) {
    const int lane = threadIdx.x & 63;
    const int prev = __shfl_up(key, 1, 64);
    const bool head = (lane == 0) || (prev != key);
    const unsigned long long heads = __ballot(head);
    const int run = __popcll(heads & (~0ull >> (63 - lane)));  // heads at or below this lane: unique per run
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int orun = __shfl_down(run, d, 64);
        const double os = shfl_down_f64(s, d);
        const double ob = SYM ? 0.0 : shfl_down_f64(b, d);
        if (lane + d < 64 && orun == run) {
            s += os;
            if (!SYM) b += ob;
        }
    }
    return head && key >= 0;
}
template <bool SYM>
__device__ __forceinline__ void segmented_wave_commit(bool adds, int key, double s, double b, double* lds_s, double* lds_b) {
    if (adds) {
        __hip_atomic_fetch_add(&lds_s[key], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (!SYM) __hip_atomic_fetch_add(&lds_b[key], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

}  // namespace lsq
