// lsq_pc_fwd.hpp -- K3 (window mode): the per-channel forward, y (and / or the one-byte levels) from x.
// Constants issued, first rows in flight, constants finished, then one of two walks: the LDS-DMA ring (DMA > 0) or
// register groups of UNROLL, UNROLL/2, ..., 1 rows.
#pragma once
#include "lsq_pc_window.hpp"

namespace lsq {

// ------------------------------------------------------------------------------------------------
// K3 (window mode): forward
// ------------------------------------------------------------------------------------------------
// DMA > 0: the rows arrive through an LDS-DMA ring of DMA stages per wave (see bwd_pc_kernel): DMA rows in flight per
// wave and no load registers.
template <typename IO, int V, int CPL, bool INIT, bool LEVELS, int UNROLL, bool NTL, bool NTS, int DMA = 0>
__global__ __launch_bounds__(kBlock) void fwd_pc_kernel(const void* __restrict__ x, void* __restrict__ y,
                                                        int8_t* __restrict__ levels, int level_bias, int aux_kind, PcGeom g,
                                                        const typename IO::arith* __restrict__ scale,
                                                        const typename IO::arith* __restrict__ shift,
                                                        Range<typename IO::arith> r) {
    using T = typename IO::arith;
    using E = typename IO::elem;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    QSlot<T>* table = reinterpret_cast<QSlot<T>*>(smem);

    // no table at all (LaneChannels::load_direct) where a lane's components are different channels: forward_per_channel's choice
    using LC = LaneChannels<T, V, CPL>;
#ifdef LSQ_TOOLS     // (knob 4: also lanes of one or two channels -- measured neutral, +-2 %, profiles/r03_fwd_direct_ab.txt)
    constexpr bool kDirectAble = DMA == 0;
#else
    constexpr bool kDirectAble = CPL == V && V > 2 && DMA == 0;     // (V == 2: CPL == 2 is the two-channel form)
#endif
    const bool direct = kDirectAble && g.direct != 0;
    // the window's raw scale / shift first (issue order = retirement order), then the first rows, then the table
    const bool raw_first = !direct && g.k_slots <= kRawSlots * kBlock;
    ChannelRaw<T> raw;
    if (raw_first) raw = load_channel_raw<T>(g.k_slots, window_first_channel(g), g.C, scale, shift);
    const LaneSite site = lane_site(g, V);
    const RowWalk walk(g, site);
    LC ch;
    T direct_s[LC::N], direct_b[LC::N];
    if constexpr (kDirectAble) {
        if (direct) ch.load_direct(scale, shift, site, g, direct_s, direct_b);
    }
    // the first group of loads does not depend on the channel constants: put it in flight before the
    // table build (a division + a barrier) so the two latencies overlap
    E first[UNROLL][V];
    const bool first_full = DMA > 0 ? false : walk.n_rows >= UNROLL;
    if (first_full) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) load_elems<IO, V, NTL>(x, walk.row(u) * g.L + site.p0, first[u]);
    }
    // ---- LDS-DMA ring (DMA > 0): this wave's DMA stages of 64 x packets ----
    static_assert(DMA == 0 || V * sizeof(E) == 16, "the LDS-DMA ring moves 16-byte packets");
    constexpr int kStage = 64 * 16;
    const int64_t dma_n = walk.n_tiles_split;
    const uint32_t front = (static_cast<uint32_t>(g.k_slots) * static_cast<uint32_t>(sizeof(QSlot<T>)) + 1023u) & ~1023u;
    unsigned char* ring = smem + front + (threadIdx.x >> 6) * (DMA * kStage);
    const uint32_t ring_lds = DMA > 0 ? __builtin_amdgcn_readfirstlane(lds_offset_of(ring)) : 0u;
    auto dma_issue = [&](int64_t i) {
        int64_t row = walk.row(i);
        row = row < g.outer ? row : g.outer - 1;
        const int64_t e = row * g.L + (site.live ? site.p0 : 0);
        glds16_rt(static_cast<const E*>(x) + e, ring_lds + static_cast<uint32_t>(i % (DMA > 0 ? DMA : 1)) * kStage, g.ring_nt);
    };
    if constexpr (DMA > 0) {
        for (int64_t i = 0; i < DMA && i < dma_n; ++i) dma_issue(i);
    }
    if (direct) {
        if constexpr (kDirectAble) ch.finish_direct(direct_s, direct_b, r);
    } else {
        if (raw_first) finish_channel_table<T>(table, g.k_slots, site.c_lo, g.C, raw, r);
        else build_channel_table<T>(table, g.k_slots, site.c_lo, g.C, scale, shift, r);
        __syncthreads();
        ch.init(table, site, g);
    }
    const T bias = static_cast<T>(level_bias);

    // fp32 arithmetic on packets: two elements at a time (forward_pair: packed multiplies and adds), the lane's constants
    // per component pair in registers for the whole walk
    constexpr bool PAIRS = std::is_same<T, float>::value && V >= 2;
    QPair qp[PAIRS ? V / 2 : 1];
    if constexpr (PAIRS) {
#pragma unroll
        for (int pr = 0; pr < V / 2; ++pr) qp[pr] = ch.pair(pr);
    }
    auto emit_row = [&](int64_t oo, const E (&in)[V], bool valid) {
        const int64_t e = oo * g.L + site.p0;
        E out[V];
        LevelPack<V> lv;
        if constexpr (PAIRS) {
#pragma unroll
            for (int pr = 0; pr < V / 2; ++pr) {
                const f2 xv = f2{static_cast<T>(in[2 * pr]), static_cast<T>(in[2 * pr + 1])};
                f2 c;
                const f2 yv = forward_pair(xv, qp[pr], r, c);
                out[2 * pr] = out_elem<IO, INIT>(INIT ? xv.x : yv.x);
                out[2 * pr + 1] = out_elem<IO, INIT>(INIT ? xv.y : yv.y);
                if (LEVELS) {
                    lv.b[2 * pr] = aux_byte<T>(c.x, r, bias, aux_kind);
                    lv.b[2 * pr + 1] = aux_byte<T>(c.y, r, bias, aux_kind);
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const QParams<T> q = ch.params(j);
                const T xv = static_cast<T>(in[j]);
                const T c = clamped<T>(xv, q, r);
                out[j] = out_elem<IO, INIT>(INIT ? xv : dequant<T>(rne(c), q));
                if (LEVELS) lv.b[j] = aux_byte<T>(c, r, bias, aux_kind);
            }
        }
        if (valid) {
            if (!LEVELS || y != nullptr) store_elems<IO, V, NTS>(y, e, out);     // y == NULL: the one-byte output only
            if (LEVELS) lv.store(levels + e);
        }
    };

    // rows = full groups of UNROLL (every load issued before the first use) + one group of UNROLL/2 + ... + one
    // single row: no padded slots (a lane walks only a handful of rows at the BASELINE shapes)
    auto group = [&](int64_t i0, auto width) {
        constexpr int H = decltype(width)::value;
        E in[H][V];
#pragma unroll
        for (int u = 0; u < H; ++u) load_elems<IO, V, NTL>(x, walk.row(i0 + u) * g.L + site.p0, in[u]);
#pragma unroll
        for (int u = 0; u < H; ++u) emit_row(walk.row(i0 + u), in[u], true);
    };
    int64_t i = 0;
    if constexpr (DMA > 0) {
        // one copy per row: younger than row i's are the copies of rows i+1 .. i+DMA-1 (the y stores in between are not
        // counted: the wait is never too short)
        const int lane = threadIdx.x & 63;
        using V4 = __attribute__((ext_vector_type(4))) unsigned int;
        auto consume = [&](int64_t it, bool refill) {
            const V4 raw = *reinterpret_cast<const V4*>(ring + static_cast<uint32_t>(it % DMA) * kStage + lane * 16);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (refill) dma_issue(it + DMA);
            E in[V];
            __builtin_memcpy(&in[0], &raw, 16);
            emit_row(walk.row(it) < g.outer ? walk.row(it) : g.outer - 1, in, it < walk.n_rows);
        };
        for (; i + DMA < dma_n; ++i) {
            wait_vm<DMA - 1>();
            consume(i, true);
        }
        for (; i < dma_n; ++i) {
            wait_vm_upto(static_cast<int>(dma_n - 1 - i));
            consume(i, false);
        }
        return;
    }
    if (first_full) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) emit_row(walk.row(u), first[u], true);
        i = UNROLL;
    }
    for (; i + UNROLL <= walk.n_rows; i += UNROLL) group(i, std::integral_constant<int, UNROLL>{});
    if constexpr (UNROLL >= 8) if (i + 4 <= walk.n_rows) { group(i, std::integral_constant<int, 4>{}); i += 4; }
    if constexpr (UNROLL >= 4) if (i + 2 <= walk.n_rows) { group(i, std::integral_constant<int, 2>{}); i += 2; }
    if constexpr (UNROLL >= 2) if (i < walk.n_rows) group(i, std::integral_constant<int, 1>{});
}

}  // namespace lsq
