// lsq_pc_bwd.hpp -- K4 (window mode): the fused per-channel backward, dx and the per-channel d_scale / d_shift sums.
// bwd_pc_kernel is three window families in one template (geometry: lsq_pc_geom.hpp make_geom / make_geom_ww /
// make_geom_own): 256-lane windows (!WW, BLOCK == kBlock), row-group windows (WW) and owner windows (!WW, BLOCK > kBlock).
// Its order: constants issued, first rows in flight, constants finished, one of three walks (LDS-DMA ring, software
// pipeline, plain groups), one of three epilogues (row groups combined in LDS / wave-ordered LDS adds + one partial row /
// owner sums stored directly).
#pragma once
#include "lsq_pc_window.hpp"

namespace lsq {

// ------------------------------------------------------------------------------------------------
// shader-clock stamps per wave (experiment build -DLSQ_TIMELINE, tools/exp_timeline.py); empty otherwise
// ------------------------------------------------------------------------------------------------
template <int BLOCK>
struct TimelineStamps {
#ifdef LSQ_TIMELINE
    unsigned long long t0 = 0, t1 = 0, t2 = 0, waited = 0;
    __device__ __forceinline__ void begin() { t0 = __builtin_readcyclecounter(); }
    __device__ __forceinline__ void rows_start() { t1 = __builtin_readcyclecounter(); }
    __device__ __forceinline__ void rows_end() { t2 = __builtin_readcyclecounter(); }
    __device__ __forceinline__ unsigned long long now() const { return __builtin_readcyclecounter(); }
    __device__ __forceinline__ void waited_since(unsigned long long a) { waited += __builtin_readcyclecounter() - a; }
    __device__ __forceinline__ void record(const PcGeom& g, const RowWalk& walk) const {
        if (g.timeline && (threadIdx.x & 63) == 0) {
            const int64_t wave = ((static_cast<int64_t>(blockIdx.y) * g.n_windows + blockIdx.x) * (BLOCK / 64)) + (threadIdx.x >> 6);
            unsigned long long* rec = g.timeline + wave * 8;
            unsigned int hw;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
            unsigned int xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            rec[0] = t0; rec[1] = t1; rec[2] = t2; rec[3] = __builtin_readcyclecounter(); rec[4] = waited;
            rec[5] = static_cast<unsigned long long>(walk.n_tiles_split); rec[6] = hw; rec[7] = xcc;
        }
    }
#else
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void rows_start() {}
    __device__ __forceinline__ void rows_end() {}
    __device__ __forceinline__ unsigned long long now() const { return 0; }
    __device__ __forceinline__ void waited_since(unsigned long long) {}
    __device__ __forceinline__ void record(const PcGeom&, const RowWalk&) const {}
#endif
};
// the ring's vector-memory waits, their cycles added to the stamps
template <int N, typename TL>
__device__ __forceinline__ void timed_wait_vm(TL& tl) {
    [[maybe_unused]] const unsigned long long a = tl.now();
    wait_vm<N>();
    tl.waited_since(a);
}
template <typename TL>
__device__ __forceinline__ void timed_wait_vm_upto(TL& tl, int n) {
    [[maybe_unused]] const unsigned long long a = tl.now();
    wait_vm_upto(n);
    tl.waited_since(a);
}

// ------------------------------------------------------------------------------------------------
// K4 (window mode): backward
// ------------------------------------------------------------------------------------------------
// WW: row-group windows (make_geom_ww: inner == 1, CPL == V) -- the lane's channels are its own, their constants are
// computed from global memory into registers (no LDS table) and the epilogue sums the row groups in a fixed order.
// DMA > 0: the rows reach the wave through an LDS ring of DMA stages filled by LDS-DMA (glds16): DMA rows of HBM requests
// stay in flight per wave without holding registers.  The arithmetic-heavy 16-bit kernels have no registers to spare for
// more than one row of ordinary loads, and one row in flight per wave does not cover the HBM latency (the dx-only
// kernel, which has the registers, streams the same tensor 20 % faster when all of a workgroup's loads are issued up
// front: profiles/r02_pc_variants_eval.txt).
template <typename IO, int V, int CPL, bool SYM, bool INIT, bool EVAL, int UNROLL, bool NTL, bool NTS, bool PIPE, bool WW = false,
          int DMA = 0, int BLOCK = kBlock>
__global__ __launch_bounds__(BLOCK) void bwd_pc_kernel(const void* __restrict__ grad, const void* __restrict__ x,
                                                        void* __restrict__ dx, PcGeom g,
                                                        const typename IO::arith* __restrict__ scale,
                                                        const typename IO::arith* __restrict__ shift,
                                                        Range<typename IO::arith> r, typename IO::arith grad_scaler,
                                                        double2* __restrict__ partials, PcDirect<typename IO::arith> direct) {
    using T = typename IO::arith;
    using E = typename IO::elem;
    using LC = LaneChannels<T, V, CPL>;
    // OWN: owner windows (make_geom_own) -- a fat workgroup of R row slots over the run of k whole channels, all rows: the
    // LDS slots end up holding FINAL sums, stored straight to d_scale / d_shift (`direct`); no partials, no finalize launch
    constexpr bool OWN = !WW && BLOCK > kBlock;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    TimelineStamps<BLOCK> tl;
    tl.begin();
    static_assert(!WW || (CPL == V && V > 1), "row-group windows: one channel per packet component");
    static_assert(BLOCK == kBlock || DMA > 0, "768/1024-lane workgroups: row-group and owner windows, on the ring only");
    static_assert(!OWN || (!EVAL && V > 1 && CPL <= 2), "owner windows: whole packets of one or two channels, training modes");
    QSlot<T>* table = reinterpret_cast<QSlot<T>*>(smem);
    // fp64 slots of the window's channels: [k_slots] d_scale sums, [k_slots] d_shift sums -- one such set per workgroup, added
    // to with LDS atomics; owner windows (their sums are FINAL) keep one set per WAVE and add the sets in wave order at the
    // end, so that d_scale / d_shift / wide come out the same bits launch after launch
    const uint32_t sum_sets = OWN ? bwd_lds_sum_sets(g) : 1u;
    double* lds_s0 = reinterpret_cast<double*>(smem + static_cast<size_t>(g.k_slots) * sizeof(QSlot<T>));
    double* lds_s = lds_s0 + (OWN ? static_cast<size_t>(threadIdx.x >> 6) * 2u * g.k_slots : 0u);
    double* lds_b = lds_s + g.k_slots;

    // The window's raw scale / shift are requested FIRST: vector-memory operations retire in issue order, so a wait for loads
    // issued behind the first rows' loads would be a wait for those rows (measured, tools/exp_timeline.py: the prologue of a
    // workgroup took 3-7 us, a quarter of its life, most of it that wait).
    //  * ring kernels (fp32 parameters): LDS-DMA dword copies into a staging area behind the fp64 slots -- asm like the
    //    row copies, invisible to the compiler's own s_waitcnt bookkeeping, ordered below with a counted wait;
    //  * register-loop kernels: ordinary loads into registers (the compiler counts its own loads in issue order).
    constexpr bool STAGE = DMA > 0 && !WW && std::is_same<T, float>::value;
    const bool raw_first = !WW && DMA == 0 && g.k_slots <= kRawSlots * kBlock;
    float* raw_stage = reinterpret_cast<float*>(smem + static_cast<size_t>(g.k_slots) * (sizeof(QSlot<T>) + 16 * sum_sets));   // [k_slots] scale, [k_slots] shift
    ChannelRaw<T> raw;
    if constexpr (STAGE) {
        const int64_t c_first = window_first_channel(g);
        const uint32_t stage_lds = __builtin_amdgcn_readfirstlane(lds_offset_of(raw_stage));
        for (int k0 = 0; k0 < g.k_slots; k0 += kBlock) {          // uniform trip count
            const int k = k0 + threadIdx.x;
            if (k < g.k_slots) {                                  // (the other lanes stay out: their dwords would land in a neighbour's slots)
                int64_t c = c_first + k;
                c = c < g.C ? c : g.C - 1;                        // slots past the last channel copy a valid address
                const uint32_t dst = __builtin_amdgcn_readfirstlane(stage_lds + static_cast<uint32_t>(k0 + (threadIdx.x & ~63)) * 4u);
                glds4(scale + c, dst);
                glds4(shift + c, dst + static_cast<uint32_t>(g.k_slots) * 4u);
            }
        }
    } else if (raw_first) {
        raw = load_channel_raw<T>(g.k_slots, window_first_channel(g), g.C, scale, shift);
    }
    int32_t lane_in_group = 0;
    const LaneSite site = WW ? lane_site_ww(g, V, lane_in_group) : (OWN ? lane_site_own(g, V) : lane_site(g, V));
    const RowWalk walk(g, site);
    // A group = UNROLL rows.  load_group never predicates: rows past the lane's last one re-read the last row.
    auto load_group = [&](E (&gb)[UNROLL][V], E (&xb)[UNROLL][V], int64_t i0) {
        const int64_t last = walk.n_rows - 1;
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int64_t e = walk.row(i0 + u < last ? i0 + u : last) * g.L + site.p0;
            load_elems<IO, V, NTL>(grad, e, gb[u]);
            load_elems<IO, V, NTL>(x, e, xb[u]);
        }
    };
    E first_g[UNROLL][V], first_x[UNROLL][V];   // first group in flight before the table build (see K3)
    const bool first_full = DMA > 0 ? false : (PIPE ? walk.n_rows > 0 : walk.n_rows >= UNROLL);
    if (first_full) load_group(first_g, first_x, 0);
    // ---- LDS-DMA ring (DMA > 0): this wave's DMA stages; stage = [64 grad packets][64 x packets] ----
    static_assert(DMA == 0 || V * sizeof(E) == 16, "the LDS-DMA ring moves 16-byte packets");
    const int64_t dma_n = walk.n_tiles_split;                          // the same for every lane of the workgroup
    unsigned char* ring = smem + bwd_lds_front_bytes(g, sizeof(QSlot<T>)) + (threadIdx.x >> 6) * (DMA * kDmaStageBytes);
    const uint32_t ring_lds = DMA > 0 ? __builtin_amdgcn_readfirstlane(lds_offset_of(ring)) : 0u;
    // row i of this lane, clamped into the tensor (rows past the lane's last one and dead lanes re-read valid memory)
    auto dma_issue = [&](int64_t i) {
        int64_t row = walk.row(i);
        row = row < g.outer ? row : g.outer - 1;
        const int64_t e = row * g.L + (site.live ? site.p0 : 0);
        const uint32_t dst = ring_lds + static_cast<uint32_t>(i % (DMA > 0 ? DMA : 1)) * kDmaStageBytes;
        glds16_rt(static_cast<const E*>(grad) + e, dst, g.ring_nt);
        glds16_rt(static_cast<const E*>(x) + e, dst + 64 * 16, g.ring_nt);
    };
    // Row-group windows on the ring, fp32 parameters: the lane's own V scale / shift values are requested BEFORE its rows, as
    // LDS-DMA copies into the last one or two ring stages (16 bytes per lane and copy; the row copies that belong into those
    // stages are issued once the parameters have been read out): see STAGE above for why the order matters.
    constexpr int kParCopies = (V * 4) / 16;                                       // 16-byte copies per parameter: 2 (V = 8), 1 (V = 4)
    constexpr int kParStages = DMA > 0 ? (2 * kParCopies * 1024 + kDmaStageBytes - 1) / kDmaStageBytes : 0;
    constexpr bool WSTAGE_ABLE = WW && DMA > kParStages && std::is_same<T, float>::value && LC::N == V && (V == 8 || V == 4);
    const bool wstage = WSTAGE_ABLE && ((reinterpret_cast<uintptr_t>(scale) | reinterpret_cast<uintptr_t>(shift)) & 15u) == 0;
    if constexpr (DMA > 0) {
        if (wstage) {
            const int64_t c0 = site.live ? site.p0 : 0;
            const uint32_t par_lds = ring_lds + static_cast<uint32_t>(DMA - kParStages) * kDmaStageBytes;
#pragma unroll
            for (int q4 = 0; q4 < kParCopies; ++q4) {
                glds16<false>(scale + c0 + 4 * q4, par_lds + static_cast<uint32_t>(q4) * 1024u);
                glds16<false>(shift + c0 + 4 * q4, par_lds + static_cast<uint32_t>(kParCopies + q4) * 1024u);
            }
            for (int64_t i = 0; i < DMA - kParStages && i < dma_n; ++i) dma_issue(i);
        } else {
            for (int64_t i = 0; i < DMA && i < dma_n; ++i) dma_issue(i);    // in flight before the constants are built
        }
    }
    LC ch;
    if constexpr (WW) {
        // channel p0 + j is component j's own: constants straight into registers (lsq_kernel.h:157-158 + :12)
        ch.split = (CPL == 2) ? 1 : V;     // V == 2 (8-byte elements): LaneChannels' two-channel form, component 1 = channel 1
        if (wstage) {
            if constexpr (WSTAGE_ABLE) {
                // younger than the parameter copies: the copies of the rows issued so far (two each)
                const int64_t rows_out = dma_n < DMA - kParStages ? dma_n : DMA - kParStages;
                wait_vm_upto(static_cast<int>(2 * rows_out));
                const unsigned char* par = ring + (DMA - kParStages) * kDmaStageBytes + (threadIdx.x & 63) * 16;
                float sv[V], bv[V];
#pragma unroll
                for (int q4 = 0; q4 < kParCopies; ++q4) {
                    __builtin_memcpy(&sv[4 * q4], par + q4 * 1024, 16);
                    __builtin_memcpy(&bv[4 * q4], par + (kParCopies + q4) * 1024, 16);
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // the stages are in registers: the rows may land
                for (int64_t i = DMA - kParStages; i < DMA && i < dma_n; ++i) dma_issue(i);
#pragma unroll
                for (int j = 0; j < LC::N; ++j) {
                    ch.q[j] = make_qparams<T>(sanitize_scale_per_channel<T>(sv[j]), bv[j], r);
                    ch.key[j] = j * g.ww_lanes + lane_in_group;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < LC::N; ++j) {
                const int64_t c = site.live ? site.p0 + j : 0;
                ch.q[j] = make_qparams<T>(sanitize_scale_per_channel<T>(scale[c]), shift[c], r);
                ch.key[j] = j * g.ww_lanes + lane_in_group;
            }
        }
    } else {
        if constexpr (STAGE) {
            // younger than this wave's staging copies: the row copies just issued (two per row)
            wait_vm_upto(static_cast<int>(2 * (dma_n < DMA ? dma_n : DMA)));
            for (int k = threadIdx.x; k < g.k_slots; k += kBlock)       // slot k was staged by this very wave
                table[k] = site.c_lo + k < g.C ? make_qslot<T>(raw_stage[k], raw_stage[g.k_slots + k], r) : idle_qslot<T>();
        } else if (raw_first) {
            finish_channel_table<T>(table, g.k_slots, site.c_lo, g.C, raw, r);
        } else {
            build_channel_table<T>(table, g.k_slots, site.c_lo, g.C, scale, shift, r);
        }
        if (!EVAL) {
            for (int k = threadIdx.x; k < static_cast<int>(2u * sum_sets) * g.k_slots; k += static_cast<int>(blockDim.x)) lds_s0[k] = 0.0;
        }
        __syncthreads();
        ch.init(table, site, g);
    }

    // CPL == 1: one accumulator pair.  CPL == 2 / V: one pair per COMPONENT of the packet (a cvt + an add per
    // term in the loop, no selects); CPL == 2 folds them into its two channels after the walk, by `split`.
    // PAIRS (fp32 arithmetic on packets): the row is computed two elements at a time (backward_pair: packed multiplies and
    // adds) and the accumulators are 2-vectors too; CPL == 1 then keeps TWO accumulators (even / odd components), added
    // up after the walk.
    constexpr bool PAIRS = std::is_same<T, float>::value && V >= 2;
    constexpr int kAcc = (LC::N == 1) ? (PAIRS ? 2 : 1) : V;
    double acc_s[kAcc], acc_b[kAcc];
#pragma unroll
    for (int j = 0; j < kAcc; ++j) { acc_s[j] = 0.0; acc_b[j] = 0.0; }
    // PRE32 (16-bit storage on the LDS-DMA ring): the kernel is VALU-bound (profiles/r02_sq_counters_before_cfg5_bf16.txt)
    // and every wave64 VALU instruction costs ~4 cycles whatever its width (profiles/r02_valu_issue_rates.txt), so the
    // reduction is made cheaper per term, within the parity bar of 1e-6 x sum|terms| (profiles/r02_pre32_ab.txt: -6 %):
    //  * the terms of up to kPreRows consecutive rows are first added per component in fp32 (one packed add for two
    //    components), then the pre-sum joins the fp64 accumulator -- a convert and an fp64 add per kPreRows
    //    terms instead of per term; at most kPreRows - 1 fp32 roundings per pre-sum, <= 1.8e-7 of the sum of the |terms|
    //    in the worst case, ~1e-9 typically (range: a pre-sum overflows where four terms of one sign exceed FLT_MAX together --
    //    gradient x level products around 1e38, where the fp32 terms themselves are about to);
    //  * the gradient scaler multiplies the fp64 sums once (backward_elem<.., RAW>) instead of every term.
    constexpr bool PRE32 = DMA > 0 && sizeof(E) < 4 && !EVAL;
    static_assert(!PRE32 || PAIRS, "16-bit storage on the ring moves packets of 8");
    constexpr int kPreRows = 4;
    f2 pre_s[PRE32 ? kAcc / 2 : 1], pre_b[PRE32 ? kAcc / 2 : 1];
#pragma unroll
    for (int j = 0; j < (PRE32 ? kAcc / 2 : 1); ++j) { pre_s[j] = f2{0.0f, 0.0f}; pre_b[j] = f2{0.0f, 0.0f}; }
    // the lane's constants per component pair, in registers for the whole walk
    QPair qp[PAIRS ? V / 2 : 1];
    if constexpr (PAIRS) {
#pragma unroll
        for (int pr = 0; pr < V / 2; ++pr) qp[pr] = ch.pair(pr);
    }

    // CLEAR = false: the caller's next row ASSIGNS the pre-sums (emit_row_at's `first`), so they need no zeroing
    auto flush_pre = [&](auto clear) {
        if constexpr (PRE32) {
#pragma unroll
            for (int a = 0; a < kAcc / 2; ++a) {
                acc_s[2 * a] += static_cast<double>(pre_s[a].x);
                acc_s[2 * a + 1] += static_cast<double>(pre_s[a].y);
                if (decltype(clear)::value) pre_s[a] = f2{0.0f, 0.0f};
                if (!SYM) {
                    acc_b[2 * a] += static_cast<double>(pre_b[a].x);
                    acc_b[2 * a + 1] += static_cast<double>(pre_b[a].y);
                    if (decltype(clear)::value) pre_b[a] = f2{0.0f, 0.0f};
                }
            }
        }
    };

    // one row of this lane: V elements at element offset e.  `first` (compile time): the row opens a pre-sum group, its
    // terms are assigned instead of added (no zeroing, no add).
    auto emit_row_at = [&](int64_t e, const E (&gi)[V], const E (&xi)[V], bool valid, auto first) {
        E out[V];
        if constexpr (PAIRS) {
#pragma unroll
            for (int pr = 0; pr < V / 2; ++pr) {
                const QPair& q = qp[pr];
                const f2 gv = f2{static_cast<T>(gi[2 * pr]), static_cast<T>(gi[2 * pr + 1])};
                const f2 xv = f2{static_cast<T>(xi[2 * pr]), static_cast<T>(xi[2 * pr + 1])};
                f2 dxv;
                if constexpr (EVAL) {
                    dxv = backward_pair_eval<INIT>(gv, xv, q, r);
                } else {
                    f2 ds_t, db_t;
                    dxv = backward_pair<SYM, INIT>(gv, xv, q, r, ds_t, db_t);
                    if (!valid) { ds_t = f2{0.0f, 0.0f}; db_t = f2{0.0f, 0.0f}; }
                    const int a = (LC::N == 1) ? 0 : pr;           // accumulator pair of this component pair (unrolled: a constant)
                    if constexpr (PRE32) {
                        if (decltype(first)::value && (LC::N != 1 || pr == 0)) {
                            pre_s[a] = ds_t;
                            if (!SYM) pre_b[a] = db_t;
                        } else {
                            pre_s[a] += ds_t;
                            if (!SYM) pre_b[a] += db_t;
                        }
                    } else {
                        ds_t *= grad_scaler;                        // :122, every term individually (reference bits)
                        acc_s[2 * a] += static_cast<double>(ds_t.x);
                        acc_s[2 * a + 1] += static_cast<double>(ds_t.y);
                        if (!SYM) {
                            db_t *= grad_scaler;
                            acc_b[2 * a] += static_cast<double>(db_t.x);
                            acc_b[2 * a + 1] += static_cast<double>(db_t.y);
                        }
                    }
                }
                out[2 * pr] = out_elem<IO, INIT>(dxv.x);                   // (init_mode: dX IS the gradient, :112)
                out[2 * pr + 1] = out_elem<IO, INIT>(dxv.y);
            }
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const QParams<T> q = ch.params(j);
                const T gv = static_cast<T>(gi[j]), xv = static_cast<T>(xi[j]);
                if (EVAL) {
                    out[j] = out_elem<IO, INIT>(backward_elem_eval<T, INIT>(gv, xv, q, r));
                } else {
                    T ds_t, db_t;
                    out[j] = out_elem<IO, INIT>(backward_elem<T, SYM, INIT>(gv, xv, q, r, grad_scaler, ds_t, db_t));
                    if (!valid) { ds_t = static_cast<T>(0); db_t = static_cast<T>(0); }
                    const double a = static_cast<double>(ds_t), c = static_cast<double>(db_t);
                    acc_s[j < kAcc ? j : 0] += a;
                    if (!SYM) acc_b[j < kAcc ? j : 0] += c;
                }
            }
        }
        // (owner windows: the stand-in lanes past the last row slot computed a row another lane stores)
        if (valid && (!OWN || site.counts)) store_elems<IO, V, NTS>(dx, e, out);
    };
    auto emit_row = [&](int64_t oo, const E (&gi)[V], const E (&xi)[V], bool valid) {
        emit_row_at(oo * g.L + site.p0, gi, xi, valid, std::false_type{});
    };

    auto emit_full = [&](int64_t i0, const E (&gb)[UNROLL][V], const E (&xb)[UNROLL][V]) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) emit_row(walk.row(i0 + u), gb[u], xb[u], true);
    };
    auto emit_ragged = [&](int64_t i0, const E (&gb)[UNROLL][V], const E (&xb)[UNROLL][V]) {
        const int64_t last = walk.n_rows - 1;
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) emit_row(walk.row(i0 + u < last ? i0 + u : last), gb[u], xb[u], i0 + u <= last);
    };
    int64_t i = 0;
    tl.rows_start();
    if constexpr (DMA > 0) {
        // Row i was requested DMA rows ago.  Younger than its two copies are the copies of rows i+1 .. i+DMA-1 (two each)
        // and the dx stores in between; only the copies are counted (a wave without a valid lane skips its stores), so
        // the wait is never too short and at least 2/3 of the ring stays in flight.
        const int lane = threadIdx.x & 63;
        using V4 = __attribute__((ext_vector_type(4))) unsigned int;
        auto consume = [&](int64_t it, bool refill, auto all_valid) {
            const unsigned char* stage = ring + static_cast<uint32_t>(it % DMA) * kDmaStageBytes + lane * 16;
            const V4 graw = *reinterpret_cast<const V4*>(stage);
            const V4 xraw = *reinterpret_cast<const V4*>(stage + 64 * 16);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // the stage is in registers: it may be refilled
            if (refill) dma_issue(it + DMA);
            E gi[V], xi[V];
            __builtin_memcpy(&gi[0], &graw, 16);
            __builtin_memcpy(&xi[0], &xraw, 16);
            if constexpr (decltype(all_valid)::value) {
                emit_row(walk.row(it), gi, xi, true);
            } else {
                emit_row(walk.row(it) < g.outer ? walk.row(it) : g.outer - 1, gi, xi, it < walk.n_rows);
            }
        };
        // ragged (owner windows only): the last row tile is short -- the lanes of the row slots past its end have one row
        // fewer.  The blocks then stop one tile early (their refills never reach the short tile) and the rows they leave are
        // walked one at a time with the validity and the row clamp of the generic form.
        auto loop = [&](auto all_valid, auto nt, auto ragged) {
            constexpr bool kTailValid = decltype(all_valid)::value && !decltype(ragged)::value;
            [[maybe_unused]] const std::integral_constant<bool, kTailValid> tail_valid{};
            const int64_t dma_blocks = dma_n - (decltype(ragged)::value ? 1 : 0);
            if constexpr (decltype(all_valid)::value) {
                // Steady state in blocks of DMA rows: the ring stage of a row is a compile-time constant (its LDS addresses
                // are instruction offsets), the lane's row addresses advance by one add (every lane walks every row: no
                // clamping), and -- PRE32 -- the first row of a block assigns the pre-sums, which are flushed un-cleared at
                // its end.
                // The wait is EXACT here.  Vector-memory operations retire in issue order and every row of this loop issues
                // the same ones -- two copies (the refill of its stage), then its dx store -- so the operations younger than
                // row i's two copies are: the copies of rows i+1 .. i+DMA-1 and the dx stores of rows i-DMA .. i-1 (row i's
                // copies were issued as the refill of row i-DMA, before that row's store); in the first block the stores of
                // rows 0 .. u-1 only.  (The generic loops below cannot know whether a wave stored, count the copies alone and
                // so wait for one more row and two store acknowledgements than they need.)
                static_assert(!PRE32 || DMA <= kPreRows, "a pre-sum group is at most kPreRows rows");
                const int64_t step_e = walk.step * g.L;
                int64_t e_cur = walk.row(0) * g.L + site.p0;          // i == 0 here
                // Owner windows: the waves of a SIMD take turns at the higher issue priority, block by block.  An owner
                // workgroup has its CU to itself and ends at a barrier, so it is as slow as its slowest wave -- and the
                // arbiter serves the OLDER wave of a SIMD first: waves 0-3 walked their rows in 20.8 us, waves 4-6 (the second
                // wave of their SIMD) in 27.9 us, and the first four then sat 7 us at the barrier
                // (profiles/r04_owner_timeline.txt).  Alternating s_setprio makes the two finish together.
                [[maybe_unused]] const int own_phase = OWN ? __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 8)) & 1 : 0;
                [[maybe_unused]] int own_blk = 0;
                auto block = [&](auto first_block) {
                    if constexpr (OWN) {
                        if (g.own_prio) {
                            if ((own_blk ^ own_phase) & 1) __builtin_amdgcn_s_setprio(2);
                            else __builtin_amdgcn_s_setprio(0);
                            ++own_blk;
                        }
                    }
#pragma unroll
                    for (int u = 0; u < DMA; ++u) {
                        if (decltype(first_block)::value) timed_wait_vm_upto(tl, 2 * (DMA - 1) + u);
                        else timed_wait_vm<2 * (DMA - 1) + DMA>(tl);
                        const unsigned char* stage = ring + u * kDmaStageBytes + lane * 16;
                        const V4 graw = *reinterpret_cast<const V4*>(stage);
                        const V4 xraw = *reinterpret_cast<const V4*>(stage + 64 * 16);
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the stage is in registers: refill it
                        const int64_t e_next = e_cur + DMA * step_e;
                        glds16<decltype(nt)::value>(static_cast<const E*>(grad) + e_next, ring_lds + u * kDmaStageBytes);
                        glds16<decltype(nt)::value>(static_cast<const E*>(x) + e_next, ring_lds + u * kDmaStageBytes + 64 * 16);
                        E gi[V], xi[V];
                        __builtin_memcpy(&gi[0], &graw, 16);
                        __builtin_memcpy(&xi[0], &xraw, 16);
                        if (u == 0) emit_row_at(e_cur, gi, xi, true, std::true_type{});
                        else emit_row_at(e_cur, gi, xi, true, std::false_type{});
                        e_cur += step_e;
                    }
                    flush_pre(std::false_type{});
                    i += DMA;
                };
                static_assert(2 * (DMA - 1) + DMA <= 15, "wait_vm_upto covers counts up to 15");
                if (i + 2 * DMA <= dma_blocks) block(std::true_type{});
                while (i + 2 * DMA <= dma_blocks) block(std::false_type{});
                if constexpr (OWN) __builtin_amdgcn_s_setprio(0);
                if constexpr (PRE32) {
#pragma unroll
                    for (int j = 0; j < kAcc / 2; ++j) { pre_s[j] = f2{0.0f, 0.0f}; pre_b[j] = f2{0.0f, 0.0f}; }
                }
            }
            // the rows the blocks left over (and every row of a wave with dead lanes or a ragged last tile): one at a time,
            // ring stage and validity at run time.  `stores`: dx stores younger than row i's copies -- known only when every
            // row of the wave stores (see above); otherwise they are left out of the count (the wait is then longer).
            auto stores = [&](int64_t row) { return kTailValid ? static_cast<int>(row < DMA ? row : DMA) : 0; };
            for (; i + DMA < dma_n; ++i) {           // the ring is full, one refill per row
                timed_wait_vm_upto(tl, 2 * (DMA - 1) + stores(i));
                consume(i, true, tail_valid);
                if (PRE32 && (i & (kPreRows - 1)) == kPreRows - 1) flush_pre(std::true_type{});
            }
            for (; i < dma_n; ++i) {                 // the last DMA rows: nothing left to request
                timed_wait_vm_upto(tl, static_cast<int>(2 * (dma_n - 1 - i)) + stores(i));
                consume(i, false, tail_valid);
                if (PRE32 && (i & (kPreRows - 1)) == kPreRows - 1) flush_pre(std::true_type{});
            }
            flush_pre(std::true_type{});
            if constexpr (PRE32) {           // the gradient scaler, once per sum
#pragma unroll
                for (int j = 0; j < kAcc; ++j) {
                    acc_s[j] *= static_cast<double>(grad_scaler);
                    acc_b[j] *= static_cast<double>(grad_scaler);
                }
            }
        };
        // every lane of this wave walks all dma_n rows (no dead lane, no ragged last tile): no per-row validity selects
        if (__builtin_amdgcn_readfirstlane(__all(site.live && walk.n_rows == dma_n) ? 1 : 0)) {
            if (g.ring_nt) loop(std::true_type{}, std::true_type{}, std::false_type{});
            else loop(std::true_type{}, std::false_type{}, std::false_type{});
        } else if (OWN && __builtin_amdgcn_readfirstlane(__all(site.live && walk.n_rows + 1 >= dma_n) ? 1 : 0)) {
            if constexpr (OWN) {       // some of this wave's row slots miss the last tile only
                if (g.ring_nt) loop(std::true_type{}, std::true_type{}, std::true_type{});
                else loop(std::true_type{}, std::false_type{}, std::true_type{});
            }
        } else {
            loop(std::false_type{}, std::false_type{}, std::false_type{});
        }
    } else if (PIPE) {
        // Software pipeline, two register buffers: the loads of group k+1 are issued BEFORE the arithmetic of
        // group k, so every wave keeps HBM requests in flight while it computes (for 16-bit storage the VALU time
        // of a group is about its HBM time: without this the two only overlap across waves).
        if (first_full) {
            E other_g[UNROLL][V], other_x[UNROLL][V];
            // sched_barrier: the machine scheduler otherwise sinks each load group below the arithmetic that
            // precedes its first use (to save registers), which undoes the pipeline
            while (i + 2 * UNROLL <= walk.n_rows) {          // groups i and i + UNROLL are both full
                load_group(other_g, other_x, i + UNROLL);
                __builtin_amdgcn_sched_barrier(0);
                emit_full(i, first_g, first_x);
                __builtin_amdgcn_sched_barrier(0);
                load_group(first_g, first_x, i + 2 * UNROLL);   // may be ragged or past the end: clamped re-reads
                __builtin_amdgcn_sched_barrier(0);
                emit_full(i + UNROLL, other_g, other_x);
                __builtin_amdgcn_sched_barrier(0);
                i += 2 * UNROLL;
            }
            if (i + UNROLL <= walk.n_rows) {                  // `first` holds a full group
                load_group(other_g, other_x, i + UNROLL);
                __builtin_amdgcn_sched_barrier(0);
                emit_full(i, first_g, first_x);
                i += UNROLL;
                if (i < walk.n_rows) emit_ragged(i, other_g, other_x);
            } else if (i < walk.n_rows) {
                emit_ragged(i, first_g, first_x);
            }
        }
    } else {
        // plain loop: full groups of UNROLL, then one group of UNROLL/2, ..., one single row -- no padded slots
        auto group = [&](int64_t i0, auto width) {
            constexpr int H = decltype(width)::value;
            E gi[H][V], xi[H][V];
#pragma unroll
            for (int u = 0; u < H; ++u) {
                const int64_t e = walk.row(i0 + u) * g.L + site.p0;
                load_elems<IO, V, NTL>(grad, e, gi[u]);
                load_elems<IO, V, NTL>(x, e, xi[u]);
            }
#pragma unroll
            for (int u = 0; u < H; ++u) emit_row(walk.row(i0 + u), gi[u], xi[u], true);
        };
        if (first_full) {
            emit_full(0, first_g, first_x);
            i = UNROLL;
        }
        for (; i + UNROLL <= walk.n_rows; i += UNROLL) group(i, std::integral_constant<int, UNROLL>{});
        if constexpr (UNROLL >= 8) if (i + 4 <= walk.n_rows) { group(i, std::integral_constant<int, 4>{}); i += 4; }
        if constexpr (UNROLL >= 4) if (i + 2 <= walk.n_rows) { group(i, std::integral_constant<int, 2>{}); i += 2; }
        if constexpr (UNROLL >= 2) if (i < walk.n_rows) group(i, std::integral_constant<int, 1>{});
    }
    tl.rows_end();
    if (EVAL) { tl.record(g, walk); return; }
    if constexpr (PAIRS && LC::N == 1) {     // one channel per lane: even + odd components
        acc_s[0] += acc_s[1];
        acc_b[0] += acc_b[1];
    }

    if constexpr (WW) {
        // R row groups, R interleaved row sets of the same w x V channels.  Every group parks its sums in LDS
        // ([group][component][lane]: a lane-contiguous 16 bytes each, conflict-free); then EVERY thread takes part in adding them
        // up: slot s = component * w + lane is summed over the groups in group order by one thread (k_slots >= workgroup size:
        // a thread takes several slots) or -- narrow windows, more threads than slots -- by P = threads / k_slots threads that
        // each take the groups part, part + P, ... and whose P results are then added in order.  (Round 4 had row group 0's
        // lanes add all R - 1 parked rows themselves: [64,197,768] bf16, 96 lanes x 56 dependent LDS reads while 672 lanes
        // idled, 2-3 us of a 14 us workgroup.)  The workgroup's partial row is stored slot-major (contiguous per component).
        double2* comb = reinterpret_cast<double2*>(smem);
        const int w = g.ww_lanes, rg = site.row_in_tile;
        const int k_slots = g.k_slots, nthr = static_cast<int>(blockDim.x), t = static_cast<int>(threadIdx.x);
        if constexpr (DMA > 0) __syncthreads();     // the combine buffer takes the ring's place: every wave is done reading
        if (rg < g.R) {
#pragma unroll
            for (int j = 0; j < V; ++j) comb[(rg * V + j) * w + lane_in_group] = make_double2(acc_s[j], acc_b[j]);
        }
        __syncthreads();
        const int64_t block_linear = static_cast<int64_t>(blockIdx.y) * g.n_windows + blockIdx.x;
        double2* out = partials + block_linear * k_slots;
        auto publish = [&](int slot, double ts, double tb) { out[slot] = make_double2(ts, tb); };
        if (k_slots >= nthr) {
            for (int slot = t; slot < k_slots; slot += nthr) {
                double ts = comb[slot].x, tb = comb[slot].y;
                for (int o = 1; o < g.R; ++o) {
                    const double2 v = comb[o * k_slots + slot];
                    ts += v.x;
                    tb += v.y;
                }
                publish(slot, ts, tb);
            }
        } else {
            const int P = nthr / k_slots, slot = t % k_slots, part = t / k_slots;
            double2* comb2 = comb + static_cast<size_t>(g.R) * k_slots;
            if (part < P && part < g.R) {
                double ts = comb[part * k_slots + slot].x, tb = comb[part * k_slots + slot].y;
                for (int o = part + P; o < g.R; o += P) {
                    const double2 v = comb[o * k_slots + slot];
                    ts += v.x;
                    tb += v.y;
                }
                comb2[part * k_slots + slot] = make_double2(ts, tb);
            }
            __syncthreads();
            if (t < k_slots) {
                const int parts = P < g.R ? P : g.R;
                double ts = comb2[t].x, tb = comb2[t].y;
                for (int q = 1; q < parts; ++q) {
                    ts += comb2[q * k_slots + t].x;
                    tb += comb2[q * k_slots + t].y;
                }
                publish(t, ts, tb);
            }
        }
        tl.record(g, walk);
        return;
    }

    // The window's slots take the waves' run totals with LDS fp64 atomics.  One slot set per workgroup (256-lane windows):
    // the adds are made in WAVE ORDER -- wave w adds between barrier w and barrier w + 1; inside a wave the order is the
    // program's and the LDS unit's lane order -- so the partial row a workgroup publishes, and with it d_scale / d_shift / the
    // un-rounded sums the sharded path all-reduces, are the same bits launch after launch (until round 6 the four waves added in
    // arrival order: two launches could differ by an fp64 rounding).  The shuffles above ran in all waves at once; what is
    // serialised is one or two LDS atomics per lane.  Owner windows keep a slot set per wave (added in wave order below).
    const int my_wave = static_cast<int>(threadIdx.x >> 6);
    auto in_wave_order = [&](auto&& adds_fn) {
        if constexpr (OWN) {
            adds_fn();
            __syncthreads();
        } else {
            for (int w = 0; w < BLOCK / 64; ++w) {
                if (my_wave == w) adds_fn();
                __syncthreads();
            }
        }
    };
    if (CPL == 2) {
        // components below `split` -> first channel, the rest -> second channel (two disjoint sums: a
        // non-finite term of one channel never reaches the other).  The second channel of lane i is
        // the FIRST channel of lane i+1 (their positions are contiguous and inner >= V), so its sums
        // travel one lane up and join that lane's run: ONE segmented reduction instead of two.  Only
        // the last lane of a wave / of a row has no neighbour and adds its second channel itself.
        const int lane = threadIdx.x & 63;
        const bool has_hi = site.counts && ch.split < V;
        double lo_s = 0.0, lo_b = 0.0, hi_s = 0.0, hi_b = 0.0;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const bool hi = j >= ch.split;
            lo_s += hi ? 0.0 : acc_s[j];
            hi_s += hi ? acc_s[j] : 0.0;
            lo_b += hi ? 0.0 : acc_b[j];
            hi_b += hi ? acc_b[j] : 0.0;
        }
        const int key_hi = has_hi ? ch.key[LC::N - 1] : -1;
        const int next_key0 = __shfl_down(site.counts ? ch.key[0] : -2, 1, 64);
        const bool handoff = has_hi && lane < 63 && next_key0 == key_hi;
        const double give_s = handoff ? hi_s : 0.0, give_b = handoff ? hi_b : 0.0;
        const double got_s = shfl_up_f64(give_s, 1), got_b = shfl_up_f64(give_b, 1);
        if (lane > 0) { lo_s += got_s; lo_b += got_b; }
        const int key_lo = site.counts ? ch.key[0] : -1;
        const bool adds_lo = segmented_wave_reduce<SYM>(key_lo, lo_s, lo_b);
        in_wave_order([&]() {
            segmented_wave_commit<SYM>(has_hi && !handoff, key_hi, hi_s, hi_b, lds_s, lds_b);
            segmented_wave_commit<SYM>(adds_lo, key_lo, lo_s, lo_b, lds_s, lds_b);
        });
    } else {
        // lanes -> window slots.  Dead lanes carry key -1 (never written).
        bool adds[LC::N];
#pragma unroll
        for (int j = 0; j < LC::N; ++j) adds[j] = segmented_wave_reduce<SYM>(site.counts ? ch.key[j] : -1, acc_s[j], acc_b[j]);
        in_wave_order([&]() {
#pragma unroll
            for (int j = 0; j < LC::N; ++j) segmented_wave_commit<SYM>(adds[j], ch.key[j], acc_s[j], acc_b[j], lds_s, lds_b);
        });
    }
    if constexpr (OWN) {
        // every element of these channels went through this workgroup: the slots are the channels' totals
        for (int k = threadIdx.x; k < g.k_slots; k += static_cast<int>(blockDim.x)) {
            const int64_t c = site.c_lo + k;
            if (c < g.C) {
                double ts = 0.0, tb = 0.0;
                for (uint32_t w = 0; w < sum_sets; ++w) {          // the waves' sums, in wave order
                    ts += lds_s0[(2u * w) * g.k_slots + k];
                    tb += lds_s0[(2u * w + 1u) * g.k_slots + k];
                }
                if (direct.sym) tb = 0.0 + static_cast<double>(direct.sym_term);
                direct.ds[c] = static_cast<T>(ts);
                direct.db[c] = static_cast<T>(tb);
                if (direct.wide) {
                    direct.wide[c] = ts;
                    direct.wide[g.C + c] = tb;
                }
            }
        }
        tl.record(g, walk);
        return;
    }
    const int64_t block_linear = static_cast<int64_t>(blockIdx.y) * g.n_windows + blockIdx.x;
    double2* out = partials + block_linear * g.k_slots;
    for (int k = threadIdx.x; k < g.k_slots; k += kBlock) out[k] = make_double2(lds_s[k], lds_b[k]);
    tl.record(g, walk);
}

}  // namespace lsq
