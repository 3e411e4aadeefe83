// lsq_grp_bwd_body.inc -- the statements of the group-wise fused backward (lsq_grp_body.hpp explains why a fragment).
// In scope: IO, SYM, INIT, EVAL, MODE; grad, x, dx, ds, db, n, G, pg_shift, per_group, groups_per_wave, scale, shift, r, gs,
// sym_term (as bwd_grp_kernel's parameters); LSQ_GRP_BLOCK, LSQ_GRP_GRID as in lsq_grp_fwd_body.inc.  It is the last
// statement of its kernel (it may return).
{
    using T = typename IO::arith;
    using Acc = GrpTerms<T, SYM, INIT, EVAL>;
    constexpr int VEC = IO::VEC;
    constexpr bool PACKET = MODE != kScanElem;
    const int lane = threadIdx.x & 63;
    const int64_t wave = LSQ_GRP_BLOCK * (kBlock / 64) + (threadIdx.x >> 6);
    const int64_t n_waves = LSQ_GRP_GRID * (kBlock / 64);
    const int64_t n_items = PACKET ? n / VEC : n;
    const int64_t gi = PACKET ? G / VEC : G;      // items per group

    // one item (packet or element) -> dx, and its terms into (s, b)
    auto item = [&](const Packet<IO>& gp, const Packet<IO>& xp, int64_t it, int64_t grp, double& s, double& b) {
        const QParams<T> q = group_qparams<T>(scale, shift, grp, r);
        if constexpr (PACKET) {
            Packet<IO> out;
#pragma unroll
            for (int j = 0; j < VEC; ++j)
                out.v[j] = out_elem<IO, INIT>(Acc::step(static_cast<T>(gp.v[j]), static_cast<T>(xp.v[j]), q, r, gs, s, b));
            store_packet_nt<IO>(dx, it * VEC, out);
        } else {
            store_out<IO, INIT>(dx, it, Acc::step(static_cast<T>(gp.v[0]), static_cast<T>(xp.v[0]), q, r, gs, s, b));
        }
    };
    auto load = [&](const void* base, int64_t it) {
        Packet<IO> pk;
        if constexpr (PACKET) {
            pk = load_packet_nt<IO>(base, it * VEC);
        } else {
            pk.v[0] = static_cast<const typename IO::elem*>(base)[it];
        }
        return pk;
    };

    if constexpr (MODE == kP2) {
        // units of max(64 * UNROLL, PG) packets: whole groups, walked 64 * UNROLL packets at a time
        constexpr int64_t kStep = 64 * kGrpUnroll;
        const int64_t pg = gi;
        const int64_t unit = pg > kStep ? pg : kStep;
        const int64_t n_units = (n_items + unit - 1) / unit;
        double acc_s = 0.0, acc_b = 0.0;          // PG > 64: the lane's share of the current group
        for (int64_t u0 = wave; u0 < n_units; u0 += n_waves) {
            const int64_t u_end = (u0 + 1) * unit < n_items ? (u0 + 1) * unit : n_items;
            for (int64_t base = u0 * unit; base < u_end; base += kStep) {
                const bool whole = base + kStep <= u_end;
                Packet<IO> gp[kGrpUnroll], xp[kGrpUnroll];
#pragma unroll
                for (int k = 0; k < kGrpUnroll; ++k) {
                    const int64_t it = base + k * 64 + lane;
                    if (whole || it < u_end) {
                        gp[k] = load(grad, it);
                        xp[k] = load(x, it);
                    }
                }
#pragma unroll
                for (int k = 0; k < kGrpUnroll; ++k) {
                    const int64_t pass = base + k * 64;            // first packet of this pass (wave-uniform)
                    if (!whole && pass >= u_end) break;            // (a partial unit ends on a group boundary)
                    const int64_t it = pass + lane;
                    const bool live = whole || it < u_end;
                    const int64_t grp = it >> pg_shift;            // (P2: PG is a power of two)
                    double s = 0.0, b = 0.0;
                    if (live) item(gp[k], xp[k], it, grp, s, b);
                    if constexpr (EVAL) {
                        if (live && (it & (pg - 1)) == 0) store_group<T, SYM, EVAL>(ds, db, grp, 0.0, 0.0, sym_term);
                    } else if (pg <= 64) {
                        for (int d = 1; d < pg; d <<= 1) {             // butterfly inside each group's PG lanes
                            s += shfl_xor_f64(s, d);
                            if (!SYM) b += shfl_xor_f64(b, d);
                        }
                        if (live && (lane & (pg - 1)) == 0) store_group<T, SYM, EVAL>(ds, db, grp, s, b, sym_term);
                    } else {
                        acc_s += s;
                        acc_b += b;
                        if (((pass + 64) & (pg - 1)) == 0) {           // the group's last pass
                            acc_s = wave_sum(acc_s);
                            if (!SYM) acc_b = wave_sum(acc_b);
                            if (lane == 0) store_group<T, SYM, EVAL>(ds, db, grp, acc_s, acc_b, sym_term);
                            acc_s = 0.0;
                            acc_b = 0.0;
                        }
                    }
                }
            }
        }
    } else {
        // SCAN: this wave's groups [g_lo, g_hi), items [g_lo * gi, g_hi * gi), 64 items per pass
        const int64_t n_groups = n / G;
        const int64_t g_lo = wave * groups_per_wave;
        if (g_lo >= n_groups) return;
        const int64_t g_hi = g_lo + groups_per_wave < n_groups ? g_lo + groups_per_wave : n_groups;
        const int64_t i_end = g_hi * gi;
        int64_t g0 = g_lo, r0 = 0;                // group and offset in it of the pass's first item (wave-uniform)
        double carry_s = 0.0, carry_b = 0.0;      // sums of the pass's first group from earlier passes
        for (int64_t base = g_lo * gi; base < i_end; base += 64 * kGrpUnroll) {
            Packet<IO> gp[kGrpUnroll], xp[kGrpUnroll];
#pragma unroll
            for (int k = 0; k < kGrpUnroll; ++k) {
                const int64_t it = base + k * 64 + lane;
                if (it < i_end) {
                    gp[k] = load(grad, it);
                    xp[k] = load(x, it);
                }
            }
#pragma unroll
            for (int k = 0; k < kGrpUnroll; ++k) {
                const int64_t it = base + k * 64 + lane;
                if (base + k * 64 >= i_end) break;
                const bool live = it < i_end;
                // this lane's group and offset: r0 + lane, reduced once (gi >= 64) or by a division (gi < 64)
                int64_t rl, gl;
                const int64_t t = r0 + lane;
                if (gi >= 64) {
                    const bool over = t >= gi;
                    rl = over ? t - gi : t;
                    gl = g0 + (over ? 1 : 0);
                } else {
                    const int64_t qd = per_group.div(t);
                    rl = t - qd * gi;
                    gl = g0 + qd;
                }
                double s = 0.0, b = 0.0;
                if (live) item(gp[k], xp[k], it, gl, s, b);
                const bool last = live && rl == gi - 1;
                if constexpr (EVAL) {
                    if (last) store_group<T, SYM, EVAL>(ds, db, gl, 0.0, 0.0, sym_term);
                } else {
                    // segmented inclusive scan; a head (an item that starts a group, or lane 0) stops the sums from below
                    int head = (rl == 0 || lane == 0) ? 1 : 0;
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) {
                        const double os = shfl_up_f64(s, d);
                        const double ob = SYM ? 0.0 : shfl_up_f64(b, d);
                        const int oh = __shfl_up(head, d, 64);
                        if (lane >= d && !head) {
                            s = os + s;
                            if (!SYM) b = ob + b;
                        }
                        if (lane >= d) head |= oh;
                    }
                    if (lane < gi - r0) {                          // the pass's first group: add what earlier passes summed
                        s = carry_s + s;
                        if (!SYM) b = carry_b + b;
                    }
                    if (last) store_group<T, SYM, EVAL>(ds, db, gl, s, b, sym_term);
                    // lane 63's group continues into the next pass unless it ends here
                    const double ts = bcast_f64(s, 63), tb = SYM ? 0.0 : bcast_f64(b, 63);
                    const bool ends = __shfl(last ? 1 : 0, 63, 64) != 0;
                    carry_s = ends ? 0.0 : ts;
                    carry_b = ends ? 0.0 : tb;
                }
                const int64_t t64 = r0 + 64;
                if (gi >= 64) {
                    const bool over = t64 >= gi;
                    r0 = over ? t64 - gi : t64;
                    g0 += over ? 1 : 0;
                } else {
                    const int64_t qd = per_group.div(t64);
                    r0 = t64 - qd * gi;
                    g0 += qd;
                }
            }
        }
    }
}
