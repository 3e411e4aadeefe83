// lsq_grp_fwd_body.inc -- the statements of the group-wise forward (lsq_grp_body.hpp explains why a fragment).
// In scope: IO, INIT, LEVELS, PACKET; x, y, levels, level_bias, aux_kind, n, G, pg_shift, per_group, scale, shift, r
// (as fwd_grp_kernel's parameters); LSQ_GRP_BLOCK, LSQ_GRP_GRID: this workgroup's index among the workgroups that walk
// the tensor, and their number (int64_t).  It is the last statement of its kernel (it may return).
{
    // per_group: division by the elements (element form) resp. packets (packet form) of one group
    using T = typename IO::arith;
    constexpr int VEC = IO::VEC;
    const T bias = static_cast<T>(level_bias);
    if constexpr (!PACKET) {
        for (int64_t i = LSQ_GRP_BLOCK * kBlock + threadIdx.x; i < n; i += LSQ_GRP_GRID * kBlock) {
            const QParams<T> q = group_qparams<T>(scale, shift, per_group.div(i), r);
            const T xv = IO::load1(x, i);
            const T c = clamped<T>(xv, q, r);
            if (!LEVELS || y != nullptr) store_out<IO, INIT>(y, i, INIT ? xv : dequant<T>(rne(c), q));
            if (LEVELS) levels[i] = aux_byte<T>(c, r, bias, aux_kind);
        }
        return;
    } else {
        const int64_t n_packets = n / VEC;          // exact: n % G == 0 and G % VEC == 0
        constexpr int64_t kTile = static_cast<int64_t>(kBlock) * kGrpUnroll;
        const int64_t n_full = n_packets / kTile;
        auto emit = [&](const Packet<IO>& in, int64_t p) {
            const QParams<T> q = group_qparams<T>(scale, shift, pg_shift >= 0 ? (p >> pg_shift) : per_group.div(p), r);
            Packet<IO> out;
            LevelPack<VEC> lv;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const T xv = static_cast<T>(in.v[j]);
                const T c = clamped<T>(xv, q, r);
                out.v[j] = out_elem<IO, INIT>(INIT ? xv : dequant<T>(rne(c), q));   // lsq_kernel.h:13
                if (LEVELS) lv.b[j] = aux_byte<T>(c, r, bias, aux_kind);
            }
            if (!LEVELS || y != nullptr) store_packet_nt<IO>(y, p * VEC, out);
            if (LEVELS) lv.store(levels + p * VEC);
        };
        for (int64_t tile = LSQ_GRP_BLOCK; tile < n_full; tile += LSQ_GRP_GRID) {
            const int64_t p0 = tile * kTile + threadIdx.x;
            Packet<IO> in[kGrpUnroll];
#pragma unroll
            for (int u = 0; u < kGrpUnroll; ++u) in[u] = load_packet_nt<IO>(x, (p0 + static_cast<int64_t>(u) * kBlock) * VEC);
#pragma unroll
            for (int u = 0; u < kGrpUnroll; ++u) emit(in[u], p0 + static_cast<int64_t>(u) * kBlock);
        }
        if (LSQ_GRP_BLOCK == n_full % LSQ_GRP_GRID) {     // the one partial tile
            for (int64_t p = n_full * kTile + threadIdx.x; p < n_packets; p += kBlock) emit(load_packet<IO>(x, p * VEC), p);
        }
    }
}
