// lsq_attn_paged_keys.hpp -- WHERE A KEY'S ROW LIES in a paged KV cache on 8-bit levels, ONCE: the PagedKeys policy of
// ../attn_decode_split_w8/lsq_attn_split_core.hpp and the host checks of the pages, for liblsq_hip_attn_paged_w8.so (the decode:
// R <= 16 rows, one tile) and liblsq_hip_attn_chunk_w8.so (the prompt chunk: row tiles).  A key's row is not T + j ld but lies in
// the page the block table names,
//     row(b, hkv, j) = pool + clamp(block_table[b, j >> log2 ps], 0, Np - 1) * page stride + hkv * head stride + (j & (ps - 1)) * slot stride,
// ps a power of two >= 16, so that an entry serves aligned runs of at least 16 keys as the core asks; READS CLAMP, and the core asks
// only for entries of keys below nmax, so table entries at logical pages >= ceil(nmax / ps) and pool bytes at keys >= nmax are
// never read.
//
// Include after lsq_companion_abi.hpp, ../attn_w8/lsq_attn_decode_checks.hpp and the core.
#pragma once
#include "../attn_decode_split_w8/lsq_attn_split_core.hpp"
#include "../../../include/lsq_hip_attn_paged_w8.h"

namespace lsq {

static_assert(LSQ_ATTN_PAGED_W8_MIN_PAGE % 16 == 0, "a sub-tile of launch 1 lies in one page");

// keys in the pages of a pool; the strides of T are (page, head, slot)
struct PagedKeys {          // kernel argument
    const int32_t* bt;      // the block table
    int64_t bt_ld;          // elements between its rows
    int Np, lps, psm;       // pages of a pool; log2 ps; ps - 1
    struct Rows {
        typedef int Entry;                      // the page
        const uint8_t* __restrict__ base;       // the kv head's slots of page 0
        const int32_t* __restrict__ btrow;
        int64_t sp, ld;
        int Np, lps, psm;
        // READS CLAMP (j < Tk = Mp ps, so j >> lps < Mp)
        __device__ __forceinline__ Entry entry(int j) const { return min(max(btrow[j >> lps], 0), Np - 1); }
        __device__ __forceinline__ const uint8_t* row(Entry e, int j) const {
            return base + static_cast<int64_t>(e) * sp + static_cast<int64_t>(j & psm) * ld;
        }
    };
    __device__ __forceinline__ Rows rows(const uint8_t* __restrict__ T, const lsq_attn_w8_strides& s, int64_t b, int64_t hkv) const {
        return Rows{T + hkv * s.s1, bt + b * bt_ld, s.s0, s.ld, Np, lps, psm};
    }
};

inline PagedKeys paged_keys(const lsq_attn_paged_w8_pages& pg, const void* block_table) {
    int lps = 0;
    while ((int64_t{1} << lps) < pg.ps) ++lps;
    return PagedKeys{static_cast<const int32_t*>(block_table), pg.bt_ld, static_cast<int>(pg.Np), lps, static_cast<int>(pg.ps - 1)};
}

// ps a power of two >= 16 (Mp ps <= 65536: the API's own limit)
inline bool paged_page_served(const lsq_attn_paged_w8_pages& pg) { return pg.ps >= LSQ_ATTN_PAGED_W8_MIN_PAGE && (pg.ps & (pg.ps - 1)) == 0; }

}  // namespace lsq

namespace {

constexpr int64_t kMaxPages = (int64_t{1} << 31) - 1;       // an entry is an int32

int check_pages(const char* what, const lsq_attn_paged_w8_pages* p) {
    if (!p) return fail(LSQ_EINVAL, "%s: NULL pages", what);
    if (p->ps < 1 || p->Mp < 1 || p->Np < 1)
        return fail(LSQ_EINVAL, "%s: [Np, ps, Mp] = [%lld, %lld, %lld], every extent must be at least 1", what, static_cast<ll>(p->Np),
                    static_cast<ll>(p->ps), static_cast<ll>(p->Mp));
    if (p->Np > kMaxPages) return fail(LSQ_EINVAL, "%s: Np = %lld pages are beyond 2^31 - 1", what, static_cast<ll>(p->Np));
    if (p->bt_ld < p->Mp)
        return fail(LSQ_EINVAL, "%s: the block table's row stride bt_ld = %lld is smaller than its row of Mp = %lld", what,
                    static_cast<ll>(p->bt_ld), static_cast<ll>(p->Mp));
    return LSQ_OK;
}

// the pages, then the checks of a decode geometry with k and v read as pools
int check_paged_geom(const char* what, const lsq_attn_decode_w8_geom* g, const lsq_attn_paged_w8_pages* p) {
    if (!g) return fail(LSQ_EINVAL, "%s: NULL geometry", what);
    if (int rc = check_pages(what, p)) return rc;
    if (p->ps > LSQ_ATTN_PAGED_W8_MAX_TK || p->Mp > LSQ_ATTN_PAGED_W8_MAX_TK || p->Mp * p->ps > LSQ_ATTN_PAGED_W8_MAX_TK)
        return fail(LSQ_EINVAL, "%s: Mp ps = %lld x %lld keys, at most %d are served (the raw sums stay in 32 bits)", what,
                    static_cast<ll>(p->Mp), static_cast<ll>(p->ps), LSQ_ATTN_PAGED_W8_MAX_TK);
    const DecodePools pools{p->Np, p->ps, p->Mp};
    return check_decode_geom(what, g, &pools);
}

}  // namespace
