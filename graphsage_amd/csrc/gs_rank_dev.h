// The sweep that gs_rank.hip (score-and-count) and gs_topk.hip (score-and-select) share: one set of device helpers for the
// 128 x 128 fp32-MFMA tile loop over (candidate slice, query tile) -- operand loads and stores, the compute stage, the
// exclusion-word builder -- and the host's slice plan.  Both kernels run THESE functions, so a (query row, candidate row) pair
// goes through the same k-ordered fmaf chain in either: a score selected by gs_topk_select is bit-equal to the t that
// gs_rank_count returns for that pair.  The layout, the pipeline and the reasons are in the header comment of gs_rank.hip.
#pragma once
#include "gs_common.h"

#define RK_BM 128
#define RK_BN 128
#define RK_BK 32
#define RK_KP 36                 // padded k stride (conflict-free ds_read_b128)
#define RK_STAGE_FLOATS ((RK_BM + RK_BN) * RK_KP)
#define RK_WG_TARGET 2048        // workgroups aimed at when the candidates are cut into slices
#define RK_MIN_TILES 4           // candidate tiles per slice, at least (the count kernel's t tile is a fifth)
#define RK_MAX_TILES 16384       // ... and at most (the count kernel's packed 16-bit per-lane counters, unsigned)

// the word of 32 exclusion bits whose first `lim` columns exist (lim <= 0: none, lim >= 32: all)
__device__ __forceinline__ uint32_t rank_tail_word(const int lim) {
    return lim <= 0 ? 0xffffffffu : (lim < 32 ? (0xffffffffu << lim) : 0u);
}

// The 128-bit exclusion word of one query row for the candidate tile [n0, n0 + BN): columns at or beyond n_cand, dd and ss
// (-1: none) and the entries of the row's sorted filter run [cur, cend) that fall into the tile; cur only moves forward.
__device__ __forceinline__ uint4 rank_excl_words(const int64_t n0, const int64_t n_cand, const int64_t dd, const int64_t ss,
                                                 const int32_t* __restrict__ f_col, int64_t& cur, const int64_t cend) {
    uint32_t w0 = 0u, w1 = 0u, w2 = 0u, w3 = 0u;         // four named words: an indexed array would live in scratch
    const int64_t hi = n0 + RK_BN;
    if (n_cand < hi) {
        const int lim = (int)(n_cand - n0);              // 1 .. BN-1 columns exist
        w0 = rank_tail_word(lim); w1 = rank_tail_word(lim - 32);
        w2 = rank_tail_word(lim - 64); w3 = rank_tail_word(lim - 96);
    }
    auto set_bit = [&](const int cidx) {
        const uint32_t b = 1u << (cidx & 31);
        const int j = cidx >> 5;
        w0 |= j == 0 ? b : 0u; w1 |= j == 1 ? b : 0u;
        w2 |= j == 2 ? b : 0u; w3 |= j == 3 ? b : 0u;
    };
    if (dd >= n0 && dd < hi) set_bit((int)(dd - n0));
    if (ss >= n0 && ss < hi) set_bit((int)(ss - n0));
    while (cur < cend) {
        const int64_t cc = f_col[cur];
        if (cc >= hi) break;
        if (cc >= n0) set_bit((int)(cc - n0));
        ++cur;
    }
    return make_uint4(w0, w1, w2, w3);
}

// [r0, r1) of the filter row of ss, clamped into the column array, and the first entry >= `first` (binary search)
__device__ __forceinline__ void rank_filter_cursor(const int64_t* __restrict__ f_rowptr, const int32_t* __restrict__ f_col,
                                                   const int64_t f_nnz, const int32_t ss, const int64_t first, int64_t& cur,
                                                   int64_t& cend) {
    int64_t r0 = f_rowptr[ss], r1 = f_rowptr[ss + 1];
    r0 = min(max(r0, (int64_t)0), f_nnz);
    r1 = min(max(r1, r0), f_nnz);
    int64_t lo = r0, hi = r1;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)f_col[mid] < first) lo = mid + 1; else hi = mid;
    }
    cur = lo;
    cend = r1;
}

// one K stage of both operands into registers: 4 query rows and 4 candidate rows per thread, a float4 each
__device__ __forceinline__ void rank_load_tiles(const int k0, const int sk, const int d, const float* (&a_row)[4],
                                                const bool (&a_ok)[4], const float* (&b_row)[4], const bool (&b_ok)[4],
                                                f32x4 (&ra)[4], f32x4 (&rb)[4]) {
    const bool k_ok = k0 + sk < d;           // d % 4 == 0: a float4 is whole or absent (the zero-padded K tail)
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (a_ok[p] && k_ok) v = *reinterpret_cast<const f32x4*>(a_row[p] + k0);
        ra[p] = v;
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (b_ok[p] && k_ok) v = *reinterpret_cast<const f32x4*>(b_row[p] + k0);
        rb[p] = v;
    }
}

__device__ __forceinline__ void rank_store_tiles(const f32x4 (&ra)[4], const f32x4 (&rb)[4], float* As, float* Bs, const int srow,
                                                 const int sk) {
#pragma unroll
    for (int p = 0; p < 4; ++p) *reinterpret_cast<f32x4*>(&As[(p * 32 + srow) * RK_KP + sk]) = ra[p];
#pragma unroll
    for (int p = 0; p < 4; ++p) *reinterpret_cast<f32x4*>(&Bs[(p * 32 + srow) * RK_KP + sk]) = rb[p];
}

// one LDS stage into the wave's 2 x 2 accumulator tiles: the k order is k0 + 8 gk + 4 (lane >> 5) + i for every cell
__device__ __forceinline__ void rank_compute(const float* As, const float* Bs, const int wm, const int wn, const int l31,
                                             const int lh, f32x16 (&acc)[2][2]) {
#pragma unroll
    for (int gk = 0; gk < RK_BK / 8; ++gk) {
        float a[2][4], b[2][4];
#pragma unroll
        for (int tm = 0; tm < 2; ++tm) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(&As[(wm * 64 + tm * 32 + l31) * RK_KP + gk * 8 + lh * 4]);
            a[tm][0] = v.x; a[tm][1] = v.y; a[tm][2] = v.z; a[tm][3] = v.w;
        }
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(&Bs[(wn * 64 + tn * 32 + l31) * RK_KP + gk * 8 + lh * 4]);
            b[tn][0] = v.x; b[tn][1] = v.y; b[tn][2] = v.z; b[tn][3] = v.w;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                for (int tn = 0; tn < 2; ++tn)
                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tm][i], b[tn][i], acc[tm][tn], 0, 0, 0);
    }
}

// (tiles per slice, slices) for Q queries against n_cand candidates: the rule of gs_rank.hip's header comment
static inline void rank_plan(const int64_t Q, const int64_t n_cand, int64_t* tiles_n, int64_t* tps, int64_t* slices) {
    *tiles_n = gs_ceil_div(n_cand, RK_BN);
    const int64_t q_tiles = std::max<int64_t>(1, gs_ceil_div(Q, RK_BM));
    const int64_t want = std::max<int64_t>(1, gs_ceil_div(RK_WG_TARGET, q_tiles));
    *tps = std::min<int64_t>(RK_MAX_TILES, std::max<int64_t>(RK_MIN_TILES, gs_ceil_div(*tiles_n, want)));
    *slices = std::max<int64_t>(1, gs_ceil_div(*tiles_n, *tps));
}
