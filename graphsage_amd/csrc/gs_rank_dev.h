// The sweep of the 128 x 128 fp32-MFMA score kernels -- gs_rank.hip (count), gs_topk.hip (select), gs_ivf.hip (inverted-file
// scan), gs_kmeans.hip (argmax) and gs_infonce.hip (softmax statistics and gradients): ONE tile pipeline (RankOperand,
// RankRegs, rank_first_loads, rank_k_loop: the stage buffers inside smem, the accumulator clear, the first two stage requests,
// the K loop), the cell-to-row map of an accumulator (rank_acc_row), the exclusion-word builder, the host's slice plan and the
// host's check of a query descriptor.  Every kernel runs THESE functions, so a (query row, candidate row) pair goes through the
// same k-ordered fmaf chain in all of them: a score selected by gs_topk_select is bit-equal to the t that gs_rank_count returns
// for that pair.  A kernel states which rows are its operands, what it does with a finished accumulator tile and what it
// overlaps with the next tile's first loads.  The layout and the reasons are in the header comment of gs_rank.hip.
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

// The four rows of one operand that a thread stages: rows p * 32 + (tid >> 3) of the tile, p < 4, each pointer already moved
// to the thread's k offset (tid & 7) * 4 -- 8 threads x float4 span BK.  A row that does not exist reads as zeros.
struct RankOperand {
    const float* row[4];
    bool ok[4];
};

// rows r0 .. r0 + 127 of a table of n rows
__device__ __forceinline__ void rank_rows(RankOperand& op, const float* __restrict__ base, const int64_t ld, const int64_t r0,
                                          const int64_t n) {
    const int srow = threadIdx.x >> 3, sk = (threadIdx.x & 7) * 4;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int64_t r = r0 + p * 32 + srow;
        op.ok[p] = r < n;
        op.row[p] = base + (op.ok[p] ? r : 0) * ld + sk;
    }
}

// row of the 32 x 32 MFMA result that accumulator cell e of a lane holds (C/D layout: col = lane & 31, lh = lane >> 5)
__device__ __forceinline__ int rank_acc_row(const int e, const int lh) { return (e & 3) + 8 * (e >> 2) + 4 * lh; }

__device__ __forceinline__ void rank_zero(f32x16 (&acc)[2][2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
}

typedef f32x4 RankRegs[4];           // one K stage of one operand in a thread's registers: 4 rows, a float4 each

// one K stage of both operands into registers
__device__ __forceinline__ void rank_load_tiles(const int k0, const int d, const RankOperand& A, const RankOperand& B, RankRegs& ra,
                                                RankRegs& rb) {
    const bool k_ok = k0 + (int)(threadIdx.x & 7) * 4 < d;       // d % 4 == 0: a float4 is whole or absent (the zero-padded K tail)
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (A.ok[p] && k_ok) v = *reinterpret_cast<const f32x4*>(A.row[p] + k0);
        ra[p] = v;
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (B.ok[p] && k_ok) v = *reinterpret_cast<const f32x4*>(B.row[p] + k0);
        rb[p] = v;
    }
}

// the stage buffers inside smem (2 * RK_STAGE_FLOATS): stage s < 2 is [128 A rows | 128 B rows][RK_KP]
__device__ __forceinline__ float* rank_stage_a(float* smem, const int s) { return smem + s * RK_STAGE_FLOATS; }
__device__ __forceinline__ float* rank_stage_b(float* smem, const int s) { return smem + s * RK_STAGE_FLOATS + RK_BM * RK_KP; }

// ... and from registers into one LDS stage
__device__ __forceinline__ void rank_store_tiles(const RankRegs& ra, const RankRegs& rb, float* As, float* Bs) {
    const int srow = threadIdx.x >> 3, sk = (threadIdx.x & 7) * 4;
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

// The tile pipeline, in two halves so that a kernel can put work between them (the next tile's requests ahead of this tile's
// epilogue).  rank_first_loads requests a tile's first two K stages from global memory; rank_k_loop clears the accumulators
// and runs the K loop over smem = two stages of RK_STAGE_FLOATS: stage s is stored and, after one barrier, consumed while the
// global loads of stage s + 2 are in flight.  The loop has ONE exit (an odd last stage is an `if`, not a `break`): with two
// exits accumulators that outlive the loop are kept in two register sets.  (rank_count_kernel, whose accumulators do not,
// keeps the `break` form written out: gs_rank.hip says why.)  Stages ascend, so the k order of every cell is
// k0 + 8 gk + 4 (lane >> 5) + i for every d that is a multiple of 4.  The caller puts a barrier between the end of one
// rank_k_loop and the next (the stage buffers change hands; an odd stage count ends on the buffer that is stored first).
// The registers of the two stages in flight (ra0, rb0: the even stages, ra1, rb1: the odd ones) are four RankRegs of the
// caller's, handed on from rank_first_loads to rank_k_loop.  (Four plain arrays on purpose: as members of one struct they
// cost rank_count_kernel 4 vector registers.)
// WHOLE_PAIRS: the caller vouches that d is a multiple of 2 RK_BK; the tests for a stage's partner then fold away (they are
// true).  Left in, they take infonce_stats_kernel from 128 to 190 vector registers and infonce_grad_kernel from 237 to 256.
template <bool WHOLE_PAIRS = false>
__device__ __forceinline__ void rank_first_loads(const RankOperand& A, const RankOperand& B, const int d, RankRegs& ra0,
                                                 RankRegs& rb0, RankRegs& ra1, RankRegs& rb1) {
    rank_load_tiles(0, d, A, B, ra0, rb0);
    if (WHOLE_PAIRS || RK_BK < d) rank_load_tiles(RK_BK, d, A, B, ra1, rb1);
}

template <bool WHOLE_PAIRS = false>
__device__ __forceinline__ void rank_k_loop(const RankOperand& A, const RankOperand& B, const int d, float* smem, RankRegs& ra0,
                                            RankRegs& rb0, RankRegs& ra1, RankRegs& rb1, const int wm, const int wn, const int l31,
                                            const int lh, f32x16 (&acc)[2][2]) {
    float* As0 = rank_stage_a(smem, 0);
    float* Bs0 = rank_stage_b(smem, 0);
    float* As1 = rank_stage_a(smem, 1);
    float* Bs1 = rank_stage_b(smem, 1);
    rank_zero(acc);
    for (int k0 = 0; k0 < d; k0 += 2 * RK_BK) {
        rank_store_tiles(ra0, rb0, As0, Bs0);
        __syncthreads();
        if (k0 + 2 * RK_BK < d) rank_load_tiles(k0 + 2 * RK_BK, d, A, B, ra0, rb0);
        rank_compute(As0, Bs0, wm, wn, l31, lh, acc);
        if (WHOLE_PAIRS || k0 + RK_BK < d) {
            rank_store_tiles(ra1, rb1, As1, Bs1);
            __syncthreads();
            if (k0 + 3 * RK_BK < d) rank_load_tiles(k0 + 3 * RK_BK, d, A, B, ra1, rb1);
            rank_compute(As1, Bs1, wm, wn, l31, lh, acc);
        }
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

// The checks that gs_rank_count, gs_topk_select and gs_ivf_search make of the query side of their descriptors (the fields carry
// the same names in all three), `who` being the entry point's name.  The pointers are looked at only when there are queries:
// with Q == 0 the caller returns at once.
template <class Desc>
static int rank_check_query(const char* who, const Desc& q) {
    GS_REQUIRE(q.n_cand <= q.n_rows, "%s: n_cand=%lld exceeds the table's n_rows=%lld", who, (long long)q.n_cand,
               (long long)q.n_rows);
    GS_REQUIRE(q.d >= 4 && q.d <= 1024 && (q.d & 3) == 0, "%s: d=%d must be a multiple of 4 in [4, 1024]", who, q.d);
    GS_REQUIRE((q.flags & ~GS_RANK_KEEP_SRC) == 0, "%s: unknown flags 0x%x", who, (unsigned)q.flags);
    if (q.Q == 0) return GS_OK;
    GS_CHECK_MAT_OF(q.Xq, q.ldq, who, "Xq");
    GS_CHECK_MAT_OF(q.Zc, q.ldz, who, "Zc");
    GS_REQUIRE(q.ldq >= q.d && q.ldz >= q.d, "%s: ld must be >= d", who);
    GS_REQUIRE((q.f_rowptr == nullptr) == (q.f_col == nullptr), "%s: f_rowptr and f_col go together", who);
    GS_REQUIRE(!q.f_rowptr || q.src, "%s: a filter is indexed by src, which is null", who);
    GS_REQUIRE(!q.src || q.n_rows >= 1, "%s: the candidate table is empty (src needs a row)", who);
    GS_REQUIRE(q.f_nnz >= 0, "%s: f_nnz=%lld", who, (long long)q.f_nnz);
    return GS_OK;
}
