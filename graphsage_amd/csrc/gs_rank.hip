// Link ranking against every node: a contraction with a compare-and-count epilogue (no score is ever written to memory).
//
//   t[q]    = <Xq[q], Zc[dst[q]]>
//   n_gt[q] = #{w in C_q : <Xq[q], Zc[w]> >  t[q]}        C_q = {0 <= w < n_cand} \ {dst[q]} \ {src[q]} \ filter row of src[q]
//   n_eq[q] = #{w in C_q : <Xq[q], Zc[w]> == t[q]}
//
// Arithmetic: plain fp32 on the matrix cores (v_mfma_f32_32x32x2_f32), the tile pipeline of gs_rank_dev.h: both operands
// k-contiguous, staged through LDS as direct float4 copies ([row][32 + 4], one ds_read_b128 per 4 k-steps), two LDS stages and
// two register stages, one barrier per stage.  An MFMA result is a k-ordered fmaf chain whose order (k0 + 4 * (lane >> 5) + i)
// does not depend on where a row or a column sits in the tile.
//
// Tie property: t is NOT computed by another kernel or another loop.  Every workgroup first runs the sweep's own tile code on
// the dst-GATHERED candidate rows (column j of that tile = Zc[dst[m0 + j]]) and keeps the diagonal; BM == BN makes that tile
// square.  A candidate row that is bit-identical to Zc[dst[q]] therefore goes through the same chain and scores bit-equal to
// t[q].  Every slice of a query tile recomputes t (one extra tile per slice, all bit-identical); slice 0 writes it out.
//
// Tiling: 256 threads = 4 waves (2 x 2), block tile BM x BN = 128 x 128 (each wave 2 x 2 MFMA tiles of 32 x 32, 64 accumulator
// registers), BK = 32.  LDS: 2 stages x (128 + 128) rows x 36 floats = 72 KB + 5.5 KB of epilogue state => two workgroups per
// CU of the 160 KB, one wave of each per SIMD, inside a budget of 256 registers per lane: the compiler reports 227 vector
// registers, no vector spill and no scratch; 18 scalar registers (the argument block is large) are parked in lanes of a
// vector register.  Measured at the Reddit shape against one workgroup per CU with 512 registers: profiles/rank_full.md.
// 128 x 128 is the tile of the dense kernels' large form: 32 FLOP per operand byte read from LDS.
//
// The grid runs over (candidate slice, query tile), query tile fastest, so the workgroups that are resident together walk
// the SAME candidate rows (shared through L2 / Infinity Cache) while each re-reads its own 128-row query panel (d * 512
// bytes, L2-resident).  A slice is a run of tiles_per_slice candidate tiles: at least 4 (the t tile costs one), and
// otherwise as few slices as give about 2048 workgroups (8 per CU: the tail of the last round stays small next to the
// launch).  At Q = 65,536, n_cand = 232,965: 512 query tiles x 4 slices of 456 tiles, a 2 MB slab.
//
// Counts: every lane keeps one packed uint32 (gt in the low half, eq in the high half; at most 2 * tiles_per_slice <= 32,768
// per lane and half, so neither half overflows) per accumulator row, in registers across the slice; they are summed over
// the 32 lanes of a half wave by shuffles, over the two column waves through LDS, and go to the int32 slab
// [slices][Q][2].  rank_sum_kernel adds the slabs.  Integers only: bitwise reproducible.  No workgroup waits on another, no atomics of any kind, plain launches on the caller's stream.
//
// Exclusions live INSIDE the tile: before a tile's K loop the thread that owns query row r (threads 0 .. 127) writes the row's
// 128-bit exclusion word for the tile's columns: columns at or beyond n_cand, dst[q], src[q] (unless the descriptor's flags
// say GS_RANK_KEEP_SRC: src then only names the filter row), and the entries of the filter
// row of src[q] that fall into the tile.  The filter row is sorted, so the thread keeps a cursor into it (binary search at the
// slice's first candidate, then it only moves forward).  The epilogue tests the bit, so a filtered cell is skipped with the
// very score that would have been counted; dst listed in its own filter row just sets the same bit twice.
//
// The tile pipeline (operand rows, stage buffers, the first two stage requests, the K loop), the exclusion-word builder, the
// slice plan and the host's check of the query descriptor live in gs_rank_dev.h, which the other score sweeps include too:
// gs_topk.hip (select), gs_ivf.hip (inverted-file scan), gs_kmeans.hip (argmax) and gs_infonce.hip (softmax).
#include "gs_rank_dev.h"

static_assert(sizeof(gs_rank_desc) == 144, "gs_rank_desc layout (mirrored by graphsage_amd/_lib.py)");

struct RankArgs {
    const float* Xq; const float* Zc;
    const int32_t* dst; const int32_t* src;
    const int64_t* f_rowptr; const int32_t* f_col;
    float* t; int32_t* slab;
    int64_t Q, ldq, n_rows, n_cand, ldz, f_nnz;
    int32_t d, tiles_n, tiles_per_slice, q_tiles;
    int32_t keep_src;            // GS_RANK_KEEP_SRC: src only indexes the filter
};

// (256, 2): a budget of 256 registers per lane, two workgroups per CU
__global__ __launch_bounds__(256, 2) void rank_count_kernel(const RankArgs g) {
    constexpr int BM = RK_BM, BN = RK_BN;
    __shared__ __attribute__((aligned(16))) float smem[2 * RK_STAGE_FLOATS];
    __shared__ __attribute__((aligned(16))) uint32_t excl[BM][4];      // bit c of row r: (query r, column c of the tile) is not a candidate
    __shared__ float tq[BM];
    __shared__ int32_t dq[BM], sq[BM];
    __shared__ int32_t cnt[2][BM][2];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;

    const int q_tile = (int)(blockIdx.x % (unsigned)g.q_tiles);
    const int slice = (int)(blockIdx.x / (unsigned)g.q_tiles);
    const int64_t m0 = (int64_t)q_tile * BM;
    const int tile0 = slice * g.tiles_per_slice;
    const int tile1 = min(tile0 + g.tiles_per_slice, g.tiles_n);
    const int d = g.d;

    // ---- per-query state: target row, own row, cursor into the filter row (threads 0 .. BM-1 own one query each)
    int64_t cur = 0, cend = 0;
    if (tid < BM) {
        const int64_t q = m0 + tid;
        int32_t dd = 0, ss = -1;
        if (q < g.Q) {
            dd = g.dst[q];
            dd = dd < 0 ? 0 : ((int64_t)dd >= g.n_rows ? (int32_t)(g.n_rows - 1) : dd);      // the caller checked; never a stray read
            if (g.src) {
                ss = g.src[q];
                ss = ss < 0 ? 0 : ((int64_t)ss >= g.n_rows ? (int32_t)(g.n_rows - 1) : ss);
                if (g.f_rowptr) rank_filter_cursor(g.f_rowptr, g.f_col, g.f_nnz, ss, (int64_t)tile0 * BN, cur, cend);
            }
        }
        dq[tid] = dd;
        sq[tid] = g.keep_src ? -1 : ss;          // the cursor above is all that a kept src is needed for
    }
    __syncthreads();

    // ---- operand rows of this thread: 4 query rows (fixed), 4 candidate rows (per tile); 8 threads x float4 span BK
    RankOperand A;
    rank_rows(A, g.Xq, g.ldq, m0, g.Q);

    uint32_t c[2][16];           // packed (gt | eq << 16) per accumulator row, both column tiles of the wave together
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int e = 0; e < 16; ++e) c[tm][e] = 0u;

    // tile -1 is the t tile (candidate rows gathered through dst, the diagonal kept), then the slice's candidate tiles
    for (int tile = tile0 - 1; tile < tile1; ++tile) {
        const bool t_tile = tile < tile0;
        const int64_t n0 = (int64_t)tile * BN;
        RankOperand B;
        if (t_tile) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                B.ok[p] = true;
                B.row[p] = g.Zc + (int64_t)dq[p * 32 + (tid >> 3)] * g.ldz + (tid & 7) * 4;
            }
        } else {
            rank_rows(B, g.Zc, g.ldz, n0, g.n_cand);
            if (tid < BM)
                *reinterpret_cast<uint4*>(&excl[tid][0]) = rank_excl_words(n0, g.n_cand, dq[tid], sq[tid], g.f_col, cur, cend);
        }

        // The pipeline of gs_rank_dev.h written out with a `break` where rank_k_loop has an `if` -- the one kernel that keeps a
        // loop of its own.  Its accumulators do not outlive the loop into a dump, so the second exit costs no registers (227
        // either way), and through rank_k_loop the kernel ran 0.2 % to 0.5 % slower than before (profiles/sweep_pipeline.md).
        // The order of the arithmetic is the same either way.
        f32x16 acc[2][2];
        rank_zero(acc);
        RankRegs ra0, rb0, ra1, rb1;
        float* As0 = rank_stage_a(smem, 0);
        float* Bs0 = rank_stage_b(smem, 0);
        float* As1 = rank_stage_a(smem, 1);
        float* Bs1 = rank_stage_b(smem, 1);
        auto load_tiles = [&](const int k0, RankRegs& ra, RankRegs& rb) { rank_load_tiles(k0, d, A, B, ra, rb); };
        auto store_tiles = [&](const RankRegs& ra, const RankRegs& rb, float* As, float* Bs) { rank_store_tiles(ra, rb, As, Bs); };
        auto compute = [&](const float* As, const float* Bs) { rank_compute(As, Bs, wm, wn, l31, lh, acc); };
        load_tiles(0, ra0, rb0);
        if (RK_BK < d) load_tiles(RK_BK, ra1, rb1);
        for (int k0 = 0; k0 < d; k0 += 2 * RK_BK) {
            store_tiles(ra0, rb0, As0, Bs0);
            __syncthreads();
            if (k0 + 2 * RK_BK < d) load_tiles(k0 + 2 * RK_BK, ra0, rb0);
            compute(As0, Bs0);
            if (k0 + RK_BK >= d) break;
            store_tiles(ra1, rb1, As1, Bs1);
            __syncthreads();
            if (k0 + 3 * RK_BK < d) load_tiles(k0 + 3 * RK_BK, ra1, rb1);
            compute(As1, Bs1);
        }

        // ---- epilogue
        if (t_tile) {
            if (wm == wn) {
#pragma unroll
                for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                    for (int e = 0; e < 16; ++e)
                        if (rank_acc_row(e, lh) == l31) tq[wm * 64 + tm * 32 + l31] = acc[tm][tm][e];
            }
        } else {
            // (the exclusion words were written before the K loop's first barrier)
#pragma unroll
            for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int lr = wm * 64 + tm * 32 + rank_acc_row(e, lh);
                    const float tv = tq[lr];
                    const uint2 mw = *reinterpret_cast<const uint2*>(&excl[lr][wn * 2]);
                    uint32_t add = 0u;
#pragma unroll
                    for (int tn = 0; tn < 2; ++tn) {
                        const float s = acc[tm][tn][e];
                        const uint32_t word = tn ? mw.y : mw.x;
                        const uint32_t hit = s > tv ? 1u : (s == tv ? 0x10000u : 0u);
                        add += ((word >> l31) & 1u) ? 0u : hit;
                    }
                    c[tm][e] += add;
                }
        }
        // the stage buffers, the exclusion words (and tq after the t tile) change hands here
        __syncthreads();
    }

    if (slice == 0 && tid < BM && m0 + tid < g.Q) g.t[m0 + tid] = tq[tid];

    // ---- counts: 32 lanes of a half wave -> LDS -> the two column waves -> slab
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            int gt = (int)(c[tm][e] & 0xffffu), eq = (int)(c[tm][e] >> 16);
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) {
                gt += __shfl_xor(gt, off, 64);
                eq += __shfl_xor(eq, off, 64);
            }
            if (l31 == 0) {
                const int lr = wm * 64 + tm * 32 + rank_acc_row(e, lh);
                cnt[wn][lr][0] = gt;
                cnt[wn][lr][1] = eq;
            }
        }
    __syncthreads();
    if (tid < BM && m0 + tid < g.Q) {
        int32_t* out = g.slab + ((int64_t)slice * g.Q + m0 + tid) * 2;
        out[0] = cnt[0][tid][0] + cnt[1][tid][0];
        out[1] = cnt[0][tid][1] + cnt[1][tid][1];
    }
}

__global__ __launch_bounds__(256) void rank_sum_kernel(const int32_t* __restrict__ slab, const int64_t Q, const int slices,
                                                       int32_t* __restrict__ n_gt, int32_t* __restrict__ n_eq) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    int gt = 0, eq = 0;
    for (int s = 0; s < slices; ++s) {
        const int2 v = *reinterpret_cast<const int2*>(slab + ((int64_t)s * Q + q) * 2);
        gt += v.x;
        eq += v.y;
    }
    n_gt[q] = gt;
    n_eq[q] = eq;
}

extern "C" int gs_rank_ws_bytes(int64_t Q, int64_t n_cand, int64_t* bytes_out_host) {
    GS_REQUIRE(bytes_out_host && Q >= 0 && n_cand >= 0 && n_cand <= 0x7fffffffll, "gs_rank_ws_bytes: bad args");
    int64_t tiles_n, tps, slices;
    rank_plan(Q, n_cand, &tiles_n, &tps, &slices);
    *bytes_out_host = slices * Q * 2 * (int64_t)sizeof(int32_t);
    return GS_OK;
}

extern "C" int gs_rank_count(const gs_rank_desc* desc_host, void* stream) {
    GS_REQUIRE(desc_host, "gs_rank_count: null descriptor");
    const gs_rank_desc& q = *desc_host;
    GS_REQUIRE(q.Q >= 0 && q.n_rows >= 0 && q.n_rows <= 0x7fffffffll && q.n_cand >= 0,
               "gs_rank_count: bad sizes Q=%lld n_rows=%lld n_cand=%lld", (long long)q.Q, (long long)q.n_rows, (long long)q.n_cand);
    GS_REQUIRE(q.Q == 0 || q.n_rows >= 1, "gs_rank_count: the candidate table is empty (dst needs a row)");
    const int rc = rank_check_query("gs_rank_count", q);
    if (rc != GS_OK || q.Q == 0) return rc;
    GS_REQUIRE(q.dst && q.t && q.n_gt && q.n_eq, "gs_rank_count: dst, t, n_gt and n_eq must be non-null");
    int64_t tiles_n, tps, slices;
    rank_plan(q.Q, q.n_cand, &tiles_n, &tps, &slices);
    const int64_t need = slices * q.Q * 2 * (int64_t)sizeof(int32_t);
    GS_REQUIRE(q.ws && (reinterpret_cast<uintptr_t>(q.ws) & 7u) == 0 && q.ws_bytes >= need,
               "gs_rank_count: needs an 8-byte aligned workspace of %lld bytes (gs_rank_ws_bytes), got %lld", (long long)need,
               (long long)q.ws_bytes);
    const int64_t q_tiles = gs_ceil_div(q.Q, RK_BM);
    const int64_t blocks = q_tiles * slices;
    GS_REQUIRE(blocks < (1ll << 31), "gs_rank_count: grid too large (%lld blocks); call it on chunks of the queries", (long long)blocks);
    RankArgs g;
    g.Xq = q.Xq; g.Zc = q.Zc; g.dst = q.dst; g.src = q.src; g.f_rowptr = q.f_rowptr; g.f_col = q.f_col;
    g.t = q.t; g.slab = reinterpret_cast<int32_t*>(q.ws);
    g.Q = q.Q; g.ldq = q.ldq; g.n_rows = q.n_rows; g.n_cand = q.n_cand; g.ldz = q.ldz; g.f_nnz = q.f_nnz;
    g.d = q.d; g.tiles_n = (int32_t)tiles_n; g.tiles_per_slice = (int32_t)tps; g.q_tiles = (int32_t)q_tiles;
    g.keep_src = (q.flags & GS_RANK_KEEP_SRC) ? 1 : 0;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rank_count_kernel, dim3((unsigned)blocks), dim3(256), 0, st, g);
    GS_LAUNCH_CHECK("rank_count_kernel");
    hipLaunchKernelGGL(rank_sum_kernel, dim3((unsigned)gs_ceil_div(q.Q, 256)), dim3(256), 0, st, g.slab, q.Q, (int)slices, q.n_gt, q.n_eq);
    GS_LAUNCH_CHECK("rank_sum_kernel");
    return GS_OK;
}
