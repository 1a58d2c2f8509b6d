// Top-k partners against every node: the sweep of gs_rank.hip with a select epilogue where that kernel counts (no score row is
// ever written to memory).
//
//   C_q     = {0 <= w < n_cand} \ {src[q]} \ filter row of src[q]        (src kept under GS_RANK_KEEP_SRC; there is no dst)
//   s(q, w) = <Xq[q], Zc[w]>
//   out     = the k members of C_q that come first in the total order (s descending, w ascending)
//
// The sweep is gs_rank_dev.h, shared with rank_count_kernel: its tile pipeline (rank_first_loads, rank_k_loop: fp32 MFMA
// v_mfma_f32_32x32x2_f32, BM = BN = 128, BK = 32, two LDS stages), the slice plan, one 128-bit exclusion word per query row
// written before a tile's K loop from the sorted filter row with a forward-only cursor.  Same code, same k-ordered chain:
// s(q, w) here is bit-equal to the t that gs_rank_count returns for dst[q] = w.
//
// Order: a key is one uint64 -- high half the score's bits mapped monotonically to unsigned (-0.0f first made +0.0f), low half
// ~w.  Keys are distinct, a larger key comes first, one unsigned compare is the whole order, and the k largest keys of a set do
// not depend on the order in which they were met.  Key 0 is no candidate ("nothing": ~w >= 2^31 for every real w).  A NaN
// score is just some key: it lands somewhere, nothing is indexed by it.
//
// Epilogue, per candidate tile.  After the K loop the two stage buffers (73,728 B) are dead until the next tile's first
// store: the 128 x 128 accumulator tile is dumped into them as [128][129] floats (66,048 B; lane = column on the way in and on
// the way out, the pad of 1 keeps both free of bank conflicts).  Then the next tile's first two K stages are requested from
// global memory, and under those loads every wave takes 32 of the 128 query rows, ONE ROW AT A TIME WITH ALL 64 LANES (two
// columns per lane; the scores of TK_ROWS = 8 rows are read from LDS together, one latency for the batch), rather than one row
// per thread: a wave-wide ballot of `key > tau` says at once whether the row has anything to keep (after warm-up: usually
// not), and what passes is appended to the row's list in the workspace at ballot-prefix positions -- fire-and-forget stores.
// With one row per thread the 64 rows of a wave would run in lockstep and every insertion of any of them (k (1 + ln(n_slice /
// k)) per row: about 740 at k = 100 in a 58 k slice) would stall all 64 behind a chain of dependent global loads.
//   Per row the slice keeps a list of cap = 64 (1 + ceil(k / 64)) keys (128 or 192) in the workspace, its length and its
// threshold tau (LDS; wave-uniform).  tau is the k-th largest key at the last compaction (0 before the first), so everything
// the list holds beyond the true top k is merely superfluous.  When an append would overflow, the wave compacts the row: all
// keys into registers (three per lane), the k-th largest found by a 64-step radix select on ballots, the k survivors written
// back in place, tau raised.  A list with room for m = cap - k >= 64 new keys multiplies the candidates seen between two
// compactions by e^(m / k): a handful of compactions per row and slice.  The lists are unsorted; only their owning wave
// touches them inside the launch (stores and loads of one workgroup: a workgroup-scope fence before the compaction's loads).
//   Three barriers per tile where the count kernel has one: stages dead -> dump -> rows -> next tile's first store.
//
// topk_merge_kernel: one wave per query pushes the `slices` lists through the same append / compact code on a list in LDS,
// compacts to k, ranks the survivors by counting (keys are distinct: ranks are a permutation) and writes ids int32 [Q, k],
// scores float [Q, k] and count int32 [Q] = min(k, |C_q|); entries at and beyond count are -1 / -inf.
//
// Integers and compares only after the MFMA chain: bitwise reproducible.  No atomics, no workgroup waits on another, plain
// launches on the caller's stream.
//
// Resources (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage; profiles/sweep_pipeline.md, and as they
// were when the kernel was written in profiles/topk_full.md):
// topk_select_kernel 204 vector registers, 102 scalar, no scratch, no spill of either kind, 77,824 B of LDS: two workgroups per
// CU under __launch_bounds__(256, 2), as the count kernel (227 registers).  topk_merge_kernel 30 registers, 6,144 B of LDS.
// The report depends on the pipeline's K loop having ONE exit (gs_rank_dev.h: with two exits the accumulators, which here
// outlive the loop into the dump, were kept in two register sets and 49 to 70 registers spilled).
#include "gs_topk_dev.h"        // the key, the list code, the dump and the offer, the merge (shared with gs_ivf.hip)

static_assert(sizeof(gs_topk_desc) == 144, "gs_topk_desc layout (mirrored by graphsage_amd/_lib.py)");
static_assert(GS_TOPK_MAX == 128, "the merge kernel ranks two keys per lane");

struct TopkArgs {
    const float* Xq; const float* Zc;
    const int32_t* src;
    const int64_t* f_rowptr; const int32_t* f_col;
    uint64_t* lists; int32_t* counts;        // workspace: [slices][Q][cap] keys, then [slices][Q] list lengths
    int64_t Q, ldq, n_rows, n_cand, ldz, f_nnz;
    int32_t d, k, cap, tiles_n, tiles_per_slice, q_tiles;
    int32_t keep_src;            // GS_RANK_KEEP_SRC: src only indexes the filter
};

// (256, 2): a budget of 256 registers per lane, two workgroups per CU
__global__ __launch_bounds__(256, 2) void topk_select_kernel(const TopkArgs g) {
    constexpr int BM = RK_BM, BN = RK_BN;
    __shared__ __attribute__((aligned(16))) float smem[2 * RK_STAGE_FLOATS];
    __shared__ __attribute__((aligned(16))) uint32_t excl[BM][4];      // bit c of row r: (query r, column c of the tile) is not a candidate
    __shared__ uint64_t tauS[BM];
    __shared__ int32_t cntS[BM], sq[BM];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = topk_uniform(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;

    const int q_tile = (int)(blockIdx.x % (unsigned)g.q_tiles);
    const int slice = (int)(blockIdx.x / (unsigned)g.q_tiles);
    const int64_t m0 = (int64_t)q_tile * BM;
    const int tile0 = slice * g.tiles_per_slice;
    const int tile1 = min(tile0 + g.tiles_per_slice, g.tiles_n);
    const int d = g.d;

    // ---- per-query state: own row, cursor into the filter row (threads 0 .. BM-1 own one query each), an empty list
    int64_t cur = 0, cend = 0;
    if (tid < BM) {
        const int64_t q = m0 + tid;
        int32_t ss = -1;
        if (q < g.Q && g.src) {
            ss = g.src[q];
            ss = ss < 0 ? 0 : ((int64_t)ss >= g.n_rows ? (int32_t)(g.n_rows - 1) : ss);      // the caller checked; never a stray read
            if (g.f_rowptr) rank_filter_cursor(g.f_rowptr, g.f_col, g.f_nnz, ss, (int64_t)tile0 * BN, cur, cend);
        }
        sq[tid] = g.keep_src ? -1 : ss;          // the cursor above is all that a kept src is needed for
        cntS[tid] = 0;
        tauS[tid] = 0ull;
    }
    __syncthreads();

    // ---- operand rows of this thread: 4 query rows (fixed), 4 candidate rows (per tile); 8 threads x float4 span BK
    RankOperand A, B;
    rank_rows(A, g.Xq, g.ldq, m0, g.Q);

    // the pipeline of gs_rank_dev.h, with a tile's first two stages requested before the previous tile's rows are scanned
    RankRegs ra0, rb0, ra1, rb1;
    auto first_loads = [&](const int tile) {
        rank_rows(B, g.Zc, g.ldz, (int64_t)tile * BN, g.n_cand);
        rank_first_loads(A, B, d, ra0, rb0, ra1, rb1);
    };
    if (tile0 < tile1) first_loads(tile0);

    for (int tile = tile0; tile < tile1; ++tile) {
        const int64_t n0 = (int64_t)tile * BN;
        if (tid < BM)
            *reinterpret_cast<uint4*>(&excl[tid][0]) = rank_excl_words(n0, g.n_cand, -1, sq[tid], g.f_col, cur, cend);

        f32x16 acc[2][2];
        rank_k_loop(A, B, d, smem, ra0, rb0, ra1, rb1, wm, wn, l31, lh, acc);

        // ---- epilogue
        topk_dump(acc, smem, wm, wn, l31, lh);
        if (tile + 1 < tile1) first_loads(tile + 1);

#pragma unroll 1
        for (int r0 = wave * (BM / 4); r0 < (wave + 1) * (BM / 4); r0 += TK_ROWS) {      // this wave's 32 query rows, 64 lanes on one row
            uint64_t key[TK_ROWS][2], tau_r[TK_ROWS];        // a batch of rows is read from LDS at once: one latency, not TK_ROWS
#pragma unroll
            for (int i = 0; i < TK_ROWS; ++i) {
                const int r = r0 + i;
                tau_r[i] = tauS[r];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const float s = smem[r * TK_LD + h * 64 + lane];
                    const uint32_t word = excl[r][h * 2 + lh];
                    key[i][h] = ((word >> l31) & 1u) ? 0ull : topk_key(s, (uint32_t)(n0 + h * 64 + lane));
                }
            }
            topk_offer(key, tau_r, r0, cntS, tauS, g.cap, g.k, lane, [&](const int r) -> uint64_t* {
                const int64_t q = m0 + r;
                return q < g.Q ? g.lists + ((int64_t)slice * g.Q + q) * g.cap : nullptr;
            });
        }
        // the stage buffers and the exclusion words change hands here
        __syncthreads();
    }

    if (tid < BM && m0 + tid < g.Q) g.counts[(int64_t)slice * g.Q + m0 + tid] = cntS[tid];
}

extern "C" int gs_topk_ws_bytes(int64_t Q, int64_t n_cand, int32_t k, int64_t* bytes_out_host) {
    GS_REQUIRE(bytes_out_host && Q >= 0 && n_cand >= 0 && n_cand <= 0x7fffffffll, "gs_topk_ws_bytes: bad args");
    GS_REQUIRE(k >= 1 && k <= GS_TOPK_MAX, "gs_topk_ws_bytes: k=%d must lie in [1, %d]", k, GS_TOPK_MAX);
    int64_t tiles_n, tps, slices;
    rank_plan(Q, n_cand, &tiles_n, &tps, &slices);
    *bytes_out_host = slices * Q * (topk_cap(k) * (int64_t)sizeof(uint64_t) + (int64_t)sizeof(int32_t));
    return GS_OK;
}

extern "C" int gs_topk_select(const gs_topk_desc* desc_host, void* stream) {
    GS_REQUIRE(desc_host, "gs_topk_select: null descriptor");
    const gs_topk_desc& q = *desc_host;
    GS_REQUIRE(q.Q >= 0 && q.n_rows >= 0 && q.n_rows <= 0x7fffffffll && q.n_cand >= 0,
               "gs_topk_select: bad sizes Q=%lld n_rows=%lld n_cand=%lld", (long long)q.Q, (long long)q.n_rows, (long long)q.n_cand);
    GS_REQUIRE(q.k >= 1 && q.k <= GS_TOPK_MAX, "gs_topk_select: k=%d must lie in [1, %d]", q.k, GS_TOPK_MAX);
    const int rc = rank_check_query("gs_topk_select", q);
    if (rc != GS_OK || q.Q == 0) return rc;
    GS_REQUIRE(q.ids && q.scores && q.count, "gs_topk_select: ids, scores and count must be non-null");
    int64_t tiles_n, tps, slices;
    rank_plan(q.Q, q.n_cand, &tiles_n, &tps, &slices);
    const int64_t cap = topk_cap(q.k);
    const int64_t need = slices * q.Q * (cap * (int64_t)sizeof(uint64_t) + (int64_t)sizeof(int32_t));
    GS_REQUIRE(q.ws && (reinterpret_cast<uintptr_t>(q.ws) & 7u) == 0 && q.ws_bytes >= need,
               "gs_topk_select: needs an 8-byte aligned workspace of %lld bytes (gs_topk_ws_bytes), got %lld", (long long)need,
               (long long)q.ws_bytes);
    const int64_t q_tiles = gs_ceil_div(q.Q, RK_BM);
    const int64_t blocks = q_tiles * slices;
    GS_REQUIRE(blocks < (1ll << 31) && gs_ceil_div(q.Q, 4) < (1ll << 31),
               "gs_topk_select: grid too large (%lld blocks); call it on chunks of the queries", (long long)blocks);
    TopkArgs g;
    g.Xq = q.Xq; g.Zc = q.Zc; g.src = q.src; g.f_rowptr = q.f_rowptr; g.f_col = q.f_col;
    g.lists = reinterpret_cast<uint64_t*>(q.ws);
    g.counts = reinterpret_cast<int32_t*>(g.lists + slices * q.Q * cap);
    g.Q = q.Q; g.ldq = q.ldq; g.n_rows = q.n_rows; g.n_cand = q.n_cand; g.ldz = q.ldz; g.f_nnz = q.f_nnz;
    g.d = q.d; g.k = q.k; g.cap = (int32_t)cap;
    g.tiles_n = (int32_t)tiles_n; g.tiles_per_slice = (int32_t)tps; g.q_tiles = (int32_t)q_tiles;
    g.keep_src = (q.flags & GS_RANK_KEEP_SRC) ? 1 : 0;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(topk_select_kernel, dim3((unsigned)blocks), dim3(256), 0, st, g);
    GS_LAUNCH_CHECK("topk_select_kernel");
    return topk_merge_launch(g.lists, g.counts, q.Q, (int)slices, (int)cap, q.k, q.ids, q.scores, q.count, st);
}
