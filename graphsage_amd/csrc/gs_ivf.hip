// Approximate top-k partners through an inverted file: the sweep of gs_topk.hip over GATHERED (query, cluster-member) tiles.
//
//   index   = centres c_j (j < C, none without members), list_j = the table rows of cluster j in ascending row id
//   P_q     = the nprobe centres that come first by (<x_q, c_j> descending, j ascending)
//   C_q     = the candidate set of gs_topk_select: rows below n_cand, without src[q] (kept under GS_RANK_KEEP_SRC), without the
//             filter row of src[q]
//   out     = the first min(k, .) members of C_q n U_{j in P_q} list_j by (<x_q, z_w> descending, w ascending)
//
// A (query row, candidate row) pair goes through rank_compute's k-ordered chain whatever tile it sits in, and the key, the list
// code, the dump, the offer and the merge are gs_topk_dev.h: with nprobe = C the ids, the score bits and the counts are those
// of gs_topk_select.
//
// Five steps per call, plain launches on the caller's stream, nothing read back in between:
//   1 probe   gs_topk_select on (queries, centres) with k = nprobe                                -> probe ids [Q][nprobe]
//   2 group   pair p = j Q + q (probe slot j of query q).  ivf_pairs_kernel writes the probe ids in that probe-major order and
//             scanned[q]; gs_kmeans_members groups the pair numbers by cluster: pair_ptr [C + 1], pairs (ascending per cluster)
//   3 plan    a work item is (cluster c, tile t of 128 of its pairs).  ivf_plan_kernel (one workgroup): item_ptr[c] = exclusive
//             scan of ceil(pairs_c / 128).  The scan grid is the bound floor(Q nprobe / 128) + C; a workgroup finds its item by a
//             binary search on item_ptr (at most 13 steps) or exits.  Integers, no atomics, no workgroup waits on another.
//   4 scan    ivf_scan_kernel, one workgroup per item: A operand rows Xq + (p mod Q) ldq of its 128 pairs (fixed), B operand
//             rows Zc + list_ids[.] ldz of one member tile after the other; the tile pipeline of gs_rank_dev.h (rank_first_loads,
//             rank_k_loop), then topk_dump and the row scan of topk_select_kernel with w = ids[col] (the tile's 128 ids wait in
//             LDS, two buffers: the next tile's are fetched under this tile's row scan).  Pair p's key list is ws + p cap, its
//             length counts[p]: the [slices][Q][cap] layout of topk_merge_kernel with slices = nprobe.  One workgroup owns a
//             pair's list for the whole launch; counts is cleared first (a pair of an empty probe slot is never scanned).
//   5 merge   topk_merge_kernel, slices = nprobe.  A row is in one list only: the keys of a query stay distinct.
//
// Exclusion is LAZY.  A list's tile spans most of the id space, so the forward cursor of rank_excl_words has nothing to walk
// along, and testing 128 columns against a 492-entry filter row for every (tile, query) would cost more than the tile's MFMA
// work.  Instead: absent columns, ids at or beyond n_cand and the self id are one compare each when the key is made; the
// filter row of src[q] is consulted only for a key that already beats the row's threshold tau -- a binary search in
// [f_rowptr[s], f_rowptr[s + 1]) clamped into f_nnz (at most 31 halvings), a hit making the key 0 before topk_push.  The
// searches of IVF_FROWS = 2 rows of a batch (two columns each: 4 per lane) advance in lockstep and branch-free, one halving
// of all of them per step, so their loads are in flight together; one search after the other, each a chain of dependent
// loads, made the filtered scan 1.9 to 2.6 times the unfiltered one, this form 1.4 to 1.8 times (profiles/topk_ivf.md).  A
// list's threshold rises only when its list is compacted, so keys beat it in many tiles, not only in the first; where none
// does, a ballot skips the group.  tau only rises, so a key tested against an older tau is at worst searched for in vain.
//
// Resources (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage; quoted in profiles/topk_ivf.md):
// ivf_scan_kernel 198 vector registers, 100 scalar, no scratch, no spill of either kind, 78,848 B of LDS (the two stage buffers
// and 5,120 B of per-pair state and member ids; topk_select_kernel: 77,824 B): two workgroups per CU under
// __launch_bounds__(256, 2).  The list and candidate bounds are 32-bit on purpose: as 64-bit values they cost 2 scalar spills.
// ivf_pairs_kernel 14 registers, ivf_plan_kernel 44 and 1,024 B of LDS.
#include "gs_topk_dev.h"

static_assert(sizeof(gs_ivf_desc) == 200, "gs_ivf_desc layout (mirrored by graphsage_amd/_lib.py)");
static_assert(GS_IVF_MAX_PROBE <= GS_TOPK_MAX, "the probe is one gs_topk_select with k = nprobe");

#define IVF_FROWS 2              // rows of a batch whose filter lookups advance together (4 searches per lane; 4 rows cost 6 scalar spills)
static_assert(TK_ROWS % IVF_FROWS == 0, "a batch of rows is whole groups of filter lookups");

struct IvfArgs {
    const float* Xq; const float* Zc;
    const int32_t* src;
    const int64_t* f_rowptr; const int32_t* f_col;
    const int64_t* list_ptr; const int32_t* list_ids;
    const int64_t* pair_ptr; const int32_t* pairs; const int32_t* item_ptr;
    uint64_t* lists; int32_t* counts;        // workspace: [nprobe][Q][cap] keys, [nprobe][Q] list lengths
    int64_t Q, n_pairs, ldq, n_rows, ldz, f_nnz;
    int32_t n_cand, n_list;      // both below 2^31 (n_cand <= n_rows)
    int32_t d, k, cap, n_clusters;
    int32_t keep_src;            // GS_RANK_KEEP_SRC: src only indexes the filter
};

// one thread per query: the probe ids [Q][P] in probe-major order [P][Q] (anything outside [0, C): -1), scanned[q]
__global__ __launch_bounds__(256) void ivf_pairs_kernel(const int32_t* __restrict__ probe_ids, const int64_t Q, const int P, const int C,
                                                        const int64_t* __restrict__ list_ptr, int32_t* __restrict__ pm,
                                                        int64_t* __restrict__ scanned) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    int64_t total = 0;
    for (int j = 0; j < P; ++j) {
        int32_t c = probe_ids[q * P + j];
        if (c < 0 || c >= C) c = -1;
        pm[(int64_t)j * Q + q] = c;
        if (c >= 0) total += max(list_ptr[c + 1] - list_ptr[c], (int64_t)0);
    }
    if (scanned) scanned[q] = total;
}

// one workgroup: item_ptr[c] = items of the clusters before c, item_ptr[C] = all   (C <= 4096: 16 per thread)
__global__ __launch_bounds__(256) void ivf_plan_kernel(const int64_t* __restrict__ pair_ptr, const int C, int32_t* __restrict__ item_ptr) {
    __shared__ int32_t part[256];
    const int per = (C + 255) / 256;
    const int j0 = threadIdx.x * per, j1 = min(j0 + per, C);
    auto items = [&](const int j) { return (int32_t)((max(pair_ptr[j + 1] - pair_ptr[j], (int64_t)0) + RK_BM - 1) / RK_BM); };
    int32_t s = 0;
    for (int j = j0; j < j1; ++j) s += items(j);
    part[threadIdx.x] = s;
    __syncthreads();
    int32_t base = 0;
    for (int t = 0; t < (int)threadIdx.x; ++t) base += part[t];
    for (int j = j0; j < j1; ++j) {
        item_ptr[j] = base;
        base += items(j);
    }
    if (threadIdx.x == 255) item_ptr[C] = base;
}

// (256, 2): a budget of 256 registers per lane, two workgroups per CU
__global__ __launch_bounds__(256, 2) void ivf_scan_kernel(const IvfArgs g) {
    constexpr int BM = RK_BM, BN = RK_BN;
    __shared__ __attribute__((aligned(16))) float smem[2 * RK_STAGE_FLOATS];
    __shared__ uint64_t tauS[BM];
    __shared__ int64_t f0S[BM];                  // the filter run of the row's query node: first entry, length
    __shared__ int32_t flenS[BM], cntS[BM], sq[BM], pairS[BM];
    __shared__ int32_t idS[2][BN];               // the table rows of a member tile (-1: the column does not exist), by tile parity

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = topk_uniform(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;
    const int d = g.d;

    // ---- the work item of this workgroup: cluster c with item_ptr[c] <= b < item_ptr[c + 1], tile t = b - item_ptr[c] of its pairs
    const int C = g.n_clusters;
    const int b = (int)blockIdx.x;
    if (b >= g.item_ptr[C]) return;              // uniform: the grid is an upper bound
    int c = 0;
    {
        int hi = C;                              // item_ptr[c] <= b < item_ptr[hi] throughout
        for (int step = 0; step < 13 && hi - c > 1; ++step) {
            const int mid = (c + hi) >> 1;
            if (g.item_ptr[mid] <= b) c = mid; else hi = mid;
        }
    }
    const int64_t pp0 = min(max(g.pair_ptr[c] + (int64_t)(b - g.item_ptr[c]) * BM, (int64_t)0), g.n_pairs);
    const int64_t pp1 = min(max(g.pair_ptr[c + 1], pp0), min(pp0 + BM, g.n_pairs));
    const int l0 = (int)min(max(g.list_ptr[c], (int64_t)0), (int64_t)g.n_list);
    const int l1 = (int)min(max(g.list_ptr[c + 1], (int64_t)l0), (int64_t)g.n_list);
    const int tiles = (l1 - l0) / BN + ((l1 - l0) % BN != 0);

    // ---- per-pair state (threads 0 .. BM-1 own one each): query, own row, filter run, an empty list
    if (tid < BM) {
        int32_t p = pp0 + tid < pp1 ? g.pairs[pp0 + tid] : -1;
        if (p < 0 || (int64_t)p >= g.n_pairs) p = -1;
        int32_t ss = -1, flen = 0;
        int64_t f0 = 0;
        if (p >= 0 && g.src) {
            ss = g.src[(int64_t)p % g.Q];
            ss = ss < 0 ? 0 : ((int64_t)ss >= g.n_rows ? (int32_t)(g.n_rows - 1) : ss);      // the caller checked; never a stray read
            if (g.f_rowptr) {
                f0 = min(max(g.f_rowptr[ss], (int64_t)0), g.f_nnz);
                const int64_t f1 = min(max(g.f_rowptr[ss + 1], f0), g.f_nnz);
                flen = (int32_t)min(f1 - f0, (int64_t)0x7fffffff);
            }
        }
        pairS[tid] = p;
        sq[tid] = g.keep_src ? -1 : ss;
        f0S[tid] = f0;
        flenS[tid] = flen;
        cntS[tid] = 0;
        tauS[tid] = 0ull;
    }
    __syncthreads();

    // ---- operand rows of this thread: 4 query rows (fixed), 4 member rows (per tile); 8 threads x float4 span BK
    const int srow = tid >> 3, sk = (tid & 7) * 4;
    RankOperand A, B;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int32_t pr = pairS[p * 32 + srow];
        A.ok[p] = pr >= 0;
        A.row[p] = g.Xq + (A.ok[p] ? (int64_t)pr % g.Q : 0) * g.ldq + sk;
    }
    auto member_rows = [&](const int tile) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int j = l0 + tile * BN + p * 32 + srow;                 // (j - l0 < tiles BN <= l1 - l0 + 127: no overflow)
            int32_t w = j < l1 ? g.list_ids[j] : -1;
            B.ok[p] = w >= 0 && w < g.n_cand;                             // the caller checked; never a stray read (n_cand <= n_rows)
            w = B.ok[p] ? w : -1;
            B.row[p] = g.Zc + (int64_t)(B.ok[p] ? w : 0) * g.ldz + sk;
            if ((tid & 7) == 0) idS[tile & 1][p * 32 + srow] = w;
        }
    };

    // the pipeline of gs_rank_dev.h, with a tile's first two stages requested before the previous tile's rows are scanned
    RankRegs ra0, rb0, ra1, rb1;
    auto first_loads = [&](const int tile) {
        member_rows(tile);
        rank_first_loads(A, B, d, ra0, rb0, ra1, rb1);
    };
    if (0 < tiles) first_loads(0);

    for (int tile = 0; tile < tiles; ++tile) {
        f32x16 acc[2][2];
        rank_k_loop(A, B, d, smem, ra0, rb0, ra1, rb1, wm, wn, l31, lh, acc);

        // ---- epilogue
        topk_dump(acc, smem, wm, wn, l31, lh);
        if (tile + 1 < tiles) first_loads(tile + 1);         // (writes the OTHER id buffer: its readers passed the barrier that ended tile - 1)

        // the two columns of this lane: their table rows (-1: no such column, or an id outside [0, n_cand): no candidate)
        const int32_t w_col[2] = {idS[tile & 1][lane], idS[tile & 1][64 + lane]};

#pragma unroll 1
        for (int r0 = wave * (BM / 4); r0 < (wave + 1) * (BM / 4); r0 += TK_ROWS) {      // this wave's 32 pairs, 64 lanes on one row
            uint64_t key[TK_ROWS][2], tau_r[TK_ROWS];        // a batch of rows is read from LDS at once: one latency, not TK_ROWS
#pragma unroll
            for (int i = 0; i < TK_ROWS; ++i) {
                const int r = r0 + i;
                tau_r[i] = tauS[r];
                const int32_t self = sq[r];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const float s = smem[r * TK_LD + h * 64 + lane];
                    key[i][h] = (w_col[h] < 0 || w_col[h] == self) ? 0ull : topk_key(s, (uint32_t)w_col[h]);
                }
            }
            // the lazy filter lookup, IVF_FROWS rows at a time: only keys that would be appended are searched for, and the 2 x
            // IVF_FROWS searches of a lane advance in lockstep.  Branch-free on purpose -- behind a branch every load would be
            // waited for before the next is issued: a search is (base, n), the run [base, base + n) of its row still holding the
            // last entry <= w; a key that needs no search has n = 1 and re-reads its row's first entry.
            if (g.f_col) {
#pragma unroll
                for (int i0 = 0; i0 < TK_ROWS; i0 += IVF_FROWS) {
                    int base[IVF_FROWS][2], n[IVF_FROWS][2], flen[IVF_FROWS];
                    const int32_t* frow[IVF_FROWS];
                    int longest = 0;
                    bool any = false;
#pragma unroll
                    for (int i = 0; i < IVF_FROWS; ++i) {
                        const int r = r0 + i0 + i;
                        flen[i] = flenS[r];                  // 0 for a pair that does not exist or has no filter row
                        frow[i] = g.f_col + (flen[i] > 0 ? f0S[r] : 0);          // (flen > 0 somewhere: f_col has an entry)
                        longest = max(longest, flen[i]);
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const bool need = key[i0 + i][h] > tau_r[i0 + i] && flen[i] > 0;
                            base[i][h] = 0;
                            n[i][h] = need ? flen[i] : 1;
                            any |= need;
                        }
                    }
                    if (__ballot(any) == 0ull) continue;     // after warm-up: the usual case
                    const int steps = 32 - __clz(topk_uniform(longest));         // halvings that bring n = longest down to 1
#pragma unroll 1
                    for (int step = 0; step < steps; ++step) {
                        int32_t v[IVF_FROWS][2];
#pragma unroll
                        for (int i = 0; i < IVF_FROWS; ++i)
#pragma unroll
                            for (int h = 0; h < 2; ++h) v[i][h] = frow[i][base[i][h] + (n[i][h] >> 1)];      // < base + n
#pragma unroll
                        for (int i = 0; i < IVF_FROWS; ++i)
#pragma unroll
                            for (int h = 0; h < 2; ++h) {
                                const int half = n[i][h] >> 1;
                                base[i][h] = v[i][h] <= w_col[h] ? base[i][h] + half : base[i][h];
                                n[i][h] -= half;
                            }
                    }
                    int32_t at[IVF_FROWS][2];
#pragma unroll
                    for (int i = 0; i < IVF_FROWS; ++i)
#pragma unroll
                        for (int h = 0; h < 2; ++h) at[i][h] = frow[i][base[i][h]];
#pragma unroll
                    for (int i = 0; i < IVF_FROWS; ++i)
#pragma unroll
                        for (int h = 0; h < 2; ++h)          // (a key that needed no search is zeroed only if its row's first entry is w)
                            if (flen[i] > 0 && at[i][h] == w_col[h]) key[i0 + i][h] = 0ull;
                }
            }
            topk_offer(key, tau_r, r0, cntS, tauS, g.cap, g.k, lane, [&](const int r) -> uint64_t* {
                const int32_t p = topk_uniform(pairS[r]);
                return p >= 0 ? g.lists + (int64_t)p * g.cap : nullptr;
            });
        }
        // the stage buffers change hands here
        __syncthreads();
    }

    if (tid < BM && pairS[tid] >= 0) g.counts[pairS[tid]] = cntS[tid];
}

// ---------------------------------------------------------------------------------------------------------------
// the workspace: every part at a multiple of 16 bytes
struct IvfLayout {
    int64_t probe_ws, probe_ws_bytes, probe_ids, probe_scores, probe_count, pm, pair_ptr, pairs, mem_ws, mem_ws_bytes, item_ptr, lists,
        counts, total;
};

static int ivf_layout(const int64_t Q, const int32_t C, const int32_t k, const int32_t P, IvfLayout* L) {
    int64_t off = 0;
    auto take = [&](const int64_t bytes) {
        const int64_t at = off;
        off += (bytes + 15) / 16 * 16;
        return at;
    };
    const int64_t n_pairs = Q * P;
    int rc = gs_topk_ws_bytes(Q, C, P, &L->probe_ws_bytes);
    if (rc != GS_OK) return rc;
    rc = gs_kmeans_members_ws_bytes(std::max<int64_t>(n_pairs, 1), C, 0, &L->mem_ws_bytes);
    if (rc != GS_OK) return rc;
    L->probe_ws = take(L->probe_ws_bytes);
    L->probe_ids = take(n_pairs * 4);
    L->probe_scores = take(n_pairs * 4);
    L->probe_count = take(Q * 4);
    L->pm = take(n_pairs * 4);
    L->pair_ptr = take(((int64_t)C + 1) * 8);
    L->pairs = take(n_pairs * 4);
    L->mem_ws = take(L->mem_ws_bytes);
    L->item_ptr = take(((int64_t)C + 1) * 4);
    L->lists = take(n_pairs * topk_cap(k) * 8);
    L->counts = take(n_pairs * 4);
    L->total = off;
    return GS_OK;
}

#define IVF_MAX_Q ((int64_t)1 << 24)         // Q nprobe stays below 2^31 at nprobe = 128

static int ivf_check_sizes(const char* who, const int64_t Q, const int32_t C, const int32_t k, const int32_t P) {
    GS_REQUIRE(Q >= 0 && Q < IVF_MAX_Q, "%s: Q=%lld must lie in [0, 2^24); call it on chunks of the queries", who, (long long)Q);
    GS_REQUIRE(C >= 1 && C <= GS_KMEANS_MAX_K, "%s: n_clusters=%d must lie in [1, %d]", who, C, GS_KMEANS_MAX_K);
    GS_REQUIRE(k >= 1 && k <= GS_TOPK_MAX, "%s: k=%d must lie in [1, %d]", who, k, GS_TOPK_MAX);
    GS_REQUIRE(P >= 1 && P <= GS_IVF_MAX_PROBE && P <= C, "%s: nprobe=%d must lie in [1, min(%d, n_clusters=%d)]", who, P,
               GS_IVF_MAX_PROBE, C);
    return GS_OK;
}

extern "C" int gs_ivf_ws_bytes(int64_t Q, int32_t n_clusters, int32_t k, int32_t nprobe, int64_t* bytes_out_host) {
    GS_REQUIRE(bytes_out_host, "gs_ivf_ws_bytes: null result pointer");
    int rc = ivf_check_sizes("gs_ivf_ws_bytes", Q, n_clusters, k, nprobe);
    if (rc != GS_OK) return rc;
    IvfLayout L;
    rc = ivf_layout(Q, n_clusters, k, nprobe, &L);
    if (rc != GS_OK) return rc;
    *bytes_out_host = L.total;
    return GS_OK;
}

extern "C" int gs_ivf_search(const gs_ivf_desc* desc_host, void* stream) {
    GS_REQUIRE(desc_host, "gs_ivf_search: null descriptor");
    const gs_ivf_desc& q = *desc_host;
    GS_REQUIRE(q.n_rows >= 0 && q.n_rows <= 0x7fffffffll && q.n_cand >= 0 && q.n_list >= 0 && q.n_list <= 0x7fffffffll,
               "gs_ivf_search: bad sizes n_rows=%lld n_cand=%lld n_list=%lld", (long long)q.n_rows, (long long)q.n_cand,
               (long long)q.n_list);
    int rc = ivf_check_sizes("gs_ivf_search", q.Q, q.n_clusters, q.k, q.nprobe);
    if (rc != GS_OK) return rc;
    GS_REQUIRE(q.stop_after >= 0 && q.stop_after <= 5, "gs_ivf_search: stop_after=%d must lie in [0, 5]", q.stop_after);
    rc = rank_check_query("gs_ivf_search", q);
    if (rc != GS_OK || q.Q == 0) return rc;
    GS_CHECK_MAT(q.centers, q.ldc, "gs_ivf_search centers");
    GS_REQUIRE(q.ldc >= q.d, "gs_ivf_search: ld must be >= d");
    GS_REQUIRE(q.list_ptr && q.list_ids, "gs_ivf_search: list_ptr and list_ids must be non-null");
    GS_REQUIRE(q.ids && q.scores && q.count, "gs_ivf_search: ids, scores and count must be non-null");
    GS_REQUIRE(q.n_list == 0 || q.n_rows >= 1, "gs_ivf_search: the candidate table is empty (the lists name rows)");
    IvfLayout L;
    rc = ivf_layout(q.Q, q.n_clusters, q.k, q.nprobe, &L);
    if (rc != GS_OK) return rc;
    GS_REQUIRE(q.ws && (reinterpret_cast<uintptr_t>(q.ws) & 15u) == 0 && q.ws_bytes >= L.total,
               "gs_ivf_search: needs a 16-byte aligned workspace of %lld bytes (gs_ivf_ws_bytes), got %lld", (long long)L.total,
               (long long)q.ws_bytes);
    const hipStream_t st = (hipStream_t)stream;
    char* ws = reinterpret_cast<char*>(q.ws);
    const int P = q.nprobe, C = q.n_clusters;
    const int64_t n_pairs = q.Q * P;
    int32_t* probe_ids = reinterpret_cast<int32_t*>(ws + L.probe_ids);

    // 1 probe
    gs_topk_desc t = {};
    t.Xq = q.Xq; t.Zc = q.centers;
    t.ids = probe_ids; t.scores = reinterpret_cast<float*>(ws + L.probe_scores); t.count = reinterpret_cast<int32_t*>(ws + L.probe_count);
    t.ws = ws + L.probe_ws; t.ws_bytes = L.probe_ws_bytes;
    t.Q = q.Q; t.ldq = q.ldq; t.n_rows = C; t.n_cand = C; t.ldz = q.ldc;
    t.d = q.d; t.k = P;
    rc = gs_topk_select(&t, stream);
    if (rc != GS_OK) return rc;
    if (q.stop_after == 1) return GS_OK;

    // 2 group
    int32_t* pm = reinterpret_cast<int32_t*>(ws + L.pm);
    hipLaunchKernelGGL(ivf_pairs_kernel, dim3((unsigned)gs_ceil_div(q.Q, 256)), dim3(256), 0, st, probe_ids, q.Q, P, C, q.list_ptr, pm,
                       q.scanned);
    GS_LAUNCH_CHECK("ivf_pairs_kernel");
    gs_kmeans_members_desc m = {};
    m.assign = pm; m.rowptr = reinterpret_cast<int64_t*>(ws + L.pair_ptr); m.members = reinterpret_cast<int32_t*>(ws + L.pairs);
    m.ws = reinterpret_cast<int32_t*>(ws + L.mem_ws); m.ws_bytes = L.mem_ws_bytes;
    m.n = n_pairs; m.k = C;
    rc = gs_kmeans_members(&m, stream);
    if (rc != GS_OK) return rc;
    if (q.stop_after == 2) return GS_OK;

    // 3 plan
    int32_t* item_ptr = reinterpret_cast<int32_t*>(ws + L.item_ptr);
    hipLaunchKernelGGL(ivf_plan_kernel, dim3(1), dim3(256), 0, st, (const int64_t*)m.rowptr, C, item_ptr);
    GS_LAUNCH_CHECK("ivf_plan_kernel");
    if (q.stop_after == 3) return GS_OK;

    // 4 scan
    IvfArgs g;
    g.Xq = q.Xq; g.Zc = q.Zc; g.src = q.src; g.f_rowptr = q.f_rowptr; g.f_col = q.f_col;
    g.list_ptr = q.list_ptr; g.list_ids = q.list_ids;
    g.pair_ptr = m.rowptr; g.pairs = m.members; g.item_ptr = item_ptr;
    g.lists = reinterpret_cast<uint64_t*>(ws + L.lists);
    g.counts = reinterpret_cast<int32_t*>(ws + L.counts);
    g.Q = q.Q; g.n_pairs = n_pairs; g.ldq = q.ldq; g.n_rows = q.n_rows; g.ldz = q.ldz; g.f_nnz = q.f_nnz;
    g.n_cand = (int32_t)q.n_cand; g.n_list = (int32_t)q.n_list;
    g.d = q.d; g.k = q.k; g.cap = (int32_t)topk_cap(q.k); g.n_clusters = C;
    g.keep_src = (q.flags & GS_RANK_KEEP_SRC) ? 1 : 0;
    GS_HIP(hipMemsetAsync(g.counts, 0, (size_t)n_pairs * sizeof(int32_t), st));
    const int64_t blocks = n_pairs / RK_BM + C;          // >= sum over the clusters of ceil(pairs_c / 128)
    hipLaunchKernelGGL(ivf_scan_kernel, dim3((unsigned)blocks), dim3(256), 0, st, g);
    GS_LAUNCH_CHECK("ivf_scan_kernel");
    if (q.stop_after == 4) return GS_OK;

    // 5 merge
    return topk_merge_launch(g.lists, g.counts, q.Q, P, g.cap, q.k, q.ids, q.scores, q.count, st);
}
