// Lloyd's k-means over the rows of an embedding table: squared norms, the fused assignment (the sweep of gs_rank.hip with an
// argmin epilogue) and the stable grouping of rows by cluster.  The centroid update is gs_csr_reduce_fwd over the grouping.
//
//   s(i, j)   = <x_i, c_j> - 0.5f * csq[j]              x_i = X[rows ? rows[i] : i], c_j = C[j]
//   assign[i] = argmax_j s(i, j), an exact tie to the lowest j          (= argmin_j |x_i - c_j|^2)
//   dist[i]   = max(0, xsq[i] - 2 s(i, assign[i]))
//
// kmeans_assign_kernel.  One workgroup owns 128 table rows and sweeps ALL centroid tiles of 128; the K loop is the tile pipeline
// of gs_rank_dev.h (rank_first_loads, rank_k_loop: fp32 MFMA, BM = BN = 128, BK = 32, two LDS stages), so a (row, centroid)
// pair goes through the k-ordered chain of gs_rank_count and two bit-identical centroid rows score bit-equal.
//   Epilogue: after a tile's K loop the next tile's first two stages are requested, and under those loads every lane folds
// its 2 x 2 x 16 accumulator cells into a running (best score, id) per (tm, e) -- the 32 table rows a lane holds cells of;
// the two cells of one row (tn = 0, 1) are taken in ascending column, replacement is by strict `>` and
// the tiles ascend, so within a lane the lowest id of a tie survives.  Nothing is written per tile: no score, no key, no
// per-slice workspace.  After the last tile the 32 x 64 lane candidates of every row meet once in the (dead) stage buffers,
// two threads per row pick the best by (score descending, id ascending), and the same threads write assign and dist; the
// workgroup's sum of dist (fp64, butterfly per wave, then the four waves in order) and its count of assign[i] != prev[i] go
// to one 16-byte slot of the workspace.  kmeans_finish_kernel (one workgroup) adds the slots in workgroup order: 256
// contiguous runs, each in order, then the runs in order.  No atomics anywhere: bitwise repeatable.
//   Columns at and beyond k (the last tile's zero rows) take csq = +inf: their score is -inf and never wins.  A NaN score
// never wins either (`>` is false).
//
// kmeans_members: per-chunk histograms in LDS (one wave per chunk of `chunk` entries; integer ds_add), a scan over the chunks
// per cluster, a scan over the clusters, and an ordered re-walk in which a wave takes 64 entries at a time and ranks the
// lanes that share a cluster id by ballot (leader loop: one pass per distinct id among the 64).  Cluster j's run holds its
// members in ascending i whatever the chunk length: the result is uniquely defined.
//
// Resources (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage; quoted in profiles/eval_clusters.md):
// kmeans_assign_kernel 234 vector registers, 90 scalar, no scratch, no spill of either kind, 73,776 B of LDS (the two stage
// buffers of the sweep and 48 B of partial sums; gs_topk.hip: 77,824 B): two workgroups per CU under __launch_bounds__(256, 2).
// The running ids are kept as one byte (2 tile + tn) packed four to a register: with one int32 per row slot (32 registers
// instead of 8) the kernel took all 256 registers and spilled 3 of them to 16 B of scratch.  kmeans_finish_kernel 61
// registers, 4,096 B of LDS; kmeans_sqnorm_kernel 12, none; kmeans_hist_kernel 50 and kmeans_place_kernel 34, 16,384 B each
// (the k <= 4096 counters of one wave); kmeans_scan_chunks_kernel 6, none; kmeans_scan_k_kernel 26, 2,048 B.  No scratch in
// any of them.
#include "gs_rank_dev.h"

static_assert(sizeof(gs_kmeans_desc) == 128, "gs_kmeans_desc layout (mirrored by graphsage_amd/_lib.py)");
static_assert(sizeof(gs_kmeans_members_desc) == 72, "gs_kmeans_members_desc layout (mirrored by graphsage_amd/_lib.py)");
static_assert(GS_KMEANS_CHUNK % 64 == 0, "a chunk is whole rounds of one wave");

#define KM_LD 65                 // row stride of the (score, id) meeting place: 64 lane candidates per row, padded
static_assert(2 * RK_BM * KM_LD <= 2 * RK_STAGE_FLOATS, "the candidates meet in the two stage buffers");

struct KmArgs {
    const float* X; const int32_t* rows; const float* C; const float* csq; const float* xsq; const int32_t* prev;
    int32_t* assign; float* dist; double* ws;
    int64_t n, n_rows, ld, ldc;
    int32_t k, d, tiles_n;
};

__device__ __forceinline__ double km_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// (256, 2): a budget of 256 registers per lane, two workgroups per CU
__global__ __launch_bounds__(256, 2) void kmeans_assign_kernel(const KmArgs g) {
    constexpr int BM = RK_BM, BN = RK_BN;
    __shared__ __attribute__((aligned(16))) float smem[2 * RK_STAGE_FLOATS];
    __shared__ double dsumS[4];
    __shared__ int32_t csumS[4];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;
    const int64_t m0 = (int64_t)blockIdx.x * BM;
    const int d = g.d;

    // ---- operand rows of this thread: 4 table rows (fixed), 4 centroid rows (per tile); 8 threads x float4 span BK
    const int srow = tid >> 3, sk = (tid & 7) * 4;
    RankOperand A, B;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int64_t i = m0 + p * 32 + srow;
        A.ok[p] = i < g.n;
        int64_t r = 0;
        if (A.ok[p]) {
            r = g.rows ? (int64_t)g.rows[i] : i;
            r = r < 0 ? 0 : (r >= g.n_rows ? g.n_rows - 1 : r);      // the caller checked; never a stray read
        }
        A.row[p] = g.X + r * g.ld + sk;
    }

    RankRegs ra0, rb0, ra1, rb1;
    auto first_loads = [&](const int tile) {
        rank_rows(B, g.C, g.ldc, (int64_t)tile * BN, g.k);
        rank_first_loads(A, B, d, ra0, rb0, ra1, rb1);
    };
    first_loads(0);

    // running best of the 32 table rows this lane holds cells of: row(tm, e) = wm 64 + tm 32 + rank_acc_row(e, lh)
    // The id is kept as the byte 2 tile + tn (k <= 4096: below 64), four to a register: 8 registers where the ids would take 32.
    float best[2][16];
    uint32_t bcode[2][4];
#pragma unroll
    for (int tm = 0; tm < 2; ++tm) {
#pragma unroll
        for (int e = 0; e < 16; ++e) best[tm][e] = -__builtin_inff();
#pragma unroll
        for (int w = 0; w < 4; ++w) bcode[tm][w] = 0u;
    }

    for (int tile = 0; tile < g.tiles_n; ++tile) {
        const int c0 = tile * BN + wn * 64 + l31, c1 = c0 + 32;      // the two centroids of this lane's cells (tn = 0, 1)
        const float h0 = c0 < g.k ? 0.5f * g.csq[c0] : __builtin_inff();
        const float h1 = c1 < g.k ? 0.5f * g.csq[c1] : __builtin_inff();

        f32x16 acc[2][2];
        rank_k_loop(A, B, d, smem, ra0, rb0, ra1, rb1, wm, wn, l31, lh, acc);

        if (tile + 1 < g.tiles_n) first_loads(tile + 1);

        // ---- epilogue: registers only
        const uint32_t code0 = 2u * (uint32_t)tile;
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float s0 = acc[tm][0][e] - h0;
                const float s1 = acc[tm][1][e] - h1;
                const int sh = 8 * (e & 3);
                const uint32_t keep = ~(0xffu << sh);
                if (s0 > best[tm][e]) { best[tm][e] = s0; bcode[tm][e >> 2] = (bcode[tm][e >> 2] & keep) | (code0 << sh); }
                if (s1 > best[tm][e]) { best[tm][e] = s1; bcode[tm][e >> 2] = (bcode[tm][e >> 2] & keep) | ((code0 + 1u) << sh); }
            }
        // the stage buffers change hands here (an odd stage count ends on the buffer that the next tile stores first)
        __syncthreads();
    }

    // ---- the 64 lane candidates of every row meet in the stage buffers: slot = wn 32 + l31
    float* sc = smem;
    int32_t* si = reinterpret_cast<int32_t*>(smem + BM * KM_LD);
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int r = wm * 64 + tm * 32 + rank_acc_row(e, lh);
            sc[r * KM_LD + wn * 32 + l31] = best[tm][e];
            const int code = (int)((bcode[tm][e >> 2] >> (8 * (e & 3))) & 0xffu);
            si[r * KM_LD + wn * 32 + l31] = (code >> 1) * BN + wn * 64 + (code & 1) * 32 + l31;
        }
    __syncthreads();

    // two threads per row, 32 slots each, then the pair; order: score descending, id ascending
    const int r = tid >> 1, half = tid & 1;
    float b = -__builtin_inff();
    int32_t id = 0x7fffffff;
#pragma unroll 8
    for (int j = 0; j < 32; ++j) {
        const float s = sc[r * KM_LD + half * 32 + j];
        const int32_t c = si[r * KM_LD + half * 32 + j];
        if (s > b || (s == b && c < id)) { b = s; id = c; }
    }
    {
        const float s = __shfl_xor(b, 1, 64);
        const int32_t c = __shfl_xor(id, 1, 64);
        if (s > b || (s == b && c < id)) { b = s; id = c; }
    }
    if (id >= g.k) id = 0;                       // every score NaN: nothing ever won

    const int64_t i = m0 + r;
    double dd = 0.0;
    bool ch = false;
    if (half == 0 && i < g.n) {
        g.assign[i] = id;
        const float xs = g.xsq ? g.xsq[i] : 0.f;
        const float dv = fmaxf(0.f, xs - 2.f * b);
        if (g.dist) g.dist[i] = dv;
        dd = (double)dv;
        ch = g.prev ? g.prev[i] != id : false;
    }
    dd = km_wave_sum(dd);
    const int cc = __popcll(__ballot(ch));
    if (lane == 0) {
        dsumS[wave] = dd;
        csumS[wave] = cc;
    }
    __syncthreads();
    if (tid == 0) {
        g.ws[2 * (int64_t)blockIdx.x] = (dsumS[0] + dsumS[1]) + (dsumS[2] + dsumS[3]);
        reinterpret_cast<int64_t*>(g.ws)[2 * (int64_t)blockIdx.x + 1] = (int64_t)((csumS[0] + csumS[1]) + (csumS[2] + csumS[3]));
    }
}

// one workgroup: the slots in workgroup order (256 contiguous runs, each in order, then the runs in order)
__global__ __launch_bounds__(256) void kmeans_finish_kernel(const double* __restrict__ ws, const int64_t wgs, void* stats) {
    __shared__ double dS[256];
    __shared__ int64_t cS[256];
    const int64_t run = gs_ceil_div(wgs, 256);
    const int64_t b0 = (int64_t)threadIdx.x * run, b1 = min(b0 + run, wgs);
    double dsum = 0.0;
    int64_t csum = 0;
    for (int64_t b = b0; b < b1; ++b) {
        dsum += ws[2 * b];
        csum += reinterpret_cast<const int64_t*>(ws)[2 * b + 1];
    }
    dS[threadIdx.x] = dsum;
    cS[threadIdx.x] = csum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double dt = 0.0;
        int64_t ct = 0;
        for (int t = 0; t < 256; ++t) {
            dt += dS[t];
            ct += cS[t];
        }
        reinterpret_cast<double*>(stats)[0] = dt;
        reinterpret_cast<int64_t*>(stats)[1] = ct;
    }
}

// one wave per row: lane l adds the squares of columns 4 l + 256 c, c ascending, as one fmaf chain; then the butterfly
__global__ __launch_bounds__(256) void kmeans_sqnorm_kernel(const float* __restrict__ X, const int64_t ld, const int64_t n_rows,
                                                           const int32_t* __restrict__ rows, const int64_t n, const int d,
                                                           float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;                          // wave-uniform
    int64_t r = rows ? (int64_t)rows[i] : i;
    r = r < 0 ? 0 : (r >= n_rows ? n_rows - 1 : r);
    const float* x = X + r * ld;
    float s = 0.f;
    for (int c = lane * 4; c < d; c += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + c);
        s = fmaf(v.x, v.x, s);
        s = fmaf(v.y, v.y, s);
        s = fmaf(v.z, v.z, s);
        s = fmaf(v.w, v.w, s);
    }
    s = gs_wave_sum(s);
    if (lane == 0) out[i] = s;
}

// ---------------------------------------------------------------------------------------------------------------
// members: chunk b = entries [b chunk, (b + 1) chunk), one wave each

// hist[b][j] = #{i in chunk b : assign[i] == j}
__global__ __launch_bounds__(64) void kmeans_hist_kernel(const int32_t* __restrict__ assign, const int64_t n, const int k,
                                                        const int chunk, int32_t* __restrict__ hist) {
    __shared__ int32_t cnt[GS_KMEANS_MAX_K];
    const int lane = threadIdx.x;
    for (int j = lane; j < k; j += 64) cnt[j] = 0;
    __syncthreads();
    const int64_t i0 = (int64_t)blockIdx.x * chunk, i1 = min(i0 + chunk, n);
    for (int64_t i = i0 + lane; i < i1; i += 64) {
        const int32_t a = assign[i];
        if (a >= 0 && a < k) atomicAdd(&cnt[a], 1);          // LDS, integers: the count does not depend on the order
    }
    __syncthreads();
    int32_t* h = hist + (int64_t)blockIdx.x * k;
    for (int j = lane; j < k; j += 64) h[j] = cnt[j];
}

// one thread per cluster: hist[.][j] becomes its exclusive prefix over the chunks; total[j] = the cluster's size
__global__ __launch_bounds__(256) void kmeans_scan_chunks_kernel(int32_t* __restrict__ hist, const int64_t chunks, const int k,
                                                               int64_t* __restrict__ rowptr) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= k) return;
    int32_t run = 0;
    for (int64_t b = 0; b < chunks; ++b) {
        const int32_t c = hist[b * k + j];
        hist[b * k + j] = run;
        run += c;
    }
    rowptr[j + 1] = run;                         // the size for now; kmeans_scan_k_kernel turns the sizes into offsets
}

// one workgroup: rowptr[0] = 0, rowptr[j + 1] = sizes[0] + .. + sizes[j]   (k <= 4096: 16 per thread)
__global__ __launch_bounds__(256) void kmeans_scan_k_kernel(int64_t* __restrict__ rowptr, const int k) {
    __shared__ int64_t part[256];
    const int per = (k + 255) / 256;
    const int j0 = threadIdx.x * per, j1 = min(j0 + per, k);
    int64_t s = 0;
    for (int j = j0; j < j1; ++j) s += rowptr[j + 1];
    part[threadIdx.x] = s;
    __syncthreads();
    int64_t base = 0;
    for (int t = 0; t < (int)threadIdx.x; ++t) base += part[t];
    for (int j = j0; j < j1; ++j) {
        base += rowptr[j + 1];
        rowptr[j + 1] = base;
    }
    if (threadIdx.x == 0) rowptr[0] = 0;
}

// the ordered re-walk: position = rowptr[j] + (members of j in earlier chunks) + (members of j earlier in this chunk)
__global__ __launch_bounds__(64) void kmeans_place_kernel(const int32_t* __restrict__ assign, const int32_t* __restrict__ rows,
                                                         const int64_t n, const int k, const int chunk,
                                                         const int32_t* __restrict__ hist, const int64_t* __restrict__ rowptr,
                                                         int32_t* __restrict__ members) {
    __shared__ int32_t cnt[GS_KMEANS_MAX_K];
    const int lane = threadIdx.x;
    const int32_t* h = hist + (int64_t)blockIdx.x * k;
    for (int j = lane; j < k; j += 64) cnt[j] = h[j];
    __syncthreads();
    const int64_t i0 = (int64_t)blockIdx.x * chunk, i1 = min(i0 + chunk, n);
    const uint64_t below = (1ull << lane) - 1ull;
    for (int64_t ib = i0; ib < i1; ib += 64) {               // uniform
        const int64_t i = ib + lane;
        int32_t a = -1;
        if (i < i1) a = assign[i];
        const bool valid = a >= 0 && a < k;
        uint64_t todo = __ballot(valid);
        int32_t pos = 0;
        while (todo != 0ull) {                               // one pass per distinct id among the 64 (uniform)
            const int leader = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)todo) - 1);
            const int32_t kk = __builtin_amdgcn_readlane(a, leader);
            const uint64_t m = __ballot(valid && a == kk);
            const int32_t base = cnt[kk];                    // one address for the wave
            if (valid && a == kk) pos = base + __popcll(m & below);
            __builtin_amdgcn_wave_barrier();
            if (lane == leader) cnt[kk] = base + __popcll(m);
            __builtin_amdgcn_wave_barrier();
            todo &= ~m;
        }
        if (valid) {
            const int64_t p = rowptr[a] + pos;
            if (p >= 0 && p < n) members[p] = rows ? rows[i] : (int32_t)i;
        }
    }
}

extern "C" int gs_kmeans_sqnorm(const float* X, int64_t ld, int64_t n_rows, const int32_t* rows, int64_t n, int32_t d, float* out,
                                void* stream) {
    GS_REQUIRE(n >= 0 && n_rows >= 0 && n < (1ll << 31), "gs_kmeans_sqnorm: bad sizes n=%lld n_rows=%lld", (long long)n,
               (long long)n_rows);
    GS_REQUIRE(d >= 4 && d <= 1024 && (d & 3) == 0, "gs_kmeans_sqnorm: d=%d must be a multiple of 4 in [4, 1024]", d);
    if (n == 0) return GS_OK;
    GS_CHECK_MAT(X, ld, "gs_kmeans_sqnorm X");
    GS_REQUIRE(ld >= d && out, "gs_kmeans_sqnorm: ld must be >= d and out non-null");
    GS_REQUIRE(n_rows >= 1 && (rows || n <= n_rows), "gs_kmeans_sqnorm: %lld rows asked of a table of %lld", (long long)n,
               (long long)n_rows);
    hipLaunchKernelGGL(kmeans_sqnorm_kernel, dim3((unsigned)gs_ceil_div(n, 4)), dim3(256), 0, (hipStream_t)stream, X, ld, n_rows,
                       rows, n, (int)d, out);
    GS_LAUNCH_CHECK("kmeans_sqnorm_kernel");
    return GS_OK;
}

extern "C" int gs_kmeans_assign_ws_bytes(int64_t n, int64_t* bytes_out_host) {
    GS_REQUIRE(bytes_out_host && n >= 0 && n < (1ll << 31), "gs_kmeans_assign_ws_bytes: bad args");
    *bytes_out_host = 16 * gs_ceil_div(n, RK_BM);
    return GS_OK;
}

extern "C" int gs_kmeans_assign(const gs_kmeans_desc* desc_host, void* stream) {
    GS_REQUIRE(desc_host, "gs_kmeans_assign: null descriptor");
    const gs_kmeans_desc& q = *desc_host;
    GS_REQUIRE(q.n >= 1 && q.n < (1ll << 31) && q.n_rows >= 1, "gs_kmeans_assign: bad sizes n=%lld n_rows=%lld", (long long)q.n,
               (long long)q.n_rows);
    GS_REQUIRE(q.k >= 1 && q.k <= GS_KMEANS_MAX_K, "gs_kmeans_assign: k=%d must lie in [1, %d]", q.k, GS_KMEANS_MAX_K);
    GS_REQUIRE(q.d >= 4 && q.d <= 1024 && (q.d & 3) == 0, "gs_kmeans_assign: d=%d must be a multiple of 4 in [4, 1024]", q.d);
    GS_CHECK_MAT(q.X, q.ld, "gs_kmeans_assign X");
    GS_CHECK_MAT(q.C, q.ldc, "gs_kmeans_assign C");
    GS_REQUIRE(q.ld >= q.d && q.ldc >= q.d, "gs_kmeans_assign: ld must be >= d");
    GS_REQUIRE(q.rows || q.n <= q.n_rows, "gs_kmeans_assign: %lld rows asked of a table of %lld", (long long)q.n,
               (long long)q.n_rows);
    GS_REQUIRE(q.csq && q.assign && q.stats, "gs_kmeans_assign: csq, assign and stats must be non-null");
    const int64_t wgs = gs_ceil_div(q.n, RK_BM);
    GS_REQUIRE(q.ws && (reinterpret_cast<uintptr_t>(q.ws) & 7u) == 0 && (reinterpret_cast<uintptr_t>(q.stats) & 7u) == 0 &&
                   q.ws_bytes >= 16 * wgs,
               "gs_kmeans_assign: needs 8-byte aligned stats and a workspace of %lld bytes (gs_kmeans_assign_ws_bytes), got %lld",
               (long long)(16 * wgs), (long long)q.ws_bytes);
    KmArgs g;
    g.X = q.X; g.rows = q.rows; g.C = q.C; g.csq = q.csq; g.xsq = q.xsq; g.prev = q.prev;
    g.assign = q.assign; g.dist = q.dist; g.ws = reinterpret_cast<double*>(q.ws);
    g.n = q.n; g.n_rows = q.n_rows; g.ld = q.ld; g.ldc = q.ldc;
    g.k = q.k; g.d = q.d; g.tiles_n = (int32_t)gs_ceil_div(q.k, RK_BN);
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(kmeans_assign_kernel, dim3((unsigned)wgs), dim3(256), 0, st, g);
    GS_LAUNCH_CHECK("kmeans_assign_kernel");
    hipLaunchKernelGGL(kmeans_finish_kernel, dim3(1), dim3(256), 0, st, g.ws, wgs, q.stats);
    GS_LAUNCH_CHECK("kmeans_finish_kernel");
    return GS_OK;
}

static int km_chunk(const int32_t chunk) { return chunk == 0 ? GS_KMEANS_CHUNK : chunk; }

extern "C" int gs_kmeans_members_ws_bytes(int64_t n, int32_t k, int32_t chunk, int64_t* bytes_out_host) {
    GS_REQUIRE(bytes_out_host && n >= 0 && n < (1ll << 31) && k >= 1 && k <= GS_KMEANS_MAX_K && chunk >= 0 && chunk % 64 == 0,
               "gs_kmeans_members_ws_bytes: bad args n=%lld k=%d chunk=%d", (long long)n, k, chunk);
    *bytes_out_host = gs_ceil_div(n, km_chunk(chunk)) * (int64_t)k * (int64_t)sizeof(int32_t);
    return GS_OK;
}

extern "C" int gs_kmeans_members(const gs_kmeans_members_desc* desc_host, void* stream) {
    GS_REQUIRE(desc_host, "gs_kmeans_members: null descriptor");
    const gs_kmeans_members_desc& q = *desc_host;
    GS_REQUIRE(q.n >= 1 && q.n < (1ll << 31), "gs_kmeans_members: n=%lld must lie in [1, 2^31)", (long long)q.n);
    GS_REQUIRE(q.k >= 1 && q.k <= GS_KMEANS_MAX_K, "gs_kmeans_members: k=%d must lie in [1, %d]", q.k, GS_KMEANS_MAX_K);
    GS_REQUIRE(q.chunk >= 0 && q.chunk % 64 == 0 && q.reserved_ == 0,
               "gs_kmeans_members: chunk=%d must be 0 or a positive multiple of 64, reserved_ 0", q.chunk);
    GS_REQUIRE(q.assign && q.rowptr && q.members, "gs_kmeans_members: assign, rowptr and members must be non-null");
    const int chunk = km_chunk(q.chunk);
    const int64_t chunks = gs_ceil_div(q.n, chunk);
    const int64_t need = chunks * (int64_t)q.k * (int64_t)sizeof(int32_t);
    GS_REQUIRE(q.ws && (reinterpret_cast<uintptr_t>(q.ws) & 3u) == 0 && q.ws_bytes >= need,
               "gs_kmeans_members: needs a workspace of %lld bytes (gs_kmeans_members_ws_bytes), got %lld", (long long)need,
               (long long)q.ws_bytes);
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(kmeans_hist_kernel, dim3((unsigned)chunks), dim3(64), 0, st, q.assign, q.n, (int)q.k, chunk, q.ws);
    GS_LAUNCH_CHECK("kmeans_hist_kernel");
    hipLaunchKernelGGL(kmeans_scan_chunks_kernel, dim3((unsigned)gs_ceil_div(q.k, 256)), dim3(256), 0, st, q.ws, chunks, (int)q.k,
                       q.rowptr);
    GS_LAUNCH_CHECK("kmeans_scan_chunks_kernel");
    hipLaunchKernelGGL(kmeans_scan_k_kernel, dim3(1), dim3(256), 0, st, q.rowptr, (int)q.k);
    GS_LAUNCH_CHECK("kmeans_scan_k_kernel");
    hipLaunchKernelGGL(kmeans_place_kernel, dim3((unsigned)chunks), dim3(64), 0, st, q.assign, q.rows, q.n, (int)q.k, chunk,
                       (const int32_t*)q.ws, (const int64_t*)q.rowptr, q.members);
    GS_LAUNCH_CHECK("kmeans_place_kernel");
    return GS_OK;
}
