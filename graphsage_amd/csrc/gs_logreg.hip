// One-vs-rest logistic regression on rows of an embedding table: one loss-and-gradient evaluation per call, the two
// contractions fused over the same LDS tile (no logit and no residual is ever written to memory).
//
//   z[i][k]  = <X[rows[i]], W[:, k]> + b[k]                         s[i][k] = +1 / -1 (the label), m = s z
//   loss[k]  = sum_i max(-m, 0) + log1p(exp(-|m|))
//   gb[k]    = sum_i r[i][k],   r = -s sigma(-m)                    (sigma(-m) = e / (1 + e) for m >= 0, 1 / (1 + e) else,
//   gW[j][k] = sum_i X[rows[i]][j] r[i][k]                           e = exp(-|m|): no overflow at either end)
//
// Tiling: 256 threads = 4 waves; a workgroup owns a contiguous run of 32-row tiles (the same for every evaluation of one
// (n, d, c): gs_logreg_plan).  Per tile
//   1. the gathered rows go to LDS once, [32][d + 4] (8 threads x float4 per row, rows >= n as zeros);
//   2. wave w < ceil(c / 32) forms the 32 x 32 logits of class block w on v_mfma_f32_32x32x2_f32: A from the LDS tile
//      (ds_read_b128 along d), B = W read along the classes (lanes contiguous, L2-resident);
//   3. the epilogue turns them into loss terms and residuals in registers; the residuals are parked in LDS [32][128 + 4];
//   4. the ceil(c / 32) x ceil(d / 32) output tiles of X^T R are dealt round-robin to the four waves (at most NT = 8 each,
//      128 accumulator registers, held across all of the workgroup's row tiles); A = the LDS tile read along d (stride 1
//      across lanes), B = the parked residuals.  When ceil(c / 32) * ceil(d / 32) > 32 the d blocks are cut over gridDim.y
//      (every y recomputes the logits; y = 0 alone writes loss and gb).
// C/D layout of the 32 x 32 MFMA: col = lane & 31, row = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5); the k of MFMA i in a group of
// four is k0 + 4 * (lane >> 5) + i for both operands.
//
// Every workgroup writes ONE fp32 partial [loss c][gb c][gW d * c] to the workspace; logreg_sum_kernel adds the partials in
// workgroup order in fp64.  No atomics, no dependence between workgroups, a fixed order everywhere: bitwise repeatable.
// GS_LOGREG_PREDICT runs steps 1-3 only: argmax over the classes (lowest class id on a tie; within a wave by shuffles over
// the 32 lanes of a half, across waves through LDS), z > 0 per label, and the loss where labels are given.
//
// gs_logreg_eval_joined is the same evaluation on rows joined from two tables and standardised in step 1 (the raw-feature and
// features + embeddings inputs of eval_scripts/); steps 2-4 and both launches are shared (gs_logreg_dev.h).  gs_col_moments, at
// the end of this file, gives the scaler its column means and variances.
#include "gs_logreg_dev.h"

static_assert(sizeof(gs_logreg_desc) == 168, "gs_logreg_desc layout (mirrored by graphsage_amd/_lib.py)");
static_assert(sizeof(gs_logreg_joined_desc) == 224, "gs_logreg_joined_desc layout (mirrored by graphsage_amd/_lib.py)");

// (256, 2) up to four gradient tiles per wave: a budget of 256 registers per lane, two workgroups per CU; measured at the
// Reddit shape (d = 256, c = 41, four tiles) that is 0.31 ms per evaluation against 0.44 ms with 512 registers and one
// workgroup per CU (profiles/eval_classifier.md).  With the body in gs_logreg_dev.h the compiler reports 118 / 155 / 227
// registers at one / two / four tiles and nothing spilled (the joined staging adds 5 or 6); eight tiles (128 accumulator
// registers) take the 512, nothing spilled.
template <int NT, bool FIT>
__global__ __launch_bounds__(256, NT <= 4 ? 2 : 1) void logreg_kernel(const LogregArgs g) {
    lr_body<NT, FIT, false>(g);
}

// The joined form: the same body behind the two-source, standardising staging (gs_logreg_dev.h).  The WHOLE row of the tile
// stays in LDS, [32][d + 4] up to d = 1024: 131,584 B, with the residuals 148,480 B -- one workgroup per CU above d = 504
// (two need 2 * (32 * (d + 4) + 4224) * 4 <= 163,840).  The other form, staging the row in column chunks, keeps two
// workgroups per CU but reads every row twice (the residuals need the whole logit before any X^T R tile can start); it is
// the build under benchmarks/variants/ and its measurement is in profiles/eval_classifier_features.md.
template <int NT, bool FIT>
__global__ __launch_bounds__(256, NT <= 4 ? 2 : 1) void logreg_joined_kernel(const LogregArgs g) {
    lr_body<NT, FIT, true>(g);
}

// out[j] = the fp64 sum over the workgroups' partials, in workgroup order; j runs over [loss c][gb c][gW d * c]
__global__ __launch_bounds__(256) void logreg_sum_kernel(const float* __restrict__ ws, const int64_t stride, const int wgs,
                                                         const int64_t count, const int c, double* __restrict__ loss,
                                                         double* __restrict__ gb, double* __restrict__ gW) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= count) return;
    double s = 0.0;
#pragma unroll 8
    for (int w = 0; w < wgs; ++w) s += (double)ws[(int64_t)w * stride + j];
    if (j < c) loss[j] = s;
    else if (j < 2 * c) gb[j - c] = s;
    else gW[j - 2 * c] = s;
}

static int logreg_check_shape(const char* who, const int64_t n, const int32_t d, const int32_t c, const int32_t max_d) {
    GS_REQUIRE(n >= 1 && n <= (1ll << 40), "%s: n=%lld must be at least 1", who, (long long)n);
    GS_REQUIRE(d >= 4 && d <= max_d && (d & 3) == 0, "%s: d=%d must be a multiple of 4 in [4, %d]", who, d, max_d);
    GS_REQUIRE(c >= 1 && c <= GS_LOGREG_MAX_C, "%s: c=%d must lie in [1, %d]", who, c, GS_LOGREG_MAX_C);
    return GS_OK;
}

static int logreg_ws_bytes(const char* who, const int64_t n, const int32_t d, const int32_t c, const int32_t max_d,
                           int64_t* bytes_out_host) {
    GS_REQUIRE(bytes_out_host, "%s: null output", who);
    if (int rc = logreg_check_shape(who, n, d, c, max_d)) return rc;
    int64_t tiles, tpw, wgs;
    logreg_plan(n, &tiles, &tpw, &wgs);
    *bytes_out_host = wgs * (2 * (int64_t)c + (int64_t)d * c) * (int64_t)sizeof(float);
    return GS_OK;
}

extern "C" int gs_logreg_ws_bytes(int64_t n, int32_t d, int32_t c, int64_t* bytes_out_host) {
    return logreg_ws_bytes("gs_logreg_ws_bytes", n, d, c, GS_LOGREG_MAX_D, bytes_out_host);
}

extern "C" int gs_logreg_joined_ws_bytes(int64_t n, int32_t d, int32_t c, int64_t* bytes_out_host) {
    return logreg_ws_bytes("gs_logreg_joined_ws_bytes", n, d, c, GS_LOGREG_JOINED_MAX_D, bytes_out_host);
}

template <int NT, bool FIT, bool JOINED>
static int logreg_launch(const LogregArgs& g, const dim3 grid, const size_t lds, const hipStream_t st) {
    if (JOINED) {
        GS_LDS_ATTR(LR_LDS_BYTES(GS_LOGREG_JOINED_MAX_D, true), logreg_joined_kernel<NT, FIT>);
        hipLaunchKernelGGL((logreg_joined_kernel<NT, FIT>), grid, dim3(256), lds, st, g);
        GS_LAUNCH_CHECK("logreg_joined_kernel");
    } else {
        GS_LDS_ATTR(LR_LDS_BYTES(GS_LOGREG_MAX_D, true), logreg_kernel<NT, FIT>);
        hipLaunchKernelGGL((logreg_kernel<NT, FIT>), grid, dim3(256), lds, st, g);
        GS_LAUNCH_CHECK("logreg_kernel");
    }
    return GS_OK;
}

// What the two descriptors share once their sources are checked: the parameters, the labels, the outputs, the workspace.
struct LogregCall {
    const float* W; const float* b; const int32_t* y_class; const uint8_t* y_multi;
    double* loss; double* gW; double* gb; int32_t* pred_class; uint8_t* pred_multi; void* ws;
    int64_t n, ldw, ldy, ldp, ws_bytes;
    int32_t d, c, mode;
};

static int logreg_check_call(const char* who, const LogregCall& q) {
    const bool fit = q.mode == GS_LOGREG_FIT;
    GS_REQUIRE(q.W && q.b && q.ldw >= q.c, "%s: W and b must be non-null, ldw=%lld >= c=%d", who, (long long)q.ldw, q.c);
    const bool labelled = q.y_class || q.y_multi;
    GS_REQUIRE(!(q.y_class && q.y_multi), "%s: y_class and y_multi exclude each other", who);
    GS_REQUIRE(!q.y_multi || q.ldy >= q.c, "%s: ldy=%lld must be >= c=%d", who, (long long)q.ldy, q.c);
    if (fit) {
        GS_REQUIRE(labelled, "%s: FIT needs y_class or y_multi", who);
        GS_REQUIRE(q.loss && q.gW && q.gb, "%s: FIT writes loss, gW and gb; none may be null", who);
        GS_REQUIRE(!q.pred_class && !q.pred_multi, "%s: predictions are written in PREDICT mode only", who);
    } else {
        GS_REQUIRE(!q.gW && !q.gb, "%s: gW and gb are written in FIT mode only", who);
        GS_REQUIRE(!q.loss || labelled, "%s: a loss needs labels", who);
        GS_REQUIRE(q.pred_class || q.pred_multi || q.loss, "%s: PREDICT has nothing to write", who);
        GS_REQUIRE(!q.pred_multi || q.ldp >= q.c, "%s: ldp=%lld must be >= c=%d", who, (long long)q.ldp, q.c);
    }
    if (q.loss) {
        int64_t tiles, tpw, wgs;
        logreg_plan(q.n, &tiles, &tpw, &wgs);
        const int64_t need = wgs * (2 * (int64_t)q.c + (int64_t)q.d * q.c) * (int64_t)sizeof(float);
        GS_REQUIRE(q.ws && (reinterpret_cast<uintptr_t>(q.ws) & 7u) == 0 && q.ws_bytes >= need,
                   "%s: needs an 8-byte aligned workspace of %lld bytes (%s), got %lld", who, (long long)need,
                   q.d > GS_LOGREG_MAX_D ? "gs_logreg_joined_ws_bytes" : "gs_logreg_ws_bytes", (long long)q.ws_bytes);
        GS_REQUIRE((reinterpret_cast<uintptr_t>(q.loss) & 7u) == 0 && (reinterpret_cast<uintptr_t>(q.gW) & 7u) == 0 &&
                   (reinterpret_cast<uintptr_t>(q.gb) & 7u) == 0, "%s: the fp64 outputs must be 8-byte aligned", who);
    }
    return GS_OK;
}

// g holds the sources; the rest comes from q.  Both launches of one evaluation.
template <bool JOINED>
static int logreg_enqueue(LogregArgs& g, const LogregCall& q, const hipStream_t st) {
    const bool fit = q.mode == GS_LOGREG_FIT;
    int64_t tiles, tpw, wgs;
    logreg_plan(q.n, &tiles, &tpw, &wgs);
    const int64_t stride = 2 * (int64_t)q.c + (int64_t)q.d * q.c;
    const bool want_loss = q.loss != nullptr;
    g.W = q.W; g.b = q.b; g.y_class = q.y_class; g.y_multi = q.y_multi;
    g.pred_class = q.pred_class; g.pred_multi = q.pred_multi; g.ws = reinterpret_cast<float*>(q.ws);
    g.n = q.n; g.ldw = q.ldw; g.ldy = q.ldy; g.ldp = q.ldp;
    g.tiles = tiles; g.tiles_per_wg = tpw; g.ws_stride = stride;
    g.d = q.d; g.c = q.c; g.cb_n = (int32_t)gs_ceil_div(q.c, 32); g.db_n = (int32_t)gs_ceil_div(q.d, 32);
    g.dbw = fit ? std::min<int32_t>(g.db_n, 4 * LR_MAX_NT / g.cb_n) : g.db_n;
    g.want_loss = want_loss ? 1 : 0;
    const int y_blocks = fit ? (int)gs_ceil_div(g.db_n, g.dbw) : 1;
    const int per_wave = (int)gs_ceil_div((int64_t)g.cb_n * g.dbw, 4);
    const dim3 grid((unsigned)wgs, (unsigned)y_blocks);
    const size_t lds = LR_LDS_BYTES(q.d, fit);
    int rc;
    if (!fit) rc = logreg_launch<1, false, JOINED>(g, grid, lds, st);
    else if (per_wave <= 1) rc = logreg_launch<1, true, JOINED>(g, grid, lds, st);
    else if (per_wave <= 2) rc = logreg_launch<2, true, JOINED>(g, grid, lds, st);
    else if (per_wave <= 4) rc = logreg_launch<4, true, JOINED>(g, grid, lds, st);
    else rc = logreg_launch<LR_MAX_NT, true, JOINED>(g, grid, lds, st);
    if (rc) return rc;
    if (want_loss) {
        const int64_t count = fit ? stride : q.c;
        hipLaunchKernelGGL(logreg_sum_kernel, dim3((unsigned)gs_ceil_div(count, 256)), dim3(256), 0, st, g.ws, stride, (int)wgs,
                           count, (int)q.c, q.loss, q.gb, q.gW);
        GS_LAUNCH_CHECK("logreg_sum_kernel");
    }
    return GS_OK;
}

extern "C" int gs_logreg_eval(const gs_logreg_desc* desc_host, void* stream) {
    const char* who = "gs_logreg_eval";
    GS_REQUIRE(desc_host, "%s: null descriptor", who);
    const gs_logreg_desc& q = *desc_host;
    GS_REQUIRE(q.mode == GS_LOGREG_FIT || q.mode == GS_LOGREG_PREDICT, "%s: unknown mode %d", who, q.mode);
    GS_REQUIRE(q.flags == 0, "%s: unknown flags 0x%x", who, (unsigned)q.flags);
    if (int rc = logreg_check_shape(who, q.n, q.d, q.c, GS_LOGREG_MAX_D)) return rc;
    GS_REQUIRE(q.n_rows >= 1 && q.n_rows <= 0x7fffffffll, "%s: n_rows=%lld must lie in [1, 2^31)", who, (long long)q.n_rows);
    GS_CHECK_MAT(q.X, q.ldx, "gs_logreg_eval X");
    GS_REQUIRE(q.ldx >= q.d, "%s: ldx=%lld must be >= d=%d", who, (long long)q.ldx, q.d);
    GS_REQUIRE(q.rows || q.n <= q.n_rows, "%s: without rows, n=%lld must not exceed n_rows=%lld", who, (long long)q.n,
               (long long)q.n_rows);
    const LogregCall k = {q.W, q.b, q.y_class, q.y_multi, q.loss, q.gW, q.gb, q.pred_class, q.pred_multi, q.ws,
                          q.n, q.ldw, q.ldy, q.ldp, q.ws_bytes, q.d, q.c, q.mode};
    if (int rc = logreg_check_call(who, k)) return rc;
    LogregArgs g = {};
    g.X = q.X; g.rows = q.rows; g.n_rows = q.n_rows; g.ldx = q.ldx; g.da = q.d;
    return logreg_enqueue<false>(g, k, (hipStream_t)stream);
}

// The two sources of a joined row: A is required, B is absent when all of its fields are null / zero.
static int logreg_check_sources(const char* who, const float* Xa, const int32_t* rows_a, const int64_t lda, const int32_t da,
                                const int64_t n_rows_a, const float* Xb, const int32_t* rows_b, const int64_t ldb,
                                const int32_t db, const int64_t n_rows_b, const int64_t n) {
    GS_REQUIRE(n >= 1 && n <= (1ll << 40), "%s: n=%lld must be at least 1", who, (long long)n);
    GS_REQUIRE(da >= 4 && (da & 3) == 0 && db >= 0 && (db & 3) == 0 && (int64_t)da + db <= GS_LOGREG_JOINED_MAX_D,
               "%s: da=%d and db=%d must be multiples of 4, da >= 4, and d = da + db = %lld at most %d", who, da, db,
               (long long)da + db, GS_LOGREG_JOINED_MAX_D);
    GS_REQUIRE(n_rows_a >= 1 && n_rows_a <= 0x7fffffffll, "%s: n_rows_a=%lld must lie in [1, 2^31)", who, (long long)n_rows_a);
    GS_REQUIRE(Xa && gs_aligned16(Xa) && (lda % 4) == 0, "%s: Xa must be non-null, 16-byte aligned, lda %% 4 == 0 (lda=%lld)", who,
               (long long)lda);
    GS_REQUIRE(lda >= da, "%s: lda=%lld must be >= da=%d", who, (long long)lda, da);
    GS_REQUIRE(rows_a || n <= n_rows_a, "%s: without rows_a, n=%lld must not exceed n_rows_a=%lld", who, (long long)n,
               (long long)n_rows_a);
    const bool has_b = Xb || rows_b || ldb || db || n_rows_b;
    if (has_b) {
        GS_REQUIRE(db >= 4, "%s: source B is given (Xb, rows_b, ldb or n_rows_b is set) with db=%d; an absent B is all null / zero",
                   who, db);
        GS_REQUIRE(n_rows_b >= 1 && n_rows_b <= 0x7fffffffll, "%s: n_rows_b=%lld must lie in [1, 2^31)", who, (long long)n_rows_b);
        GS_REQUIRE(Xb && gs_aligned16(Xb) && (ldb % 4) == 0, "%s: Xb must be non-null, 16-byte aligned, ldb %% 4 == 0 (ldb=%lld)", who,
                   (long long)ldb);
        GS_REQUIRE(ldb >= db, "%s: ldb=%lld must be >= db=%d", who, (long long)ldb, db);
        GS_REQUIRE(rows_b || n <= n_rows_b, "%s: without rows_b, n=%lld must not exceed n_rows_b=%lld", who, (long long)n,
                   (long long)n_rows_b);
    }
    return GS_OK;
}

extern "C" int gs_logreg_eval_joined(const gs_logreg_joined_desc* desc_host, void* stream) {
    const char* who = "gs_logreg_eval_joined";
    GS_REQUIRE(desc_host, "%s: null descriptor", who);
    const gs_logreg_joined_desc& q = *desc_host;
    GS_REQUIRE(q.mode == GS_LOGREG_FIT || q.mode == GS_LOGREG_PREDICT, "%s: unknown mode %d", who, q.mode);
    GS_REQUIRE(q.flags == 0 && q.reserved_ == 0, "%s: unknown flags 0x%x", who, (unsigned)(q.flags | q.reserved_));
    if (int rc = logreg_check_sources(who, q.Xa, q.rows_a, q.lda, q.da, q.n_rows_a, q.Xb, q.rows_b, q.ldb, q.db, q.n_rows_b, q.n))
        return rc;
    const int32_t d = q.da + q.db;
    if (int rc = logreg_check_shape(who, q.n, d, q.c, GS_LOGREG_JOINED_MAX_D)) return rc;
    GS_REQUIRE((q.mu != nullptr) == (q.inv != nullptr), "%s: mu and inv are given together or not at all", who);
    GS_REQUIRE(!q.mu || (gs_aligned16(q.mu) && gs_aligned16(q.inv)), "%s: mu and inv must be 16-byte aligned", who);
    const LogregCall k = {q.W, q.b, q.y_class, q.y_multi, q.loss, q.gW, q.gb, q.pred_class, q.pred_multi, q.ws,
                          q.n, q.ldw, q.ldy, q.ldp, q.ws_bytes, d, q.c, q.mode};
    if (int rc = logreg_check_call(who, k)) return rc;
    LogregArgs g = {};
    g.X = q.Xa; g.rows = q.rows_a; g.n_rows = q.n_rows_a; g.ldx = q.lda; g.da = q.da;
    g.Xb = q.Xb; g.rows_b = q.rows_b; g.n_rows_b = q.n_rows_b; g.ldb = q.ldb;
    g.mu = q.mu; g.inv = q.inv;
    return logreg_enqueue<true>(g, k, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------------- moments
// Column mean and population variance of the joined rows in fp64, centred: the means first, then the squares of (x - mean).
// The rows are cut into at most CM_MAX_CHUNKS contiguous chunks (a function of n alone); a workgroup takes one chunk of a
// strip of 64 columns (lanes along the columns: 256-byte row segments), its four waves every fourth row each, and writes one
// fp64 partial per column; a second launch adds the partials in chunk order and divides by n.  No atomics, a fixed order.
// A column whose entries are all x: every partial sum is k * x exactly (24 + log2 n bits), (n * x) / n rounds to x, every
// centred term is zero.
#define CM_COLS 64
#define CM_MAX_CHUNKS GS_COL_MOMENTS_MAX_CHUNKS

template <bool CENTRED>
__global__ __launch_bounds__(256) void col_moments_partial_kernel(const LogregArgs g, const int64_t rows_per_chunk,
                                                                  const double* __restrict__ mean, double* __restrict__ partial) {
    __shared__ double part[4][CM_COLS];
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int col = (int)blockIdx.y * CM_COLS + l;
    const bool cok = col < g.d;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_chunk, r1 = min(r0 + rows_per_chunk, g.n);
    double s = 0.0;
    if (cok) {
        const bool from_a = col < g.da;
        const double mu = CENTRED ? mean[col] : 0.0;
        for (int64_t i = r0 + w; i < r1; i += 4) {
            const float x = from_a ? g.X[lr_row(g.rows, i, true, g.n_rows) * g.ldx + col]
                                   : g.Xb[lr_row(g.rows_b, i, true, g.n_rows_b) * g.ldb + (col - g.da)];
            const double t = (double)x - mu;
            s += CENTRED ? t * t : t;
        }
    }
    part[w][l] = s;
    __syncthreads();
    if (w == 0 && cok) partial[(int64_t)blockIdx.x * g.d + col] = ((part[0][l] + part[1][l]) + part[2][l]) + part[3][l];
}

__global__ __launch_bounds__(256) void col_moments_sum_kernel(const double* __restrict__ partial, const int chunks, const int d,
                                                              const int64_t n, double* __restrict__ out) {
    const int j = (int)blockIdx.x * 256 + threadIdx.x;
    if (j >= d) return;
    double s = 0.0;
    for (int k = 0; k < chunks; ++k) s += partial[(int64_t)k * d + j];
    out[j] = s / (double)n;
}

extern "C" int gs_col_moments(const float* Xa, const int32_t* rows_a, int64_t lda, int32_t da, int64_t n_rows_a,
                              const float* Xb, const int32_t* rows_b, int64_t ldb, int32_t db, int64_t n_rows_b, int64_t n,
                              double* mean, double* var, void* ws, int64_t ws_bytes, void* stream) {
    const char* who = "gs_col_moments";
    if (int rc = logreg_check_sources(who, Xa, rows_a, lda, da, n_rows_a, Xb, rows_b, ldb, db, n_rows_b, n)) return rc;
    const int32_t d = da + db;
    GS_REQUIRE(mean && var && (reinterpret_cast<uintptr_t>(mean) & 7u) == 0 && (reinterpret_cast<uintptr_t>(var) & 7u) == 0,
               "%s: mean and var must be non-null and 8-byte aligned", who);
    const int64_t need = (int64_t)CM_MAX_CHUNKS * d * (int64_t)sizeof(double);
    GS_REQUIRE(ws && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0 && ws_bytes >= need,
               "%s: needs an 8-byte aligned workspace of %lld bytes (GS_COL_MOMENTS_MAX_CHUNKS * d * 8), got %lld", who,
               (long long)need, (long long)ws_bytes);
    const int64_t rpc = gs_ceil_div(n, std::min<int64_t>(CM_MAX_CHUNKS, gs_ceil_div(n, CM_COLS)));
    const int chunks = (int)gs_ceil_div(n, rpc);
    LogregArgs g = {};
    g.X = Xa; g.rows = rows_a; g.n_rows = n_rows_a; g.ldx = lda; g.da = da;
    g.Xb = Xb; g.rows_b = rows_b; g.n_rows_b = n_rows_b; g.ldb = ldb;
    g.n = n; g.d = d;
    double* partial = reinterpret_cast<double*>(ws);
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)chunks, (unsigned)gs_ceil_div(d, CM_COLS));
    const dim3 sum_grid((unsigned)gs_ceil_div(d, 256));
    hipLaunchKernelGGL(col_moments_partial_kernel<false>, grid, dim3(256), 0, st, g, rpc, (const double*)nullptr, partial);
    GS_LAUNCH_CHECK("col_moments_partial_kernel");
    hipLaunchKernelGGL(col_moments_sum_kernel, sum_grid, dim3(256), 0, st, partial, chunks, (int)d, n, mean);
    GS_LAUNCH_CHECK("col_moments_sum_kernel");
    hipLaunchKernelGGL(col_moments_partial_kernel<true>, grid, dim3(256), 0, st, g, rpc, (const double*)mean, partial);
    GS_LAUNCH_CHECK("col_moments_partial_kernel");
    hipLaunchKernelGGL(col_moments_sum_kernel, sum_grid, dim3(256), 0, st, partial, chunks, (int)d, n, var);
    GS_LAUNCH_CHECK("col_moments_sum_kernel");
    return GS_OK;
}

