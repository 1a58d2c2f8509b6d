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
#include "gs_common.h"

static_assert(sizeof(gs_logreg_desc) == 168, "gs_logreg_desc layout (mirrored by graphsage_amd/_lib.py)");

#define LR_ROWS 32               // rows per tile (the MFMA's M in the logits, its K in the gradient)
#define LR_RP 132                // padded stride of the residual tile (128 classes + 4)
#define LR_WG_CAP 512            // workgroups along x, at most: the partials' count
#define LR_MAX_NT 8              // gradient tiles per wave, at most
#define LR_MAX_LDS ((LR_ROWS * (GS_LOGREG_MAX_D + 4) + LR_ROWS * LR_RP) * 4)

struct LogregArgs {
    const float* X; const int32_t* rows; const float* W; const float* b;
    const int32_t* y_class; const uint8_t* y_multi;
    int32_t* pred_class; uint8_t* pred_multi; float* ws;
    int64_t n, n_rows, ldx, ldw, ldy, ldp, tiles, tiles_per_wg, ws_stride;
    int32_t d, c, cb_n, db_n, dbw, want_loss;
};

// (row tiles, row tiles per workgroup, workgroups along x) for n rows
static inline void logreg_plan(const int64_t n, int64_t* tiles, int64_t* tpw, int64_t* wgs) {
    *tiles = std::max<int64_t>(1, gs_ceil_div(n, LR_ROWS));
    *tpw = gs_ceil_div(*tiles, LR_WG_CAP);
    *wgs = gs_ceil_div(*tiles, *tpw);
}

// (256, 2) up to four gradient tiles per wave: a budget of 256 registers per lane, two workgroups per CU.  At four tiles the
// compiler reports 256 registers and ONE spilled register (8 bytes of scratch per lane); measured at the Reddit shape
// (d = 256, c = 41) that is 0.31 ms per evaluation against 0.44 ms with 512 registers and one workgroup per CU
// (profiles/eval_classifier.md).  Eight tiles (128 accumulator registers) take the 512, nothing spilled.
template <int NT, bool FIT>
__global__ __launch_bounds__(256, NT <= 4 ? 2 : 1) void logreg_kernel(const LogregArgs g) {
    extern __shared__ __attribute__((aligned(16))) float lr_smem[];
    __shared__ int32_t ycls[LR_ROWS];
    __shared__ float bestv[4][LR_ROWS];
    __shared__ int32_t besti[4][LR_ROWS];

    const int d = g.d, c = g.c, XP = d + 4, CB = g.cb_n;
    float* Xs = lr_smem;                         // [32][XP]
    float* Rs = lr_smem + LR_ROWS * XP;          // [32][LR_RP]
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;

    const int db0 = (int)blockIdx.y * g.dbw;                 // this workgroup's d blocks of the gradient
    const int ntl = CB * min(g.dbw, g.db_n - db0);           // ... and its output tiles (<= 4 * NT)
    const int64_t tile0 = (int64_t)blockIdx.x * g.tiles_per_wg;
    const int64_t tile1 = min(tile0 + g.tiles_per_wg, g.tiles);

    const int cls = wave * 32 + l31;                         // the lane's class in the logits phase
    const bool cls_ok = wave < CB && cls < c;
    const float bias = cls_ok ? g.b[cls] : 0.f;
    const float* wcol = g.W + (cls_ok ? cls : 0);
    const bool labelled = g.y_class != nullptr || g.y_multi != nullptr;

    f32x16 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
    float lossl = 0.f, gbl = 0.f;

    const int srow = tid >> 3, sq = tid & 7;
    for (int64_t tile = tile0; tile < tile1; ++tile) {
        const int64_t i0 = tile * LR_ROWS;
        // ---- 1. the gathered rows -> LDS
        {
            const int64_t i = i0 + srow;
            const bool ok = i < g.n;
            int64_t r = ok ? (g.rows ? (int64_t)g.rows[i] : i) : 0;
            r = r < 0 ? 0 : (r >= g.n_rows ? g.n_rows - 1 : r);       // the caller checked; never a stray read
            const float* xr = g.X + r * g.ldx;
            for (int q = sq; 4 * q < d; q += 8) {
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (ok) v = *reinterpret_cast<const f32x4*>(xr + 4 * q);
                *reinterpret_cast<f32x4*>(&Xs[srow * XP + 4 * q]) = v;
            }
            if (tid < LR_ROWS) ycls[tid] = (g.y_class && i0 + tid < g.n) ? g.y_class[i0 + tid] : -1;
        }
        __syncthreads();

        // ---- 2. logits of class block `wave`, 3. loss terms and residuals
        if (wave < CB) {
            f32x16 z;
#pragma unroll
            for (int e = 0; e < 16; ++e) z[e] = 0.f;
            for (int k0 = 0; k0 < d; k0 += 8) {
                const int k = k0 + 4 * lh;
                const bool kok = k < d;                      // d % 4 == 0: a group of four is whole or absent
                f32x4 a = {0.f, 0.f, 0.f, 0.f};
                float w[4] = {0.f, 0.f, 0.f, 0.f};
                if (kok) {
                    a = *reinterpret_cast<const f32x4*>(&Xs[l31 * XP + k]);
                    if (cls_ok) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) w[i] = wcol[(int64_t)(k + i) * g.ldw];
                    }
                }
                z = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, w[0], z, 0, 0, 0);
                z = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, w[1], z, 0, 0, 0);
                z = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, w[2], z, 0, 0, 0);
                z = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, w[3], z, 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = (e & 3) + 8 * (e >> 2) + 4 * lh;
                const int64_t i = i0 + row;
                const bool valid = cls_ok && i < g.n;
                const float zz = z[e] + bias;
                float r = 0.f;
                if (labelled && valid) {
                    const bool pos = g.y_class ? (ycls[row] == cls) : (g.y_multi[i * g.ldy + cls] != 0);
                    const float s = pos ? 1.f : -1.f;
                    const float m = s * zz;
                    const float ex = expf(-fabsf(m));
                    lossl += fmaxf(-m, 0.f) + log1pf(ex);
                    r = -s * ((m >= 0.f ? ex : 1.f) / (1.f + ex));
                    gbl += r;
                }
                if (FIT) {
                    Rs[row * LR_RP + cls] = r;               // every column of the class blocks in use, zeros past c and n
                } else {
                    if (g.pred_multi && valid) g.pred_multi[i * g.ldp + cls] = zz > 0.f ? 1 : 0;
                    if (g.pred_class) {
                        float v = valid ? zz : -INFINITY;
                        int idx = cls;
#pragma unroll
                        for (int off = 16; off > 0; off >>= 1) {          // the 32 lanes of a half hold one row's classes
                            const float ov = __shfl_xor(v, off, 64);
                            const int oi = __shfl_xor(idx, off, 64);
                            if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
                        }
                        if (l31 == 0) { bestv[wave][row] = v; besti[wave][row] = idx; }
                    }
                }
            }
        }
        __syncthreads();

        if (FIT) {
            // ---- 4. X^T R: output tile t = (d block t / CB, class block t % CB), waves take t = wave, wave + 4, ..
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int t = wave + 4 * j;
                if (t < ntl) {
                    const int dcol = (db0 + t / CB) * 32 + l31;
                    const int rcol = (t % CB) * 32 + l31;
                    const bool dok = dcol < d;
#pragma unroll
                    for (int k0 = 0; k0 < LR_ROWS; k0 += 8) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int k = k0 + 4 * lh + i;
                            const float a = dok ? Xs[k * XP + dcol] : 0.f;
                            const float bv = Rs[k * LR_RP + rcol];
                            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc[j], 0, 0, 0);
                        }
                    }
                }
            }
        } else if (g.pred_class && tid < LR_ROWS && i0 + tid < g.n) {
            float v = bestv[0][tid];
            int idx = besti[0][tid];
            for (int w = 1; w < CB; ++w)
                if (bestv[w][tid] > v) { v = bestv[w][tid]; idx = besti[w][tid]; }     // strict: the lower block keeps a tie
            g.pred_class[i0 + tid] = idx;
        }
        __syncthreads();             // the tiles in LDS change hands
    }

    // ---- this workgroup's partial: [loss c][gb c][gW d * c]
    float* slab = g.ws + (int64_t)blockIdx.x * g.ws_stride;
    if (g.want_loss && blockIdx.y == 0 && wave < CB) {
        lossl += __shfl_xor(lossl, 32, 64);
        gbl += __shfl_xor(gbl, 32, 64);
        if (lh == 0 && cls < c) {
            slab[cls] = lossl;
            if (FIT) slab[c + cls] = gbl;
        }
    }
    if (FIT) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int t = wave + 4 * j;
            if (t < ntl) {
                const int drow0 = (db0 + t / CB) * 32 + 4 * lh;
                const int ccol = (t % CB) * 32 + l31;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int drow = drow0 + (e & 3) + 8 * (e >> 2);
                    if (drow < d && ccol < c) slab[2 * c + (int64_t)drow * c + ccol] = acc[j][e];
                }
            }
        }
    }
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

static int logreg_check_shape(const char* who, const int64_t n, const int32_t d, const int32_t c) {
    GS_REQUIRE(n >= 1 && n <= (1ll << 40), "%s: n=%lld must be at least 1", who, (long long)n);
    GS_REQUIRE(d >= 4 && d <= GS_LOGREG_MAX_D && (d & 3) == 0, "%s: d=%d must be a multiple of 4 in [4, %d]", who, d,
               GS_LOGREG_MAX_D);
    GS_REQUIRE(c >= 1 && c <= GS_LOGREG_MAX_C, "%s: c=%d must lie in [1, %d]", who, c, GS_LOGREG_MAX_C);
    return GS_OK;
}

extern "C" int gs_logreg_ws_bytes(int64_t n, int32_t d, int32_t c, int64_t* bytes_out_host) {
    GS_REQUIRE(bytes_out_host, "gs_logreg_ws_bytes: null output");
    if (int rc = logreg_check_shape("gs_logreg_ws_bytes", n, d, c)) return rc;
    int64_t tiles, tpw, wgs;
    logreg_plan(n, &tiles, &tpw, &wgs);
    *bytes_out_host = wgs * (2 * (int64_t)c + (int64_t)d * c) * (int64_t)sizeof(float);
    return GS_OK;
}

template <int NT, bool FIT>
static int logreg_launch(const LogregArgs& g, const dim3 grid, const size_t lds, const hipStream_t st) {
    GS_LDS_ATTR(LR_MAX_LDS, logreg_kernel<NT, FIT>);
    hipLaunchKernelGGL((logreg_kernel<NT, FIT>), grid, dim3(256), lds, st, g);
    GS_LAUNCH_CHECK("logreg_kernel");
    return GS_OK;
}

extern "C" int gs_logreg_eval(const gs_logreg_desc* desc_host, void* stream) {
    GS_REQUIRE(desc_host, "gs_logreg_eval: null descriptor");
    const gs_logreg_desc& q = *desc_host;
    GS_REQUIRE(q.mode == GS_LOGREG_FIT || q.mode == GS_LOGREG_PREDICT, "gs_logreg_eval: unknown mode %d", q.mode);
    GS_REQUIRE(q.flags == 0, "gs_logreg_eval: unknown flags 0x%x", (unsigned)q.flags);
    if (int rc = logreg_check_shape("gs_logreg_eval", q.n, q.d, q.c)) return rc;
    const bool fit = q.mode == GS_LOGREG_FIT;
    GS_REQUIRE(q.n_rows >= 1 && q.n_rows <= 0x7fffffffll, "gs_logreg_eval: n_rows=%lld must lie in [1, 2^31)", (long long)q.n_rows);
    GS_CHECK_MAT(q.X, q.ldx, "gs_logreg_eval X");
    GS_REQUIRE(q.ldx >= q.d, "gs_logreg_eval: ldx=%lld must be >= d=%d", (long long)q.ldx, q.d);
    GS_REQUIRE(q.rows || q.n <= q.n_rows, "gs_logreg_eval: without rows, n=%lld must not exceed n_rows=%lld", (long long)q.n,
               (long long)q.n_rows);
    GS_REQUIRE(q.W && q.b && q.ldw >= q.c, "gs_logreg_eval: W and b must be non-null, ldw=%lld >= c=%d", (long long)q.ldw, q.c);
    const bool labelled = q.y_class || q.y_multi;
    GS_REQUIRE(!(q.y_class && q.y_multi), "gs_logreg_eval: y_class and y_multi exclude each other");
    GS_REQUIRE(!q.y_multi || q.ldy >= q.c, "gs_logreg_eval: ldy=%lld must be >= c=%d", (long long)q.ldy, q.c);
    if (fit) {
        GS_REQUIRE(labelled, "gs_logreg_eval: FIT needs y_class or y_multi");
        GS_REQUIRE(q.loss && q.gW && q.gb, "gs_logreg_eval: FIT writes loss, gW and gb; none may be null");
        GS_REQUIRE(!q.pred_class && !q.pred_multi, "gs_logreg_eval: predictions are written in PREDICT mode only");
    } else {
        GS_REQUIRE(!q.gW && !q.gb, "gs_logreg_eval: gW and gb are written in FIT mode only");
        GS_REQUIRE(!q.loss || labelled, "gs_logreg_eval: a loss needs labels");
        GS_REQUIRE(q.pred_class || q.pred_multi || q.loss, "gs_logreg_eval: PREDICT has nothing to write");
        GS_REQUIRE(!q.pred_multi || q.ldp >= q.c, "gs_logreg_eval: ldp=%lld must be >= c=%d", (long long)q.ldp, q.c);
    }
    int64_t tiles, tpw, wgs;
    logreg_plan(q.n, &tiles, &tpw, &wgs);
    const int64_t stride = 2 * (int64_t)q.c + (int64_t)q.d * q.c;
    const bool want_loss = q.loss != nullptr;
    if (want_loss) {
        const int64_t need = wgs * stride * (int64_t)sizeof(float);
        GS_REQUIRE(q.ws && (reinterpret_cast<uintptr_t>(q.ws) & 7u) == 0 && q.ws_bytes >= need,
                   "gs_logreg_eval: needs an 8-byte aligned workspace of %lld bytes (gs_logreg_ws_bytes), got %lld",
                   (long long)need, (long long)q.ws_bytes);
        GS_REQUIRE((reinterpret_cast<uintptr_t>(q.loss) & 7u) == 0 && (reinterpret_cast<uintptr_t>(q.gW) & 7u) == 0 &&
                   (reinterpret_cast<uintptr_t>(q.gb) & 7u) == 0, "gs_logreg_eval: the fp64 outputs must be 8-byte aligned");
    }
    LogregArgs g;
    g.X = q.X; g.rows = q.rows; g.W = q.W; g.b = q.b; g.y_class = q.y_class; g.y_multi = q.y_multi;
    g.pred_class = q.pred_class; g.pred_multi = q.pred_multi; g.ws = reinterpret_cast<float*>(q.ws);
    g.n = q.n; g.n_rows = q.n_rows; g.ldx = q.ldx; g.ldw = q.ldw; g.ldy = q.ldy; g.ldp = q.ldp;
    g.tiles = tiles; g.tiles_per_wg = tpw; g.ws_stride = stride;
    g.d = q.d; g.c = q.c; g.cb_n = (int32_t)gs_ceil_div(q.c, 32); g.db_n = (int32_t)gs_ceil_div(q.d, 32);
    g.dbw = fit ? std::min<int32_t>(g.db_n, 4 * LR_MAX_NT / g.cb_n) : g.db_n;
    g.want_loss = want_loss ? 1 : 0;
    const int y_blocks = fit ? (int)gs_ceil_div(g.db_n, g.dbw) : 1;
    const int per_wave = (int)gs_ceil_div((int64_t)g.cb_n * g.dbw, 4);
    const dim3 grid((unsigned)wgs, (unsigned)y_blocks);
    const size_t lds = (size_t)(LR_ROWS * (q.d + 4) + (fit ? LR_ROWS * LR_RP : 0)) * sizeof(float);
    const hipStream_t st = (hipStream_t)stream;
    int rc;
    if (!fit) rc = logreg_launch<1, false>(g, grid, lds, st);
    else if (per_wave <= 1) rc = logreg_launch<1, true>(g, grid, lds, st);
    else if (per_wave <= 2) rc = logreg_launch<2, true>(g, grid, lds, st);
    else if (per_wave <= 4) rc = logreg_launch<4, true>(g, grid, lds, st);
    else rc = logreg_launch<LR_MAX_NT, true>(g, grid, lds, st);
    if (rc) return rc;
    if (want_loss) {
        const int64_t count = fit ? stride : q.c;
        hipLaunchKernelGGL(logreg_sum_kernel, dim3((unsigned)gs_ceil_div(count, 256)), dim3(256), 0, st, g.ws, stride, (int)wgs,
                           count, (int)q.c, q.loss, q.gb, q.gW);
        GS_LAUNCH_CHECK("logreg_sum_kernel");
    }
    return GS_OK;
}
