// The tile loop that gs_logreg_eval and gs_logreg_eval_joined share: the staging of the 32-row tile (lr_stage) and the body of
// the kernel (lr_body: the logits on v_mfma_f32_32x32x2_f32, the epilogue, the parked residuals, the X^T R tiles, the
// workgroup's partial), and the host's plan.  Both kernels run THESE functions; they differ in the staging alone (JOINED: two
// sources and an affine), so with one source and no affine the joined kernel stages the same floats and every output is
// bit-equal.  The two contraction loops stand in lr_body itself: as functions of their own (the accumulators passed by
// reference) the compiler held 147 / 196 / 256 + 21 spilled registers at 1 / 2 / 4 gradient tiles per wave against
// 118 / 155 / 227 and none spilled this way.  The layout and the reasons are in the header comment of gs_logreg.hip.
#pragma once
#include "gs_common.h"

#define LR_ROWS 32               // rows per tile (the MFMA's M in the logits, its K in the gradient)
#define LR_RP 132                // padded stride of the residual tile (128 classes + 4)
#define LR_WG_CAP 512            // workgroups along x, at most: the partials' count
#define LR_MAX_NT 8              // gradient tiles per wave, at most
#define LR_LDS_BYTES(d, fit) ((size_t)(LR_ROWS * ((d) + 4) + ((fit) ? LR_ROWS * LR_RP : 0)) * sizeof(float))

struct LogregArgs {
    const float* X; const int32_t* rows;                     // source A (the only one of gs_logreg_eval)
    const float* Xb; const int32_t* rows_b;                  // source B, columns [da, d); JOINED only, null: absent
    const float* mu; const float* inv;                       // the affine (x - mu[j]) * inv[j]; JOINED only, null: none
    const float* W; const float* b;
    const int32_t* y_class; const uint8_t* y_multi;
    int32_t* pred_class; uint8_t* pred_multi; float* ws;
    int64_t n, n_rows, ldx, n_rows_b, ldb, ldw, ldy, ldp, tiles, tiles_per_wg, ws_stride;
    int32_t d, da, c, cb_n, db_n, dbw, want_loss;
};

// (row tiles, row tiles per workgroup, workgroups along x) for n rows
static inline void logreg_plan(const int64_t n, int64_t* tiles, int64_t* tpw, int64_t* wgs) {
    *tiles = std::max<int64_t>(1, gs_ceil_div(n, LR_ROWS));
    *tpw = gs_ceil_div(*tiles, LR_WG_CAP);
    *wgs = gs_ceil_div(*tiles, *tpw);
}

// a row index clamped into its table: the caller checked; never a stray read
__device__ __forceinline__ int64_t lr_row(const int32_t* rows, const int64_t i, const bool ok, const int64_t n_rows) {
    const int64_t r = ok ? (rows ? (int64_t)rows[i] : i) : 0;
    return r < 0 ? 0 : (r >= n_rows ? n_rows - 1 : r);
}

// ---- 1. the gathered rows -> LDS [32][XP]: 8 threads x float4 per row, rows >= n as zeros.  JOINED: columns [0, da) from
// source A and [da, d) from source B (da % 4 == 0: a float4 never straddles the seam), then ONE fp32 subtract and ONE fp32
// multiply per element -- not fma(x, inv, -mu * inv), which cancels for a column whose mean is large against its spread.
// Rows >= n are zeros AFTER the affine.
template <bool JOINED>
__device__ __forceinline__ void lr_stage(const LogregArgs& g, float* Xs, const int XP, const int64_t i0, const int tid) {
    const int srow = tid >> 3, sq = tid & 7;
    const int d = g.d;
    const int64_t i = i0 + srow;
    const bool ok = i < g.n;
    const float* xr = g.X + lr_row(g.rows, i, ok, g.n_rows) * g.ldx;
    if (!JOINED) {
        for (int q = sq; 4 * q < d; q += 8) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (ok) v = *reinterpret_cast<const f32x4*>(xr + 4 * q);
            *reinterpret_cast<f32x4*>(&Xs[srow * XP + 4 * q]) = v;
        }
    } else {
        const int da = g.da;
        const float* xb = g.Xb ? g.Xb + lr_row(g.rows_b, i, ok, g.n_rows_b) * g.ldb : xr;
        const bool affine = g.mu != nullptr;
        for (int q = sq; 4 * q < d; q += 8) {
            const int j = 4 * q;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (ok) {
                v = *reinterpret_cast<const f32x4*>(j < da ? xr + j : xb + (j - da));
                if (affine) {
                    const f32x4 m = *reinterpret_cast<const f32x4*>(g.mu + j);
                    const f32x4 s = *reinterpret_cast<const f32x4*>(g.inv + j);
                    v = (v - m) * s;
                }
            }
            *reinterpret_cast<f32x4*>(&Xs[srow * XP + j]) = v;
        }
    }
}

// The whole kernel body: a workgroup's run of row tiles, then its partial [loss c][gb c][gW d * c].
template <int NT, bool FIT, bool JOINED>
__device__ __forceinline__ void lr_body(const LogregArgs& g) {
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

    for (int64_t tile = tile0; tile < tile1; ++tile) {
        const int64_t i0 = tile * LR_ROWS;
        lr_stage<JOINED>(g, Xs, XP, i0, tid);
        if (tid < LR_ROWS) ycls[tid] = (g.y_class && i0 + tid < g.n) ? g.y_class[i0 + tid] : -1;
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
