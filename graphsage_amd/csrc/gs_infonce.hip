// The in-batch softmax (InfoNCE) link-prediction head: gs_linkpred_infonce_fwd_bwd[_step].
//
//   C      = [y2 ; neg]                       B + n_neg candidate rows (rows [B, 2B + n_neg) of X, normalised)
//   L_ij   = <u_i, C_j> / tau                 u = the left operand U [B, d]
//   mask   : j < B, j != i, (ids2[j] == ids2[i] or ids2[j] == ids1[i])     candidate j is left out of row i
//   loss_i = logsumexp_{j not masked} L_ij - L_ii
//   G      = scale (P - I) / tau,  P = the row softmax over the same set (0 where masked)
//   dU = G . C        dC = G^T . U            (dC = rows [B, 2B + n_neg) of dX)
//   aff_all row = [<u_i, neg_q> .. | <u_i, y2_i>] (raw, not divided by tau);  rr_i = 1 / (1 + #{q : <u_i, neg_q> >= <u_i, y2_i>})
//
// The logit tiles run the 128 x 128 fp32-MFMA tile pipeline of gs_rank_dev.h (rank_first_loads, rank_k_loop: BK = 32, two LDS
// stages), the gradient contractions its rank_compute alone.
// After a tile's K loop the 2 x 2 x 16 accumulator cells of every lane go to a tile buffer in LDS,
// laid out as four [128][RK_KP] chunks of 32 columns -- the layout rank_compute reads an A operand in -- and two threads per
// row (columns [0, 64) and [64, 128), ascending) take it from there.  The B x (B + n_neg) matrix is never written to memory.
// One such tile is 13.6 us of fp32 MFMA at d = 256 (the rate of ONE CU), so the cut that matters at the driver's B = 512 is
// how many workgroups share the work, not the tile's height (profiles/linkpred_infonce.md has both forms measured):
//
// infonce_stats_kernel   (ceil(B / 128), ceil((B + n_neg) / 128)) workgroups, one tile each.  A row's two threads find the
//   cells that count and their maximum, then sum 64 independent exponentials; the halves meet in LDS (half 0 first) and
//   part[tile][row] = (maximum, sum) is written.  The raw scores of the sampled negatives and <u_i, y2_i> go to aff_all.
// infonce_finish_kernel  one wave per row: the tiles' pairs meet (lane l takes tiles l, l + 64, .., then the xor butterfly), the
//   negatives >= aff_i are counted from aff_all, and loss_rows, rr_rows and stats [B, 2] = (maximum, log sum) are written.
// infonce_grad_kernel    A row owner (128 rows of U) recomputes logit tiles, turns each into the G tile in place (from the
//   row's stats) and contracts it against 128 output columns of the candidate rows: the G chunk is rank_compute's A operand
//   as it lies, the candidate rows pass through the (idle) B stages transposed.  A column owner (128 candidate rows) does the
//   transposed job with the queries' stats for dC.  The output columns are cut over blockIdx.y because 128 x d accumulators
//   do not fit the registers at d = 512 (the logit tile is recomputed per cut), and an owner's sweep is cut over at most
//   NCE_MAX_CUT workgroups of consecutive swept tiles, each writing its partial sum to a slab of its own.
// infonce_reduce_kernel  adds an element's slabs in ascending order (a sweep that was not cut was written in place); its last
//   workgroup is the step epilogue (loss / mrr means, device counters), which a forward-only step runs as a launch of its own.
// Every element has one writer per launch and one fixed summation order (k order of rank_compute, tiles ascending inside a
// cut, cuts ascending): no float atomics; two runs give the same bits.
//
// Padded rows and columns of a tile (B and B + n_neg are rarely multiples of 128) are loaded as zeros AND skipped by index, and
// a masked cell is skipped the same way: none of them enters the maximum, the sum or either gradient.  A row's own positive is
// never masked, so its set is never empty and the maximum is finite.
//
// Resources (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage) are quoted in profiles/linkpred_infonce.md.
#include "gs_rank_dev.h"

#define NCE_CH (RK_BM * RK_KP)          // floats of one 32-column chunk of the tile buffer: [128 rows][RK_KP]

struct NceArgs {
    const float* U; int64_t ldu;        // [B, d] left operand
    const float* C; int64_t ldc;        // [B + n_neg, d] candidates
    const int32_t* ids1; const int32_t* ids2;      // both or neither
    float* stats;                       // [B, 2] (max, log sum)
    float* part;                        // [tiles_c, B, 2] per candidate tile (max, sum of exp(L - max))
    float* slabU; float* slabC;         // [nzU, B, d] / [nzC, B + n_neg, d] partial gradients (nz > 1 only)
    int32_t nzU, perU, nzC, perC;       // cuts of the gradient sweeps: nz workgroups of `per` swept tiles each
    float* loss_rows; float* rr_rows; float* aff_all; int64_t ld_aff;
    float* dU; int64_t lddu; float* dC; int64_t lddc;
    int64_t B; int32_t n_neg, d, tiles_m, tiles_c;
    float inv_tau, gscale;              // 1 / tau, scale / tau
};

// acc = P[p0 .. p0 + 128, :] . S[s0 .. s0 + 128, :]^T over K = d through the pipeline of gs_rank_dev.h.  Rows at or beyond
// n_p / n_s read as zeros.  The caller puts a __syncthreads between two calls (the stage buffers change hands).
__device__ __forceinline__ void nce_tile(const float* __restrict__ P, const int64_t ldp, const int64_t n_p, const int64_t p0,
                                         const float* __restrict__ S, const int64_t lds_, const int64_t n_s, const int64_t s0,
                                         const int d, float* smem, const int wm, const int wn, const int l31, const int lh,
                                         f32x16 (&acc)[2][2]) {
    RankOperand A, B;
    rank_rows(A, P, ldp, p0, n_p);
    rank_rows(B, S, lds_, s0, n_s);
    RankRegs ra0, rb0, ra1, rb1;
    rank_first_loads<true>(A, B, d, ra0, rb0, ra1, rb1);      // d is 64, 128, 256 or 512: whole pairs of stages
    rank_k_loop<true>(A, B, d, smem, ra0, rb0, ra1, rb1, wm, wn, l31, lh, acc);
}

// the lane's accumulator cells into the tile buffer: cell (row, col) at T[(col >> 5) NCE_CH + row RK_KP + (col & 31)]
__device__ __forceinline__ void nce_dump(const f32x16 (&acc)[2][2], float* T, const int wm, const int wn, const int l31,
                                         const int lh) {
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = wm * 64 + tm * 32 + rank_acc_row(e, lh);
                T[(wn * 2 + tn) * NCE_CH + row * RK_KP + l31] = acc[tm][tn][e];
            }
}

__device__ __forceinline__ int nce_cell(const int row, const int col) { return (col >> 5) * NCE_CH + row * RK_KP + (col & 31); }

// one (query tile, candidate tile) pair per workgroup: part[tile][i] = (maximum, sum of exp(L - maximum)) of row i over the tile
__global__ __launch_bounds__(256) void infonce_stats_kernel(const NceArgs g) {
    __shared__ __attribute__((aligned(16))) float smem[2 * RK_STAGE_FLOATS];
    __shared__ __attribute__((aligned(16))) float T[4 * NCE_CH];
    __shared__ int32_t cid2[RK_BN];
    __shared__ float mS[RK_BM], sS[RK_BM];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;
    const int64_t B = g.B, n_cand = g.B + g.n_neg;
    const int64_t m0 = (int64_t)blockIdx.x * RK_BM, n0 = (int64_t)blockIdx.y * RK_BN;
    const bool has_ids = g.ids1 != nullptr;

    // the row this thread walks: columns [64 half, 64 half + 64) of the tile
    const int r = tid & 127, half = tid >> 7;
    const int64_t i = m0 + r;
    const bool live = i < B;
    int32_t id1 = 0, id2 = 0;
    if (live && has_ids) {
        id1 = g.ids1[i];
        id2 = g.ids2[i];
    }
    f32x16 acc[2][2];
    nce_tile(g.U, g.ldu, B, m0, g.C, g.ldc, n_cand, n0, g.d, smem, wm, wn, l31, lh, acc);
    if (tid < RK_BN) cid2[tid] = (has_ids && n0 + tid < B) ? g.ids2[n0 + tid] : 0;
    nce_dump(acc, T, wm, wn, l31, lh);
    __syncthreads();

    // pass 1: which cells count (one bit each) and their maximum; pass 2: the sum, 64 independent exponentials
    float m = -__builtin_inff(), s = 0.f;
    uint64_t used = 0ull;
    if (live) {
        if (blockIdx.y == blockIdx.x && half == 0) g.aff_all[i * g.ld_aff + g.n_neg] = T[nce_cell(r, r)];     // <u_i, y2_i>
#pragma unroll 8
        for (int jj = 0; jj < 64; ++jj) {
            const int c = half * 64 + jj;
            const int64_t j = n0 + c;
            if (j >= n_cand) break;
            const float raw = T[nce_cell(r, c)];
            bool use = true;
            if (j < B) {
                if (has_ids && j != i) {
                    const int32_t cj = cid2[c];
                    use = !(cj == id2 || cj == id1);
                }
            } else {                                                      // a sampled negative: never masked
                g.aff_all[i * g.ld_aff + (j - B)] = raw;
            }
            if (use) {
                used |= 1ull << jj;
                m = fmaxf(m, raw * g.inv_tau);
            }
        }
#pragma unroll 8
        for (int jj = 0; jj < 64; ++jj)
            if ((used >> jj) & 1ull) s += expf(T[nce_cell(r, half * 64 + jj)] * g.inv_tau - m);
    }
    if (half == 1) {
        mS[r] = m;
        sS[r] = s;
    }
    __syncthreads();
    if (half == 0 && live) {
        // half 0 first; a half (or a whole tile row) without a counted cell has (-inf, 0) and adds nothing
        const float m1 = mS[r], s1 = sS[r];
        const float M = fmaxf(m, m1);
        float S = 0.f;
        if (s > 0.f) S = s * expf(m - M);
        if (s1 > 0.f) S += s1 * expf(m1 - M);
        float* pp = g.part + ((int64_t)blockIdx.y * B + i) * 2;
        pp[0] = M;
        pp[1] = S;
    }
}

// One wave per row: the tiles' (maximum, sum) pairs meet -- lane l takes tiles l, l + 64, .. in ascending order, then the xor
// butterfly -- and the sampled negatives >= aff_i are counted from aff_all (the bits the sweep wrote).  The row's own positive
// is never masked, so its tile has a finite maximum and M is finite.
__global__ __launch_bounds__(256) void infonce_finish_kernel(const NceArgs g) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= g.B) return;                                    // wave-uniform
    float M = -__builtin_inff();
    for (int t = lane; t < g.tiles_c; t += 64) M = fmaxf(M, g.part[((int64_t)t * g.B + i) * 2]);
    M = gs_wave_max(M);
    float S = 0.f;
    for (int t = lane; t < g.tiles_c; t += 64) {
        const float* pp = g.part + ((int64_t)t * g.B + i) * 2;
        if (pp[1] > 0.f) S += pp[1] * expf(pp[0] - M);
    }
    S = gs_wave_sum(S);
    const float* row = g.aff_all + i * g.ld_aff;
    const float aff = row[g.n_neg];
    int cnt = 0;
    for (int q = lane; q < g.n_neg; q += 64) cnt += row[q] >= aff ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if (lane == 0) {
        const float ls = logf(S);
        g.stats[2 * i] = M;
        g.stats[2 * i + 1] = ls;
        g.loss_rows[i] = (M + ls) - aff * g.inv_tau;
        g.rr_rows[i] = 1.0f / (float)(cnt + 1);
    }
}

__global__ __launch_bounds__(256) void infonce_grad_kernel(const NceArgs g, const StepEpilogue epi) {
    __shared__ __attribute__((aligned(16))) float smem[2 * RK_STAGE_FLOATS];
    __shared__ __attribute__((aligned(16))) float T[4 * NCE_CH];
    __shared__ int32_t cid1[RK_BN], cid2[RK_BN];
    __shared__ float cM[RK_BN], cL[RK_BN];
    __shared__ float red[2][4];

    const int wgU = g.tiles_m * g.nzU, wgC = g.tiles_c * g.nzC;
    if ((int)blockIdx.x == wgU + wgC) {                      // the step epilogue (the launch has this column only when asked)
        if (blockIdx.y == 0) gs_step_epilogue_block(epi, red[0], red[1]);
        return;
    }
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;
    const int64_t B = g.B, n_cand = g.B + g.n_neg;
    const bool has_ids = g.ids1 != nullptr;
    const int d = g.d;

    // role (workgroup-uniform): a row owner holds queries and sweeps candidates, a column owner the other way round
    const bool rows = (int)blockIdx.x < wgU;
    const int nz = rows ? g.nzU : g.nzC, per = rows ? g.perU : g.perC;
    const int bx = rows ? (int)blockIdx.x : (int)blockIdx.x - wgU;
    const int ptile = bx / nz, z = bx % nz;
    const float* P = rows ? g.U : g.C;
    const float* S = rows ? g.C : g.U;
    const int64_t ldp = rows ? g.ldu : g.ldc, lds_ = rows ? g.ldc : g.ldu;
    const int64_t n_p = rows ? B : n_cand, n_s = rows ? n_cand : B;
    // nz == 1: the rows of the output itself; else this cut's slab
    float* out = rows ? g.dU : g.dC;
    int64_t ldo = rows ? g.lddu : g.lddc;
    if (nz > 1) {
        out = (rows ? g.slabU : g.slabC) + (int64_t)z * n_p * g.d;
        ldo = g.d;
    }
    const int tiles_s = rows ? g.tiles_c : g.tiles_m;
    const int t0 = z * per, t1 = min(t0 + per, tiles_s);
    const int64_t p0 = (int64_t)ptile * RK_BM;
    const int col0 = blockIdx.y * 128;

    const int r = tid & 127, half = tid >> 7;
    const int64_t pr = p0 + r;
    int32_t my1 = 0, my2 = 0;
    float myM = 0.f, myL = 0.f;
    if (rows) {
        if (pr < B) {
            myM = g.stats[2 * pr];
            myL = g.stats[2 * pr + 1];
            if (has_ids) {
                my1 = g.ids1[pr];
                my2 = g.ids2[pr];
            }
        }
    } else if (has_ids && pr < B) {
        my2 = g.ids2[pr];
    }

    f32x16 oacc[2][2];
    rank_zero(oacc);

    // the swept rows' output columns, transposed into a B stage: lane k = tid & 31 takes swept row k of the chunk
    const int tk = tid & 31, tc = tid >> 5;

    for (int tile = t0; tile < t1; ++tile) {
        const int64_t s0 = (int64_t)tile * RK_BN;
        f32x16 acc[2][2];
        nce_tile(P, ldp, n_p, p0, S, lds_, n_s, s0, d, smem, wm, wn, l31, lh, acc);
        if (tid < RK_BN) {
            const int64_t c = s0 + tid;
            int32_t a1 = 0, a2 = 0;
            float vm = 0.f, vl = 0.f;
            if (c < B) {
                if (has_ids) {
                    a2 = g.ids2[c];
                    if (!rows) a1 = g.ids1[c];
                }
                if (!rows) {
                    vm = g.stats[2 * c];
                    vl = g.stats[2 * c + 1];
                }
            }
            cid1[tid] = a1; cid2[tid] = a2; cM[tid] = vm; cL[tid] = vl;
        }
        nce_dump(acc, T, wm, wn, l31, lh);
        __syncthreads();

        // ---- the logit tile becomes the G tile, in place
#pragma unroll 8
        for (int jj = 0; jj < 64; ++jj) {
            const int c = half * 64 + jj;
            const int64_t sc = s0 + c;
            const int64_t qi = rows ? pr : sc;               // query
            const int64_t cj = rows ? sc : pr;               // candidate
            float gv = 0.f;
            if (qi < B && cj < n_cand) {
                bool use = true;
                if (has_ids && cj < B && cj != qi) {
                    const int32_t j2 = rows ? cid2[c] : my2;
                    const int32_t i1 = rows ? my1 : cid1[c];
                    const int32_t i2 = rows ? my2 : cid2[c];
                    use = !(j2 == i2 || j2 == i1);
                }
                if (use) {
                    const float mm = rows ? myM : cM[c];
                    const float ll = rows ? myL : cL[c];
                    const float p = expf((T[nce_cell(r, c)] * g.inv_tau - mm) - ll);
                    gv = g.gscale * (p - (cj == qi ? 1.0f : 0.f));
                }
            }
            T[nce_cell(r, c)] = gv;
        }

        // ---- oacc += G[128 x 128] . S[s0 .. s0 + 128, col0 .. col0 + 128): four chunks of 32 swept rows
        f32x4 sv[4];
        auto load_chunk = [&](const int ch) {
            const int64_t srow = s0 + ch * 32 + tk;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int cc = col0 + (p * 8 + tc) * 4;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (srow < n_s && cc < d) v = *reinterpret_cast<const f32x4*>(S + srow * lds_ + cc);
                sv[p] = v;
            }
        };
        load_chunk(0);
        for (int ch = 0; ch < 4; ++ch) {
            float* Bs = rank_stage_b(smem, ch & 1);
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int cc = (p * 8 + tc) * 4;
                Bs[(cc + 0) * RK_KP + tk] = sv[p].x;
                Bs[(cc + 1) * RK_KP + tk] = sv[p].y;
                Bs[(cc + 2) * RK_KP + tk] = sv[p].z;
                Bs[(cc + 3) * RK_KP + tk] = sv[p].w;
            }
            __syncthreads();               // (ch == 0: also the G tile is complete)
            if (ch + 1 < 4) load_chunk(ch + 1);
            rank_compute(T + ch * NCE_CH, Bs, wm, wn, l31, lh, oacc);
        }
        __syncthreads();                   // T, the column arrays and the stage buffers change hands
    }

#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int64_t row = p0 + wm * 64 + tm * 32 + rank_acc_row(e, lh);
                const int col = col0 + wn * 64 + tn * 32 + l31;
                if (row < n_p && col < d) out[row * ldo + col] = oacc[tm][tn][e];
            }
}

// the step epilogue alone (a forward-only step has no gradient launch to carry it)
__global__ __launch_bounds__(256) void infonce_epilogue_kernel(const StepEpilogue epi) {
    __shared__ float red[2][4];
    gs_step_epilogue_block(epi, red[0], red[1]);
}

// out = slab 0 + slab 1 + .. in that order, one float4 per thread: the rows of dU first, then the rows of dC (a side whose sweep
// was not cut was written in place and is skipped).  The last workgroup is the step epilogue when the launch has one.
__global__ __launch_bounds__(256) void infonce_reduce_kernel(const NceArgs g, const int64_t n4U, const int64_t n4C, const int64_t wgs,
                                                             const StepEpilogue epi) {
    __shared__ float red[2][4];
    if ((int64_t)blockIdx.x == wgs) {
        gs_step_epilogue_block(epi, red[0], red[1]);
        return;
    }
    int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int d4 = g.d >> 2;
    const bool sideU = e < n4U;
    if (!sideU) e -= n4U;
    if (!sideU && e >= n4C) return;
    const int nz = sideU ? g.nzU : g.nzC;
    if (nz <= 1) return;
    const int64_t rows = sideU ? g.B : g.B + g.n_neg;
    const f32x4* sp = reinterpret_cast<const f32x4*>(sideU ? g.slabU : g.slabC) + e;
    f32x4 v = sp[0];
    for (int z = 1; z < nz; ++z) v += sp[(int64_t)z * rows * d4];
    const int64_t row = e / d4;
    const int c4 = (int)(e % d4);
    float* out = sideU ? g.dU + row * g.lddu : g.dC + row * g.lddc;
    *reinterpret_cast<f32x4*>(out + 4 * c4) = v;
}

#define NCE_MAX_CUT 8                   // at most this many workgroups share one owner's sweep (the slabs stay linear in B)

// the layout of the workspace: stats [B, 2] | part [tiles_c, B, 2] | slabs of dU | slabs of dC, every piece whole float4
struct NcePlan {
    int32_t tiles_m, tiles_c, nzU, perU, nzC, perC;
    int64_t off_part, off_slabU, off_slabC, floats;
};
static NcePlan nce_plan(const int64_t B, const int32_t d, const int32_t n_neg, const bool train) {
    NcePlan p;
    p.tiles_m = (int32_t)gs_ceil_div(B, RK_BM);
    p.tiles_c = (int32_t)gs_ceil_div(B + n_neg, RK_BN);
    p.perU = (int32_t)gs_ceil_div(p.tiles_c, NCE_MAX_CUT);
    p.nzU = (int32_t)gs_ceil_div(p.tiles_c, p.perU);
    p.perC = (int32_t)gs_ceil_div(p.tiles_m, NCE_MAX_CUT);
    p.nzC = (int32_t)gs_ceil_div(p.tiles_m, p.perC);
    p.off_part = 4 * gs_ceil_div(2 * B, 4);
    p.off_slabU = p.off_part + 4 * gs_ceil_div(2 * (int64_t)p.tiles_c * B, 4);
    p.off_slabC = p.off_slabU + ((train && p.nzU > 1) ? (int64_t)p.nzU * B * d : 0);
    p.floats = p.off_slabC + ((train && p.nzC > 1) ? (int64_t)p.nzC * (B + n_neg) * d : 0);
    return p;
}

#define NCE_MAX_CAND (65535ll * RK_BN)  // the candidate tiles are gridDim.y of the stats launch

static bool nce_sizes_ok(const int64_t B, const int32_t d, const int32_t n_neg) {
    return (d == 64 || d == 128 || d == 256 || d == 512) && B >= 1 && n_neg >= 0 && B + (int64_t)n_neg <= NCE_MAX_CAND;
}

extern "C" int gs_linkpred_infonce_ws_floats(int64_t B, int32_t d, int32_t n_neg, int train, int64_t* floats_out_host) {
    GS_REQUIRE(d == 64 || d == 128 || d == 256 || d == 512, "gs_linkpred_infonce_ws_floats: d must be 64/128/256/512 (got %d)", d);
    GS_REQUIRE(floats_out_host && nce_sizes_ok(B, d, n_neg), "gs_linkpred_infonce_ws_floats: bad args B=%lld n_neg=%d (B >= 1, n_neg >= 0, B + n_neg <= %lld)", (long long)B, n_neg,
               (long long)NCE_MAX_CAND);
    *floats_out_host = nce_plan(B, d, n_neg, train != 0).floats;
    return GS_OK;
}

static int infonce_launch(const char* who, const float* X, int64_t ldx, const float* U, int64_t ldu, int64_t B, int32_t d,
                          int32_t n_neg, float tau, float scale, const int32_t* ids1, const int32_t* ids2, float* loss_rows,
                          float* rr_rows, float* aff_all, int64_t ld_aff, float* ws, int64_t ws_floats, float* dX, int64_t lddx,
                          float* dU, int64_t lddu, const StepEpilogue* epi, void* stream) {
    GS_REQUIRE(d == 64 || d == 128 || d == 256 || d == 512, "%s: d must be 64/128/256/512 (got %d)", who, d);
    GS_REQUIRE(nce_sizes_ok(B, d, n_neg), "%s: bad sizes B=%lld n_neg=%d (B >= 1, n_neg >= 0, B + n_neg <= %lld)", who,
               (long long)B, n_neg, (long long)NCE_MAX_CAND);
    GS_REQUIRE(tau >= 0.01f && tau <= 10.0f, "%s: the temperature must lie in [0.01, 10] (got %g)", who, (double)tau);
    GS_CHECK_MAT(X, ldx, who);
    GS_CHECK_MAT(U, ldu, who);
    GS_REQUIRE(ldx >= d && ldu >= d, "%s: ldx / ldu must be >= d", who);
    GS_REQUIRE(loss_rows && rr_rows, "%s: loss_rows and rr_rows must be non-null", who);
    GS_REQUIRE(aff_all && ld_aff >= (int64_t)n_neg + 1, "%s: aff_all must be non-null with ld_aff >= n_neg + 1", who);
    GS_REQUIRE((ids1 == nullptr) == (ids2 == nullptr), "%s: ids1 and ids2 must be given together", who);
    GS_REQUIRE((dU == nullptr) == (dX == nullptr), "%s: dU and dX must both be given or both be null (forward only)", who);
    if (dU) {
        GS_CHECK_MAT(dX, lddx, who);
        GS_CHECK_MAT(dU, lddu, who);
        GS_REQUIRE(lddx >= d && lddu >= d, "%s: lddx / lddu must be >= d", who);
    }
    const NcePlan p = nce_plan(B, d, n_neg, dU != nullptr);
    GS_REQUIRE(ws && gs_aligned16(ws) && ws_floats >= p.floats,
               "%s: needs a 16-byte aligned workspace of %lld floats (gs_linkpred_infonce_ws_floats), got %lld", who,
               (long long)p.floats, (long long)ws_floats);
    NceArgs g;
    g.U = U; g.ldu = ldu; g.C = X + B * ldx; g.ldc = ldx;
    g.ids1 = ids1; g.ids2 = ids2;
    g.stats = ws; g.part = ws + p.off_part; g.slabU = ws + p.off_slabU; g.slabC = ws + p.off_slabC;
    g.nzU = p.nzU; g.perU = p.perU; g.nzC = p.nzC; g.perC = p.perC;
    g.loss_rows = loss_rows; g.rr_rows = rr_rows; g.aff_all = aff_all; g.ld_aff = ld_aff;
    g.dU = dU; g.lddu = lddu; g.dC = dX ? dX + B * lddx : nullptr; g.lddc = lddx;
    g.B = B; g.n_neg = n_neg; g.d = d;
    g.tiles_m = p.tiles_m; g.tiles_c = p.tiles_c;
    g.inv_tau = 1.0f / tau;
    g.gscale = scale / tau;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(infonce_stats_kernel, dim3((unsigned)g.tiles_m, (unsigned)g.tiles_c), dim3(256), 0, st, g);
    GS_LAUNCH_CHECK("infonce_stats_kernel");
    hipLaunchKernelGGL(infonce_finish_kernel, dim3((unsigned)gs_ceil_div(B, 4)), dim3(256), 0, st, g);
    GS_LAUNCH_CHECK("infonce_finish_kernel");
    const StepEpilogue none = {};
    if (!dU) {
        if (epi) {
            hipLaunchKernelGGL(infonce_epilogue_kernel, dim3(1), dim3(256), 0, st, *epi);
            GS_LAUNCH_CHECK("infonce_epilogue_kernel");
        }
        return GS_OK;
    }
    const bool reduce = p.nzU > 1 || p.nzC > 1;
    const unsigned gx = (unsigned)(g.tiles_m * g.nzU + g.tiles_c * g.nzC + ((epi && !reduce) ? 1 : 0));
    hipLaunchKernelGGL(infonce_grad_kernel, dim3(gx, (unsigned)gs_ceil_div(d, 128)), dim3(256), 0, st, g,
                       (epi && !reduce) ? *epi : none);
    GS_LAUNCH_CHECK("infonce_grad_kernel");
    if (reduce) {
        const int64_t n4U = B * (d >> 2), n4C = (B + n_neg) * (d >> 2);
        const int64_t wgs = gs_ceil_div(n4U + n4C, 256);
        hipLaunchKernelGGL(infonce_reduce_kernel, dim3((unsigned)(wgs + (epi ? 1 : 0))), dim3(256), 0, st, g, n4U, n4C, wgs,
                           epi ? *epi : none);
        GS_LAUNCH_CHECK("infonce_reduce_kernel");
    }
    return GS_OK;
}

extern "C" int gs_linkpred_infonce_fwd_bwd(const float* X, int64_t ldx, const float* U, int64_t ldu, int64_t B, int32_t d,
                                           int32_t n_neg, float tau, float scale, const int32_t* ids1, const int32_t* ids2,
                                           float* loss_rows, float* rr_rows, float* aff_all, int64_t ld_aff, float* ws,
                                           int64_t ws_floats, float* dX, int64_t lddx, float* dU, int64_t lddu, void* stream) {
    return infonce_launch("gs_linkpred_infonce_fwd_bwd", X, ldx, U, ldu, B, d, n_neg, tau, scale, ids1, ids2, loss_rows, rr_rows,
                          aff_all, ld_aff, ws, ws_floats, dX, lddx, dU, lddu, nullptr, stream);
}

extern "C" int gs_linkpred_infonce_fwd_bwd_step(const float* X, int64_t ldx, const float* U, int64_t ldu, int64_t B, int32_t d,
                                                int32_t n_neg, float tau, float scale, const int32_t* ids1, const int32_t* ids2,
                                                float* loss_rows, float* rr_rows, float* aff_all, int64_t ld_aff, float* ws,
                                                int64_t ws_floats, float* dX, int64_t lddx, float* dU, int64_t lddu,
                                                float* loss_out, int accumulate, float* mrr_out, uint64_t* c0, uint64_t d0,
                                                uint64_t* c1, uint64_t d1, uint64_t* c2, uint64_t d2, void* stream) {
    GS_REQUIRE(loss_out && mrr_out, "gs_linkpred_infonce_fwd_bwd_step: loss_out / mrr_out missing");
    GS_REQUIRE(B >= 1, "gs_linkpred_infonce_fwd_bwd_step: B must be >= 1");
    const float inv_b = 1.0f / (float)B;
    const StepEpilogue epi = {loss_rows, B, inv_b, loss_out, accumulate, rr_rows, inv_b, mrr_out, c0, d0, c1, d1, c2, d2};
    return infonce_launch("gs_linkpred_infonce_fwd_bwd_step", X, ldx, U, ldu, B, d, n_neg, tau, scale, ids1, ids2, loss_rows,
                          rr_rows, aff_all, ld_aff, ws, ws_floats, dX, lddx, dU, lddu, &epi, stream);
}
