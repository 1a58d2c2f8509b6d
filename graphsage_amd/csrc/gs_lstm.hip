// LSTM neighbor aggregator (SeqAggregator, graphsage/aggregators.py:363-449): the recurrence of TF 1.x BasicLSTMCell under
// dynamic_rnn(sequence_length = L) over every neighbor sequence of a layer, all hops in ONE launch (one segment per hop,
// each with its own step count T).  The input projection G = X . W_x + b of all n*T neighbor rows and every weight / input
// gradient are ordinary contractions of the existing kernels; what lives here is what they cannot do:
//
//   gs_lstm_lengths  L_r = max(1, #{t < T : max_j |x[r, t, j]| > 0})          (aggregators.py:411-414)
//   gs_lstm_fwd      for t < L_r:  [i j f o] = G[r, t] + h_{t-1} . W_h
//                                  c_t = c_{t-1} sigma(f + 1) + sigma(i) tanh(j),   h_t = tanh(c_t) sigma(o)
//                    h_last[r] = h_{L_r - 1}; saved for the backward: activated gates, c_t, h_{t-1}
//   gs_lstm_bwd      BPTT from d h_last: dG[r, t] (zero for t >= L_r), dh / dc carried backwards through W_h^T
//
// Layout: a workgroup owns a tile of LSTM_TILE sequences of one segment for all of its steps; it has 4H threads, thread
// (g = tid / H, j = tid % H).  In the gate contraction thread (g, j) owns gate column g*H + j for all sequences of the
// tile (W_h is read from L2 once per workgroup and step, coalesced along j); in the cell update it owns hidden unit j of
// sequences 4g .. 4g+3 (c_t lives in its registers).  h_{t-1} and the gate pre-activations pass through LDS, two
// barriers per step.  fp32 throughout (FMA on the vector ALUs): the recurrence runs up to 25 dependent steps.
#include <string.h>

#include "gs_common.h"

static_assert(sizeof(gs_lstm_seg) == 56, "gs_lstm_seg layout (mirrored by graphsage_amd/_lib.py LstmSeg)");

#define LSTM_TILE 16   // sequences per workgroup
#define LSTM_QPT 4     // sequences per thread in the cell update (LSTM_TILE / 4 gate groups)

struct LstmSegK {
    const float* X;
    const int32_t* ids;
    int64_t ldx, n, row0, seq0;
    int32_t T;
};
struct LstmSegs {
    LstmSegK s[GS_LSTM_MAX_SEG];
    int64_t tile0[GS_LSTM_MAX_SEG + 1];   // first workgroup of each segment
    int32_t n_seg;
};

__device__ __forceinline__ int lstm_find_seg(const LstmSegs& S, int64_t b) {
    int k = 0;
    while (k + 1 < S.n_seg && b >= S.tile0[k + 1]) ++k;
    return k;
}

__device__ __forceinline__ float lstm_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---- lengths: one wave per sequence ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lstm_lengths_kernel(LstmSegs S, int32_t d, int64_t n_total, int32_t* __restrict__ L) {
    const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (gw >= n_total) return;
    int k = 0;
    while (k + 1 < S.n_seg && gw >= S.s[k + 1].seq0) ++k;
    const LstmSegK& g = S.s[k];
    const int64_t r = gw - g.seq0;
    int count = 0;
    for (int t = 0; t < g.T; ++t) {
        const int64_t row = r * g.T + t;                       // row within the segment's inputs
        const int64_t src = g.ids ? (int64_t)g.ids[row] : row;
        const float* x = g.X + src * g.ldx;
        bool nz = false;
        for (int c = lane; c < d; c += 64) nz |= (x[c] != 0.0f);
        if (__any(nz)) ++count;
    }
    if (lane == 0) L[gw] = count > 1 ? count : 1;
}

// ---- forward recurrence ---------------------------------------------------------------------------------------
template <int H>
__global__ __launch_bounds__(4 * H) void lstm_fwd_kernel(LstmSegs S, const float* W_h, int64_t ldw,
                                                         const int32_t* __restrict__ L, const float* G, int64_t ldg,
                                                         float* A, int64_t lda, float* __restrict__ C, int64_t ldc,
                                                         float* __restrict__ Hp, int64_t ldhp, float* __restrict__ h_last,
                                                         int64_t ldh) {
    __shared__ float h_sh[LSTM_TILE][H];
    __shared__ float g_sh[LSTM_TILE][4 * H];
    const int tid = threadIdx.x;
    const int g = tid / H, j = tid - g * H;
    const int k = lstm_find_seg(S, blockIdx.x);
    const LstmSegK seg = S.s[k];
    const int64_t r0 = (blockIdx.x - S.tile0[k]) * LSTM_TILE;     // first sequence of the tile (within the segment)
    const int T = seg.T;
    int tmax = 0;
    for (int q = 0; q < LSTM_TILE; ++q)
        if (r0 + q < seg.n) tmax = max(tmax, L[seg.seq0 + r0 + q]);
    // this thread's sequences in the cell update: 4g + i
    int len[LSTM_QPT];
    float c[LSTM_QPT], h[LSTM_QPT];
#pragma unroll
    for (int i = 0; i < LSTM_QPT; ++i) {
        const int64_t r = r0 + LSTM_QPT * g + i;
        len[i] = r < seg.n ? L[seg.seq0 + r] : 0;
        c[i] = 0.f;
        h[i] = 0.f;
        h_sh[LSTM_QPT * g + i][j] = 0.f;
    }
    const int col = g * H + j;
    __syncthreads();
    for (int t = 0; t < tmax; ++t) {
        // gate column `col` of every sequence of the tile: h_{t-1} . W_h[:, col]
        float acc[LSTM_TILE];
#pragma unroll
        for (int q = 0; q < LSTM_TILE; ++q) acc[q] = 0.f;
        const float* w = W_h + col;
#pragma unroll 4
        for (int kk = 0; kk < H; ++kk) {
            const float wv = w[(int64_t)kk * ldw];
#pragma unroll
            for (int q = 0; q < LSTM_TILE; ++q) acc[q] = fmaf(h_sh[q][kk], wv, acc[q]);
        }
#pragma unroll
        for (int q = 0; q < LSTM_TILE; ++q) g_sh[q][col] = acc[q];
        __syncthreads();
        // cell update of unit j for sequences 4g .. 4g+3
#pragma unroll
        for (int i = 0; i < LSTM_QPT; ++i) {
            const int q = LSTM_QPT * g + i;
            if (t < len[i]) {
                const int64_t row = seg.row0 + (r0 + q) * T + t;
                const float* gx = G + row * ldg;
                const float pi = g_sh[q][j] + gx[j];
                const float pj = g_sh[q][H + j] + gx[H + j];
                const float pf = g_sh[q][2 * H + j] + gx[2 * H + j];
                const float po = g_sh[q][3 * H + j] + gx[3 * H + j];
                const float ai = lstm_sigmoid(pi), aj = tanhf(pj), af = lstm_sigmoid(pf + 1.0f), ao = lstm_sigmoid(po);
                Hp[row * ldhp + j] = h[i];
                c[i] = c[i] * af + ai * aj;
                h[i] = tanhf(c[i]) * ao;
                float* a = A + row * lda;        // (may alias G: this thread read these four elements above)
                a[j] = ai;
                a[H + j] = aj;
                a[2 * H + j] = af;
                a[3 * H + j] = ao;
                C[row * ldc + j] = c[i];
                h_sh[q][j] = h[i];
            }
        }
        __syncthreads();
    }
    // rows past a sequence's length: h_{t-1} = 0 (their dG is zero; the weight gradient H_prev^T . dG then reads no stale data)
#pragma unroll
    for (int i = 0; i < LSTM_QPT; ++i) {
        const int64_t r = r0 + LSTM_QPT * g + i;
        if (r < seg.n) {
            for (int t = len[i]; t < T; ++t) Hp[(seg.row0 + r * T + t) * ldhp + j] = 0.f;
            h_last[(seg.seq0 + r) * ldh + j] = h[i];
        }
    }
}

// ---- W_h^T (the backward's dh = dG . W_h^T reads it along rows) ------------------------------------------------
__global__ __launch_bounds__(256) void lstm_transpose_kernel(const float* __restrict__ W, int64_t ldw, int32_t rows,
                                                             int32_t cols, float* __restrict__ WT) {
    const int64_t total = (int64_t)rows * cols;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t cidx = e / rows;              // output row = input column
        const int r = (int)(e - cidx * rows);
        WT[cidx * rows + r] = W[(int64_t)r * ldw + cidx];
    }
}

// ---- backward recurrence (BPTT) -------------------------------------------------------------------------------
template <int H>
__global__ __launch_bounds__(4 * H) void lstm_bwd_kernel(LstmSegs S, const float* __restrict__ WT,
                                                         const int32_t* __restrict__ L, const float* A, int64_t lda,
                                                         const float* __restrict__ C, int64_t ldc,
                                                         const float* __restrict__ dh_last, int64_t lddh, float* dG,
                                                         int64_t lddg) {
    __shared__ float dg_sh[LSTM_TILE][4 * H];
    __shared__ float p_sh[4][LSTM_TILE][H];
    const int tid = threadIdx.x;
    const int g = tid / H, j = tid - g * H;
    const int k = lstm_find_seg(S, blockIdx.x);
    const LstmSegK seg = S.s[k];
    const int64_t r0 = (blockIdx.x - S.tile0[k]) * LSTM_TILE;
    const int T = seg.T;
    int tmax = 0;
    for (int q = 0; q < LSTM_TILE; ++q)
        if (r0 + q < seg.n) tmax = max(tmax, L[seg.seq0 + r0 + q]);
    int len[LSTM_QPT];
    float dc[LSTM_QPT], dh[LSTM_QPT];
#pragma unroll
    for (int i = 0; i < LSTM_QPT; ++i) {
        const int64_t r = r0 + LSTM_QPT * g + i;
        len[i] = r < seg.n ? L[seg.seq0 + r] : 0;
        dc[i] = 0.f;
        dh[i] = 0.f;
        if (r < seg.n)              // steps past the length take no gradient
            for (int t = len[i]; t < T; ++t) {
                float* o = dG + (seg.row0 + r * T + t) * lddg;
                o[j] = 0.f;
                o[H + j] = 0.f;
                o[2 * H + j] = 0.f;
                o[3 * H + j] = 0.f;
            }
    }
    for (int t = tmax - 1; t >= 0; --t) {
#pragma unroll
        for (int i = 0; i < LSTM_QPT; ++i) {
            const int q = LSTM_QPT * g + i;
            float gi = 0.f, gj = 0.f, gf = 0.f, go = 0.f;
            if (t < len[i]) {
                const int64_t r = r0 + q;
                const int64_t row = seg.row0 + r * T + t;
                float dht = dh[i];
                if (t == len[i] - 1) dht += dh_last[(seg.seq0 + r) * lddh + j];
                const float* a = A + row * lda;
                const float ai = a[j], aj = a[H + j], af = a[2 * H + j], ao = a[3 * H + j];
                const float ct = C[row * ldc + j];
                const float cp = t > 0 ? C[(row - 1) * ldc + j] : 0.f;
                const float tc = tanhf(ct);
                const float dct = dc[i] + dht * ao * (1.0f - tc * tc);
                go = dht * tc * ao * (1.0f - ao);
                gi = dct * aj * ai * (1.0f - ai);
                gj = dct * ai * (1.0f - aj * aj);
                gf = dct * cp * af * (1.0f - af);
                dc[i] = dct * af;
                float* o = dG + row * lddg;     // (may alias A: this thread read these four elements above)
                o[j] = gi;
                o[H + j] = gj;
                o[2 * H + j] = gf;
                o[3 * H + j] = go;
            }
            dg_sh[q][j] = gi;
            dg_sh[q][H + j] = gj;
            dg_sh[q][2 * H + j] = gf;
            dg_sh[q][3 * H + j] = go;
        }
        __syncthreads();
        if (t == 0) break;
        // dh_{t-1}[q, j] = sum_c dG[q, c] W_h[j, c]: thread (g, j) sums over the columns of gate g, the four partial sums meet in LDS
        float acc[LSTM_TILE];
#pragma unroll
        for (int q = 0; q < LSTM_TILE; ++q) acc[q] = 0.f;
        const float* w = WT + (int64_t)g * H * H + j;
#pragma unroll 4
        for (int kk = 0; kk < H; ++kk) {
            const float wv = w[(int64_t)kk * H];
#pragma unroll
            for (int q = 0; q < LSTM_TILE; ++q) acc[q] = fmaf(dg_sh[q][g * H + kk], wv, acc[q]);
        }
#pragma unroll
        for (int q = 0; q < LSTM_TILE; ++q) p_sh[g][q][j] = acc[q];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < LSTM_QPT; ++i) {
            const int q = LSTM_QPT * g + i;
            dh[i] = (p_sh[0][q][j] + p_sh[1][q][j]) + (p_sh[2][q][j] + p_sh[3][q][j]);
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------
static int lstm_segs(const gs_lstm_seg* segs_host, int32_t n_seg, const char* who, LstmSegs* out, int64_t* n_total,
                     int64_t* rows_total) {
    GS_REQUIRE(segs_host && n_seg >= 1 && n_seg <= GS_LSTM_MAX_SEG, "%s: 1 <= n_seg <= %d segments", who, GS_LSTM_MAX_SEG);
    LstmSegs S;
    memset(&S, 0, sizeof(S));
    S.n_seg = n_seg;
    int64_t tiles = 0, seqs = 0, rows = 0;
    for (int k = 0; k < n_seg; ++k) {
        const gs_lstm_seg& g = segs_host[k];
        GS_REQUIRE(g.n >= 0 && g.T >= 1 && g.row0 >= 0 && g.seq0 >= 0, "%s: segment %d: n >= 0, T >= 1, row0, seq0 >= 0", who, k);
        GS_REQUIRE(g.seq0 == seqs, "%s: segment %d: seq0 must continue the previous segment's sequences", who, k);
        S.s[k].X = g.X; S.s[k].ids = g.ids; S.s[k].ldx = g.ldx;
        S.s[k].n = g.n; S.s[k].row0 = g.row0; S.s[k].seq0 = g.seq0; S.s[k].T = g.T;
        S.tile0[k] = tiles;
        tiles += gs_ceil_div(g.n, LSTM_TILE);
        seqs += g.n;
        rows = std::max(rows, g.row0 + g.n * (int64_t)g.T);
    }
    S.tile0[n_seg] = tiles;
    for (int k = n_seg + 1; k <= GS_LSTM_MAX_SEG; ++k) S.tile0[k] = tiles;
    // empty segments own no workgroup: the segment search skips them because their tile0 equals the next one's
    *out = S;
    *n_total = seqs;
    *rows_total = rows;
    return GS_OK;
}

extern "C" int gs_lstm_lengths(const gs_lstm_seg* segs_host, int32_t n_seg, int32_t d, int32_t* lengths, void* stream) {
    LstmSegs S;
    int64_t n_total = 0, rows = 0;
    int rc = lstm_segs(segs_host, n_seg, "gs_lstm_lengths", &S, &n_total, &rows);
    if (rc != GS_OK) return rc;
    GS_REQUIRE(lengths && d >= 1, "gs_lstm_lengths: lengths must be non-null, d >= 1");
    for (int k = 0; k < n_seg; ++k)
        GS_REQUIRE(segs_host[k].n == 0 || (segs_host[k].X && segs_host[k].ldx >= d),
                   "gs_lstm_lengths: segment %d needs its input rows X (ldx >= d)", k);
    if (n_total == 0) return GS_OK;
    hipLaunchKernelGGL(lstm_lengths_kernel, dim3((unsigned)gs_ceil_div(n_total, 4)), dim3(256), 0, (hipStream_t)stream, S, d,
                       n_total, lengths);
    GS_LAUNCH_CHECK("lstm_lengths_kernel");
    return GS_OK;
}

extern "C" int gs_lstm_fwd(const gs_lstm_seg* segs_host, int32_t n_seg, int32_t H, const float* W_h, int64_t ldw,
                           const int32_t* lengths, const float* G, int64_t ldg, float* A, int64_t lda, float* C, int64_t ldc,
                           float* H_prev, int64_t ldhp, float* h_last, int64_t ldh, void* stream) {
    LstmSegs S;
    int64_t n_total = 0, rows = 0;
    int rc = lstm_segs(segs_host, n_seg, "gs_lstm_fwd", &S, &n_total, &rows);
    if (rc != GS_OK) return rc;
    GS_REQUIRE(H == 128 || H == 256, "gs_lstm_fwd: hidden size %d (supported: 128, 256)", H);
    GS_REQUIRE(W_h && lengths && G && A && C && H_prev && h_last, "gs_lstm_fwd: null pointer");
    GS_REQUIRE(ldw >= 4 * H && ldg >= 4 * H && lda >= 4 * H && ldc >= H && ldhp >= H && ldh >= H, "gs_lstm_fwd: bad leading dimension");
    GS_REQUIRE(G != A || ldg == lda, "gs_lstm_fwd: G may alias A only with the same leading dimension");
    if (n_total == 0) return GS_OK;
    const unsigned blocks = (unsigned)S.tile0[n_seg];
    if (H == 128)
        hipLaunchKernelGGL(lstm_fwd_kernel<128>, dim3(blocks), dim3(512), 0, (hipStream_t)stream, S, W_h, ldw, lengths, G, ldg,
                           A, lda, C, ldc, H_prev, ldhp, h_last, ldh);
    else
        hipLaunchKernelGGL(lstm_fwd_kernel<256>, dim3(blocks), dim3(1024), 0, (hipStream_t)stream, S, W_h, ldw, lengths, G, ldg,
                           A, lda, C, ldc, H_prev, ldhp, h_last, ldh);
    GS_LAUNCH_CHECK("lstm_fwd_kernel");
    return GS_OK;
}

extern "C" int gs_lstm_bwd(const gs_lstm_seg* segs_host, int32_t n_seg, int32_t H, const float* W_h, int64_t ldw, float* W_hT_ws,
                           const int32_t* lengths, const float* A, int64_t lda, const float* C, int64_t ldc,
                           const float* dh_last, int64_t lddh, float* dG, int64_t lddg, void* stream) {
    LstmSegs S;
    int64_t n_total = 0, rows = 0;
    int rc = lstm_segs(segs_host, n_seg, "gs_lstm_bwd", &S, &n_total, &rows);
    if (rc != GS_OK) return rc;
    GS_REQUIRE(H == 128 || H == 256, "gs_lstm_bwd: hidden size %d (supported: 128, 256)", H);
    GS_REQUIRE(W_h && W_hT_ws && lengths && A && C && dh_last && dG, "gs_lstm_bwd: null pointer");
    GS_REQUIRE(ldw >= 4 * H && lda >= 4 * H && ldc >= H && lddh >= H && lddg >= 4 * H, "gs_lstm_bwd: bad leading dimension");
    GS_REQUIRE(A != dG || lda == lddg, "gs_lstm_bwd: dG may alias A only with the same leading dimension");
    if (n_total == 0) return GS_OK;
    hipLaunchKernelGGL(lstm_transpose_kernel, dim3((unsigned)gs_ceil_div(4 * H * H, 256)), dim3(256), 0, (hipStream_t)stream, W_h,
                       ldw, H, 4 * H, W_hT_ws);
    GS_LAUNCH_CHECK("lstm_transpose_kernel");
    const unsigned blocks = (unsigned)S.tile0[n_seg];
    if (H == 128)
        hipLaunchKernelGGL(lstm_bwd_kernel<128>, dim3(blocks), dim3(512), 0, (hipStream_t)stream, S, W_hT_ws, lengths, A, lda, C,
                           ldc, dh_last, lddh, dG, lddg);
    else
        hipLaunchKernelGGL(lstm_bwd_kernel<256>, dim3(blocks), dim3(1024), 0, (hipStream_t)stream, S, W_hT_ws, lengths, A, lda, C,
                           ldc, dh_last, lddh, dG, lddg);
    GS_LAUNCH_CHECK("lstm_bwd_kernel");
    return GS_OK;
}
