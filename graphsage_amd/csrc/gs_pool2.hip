// K4, two-layer max-pool (TwoMaxLayerPoolingAggregator): the input gradient of the FIRST dense layer's activations from
// the gradient of the pooled SECOND layer, without the [n*s, hid2] matrix between them.
//
//   dH1[i*s + j, k] = H1[h(i*s + j), k] > 0 ?  sum over { c : argmax[i, c] == j } of dpm[i, c] * W2[k, c]  :  0
//
// One 256-thread workgroup per group i.  The group's columns are bucketed by winning row with a STABLE counting sort in LDS
// (every row's column list stays ascending, so the sum runs in ascending c: one fixed order); columns whose dpm is exactly 0
// add nothing and are dropped in the sort.  Then wave w takes rows w, w + 4, ..: a lane owns float4s of k and walks the row's
// list, reading W2^T [hid2, hid1] rows coalesced along k (W2 itself would be read at a stride of ldw per lane).  The relu
// mask of H1 is applied in the store; every row of the group is stored, rows that won nothing as zeros.
#include "gs_common.h"

#define GS_P2_THREADS 256
#define GS_P2_MAX_HID2 1024
#define GS_P2_MAX_S 64
#define GS_P2_SEGS (GS_P2_MAX_HID2 / GS_WAVE)   // 64-column segments of a group's row
#define GS_P2_PASSES (GS_P2_MAX_HID2 / GS_P2_THREADS)
#define GS_P2_U 4                                // float4s of k per lane and trip

__global__ __launch_bounds__(GS_P2_THREADS) void pool2_dgrad_kernel(const float* __restrict__ dpm, int64_t ldd,
                                                                    const int32_t* __restrict__ argmax, int64_t lda,
                                                                    const float* __restrict__ W2T, int64_t ldt,
                                                                    const float* __restrict__ H1, int64_t ldh,
                                                                    const int32_t* __restrict__ h_idx, int32_t s, int32_t hid1,
                                                                    int32_t hid2, float* __restrict__ dH1, int64_t ldo) {
    __shared__ float l_val[GS_P2_MAX_HID2];               // the sorted lists: dpm value ...
    __shared__ int32_t l_col[GS_P2_MAX_HID2];             // ... and column
    __shared__ int32_t seg_cnt[GS_P2_SEGS][GS_P2_MAX_S];  // columns of (segment, row); then their offset inside the row's list
    __shared__ int32_t row_start[GS_P2_MAX_S], row_cnt[GS_P2_MAX_S];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i = blockIdx.x;
    const int n_seg = (hid2 + 63) >> 6;
    for (int t = tid; t < n_seg * GS_P2_MAX_S; t += GS_P2_THREADS) (&seg_cnt[0][0])[t] = 0;
    __syncthreads();
    // ---- rank of every live column among the earlier columns of its segment with the same winner (six ballots)
    float v[GS_P2_PASSES];
    int32_t a[GS_P2_PASSES], rank[GS_P2_PASSES];
    const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
    for (int p = 0; p < GS_P2_PASSES; ++p) {
        const int c = p * GS_P2_THREADS + tid;            // wave-uniform whether the segment exists at all
        v[p] = 0.f; a[p] = -1; rank[p] = 0;
        if (p * GS_P2_THREADS + wave * 64 >= hid2) continue;
        if (c < hid2) {
            v[p] = dpm[i * ldd + c];
            const int32_t w = argmax[i * lda + c];
            a[p] = (v[p] != 0.f && (uint32_t)w < (uint32_t)s) ? w : -1;   // an index outside [0, s) collects nowhere
        }
        const bool live = a[p] >= 0;
        uint64_t same = __ballot(live);
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            const uint64_t bit = __ballot(live && ((a[p] >> b) & 1));
            same &= ((a[p] >> b) & 1) ? bit : ~bit;
        }
        rank[p] = __popcll(same & below);
        if (live && rank[p] == 0) seg_cnt[p * (GS_P2_THREADS / 64) + wave][a[p]] = __popcll(same);
    }
    __syncthreads();
    // ---- list offsets: rows in order, inside a row its segments in order
    if (wave == 0) {
        int tot = 0;
        for (int g = 0; g < n_seg; ++g) {
            const int t = seg_cnt[g][lane];
            seg_cnt[g][lane] = tot;
            tot += t;
        }
        int inc = tot;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(inc, off, 64);
            if (lane >= off) inc += up;
        }
        row_start[lane] = inc - tot;
        row_cnt[lane] = tot;
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < GS_P2_PASSES; ++p) {
        if (a[p] >= 0) {
            const int pos = row_start[a[p]] + seg_cnt[p * (GS_P2_THREADS / 64) + wave][a[p]] + rank[p];
            l_col[pos] = p * GS_P2_THREADS + tid;
            l_val[pos] = v[p];
        }
    }
    __syncthreads();
    // ---- the rows
    const int nq = hid1 >> 2;
    for (int j = wave; j < s; j += GS_P2_THREADS / 64) {
        const int64_t r = i * s + j;
        const int64_t hr = h_idx ? (int64_t)h_idx[r] : r;
        const int t0 = row_start[j], t1 = t0 + row_cnt[j];
        for (int q0 = 0; q0 < nq; q0 += 64 * GS_P2_U) {
            f32x4 acc[GS_P2_U];
            bool on[GS_P2_U];
#pragma unroll
            for (int u = 0; u < GS_P2_U; ++u) {
                acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                on[u] = q0 + u * 64 + lane < nq;
            }
            for (int t = t0; t < t1; ++t) {
                const float x = l_val[t];
                const float* wrow = W2T + (int64_t)l_col[t] * ldt + 4 * (q0 + lane);
#pragma unroll
                for (int u = 0; u < GS_P2_U; ++u) {
                    if (on[u]) {
                        const f32x4 w = *reinterpret_cast<const f32x4*>(wrow + 256 * u);
                        acc[u].x = fmaf(x, w.x, acc[u].x); acc[u].y = fmaf(x, w.y, acc[u].y);
                        acc[u].z = fmaf(x, w.z, acc[u].z); acc[u].w = fmaf(x, w.w, acc[u].w);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < GS_P2_U; ++u) {
                if (on[u]) {
                    const int k = 4 * (q0 + u * 64 + lane);
                    const f32x4 h = *reinterpret_cast<const f32x4*>(H1 + hr * ldh + k);
                    f32x4 o;
                    o.x = h.x > 0.f ? acc[u].x : 0.f; o.y = h.y > 0.f ? acc[u].y : 0.f;
                    o.z = h.z > 0.f ? acc[u].z : 0.f; o.w = h.w > 0.f ? acc[u].w : 0.f;
                    *reinterpret_cast<f32x4*>(dH1 + r * ldo + k) = o;
                }
            }
        }
    }
}

// out[c, r] = W[r, c]: 32 x 32 tiles through LDS (padded rows), both sides coalesced
__global__ __launch_bounds__(256) void pool2_transpose_kernel(const float* __restrict__ W, int64_t ldw, int32_t rows, int32_t cols,
                                                              float* __restrict__ out, int64_t ldo) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    for (int y = ty; y < 32; y += 8)
        if (r0 + y < rows && c0 + tx < cols) tile[y][tx] = W[(int64_t)(r0 + y) * ldw + c0 + tx];
    __syncthreads();
    for (int y = ty; y < 32; y += 8)
        if (c0 + y < cols && r0 + tx < rows) out[(int64_t)(c0 + y) * ldo + r0 + tx] = tile[tx][y];
}

// out[i] = i: the row index gs_maxpool_sparse_wgrad reads H1 through when H1 already holds one row per sampled row
__global__ __launch_bounds__(256) void pool2_iota_kernel(int32_t* __restrict__ out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = (int32_t)i;
}

extern "C" int gs_pool2_iota(int32_t* out, int64_t n, void* stream) {
    if (n == 0) return GS_OK;
    GS_REQUIRE(out && n > 0 && n < (1ll << 31), "gs_pool2_iota: bad args");
    hipLaunchKernelGGL(pool2_iota_kernel, dim3((unsigned)std::min<int64_t>(gs_ceil_div(n, 256), 1024)), dim3(256), 0,
                       (hipStream_t)stream, out, n);
    GS_LAUNCH_CHECK("pool2_iota_kernel");
    return GS_OK;
}

static int pool2_supported(int32_t s, int32_t hid1, int32_t hid2, const char* who) {
    if (s < 1 || s > GS_P2_MAX_S || hid1 < 4 || hid2 < 4 || hid1 % 4 || hid2 % 4 || hid2 > GS_P2_MAX_HID2) {
        gs_set_error("%s: needs 1 <= s <= %d, hid1 %% 4 == 0, hid2 %% 4 == 0, hid2 <= %d (s=%d, hid1=%d, hid2=%d); use "
                     "gs_segment_max_bwd + gs_dense_dgrad + gs_act_bwd", who, GS_P2_MAX_S, GS_P2_MAX_HID2, s, hid1, hid2);
        return GS_ENOTSUP;
    }
    return GS_OK;
}

extern "C" int gs_pool2_transpose(const float* W, int64_t ldw, int32_t rows, int32_t cols, float* out, int64_t ldo, void* stream) {
    GS_REQUIRE(W && out && rows > 0 && cols > 0 && ldw >= cols && ldo >= rows, "gs_pool2_transpose: bad args");
    hipLaunchKernelGGL(pool2_transpose_kernel, dim3((unsigned)gs_ceil_div(cols, 32), (unsigned)gs_ceil_div(rows, 32)), dim3(256), 0,
                       (hipStream_t)stream, W, ldw, rows, cols, out, ldo);
    GS_LAUNCH_CHECK("pool2_transpose_kernel");
    return GS_OK;
}

extern "C" int gs_pool2_dgrad_t(const float* d_pooled_masked, int64_t ldd, const int32_t* argmax, int64_t lda, const float* W2T,
                                int64_t ldt, const float* H1, int64_t ldh, const int32_t* h_idx, int64_t n, int32_t s,
                                int32_t hid1, int32_t hid2, float* dH1, int64_t ldo, void* stream) {
    const int rc = pool2_supported(s, hid1, hid2, "gs_pool2_dgrad_t");
    if (rc != GS_OK) return rc;
    if (n == 0) return GS_OK;
    GS_CHECK_MAT(W2T, ldt, "gs_pool2_dgrad_t W2T");
    GS_CHECK_MAT(H1, ldh, "gs_pool2_dgrad_t H1");
    GS_CHECK_MAT(dH1, ldo, "gs_pool2_dgrad_t dH1");
    GS_REQUIRE(d_pooled_masked && argmax && n > 0 && n < (1ll << 31) && ldd >= hid2 && lda >= hid2 && ldt >= hid1 && ldh >= hid1 &&
               ldo >= hid1, "gs_pool2_dgrad_t: bad args");
    hipLaunchKernelGGL(pool2_dgrad_kernel, dim3((unsigned)n), dim3(GS_P2_THREADS), 0, (hipStream_t)stream, d_pooled_masked, ldd,
                       argmax, lda, W2T, ldt, H1, ldh, h_idx, s, hid1, hid2, dH1, ldo);
    GS_LAUNCH_CHECK("pool2_dgrad_kernel");
    return GS_OK;
}

// The self-contained form: W2 as the Dense stores it.  The transposed copy lives for the call (allocated and freed here, and
// hipFree waits for the launches), so this form cannot be captured into a graph; a training step keeps the copy in its own
// workspace (gs_pool2_transpose once per step) and calls gs_pool2_dgrad_t.
extern "C" int gs_pool2_dgrad(const float* d_pooled_masked, int64_t ldd, const int32_t* argmax, int64_t lda, const float* W2,
                              int64_t ldw, const float* H1, int64_t ldh, const int32_t* h_idx, int64_t n, int32_t s, int32_t hid1,
                              int32_t hid2, float* dH1, int64_t ldo, void* stream) {
    const int rc = pool2_supported(s, hid1, hid2, "gs_pool2_dgrad");
    if (rc != GS_OK) return rc;
    if (n == 0) return GS_OK;
    GS_REQUIRE(W2 && ldw >= hid2, "gs_pool2_dgrad: bad W2");
    float* wt = nullptr;
    GS_HIP(hipMalloc(&wt, (size_t)hid2 * hid1 * sizeof(float)));
    int st = gs_pool2_transpose(W2, ldw, hid1, hid2, wt, hid1, stream);
    if (st == GS_OK)
        st = gs_pool2_dgrad_t(d_pooled_masked, ldd, argmax, lda, wt, hid1, H1, ldh, h_idx, n, s, hid1, hid2, dH1, ldo, stream);
    const hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    (void)hipFree(wt);
    if (st == GS_OK && e != hipSuccess) {
        gs_set_error("gs_pool2_dgrad: %s", hipGetErrorString(e));
        return GS_EHIP;
    }
    return st;
}
