// Full-neighborhood inference: variable-degree segmented reduce over a CSR adjacency (HBM-bound, like K2 which it generalises).
//
//   out[r - row0, :] = reduce over e in [rowptr[r], rowptr[r+1]) of X[col[e], :]        for r in [row0, row0 + n)
//
// Work decomposition: one WAVE per (work item, 64-float4 column chunk).  A work item is a run of at most split_len consecutive
// edges of one row (plan built once per graph, graphsage_amd/inference.py:plan_work_items): a row of degree <= split_len is
// ONE item that writes its output row; a longer row (a hub) is cut into ceil(deg / split_len) items that write their raw
// partial to a workspace slot each, and a second small launch combines each such row's partials IN SEGMENT ORDER.  A hub of
// thousands of neighbors therefore costs the launch as many evenly sized waves as its length asks for instead of one wave
// that outlives every other.  No float atomics; the order of every addition is fixed => bitwise reproducible run to run.
// The item's column ids are loaded 64 at a time and broadcast through v_readlane, U independent 16-byte row loads per lane
// are in flight before the first add, the last float4 of a row is masked (gs_mask_tail).
#include "gs_common.h"
#include "gs_gather_dev.h"

static_assert(sizeof(gs_csr_reduce_desc) == 200, "gs_csr_reduce_desc layout (mirrored by graphsage_amd/_lib.py)");

#define CSR_ITEM_WORDS 4    // (row, first edge, count, partial slot or -1)
#define CSR_SPLIT_WORDS 3   // (row, first partial slot, partials)

template <int OP>
__device__ __forceinline__ f32x4 csr_identity() {
    if (OP == GS_CSR_MAX) {
        const float ninf = -__builtin_inff();
        return f32x4{ninf, ninf, ninf, ninf};
    }
    return f32x4{0.f, 0.f, 0.f, 0.f};
}

template <int OP>
__device__ __forceinline__ f32x4 csr_combine(const f32x4 a, const f32x4 v) {
    if (OP == GS_CSR_MAX) return f32x4{fmaxf(a.x, v.x), fmaxf(a.y, v.y), fmaxf(a.z, v.z), fmaxf(a.w, v.w)};
    return a + v;
}

// the row's value from the reduced neighbors: mean = sum / deg, mean-with-self = (sum + X[r]) / (deg + 1), max; an empty row
// gives 0 (mean, max) or X[r] (mean-with-self); then the optional relu
template <int OP>
__device__ __forceinline__ f32x4 csr_finish(f32x4 acc, const gs_csr_reduce_desc& q, const int64_t row, const int64_t deg,
                                            const int col) {
    if (OP == GS_CSR_MEAN_SELF) {
        acc += *reinterpret_cast<const f32x4*>(q.X + row * q.ldx + col);
        acc *= 1.0f / (float)(deg + 1);
    } else if (deg == 0) {
        acc = f32x4{0.f, 0.f, 0.f, 0.f};
    } else if (OP == GS_CSR_MEAN) {
        acc *= 1.0f / (float)deg;
    }
    if (q.act == GS_ACT_RELU) acc = f32x4{fmaxf(acc.x, 0.f), fmaxf(acc.y, 0.f), fmaxf(acc.z, 0.f), fmaxf(acc.w, 0.f)};
    return gs_mask_tail(acc, col, q.d);
}

template <int OP, int U>
__global__ __launch_bounds__(256) void csr_reduce_kernel(const gs_csr_reduce_desc q, const int chunks) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t n_items = q.item1 - q.item0;
    if (w >= n_items * chunks) return;                       // wave-uniform
    const int64_t it = w / chunks;
    const int c = (int)(w - it * chunks);
    const int64_t* __restrict__ item = q.items + (q.item0 + it) * CSR_ITEM_WORDS;
    const int64_t row = item[0], e0 = item[1], slot = item[3];
    const int cnt = (int)item[2];
    // a plan that does not belong to this window / graph / workspace must not turn into a stray access (wave-uniform)
    if (row < q.row0 || row >= q.row0 + q.n || cnt < 0 || cnt > q.split_len || e0 < 0 || e0 + cnt > q.nnz) return;
    if (slot >= 0 && (slot < q.slot0 || slot >= q.slot1)) return;
    const int col = (c * 64 + lane) * 4;
    const bool active = col < q.d;
    const float* __restrict__ X = q.X;
    const int32_t* __restrict__ cols = q.col + e0;
    const int64_t ldx = q.ldx;

    f32x4 acc = csr_identity<OP>();
    for (int jb = 0; jb < cnt; jb += 64) {
        const int m = min(64, cnt - jb);                     // uniform
        int32_t my = 0;
        if (lane < m) my = cols[jb + lane];
        if (active) {
            int j = 0;
            for (; j + U <= m; j += U) {
                f32x4 v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int32_t r = __builtin_amdgcn_readlane(my, j + u);
                    v[u] = *reinterpret_cast<const f32x4*>(X + (int64_t)r * ldx + col);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) acc = csr_combine<OP>(acc, v[u]);
            }
            if (j < m) {
                // remainder batch: every load is issued (index clamped to the last entry), the surplus dropped afterwards
                f32x4 v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int32_t r = __builtin_amdgcn_readlane(my, min(j + u, m - 1));
                    v[u] = *reinterpret_cast<const f32x4*>(X + (int64_t)r * ldx + col);
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (j + u < m) acc = csr_combine<OP>(acc, v[u]);
            }
        }
    }
    if (!active) return;
    if (slot >= 0) {
        // one segment of a long row: the raw partial; csr_combine_kernel finishes the row
        *reinterpret_cast<f32x4*>(q.ws + (slot - q.slot0) * (int64_t)(chunks * 256) + col) = acc;
        return;
    }
    *reinterpret_cast<f32x4*>(q.out + (row - q.row0) * q.ldo + col) = csr_finish<OP>(acc, q, row, cnt, col);
}

// one wave per (long row, column chunk): its partials in segment order
template <int OP>
__global__ __launch_bounds__(256) void csr_combine_kernel(const gs_csr_reduce_desc q, const int chunks) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= (q.split1 - q.split0) * chunks) return;         // wave-uniform
    const int64_t si = w / chunks;
    const int c = (int)(w - si * chunks);
    const int64_t* __restrict__ sp = q.splits + (q.split0 + si) * CSR_SPLIT_WORDS;
    const int64_t row = sp[0], s0 = sp[1], parts = sp[2];
    if (row < q.row0 || row >= q.row0 + q.n || parts < 0 || s0 < q.slot0 || s0 + parts > q.slot1) return;
    const int col = (c * 64 + lane) * 4;
    if (col >= q.d) return;
    const int64_t ldw = (int64_t)chunks * 256;
    const float* __restrict__ p = q.ws + (s0 - q.slot0) * ldw + col;
    f32x4 acc = csr_identity<OP>();
    for (int64_t k = 0; k < parts; ++k) acc = csr_combine<OP>(acc, *reinterpret_cast<const f32x4*>(p + k * ldw));
    const int64_t deg = q.rowptr[row + 1] - q.rowptr[row];
    *reinterpret_cast<f32x4*>(q.out + (row - q.row0) * q.ldo + col) = csr_finish<OP>(acc, q, row, deg, col);
}

static inline int csr_chunks(int32_t d) { return ((d + 3) / 4 + 63) / 64; }

extern "C" int gs_csr_reduce_ws_bytes(int64_t n_slots, int32_t d, int64_t* bytes_out_host) {
    GS_REQUIRE(bytes_out_host && n_slots >= 0 && d > 0, "gs_csr_reduce_ws_bytes: bad args");
    *bytes_out_host = n_slots * (int64_t)csr_chunks(d) * 256 * (int64_t)sizeof(float);
    return GS_OK;
}

template <int OP>
static int csr_launch(const gs_csr_reduce_desc& q, const int chunks, hipStream_t st) {
    const int64_t blocks = gs_ceil_div((q.item1 - q.item0) * chunks, 4);
    GS_REQUIRE(blocks < (1ll << 31), "gs_csr_reduce_fwd: grid too large (%lld blocks)", (long long)blocks);
    hipLaunchKernelGGL((csr_reduce_kernel<OP, 8>), dim3((unsigned)blocks), dim3(256), 0, st, q, chunks);
    GS_LAUNCH_CHECK("csr_reduce_kernel");
    if (q.split1 > q.split0) {
        const int64_t b2 = gs_ceil_div((q.split1 - q.split0) * chunks, 4);
        hipLaunchKernelGGL((csr_combine_kernel<OP>), dim3((unsigned)b2), dim3(256), 0, st, q, chunks);
        GS_LAUNCH_CHECK("csr_combine_kernel");
    }
    return GS_OK;
}

extern "C" int gs_csr_reduce_fwd(const gs_csr_reduce_desc* desc_host, void* stream) {
    GS_REQUIRE(desc_host, "gs_csr_reduce_fwd: null descriptor");
    const gs_csr_reduce_desc& q = *desc_host;
    GS_REQUIRE(q.op == GS_CSR_MEAN || q.op == GS_CSR_MEAN_SELF || q.op == GS_CSR_MAX, "gs_csr_reduce_fwd: unknown op %d", q.op);
    GS_REQUIRE(q.act == GS_ACT_IDENTITY || q.act == GS_ACT_RELU, "gs_csr_reduce_fwd: unknown act %d", q.act);
    GS_REQUIRE(q.n_rows >= 0 && q.nnz >= 0 && q.d > 0 && q.split_len > 0 && q.row0 >= 0 && q.n >= 0 && q.row0 + q.n <= q.n_rows,
               "gs_csr_reduce_fwd: bad sizes n_rows=%lld nnz=%lld d=%d split_len=%d window=[%lld, +%lld)", (long long)q.n_rows,
               (long long)q.nnz, q.d, q.split_len, (long long)q.row0, (long long)q.n);
    if (q.n == 0) return GS_OK;
    GS_REQUIRE(q.rowptr && q.col && q.items, "gs_csr_reduce_fwd: rowptr, col and items must be non-null");
    GS_CHECK_MAT(q.X, q.ldx, "gs_csr_reduce_fwd X");
    GS_CHECK_MAT(q.out, q.ldo, "gs_csr_reduce_fwd out");
    const int d4x4 = ((q.d + 3) / 4) * 4;
    GS_REQUIRE(q.ldx >= d4x4 && q.ldo >= d4x4, "gs_csr_reduce_fwd: ld must be >= round_up(d,4)");
    // every column id is < n_rows (the owner of the graph checked it once): the table must hold that many rows
    GS_REQUIRE(q.x_rows >= q.n_rows, "gs_csr_reduce_fwd: X has %lld rows, the graph %lld", (long long)q.x_rows, (long long)q.n_rows);
    GS_REQUIRE(0 <= q.item0 && q.item0 <= q.item1 && q.item1 <= q.n_items && q.item1 - q.item0 >= q.n,
               "gs_csr_reduce_fwd: bad item range [%lld, %lld) of %lld for %lld rows", (long long)q.item0, (long long)q.item1,
               (long long)q.n_items, (long long)q.n);
    GS_REQUIRE(0 <= q.split0 && q.split0 <= q.split1 && q.split1 <= q.n_split && 0 <= q.slot0 && q.slot0 <= q.slot1,
               "gs_csr_reduce_fwd: bad split / slot range");
    const int chunks = csr_chunks(q.d);
    if (q.slot1 > q.slot0 || q.split1 > q.split0) {
        GS_REQUIRE(q.splits && q.ws && gs_aligned16(q.ws), "gs_csr_reduce_fwd: long rows need splits and a 16-byte aligned workspace");
        GS_REQUIRE(q.ws_bytes >= (q.slot1 - q.slot0) * (int64_t)chunks * 256 * (int64_t)sizeof(float),
                   "gs_csr_reduce_fwd: workspace of %lld bytes is too small (gs_csr_reduce_ws_bytes)", (long long)q.ws_bytes);
    }
    const hipStream_t st = (hipStream_t)stream;
    if (q.op == GS_CSR_MEAN) return csr_launch<GS_CSR_MEAN>(q, chunks, st);
    if (q.op == GS_CSR_MEAN_SELF) return csr_launch<GS_CSR_MEAN_SELF>(q, chunks, st);
    return csr_launch<GS_CSR_MAX>(q, chunks, st);
}
