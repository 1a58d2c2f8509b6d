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
static_assert(sizeof(gs_csr_rows_desc) == 168, "gs_csr_rows_desc layout (mirrored by graphsage_amd/_lib.py)");

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

// the row's value from the reduced neighbors: mean = sum / deg, mean-with-self = (sum + self) / (deg + 1), max, softmax = the
// weighted sum / the sum of the weights l; an empty row gives 0 (mean, max, softmax) or self (mean-with-self); then the optional relu.  `self` points at the row's own float4 of the table
// (read for GS_CSR_MEAN_SELF only)
template <int OP>
__device__ __forceinline__ f32x4 csr_finish(f32x4 acc, const float* __restrict__ self, const int64_t deg, const int col,
                                            const int d, const int act, const float l) {
    if (OP == GS_CSR_SOFTMAX) {
        acc = deg == 0 ? f32x4{0.f, 0.f, 0.f, 0.f} : acc * (1.0f / l);
    } else if (OP == GS_CSR_MEAN_SELF) {
        acc += *reinterpret_cast<const f32x4*>(self);
        acc *= 1.0f / (float)(deg + 1);
    } else if (deg == 0) {
        acc = f32x4{0.f, 0.f, 0.f, 0.f};
    } else if (OP == GS_CSR_MEAN) {
        acc *= 1.0f / (float)deg;
    }
    if (act == GS_ACT_RELU) acc = f32x4{fmaxf(acc.x, 0.f), fmaxf(acc.y, 0.f), fmaxf(acc.z, 0.f), fmaxf(acc.w, 0.f)};
    return gs_mask_tail(acc, col, d);
}

// The per-item loop of BOTH reduce kernels (window and row list): the item's `cnt` column ids 64 at a time, broadcast through
// v_readlane, U independent 16-byte row loads per lane in flight before the first add, the remainder batch clamped.  One
// function, so a row is reduced in the same order of additions whichever kernel reduces it.  MAPPED: every id goes through
// x_pos (nullable: the table is indexed by id) and is held to [0, n_ids) before and [0, x_rows) after; one id outside makes
// the whole wave give the item up (returns false, wave-uniform) before any row load of that batch.
template <int OP, int U, bool MAPPED>
__device__ __forceinline__ bool csr_item_sum(f32x4& acc, const float* __restrict__ X, const int64_t ldx,
                                             const int32_t* __restrict__ cols, const int cnt, const int col, const bool active,
                                             const int lane, const int32_t* __restrict__ x_pos, const int64_t n_ids,
                                             const int64_t x_rows) {
    acc = csr_identity<OP>();
    for (int jb = 0; jb < cnt; jb += 64) {
        const int m = min(64, cnt - jb);                     // uniform
        int32_t my = 0;
        if (lane < m) my = cols[jb + lane];
        if (MAPPED) {
            bool bad = false;
            if (lane < m) {
                bad = my < 0 || my >= n_ids;
                if (!bad && x_pos) my = x_pos[my];
                bad = bad || my < 0 || my >= x_rows;
            }
            if (__ballot(bad) != 0) return false;
        }
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
    return true;
}

__device__ __forceinline__ float csr_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ float csr_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// GS_CSR_SOFTMAX: the logit of table row r is X[r][d], the column behind the d value columns.  csr_item_sum's loop with a
// running maximum m, running sum l of exp(logit - m) and an accumulator rescaled whenever m moves (online softmax): per batch
// of 64 ids every lane loads one logit, the batch maximum and the sum of the batch's weights are butterfly reductions (the same
// bits in every lane and in the waves of every column chunk), then the rows are added weight * row in list order.
template <int U, bool MAPPED>
__device__ __forceinline__ bool csr_item_softmax(f32x4& acc, float& m, float& l, const float* __restrict__ X, const int64_t ldx,
                                                 const int d, const int32_t* __restrict__ cols, const int cnt, const int col,
                                                 const bool active, const int lane, const int32_t* __restrict__ x_pos,
                                                 const int64_t n_ids, const int64_t x_rows) {
    acc = f32x4{0.f, 0.f, 0.f, 0.f};
    m = -__builtin_inff();
    l = 0.f;
    for (int jb = 0; jb < cnt; jb += 64) {
        const int n64 = min(64, cnt - jb);                   // uniform
        int32_t my = 0;
        if (lane < n64) my = cols[jb + lane];
        if (MAPPED) {
            bool bad = false;
            if (lane < n64) {
                bad = my < 0 || my >= n_ids;
                if (!bad && x_pos) my = x_pos[my];
                bad = bad || my < 0 || my >= x_rows;
            }
            if (__ballot(bad) != 0) return false;
        }
        float t = -__builtin_inff();
        if (lane < n64) t = X[(int64_t)my * ldx + d];
        const float m_new = fmaxf(m, csr_wave_max(t));
        const float sc = expf(m - m_new);                    // 0 at the first batch (m = -inf)
        const float wgt = lane < n64 ? expf(t - m_new) : 0.f;
        l = l * sc + csr_wave_sum(wgt);
        m = m_new;
        if (active) {
            acc *= sc;
            const int wbits = __float_as_int(wgt);
            int j = 0;
            for (; j + U <= n64; j += U) {
                f32x4 v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int32_t r = __builtin_amdgcn_readlane(my, j + u);
                    v[u] = *reinterpret_cast<const f32x4*>(X + (int64_t)r * ldx + col);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) acc += v[u] * __int_as_float(__builtin_amdgcn_readlane(wbits, j + u));
            }
            if (j < n64) {
                f32x4 v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int32_t r = __builtin_amdgcn_readlane(my, min(j + u, n64 - 1));
                    v[u] = *reinterpret_cast<const f32x4*>(X + (int64_t)r * ldx + col);
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (j + u < n64) acc += v[u] * __int_as_float(__builtin_amdgcn_readlane(wbits, min(j + u, n64 - 1)));
            }
        }
    }
    return true;
}

// one item of either kind: (acc, m, l); m and l are the softmax state and stay untouched for the other ops
template <int OP, int U, bool MAPPED>
__device__ __forceinline__ bool csr_item(f32x4& acc, float& m, float& l, const float* __restrict__ X, const int64_t ldx, const int d,
                                         const int32_t* __restrict__ cols, const int cnt, const int col, const bool active,
                                         const int lane, const int32_t* __restrict__ x_pos, const int64_t n_ids,
                                         const int64_t x_rows) {
    if (OP == GS_CSR_SOFTMAX) return csr_item_softmax<U, MAPPED>(acc, m, l, X, ldx, d, cols, cnt, col, active, lane, x_pos, n_ids, x_rows);
    return csr_item_sum<OP, U, MAPPED>(acc, X, ldx, cols, cnt, col, active, lane, x_pos, n_ids, x_rows);
}

__host__ __device__ static inline int csr_chunks(int32_t d) { return ((d + 3) / 4 + 63) / 64; }

// floats per partial slot: whole column chunks; the softmax partial is wider by its (m, l) pair, kept at columns round_up(d, 4)
// and round_up(d, 4) + 1
template <int OP>
__host__ __device__ static inline int64_t csr_slot_words(int32_t d) {
    return (int64_t)csr_chunks(OP == GS_CSR_SOFTMAX ? d + 4 : d) * 256;
}

// one segment of a long row: the raw partial (and, once per slot, the softmax state)
template <int OP>
__device__ __forceinline__ void csr_store_partial(float* __restrict__ p, const int col, const int d, const bool first,
                                                  const f32x4 acc, const float m, const float l) {
    *reinterpret_cast<f32x4*>(p + col) = acc;
    if (OP == GS_CSR_SOFTMAX && first) {
        p[(d + 3) / 4 * 4] = m;
        p[(d + 3) / 4 * 4 + 1] = l;
    }
}

// a long row's partials in segment order (both combine kernels); softmax: each rescaled to the row's maximum, l = the weights' sum
template <int OP>
__device__ __forceinline__ f32x4 csr_parts_sum(const float* __restrict__ p, const int64_t ldw, const int64_t parts, const int col,
                                               const int d, float& l) {
    f32x4 acc = csr_identity<OP>();
    if (OP == GS_CSR_SOFTMAX) {
        const int ms = (d + 3) / 4 * 4;
        float m = -__builtin_inff();
        for (int64_t k = 0; k < parts; ++k) m = fmaxf(m, p[k * ldw + ms]);
        l = 0.f;
        for (int64_t k = 0; k < parts; ++k) {
            const float sc = expf(p[k * ldw + ms] - m);
            l += p[k * ldw + ms + 1] * sc;
            acc += *reinterpret_cast<const f32x4*>(p + k * ldw + col) * sc;
        }
        return acc;
    }
    for (int64_t k = 0; k < parts; ++k) acc = csr_combine<OP>(acc, *reinterpret_cast<const f32x4*>(p + k * ldw + col));
    return acc;
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

    f32x4 acc;
    float m = 0.f, l = 0.f;
    csr_item<OP, U, false>(acc, m, l, X, ldx, q.d, cols, cnt, col, active, lane, nullptr, 0, 0);
    if (!active) return;
    if (slot >= 0) {
        // one segment of a long row: the raw partial; csr_combine_kernel finishes the row
        csr_store_partial<OP>(q.ws + (slot - q.slot0) * csr_slot_words<OP>(q.d), col, q.d, c == 0 && lane == 0, acc, m, l);
        return;
    }
    *reinterpret_cast<f32x4*>(q.out + (row - q.row0) * q.ldo + col) =
        csr_finish<OP>(acc, X + row * ldx + col, cnt, col, q.d, q.act, l);
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
    const int64_t ldw = csr_slot_words<OP>(q.d);
    float l = 0.f;
    const f32x4 acc = csr_parts_sum<OP>(q.ws + (s0 - q.slot0) * ldw, ldw, parts, col, q.d, l);
    const int64_t deg = q.rowptr[row + 1] - q.rowptr[row];
    *reinterpret_cast<f32x4*>(q.out + (row - q.row0) * q.ldo + col) =
        csr_finish<OP>(acc, q.X + row * q.ldx + col, deg, col, q.d, q.act, l);
}

// ---------------------------------------------------------------------------------------------------------------
// Row-list form (gs_csr_reduce_rows): the rows of a plan that covers a row SUBSET (FullGraph.plan_rows: the graph plan's items
// of those rows, in its order, partial slots re-based to 0 ...), read through x_pos and written through out_pos.  The item
// loop, the partial sum and the finish are the functions above, so every row gets the window kernel's order of additions.
// Nothing of the plan or the maps is trusted: a row, slot or mapped position out of range makes the wave give its item up.
template <int OP, int U>
__global__ __launch_bounds__(256) void csr_rows_kernel(const gs_csr_rows_desc q, const int chunks) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= q.n_items * chunks) return;                     // wave-uniform
    const int64_t it = w / chunks;
    const int c = (int)(w - it * chunks);
    const int64_t* __restrict__ item = q.items + it * CSR_ITEM_WORDS;
    const int64_t row = item[0], e0 = item[1], slot = item[3];
    const int cnt = (int)item[2];
    if (row < 0 || row >= q.n_rows || item[2] < 0 || item[2] > q.split_len || e0 < 0 || e0 + cnt > q.nnz) return;
    if (slot >= q.n_slots) return;
    const int col = (c * 64 + lane) * 4;
    const bool active = col < q.d;
    int64_t orow = 0, srow = 0;
    if (slot < 0) {
        orow = q.out_pos[row];
        if (orow < 0 || orow >= q.out_rows) return;
        if (OP == GS_CSR_MEAN_SELF) {
            srow = q.x_pos ? (int64_t)q.x_pos[row] : row;
            if (srow < 0 || srow >= q.x_rows) return;
        }
    }
    f32x4 acc;
    float m = 0.f, l = 0.f;
    if (!csr_item<OP, U, true>(acc, m, l, q.X, q.ldx, q.d, q.col + e0, cnt, col, active, lane, q.x_pos, q.n_rows, q.x_rows)) return;
    if (!active) return;
    if (slot >= 0) {
        csr_store_partial<OP>(q.ws + slot * csr_slot_words<OP>(q.d), col, q.d, c == 0 && lane == 0, acc, m, l);
        return;
    }
    *reinterpret_cast<f32x4*>(q.out + orow * q.ldo + col) = csr_finish<OP>(acc, q.X + srow * q.ldx + col, cnt, col, q.d, q.act, l);
}

template <int OP>
__global__ __launch_bounds__(256) void csr_rows_combine_kernel(const gs_csr_rows_desc q, const int chunks) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= q.n_split * chunks) return;                     // wave-uniform
    const int64_t si = w / chunks;
    const int c = (int)(w - si * chunks);
    const int64_t* __restrict__ sp = q.splits + si * CSR_SPLIT_WORDS;
    const int64_t row = sp[0], s0 = sp[1], parts = sp[2];
    if (row < 0 || row >= q.n_rows || parts < 0 || s0 < 0 || parts > q.n_slots || s0 > q.n_slots - parts) return;
    const int64_t orow = q.out_pos[row];
    if (orow < 0 || orow >= q.out_rows) return;
    int64_t srow = 0;
    if (OP == GS_CSR_MEAN_SELF) {
        srow = q.x_pos ? (int64_t)q.x_pos[row] : row;
        if (srow < 0 || srow >= q.x_rows) return;
    }
    const int col = (c * 64 + lane) * 4;
    if (col >= q.d) return;
    const int64_t ldw = csr_slot_words<OP>(q.d);
    float l = 0.f;
    const f32x4 acc = csr_parts_sum<OP>(q.ws + s0 * ldw, ldw, parts, col, q.d, l);
    const int64_t deg = q.rowptr[row + 1] - q.rowptr[row];
    *reinterpret_cast<f32x4*>(q.out + orow * q.ldo + col) = csr_finish<OP>(acc, q.X + srow * q.ldx + col, deg, col, q.d, q.act, l);
}

static inline int64_t csr_slot_words_of(int32_t op, int32_t d) {
    return op == GS_CSR_SOFTMAX ? csr_slot_words<GS_CSR_SOFTMAX>(d) : csr_slot_words<GS_CSR_MEAN>(d);
}

// d: the width of the partial -- the table's d, or d + 4 for GS_CSR_SOFTMAX (its partial carries the (max, sum) pair)
extern "C" int gs_csr_reduce_ws_bytes(int64_t n_slots, int32_t d, int64_t* bytes_out_host) {
    GS_REQUIRE(bytes_out_host && n_slots >= 0 && d > 0, "gs_csr_reduce_ws_bytes: bad args");
    *bytes_out_host = n_slots * (int64_t)csr_chunks(d) * 256 * (int64_t)sizeof(float);
    return GS_OK;
}

// the two launches of both entry points: one wave per (item, chunk), then one per (long row, chunk)
template <class Desc, class Reduce, class Combine>
static int csr_launch_pair(const char* who, const Desc& q, const int64_t n_items, const int64_t n_split, const int chunks,
                           Reduce reduce, Combine combine, hipStream_t st) {
    const int64_t blocks = gs_ceil_div(n_items * chunks, 4);
    GS_REQUIRE(blocks < (1ll << 31), "%s: grid too large (%lld blocks)", who, (long long)blocks);
    hipLaunchKernelGGL(reduce, dim3((unsigned)blocks), dim3(256), 0, st, q, chunks);
    GS_LAUNCH_CHECK("csr_reduce_kernel");
    if (n_split > 0) {
        const int64_t b2 = gs_ceil_div(n_split * chunks, 4);
        hipLaunchKernelGGL(combine, dim3((unsigned)b2), dim3(256), 0, st, q, chunks);
        GS_LAUNCH_CHECK("csr_combine_kernel");
    }
    return GS_OK;
}

template <int OP>
static int csr_launch(const gs_csr_reduce_desc& q, const int chunks, hipStream_t st) {
    return csr_launch_pair("gs_csr_reduce_fwd", q, q.item1 - q.item0, q.split1 - q.split0, chunks, csr_reduce_kernel<OP, 8>,
                           csr_combine_kernel<OP>, st);
}

template <int OP>
static int csr_rows_launch(const gs_csr_rows_desc& q, const int chunks, hipStream_t st) {
    return csr_launch_pair("gs_csr_reduce_rows", q, q.n_items, q.n_split, chunks, csr_rows_kernel<OP, 8>,
                           csr_rows_combine_kernel<OP>, st);
}

extern "C" int gs_csr_reduce_fwd(const gs_csr_reduce_desc* desc_host, void* stream) {
    GS_REQUIRE(desc_host, "gs_csr_reduce_fwd: null descriptor");
    const gs_csr_reduce_desc& q = *desc_host;
    GS_REQUIRE(q.op == GS_CSR_MEAN || q.op == GS_CSR_MEAN_SELF || q.op == GS_CSR_MAX || q.op == GS_CSR_SOFTMAX,
               "gs_csr_reduce_fwd: unknown op %d", q.op);
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
    GS_REQUIRE(q.op != GS_CSR_SOFTMAX || q.ldx >= ((q.d + 4) / 4) * 4,
               "gs_csr_reduce_fwd: GS_CSR_SOFTMAX reads the logit in column d of X: ldx must be >= round_up(d + 1, 4)");
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
        GS_REQUIRE(q.ws_bytes >= (q.slot1 - q.slot0) * csr_slot_words_of(q.op, q.d) * (int64_t)sizeof(float),
                   "gs_csr_reduce_fwd: workspace of %lld bytes is too small (gs_csr_reduce_ws_bytes)", (long long)q.ws_bytes);
    }
    const hipStream_t st = (hipStream_t)stream;
    if (q.op == GS_CSR_MEAN) return csr_launch<GS_CSR_MEAN>(q, chunks, st);
    if (q.op == GS_CSR_MEAN_SELF) return csr_launch<GS_CSR_MEAN_SELF>(q, chunks, st);
    if (q.op == GS_CSR_SOFTMAX) return csr_launch<GS_CSR_SOFTMAX>(q, chunks, st);
    return csr_launch<GS_CSR_MAX>(q, chunks, st);
}

extern "C" int gs_csr_reduce_rows(const gs_csr_rows_desc* desc_host, void* stream) {
    GS_REQUIRE(desc_host, "gs_csr_reduce_rows: null descriptor");
    const gs_csr_rows_desc& q = *desc_host;
    GS_REQUIRE(q.op == GS_CSR_MEAN || q.op == GS_CSR_MEAN_SELF || q.op == GS_CSR_MAX || q.op == GS_CSR_SOFTMAX,
               "gs_csr_reduce_rows: unknown op %d", q.op);
    GS_REQUIRE(q.act == GS_ACT_IDENTITY || q.act == GS_ACT_RELU, "gs_csr_reduce_rows: unknown act %d", q.act);
    GS_REQUIRE(q.n_rows >= 0 && q.n_rows < (1ll << 31) && q.nnz >= 0 && q.d > 0 && q.split_len > 0 && q.n_items >= 0 &&
                   q.n_split >= 0 && q.n_slots >= 0 && q.x_rows >= 0 && q.out_rows >= 0 && q.x_rows < (1ll << 31) &&
                   q.out_rows < (1ll << 31),
               "gs_csr_reduce_rows: bad sizes n_rows=%lld nnz=%lld d=%d split_len=%d items=%lld splits=%lld slots=%lld x_rows=%lld "
               "out_rows=%lld", (long long)q.n_rows, (long long)q.nnz, q.d, q.split_len, (long long)q.n_items,
               (long long)q.n_split, (long long)q.n_slots, (long long)q.x_rows, (long long)q.out_rows);
    if (q.n_items == 0) return GS_OK;
    GS_REQUIRE(q.rowptr && q.col && q.items && q.out_pos, "gs_csr_reduce_rows: rowptr, col, items and out_pos must be non-null");
    GS_CHECK_MAT(q.X, q.ldx, "gs_csr_reduce_rows X");
    GS_CHECK_MAT(q.out, q.ldo, "gs_csr_reduce_rows out");
    const int d4x4 = ((q.d + 3) / 4) * 4;
    GS_REQUIRE(q.ldx >= d4x4 && q.ldo >= d4x4, "gs_csr_reduce_rows: ld must be >= round_up(d,4)");
    GS_REQUIRE(q.op != GS_CSR_SOFTMAX || q.ldx >= ((q.d + 4) / 4) * 4,
               "gs_csr_reduce_rows: GS_CSR_SOFTMAX reads the logit in column d of X: ldx must be >= round_up(d + 1, 4)");
    // without a map the table is indexed by node id: it must hold every row of the graph
    GS_REQUIRE(q.x_pos || q.x_rows >= q.n_rows, "gs_csr_reduce_rows: no x_pos and X has %lld rows, the graph %lld",
               (long long)q.x_rows, (long long)q.n_rows);
    const int chunks = csr_chunks(q.d);
    if (q.n_slots > 0 || q.n_split > 0) {
        GS_REQUIRE(q.splits && q.ws && gs_aligned16(q.ws), "gs_csr_reduce_rows: long rows need splits and a 16-byte aligned workspace");
        GS_REQUIRE(q.ws_bytes >= q.n_slots * csr_slot_words_of(q.op, q.d) * (int64_t)sizeof(float),
                   "gs_csr_reduce_rows: workspace of %lld bytes is too small (gs_csr_reduce_ws_bytes)", (long long)q.ws_bytes);
    }
    const hipStream_t st = (hipStream_t)stream;
    if (q.op == GS_CSR_MEAN) return csr_rows_launch<GS_CSR_MEAN>(q, chunks, st);
    if (q.op == GS_CSR_MEAN_SELF) return csr_rows_launch<GS_CSR_MEAN_SELF>(q, chunks, st);
    if (q.op == GS_CSR_SOFTMAX) return csr_rows_launch<GS_CSR_SOFTMAX>(q, chunks, st);
    return csr_rows_launch<GS_CSR_MAX>(q, chunks, st);
}
