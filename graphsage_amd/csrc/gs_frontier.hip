// Receptive field of a row list, on the device: rows_out = rows_in U {col[e] : e in a row of rows_in}, ascending and
// duplicate-free, with the position map pos[id] (-1 for a non-member) and the member count as a device word.
//
// Why on the device: a FullGraph may be built from a device-resident CSR (the RMAT graph only ever exists in HBM), and exact
// inference for a node subset (inference.layers_nodes) needs S_{l-1} = S_l U N(S_l) once per layer.
//
// The method is gs_dedup.hip's: a flag array written with plain stores of the SAME value from every writer, a block count, and a
// rank pass that also clears the flags behind its read -- no atomics, no sort, the result a function of the inputs alone.  The
// count / rank kernels are the twins of dd_count_kernel / dd_rank_kernel (kept apart: gs_unique_ids writes the rank of EVERY
// value and no -1, and its launches stay as they are).
// Mark: one WAVE per input row, the row's edges spread over the 64 lanes with four loads in flight per lane, so a hub of
// 21,000 edges is 83 rounds of one wave, not one lane's loop.
#include "gs_common.h"

static_assert(sizeof(gs_frontier_desc) == 96, "gs_frontier_desc layout (mirrored by graphsage_amd/_lib.py)");

#define FR_BLOCKS 256

__global__ __launch_bounds__(256) void fr_mark_kernel(const gs_frontier_desc q, int32_t* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < q.m; i += n_waves) {       // wave-uniform
        const int64_t r = q.rows_in[i];
        if (r < 0 || r >= q.n_rows) continue;
        if (lane == 0) flags[r] = 1;                             // same value from every writer: no race that matters
        const int64_t e0 = q.rowptr[r], e1 = q.rowptr[r + 1];
        if (e0 < 0 || e1 < e0 || e1 > q.nnz) continue;
        for (int64_t e = e0 + lane; e < e1; e += 256) {
            int32_t c[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) c[u] = (e + 64 * u < e1) ? q.col[e + 64 * u] : -1;
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (c[u] >= 0 && (int64_t)c[u] < q.n_rows) flags[c[u]] = 1;
        }
    }
}

__device__ __forceinline__ int fr_block_sum(int v, int* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const int tot = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return tot;
}

__global__ __launch_bounds__(256) void fr_count_kernel(const int32_t* __restrict__ flags, int64_t nv, int64_t chunk,
                                                       int32_t* __restrict__ sums) {
    __shared__ int red[4];
    const int64_t lo = min((int64_t)blockIdx.x * chunk, nv), hi = min(lo + chunk, nv);
    int c = 0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) c += flags[i] != 0;
    const int tot = fr_block_sum(c, red);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

// flags -> pos (rank of a member among the members, -1 for every other id), rows_out[rank] = id; the flags are cleared behind the
// read; block b's offset = sum of the block counts before it (FR_BLOCKS = blockDim: one count per thread); the last block
// writes the total
__global__ __launch_bounds__(FR_BLOCKS) void fr_rank_kernel(int32_t* __restrict__ flags, int64_t nv, int64_t chunk,
                                                            const int32_t* __restrict__ sums, int32_t* __restrict__ pos,
                                                            int32_t* __restrict__ rows_out, int64_t cap,
                                                            int32_t* __restrict__ count_out) {
    __shared__ int part[256];
    __shared__ int red[4];
    const int own = sums[threadIdx.x];
    const int before = fr_block_sum((int)threadIdx.x < (int)blockIdx.x ? own : 0, red);
    if (blockIdx.x == FR_BLOCKS - 1) {
        const int total = fr_block_sum(own, red);
        if (threadIdx.x == 0) count_out[0] = total;
    }
    const int64_t lo = min((int64_t)blockIdx.x * chunk, nv), hi = min(lo + chunk, nv);
    const int64_t per = (chunk + 255) / 256;
    const int64_t a = min(lo + (int64_t)threadIdx.x * per, hi), b = min(a + per, hi);
    int c = 0;
    for (int64_t i = a; i < b; ++i) c += flags[i] != 0;
    part[threadIdx.x] = c;
    __syncthreads();
    // exclusive scan of the 256 per-thread counts (Hillis-Steele, in place with a double read per step)
    for (int off = 1; off < 256; off <<= 1) {
        const int v = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int r = before + part[threadIdx.x] - c;
    for (int64_t i = a; i < b; ++i) {
        const int f = flags[i];
        pos[i] = f ? r : -1;
        if (f) {
            flags[i] = 0;
            if (r < cap) rows_out[r] = (int32_t)i;
            ++r;
        }
    }
}

extern "C" int gs_frontier_ws_bytes(int64_t n_rows, int64_t* bytes_out_host) {
    GS_REQUIRE(bytes_out_host && n_rows >= 0 && n_rows < (1ll << 31), "gs_frontier_ws_bytes: bad args");
    *bytes_out_host = (n_rows + FR_BLOCKS) * (int64_t)sizeof(int32_t);
    return GS_OK;
}

extern "C" int gs_frontier_expand(const gs_frontier_desc* desc_host, void* stream) {
    GS_REQUIRE(desc_host, "gs_frontier_expand: null descriptor");
    const gs_frontier_desc& q = *desc_host;
    GS_REQUIRE(q.n_rows > 0 && q.n_rows < (1ll << 31) && q.nnz >= 0 && q.m >= 0 && q.m <= q.n_rows && q.rows_out_cap >= 0,
               "gs_frontier_expand: bad sizes n_rows=%lld nnz=%lld m=%lld rows_out_cap=%lld (0 <= m <= n_rows < 2^31)",
               (long long)q.n_rows, (long long)q.nnz, (long long)q.m, (long long)q.rows_out_cap);
    GS_REQUIRE(q.rowptr && (q.col || q.nnz == 0) && (q.rows_in || q.m == 0) && q.rows_out && q.pos && q.count,
               "gs_frontier_expand: rowptr, col, rows_in, rows_out, pos and count must be non-null");
    GS_REQUIRE(q.ws && gs_aligned16(q.ws), "gs_frontier_expand: the workspace must be non-null and 16-byte aligned");
    GS_REQUIRE(q.ws_bytes >= (q.n_rows + FR_BLOCKS) * (int64_t)sizeof(int32_t),
               "gs_frontier_expand: workspace of %lld bytes is too small (gs_frontier_ws_bytes)", (long long)q.ws_bytes);
    const hipStream_t st = (hipStream_t)stream;
    int32_t* flags = q.ws;
    int32_t* sums = q.ws + q.n_rows;
    const int64_t chunk = gs_ceil_div(q.n_rows, FR_BLOCKS);
    if (q.m > 0) {
        const int mblocks = (int)std::min<int64_t>(gs_ceil_div(q.m, 4), 16384);
        hipLaunchKernelGGL(fr_mark_kernel, dim3(mblocks), dim3(256), 0, st, q, flags);
    }
    hipLaunchKernelGGL(fr_count_kernel, dim3(FR_BLOCKS), dim3(256), 0, st, flags, q.n_rows, chunk, sums);
    hipLaunchKernelGGL(fr_rank_kernel, dim3(FR_BLOCKS), dim3(FR_BLOCKS), 0, st, flags, q.n_rows, chunk, sums, q.pos, q.rows_out,
                       q.rows_out_cap, q.count);
    GS_LAUNCH_CHECK("gs_frontier_expand");
    return GS_OK;
}
