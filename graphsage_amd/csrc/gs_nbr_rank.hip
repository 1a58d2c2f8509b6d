// NBR link-ranking baselines from neighbor overlap (common neighbors, Adamic-Adar, resource allocation, Jaccard): for every edge
// (src, dst) the score t = s(src, dst) and the numbers of candidates that score higher / equal, s(u, x) = sum of q[w] over the
// w in N(u) with x in N(w) -- one row of A diag(q) A per distinct source, formed tile by tile in LDS and ranked in the same
// launch.  Integers only: no floating point, no global atomics, no score vector in memory.  The contract is in
// include/graphsage_amd.h (section NBR); the law is restated in tests/nbr_rank_oracle.py.
#include "gs_common.h"

static_assert(sizeof(gs_nbr_rank_desc) == 160, "gs_nbr_rank_desc layout (mirrored by _lib.NbrRankDesc)");

namespace {

constexpr int NBR_THREADS = 256;
constexpr int NBR_SHORT = 8;                    // a row's run inside a tile of up to this many ids is added by the lane that found it
constexpr uint32_t NBR_NONE = 0xffffffffu;      // "no further id": above every node id (ids < 2^31)

struct NbrRun {                                 // a long run of one row inside the resident tile, taken by a whole wave
    int64_t first;                              // index into col
    int32_t len;
    uint32_t q;
};

// first offset in [lo, hi) of the ascending run col[base + lo .. base + hi) whose id is >= key (hi if none)
__device__ __forceinline__ int32_t nbr_lower_bound(const int32_t* __restrict__ col, const int64_t base, int32_t lo, int32_t hi,
                                                   const uint32_t key) {
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if ((uint32_t)col[base + mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool nbr_contains(const int32_t* __restrict__ col, const int64_t r0, const int64_t r1, const uint32_t key) {
    const int32_t len = (int32_t)(r1 - r0);
    const int32_t p = nbr_lower_bound(col, r0, 0, len, key);
    return p < len && (uint32_t)col[r0 + p] == key;
}

// JACCARD: s / den compared by cross-multiplication in 64-bit unsigned integers (s < 2^31, den < 2^32)
template <bool JACCARD>
__device__ __forceinline__ void nbr_compare(const uint32_t s, const uint32_t den, const uint32_t t, const uint32_t tden, bool& gt,
                                            bool& eq) {
    if (JACCARD) {
        const uint64_t a = (uint64_t)s * (uint64_t)tden, b = (uint64_t)t * (uint64_t)den;
        gt = a > b;
        eq = a == b;
    } else {
        gt = s > t;
        eq = s == t;
    }
}

template <bool JACCARD>
__global__ __launch_bounds__(NBR_THREADS) void nbr_rank_kernel(const gs_nbr_rank_desc d, const int tile_shift) {
    extern __shared__ uint32_t acc[];                        // [tile]: the scores of the resident tile; all zero between tiles
    __shared__ uint32_t cur_lds[GS_NBR_CURSORS];             // per w in N(u): offset of its row's first id not yet consumed
    __shared__ NbrRun runs[NBR_THREADS];
    __shared__ uint32_t pt[GS_NBR_PARTNER_CHUNK], pden[GS_NBR_PARTNER_CHUNK], pdst[GS_NBR_PARTNER_CHUNK];
    __shared__ uint32_t pgt[GS_NBR_PARTNER_CHUNK], peq[GS_NBR_PARTNER_CHUNK];
    __shared__ uint32_t n_runs, next_id;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t tile = 1u << tile_shift;
    const uint32_t N = (uint32_t)d.n_nodes;
    for (uint32_t j = tid; j < tile; j += NBR_THREADS) acc[j] = 0u;
    if (tid == 0) n_runs = 0u;
    uint32_t runs_done = 0u;                                 // n_runs only grows; a batch's runs are the slots runs_done .. n_runs - 1
    __syncthreads();

    for (int64_t g = blockIdx.x; g < d.n_groups; g += gridDim.x) {
        const uint32_t u = (uint32_t)d.group_src[g];
        const int64_t g0 = d.group_ptr[g];
        const int64_t P = d.group_ptr[g + 1] - g0;
        const int64_t u0 = d.rowptr[u];
        const int32_t du = (int32_t)(d.rowptr[u + 1] - u0);
        const int64_t f0 = d.f_rowptr ? d.f_rowptr[u] : 0, f1 = d.f_rowptr ? d.f_rowptr[u + 1] : 0;
        uint32_t* cur = du <= GS_NBR_CURSORS ? cur_lds
                        : (d.ws && (int64_t)du <= d.ws_stride ? d.ws + (int64_t)blockIdx.x * d.ws_stride : nullptr);

        // ---- the partners' own scores, t = sum of q[w] over the w in N(u) whose row holds dst: a search per (w, partner), added
        //      in LDS one chunk of partners at a time; the counts start at 0
        for (int64_t c0 = 0; c0 < P; c0 += GS_NBR_PARTNER_CHUNK) {
            const int pc = (int)(P - c0 < GS_NBR_PARTNER_CHUNK ? P - c0 : GS_NBR_PARTNER_CHUNK);
            if (tid < pc) {
                pt[tid] = 0u;
                pdst[tid] = (uint32_t)d.dst[g0 + c0 + tid];
            }
            __syncthreads();
            for (int64_t k = tid; k < (int64_t)du * pc; k += NBR_THREADS) {
                const int32_t i = (int32_t)(k / pc);
                const int p = (int)(k - (int64_t)i * pc);
                const uint32_t w = (uint32_t)d.col[u0 + i];
                if (nbr_contains(d.col, d.rowptr[w], d.rowptr[w + 1], pdst[p])) atomicAdd(&pt[p], d.q ? d.q[w] : 1u);
            }
            __syncthreads();
            if (tid < pc) {
                d.t[g0 + c0 + tid] = pt[tid];
                d.n_gt[g0 + c0 + tid] = 0;
                d.n_eq[g0 + c0 + tid] = 0;
            }
            __syncthreads();
        }

        // ---- the first id of every row N(w): where the sweep starts
        if (tid == 0) next_id = NBR_NONE;
        __syncthreads();
        {
            uint32_t first = NBR_NONE;
            for (int32_t i = tid; i < du; i += NBR_THREADS) {
                const uint32_t w = (uint32_t)d.col[u0 + i];
                const int64_t r0 = d.rowptr[w];
                if (d.rowptr[w + 1] > r0) first = min(first, (uint32_t)d.col[r0]);
                if (cur) cur[i] = 0u;
            }
            if (first != NBR_NONE) atomicMin(&next_id, first);
        }
        __syncthreads();

        // ---- the sweep: only tiles that some row touches are visited, in ascending order
        while (true) {
            const uint32_t nid = next_id;
            if (nid == NBR_NONE) break;
            const uint32_t base = (nid >> tile_shift) << tile_shift;
            const uint32_t end = min(base + tile, N);
            __syncthreads();                                  // everyone has read next_id
            if (tid == 0) next_id = NBR_NONE;
            __syncthreads();
            // accumulate: a lane per w finds its row's run inside [base, end); short runs are added at once, long ones by a wave
            for (int32_t i0 = 0; i0 < du; i0 += NBR_THREADS) {
                const int32_t i = i0 + tid;
                if (i < du) {
                    const uint32_t w = (uint32_t)d.col[u0 + i];
                    const int64_t r0 = d.rowptr[w];
                    const int32_t len = (int32_t)(d.rowptr[w + 1] - r0);
                    const int32_t lo = cur ? (int32_t)cur[i] : nbr_lower_bound(d.col, r0, 0, len, base);
                    if (lo < len) {
                        const int32_t hi = nbr_lower_bound(d.col, r0, lo, len, end);
                        const uint32_t qw = d.q ? d.q[w] : 1u;
                        if (hi - lo <= NBR_SHORT) {
                            for (int32_t j = lo; j < hi; ++j) atomicAdd(&acc[(uint32_t)d.col[r0 + j] - base], qw);
                        } else {
                            const uint32_t slot = atomicAdd(&n_runs, 1u);
                            runs[slot % NBR_THREADS] = NbrRun{r0 + lo, hi - lo, qw};
                        }
                        if (cur) cur[i] = (uint32_t)hi;
                        if (hi < len) atomicMin(&next_id, (uint32_t)d.col[r0 + hi]);
                    }
                }
                __syncthreads();
                const uint32_t nr = n_runs - runs_done;     // at most NBR_THREADS: one per lane of this batch
                for (uint32_t r = wave; r < nr; r += NBR_THREADS / 64) {
                    const NbrRun run = runs[(runs_done + r) % NBR_THREADS];
                    for (int32_t j = lane; j < run.len; j += 64) atomicAdd(&acc[(uint32_t)d.col[run.first + j] - base], run.q);
                }
                runs_done += nr;
                __syncthreads();                             // the slots may be written again; acc is complete after the last batch
            }
            // the ids that are no candidates for u score 0 from here on: u itself and its filter row's part of the tile
            if (f1 > f0) {
                const int32_t flen = (int32_t)(f1 - f0);
                const int32_t a = nbr_lower_bound(d.f_col, f0, 0, flen, base);
                const int32_t b = nbr_lower_bound(d.f_col, f0, a, flen, end);
                for (int32_t j = a + tid; j < b; j += NBR_THREADS) acc[(uint32_t)d.f_col[f0 + j] - base] = 0u;
            }
            if (tid == 0 && u >= base && u < end) acc[u - base] = 0u;
            __syncthreads();
            // rank: every positive entry against the partners, one chunk at a time; lane p of a wave keeps partner p's counts
            for (int64_t c0 = 0; c0 < P; c0 += GS_NBR_PARTNER_CHUNK) {
                const int pc = (int)(P - c0 < GS_NBR_PARTNER_CHUNK ? P - c0 : GS_NBR_PARTNER_CHUNK);
                const bool last = c0 + GS_NBR_PARTNER_CHUNK >= P;
                if (tid < pc) {
                    const uint32_t t = d.t[g0 + c0 + tid], x = (uint32_t)d.dst[g0 + c0 + tid];
                    pt[tid] = t;
                    pdst[tid] = x;
                    pden[tid] = JACCARD ? (uint32_t)du + (uint32_t)d.deg[x] - t : 1u;
                    pgt[tid] = 0u;
                    peq[tid] = 0u;
                }
                __syncthreads();
                uint32_t mygt = 0u, myeq = 0u;
                for (uint32_t j0 = 0; j0 < end - base; j0 += NBR_THREADS) {
                    const uint32_t j = j0 + tid;
                    const uint32_t s = j < end - base ? acc[j] : 0u;
                    if (last && s) acc[j] = 0u;
                    if (__ballot(s != 0u) == 0ull) continue;
                    const uint32_t x = base + j;
                    const uint32_t den = (JACCARD && s) ? (uint32_t)du + (uint32_t)d.deg[x] - s : 1u;
                    for (int p = 0; p < pc; ++p) {
                        bool gt, eq;
                        nbr_compare<JACCARD>(s, den, pt[p], pden[p], gt, eq);
                        const bool ok = s != 0u && x != pdst[p];
                        const uint64_t bg = __ballot(ok && gt), be = __ballot(ok && eq);
                        if (lane == p) {
                            mygt += (uint32_t)__popcll(bg);
                            myeq += (uint32_t)__popcll(be);
                        }
                    }
                }
                if (lane < pc && (mygt | myeq)) {
                    atomicAdd(&pgt[lane], mygt);
                    atomicAdd(&peq[lane], myeq);
                }
                __syncthreads();
                if (tid < pc) {
                    d.n_gt[g0 + c0 + tid] += (int32_t)pgt[tid];
                    d.n_eq[g0 + c0 + tid] += (int32_t)peq[tid];
                }
                __syncthreads();
            }
        }

        // ---- a partner that scores 0 ties with every candidate that was not visited: counted, not swept
        {
            const bool u_filtered = f1 > f0 && nbr_contains(d.f_col, f0, f1, u);
            const int64_t n_valid = (int64_t)N - (f1 - f0) - (u_filtered ? 0 : 1);
            // (thread p % chunk wrote t and the counts of partner p and reads them back here)
            for (int64_t p = tid; p < P && tid < GS_NBR_PARTNER_CHUNK; p += GS_NBR_PARTNER_CHUNK) {
                if (d.t[g0 + p] != 0u) continue;
                const uint32_t x = (uint32_t)d.dst[g0 + p];
                const bool x_valid = x != u && !(f1 > f0 && nbr_contains(d.f_col, f0, f1, x));
                d.n_eq[g0 + p] = (int32_t)(n_valid - (x_valid ? 1 : 0) - (int64_t)d.n_gt[g0 + p]);
            }
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int gs_nbr_rank_ws_bytes(int64_t n_workgroups, int64_t max_src_degree, int64_t* bytes_out_host) {
    GS_REQUIRE(bytes_out_host && n_workgroups >= 0 && max_src_degree >= 0, "gs_nbr_rank_ws_bytes: bad arguments");
    *bytes_out_host = max_src_degree > GS_NBR_CURSORS ? n_workgroups * max_src_degree * (int64_t)sizeof(uint32_t) : 0;
    return GS_OK;
}

extern "C" int gs_nbr_rank_grid(int64_t n_groups, int32_t max_workgroups, int64_t* grid_out_host) {
    GS_REQUIRE(grid_out_host && n_groups >= 0 && max_workgroups >= 0, "gs_nbr_rank_grid: bad arguments");
    int dev = 0;
    GS_HIP(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    GS_HIP(hipGetDeviceProperties(&prop, dev));
    int64_t grid = (int64_t)prop.multiProcessorCount * GS_NBR_WG_PER_CU;
    if (max_workgroups > 0) grid = std::min<int64_t>(grid, max_workgroups);
    *grid_out_host = std::max<int64_t>(1, std::min(grid, n_groups));
    return GS_OK;
}

extern "C" int gs_nbr_rank(const gs_nbr_rank_desc* desc_host, void* stream) {
    GS_REQUIRE(desc_host, "gs_nbr_rank: null descriptor");
    const gs_nbr_rank_desc& q = *desc_host;
    GS_REQUIRE(q.n_nodes >= 0 && q.n_nodes < (1ll << 31) && q.n_groups >= 0 && q.n_queries >= q.n_groups && q.n_queries < (1ll << 31),
               "gs_nbr_rank: bad sizes n_nodes=%lld n_groups=%lld n_queries=%lld", (long long)q.n_nodes, (long long)q.n_groups,
               (long long)q.n_queries);
    GS_REQUIRE(q.kind == GS_NBR_SUM || q.kind == GS_NBR_JACCARD, "gs_nbr_rank: kind = %d", q.kind);
    const int tile = q.tile > 0 ? q.tile : GS_NBR_TILE;
    GS_REQUIRE(tile >= GS_NBR_MIN_TILE && tile <= GS_NBR_MAX_TILE && (tile & (tile - 1)) == 0,
               "gs_nbr_rank: tile = %d must be a power of two in [%d, %d]", tile, GS_NBR_MIN_TILE, GS_NBR_MAX_TILE);
    GS_REQUIRE(q.max_workgroups >= 0 && q.ws_stride >= 0, "gs_nbr_rank: max_workgroups and ws_stride must not be negative");
    if (q.n_groups == 0) return GS_OK;
    GS_REQUIRE(q.rowptr && q.col && q.group_ptr && q.group_src && q.dst && q.t && q.n_gt && q.n_eq,
               "gs_nbr_rank: rowptr, col, group_ptr, group_src, dst, t, n_gt and n_eq must be non-null");
    GS_REQUIRE(q.kind != GS_NBR_JACCARD || (q.deg && !q.q), "gs_nbr_rank: the Jaccard ratio takes deg and no weights");
    GS_REQUIRE((q.f_rowptr == nullptr) == (q.f_col == nullptr), "gs_nbr_rank: the filter is f_rowptr with f_col, or neither");
    int64_t grid = 0;
    if (const int rc = gs_nbr_rank_grid(q.n_groups, q.max_workgroups, &grid)) return rc;
    GS_REQUIRE(!q.ws || q.ws_bytes >= grid * q.ws_stride * (int64_t)sizeof(uint32_t),
               "gs_nbr_rank: workspace of %lld bytes is too small for %lld workgroups of %lld cursors (gs_nbr_rank_ws_bytes)",
               (long long)q.ws_bytes, (long long)grid, (long long)q.ws_stride);
    int shift = 0;
    while ((1 << shift) < tile) ++shift;
    const size_t lds = (size_t)tile * sizeof(uint32_t);
    const hipStream_t st = (hipStream_t)stream;
    if (q.kind == GS_NBR_JACCARD) {
        GS_LDS_ATTR(GS_NBR_MAX_TILE * sizeof(uint32_t), nbr_rank_kernel<true>);
        hipLaunchKernelGGL(nbr_rank_kernel<true>, dim3((unsigned)grid), dim3(NBR_THREADS), lds, st, q, shift);
    } else {
        GS_LDS_ATTR(GS_NBR_MAX_TILE * sizeof(uint32_t), nbr_rank_kernel<false>);
        hipLaunchKernelGGL(nbr_rank_kernel<false>, dim3((unsigned)grid), dim3(NBR_THREADS), lds, st, q, shift);
    }
    GS_LAUNCH_CHECK("nbr_rank_kernel");
    return GS_OK;
}
