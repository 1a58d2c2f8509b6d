// Second-order (p, q) random walks of node2vec over a CSR adjacency, and the reference's (start, current) co-occurrence pairs
// (utils.py:77-92) from them.  The law, the stream and the descriptor: include/graphsage_amd.h, section WALK; restated in
// NumPy uint64 arithmetic in tests/walk_oracle.py and checked bit for bit.
//
// walk_paths_kernel: one lane per walk, grid-strided.  Walk g = walk0 + i starts at starts[g / num_walks]: the walks of one
// start are adjacent lanes, so a wave's first row reads (rowptr and the first col entries) hit a handful of cache lines.
// After that every lane is somewhere else in the graph and the kernel is a chain of dependent loads per lane: per attempt
// one col entry, then -- only when the draw falls between thr_common and thr_far, where the class of x decides -- up to
// ceil(log2(deg(t) + 1)) probes of t's row; per move the two rowptr entries of the new node.
// Nothing hides that chain but other waves, so the kernel keeps no LDS and few registers (report below) and a lane's state
// is (v, its row, t's row, j, a).  t's row is v's row of the step before: no rowptr read for it.
//   Rejection sampling diverges: lanes of one wave accept at different attempts.  The loop is therefore over ATTEMPTS, not
// over steps: an iteration is one attempt of whatever step its lane is at, a lane that accepts goes on to its next step in
// the following iteration, and a wave runs for the largest TOTAL number of attempts among its lanes, not for the sum over
// the steps of the largest number per step.
//   Bounds.  Every iteration either moves its lane to the next step or raises its attempt count, which stops at
// GS_WALK_ATTEMPTS (the last attempt is taken whatever it draws): at most (walk_len - 1) * GS_WALK_ATTEMPTS iterations.  The
// search is a for loop of 32 halvings.  An id is range-checked before it indexes rowptr, row bounds are clamped to [0, nnz]
// before they index col, so neither a stray id nor a broken rowptr reads outside the two arrays.
//   UNIFORM (all three thresholds 2^32, p = q = 1): attempt 0 is always accepted, the compare and the search are compiled out.
// The general kernel run at those thresholds gives the same bits (it accepts attempt 0 too and draws the same slot).
//
// walk_pairs_kernel: one lane per walk writes its counts[i] pairs at offsets[i], by walk and then by position.
//
// Resources (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage): quoted in DESIGN.md and
// profiles/random_walks.md.
#include "gs_common.h"

static_assert(sizeof(gs_walk_desc) == 152, "gs_walk_desc layout (mirrored by graphsage_amd/_lib.py)");
static_assert(GS_WALK_ATTEMPTS == 256, "the draw counter is 256 * step + attempt");

#define WALK_THREADS 256
#define WALK_MAX_BLOCKS 2048     // 8 workgroups of 256 on each of 256 CUs; the rest of the walks by grid stride
#define WALK_FULL 0x100000000ull // a threshold that accepts every draw

struct WalkArgs {
    const int64_t* rowptr; const int32_t* col; const int32_t* starts;
    int32_t* paths; int32_t* counts;
    int64_t n_nodes, nnz, n_starts, walk0, n_walks, ld_paths;
    uint64_t key, thr_return, thr_common, thr_far;
    int32_t num_walks, walk_len;
};

// row of node v, clamped into col: [beg, beg + deg), deg < 2^31.  v is in [0, n_nodes).
__device__ __forceinline__ void walk_row(const WalkArgs& g, const int32_t v, int64_t& beg, uint32_t& deg) {
    const int64_t b = min(max(g.rowptr[v], (int64_t)0), g.nnz);
    const int64_t e = min(max(g.rowptr[v + 1], b), g.nnz);
    beg = b;
    deg = (uint32_t)min(e - b, (int64_t)0x7fffffff);
}

// does x occur in the ascending row col[beg .. beg + deg)?  lower bound in at most 32 halvings
__device__ __forceinline__ bool walk_has(const int32_t* __restrict__ col, const int64_t beg, const uint32_t deg, const int32_t x) {
    uint32_t lo = 0u, hi = deg;
#pragma unroll 1
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (col[beg + mid] < x) lo = mid + 1u; else hi = mid;
    }
    return lo < deg && col[beg + lo] == x;
}

template <bool UNIFORM>
__global__ __launch_bounds__(WALK_THREADS) void walk_paths_kernel(const WalkArgs g) {
    const int64_t stride = (int64_t)gridDim.x * WALK_THREADS;
    // the class of x != t matters only for a draw between the two thresholds (never at q = 1, where they are equal)
    const uint64_t thr_lo = min(g.thr_common, g.thr_far), thr_hi = max(g.thr_common, g.thr_far);
    for (int64_t i = (int64_t)blockIdx.x * WALK_THREADS + threadIdx.x; i < g.n_walks; i += stride) {
        const int64_t gw = g.walk0 + i;
        const int64_t si = gw / g.num_walks;
        int32_t* path = g.paths + i * g.ld_paths;
        const int32_t start = si < g.n_starts ? g.starts[si] : -1;
        if (start < 0 || (int64_t)start >= g.n_nodes) {      // no such node: a row of -1, no pairs
            for (int j = 0; j < g.walk_len; ++j) path[j] = -1;
            g.counts[i] = 0;
            continue;
        }
        const uint64_t walkkey = g.key + (uint64_t)gw * 0xD1342543DE82EF95ull;
        path[0] = start;
        int32_t v = start, t = -1, count = 0;
        int64_t vbeg, tbeg = 0;
        uint32_t vdeg, tdeg = 0u;
        walk_row(g, v, vbeg, vdeg);
        int j = 1, a = 0;
        while (j < g.walk_len) {                         // one attempt per iteration
            int32_t x = v;
            bool take = true;
            if (vdeg != 0u) {
                const uint64_t h = gs_mix64(walkkey + (uint64_t)j * GS_WALK_ATTEMPTS + (uint64_t)a);
                x = g.col[vbeg + (int64_t)(((h >> 32) * (uint64_t)vdeg) >> 32)];
                if (!UNIFORM && t >= 0 && a < GS_WALK_ATTEMPTS - 1) {
                    const uint64_t r = h & 0xFFFFFFFFull;
                    if (x == t) take = r < g.thr_return;
                    else if (r < thr_lo) take = true;            // below both thresholds: taken, whichever class x is in
                    else if (r >= thr_hi) take = false;          // at or above both: not taken
                    else take = r < (walk_has(g.col, tbeg, tdeg, x) ? g.thr_common : g.thr_far);
                }
            }
            if (!take) {
                ++a;
                continue;
            }
            if (vdeg != 0u) {                            // a move: v's row becomes t's; a node without a row stays put
                t = v; tbeg = vbeg; tdeg = vdeg;
                v = x;
                if (x >= 0 && (int64_t)x < g.n_nodes) walk_row(g, x, vbeg, vdeg);
                else { vbeg = 0; vdeg = 0u; }            // an id without a row (the pad id): walked to, never from
            }
            path[j] = v;
            count += v != start ? 1 : 0;
            ++j;
            a = 0;
        }
        g.counts[i] = count;
    }
}

__global__ __launch_bounds__(WALK_THREADS) void walk_pairs_kernel(const int32_t* __restrict__ paths, const int64_t* __restrict__ offsets,
                                                                  int32_t* __restrict__ pairs, const int64_t n_walks, const int64_t ld_paths,
                                                                  const int64_t pairs_cap, const int walk_len) {
    const int64_t stride = (int64_t)gridDim.x * WALK_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * WALK_THREADS + threadIdx.x; i < n_walks; i += stride) {
        const int32_t* path = paths + i * ld_paths;
        const int32_t start = path[0];
        if (start < 0) continue;                         // a start that is no node
        int64_t o = offsets[i];
        if (o < 0) continue;
        for (int j = 1; j < walk_len; ++j) {
            const int32_t x = path[j];
            if (x == start) continue;
            if (o < pairs_cap) *reinterpret_cast<int2*>(pairs + 2 * o) = make_int2(start, x);
            ++o;
        }
    }
}

static unsigned walk_blocks(const int64_t n_walks) {
    return (unsigned)std::min<int64_t>(gs_ceil_div(n_walks, WALK_THREADS), WALK_MAX_BLOCKS);
}

static int walk_check_shape(const gs_walk_desc& q, const char* who) {
    GS_REQUIRE(q.n_walks >= 0 && q.walk_len >= 1 && q.walk_len <= GS_WALK_MAX_LEN && q.ld_paths >= q.walk_len,
               "%s: bad sizes n_walks=%lld walk_len=%d (1 .. %d) ld_paths=%lld", who, (long long)q.n_walks, q.walk_len,
               GS_WALK_MAX_LEN, (long long)q.ld_paths);
    GS_REQUIRE(q.n_walks < (1ll << 40), "%s: n_walks=%lld; call it on chunks of the walks", who, (long long)q.n_walks);
    return GS_OK;
}

extern "C" int gs_walk_paths(const gs_walk_desc* desc_host, void* stream) {
    GS_REQUIRE(desc_host, "gs_walk_paths: null descriptor");
    const gs_walk_desc& q = *desc_host;
    if (int rc = walk_check_shape(q, "gs_walk_paths")) return rc;
    GS_REQUIRE(q.n_nodes >= 0 && q.n_nodes <= 0x7fffffffll && q.nnz >= 0 && q.n_starts >= 0 && q.num_walks >= 1 && q.walk0 >= 0 &&
                   q.walk0 < (1ll << 62),
               "gs_walk_paths: bad sizes n_nodes=%lld nnz=%lld n_starts=%lld num_walks=%d walk0=%lld", (long long)q.n_nodes,
               (long long)q.nnz, (long long)q.n_starts, q.num_walks, (long long)q.walk0);
    GS_REQUIRE(q.n_starts <= 0x7fffffffll && q.walk0 + q.n_walks <= q.n_starts * (int64_t)q.num_walks,
               "gs_walk_paths: walks %lld .. %lld lie outside the job of %lld starts x %d walks", (long long)q.walk0,
               (long long)(q.walk0 + q.n_walks), (long long)q.n_starts, q.num_walks);
    const uint64_t lo = std::min(q.thr_return, std::min(q.thr_common, q.thr_far));
    const uint64_t hi = std::max(q.thr_return, std::max(q.thr_common, q.thr_far));
    GS_REQUIRE(hi == WALK_FULL && lo >= (WALK_FULL >> 4),
               "gs_walk_paths: thresholds (%llu, %llu, %llu): the largest must be 2^32 and the smallest at least 2^28, i.e. "
               "min(1/p, 1, 1/q) / max(1/p, 1, 1/q) >= 1/16 (the attempt cap's bound rests on it)",
               (unsigned long long)q.thr_return, (unsigned long long)q.thr_common, (unsigned long long)q.thr_far);
    if (q.n_walks == 0) return GS_OK;
    GS_REQUIRE(q.rowptr && q.starts && q.paths && q.counts && (q.col || q.nnz == 0),
               "gs_walk_paths: rowptr, col, starts, paths and counts must be non-null");
    WalkArgs g;
    g.rowptr = q.rowptr; g.col = q.col; g.starts = q.starts; g.paths = q.paths; g.counts = q.counts;
    g.n_nodes = q.n_nodes; g.nnz = q.nnz; g.n_starts = q.n_starts; g.walk0 = q.walk0; g.n_walks = q.n_walks; g.ld_paths = q.ld_paths;
    g.key = 0ull; g.thr_return = q.thr_return; g.thr_common = q.thr_common; g.thr_far = q.thr_far;
    g.num_walks = q.num_walks; g.walk_len = q.walk_len;
    {   // gs_mix64 on the host: the key is the same for every lane
        uint64_t z = q.seed ^ GS_WALK_TAG;
        z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 27; z *= 0x94D049BB133111EBull; z ^= z >> 31;
        g.key = z;
    }
    const hipStream_t st = (hipStream_t)stream;
    if (lo == WALK_FULL) hipLaunchKernelGGL(walk_paths_kernel<true>, dim3(walk_blocks(q.n_walks)), dim3(WALK_THREADS), 0, st, g);
    else hipLaunchKernelGGL(walk_paths_kernel<false>, dim3(walk_blocks(q.n_walks)), dim3(WALK_THREADS), 0, st, g);
    GS_LAUNCH_CHECK("walk_paths_kernel");
    return GS_OK;
}

extern "C" int gs_walk_pairs(const gs_walk_desc* desc_host, void* stream) {
    GS_REQUIRE(desc_host, "gs_walk_pairs: null descriptor");
    const gs_walk_desc& q = *desc_host;
    if (int rc = walk_check_shape(q, "gs_walk_pairs")) return rc;
    GS_REQUIRE(q.pairs_cap >= 0, "gs_walk_pairs: pairs_cap=%lld", (long long)q.pairs_cap);
    if (q.n_walks == 0) return GS_OK;
    GS_REQUIRE(q.paths && q.offsets && (q.pairs || q.pairs_cap == 0), "gs_walk_pairs: paths, offsets and pairs must be non-null");
    GS_REQUIRE((reinterpret_cast<uintptr_t>(q.pairs) & 7u) == 0, "gs_walk_pairs: pairs must be 8-byte aligned");
    hipLaunchKernelGGL(walk_pairs_kernel, dim3(walk_blocks(q.n_walks)), dim3(WALK_THREADS), 0, (hipStream_t)stream, q.paths,
                       q.offsets, q.pairs, q.n_walks, q.ld_paths, q.pairs_cap, (int)q.walk_len);
    GS_LAUNCH_CHECK("walk_pairs_kernel");
    return GS_OK;
}
