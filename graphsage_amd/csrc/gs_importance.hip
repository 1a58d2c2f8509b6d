// Importance neighborhoods (PinSage): the nodes that short random walks from u visit most often, as a [n_starts][slots] table in
// which a node's multiplicity is its share of the visits.  The rule, the limits and the descriptor: include/graphsage_amd.h,
// section IMPORTANCE; restated in NumPy in tests/importance_oracle.py and checked bit for bit.
//
// importance_table_kernel: one wave per start (a workgroup IS one wave, so __syncthreads() orders the wave's LDS traffic and
// is no workgroup barrier: the backend emits the waits alone), starts by grid stride.  Per start, with V = num_walks *
// (walk_len - 1) visits and P = max(64, the power of two >= V):
//   1. the visits into LDS as int32 keys, a visit that is not kept (out of range, the start itself) as INT32_MAX; a bitonic
//      sort of the P keys: the kept visits come out first, ascending;
//   2. run heads by comparison with the left neighbor, their run index by ballot + popcount: pos[run] = first position,
//      pos[m] = kept, so c(run) = pos[run + 1] - pos[run]; ids[run] = the id.  Runs are in ascending id order, so "id
//      ascending" is "run index ascending" from here on and no later key carries an id;
//   3. a bitonic sort of the m keys (4096 - c) << 32 | run: the first s = min(m, top) are the selected set;
//   4. C and sum q by wave reductions, then a bitonic sort of the s keys (C - r) << 32 | run << 16 | q: the first `rest` get
//      one more slot; n_k goes to nk[run] (zero for a run that was not selected);
//   5. a running sum of nk over the runs, and slot j of the row is the id of the first run whose running sum exceeds j (binary
//      search, at most 12 probes): lane j writes slot j, 64 consecutive dwords per store instruction.
// Every sort is over the power of two at or above ITS count (m and s are wave-uniform), so at the drivers' sizes (V = 100 ..
// 400, a few dozen distinct nodes) sorts 3 and 4 are a handful of stages.  One form for every V from 1 to 4096: there is no
// switch point.  Integers only, no atomics, every lane writes its own entries: bitwise reproducible.
//   Bounds.  Every LDS index is below P (pos: at most P, the array has P + 1 entries): positions are < kept <= V <= P, run
// indices < m <= kept, selected ranks < s <= m.  A path entry is read only for r < num_walks and 1 <= j < walk_len <= ld_paths,
// a table entry is written only for j < slots, both inside start i's rows, i < n_starts.  The search keeps lo in [0, m - 1]
// whatever the running sums hold.
//
// Resources (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage): quoted in DESIGN.md §8h and
// profiles/importance_neighbors.md.
#include "gs_common.h"

static_assert(sizeof(gs_importance_desc) == 72, "gs_importance_desc layout (mirrored by graphsage_amd/_lib.py)");
static_assert(GS_IMPORTANCE_MAX_VISITS == 4096, "a count fits 13 bits and a run index 12 in the sort keys");
static_assert(GS_IMPORTANCE_MAX_SLOTS <= 1024, "a quotient fits the 16 low bits of the remainder key; c * slots <= 2^22");

#define IMP_LANES 64
#define IMP_MAX_BLOCKS (1 << 16)     // 256 workgroups of one wave on each of 256 CUs; the rest of the starts by grid stride
#define IMP_NONE 0x7fffffff          // key of a visit that is not kept: above every node id (n_nodes <= 2^31 - 1)

struct ImpArgs {
    const int32_t* paths; int32_t* table; int32_t* stats;
    int64_t n_starts, ld_paths;
    int32_t n_nodes, num_walks, walk_len, top, slots, pad_id, V, P;
};

static inline int imp_pow2(int n) {           // the power of two at or above max(n, 2)
    int p = 2;
    while (p < n) p <<= 1;
    return p;
}
static inline size_t imp_lds_bytes(const int P) { return (size_t)P * 20 + 16; }

__device__ __forceinline__ int imp_pow2_dev(const int n) { return n <= 2 ? 2 : 1 << (32 - __clz(n - 1)); }

__device__ __forceinline__ int imp_wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// ascending bitonic sort of a[0 .. n), n a power of two >= 2 (wave-uniform), by the one wave of the workgroup; ends in the barrier
template <typename T>
__device__ __forceinline__ void imp_sort(T* a, const int n, const int lane) {
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (n >> 1); t += IMP_LANES) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int p = i | j;
                const T x = a[i], y = a[p];
                if ((x > y) == ((i & k) == 0)) { a[i] = y; a[p] = x; }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(IMP_LANES) void importance_table_kernel(const ImpArgs g) {
    extern __shared__ __align__(16) unsigned char imp_lds[];
    uint64_t* a = reinterpret_cast<uint64_t*>(imp_lds);     // [P] keys of sorts 3 and 4
    int32_t* key = reinterpret_cast<int32_t*>(a + g.P);     // [P] the visits (sort 1)
    int32_t* ids = key + g.P;                               // [P] id of run r
    int32_t* pos = ids + g.P;                               // [P + 1] first position of run r; then n_k by run; then its running sum
    const int lane = threadIdx.x;
    const int lm1 = g.walk_len - 1;
    for (int64_t i = blockIdx.x; i < g.n_starts; i += gridDim.x) {
        int32_t* row = g.table + i * g.slots;
        const int32_t* wp = g.paths + i * g.num_walks * g.ld_paths;
        const int32_t u = wp[0];
        int kept = 0;
        if (u >= 0 && u < g.n_nodes) {
            for (int v = lane; v < g.P; v += IMP_LANES) {
                int32_t x = IMP_NONE;
                if (v < g.V) {
                    const int r = v / lm1;
                    x = wp[(int64_t)r * g.ld_paths + 1 + (v - r * lm1)];
                    if (x < 0 || x >= g.n_nodes || x == u) x = IMP_NONE;
                }
                key[v] = x;
                kept += __popcll(__ballot(x != IMP_NONE));
            }
        }
        if (kept == 0) {                                    // a start that is no node, or no visit kept: uniform over the wave
            for (int j = lane; j < g.slots; j += IMP_LANES) row[j] = g.pad_id;
            if (lane == 0) { g.stats[2 * i] = 0; g.stats[2 * i + 1] = 0; }
            __syncthreads();                                // (the keys written above, before the next start's)
            continue;
        }
        __syncthreads();
        imp_sort<int32_t>(key, g.P, lane);

        int m = 0;                                          // runs
        for (int base = 0; base < kept; base += IMP_LANES) {
            const int p = base + lane;
            const bool head = p < kept && (p == 0 || key[p] != key[p - 1]);
            const uint64_t mask = __ballot(head);
            if (head) {
                const int r = m + __popcll(mask & ((1ull << lane) - 1ull));
                pos[r] = p;
                ids[r] = key[p];
            }
            m += __popcll(mask);
        }
        if (lane == 0) pos[m] = kept;
        __syncthreads();

        const int n2 = imp_pow2_dev(m);
        for (int r = lane; r < n2; r += IMP_LANES)
            a[r] = r < m ? ((uint64_t)(uint32_t)(GS_IMPORTANCE_MAX_VISITS - (pos[r + 1] - pos[r])) << 32) | (uint32_t)r : ~0ull;
        __syncthreads();
        for (int r = lane; r < m; r += IMP_LANES) pos[r] = 0;     // pos is nk from here (the sort's barriers stand between)
        imp_sort<uint64_t>(a, n2, lane);

        const int s = min(m, g.top);
        int C = 0;
        for (int r = lane; r < s; r += IMP_LANES) C += GS_IMPORTANCE_MAX_VISITS - (int)(a[r] >> 32);
        C = imp_wave_sum(C);
        const int n3 = imp_pow2_dev(s);
        int sumq = 0;
        for (int r = lane; r < n3; r += IMP_LANES) {
            uint64_t k3 = ~0ull;
            if (r < s) {
                const uint64_t k2 = a[r];
                const int t = (GS_IMPORTANCE_MAX_VISITS - (int)(k2 >> 32)) * g.slots;
                const int q = t / C;
                sumq += q;
                k3 = ((uint64_t)(uint32_t)(C - (t - q * C)) << 32) | ((uint32_t)k2 << 16) | (uint32_t)q;
            }
            a[r] = k3;                                      // each lane rewrites the entries it read
        }
        const int rest = g.slots - imp_wave_sum(sumq);
        __syncthreads();
        imp_sort<uint64_t>(a, n3, lane);

        int nz = 0;
        for (int base = 0; base < s; base += IMP_LANES) {
            const int r = base + lane;
            int n = 0;
            if (r < s) {
                const uint32_t lo = (uint32_t)a[r];
                n = (int)(lo & 0xffffu) + (r < rest ? 1 : 0);
                pos[lo >> 16] = n;                          // run indices are distinct
            }
            nz += __popcll(__ballot(n > 0));
        }
        __syncthreads();

        int carry = 0;                                      // running sum of nk over the runs, in place
        for (int base = 0; base < m; base += IMP_LANES) {
            const int r = base + lane;
            int v = r < m ? pos[r] : 0;
#pragma unroll
            for (int off = 1; off < IMP_LANES; off <<= 1) {
                const int t = __shfl_up(v, off, 64);
                if (lane >= off) v += t;
            }
            v += carry;
            if (r < m) pos[r] = v;
            carry = __shfl(v, IMP_LANES - 1, 64);
        }
        __syncthreads();

        for (int j = lane; j < g.slots; j += IMP_LANES) {
            int lo = 0, hi = m - 1;                         // pos[m - 1] == slots > j
#pragma unroll 1
            for (int it = 0; it < 13 && lo < hi; ++it) {
                const int mid = (lo + hi) >> 1;
                if (pos[mid] > j) hi = mid; else lo = mid + 1;
            }
            row[j] = ids[lo];
        }
        if (lane == 0) { g.stats[2 * i] = m; g.stats[2 * i + 1] = nz; }
        __syncthreads();                                    // LDS is the next start's
    }
}

extern "C" int gs_importance_table(const gs_importance_desc* desc_host, void* stream) {
    GS_REQUIRE(desc_host, "gs_importance_table: null descriptor");
    const gs_importance_desc& q = *desc_host;
    GS_REQUIRE(q.num_walks >= 1 && q.walk_len >= 2, "gs_importance_table: num_walks=%d must be at least 1 and walk_len=%d at least 2",
               q.num_walks, q.walk_len);
    const int64_t V = (int64_t)q.num_walks * (q.walk_len - 1);
    GS_REQUIRE(V <= GS_IMPORTANCE_MAX_VISITS, "gs_importance_table: num_walks * (walk_len - 1) = %lld visits per start; at most %d",
               (long long)V, GS_IMPORTANCE_MAX_VISITS);
    GS_REQUIRE(q.top >= 1 && q.top <= GS_IMPORTANCE_MAX_TOP && q.slots >= 1 && q.slots <= GS_IMPORTANCE_MAX_SLOTS,
               "gs_importance_table: top=%d (1 .. %d) slots=%d (1 .. %d)", q.top, GS_IMPORTANCE_MAX_TOP, q.slots,
               GS_IMPORTANCE_MAX_SLOTS);
    GS_REQUIRE(q.ld_paths >= q.walk_len && q.n_starts >= 0 && q.n_starts < (1ll << 40) && q.n_nodes >= 0 && q.n_nodes <= 0x7fffffffll,
               "gs_importance_table: bad sizes n_starts=%lld n_nodes=%lld ld_paths=%lld (>= walk_len=%d)", (long long)q.n_starts,
               (long long)q.n_nodes, (long long)q.ld_paths, q.walk_len);
    GS_REQUIRE(q.reserved_ == 0, "gs_importance_table: reserved_ must be 0");
    if (q.n_starts == 0) return GS_OK;
    GS_REQUIRE(q.paths && q.table && q.stats, "gs_importance_table: paths, table and stats must be non-null");
    ImpArgs g;
    g.paths = q.paths; g.table = q.table; g.stats = q.stats;
    g.n_starts = q.n_starts; g.ld_paths = q.ld_paths;
    g.n_nodes = (int32_t)q.n_nodes; g.num_walks = q.num_walks; g.walk_len = q.walk_len; g.top = q.top; g.slots = q.slots;
    g.pad_id = q.pad_id; g.V = (int32_t)V; g.P = std::max(IMP_LANES, imp_pow2((int)V));
    const size_t lds = imp_lds_bytes(g.P);
    if (lds > 48 * 1024) GS_LDS_ATTR(imp_lds_bytes(GS_IMPORTANCE_MAX_VISITS), importance_table_kernel);
    const unsigned blocks = (unsigned)std::min<int64_t>(q.n_starts, IMP_MAX_BLOCKS);
    hipLaunchKernelGGL(importance_table_kernel, dim3(blocks), dim3(IMP_LANES), lds, (hipStream_t)stream, g);
    GS_LAUNCH_CHECK("importance_table_kernel");
    return GS_OK;
}
