// The select machinery that gs_topk.hip (exhaustive) and gs_ivf.hip (inverted-file scan) share: the uint64 key and its order,
// the append / compact code of a per-row key list, the dump of a finished accumulator tile and the offer of its rows' keys to
// the lists (the epilogue of both scan kernels), the merge kernel over [slices][Q][cap] lists and its host launcher.  Both
// files run THESE functions, so a (score, id) pair maps to the same key, meets the same compares and is reported with the
// same bits in either.  The order, the lists and the reasons are in the header comment of gs_topk.hip.
#pragma once
#include "gs_rank_dev.h"

#define TK_LD 129                // row stride of the dumped accumulator tile, in floats
#define TK_E 3                   // keys per lane when a list is compacted: cap <= 192
#define TK_ROWS 8                // query rows whose scores a wave reads from LDS together
static_assert(RK_BM * TK_LD <= 2 * RK_STAGE_FLOATS, "the dumped tile lives in the two stage buffers");
static_assert(64 * TK_E >= GS_TOPK_MAX + 64, "a compacted list takes 64 more keys");

__device__ __forceinline__ uint64_t topk_key(const float s, const uint32_t w) {
    uint32_t b = s == 0.f ? 0u : __float_as_uint(s);
    b ^= (b >> 31) ? 0xffffffffu : 0x80000000u;
    return ((uint64_t)b << 32) | (uint64_t)(uint32_t)~w;
}
__device__ __forceinline__ float topk_score(const uint64_t key) {
    uint32_t b = (uint32_t)(key >> 32);
    b ^= (b >> 31) ? 0x80000000u : 0xffffffffu;
    return __uint_as_float(b);
}
__device__ __forceinline__ int topk_uniform(const int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t topk_uniform(const uint64_t v) {
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32) |
           (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}

// One wave: keep the k largest of list[0 .. cnt) (distinct keys, k <= cnt <= 64 TK_E) in place and return the k-th largest.
__device__ __forceinline__ uint64_t topk_compact(uint64_t* list, const int cnt, const int k, const int lane) {
    uint64_t key[TK_E];
#pragma unroll
    for (int e = 0; e < TK_E; ++e) key[e] = e * 64 + lane < cnt ? list[e * 64 + lane] : 0ull;
    uint64_t kth = 0ull;         // radix select from the top bit down: wave-uniform all along
    int rem = k;
#pragma unroll 1
    for (int bit = 63; bit >= 0; --bit) {
        const uint64_t want = kth | (1ull << bit);
        const uint64_t mask = ~((1ull << bit) - 1ull);
        int c = 0;
#pragma unroll
        for (int e = 0; e < TK_E; ++e) c += __popcll(__ballot((key[e] & mask) == want));
        if (c >= rem) kth = want; else rem -= c;
    }
    const uint64_t below = (1ull << lane) - 1ull;
    int pos = 0;
#pragma unroll
    for (int e = 0; e < TK_E; ++e) {
        const bool keep = key[e] >= kth && key[e] != 0ull;
        const uint64_t b = __ballot(keep);
        if (keep) list[pos + __popcll(b & below)] = key[e];
        pos += __popcll(b);
    }
    return kth;
}

// One wave appends the keys of its lanes that beat tau (key 0: nothing to offer) to a list of capacity cap >= k + 64.
__device__ __forceinline__ void topk_push(uint64_t* list, const int cap, const int k, int& cnt, uint64_t& tau, const uint64_t key,
                                          const int lane) {
    uint64_t b = __ballot(key > tau);
    if (b == 0ull) return;
    if (cnt + __popcll(b) > cap) {           // cnt > cap - 64 >= k: there is something to drop
        __threadfence_block();               // the appends of this wave's other lanes
        tau = topk_compact(list, cnt, k, lane);
        cnt = k;
        b = __ballot(key > tau);
    }
    if (key > tau) list[cnt + __popcll(b & ((1ull << lane) - 1ull))] = key;
    cnt += __popcll(b);
}

// The finished 128 x 128 accumulator tile into the two stage buffers as [128][TK_LD] floats (lane = column on the way in and on
// the way out: the pad of 1 keeps both free of bank conflicts).  Barriers: every wave is done with the stages; the tile is whole.
__device__ __forceinline__ void topk_dump(const f32x16 (&acc)[2][2], float* smem, const int wm, const int wn, const int l31,
                                          const int lh) {
    __syncthreads();
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int e = 0; e < 16; ++e)
                smem[(wm * 64 + tm * 32 + rank_acc_row(e, lh)) * TK_LD + wn * 64 + tn * 32 + l31] = acc[tm][tn][e];
    __syncthreads();
}

// One wave offers the keys of tile rows r0 .. r0 + TK_ROWS - 1 (two per lane and row; tau_r: the rows' thresholds as read with
// the keys) to the rows' lists: list_of(r) is row r's list, nullptr for a row that does not exist.  A row's length and threshold
// live in cntS / tauS (LDS, touched by this wave only).  list_of is called behind the ballot: ahead of it, whatever it
// computes sits on the critical path of every row (the address: 2.8 % of topk_select_kernel; a slot number alone: 1.5 %).
template <class ListOf>
__device__ __forceinline__ void topk_offer(const uint64_t (&key)[TK_ROWS][2], const uint64_t (&tau_r)[TK_ROWS], const int r0,
                                           int32_t* cntS, uint64_t* tauS, const int cap, const int k, const int lane,
                                           const ListOf list_of) {
#pragma unroll
    for (int i = 0; i < TK_ROWS; ++i) {
        const int r = r0 + i;
        uint64_t tau = topk_uniform(tau_r[i]);
        if (__ballot(key[i][0] > tau || key[i][1] > tau) == 0ull) continue;      // after warm-up: the usual case
        uint64_t* list = list_of(r);
        if (list == nullptr) continue;
        int cnt = topk_uniform(cntS[r]);
        topk_push(list, cap, k, cnt, tau, key[i][0], lane);
        topk_push(list, cap, k, cnt, tau, key[i][1], lane);
        if (lane == 0) {
            cntS[r] = cnt;
            tauS[r] = tau;
        }
    }
}

// one wave per query: the slices' lists -> the k first keys, in order  (static: every file that includes this launches its own)
static __global__ __launch_bounds__(256) void topk_merge_kernel(const uint64_t* __restrict__ lists, const int32_t* __restrict__ counts,
                                                                const int64_t Q, const int slices, const int cap, const int k,
                                                                int32_t* __restrict__ ids, float* __restrict__ scores,
                                                                int32_t* __restrict__ count) {
    __shared__ uint64_t listS[4][64 * TK_E];
    const int lane = threadIdx.x & 63, wave = topk_uniform((int)(threadIdx.x >> 6));
    const int64_t q = (int64_t)blockIdx.x * 4 + wave;
    if (q >= Q) return;                          // (no barrier below: a wave only reads what it wrote)
    uint64_t* list = listS[wave];
    int cnt = 0;
    uint64_t tau = 0ull;
    for (int s = 0; s < slices; ++s) {
        const int n = min(max(topk_uniform(counts[(int64_t)s * Q + q]), 0), cap);
        const uint64_t* in = lists + ((int64_t)s * Q + q) * cap;
        for (int c0 = 0; c0 < n; c0 += 64)
            topk_push(list, 64 * TK_E, k, cnt, tau, c0 + lane < n ? in[c0 + lane] : 0ull, lane);
    }
    __threadfence_block();
    if (cnt > k) {
        topk_compact(list, cnt, k, lane);
        cnt = k;
        __threadfence_block();
    }
    // rank by counting: at most 128 distinct keys, two per lane
    const uint64_t key0 = lane < cnt ? list[lane] : 0ull;
    const uint64_t key1 = lane + 64 < cnt ? list[lane + 64] : 0ull;
    int r0 = 0, r1 = 0;
    for (int j = 0; j < cnt; ++j) {
        const uint64_t kj = list[j];
        r0 += kj > key0 ? 1 : 0;
        r1 += kj > key1 ? 1 : 0;
    }
    int32_t* ids_q = ids + q * k;
    float* scores_q = scores + q * k;
    if (lane < cnt) {
        ids_q[r0] = (int32_t)~(uint32_t)key0;
        scores_q[r0] = topk_score(key0);
    }
    if (lane + 64 < cnt) {
        ids_q[r1] = (int32_t)~(uint32_t)key1;
        scores_q[r1] = topk_score(key1);
    }
    for (int p = lane; p < k; p += 64)
        if (p >= cnt) {
            ids_q[p] = -1;
            scores_q[p] = -INFINITY;
        }
    if (lane == 0) count[q] = cnt;
}

static inline int64_t topk_cap(const int k) { return 64 * (1 + gs_ceil_div(k, 64)); }

// lists [slices][Q][cap] and counts [slices][Q] -> ids, scores [Q][k], count [Q]; Q >= 1, ceil(Q / 4) < 2^31 (the caller checked)
static inline int topk_merge_launch(const uint64_t* lists, const int32_t* counts, const int64_t Q, const int slices, const int cap,
                                    const int k, int32_t* ids, float* scores, int32_t* count, const hipStream_t st) {
    hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)gs_ceil_div(Q, 4)), dim3(256), 0, st, lists, counts, Q, slices, cap, k, ids,
                       scores, count);
    GS_LAUNCH_CHECK("topk_merge_kernel");
    return GS_OK;
}
