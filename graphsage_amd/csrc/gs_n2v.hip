// N2V: the node2vec / DeepWalk baseline (graphsage/models.py:408-504, Node2VecModel): two trainable embedding tables and a
// bias vector that are gathered, scored and updated in place by plain SGD, rows repeated within a batch.  A step is three
// launches; the tables are never copied or densified and no float atomic is used, so a step is bitwise reproducible:
//   n2v_stage_kernel    edge pairs through the device cursor (as unsup_stage_kernel) + n_neg DISTINCT negatives
//                       (tf.nn.fixed_unigram_candidate_sampler(unique=True), models.py:449-456)
//   n2v_fwd_bwd_kernel  gather, affinities with and without the bias, loss / aff_all / reciprocal ranks / outputs1
//                       (models.py:477-503) and the gradient ROWS into a per-step staging buffer
//   n2v_apply_kernel    GradientDescentOptimizer on indexed slices: per destination row ONE owner sums the staged rows
//                       of every slot with that id in ascending slot order and subtracts once
// ids = [batch1 (B) | batch2 (B) | negatives (n_neg)] everywhere.  Row offsets are 64-bit (tables of 10^7 rows).
#include "gs_linkpred_dev.h"
#include "gs_sample_dev.h"

#define N2V_MAX_NEG 1024          // kept list of the unique sampler (LDS)
#define N2V_MAX_ROUNDS 4096       // 64 draws each; the host refuses a distribution with fewer than n_neg reachable nodes
#define N2V_LDS_IDS 4096          // id list of the apply launch staged in LDS up to this many slots

// One wave walks the counter-hash stream of draws of unsup_stage_kernel (draw t: the first node whose cdf exceeds the high
// word of mix64(key + t + slot_offset)) 64 at a time and keeps the first n_neg distinct nodes in stream order.
// Restated in tests/n2v_oracle.py::sample_unigram_unique.
__global__ __launch_bounds__(256) void n2v_stage_kernel(const int32_t* __restrict__ pairs, int64_t n_pairs,
                                                        const uint64_t* __restrict__ cursor, int64_t B,
                                                        const uint32_t* __restrict__ cdf, int64_t n_nodes, int32_t n_neg,
                                                        uint64_t seed, const uint64_t* __restrict__ clock, int64_t slot_offset,
                                                        int32_t* __restrict__ ids_out, int32_t* __restrict__ status,
                                                        int32_t pair_blocks, const int32_t* __restrict__ guide,
                                                        int32_t guide_bits) {
    __shared__ int32_t kept[N2V_MAX_NEG];
    if ((int)blockIdx.x < pair_blocks) {
        const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (t < B) {
            const uint64_t c = cursor ? *cursor : 0ull;
            ids_out[t] = gs_stage_pair(pairs, n_pairs, c, t, 0);
            ids_out[B + t] = gs_stage_pair(pairs, n_pairs, c, t, 1);
        }
        return;
    }
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    const uint64_t st = clock ? *clock : 0ull;
    int n_kept = 0;
    for (int round = 0; round < N2V_MAX_ROUNDS && n_kept < n_neg; ++round) {
        const uint64_t t = (uint64_t)round * 64ull + (uint64_t)lane;
        const int32_t id = gs_unigram_pick(cdf, n_nodes, guide, guide_bits, gs_unigram_draw32(seed, st, t + (uint64_t)slot_offset));
        bool fresh = true;
        for (int k = 0; k < n_kept; ++k) fresh = fresh && kept[k] != id;
        for (int l = 0; l < 63; ++l) {                         // an earlier draw of this round with the same node
            const int32_t o = __shfl(id, l, 64);
            fresh = fresh && !(l < lane && o == id);
        }
        const uint64_t mask = __ballot(fresh);
        const int pos = n_kept + __popcll(mask & ((1ull << lane) - 1ull));
        if (fresh && pos < n_neg) kept[pos] = id;
        n_kept = min(n_neg, n_kept + (int)__popcll(mask));
        // the other lanes' writes are read in the next round: one wave, so a fence and a wave barrier are enough
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
    // unreachable after the host's check; never spin: repeat the first node and report through *status
    for (int k = lane; k < n_neg; k += 64) ids_out[2 * B + k] = k < n_kept ? kept[k] : (n_kept > 0 ? kept[0] : 0);
    if (status && lane == 0 && n_kept < n_neg) *status = 1;
}

extern "C" int gs_n2v_stage(const int32_t* pairs, int64_t n_pairs, const uint64_t* cursor_dev, int64_t B, const uint32_t* cdf,
                            int64_t n_nodes, int32_t n_neg, uint64_t seed, const uint64_t* clock_dev, int64_t slot_offset,
                            const int32_t* guide, int32_t guide_bits, int32_t* ids_out, int32_t* status, void* stream) {
    GS_REQUIRE(ids_out && B >= 0 && n_neg >= 0, "gs_n2v_stage: bad args");
    GS_REQUIRE(!guide || (cdf && guide_bits >= 1 && guide_bits <= 20), "gs_n2v_stage: guide_bits in 1..20");
    GS_REQUIRE(!pairs || n_pairs > 0, "gs_n2v_stage: empty pair list");
    GS_REQUIRE(!cdf || (n_nodes > 0 && n_nodes <= 0x7fffffffll), "gs_n2v_stage: bad cdf length %lld", (long long)n_nodes);
    GS_REQUIRE(n_neg <= N2V_MAX_NEG, "gs_n2v_stage: at most %d distinct negatives (got %d)", N2V_MAX_NEG, n_neg);
    GS_REQUIRE(!cdf || n_neg <= n_nodes, "gs_n2v_stage: %d distinct negatives out of %lld nodes", n_neg, (long long)n_nodes);
    const int32_t pair_blocks = pairs ? (int32_t)gs_ceil_div(B, 256) : 0;
    const int32_t neg_blocks = (cdf && n_neg > 0) ? 1 : 0;
    if (pair_blocks + neg_blocks == 0) return GS_OK;
    hipLaunchKernelGGL(n2v_stage_kernel, dim3((unsigned)(pair_blocks + neg_blocks)), dim3(256), 0, (hipStream_t)stream, pairs,
                       n_pairs, cursor_dev, B, cdf, n_nodes, n_neg, seed, clock_dev, slot_offset, ids_out, status, pair_blocks, guide,
                       guide_bits);
    GS_LAUNCH_CHECK("n2v_stage_kernel");
    return GS_OK;
}

struct N2vFwd {
    const float* target; int64_t ldt;
    const float* context; int64_t ldc;
    const float* bias;
    const int32_t* ids; int64_t B; int32_t n_neg; int32_t train; float scale;
    float* loss_rows; float* rr_rows; float* aff_all; int64_t ld_aff; float* outputs1; int64_t ldo;
    float* g_target;    // [B, d]          d loss / d target[batch1[i]]
    float* g_ctx;       // [B, d]          d loss / d context[batch2[i]]   (the negatives' rows: neg_slabs)
    float* g_bias;      // [B]
    float* neg_slabs;   // [workgroups][n_neg][d]
    float* bias_slabs;  // [workgroups][n_neg]
};

// One wave = one pair against all negatives; blockDim.x / 64 pairs per workgroup (4, or fewer where 4 partial-gradient
// images do not fit LDS beside the negatives' rows).  With o1 = target[batch1[i]], o2 = context[batch2[i]], neg_q =
// context[neg[q]] (once per workgroup into LDS):
//   aff = <o1, o2>, nav_q = <o1, neg_q>                          -> aff_all, ranks (prediction.py: WITHOUT the bias)
//   loss_i = xent(1, aff + bias[batch2[i]]) + sum_q xent(0, nav_q + bias[neg[q]])                    (models.py:477-487)
//   da = scale (sigmoid(aff + b) - 1), gq = scale sigmoid(nav_q + b_q)
//   g_target[i] = da o2 + sum_q gq neg_q;  g_ctx[i] = da o1;  g_bias[i] = da;  slab[q] = sum_waves gq o1;  bslab[q] = sum gq
template <int DJ>
__global__ __launch_bounds__(256) void n2v_fwd_bwd_kernel(const N2vFwd a) {
    constexpr int d = DJ * 64;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int nw = blockDim.x >> 6, n_neg = a.n_neg;
    float* negs = lds;                                 // [n_neg][d]
    float* part = negs + (size_t)n_neg * d;            // [nw][n_neg][d]
    float* nbias = part + (size_t)nw * n_neg * d;      // [n_neg]
    float* partb = nbias + n_neg;                      // [nw][n_neg]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t B = a.B;
    const int32_t* nid = a.ids + 2 * B;
    // the pair's own rows first: their loads fly while the negatives are staged
    const int64_t i = (int64_t)blockIdx.x * nw + wave;
    const bool live = i < B;
    const int64_t ic = live ? i : 0;
    const int64_t v1 = a.ids[ic], v2 = a.ids[B + ic];
    const bool train = a.train != 0;
    float o1[DJ], o2[DJ], g1[DJ];
#pragma unroll
    for (int j = 0; j < DJ; ++j) {
        o1[j] = a.target[v1 * a.ldt + j * 64 + lane];
        o2[j] = a.context[v2 * a.ldc + j * 64 + lane];
    }
    const float bias2 = a.bias[v2];
    // the negatives' rows, one per wave at a time and four in flight: first the four ids, then every load of the four rows,
    // then the LDS stores (a loop of id load -> row load -> store is n_neg * d / 256 times two dependent round trips)
    // (rows past the end are clamped to the last one and loaded unconditionally: branch-free, so the loads stay batched)
    const float nb0 = a.bias[nid[min(tid, n_neg - 1)]];
    for (int q0 = wave; q0 < n_neg; q0 += 4 * nw) {
        int64_t vq[4];
        float r[4][DJ];
#pragma unroll
        for (int u = 0; u < 4; ++u) vq[u] = nid[min(q0 + u * nw, n_neg - 1)];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < DJ; ++j) r[u][j] = a.context[vq[u] * a.ldc + j * 64 + lane];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (q0 + u * nw < n_neg) {
#pragma unroll
                for (int j = 0; j < DJ; ++j) negs[(size_t)(q0 + u * nw) * d + j * 64 + lane] = r[u][j];
            }
    }
    if (tid < n_neg) nbias[tid] = nb0;
    for (int t = tid + blockDim.x; t < n_neg; t += blockDim.x) nbias[t] = a.bias[nid[t]];
    __syncthreads();
    float aff = 0.f;
#pragma unroll
    for (int j = 0; j < DJ; ++j) aff += o1[j] * o2[j];
    aff = gs_wave_sum(aff);
    const float affb = aff + bias2;
    float sa, lga;
    gs_sigmoid_lg(affb, sa, lga);
    const float da = (sa - 1.0f) * a.scale;
    float loss = fmaxf(affb, 0.f) - affb + lga;
    int rank = 0;
#pragma unroll
    for (int j = 0; j < DJ; ++j) g1[j] = da * o2[j];
    float* mypart = part + (size_t)wave * n_neg * d;
    float* mypartb = partb + (size_t)wave * n_neg;
    for (int qb = 0; qb < n_neg; qb += 64) {
        const int nq = min(64, n_neg - qb);                       // wave-uniform
        const float nav = lp_neg_affinities<DJ>(o1, negs, qb, nq, lane);   // lane q: negative qb + q
        const bool in = lane < nq;
        const float navb = nav + (in ? nbias[qb + lane] : 0.f);
        float sg, lg;                                             // sigmoid(nav + bias)
        gs_sigmoid_lg(navb, sg, lg);
        loss += gs_wave_sum(in ? fmaxf(navb, 0.f) + lg : 0.f);
        rank += __popcll(__ballot(in && nav >= aff));
        if (live && in && a.aff_all) a.aff_all[i * a.ld_aff + qb + lane] = nav;
        if (train) {
            const float gqv = (in && live) ? a.scale * sg : 0.f;
            if (in) mypartb[qb + lane] = gqv;
            for (int q = 0; q < nq; ++q) {
                const float gq = __shfl(gqv, q, 64);
                const float* nr = negs + (size_t)(qb + q) * d + lane;
                float* mp = mypart + (size_t)(qb + q) * d + lane;
#pragma unroll
                for (int j = 0; j < DJ; ++j) {
                    g1[j] += gq * nr[j * 64];
                    mp[j * 64] = gq * o1[j];
                }
            }
        }
    }
    if (live) {
#pragma unroll
        for (int j = 0; j < DJ; ++j) {
            a.outputs1[i * a.ldo + j * 64 + lane] = o1[j];
            if (train) {
                a.g_target[i * d + j * 64 + lane] = g1[j];
                a.g_ctx[i * d + j * 64 + lane] = da * o1[j];
            }
        }
        if (lane == 0) {
            a.loss_rows[i] = loss;
            a.rr_rows[i] = 1.0f / (float)(rank + 1);
            if (a.aff_all) a.aff_all[i * a.ld_aff + n_neg] = aff;
            if (train) a.g_bias[i] = da;
        }
    }
    if (!train) return;                                           // kernel-uniform
    __syncthreads();
    // the workgroup's slab: its waves' images summed in a fixed order, 16 bytes per lane (the wave count is spelled out: a
    // runtime loop over the images is a chain of dependent LDS reads per element)
    const int img4 = n_neg * (d >> 2);
    const f32x4* p4 = reinterpret_cast<const f32x4*>(part);
    f32x4* slab4 = reinterpret_cast<f32x4*>(a.neg_slabs + (size_t)blockIdx.x * n_neg * d);
    if (nw == 4) {
#pragma unroll 2
        for (int t = tid; t < img4; t += 256) slab4[t] = (p4[t] + p4[img4 + t]) + (p4[2 * img4 + t] + p4[3 * img4 + t]);
    } else if (nw == 2) {
#pragma unroll 2
        for (int t = tid; t < img4; t += 128) slab4[t] = p4[t] + p4[img4 + t];
    } else {
        for (int t = tid; t < img4; t += 64) slab4[t] = p4[t];
    }
    float* bslab = a.bias_slabs + (size_t)blockIdx.x * n_neg;
    for (int t = tid; t < n_neg; t += blockDim.x) {
        float s = partb[t];
        for (int w = 1; w < nw; ++w) s += partb[w * n_neg + t];
        bslab[t] = s;
    }
}

#define N2V_LDS_CAP (160 * 1024)
static size_t n2v_lds_bytes(int nw, int n_neg, int d) { return ((size_t)(1 + nw) * n_neg * d + (size_t)(1 + nw) * n_neg) * sizeof(float); }
// pairs per workgroup: 4 where the images fit, else 2, else 1, else 0 (refused)
static int n2v_waves(int n_neg, int d) {
    for (int nw = 4; nw >= 1; nw >>= 1)
        if (n2v_lds_bytes(nw, n_neg, d) <= N2V_LDS_CAP) return nw;
    return 0;
}

extern "C" int gs_n2v_supported(int32_t d, int32_t n_neg) {
    return (d == 64 || d == 128 || d == 256 || d == 512) && n_neg >= 1 && n_neg <= N2V_MAX_NEG && n2v_waves(n_neg, d) > 0;
}

extern "C" int gs_n2v_slabs(int64_t B, int32_t d, int32_t n_neg) {
    const int nw = n2v_waves(n_neg, d);
    return nw > 0 ? (int)gs_ceil_div(B, nw) : 0;
}

extern "C" int gs_n2v_fwd_bwd(const float* target, int64_t ldt, const float* context, int64_t ldc, const float* bias,
                              int64_t n_rows, const int32_t* ids, int64_t B, int32_t d, int32_t n_neg, int train,
                              float* loss_rows, float* rr_rows, float* aff_all, int64_t ld_aff, float* outputs1, int64_t ldo,
                              float* g_target, float* g_ctx, float* g_bias, float* neg_slabs, float* bias_slabs, void* stream) {
    GS_REQUIRE(target && context && bias && ids && loss_rows && rr_rows && outputs1 && B > 0 && n_rows > 0,
               "gs_n2v_fwd_bwd: bad args");
    GS_REQUIRE(B <= 0x3fffffffll && n_rows <= 0x7fffffffll, "gs_n2v_fwd_bwd: B / table rows out of range");
    GS_REQUIRE(d == 64 || d == 128 || d == 256 || d == 512, "gs_n2v_fwd_bwd: d must be 64/128/256/512 (got %d)", d);
    GS_REQUIRE(n_neg >= 1 && n_neg <= N2V_MAX_NEG, "gs_n2v_fwd_bwd: n_neg must be in [1, %d] (got %d)", N2V_MAX_NEG, n_neg);
    GS_REQUIRE(ldt >= d && ldc >= d && ldo >= d && (!aff_all || ld_aff >= n_neg + 1), "gs_n2v_fwd_bwd: ld too small");
    GS_REQUIRE(!train || (g_target && g_ctx && g_bias && neg_slabs && bias_slabs && gs_aligned16(neg_slabs)),
               "gs_n2v_fwd_bwd: gradient buffers missing (neg_slabs 16-byte aligned)");
    const int nw = n2v_waves(n_neg, d);
    GS_REQUIRE(nw > 0, "gs_n2v_fwd_bwd: %d negatives x d=%d do not fit LDS", n_neg, d);
    const size_t lds_bytes = n2v_lds_bytes(nw, n_neg, d);
    const int64_t blocks = gs_ceil_div(B, nw);
    const N2vFwd a = {target, ldt, context, ldc, bias, ids, B, n_neg, train ? 1 : 0, 1.0f / (float)B, loss_rows, rr_rows, aff_all,
                      ld_aff, outputs1, ldo, g_target, g_ctx, g_bias, neg_slabs, bias_slabs};
    hipStream_t st = (hipStream_t)stream;
#define GS_N2V(DJ)                                                                                                       \
    do {                                                                                                                 \
        GS_LDS_ATTR(N2V_LDS_CAP, n2v_fwd_bwd_kernel<DJ>);                                                                \
        hipLaunchKernelGGL((n2v_fwd_bwd_kernel<DJ>), dim3((unsigned)blocks), dim3(64 * nw), lds_bytes, st, a);           \
    } while (0)
    if (d == 64) GS_N2V(1); else if (d == 128) GS_N2V(2); else if (d == 256) GS_N2V(4); else GS_N2V(8);
#undef GS_N2V
    GS_LAUNCH_CHECK("n2v_fwd_bwd_kernel");
    return GS_OK;
}

struct N2vApply {
    float* target; int64_t ldt;
    float* context; int64_t ldc;
    float* bias;
    const int32_t* ids; int64_t B; int32_t n_neg; int32_t n_slabs; float lr;
    const float* g_target; const float* g_ctx; const float* g_bias; const float* neg_slabs; const float* bias_slabs;
    int32_t pair_blocks;
    StepEpilogue epi;
};

// Slots of the context table / bias in ascending order: [negatives (n_neg) | batch2 (B)]; of the target table: batch1 (B).
// The owner of a destination row is the first slot that holds its id.  Negatives are distinct, so a negative's slot always
// owns its row and a batch2 slot owns its row iff the id is no negative and no earlier batch2 slot holds it.
//   workgroups [0, n_neg)             one per negative q: the row's gradient = sum of the per-workgroup slabs of the forward
//                                     launch in a fixed order, then + g_ctx[s] of every batch2 slot s with that id, ascending
//   [n_neg, n_neg + pair_blocks)      target table, one wave per batch1 slot
//   [.., n_neg + 2 pair_blocks)       context table and bias, one wave per batch2 slot
//   last (has_epi)                    the step epilogue: mean loss / mrr and the device counters
// Every read of the tables happened in the launch before; here each touched row is read and written by its owner only.
template <int DJ>
__global__ __launch_bounds__(256) void n2v_apply_kernel(const N2vApply a) {
    constexpr int d = DJ * 64;
    __shared__ int32_t ids_lds[N2V_LDS_IDS];
    __shared__ f32x4 gpart[256];
    __shared__ unsigned long long masks[4];
    __shared__ float red[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_neg = a.n_neg;
    const int64_t B = a.B;
    const int blk = blockIdx.x;
    if (blk == n_neg + 2 * a.pair_blocks) {
        gs_step_epilogue_block(a.epi, red[0], red[1]);
        return;
    }
    // the list this workgroup scans: batch1 for the target table, [batch2 | negatives] otherwise
    const bool is_target = blk >= n_neg && blk < n_neg + a.pair_blocks;
    const int32_t* gl = is_target ? a.ids : a.ids + B;
    const int64_t n_list = is_target ? B : B + n_neg;
    const int32_t* list = gl;
    if (n_list <= N2V_LDS_IDS) {
        for (int t = tid; t < (int)n_list; t += 256) ids_lds[t] = gl[t];
        list = ids_lds;
    }
    __syncthreads();
    if (blk < n_neg) {
        const int q = blk;
        const int64_t v = list[B + q];
        constexpr int d4 = d >> 2, SG = 256 / d4;          // d in {64 .. 512}: d4 in {16 .. 128}, SG in {16 .. 2}
        const int cg = tid % d4, sg = tid / d4;
        const f32x4* sp = reinterpret_cast<const f32x4*>(a.neg_slabs + (size_t)q * d) + cg;
        const size_t stride4 = (size_t)n_neg * d4;         // float4 per slab
        const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
        f32x4 acc[4] = {zero4, zero4, zero4, zero4};
        int sI = sg;
        for (; sI + 15 * SG < a.n_slabs; sI += 16 * SG) {
            f32x4 u[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) u[k] = sp[(size_t)(sI + k * SG) * stride4];
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[k & 3] += u[k];
        }
        for (; sI < a.n_slabs; sI += SG) acc[0] += sp[(size_t)sI * stride4];
        gpart[tid] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
        float gb = 0.f;                                    // bias: wave 0 sums the slabs' entries, lane-strided then butterfly
        if (wave == 0) {
            for (int k = lane; k < a.n_slabs; k += 64) gb += a.bias_slabs[(size_t)k * n_neg + q];
            gb = gs_wave_sum(gb);
        }
        __syncthreads();
        f32x4 g = zero4;
        if (tid < d4) {
            g = gpart[tid];
            for (int k = 1; k < SG; ++k) g += gpart[k * d4 + tid];
        }
        // + the rows of the batch2 slots that hold the same id, ascending
        for (int64_t base = 0; base < B; base += 256) {
            const int64_t s = base + tid;
            const unsigned long long m = __ballot(s < B && (int64_t)list[s] == v);
            if (lane == 0) masks[wave] = m;
            __syncthreads();
            for (int w = 0; w < 4; ++w) {
                unsigned long long mm = masks[w];
                while (mm) {
                    const int b = __ffsll((long long)mm) - 1;
                    mm &= mm - 1ull;
                    const int64_t sp2 = base + w * 64 + b;
                    if (tid < d4) g += *reinterpret_cast<const f32x4*>(a.g_ctx + sp2 * d + 4 * tid);
                    if (tid == 0) gb += a.g_bias[sp2];
                }
            }
            __syncthreads();
        }
        if (tid < d4) {
            f32x4* p = reinterpret_cast<f32x4*>(a.context + v * a.ldc + 4 * tid);
            *p = *p - g * a.lr;
        }
        if (tid == 0) a.bias[v] = a.bias[v] - a.lr * gb;
        return;
    }
    const int64_t s = (int64_t)(is_target ? blk - n_neg : blk - n_neg - a.pair_blocks) * 4 + wave;
    if (s >= B) return;
    const int64_t v = list[s];
    if (!is_target) {                                      // a negative's slot owns the row
        for (int base = 0; base < n_neg; base += 64)
            if (__ballot(base + lane < n_neg && (int64_t)list[B + base + lane] == v)) return;
    }
    const float* G = is_target ? a.g_target : a.g_ctx;
    float acc[DJ];
#pragma unroll
    for (int j = 0; j < DJ; ++j) acc[j] = 0.f;
    float gb = 0.f;
    bool owner = false;
    for (int64_t base = 0; base < B; base += 64) {
        unsigned long long mm = __ballot(base + lane < B && (int64_t)list[base + lane] == v);
        while (mm) {
            const int b = __ffsll((long long)mm) - 1;
            mm &= mm - 1ull;
            const int64_t sp = base + b;
            if (!owner) {
                if (sp != s) return;                       // an earlier slot holds this id (wave-uniform)
                owner = true;
            }
#pragma unroll
            for (int j = 0; j < DJ; ++j) acc[j] += G[sp * d + j * 64 + lane];
            if (!is_target) gb += a.g_bias[sp];
        }
    }
    float* row = is_target ? a.target + v * a.ldt : a.context + v * a.ldc;
#pragma unroll
    for (int j = 0; j < DJ; ++j) row[j * 64 + lane] = row[j * 64 + lane] - a.lr * acc[j];
    if (!is_target && lane == 0) a.bias[v] = a.bias[v] - a.lr * gb;
}

extern "C" int gs_n2v_apply(float* target, int64_t ldt, float* context, int64_t ldc, float* bias, int64_t n_rows,
                            const int32_t* ids, int64_t B, int32_t d, int32_t n_neg, float lr, const float* g_target,
                            const float* g_ctx, const float* g_bias, const float* neg_slabs, const float* bias_slabs,
                            int32_t n_slabs, const float* loss_rows, const float* rr_rows, float* loss_out, float* mrr_out,
                            uint64_t* c0, uint64_t d0, uint64_t* c1, uint64_t d1, void* stream) {
    GS_REQUIRE(target && context && bias && ids && g_target && g_ctx && g_bias && neg_slabs && bias_slabs && B > 0 && n_rows > 0,
               "gs_n2v_apply: bad args");
    GS_REQUIRE(B <= 0x3fffffffll && n_rows <= 0x7fffffffll, "gs_n2v_apply: B / table rows out of range");
    GS_REQUIRE(d == 64 || d == 128 || d == 256 || d == 512, "gs_n2v_apply: d must be 64/128/256/512 (got %d)", d);
    GS_REQUIRE(n_neg >= 1 && n_neg <= N2V_MAX_NEG, "gs_n2v_apply: n_neg must be in [1, %d] (got %d)", N2V_MAX_NEG, n_neg);
    GS_REQUIRE(ldt >= d && ldc >= d && ldt % 4 == 0 && ldc % 4 == 0 && gs_aligned16(context) && gs_aligned16(neg_slabs) &&
                   gs_aligned16(g_ctx), "gs_n2v_apply: tables and staging rows must be 16-byte aligned, ld %% 4 == 0");
    GS_REQUIRE(n_slabs == gs_n2v_slabs(B, d, n_neg), "gs_n2v_apply: n_slabs %d does not match the forward launch", n_slabs);
    GS_REQUIRE(!loss_rows || (loss_out && rr_rows && mrr_out), "gs_n2v_apply: loss_out / rr_rows / mrr_out missing");
    const bool has_epi = loss_rows || c0 || c1;
    const float inv_b = 1.0f / (float)B;
    const int32_t pair_blocks = (int32_t)gs_ceil_div(B, 4);
    const StepEpilogue epi = {loss_rows, B, inv_b, loss_out, 0, rr_rows, inv_b, mrr_out, c0, d0, c1, d1, nullptr, 0};
    const N2vApply a = {target, ldt, context, ldc, bias, ids, B, n_neg, n_slabs, lr, g_target, g_ctx, g_bias, neg_slabs,
                        bias_slabs, pair_blocks, epi};
    const unsigned blocks = (unsigned)(n_neg + 2 * pair_blocks + (has_epi ? 1 : 0));
    hipStream_t st = (hipStream_t)stream;
    if (d == 64) hipLaunchKernelGGL((n2v_apply_kernel<1>), dim3(blocks), dim3(256), 0, st, a);
    else if (d == 128) hipLaunchKernelGGL((n2v_apply_kernel<2>), dim3(blocks), dim3(256), 0, st, a);
    else if (d == 256) hipLaunchKernelGGL((n2v_apply_kernel<4>), dim3(blocks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((n2v_apply_kernel<8>), dim3(blocks), dim3(256), 0, st, a);
    GS_LAUNCH_CHECK("n2v_apply_kernel");
    return GS_OK;
}
