// N3: stand-alone root staging of the unsupervised objective (models.py:332-357); the head is gs_linkpred_loss.hip.
//   unsup_stage_kernel     edge-pair batch selection (minibatch.py:113-132 on the device) + the 20 negative samples
//                          of tf.nn.fixed_unigram_candidate_sampler(distortion=0.75, unique=False) (models.py:336-343)
#include "gs_sample_dev.h"


// ids_out = [batch1 (B) | batch2 (B) | negatives (n_neg)].  pairs: int32 [n_pairs, 2] (may be NULL: roots already
// staged by the host).  cdf: see gs_unigram_pick (gs_sample_dev.h) -- bit-exact vs oracle/sampler_hash.py.
__global__ __launch_bounds__(256) void unsup_stage_kernel(const int32_t* __restrict__ pairs, int64_t n_pairs,
                                                          const uint64_t* __restrict__ cursor, int64_t B,
                                                          const uint32_t* __restrict__ cdf, int64_t n_nodes, int32_t n_neg,
                                                          uint64_t seed, const uint64_t* __restrict__ clock,
                                                          int64_t slot_offset, int32_t* __restrict__ ids_out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pairs && t < B) {
        const uint64_t c = cursor ? *cursor : 0ull;
        ids_out[t] = gs_stage_pair(pairs, n_pairs, c, t, 0);
        ids_out[B + t] = gs_stage_pair(pairs, n_pairs, c, t, 1);
    }
    if (cdf && t < n_neg) {
        const uint32_t r = gs_unigram_draw32(seed, clock ? *clock : 0ull, (uint64_t)t + (uint64_t)slot_offset);
        ids_out[2 * B + t] = gs_unigram_pick(cdf, n_nodes, nullptr, 0, r);
    }
}

extern "C" int gs_unsup_stage(const int32_t* pairs, int64_t n_pairs, const uint64_t* cursor_dev, int64_t B,
                              const uint32_t* cdf, int64_t n_nodes, int32_t n_neg, uint64_t seed,
                              const uint64_t* clock_dev, int64_t slot_offset, int32_t* ids_out, void* stream) {
    GS_REQUIRE(ids_out && B >= 0 && n_neg >= 0, "gs_unsup_stage: bad args");
    GS_REQUIRE(!pairs || n_pairs > 0, "gs_unsup_stage: empty pair list");
    GS_REQUIRE(!cdf || n_nodes > 0, "gs_unsup_stage: empty cdf");
    const int64_t n = std::max<int64_t>(pairs ? B : 0, cdf ? n_neg : 0);
    if (n == 0) return GS_OK;
    hipLaunchKernelGGL(unsup_stage_kernel, dim3((unsigned)gs_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, pairs,
                       n_pairs, cursor_dev, B, cdf, n_nodes, n_neg, seed, clock_dev, slot_offset, ids_out);
    GS_LAUNCH_CHECK("unsup_stage_kernel");
    return GS_OK;
}
