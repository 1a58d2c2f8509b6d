// Device pieces shared by the link-prediction head (gs_linkpred_loss.hip) and the node2vec step (gs_n2v.hip); the sigmoid
// pieces also serve the fused unsupervised tail (gs_unsup_tail.hip).
#pragma once
#include "gs_common.h"

// sg = sigmoid(x) and lg = log(1 + exp(-|x|)) from ONE round of v_exp / v_rcp / v_log (__expf / __logf: ~1e-6 relative):
//   softplus(x) = xent(0, x) = fmaxf(x, 0) + lg;   softplus(-x) = xent(1, x) = fmaxf(x, 0) - x + lg
__device__ __forceinline__ void gs_sigmoid_lg(const float x, float& sg, float& lg) {
    const float e = __expf(-fabsf(x));
    const float r = __builtin_amdgcn_rcpf(1.0f + e);
    sg = x >= 0.f ? r : e * r;
    lg = __logf(1.0f + e);
}

// Affinities of the wave's left row o1 (one 64-column group per register) against the rows negs[qb .. qb + nq) of an LDS
// image [n][d] (nq <= 64, wave-uniform): lane q returns row qb + q's (lanes >= nq return 0).  Four independent dot
// products / reductions in flight, so that the sigmoid / softplus of the whole block is then ONE round of v_exp / v_log /
// v_rcp (the first version walked the negatives one by one with libm expf / log1pf: 21 us for 512 pairs x 20 negatives).
template <int DJ>
__device__ __forceinline__ float lp_neg_affinities(const float (&o1)[DJ], const float* __restrict__ negs, const int qb,
                                                   const int nq, const int lane) {
    constexpr int d = DJ * 64;
    float nav = 0.f;
    int q = 0;
    for (; q + 4 <= nq; q += 4) {
        float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
        const float* nr = negs + (size_t)(qb + q) * d + lane;
#pragma unroll
        for (int j = 0; j < DJ; ++j) {
            p0 += o1[j] * nr[j * 64];
            p1 += o1[j] * nr[d + j * 64];
            p2 += o1[j] * nr[2 * d + j * 64];
            p3 += o1[j] * nr[3 * d + j * 64];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            p0 += __shfl_xor(p0, off, 64);
            p1 += __shfl_xor(p1, off, 64);
            p2 += __shfl_xor(p2, off, 64);
            p3 += __shfl_xor(p3, off, 64);
        }
        nav = lane == q ? p0 : nav;
        nav = lane == q + 1 ? p1 : nav;
        nav = lane == q + 2 ? p2 : nav;
        nav = lane == q + 3 ? p3 : nav;
    }
    for (; q < nq; ++q) {
        float p0 = 0.f;
#pragma unroll
        for (int j = 0; j < DJ; ++j) p0 += o1[j] * negs[(size_t)(qb + q) * d + j * 64 + lane];
        p0 = gs_wave_sum(p0);
        nav = lane == q ? p0 : nav;
    }
    return nav;
}
