// The link-prediction head (prediction.py:68-125, models.py:393-405): the ONE definition behind gs_linkpred_fwd_bwd,
// gs_linkpred_norm_fwd_bwd[_step] and gs_linkpred_loss_fwd_bwd[_step].
//   linkpred_loss_kernel     one wave per pair, four pairs per workgroup, the (normalised) negatives staged once per workgroup
//                            in LDS, with
//                              KIND  xent (:102-110) | skipgram (:112-117) | hinge (:119-125)
//                              NORM  true:  X = RAW aggregator outputs; the kernel normalises them (models.py:368-370), the
//                                           left operand is the normalised outputs1 and the gradient is carried back through
//                                           the normalisation:  dZ = inv * (g - y <g, y>)  (inv = rsqrt(max(sum z^2, 1e-12));
//                                           clamped rows: dZ = g * inv)
//                                    false: X = normalised rows, the left operand is a separate U [B, d] (bilinear weights:
//                                           U = l2_normalize(outputs1) . W, not unit-norm; or the rows [0, B) of X themselves);
//                                           the kernel returns dU and the gradient w.r.t. the normalised outputs2 / negatives
//   linkpred_loss_neg_kernel the negatives' gradient: per-workgroup slabs summed in a fixed order (no float atomics, bitwise
//                            reproducible), optionally through the normalisation; the step epilogue rides as one more block.
#include "gs_common.h"
#include "gs_linkpred_dev.h"

enum { LP_XENT = GS_LP_LOSS_XENT, LP_SKIPGRAM = GS_LP_LOSS_SKIPGRAM, LP_HINGE = GS_LP_LOSS_HINGE };

struct LpLossArgs {
    const float* X; int64_t ldx;       // [2B + n_neg, d]: rows [0,B) outputs1, [B,2B) outputs2, [2B, ..) negatives
    const float* U; int64_t ldu;       // [B, d] left operand (NORM == false)
    int64_t B; int32_t n_neg;
    float neg_w, margin, scale;
    float* Y; int64_t ldy;             // NORM: the normalised rows
    float* loss_rows; float* rr_rows; float* aff_all; int64_t ld_aff;
    float* dX; int64_t lddx;           // NORM: d/dZ of the 2B pair rows; else d/d(normalised outputs2) in rows [B, 2B)
    float* dU; int64_t lddu;           // NORM == false
    float* neg_slabs;                  // [gridDim.x][n_neg][d] w.r.t. the normalised negatives
};

// Per pair i (a = affinity, n_j = neg_cost, left = normalised outputs1 or U):
//   xent      loss = xent(1, a) + w sum_j xent(0, n_j);       dl/da = sig(a) - 1;          dl/dn_j = w sig(n_j)
//   skipgram  loss = a - log sum_j exp(n_j) (the reference's sign, row maximum subtracted);  dl/da = 1;  dl/dn_j = -softmax_j
//   hinge     loss = sum_j relu(n_j - (a - margin));  m_j = [n_j - (a - margin) > 0];  dl/da = -sum_j m_j;  dl/dn_j = m_j
//   rr = 1 / (1 + #{j : n_j >= a});   aff_all row = [n_0 .. n_{n_neg-1} | a]
// n_neg <= 128 (the LDS bound with d >= 64): two blocks of 64 affinities, lane q holds negatives q and 64 + q.
template <int DJ, int KIND, bool NORM>
__global__ __launch_bounds__(256) void linkpred_loss_kernel(const LpLossArgs a) {
    constexpr int d = DJ * 64;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int n_neg = a.n_neg;
    const int64_t B = a.B;
    float* negs = lds;                       // [n_neg][d]  normalised negative rows
    float* part = lds + (size_t)n_neg * d;   // [4 waves][n_neg][d] partial dneg (w.r.t. the normalised rows)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int q = wave; q < n_neg; q += 4) {
        float v[DJ], ss = 0.f;
#pragma unroll
        for (int j = 0; j < DJ; ++j) {
            v[j] = a.X[(2 * B + q) * a.ldx + j * 64 + lane];
            ss += v[j] * v[j];
        }
        float inv = 1.0f;
        if (NORM) inv = __builtin_amdgcn_rsqf(fmaxf(gs_wave_sum(ss), 1e-12f));
#pragma unroll
        for (int j = 0; j < DJ; ++j) {
            const float y = NORM ? v[j] * inv : v[j];
            negs[q * d + j * 64 + lane] = y;
            if (NORM && blockIdx.x == 0) a.Y[(2 * B + q) * a.ldy + j * 64 + lane] = y;
        }
    }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 4 + wave;
    const bool live = i < B;
    const int64_t ic = live ? i : 0;
    float o1[DJ], o2[DJ], g1[DJ];
    float inv1 = 1.0f, inv2 = 1.0f;
    if (NORM) {
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < DJ; ++j) {
            o1[j] = a.X[ic * a.ldx + j * 64 + lane];
            o2[j] = a.X[(B + ic) * a.ldx + j * 64 + lane];
            s1 += o1[j] * o1[j];
            s2 += o2[j] * o2[j];
        }
        inv1 = __builtin_amdgcn_rsqf(fmaxf(gs_wave_sum(s1), 1e-12f));
        inv2 = __builtin_amdgcn_rsqf(fmaxf(gs_wave_sum(s2), 1e-12f));
#pragma unroll
        for (int j = 0; j < DJ; ++j) {
            o1[j] *= inv1;
            o2[j] *= inv2;
        }
    } else {
#pragma unroll
        for (int j = 0; j < DJ; ++j) {
            o1[j] = a.U[ic * a.ldu + j * 64 + lane];
            o2[j] = a.X[(B + ic) * a.ldx + j * 64 + lane];
        }
    }
    float aff = 0.f;
#pragma unroll
    for (int j = 0; j < DJ; ++j) aff += o1[j] * o2[j];
    aff = gs_wave_sum(aff);

    const int nq0 = min(64, n_neg), nq1 = max(0, n_neg - 64);
    float nav[2];
    nav[0] = lp_neg_affinities<DJ>(o1, negs, 0, nq0, lane);
    nav[1] = nq1 > 0 ? lp_neg_affinities<DJ>(o1, negs, 64, nq1, lane) : 0.f;
    const bool in[2] = {lane < nq0, lane < nq1};
    const int rank = __popcll(__ballot(in[0] && nav[0] >= aff)) + __popcll(__ballot(in[1] && nav[1] >= aff));
    float gq[2], da, loss;
    if (KIND == LP_XENT) {
        float sa, lga;
        gs_sigmoid_lg(aff, sa, lga);
        da = (sa - 1.0f) * a.scale;
        loss = fmaxf(aff, 0.f) - aff + lga;
        float ln = 0.f;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            float sg, lg;
            gs_sigmoid_lg(nav[b], sg, lg);
            ln += in[b] ? fmaxf(nav[b], 0.f) + lg : 0.f;
            gq[b] = in[b] ? a.neg_w * a.scale * sg : 0.f;
        }
        loss += a.neg_w * gs_wave_sum(ln);
    } else if (KIND == LP_SKIPGRAM) {
        const float mx = gs_wave_max(fmaxf(in[0] ? nav[0] : -INFINITY, in[1] ? nav[1] : -INFINITY));
        const float e0 = in[0] ? __expf(nav[0] - mx) : 0.f, e1 = in[1] ? __expf(nav[1] - mx) : 0.f;
        const float S = gs_wave_sum(e0 + e1);                             // >= 1: the maximum's own term
        const float rS = 1.0f / S;
        loss = aff - (mx + __logf(S));
        da = a.scale;
        gq[0] = -a.scale * e0 * rS;
        gq[1] = -a.scale * e1 * rS;
    } else {
        const float thr = aff - a.margin;                             // tf.subtract(neg_aff, aff - margin), relu'(0) = 0
        const float t0 = nav[0] - thr, t1 = nav[1] - thr;
        const bool m0 = in[0] && t0 > 0.f, m1 = in[1] && t1 > 0.f;
        loss = gs_wave_sum((m0 ? t0 : 0.f) + (m1 ? t1 : 0.f));
        da = -a.scale * (float)(__popcll(__ballot(m0)) + __popcll(__ballot(m1)));
        gq[0] = m0 ? a.scale : 0.f;
        gq[1] = m1 ? a.scale : 0.f;
    }
    if (!live) gq[0] = gq[1] = 0.f;                                    // a dead wave still clears its part of the slab
    float* aff_row = (a.aff_all && live) ? a.aff_all + i * a.ld_aff : nullptr;
    if (aff_row) {
        if (in[0]) aff_row[lane] = nav[0];
        if (in[1]) aff_row[64 + lane] = nav[1];
    }
#pragma unroll
    for (int j = 0; j < DJ; ++j) g1[j] = da * o2[j];
    float* mypart = part + (size_t)wave * n_neg * d;
    //   g1 += sum_q gq * neg_q;   mypart[q] = gq * left   (the negatives' gradient contribution of this pair)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int nq = b == 0 ? nq0 : nq1;
        for (int q = 0; q < nq; ++q) {
            const float g = __shfl(gq[b], q, 64);
            const float* nr = negs + (size_t)(b * 64 + q) * d + lane;
            float* mp = mypart + (size_t)(b * 64 + q) * d + lane;
#pragma unroll
            for (int j = 0; j < DJ; ++j) {
                g1[j] += g * nr[j * 64];
                mp[j * 64] = g * o1[j];
            }
        }
    }
    if (live) {
        if (NORM) {
            // back through y = z * inv:  dz = inv (g - y <g, y>);  clamped (sum z^2 < 1e-12, inv = 1e6): dz = g * inv
            float dot1 = 0.f, dot2 = 0.f;
#pragma unroll
            for (int j = 0; j < DJ; ++j) {
                dot1 += g1[j] * o1[j];
                dot2 += da * o1[j] * o2[j];
            }
            dot1 = gs_wave_sum(dot1);
            dot2 = gs_wave_sum(dot2);
            const bool c1 = inv1 >= 1.0e6f, c2 = inv2 >= 1.0e6f;
#pragma unroll
            for (int j = 0; j < DJ; ++j) {
                const float ga = g1[j], gb = da * o1[j];
                a.Y[i * a.ldy + j * 64 + lane] = o1[j];
                a.Y[(B + i) * a.ldy + j * 64 + lane] = o2[j];
                a.dX[i * a.lddx + j * 64 + lane] = c1 ? ga * inv1 : inv1 * (ga - o1[j] * dot1);
                a.dX[(B + i) * a.lddx + j * 64 + lane] = c2 ? gb * inv2 : inv2 * (gb - o2[j] * dot2);
            }
        } else {
#pragma unroll
            for (int j = 0; j < DJ; ++j) {
                a.dU[i * a.lddu + j * 64 + lane] = g1[j];
                a.dX[(B + i) * a.lddx + j * 64 + lane] = da * o1[j];
            }
        }
        if (lane == 0) {
            a.loss_rows[i] = loss;
            a.rr_rows[i] = 1.0f / (float)(rank + 1);
            if (a.aff_all) a.aff_all[i * a.ld_aff + n_neg] = aff;
        }
    }
    __syncthreads();
    float* slab = a.neg_slabs + (size_t)blockIdx.x * n_neg * d;
    for (int t = tid; t < n_neg * d; t += 256)
        slab[t] = (part[t] + part[(size_t)n_neg * d + t]) + (part[2 * (size_t)n_neg * d + t] + part[3 * (size_t)n_neg * d + t]);
}

// One workgroup per negative row q: g = sum of the n_slabs per-workgroup slabs in a fixed order.  The row's d/4 float4 columns
// x SG = 1024/d slab groups are spread over the 256 threads; a group walks its slabs (sg, sg + SG, ...) with 16 independent
// 16-byte loads in flight (the first version: 8 dword loads per batch, 16 dependent round trips for 128 slabs -- 8 us of pure
// latency), the groups meet in LDS and are summed group 0, 1, ...  through_norm: X holds the RAW row and g goes back through
// its normalisation (the row's own inv recomputed from X); otherwise the row of dX is g itself.  Block n_neg (when has_epi) is
// the step epilogue (mean loss / mrr + device counters): it only needs the rows the previous launch wrote.
__global__ __launch_bounds__(256) void linkpred_loss_neg_kernel(const float* __restrict__ slabs, int32_t n_slabs, int32_t n_neg,
                                                                int32_t d, const float* __restrict__ X, int64_t ldx,
                                                                int64_t row0, float* __restrict__ dX, int64_t lddx,
                                                                int through_norm, const StepEpilogue epi) {
    __shared__ f32x4 gpart[256];
    __shared__ float red[2][4];
    if ((int)blockIdx.x == n_neg) {
        gs_step_epilogue_block(epi, red[0], red[1]);
        return;
    }
    const int q = blockIdx.x, tid = threadIdx.x;
    const int d4 = d >> 2, SG = 256 / d4;                  // d in {64, 128, 256, 512}: d4 in {16 .. 128}, SG in {16 .. 2}
    const int cg = tid % d4, sg = tid / d4;
    const f32x4* sp = reinterpret_cast<const f32x4*>(slabs + (size_t)q * d) + cg;
    const size_t stride4 = (size_t)n_neg * d4;             // float4 per slab
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[4] = {zero4, zero4, zero4, zero4};
    int sI = sg;
    for (; sI + 15 * SG < n_slabs; sI += 16 * SG) {
        f32x4 v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = sp[(size_t)(sI + u * SG) * stride4];
#pragma unroll
        for (int u = 0; u < 16; ++u) acc[u & 3] += v[u];
    }
    for (; sI < n_slabs; sI += SG) acc[0] += sp[(size_t)sI * stride4];
    gpart[tid] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    __syncthreads();
    f32x4 g = zero4, z = zero4;
    if (tid < d4) {
        g = gpart[tid];
        for (int k = 1; k < SG; ++k) g += gpart[k * d4 + tid];
    }
    if (!through_norm) {                                   // launch-uniform
        if (tid < d4) *reinterpret_cast<f32x4*>(dX + (row0 + q) * lddx + 4 * tid) = g;
        return;
    }
    float ss = 0.f;
    if (tid < d4) {
        z = *reinterpret_cast<const f32x4*>(X + (row0 + q) * ldx + 4 * tid);
        ss = (z.x * z.x + z.y * z.y) + (z.z * z.z + z.w * z.w);
    }
    ss = gs_wave_sum(ss);
    if ((tid & 63) == 0) red[0][tid >> 6] = ss;
    __syncthreads();
    ss = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    const float inv = __builtin_amdgcn_rsqf(fmaxf(ss, 1e-12f));
    float dot = ((g.x * z.x + g.y * z.y) + (g.z * z.z + g.w * z.w)) * inv;
    dot = gs_wave_sum(dot);
    if ((tid & 63) == 0) red[1][tid >> 6] = dot;
    __syncthreads();
    dot = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    const bool clamped = inv >= 1.0e6f;
    if (tid < d4) {
        const f32x4 o = clamped ? g * inv : (g - z * (inv * dot)) * inv;
        *reinterpret_cast<f32x4*>(dX + (row0 + q) * lddx + 4 * tid) = o;
    }
}

template <int DJ, int KIND, bool NORM>
static int lp_loss_launch_one(const LpLossArgs& a, int64_t blocks, size_t lds_bytes, hipStream_t st) {
    GS_LDS_ATTR(160 * 1024, linkpred_loss_kernel<DJ, KIND, NORM>);
    hipLaunchKernelGGL((linkpred_loss_kernel<DJ, KIND, NORM>), dim3((unsigned)blocks), dim3(256), lds_bytes, st, a);
    return GS_OK;
}

template <int KIND, bool NORM>
static int lp_loss_launch_d(const LpLossArgs& a, int32_t d, int64_t blocks, size_t lds_bytes, hipStream_t st) {
    if (d == 64) return lp_loss_launch_one<1, KIND, NORM>(a, blocks, lds_bytes, st);
    if (d == 128) return lp_loss_launch_one<2, KIND, NORM>(a, blocks, lds_bytes, st);
    if (d == 256) return lp_loss_launch_one<4, KIND, NORM>(a, blocks, lds_bytes, st);
    return lp_loss_launch_one<8, KIND, NORM>(a, blocks, lds_bytes, st);
}

template <bool NORM>
static int lp_loss_launch_kind(int32_t kind, const LpLossArgs& a, int32_t d, int64_t blocks, size_t lds_bytes, hipStream_t st) {
    if (kind == LP_XENT) return lp_loss_launch_d<LP_XENT, NORM>(a, d, blocks, lds_bytes, st);
    if (kind == LP_SKIPGRAM) return lp_loss_launch_d<LP_SKIPGRAM, NORM>(a, d, blocks, lds_bytes, st);
    return lp_loss_launch_d<LP_HINGE, NORM>(a, d, blocks, lds_bytes, st);
}

// `who`: the entry point's name for its error messages.  n_slabs_out != nullptr: the first launch only -- the slabs are left
// for the caller's gs_reduce_slabs and their count is returned (gs_linkpred_fwd_bwd).
static int linkpred_loss_launch(const char* who, int32_t loss_kind, const float* X, int64_t ldx, const float* U, int64_t ldu,
                                int64_t B, int32_t d, int32_t n_neg, float neg_weight, float margin, float scale, float* Y,
                                int64_t ldy, float* loss_rows, float* rr_rows, float* aff_all, int64_t ld_aff, float* dX,
                                int64_t lddx, float* dU, int64_t lddu, float* neg_slabs, const StepEpilogue* epi,
                                int32_t* n_slabs_out, void* stream) {
    GS_REQUIRE(loss_kind == LP_XENT || loss_kind == LP_SKIPGRAM || loss_kind == LP_HINGE, "%s: unknown loss kind %d", who, loss_kind);
    GS_REQUIRE(X && loss_rows && rr_rows && dX && neg_slabs && B > 0 && n_neg > 0, "%s: bad args", who);
    GS_REQUIRE(d == 64 || d == 128 || d == 256 || d == 512, "%s: d must be 64/128/256/512 (got %d)", who, d);
    const bool norm = U == nullptr;
    GS_REQUIRE(norm ? (Y != nullptr && ldy >= d) : (dU != nullptr && ldu >= d && lddu >= d), "%s: %s", who,
               norm ? "Y missing or ldy too small" : "dU missing or ldu / lddu too small");
    GS_REQUIRE(ldx >= d && lddx >= d && (!aff_all || ld_aff >= n_neg + 1), "%s: ld too small", who);
    const size_t lds_bytes = (size_t)5 * n_neg * d * sizeof(float);
    GS_REQUIRE(lds_bytes <= 160 * 1024, "%s: %d negatives x d=%d do not fit LDS", who, n_neg, d);
    // the second launch moves whole float4: 16-byte rows
    GS_REQUIRE(n_slabs_out || (ldx % 4 == 0 && lddx % 4 == 0 && gs_aligned16(X) && gs_aligned16(dX) && gs_aligned16(neg_slabs)),
               "%s: X / dX / neg_slabs must be 16-byte aligned with ld %% 4 == 0", who);
    const int64_t blocks = gs_ceil_div(B, 4);
    hipStream_t st = (hipStream_t)stream;
    const LpLossArgs a = {X, ldx, U, ldu, B, n_neg, neg_weight, margin, scale, Y, ldy, loss_rows, rr_rows, aff_all, ld_aff,
                          dX, lddx, dU, lddu, neg_slabs};
    const int rc = norm ? lp_loss_launch_kind<true>(loss_kind, a, d, blocks, lds_bytes, st)
                        : lp_loss_launch_kind<false>(loss_kind, a, d, blocks, lds_bytes, st);
    if (rc != GS_OK) return rc;
    GS_LAUNCH_CHECK("linkpred_loss_kernel");
    if (n_slabs_out) {
        *n_slabs_out = (int32_t)blocks;
        return GS_OK;
    }
    const StepEpilogue none = {};
    hipLaunchKernelGGL(linkpred_loss_neg_kernel, dim3((unsigned)(n_neg + (epi ? 1 : 0))), dim3(256), 0, st, neg_slabs,
                       (int32_t)blocks, n_neg, d, X, ldx, 2 * B, dX, lddx, norm ? 1 : 0, epi ? *epi : none);
    GS_LAUNCH_CHECK("linkpred_loss_neg_kernel");
    return GS_OK;
}

static StepEpilogue lp_step_epilogue(int64_t B, float* loss_rows, float* rr_rows, float* loss_out, int accumulate, float* mrr_out,
                                     uint64_t* c0, uint64_t d0, uint64_t* c1, uint64_t d1, uint64_t* c2, uint64_t d2) {
    const float inv_b = B > 0 ? 1.0f / (float)B : 0.f;
    return {loss_rows, B, inv_b, loss_out, accumulate, rr_rows, inv_b, mrr_out, c0, d0, c1, d1, c2, d2};
}

extern "C" int gs_linkpred_loss_fwd_bwd(int32_t loss_kind, const float* X, int64_t ldx, const float* U, int64_t ldu, int64_t B,
                                        int32_t d, int32_t n_neg, float neg_weight, float margin, float scale, float* Y,
                                        int64_t ldy, float* loss_rows, float* rr_rows, float* aff_all, int64_t ld_aff,
                                        float* dX, int64_t lddx, float* dU, int64_t lddu, float* neg_slabs, void* stream) {
    return linkpred_loss_launch("gs_linkpred_loss_fwd_bwd", loss_kind, X, ldx, U, ldu, B, d, n_neg, neg_weight, margin, scale, Y,
                                ldy, loss_rows, rr_rows, aff_all, ld_aff, dX, lddx, dU, lddu, neg_slabs, nullptr, nullptr, stream);
}

extern "C" int gs_linkpred_loss_fwd_bwd_step(int32_t loss_kind, const float* X, int64_t ldx, const float* U, int64_t ldu,
                                             int64_t B, int32_t d, int32_t n_neg, float neg_weight, float margin, float scale,
                                             float* Y, int64_t ldy, float* loss_rows, float* rr_rows, float* aff_all,
                                             int64_t ld_aff, float* dX, int64_t lddx, float* dU, int64_t lddu, float* neg_slabs,
                                             float* loss_out, int accumulate, float* mrr_out, uint64_t* c0, uint64_t d0,
                                             uint64_t* c1, uint64_t d1, uint64_t* c2, uint64_t d2, void* stream) {
    GS_REQUIRE(loss_out && mrr_out, "gs_linkpred_loss_fwd_bwd_step: loss_out / mrr_out missing");
    const StepEpilogue epi = lp_step_epilogue(B, loss_rows, rr_rows, loss_out, accumulate, mrr_out, c0, d0, c1, d1, c2, d2);
    return linkpred_loss_launch("gs_linkpred_loss_fwd_bwd", loss_kind, X, ldx, U, ldu, B, d, n_neg, neg_weight, margin, scale, Y,
                                ldy, loss_rows, rr_rows, aff_all, ld_aff, dX, lddx, dU, lddu, neg_slabs, &epi, nullptr, stream);
}

// ---- the xent head's older entry points: the same kernels ----
// Rows of Y already normalised: the gradient of the pair rows into dY, the negatives' slabs left for gs_reduce_slabs.
extern "C" int gs_linkpred_fwd_bwd(const float* Y, int64_t ldy, int64_t B, int32_t d, int32_t n_neg, float neg_weight,
                                   float scale, float* loss_rows, float* rr_rows, float* aff_all, int64_t ld_aff,
                                   float* dY, int64_t lddy, float* neg_slabs, int32_t* n_slabs_out, void* stream) {
    int32_t n_slabs = 0;
    const int rc = linkpred_loss_launch("gs_linkpred_fwd_bwd", LP_XENT, Y, ldy, Y, ldy, B, d, n_neg, neg_weight, 0.f, scale, nullptr,
                                        0, loss_rows, rr_rows, aff_all, ld_aff, dY, lddy, dY, lddy, neg_slabs, nullptr, &n_slabs,
                                        stream);
    if (rc == GS_OK && n_slabs_out) *n_slabs_out = n_slabs;
    return rc;
}

// RAW rows Z: Y = l2_normalize(Z), the gradient back through the normalisation into dZ, negatives' rows included.
extern "C" int gs_linkpred_norm_fwd_bwd(const float* Z, int64_t ldz, int64_t B, int32_t d, int32_t n_neg, float neg_weight,
                                        float scale, float* Y, int64_t ldy, float* loss_rows, float* rr_rows, float* aff_all,
                                        int64_t ld_aff, float* dZ, int64_t lddz, float* neg_slabs, void* stream) {
    return linkpred_loss_launch("gs_linkpred_norm_fwd_bwd", LP_XENT, Z, ldz, nullptr, 0, B, d, n_neg, neg_weight, 0.f, scale, Y, ldy,
                                loss_rows, rr_rows, aff_all, ld_aff, dZ, lddz, nullptr, 0, neg_slabs, nullptr, nullptr, stream);
}

extern "C" int gs_linkpred_norm_fwd_bwd_step(const float* Z, int64_t ldz, int64_t B, int32_t d, int32_t n_neg, float neg_weight,
                                             float scale, float* Y, int64_t ldy, float* loss_rows, float* rr_rows,
                                             float* aff_all, int64_t ld_aff, float* dZ, int64_t lddz, float* neg_slabs,
                                             float* loss_out, int accumulate, float* mrr_out, uint64_t* c0, uint64_t d0,
                                             uint64_t* c1, uint64_t d1, uint64_t* c2, uint64_t d2, void* stream) {
    GS_REQUIRE(loss_out && mrr_out, "gs_linkpred_norm_fwd_bwd_step: loss_out / mrr_out missing");
    const StepEpilogue epi = lp_step_epilogue(B, loss_rows, rr_rows, loss_out, accumulate, mrr_out, c0, d0, c1, d1, c2, d2);
    return linkpred_loss_launch("gs_linkpred_norm_fwd_bwd", LP_XENT, Z, ldz, nullptr, 0, B, d, n_neg, neg_weight, 0.f, scale, Y, ldy,
                                loss_rows, rr_rows, aff_all, ld_aff, dZ, lddz, nullptr, 0, neg_slabs, &epi, nullptr, stream);
}
