// Attention pooling over the s sampled neighbors of a node (the graphsage_attn aggregator, DESIGN "Attention pooling"):
//
//   t_j = <V_j, a>;   alpha = softmax_j(t_j);   pooled = sum_j alpha_j V_j          V_j = H[inv[i*s + j]]  (inv NULL: H[i*s + j])
//
// V is the output of the aggregator's relu-Dense, so V > 0 is the Dense's relu mask.  The gate does not depend on the node that
// asks: H may hold one row per DISTINCT sampled id, read through `inv`.
//
// Forward: ONE WAVE per group, lanes own columns (lane l holds the float4 at columns (k * 64 + l) * 4, k < CH), one pass over the
// s rows with a running maximum, running sum and rescaled accumulator (online softmax); the dot product is a butterfly wave
// reduction, so every lane holds the same score; the next row's loads are in flight while the current row is folded in.  Each H
// row is read once.  The scores stay in registers (lane j & 63 keeps t_j) and leave as alpha [n, s] for the backward pass.
//
// Backward, given dP = d_pooled:   g_j = <dP_i, V_j>;  G = sum_j alpha_j g_j;  dt_j = alpha_j (g_j - G)
//                                  dV_j = (alpha_j dP_i + dt_j a) * (V_j > 0);  da = sum_{i,j} dt_j V_j
// one wave per group again, two passes over its rows (g_j, then dV_j and da; the second pass hits in the cache).  Every wave keeps
// its da in registers across the groups it walks (group = block * W + wave, stride W * blocks; W = 16 waves up to 512 columns, 8
// beyond), the waves of a workgroup are added in wave order through LDS and workgroup b writes slab b: [n_slabs, hidden] partial
// sums that the optimizer launch adds in slab order, as it adds the weight gradients' slabs.  No [n*s, hidden] temporary, no
// atomics, a fixed order of every addition.
//
// gs_attn_scores writes <H_r, a> into column `hidden` of every row of H (ld >= hidden + 4): the logit column that
// gs_csr_reduce_fwd / gs_csr_reduce_rows read for GS_CSR_SOFTMAX.
#include "gs_common.h"

#define GS_ATTN_MAX_S 128
#define GS_ATTN_MAX_HIDDEN 1024

__device__ __forceinline__ float attn_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float attn_lane(const float v, const int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

template <int CH>
__device__ __forceinline__ void attn_load(f32x4 (&v)[CH], const float* __restrict__ row, const int lane, const int hidden) {
#pragma unroll
    for (int k = 0; k < CH; ++k) {
        const int col = (k * 64 + lane) * 4;
        v[k] = col < hidden ? *reinterpret_cast<const f32x4*>(row + col) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

template <int CH>
__device__ __forceinline__ float attn_dot(const f32x4 (&x)[CH], const f32x4 (&y)[CH]) {
    float p = 0.f;
#pragma unroll
    for (int k = 0; k < CH; ++k) p += x[k].x * y[k].x + x[k].y * y[k].y + x[k].z * y[k].z + x[k].w * y[k].w;
    return attn_wave_sum(p);
}

// the group's row ids, lane l holding those of samples l and l + 64 (inv NULL: consecutive rows)
__device__ __forceinline__ void attn_ids(const int32_t* __restrict__ inv, const int64_t i, const int s, const int lane,
                                         int32_t& lo, int32_t& hi) {
    lo = hi = 0;
    if (inv) {
        if (lane < s) lo = inv[i * s + lane];
        if (lane + 64 < s) hi = inv[i * s + lane + 64];
    }
}

__device__ __forceinline__ int64_t attn_row(const int32_t* inv, const int64_t i, const int s, const int j, const int32_t lo,
                                            const int32_t hi) {
    if (!inv) return i * s + j;
    return (int64_t)__builtin_amdgcn_readlane(j < 64 ? lo : hi, j & 63);
}

template <int CH>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const float* __restrict__ H, const int64_t ldh,
                                                       const int32_t* __restrict__ inv, const float* __restrict__ a,
                                                       const int64_t n, const int s, const int hidden,
                                                       float* __restrict__ pooled, const int64_t ldp, float* __restrict__ alpha) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;                                      // wave-uniform
    f32x4 av[CH], acc[CH], v[CH], vn[CH];
    attn_load<CH>(av, a, lane, hidden);
#pragma unroll
    for (int k = 0; k < CH; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    int32_t id_lo, id_hi;
    attn_ids(inv, i, s, lane, id_lo, id_hi);
    float m = -__builtin_inff(), l = 0.f, t_lo = 0.f, t_hi = 0.f;
    attn_load<CH>(vn, H + attn_row(inv, i, s, 0, id_lo, id_hi) * ldh, lane, hidden);
    for (int j = 0; j < s; ++j) {
#pragma unroll
        for (int k = 0; k < CH; ++k) v[k] = vn[k];
        if (j + 1 < s) attn_load<CH>(vn, H + attn_row(inv, i, s, j + 1, id_lo, id_hi) * ldh, lane, hidden);
        const float t = attn_dot<CH>(v, av);
        const float m_new = fmaxf(m, t);
        const float sc = expf(m - m_new);                    // 0 at the first row (m = -inf)
        const float w = expf(t - m_new);
        l = l * sc + w;
#pragma unroll
        for (int k = 0; k < CH; ++k) acc[k] = acc[k] * sc + v[k] * w;
        m = m_new;
        if ((j & 63) == lane) {
            if (j < 64) t_lo = t; else t_hi = t;
        }
    }
    const float inv_l = 1.0f / l;
#pragma unroll
    for (int k = 0; k < CH; ++k) {
        const int col = (k * 64 + lane) * 4;
        if (col < hidden) *reinterpret_cast<f32x4*>(pooled + i * ldp + col) = acc[k] * inv_l;
    }
    if (lane < s) alpha[i * s + lane] = expf(t_lo - m) * inv_l;
    if (lane + 64 < s) alpha[i * s + lane + 64] = expf(t_hi - m) * inv_l;
}

// WAVES waves per workgroup, U rows of a group in flight per wave (the loads of a batch are issued before the first is used:
// the wave reductions of a row depend on its loads, and one row at a time leaves the launch waiting on memory latency)
template <int CH, int WAVES, int U>
__global__ __launch_bounds__(64 * WAVES) void attn_bwd_kernel(
    const float* __restrict__ dP, const int64_t ldd, const float* __restrict__ H, const int64_t ldh,
    const int32_t* __restrict__ inv, const float* __restrict__ a, const float* __restrict__ alpha, const int64_t n, const int s,
    const int hidden, float* __restrict__ dV, const int64_t ldv, float* __restrict__ da_slabs) {
    __shared__ float red[WAVES][CH * 256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    f32x4 av[CH], da[CH], dp[CH], v[U][CH];
    attn_load<CH>(av, a, lane, hidden);
#pragma unroll
    for (int k = 0; k < CH; ++k) da[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int64_t i = (int64_t)blockIdx.x * WAVES + wave; i < n; i += (int64_t)gridDim.x * WAVES) {
        attn_load<CH>(dp, dP + i * ldd, lane, hidden);
        int32_t id_lo, id_hi;
        attn_ids(inv, i, s, lane, id_lo, id_hi);
        const float al_lo = lane < s ? alpha[i * s + lane] : 0.f;
        const float al_hi = lane + 64 < s ? alpha[i * s + lane + 64] : 0.f;
        float g_lo = 0.f, g_hi = 0.f;
        for (int j0 = 0; j0 < s; j0 += U) {
#pragma unroll
            for (int u = 0; u < U; ++u)          // the surplus rows of the last batch re-load row s - 1 and are dropped
                attn_load<CH>(v[u], H + attn_row(inv, i, s, min(j0 + u, s - 1), id_lo, id_hi) * ldh, lane, hidden);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int j = j0 + u;
                const float g = attn_dot<CH>(dp, v[u]);
                if (j < s && (j & 63) == lane) {
                    if (j < 64) g_lo = g; else g_hi = g;
                }
            }
        }
        const float G = attn_wave_sum(al_lo * g_lo + al_hi * g_hi);
        const float dt_lo = al_lo * (g_lo - G), dt_hi = al_hi * (g_hi - G);
        for (int j0 = 0; j0 < s; j0 += U) {
#pragma unroll
            for (int u = 0; u < U; ++u)
                attn_load<CH>(v[u], H + attn_row(inv, i, s, min(j0 + u, s - 1), id_lo, id_hi) * ldh, lane, hidden);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int j = j0 + u;
                if (j < s) {                     // wave-uniform
                    const float aj = attn_lane(j < 64 ? al_lo : al_hi, j & 63);
                    const float dt = attn_lane(j < 64 ? dt_lo : dt_hi, j & 63);
                    float* __restrict__ out = dV + (i * s + j) * ldv;
#pragma unroll
                    for (int k = 0; k < CH; ++k) {
                        const int col = (k * 64 + lane) * 4;
                        const f32x4 x = v[u][k];
                        const f32x4 d = dp[k] * aj + av[k] * dt;
                        const f32x4 r = {x.x > 0.f ? d.x : 0.f, x.y > 0.f ? d.y : 0.f, x.z > 0.f ? d.z : 0.f, x.w > 0.f ? d.w : 0.f};
                        if (col < hidden) *reinterpret_cast<f32x4*>(out + col) = r;
                        da[k] += x * dt;
                    }
                }
            }
        }
    }
    // the workgroup's waves in wave order, then slab blockIdx.x
#pragma unroll
    for (int k = 0; k < CH; ++k) *reinterpret_cast<f32x4*>(&red[wave][(k * 64 + lane) * 4]) = da[k];
    __syncthreads();
    for (int c = threadIdx.x; c < hidden; c += 64 * WAVES) {
        float sum = red[0][c];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) sum += red[w][c];
        da_slabs[(int64_t)blockIdx.x * hidden + c] = sum;
    }
}

// one wave per row: H[r, hidden] = <H[r, :hidden], a>
template <int CH>
__global__ __launch_bounds__(256) void attn_scores_kernel(float* __restrict__ H, const int64_t ldh, const int64_t rows,
                                                          const int hidden, const float* __restrict__ a) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;                                   // wave-uniform
    f32x4 av[CH], v[CH];
    attn_load<CH>(av, a, lane, hidden);
    attn_load<CH>(v, H + r * ldh, lane, hidden);
    const float t = attn_dot<CH>(v, av);
    if (lane == 0) H[r * ldh + hidden] = t;
}

static int attn_supported(int32_t s, int32_t hidden, const char* who) {
    if (s < 1 || s > GS_ATTN_MAX_S || hidden < 4 || hidden % 4 || hidden > GS_ATTN_MAX_HIDDEN) {
        gs_set_error("%s: needs 1 <= s <= %d, hidden %% 4 == 0, 4 <= hidden <= %d (s=%d, hidden=%d)", who, GS_ATTN_MAX_S,
                     GS_ATTN_MAX_HIDDEN, s, hidden);
        return GS_ENOTSUP;
    }
    return GS_OK;
}

#define GS_ATTN_DISPATCH(hidden, LAUNCH) \
    do {                                 \
        if ((hidden) <= 256) {           \
            LAUNCH(1);                   \
        } else if ((hidden) <= 512) {    \
            LAUNCH(2);                   \
        } else {                         \
            LAUNCH(4);                   \
        }                                \
    } while (0)

extern "C" int gs_segment_attn_fwd(const float* H, int64_t ldh, const int32_t* inv, const float* a, int64_t n, int32_t s,
                                   int32_t hidden, float* pooled, int64_t ldp, float* alpha, void* stream) {
    const int rc = attn_supported(s, hidden, "gs_segment_attn_fwd");
    if (rc != GS_OK) return rc;
    if (n == 0) return GS_OK;
    GS_CHECK_MAT(H, ldh, "gs_segment_attn_fwd H");
    GS_CHECK_MAT(pooled, ldp, "gs_segment_attn_fwd pooled");
    GS_REQUIRE(a && gs_aligned16(a) && alpha && n > 0 && ldh >= hidden && ldp >= hidden, "gs_segment_attn_fwd: bad args");
    const int64_t blocks = gs_ceil_div(n, 4);
    GS_REQUIRE(blocks < (1ll << 31) && n * (int64_t)s < (1ll << 40), "gs_segment_attn_fwd: grid too large");
#define LAUNCH(CH)                                                                                                            \
    hipLaunchKernelGGL(attn_fwd_kernel<CH>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, H, ldh, inv, a, n, s, \
                       hidden, pooled, ldp, alpha)
    GS_ATTN_DISPATCH(hidden, LAUNCH);
#undef LAUNCH
    GS_LAUNCH_CHECK("attn_fwd_kernel");
    return GS_OK;
}

extern "C" int gs_segment_attn_bwd(const float* dP, int64_t ldd, const float* H, int64_t ldh, const int32_t* inv, const float* a,
                                   const float* alpha, int64_t n, int32_t s, int32_t hidden, float* dV, int64_t ldv,
                                   float* da_slabs, int32_t n_slabs, void* stream) {
    const int rc = attn_supported(s, hidden, "gs_segment_attn_bwd");
    if (rc != GS_OK) return rc;
    GS_REQUIRE(da_slabs && n_slabs > 0 && n_slabs <= 65535 && n >= 0, "gs_segment_attn_bwd: needs 1 <= n_slabs <= 65535, n >= 0");
    GS_REQUIRE(a && gs_aligned16(a), "gs_segment_attn_bwd: a must be non-null and 16-byte aligned");
    if (n > 0) {
        GS_CHECK_MAT(dP, ldd, "gs_segment_attn_bwd dP");
        GS_CHECK_MAT(H, ldh, "gs_segment_attn_bwd H");
        GS_CHECK_MAT(dV, ldv, "gs_segment_attn_bwd dV");
        GS_REQUIRE(alpha && ldd >= hidden && ldh >= hidden && ldv >= hidden && n * (int64_t)s < (1ll << 40),
                   "gs_segment_attn_bwd: bad args");
    }
    // n == 0 still writes the (all-zero) slabs: the caller has counted them
    // up to 512 columns: 16 waves of 4 rows in flight; beyond (16 floats per lane and row): 8 waves of 2, inside the register file
#define LAUNCH(CH)                                                                                                             \
    hipLaunchKernelGGL((attn_bwd_kernel<CH, (CH) <= 2 ? 16 : 8, (CH) <= 2 ? 4 : 2>), dim3((unsigned)n_slabs),                     \
                       dim3(64 * ((CH) <= 2 ? 16 : 8)), 0, (hipStream_t)stream, dP, ldd, H, ldh, inv, a, alpha, n, s, hidden, dV, \
                       ldv, da_slabs)
    GS_ATTN_DISPATCH(hidden, LAUNCH);
#undef LAUNCH
    GS_LAUNCH_CHECK("attn_bwd_kernel");
    return GS_OK;
}

extern "C" int gs_attn_scores(float* H, int64_t ldh, int64_t rows, int32_t hidden, const float* a, void* stream) {
    const int rc = attn_supported(1, hidden, "gs_attn_scores");
    if (rc != GS_OK) return rc;
    if (rows == 0) return GS_OK;
    GS_CHECK_MAT(H, ldh, "gs_attn_scores H");
    GS_REQUIRE(a && gs_aligned16(a) && rows > 0 && ldh >= hidden + 4, "gs_attn_scores: needs ld >= hidden + 4 (the score column)");
    const int64_t blocks = gs_ceil_div(rows, 4);
    GS_REQUIRE(blocks < (1ll << 31), "gs_attn_scores: grid too large");
#define LAUNCH(CH) \
    hipLaunchKernelGGL(attn_scores_kernel<CH>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, H, ldh, rows, hidden, a)
    GS_ATTN_DISPATCH(hidden, LAUNCH);
#undef LAUNCH
    GS_LAUNCH_CHECK("attn_scores_kernel");
    return GS_OK;
}
