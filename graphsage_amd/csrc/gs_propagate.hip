// Correct and Smooth / label propagation: one step of  out = clamp(alpha * D^-1/2 A D^-1/2 X + R)  over a CSR adjacency, for
// NARROW tables (d = the number of classes, 1 .. 256).
//
//   deg[r] = entries of row r that are not `pad` (duplicates count; deg[pad] = 0),  w[r] = fp32(1 / sqrt((double)deg[r])), 0 at deg 0
//   s      = w[r] * sum_e w[col[e]] * X[col[e]][j]            an entry equal to pad contributes exactly 0
//   out[r][j] = min(max(fmaf(alpha, s, R ? R[r][j] : 0), lo), hi),   out[pad][:] = 0
//
// Work decomposition: the work-item plan of gs_csr_reduce_fwd (one WAVE per item = a run of at most split_len edges of one
// row), but a wave is cut into G = 64 / Lg lane groups of Lg = 16 | 32 | 64 lanes (round_up(d, 4) <= 64 | 128 | 256): a lane
// holds ONE float4 of the row, group g takes the entries g, g + G, ... of the item in ascending order and adds them with
// fmaf(w_c, x, acc).  The item's column ids and their weights are loaded 64 at a time, one per lane, and handed to the groups
// by lane reads; PROP_U independent 16-byte row loads per lane are in flight before the first add.  The groups are then added
// in one fixed order by cross-lane moves (xor 32, then xor 16), group 0 finishes the row: scale, fmaf, clamp, store.  A cut
// row's plain sum goes to its partial slot and a second small launch adds the partials in slot order and finishes the row.
// No float atomics; the order of every addition is fixed => bitwise repeatable.
#include "gs_common.h"
#include "gs_gather_dev.h"

static_assert(sizeof(gs_prop_desc) == 176, "gs_prop_desc layout (mirrored by graphsage_amd/_lib.py)");

#define PROP_ITEM_WORDS 4    // (row, first edge, count, partial slot or -1): the plan of gs_csr_reduce_fwd
#define PROP_SPLIT_WORDS 3   // (row, first partial slot, partials)
#define PROP_U 8             // independent row loads per lane in flight

__host__ __device__ static inline int prop_cpad(int32_t d) { return (d + 3) / 4 * 4; }
static inline int prop_lg(int32_t d) { return prop_cpad(d) <= 64 ? 16 : (prop_cpad(d) <= 128 ? 32 : 64); }

// ---------------------------------------------------------------------------------------------------------------
// degrees and weights: one wave per row, its entries spread over the lanes, counted through ballots (integers only)
__global__ __launch_bounds__(256) void prop_weights_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                           const int64_t n_rows, const int64_t pad, int32_t* __restrict__ deg,
                                                           float* __restrict__ w) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_rows) return;                                 // wave-uniform
    const int64_t e0 = rowptr[r], e1 = rowptr[r + 1];
    int cnt = 0;
    if (r != pad)
        for (int64_t e = e0; e < e1; e += 64) {
            const bool real = e + lane < e1 && (int64_t)col[e + lane] != pad;
            cnt += __popcll(__ballot(real));
        }
    if (lane == 0) {
        deg[r] = cnt;
        w[r] = cnt > 0 ? (float)(1.0 / sqrt((double)cnt)) : 0.f;
    }
}

extern "C" int gs_prop_weights(const int64_t* rowptr, const int32_t* col, int64_t n_rows, int64_t pad, int32_t* deg, float* w,
                               void* stream) {
    GS_REQUIRE(n_rows >= 0 && pad >= 0 && pad <= n_rows, "gs_prop_weights: bad sizes n_rows=%lld pad=%lld", (long long)n_rows,
               (long long)pad);
    if (n_rows == 0) return GS_OK;
    GS_REQUIRE(rowptr && col && deg && w, "gs_prop_weights: rowptr, col, deg and w must be non-null");
    const int64_t blocks = gs_ceil_div(n_rows, 4);
    GS_REQUIRE(blocks < (1ll << 31), "gs_prop_weights: grid too large (%lld blocks)", (long long)blocks);
    hipLaunchKernelGGL(prop_weights_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rowptr, col, n_rows, pad,
                       deg, w);
    GS_LAUNCH_CHECK("prop_weights_kernel");
    return GS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// the row's value from its plain weighted sum: scale by w[r], fmaf with the residual, clamp; columns d .. round_up(d, 4) - 1 get 0
__device__ __forceinline__ f32x4 prop_finish(const f32x4 acc, const float wr, const float* __restrict__ R, const int64_t ldr,
                                             const int64_t row, const int col, const int d, const float alpha, const float lo,
                                             const float hi) {
    f32x4 r = f32x4{0.f, 0.f, 0.f, 0.f};
    if (R) r = *reinterpret_cast<const f32x4*>(R + row * ldr + col);
    f32x4 y;
    y.x = fminf(fmaxf(fmaf(alpha, wr * acc.x, r.x), lo), hi);
    y.y = fminf(fmaxf(fmaf(alpha, wr * acc.y, r.y), lo), hi);
    y.z = fminf(fmaxf(fmaf(alpha, wr * acc.z, r.z), lo), hi);
    y.w = fminf(fmaxf(fmaf(alpha, wr * acc.w, r.w), lo), hi);
    return gs_mask_tail(y, col, d);
}

// the entry at position `idx` of the current batch, for this lane's group: (row id or -1, weight)
template <int LG>
__device__ __forceinline__ void prop_entry(const int32_t my, const int wbits, const int idx, int32_t& r, float& wc) {
    if (LG == 64) {                                          // one group: the index is wave-uniform
        r = __builtin_amdgcn_readlane(my, idx);
        wc = __int_as_float(__builtin_amdgcn_readlane(wbits, idx));
    } else {
        r = __shfl(my, idx, 64);
        wc = __int_as_float(__shfl(wbits, idx, 64));
    }
}

template <int LG>
__global__ __launch_bounds__(256) void prop_step_kernel(const gs_prop_desc q) {
    constexpr int G = 64 / LG;
    const int lane = threadIdx.x & 63;
    const int64_t it = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (it >= q.n_items) return;                             // wave-uniform
    const int64_t* __restrict__ item = q.items + it * PROP_ITEM_WORDS;
    const int64_t row = item[0], e0 = item[1], cnt64 = item[2], slot = item[3];
    // a plan that does not belong to this graph / workspace must not turn into a stray access (wave-uniform)
    if (row < 0 || row >= q.n_rows || cnt64 < 0 || cnt64 > q.split_len || e0 < 0 || e0 + cnt64 > q.nnz || slot >= q.n_slots) return;
    const int cnt = (int)cnt64;
    const int g = lane / LG;
    const int col = (lane - g * LG) * 4;
    const bool active = col < q.d;
    const int lcol = active ? col : 0;                       // the column this lane loads: inside the row for every lane
    const float* __restrict__ X = q.X;
    const float* __restrict__ wt = q.w;
    const int32_t* __restrict__ cols = q.col + e0;
    const int64_t ldx = q.ldx;
    const int32_t pad = (int32_t)q.pad;

    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    if (row != q.pad) {
        for (int jb = 0; jb < cnt; jb += 64) {
            const int m = min(64, cnt - jb);                 // uniform
            // one entry per lane: a pad entry, an id outside the table and the lanes behind the batch are dead (-1, weight 0)
            int32_t my = -1;
            float myw = 0.f;
            if (lane < m) {
                const int32_t c = cols[jb + lane];
                if (c != pad && c >= 0 && c < q.n_rows) {
                    my = c;
                    myw = wt[c];
                }
            }
            const int wbits = __float_as_int(myw);
            const int steps = (m + G - 1) / G;               // uniform: entries t * G + g, t < steps
            for (int t0 = 0; t0 < steps; t0 += PROP_U) {
                // every load is issued, none under a branch: a dead entry reads row 0 and a lane behind the row column 0 (both
                // inside the table); the dead entry's values are dropped afterwards, the lane's sum is never stored
                f32x4 v[PROP_U];
                float wc[PROP_U];
                int32_t r[PROP_U];
#pragma unroll
                for (int u = 0; u < PROP_U; ++u) {
                    // t0 + u < LG whenever t0 < steps <= LG and LG % PROP_U == 0: the index stays inside the wave
                    prop_entry<LG>(my, wbits, (t0 + u) * G + g, r[u], wc[u]);
                    v[u] = *reinterpret_cast<const f32x4*>(X + (int64_t)max(r[u], 0) * ldx + lcol);
                }
#pragma unroll
                for (int u = 0; u < PROP_U; ++u) {
                    const bool dead = r[u] < 0;
                    acc.x = fmaf(wc[u], dead ? 0.f : v[u].x, acc.x);
                    acc.y = fmaf(wc[u], dead ? 0.f : v[u].y, acc.y);
                    acc.z = fmaf(wc[u], dead ? 0.f : v[u].z, acc.z);
                    acc.w = fmaf(wc[u], dead ? 0.f : v[u].w, acc.w);
                }
            }
        }
        // the groups in one fixed order: (g0 + g2) + (g1 + g3) for four, g0 + g1 for two
        if (G == 4) {
            acc.x += __shfl_xor(acc.x, 32, 64); acc.y += __shfl_xor(acc.y, 32, 64);
            acc.z += __shfl_xor(acc.z, 32, 64); acc.w += __shfl_xor(acc.w, 32, 64);
            acc.x += __shfl_xor(acc.x, 16, 64); acc.y += __shfl_xor(acc.y, 16, 64);
            acc.z += __shfl_xor(acc.z, 16, 64); acc.w += __shfl_xor(acc.w, 16, 64);
        } else if (G == 2) {
            acc.x += __shfl_xor(acc.x, 32, 64); acc.y += __shfl_xor(acc.y, 32, 64);
            acc.z += __shfl_xor(acc.z, 32, 64); acc.w += __shfl_xor(acc.w, 32, 64);
        }
    }
    if (g != 0 || !active) return;
    if (slot >= 0) {                                         // one segment of a cut row: the plain sum; prop_combine_kernel finishes
        *reinterpret_cast<f32x4*>(q.ws + slot * prop_cpad(q.d) + col) = acc;
        return;
    }
    if (row == q.pad) {
        *reinterpret_cast<f32x4*>(q.out + row * q.ldo + col) = f32x4{0.f, 0.f, 0.f, 0.f};
        return;
    }
    *reinterpret_cast<f32x4*>(q.out + row * q.ldo + col) = prop_finish(acc, wt[row], q.R, q.ldr, row, col, q.d, q.alpha, q.lo, q.hi);
}

// one thread per (cut row, float4 column): its partials in slot order, then the finish
__global__ __launch_bounds__(256) void prop_combine_kernel(const gs_prop_desc q, const int c4) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= q.n_split * c4) return;
    const int64_t si = t / c4;
    const int col = (int)(t - si * c4) * 4;
    const int64_t* __restrict__ sp = q.splits + si * PROP_SPLIT_WORDS;
    const int64_t row = sp[0], s0 = sp[1], parts = sp[2];
    if (row < 0 || row >= q.n_rows || parts < 0 || s0 < 0 || parts > q.n_slots || s0 > q.n_slots - parts) return;
    const int64_t ldw = prop_cpad(q.d);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int64_t k = 0; k < parts; ++k) acc += *reinterpret_cast<const f32x4*>(q.ws + (s0 + k) * ldw + col);
    if (row == q.pad) {
        *reinterpret_cast<f32x4*>(q.out + row * q.ldo + col) = f32x4{0.f, 0.f, 0.f, 0.f};
        return;
    }
    *reinterpret_cast<f32x4*>(q.out + row * q.ldo + col) = prop_finish(acc, q.w[row], q.R, q.ldr, row, col, q.d, q.alpha, q.lo, q.hi);
}

extern "C" int gs_prop_ws_bytes(int64_t n_slots, int32_t d, int64_t* bytes_out_host) {
    GS_REQUIRE(bytes_out_host && n_slots >= 0 && d > 0, "gs_prop_ws_bytes: bad args");
    *bytes_out_host = n_slots * (int64_t)prop_cpad(d) * (int64_t)sizeof(float);
    return GS_OK;
}

// the range of d shared by gs_prop_step and gs_prop_correct
static int prop_check_d(const char* who, int32_t d) {
    if (d < 1 || d > GS_PROP_MAX_D) {
        gs_set_error("%s: d = %d, the narrow-table kernels take 1 <= d <= %d", who, d, GS_PROP_MAX_D);
        return GS_ENOTSUP;
    }
    return GS_OK;
}

extern "C" int gs_prop_step(const gs_prop_desc* desc_host, void* stream) {
    GS_REQUIRE(desc_host, "gs_prop_step: null descriptor");
    const gs_prop_desc& q = *desc_host;
    if (const int rc = prop_check_d("gs_prop_step", q.d)) return rc;
    GS_REQUIRE(q.n_rows >= 0 && q.n_rows < (1ll << 31) && q.nnz >= 0 && q.split_len > 0 && q.n_items >= 0 && q.n_split >= 0 &&
                   q.n_slots >= 0 && q.pad >= 0 && q.pad <= q.n_rows,
               "gs_prop_step: bad sizes n_rows=%lld nnz=%lld split_len=%d items=%lld splits=%lld slots=%lld pad=%lld",
               (long long)q.n_rows, (long long)q.nnz, q.split_len, (long long)q.n_items, (long long)q.n_split,
               (long long)q.n_slots, (long long)q.pad);
    GS_REQUIRE(q.alpha == q.alpha && q.lo == q.lo && q.hi == q.hi && q.lo <= q.hi, "gs_prop_step: alpha, lo <= hi must be numbers");
    if (q.n_items == 0) return GS_OK;
    GS_REQUIRE(q.rowptr && q.col && q.items && q.w, "gs_prop_step: rowptr, col, items and w must be non-null");
    GS_REQUIRE(q.n_items >= q.n_rows, "gs_prop_step: %lld items for %lld rows (the plan covers every row)", (long long)q.n_items,
               (long long)q.n_rows);
    GS_CHECK_MAT(q.X, q.ldx, "gs_prop_step X");
    GS_CHECK_MAT(q.out, q.ldo, "gs_prop_step out");
    if (q.R) GS_CHECK_MAT(q.R, q.ldr, "gs_prop_step R");
    const int cpad = prop_cpad(q.d);
    GS_REQUIRE(q.ldx >= cpad && q.ldo >= cpad && (!q.R || q.ldr >= cpad), "gs_prop_step: ld must be >= round_up(d,4) = %d", cpad);
    GS_REQUIRE(q.out != q.X, "gs_prop_step: out must not be X (a row is read by its neighbors' waves while its own writes it)");
    if (q.n_slots > 0 || q.n_split > 0) {
        GS_REQUIRE(q.splits && q.ws && gs_aligned16(q.ws), "gs_prop_step: cut rows need splits and a 16-byte aligned workspace");
        GS_REQUIRE(q.ws_bytes >= q.n_slots * (int64_t)cpad * (int64_t)sizeof(float),
                   "gs_prop_step: workspace of %lld bytes is too small (gs_prop_ws_bytes)", (long long)q.ws_bytes);
    }
    const hipStream_t st = (hipStream_t)stream;
    const int64_t blocks = gs_ceil_div(q.n_items, 4);
    GS_REQUIRE(blocks < (1ll << 31), "gs_prop_step: grid too large (%lld blocks)", (long long)blocks);
    const int lg = prop_lg(q.d);
    if (lg == 16) hipLaunchKernelGGL(prop_step_kernel<16>, dim3((unsigned)blocks), dim3(256), 0, st, q);
    else if (lg == 32) hipLaunchKernelGGL(prop_step_kernel<32>, dim3((unsigned)blocks), dim3(256), 0, st, q);
    else hipLaunchKernelGGL(prop_step_kernel<64>, dim3((unsigned)blocks), dim3(256), 0, st, q);
    GS_LAUNCH_CHECK("prop_step_kernel");
    if (q.n_split > 0) {
        const int c4 = cpad / 4;
        const int64_t b2 = gs_ceil_div(q.n_split * c4, 256);
        GS_REQUIRE(b2 < (1ll << 31), "gs_prop_step: combine grid too large (%lld blocks)", (long long)b2);
        hipLaunchKernelGGL(prop_combine_kernel, dim3((unsigned)b2), dim3(256), 0, st, q, c4);
        GS_LAUNCH_CHECK("prop_combine_kernel");
    }
    return GS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// the autoscaled correction and the label overwrite: one lane group per row (the groups of the step kernel), l1 = sum |E[i]|
// added per lane in column order, then over the group by the xor butterfly Lg/2 .. 1
template <int LG>
__global__ __launch_bounds__(256) void prop_correct_kernel(const float* __restrict__ P, const int64_t ldp, const float* __restrict__ E,
                                                           const int64_t lde, const float* __restrict__ Y, const int64_t ldy,
                                                           const int32_t* __restrict__ known, const int64_t n, const int d,
                                                           const float sigma, float* __restrict__ out, const int64_t ldo) {
    constexpr int G = 64 / LG;
    const int lane = threadIdx.x & 63;
    const int g = lane / LG;
    const int col = (lane - g * LG) * 4;
    const int64_t i = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * G + g;
    const bool active = i < n && col < d;
    f32x4 e = f32x4{0.f, 0.f, 0.f, 0.f};
    if (active) e = gs_mask_tail(*reinterpret_cast<const f32x4*>(E + i * lde + col), col, d);
    float l1 = (fabsf(e.x) + fabsf(e.y)) + (fabsf(e.z) + fabsf(e.w));
#pragma unroll
    for (int o = LG / 2; o > 0; o >>= 1) l1 += __shfl_xor(l1, o, 64);
    if (!active) return;
    f32x4 y;
    if (Y && known[i] != 0) {
        y = *reinterpret_cast<const f32x4*>(Y + i * ldy + col);
    } else {
        float scale = sigma / l1;
        if (!(fabsf(scale) <= 1000.0f) || scale > 1000.0f) scale = 1.0f;          // not finite (l1 = 0, NaN) or beyond the cap
        const f32x4 p = *reinterpret_cast<const f32x4*>(P + i * ldp + col);
        y = f32x4{fmaf(scale, e.x, p.x), fmaf(scale, e.y, p.y), fmaf(scale, e.z, p.z), fmaf(scale, e.w, p.w)};
    }
    *reinterpret_cast<f32x4*>(out + i * ldo + col) = gs_mask_tail(y, col, d);
}

extern "C" int gs_prop_correct(const float* P, int64_t ldp, const float* E, int64_t lde, const float* Y, int64_t ldy,
                               const int32_t* known, int64_t n, int32_t d, float sigma, float* out, int64_t ldo, void* stream) {
    if (const int rc = prop_check_d("gs_prop_correct", d)) return rc;
    GS_REQUIRE(n >= 0, "gs_prop_correct: n = %lld", (long long)n);
    if (n == 0) return GS_OK;
    GS_CHECK_MAT(P, ldp, "gs_prop_correct P");
    GS_CHECK_MAT(E, lde, "gs_prop_correct E");
    GS_CHECK_MAT(out, ldo, "gs_prop_correct out");
    if (Y) GS_CHECK_MAT(Y, ldy, "gs_prop_correct Y");
    GS_REQUIRE(!Y || known, "gs_prop_correct: Y needs the known flags");
    const int cpad = prop_cpad(d);
    GS_REQUIRE(ldp >= cpad && lde >= cpad && ldo >= cpad && (!Y || ldy >= cpad), "gs_prop_correct: ld must be >= round_up(d,4) = %d",
               cpad);
    const int lg = prop_lg(d);
    const int64_t blocks = gs_ceil_div(n, 4 * (64 / lg));
    GS_REQUIRE(blocks < (1ll << 31), "gs_prop_correct: grid too large (%lld blocks)", (long long)blocks);
    const hipStream_t st = (hipStream_t)stream;
    if (lg == 16)
        hipLaunchKernelGGL(prop_correct_kernel<16>, dim3((unsigned)blocks), dim3(256), 0, st, P, ldp, E, lde, Y, ldy, known, n, d, sigma, out, ldo);
    else if (lg == 32)
        hipLaunchKernelGGL(prop_correct_kernel<32>, dim3((unsigned)blocks), dim3(256), 0, st, P, ldp, E, lde, Y, ldy, known, n, d, sigma, out, ldo);
    else
        hipLaunchKernelGGL(prop_correct_kernel<64>, dim3((unsigned)blocks), dim3(256), 0, st, P, ldp, E, lde, Y, ldy, known, n, d, sigma, out, ldo);
    GS_LAUNCH_CHECK("prop_correct_kernel");
    return GS_OK;
}
