/*
 * graphsage_amd.h -- C ABI of the MI355X (gfx950) GraphSAGE sample-and-aggregate engine.
 *
 * The reference (williamleif/GraphSAGE, 100 % Python on TensorFlow 1.x) has no FFI of its own;
 * its hot path bottoms out in TF ops.  Each entry point below replaces the TF-op call sites of
 * one reference operator (cited as graphsage/<file>:<line>, relative to the reference tree) and
 * is what a ctypes binding of that operator binds.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.
 *   - Every pointer is a DEVICE pointer owned by the caller unless the name ends in _host.
 *   - Every function enqueues work on `stream` (a hipStream_t passed as void*; must not be the
 *     legacy NULL stream if the caller wants to capture it into a hipGraph) and returns
 *     immediately.  The library allocates no device memory; scratch is caller-supplied.
 *   - Return value: 0 = ok, <0 = error (GS_E*); gs_last_error() gives a thread-local message.
 *     No C++ exception crosses the boundary.
 *   - Matrices are row-major fp32 with an explicit leading dimension `ld*` (elements).  Every
 *     fp32 matrix base pointer must be 16-byte aligned and every ld a multiple of 4 floats;
 *     the logical width d may be anything <= ld.  Columns [d, round_up(d,4)) of OUTPUT matrices
 *     are written as zeros; further pad columns are left untouched.
 *   - Index arrays are int32 (the reference feeds int32 placeholders, supervised_train.py:116);
 *     CSR row pointers are int64.
 */
#ifndef GRAPHSAGE_AMD_H
#define GRAPHSAGE_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS_OK 0
#define GS_EINVAL (-1)  /* bad argument (null pointer, misaligned, bad size)  */
#define GS_EHIP (-2)    /* a HIP runtime call failed                           */
#define GS_ENOTSUP (-3) /* combination not supported by the gfx950 kernels     */

#define GS_ACT_IDENTITY 0
#define GS_ACT_RELU 1

/* bumped when a struct layout or an existing signature changes; added entry points alone (gs_pool2_*, gs_logreg_*) leave it as it is */
#define GS_ABI_VERSION 12

const char* gs_last_error(void);
int gs_abi_version(void);
/* sizeof() of the descriptor structs below, in declaration order (gs_gather_desc, gs_wgrad_desc, gs_var_desc,
 * gs_fanout_desc, gs_tail_desc, gs_dropout, gs_pull_desc, gs_lp_tail_desc): writes min(count, capacity) values, returns the count.  A
 * binding compares them with its own struct definitions at load time. */
int gs_abi_struct_sizes(int32_t* sizes_out_host, int32_t capacity);
/* Fills CU count, XCD count (8 on MI355X), gcnArchName (>= 64 bytes) of the current device. */
int gs_device_info(int* cu_count, int* xcd_count, char* arch_name_host, int arch_name_len);

/* ---------------------------------------------------------------------------------------------
 * K1  neighbor sampling      replaces UniformNeighborSampler._call, neigh_samplers.py:24-29
 *                            (called at models.py:272, result flattened at models.py:273)
 * ------------------------------------------------------------------------------------------- */

/* Exact reference semantics on the padded table of minibatch.py:227-259:
 *   out[i, j] = adj[ids[i], col_perm[j]],  j < num_samples
 * i.e. embedding_lookup (:26) + ONE column permutation shared by all rows (:27) + slice (:28).
 * TF's random_shuffle stream is not reproducible, so the permutation is an input.
 * adj is [n_adj_rows, max_deg] int32 (n_adj_rows = N+1, row N = all-pad).  Bit-exact. */
int gs_sample_padded(const int32_t* adj, int64_t n_adj_rows, int32_t max_deg,
                     const int32_t* ids, int64_t n,
                     const int32_t* col_perm, int32_t num_samples,
                     int32_t* out, void* stream);

/* MI355X-native sampler over a CSR adjacency (rowptr int64 [n_nodes+1], col int32 [nnz]):
 *   deg = rowptr[id+1]-rowptr[id];  out[i,j] = deg ? col[rowptr[id] + ((u(i,j) >> 32) * deg >> 32)] : pad_id
 * u(i,j) is a counter-based xorshift-multiply hash of
 *   (seed, step + *step_dev, hop, global_row_offset + i, j)
 * so the draw for a given root row does not depend on how rows are sharded over GPUs.
 * ids >= n_nodes (the pad id) yield pad_id (the all-pad row N of the reference table).
 * law = GS_LAW_IID: uniform WITH replacement over the true neighbor set (the formula above): the per-slot marginal
 *   equals the reference's (padded row resampled once + distinct columns); max_degree ignored.
 * law = GS_LAW_REFERENCE: the reference's joint law without its table.  Node v's row of the padded [N+1, max_degree]
 *   table of minibatch.py:227-245 is VIRTUAL -- entry c is a pure function of (seed, v, c): the first max_degree
 *   elements of a keyed permutation of the neighbor list when deg > max_degree (np.random.choice(replace=False),
 *   :240-241), max_degree frozen iid draws when deg < max_degree (replace=True, :242-243), the list itself when equal
 *   -- frozen for the run like the reference's table; per call, num_samples DISTINCT columns are the head of ONE keyed
 *   permutation of [0, max_degree) shared by all rows (tf.random_shuffle of the transposed rows, neigh_samplers.py:27-28).
 *   Requires num_samples <= max_degree (tf.slice fails otherwise).
 * law = GS_LAW_DISTINCT: per-row independent draws WITHOUT replacement whenever the list (capped to a frozen
 *   max_degree subset if max_degree > 0) holds >= num_samples entries, with replacement otherwise.
 * All three are pure functions of (seed, step, hop, global row, j[, node id]); restated in oracle/sampler_hash.py.
 * step_dev may be NULL. */
#define GS_LAW_IID 0
#define GS_LAW_REFERENCE 1
#define GS_LAW_DISTINCT 2
int gs_sample_uniform_csr(const int64_t* rowptr, const int32_t* col, int64_t n_nodes, int32_t pad_id,
                          const int32_t* ids, int64_t n, int32_t num_samples,
                          uint64_t seed, uint64_t step, const uint64_t* step_dev, uint32_t hop,
                          int64_t global_row_offset, int32_t law, int32_t max_degree, int32_t* out, void* stream);

/* Fused multi-hop fan-out (replaces the K calls of models.py:268-274 with ONE launch): one workgroup per root,
 * hop h kept in an LDS fan-out buffer for hop h+1, all hops written to the contiguous buffer
 *   ids_all = [roots (B) | hop 1 (B*fan[0]) | hop 2 (B*fan[0]*fan[1]) | ...]   at offsets_host[0..n_hops].
 * fan_host[h] is the fan-out of the h-th sampler call (= layer_infos[K-1-h].num_samples).  Draws are bit-identical
 * to n_hops calls of gs_sample_uniform_csr with hop = hop0 + h and global_row_offset = root_offset*support[h].
 * If order != NULL the roots are first staged as ids_all[i] = order[(*cursor_dev + i) % n_order] and, if
 * label_table != NULL, labels_out[i] = label_table[root_i] (minibatch.py:264-274, 302-307 on the device). */
int gs_sample_fanout_csr(const int64_t* rowptr, const int32_t* col, int64_t n_nodes, int32_t pad_id,
                         int32_t n_hops, const int32_t* fan_host, const int64_t* offsets_host,
                         int32_t* ids_all, int64_t B, uint64_t seed, uint64_t step, const uint64_t* step_dev,
                         uint32_t hop0, int64_t root_offset,
                         const int32_t* order, int64_t n_order, const uint64_t* cursor_dev,
                         const float* label_table, int64_t ld_table, int32_t C, float* labels_out, int64_t ld_out,
                         int32_t law, int32_t max_degree, void* stream);

/* batch[i] = order[(*cursor_dev + i) % n_order] for i < n  (epoch order lives on the device so the
 * whole training step can be one hipGraph).  Replaces the host slicing of minibatch.py:302-307. */
int gs_select_batch(const int32_t* order, int64_t n_order, const uint64_t* cursor_dev,
                    int64_t n, int32_t* batch, void* stream);

/* *counter_dev += delta  (advances step / cursor inside a captured graph). */
int gs_advance_counter(uint64_t* counter_dev, uint64_t delta, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K2  feature gather (+ segmented mean)
 *     replaces tf.nn.embedding_lookup at models.py:299, the reshape at models.py:326-327 and
 *     reduce_mean(axis=1) at aggregators.py:48 (Mean) / :106-107 (GCN)
 * ------------------------------------------------------------------------------------------- */

/* out[i, :] = X[ids[i], :d] */
int gs_gather_rows(const float* X, int64_t ldx, const int32_t* ids, int64_t n, int32_t d,
                   float* out, int64_t ldo, void* stream);

/* mean[i, :] = scale * ( sum_{j<s} X[idx[i*s+j], :d]  [+ S[self_idx ? self_idx[i] : i, :d]] )
 *   idx == NULL       -> neighbor row is i*s+j (contiguous groups; hidden layers, models.py:327)
 *   self_src == NULL  -> MeanAggregator, scale = 1/s          (aggregators.py:48)
 *   self_src != NULL  -> GCNAggregator,  scale = 1/(s+1)      (aggregators.py:106-107)
 * The [n*s, d] gathered tensor of models.py:299 is never materialised. */
int gs_gather_mean_fwd(const float* X, int64_t ldx, const int32_t* idx, int64_t n, int32_t s, int32_t d,
                       const float* self_src, int64_t ld_self, const int32_t* self_idx,
                       float* mean, int64_t ldm, void* stream);

/* Backward of the segmented mean for hidden layers (gradient of aggregators.py:48 / :106-107):
 *   g = d_mean[r / s, :] * scale;  if (mask_y) g *= (mask_y[r, :] > 0)   (fused relu grad of the
 *   producing layer, aggregators.py:64);  d_neigh[r, :] (+)= g   for r < n*s. */
int gs_mean_bwd(const float* d_mean, int64_t ldd, int64_t n, int32_t s, int32_t d, float scale,
                const float* mask_y, int64_t ldy, float* d_neigh, int64_t ldn, int accumulate,
                void* stream);

/* ---------------------------------------------------------------------------------------------
 * K3  dense contraction (fp32 MFMA, v_mfma_f32_32x32x2_f32)
 *     replaces tf.matmul at aggregators.py:51,53 (Mean), :110 (GCN), :183-184 (MaxPool),
 *     concat/add_n at :56-58, bias :61-62, act :64, and Dense._call layers.py:104-116
 *
 *     Operand contract of every entry point of this section and of gs_dense_pool_max_fwd / gs_dense_fwd_rows_dev: an operand is
 *     read as whole float4, so columns up to round_up(width, 4) (from col0 where there is one) must be READABLE, but nothing
 *     outside the logical operand is ever used -- pad columns, the columns next to a [col0, col0 + out_dim) slice (a column
 *     slice of a wider matrix is a valid operand), table rows that no index names and rows beyond the row count may hold
 *     anything, NaN included.  Outputs: the logical block is written, columns [N, round_up(N, 4)) are written as zeros except
 *     by the split-K slab forms (gs_dense_wgrad*: logical columns only; a slab whose row slice is empty is zeros) and the
 *     pooled / argmax outputs of gs_dense_pool_max_fwd (logical columns only, stored word by word: ldp, lda >= hidden is all
 *     they need); no other word is touched.  tests/test_gemm_edges_gpu.py holds this.
 * ------------------------------------------------------------------------------------------- */

/* out = act( [ self·W_self  ||  agg·W_neigh ] + bias )          concat != 0   (out is [n, 2*out_dim])
 * out = act(   self·W_self  +   agg·W_neigh   + bias )          concat == 0   (out is [n, out_dim])
 * self == NULL -> single term  out = act(agg·W_neigh + bias)  (GCN / Dense).
 * self_idx != NULL gathers the self rows from `self` on the fly (self row i = self[self_idx[i]]),
 * which is how layer 0 consumes X[samples[hop]] without materialising it.  Same for agg_idx. */
int gs_sage_dense_fwd(const float* self, int64_t ld_self, const int32_t* self_idx, int32_t d_self,
                      const float* agg, int64_t ld_agg, const int32_t* agg_idx, int32_t d_agg,
                      int64_t n,
                      const float* W_self, int64_t ldw_self, const float* W_neigh, int64_t ldw_neigh,
                      int32_t out_dim, int concat, int act, const float* bias,
                      float* out, int64_t ldo, void* stream);

/* Horizontally fused launch: gs_sage_dense_fwd (two-term form) PLUS up to 4 independent gs_gather_mean_fwd jobs in
 * the SAME kernel launch -- the GEMM tiles are the first workgroups, the gather waves back-fill the CUs.  Used to
 * overlap the MFMA-bound layer-0 contraction of step t with the HBM-bound neighbor gather of step t+1 (which needs
 * no weights) without cross-stream synchronisation.  Results are identical to the separate calls. */
typedef struct gs_gather_desc {
    const float* X;            /* [*, ldx] table                                         */
    const int32_t* idx;        /* [n*s] (NULL -> contiguous groups)                       */
    const float* self_src;     /* GCN: self rows (NULL -> MeanAggregator scale 1/s)       */
    const int32_t* self_idx;
    float* out;                /* [n, ldo]                                                */
    int64_t ldx, ld_self, ldo, n;
    int32_t s, d;
} gs_gather_desc;
int gs_sage_dense_fwd_cogather(const float* self, int64_t ld_self, const int32_t* self_idx, int32_t d_self,
                               const float* agg, int64_t ld_agg, const int32_t* agg_idx, int32_t d_agg,
                               int64_t n,
                               const float* W_self, int64_t ldw_self, const float* W_neigh, int64_t ldw_neigh,
                               int32_t out_dim, int concat, int act, const float* bias,
                               float* out, int64_t ldo,
                               const gs_gather_desc* jobs_host, int32_t n_jobs, void* stream);

/* Weight gradient as split-K slabs (deterministic; no atomics):
 *   slab[z][:, :] = sum_{r in slice z} A[a_idx? a_idx[r] : r, :d]^T · dZ[r, col0:col0+out_dim]
 * for z < n_slabs (row slices of equal size).  slabs is [n_slabs, d, ld_slab].  The caller sums
 * the slabs with gs_reduce_slabs.  Gradient of the tf.matmul call sites above w.r.t. the weights. */
int gs_dense_wgrad(const float* A, int64_t lda, const int32_t* a_idx, int32_t d,
                   const float* dZ, int64_t ldz, int32_t col0, int32_t out_dim, int64_t n,
                   int32_t n_slabs, float* slabs, int64_t ld_slab, void* stream);

/* Both input gradients of a SAGE dense layer in ONE launch (two-term NT GEMM, concatenated output):
 *   dX2[:, 0:d_in]       = dZ_self  · W_self^T      dZ_self  = dZ[:, 0:out_dim]
 *   dX2[:, d_in:2*d_in]  = dZ_neigh · W_neigh^T     dZ_neigh = dZ[:, out_dim:2*out_dim] if fwd_concat else dZ_self
 * d_in % 4 == 0 and (if fwd_concat) out_dim % 4 == 0.  Gradient of aggregators.py:51,53. */
int gs_sage_dense_dgrad(const float* dZ, int64_t ldz, int64_t n, int32_t out_dim, int fwd_concat,
                        const float* W_self, int64_t ldw_self, const float* W_neigh, int64_t ldw_neigh,
                        int32_t d_in, float* dX2, int64_t ldx, void* stream);

/* All weight gradients of one backward pass in ONE launch (grouped split-K GEMM).  Each descriptor is one
 * gs_dense_wgrad problem; a bias gradient is the problem A = ones[n, 1] (d = 1).  descs_host is a HOST array
 * that is consumed at call time (kernel arguments are copied), so it may be freed right after the call. */
typedef struct gs_wgrad_desc {
    const float* A;        /* [rows, lda] source of the reduction (row-gathered through a_idx if non-null) */
    const int32_t* a_idx;
    const float* dZ;       /* [n, ldz] */
    float* slabs;          /* [n_slabs, d, ld_slab] */
    int64_t lda, ldz, ld_slab, n;
    int32_t d, col0, out_dim, n_slabs;
    int64_t a_rows;        /* rows of the A table when a_idx != NULL (0 = not stated; gs_dense_wgrad_grouped_stream needs it) */
} gs_wgrad_desc;
int gs_dense_wgrad_grouped(const gs_wgrad_desc* descs_host, int32_t n_desc, void* stream);
/* The grouped weight-gradient launch + up to 4 gather+mean jobs (see gs_sage_dense_fwd_cogather) in ONE horizontally
 * fused launch: lets the next step's HBM-bound gather be split between the layer-0 forward and the weight-gradient
 * launch of the current step.  Results are those of the separate calls. */
int gs_dense_wgrad_grouped_cogather(const gs_wgrad_desc* descs_host, int32_t n_desc, const gs_gather_desc* jobs_host,
                                    int32_t n_jobs, void* stream);

/* "Stream" forms of the two launches above (same maths, same co-scheduled gather jobs, up to 6 of them): the
 * contraction waves stage no operand through LDS and meet no barrier inside the K loop -- operands go from L2 into the
 * MFMA registers through a register ring -- so that the gather waves sharing the launch keep their occupancy.
 *   gs_sage_dense_fwd_stream: out[:, 0:out_dim] = act(self[self_idx] . W_self + bias), out[:, out_dim:2*out_dim] =
 *     act(agg . W_neigh + bias)  (concat form of aggregators.py:51-58; self == NULL: the single GCN contraction,
 *     aggregators.py:110).  self_idx (nullable) gathers the self rows inside the A loads; agg is [n, d] dense; pad
 *     columns [d, round_up(d, 4)) must be readable.  out_dim and ldo even.  One workgroup per 32 x 64 output tile,
 *     K split over its four waves and summed in a fixed order (deterministic).
 *   gs_dense_wgrad_grouped_stream: as gs_dense_wgrad_grouped (<= 12 problems; a row-gathered problem needs
 *     ceil(n / n_slabs) <= 512 -- the slice's row offsets live in registers -- and a_rows). */
int gs_sage_dense_fwd_stream(const float* self, int64_t ld_self, const int32_t* self_idx, const float* agg, int64_t ld_agg,
                             int32_t d, int64_t n, const float* W_self, int64_t ldw_self, const float* W_neigh,
                             int64_t ldw_neigh, int32_t out_dim, int act, const float* bias, float* out, int64_t ldo,
                             const gs_gather_desc* jobs_host, int32_t n_jobs, void* stream);
/* gs_sage_dense_fwd_stream2 (ABI 8): the same launch with different reduction lengths of the two terms -- the pooling
 * aggregators' from_self = self[self_idx] . W_self over d_self features and from_neighs = pooled . W_neigh over d_agg = hidden_dim
 * (aggregators.py:183-187, :261-265), concat form; pad columns of both operands readable as above. */
int gs_sage_dense_fwd_stream2(const float* self, int64_t ld_self, const int32_t* self_idx, int32_t d_self, const float* agg,
                              int64_t ld_agg, int32_t d_agg, int64_t n, const float* W_self, int64_t ldw_self,
                              const float* W_neigh, int64_t ldw_neigh, int32_t out_dim, int act, const float* bias, float* out,
                              int64_t ldo, const gs_gather_desc* jobs_host, int32_t n_jobs, void* stream);
int gs_dense_wgrad_grouped_stream(const gs_wgrad_desc* descs_host, int32_t n_desc, const gs_gather_desc* jobs_host,
                                  int32_t n_jobs, void* stream);
/* gs_dense_wgrad_grouped_tiled3 (ABI 9, round 6): gs_dense_wgrad_grouped_stream -- same descriptors, same split-K slabs, same
 * co-scheduled gather jobs -- in the three-piece bf16 arithmetic of gs_sage_dense_fwd_tiled3 (fp32 in and out, the accuracy of an
 * fp32 FMA chain), LDS-tiled: one four-wave workgroup per (64 x 128 tile of dW, reduction slice), stage = 16 k, both operands moved
 * HBM -> LDS raw by LDS-DMA and cut by the waves that read them (form 0; gs_set_wgrad_tiled3_form).  <= 12 problems; a slice is round_up(ceil(n / n_slabs), 32) rows and must not
 * exceed 1024 (any problem, gathered or dense); row addresses are 64-bit (tables beyond 4 GB are fine: a_rows is not needed).  A slab whose slice is empty is
 * written as zeros.  Replaces the TF-op group of aggregators.py:51-58's gradient (tf.gradients of the two matmuls). */
int gs_dense_wgrad_grouped_tiled3(const gs_wgrad_desc* descs_host, int32_t n_desc, const gs_gather_desc* jobs_host,
                                  int32_t n_jobs, void* stream);
/* Which kernel gs_dense_wgrad_grouped_tiled3 / _sample launch (process-wide, read at launch; no ABI change: same descriptors, same
 * slabs bit for bit): 0 = every wave reads and cuts the raw A tile for itself (both operands by LDS-DMA, an LDS list of the
 * slice's rows); 1 = A travels through registers and is cut once per workgroup into bf16 piece buffers that the four waves share
 * (the A path of gs_sage_dense_fwd_tiled3, transposed; dZ as in form 0; the slice's row ids live in registers).  GS_EINVAL
 * for any other value. */
int gs_set_wgrad_tiled3_form(int form);
/* gs_sage_dense_fwd_tiled3 (ABI 9, round 6): the contraction of gs_sage_dense_fwd_stream2 -- same arguments, fp32 operands in and
 * out -- on the bf16 matrix pipe in the three-piece arithmetic described below (every fp32 operand = three bf16 pieces, six exact
 * piece products per element pair, fp32 accumulation: the accuracy of an fp32 FMA chain), LDS-tiled: one four-wave workgroup per
 * 64 x 128 output tile of a term, stage = 16 k; the A rows ((gathered) fp32) are cut once per workgroup in registers, the weights
 * go global -> LDS by DMA as fp32 and are cut by the wave that contracts them (no pre-cut copy, nothing to refresh after an
 * optimizer step); a wave contracts every stage of its 64 x 32 tile, so an element's K reduction has one fixed order
 * (deterministic).  Pad columns [d, round_up(d, 4)) of self / agg must be readable (any value: masked); out_dim and ldo multiples
 * of 4.  self == NULL: one term (GCN).  Gather jobs ride as in gs_sage_dense_fwd_stream. */
int gs_sage_dense_fwd_tiled3(const float* self, int64_t ld_self, const int32_t* self_idx, int32_t d_self, const float* agg,
                             int64_t ld_agg, int32_t d_agg, int64_t n, const float* W_self, int64_t ldw_self, const float* W_neigh,
                             int64_t ldw_neigh, int32_t out_dim, int act, const float* bias, float* out, int64_t ldo,
                             const gs_gather_desc* jobs_host, int32_t n_jobs, void* stream);
/* gs_sage_dense_fwd_tiled3_means (added entry point): gs_sage_dense_fwd_tiled3 (concat form: self != NULL) over the rows
 * [roots (n_roots) | hop 1 (n_roots * s; rows n_roots + i*s .. + s - 1 belong to root i)], n = n_roots * (1 + s), 1 <= s <= 64, that
 * ALSO writes the next layer's neighbor means from the finished tiles (reduce_mean of aggregators.py:48 over the layer's own output):
 *   l1_means[i, c] = (((0 + out[n_roots + i*s, c]) + out[n_roots + i*s + 1, c]) + ...) * (1.f / s),  i < n_roots, c < 2 * out_dim
 * (fp32, this order: the bits the fused tail's helper workgroups form from `out`); l1_means is [n_roots, ld_means >= 2 * out_dim],
 * 16-byte aligned, ld_means % 4 == 0; no other word of it is touched.  `out` is bit-identical to gs_sage_dense_fwd_tiled3's: hop
 * rows are tiled (64 / s) * s to a workgroup so that no root's rows straddle two, and an element's K reduction does not depend
 * on the tiling. */
int gs_sage_dense_fwd_tiled3_means(const float* self, int64_t ld_self, const int32_t* self_idx, int32_t d_self, const float* agg,
                                   int64_t ld_agg, int32_t d_agg, int64_t n, const float* W_self, int64_t ldw_self,
                                   const float* W_neigh, int64_t ldw_neigh, int32_t out_dim, int act, const float* bias, float* out,
                                   int64_t ldo, const gs_gather_desc* jobs_host, int32_t n_jobs, int64_t n_roots, int32_t s,
                                   float* l1_means, int64_t ld_means, void* stream);
/* Contractions on the bf16 matrix pipe WITHOUT giving up fp32: every fp32 operand x is cut into three bf16 pieces
 * x = h + m + l (top / middle / low 8 significant bits: nothing is lost), a product is the sum of piece products -- each formed
 * exactly by v_mfma_f32_32x32x16_bf16 and accumulated in fp32 -- and six of the nine are kept (hh, hm, mh, mm, hl, lh; the
 * dropped ml, lm, ll are <= 3 * 2^-24 |x y|, one fp32 rounding).  Accuracy of an fp32 FMA chain at 6/16 of the fp32 MFMA's
 * matrix-pipe time (fp32 MFMA runs at the vector rate on gfx950, 1/16 of bf16).  Inputs, outputs, accumulation: fp32.
 *   gs_split_rows: W [K, ldw >= N] fp32 -> W3 [G][3][N][8] bf16 (per group of 8 k and piece: the N columns side by side,
 *     16 bytes each -- a B-fragment load of 32 lanes reads 512 contiguous bytes; G = groups up to an even count of 32-k
 *     stages, zero for k >= K: the kernels neither mask nor clamp their B loads); gs_split_rows_bytes gives the size.  Call it after every update of W.
 *   gs_dense_fwd_rows_split: gs_dense_fwd_rows_dev in the same arithmetic, LDS-tiled (128 x 128 per workgroup, A rows gathered
 *     through idx and cut once per workgroup): the pooling MLP of the max-pool aggregator on the step's distinct ids.
 */
int gs_split_rows_bytes(int32_t K, int32_t N, int64_t* bytes_out_host);
int gs_dense_fwd_rows_split(const float* X, int64_t ldx, const int32_t* idx, int32_t d, int64_t n_max, const int32_t* n_dev,
                            const void* W3, int32_t out_dim, int act, const float* bias, float* out, int64_t ldo, void* stream);
/* gs_dense_fwd_rows_split with a workspace (ABI 8): the wide form's workgroups run one per CU in lock step, so a tile count
 * that is not a multiple of the CU count ends in a round that keeps a few CUs busy (Reddit max-pool step: 1300 tiles on 256 CUs
 * = six rounds for 5.08 rounds of work).  With ws (>= gs_dense_fwd_rows_split_ws_bytes, 16-byte aligned, contents undefined
 * on entry and on return) the tiles of that last round are cut along K into up to ten parts whose fp32 partial tiles are summed
 * in part order by a second, small launch: deterministic, same accuracy class, NOT bit-identical to the call without ws for
 * the rows of those tiles (one more association of the same products).  ws = NULL: gs_dense_fwd_rows_split. */
int gs_dense_fwd_rows_split_ws_bytes(int64_t* bytes_out_host);
int gs_dense_fwd_rows_split_ws(const float* X, int64_t ldx, const int32_t* idx, int32_t d, int64_t n_max, const int32_t* n_dev,
                               const void* W3, int32_t out_dim, int act, const float* bias, float* out, int64_t ldo,
                               float* ws, int64_t ws_bytes, void* stream);
/* ---- The same contraction on the fp16 matrix pipe with TWO pieces per operand (ABI 8, csrc/gs_split16.hip).
 * Why: the three-piece kernel runs the chip into its power cap (1400 W, engine clock down to 2.02 GHz:
 * profiles/r05_pool_clock_probe.txt), and its ~310 G MACs are most of that energy.  Here x 2^e = h + m + r with h = fp16(x 2^e),
 * m = fp16(x 2^e - h), round to nearest: |r| <= 2^-23 |x 2^e| -- at most ONE fp32 ulp: h keeps 11 bits, the residual has <= 12 of which
 * m keeps 11 (2^-25 on average) -- under a power-of-two scale per feature-table
 * row / weight column that puts its largest element at 2^13..2^14 (no overflow; m stays a normal fp16 for every element within
 * 2^-15 of the largest; below that the absolute error is <= 2^-25 in scaled units, 2^-38 of the largest element).  A product is
 * h h' + h m' + m h' (exact 11 x 11 bit products, fp32 accumulation; the dropped m m' is <= 2^-22 |x y| worst case, 2^-24 rms),
 * the scales are taken out exactly in the epilogue.  Over a K-term dot product what is given up is a random walk of sqrt(K)
 * 2^-23 against the K-term sum, one to two orders of magnitude below the rounding of the fp32 accumulation itself: measured
 * against fp64 the outputs are as accurate as the three-piece kernel's and more accurate than an fp32 FMA chain
 * (tests/test_split_gemm_gpu.py prints all three), at HALF the matrix-pipe work.  Inputs, outputs, accumulation: fp32; the
 * three-piece form stays available (GS_POOL_F16=0) and bench.py reports the step with both.
 *   gs_split_rows_f16: W [K, ldw >= N] fp32 -> W2 [KP / 8][2][N][8] fp16 + N int32 column exponents (KP = K rounded up to an even
 *     count of 32-k stages, zero beyond K); call it after every update of W (Engine.split_of(form="f16x2") does).
 *   gs_split_table_f16: a CONSTANT table X [rows, ldx >= d] -> X2 [rows][2][KP] fp16 + rows int32 row exponents, once (the
 *     reference's features are a non-trainable tf.Variable: models.py:299); 2 x 2 bytes per element = the fp32 table's bytes.
 *   gs_dense_fwd_rows_split16: out[i] = act(X[idx[i]] . W + bias), i < min(n_max, *n_dev), from X2 / W2 (aggregators.py:176-179 via
 *     layers.py:104-116 on the step's distinct ids): 128 x 256 workgroup tiles, both operand tiles are plain copies global -> LDS,
 *     24 MFMAs (v_mfma_f32_32x32x16_f16) per 16 fragment reads; ws as for gs_dense_fwd_rows_split_ws (nullable). */
int gs_split_rows_f16_bytes(int32_t K, int32_t N, int64_t* bytes_out_host);
int gs_split_rows_f16(const float* W, int64_t ldw, int32_t K, int32_t N, void* W2, void* stream);
int gs_split_table_f16_bytes(int64_t rows, int32_t d, int64_t* table_bytes_out_host, int64_t* exp_bytes_out_host);
int gs_split_table_f16(const float* X, int64_t ldx, int64_t rows, int32_t d, void* X2, int32_t* rexp, void* stream);
int gs_dense_fwd_rows_split16(const void* X2, const int32_t* rexp, const int32_t* idx, int32_t d, int64_t n_max, const int32_t* n_dev,
                              const void* W2, int32_t out_dim, int act, const float* bias, float* out, int64_t ldo, float* ws,
                              int64_t ws_bytes, void* stream);
int gs_split_rows(const float* W, int64_t ldw, int32_t K, int32_t N, void* W3, void* stream);

/* Input gradient:  dX[n, d] (+)= dZ[:, col0:col0+out_dim] · W[d, out_dim]^T */
int gs_dense_dgrad(const float* dZ, int64_t ldz, int32_t col0, int32_t out_dim, int64_t n,
                   const float* W, int64_t ldw, int32_t d, float* dX, int64_t ldx, int accumulate,
                   void* stream);

/* dZ = dY * (Y > 0) for relu (tf relu grad, aggregators.py:64), dY for identity.  In-place allowed. */
int gs_act_bwd(const float* dY, int64_t lddy, const float* Y, int64_t ldy, int64_t n, int32_t n_cols,
               int act, float* dZ, int64_t lddz, void* stream);
/* Bias gradient as slabs: slabs[z][c] = sum_{r in row slice z} Z[r, c]; sum them with gs_reduce_slabs
 * (rows = 1).  Deterministic.  slabs is [n_slabs, ld_slab]. */
int gs_colsum_slabs(const float* Z, int64_t ldz, int64_t n, int32_t n_cols, int32_t n_slabs,
                    float* slabs, int64_t ld_slab, void* stream);

/* General fp32 GEMM on the same MFMA kernel family (used by the operators above; exported for tests):
 *   C[M,N] = act( opA(A)·opB(B) + bias ),  opA = A^T if transA (A stored [K, M]), same for B.
 * a_row_idx gathers the SOURCE rows of A (rows of A as stored). */
int gs_gemm_f32(int transA, int transB, int64_t M, int32_t N, int64_t K,
                const float* A, int64_t lda, const int32_t* a_row_idx,
                const float* B, int64_t ldb,
                const float* bias, int act, float* C, int64_t ldc, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K4  pooling aggregators     replaces aggregators.py:176-181 (MaxPool) / :254-259 (MeanPool)
 * ------------------------------------------------------------------------------------------- */

/* Pooling MLP + reduce_max in ONE launch (aggregators.py:176-181):
 *   pooled[i, c] = max_j relu( X[idx[i*s + j]] . W[:, c] + bias[c] ),   argmax[i, c] = first j attaining it
 * The [n*s, hidden] activations are never written: a GEMM tile holds whole groups of s rows (s <= 64) and reduces them
 * in its epilogue.  Same results as gs_sage_dense_fwd(self = NULL) followed by gs_segment_max_fwd. */
int gs_dense_pool_max_fwd(const float* X, int64_t ldx, const int32_t* idx, int32_t d, int64_t n_groups, int32_t s,
                          const float* W, int64_t ldw, int32_t hidden, const float* bias, float* pooled, int64_t ldp,
                          int32_t* argmax, int64_t lda, void* stream);

/* The pooling MLP on the step's DISTINCT sampled ids (its output depends on the node id only; at Reddit's degree 37 % of a
 * step's 133 k sampled ids are duplicates):
 *   gs_unique_ids            ids [m] in [0, n_values) -> uniq [count] (ascending), inv [m] (position of ids[j] in uniq) and the
 *                            device word count, by flag array + prefix sum (deterministic, static launch shapes);
 *                            rank_ws: 2 * n_values int32 words whose FIRST n_values are zero on first use (every call leaves them
 *                            zero again: no clear launch; ABI 8), sums_ws: 256
 *   gs_dense_fwd_rows_dev    out[i] = act(X[idx[i]] . W + bias) for i < min(n_max, *n_dev): the row count is a device word
 *   gs_segment_max_gather_fwd  pooled[i, c] = max_j H[inv[i*s + j], c], argmax = first j attaining it: the bits of
 *                            gs_dense_pool_max_fwd on the expanded rows */
int gs_unique_ids(const int32_t* ids, int64_t m, int64_t n_values, int32_t* rank_ws, int32_t* sums_ws, int32_t* uniq_out,
                  int32_t* inv_out, int32_t* count_out, void* stream);
int gs_dense_fwd_rows_dev(const float* X, int64_t ldx, const int32_t* idx, int32_t d, int64_t n_max, const int32_t* n_dev,
                          const float* W, int64_t ldw, int32_t out_dim, int act, const float* bias, float* out, int64_t ldo,
                          void* stream);
int gs_segment_max_gather_fwd(const float* H, int64_t ldh, const int32_t* inv, int64_t n, int32_t s, int32_t hidden,
                              float* pooled, int64_t ldp, int32_t* argmax, int64_t lda, void* stream);

/* Attention pooling over each group's s sampled rows (graphsage_attn; csrc/gs_attn.hip).  Row j of group i is V_j =
 * H[inv[i*s + j]], or H[i*s + j] when inv == NULL; H is the output of the aggregator's relu-Dense and a [hidden] the gate:
 *   gs_segment_attn_fwd  t_j = <V_j, a>; alpha[i, j] = softmax_j(t_j) (maximum subtracted); pooled[i] = sum_j alpha[i, j] V_j.
 *                        One wave per group, one pass with a running maximum / sum / rescaled accumulator: every row of H is
 *                        read once, no [n*s, hidden] temporary, no atomics, bitwise repeatable.  alpha: [n, s], dense.
 *   gs_segment_attn_bwd  from dP = d_pooled [n, hidden]: g_j = <dP_i, V_j>, G = sum_j alpha_j g_j, dt_j = alpha_j (g_j - G),
 *                        dV[i*s + j] = (alpha_j dP_i + dt_j a) * (V_j > 0) (one row per SAMPLED row, the Dense's relu mask applied)
 *                        and da_slabs [n_slabs, hidden] (row stride hidden): partial sums of da = sum_{i,j} dt_j V_j, one slab
 *                        per workgroup, each fully written; their sum in slab order is da (the optimizer launch adds them as it
 *                        adds the weight gradients' slabs).  No float atomics; the same n_slabs gives the same bits.
 *   gs_attn_scores       H[r, hidden] = <H[r, :hidden], a> for every row: the logit column GS_CSR_SOFTMAX reads (ldh >= hidden + 4).
 * Range: hidden % 4 == 0, 4 <= hidden <= 1024, 1 <= s <= 128; GS_ENOTSUP otherwise.  a must be 16-byte aligned. */
int gs_segment_attn_fwd(const float* H, int64_t ldh, const int32_t* inv, const float* a, int64_t n, int32_t s, int32_t hidden,
                        float* pooled, int64_t ldp, float* alpha, void* stream);
int gs_segment_attn_bwd(const float* dP, int64_t ldd, const float* H, int64_t ldh, const int32_t* inv, const float* a,
                        const float* alpha, int64_t n, int32_t s, int32_t hidden, float* dV, int64_t ldv, float* da_slabs,
                        int32_t n_slabs, void* stream);
int gs_attn_scores(float* H, int64_t ldh, int64_t rows, int32_t hidden, const float* a, void* stream);

/* H[n*s, hidden] = relu(X[idx] · W_mlp + b_mlp)  (Dense, layers.py:104-116) is produced by
 * gs_sage_dense_fwd(self=NULL, agg=X, agg_idx=idx, ...).  This reduces it:
 *   pooled[i, c] = max_j H[i*s+j, c];  argmax[i, c] = first j attaining it   (reduce_max, :181) */
int gs_segment_max_fwd(const float* H, int64_t ldh, int64_t n, int32_t s, int32_t hidden,
                       float* pooled, int64_t ldp, int32_t* argmax, int64_t lda, void* stream);

/* dH[i*s+j, c] = (j == argmax[i,c] && pooled[i,c] > 0) ? d_pooled[i,c] : 0
 * (reduce_max gradient followed by the relu gradient of the Dense; ties: see DESIGN.md). */
int gs_segment_max_bwd(const float* d_pooled, int64_t ldd, const float* pooled, int64_t ldp,
                       const int32_t* argmax, int64_t lda, int64_t n, int32_t s, int32_t hidden,
                       float* dH, int64_t ldh, void* stream);

/* Sparse weight gradient of the MaxPool MLP when its input rows need no gradient (layer 0):
 *   slab[z][f, c] = sum_{g in slice z} v[g, c] * X[ids[g*s + argmax[g, c]], f],   v = d_pooled_masked
 * (d_pooled_masked = d_pooled * (pooled > 0), e.g. from gs_act_bwd).  Equals X[ids]^T · dH of the dense path
 * (gs_segment_max_bwd + gs_dense_wgrad) without materialising dH = [n*s, hidden]; ~s times fewer flops.
 * Needs 16*s <= 4*min(512, round_up(hidden,64)); returns GS_ENOTSUP otherwise.  slabs: [n_slabs, d, ld_slab]. */
int gs_maxpool_sparse_wgrad(const float* X, int64_t ldx, const int32_t* ids, int64_t n_groups, int32_t s, int32_t d,
                            const int32_t* argmax, int64_t lda, const float* d_pooled_masked, int64_t ldd,
                            int32_t hidden, int32_t n_slabs, float* slabs, int64_t ld_slab, void* stream);

/* Two-layer max-pool (TwoMaxLayerPoolingAggregator, aggregators.py:276-361): the gradient of the FIRST dense layer's
 * activations H1 from the gradient of the pooled SECOND layer, back through W2 and the first relu:
 *   dH1[i*s + j, k] = H1[h(i*s + j), k] > 0 ?  sum over { c : argmax[i, c] == j } of d_pooled_masked[i, c] * W2[k, c]  :  0
 * with d_pooled_masked = d_pooled2 * (pooled2 > 0) [n, hid2] (e.g. from gs_act_bwd), argmax [n, hid2] in [0, s) (a value
 * outside collects nowhere), W2 [hid1, hid2] as the Dense stores it, h(r) = h_idx[r], or r when h_idx is NULL (h_idx: the
 * `inv` of gs_unique_ids, H1 then holds one row per distinct node).  The sum runs in ascending c (columns whose
 * d_pooled_masked is exactly 0 are skipped), so two launches give the same bits; every row of dH1 [n*s, hid1] is written, a
 * row that won no column as zeros.  Equals gs_segment_max_bwd + gs_dense_dgrad + gs_act_bwd without the [n*s, hid2] matrix
 * and with 1/s of the flops.  Needs 1 <= s <= 64, hid1 % 4 == 0, hid2 % 4 == 0, hid2 <= 1024; GS_ENOTSUP otherwise.
 *   gs_pool2_transpose  out [cols, rows] = W [rows, cols]^T
 *   gs_pool2_iota       out[i] = i for i < n (the row index gs_maxpool_sparse_wgrad wants over an H1 with one row per sample)
 *   gs_pool2_dgrad_t    the kernel itself: reads W2T = W2^T [hid2, hid1] (rows coalesced along k)
 *   gs_pool2_dgrad      takes W2: makes the transposed copy for the call (allocates, transposes, launches, waits, frees);
 *                       not capturable into a graph -- a training step keeps W2T in a workspace and calls gs_pool2_dgrad_t */
int gs_pool2_transpose(const float* W, int64_t ldw, int32_t rows, int32_t cols, float* out, int64_t ldo, void* stream);
int gs_pool2_iota(int32_t* out, int64_t n, void* stream);
int gs_pool2_dgrad_t(const float* d_pooled_masked, int64_t ldd, const int32_t* argmax, int64_t lda, const float* W2T,
                     int64_t ldt, const float* H1, int64_t ldh, const int32_t* h_idx, int64_t n, int32_t s, int32_t hid1,
                     int32_t hid2, float* dH1, int64_t ldo, void* stream);
int gs_pool2_dgrad(const float* d_pooled_masked, int64_t ldd, const int32_t* argmax, int64_t lda, const float* W2, int64_t ldw,
                   const float* H1, int64_t ldh, const int32_t* h_idx, int64_t n, int32_t s, int32_t hid1, int32_t hid2,
                   float* dH1, int64_t ldo, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K5  supervised head         replaces supervised_models.py:85 (l2_normalize), :111-118 (losses),
 *                             :122-126 (predict)
 * ------------------------------------------------------------------------------------------- */

/* y = x * rsqrt(max(sum(x^2), 1e-12)) per row; inv_norm[n] saved for backward. */
int gs_l2norm_fwd(const float* x, int64_t ldx, int64_t n, int32_t d, float* y, int64_t ldy,
                  float* inv_norm, void* stream);
int gs_l2norm_bwd(const float* dy, int64_t lddy, const float* y, int64_t ldy, const float* inv_norm,
                  int64_t n, int32_t d, float* dx, int64_t lddx, void* stream);

/* Fused classification loss forward+backward on logits [n, C] with float labels [n, C]
 * (one-hot or multi-hot, the reference's feed contract, minibatch.py:264-274):
 *   sigmoid_loss == 0: softmax CE, loss_rows[r] = -sum_c z log p;  dlogits = (p*sum(z) - z)/n
 *   sigmoid_loss != 0: loss_rows[r] = sum_c (max(x,0) - x z + log1p(exp(-|x|)))/C ;
 *                      dlogits = (sigmoid(x) - z)/(n*C)
 * preds = softmax(logits) or sigmoid(logits) (supervised_models.py:122-126).
 * mean(loss_rows) is the classification loss of :112-118.  preds / dlogits may be NULL. */
int gs_class_loss(const float* logits, int64_t ldl, const float* labels, int64_t ldlab,
                  int64_t n, int32_t C, int sigmoid_loss,
                  float* loss_rows, float* preds, int64_t ldp, float* dlogits, int64_t lddl,
                  void* stream);

/* Fused head, forward AND backward in one launch (one wave per row, W staged in LDS):
 *   y = l2_normalize(x) (:85);  logits = y·W + b (:88-92);  loss_rows / preds / dlogits as gs_class_loss;
 *   dx = l2norm_bwd(dlogits·W^T)   (dx may be NULL for evaluation).  Supports d in {64,128,256,512}, C <= 128 and
 *   W fitting LDS; returns GS_ENOTSUP otherwise (callers then use the unfused kernels above). */
int gs_head_fwd_bwd(const float* x, int64_t ldx, int64_t n, int32_t d, const float* W, int64_t ldw,
                    const float* bias, const float* labels, int64_t ldlab, int32_t C, int sigmoid_loss,
                    float* y, int64_t ldy, float* logits, int64_t ldlo, float* preds, int64_t ldp,
                    float* dlogits, int64_t lddl, float* loss_rows, float* dx, int64_t lddx, void* stream);

/* ---------------------------------------------------------------------------------------------
 * N3  unsupervised objective   replaces models.py:336-343 (negative sampler), minibatch.py:113-132 (pair batches),
 *                              prediction.py:68-110 (BipartiteEdgePredLayer xent loss), models.py:393-405 (MRR)
 * ------------------------------------------------------------------------------------------- */

/* ids_out = [batch1 (B) | batch2 (B) | negatives (n_neg)]:
 *   pairs != NULL: batch1[i], batch2[i] = pairs[(*cursor_dev + i) % n_pairs]   (int32 [n_pairs, 2])
 *   cdf   != NULL: negatives drawn from the fixed unigram distribution ~ degree^0.75 with replacement
 *                  (tf.nn.fixed_unigram_candidate_sampler, unique=False): cdf is uint32 [n_nodes],
 *                  cdf[i] = floor(2^32 * P(node <= i)); draw = first i with cdf[i] > hash32(seed, *clock_dev, slot_offset + slot):
 *                  slot_offset = this rank's first global root (data-parallel ranks draw different negatives). */
int gs_unsup_stage(const int32_t* pairs, int64_t n_pairs, const uint64_t* cursor_dev, int64_t B,
                   const uint32_t* cdf, int64_t n_nodes, int32_t n_neg, uint64_t seed, const uint64_t* clock_dev,
                   int64_t slot_offset, int32_t* ids_out, void* stream);

/* Skip-gram cross-entropy head on the l2-normalised embeddings Y = [outputs1 (B) | outputs2 (B) | neg_outputs (n_neg)]:
 *   loss_rows[i] = xent(1, <o1_i,o2_i>) + neg_weight * sum_j xent(0, <o1_i,neg_j>)         (prediction.py:102-110)
 *   rr_rows[i]   = 1 / (1 + #{j : <o1_i,neg_j> >= <o1_i,o2_i>})                            (models.py:399-404)
 *   aff_all[i]   = [neg_aff_i (n_neg) | aff_i]  (optional, models.py:400)
 *   dY rows [0,2B) = scale * dLoss/dY;  the negatives' gradient arrives as ceil(B/4) slabs [n_neg, d] in neg_slabs
 *   (sum them with gs_reduce_slabs into dY rows [2B, 2B+n_neg)).  scale = 1/batch_size (models.py:378).
 * d in {64,128,256,512}; 5*n_neg*d*4 bytes must fit LDS. */
int gs_linkpred_fwd_bwd(const float* Y, int64_t ldy, int64_t B, int32_t d, int32_t n_neg, float neg_weight, float scale,
                        float* loss_rows, float* rr_rows, float* aff_all, int64_t ld_aff,
                        float* dY, int64_t lddy, float* neg_slabs, int32_t* n_slabs_out_host, void* stream);

/* The same objective FUSED with the normalisation on both sides (one launch + a 20-workgroup one instead of
 * l2norm_fwd | linkpred | reduce_slabs | l2norm_bwd):  Z [2B + n_neg, d] are the RAW aggregator outputs,
 *   Y = l2_normalize(Z) (models.py:368-370) is written (outputs1 / outputs2 / neg_outputs),
 *   loss_rows / rr_rows / aff_all as gs_linkpred_fwd_bwd on Y,
 *   dZ [2B + n_neg, d] = scale * dLoss/dZ (the gradient carried back through the normalisation; the negatives' rows are
 *   summed from ceil(B/4) per-workgroup slabs in neg_slabs [ceil(B/4), n_neg, d] in a fixed order). */
int gs_linkpred_norm_fwd_bwd(const float* Z, int64_t ldz, int64_t B, int32_t d, int32_t n_neg, float neg_weight, float scale,
                             float* Y, int64_t ldy, float* loss_rows, float* rr_rows, float* aff_all, int64_t ld_aff,
                             float* dZ, int64_t lddz, float* neg_slabs, void* stream);
/* ... and the step epilogue of gs_finalize_step2 as one more workgroup of its second launch (it only needs loss_rows /
 * rr_rows): loss_out[0] (+)= mean(loss_rows) (models.py:378), mrr_out[0] = mean(rr_rows) (models.py:404), then the device
 * counters c0..c2 (nullable) advance by d0..d2 -- one launch less per unsupervised step. */
int gs_linkpred_norm_fwd_bwd_step(const float* Z, int64_t ldz, int64_t B, int32_t d, int32_t n_neg, float neg_weight,
                                  float scale, float* Y, int64_t ldy, float* loss_rows, float* rr_rows, float* aff_all,
                                  int64_t ld_aff, float* dZ, int64_t lddz, float* neg_slabs, float* loss_out, int accumulate,
                                  float* mrr_out, uint64_t* c0, uint64_t d0, uint64_t* c1, uint64_t d1, uint64_t* c2,
                                  uint64_t d2, void* stream);

/* The head generalised over the loss (prediction.py:58-63) and the left operand (bilinear weights, prediction.py:68-92).
 * With a_i = affinity, n_ij = neg_cost and `scale` multiplying every gradient:
 *   GS_LP_LOSS_XENT      as gs_linkpred_fwd_bwd                                               (prediction.py:102-110)
 *   GS_LP_LOSS_SKIPGRAM  loss_i = a_i - log sum_j exp(n_ij)  (the reference's sign, prediction.py:112-117: minimising it
 *                        pushes pairs apart; the log-sum-exp has the row maximum subtracted);  d/da_i = 1,  d/dn_ij = -softmax_j
 *   GS_LP_LOSS_HINGE     loss_i = sum_j relu(n_ij - (a_i - margin))  (prediction.py:119-125);  m_ij = [n_ij - (a_i - margin) > 0],
 *                        d/dn_ij = m_ij,  d/da_i = -sum_j m_ij  (relu'(0) = 0)
 * neg_weight enters the xent loss only.  rr_rows / aff_all as gs_linkpred_fwd_bwd (from the same a_i / n_ij).
 *   U == NULL: X [2B + n_neg, d] are the RAW aggregator outputs; Y = l2_normalize(X) is written, the left operand is the
 *              normalised outputs1 and dX [2B + n_neg, d] = scale * dLoss/dX through the normalisation (dU is not used) --
 *              gs_linkpred_norm_fwd_bwd for every loss kind.
 *   U != NULL: X are the NORMALISED rows, U [B, d] is the left operand (l2_normalize(outputs1) . W, not unit-norm):
 *              a_i = <U_i, X_{B+i}>, n_ij = <U_i, X_{2B+j}>.  dU [B, d] = scale * dLoss/dU and rows [B, 2B + n_neg) of dX =
 *              scale * dLoss/d(normalised outputs2 | negatives) are written; rows [0, B) of dX are left alone (the caller
 *              forms dU . W^T there); Y is not used.
 * Two launches: the pairs (one wave per pair, ceil(B/4) workgroups, slabs of the negatives' gradient in
 * neg_slabs [ceil(B/4), n_neg, d]), then n_neg workgroups that sum the slabs in a fixed order (no float atomics).  The _step
 * form carries the epilogue of gs_linkpred_norm_fwd_bwd_step in the second launch.
 * d in {64,128,256,512}; 5*n_neg*d*4 bytes must fit 160 KB of LDS; X / dX / neg_slabs 16-byte aligned with ld % 4 == 0. */
#define GS_LP_LOSS_XENT 0
#define GS_LP_LOSS_SKIPGRAM 1
#define GS_LP_LOSS_HINGE 2
int gs_linkpred_loss_fwd_bwd(int32_t loss_kind, const float* X, int64_t ldx, const float* U, int64_t ldu, int64_t B, int32_t d,
                             int32_t n_neg, float neg_weight, float margin, float scale, float* Y, int64_t ldy,
                             float* loss_rows, float* rr_rows, float* aff_all, int64_t ld_aff, float* dX, int64_t lddx,
                             float* dU, int64_t lddu, float* neg_slabs, void* stream);
int gs_linkpred_loss_fwd_bwd_step(int32_t loss_kind, const float* X, int64_t ldx, const float* U, int64_t ldu, int64_t B,
                                  int32_t d, int32_t n_neg, float neg_weight, float margin, float scale, float* Y, int64_t ldy,
                                  float* loss_rows, float* rr_rows, float* aff_all, int64_t ld_aff, float* dX, int64_t lddx,
                                  float* dU, int64_t lddu, float* neg_slabs, float* loss_out, int accumulate, float* mrr_out,
                                  uint64_t* c0, uint64_t d0, uint64_t* c1, uint64_t d1, uint64_t* c2, uint64_t d2,
                                  void* stream);

/* The in-batch softmax (InfoNCE) head (csrc/gs_infonce.hip): every normalised outputs2 row of the batch and every sampled
 * negative is a candidate for every left-operand row.  X [2B + n_neg, d] are the NORMALISED rows, U [B, d] the left operand
 * (rows [0, B) of X themselves, or l2_normalize(outputs1) . W), C = rows [B, 2B + n_neg) of X:
 *   L_ij   = <U_i, C_j> / tau
 *   mask   : j < B, j != i and (ids2[j] == ids2[i] or ids2[j] == ids1[i]) -> candidate j is left out of row i (ids1 / ids2: the
 *            int32 node ids of the pairs, both given or both NULL = nothing masked; sampled negatives are never masked)
 *   loss_rows[i] = logsumexp_{j not masked} L_ij - L_ii
 *   dU = G . C,  rows [B, 2B + n_neg) of dX = G^T . U,   G = scale (softmax - I) / tau   (rows [0, B) of dX are left alone)
 *   aff_all [B, n_neg + 1] = [<U_i, neg_q> | <U_i, y2_i>] (raw, not divided by tau; required: the ranks are counted from it)
 *   and rr_rows as gs_linkpred_loss_fwd_bwd.
 * ws: fp32 workspace of gs_linkpred_infonce_ws_floats(B, d, n_neg, train) floats, 16-byte aligned: the rows' statistics
 * (maximum, log of the rescaled sum), the per-tile partial statistics and, when training, the partial gradients of the cut
 * sweeps.  dU == dX == NULL: forward only (train = 0; the same loss_rows / rr_rows / aff_all bits).  No float atomics, every
 * sum in a fixed order: bitwise repeatable.  The _step form carries the epilogue of gs_linkpred_norm_fwd_bwd_step, once.
 * d in {64,128,256,512}; B >= 1; n_neg >= 0 (no LDS bound; B + n_neg <= 65,535 * 128, refused beyond); tau in [0.01, 10];
 * X / U / dX / dU 16-byte aligned, ld % 4 == 0, ld >= d.  The workspace grows with B * (B + n_neg) / 64 floats (two per row and
 * candidate tile) plus at most 8 * (2B + n_neg) * d for the partial gradients. */
int gs_linkpred_infonce_ws_floats(int64_t B, int32_t d, int32_t n_neg, int train, int64_t* floats_out_host);
int gs_linkpred_infonce_fwd_bwd(const float* X, int64_t ldx, const float* U, int64_t ldu, int64_t B, int32_t d, int32_t n_neg,
                                float tau, float scale, const int32_t* ids1, const int32_t* ids2, float* loss_rows,
                                float* rr_rows, float* aff_all, int64_t ld_aff, float* ws, int64_t ws_floats, float* dX,
                                int64_t lddx, float* dU, int64_t lddu, void* stream);
int gs_linkpred_infonce_fwd_bwd_step(const float* X, int64_t ldx, const float* U, int64_t ldu, int64_t B, int32_t d,
                                     int32_t n_neg, float tau, float scale, const int32_t* ids1, const int32_t* ids2,
                                     float* loss_rows, float* rr_rows, float* aff_all, int64_t ld_aff, float* ws,
                                     int64_t ws_floats, float* dX, int64_t lddx, float* dU, int64_t lddu, float* loss_out,
                                     int accumulate, float* mrr_out, uint64_t* c0, uint64_t d0, uint64_t* c1, uint64_t d1,
                                     uint64_t* c2, uint64_t d2, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K6  optimizer              replaces supervised_models.py:95-99 (clip_by_value +-5, Adam) and the
 *                             weight-decay terms :104-108
 * ------------------------------------------------------------------------------------------- */

/* grad[i] = sum_{z<n_slabs} slabs[z*slab_stride + i] + weight_decay * w[i],  i < count.
 * Rows of the slab are [rows, ld_slab] and the destination is dense [rows, cols]. */
int gs_reduce_slabs(const float* slabs, int32_t n_slabs, int64_t slab_stride, int32_t rows, int32_t cols,
                    int64_t ld_slab, float weight_decay, const float* w, int64_t ldw,
                    float* grad, int64_t ldg, int accumulate, void* stream);

/* TF-1.x Adam on a flat buffer with elementwise clip (tf.clip_by_value, supervised_models.py:96):
 *   g = clamp(grad*grad_scale, -clip, clip) (clip <= 0 disables);  t = *step_dev + 1
 *   m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2
 *   p -= lr * sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v) + eps)          (epsilon OUTSIDE the sqrt) */
int gs_adam_step(float* p, const float* grad, float* m, float* v, int64_t count,
                 float lr, float beta1, float beta2, float eps, float clip, float grad_scale,
                 const uint64_t* step_dev, int32_t step_offset, void* stream);

/* Gradient finalisation over the whole flat parameter buffer in ONE launch:
 *   grads[i] = sum_{z < n_slabs(var)} slabs_var[z*size_var + (i - offset_var)] + (decay_var ? weight_decay*params[i] : 0)
 * and, when fuse_adam != 0, the clip + Adam update of gs_adam_step on the same element (single-GPU step).
 * vars_host: HOST array of per-variable descriptors (consumed at call time). */
typedef struct gs_var_desc {
    int64_t offset, size;  /* segment of the flat buffers, in floats (size includes ld padding) */
    float* slabs;
    int32_t n_slabs, decay;
    int32_t clear;         /* != 0: slab 0 is an atomically accumulated gradient (gs_scatter_add_rows); it is zeroed
                              after being read so that the next backward pass starts from 0 (needs n_slabs == 1) */
    int32_t reserved_;
} gs_var_desc;
/* step_offset: Adam's t = *step_dev + step_offset (1 when the counter is advanced AFTER this launch, 0 when an earlier
 * launch of the step -- gs_sage_tail_fwd_bwd -- already advanced it).  loss_rows (nullable): the step's scalar loss
 * loss_out[0] (+)= loss_scale * sum(loss_rows[0:loss_n]) is formed by workgroup 0 in a fixed order (replaces the
 * gs_finalize_step launch of a training step). */
int gs_flat_reduce_adam(const gs_var_desc* vars_host, int32_t n_vars, float* params, float* grads, float* m, float* v,
                        int64_t total, float weight_decay, int fuse_adam, float lr, float beta1, float beta2,
                        float eps, float clip, float grad_scale, const uint64_t* step_dev, int32_t step_offset,
                        const float* loss_rows, int64_t loss_n, float loss_scale, float* loss_out, int loss_accumulate,
                        void* stream);

/* gs_flat_reduce_adam + riders in ONE launch: the fan-out sampler of a LATER mini-batch (sampler_host, nullable: the
 * arguments of gs_sample_fanout_csr in a struct) and up to 6 gather+mean jobs of the NEXT mini-batch (as
 * gs_sage_dense_fwd_cogather).  The optimizer launch is a short latency-bound pass over ~1 MB of parameters; the
 * sampler (a chain of dependent round trips with almost no work) hides completely under it and the gather waves use
 * the idle wave slots.  The per-root id count of every kept hop must be <= 512 (else GS_ENOTSUP: launch
 * gs_sample_fanout_csr on its own). */
typedef struct gs_fanout_desc {
    const int64_t* rowptr; const int32_t* col; int64_t n_nodes;
    int32_t* ids_all; int64_t B;
    uint64_t seed, step; const uint64_t* step_dev;
    int64_t root_offset;
    const int32_t* order; int64_t n_order; const uint64_t* cursor_dev;
    const float* label_table; int64_t ld_table;
    float* labels_out; int64_t ld_out;
    int64_t offsets[4];
    int32_t fan[3];
    int32_t pad_id, n_hops, C;
    uint32_t hop0;
    int32_t law, max_degree;      /* GS_LAW_*, see gs_sample_uniform_csr */
    /* optional unsupervised root staging (pairs != NULL, exclusive with order): the roots are
     *   [pairs[e][0] (n_pair_roots) | pairs[e][1] (n_pair_roots) | n_neg negatives],  e = (*cursor_dev + i) % n_pairs,
     * B == 2 * n_pair_roots + n_neg; negative t = first node whose cdf exceeds the 32-bit draw of gs_unsup_stage
     * (neg_seed, *step_dev, t) -- same draws bit for bit; guide (nullable, 2^guide_bits + 1 entries: guide[b] = first
     * index with cdf > b << (32 - guide_bits)) only shortens the binary search. */
    const int32_t* pairs; int64_t n_pairs, n_pair_roots;
    const uint32_t* cdf; const int32_t* guide; int64_t n_cdf;
    int32_t n_neg, guide_bits;
    uint64_t neg_seed;
    /* GS_LAW_REFERENCE only, nullable: the law's virtual padded table materialised by gs_build_padded_table
     * ([n_nodes + 1, max_degree] int32, same seed / max_degree): a draw becomes one lookup table[id][column].  Same ids,
     * bit for bit, as without it. */
    const int32_t* padded_table;
    /* GS_LAW_REFERENCE only: the roots [0, seg_begin[0]) | [seg_begin[0], seg_begin[1]) | [seg_begin[1], B) come from
     * DIFFERENT sampler calls of the reference -- SampleAndAggregate._build runs sample(batch1), sample(batch2) and
     * sample(neg_samples) (models.py:347-357), each with its own tf.random_shuffle per hop (neigh_samplers.py:27) -- so
     * segment g uses the call ids hop0 + g * n_hops + h: six independent column permutations per unsupervised step.
     * {0, 0} = one call (supervised); with pair staging the boundaries default to {n_pair_roots, 2 * n_pair_roots}.
     * The staged negatives are keyed by root_offset + t, so data-parallel ranks draw different negatives. */
    int64_t seg_begin[2];
} gs_fanout_desc;
/* The padded adjacency table of minibatch.py:227-245 under GS_LAW_REFERENCE's keyed law, built ON THE DEVICE from the CSR:
 * table[v][c] = the c-th entry of node v's (frozen) padded row -- a keyed sample without replacement of max_degree
 * neighbors when deg > max_degree, max_degree keyed draws with replacement when deg < max_degree, the list itself when
 * equal; pad_id for degree-0 nodes and for row n_nodes.  table_out: [(n_nodes + 1) * max_degree] int32. */
int gs_build_padded_table(const int64_t* rowptr, const int32_t* col, int64_t n_nodes, int32_t pad_id, int32_t max_degree,
                          uint64_t seed, int32_t* table_out, void* stream);
/* gs_sample_fanout_csr from a descriptor (incl. the unsupervised root staging and the materialised table). */
int gs_sample_fanout_desc(const gs_fanout_desc* desc_host, void* stream);
int gs_flat_reduce_adam_sample(const gs_var_desc* vars_host, int32_t n_vars, float* params, float* grads, float* m, float* v,
                               int64_t total, float weight_decay, int fuse_adam, float lr, float beta1, float beta2,
                               float eps, float clip, float grad_scale, const uint64_t* step_dev, int32_t step_offset,
                               const float* loss_rows, int64_t loss_n, float loss_scale, float* loss_out, int loss_accumulate,
                               const gs_fanout_desc* sampler_host, const gs_gather_desc* jobs_host, int32_t n_jobs, void* stream);
/* gs_dense_wgrad_grouped_tiled3 with the fan-out sampler of a LATER mini-batch riding in the launch (ABI 10; sampler_host as gs_sample_fanout_desc takes
 * it, nullable; per-root id count of every kept hop <= 512, else GS_ENOTSUP).  The sampler is a chain of dependent round trips:
 * as a rider of the optimizer launch (gs_flat_reduce_adam_sample) it is what that launch waits for, here it ends long before
 * the contraction.  No problem may gather its rows (a_idx) through the id buffer that sampler fills -- GS_EINVAL; the private
 * copy gs_tail_desc.ids_copy_* makes is what the step's weight gradients read instead.  Same draws as the standalone launch. */
int gs_dense_wgrad_grouped_tiled3_sample(const gs_wgrad_desc* descs_host, int32_t n_desc, const gs_gather_desc* jobs_host,
                                         int32_t n_jobs, const gs_fanout_desc* sampler_host, void* stream);

/* Fused tail of the supervised two-layer GraphSAGE-mean model: layer 1 (MeanAggregator._call on the layer-0 outputs,
 * aggregators.py:43-64, identity act: last layer, models.py:307-310), l2_normalize + Dense head + loss/preds
 * (supervised_models.py:85-126) and their gradients down to dLoss/d(layer-0 pre-activations), ONE launch.  Every batch
 * row is independent given the weights: a workgroup takes 16 rows through the whole chain (fp32 MFMA 16x16x4).
 *   h0      [n + n*s, d_in]  relu outputs of layer 0: rows 0..n-1 = batch nodes, row n + i*s + j = j-th sample of node i
 *   means   [n, d_in], z [n, 2*out_dim] (pre-normalisation), y [n, 2*out_dim] (= outputs1), logits / preds / dlogits
 *           [n, C], loss_rows [n]: written (inputs of the weight-gradient launch and model outputs)
 *   train != 0: dz [n, 2*out_dim] = dLoss/dz and d_h0 [n + n*s, d_in] = relu'(h0) * dLoss/dh0 are written too
 *   c0..c2 (nullable device counters) are advanced by d0..d2 at the end of the launch.
 * Supported: concat, no aggregator bias, s <= 11, d_in in {128, 256}, out_dim in {64, 128}, C <= 128
 * (gs_sage_tail_supported);
 * anything else returns GS_ENOTSUP and the caller uses the per-operator entry points.
 *
 * Operand / output contract of every entry point of this section (gs_sage_tail_fwd_bwd[_means], gs_sage_tail_z[_means],
 * gs_sage_tail_dh0, gs_linkpred_tail[_means], gs_linkpred_tail_neg), as K3's:
 *   readable: operands are read as whole float4 / float2, so columns up to round_up(width, 4) of a row must be readable
 *     (W_head: ldwh >= round_up(C, 4)); of h0 the n + n*s rows; bias and labels the C logical elements only.
 *   may hold anything, NaN included (masks are selects, never products): every pad column -- of h0, W_self, W_neigh, W_head
 *     (columns [C, round_up(C, 4)) among them), labels, dz (gs_sage_tail_dh0), means (the *_means entries) --, h0 rows behind row
 *     n + n*s, the words behind the bias.  gcn: the pad is behind column 2*out_dim of the ONE matrix.
 *   written: the logical block of every output of the form; columns [C, round_up(C, 4)) of logits / preds / dlogits as
 *     zeros; d_h0 elements with h0 <= 0 (-0 included; a positive subnormal keeps its gradient) as +0; all n + n*s rows of d_h0.
 *     No other word: not the rows around a row-sliced output, not the columns from round_up(width, 4) on.
 *   untouched by form: means under the *_means entries; z and means in the z_ready launch (they are its inputs); dz and d_h0
 *     with train == 0 (gs_linkpred_tail*: neg_slabs too); logits / preds / aff_all when NULL; loss_out / mrr_out and the
 *     counters when loss_out == NULL; ids_copy_dst under z_ready; every output when an entry refuses its arguments (nothing is
 *     launched) or n == 0 (GS_OK).
 * tests/test_tail_edges_gpu.py holds this, and every stage to a float64 reference (tests/tail_oracle.py). */
typedef struct gs_tail_desc {
    const float* h0; int64_t ldh; int64_t n;
    const float* W_self; int64_t ldws;
    const float* W_neigh; int64_t ldwn;
    const float* W_head; int64_t ldwh;
    const float* b_head;
    const float* labels; int64_t ldlab;
    float* means; int64_t ldm;      /* (an INPUT of the *_means entry points) */
    float* z; int64_t ldz;
    float* y; int64_t ldy;
    float* logits; int64_t ldlo;
    float* preds; int64_t ldp;
    float* dlogits; int64_t lddl;
    float* loss_rows;
    float* dz; int64_t lddz;
    float* d_h0; int64_t lddh;
    uint64_t* c0; uint64_t d0;
    uint64_t* c1; uint64_t d1;
    uint64_t* c2; uint64_t d2;
    int32_t s, d_in, out_dim, C, sigmoid, train;
    uint32_t* sync;        /* [2 * G + 2 + 64 * G * out_dim] device words, G = ceil(n / 16), 8-byte aligned, zero-initialised ONCE by
                              the caller, private to one stream and to ONE n (ABI 10; in-kernel hand-over of the layer-1
                              pre-activations from the helper workgroups to the row-group workgroups): words [G, 2 G) = the
                              groups' launch epochs, word 2 G = an error word the caller should check when it fetches results
                              (bit 0: a row-group workgroup gave up waiting -- the wait is bounded), and from word 2 G + 2 on
                              G x 16 x 2*out_dim eight-byte granules {z element, epoch tag}.  May be NULL when z_ready != 0. */
    int32_t z_ready;       /* != 0: z and means were written by gs_sage_tail_z on this stream (split form): the launch has no
                              helper workgroups, no in-kernel hand-over and needs no sync buffer */
    int32_t gcn;           /* != 0: GCNAggregator form of layer 1 (aggregators.py:101-116; gs_sage_tail_fwd_bwd and gs_sage_tail_z):
                              ONE weight matrix W [d_in, 2*out_dim] passed as W_self = W, W_neigh = W + out_dim (same ld); both
                              column halves of z contract the mean over {neighbors} U {self} = (sum_j h_neigh_j + h_self)/(s+1),
                              which `means` receives; d_h0 rows (self and neighbors) = relu'(h0) * (dz . W^T) / (s + 1) */
    const int32_t* ids_copy_src; /* optional (ids_copy_n > 0; ABI 10): the launch's helper workgroups also copy ids_copy_n int32 from */
    int32_t* ids_copy_dst;       /* src to dst (gs_sage_tail_fwd_bwd without z_ready, or gs_sage_tail_z): the private copy of the step's */
    int64_t ids_copy_n;          /* node ids that the weight gradients gather through when the NEXT-next step's sampler rides in their launch */
} gs_tail_desc;
int gs_sage_tail_supported(int32_t d_in, int32_t out_dim, int32_t C);

/* Fused tail of the UNSUPERVISED two-layer mean model (models.py:362-405, prediction.py:68-110), two launches:
 *   gs_linkpred_tail      layer 1 (z helpers, as gs_sage_tail_fwd_bwd) -> main workgroups of 8 PAIRS each: l2_normalize
 *                         (models.py:368-370), affinities / xent loss / MRR rank (prediction.py:102-110, models.py:393-405), dY,
 *                         dz = l2norm'(dY) of the 2 B pair rows, [d_self | d_means] = dz . W^T, d_h0 = relu'(h0) * (...) of
 *                         their rows, and one slab [n_neg, 2*out_dim] per main of the negatives' gradient w.r.t. their
 *                         normalised rows; + gather jobs riding as extra workgroups (a long, thin launch: the rest of the
 *                         chip streams the next step's gather at the full HBM rate);
 *   gs_linkpred_tail_neg  the negatives' rows: slabs summed in main order -> dz -> d_h0 of their rows; + the step epilogue
 *                         (loss_out = mean(loss_rows) (+= if accumulate), mrr_out = mean(rr_rows), counters c0..c2 advanced
 *                         by d0..d2; loss_out == NULL: no epilogue) + the commit of the hand-over state + gather jobs riding (nine
 *                         workgroups of dependent round trips leave the chip free).  MUST follow every
 *                         gs_linkpred_tail on the same stream (train == 0: only the epilogue / commit run).
 * Rows: h0 [n + n*s, d_in] with n = 2 B + n_neg roots [batch1 | batch2 | negatives] (row n + i*s + j = j-th sample of root
 * i); z / y / dz [n, 2*out_dim]; means [n, d_in]; loss_rows / rr_rows [B]; aff_all [B, n_neg + 1] = [neg_aff | aff]
 * (nullable); neg_slabs [ceil(B / 8)][n_neg][2*out_dim]; sync: 2 * (ceil(B / 8) + ceil(n_neg / 16)) + 2 device words,
 * zero-initialised once, private to one stream (word 2 G = error flags as gs_tail_desc.sync).
 * Supported (gs_linkpred_tail_supported): d_in in {128, 256}, out_dim in {64, 128}, n_neg <= 32, s <= 11; concat, no bias. */
typedef struct gs_lp_tail_desc {
    const float* h0; int64_t ldh;
    int64_t B; int32_t n_neg, s, d_in, out_dim, train;
    const float* W_self; int64_t ldws;
    const float* W_neigh; int64_t ldwn;
    float* means; int64_t ldm;
    float* z; int64_t ldz;
    float* y; int64_t ldy;
    float* dz; int64_t lddz;
    float* d_h0; int64_t lddh;
    float* loss_rows; float* rr_rows;
    float* aff_all; int64_t ld_aff;
    float* neg_slabs;
    float neg_weight, scale;
    uint32_t* sync;
} gs_lp_tail_desc;
int gs_linkpred_tail_supported(int32_t d_in, int32_t out_dim, int32_t n_neg);
int gs_linkpred_tail(const gs_lp_tail_desc* desc_host, const gs_gather_desc* jobs_host, int32_t n_jobs, void* stream);
int gs_linkpred_tail_neg(const gs_lp_tail_desc* desc_host, float* loss_out, int accumulate, float* mrr_out, uint64_t* c0,
                         uint64_t d0, uint64_t* c1, uint64_t d1, uint64_t* c2, uint64_t d2, const gs_gather_desc* jobs_host,
                         int32_t n_jobs, void* stream);
/* Split form of the fused tail, first launch: the layer-1 pre-activations z = [h_self . W_self | mean(h_neigh) . W_neigh]
 * and the neighbor means of the descriptor (its head / label / gradient fields are ignored) as a LEAN kernel -- 4 x 64-column
 * helper workgroups per 16 rows, <= 128 VGPRs, 49 KB of LDS -- so that the gather jobs riding in the launch stream at the
 * full HBM rate, also on the CUs that run helpers (in the one-launch form every workgroup inherits the row-group
 * workgroups' 246 VGPRs / 88 KB and a CU holds one of them).  Follow with gs_sage_tail_fwd_bwd(desc with z_ready = 1).
 * Results are bit-identical to the one-launch form. */
int gs_sage_tail_z(const gs_tail_desc* desc_host, const gs_gather_desc* jobs_host, int32_t n_jobs, void* stream);
/* The matching backward half as a launch of its own (the fused kernel's last two phases): from dz = dLoss/dz [n, 2*out_dim],
 *   [d_self | d_means] = [dz[:, :out_dim] . W_self^T | dz[:, out_dim:] . W_neigh^T]      (aggregators.py:51-58 backward)
 *   d_h0 [n + n*s, d_in] = relu'(h0) * (d_self on row i, d_means / s on rows n + i*s + j)  (aggregators.py:48, :64)
 * instead of a small GEMM + gs_input_grad_pull.  Descriptor fields used: h0, W_self, W_neigh, dz, d_h0, n, s, d_in,
 * out_dim.  gs_sage_tail_z / gs_sage_tail_dh0 serve last mean layers of models that do not take the fused tail. */
int gs_sage_tail_dh0(const gs_tail_desc* desc_host, const gs_gather_desc* jobs_host, int32_t n_jobs, void* stream);
/* jobs_host / n_jobs (0..6): gather+mean jobs of the NEXT step co-scheduled in the launch (as gs_sage_dense_fwd_cogather):
 * the tail keeps n/16 CUs busy, the rest of the chip streams the gather meanwhile. */
int gs_sage_tail_fwd_bwd(const gs_tail_desc* desc_host, const gs_gather_desc* jobs_host, int32_t n_jobs, void* stream);
/* The three tail launches with `means` of the descriptor as an INPUT (added entry points, same descriptors): the layer-0 forward
 * that wrote h0 has written the layer-1 neighbor means as well (gs_sage_dense_fwd_tiled3_means, earlier on the same stream), so
 * the neighbor-term helper workgroups load 16 rows of means instead of 16 * s rows of h0 and do not write means.  Every output is
 * bit-identical to the plain entry's when means[i] = (((0 + h0[n + i*s]) + h0[n + i*s + 1]) + ...) * (1.f / s) in fp32, which is
 * what that forward writes.  gcn != 0 returns GS_ENOTSUP (the GCN mean includes the self row). */
int gs_sage_tail_fwd_bwd_means(const gs_tail_desc* desc_host, const gs_gather_desc* jobs_host, int32_t n_jobs, void* stream);
int gs_sage_tail_z_means(const gs_tail_desc* desc_host, const gs_gather_desc* jobs_host, int32_t n_jobs, void* stream);
int gs_linkpred_tail_means(const gs_lp_tail_desc* desc_host, const gs_gather_desc* jobs_host, int32_t n_jobs, void* stream);

/* Inverted dropout tf.nn.dropout(x, keep_prob = 1 - rate) (aggregators.py:46-47,104-105; layers.py:107): kept
 * elements are scaled by 1/keep_prob.  The keep mask is a counter hash of (seed, *clock_dev, site, row0 + row,
 * column), so forward and backward regenerate it and a replayed hipGraph draws new masks every step (clock_dev is the
 * device step counter).  A NULL descriptor or rate == 0 means "off". */
typedef struct gs_dropout {
    uint64_t seed;
    const uint64_t* clock_dev; /* device pointer, nullable (= 0) */
    uint32_t site;             /* distinct per dropout call site of a step */
    float rate;                /* in [0, 1) */
    int64_t row0;              /* global index of this call's first row */
    /* Parity-test hook (NULL in production): when set, the keep mask is READ from this device buffer instead of the
     * counter hash -- element (row0 + i, c) is kept iff keep_bits[(row0 + i) * keep_ld + c] != 0 -- so that a test can
     * feed the masks the reference run's tf.nn.dropout drew (aggregators.py:46-47, layers.py:107), like the sampler's
     * permutations.  4-byte aligned base, keep_ld % 4 == 0 and >= round_up(d, 4). */
    const uint8_t* keep_bits;
    int64_t keep_ld;
} gs_dropout;
/* out[i, :] = mask(row0 + i, :) * X[ids ? ids[i] : i, :] / keep_prob     (in place allowed when ids == NULL).
 * The same call is the backward of itself (X = upstream gradient). */
int gs_dropout_rows(const float* X, int64_t ldx, const int32_t* ids, int64_t n, int32_t d, const gs_dropout* drop,
                    float* out, int64_t ldo, void* stream);
/* K2 with dropout applied to every gathered neighbor row BEFORE the mean (aggregators.py:46-48):
 *   mean[i, :] = (1/s) * sum_j mask(row0 + i*s + j, :) * X[idx[i*s + j], :] / keep_prob
 * (self_src as in gs_gather_mean_fwd; the caller passes already-dropped self rows). */
int gs_gather_mean_dropout_fwd(const float* X, int64_t ldx, const int32_t* idx, int64_t n, int32_t s, int32_t d,
                               const float* self_src, int64_t ld_self, const int32_t* self_idx, float* mean,
                               int64_t ldm, const gs_dropout* drop, void* stream);

/* Trainable identity features ("node_embeddings", models.py:229-240 / supervised_models.py:49-60): gradient of the
 * layer-0 row gathers w.r.t. the leading `cols` columns of the gathered table, accumulated with fp32 atomics
 * (tf.gradients of embedding_lookup: IndexedSlices summed per id):
 *   table[ids[i*s + j], c] += scale * d[i, c]      i < n, j < s, c < cols */
int gs_scatter_add_rows(const float* d, int64_t ldd, int64_t n, int32_t s, int32_t cols, float scale,
                        const int32_t* ids, float* table, int64_t ldt, void* stream);
/* dst[r, 0:cols] = src[r, 0:cols]: refreshes the embedding columns of the combined feature table (the
 * tf.concat([embeds, features], axis=1) of models.py:240, kept materialised) after an optimizer step. */
int gs_copy_cols(const float* src, int64_t ld_src, float* dst, int64_t ld_dst, int64_t rows, int32_t cols, void* stream);

/* ---- LSTM aggregator (SeqAggregator, aggregators.py:363-449; ABI 11, csrc/gs_lstm.hip) ----------------------------------
 * TF 1.x BasicLSTMCell (gate order i, j, f, o; forget_bias 1.0 added at call time) under dynamic_rnn(sequence_length = L):
 *   [i j f o] = G[r, t] + h_{t-1} . W_h,  c_t = c_{t-1} sigma(f + 1) + sigma(i) tanh(j),  h_t = tanh(c_t) sigma(o),
 * zero initial state, steps t < L_r run, h_last[r] = h_{L_r - 1}.  G = X . W_x + b (the input projection of every step's row)
 * and all weight / input gradients are ordinary contractions (gs_sage_dense_fwd, gs_dense_wgrad*, gs_dense_dgrad).
 * One launch covers every hop of a layer: segment k holds n sequences of T steps; the step rows of sequence r of segment k
 * are row0 + r*T + t of the [rows, *] step arrays (G, A, C, H_prev, dG); its row of lengths / h_last / dh_last is
 * seq0 + r (seq0 = the sequences of the segments before it).  Hidden size H in {128, 256}.
 * gs_lstm_seg is 56 bytes on every target (checked at compile time here and by the binding). */
#define GS_LSTM_MAX_SEG 4
typedef struct gs_lstm_seg {
    const float* X;        /* gs_lstm_lengths only: the segment's input rows X[ids ? ids[i] : i], i < n*T */
    const int32_t* ids;    /* nullable */
    int64_t ldx;
    int64_t n;             /* sequences */
    int64_t row0;          /* first step row of the segment */
    int64_t seq0;          /* first sequence row of the segment (== sum of n of the segments before it) */
    int32_t T;             /* steps (>= 1) */
    int32_t reserved_;
} gs_lstm_seg;
/* lengths[seq0 + r] = max(1, #{t < T : some x[r, t, c] != 0, c < d})     (aggregators.py:411-414) */
int gs_lstm_lengths(const gs_lstm_seg* segs_host, int32_t n_seg, int32_t d, int32_t* lengths, void* stream);
/* Forward recurrence.  W_h: [H, 4H]; G: [rows, 4H] pre-activations from the input projection; writes the activated gates
 * A [rows, 4H] (A may alias G), the cell states C [rows, H], the previous hidden states H_prev [rows, H] (0 for t >= L_r)
 * and h_last [n_total, H].  Step rows t >= L_r of A and C are left untouched. */
int gs_lstm_fwd(const gs_lstm_seg* segs_host, int32_t n_seg, int32_t H, const float* W_h, int64_t ldw, const int32_t* lengths,
                const float* G, int64_t ldg, float* A, int64_t lda, float* C, int64_t ldc, float* H_prev, int64_t ldhp,
                float* h_last, int64_t ldh, void* stream);
/* Backward recurrence (BPTT) from dh_last [n_total, H]: dG [rows, 4H] = d loss / d(pre-activations), zero for t >= L_r
 * (dG may alias A).  W_hT_ws: caller scratch of 4H * H floats (W_h^T, written by the launch). */
int gs_lstm_bwd(const gs_lstm_seg* segs_host, int32_t n_seg, int32_t H, const float* W_h, int64_t ldw, float* W_hT_ws,
                const int32_t* lengths, const float* A, int64_t lda, const float* C, int64_t ldc, const float* dh_last,
                int64_t lddh, float* dG, int64_t lddg, void* stream);

/* Input gradient of one aggregator layer w.r.t. the previous layer's hidden rows, in ONE launch ("pull" form: every
 * output row sums the contributions it receives, so no accumulation order is involved):
 *   out[r, :] = relu'(mask_y[r, :]) * ( [r < n_self] d_self[r, :]
 *                                       + sum_k [row0_k <= r < row0_k + n_k*s_k] scale_k * src_k[(r - row0_k) / s_k, :] )
 * Segment k is the reverse of a segmented mean over s_k rows (scale 1/s_k), of a GCN self term (s = 1, scale
 * 1/(s+1)) or of a plain row copy (s = 1, scale 1).  Replaces gs_act_bwd + one gs_mean_bwd per hop. */
#define GS_PULL_MAX 6
typedef struct gs_pull_desc {
    const float* d_self;   /* [n_self, ld_self], nullable */
    int64_t ld_self, n_self;
    int32_t n_seg, d;
    const float* src[GS_PULL_MAX];
    int64_t ld_src[GS_PULL_MAX], row0[GS_PULL_MAX], n[GS_PULL_MAX];
    int32_t s[GS_PULL_MAX];
    float scale[GS_PULL_MAX];
    const float* mask_y;   /* [rows, ldy] activations of the previous layer (relu mask), nullable */
    int64_t ldy;
    float* out;            /* [rows, ldo] */
    int64_t ldo, rows;
} gs_pull_desc;
int gs_input_grad_pull(const gs_pull_desc* desc_host, void* stream);

/* gs_finalize_step with a second mean in the same launch: aux_out[0] = aux_scale * sum(aux_rows[0:n]) (the unsupervised
 * model's mrr, models.py:404). */
int gs_finalize_step2(const float* loss_rows, int64_t n, float scale, float* loss_out, int accumulate,
                      const float* aux_rows, float aux_scale, float* aux_out, uint64_t* c0, uint64_t d0, uint64_t* c1,
                      uint64_t d1, uint64_t* c2, uint64_t d2, void* stream);

/* Up to three device counters advanced by one launch (cursor / sampler clock / optimizer step). */
int gs_advance_counters(uint64_t* c0, uint64_t d0, uint64_t* c1, uint64_t d1, uint64_t* c2, uint64_t d2, void* stream);

/* Step epilogue in one launch: loss_out[0] (+)= scale * sum(loss_rows[0:n]) (skipped if loss_rows == NULL), then
 * the (non-NULL) counters are advanced. */
int gs_finalize_step(const float* loss_rows, int64_t n, float scale, float* loss_out, int accumulate,
                     uint64_t* c0, uint64_t d0, uint64_t* c1, uint64_t d1, uint64_t* c2, uint64_t d2, void* stream);

/* batch[i] = order[(*cursor + i) % n_order];  labels_out[i, :C] = label_table[batch[i], :C]   (one launch;
 * replaces minibatch.py:264-274 + 302-307 for the device-resident epoch). */
int gs_stage_batch(const int32_t* order, int64_t n_order, const uint64_t* cursor_dev, int64_t n, int32_t* batch,
                   const float* label_table, int64_t ld_table, int32_t C, float* labels_out, int64_t ld_out,
                   void* stream);

/* out[0] = scale * sum_{i<count} x[i]   (single block, deterministic order) */
int gs_sum_scaled(const float* x, int64_t count, float scale, float* out, int accumulate, void* stream);
/* out[0] (+)= scale * sum x[i]^2  -- weight_decay * tf.nn.l2_loss(var), supervised_models.py:106 */
int gs_sumsq_scaled(const float* x, int64_t count, float scale, float* out, int accumulate, void* stream);

/* ---------------------------------------------------------------------------------------------
 * C1  gradient all-reduce over RCCL / xGMI (data-parallel training; the reference is single-device,
 * supervised_train.py:55-59).  One process per GPU; ONE in-place sum over the flat fp32 gradient buffer per step,
 * enqueued on `stream` and capturable into the step's hipGraph.  RCCL is bound at run time (dlopen) -- the copy
 * already mapped in the process is reused.
 *   gs_comm_unique_id : rank 0 fills a >= 128-byte HOST buffer which the host code ships to every rank
 *                       (torch.distributed / MPI / a file -- not this library's business)
 *   gs_comm_init_rank : collective over all ranks; uses the calling thread's current HIP device
 *   gs_comm_available : GS_OK iff RCCL can be bound in this process -- ranks agree on this over their bootstrap
 *                       transport BEFORE any of them enters the collective gs_comm_init_rank
 *   gs_comm_count     : ncclCommCount of the communicator (a run can report the size RCCL really has)
 * ------------------------------------------------------------------------------------------- */
#define GS_COMM_ID_BYTES 128
int gs_comm_available(void);
int gs_comm_count(void* comm, int32_t* n_ranks_out_host);
int gs_comm_unique_id(void* id_out_host, int32_t len);
int gs_comm_init_rank(void** comm_out, int32_t nranks, int32_t rank, const void* id_host, int32_t len);
int gs_comm_allreduce_sum_f32(void* comm, float* buf, int64_t count, void* stream);
int gs_comm_destroy(void* comm);

/* ---------------------------------------------------------------------------------------------
 * C2: the same exchange as direct peer stores over xGMI (opt-in; gs_comm_* stays the default).  The flat gradient is
 * 0.9 MB: instead of a ring (2(N-1) latency-bound hops) every rank stores slice p of its gradient straight into rank
 * p's window (reduce-scatter, N-1 links in parallel), rank p sums the N copies IN RANK ORDER and stores the sum into
 * every rank's window (all-gather): one hop out, one hop back, ONE kernel launch on `stream`, capturable into the
 * step's hipGraph.  Windows are uncached device memory owned by this library and shared with hipIpcMemHandle.
 *   gs_peer_create        : allocates this rank's window for an n_floats buffer (chunks: workgroups per peer, 0 = sized
 *                           so that a thread moves ~2 float4 per pass, <= 256 workgroups in all; spin_limit: polls before
 *                           a wait gives up, 0 = 2^24, of the order of ten seconds)
 *   gs_peer_export/attach : the 64-byte IPC handle of the own window / maps rank `peer_rank`'s window (the host code
 *                           ships handles between processes -- torch.distributed / MPI / a file)
 *   gs_peer_attach_local  : another rank of the SAME process, by object (several streams or devices in one process)
 *   gs_peer_allreduce_sum_f32 : in-place sum over ranks; every rank ends with identical bits
 *   gs_peer_status        : epochs completed and the error word (0 ok; bit 0: a peer's copies never arrived, bit 1: a
 *                           reduced slice never arrived, bits 8..: the ranks waited for in vain) -- every device-side
 *                           wait is bounded, a missing peer cannot hang the GPU; the error is sticky (later exchanges
 *                           return at once, the buffer untouched): re-create the windows
 * ------------------------------------------------------------------------------------------- */
#define GS_PEER_HANDLE_BYTES 64
int gs_peer_create(int64_t n_floats, int32_t world, int32_t rank, int32_t chunks, int64_t spin_limit, void** peer_out);
int gs_peer_export(void* peer, void* handle_out_host, int32_t len);
int gs_peer_attach(void* peer, int32_t peer_rank, const void* handle_host, int32_t len);
int gs_peer_attach_local(void* peer, void* other_peer);
int gs_peer_allreduce_sum_f32(void* peer, float* buf, int64_t count, void* stream);
int gs_peer_status(void* peer, int64_t* epoch_out_host, int32_t* error_out_host);
int gs_peer_destroy(void* peer);

/* ---------------------------------------------------------------------------------------------
 * hipGraph helpers: the per-step kernel chain is captured once and replayed (no tracing compiler).
 * ------------------------------------------------------------------------------------------- */
int gs_stream_create(void** stream_out);
/* Diagnostics: one wave sleeping `us` microseconds on `stream` (the stand-in for a latency-bound collective when the
 * data-parallel step schedule is probed on one GPU; bench.py GS_PROBE_DP_SCHEDULE). */
int gs_spin_us(float us, void* stream);
int gs_stream_destroy(void* stream);
int gs_stream_sync(void* stream);
int gs_capture_begin(void* stream);
int gs_capture_end(void* stream, void** graph_exec_out);
int gs_graph_launch(void* graph_exec, void* stream);
int gs_graph_destroy(void* graph_exec);
/* hipEvent timing on `stream` (torch.cuda.Event only sees torch's current stream). */
int gs_event_create(void** ev_out);
int gs_event_record(void* ev, void* stream);
/* Makes `stream` wait for `ev` (fork/join of a second stream; inside a capture this becomes a graph edge). */
int gs_stream_wait_event(void* stream, void* ev);
int gs_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms_out_host); /* synchronises ev_stop */
int gs_event_destroy(void* ev);

/* ---------------------------------------------------------------------------------------------
 * N2V  node2vec / DeepWalk baseline   replaces models.py:408-504 (Node2VecModel): trainable target / context embedding tables
 *      [n_rows, d] and a context bias [n_rows], gathered, scored and updated in place by plain SGD.  A step is
 *      gs_n2v_stage | gs_n2v_fwd_bwd | gs_n2v_apply; no float atomics, the tables are never copied or densified, row offsets
 *      are 64-bit.  ids = [batch1 (B) | batch2 (B) | negatives (n_neg)], every id in [0, n_rows) (the caller checks).
 *      d in {64, 128, 256, 512}; n_neg as gs_n2v_supported says (the negatives' rows and one partial-gradient image per
 *      pair of the workgroup share LDS: 20 fit at every d).
 * ------------------------------------------------------------------------------------------- */

/* gs_unsup_stage with n_neg DISTINCT negatives (tf.nn.fixed_unigram_candidate_sampler(unique=True), models.py:449-456):
 * the first n_neg distinct nodes of gs_unsup_stage's stream of draws (draw t keyed by slot_offset + t, t = 0, 1, ...).
 * The cdf must reach at least n_neg nodes (the caller checks; TensorFlow would spin for ever).  *status (nullable, device)
 * is set to 1 if the stream was given up after 2^18 draws; the missing slots then repeat the first node.
 * guide (nullable): int32 [2^guide_bits + 1], guide[b] = first index whose cdf exceeds b << (32 - guide_bits), clipped to
 * n_nodes - 1, as in gs_fanout_desc: the same draws from a search of a few entries instead of log2(n_nodes) dependent loads. */
int gs_n2v_stage(const int32_t* pairs, int64_t n_pairs, const uint64_t* cursor_dev, int64_t B, const uint32_t* cdf,
                 int64_t n_nodes, int32_t n_neg, uint64_t seed, const uint64_t* clock_dev, int64_t slot_offset,
                 const int32_t* guide, int32_t guide_bits, int32_t* ids_out, int32_t* status, void* stream);

/* 1 if (d, n_neg) is a shape the launches below take, else 0.  gs_n2v_slabs: the number of [n_neg, d] slabs (and [n_neg]
 * bias slabs) gs_n2v_fwd_bwd writes for B pairs, 0 if unsupported. */
int gs_n2v_supported(int32_t d, int32_t n_neg);
int gs_n2v_slabs(int64_t B, int32_t d, int32_t n_neg);

/* With o1 = target[batch1[i]], o2 = context[batch2[i]], neg_q = context[neg[q]] and scale = 1/B:
 *   aff_all[i]   = [<o1, neg_q> (n_neg) | <o1, o2>]            WITHOUT the bias (models.py:489-500, prediction.py)
 *   rr_rows[i]   = 1 / (1 + #{q : <o1, neg_q> >= <o1, o2>})    (the convention of gs_linkpred_fwd_bwd)
 *   loss_rows[i] = xent(1, <o1,o2> + bias[batch2[i]]) + sum_q xent(0, <o1,neg_q> + bias[neg[q]])     (models.py:477-487)
 *   outputs1[i]  = o1
 * train != 0 also writes the gradient rows of scale * sum_i loss_rows[i] (dense, ld = d):
 *   g_target [B, d]  w.r.t. target[batch1[i]];   g_ctx [B, d], g_bias [B]  w.r.t. context / bias[batch2[i]];
 *   neg_slabs [gs_n2v_slabs, n_neg, d], bias_slabs [gs_n2v_slabs, n_neg]: per-workgroup partial sums over the batch of the
 *   gradient w.r.t. context / bias[neg[q]]  (summed in a fixed order by gs_n2v_apply).
 * train == 0 (evaluation, embedding export) writes no gradient; the five buffers may be NULL. */
int gs_n2v_fwd_bwd(const float* target, int64_t ldt, const float* context, int64_t ldc, const float* bias, int64_t n_rows,
                   const int32_t* ids, int64_t B, int32_t d, int32_t n_neg, int train, float* loss_rows, float* rr_rows,
                   float* aff_all, int64_t ld_aff, float* outputs1, int64_t ldo, float* g_target, float* g_ctx, float* g_bias,
                   float* neg_slabs, float* bias_slabs, void* stream);

/* tf.train.GradientDescentOptimizer on the indexed slices of gs_n2v_fwd_bwd (a launch of its own: every read of the step's
 * rows precedes every write): for each destination row ONE owner -- the first slot holding that id, slots ordered
 * batch1 for the target table and [negatives | batch2] for the context table and the bias -- adds the staged rows of all
 * slots with the same id in ascending slot order and performs one p -= lr * sum.  O(touched rows); bitwise reproducible.
 * loss_rows != NULL: an extra workgroup writes loss_out = mean(loss_rows), mrr_out = mean(rr_rows) and advances the
 * device counters (*c0 += d0, *c1 += d1; nullable). */
int gs_n2v_apply(float* target, int64_t ldt, float* context, int64_t ldc, float* bias, int64_t n_rows, const int32_t* ids,
                 int64_t B, int32_t d, int32_t n_neg, float lr, const float* g_target, const float* g_ctx, const float* g_bias,
                 const float* neg_slabs, const float* bias_slabs, int32_t n_slabs, const float* loss_rows,
                 const float* rr_rows, float* loss_out, float* mrr_out, uint64_t* c0, uint64_t d0, uint64_t* c1, uint64_t d1,
                 void* stream);

/* ---------------------------------------------------------------------------------------------
 * INF  full-neighborhood inference: a variable-degree segmented reduce over a CSR adjacency (rowptr int64 [n_rows + 1],
 *      col int32 [nnz], as gs_sample_uniform_csr), for the rows of a window [row0, row0 + n):
 *        GS_CSR_MEAN       out[r - row0] = sum_e X[col[e]] / deg                       (aggregators.py:48, all neighbors)
 *        GS_CSR_MEAN_SELF  out[r - row0] = (sum_e X[col[e]] + X[r]) / (deg + 1)        (the GCN mean, aggregators.py:96-99)
 *        GS_CSR_MAX        out[r - row0] = max_e X[col[e]]                             (no arg-max: inference only)
 *      over e in [rowptr[r], rowptr[r+1]); duplicate entries count as often as they occur; an empty row gives 0 (X[r] for
 *      GS_CSR_MEAN_SELF); act = GS_ACT_RELU applies relu to the result.  fp32 rows, ld >= round_up(d, 4); columns at and
 *      beyond round_up(d, 4) and rows outside the window are not written.
 *      The launch follows a work-item plan built once per graph by the caller (graphsage_amd/inference.py):
 *        items  int64 [n_items][4] = (row, first edge, count <= split_len, partial slot or -1), rows ascending, every row at
 *               least one item (count 0 for an empty row); a row longer than split_len is cut into items of at most
 *               split_len edges, numbered by consecutive partial slots;
 *        splits int64 [n_split][3] = (row, first partial slot, partials) of those rows, rows ascending.
 *      [item0, item1), [split0, split1) and [slot0, slot1) are the window's ranges.  Partials go to ws (gs_csr_reduce_ws_bytes
 *      for slot1 - slot0 slots) and a second launch combines each long row's partials in slot order: no float atomics, a fixed
 *      order of additions, bitwise reproducible.  EVERY col entry must lie in [0, n_rows) and x_rows >= n_rows: the caller
 *      checks its graph once (the kernel does not look at the ids again).
 *      gs_csr_reduce_desc is 200 bytes on every target (checked at compile time and by the binding; passed by pointer, not
 *      part of gs_abi_struct_sizes).
 * ------------------------------------------------------------------------------------------- */
#define GS_CSR_MEAN 0
#define GS_CSR_MEAN_SELF 1
#define GS_CSR_MAX 2
/*      GS_CSR_SOFTMAX    out[r - row0] = sum_e softmax_e(X[col[e]][d]) * X[col[e]][:d]      (attention pooling, all neighbors)
 *      The logit of table row r is column d of X, the column right behind the d value columns: ldx >= round_up(d + 1, 4)
 *      (gs_attn_scores fills it).  The maximum is subtracted; an empty row gives 0; a duplicate entry counts as often as it
 *      occurs.  A partial of a cut row carries (max, sum, accumulator) and the combine launch rescales the partials to their
 *      common maximum in slot order; size the workspace with gs_csr_reduce_ws_bytes(n_slots, d + 4). */
#define GS_CSR_SOFTMAX 3
typedef struct gs_csr_reduce_desc {
    const int64_t* rowptr;     /* device [n_rows + 1] */
    const int32_t* col;        /* device [nnz] */
    const int64_t* items;      /* device [n_items][4] */
    const int64_t* splits;     /* device [n_split][3]; nullable when n_split == 0 */
    const float* X;            /* [x_rows, ldx] */
    float* out;                /* [n, ldo]: row r of the window is out row r - row0 */
    float* ws;                 /* partials of the window's long rows; nullable when it has none */
    int64_t n_rows, nnz, n_items, n_split;
    int64_t ldx, x_rows, ldo, ws_bytes;
    int64_t row0, n;
    int64_t item0, item1, split0, split1, slot0, slot1;
    int32_t d, op, act, split_len;
} gs_csr_reduce_desc;
int gs_csr_reduce_ws_bytes(int64_t n_slots, int32_t d, int64_t* bytes_out_host);
int gs_csr_reduce_fwd(const gs_csr_reduce_desc* desc_host, void* stream);

/* ---------------------------------------------------------------------------------------------
 * INF-ROWS  exact inference for a node SUBSET: the receptive field on the device, and the reduce over a row list.
 *
 *      gs_frontier_expand: rows_in is an ascending, duplicate-free int32 list [m] of rows in [0, n_rows) of the CSR;
 *        rows_out = the ascending, duplicate-free list of rows_in U {col[e] : e in a row of rows_in}   (at most rows_out_cap)
 *        pos[id]  = index of id in rows_out, -1 for every id in [0, n_rows) that is no member           (int32 [n_rows])
 *        count[0] = the number of members                                                             (device word)
 *      A flag array written with plain stores of one value, then a block count and a rank pass (the method of
 *      gs_unique_ids): no atomics, no sort, a deterministic result.  One wave walks one input row, its edges spread over the
 *      lanes.  ws = int32 [n_rows + 256] (gs_frontier_ws_bytes), 16-byte aligned; its first n_rows words must be ZERO on first
 *      use and every call leaves them zero.  Entries of rows_in or col outside [0, n_rows) are skipped.
 *
 *      gs_csr_reduce_rows: the ops and the optional relu of gs_csr_reduce_fwd over the rows of a plan that covers a row subset
 *      (items / splits as above, cut from the graph's plan in its order, partial slots re-based to 0 .. n_slots):
 *        out[out_pos[r]] = reduce over e of X[x_pos[col[e]]]        (GS_CSR_MEAN_SELF: the self row is X[x_pos[r]])
 *      x_pos, out_pos: int32 [n_rows] maps from node id to table row; x_pos == NULL means X is indexed by node id (then
 *      x_rows >= n_rows).  The item loop and the combine are the code of gs_csr_reduce_fwd, so a row gets bit for bit the value
 *      the window form gives it.  An id outside [0, n_rows) or a mapped position outside [0, x_rows) / [0, out_rows) makes the
 *      wave give its item up: an uncut row is then not written (a cut row combines what its partial slot held), and nothing
 *      outside the tables is touched.
 *      gs_frontier_desc is 96 and gs_csr_rows_desc 168 bytes on every target (checked at compile time and by the binding;
 *      passed by pointer, not part of gs_abi_struct_sizes).
 * ------------------------------------------------------------------------------------------- */
typedef struct gs_frontier_desc {
    const int64_t* rowptr;     /* device [n_rows + 1] */
    const int32_t* col;        /* device [nnz] */
    const int32_t* rows_in;    /* device [m]; nullable when m == 0 */
    int32_t* rows_out;         /* device [rows_out_cap] */
    int32_t* pos;              /* device [n_rows] */
    int32_t* count;            /* device [1] */
    int32_t* ws;               /* device [n_rows + 256] */
    int64_t n_rows, nnz, m, rows_out_cap, ws_bytes;
} gs_frontier_desc;
int gs_frontier_ws_bytes(int64_t n_rows, int64_t* bytes_out_host);
int gs_frontier_expand(const gs_frontier_desc* desc_host, void* stream);

typedef struct gs_csr_rows_desc {
    const int64_t* rowptr;     /* device [n_rows + 1] */
    const int32_t* col;        /* device [nnz] */
    const int64_t* items;      /* device [n_items][4] */
    const int64_t* splits;     /* device [n_split][3]; nullable when n_split == 0 */
    const int32_t* x_pos;      /* device [n_rows]; NULL: X is indexed by node id */
    const int32_t* out_pos;    /* device [n_rows] */
    const float* X;            /* [x_rows, ldx] */
    float* out;                /* [out_rows, ldo] */
    float* ws;                 /* partials of the list's long rows; nullable when it has none */
    int64_t n_rows, nnz, n_items, n_split, n_slots;
    int64_t ldx, x_rows, ldo, out_rows, ws_bytes;
    int32_t d, op, act, split_len;
} gs_csr_rows_desc;
int gs_csr_reduce_rows(const gs_csr_rows_desc* desc_host, void* stream);

/* ---------------------------------------------------------------------------------------------
 * RANK link ranking against every node: a contraction with a compare-and-count epilogue; no score is written to memory.
 *        t[q]    = <Xq[q], Zc[dst[q]]>                                   (fp32 on the matrix cores, fp32 operands)
 *        n_gt[q] = #{w in C_q : <Xq[q], Zc[w]> >  t[q]}
 *        n_eq[q] = #{w in C_q : <Xq[q], Zc[w]> == t[q]}
 *      C_q = {0 <= w < n_cand} without dst[q], without src[q] (if src is given and flags lacks GS_RANK_KEEP_SRC) and without
 *      the filter row of src[q] (if a filter is given; it needs src, which only indexes it under GS_RANK_KEEP_SRC).  dst[q] may lie at or beyond n_cand; dst and src entries must lie in [0, n_rows) (the
 *      caller checks them once).  The filter is a CSR over the table's rows: f_rowptr int64 [n_rows + 1], f_col int32
 *      [f_nnz], strictly ascending within each row, entries in [0, n_rows).
 *      t comes out of the sweep's own tile code run on the dst-gathered rows, so a candidate row that is bit-identical to
 *      Zc[dst[q]] scores bit-equal to t[q] and is counted in n_eq.  d is a multiple of 4 in [4, 1024]; ld >= d.
 *      The grid runs over (query tile of 128) x (candidate slice); per-slice counts go to the int32 workspace
 *      [slices][Q][2] and a second small launch sums them: integers only, bitwise reproducible, no atomics.
 *      gs_rank_ws_bytes(Q, n_cand) = slices * Q * 2 * sizeof(int32_t), where, with tiles = ceil(n_cand / 128) and
 *      q_tiles = max(1, ceil(Q / 128)):  tiles_per_slice = min(16384, max(4, ceil(tiles / max(1, ceil(2048 / q_tiles))))),
 *      slices = max(1, ceil(tiles / tiles_per_slice)).  Callers with many queries pass them in chunks (the binding: 65,536)
 *      so that the workspace does not grow with Q.
 *      gs_rank_desc is 144 bytes on every target (checked at compile time and by the binding; passed by pointer, not part
 *      of gs_abi_struct_sizes).
 * ------------------------------------------------------------------------------------------- */
#define GS_RANK_KEEP_SRC 1     /* gs_rank_desc.flags: src[q] stays a candidate (src is then only the filter's row index) */
typedef struct gs_rank_desc {
    const float* Xq;           /* device [Q][ldq] query rows */
    const float* Zc;           /* device [n_rows][ldz] candidate table */
    const int32_t* dst;        /* device [Q]: table row of the true partner */
    const int32_t* src;        /* device [Q]: table row of the query node; nullable */
    const int64_t* f_rowptr;   /* device [n_rows + 1]; nullable (with f_col) */
    const int32_t* f_col;      /* device [f_nnz] */
    float* t;                  /* device [Q] */
    int32_t* n_gt;             /* device [Q] */
    int32_t* n_eq;             /* device [Q] */
    void* ws;                  /* device, 8-byte aligned, ws_bytes >= gs_rank_ws_bytes(Q, n_cand) */
    int64_t Q, ldq, n_rows, n_cand, ldz, f_nnz, ws_bytes;
    int32_t d, flags;          /* flags: 0 or GS_RANK_KEEP_SRC */
} gs_rank_desc;
int gs_rank_ws_bytes(int64_t Q, int64_t n_cand, int64_t* bytes_out_host);
int gs_rank_count(const gs_rank_desc* desc_host, void* stream);

/* ---------------------------------------------------------------------------------------------
 * TOPK the k best-scoring partners of every query among all nodes: the sweep of gs_rank_count with a select epilogue; no score
 *      row is written to memory.
 *        C_q     = {0 <= w < n_cand} without src[q] (if src is given and flags lacks GS_RANK_KEEP_SRC) and without the filter
 *                  row of src[q] (filter and src as in gs_rank_desc; there is no dst)
 *        s(q, w) = <Xq[q], Zc[w]>                                        (the arithmetic of gs_rank_count, bit for bit: s(q, w)
 *                  equals the t that gs_rank_count returns for dst[q] = w)
 *        ids[q], scores[q] = the first count[q] = min(k, |C_q|) members of C_q in the total order (s descending, w ascending)
 *                  and their scores; entries at and beyond count[q] are -1 / -inf.  A score of -0.0f is reported as +0.0f.
 *      Inputs are finite by contract (a NaN score lands at an unspecified position).  1 <= k <= GS_TOPK_MAX; d is a multiple
 *      of 4 in [4, 1024]; ld >= d; ids and scores are dense [Q][k].  src entries must lie in [0, n_rows).
 *      Per (slice, query) the first launch keeps an unsorted list of at most cap = 64 * (1 + ceil(k / 64)) uint64 keys
 *      (score bits mapped monotonically to unsigned in the high half, ~w in the low half) and its length; a second launch
 *      merges the slices.  Compares only: bitwise reproducible, no atomics.
 *      gs_topk_ws_bytes(Q, n_cand, k) = slices * Q * (8 * cap + 4) with the slices of gs_rank_ws_bytes.  Callers with many
 *      queries pass them in chunks (the binding: 65,536).
 *      gs_topk_desc is 144 bytes on every target (checked at compile time and by the binding; passed by pointer).
 * ------------------------------------------------------------------------------------------- */
#define GS_TOPK_MAX 128
typedef struct gs_topk_desc {
    const float* Xq;           /* device [Q][ldq] query rows */
    const float* Zc;           /* device [n_rows][ldz] candidate table */
    const int32_t* src;        /* device [Q] or NULL: table row of the query node */
    const int64_t* f_rowptr;   /* device [n_rows + 1] or NULL */
    const int32_t* f_col;      /* device [f_nnz] or NULL (with f_rowptr) */
    int32_t* ids;              /* device [Q][k] */
    float* scores;             /* device [Q][k] */
    int32_t* count;            /* device [Q] */
    void* ws;                  /* device, 8-byte aligned, ws_bytes >= gs_topk_ws_bytes(Q, n_cand, k) */
    int64_t Q, ldq, n_rows, n_cand, ldz, f_nnz, ws_bytes;
    int32_t d, k, flags;       /* flags: 0 or GS_RANK_KEEP_SRC */
} gs_topk_desc;
int gs_topk_ws_bytes(int64_t Q, int64_t n_cand, int32_t k, int64_t* bytes_out_host);
int gs_topk_select(const gs_topk_desc* desc_host, void* stream);

/* ---------------------------------------------------------------------------------------------
 * WALK second-order (p, q) random walks of node2vec over a CSR adjacency (rowptr int64 [n_nodes + 1], col int32 [nnz], every
 *      row ASCENDING; duplicates allowed and drawn as often as they are stored).  The job is the walk list
 *      g = 0 .. n_starts * num_walks - 1, walk g starting at starts[g / num_walks]; one call runs the n_walks walks
 *      g = walk0 .. walk0 + n_walks - 1 and its outputs are indexed by i = g - walk0.  The stream of walk g depends on
 *      (seed, g) only: a job cut into several calls gives the walks of one call.
 *        paths[i][0] = start; paths[i][j], 1 <= j < walk_len, the node after j steps.
 *        Step j from v (previous node t; none before the first move): a node with no row entries keeps the walk where it is
 *        and leaves t as it was.  Otherwise attempt a = 0, 1, .. draws h = mix64(walkkey + 256 j + a) with
 *        walkkey = mix64(seed ^ GS_WALK_TAG) + g * 0xD1342543DE82EF95 (mix64: the sampler's splitmix64 finalizer), takes
 *        x = col[rowptr[v] + (((h >> 32) * deg) >> 32)] and accepts it iff (h & 0xFFFFFFFF) < thr, where thr = 2^32 when there
 *        is no t, thr_return when x == t, thr_common when x occurs in t's row (binary search, at most 32 probes), thr_far
 *        otherwise.  Attempt 255 is taken whatever it draws.  On a move t = v, v = x.
 *        thr_* = floor(w / wmax * 2^32) for the weights w = (1/p, 1, 1/q): the largest must be exactly 2^32 and the smallest
 *        at least 2^28 (min(w) / wmax >= 1/16: a step then reaches the cap with probability <= (15/16)^256); else GS_EINVAL.
 *        No float reaches the kernel.  With all three at 2^32 the search is skipped; the walks are the same.
 *        A start id outside [0, n_nodes) gives a row of -1 and counts[i] = 0.  A col entry outside [0, n_nodes) can be walked
 *        to but never from (it has no row), and appears in paths and pairs as it is stored.
 *        counts[i] = #{1 <= j < walk_len : paths[i][j] != paths[i][0]}   (utils.py:87-88: no self co-occurrences)
 *      gs_walk_paths writes paths (ld_paths >= walk_len) and counts.  The caller forms offsets = the exclusive prefix sum of
 *      counts (int64 [n_walks]); gs_walk_pairs then writes pairs[offsets[i] + k] = (paths[i][0], k-th position of walk i that
 *      differs from it), rows at or beyond pairs_cap are not written.  One lane per walk in both launches, integers only, no
 *      atomics: bitwise reproducible.  gs_walk_desc is 152 bytes on every target (checked at compile time and by the binding;
 *      passed by pointer, not part of gs_abi_struct_sizes).
 * ------------------------------------------------------------------------------------------- */
#define GS_WALK_TAG 0xA700000000000000ull      /* domain tag of the walk stream (the sampler's tags: gs_sample_dev.h) */
#define GS_WALK_ATTEMPTS 256
#define GS_WALK_MAX_LEN 4096
typedef struct gs_walk_desc {
    const int64_t* rowptr;     /* device [n_nodes + 1] */
    const int32_t* col;        /* device [nnz] */
    const int32_t* starts;     /* device [n_starts]: the whole job's start ids */
    int32_t* paths;            /* device [n_walks][ld_paths] */
    int32_t* counts;           /* device [n_walks]; gs_walk_paths only */
    const int64_t* offsets;    /* device [n_walks]; gs_walk_pairs only */
    int32_t* pairs;            /* device [pairs_cap][2]; gs_walk_pairs only */
    int64_t n_nodes, nnz, n_starts, walk0, n_walks, ld_paths, pairs_cap;
    uint64_t seed, thr_return, thr_common, thr_far;
    int32_t num_walks, walk_len;
} gs_walk_desc;
int gs_walk_paths(const gs_walk_desc* desc_host, void* stream);
int gs_walk_pairs(const gs_walk_desc* desc_host, void* stream);

/* ---------------------------------------------------------------------------------------------
 * IMPORTANCE importance neighborhoods (PinSage): the neighborhood of a start u is the set of nodes that short random walks
 *      from u visit most often, and the table row of u stores each of them as often as its share of the visits asks.  Input
 *      is what gs_walk_paths wrote: paths int32 [n_starts * num_walks][ld_paths], the walks of start i in rows
 *      i * num_walks .. (i + 1) * num_walks - 1.  Output: table int32 [n_starts][slots] (dense) and stats int32 [n_starts][2].
 *      The rule for start i, integers only:
 *        1. u = paths[i * num_walks][0].  u outside [0, n_nodes) (the walker's row of -1): the row is all pad_id, stats (0, 0).
 *        2. A visit is x = paths[i * num_walks + r][j], 0 <= r < num_walks, 1 <= j < walk_len; it is KEPT iff 0 <= x < n_nodes
 *           and x != u (a stored pad id, -1 and the start itself never become neighbors).
 *        3. c(x) = the kept visits of x, m = the distinct x.  m == 0: the row is all pad_id, stats (0, 0).
 *        4. The selected set: the first min(m, top) nodes in the order (c descending, id ascending).
 *        5. Largest remainder over the selected set: C = sum c; q_k = floor(c_k * slots / C), r_k = c_k * slots - q_k * C;
 *           rest = slots - sum q_k; the first `rest` selected nodes in the order (r descending, id ascending) get one more
 *           slot.  (c * slots <= 2^22; rest is smaller than the number of non-zero remainders, so the rule is total.)
 *        6. Row i holds the selected ids ascending, id k repeated n_k times: exactly `slots` entries, ids with n_k == 0 absent.
 *           stats[i] = (m, #{k : n_k > 0}).
 *      A CSR whose non-empty rows hold exactly max_degree = slots entries is used as it stands by GS_LAW_REFERENCE and a
 *      repeated entry is drawn as often as it is stored, so an entry stored n times weighs n / slots in the sampled mean and
 *      in the exact one (csr_reduce over the table): importance pooling by multiplicity, no other kernel involved.
 *      Limits, checked before any launch (else GS_EINVAL): num_walks >= 1, walk_len >= 2, V = num_walks * (walk_len - 1) <=
 *      GS_IMPORTANCE_MAX_VISITS, 1 <= top <= GS_IMPORTANCE_MAX_TOP, 1 <= slots <= GS_IMPORTANCE_MAX_SLOTS, ld_paths >= walk_len,
 *      0 <= n_nodes <= 2^31 - 1, reserved_ == 0; n_starts == 0 is a no-op.  pad_id is any int32.
 *      One wave per start, sorts in LDS, ONE kernel form for every V (no switch point); no atomics, no floats: bitwise
 *      reproducible (csrc/gs_importance.hip).  gs_importance_desc is 72 bytes on every target (checked at compile time and
 *      by the binding; passed by pointer, not part of gs_abi_struct_sizes).
 * ------------------------------------------------------------------------------------------- */
#define GS_IMPORTANCE_MAX_VISITS 4096
#define GS_IMPORTANCE_MAX_TOP 4096
#define GS_IMPORTANCE_MAX_SLOTS 1024
typedef struct gs_importance_desc {
    const int32_t* paths;      /* device [n_starts * num_walks][ld_paths] */
    int32_t* table;            /* device [n_starts][slots] */
    int32_t* stats;            /* device [n_starts][2]: (distinct kept nodes, nodes with a slot) */
    int64_t n_starts, n_nodes, ld_paths;
    int32_t num_walks, walk_len, top, slots, pad_id, reserved_;   /* reserved_: 0 */
} gs_importance_desc;
int gs_importance_table(const gs_importance_desc* desc_host, void* stream);

/* ---------------------------------------------------------------------------------------------
 * LOGREG one loss-and-gradient evaluation of a one-vs-rest logistic regression on rows of an embedding table (the downstream
 *      node classification of eval_scripts/: SGDClassifier(loss="log") per class; csrc/gs_logreg.hip).  With
 *        z[i][k] = <X[rows[i]], W[:, k]> + b[k]   (fp32 on the matrix cores),   s[i][k] = +1 / -1,   m = s z
 *      where s comes from y_class (int32 [n] in [0, c): +1 for the row's class, -1 for every other class) or from y_multi
 *      (uint8 [n][ldy]: +1 where the entry is non-zero):
 *      GS_LOGREG_FIT writes three fp64 arrays -- sums over the rows, NOT means, and without any regulariser:
 *        loss[k]  = sum_i max(-m, 0) + log1p(exp(-|m|))            (= log(1 + exp(-m)), safe at both ends)
 *        gb[k]    = sum_i r[i][k],   r = -s sigma(-m)
 *        gW[j][k] = sum_i X[rows[i]][j] r[i][k]                    (dense [d][c])
 *      GS_LOGREG_PREDICT forms the logits only and writes, where the pointer is given, pred_class[i] = argmax_k z[i][k]
 *      (int32 [n], the lowest class id on an exact tie), pred_multi[i][k] = z[i][k] > 0 (uint8 [n][ldp]) and, if labels are
 *      given too, loss.  gW, gb (PREDICT) and pred_* (FIT) must be null.
 *      rows is nullable (rows 0 .. n-1 of X); entries may repeat and must lie in [0, n_rows) (the caller checks them once).
 *      Exactly one label form in FIT mode; none or one in PREDICT mode.  d % 4 == 0, 4 <= d <= GS_LOGREG_MAX_D,
 *      1 <= c <= GS_LOGREG_MAX_C, n >= 1, ldx >= d (ldx % 4 == 0, X 16-byte aligned), ldw, ldy, ldp >= c; anything else is
 *      refused with a message and no launch.
 *      A workgroup owns a contiguous run of 32-row tiles, keeps the gathered tile in LDS for both contractions and writes one
 *      fp32 partial; a second launch adds the partials in workgroup order in fp64.  No n x c array exists in memory, no
 *      atomics: bitwise repeatable.  gs_logreg_ws_bytes(n, d, c) = wgs * (2 c + d c) * 4 with tiles = ceil(n / 32),
 *      wgs = ceil(tiles / ceil(tiles / 512)); the workspace is needed whenever loss is written.
 *      gs_logreg_desc is 168 bytes on every target (checked at compile time and by the binding; passed by pointer, not part
 *      of gs_abi_struct_sizes).
 * ------------------------------------------------------------------------------------------- */
#define GS_LOGREG_FIT 0
#define GS_LOGREG_PREDICT 1
#define GS_LOGREG_MAX_D 512
#define GS_LOGREG_MAX_C 128
typedef struct gs_logreg_desc {
    const float* X;            /* device [n_rows][ldx] embedding table */
    const int32_t* rows;       /* device [n] rows of X; nullable (0 .. n-1) */
    const float* W;            /* device [d][ldw] */
    const float* b;            /* device [c] */
    const int32_t* y_class;    /* device [n]; nullable */
    const uint8_t* y_multi;    /* device [n][ldy]; nullable */
    double* loss;              /* device [c]; FIT: required, PREDICT: nullable (needs labels) */
    double* gW;                /* device [d][c]; FIT only */
    double* gb;                /* device [c]; FIT only */
    int32_t* pred_class;       /* device [n]; PREDICT only, nullable */
    uint8_t* pred_multi;       /* device [n][ldp]; PREDICT only, nullable */
    void* ws;                  /* device, 8-byte aligned, ws_bytes >= gs_logreg_ws_bytes(n, d, c); needed with loss */
    int64_t n, n_rows, ldx, ldw, ldy, ldp, ws_bytes;
    int32_t d, c, mode, flags; /* mode: GS_LOGREG_FIT | GS_LOGREG_PREDICT; flags: 0 */
} gs_logreg_desc;
int gs_logreg_ws_bytes(int64_t n, int32_t d, int32_t c, int64_t* bytes_out_host);
int gs_logreg_eval(const gs_logreg_desc* desc_host, void* stream);

/* ---------------------------------------------------------------------------------------------
 * LOGREG, joined  the same evaluation on rows that are formed from TWO tables and standardised while they are staged (the
 *      `feat` and features + embeddings inputs of eval_scripts/: hstack, StandardScaler, then the regression).  Row i is
 *        x[i][j] = ((j < da ? Xa[rows_a[i]][j] : Xb[rows_b[i]][j - da]) - mu[j]) * inv[j],    0 <= j < d = da + db
 *      one fp32 subtract, then one fp32 multiply (the scaler is NOT folded into W and b: that cancels for a column whose mean
 *      is large against its spread).  mu and inv (fp32 [d], 16-byte aligned) are given together or both null (no affine).
 *      Source B is absent when Xb, rows_b, ldb, db and n_rows_b are all null / zero.  rows_a and rows_b are independent, each
 *      nullable (rows 0 .. n-1 of its table), entries may repeat and must lie in [0, n_rows_a) / [0, n_rows_b).
 *      da % 4 == 0, db % 4 == 0, da >= 4, 4 <= d <= GS_LOGREG_JOINED_MAX_D, lda >= da, ldb >= db; W is [d][ldw], gW [d][c].
 *      Everything else -- modes, labels, outputs, the arithmetic after staging, the order of every sum -- is gs_logreg_eval's
 *      (the two kernels share their device code, csrc/gs_logreg_dev.h): with B absent, mu null and d <= GS_LOGREG_MAX_D every
 *      output is bit-equal to gs_logreg_eval on the same inputs.  gs_logreg_joined_ws_bytes is gs_logreg_ws_bytes' formula
 *      with d up to GS_LOGREG_JOINED_MAX_D.  Anything else is refused with a message and no launch.
 *      gs_logreg_joined_desc is 224 bytes on every target (checked at compile time and by the binding; passed by pointer, not
 *      part of gs_abi_struct_sizes).
 *
 *      gs_col_moments writes the column means and POPULATION variances of the same joined rows, without any affine, as fp64
 *      mean[d] and var[d]: centred (the means first, then the squares of x - mean), no atomics, a fixed summation order,
 *      bitwise repeatable; a column whose selected entries are all equal has var == 0.0 exactly.  ws: device, 8-byte aligned,
 *      ws_bytes >= GS_COL_MOMENTS_MAX_CHUNKS * d * 8.  (StandardScaler: scale = sqrt(var), 1 where var == 0; the caller
 *      uploads mu = mean and inv = 1 / scale as fp32.)
 * ------------------------------------------------------------------------------------------- */
#define GS_LOGREG_JOINED_MAX_D 1024
#define GS_COL_MOMENTS_MAX_CHUNKS 256
typedef struct gs_logreg_joined_desc {
    const float* Xa;           /* device [n_rows_a][lda] source A: columns [0, da) */
    const int32_t* rows_a;     /* device [n] rows of Xa; nullable (0 .. n-1) */
    const float* Xb;           /* device [n_rows_b][ldb] source B: columns [da, da + db); NULL: absent */
    const int32_t* rows_b;     /* device [n] rows of Xb; nullable (0 .. n-1) */
    const float* mu;           /* device [d]; nullable (with inv) */
    const float* inv;          /* device [d]; nullable (with mu) */
    const float* W;            /* device [d][ldw] */
    const float* b;            /* device [c] */
    const int32_t* y_class;    /* device [n]; nullable */
    const uint8_t* y_multi;    /* device [n][ldy]; nullable */
    double* loss;              /* device [c]; FIT: required, PREDICT: nullable (needs labels) */
    double* gW;                /* device [d][c]; FIT only */
    double* gb;                /* device [c]; FIT only */
    int32_t* pred_class;       /* device [n]; PREDICT only, nullable */
    uint8_t* pred_multi;       /* device [n][ldp]; PREDICT only, nullable */
    void* ws;                  /* device, 8-byte aligned, ws_bytes >= gs_logreg_joined_ws_bytes(n, d, c); needed with loss */
    int64_t n, n_rows_a, lda, n_rows_b, ldb, ldw, ldy, ldp, ws_bytes;
    int32_t da, db, c, mode, flags, reserved_; /* mode: GS_LOGREG_FIT | GS_LOGREG_PREDICT; flags, reserved_: 0 */
} gs_logreg_joined_desc;
int gs_logreg_joined_ws_bytes(int64_t n, int32_t d, int32_t c, int64_t* bytes_out_host);
int gs_logreg_eval_joined(const gs_logreg_joined_desc* desc_host, void* stream);
int gs_col_moments(const float* Xa, const int32_t* rows_a, int64_t lda, int32_t da, int64_t n_rows_a,
                   const float* Xb, const int32_t* rows_b, int64_t ldb, int32_t db, int64_t n_rows_b, int64_t n,
                   double* mean, double* var, void* ws, int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * KMEANS Lloyd's k-means over the rows of an embedding table (csrc/gs_kmeans.hip): squared norms, the fused assignment, and the
 *      stable grouping of rows by cluster.  The centroid update is gs_csr_reduce_fwd (GS_CSR_MEAN) over (rowptr, members).
 *
 *      gs_kmeans_sqnorm: out[i] = sum_j X[rows ? rows[i] : i][j]^2 over fp32 rows, i < n.  One wave per row: every lane adds
 *      the squares of its float4 columns in ascending column order (fmaf chain), then the xor butterfly; the order of the
 *      additions is fixed, so two bit-identical rows give the same bits.  d % 4 == 0, 4 <= d <= 1024, ld >= d.
 *
 *      gs_kmeans_assign: with the table rows x_i = X[rows ? rows[i] : i], i < n, and the centroids c_j = C[j], j < k,
 *        s(i, j)   = <x_i, c_j> - 0.5f * csq[j]             (the sweep of gs_rank_count: fp32 on the matrix cores, the same
 *                                                             k-ordered chain for every cell; then ONE fp32 subtract)
 *        assign[i] = argmax_j s(i, j), an exact tie going to the LOWEST j  (= argmin_j |x_i - c_j|^2 when csq[j] = |c_j|^2)
 *        dist[i]   = max(0, xsq[i] - 2 s(i, assign[i]))      (dist nullable; xsq nullable: taken as 0)
 *        stats     = { double inertia = sum_i dist[i];  int64 changed = #{i : assign[i] != prev[i]} }   (16 bytes; prev
 *                    nullable: changed = 0)
 *      One workgroup takes 128 rows and sweeps every centroid tile of 128, keeping a running (best score, id) in registers;
 *      no score is written to memory.  It writes one fp64 partial of sum dist and one int64 partial of the changed count to
 *      ws ([workgroups][2] words of 8 bytes, gs_kmeans_assign_ws_bytes(n) = 16 * ceil(n / 128)); a second launch of one
 *      workgroup adds them in workgroup order (256 contiguous runs, each in order, then the runs in order).  No atomics:
 *      bitwise repeatable.  Two bit-identical centroid rows score bit-equal.  Inputs are finite by contract (a NaN score never
 *      wins; a row whose scores are all NaN gets 0).  1 <= k <= GS_KMEANS_MAX_K, d % 4 == 0, 4 <= d <= 1024, ld, ldc >= d,
 *      1 <= n < 2^31; rows entries must lie in [0, n_rows) (the caller checks them once; the kernel clamps).
 *
 *      gs_kmeans_members: the stable grouping.  From assign int32 [n] it writes rowptr int64 [k + 1] (rowptr[j + 1] -
 *      rowptr[j] = the members of cluster j) and members int32 [n]: cluster j's run holds rows[i] (i when rows is NULL) for
 *      its members in ascending i.  Entries of assign outside [0, k) are skipped (rowptr[k] is then below n).  Per-chunk
 *      histograms, a scan over the chunks and over the clusters, and an ordered re-walk: integers only, no global atomics,
 *      and a result that does not depend on `chunk`, the entries one wave walks (0: the default, 2048; else a multiple of 64).
 *      ws: int32 [ceil(n / chunk)][k] (gs_kmeans_members_ws_bytes(n, k, chunk)), 4-byte aligned.  n < 2^31.
 *      gs_kmeans_desc is 128 and gs_kmeans_members_desc 72 bytes on every target (checked at compile time and by the
 *      binding; passed by pointer, not part of gs_abi_struct_sizes).
 * ------------------------------------------------------------------------------------------- */
#define GS_KMEANS_MAX_K 4096
#define GS_KMEANS_CHUNK 2048
typedef struct gs_kmeans_desc {
    const float* X;            /* device [n_rows][ld] table */
    const int32_t* rows;       /* device [n] rows of X; nullable (0 .. n-1) */
    const float* C;            /* device [k][ldc] centroids */
    const float* csq;          /* device [k]: |c_j|^2 (gs_kmeans_sqnorm) */
    const float* xsq;          /* device [n]: |x_i|^2 by position i; nullable */
    const int32_t* prev;       /* device [n]: the previous assignment; nullable */
    int32_t* assign;           /* device [n] */
    float* dist;               /* device [n]; nullable */
    void* stats;               /* device, 8-byte aligned, 16 bytes: double inertia, int64 changed */
    void* ws;                  /* device, 8-byte aligned, ws_bytes >= gs_kmeans_assign_ws_bytes(n) */
    int64_t n, n_rows, ld, ldc, ws_bytes;
    int32_t k, d;
} gs_kmeans_desc;
typedef struct gs_kmeans_members_desc {
    const int32_t* assign;     /* device [n] */
    const int32_t* rows;       /* device [n]; nullable (the members are 0 .. n-1) */
    int64_t* rowptr;           /* device [k + 1] */
    int32_t* members;          /* device [n] */
    int32_t* ws;               /* device, ws_bytes >= gs_kmeans_members_ws_bytes(n, k, chunk) */
    int64_t n, ws_bytes;
    int32_t k, chunk;          /* chunk: 0 (GS_KMEANS_CHUNK) or a positive multiple of 64 */
    int64_t reserved_;         /* 0 */
} gs_kmeans_members_desc;
int gs_kmeans_sqnorm(const float* X, int64_t ld, int64_t n_rows, const int32_t* rows, int64_t n, int32_t d, float* out,
                     void* stream);
int gs_kmeans_assign_ws_bytes(int64_t n, int64_t* bytes_out_host);
int gs_kmeans_assign(const gs_kmeans_desc* desc_host, void* stream);
int gs_kmeans_members_ws_bytes(int64_t n, int32_t k, int32_t chunk, int64_t* bytes_out_host);
int gs_kmeans_members(const gs_kmeans_members_desc* desc_host, void* stream);

/* ---------------------------------------------------------------------------------------------
 * IVF  approximate top-k partners through an inverted file over a k-means partition (csrc/gs_ivf.hip): the sweep of TOPK over
 *      gathered (query, cluster-member) tiles.
 *        index   = centers [n_clusters][ldc] and the lists of gs_kmeans_members: list_ptr int64 [n_clusters + 1], list_ids int32
 *                  [n_list], cluster j's run in ascending row id, every entry in [0, n_cand) and in one list only (the caller
 *                  checks them once; the kernel clamps and never makes a stray read)
 *        P_q     = the nprobe centres that come first in the order (<Xq[q], c_j> descending, j ascending)
 *        C_q     = the candidate set of gs_topk_select (src, filter and flags as there)
 *        ids[q], scores[q] = the first count[q] = min(k, .) members of C_q n U_{j in P_q} list_j in the total order (s
 *                  descending, w ascending), s(q, w) = <Xq[q], Zc[w]>; entries at and beyond count[q] are -1 / -inf, a score of
 *                  -0.0f is reported as +0.0f.  scanned[q] (nullable) = the members of the probed lists.
 *      s(q, w) is the arithmetic of gs_topk_select bit for bit, and so are the key, the lists and the merge: with nprobe =
 *      n_clusters the ids, the score bits and the counts are those of gs_topk_select.
 *      Five steps, plain launches on the caller's stream, nothing read back: probe (gs_topk_select on the centres with k =
 *      nprobe), group (gs_kmeans_members over the pairs p = j * Q + q of probe slot j and query q), plan (one workgroup: an
 *      exclusive scan of ceil(pairs_c / 128)), scan (one workgroup per (cluster, 128 of its pairs) sweeps the list's member
 *      tiles; grid floor(Q * nprobe / 128) + n_clusters, a workgroup without an item exits), merge (topk_merge_kernel with
 *      slices = nprobe).  The filter row of src[q] is consulted by binary search, and only for a key that already beats the
 *      row's threshold.  Integers and compares only after the MFMA chain, no atomics: bitwise reproducible.
 *      1 <= k <= GS_TOPK_MAX; 1 <= nprobe <= min(GS_IVF_MAX_PROBE, n_clusters); 1 <= n_clusters <= GS_KMEANS_MAX_K; d is a
 *      multiple of 4 in [4, 1024]; ld >= d; Q < 2^24 (the binding passes chunks of 65,536).  stop_after: 0, or 1 .. 5 to return
 *      after that step (for measuring the steps; the outputs are then not written).
 *      gs_ivf_ws_bytes(Q, n_clusters, k, nprobe): the probe's workspace and results, the pairs and their grouping, item_ptr and
 *      Q * nprobe lists of cap = 64 * (1 + ceil(k / 64)) uint64 keys with their lengths, every part at a multiple of 16 bytes.
 *      gs_ivf_desc is 200 bytes on every target (checked at compile time and by the binding; passed by pointer).
 * ------------------------------------------------------------------------------------------- */
#define GS_IVF_MAX_PROBE 128
typedef struct gs_ivf_desc {
    const float* Xq;           /* device [Q][ldq] query rows */
    const float* Zc;           /* device [n_rows][ldz] candidate table */
    const float* centers;      /* device [n_clusters][ldc] */
    const int64_t* list_ptr;   /* device [n_clusters + 1] */
    const int32_t* list_ids;   /* device [n_list] */
    const int32_t* src;        /* device [Q] or NULL: table row of the query node */
    const int64_t* f_rowptr;   /* device [n_rows + 1] or NULL */
    const int32_t* f_col;      /* device [f_nnz] or NULL (with f_rowptr) */
    int32_t* ids;              /* device [Q][k] */
    float* scores;             /* device [Q][k] */
    int32_t* count;            /* device [Q] */
    int64_t* scanned;          /* device [Q]; nullable */
    void* ws;                  /* device, 16-byte aligned, ws_bytes >= gs_ivf_ws_bytes(Q, n_clusters, k, nprobe) */
    int64_t Q, ldq, n_rows, n_cand, ldz, ldc, n_list, f_nnz, ws_bytes;
    int32_t d, k, nprobe, n_clusters, flags, stop_after;     /* flags: 0 or GS_RANK_KEEP_SRC */
} gs_ivf_desc;
int gs_ivf_ws_bytes(int64_t Q, int32_t n_clusters, int32_t k, int32_t nprobe, int64_t* bytes_out_host);
int gs_ivf_search(const gs_ivf_desc* desc_host, void* stream);

/* ---------------------------------------------------------------------------------------------
 * PROP label propagation / Correct and Smooth (Huang et al., ICLR 2021) over a CSR adjacency (csrc/gs_propagate.hip): the
 *      normalised operator applied to a NARROW table (d = the number of classes), one fused launch per step.
 *
 *      gs_prop_weights: for every row r of the CSR (rowptr int64 [n_rows + 1], col int32)
 *        deg[r] = the number of entries of row r that are not `pad`; a duplicate counts as often as it occurs; deg[pad] = 0
 *        w[r]   = the fp32 nearest to 1.0 / sqrt((double)deg[r]) (one fp64 square root and division, rounded once); 0 at deg 0
 *      One wave per row, integer counts only, no atomics.
 *
 *      gs_prop_step: one step for every row r < n_rows and column j < d
 *        s         = w[r] * sum_e w[col[e]] * X[col[e]][j]       e over the row's entries; an entry equal to pad contributes
 *                                                                exactly 0 (its table row is not read)
 *        y         = fmaf(alpha, s, R ? R[r][j] : 0)             R: the residual table, nullable
 *        out[r][j] = min(max(y, lo), hi)                         lo = -inf, hi = +inf: no clamp
 *        out[pad][:] = 0
 *      Rows may be directed, hold duplicates and hold pad entries anywhere.  The launch follows the work-item plan of INF
 *      (items / splits over ALL rows, no window): one wave reduces one item.  With cpad = round_up(d, 4) the wave is cut into
 *      G = 64 / Lg groups of Lg lanes, Lg = 16 (cpad <= 64), 32 (cpad <= 128), 64 (cpad <= 256); group g takes the entries
 *      g, g + G, ... of the item in ascending order, a lane holds one float4 of the row and adds with fmaf(w_c, x, acc); the
 *      groups are then added in one fixed order ((g0 + g2) + (g1 + g3); g0 + g1).  An uncut row is finished by its wave; a cut
 *      row's plain sum (before w[r]) goes to its slot of ws ([n_slots][cpad] floats, gs_prop_ws_bytes) and a second launch adds
 *      the partials in slot order and finishes the row.  No float atomics: bitwise repeatable.  Columns d .. cpad - 1 of out are
 *      written 0; columns at and beyond cpad are not written.  An item, split or column id outside the graph is skipped.
 *      1 <= d <= GS_PROP_MAX_D (else GS_ENOTSUP); ldx, ldr, ldo >= cpad, out != X, X and R hold n_rows rows (else GS_EINVAL).
 *      gs_prop_desc is 176 bytes on every target (checked at compile time and by the binding; passed by pointer, not part of
 *      gs_abi_struct_sizes).
 *
 *      gs_prop_correct: the autoscaled correction and the label overwrite in one launch, for every row i < n
 *        l1     = sum_j |E[i][j]|                 one lane group per row: per lane in column order, then the xor butterfly
 *        scale  = sigma / l1, replaced by 1 where it is not finite or exceeds 1000
 *        out[i] = known[i] ? Y[i] : P[i] + scale * E[i]          (fmaf; out may be P)
 *      known: int32 [n] flags; Y (and known) may be NULL: no row is known.  1 <= d <= GS_PROP_MAX_D, every ld >= cpad.
 * ------------------------------------------------------------------------------------------- */
#define GS_PROP_MAX_D 256
typedef struct gs_prop_desc {
    const int64_t* rowptr;     /* device [n_rows + 1] */
    const int32_t* col;        /* device [nnz] */
    const int64_t* items;      /* device [n_items][4]: the plan of INF over all rows */
    const int64_t* splits;     /* device [n_split][3]; nullable when n_split == 0 */
    const float* X;            /* device [n_rows][ldx] */
    const float* R;            /* device [n_rows][ldr]; nullable */
    const float* w;            /* device [n_rows] (gs_prop_weights) */
    float* out;                /* device [n_rows][ldo]; not X */
    float* ws;                 /* partials of the cut rows; nullable when there are none */
    int64_t n_rows, nnz, n_items, n_split, n_slots, pad;
    int64_t ldx, ldr, ldo, ws_bytes;
    float alpha, lo, hi;
    int32_t d, split_len, reserved_;       /* reserved_: 0 */
} gs_prop_desc;
int gs_prop_weights(const int64_t* rowptr, const int32_t* col, int64_t n_rows, int64_t pad, int32_t* deg, float* w, void* stream);
int gs_prop_ws_bytes(int64_t n_slots, int32_t d, int64_t* bytes_out_host);
int gs_prop_step(const gs_prop_desc* desc_host, void* stream);
int gs_prop_correct(const float* P, int64_t ldp, const float* E, int64_t lde, const float* Y, int64_t ldy, const int32_t* known,
                    int64_t n, int32_t d, float sigma, float* out, int64_t ldo, void* stream);

/* ---------------------------------------------------------------------------------------------
 * NBR  link-ranking baselines from neighbor overlap (csrc/gs_nbr_rank.hip): common neighbors, Adamic-Adar, resource allocation
 *      and the Jaccard ratio of every edge (src, dst), ranked against ALL nodes in the launch that forms the scores.
 *
 *      The CSR (rowptr int64 [n_nodes + 1], col int32) is a SIMPLE graph: every row strictly ascending, ids in [0, n_nodes),
 *      no self loops; it need not be symmetric.  N(w) is the stored row of w.  With the weights q (uint32 [n_nodes]; NULL: 1)
 *        s(u, x) = sum of q[w] over the w in N(u) with x in N(w)            (row u of A diag(q) A; every sum < 2^32)
 *      GS_NBR_SUM ranks by s.  GS_NBR_JACCARD (q NULL, deg = the row lengths, int32 [n_nodes]) ranks by the ratio
 *      s / (deg[u] + deg[x] - s), 0 where s = 0; two ratios a / b and c / e compare as a * e against c * b in uint64, never in
 *      floating point.
 *
 *      The queries come grouped by source: group g is the source group_src[g] with the partners dst[group_ptr[g] ..
 *      group_ptr[g + 1]) (n_queries = group_ptr[n_groups]; a source may own several groups, a partner may repeat, dst == src is
 *      legal).  For query k of source u, over the candidates x in [0, n_nodes) with x != dst[k], x != u and x not in the filter
 *      row of u (f_rowptr int64 [n_nodes + 1], f_col int32: rows strictly ascending, ids in [0, n_nodes); both NULL: no filter)
 *        t[k]    = s(u, dst[k])                                              (the numerator, also for GS_NBR_JACCARD)
 *        n_gt[k] = the candidates that rank above dst[k], n_eq[k] = those that tie with it
 *      A candidate that shares no neighbor scores 0 and is counted, not visited.  Every id is the caller's to validate: the
 *      kernel reads rows of whatever id it is given.
 *
 *      One workgroup takes the groups blockIdx, blockIdx + grid, ...; grid = min(n_groups, CUs * GS_NBR_WG_PER_CU,
 *      max_workgroups if > 0) (gs_nbr_rank_grid).  The candidate ids are cut into tiles of `tile` ids (a power of two in
 *      [GS_NBR_MIN_TILE, GS_NBR_MAX_TILE]; 0: GS_NBR_TILE) whose uint32 scores live in LDS; only tiles that a row N(w) touches
 *      are visited, in ascending order.  Every w in N(u) keeps the offset of its row's first unconsumed id: in LDS for up to
 *      GS_NBR_CURSORS rows, else in ws (grid * ws_stride uint32, ws_stride >= the longest source row; gs_nbr_rank_ws_bytes),
 *      else (ws NULL or too narrow) the offset is searched again per tile.  Integer LDS atomics only: no floating point, no
 *      global atomics, no score vector in memory; the results do not depend on the grid, the tile or the run.
 *      gs_nbr_rank_desc is 160 bytes on every target (checked at compile time and by the binding; passed by pointer).
 * ------------------------------------------------------------------------------------------- */
#define GS_NBR_TILE 8192
#define GS_NBR_MIN_TILE 64
#define GS_NBR_MAX_TILE 16384
#define GS_NBR_PARTNER_CHUNK 64
#define GS_NBR_CURSORS 2048
#define GS_NBR_WG_PER_CU 3
#define GS_NBR_SUM 0
#define GS_NBR_JACCARD 1
typedef struct gs_nbr_rank_desc {
    const int64_t* rowptr;     /* device [n_nodes + 1] */
    const int32_t* col;        /* device [nnz] */
    const uint32_t* q;         /* device [n_nodes]; NULL: every weight 1 (required NULL for GS_NBR_JACCARD) */
    const int32_t* deg;        /* device [n_nodes]; GS_NBR_JACCARD only */
    const int64_t* f_rowptr;   /* device [n_nodes + 1]; nullable with f_col */
    const int32_t* f_col;
    const int64_t* group_ptr;  /* device [n_groups + 1] */
    const int32_t* group_src;  /* device [n_groups] */
    const int32_t* dst;        /* device [n_queries], in group order */
    uint32_t* t;               /* device [n_queries], in group order */
    int32_t* n_gt;             /* device [n_queries] */
    int32_t* n_eq;             /* device [n_queries] */
    uint32_t* ws;              /* cursors of sources with more than GS_NBR_CURSORS neighbors; nullable */
    int64_t n_nodes, n_groups, n_queries, ws_stride, ws_bytes;
    int32_t kind, tile, max_workgroups, reserved_;      /* reserved_: 0 */
} gs_nbr_rank_desc;
int gs_nbr_rank_grid(int64_t n_groups, int32_t max_workgroups, int64_t* grid_out_host);
int gs_nbr_rank_ws_bytes(int64_t n_workgroups, int64_t max_src_degree, int64_t* bytes_out_host);
int gs_nbr_rank(const gs_nbr_rank_desc* desc_host, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Host-side graph ingestion (C++, multithreaded): edge list -> CSR. Replaces the networkx loops of
 * minibatch.py:227-259 for the CSR engine (N2 "next" row).  All pointers are HOST pointers.
 * keep_mask_host (nullable, per edge) drops edges (train_removed / val-test endpoints).
 * Adjacency lists come out sorted and de-duplicated (networkx.Graph semantics: one edge per node pair).
 * ------------------------------------------------------------------------------------------- */
int gs_build_csr_host(const int32_t* src_host, const int32_t* dst_host, const uint8_t* keep_mask_host,
                      int64_t n_edges, int64_t n_nodes, int symmetrize,
                      int64_t* rowptr_out_host /* [n_nodes+1] */, int32_t* col_out_host /* cap */,
                      int64_t col_capacity, int64_t* nnz_out_host);

#ifdef __cplusplus
}
#endif
#endif /* GRAPHSAGE_AMD_H */
