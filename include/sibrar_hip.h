/*
 * sibrar_hip.h — C ABI of libsibrar_hip.so, the MI355X (gfx950) engine for the SiBraR SingleBranchNet hot path.
 *
 * Conventions:
 *   - plain C: raw DEVICE pointers (e.g. torch's tensor.data_ptr()), explicit sizes / leading dimensions in ELEMENTS,
 *     scalar hyper-parameters, and a `void* stream` that is a hipStream_t (NULL = default stream);
 *   - no ownership transfer: every buffer (parameters, gradients, activations, workspaces) is allocated and freed by
 *     the caller; kernels are stateless, asynchronous on the given stream and re-entrant per stream;
 *   - return value: 0 = ok, non-zero = error; sbr_last_error() returns the message of the calling thread's last error;
 *   - row-index arrays (`*_idx`, `rows`, `slots`) are int32 device arrays, entity ids are int64 (torch.long) as the
 *     reference's loaders produce them (data/dataloader.py:196-198); NULL index array = identity.
 *
 * The reference (Tigxy/SiBraR---Single-Branch-Recommender) has no native code and therefore no FFI: each entry point
 * below names the PyTorch call site(s) of the reference that it replaces (paths relative to the reference root).
 * INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 */
#ifndef SIBRAR_HIP_H
#define SIBRAR_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* activation codes — modules/polylinear.py:5-10 (ACTIVATION_FN_MAP) */
#define SBR_ACT_NONE 0
#define SBR_ACT_RELU 1
#define SBR_ACT_TANH 2
#define SBR_ACT_SIGMOID 3
#define SBR_ACT_SELU 4

/* recommendation-loss kinds — train/rec_losses.py:116-119 (RecommenderSystemLossesEnum) */
#define SBR_LOSS_BCE 0
#define SBR_LOSS_BPR 1
#define SBR_LOSS_SAMPLED_SOFTMAX 2

const char* sbr_last_error(void);
int sbr_abi_version(void);

/* ---- deterministic mode — utilities/utils.py:22-27 (reproducible(seed): the seeds + torch.backends.cudnn.deterministic) ------
 * A process-wide switch (additive to ABI 4; off by default). While it is on, no entry point launches a kernel that accumulates
 * floats or doubles with atomics in arrival order: an entry point that has such a path takes its fixed-order form (every sum has one
 * owner and a fixed order of addition, so repeated runs give the same bits) or returns an error whose message names the entry point
 * and says "no deterministic form" — never the atomic path. The fixed-order forms keep a library-owned scratch block per device:
 * drive one stream per device while the mode is on, and run a step once with plain launches before capturing it into a graph.
 * sbr_nondeterministic_launches(): how many launches of arrival-order float accumulation the entry points have made since the last
 * sbr_reset_nondeterministic_launches(), counted on the host in BOTH modes (0 over a training = it stayed on fixed-order paths). */
int sbr_set_deterministic(int on);
int sbr_get_deterministic(void);
long sbr_nondeterministic_launches(void);
int sbr_reset_nondeterministic_launches(void);

/* The fixed-order form of sbr_scatter_add_rows (what that entry point runs while the mode is on; callable in either mode) —
 * utilities/utils.py:22-27 applied to the dense nn.Embedding gradient of algorithms/sgd_alg.py:144-145: the rows are grouped by
 * destination on the device, one wave owns a destination row and adds its source rows in ascending j. D <= 512; source rows that
 * are all zero are skipped (the padded slots of a captured step). */
int sbr_scatter_add_rows_det(const float* dOut, long ldo, const int* in_idx, const int* rows, float* dW, long ldw, long n, int D,
                             void* stream);

/* ---- dense products on the matrix cores (fp32 in / fp32 accumulate, v_mfma_f32_32x32x2_f32) -------------------------
 * mode 0 (NT): C[ci(m), n] = act(sum_k A[ai(m), k] * B[n, k] + bias[n])     nn.Linear forward — modules/polylinear.py:51,
 *              the modality projectors algorithms/sgd_alg.py:1342-1357 with the row gather of sgd_alg.py:1960-1974 fused
 *              in, and the all-pairs scorer einsum('be,ce->bc') algorithms/sgd_alg.py:2109 / eval/eval.py:217.
 * mode 1 (NN): C[m, n] = sum_k A[ai(m), k] * B[k, n]                        autograd of nn.Linear w.r.t. its input.
 * mode 2 (TN): C[m, n] += sum_k A[ak(k), m] * B[bk(k), n]                   autograd of nn.Linear w.r.t. its weight; split
 *              over k with float atomics, so C must be zero-initialised and accumulate_atomic must be 1.
 * a_idx / b_idx / c_idx: optional int32 row maps (NULL = identity).
 * K = 0 is an empty sum: modes 0 and 1 store act(bias[n]) (act(0) without a bias), mode 2 adds nothing and launches nothing (C keeps
 * what it holds; valid in deterministic mode and not counted by sbr_nondeterministic_launches); sbr_gemm_tn_f32 stores zeros. M = 0 or N = 0 returns at once. */
int sbr_gemm_f32(int mode, const float* A, long lda, const int* a_idx, const float* B, long ldb, const int* b_idx,
                 const float* bias, float* C, long ldc, const int* c_idx, int M, int N, int K, int act,
                 int accumulate_atomic, void* stream);

/* NT (mode 0 of sbr_gemm_f32: nn.Linear forward with fused bias / activation / row gather / row scatter) for products with few
 * output tiles and a long K — the modality projectors at the reference's default batch of 256: K is split over workgroups, the
 * partial tiles are summed in a fixed order by a second kernel that applies bias, activation and the scatter.
 * sbr_gemm_nt_splitk_workspace() returns 0 for shapes that should go to sbr_gemm_f32 instead. */
long sbr_gemm_nt_splitk_workspace(int M, int N, int K);
int sbr_gemm_nt_splitk_f32(const float* A, long lda, const int* a_idx, const float* B, long ldb, const float* bias, float* C,
                           long ldc, const int* c_idx, int M, int N, int K, int act, void* workspace, long workspace_bytes,
                           void* stream);

/* The same fp32 products for WIDE layers on the bf16 matrix pipe (csrc/gemm_split_wide_f32.hip; new in ABI 3): N a multiple of 256,
 * K a multiple of 32 of at least 64 — modules/polylinear.py:51 with hidden widths 256 / 512, forward (mode 0, NT: W [N][K]) and input
 * gradient (mode 1, NN: W [K][N]): C[ci(m), :] = act(A[ai(m), :] x W (+ bias)). a_idx / c_idx / bias may be NULL. */
int sbr_gemm_split_wide_supported(long M, int N, int K);
int sbr_gemm_split_wide_f32(int mode, const float* A, long lda, const int* a_idx, const float* W, long ldw, const float* bias, float* C,
                            long ldc, const int* c_idx, long M, int N, int K, int act, void* stream);
/* TN with a deterministic split-K slab reducer (no atomics): C[m, n] = sum_k A[ak(k), m] * B[bk(k), n], C overwritten.
 * autograd of nn.Linear w.r.t. its weight (dW = dZ^T X[rows]). workspace: sbr_gemm_tn_f32_workspace(M, N, K) bytes. */
long sbr_gemm_tn_f32_workspace(int M, int N, int K);
/* 1 when sbr_gemm_tn_f32 / _slabs serve this shape with the bf16-split kernel (csrc/gemm_split_tn_f32.hip), 0: fp32 ring kernel */
int sbr_gemm_tn_split_supported(int M, int N, int K);
int sbr_gemm_tn_f32(const float* A, long lda, const int* a_idx, const float* B, long ldb, const int* b_idx, float* C, long ldc,
                    int M, int N, int K, void* workspace, long workspace_bytes, void* stream);
/* The same product with the reduction deferred: sbr_gemm_tn_f32_slabs writes only the partial slabs (the workspace then belongs to
 * the product; *splits_out, a HOST int, receives the slab count) and sbr_splitk_reduce_multi sums the slabs of up to 8 products in
 * the same fixed order with ONE launch (a training step needs its weight gradients only at the optimizer). slabs / outs: HOST
 * arrays of device pointers; ldcs / Ms / Ns / splits: HOST arrays. */
int sbr_gemm_tn_f32_slabs(const float* A, long lda, const int* a_idx, const float* B, long ldb, const int* b_idx, int M, int N, int K,
                          void* workspace, long workspace_bytes, int* splits_out, void* stream);
int sbr_splitk_reduce_multi(int count, const void* const* slabs, const void* const* outs, const long* ldcs, const int* Ms, const int* Ns,
                            const int* splits, void* stream);
/* the same launch also finishes up to 8 pending column reductions (sbr_colred_finish: out[i] = sum of the replicas of entry i of
 * its workspace, replicas left zeroed): the two finishing launches at the end of a backward pass become one. */
int sbr_splitk_reduce_multi_fin(int count, const void* const* slabs, const void* const* outs, const long* ldcs, const int* Ms,
                                const int* Ns, const int* splits, int fin_count, const void* const* fin_workspaces,
                                const void* const* fin_outs, const int* fin_widths, void* stream);

/* Weights-resident variant for the shared MLP's own products (N = K = 128, no gathers): every wave keeps its half of the 128 x 128
 * weight in registers, only A streams through LDS (csrc/gemm_wres_f32.hip); bit-identical to sbr_gemm_f32 on the same operands.
 * mode 0 (NT): C = act(A W^T + bias) — nn.Linear forward, modules/polylinear.py:51,63-72; mode 1 (NN): C = A W — its autograd
 * w.r.t. the input. Y != NULL (mode 1): C = (A W) * act'(Y), the gradient at the pre-activation of the layer in front whose OUTPUT
 * is Y, and colsum_ws (17 * 128 doubles, contract of sbr_colsum; may be NULL) receives the pending column sums of C — that layer's
 * bias gradient, completed by sbr_colred_finish. A and W: 16-byte aligned base, leading dimension a multiple of 4; C and Y are
 * accessed one float per lane and take any base and leading dimension (the same holds for C / Y of sbr_gemm_split_f32, and for C of
 * sbr_gemm_split_proj_f32 and sbr_gemm_split_wide_f32). */
int sbr_gemm_wres_supported(long M, int N, int K);
int sbr_gemm_wres_f32(int mode, const float* A, long lda, const float* W, long ldw, const float* bias, float* C, long ldc, long M, int N,
                      int K, int act, const float* Y, long ldy, double* colsum_ws, void* stream);

/* The same products (same arguments, same epilogues) on the bf16 matrix pipe: both fp32 operands are split exactly into three bf16
 * numbers each (8 + 8 + 8 significand bits) and the six leading partial products are accumulated in fp32 by
 * v_mfma_f32_32x32x16_bf16 (csrc/gemm_split_f32.hip). The dropped terms are below 2^-23 of each product, i.e. the result carries
 * the error of an fp32 GEMM (summation order differs from sbr_gemm_f32, so it is not bit-identical to it); the kernel is bound by
 * HBM instead of the fp32 matrix pipe. Non-finite inputs give NaN. Replaces the same reference lines as sbr_gemm_wres_f32. */
int sbr_gemm_split_supported(long M, int N, int K);
int sbr_gemm_split_f32(int mode, const float* A, long lda, const float* W, long ldw, const float* bias, float* C, long ldc, long M, int N,
                       int K, int act, const float* Y, long ldy, double* colsum_ws, void* stream);
/* mode 0 with the statistics epilogue and sbr_bn_finalize_stats in ONE launch (new): the last workgroup to arrive turns the pending
 * sums into save_mean / save_rstd of the M rows of C, updates running_mean / running_var (may both be NULL) and
 * num_batches_tracked (may be NULL); colsum_ws (zero on entry) and *arrive (one zeroed 64-bit word owned by the BatchNorm) are
 * left zeroed. */
int sbr_gemm_split_bnstats_f32(const float* A, long lda, const float* W, long ldw, const float* bias, float* C, long ldc, long M, int N,
                               int K, int act, double* colsum_ws, void* arrive, float* running_mean, float* running_var,
                               long* num_batches_tracked, float* save_mean, float* save_rstd, float eps, float momentum, void* stream);
/* The dense modality projector on the same arithmetic — FeatureEmbedding's nn.Linear(F, C) over gathered feature rows
 * (algorithms/sgd_alg.py:1279-1396, forward of 1960-1974): C[ci(m), 0..127] = act(A[ai(m), 0..K-1] x W^T + bias), W [128][K],
 * N = 128, K = 128 j >= 256; a_idx (feature row of every slot), c_idx (row of the shared network's input), bias may be NULL.
 * The weight is walked in K chunks of 128 whose three bf16 planes are rebuilt in LDS (csrc/gemm_split_f32.hip). */
int sbr_gemm_split_proj_supported(long M, int N, int K);
int sbr_gemm_split_proj_f32(const float* A, long lda, const int* a_idx, const float* W, long ldw, const float* bias, float* C, long ldc,
                            const int* c_idx, long M, int N, int K, int act, void* stream);

/* HOST function (no device work): numpy's legacy `np.random.randint(0, high, size=n)` on a caller-owned MT19937 state
 * (key[624] + position from np.random.get_state(), advanced in place) — the draws of the default negative-sampling collate
 * (data/dataloader.py:154-198, np.random.choice(items_in_split, n) on the global RandomState). Bit-identical values and final
 * state for high - 1 < 2^32. */
int sbr_host_mt19937_randint(unsigned int* key, int* pos, long high, long n, long* out);

/* HOST function: out[q] = (items[q] in row users[q]) over a HOST copy of the sorted interaction CSR — the membership test of
 * the collate (data/dataloader.py:184-191) for its small redraw rounds, where a device round trip costs more than the search. */
int sbr_host_csr_contains(const long* indptr, const int* indices, const long* users, const long* items, long n,
                          unsigned char* out);
/* HOST: the layout step of the collate (data/dataloader.py:192-195): items[b, 0] = pos_items[b], items[b, 1 + j] = values[j * B + b]. */
int sbr_host_assemble_items(const long* pos_items, const long* values, long B, int n_neg, long* out_items);
/* the whole default collate (NegativeSamplingDataLoader._neg_sampling_collate_fn, data/dataloader.py:154-198) of a small batch in one
 * host call: draws every slot from the MT19937 stream (key, pos as for sbr_host_mt19937_randint), redraws the slots that hit one of
 * their user's interactions (sorted CSR) round by round in ascending slot order, writes [B, 1 + n_neg] items (column 0 = positive).
 * items_in_split NULL = identity; values, todo: scratch of B * n_neg longs. */
int sbr_host_recbole_collate(unsigned int* key, int* pos, const long* users, const long* pos_items, long B, int n_neg, long n_cand,
                             const long* items_in_split, const long* indptr, const int* indices, long* out_items, long* values,
                             long* todo);

/* Stable counting sort of the modality draw: the boolean-mask grouping of the flattened index tensor by sampled modality
 * (algorithms/sgd_alg.py:1934-1957). pos: int8 [R] modality position of every slot; segment m of slots_out
 * ([seg_offsets[m], seg_offsets[m+1]), HOST array of n_mod + 1 offsets, n_mod <= 8) receives the slots of modality m in
 * ascending order, its unused tail (capacity > count) is filled with the sentinel R. workspace: device scratch of
 * sbr_partition_slots_workspace(R) bytes (per-chunk histograms). */
long sbr_partition_slots_workspace(long R);
int sbr_partition_slots(const signed char* pos, long R, int n_mod, const int* seg_offsets, int* slots_out, void* workspace,
                        long workspace_bytes, void* stream);

/* ---- index plumbing ----------------------------------------------------------------------------------------------------
 * rows_out[j] = rowmap_seg(j)[ idx[slots[j] / k] ] for the concatenated per-modality slot lists (segment s covers
 * [seg_offsets[s], seg_offsets[s+1])): the id -> row lookup of Feature.__getitem__ (data/Feature.py:146) on the
 * repeat_interleave'd index vector of algorithms/sgd_alg.py:1944-1946. rowmaps is a HOST array of n_seg device pointers
 * (NULL entry = identity), rowmap_lens a HOST array with the number of ids each map covers (identity: the number of rows).
 * An id outside its map or mapped to -1 has no row in that feature's split: err_flag (device int, sticky) is set to 1 and
 * row 0 is used instead, so that no consumer indexes out of bounds; the host turns the flag into the reference's KeyError. */
int sbr_resolve_rows(const long* idx, int k, const int* slots, int n, int n_seg, const int* seg_offsets,
                     const int* const* rowmaps, const int* rowmap_lens, int* rows_out, int* err_flag, void* stream);

/* out[j] = 1 iff (rows[j], cols[j]) is a stored entry of the CSR matrix (sorted column indices): the `v in positives` test of
 * the negative-sampling collate, data/dataloader.py:184-191, for all slots of a round at once. */
int sbr_csr_contains(const long* indptr, const int* indices, const long* rows, const long* cols, long n, unsigned char* out,
                     void* stream);

/* dense interaction vectors of a batch of entities — InteractionRecDataset._get_interaction_vectors, data/dataset.py:306-319
 * (matrix[indices].toarray()), as consumed by DropoutNet's preference networks (algorithms/sgd_alg.py:1693-1725):
 * out[j, 0..dim) = CSR row ent[j] (data NULL: ones), all zeros for ent[j] < 0 (dropped preferences). */
int sbr_csr_rows_to_dense(const long* indptr, const int* indices, const float* data, const long* ent, long n, int dim, float* out,
                          long ldo, void* stream);

/* nn.Embedding forward — algorithms/sgd_alg.py:1331,1386: out[oi(j), :] = W[rows[j], :] */
int sbr_gather_rows(const float* W, long ldw, const int* rows, float* out, long ldo, const int* out_idx, long n, int D,
                    void* stream);
/* a plain embedding-lookup side in ONE launch (new: the fused training step): sbr_resolve_rows with one segment and k = 1
 * (data/Feature.py:146: id -> row through rowmap, or the id itself when rowmap is NULL and id < rowmap_len) + sbr_gather_rows;
 * rows_out [n] keeps the rows for sbr_scatter_add_rows. Ids without a row set *err_flag and read row 0. */
int sbr_lookup_rows_supported(const float* W, long ldw, const float* out, long ldo, int D);
int sbr_lookup_rows(const long* idx, long n, const int* rowmap, int rowmap_len, const float* W, long ldw, int* rows_out, float* out,
                    long ldo, int D, int* err_flag, void* stream);
/* its dense gradient: dW[rows[j], :] += dOut[ii(j), :] (dW zero-initialised by the caller) */
int sbr_scatter_add_rows(const float* dOut, long ldo, const int* in_idx, const int* rows, float* dW, long ldw, long n, int D,
                         void* stream);
/* the same dense gradient without float atomics, from row lists sorted by table row (new: the data-parallel exchange of
 * lookup gradients, SURVEY.md 8(e) — every rank must produce the same bits). rows_sorted[j] = table row of sorted position j,
 * perm[j] = its source row p: block p / blk (blocks are block_stride floats apart), row p % blk (rows ldo floats apart).
 * Equal rows are added in sorted order by one thread; dW[row, :] += sum. */
int sbr_scatter_add_rows_sorted(const float* dOut, long ldo, long blk, long block_stride, const long* perm,
                                const int* rows_sorted, float* dW, long ldw, long n, int D, void* stream);

/* nn.EmbeddingBag(mode='mean', padding_idx=pad) over padded tag lists — algorithms/sgd_alg.py:1336-1337, 1383-1386;
 * data/Feature.py:254-255. tags: [n_table_rows, T] int32. */
int sbr_bag_mean_fwd(const float* W, long ldw, const int* tags, int T, int pad, const int* rows, float* out, long ldo,
                     const int* out_idx, long n, int D, void* stream);
int sbr_bag_mean_bwd(const float* dOut, long ldo, const int* in_idx, const int* tags, int T, int pad, const int* rows,
                     float* dW, long ldw, long n, int D, void* stream);

/* Linear over the CSR "interactions" modality without densifying — replaces data/Feature.py:149-150 (.toarray()) +
 * algorithms/sgd_alg.py:1380 (x.float()) + modules/polylinear.py:51. Wt is the projector weight stored column-major
 * (row c of Wt = column c of the [C, n_cols] nn.Linear weight). vals may be NULL (all ones). */
int sbr_csr_project_fwd(const long* indptr, const int* indices, const float* vals, const float* Wt, long ldw,
                        const float* bias, const int* rows, float* out, long ldo, const int* out_idx, long n, int C, int act,
                        void* stream);
int sbr_csr_project_bwd(const long* indptr, const int* indices, const float* vals, const float* dZ, long ldz, const int* rows,
                        float* dWt, long ldw, long n, int C, void* stream);
/* the same gradient in gather form (new in ABI 3): the slot gradients are added up per entity into the workspace dZe
 * [n_entities, C] (overwritten; lde = C), and every feature column then sums the rows of the entities that have it — the forward
 * kernel over the TRANSPOSED feature matrix (t_indptr / t_indices / t_vals: its CSR form, [n_cols, n_entities]), no atomics on
 * dWt, fixed summation order. One float atomic per (slot, column) instead of one per (slot, nnz, column): Onion18 at batch 4096,
 * 1.25 ms -> see DESIGN.md. Needs C % 4 == 0, C <= 1024. (algorithms/sgd_alg.py:1380, the backward of that Linear.) */
int sbr_csr_project_bwd_gather(const long* t_indptr, const int* t_indices, const float* t_vals, const float* dZ, long ldz,
                               const int* dz_idx, const int* rows, long n, float* dZe, long lde, long n_entities, float* dWt,
                               long ldw, long n_cols, int C, void* stream);
/* dz_idx (may be NULL): slot j's gradient row is dZ[dz_idx[j], :]. sbr_bag_mean_bwd in gather form is this entry point with the
 * transpose of X[entity, tag] = 1 / (number of tags of the entity). */

/* dZ[j, :] = dY[ii(j), :] * act'(Y[ii(j), :]) — autograd of the activations of modules/polylinear.py:63-72 */
int sbr_act_grad_gather(const float* dY, const float* Y, long ld, const int* in_idx, float* dZ, long ldz, long n, int C,
                        int act, void* stream);
/* out[c] = sum_j X[j, c] (bias gradients). workspace: 17*C doubles (totals + 16 replicas that spread the per-block atomics);
 * it must be ZERO on first use and every call leaves it zeroed again (no memset per call). */
int sbr_colsum(const float* X, long ld, long n, int C, float* out, double* workspace, void* stream);

/* F.normalize(p=2, dim=-1, eps) — algorithms/sgd_alg.py:1873-1874 */
int sbr_l2norm_fwd(const float* X, float* Y, float* inv_norm, long n, int C, float eps, void* stream);
int sbr_l2norm_bwd(const float* dY, const float* Y, const float* inv_norm, float* dX, long n, int C, float eps, void* stream);

/* nn.Dropout(p) — algorithms/sgd_alg.py:1815, modules/polylinear.py:48; counter-based mask from (seed, element index),
 * the same call maps dY -> dX in the backward pass. */
int sbr_dropout(const float* X, float* Y, long total, float p, unsigned long long seed, void* stream);
/* the same with the seed in device memory (seed = seed_dev[0] + seed_offset, read when the kernel runs): a captured hipGraph
 * replays the launch while the host refreshes seed_dev[0] per step. sbr_dropout(seed) == sbr_dropout_dev with
 * seed_dev[0] + seed_offset == seed. */
int sbr_dropout_dev(const float* X, float* Y, long total, float p, const long* seed_dev, long seed_offset, void* stream);

/* aggregation over the k sampled modalities — algorithms/sgd_alg.py:27-31, 1861. mode 0 mean, 1 max. */
int sbr_aggregate_fwd(const float* E, float* out, unsigned char* argmax, long S, int k, int D, int mode, void* stream);
int sbr_aggregate_bwd(const float* dOut, const unsigned char* argmax, float* dE, long S, int k, int D, int mode, void* stream);

/* training scorer einsum('be,bce->bc') — algorithms/sgd_alg.py:2114 */
int sbr_score_dot_fwd(const float* U, const float* I, float* out, long B, int N, int D, void* stream);
int sbr_score_dot_bwd(const float* G, const float* U, const float* I, float* dU, float* dI, long B, int N, int D, void* stream);
/* DeepMF's training scorer — algorithms/sgd_alg.py:1238-1242: nn.CosineSimilarity(dim=-1)(u[:, None, :], i) with each norm clamped
 * at eps, then sim[sim < mu] = mu. U [B, D], I [B, N, D] -> out [B, N] (additive to ABI 4; csrc/score_cos.hip). The forward pass
 * also writes, once, what the backward pass needs: cos_raw [B, N] (the un-floored cosine), u_stat [B, 2] and i_stat [B, N, 2] =
 * {1 / max(|row|, eps), |row| > 0 ? 1 / |row| : 0}. Backward: a floored entry (cos_raw < mu) passes no gradient; a row at or below
 * eps takes the gradient of torch's autograd for its clamp (finite). dU or dI may be NULL. One wavefront per batch row, no atomics:
 * the same bits on every run. Any D >= 1, N >= 1. */
int sbr_score_cos_fwd(const float* U, const float* I, float* out, float* cos_raw, float* u_stat, float* i_stat, long B, int N, int D,
                      float mu, float eps, void* stream);
int sbr_score_cos_bwd(const float* G, const float* U, const float* I, const float* cos_raw, const float* u_stat, const float* i_stat,
                      float* dU, float* dI, long B, int N, int D, float mu, void* stream);
/* the floor of the all-pairs evaluation form — algorithms/sgd_alg.py:1241 on the [n, n_cols] score matrix of eval/eval.py:216
 * (row stride ld), in place: x[x < mu] = mu, NaN left alone. Applied before the exclusion mask (eval/eval.py:219-220). */
int sbr_floor_scores(float* scores, long n, long n_cols, long ld, float mu, void* stream);
/* ProtoMF's similarity to the prototypes — algorithms/sgd_alg.py:48-59 (compute_shifted_cosine_sim) behind the lookups of
 * sgd_alg.py:381-382, 486-488, with the regularisers of sgd_alg.py:394-399, 505-510 (additive to ABI 4; csrc/proto_cos.hip):
 *   e = W[rows[j], :] (rows NULL: row j; the gather is fused)      sim_out[j, p] = clamp(1 + e^ . p^, 0, 2),  x^ = x / max(|x|, 1e-12)
 *   *proto_loss = mean_p min_j (2 - sim)      *batch_loss = mean_j min_p (2 - sim)      (device scalars, no host sync)
 * 1 <= D <= 512, 2 <= n_proto <= 256 (anything else fails through sbr_last_error), R = 0 returns SBR_OK. Saved for the backward pass:
 * cos_raw [R, P] (the un-clamped cosine), row_stat [R, 2] and proto_stat [P, 2] = {max(|x|, eps), |x| >= eps ? 1 : 0},
 * row_best [R] = argmin_p, col_best_row [P] = argmin_j with col_best_val [P] its value.
 * TIE RULE: a minimum attained more than once goes to the lowest index (lowest p for a row, lowest j for a prototype); the values
 * compared are the fp32 distances 2 - sim.
 * Evaluation form: cos_raw, row_stat, proto_stat may be NULL, and row_best, col_best_val, col_best_row, proto_loss, batch_loss are
 * NULL together. workspace: sbr_proto_sim_workspace(R, D, n_proto, 0) bytes (backward: (..., 1)).
 * Backward: G [R, P] is the upstream gradient of sim, *g_proto / *g_batch (device scalars, NULL = 0) those of the two losses; the
 * arg-min contributions -g_proto / P and -g_batch / R are added inside the kernel, the clamp passes the gradient where
 * 0 <= 1 + cos <= 2 (torch.clamp), a norm below eps takes torch's clamp_min gradient. dE [R, D] is the gradient of the gathered rows
 * (scatter it with sbr_scatter_add_rows), dP [P, D] that of the prototypes; either may be NULL.
 * One form only: per-workgroup partials folded in a fixed order, no atomics — valid in deterministic mode. */
long sbr_proto_sim_workspace(long R, int D, int n_proto, int backward);
int sbr_proto_sim_fwd(const float* W, long ldw, const int* rows, long R, int D, const float* P, int n_proto, float* sim_out,
                      float* cos_raw, float* row_stat, float* proto_stat, int* row_best, float* col_best_val, int* col_best_row,
                      float* proto_loss, float* batch_loss, void* workspace, long workspace_bytes, void* stream);
int sbr_proto_sim_bwd(const float* G, const float* g_proto, const float* g_batch, const float* W, long ldw, const int* rows, long R,
                      int D, const float* P, int n_proto, const float* cos_raw, const float* row_stat, const float* proto_stat,
                      const int* row_best, const int* col_best_row, float* dE, float* dP, void* workspace, long workspace_bytes,
                      void* stream);
/* The simplified ProtoMF family's prototype side — algorithms/sgd_alg.py:62-73 (compute_cosine_sim) behind the lookups of
 * sgd_alg.py:677-678, 742-744, with the ReLU of sgd_alg.py:683, 739, 808, 814 on the other entity's weights and the dot over the
 * prototypes of sgd_alg.py:687, 750, 823-824 (additive to ABI 4; csrc/proto_cos.hip). Two forms of one op, selected by Wt:
 *   e = W[rows[j], :] (rows NULL: row j; the gather is fused)      cos[j, p] = clamp(e^ . P^_p, -1, 1),  x^ = x / max(|x|, 1e-12)
 *   cosine form (Wt NULL; out, widx NULL; fan ignored but >= 1): cos_out [R, P] is written
 *   score form: every row j carries fan >= 1 weight rows w[j, f, :] = Wt[widx[j fan + f], :] (widx NULL: row j fan + f; row stride
 *     ldwt >= n_proto):  out[j, f] = sum_p cos[j, p] max(w[j, f, p], 0); cos_out may be NULL. The gathered, relu'd weights are never
 *     written; for n_proto > 64 the partial dots of the 64-wide prototype tiles are added in tile order.
 * A NaN stays a NaN (torch.clamp). 1 <= D <= 512, 2 <= n_proto <= 256, 1 <= fan, R fan < 2^31 (anything else fails through
 * sbr_last_error; sbr_proto_score_workspace returns 0), R = 0 returns SBR_OK. Saved for the backward pass (what sbr_proto_sim_fwd
 * keeps): cos_raw [R, P] (the un-clamped cosine), row_stat [R, 2] and proto_stat [P, 2] = {max(|x|, eps), |x| >= eps ? 1 : 0}; any may
 * be NULL in the evaluation form. workspace: sbr_proto_score_workspace(R, D, n_proto, 0) bytes (backward: (..., 1)).
 * Backward: G is the upstream gradient — of cos, [R, P], in the cosine form; of out, [R, fan], in the score form, where
 * dcos[j, p] = sum_f G[j, f] max(w[j, f, p], 0) is formed inside the kernels. The clamp passes the gradient where -1 <= cos <= 1
 * (torch.clamp), a norm below eps takes torch's clamp_min gradient. dE [R, D] is the gradient of the gathered rows (scatter it with
 * sbr_scatter_add_rows), dP [P, D] that of the prototypes, dWrows [R fan, P] (score form) that of the gathered weight rows:
 * G[j, f] cos[j, p] where w > 0, else 0 (torch's ReLU: 0 at w == 0); each may be NULL. R = 0 zeroes dP.
 * One form only: dP is one partial per row split folded in split order, no atomics; the split count depends on (R, D, n_proto) only —
 * valid in deterministic mode, never a non-deterministic launch. */
long sbr_proto_score_workspace(long R, int D, int n_proto, int backward);
int sbr_proto_score_fwd(const float* W, long ldw, const int* rows, long R, int D, const float* P, int n_proto, const float* Wt,
                        long ldwt, const int* widx, int fan, float* cos_out, float* out, float* cos_raw, float* row_stat,
                        float* proto_stat, void* workspace, long workspace_bytes, void* stream);
int sbr_proto_score_bwd(const float* G, const float* W, long ldw, const int* rows, long R, int D, const float* P, int n_proto,
                        const float* Wt, long ldwt, const int* widx, int fan, const float* cos_raw, const float* row_stat,
                        const float* proto_stat, float* dE, float* dP, float* dWrows, void* workspace, long workspace_bytes,
                        void* stream);
/* ACF's anchor mixing — algorithms/sgd_alg.py:261-276 (ACF.get_user_representations / get_item_representations: lookup, e @ anchors^T,
 * softmax, c @ anchors) with the two entropy regularisers of ACF.forward, sgd_alg.py:246-254, whose exclusiveness term is
 * entropy_from_softmax, sgd_alg.py:76-85 (additive to ABI 4; csrc/anchor_mix.hip):
 *   e = W[rows[j], :] (rows NULL: row j; the gather is fused)     s = e . A^T     c_out[j, :] = softmax(s[j, :]) (max-subtracted)
 *   r_out[j, :] = c[j, :] . A      lse_out[j] = logsumexp_k s[j, k]
 *   *exc_loss = mean_j H_j, H_j = -sum_k c[j, k] (s[j, k] - lse[j])       *inc_loss = log K + sum_k q_k log q_k,
 *   q_out[k] = sum_j c[j, k] / sum_jk c[j, k]       dinc_out[k] = log q_k / sum_jk c[j, k] (d inc / d c[j, k] up to per-row constants)
 * 1 <= D <= 512, 2 <= n_anchors <= 256 (anything else fails through sbr_last_error), R = 0 returns SBR_OK and launches nothing.
 * Training form: every output. Evaluation / user-side form: q_out, dinc_out, exc_loss, inc_loss NULL together (no workspace needed),
 * and any of r_out, c_out, lse_out may be NULL as long as r_out or c_out is given. The logits s are never written; log c is never
 * taken (c underflows to exact zeros at large D and K; s - lse stays finite).
 * NaN CONTRACT (the reference's): a column of c that is 0 in every row gives q_k == 0 and *inc_loss = NaN (0 log 0), and so are the
 * gradients through g_inc; nothing is clamped. r, c, lse and *exc_loss do not depend on q.
 * workspace: sbr_anchor_mix_workspace(R, D, n_anchors, 0) bytes (backward: (..., 1)); 0 for a shape outside the range.
 * Backward: G [R, D] is the upstream gradient of r, *g_exc / *g_inc (device scalars, NULL = 0; both NULL: the user-side form, lse and
 * dinc are not read) those of the two losses. c is not differentiable on its own. ds = softmax backward of
 * dc = G . A^T + g_inc dinc[k], plus the exclusiveness term -g_exc / R c (s - lse + H) taken with respect to s directly (s is
 * recomputed); the gradient through the denominator sum_jk c is a per-row constant of dc and vanishes in the softmax backward.
 * dE [R, D] = ds . A is the gradient of the gathered rows (scatter it with sbr_scatter_add_rows), dA [K, D] = c^T . G + ds^T . e that of
 * the anchors; either may be NULL.
 * One form only: per-workgroup partials (column sums of c, entropy sums, dA) folded in a fixed order, no atomics; grid and split
 * counts depend on (R, D, n_anchors) only — valid in deterministic mode. */
long sbr_anchor_mix_workspace(long R, int D, int n_anchors, int backward);
int sbr_anchor_mix_fwd(const float* W, long ldw, const int* rows, long R, int D, const float* A, int n_anchors, float* r_out,
                       float* c_out, float* lse_out, float* q_out, float* dinc_out, float* exc_loss, float* inc_loss, void* workspace,
                       long workspace_bytes, void* stream);
int sbr_anchor_mix_bwd(const float* G, const float* g_exc, const float* g_inc, const float* W, long ldw, const int* rows, long R,
                       int D, const float* A, int n_anchors, const float* c, const float* lse, const float* dinc, float* dE, float* dA,
                       void* workspace, long workspace_bytes, void* stream);
/* ECF's sparse affiliation of a row to its clusters — algorithms/sgd_alg.py:1020-1037 (ECF._generate_item_representations, the item
 * side) and sgd_alg.py:988-1009 (ECF.get_user_representations, the user side); ECF is sgd_alg.py:891-1138 (additive to ABI 4;
 * csrc/cluster_affil.hip). Two forms of one op, selected by which operand is NULL:
 *   cosine form (t_in NULL): the rows are the whole table W [R, D] (row stride ldw, no index list) against Cl [n_clusters, D]:
 *     t_out[r, k] = clamp(W_r^ . Cl_k^, -1, 1),  x^ = x / max(|x|, 1e-12)      (compute_cosine_sim, sgd_alg.py:62-73)
 *   logit form (W and Cl NULL): t = t_in [R, n_clusters] is an input (D is ignored, t_out is not written)
 *   m = 1 at the `top` largest entries of a row      p = softmax(t / temp)      mh = p + (m - p)      x_out = sigmoid(t) * mh
 * mh is formed in fp32 as the reference forms it: exactly 0 off the mask, fl(p + fl(1 - p)) on it.
 * TIE RULE: equal logits at the mask boundary go to the LOWEST cluster index (-0 == +0); torch.topk leaves the order of ties
 * unspecified, so a reference run may pick another member of a tie.
 * 1 <= D <= 512 (cosine form), 2 <= n_clusters <= 256, 1 <= top <= n_clusters, temp > 0: anything else fails through sbr_last_error
 * and sbr_cluster_affil_workspace returns 0. R = 0 returns SBR_OK and launches nothing.
 * Saved for the backward pass (may both be NULL: the evaluation form): row_state [R, 4] = {max_k t / temp, sum_k exp(t / temp - max),
 * max(|W_r|, eps), |W_r| >= eps ? 1 : 0} (16-byte aligned) and mask [R, ceil(n_clusters / 4)] bytes (bits 0 .. 3 of byte q: m of clusters
 * 4 q .. 4 q + 3; bits 4 .. 7: the [-1, 1] clamp was active there). Everything else is recomputed from t.
 * workspace: sbr_cluster_affil_workspace(R, D, n_clusters, 0) bytes for the cosine form (backward: (..., 1)); the logit form needs none.
 * Backward: G [R, C] = dL/dx; the mask carries no gradient (the reference detaches m - p):
 *   dt_k = g_k s'(t_k) mh_k + p_k (g_k s(t_k) - sum_j p_j g_j s(t_j)) / temp,   s = sigmoid
 * logit form: t is the forward input, dt_out [R, C] is written. Cosine form: t is the saved t_out, Gt [R, C] (may be NULL) is an upstream
 * dL/dt_out added inside the kernel (the user side's gradient into the item logits); the sum passes where the clamp was not active
 * (torch.clamp), a norm below eps takes torch's clamp_min gradient; dW [R, D] (row stride lddw) is written directly — the rows are the
 * table — and dCl [C, D]; either may be NULL.
 * One form only: dCl is one partial per workgroup folded in workgroup order, no atomics; the number of workgroups depends on
 * (R, D, n_clusters) only — valid in deterministic mode, never a non-deterministic launch. */
long sbr_cluster_affil_workspace(long R, int D, int n_clusters, int backward);
int sbr_cluster_affil_fwd(const float* W, long ldw, const float* Cl, const float* t_in, long R, int D, int n_clusters, int top,
                          float temp, float* t_out, float* x_out, float* row_state, unsigned char* mask, void* workspace,
                          long workspace_bytes, void* stream);
int sbr_cluster_affil_bwd(const float* G, const float* Gt, const float* W, long ldw, const float* Cl, const float* t, long R, int D,
                          int n_clusters, float temp, const float* row_state, const unsigned char* mask, float* dW, long lddw,
                          float* dCl, float* dt_out, void* workspace, long workspace_bytes, void* stream);
/* SGDBaseline — algorithms/sgd_alg.py:110-119 */
int sbr_bias_score_fwd(const float* user_bias, const float* item_bias, const float* global_bias, const long* u, const long* i,
                       float* out, long B, int N, void* stream);
/* bias terms of SGDMatrixFactorization.combine_user_item_representations — algorithms/sgd_alg.py:186-194 (and SGDBaseline in
 * training): out[b, n] = base[b, n] + user_bias[u[b]] + item_bias[i[b, n]] + global_bias[0]; every term may be NULL; u NULL: row b,
 * i NULL: column n (all-pairs scoring against a gathered bias vector). Backward: the bias-table gradients are accumulated
 * (zero-initialise them), NULL ones skipped; d base = g. */
int sbr_bias_score_add_fwd(const float* user_bias, const float* item_bias, const float* global_bias, const long* u, const long* i,
                           const float* base, float* out, long B, int N, void* stream);
int sbr_bias_score_bwd(const float* g, const long* u, const long* i, float* d_user_bias, float* d_item_bias, float* d_global_bias,
                       long B, int N, void* stream);

/* ---- BatchNorm1d (+ fused activation) — modules/polylinear.py:61,68; algorithms/sgd_alg.py:1837 ---------------------------
 * ws: 34*D doubles of workspace (2*D totals + 16 replicas that spread the per-block atomics); ZERO on first use, every call
 * leaves the replicas zeroed again (forward and backward may share one workspace). running_mean/var/num_batches_tracked may be NULL. */
int sbr_bn_train_fwd(const float* X, float* Y, long n, int D, const float* weight, const float* bias, float* running_mean,
                     float* running_var, long* num_batches_tracked, float* save_mean, float* save_rstd, double* ws, float eps,
                     float momentum, int act, void* stream);
int sbr_bn_eval_fwd(const float* X, float* Y, long n, int D, const float* weight, const float* bias, const float* running_mean,
                    const float* running_var, float eps, int act, void* stream);
int sbr_bn_train_bwd(const float* dY, const float* Y, const float* X, float* dX, long n, int D, const float* weight,
                     const float* save_mean, const float* save_rstd, float* dWeight, float* dBias, double* ws, int act,
                     void* stream);

/* statistics half of sbr_bn_train_fwd: batch mean / rstd + running-statistics update, no normalising pass (the consumer
 * normalises on the fly: sbr_bn_score_fwd). */
int sbr_bn_train_stats(const float* X, long n, int D, float* running_mean, float* running_var, long* num_batches_tracked,
                       float* save_mean, float* save_rstd, double* ws, float eps, float momentum, void* stream);
/* the same statistics from sums that the producing GEMM left pending in `ws` (sbr_gemm_split_f32, mode 0, colsum_ws != NULL: per-column
 * sums and sums of squares of its output in the column-reduction replica layout): no pass over the BatchNorm's input at all */
int sbr_bn_finalize_stats(long n, int D, float* running_mean, float* running_var, long* num_batches_tracked, float* save_mean,
                          float* save_rstd, double* ws, float eps, float momentum, void* stream);

/* ---- trailing BatchNorm1d fused with the training scorer (one modality per slot) — algorithms/sgd_alg.py:1834-1837,
 * 1871-1877 (sb_net's trailing BatchNorm1d, no activation) followed by einsum('be,bce->bc') sgd_alg.py:2114, forward and
 * autograd: the normalised item representation [B*N, D] and its gradient are never stored (csrc/fused_tail.hip).
 *   fwd:        logits[b, n] = sum_d U[b, d] * ((Z[s, d] - mean[d]) * rstd[d] * weight[d] + bias[d]),  s = b*N + n
 *   bwd_stats:  dU[b, :] = sum_n G[b, n] * y[s, :];  ws[0..2D) = column sums of dy and dy * xhat, dy[s, :] = G[s] * U[b, :]
 *   bwd_apply:  dX = weight * rstd * (dy - mean(dy) - xhat * mean(dy * xhat)); dWeight / dBias of the BatchNorm from ws;
 *               ws_colsum (17*D doubles, may be NULL): pending column sums of dX (bias gradient of the Linear in front of the
 *               BatchNorm), completed by sbr_colred_finish.
 * ws: the BatchNorm's 34*D-double workspace (contract of sbr_bn_train_fwd). D % 4 == 0, D <= 256, 16-byte aligned operands
 * (sbr_bn_score_supported). */
int sbr_bn_score_supported(int D);
int sbr_bn_score_fwd(const float* Z, const float* U, const float* mean, const float* rstd, const float* weight, const float* bias,
                     float* logits, long B, int N, int D, void* stream);
int sbr_bn_score_bwd_stats(const float* G, const float* U, const float* Z, float* dU, long B, int N, int D, const float* weight,
                           const float* bias, const float* save_mean, const float* save_rstd, double* ws, void* stream);
int sbr_bn_score_bwd_apply(const float* G, const float* U, const float* Z, float* dX, long B, int N, int D, const float* weight,
                           const float* save_mean, const float* save_rstd, const double* ws, float* dWeight, float* dBias,
                           double* ws_colsum, void* stream);
/* sbr_bn_score_fwd + sbr_rec_loss_fwd_bwd (train/rec_losses.py:43-113, upstream gradient 1) + sbr_bn_score_bwd_stats in ONE
 * launch (new: the fused training step): a user's N slot rows of Z stay in registers between the logits and the backward
 * statistics, logits / dlogits make no round trip between kernels. logits may be NULL; dlogits [B, N]; dU [B, D]; loss_out [1];
 * out3 (may be NULL) = (loss, loss, 0): the packed (total, rec, reg) scalars of a step without regularisation losses. ws: the
 * BatchNorm's workspace as for sbr_bn_score_bwd_stats (totals in ws[0 .. 2 D) afterwards, ready for sbr_bn_score_bwd_apply);
 * lws: sbr_bn_score_loss_workspace() bytes, zeroed ONCE by the caller; every call resets the arrival counter in its first word and
 * overwrites the block partial sums behind it before it reads them (calls that share it must not overlap). kind / labels / scale / shift as for sbr_rec_loss_fwd_bwd. N <= D / 4 and N <= 16 (sbr_bn_score_loss_supported). */
int sbr_bn_score_loss_supported(int D, int N);
long sbr_bn_score_loss_workspace(void);
int sbr_bn_score_loss_fwd_bwd(const float* Z, const float* U, const float* save_mean, const float* save_rstd, const float* weight,
                              const float* bias, int kind, const double* labels, double scale, float shift, float* logits,
                              float* dlogits, float* dU, double* loss_out, double* out3, long B, int N, int D, double* ws, void* lws,
                              long lws_bytes, void* stream);

/* sbr_act_grad_gather that also accumulates the column sums of dZ (the bias gradient of its layer, modules/polylinear.py:51)
 * into a column-reduction workspace (17*C doubles, contract of sbr_colsum); sbr_colred_finish turns up to 8 pending
 * workspaces into float vectors (out[q][c] = sum over the replicas of workspaces[q], replicas re-zeroed) with one launch.
 * workspaces / outs: HOST arrays of device pointers, widths: HOST array. */
int sbr_act_grad_colsum_supported(int C);
int sbr_act_grad_gather_colsum(const float* dY, const float* Y, long ld, const int* in_idx, float* dZ, long ldz, long n, int C,
                               int act, double* ws, void* stream);
int sbr_colred_finish(int count, const void* const* workspaces, const void* const* outs, const int* widths, void* stream);

/* ---- losses ----------------------------------------------------------------------------------------------------------------
 * RecBinaryCrossEntropy / RecBayesianPersonalizedRankingLoss / RecSampledSoftmaxLoss .compute_loss —
 * train/rec_losses.py:43-58, 63-83, 88-113. labels: float64 [B, N] (unused for sampled softmax). scale = 1/count for
 * aggregator 'mean' (count = B*N bce, B*(N-1) bpr, B sampled softmax), 1 for 'sum'. shift = log(n_items / n_neg) for the
 * 'uniform' strategy of sampled softmax, else 0. loss_out: one double. */
int sbr_rec_loss_fwd(int kind, const float* logits, const double* labels, long B, int N, double scale, float shift,
                     double* loss_out, void* stream);
int sbr_rec_loss_bwd(int kind, const float* logits, const double* labels, long B, int N, double scale, float shift,
                     const void* grad_out, int grad_out_is_double, float* dlogits, void* stream);
/* both in one pass with upstream gradient 1 (the training step: total.backward() of train/trainer.py:213-221) */
int sbr_rec_loss_fwd_bwd(int kind, const float* logits, const double* labels, long B, int N, double scale, float shift,
                         double* loss_out, float* dlogits, void* stream);
/* the same in ONE launch (new: the fused training step; sbr_rec_loss_fwd_bwd zeroes loss_out with a launch of its own and sums the
 * block partial sums with double atomics): the partial sums go through ws — sbr_rec_loss_workspace(B) bytes, zeroed ONCE by the
 * caller; every call resets the arrival counter in its first word and overwrites the partial sums behind it before it reads them;
 * calls sharing a workspace must not overlap — and are added in block order (the same bits on
 * every run). out3 (may be NULL): also writes (loss, loss, 0), the packed (total, rec, reg) scalars of a step without
 * regularisation losses (what sbr_pack_losses would produce). B >= 1. */
long sbr_rec_loss_workspace(long B);
int sbr_rec_loss_fwd_bwd_ws(int kind, const float* logits, const double* labels, long B, int N, double scale, float shift,
                            double* loss_out, float* dlogits, double* out3, void* ws, long ws_bytes, void* stream);

/* InfoNCE.forward — train/regularization_losses.py:14-43, called from algorithms/sgd_alg.py:1989 on e[..., 0, :] and
 * e[..., 1, :]. G groups of N rows, row stride ld; N <= sbr_infonce_max_n(). scale = 1/(G*N) for 'mean'. */
int sbr_infonce_max_n(void);
int sbr_infonce_fwd(const float* A, const float* B, long ld, long G, int N, int D, float tau, double scale, double* loss_out,
                    void* stream);
int sbr_infonce_bwd(const float* A, const float* B, long ld, long G, int N, int D, float tau, double scale,
                    const float* grad_out, float* dA, float* dB, long ldg, void* stream);

/* out3 = (rec + reg, rec, reg), reg = w_a * reg_a + w_b * reg_b: the total loss of train/trainer.py:213-216 from the device-side
 * loss scalars (reg_a / reg_b may be NULL). */
int sbr_pack_losses(const double* rec, const double* reg_a, double w_a, const double* reg_b, double w_b, double* out3,
                    void* stream);

/* The same loss for groups of any size (in-batch contrast of B user rows, sgd_alg.py:1994-2002): the N x N logits go
 * through the fp32 MFMA GEMMs (sbr_gemm_f32 / sbr_gemm_tn_f32) instead of LDS. workspace: sbr_infonce_gemm_workspace(N, D)
 * bytes of device memory (logits, log-sum-exps, split-K slabs); groups are processed sequentially. Same argument meaning as
 * sbr_infonce_fwd / sbr_infonce_bwd; the backward recomputes the logits. */
long sbr_infonce_gemm_workspace(int N, int D);
int sbr_infonce_gemm_fwd(const float* A, const float* B, long ld, long G, int N, int D, float tau, double scale,
                         double* loss_out, void* workspace, long workspace_bytes, void* stream);
int sbr_infonce_gemm_bwd(const float* A, const float* B, long ld, long G, int N, int D, float tau, double scale,
                         const float* grad_out, float* dA, float* dB, long ldg, void* workspace, long workspace_bytes,
                         void* stream);

/* ---- dense optimizers over one flat fp32 buffer — train/trainer.py:62-68, 222 ---------------------------------------------
 * kind 0 = torch.optim.AdamW, 1 = torch.optim.Adam; step is the 1-based step count. */
int sbr_adam_step(int kind, float* p, const float* g, float* m, float* v, long n, double lr, double b1, double b2, double eps,
                  double wd, long step, void* stream);
/* optimizer.step(); optimizer.zero_grad() (train/trainer.py:221-222) in one launch: every gradient element is reset to +0 once it
 * has been consumed; elements that are +0 already are not written. */
int sbr_adam_step_zero_grad(int kind, float* p, float* g, float* m, float* v, long n, double lr, double b1, double b2, double eps,
                            double wd, long step, const double* copy_src, double* copy_dst, int copy_n, void* stream);
/* copy_n (0 .. 256) doubles copy_src -> copy_dst ride on the same launch: the loss scalars of a captured step, whose buffer the
 * next replay overwrites (copy_n = 0: no copy). */
/* The same dense-optimizer semantics for a [n_rows, D] lookup table, deferred row by row (train/trainer.py:62-68 updates every row
 * every step; a row without gradient can take its zero-gradient updates later, in order, bit-identically — for every eps the
 * caller passes: the replay's short cut for rows whose first moment is exactly zero is taken only when eps > 0 (as rounded to fp32),
 * where the dense step's denominator is positive; with eps = 0 such a row is replayed through the full step and, like the dense
 * kernel and torch.optim.AdamW, ends with NaN parameters where its second moment is zero). mode 0: bring the rows
 * named by ids (int64 or int32, optionally through rowmap) up to step - 1 (before the forward pass reads them); mode 1: the same,
 * then apply `step` with their gradient rows, zero those gradient rows, record the step's scalars in sched[step]; mode 2: flush
 * every row to `step` (before any other reader). claim, last: int32 [n_rows * ceil(D / 64)] (one entry per 64-element sub-row, the
 * work of one wave), zero-initialised; sched: float2 [> step]. */
int sbr_adam_rows(int kind, int mode, float* p, float* g, float* m, float* v, long n_rows, int D, const long* ids64, const int* ids32,
                  const int* rowmap, long n, int* claim, int* last, void* sched, double lr, double b1, double b2, double eps,
                  double wd, long step, void* stream);
/* optimizer.step() + zero_grad() of a step whose flat buffers (n elements) hold ONE deferred table in [lo, hi): mode 1 of
 * sbr_adam_rows for the table's rows named by ids and sbr_adam_step_zero_grad for every other element, in one launch; rows of the
 * table that received no gradient are not touched — except the n_sweep sub-rows (64-element pieces of rows, in table order) from
 * sweep_lo on, cyclically, which are brought up to `step` beside the dense part's memory stream: a caller that sweeps 1 / W of the
 * table per step bounds every row's backlog — the length of a catch-up or flush replay — by W steps. n_sweep > 0 requires that
 * the step's catch-up (sbr_adam_rows mode 0 with the same ids and step) ran before: the sweep recognises the batch's rows by its
 * claims and leaves them to their update (new in ABI 3). p / g / m / v need only 4-byte alignment: the dense part uses 16-byte
 * accesses when lo, hi, n are multiples of 4 and all four pointers are 16-byte aligned, and the element loop (same bits) otherwise. */
int sbr_adam_step_rows(int kind, float* p, float* g, float* m, float* v, long n, long lo, long hi, int D, const long* ids64,
                       const int* ids32, const int* rowmap, long n_ids, int* claim, int* last, void* sched, double lr, double b1,
                       double b2, double eps, double wd, long step, long sweep_lo, long n_sweep, const double* copy_src,
                       double* copy_dst, int copy_n, void* stream);
int sbr_adagrad_step(float* p, const float* g, float* state_sum, long n, double lr, double eps, double wd, void* stream);

/* ---- full-catalogue evaluation — eval/eval.py:205-222 ------------------------------------------------------------------------
 * exclusion mask out[b, excl(u_b)] = -inf (eval/eval.py:219-220) from the CSR `exclude_data` (data/dataset.py:416-438) */
int sbr_mask_scores(float* scores, long ld, const long* u_idx, const long* excl_indptr, const int* excl_indices, long Bu,
                    void* stream);
/* the same when `scores` holds the item columns [item_offset, item_offset + n_cols) only (new: item-sharded evaluation) */
int sbr_mask_scores_shard(float* scores, long ld, const long* u_idx, const long* excl_indptr, const int* excl_indices, long Bu,
                          int item_offset, int n_cols, void* stream);
/* exact per-row top-k, sorted by (score desc, index asc) — torch.topk at eval/eval.py:320 and inside rmet.calculate. The list is the
 * first k of the stable descending order of the row (torch.sort(descending=True, stable=True)): every NaN, whatever its sign bit,
 * ranks ahead of +inf; -0.0 and +0.0 are the same score; equal scores (NaNs among themselves, the two zeros) go in ascending index.
 * A NaN is returned as a NaN (not necessarily the same bits), a zero as +0.0, every other value bit for bit. 1 <= k <= min(I, 256). */
int sbr_topk_rows(const float* scores, long ld, long Bu, int I, int k, float* out_val, int* out_idx, void* stream);
/* exact merge of W per-shard top-k lists of an item-sharded evaluation (new: the reference has no multi-GPU path):
 * vals / idxs: [W, Bu, k] (all-gathered; idx < 0 = empty slot, idx = global item index), W * k <= 256 -> [Bu, k] sorted by
 * (score desc, index asc) under the rule of sbr_topk_rows (NaN first, -0.0 == +0.0, ties by ascending item index). An empty slot
 * ranks behind every real entry — a real entry whose score is -inf keeps its index and precedes it — and comes out as (-inf, -1). */
int sbr_merge_topk(const float* vals, const int* idxs, int W, long Bu, int k, float* out_val, int* out_idx, void* stream);
/* NDCG / recall / precision @ ks from top-k indices and CSR labels — eval/metrics.py:4-105. out: [3, n_ks, Bu]. */
int sbr_rank_metrics(const int* topk_idx, int kmax, const long* u_idx, const long* label_indptr, const int* label_indices,
                     long Bu, const int* ks, int n_ks, float* out, void* stream);
/* The rank-position metrics DCG / average precision / reciprocal rank @ ks: what `config.metrics` may name beyond the three above when
 * the reference hands it to `rmet.calculate` (eval/eval.py:99-102; its analysis configuration asks for 'ap',
 * utilities/analysis_utils.py:260). `rmet` is absent offline, so the definitions are this project's and parity-unpinned against it.
 * Binary relevance; hit_r = [topk_idx[b, r] in labels(u_b)] (a slot holding -1 is never a hit; a repeated item counts again),
 * h_r = the hits at ranks <= r, n_pos = the length of the label row:
 *   dcg@k = sum_{r < k, hit_r} 1 / log2(r + 2)
 *   ap@k  = (sum_{r < k, hit_r} h_r / (r + 1)) / min(k, n_pos)        (0 when n_pos == 0)
 *   rr@k  = 1 / (r0 + 1), r0 the smallest r < k with hit_r             (0 without one)
 * out: [3, n_ks, Bu] in the order (dcg, ap, rr). Operands and conventions of sbr_rank_metrics: CSR labels over user ids, columns
 * ascending within a row, u_idx == NULL means row b, ks ascending and <= kmax, at most 8 cut-offs; any kmax >= 1. The float order is
 * fixed: both sums run over the hits in ascending rank, one fp32 addition per hit starting from 0.f; a term is one correctly rounded
 * fp32 division (1.f / log2f((float)(r + 2)), (float)h_r / (float)(r + 1)) of exactly converted integers, and so are the final
 * apn / (float)min(k, n_pos) and 1.f / (float)(r0 + 1). One wave per user, 64 ranks per step: a coalesced load, a binary search per
 * lane, a ballot for the hit mask, and a walk of its set bits (serial in the hits, not in kmax). No LDS, no atomics, one writer per
 * element: the same bits on every run, valid in deterministic mode. A refused call writes nothing; Bu == 0 returns without a launch.
 * New (additive to ABI 4). */
int sbr_rank_metrics_pos(const int* topk_idx, int kmax, const long* u_idx, const long* label_indptr, const int* label_indices,
                         long Bu, const int* ks, int n_ks, float* out, void* stream);
/* fused scorer: fp16 MFMA  U[Bu, D] x I[I_s, D]^T  with the exclusion mask and the running per-user top-k kept on chip; the
 * [Bu, I_s] score matrix is never written (BASELINE config 5). D in {64, 128, 256}, 1 <= k <= 128 (k > 32 runs the wide
 * instantiation of the one-pass kernel: same contract, same score bits; the two-pass route takes k <= 32 only and answers a longer
 * list with an error). Output sorted by (score desc, item
 * index asc); indices are global (item_offset + column). u_idx: exclusion-CSR row of every scored row (NULL: identity).
 * excl_nnz: number of entries of `excl_indices` (an upper bound of the exclusions of the scored rows).
 * PRECONDITION: the lengths of the scored rows' parts inside [item_offset, item_offset + I), summed over all Bu scored rows, must not
 * exceed excl_nnz; a row that u_idx names more than once counts once per repetition. The event buffer is sized from excl_nnz: past
 * the bound a user group's slice of the stream is left unwritten and the kernel reads events that were never built. The CSR's total
 * (what the Python layer `ops` passes) satisfies it whenever the entries of u_idx are distinct; a user list with repetitions may
 * exceed it, and such a caller has to pass a CSR (or an excl_nnz together with an event buffer) sized for the repeated rows.
 * Exclusions reach the kernel as an EVENT STREAM built from the CSR rows (csrc/score_topk_f16_n.hip) in the caller-owned buffer
 * `events` (sbr_score_topk_f16_events_bytes(Bu, excl_nnz) bytes; NULL without exclusions): build_events != 0 builds it first (three
 * small launches), 0 means the buffer holds the stream an earlier call with the same (u_idx, CSR, item_offset, I, D) built — the
 * exclusion mask of an evaluation split (eval/eval.py:219: dataset.exclude_data) is the same for every evaluation of the split.
 * ABI 3: events / events_bytes / build_events are new, the workspace no longer holds the event stream. */
int sbr_score_topk_f16(const void* U_f16, const void* I_f16, int D, long Bu, int I, const long* u_idx,
                       const long* excl_indptr, const int* excl_indices, long excl_nnz, int item_offset, int k, float* out_val,
                       int* out_idx, void* workspace, long workspace_bytes, void* events, long events_bytes, int build_events,
                       void* stream);
/* bytes of `workspace` for the call above on the route selected now (sbr_score_topk_f16_route): per-user candidate buffers (4 KB per
 * user: scratch written by the wave that owns the user and read by the final-selection launch of the same call; contents need no
 * initialisation) + their fill counts; under route 2 the larger of that and the two-pass scorer's buffers. Query again after switching
 * the route: a call with a workspace too small for its route fails with an error. */
long sbr_score_topk_f16_workspace(long Bu, int I, int k);
long sbr_score_topk_f16_events_bytes(long Bu, long excl_nnz);
/* ABI 4: which of the two fused scorers sbr_score_topk_f16 runs. 0 (default): the one-pass kernel (csrc/score_topk_f16_n.hip) for every
 * shape (automatic: it stays there until the two-pass scorer is the faster one); 1: always one-pass; 2: the two-pass scorer
 * (csrc/score_topk_f16_2p.hip: a pure MFMA + group-maxima pass, then the ~3 % of the scores at or above each user's bound are recomputed
 * group by group) for catalogues of >= 8,192 items, or an error. Both return the same lists bit for bit (same MFMA chain per score); the
 * switch exists for tests and A/B timing. Returns the previous setting; a value outside 0..2 only queries. Process-wide. */
int sbr_score_topk_f16_route(int route);
/* fp32 -> fp16 cast of an embedding matrix (row-major, contiguous) */
int sbr_cast_f32_to_f16(const float* X, void* Y_f16, long n, void* stream);
/* fused scorer with fp32-class products (eval/eval.py:216-222: einsum('be,ce->bc') in fp32, -inf on the exclusions, top-k): the
 * contract of sbr_score_topk_f16 (output order, global indices, u_idx, (-inf, -1) padding, event-buffer protocol) on fp32 user rows
 * U_f32 [Bu, D] and the three bf16 planes of the item matrix (sbr_split_f32_to_bf16x3), multiplied on the bf16 matrix pipe as the six
 * leading partial products of the exact splits with fp32 accumulation (csrc/score_topk_f32s.hip). D in {64, 128}, 1 <= k <= 128
 * (k > 32: the wide instantiation). The event
 * buffer has sbr_score_topk_f16_events_bytes(Bu, excl_nnz) bytes, but the stream in it is laid out for this kernel's 32-item tiles:
 * a buffer built by sbr_score_topk_f16 must not be passed with build_events = 0, nor the other way round. New (additive to ABI 4). */
int sbr_score_topk_f32s(const float* U_f32, const void* I_bf16x3, int D, long Bu, int I, const long* u_idx,
                        const long* excl_indptr, const int* excl_indices, long excl_nnz, int item_offset, int k, float* out_val,
                        int* out_idx, void* workspace, long workspace_bytes, void* events, long events_bytes, int build_events,
                        void* stream);
/* bytes of `workspace` for sbr_score_topk_f32s (candidate buffers + fill counts of this route only; eval/eval.py:216-222) */
long sbr_score_topk_f32s_workspace(long Bu, int I, int k);
/* sbr_score_topk_f32s for 256-wide representations (eval/eval.py:216-222): the same operands, arithmetic, output contract and
 * event-buffer protocol (32-item tiles: a stream built by either of the two entries for the same users, mask, item range and D may
 * be handed to that entry again), from kernels of their own: one wave per SIMD, three consumer waves and a loader wave per workgroup
 * (csrc/score_topk_f32s.hip). D must be 256 and k lie in [1, 128] (k > 32: the wide instantiation). New (additive to ABI 4). */
int sbr_score_topk_f32s_d256(const float* U_f32, const void* I_bf16x3, int D, long Bu, int I, const long* u_idx,
                             const long* excl_indptr, const int* excl_indices, long excl_nnz, int item_offset, int k, float* out_val,
                             int* out_idx, void* workspace, long workspace_bytes, void* events, long events_bytes, int build_events,
                             void* stream);
/* bytes of `workspace` for sbr_score_topk_f32s_d256 (candidate buffers + fill counts of its workgroup geometry; does not depend on I
 * or k; eval/eval.py:216-222) */
long sbr_score_topk_f32s_d256_workspace(long Bu, int I, int k);
/* X (fp32, n elements, contiguous) -> three bf16 planes Y[0..n), Y[n..2n), Y[2n..3n) (each plane rounded to nearest even from the
 * remainder); X = Y0 + Y1 + Y2 exactly for x = 0 and 2^-100 <= |x| <= 3.38e38 (below, the third plane underflows; above, and for inf / NaN,
 * the remainder planes are NaN: such item values are not supported): the item operand of sbr_score_topk_f32s (eval/eval.py:216-222) */
int sbr_split_f32_to_bf16x3(const float* X, void* Y_bf16x3, long n, void* stream);

/* ---- neighbourhood models on 0/1 data (csrc/knn.hip) ---------------------------------------------------------------------------
 * compute_similarity_top_k + compute_*_sim_mtx — utilities/similarities.py:18-130 (called from algorithms/knn_algs.py:94, :114).
 * X [n, m]: binary CSR (indptr int64 [n + 1], indices int32 sorted ascending within a row, unique; no values: every entry is 1),
 * X^T [m, n] in the same form (t_indptr, t_indices); m <= 2^24. For every row i of [r0, r1) the candidates are the rows j != i with
 * c = |row i & row j| > 0; with ni, nj the entry counts of the two rows, all in fp32, one correctly rounded operation per step, no
 * contraction, integers converted once (they are exact):
 *   sim 0 cosine             v = c / (sqrtf(ni) * sqrtf(nj))
 *   sim 1 jaccard            v = c / float(ni + nj - c)
 *   sim 2 asymmetric_cosine  v = c / (powf(ni, alpha) * powf(nj, 1.f - alpha))
 *   sim 3 sorensen_dice      v = (2.f * c) / float(ni + nj)
 *   sim 4 tversky            v = c / ((c + alpha * float(ni - c)) + beta * float(nj - c))
 *   value = v * (c / (c + shrinkage))
 * The list of row i is the first min(k, candidates) of them by (value descending, index ascending), the rule of sbr_topk_rows:
 * nbr_idx int32 [n, k], nbr_val fp32 [n, k], nbr_len int32 [n]; the slots behind nbr_len[i] hold (-1, 0). Only the rows of [r0, r1)
 * are written. 1 <= k <= 256; alpha, beta, shrinkage >= 0. tile_cols: entity columns per tile of LDS counters (4 bytes each);
 * 0 = min(max(n, 64), 32768); a request over 160 KiB of LDS is an error. Integer LDS atomics only: the same bits on every run,
 * valid in deterministic mode. New (additive to ABI 4). */
int sbr_knn_topk(const long* indptr, const int* indices, const long* t_indptr, const int* t_indices, int n, int m, int r0, int r1,
                 int sim, float alpha, float beta, float shrinkage, int k, int tile_cols, int* nbr_idx, float* nbr_val, int* nbr_len,
                 void* stream);
/* out[b, 0 .. n_cols) = X[rows[b]] . Y as dense fp32 rows with leading dimension ld (rows NULL: row b) — both predictions:
 * `matrix @ sim_mtx.T` (algorithms/knn_algs.py:116: X = interactions, Y = S^T) and `sim_mtx @ matrix` (knn_algs.py:96: X = S,
 * Y = interactions). X and Y are CSR (indptr int64, indices int32 sorted ascending and unique within a row); x_data / y_data fp32 or
 * NULL = ones. An element starts at +0 and receives its terms in ascending order of X's column as acc = fmaf(x, y, acc): one owner, one
 * rounding per term, no atomics, the same bits on every run. Every element of the addressed rows' [0, n_cols) is written (zeros
 * included), nothing else. tile_cols: columns per workgroup (0 = min(n_cols, 8192); at most 16384). New (additive to ABI 4). */
int sbr_csr_rows_times_csr(const long* x_indptr, const int* x_indices, const float* x_data, const long* rows, long B,
                           const long* y_indptr, const int* y_indices, const float* y_data, int n_cols, int tile_cols, float* out,
                           long ld, void* stream);

/* ---- neighbourhood model on dense features (csrc/dense_knn.hip) ------------------------------------------------------------------
 * compute_similarity_top_k + dense_compute_cosine_sim_mtx — utilities/similarities.py:18-61, :86-93 (called from
 * algorithms/knn_algs.py:136, ItemFeatureKNN). F [n, d]: fp32 rows with leading dimension ld >= d; 1 <= d <= 8192. All in fp32, one
 * correctly rounded operation per step, no contraction other than the fmaf named here:
 *   q_i     = sum_k F[i,k]^2      as q = fmaf(F[i,k], F[i,k], q) from +0 over k ascending;   norm_i = sqrtf(q_i)
 *   dot_ij  = sum_k F[i,k] F[j,k] as acc = fmaf(F[i,k], F[j,k], acc) from +0 over k ascending (the fp32 matrix pipe computes exactly
 *             this chain): the same order for every pair, whatever tile it falls in and whatever [r0, r1) is, so dot_ij and dot_ji,
 *             and dot_ii and q_i, carry the same bits
 *   j != i  v = dot_ij / (norm_i * norm_j);  shrinkage > 0: value = v * (dot_ij / (dot_ij + shrinkage));  shrinkage == 0: value = v
 *   j == i  value = +0
 * j is a candidate of i iff dot_ij != 0 (j = i included when q_i > 0): the entries scipy's coo_matrix keeps of the dense product. A
 * value of -0 is ranked and written as +0. The list of row i is the first min(k, candidates) of them by (value descending, index
 * ascending), the rule of sbr_topk_rows, selected on the order-preserving unsigned key of the float (negative: all bits flipped;
 * otherwise: the sign bit set), so negative values rank below the self entry's +0: nbr_idx int32 [n, k], nbr_val fp32 [n, k],
 * nbr_len int32 [n]; the slots behind nbr_len[i] hold (-1, +0). Only the rows of [r0, r1) are written; r0 == r1 returns without a
 * launch. sbr_row_norms_f32 writes norm_i of every row into norms [n]; sbr_dense_knn_topk takes that array (the caller may look at
 * it in between: a non-finite or overflowed norm is the caller's to refuse). Columns [d, ld) and rows >= n of a larger allocation are
 * never multiplied. 1 <= k <= 256; n k < 2^31; shrinkage >= 0 (a negative dot with shrinkage > 0 can meet the pole of
 * dot / (dot + shrinkage): the result is then whatever fp32 gives, ranked by its key). No workspace: nothing of size n x n or
 * rows x n leaves the chip. No float atomics (integer LDS atomics hand out buffer slots; the selection does not depend on the slot
 * order): the same bits on every run and for every split of the row range, valid in deterministic mode. New (additive to ABI 4). */
int sbr_row_norms_f32(const float* F, int n, int d, long ld, float* norms, void* stream);
int sbr_dense_knn_topk(const float* F, const float* norms, int n, int d, long ld, int r0, int r1, float shrinkage, int k,
                       int* nbr_idx, float* nbr_val, int* nbr_len, void* stream);

/* ---- EASE on 0/1 data (csrc/ease.hip) ------------------------------------------------------------------------------------------
 * G = X^T X + diag_add I — algorithms/linear_algs.py:150-153 (`matrix.transpose().dot(matrix).toarray()`, `G[diag] += int(lam)`) as
 * dense fp32 rows G [m, m] with leading dimension ld >= m. X [n, m] and X^T in the forms sbr_knn_topk takes (binary CSR, sorted,
 * unique); n <= 2^24, so every count converts to fp32 exactly. A workgroup owns row i of [r0, r1): it walks X^T's row i and, for every
 * user in it, that user's row of X, counting into int32 LDS counters (integer atomics); each count is converted once, diag_add is
 * added to the diagonal element (one fp32 addition) and the whole row [0, m) is written, zeros included. Only the rows of [r0, r1)
 * are written. tile_cols: columns per tile of counters (4 bytes each); 0 = min(max(m, 64), 32768), the default of sbr_knn_topk; a
 * request over 160 KiB of LDS is an error. The same bits on every run, valid in deterministic mode. New (additive to ABI 4). */
int sbr_gram_dense(const long* indptr, const int* indices, const long* t_indptr, const int* t_indices, int n, int m, int r0, int r1,
                   float diag_add, int tile_cols, float* G, long ld, void* stream);
/* A <- A^-1 in place for a symmetric positive definite fp32 A [n, n], leading dimension ld >= n — `np.linalg.inv(G)`,
 * algorithms/linear_algs.py:155. Blocked symmetric sweep, pivot blocks K = [k0, min(k0 + 64, n)) in ascending order, three launches
 * per block:
 *   1. one workgroup inverts D = A[K, K] by unpivoted Gauss-Jordan (step p: d = 1 / D[p][p]; D[p][p] = d; D[p][j] = D[p][j] * d;
 *      D[i][p] = -D[i][p] * d; D[i][j] = D[i][j] - D[i][p] * (D[p][j] * d) for i, j != p) and sets *info = 1 + (k0 + p) at the first
 *      pivot that is <= 0 or not finite, if *info is still 0;
 *   2. P = A[K, :], R = D^-1 P with R[p][j] = fmaf(D^-1[p][q], P[q][j], .) over q ascending from +0;
 *   3. A[i][j] <- A[i][j] - S[i][j], S[i][j] = fmaf(P[p][i], R[p][j], .) over p ascending from +0 (the fp32 matrix pipe: the same
 *      bits as the fmaf chain), for i, j outside K; A[K, j] <- R[:, j], A[i, K] <- R[:, i]^T, A[K, K] <- -D^-1.
 * After the last block A = -A_in^-1; the last update stores the negated values. Every element has one owner per launch, no float
 * atomics: the same bits on every run, valid in deterministic mode. Elements outside the n x n view are neither read nor written.
 * info: one device int32, zero on entry; non-zero afterwards = the matrix was not positive definite in fp32 and A holds no inverse
 * (an error return, not a fault). workspace: sbr_spd_inverse_f32_workspace(n) bytes at a 16-byte boundary. n = 0 returns at once.
 * New (additive to ABI 4). */
int sbr_spd_inverse_f32(float* A, int n, long ld, void* workspace, long workspace_bytes, int* info, void* stream);
/* bytes of `workspace` for sbr_spd_inverse_f32: D^-1 [64, 64] and the two panels P, R [64, n rounded up to 128]
 * (algorithms/linear_algs.py:155) */
long sbr_spd_inverse_f32_workspace(int n);
/* B[i][j] = P[i][j] / (-P[j][j]) for i != j, B[j][j] = 0, in place on P [n, n] with leading dimension ld —
 * algorithms/linear_algs.py:157-158 (`P / (-np.diag(P))` divides column j; B is not symmetric). One correctly rounded fp32
 * division per element. diag: n floats of scratch (the diagonal is read before it is overwritten; it holds the original diagonal
 * afterwards). New (additive to ABI 4). */
int sbr_ease_weights_f32(float* P, int n, long ld, float* diag, void* stream);

/* ---- SLIM on 0/1 data (csrc/slim.hip) ------------------------------------------------------------------------------------------
 * The item-item weights of algorithms/linear_algs.py:39-112 (sklearn's ElasticNet with positive=True, fit_intercept=False, once per
 * item j on the users x items matrix with column j zeroed), solved from the Gram matrix alone. G [m, m]: X^T X as sbr_gram_dense
 * counts it (diag_add = 0), symmetric fp32 with leading dimension ldg; its diagonal is read in place. With q = G[:, j], q_j = 0, and
 * l1 = n alpha l1_ratio, l2 = n alpha (1 - l1_ratio) for n users, column j minimises sklearn's objective times n,
 *   1/2 (G_jj - 2 w.q + w.G w) + l1 sum(w) + 1/2 l2 w.w   over w >= 0, w_j = 0,
 * by cyclic coordinate descent in ASCENDING k (the reference: random order; with l2 > 0 the optimum is unique and the order only
 * changes the path). State: w = 0, r = q. A sweep takes every k != j with G_kk > 0 (a zero-norm column is skipped and stays 0):
 *   new = max((r_k + G_kk * w_k) - l1, 0) / (G_kk + l2);  d = new - w_k;  if d != 0: r_x = r_x - d * G[k, x] for every x;  w_k = new,
 * every operation one rounded fp32 operation, nothing fused. The kernel searches for the next coordinate with w_k > 0 or r_k > l1
 * and passes over the others, whose step is zero, so it gives what the plain loop gives. After a sweep, with w_max = max |w_k| and
 * d_w_max = max |d| over it, the column stops when w_max == 0 or d_w_max <= tol * w_max (sklearn's first stopping test; its dual-gap
 * test is not reproduced), or after max_iter sweeps. tol = 0 stops at an exact fixed point or at max_iter.
 * One workgroup owns one target column j of [c0, c1) and writes W[k, j] for every k in [0, m), zeros included (W [m, m] fp32, leading
 * dimension ldw; matrix[u] @ W is the prediction, linear_algs.py:59-61); columns outside the range are untouched. n_iter[j]: the
 * sweeps run, negated when the column stopped at max_iter without meeting the stopping test. r lives in LDS: m <= 40,832 (4 m
 * bytes beside 512 bytes of fixed state in 160 KiB); w lives in the output column. No atomics, no cooperative launch, no workgroup
 * waits on another; every element of r and W has one owner thread: the same bits on every run and for every split of [c0, c1),
 * valid in deterministic mode. l1, l2 and tol must be finite and >= 0, max_iter >= 1. m == 0 or c0 == c1 return at once, before the
 * operands are looked at; a null operand is an error otherwise. New (additive to ABI 4). */
int sbr_slim_cd_f32(const float* G, int m, long ldg, int c0, int c1, float l1, float l2, int max_iter, float tol, float* W, long ldw,
                    int* n_iter, void* stream);

/* ---- the two baselines without a score matrix (csrc/shared_rank.hip) — algorithms/naive_algs.py:11-60 -----------------------------
 * PopularItems (algorithms/naive_algs.py:35-60: `self.pop_distribution[i_idxs]`) gives every user the same score row, so a user's list
 * is the shared ranking minus the user's exclusions (eval/eval.py:219-220, then torch.topk at :320), found with about k + |excl(u)|
 * reads instead of a [Bu, n_items] score matrix. order: int32 [n_items], a permutation of the split's item positions, best first;
 * score: fp32 [n_items], indexed by position, not by rank. The kernel does not sort: whatever `order` says is the ranking (the value
 * rules live where `order` is made: the stable descending order of sbr_topk_rows). The exclusion CSR is the one sbr_mask_scores takes:
 * indptr int64 over user ids, indices int32 ascending and unique within a row, columns = positions in the split; u_idx: int64 [Bu]
 * (NULL = identity), in any order, repeats allowed. Row b of out_val / out_idx [Bu, k] gets (score[p], p) for the first k entries p of
 * `order` that excl(u_b) does not contain, in rank order. One wave per user steps through `order` 64 ranks at a time: a lane tests its
 * entry by a binary search in the CSR row (an empty row skips the test), a ballot of the kept lanes gives each its slot, and the walk
 * stops once k are found or `order` ends. Slots behind a user's last scoreable item get (-inf, -1), the empty-slot convention of the
 * fused scorers and of sbr_merge_topk; a kept item whose score is -inf keeps its index: only empty slots carry -1. k >= 1 with no upper
 * limit (nothing is held on chip; k > n_items just pads). An entry of `order` outside [0, n_items) is passed over, never read through.
 * Bu == 0 returns without a launch. No LDS, no atomics, one writer per output element: the same bits on every run, valid in
 * deterministic mode. New (additive to ABI 4). */
int sbr_shared_rank_topk(const int* order, const float* score, int n_items, const long* u_idx, const long* excl_indptr,
                         const int* excl_indices, long Bu, int k, float* out_val, int* out_idx, void* stream);
/* RandomItems (algorithms/naive_algs.py:11-32: `torch.rand(i_idxs.shape)` from the CPU's global generator, so a list there depends on
 * the batch size, the order of the batches and whatever drew before) as a pure function: out[b, j] = U(seed, u_idx[b], j) for j in
 * [0, n_items), out fp32 with leading dimension ld >= n_items, u_idx int64 [Bu] (NULL = identity). The generator is Philox4x32-10
 * (Salmon et al., SC 2011; written out in csrc/philox.h, no generator library): key = (low, high) 32-bit halves of `seed`, counter =
 * (low half of the user id, high half of the user id, j / 4, 0), and word j % 4 of the output block x maps to (x >> 8) * 2^-24, an
 * exact fp32 in [0, 1). A value depends on nothing but (seed, user id, j): not on the chunk, the launch geometry, ld or the row's
 * place in the batch. Bu == 0 or n_items == 0 returns without a launch. One writer per element, no atomics: valid in deterministic
 * mode. New (additive to ABI 4). */
int sbr_uniform_rows_f32(unsigned long seed, const long* u_idx, long Bu, int n_items, float* out, long ld, void* stream);

/* ---- P3alpha on 0/1 data (csrc/p3alpha.hip) --------------------------------------------------------------------------------------
 * The users x items block of the reference's P^3 (algorithms/graph_algs.py:35-65) is (D_u^-1 X)(D_i^-1 X^T)(D_u^-1 X); its last two
 * factors are the item-item model W [m, m], dense fp32 rows with leading dimension ld >= m — algorithms/graph_algs.py:35-59 (the
 * degree sums, `P = D @ A`, `P ** 3`) without the (U + I) x (U + I) matrices. X [n, m] and X^T in the forms sbr_knn_topk takes (binary
 * CSR, indices ascending and unique); n, m <= 2^24, so every degree converts to fp32 exactly. Degrees are indptr differences;
 * inv(d) = 1.0f / (float)d, one correctly rounded division. For a row i of [r0, r1) the accumulator of column j starts at +0.0f and
 * receives inv(d_v) for the users v of item i that hold item j, in ascending v, by plain fp32 additions (one owner, no atomics); the
 * stored value is acc * inv(d_i): one multiplication, not fused with an addition. A row of an item nobody holds is zeros. Every
 * element [0, m) of an owned row is written, zeros included; only the rows of [r0, r1) are written. tile_cols: columns per tile of
 * LDS accumulators (4 bytes each; each of the workgroup's 16 waves owns a strip of ceil(tile / 16) of them and walks the users by
 * itself, so the order does not depend on the tiling); 0 = min(max(m, 64), 32768), the default of sbr_gram_dense; a request over
 * 160 KiB of LDS is an error. The same bits on every run, valid in deterministic mode. New (additive to ABI 4). */
int sbr_p3_walk_dense(const long* indptr, const int* indices, const long* t_indptr, const int* t_indices, int n, int m, int r0, int r1,
                      int tile_cols, float* W, long ld, void* stream);
/* out[b, j] = (inv(d_u) * sum_i W[i, j]) ^ alpha for u = rows[b] (rows NULL: u = b; duplicates allowed) and 0 <= j < m — the last
 * factor D_u^-1 X of P^3 and `P3.power(self.alpha)`, algorithms/graph_algs.py:59-68, one user chunk at a time (the reference's
 * users x items pred_mtx is never built). X's CSR as above; W [m, m] fp32 with leading dimension ldw; out [B, m] with leading
 * dimension ldo. A thread owns column j: its accumulator starts at +0.0f and receives W[i, j] over the user's items i in ascending
 * order by plain fp32 additions, is multiplied once by inv(d_u) and then raised by powf(., alpha); the power is skipped when
 * alpha == 1.0f (the result is then the product bit for bit) and for a zero, which stays +0. A user without items gives a zero row.
 * alpha must be positive and finite; m <= 2^24. No atomics: the same bits on every run, valid in deterministic mode. New (additive to
 * ABI 4). */
int sbr_p3_score_rows(const long* indptr, const int* indices, const long* rows, long B, const float* W, long ldw, int m, float alpha,
                      float* out, long ldo, void* stream);

/* ---- LightGCN's propagation on 0/1 data (csrc/graph_prop.hip) --------------------------------------------------------------------------
 * y = A^ x with A^ = D^-1/2 A D^-1/2 the normalised adjacency of the bipartite user-item graph (He et al., SIGIR 2020, equation 7), over
 * the joint row space [0, n_users + n_items): joint row r < n_users is user r, whose neighbours are the joint rows n_users + i for the
 * items i of row r of (u_indptr, u_indices), the users x items matrix; joint row r >= n_users is item r - n_users, whose neighbours are
 * the users of row r - n_users of (i_indptr, i_indices), its transpose (both binary CSR in the forms sbr_p3_walk_dense takes: indices
 * ascending and unique; n_users, n_items <= 2^24, so every degree converts to fp32 exactly). x, y and sum are contiguous fp32 tables
 * [n_users + n_items, D] with row stride D (no leading dimension), 1 <= D <= 512. For every row r of [r0, r1) and every d < D:
 *   deg_r = the indptr difference of r's own side;  s_r = 1.0f / sqrtf((float)deg_r): one correctly rounded square root, then one
 *     correctly rounded division (no rsqrt), and s_r = +0.0f when deg_r == 0; s_c likewise from the neighbour's side;
 *   acc starts at +0.0f and takes acc = fmaf(s_c, x[c][d], acc) over the neighbours c of r in ascending CSR order;
 *   y[r][d] = s_r * acc: one multiplication, not fused with an addition;
 *   if sum is not NULL: sum[r][d] = (sum[r][d] + y[r][d]) * sum_scale: one addition, then one multiplication, not fused (the running
 *     layer sum of LightGCN: 1.0f on inner layers, 1 / (L + 1) on the last).
 * A row without neighbours writes +0.0f to y. Every element has one owner, a lane that takes the whole chain: no atomics, no reduction
 * across lanes, so the bits do not depend on the run or on the split of the rows into ranges. Only the rows of [r0, r1) of y and sum
 * are written. Rows are read from other rows, so x must not overlap y or sum (y and sum must not overlap either): refused, like a D
 * outside [1, 512], a range outside [0, n_users + n_items] and a NULL u_indptr, i_indptr, x or y, before any launch. An empty range
 * returns at once. A^ is symmetric: the same call on the incoming gradient is the backward pass. Valid in deterministic mode. New
 * (additive to ABI 4). */
int sbr_graph_propagate_f32(const long* u_indptr, const int* u_indices, const long* i_indptr, const int* i_indices, int n_users,
                            int n_items, long r0, long r1, const float* x, float* y, float* sum, float sum_scale, int D, void* stream);
/* The propagation of SimGCL / XSimGCL (Yu et al., SIGIR 2022 and TKDE 2023): the same y, perturbed by a random direction of length eps
 * in the orthant of y before it is stored and summed. Operands, tables (contiguous, row stride D, no leading dimension, 1 <= D <= 512)
 * and row range as for sbr_graph_propagate_f32. For every row r of [r0, r1) and every d < D:
 *   p[r][d] = y[r][d] of sbr_graph_propagate_f32, bit for bit: the same scales, the same fmaf chain in ascending CSR order, the same
 *     final multiplication;
 *   u[r][d] = Philox4x32-10 as in sbr_uniform_rows_f32 (one block function, csrc/philox.h): key = (low, high) 32-bit halves of `seed`,
 *     counter = (r, d / 4, low half of stream_id, high half of stream_id), word d % 4 of the output block x mapped to (x >> 8) * 2^-24;
 *   n_r = fmaxf(sqrtf(q_r), 1e-12f), with q_r the sum of u[r][d]^2 over d < D in this order, a function of D alone: take the row in
 *     blocks of four columns b = 0 .. ceil(D / 4) - 1 and G4 = the smallest power of two >= ceil(D / 4), 64 at the most. Partial sum
 *     l (0 <= l < G4) starts at +0.0f and takes t = t + u * u (one multiplication, then one addition, not fused) over the columns of
 *     its blocks l, l + G4, ... in ascending column order; columns past D and partial sums without a block contribute +0.0f. The G4
 *     partial sums then combine by an xor butterfly from the widest offset down: for o = G4 / 2, G4 / 4, ..., 1 every t_l becomes
 *     t_l + t_(l xor o) (all of a step at once); t_0 is q_r. One correctly rounded square root;
 *   y[r][d] = p + sgn(p) * ((eps * u) / n_r) where p is not a zero: one multiplication, one correctly rounded division, the sign, one
 *     addition, nothing fused; sgn is torch.sign's, so where p is +-0.0f, y = p: a row without neighbours stays +0.0f and gets no noise;
 *   if sum is not NULL: sum[r][d] = (sum[r][d] + y[r][d]) * sum_scale on the perturbed y, as above.
 * eps == 0 writes exactly p (and the sum of sbr_graph_propagate_f32). The noise is a pure function of (seed, stream_id, r, d): it does
 * not depend on r0, r1, the launch geometry, the alignment of the tables or the run. An element has one owner and the butterfly runs
 * inside the owner's lane group: no atomics, valid in deterministic mode. Refused before any launch: what sbr_graph_propagate_f32
 * refuses, and an eps that is negative or not finite. The derivative of y with respect to x is A^ (the noise is a constant, sgn has
 * derivative zero): the backward pass is sbr_graph_propagate_f32 on the incoming gradient. New (additive to ABI 4). */
int sbr_graph_propagate_noise_f32(const long* u_indptr, const int* u_indices, const long* i_indptr, const int* i_indices, int n_users,
                                  int n_items, long r0, long r1, const float* x, float* y, float* sum, float sum_scale, int D, float eps,
                                  unsigned long seed, unsigned long stream_id, void* stream);

/* ---- NGCF's layer on 0/1 data (csrc/ngcf.hip) ------------------------------------------------------------------------------------------
 * One layer of NGCF (Wang et al., SIGIR 2019) in one launch: the gather of sbr_graph_propagate_f32, the two products, LeakyReLU, message
 * dropout and the row normalisation. Graph operands, their preconditions and the row range as for sbr_graph_propagate_f32. x [n, Din]
 * (n = n_users + n_items) and h [n, Dout] are contiguous fp32 tables (row stride = width); W1 and W2 are [Din, Dout] row-major, bias
 * [Dout]; out is a column slice of a wider table: element (r, j) is out[r * out_ld + j], out_ld >= Dout, and nothing outside the Dout
 * columns of the rows of [r0, r1) is written. 1 <= Din, Dout <= 128. For every row r of [r0, r1):
 *   s[k] = y[r][k] of sbr_graph_propagate_f32 on x, bit for bit: the same scales, the same fmaf chain in ascending CSR order, the same
 *     final multiplication;
 *   a[k] = s[k] + x[r][k]: one addition;  b[k] = s[k] * x[r][k]: one multiplication; nothing fused;
 *   z[j]: acc starts at +0.0f, takes acc = fmaf(a[k], W1[k][j], acc) over k = 0 .. Din - 1 ascending, then acc = fmaf(b[k], W2[k][j], acc)
 *     over k ascending, then z[j] = acc + bias[j]: one addition. The order is a function of (Din, Dout) alone;
 *   h[j] = z[j] > 0 ? z[j] : slope * z[j];
 *   if p > 0: u = Philox4x32-10 keyed as in sbr_graph_propagate_noise_f32 (key = the halves of seed, counter = (r, j / 4, low half of
 *     stream_id, high half of stream_id), word j % 4, mapped to (x >> 8) * 2^-24); where u >= p, h[j] = h[j] * inv_keep with inv_keep =
 *     1.0f / (1.0f - p) computed once on the host in fp32; elsewhere h[j] = +0.0f. With p == 0 no Philox call is made and h passes;
 *   q = the sum of h[j]^2 in this order, the same for every Dout: partial sum l (0 <= l < 16) starts at +0.0f and takes t = t + h[j] *
 *     h[j] (one multiplication, then one addition, not fused) over the columns j with (j / 4) % 16 == l in ascending order; the partial
 *     sums combine by an xor butterfly over the offsets 1, 2, 4, 8: every t_l becomes t_l + t_(l xor o), all of a step at once;
 *   nrm = fmaxf(sqrtf(q), 1e-12f): one correctly rounded square root;  out[j] = h[j] / nrm: one correctly rounded division.
 * h (after the dropout) is the next layer's x. A row whose h is all zeros (every element dropped, or z == 0 throughout) writes +0.0f
 * to h and to out. The mask is a pure function of (seed, stream_id, r, j) and every bit of h and out a function of the row alone: not
 * of r0, r1, the launch geometry, the alignment of the tables or the run. Every element has one owner: no atomics, valid in
 * deterministic mode. Refused before any launch: what sbr_graph_propagate_f32 refuses, a width outside [1, 128], out_ld < Dout, a
 * slope outside (0, 1] or not finite, p outside [0, 1), x, W1, W2 or bias overlapping h or out, h overlapping out, and a NULL
 * u_indptr, i_indptr, x, W1, W2, bias, h or out. An empty range returns at once. Nothing is saved for the backward pass: it takes x and
 * h and recomputes s, the mask and nrm. New (additive to ABI 4). */
int sbr_ngcf_layer_fwd(const long* u_indptr, const int* u_indices, const long* i_indptr, const int* i_indices, int n_users, int n_items,
                       long r0, long r1, const float* x, int Din, const float* W1, const float* W2, const float* bias, int Dout, float slope,
                       float p, unsigned long seed, unsigned long stream_id, float* h, float* out, long out_ld, void* stream);
/* Bytes of workspace sbr_ngcf_layer_bwd needs for a range of n_rows rows (0 for an empty range or widths outside the cap). */
long sbr_ngcf_layer_bwd_workspace(long n_rows, int Din, int Dout);
/* The backward pass of sbr_ngcf_layer_fwd over the rows of [r0, r1), from the same graph, x, W1, W2, slope, p, seed and stream_id and
 * the h the forward pass wrote. g_out is the gradient with respect to out (strided by out_ld like out), g_h the gradient with
 * respect to h that the next layer sends back (NULL: none, the last layer). With nrm and the mask recomputed as above (the same bits),
 * o = h / nrm and f = 1 where sqrtf(q) >= 1e-12f, else 0:
 *   dh[j] = (g_out[j] - f * o[j] * <g_out, o>) / nrm + g_h[j];   dz[j] = dh[j] * (kept ? inv_keep : 0) * (h[j] > 0 ? 1 : slope);
 *   da = dz W1^T, db = dz W2^T;   ds[r][k] = da[k] + db[k] * x[r][k];   dx_direct[r][k] = da[k] + db[k] * s[k]
 * (ds and dx_direct contiguous [n, Din]; only the rows of the range are written). The gradient of x is dx_direct + A^ ds: the caller
 * runs sbr_graph_propagate_f32 on ds with sum = dx_direct and sum_scale = 1 (A^ is symmetric). dW1 = a^T dz, dW2 = b^T dz [Din, Dout]
 * and dbias = colsum(dz) [Dout] over the rows of the range are OVERWRITTEN: a workgroup adds its row tiles into a partial of its own
 * in the workspace, in ascending row order, and the partials are added in workgroup order in double and rounded once. No atomics: the
 * same bits on every run (they depend on the number of rows of the range), valid in deterministic mode. workspace: at least
 * sbr_ngcf_layer_bwd_workspace(r1 - r0, Din, Dout) bytes. Refused before any launch: what the forward entry refuses, any written table
 * (ds, dx_direct, dW1, dW2, dbias, the workspace) overlapping any other operand, a NULL operand other than g_h, a workspace that is
 * too small. An empty range returns at once and writes nothing. New (additive to ABI 4). */
int sbr_ngcf_layer_bwd(const long* u_indptr, const int* u_indices, const long* i_indptr, const int* i_indices, int n_users, int n_items,
                       long r0, long r1, const float* x, int Din, const float* W1, const float* W2, int Dout, float slope, float p,
                       unsigned long seed, unsigned long stream_id, const float* h, const float* g_out, long out_ld, const float* g_h,
                       float* ds, float* dx_direct, float* dW1, float* dW2, float* dbias, void* workspace, long workspace_bytes,
                       void* stream);

/* ---- the multinomial log-likelihood of Mult-VAE / Mult-DAE on 0/1 data (csrc/multinomial.hip) ----------------------------------------
 * The loss of Liang et al. (WWW 2018, equation 2) for a logit matrix [B, n_items] against the users' rows of a users x items binary
 * CSR matrix (indptr int64, indices int32 ascending and unique within a row and below n_items), with its gradient, in one launch.
 * rows[b] is the user of logits row b. logits and dlogits are contiguous fp32 with row stride n_items (no leading dimension; row offsets
 * are (long)b * n_items). For row b with u = rows[b], n = indptr[u + 1] - indptr[u] and z = logits[b]:
 *   m = max_j z_j,  s = sum_j expf(z_j - m),  lse = m + logf(s);   pos = the sum of z_i over the items i of row u;
 *   row_loss[b] = (float)n * lse - pos;   row_lse[b] = lse (row_lse may be NULL);
 *   dlogits[b][j] = grad_scale * ((float)n * expf(z_j - lse) - [j in row u]).
 * A row with n == 0 writes +0.0f to row_loss[b] and to every element of its gradient row (its row_lse is still lse). The mean over the
 * batch and its 1 / B (grad_scale) are the caller's. dlogits == NULL: forward only; dlogits == logits: in place, the logit matrix
 * becomes its own gradient; otherwise a disjoint [B, n_items] matrix, and logits is not written.
 * Order of the operations. The row is cut into chunks of four consecutive elements; chunk c belongs to thread c % T of the T threads
 * that own the row (T = 64, a wave, for n_items <= 1024; T = 256, a workgroup, above; up to n_items = 12,288 the workgroup keeps the
 * row in LDS between its two passes, above it reads the row again), whether the chunk is loaded as one float4 (n_items % 4 == 0 and
 * 16-byte aligned bases) or as four floats. A thread keeps a pair (m_t, s_t), from (-inf, 0): for each of its chunks in ascending
 * order, m' = max(m_t, the four), s_t = s_t * e(m_t, m') and then + expf(z - m') for the four in ascending order (e(a, b) = expf(a - b),
 * and exactly 1 where a == b). Pairs merge as (max, s_a * e(m_a, max) + s_b * e(m_b, max)), not fused: by an xor butterfly over the
 * lanes of a wave (offsets 1, 2, .. 32), then over the waves in ascending order. pos: thread t adds the row's entries t, t + T, ... in
 * that order from +0, and the partial sums are added by the same butterfly and wave order. The dense part of the gradient is
 * grad_scale * ((float)n * expf(z_j - lse)); grad_scale is then subtracted once at each item of the row (a plain read-modify-write by
 * one owner per element, behind the owner's dense write of the row). None of this depends on B, b, the run or the other rows; no float
 * atomics; the entry never counts as a nondeterministic launch and is valid in deterministic mode.
 * Refused before any launch: a NULL indptr, rows, logits or row_loss; n_items < 1; B < 0; dlogits overlapping logits in part; row_loss
 * or row_lse overlapping a matrix or each other. B == 0 returns at once. A row id outside the matrix cannot be checked without a
 * synchronisation: rows[b] in [0, users) is the caller's contract (ops.multinomial_nll checks it). Finite logits are the defined
 * domain; for any logit values, and for indices outside [0, n_items) (which are skipped), nothing outside the operands is read or
 * written. New (additive to ABI 4). */
int sbr_multinomial_nll_f32(const long* indptr, const int* indices, const long* rows, long B, int n_items, const float* logits,
                            float* dlogits, float grad_scale, float* row_loss, float* row_lse, void* stream);

/* ---- RecVAE's row-wise tails: swish + LayerNorm, and the composite-prior KL (csrc/recvae.hip) --------------------------------------------
 * Every operand is a contiguous fp32 matrix with row stride equal to its width (row offsets are (long)b * width), or a vector; operands
 * must not overlap. One wave owns a row: element j belongs to lane j % 64, a lane walks its elements in ascending order, and a sum over
 * a row is the lanes' partial sums (from +0) added by an xor butterfly with the offsets 32, 16, .. 1. No product and sum is fused. The
 * bits of a row's results depend on the row and the width alone: not on B, b, the run or the other rows. No atomics; none of these
 * entries ever counts as a nondeterministic launch; all are valid in deterministic mode. New (additive to ABI 4).
 *
 * sbr_swish_ln_fwd: a [B, H], r_in [B, H] or NULL (read as zero, nothing added), gamma, beta [H], eps > 0 finite, 1 <= H <= 1024.
 *   s = a + r_in;  y = s * (1 / (1 + expf(-s)));  mean = sum_j(y) / H;  d = y - mean;  rstd = 1 / sqrtf(sum_j(d * d) / H + eps);
 *   h = ((d * rstd) * gamma) + beta;  r_out = r_in + h (h itself where r_in is NULL; r_out may be NULL: nothing is written).
 *   Written: s, h [B, H], mean, rstd [B], r_out. The mean is taken first and the squares are those of the centred values.
 *   Refused before any launch: H outside [1, 1024], B < 0, eps not positive and finite, a NULL a, gamma, beta, s, h, mean or rstd.
 *   B == 0 returns at once.
 * sbr_swish_ln_bwd: s, mean, rstd as the forward pass wrote them, gamma [H], dh and dr_out [B, H] (either may be NULL, not both).
 *   g = dh + dr_out (the one given where the other is NULL);  sig, y as above;  xhat = (y - mean) * rstd;  gg = g * gamma;
 *   c1 = sum_j(gg) / H;  c2 = sum_j(gg * xhat) / H;  ds = (rstd * ((gg - c1) - xhat * c2)) * (sig + y * (1 - sig));
 *   da = ds;  dr_in = ds + dr_out (ds where dr_out is NULL; dr_in may be NULL);  dgamma = sum_b g * xhat;  dbeta = sum_b g.
 *   The column sums: workgroup w is slab w and owns the rows [4 rps w, 4 rps (w + 1)), rps = max(1, ceil(B / 4096)); wave q adds its
 *   rows first + q, first + q + 4, .. in that order from +0, the four waves are added in ascending order, and the slab's two rows of H
 *   sums go to partials [sbr_swish_ln_slabs(B)][2][H] (written before it is read: no zeroing). A second launch adds the slabs in
 *   ascending order in double and rounds once. dgamma, dbeta and partials are given together or all NULL (no column sums).
 *   Refused before any launch: H outside [1, 1024], B < 0, a NULL s, mean, rstd, gamma or da, dh and dr_out both NULL, dgamma, dbeta
 *   and partials not given together. B == 0 returns at once (dgamma and dbeta are then not written).
 * sbr_swish_ln_slabs: the number of slabs for B rows (0 for B <= 0, at most 1,024): a count, not a status. */
int sbr_swish_ln_fwd(const float* a, const float* r_in, const float* gamma, const float* beta, float eps, long B, int H, float* s, float* h,
                     float* r_out, float* mean, float* rstd, void* stream);
int sbr_swish_ln_bwd(const float* s, const float* mean, const float* rstd, const float* gamma, const float* dh, const float* dr_out, long B,
                     int H, float* da, float* dr_in, float* dgamma, float* dbeta, float* partials, void* stream);
int sbr_swish_ln_slabs(long B);
/* sbr_prior_kl_fwd: mu, logvar, eps, mu_old, logvar_old [B, L], weight [B], 1 <= L <= 1024. Per element, with LOG2PI = log(2 pi):
 *   z = mu + eps * E(0.5 * logvar), E the correctly rounded fp32 exponential (the double one, rounded once);
 *   lq = -0.5 * (logvar + LOG2PI + eps * eps)             (log N(z; mu, logvar): (z - mu)^2 / exp(logvar) is eps^2)
 *   l0 = log(3/20) - 0.5 * (LOG2PI + z * z);   l1 = log(3/4) - 0.5 * (logvar_old + LOG2PI + (z - mu_old)^2 / expf(logvar_old));
 *   l2 = log(1/10) - 0.5 * (10 + LOG2PI + z * z / exp(10));   mx = max(l0, l1, l2);   se = expf(l0 - mx) + expf(l1 - mx) + expf(l2 - mx);
 *   lp = mx + logf(se);   row_kl[b] = weight[b] * sum_j (lq - lp).
 *   The largest of the three exponents is exactly 0, so se lies in [1, 3] whatever z and logvar_old are (finite l's).
 *   Written: z [B, L], row_kl [B]. The mean over the batch is the caller's.
 *   Refused before any launch: L outside [1, 1024], B < 0, a NULL operand. B == 0 returns at once.
 * sbr_prior_kl_bwd: logvar, eps, mu_old, logvar_old, weight as above, z as the forward pass wrote it, dz [B, L] or NULL (the gradient that
 *   reaches z from elsewhere), upstream: one fp32 on the device or NULL (read as 1), scale (the caller's 1 / B). c = upstream * scale *
 *   weight[b];  e_c = expf(l_c - mx);  dlp = -((e_0 * z + e_1 * ((z - mu_old) / expf(logvar_old)) + e_2 * (z / exp(10))) / se);
 *   t = dz - c * dlp;   dmu = t;   dlogvar = t * (0.5 * (eps * E(0.5 * logvar))) - 0.5 * c.   (lq gives mu nothing and logvar -c / 2.)
 *   No gradient goes to mu_old, logvar_old or weight. Refused before any launch: L outside [1, 1024], B < 0, a NULL logvar, eps, mu_old,
 *   logvar_old, weight, z, dmu or dlogvar. B == 0 returns at once. */
int sbr_prior_kl_fwd(const float* mu, const float* logvar, const float* eps, const float* mu_old, const float* logvar_old, const float* weight,
                     long B, int L, float* z, float* row_kl, void* stream);
int sbr_prior_kl_bwd(const float* logvar, const float* eps, const float* mu_old, const float* logvar_old, const float* weight, const float* z,
                     const float* dz, const float* upstream, float scale, long B, int L, float* dmu, float* dlogvar, void* stream);

/* ---- DirectAU's loss terms: uniformity and alignment (csrc/directau.hip) --------------------------------------------------------------
 * Uniformity (Wang and Isola, ICML 2020; Wang et al., KDD 2022) of the rows of a contiguous fp32 x [n, D] with row stride D (no leading
 * dimension), 2 <= n, 1 <= D <= 256, t > 0. The rows need not be normalised. With
 *   sq_i = |x_i|^2,  g_ij = x_i . x_j,  d_ij^2 = max(0, (sq_i + sq_j) - 2 g_ij),  w_ij = expf(-(t * d_ij^2)):
 *   S = sum_{i<j} w_ij (fp32),   loss = log(S * 2 / (n (n - 1))) (fp32).
 * A pair (i, i) is never counted; two equal rows are an ordinary pair (its w is the exponential of the rounding error of d^2, at most 1).
 * Order of the operations. Rows are cut into tiles of 64; a workgroup of 256 threads owns a row tile and takes the column tiles from its
 * own upwards in ascending order. sq_i: 32 fmaf chains from +0, chain s over d = s, s + 32, .., added by an xor butterfly with offsets
 * 16, 8, 4, 2, 1: the same bits wherever the row is used. g_ij: one fmaf chain from +0 over d = 0 .. D - 1. A thread holds the 4 x 4
 * pairs (rows 4 rg .. + 3 of the row tile, columns 4 cg .. + 3 of the column tile, thread = 16 rg + cg), excluded pairs as +0, adds
 * them as ((w0 + w1) + (w2 + w3)) per row and ((r0 + r1) + (r2 + r3)) over its rows in fp32, and adds that to a double that it keeps
 * over the column tiles. The 256 doubles of a row tile are added by an xor butterfly (offsets 32 .. 1) within a wave and as
 * ((w0 + w1) + (w2 + w3)) over the waves: the row tile's partial, ws[tile]. A second launch adds the partials in tile order in double
 * and rounds once: S. loss is computed from that fp32 S in double and rounded once. ws: sbr_uniformity_workspace(n, D) bytes (one
 * double per row tile), written before it is read: it needs no zeroing; calls that share it must not overlap in time.
 * max_wg: the most workgroups to launch, 0 for the default (one per row tile up to 1,024); further row tiles are taken by a
 * grid-stride loop. The bits of S and loss depend on (x, n, D, t) alone: not on the run, max_wg, or which workgroup took which tile.
 * Defined domain: t * max d^2 < 80 (no term underflows; unit rows with t <= 16 are inside it).
 * Refused before any launch: n < 2, D outside [1, 256], t <= 0 or not finite, a negative max_wg, a NULL x, S, loss or ws, ws_bytes below
 * sbr_uniformity_workspace(n, D). No float atomics; never counts as a nondeterministic launch; valid in deterministic mode. New
 * (additive to ABI 4). */
long sbr_uniformity_workspace(long n, int D);
int sbr_uniformity_fwd(const float* x, long n, int D, float t, float* S, float* loss, void* ws, long ws_bytes, int max_wg, void* stream);
/* The gradient of that loss, from x, the forward pass's S and the upstream gradient grad, both read from device memory (fp32 scalars: no
 * host read-back), with w recomputed as above:
 *   coef = grad * (-2 * t / S);   dx[i][d] = coef * (x[i][d] * rs_i - acc_i[d]),   rs_i = sum_{j != i} w_ij,  acc_i = sum_{j != i} w_ij x_j.
 * Order. The workgroup that owns a row tile takes EVERY column tile in ascending order. rs_i: per column tile the thread's four weights
 * of the row as (w0 + w1) + (w2 + w3), the row's 16 threads by an xor butterfly (offsets 1, 2, 4, 8), then added to the running fp32 sum.
 * acc_i[d]: one fmaf chain from +0 over j = 0 .. n - 1 (w_ii enters as +0), in registers for the whole pass (a thread holds 4 x 4 per 64
 * columns of D: hence D <= 256). The last line is two multiplications and a subtraction, not fused. Every dx element has one owner; the
 * bits depend on (x, n, D, t, S, grad) alone. dx is contiguous [n, D] and must not overlap x. Refused before any launch: what
 * sbr_uniformity_fwd refuses of n, D, t and max_wg, a NULL x, S, grad or dx, dx overlapping x. No workspace. Valid in deterministic
 * mode. New (additive to ABI 4). */
int sbr_uniformity_bwd(const float* x, long n, int D, float t, const float* S, const float* grad, float* dx, int max_wg, void* stream);
/* Alignment as a row loss on logits [B, N] (contiguous fp32) and labels (float64 0 / 1), with the conventions of sbr_rec_loss_fwd / _bwd:
 *   loss_out = scale * sum over the elements with label == 1 of (2 - 2 z)   (float64);   dlogits = -2 * scale * g there, +0 elsewhere.
 * On cosine logits with one positive per row and scale = 1 / B this is mean_b |u^_b - i^_b|^2. Negative columns are ignored. Order: one
 * thread per row adds its positives in column order in double; a block of 256 rows adds its threads by an xor butterfly (offsets 32 .. 1)
 * and its waves in order, times scale; the block partials (library scratch) are added in a fixed pattern by one workgroup. No double
 * atomics in either mode; never counts as a nondeterministic launch. g: the upstream gradient in device memory, float64 when
 * grad_out_is_double, else fp32; the gradient is rounded to fp32 once. Refused: a NULL operand, B < 0, N < 1. B == 0: loss_out = 0,
 * nothing else is written. New (additive to ABI 4). */
int sbr_align_fwd(const float* logits, const double* labels, long B, int N, double scale, double* loss_out, void* stream);
int sbr_align_bwd(const double* labels, long B, int N, double scale, const void* grad_out, int grad_out_is_double, float* dlogits,
                  void* stream);

/* ---- implicit-feedback ALS (csrc/als.hip) ------------------------------------------------------------------------------------------
 * One half-sweep of algorithms/mf_algs.py:69-142 (Hu, Koren and Volinsky 2008) recomputes every row of one factor matrix X from the
 * other one, Y [n_y, f] fp32 with leading dimension ldy, 1 <= f <= 128. The confidence of an observed entry is c = alpha * r, of every
 * other entry 1; the preference is 1 for observed entries and 0 elsewhere. For row r with observed columns S:
 *   A_r = (Y^T Y + reg I) + sum_{i in S} (alpha r_i - 1) y_i y_i^T,   b_r = sum_{i in S} alpha r_i y_i,   x_r = A_r^-1 b_r.
 *
 * G = Y^T Y + reg I as fp32 [f, f] with leading dimension ldg. Rows of Y are taken in slabs of 512: within a slab G[i][j] starts at
 * +0 and receives fmaf(Y[k][i], Y[k][j], .) in ascending k; the slabs' partial sums are then added in ascending slab order from +0 by
 * plain fp32 additions and reg is added to the diagonal last (one addition). G is symmetric bit for bit. No float atomics: the same
 * bits on every run, valid in deterministic mode, whatever the deterministic switch says. Only the f x f view of G is written.
 * workspace: sbr_als_gram_f32_workspace(n_y, f) bytes (the slabs' partial sums). reg must be positive and finite. n_y = 0 gives
 * reg I. New (additive to ABI 4). */
int sbr_als_gram_f32(const float* Y, long n_y, long ldy, int f, float reg, float* G, long ldg, void* workspace, long workspace_bytes,
                     void* stream);
/* bytes of `workspace` for sbr_als_gram_f32: ceil(n_y / 512) partial sums [f, f] of fp32. New (additive to ABI 4). */
long sbr_als_gram_f32_workspace(long n_y, int f);
/* X[r, 0:f] = A_r^-1 b_r for the rows r of [r0, r1) of a CSR matrix (indptr int64, indices int32 ascending and unique within a row and
 * below n_y, data fp32 or NULL = all ones). G: the contiguous fp32 [f, f] result of sbr_als_gram_f32 on the same Y. One workgroup owns
 * a row. c_i = alpha * r_i (one fp32 product). An element A_r[i][j], j <= i, starts at G[i][j] and receives
 * fmaf((c_k - 1) * y_k[i], y_k[j], .) over the row's entries k in ascending CSR order; b_r[i] starts at +0 and receives
 * fmaf(c_k, y_k[i], .) in the same order (each element has one owner; the rows of Y are staged through LDS 24 at a time). A_r, with
 * b_r as one more row, is then factored in LDS by an unpivoted Cholesky by columns: for p ascending, q = A[p][p] - sum_{k<p} L[p][k]^2
 * and s_i = A[i][p] - sum_{k<p} L[i][k] L[p][k] as fmaf chains in ascending k, L[p][p] = sqrtf(q), L[i][p] = s_i / L[p][p] (the row of
 * b_r gives z = L^-1 b_r on the way); L^T x = z follows by columns, p descending: x[p] = z[p] / L[p][p], z[i] = fmaf(-L[p][i], x[p],
 * z[i]) for i < p. An empty row writes +0.0f in every one of its f elements. Only X[r0:r1, 0:f] is written (leading dimension ldx).
 * info: one device int32, zero on entry; a row that meets a pivot q that is <= 0 or not finite sets it to 1 + r unless it already holds
 * a smaller non-zero value, so that it names the first such row (an error return, not a fault: the kernel finishes; that row's output
 * is unspecified). The bits of a row do not depend on [r0, r1) or on the run; valid in deterministic mode (integer atomics on info
 * only). alpha must be positive and finite, ldx >= f, ldy >= f, 0 <= r0 <= r1 <= 2^31 - 2; an empty range returns at once.
 * New (additive to ABI 4). */
int sbr_als_solve_rows_f32(const long* indptr, const int* indices, const float* data, long r0, long r1, const float* Y, long n_y, long ldy,
                           int f, const float* G, float alpha, float* X, long ldx, int* info, void* stream);

/* ---- truncated SVD by block subspace iteration (csrc/svd.hip) ----------------------------------------------------------------------
 * algorithms/mf_algs.py:14-66 calls ARPACK (scipy's svds); here a block V [n_items, b], b <= 128, is iterated: Y = X V, U = orth(Y),
 * Z = X^T U, (V, s, W) = orth(Z), U <- U W, where orth(Y) = Y W diag(1 / s) with Y^T Y = W diag(lam) W^T, lam descending, and
 * s = sqrt(max(lam, tiny)). Every entry below has one owner per output element and a stated order: the same bits on every run, valid in
 * deterministic mode, whatever the deterministic switch says.
 *
 * G = Y^T Y as fp32 [f, f]: sbr_als_gram_f32's two launches (slabs of 512 rows, fmaf in ascending row order from +0, the slabs' partial
 * sums added in ascending slab order) with nothing added to the diagonal; G is symmetric bit for bit; the workspace is
 * sbr_als_gram_f32_workspace(n_y, f) bytes. New (additive to ABI 4). */
int sbr_gram_f32(const float* Y, long n_y, long ldy, int f, float* G, long ldg, void* workspace, long workspace_bytes, void* stream);
/* A = W diag(lam) W^T for a symmetric fp32 A [n, n], 1 <= n <= 128 (leading dimension lda; the lower triangle of the n x n view is read
 * and mirrored, nothing else): W fp32 [n, n] with leading dimension ldw holds the eigenvectors as columns, lam [n] the eigenvalues in
 * descending order. Parallel cyclic Jacobi by one workgroup. The elements are converted to double, the whole iteration is in double
 * and the results are rounded to fp32 once, at the end: an fp32 iteration leaves errors of 1e-6 at n = 128 (about a thousand rotations
 * per column), forty times the rounding of the results. The matrix is in LDS (8 N (N + 1) bytes), the accumulated rotations in
 * `workspace`, transposed: both in double do not fit 160 KiB.
 *   pair ordering: with N = n rounded up to even (an odd n adds one index that is a bye: the pair that holds it is left alone), a sweep
 *     is the N - 1 steps r = 0 .. N - 2 of the round robin in which index N - 1 stays and the others move round: step r rotates the
 *     N / 2 disjoint pairs {r, N - 1} and {(r + k) mod (N - 1), (r - k) mod (N - 1)}, k = 1 .. N / 2 - 1, each as (p, q) with p < q, all at
 *     once (A <- J^T A J, W <- W J with J the product of the step's rotations);
 *   rotation: a pair is left alone when |a_pq| <= 2^-40 * (sqrt(|a_pp|) * sqrt(|a_qq|)), the relative test that keeps a graded matrix
 *     accurate; otherwise tau = (a_qq - a_pp) / (2 a_pq), t = sign(tau) / (|tau| + sqrt(1 + tau^2)) (sign(0) = +1),
 *     c = 1 / sqrt(1 + t^2), s = t c; column p becomes c x_p - s x_q, column q becomes s x_p + c x_q, rows p and q likewise;
 *     a_pp <- a_pp - t a_pq, a_qq <- a_qq + t a_pq, a_pq <- 0 exactly. Each 2 x 2 block of A (the rows of one pair, the columns of
 *     another: rows first, then columns) has one owner, which also writes its mirror image: A stays symmetric bit for bit;
 *   the iteration stops after a sweep without a rotation; the sweep cap is 30 (EIG_MAX_SWEEPS in csrc/svd.hip);
 *   order: lam descending, equal values by ascending index of their position on the diagonal, the eigenvectors permuted along;
 *   length and sign: every eigenvector is divided by its length (the sum of squares in ascending index) and multiplied by -1 if the
 *     component of largest magnitude of the rounded result (the lowest index on a tie) is negative.
 * info: one device int32, zero on entry: it is left alone on success and set to 31 (the sweeps run plus one) when the cap was reached
 * with rotations still happening (an error return, not a fault: the kernel always finishes and writes W and lam as they then are).
 * workspace: sbr_sym_eig_f32_workspace(n) bytes at an 8-byte boundary. No atomics: the same bits on every run. n outside [1, 128] is
 * refused before any launch. New (additive to ABI 4). */
int sbr_sym_eig_f32(const float* A, int n, long lda, float* W, long ldw, float* lam, int* info, void* workspace, long workspace_bytes,
                    void* stream);
/* bytes of `workspace` for sbr_sym_eig_f32: N x N doubles, N = n rounded up to even (0 for an n outside [1, 128]). New (additive to
 * ABI 4). */
long sbr_sym_eig_f32_workspace(int n);
/* out[r, 0:c] = sum_k data_k D[col_k, 0:c] over the entries k of row r in ascending CSR order, for the rows r of [r0, r1) of a CSR
 * matrix (indptr int64, indices int32 ascending and unique within a row and below n_d, data fp32 or NULL = all ones); D fp32 [n_d, c]
 * with leading dimension ldd, out with leading dimension ldo, 1 <= c <= 128. Every element has one owner: it starts at +0.0f and
 * receives fmaf(data_k, D[col_k][j], .) in that order, so an empty row writes +0.0f, and the bits of a row do not depend on [r0, r1).
 * Only out[r0:r1, 0:c] is written. No atomics. 0 <= r0 <= r1 <= 2^31 - 2; an empty range returns at once. (sbr_csr_project_fwd is
 * the training path's product: int32 row lists, a bias, an activation.) New (additive to ABI 4). */
int sbr_csr_times_dense_f32(const long* indptr, const int* indices, const float* data, long r0, long r1, const float* D, long n_d,
                            long ldd, int c, float* out, long ldo, void* stream);
/* out = Y W diag(1 / s) for Y fp32 [n, b], W fp32 [b, b], 1 <= b <= 128 (leading dimensions ldy, ldw, ldo; out may be Y itself: a
 * workgroup reads its 32 rows before it writes them). out[r][j] starts at +0.0f, receives fmaf(Y[r][k], W[k][j], .) in ascending k and
 * is multiplied once by 1.0f / s[j], with s[j] = sqrtf(max(lam[j], tiny)), tiny = max(lam[0] * 2^-46, FLT_MIN): a direction whose
 * eigenvalue drowned in the rounding of lam[0] is scaled by about 1 / (2^-23 sqrt(lam[0])) at the most instead of by 1 / 0. s [b] is
 * written too, also when n = 0 (Y and out may then be NULL). lam NULL: the plain product Y W, s is not touched. An fp32 fmaf chain of
 * its own, not the `ops` GEMM: that one picks its kernel by shape (the bf16-split kernels from 4,096 rows at N = K = 128), which would
 * tie the bits to n. New (additive to
 * ABI 4). */
int sbr_rotate_cols_f32(const float* Y, long n, long ldy, int b, const float* W, long ldw, const float* lam, float* s, float* out, long ldo,
                        void* stream);
/* res[j] = ||Y[:, j] - s[j] U[:, j]||_2 for j < f <= 128 over n rows: d = fmaf(-s[j], U[r][j], Y[r][j]), its square added by fmaf in
 * ascending row order within slabs of 256 rows from +0, the slabs' sums added in ascending slab order, one sqrtf. workspace:
 * sbr_col_residual_f32_workspace(n, f) bytes. New (additive to ABI 4). */
int sbr_col_residual_f32(const float* Y, long ldy, const float* U, long ldu, const float* s, long n, int f, float* res, void* workspace,
                         long workspace_bytes, void* stream);
/* bytes of `workspace` for sbr_col_residual_f32: ceil(n / 256) partial sums [f] of fp32. New (additive to ABI 4). */
long sbr_col_residual_f32_workspace(long n, int f);

/* ---- RBMF: representative rows by maxvol, and the ridge solve (csrc/rbmf.hip) --------------------------------------------------------
 * algorithms/mf_algs.py:168-186 picks `indxs, _ = maxvolpy.maxvol.maxvol(u)` from the left singular vectors u [n, r] and solves
 * X = matrix C^T inv(C C^T + lam I) with C = matrix[indxs]. maxvol (Goreinov, Oseledets, Savostyanov, Tyrtyshnikov, Zamarashkin 2010):
 * start from the pivot rows of a row-pivoted LU of u, form B = u inv(u[idx]), and while the largest |B_ij| exceeds tol put row i in
 * place of basis row j. Both loops are chains of launches: a launch leaves one candidate per slab of `slab_rows` rows (0: 256; at most
 * 1,024) for the arg-max of the next, whose workgroups all reduce every candidate again and so agree; no cooperative launch, and no
 * workgroup waits for another. Every arg-max takes the largest magnitude, then the lowest row, then the lowest column; a NaN never
 * wins. fp32, no float atomics, one owner and one stated order per element: the same bits on every run and for every slab_rows, valid
 * in deterministic mode, whatever the deterministic switch says.
 *
 * bytes of `workspace` of both chains: 4 (6 ceil(n / slab) + n + 4) — two generations of per-slab candidates, a state word per row
 * and the largest pivot so far; 0 for an n outside [1, 2^31 - 2] or a slab_rows outside [0, 1024]. The LU chain owns it from its
 * step 0 to its last step, a swap chain from its step 0 on. New (additive to ABI 4). */
long sbr_maxvol_f32_workspace(long n, int slab_rows);
/* Step k of the row-pivoted LU of A fp32 [n, r] (leading dimension lda), in place, 1 <= r <= 128, n >= r (mf_algs.py:168-186: the
 * start of maxvol). Call it for k = 0 .. r - 1 on one stream with the same arguments; nothing is read back in between. k = 0 first
 * marks every row as not chosen and leaves the candidates of column 0. Step k: the pivot is the row not yet chosen with the largest
 * |a_ik|; idx[k] <- that row; every other row i not yet chosen stores l = a_ik / p_kk in place of a_ik and takes
 * a_ij <- fmaf(-l, p_kj, a_ij) for j > k (p: the pivot row, which is final by then). A pivot whose magnitude is zero or not above
 * r * 2^-24 * (the largest pivot magnitude of the steps before) sets *info to k + 1 unless it is set already (zero on entry; an error
 * return, not a fault: the chain runs on): the block has numerical rank below r. The step k = r - 1 also unpacks: A becomes the unit
 * lower factor L over all rows (a pivot row's diagonal element 1, zeros behind it), Ltop [r, r] (ldl) its pivot rows in pivot order,
 * and Utop [r, r] (ldu; may be NULL) the upper factor, so that A_in[idx] = Ltop Utop. Only the n x r view of A is written.
 * New (additive to ABI 4). */
int sbr_maxvol_lu_step_f32(float* A, long n, long lda, int r, int k, int* idx, float* Ltop, long ldl, float* Utop, long ldu, int* info,
                           void* workspace, long workspace_bytes, int slab_rows, void* stream);
/* out[i, 0:r] = in[i, 0:r] T^-1 for the n rows of `in` (ldi) with T fp32 [r, r] triangular (ldt), 1 <= r <= 128; upper = 0: the lower
 * triangle of T is read, 1: the upper one; unit = 1: the diagonal is taken as 1 and not read. T is staged once per workgroup in LDS on
 * a padded row stride (r | 1 floats: 66 KiB at r = 128, two workgroups per CU); a wave owns a row. x T = b by columns: lower T, j
 * descending: x_j = b_j / T_jj (one division; none when unit), then b_m <- fmaf(-x_j, T[j][m], b_m) for every m < j; upper T: j
 * ascending and m > j. out may be `in` itself (a wave reads its row before it writes it). It serves mf_algs.py:168-186 three times:
 * B = L Ltop^-1 = u inv(u[idx]) with no r x r inverse ever formed, and X = (M R^-T) R^-1 with C C^T + lam I = R R^T.
 * New (additive to ABI 4). */
int sbr_tri_solve_rows_f32(const float* in, long ldi, long n, int r, const float* T, long ldt, int upper, int unit, float* out, long ldo,
                           void* stream);
/* Iteration s of maxvol's swap loop (mf_algs.py:168-186) on B fp32 [n, r] = u inv(u[idx]) (ldb), in place. Call it for s = 0, 1, ..
 * on one stream; s = 0 first derives the rows' state from idx and leaves the candidates of B as it is. The rows of the basis are not
 * stored: row idx[c] stands for e_c, and what B holds of it is neither read nor written. Iteration s takes the largest |B_ij| over the
 * other rows. If it is <= tol the launch leaves B, idx and *n_swaps alone and only hands the candidates on: a converged chain idles.
 * Otherwise row i replaces idx[j]: w_c = (B_ic - [c = j]) / B_ij (one subtraction, one division), every other row m outside the basis
 * takes B_mc <- fmaf(-B_mj, w_c, B_mc) with the B_mj of before the update, the row that leaves the basis becomes fmaf(-1, w_c, [c = j]),
 * idx[j] <- i and *n_swaps is raised by one (a device int32 the caller zeroes). tol must be finite and >= 1 (the largest |B_ij| is
 * never below 1). One launch makes at most one swap, so the caller bounds the swaps by the launches it enqueues.
 * New (additive to ABI 4). */
int sbr_maxvol_swap_step_f32(float* B, long n, long ldb, int r, float tol, int s, int* idx, int* n_swaps, void* workspace,
                             long workspace_bytes, int slab_rows, void* stream);
/* K = R R^T for a symmetric positive definite fp32 K [n, n], 1 <= n <= 128 (ldk; the lower triangle is read): the ridge system
 * C C^T + lam I of mf_algs.py:168-186. One workgroup factors it in LDS by the unpivoted Cholesky by columns of sbr_als_solve_rows_f32
 * (the same device function, sbr_chol_lds of csrc/block128.h, once csrc/chol_lds.h): q = K[p][p] - sum_{k<p} R[p][k]^2 and s_i = K[i][p] - sum_{k<p} R[i][k] R[p][k] as fmaf
 * chains in ascending k, R[p][p] = sqrtf(q), R[i][p] = s_i / R[p][p]. R [n, n] (ldr) is written whole, zeros above the diagonal.
 * info: one device int32, zero on entry; the first pivot p with q <= 0 or not finite sets it to p + 1 (an error return, not a fault; R
 * is then unspecified). New (additive to ABI 4). */
int sbr_chol_f32(const float* K, int n, long ldk, float* R, long ldr, int* info, void* stream);

/* ---- UltraGCN (csrc/ultragcn.hip) -------------------------------------------------------------------------------------------------
 * Mao et al., CIKM 2021; the reference has no such model. The definitions are the authors' code as remembered.
 *
 * sbr_cooc_weight_topk: X [n, m] binary CSR and X^T in the form of sbr_knn_topk; m <= 2^24. For every row i of [r0, r1) the
 * candidates are the rows j with c = |row i & row j| > 0 (j = i among them when include_self != 0) and
 *   value = (float(c) * row_scale[i]) * col_scale[j]        two rounded fp32 multiplications, nothing contracted, c converted exactly;
 * a value that is not > 0 is no candidate. row_scale, col_scale: fp32 [n]. The list of row i is the first min(k, candidates) by (value
 * descending, index ascending): nbr_idx int32 [n, k], nbr_val fp32 [n, k], nbr_len int32 [n], (-1, 0) behind the length; only the rows
 * of [r0, r1) are written. 1 <= k <= 64. tile_cols as for sbr_knn_topk. The counting and the selection are sbr_knn_topk's device code
 * (csrc/csr_walk.h, csrc/cooc_topk.h). Nothing of size n x n exists. Integer LDS atomics only: the same bits on every run and for
 * every split of the rows, valid in deterministic mode. UltraGCN's item-item lists: X^T as the matrix, row_scale[i] = sqrt(g_i + 1) / g_i,
 * col_scale[j] = 1 / sqrt(g_j + 1), g = the row sums of X^T X. New (additive to ABI 4). */
int sbr_cooc_weight_topk(const long* indptr, const int* indices, const long* t_indptr, const int* t_indices, int n, int m, int r0, int r1,
                         const float* row_scale, const float* col_scale, int include_self, int k, int tile_cols, int* nbr_idx,
                         float* nbr_val, int* nbr_len, void* stream);
/* sbr_ultragcn_loss_fwd_bwd: the loss of a batch, its gradient by the user rows and its gradient by the scores, in one pass.
 * Ub fp32 [B, D]: the users' rows (contiguous). V fp32 [n_items, D]: the item table, contiguous, row j at (long)j * D. u_idxs int32 [B],
 * i_idxs int32 [B, 1 + N]: the positive in column 0, N negatives behind it. beta_u fp32 [n_users], beta_i fp32 [n_items]. nbr_idx /
 * nbr_val / nbr_len: lists [n_items, K] in the form sbr_cooc_weight_topk writes. Batch row b has the slots c = 0 (item p = i_idxs[b, 0]),
 * 1 .. N (the negatives), 1 + N + k (nbr_idx[p, k], k < K). With s = <Ub[b], V[item of the slot]>, sp(x) = max(x, 0) + log1pf(expf(-|x|)),
 * sig(x) = x >= 0 ? 1 / (1 + e) : e / (1 + e), e = expf(-|x|), every product and sum below one rounded fp32 operation in the order written:
 *   slot 0        w = w1 + w2 * (beta_u[u] * beta_i[p])      term w * sp(-s)   coef = -(w * sig(-s))
 *   slot 1 .. N   w = w3 + w4 * (beta_u[u] * beta_i[j])      term w * sp(s)    coef = (fl(negative_weight / N) * w) * sig(s)
 *   neighbour k   w = nbr_val[p, k], k < nbr_len[p]          term w * sp(-s)   coef = -((lam * w) * sig(-s))
 * A neighbour slot at or behind nbr_len[p], and any slot whose item index lies outside [0, n_items), has coef +0, adds nothing and
 * reads no table row (an index of -1 never addresses the table). A user index outside [0, n_users) takes beta_u = 0.
 * The row belongs to a group of G lanes: V = 4 columns per chunk when D % 4 == 0 (Ub, V, dUb must then start on a 16-byte boundary),
 * else 1; G = the smallest power of two with G * V >= D, 64 at the most; lane l owns the chunks l, l + G, ... . s is the lane's fmaf
 * chain over its columns in ascending order from +0, then an xor butterfly over the group from offset G / 2 down to 1. dUb[b, d] is one
 * fmaf chain from +0 of coef * V[item][d] over the slots in ascending c. The terms of a row are added in double in ascending c per part;
 * the negatives' sum is divided by N. The rows' partials (workspace: 24 B bytes, sbr_ultragcn_loss_workspace) are folded in double by a
 * second, one-wave launch: lane l adds the rows l, l + 64, ... in ascending order, then an xor butterfly from offset 32 down to 1.
 * All orders are functions of (D, N, K, B) alone. parts fp32 [4] = (pos, neg, nbr, pos + negative_weight * neg + lam * nbr), each
 * rounded once; dUb fp32 [B, D]; coef fp32 [B, 1 + N + K]; scores fp32 [B, 1 + N] = s of the first 1 + N slots (may be NULL; 0 where the
 * index lies outside the table). 1 <= D <= 256, N >= 1, 1 <= K <= 64, B (1 + N + K) < 2^31. No atomics:
 * valid in deterministic mode. New (additive to ABI 4). */
long sbr_ultragcn_loss_workspace(int B);
int sbr_ultragcn_loss_fwd_bwd(const float* Ub, const float* V, const int* u_idxs, const int* i_idxs, const float* beta_u,
                              const float* beta_i, const int* nbr_idx, const float* nbr_val, const int* nbr_len, int B, int D, int N, int K,
                              int n_users, int n_items, float w1, float w2, float w3, float w4, float negative_weight, float lam,
                              float* parts, float* dUb, float* coef, float* scores, void* workspace, long workspace_bytes, void* stream);
/* sbr_scatter_add_scaled_rows_sorted: dst[j, d] += grad[0] * S_j[d] for every row j of dst fp32 [n_rows, D] (contiguous) that a slot
 * names, S_j[d] = the fmaf chain from +0 of coef[pos] * src[pos / slots_per_row, d] over the slot positions pos whose key is j, in
 * ascending pos. sorted_keys int32 [n_slots]: the slots' keys after a stable ascending sort; order int64 [n_slots]: the position each
 * sorted entry came from (torch.sort(stable=True)). A key outside [0, n_rows), the sentinel of a padded slot, belongs to no row and
 * is skipped on the device; nothing is counted on the host. coef fp32 [n_slots]; src fp32 [n_slots / slots_per_row, D]; grad: one fp32
 * on the device. One wave per row of dst (its segment by two binary searches), one writer per row, one rounded multiplication by grad
 * and one rounded addition per element; rows that no slot names are not touched. 1 <= D <= 256, n_slots < 2^31. The only form: valid
 * in deterministic mode. UltraGCN's item-table gradient: keys = the slots' item indices, src = Ub. New (additive to ABI 4). */
int sbr_scatter_add_scaled_rows_sorted(const float* coef, const float* src, const int* sorted_keys, const long* order, long n_slots,
                                       int slots_per_row, const float* grad, float* dst, int n_rows, int D, void* stream);

/* ---- SimpleX (csrc/simplex.hip) ---------------------------------------------------------------------------------------------------
 * Mao et al., CIKM 2021; the reference has no such model. The definitions are the authors' code as remembered.
 *
 * sbr_ccl_loss_fwd_bwd: the cosine contrastive loss of a batch, its gradient by the user representations and the two coefficient
 * arrays that carry the item table's gradient, in one pass. H fp32 [B, D]: the user representations (contiguous). V fp32 [n_items, D]:
 * the item table, contiguous, row j at (long)j * D, read in place. i_idxs int32 [B, 1 + N]: the positive in column 0, N negatives
 * behind it. The row belongs to a group of G lanes, the geometry of sbr_ultragcn_loss_fwd_bwd: 4 columns per chunk when D % 4 == 0 (H, V,
 * dH must then start on a 16-byte boundary), else 1; G = the smallest power of two with G * (4 or 1) >= D, 64 at the most; lane l owns
 * the chunks l, l + G, ... . Every dot product is the lane's fmaf chain over its columns in ascending order from +0, then an xor
 * butterfly over the group from offset G / 2 down to 1. Every operation below is one rounded fp32 operation in the order written
 * (sqrtf and the divisions correctly rounded, nothing contracted):
 *   hh = <H[b], H[b]>   rh = sqrtf(hh)   nh = max(rh, eps)
 *   per slot c, item j = i_idxs[b, c], H[b] in registers and V[j] read once:
 *     s = <H[b], V[j]>   vv = <V[j], V[j]>   rv = sqrtf(vv)   nv = max(rv, eps)   den = nh * nv   y = s / den
 *     c = 0    term = 1 - y                 g = -fl(1 / B)
 *     c >= 1   term = max(y - margin, 0)    g = y > margin ? fl(fl(negative_weight / N) * fl(1 / B)) : +0      (strictly above)
 *     g == 0:  coef_a = coef_s = +0
 *     else     coef_a = g / den   gy = g * y   sgy = sgy + gy (from +0, ascending c)   coef_s = rv < eps ? +0 : -(gy / (nv * nv))
 *   dH[b, d] = fmaf(-k, H[b, d], A[d])   A[d] = one fmaf chain from +0 of coef_a * V[j][d] over the slots in ascending c
 *                                        k = rh < eps ? +0 : sgy / (nh * nh)             (the clamp has no gradient)
 * A slot whose index lies outside [0, n_items) reads no table row (an index of -1 never addresses the table), has y = 0, both
 * coefficients +0 and adds no term. The terms of a row are added in double in ascending c, the positive's and the negatives' apart;
 * the negatives' sum is divided by N. The rows' partials (workspace: 16 B bytes, sbr_ccl_loss_workspace) are folded in double by a
 * second, one-wave launch: lane l adds the rows l, l + 64, ... in ascending order, then an xor butterfly from offset 32 down to 1.
 * All orders are functions of (B, D, N) alone. parts fp32 [3] = (pos / B, neg / B, (pos + negative_weight * neg) / B), each rounded
 * once; dH fp32 [B, D]; coef_a, coef_s fp32 [B, 1 + N]: dL/dV[j] = sum over the slots that name j of coef_a * H[b] + coef_s * V[j];
 * scores fp32 [B, 1 + N] = y (may be NULL). 1 <= D <= 256, N >= 1, B (1 + N) < 2^31, eps > 0. No atomics: valid in deterministic
 * mode. New (additive to ABI 4). */
long sbr_ccl_loss_workspace(int B);
int sbr_ccl_loss_fwd_bwd(const float* H, const float* V, const int* i_idxs, int B, int D, int N, int n_items, float margin,
                         float negative_weight, float eps, float* parts, float* dH, float* coef_a, float* coef_s, float* scores,
                         void* workspace, long workspace_bytes, void* stream);
/* sbr_scatter_add_cos_rows_sorted: dst[j, d] += grad[0] * (S_j[d] + T_j * V[j, d]) for every row j of dst fp32 [n_rows, D] (contiguous)
 * that a slot names. S_j[d] = the fmaf chain from +0 of coef_a[pos] * src[pos / slots_per_row, d] over the slot positions pos whose key
 * is j, in ascending pos; T_j = the sum from +0 of coef_s[pos] over the same positions in the same order (T = T + coef_s[pos]); then
 * r = fmaf(T_j, V[j, d], S_j[d]), t = grad[0] * r, dst[j, d] = dst[j, d] + t, one rounding each. sorted_keys, order, the sentinel key
 * of a padded slot, grad, the wave per row and the one writer per row are those of sbr_scatter_add_scaled_rows_sorted, whose segment
 * search and row walk this entry shares (csrc/slot_rows.h). coef_a, coef_s fp32 [n_slots]; src fp32 [n_slots / slots_per_row, D];
 * V fp32 [n_rows, D] contiguous; rows that no slot names are not touched. 1 <= D <= 256, n_slots < 2^31. The only form: valid in
 * deterministic mode. SimpleX's item-table gradient: keys = the slots' item indices, src = H. New (additive to ABI 4). */
int sbr_scatter_add_cos_rows_sorted(const float* coef_a, const float* coef_s, const float* src, const float* V, const int* sorted_keys,
                                    const long* order, long n_slots, int slots_per_row, const float* grad, float* dst, int n_rows, int D,
                                    void* stream);

/* ---- NeuMF (csrc/neumf.hip) --------------------------------------------------------------------------------------------------------
 * He et al., "Neural Collaborative Filtering", WWW 2017; the reference has no such model. The definitions are the paper as remembered
 * (DESIGN.md §4.36).
 *
 * sbr_neumf_score_all: the MLP term of every (user, item) pair without the [Bu, I, H1] activation. The first layer is separable, so it
 * arrives split by side: A fp32 [Bu, H1] = W1u pm_u + b1 (row u at (long)u * stride_a), Bt fp32 [I, H1] = W1i qm_i (row i at
 * (long)i * stride_b). tail fp32 [tail_len]: the packed rest of the network for the widths (h1 .. h_L), L = n_layers, unused widths
 * ignored: W_2 .. W_L row-major [H_l, H_{l-1}], then b_2 .. b_L, then w_h [H_L], then c; tail_len must be exactly that many floats.
 * Per pair, every operation one rounded fp32 operation in the order written, nothing contracted:
 *   z_1[k] = relu(A[u, k] + Bt[i, k])
 *   z_l[j] = relu(t),  t = b_l[j];  t = fmaf(W_l[j, k], z_{l-1}[k], t) for k = 0, 1, ... ascending               l = 2 .. L
 *   m      = t,        t = +0;      t = fmaf(w_h[k], z_L[k], t)        for k = 0, 1, ... ascending
 *   s      = m + c
 *   out[u, i] = accumulate ? out[u, i] + s : s                    out fp32 [Bu, I], row u at (long)u * stride_o
 * relu(x) = x < 0 ? 0 : x (a NaN stays a NaN). Each chain runs on to the next multiple of 4 over +0 weights and +0 inputs, which
 * changes no value (only a -0 sum to +0). The order depends on the widths alone, never on the pair's place in a tile, on Bu, on I or on
 * the launch: a pair has the same bits however the users are chunked and the items sharded, and through sbr_neumf_score_pairs, which
 * runs the same device function. A lane owns one item of a 64-item tile and keeps its Bt row in registers; a workgroup of four waves
 * walks a block of 32 users whose A rows and the padded weights sit in LDS (at most 58,384 bytes, under the 64 KiB default limit) and
 * are read as broadcasts. No atomics: valid in deterministic mode. 1 <= n_layers <= 4, 1 <= H_l <= 64; Bu = 0 or I = 0 returns
 * without a launch; ceil(I / 64) * ceil(Bu / 32) <= 2^24 workgroups. With accumulate = 1 the caller has laid the GMF term down in out first (the
 * fp32 GEMM). The three row strides are in elements and at least the row lengths; all offsets are 64-bit.
 * New (additive to ABI 4). */
int sbr_neumf_score_all(const float* A, long stride_a, const float* Bt, long stride_b, const float* tail, long tail_len, int n_layers,
                        int h1, int h2, int h3, int h4, float* out, long stride_o, int Bu, int I, int accumulate, void* stream);
/* sbr_neumf_score_pairs: the same score for R listed pairs: out[r] = accumulate ? out[r] + s : s with s of the pair (A row u_slot[r],
 * Bt row i_slot[r]); u_slot, i_slot int32 [R]; out fp32 [R]. A slot outside [0, Bu) or [0, I) reads no row and gives a NaN. R = 0
 * returns without a launch; at most 2^24 workgroups of 1,024, 512 or 256 pairs (widest layer up to 16, 32, 64). The operands, the order and the limits are those of sbr_neumf_score_all. New (additive to ABI 4). */
int sbr_neumf_score_pairs(const float* A, long stride_a, int Bu, const float* Bt, long stride_b, int I, const int* u_slot,
                          const int* i_slot, const float* tail, long tail_len, int n_layers, int h1, int h2, int h3, int h4, float* out,
                          long R, int accumulate, void* stream);

/* ---- native batch producer (csrc/producer.hip) --------------------------------------------------------------------------------
 * One C++ thread runs the host side of the training step ahead of the launch thread: the default collate of the reference
 * (data/dataloader.py:154-198: bit-exact draws from numpy's legacy MT19937 stream, `v in positives` on the resident interaction
 * CSR), the modality draw of every index slot (algorithms/sgd_alg.py:1904-1927, utilities/utils.py:60-90: PCG64 + numpy's Lemire
 * draws), the per-modality launch plan, and ONE packed host-to-device copy per batch into a ring of caller-allocated device
 * slots: [users | users[0] | items | items[0] | user draw | item draw | dropout seed], 16-byte aligned segments.
 * Generator states are handed in by sbr_producer_start and back by sbr_producer_stop. Exception to the "no ownership" rule:
 * the handle owns its pinned staging buffers, query scratch, stream and events. Batches must be consumed in order, one at a
 * time: sbr_producer_next -> sbr_producer_wait(stream) -> launches that read the slot -> sbr_producer_release(stream).
 * descriptor (32 longs): 0 slot, 1 B, 2 packed bytes, 3..8 segment offsets (users, items, user draw, item draw, seed, end),
 * 9 / 10 rows of the user / item draw, 11..18 user counts per modality (padded to the graph's bucket grid when pad != 0),
 * 19..26 item counts, 27 batch number. */
void* sbr_producer_create(int device, long B, int n_neg, long n_cand, const long* items_in_split, const long* h_indptr,
                          const int* h_indices, const long* d_indptr, const int* d_indices, long host_below, int pad, int n_slots,
                          long slot_bytes, void* const* slot_dev);
int sbr_producer_set_entity(void* handle, int which, int enabled, int n_mod, int k, int central);
int sbr_producer_start(void* handle, const long* rows_e, const long* cols_e, long n_inter, long first, long stride, long n_batches,
                       const unsigned int* mt_key, int mt_pos, const unsigned long long* pcg, long seed_base, long n_prepared);
int sbr_producer_next(void* handle, long* desc);
int sbr_producer_wait(void* handle, int slot, void* stream);
int sbr_producer_release(void* handle, int slot, void* stream);
int sbr_producer_stop(void* handle, unsigned int* mt_key, int* mt_pos, unsigned long long* pcg, long* out_counters);
int sbr_producer_destroy(void* handle);
/* the producer's generator replica and plan padding on their own (host only; pinned against numpy / the Python formulation by
 * tests/test_host_cpu.py). pcg: (state hi, state lo, inc hi, inc lo, has_uint32, uinteger) of numpy's PCG64, updated in place. */
int sbr_host_pcg64_modalities(unsigned long long* pcg, long n_slots, int n_mod, int k, int central, signed char* out, long* counts);
int sbr_host_pad_counts(long* counts, int n_mod, long R);

#ifdef __cplusplus
}
#endif
#endif
