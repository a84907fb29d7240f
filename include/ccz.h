/*
 * libccz -- MI355X (gfx950) CCA solver core: C ABI.
 *
 * The reference (jameschapman19/cca_zoo) is pure Python and has NO FFI: its
 * hot path calls NumPy/SciPy/scikit-learn/torch directly.  This header is the
 * flat C boundary a maintainer would bind (ctypes) to put
 * the device path behind the reference's own seams.  Each entry cites the
 * reference call site(s) it replaces, relative to the reference repo root.
 *
 * Conventions
 *   - return 0 (CCZ_OK) or a negative CCZ_E* code; text via ccz_last_error()
 *   - the caller owns every input/output buffer; the handle owns only scratch
 *   - "dev" pointers are device (HBM) addresses, "host" pointers host addresses
 *   - matrices are row-major, leading dimension in ELEMENTS, sizes int64_t
 *   - a handle is bound to one device and one HIP stream; not thread-safe
 *   - no C++/torch types cross this boundary
 *   - the CCZ_* environment variables the library reads (two are named below) are listed, with their defaults and the
 *     moment each is read, in the one table of cca_zoo_amd/csrc/env.h
 */
#ifndef CCZ_H
#define CCZ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCZ_VERSION 150 /* 0.1.5: ccz_k1_route (split-bf16 route of K1 and of the loss's large backward), ccz_moments_last_route,
                          * ccz_loss_last_route, ccz_pool_trim; the loss state grew by 2 D doubles (opaque: ccz_pair_loss_state_bytes).
                          * (Two constants since, no new entry: CCZ_BF16 and CCZ_F16, the 2-byte formats of the deep objectives.)
                          * (Two entries since: ccz_transform_wide and ccz_transform_last_route, bfloat16 views of the closed-form estimators.)
                          * 0.1.4: ccz_pair_loss_forward / _backward / _state_bytes (the loss as an autograd node in two phases),
                          * ccz_moments_exchange (the whole exchange step), ccz_solve_defer(h, NULL) = await a pending deferral now */

#if defined(__GNUC__)
#define CCZ_API __attribute__((visibility("default")))
#else
#define CCZ_API
#endif

#define CCZ_OK 0
#define CCZ_EINVAL (-1)   /* bad argument                                   -> ValueError   */
#define CCZ_ENOMEM (-2)   /* device allocation failed                       -> MemoryError  */
#define CCZ_EHIP (-3)     /* HIP runtime error                              -> RuntimeError */
#define CCZ_ENOCONV (-4)  /* iterative solver did not converge              -> LinAlgError  */
#define CCZ_ENOTSPD (-5)  /* Cholesky met a non-positive pivot              -> LinAlgError  */
#define CCZ_EUNSUP (-6)   /* unsupported dtype / configuration              -> ValueError   */
#define CCZ_ERCCL (-7)    /* RCCL unavailable / collective failed           -> RuntimeError */

#define CCZ_F32 0
#define CCZ_F64 1
/* The 2-byte formats of the deep objectives' batches (torch.autocast): DEVICE rows only, accepted by ccz_moments / _opts,
 * ccz_transform, ccz_transform_wide (float32 out_dev), ccz_cca_loss, ccz_pair_loss / _forward / _backward / _state_bytes and ccz_moment_loss_forward /
 * _state_bytes; every other entry that takes a dtype, and host views, answer CCZ_EUNSUP.  An element is widened exactly to
 * float32 on load and everything after that is the CCZ_F32 route; rows that are written (gradients, projections) are formed in
 * float32 and rounded once, to nearest even.  For these dtypes loss_dev and grad_out_dev are ONE float32 element (a bfloat16
 * scalar has 8 bits), the state has the CCZ_F32 layout, and g_dev / out_dev are of `dtype`. */
#define CCZ_BF16 2
#define CCZ_F16 3

typedef struct ccz_ctx* ccz_handle;

/* One view (an n x cols block of the sample matrix), row-major. */
typedef struct ccz_view {
  const void* data; /* first element (host or device, see the call) */
  int64_t cols;     /* features d_i                                  */
  int64_t ld;       /* elements between consecutive rows (>= cols)   */
} ccz_view;

typedef struct ccz_devinfo {
  char name[128];
  char arch[32];
  int compute_units;
  int wavefront;
  int64_t hbm_bytes;
  int64_t lds_bytes_per_cu;
} ccz_devinfo;

/* ---- lifecycle ---------------------------------------------------------- */
CCZ_API int ccz_version(void);
CCZ_API int ccz_create(ccz_handle* out, int device);
CCZ_API int ccz_destroy(ccz_handle h);
CCZ_API const char* ccz_last_error(ccz_handle h);
/* stream = hipStream_t as void* (torch: torch.cuda.current_stream().cuda_stream); NULL = the handle's own stream.
 * Waits for the handle's pending work first (a host synchronisation: see ccz_stream_adopt for the non-blocking form) */
CCZ_API int ccz_set_stream(ccz_handle h, void* stream);
CCZ_API int ccz_sync(ccz_handle h);
/* Stream-native use from a framework that owns its streams (the DCCA objective inside a training step,
 * deep/_base.py:78-104: the loss is one autograd node between the encoders' forward and backward): instead of
 * draining the caller's stream before a libccz call and libccz's stream after it,
 *   ccz_stream_acquire(h, s):  the handle's stream waits (on the DEVICE) for everything enqueued on s so far;
 *   ccz_stream_release(h, s):  s waits (on the device) for everything the handle has enqueued so far.
 * Neither blocks the host.  s = hipStream_t as void*; NULL = the legacy default stream, with which the handle's own
 * (blocking) stream is ordered implicitly -- then nothing is enqueued at all. */
CCZ_API int ccz_stream_acquire(ccz_handle h, void* stream);
CCZ_API int ccz_stream_release(ccz_handle h, void* stream);
/* ccz_stream_adopt(h, s): from now on the handle ENQUEUES INTO s itself (ordered after what it had pending on its previous
 * stream) -- the objective's kernels then sit in the same hardware queue as the encoders' and no cross-queue signal is
 * waited for on either side (measured: ~0.1 ms per hand-over at configs[3]).  It stays there until the next
 * ccz_stream_acquire (which first returns to the handle's own stream) or ccz_set_stream; ccz_stream_release(h, s) after
 * an adopt of the same s is a no-op.  Sequences the library replays as hipGraphs are launched directly on the legacy
 * default stream (it cannot be captured). */
CCZ_API int ccz_stream_adopt(ccz_handle h, void* stream);
CCZ_API int ccz_device_info(ccz_handle h, ccz_devinfo* out);

/* ---- raw device memory for callers that do not bring torch tensors ------- */
CCZ_API int ccz_dev_alloc(ccz_handle h, void** out, size_t bytes);
CCZ_API int ccz_dev_free(ccz_handle h, void* p);
CCZ_API int ccz_memcpy_h2d(ccz_handle h, void* dst_dev, const void* src_host, size_t bytes);
CCZ_API int ccz_memcpy_d2h(ccz_handle h, void* dst_host, const void* src_dev, size_t bytes);
CCZ_API int ccz_memset0(ccz_handle h, void* dst_dev, size_t bytes);
/* The handle keeps released scratch (solver blocks, the split route's bf16 planes and partial tiles: tens of GB at
 * n = 1e6) in a pool for the next call.  ccz_pool_trim waits for the handle's stream and returns every unused block to
 * the driver -- for callers about to allocate most of HBM themselves (torch.cuda.empty_cache() is the analogue). */
CCZ_API int ccz_pool_trim(ccz_handle h, size_t* released_bytes);

/* ---- K1: second moments ---------------------------------------------------
 * moments = [ G (D x D, ld = D) | colsum (D) ]  float64, D = sum cols, device.
 *   G      += [X_1..X_m]' [X_1..X_m]   (upper-triangular TILES only; the solves read
 *                                        the upper triangle, ccz_moments_symmetrize
 *                                        completes G for other consumers)
 *   colsum += 1' [X_1..X_m]
 * One call handles one row shard; accumulate=0 zeroes `moments` first.  fp32
 * views are multiplied on the fp32 MFMA pipe in row chunks and accumulated in
 * fp64 across chunks; fp64 views use the fp64 MFMA pipe throughout.
 * Replaces: np.linalg.svd(X) _utils/_linalg.py:28 + X1_w.T @ X2_w
 *   linear/_rcca.py:96; np.cov linear/_mcca.py:151-152,166, linear/_gcca.py:101;
 *   v.mean(axis=0) / v - m  _base.py:97-99.
 */
CCZ_API int ccz_moments(ccz_handle h, int dtype, const ccz_view* views, int n_views, int64_t n_rows,
                int views_on_device, double* moments_dev, int accumulate);
/* ccz_moments with its two policies exposed: pilot_mode 0 = never shift, 1 = automatic (ccz_moments; one small
 * read-back of the column sums decides), 2 = always shift fp32 views (no read-back); timed = 0 skips the HIP-event
 * timing of ccz_moments_last_ms, whose read-out makes the host wait for K1 -- with (2, 0) or fp64 views the call only
 * ENQUEUES work on the handle's stream (the stream-native losses use it that way). */
CCZ_API int ccz_moments_opts(ccz_handle h, int dtype, const ccz_view* views, int n_views, int64_t n_rows,
                int views_on_device, double* moments_dev, int accumulate, int pilot_mode, int timed);
CCZ_API int ccz_moments_symmetrize(ccz_handle h, double* moments_dev, int64_t D);
/* Packed form for the one collective of the sharded path: [ upper triangle of G, row-major,
 * D(D+1)/2 | colsum (D) ] -- half the bytes of the full buffer on the wire.  pack: moments -> packed;
 * unpack: packed -> upper triangle of moments (+ colsum); the lower triangle is left untouched. */
CCZ_API int ccz_moments_pack(ccz_handle h, const double* moments_dev, int64_t D, double* packed_dev);
CCZ_API int ccz_moments_unpack(ccz_handle h, const double* packed_dev, int64_t D, double* moments_dev);
/* The same exchange in TWO parts, ordered so that the solve can start before the exchange has finished (SURVEY.md 8(e):
 * the per-view factorizations need the diagonal blocks only).  Blocks layout, doubles:
 *   head = [ upper triangle of C_11 | .. | upper triangle of C_mm | colsum (D) | 1 spare slot for the caller's row count ]
 *   tail = [ C_12 | C_13 | .. | C_(m-1)m ]   (each d_i x d_j, row-major)
 *   packed = [ head | tail ],  sum d_i (d_i + 1) / 2 + D + 1 + sum_{i<j} d_i d_j  =  D (D + 1) / 2 + D + 1 doubles.
 * which: 1 = head, 2 = tail, 3 = both.  unpack's on_stream (hipStream_t as void*, NULL = the handle's stream) lets the
 * tail be unpacked on the stream the collective completes on; ccz_solve_defer(h, event) then makes the NEXT
 * ccz_{rcca,mcca,gcca}_solve wait for `event` (hipEvent_t as void*, recorded after that unpack) on the device right
 * before its first read of an off-diagonal block -- i.e. after the Cholesky chain of the diagonal blocks.
 * ccz_solve_defer(h, NULL): whatever is pending (this registration, a foreign-stream unpack's, ccz_moments_exchange's tail) is
 * awaited NOW on the handle's stream (device-side; the host does not block) and cleared -- for callers that read off-diagonal
 * blocks of the moments through entry points other than the three solves. */
CCZ_API int ccz_moments_pack_blocks(ccz_handle h, const double* moments_dev, int64_t D, const int64_t* dims, int n_views,
                                    double* packed_dev, int which);
CCZ_API int ccz_moments_unpack_blocks(ccz_handle h, const double* packed_dev, int64_t D, const int64_t* dims, int n_views,
                                      double* moments_dev, int which, void* on_stream);
CCZ_API int ccz_solve_defer(ccz_handle h, void* event);
/* ---- the exchange step itself: RCCL all-reduce(sum) over xGMI (SURVEY.md 8(b) "ccz_allreduce_sum_f64", 8(e)) ----------
 * The reference has no counterpart (single process, NumPy).  A caller WITHOUT torch.distributed shards like this:
 *   one process per GPU:  rank 0 calls ccz_comm_unique_id and ships the 128 bytes to the other ranks (file, socket, MPI);
 *     every rank: ccz_comm_init_rank(h, id, world, rank);  per fit: ccz_moments -> ccz_moments_pack[_blocks] ->
 *     ccz_allreduce_sum_f64(h, packed_dev, count) -> ccz_moments_unpack[_blocks] -> ccz_*_solve.
 *   one process, several GPUs:  ccz_comm_init_all(handles, n) once; per fit the packed buffers of all devices go through
 *     ONE grouped call, ccz_allreduce_sum_f64_multi(handles, bufs_dev, n, count).
 * The collective is enqueued on the handle's stream (in place, float64, sum) and does not block the host.  librccl is
 * dlopen'ed at the first of these calls (CCZ_ERCCL if it cannot be found); ccz_comm_destroy (or ccz_destroy) frees the
 * communicator.  ccz_comm_info: world size (0: none) and this handle's rank. */
CCZ_API int ccz_comm_unique_id(ccz_handle h, void* id_out_128);
CCZ_API int ccz_comm_init_rank(ccz_handle h, const void* id_128, int world, int rank);
CCZ_API int ccz_comm_init_all(ccz_handle* handles, int n);
CCZ_API int ccz_comm_info(ccz_handle h, int* world_out, int* rank_out);
CCZ_API int ccz_comm_destroy(ccz_handle h);
CCZ_API int ccz_allreduce_sum_f64(ccz_handle h, double* buf_dev, int64_t count);
CCZ_API int ccz_allreduce_sum_f64_multi(ccz_handle* handles, double* const* bufs_dev, int n, int64_t count);
/* The whole exchange step of a row-sharded fit in ONE call -- what cca_zoo's fit would run between its second-moment pass and
 * its solve (linear/_rcca.py:69-101, _mcca.py:99-197, _gcca.py:80-110 on a rank's rows): moments_dev ([G | s] of THIS rank's
 * n_local rows) is packed in the blocks layout into a buffer the handle keeps between fits, the row count is written into the
 * head's spare slot on the device, head and tail are all-reduced on a stream of the handle's own, the head is unpacked on the
 * handle's stream, the tail behind its collective -- the next ccz_{rcca,mcca,gcca}_solve waits for that on the device right
 * before its first off-diagonal read, i.e. the tail's transfer overlaps the per-view factorizations (any OTHER reader of the
 * off-diagonal blocks calls ccz_solve_defer(h, NULL) first).  *n_total_out: the global row count (the call's only host read).  Needs ccz_comm_init_rank / _init_all.  CCZ_RCCL_LIB=path pins the RCCL
 * library that is dlopen'ed. */
CCZ_API int ccz_moments_exchange(ccz_handle h, double* moments_dev, int64_t D, const int64_t* dims, int n_views,
                                 int64_t n_local, int64_t* n_total_out);
/* Moments are additive over disjoint row sets: y <- alpha x + beta y over the D*D + D doubles of two
 * moment buffers.  With (alpha, beta) = (-1, 1) it turns the moments of all rows into those of the rows
 * outside a cross-validation fold -- the Gram reuse behind cca_zoo_amd.model_selection.GridSearchCV
 * (the reference refits from the data for every fold and setting: cca_zoo/model_selection/_search.py:211-262). */
CCZ_API int ccz_moments_axpby(ccz_handle h, int64_t D, double alpha, const double* x_dev, double beta, double* y_dev);
/* Moments of a contiguous subset [col0, col0 + D_sub) of the stacked columns: the D_sub x D_sub block of G
 * (upper triangle authoritative, as produced by ccz_moments) and the matching column sums, repacked into a
 * [G | s] buffer of width D_sub.  Lets one K1 pass over [confounds | views] serve PartialCCA
 * (cca_zoo/linear/_partialcca.py:67-103: the views' block is then corrected by a rank-(1 + dz) GEMM). */
CCZ_API int ccz_moments_subset(ccz_handle h, const double* moments_dev, int64_t D, int64_t col0, int64_t D_sub,
                               double* subset_dev);
/* kernel timing of the last ccz_moments call on this handle (HIP events on the
 * handle's stream): milliseconds of the Gram kernel(s) and of the column-sum pass */
CCZ_API int ccz_moments_last_ms(ccz_handle h, double* gram_ms, double* colsum_ms);
/* fp32 views whose column means are large against their spread (max_j |mean_j| / std_j > 2, read off the column
 * sums and sums of squares that K1 forms first) are multiplied as (x - p)(x - p)' with the pilot p = fl32(mean of
 * the launch's rows) subtracted while staging, and the shift is undone on the d x d side in fp64 -- the reference
 * centres before any product (_base.py:97-99) and raw fp32 products would cancel catastrophically.  *used = 1 if
 * the last ccz_moments launch on this handle took that path. */
CCZ_API int ccz_moments_last_pilot(ccz_handle h, int* used);
/* Arithmetic route of fp32 views through K1 (fp64 views always run on the fp64 matrix pipe).
 *   CCZ_K1_FP32    v_mfma_f32_32x32x2_f32 on the fp32 rows as they lie (the reference's own precision:
 *                  np.linalg.svd in float32, _utils/_linalg.py:28; X1_w.T @ X2_w, linear/_rcca.py:96);
 *   CCZ_K1_BF16X2  x - pilot = hi + mid (two bf16 planes, written by one transposing pass over the rows), the
 *                  products hi'hi + hi'mid + mid'hi as three v_mfma_f32_32x32x16_bf16 into one fp32 accumulator,
 *                  diag(sum mid^2) added back exactly -- 3 bf16 MFMAs for each fp32 one at 16x the rate; agreement
 *                  with float64 moments is measured beside the fp32 route's in bench.py (k1_rel_err).  The pilot of a float32
 *                  column is the mean of a row sample; where the sampled values lie on a grid (0/1, one-hot, pixel values,
 *                  counts, integers, values up-cast from bfloat16) that mean rounded to few bits (2^(ilogb(sd) - 3)), so
 *                  that such columns keep their grid and their moments are exact.  Deliberately NOT
 *                  float64's result: an off-diagonal entry of two identical columns (a view passed twice, columns shared
 *                  between views) lacks sum mid^2, about 3e-6 of the entry whatever the row count -- rCCA on [X, X] reports
 *                  canonical correlations of 1 - 2.5e-6 (tests/test_gpu_k1_split_structured.py pins it);
 *   CCZ_K1_AUTO    (default) CCZ_K1_BF16X2 where it pays AND is at least as accurate as the fp32 kernel (n >= 32768 rows,
 *                  n D (D+1) >= 1e11, D >= 256), else CCZ_K1_FP32.
 * The environment variable CCZ_K1_ROUTE = fp32 | bf16x2 overrides AUTO.  route = -1 only queries; *previous (may be
 * NULL) receives the handle's setting before the call. */
#define CCZ_K1_AUTO 0
#define CCZ_K1_FP32 1
#define CCZ_K1_BF16X2 2
#define CCZ_K1_FP64 3
CCZ_API int ccz_k1_route(ccz_handle h, int route, int* previous);
/* route the last ccz_moments launch on this handle took (CCZ_K1_FP32 / CCZ_K1_BF16X2 / CCZ_K1_FP64) and, for a timed
 * CCZ_K1_BF16X2 launch, the HIP-event milliseconds of its three stages: the split pass (HBM-bound), the bf16 MFMA kernel
 * and the fp64 reduce of the partial tiles (0 otherwise).  Any pointer may be NULL. */
CCZ_API int ccz_moments_last_route(ccz_handle h, int* route, double* split_ms, double* mfma_ms, double* reduce_ms);

/* ---- fused solves on reduced moments (replicated after the all-reduce) ----
 * Inputs: moments (device; only the upper triangle of G is read, so no symmetrisation is
 * needed), total rows n, per-view widths.
 * Outputs (HOST, float64, row-major): weights packed view after view, each
 * (d_i x k_out); means (D) ; vals (k_out).
 */
/* linear/_rcca.py:69-101 (rCCA.fit; CCA c=0 linear/_cca.py:52; PLS c=1 linear/_pls.py:53) */
CCZ_API int ccz_rcca_solve(ccz_handle h, const double* moments_dev, int64_t n, const int64_t dims[2],
                   const double c[2], int center, int k, double* weights_host,
                   double* means_host, double* vals_host, int* k_out);
/* linear/_mcca.py:99-197 (MCCA.fit, _build_A, _build_B, _build_B_pca, gevp) */
CCZ_API int ccz_mcca_solve(ccz_handle h, const double* moments_dev, int64_t n, const int64_t* dims,
                   int n_views, const double* c, double eps, int center, int k,
                   double* weights_host, double* means_host, double* vals_host, int* k_out);
/* linear/_gcca.py:80-110 (GCCA.fit) restated in D x D Gram form */
CCZ_API int ccz_gcca_solve(ccz_handle h, const double* moments_dev, int64_t n, const int64_t* dims,
                   int n_views, const double* c, const double* view_weights, double eps,
                   int center, int k, double* weights_host, double* means_host,
                   double* vals_host, int* k_out);

/* ---- dense function seams (device in/out, float64) ------------------------ */
/* full symmetric EVD by one-sided Jacobi: A (d x d, overwritten) -> w (d, descending),
 * V (d x d, row i = eigenvector i).  torch.linalg.eigh deep/objectives.py:19;
 * np.linalg.eigvalsh linear/_mcca.py:170,194, linear/_gcca.py:102 */
CCZ_API int ccz_syevj(ccz_handle h, double* A_dev, int64_t d, double* w_dev, double* V_dev,
              int* sweeps_out);
/* full SVD by one-sided Jacobi: A (p x q) = U diag(s) Vt, r = min(p,q); U (p x r),
 * s (r, descending), Vt (r x q).  np.linalg.svd linear/_rcca.py:97 */
CCZ_API int ccz_gesvj(ccz_handle h, const double* A_dev, int64_t p, int64_t q, double* U_dev,
              double* s_dev, double* Vt_dev, int* sweeps_out);
/* top-k symmetric (generalised) eigenpairs, descending; B_dev may be NULL.
 * V (p x k), B-normalised (v'Bv = 1).  gevp _utils/_linalg.py:44-73 */
CCZ_API int ccz_gevp_topk(ccz_handle h, const double* A_dev, const double* B_dev, int64_t p, int k,
                  double* w_dev, double* V_dev);
/* top-k singular triplets of T (p x q): U (p x k), s (k), V (q x k) */
CCZ_API int ccz_svd_topk(ccz_handle h, const double* T_dev, int64_t p, int64_t q, int k,
                 double* U_dev, double* s_dev, double* V_dev);
/* whitening matrix from the Gram of a centred view: lam (r) descending eigenvalues of
 * Gxx/(n-1), W (d x r) = V ((1-ridge) lam + ridge)^-1/2, r = min(n, d).
 * svd_whiten _utils/_linalg.py:9-41 */
CCZ_API int ccz_whitener(ccz_handle h, const double* Gxx_dev, int64_t d, int64_t n, double ridge,
                 double* W_dev, double* lam_dev, int64_t* r_out);
/* A^-1/2 with eigenvalues clamped at eps.  _inv_sqrtm deep/objectives.py:9-21 */
CCZ_API int ccz_inv_sqrtm(ccz_handle h, const double* A_dev, int64_t d, double eps, double* out_dev);

/* building blocks (exported for tests and for the seams above) */
CCZ_API int ccz_potrf_lower(ccz_handle h, double* A_dev, int64_t d, int64_t lda);
/* X (r x d) <- X L^-T (trans=1) or X L^-1 (trans=0), L lower (d x d) */
CCZ_API int ccz_trsm_right_lower(ccz_handle h, int trans, int64_t r, int64_t d, const double* L_dev,
                         int64_t ldl, double* X_dev, int64_t ldx);
/* C (M x N) = alpha op(A) op(B) + beta C; op = transpose when the flag is 1 */
CCZ_API int ccz_gemm_f64(ccz_handle h, int transA, int transB, int64_t M, int64_t N, int64_t K,
                 double alpha, const double* A_dev, int64_t lda, const double* B_dev, int64_t ldb,
                 double beta, double* C_dev, int64_t ldc);

/* ---- DCCA correlation loss -------------------------------------------------
 * loss = -tr(S11^-1 S12 S22^-1 S21), S from the centred batch (+ eps I), and the
 * closed-form input gradients.  dtype CCZ_F32 or CCZ_F64 for z / grads / loss.
 * Any of g1/g2 may be NULL (forward only).  loss_dev: one element of `dtype`.
 * deep/objectives.py:61-102 (CCALoss.forward) + its autograd backward.
 */
CCZ_API int ccz_cca_loss(ccz_handle h, int dtype, const void* z1_dev, const void* z2_dev, int64_t n,
                 int64_t d1, int64_t d2, int64_t ld1, int64_t ld2, double eps, void* loss_dev,
                 void* g1_dev, void* g2_dev, int64_t ldg1, int64_t ldg2);
/* The sum over all view pairs a < b of that loss for n_views (2 .. 8) views of one batch, any widths -- MCCALoss,
 * deep/objectives.py:138-153 (n_views = 2 IS ccz_cca_loss) -- and its gradient with respect to every view: ONE K1
 * pass over [z_1 .. z_m], ONE Cholesky + inverse per VIEW (the reference re-centres every view and recomputes its
 * S_aa^-1/2 once per PAIR).  z_dev: HOST array of n_views device views; g_dev: NULL (forward only) or a HOST array of
 * n_views device pointers (entries may be NULL), ldg their leading dimensions; loss_dev: one element of `dtype`. */
CCZ_API int ccz_pair_loss(ccz_handle h, int dtype, const ccz_view* z_dev, int n_views, int64_t n, double eps,
                  void* loss_dev, void* const* g_dev, const int64_t* ldg);
/* The same loss in two phases, for callers inside an autograd graph (the reference's loss IS such a node: CCALoss.forward,
 * deep/objectives.py:61-102, is differentiated by torch; its backward receives the upstream gradient of the scalar loss,
 * cca_zoo/deep/_base.py:78-104).  ccz_pair_loss_forward evaluates the loss and leaves what the backward needs -- Gamma, the
 * centring row, for fp32 views also Gamma in fp32 -- in state_dev: caller-owned device memory of
 * ccz_pair_loss_state_bytes(dtype, dims, n_views) bytes (state_dev = NULL: forward only).  ccz_pair_loss_backward writes
 *   g_a = (*grad_out_dev) * d loss / d z_a     (grad_out_dev: ONE element of `dtype` on the device, NULL = 1)
 * for the SAME views (entries of g_dev may be NULL).  Two aligned fp32 views: one fp32 MFMA product that reads the views
 * where they lie; the upstream gradient is applied inside it.  ccz_pair_loss == forward + backward(NULL). */
CCZ_API int64_t ccz_pair_loss_state_bytes(int dtype, const int64_t* dims, int n_views);
CCZ_API int ccz_pair_loss_forward(ccz_handle h, int dtype, const ccz_view* z_dev, int n_views, int64_t n, double eps,
                          void* loss_dev, void* state_dev);
CCZ_API int ccz_pair_loss_backward(ccz_handle h, int dtype, const ccz_view* z_dev, int n_views, int64_t n,
                           const void* state_dev, const void* grad_out_dev, void* const* g_dev, const int64_t* ldg);
/* Moment-map losses of the reference's self-supervised models (cca_zoo/deep/_dcca_ey.py:10-111, _barlowtwins.py:83-112,
 * _vicreg.py:12-67 and :142-169, _dcca_sdl.py:12-26 and :100-121) for n_views views of ONE width d: the value and the terms from one K1
 * pass over [z_1 .. z_m], a map on the D x D moments and, for VICReg / SDL, a streaming pass for mean((z_1 - z_2)^2).
 *   kind            params                              views    terms_dev (3 doubles, may be NULL)
 *   CCZ_MOMENT_EY      --  (params may be NULL)            2 .. 8   rewards, penalties, 0
 *   CCZ_MOMENT_BARLOW  lam                                 2        invariance, redundancy, 0
 *   CCZ_MOMENT_VICREG  sim_coeff, std_coeff, cov_coeff     2        sim_loss, var_loss, cov_loss
 *   CCZ_MOMENT_SDL     lam                                 2 .. 8   l2, sdl, 0        (d >= 2)
 * loss_dev: ONE element of `dtype`, the objective.  state_dev (NULL: forward only): ccz_moment_loss_state_bytes(dtype, d, n_views)
 * bytes in the layout of ccz_pair_loss_forward's state -- the gradients are ccz_pair_loss_backward on the same views and that state.
 * EY takes an optional independent batch (ind_dev: n_views views of width d, n_ind rows; the penalty becomes tr(V V_ind)); its own
 * gradient is ccz_pair_loss_backward on ind_dev, n_ind and state_ind_dev (NULL: not wanted).  Enqueue-only, no host synchronisation. */
#define CCZ_MOMENT_EY 0
#define CCZ_MOMENT_BARLOW 1
#define CCZ_MOMENT_VICREG 2
#define CCZ_MOMENT_SDL 3
CCZ_API int64_t ccz_moment_loss_state_bytes(int dtype, int64_t d, int n_views);
CCZ_API int ccz_moment_loss_forward(ccz_handle h, int dtype, int kind, const double* params, const ccz_view* z_dev, int n_views, int64_t n,
                                    const ccz_view* ind_dev, int64_t n_ind, void* loss_dev, double* terms_dev, void* state_dev,
                                    void* state_ind_dev);
/* ccz_cca_loss / ccz_pair_loss never read the factorization's pivot flags back (no host synchronisation between the encoders' forward
 * and backward).  If S_aa + eps I was not positive definite the loss written to loss_dev is NaN and the handle keeps a
 * sticky record: *view = 1 + index of the failing view (0: none since the last query), *pivot = the failing pivot;
 * querying clears it.  synchronise = 0 reads what has been recorded so far without waiting (a wrapper calls this
 * before its NEXT loss call); synchronise = 1 drains the handle's stream first.  (The reference clamps eigenvalues at
 * eps instead, deep/objectives.py:9-21, and cannot fail; with eps > 0 neither can this, short of NaN inputs.) */
CCZ_API int ccz_loss_status(ccz_handle h, int synchronise, int* view, int* pivot);
/* Arithmetic routes of the last loss on this handle: *forward_route = route of its K1 (as ccz_moments_last_route),
 * *backward_route = route of the gradient product ([dz_1 | dz_2] = ([z_1 | z_2] - 1 mean') Gamma): CCZ_K1_BF16X2 when a
 * two-view fp32 backward is a large product (n >= 32768, 2 n D^2 >= 2e11) and the handle's ccz_k1_route is not CCZ_K1_FP32 --
 * the same split arithmetic as K1's (csrc/gemm_split.hip) -- else CCZ_K1_FP32 / CCZ_K1_FP64; 0 before the first backward. */
CCZ_API int ccz_loss_last_route(ccz_handle h, int* forward_route, int* backward_route);
/* The same loss for a batch that is row-sharded over ranks: `moments_dev` holds the batch moments of
 * [z1 | z2] summed over all shards (ccz_moments per rank + one all-reduce), n_rows the total batch size.
 * Returns the loss (host) and, if gamma_dev != NULL, the (d1+d2) x (d1+d2) matrix Gamma and the batch mean
 * (d1+d2) such that  [dz1 | dz2] = ([z1 | z2] - 1 mean') Gamma  for ANY subset of the rows: each rank
 * applies it to its own shard with ccz_transform.  (Reference: the single-process CCALoss.forward,
 * cca_zoo/deep/objectives.py:61-102; a DDP batch would otherwise need an all-gather of the embeddings.) */
CCZ_API int ccz_cca_loss_moments(ccz_handle h, const double* moments_dev, int64_t n_rows, int64_t d1, int64_t d2,
                                 double eps, double* loss_host, double* gamma_dev, double* mean_dev);

/* Sum over all pairs a < b of the CCA loss of views a and b -- MCCALoss, cca_zoo/deep/objectives.py:138-153, which
 * re-centres every view and recomputes its S_aa^-1/2 once per PAIR -- from ONE set of batch moments of [z_1 .. z_m]
 * with ONE Cholesky + inverse per VIEW.  Outputs as ccz_cca_loss_moments (n_views = 2 is that entry). */
CCZ_API int ccz_pair_loss_moments(ccz_handle h, const double* moments_dev, int64_t n_rows, const int64_t* dims,
                                  int n_views, double eps, double* loss_host, double* gamma_dev, double* mean_dev);

/* MAX-VAR GCCA loss of a batch from its moments (ccz_moments over [z_1 .. z_m], summed over the ranks when the
 * batch is row-sharded): loss = -(n-1) sum of the top-k generalised eigenvalues of  C u = lam B u  with C the
 * centred covariance of the stacked views and B = blockdiag(C_ii) + eps I -- the non-zero spectrum of the
 * reference's n x n matrix sum_i H_i H_i' -- and, if gamma_dev != NULL, the D x D matrix Gamma and the batch mean
 * (D) with  [dz_1 .. dz_m] = ([z_1 .. z_m] - 1 mean') Gamma  (apply with ccz_transform).  All D x D work stays on
 * the device.  cca_zoo/deep/objectives.py:155-220 (GCCALoss.forward) + its autograd backward. */
CCZ_API int ccz_gcca_loss_moments(ccz_handle h, const double* moments_dev, int64_t n_rows, const int64_t* dims,
                                  int n_views, double eps, int k, double* loss_host, double* gamma_dev,
                                  double* mean_dev);

/* ---- transform / score -------------------------------
 * out (n x k, dtype) = (X - mean) W ; X,out device; mean (d), W (d x k) device float64.
 * Enqueue-only on the handle's stream (no host synchronisation): follow with ccz_sync / ccz_stream_release /
 * ccz_memcpy_d2h before another stream or the host reads `out`.
 * _base.py:108-123 */
CCZ_API int ccz_transform(ccz_handle h, int dtype, const void* X_dev, int64_t n, int64_t d, int64_t ld,
                  const double* mean_dev, const double* W_dev, int64_t k, void* out_dev,
                  int64_t ldo);
/* The same projection for 2-byte device rows with a FLOAT32 result (the closed-form estimators' transform / score on bfloat16
 * views: the variates are never rounded to the rows' format).  dtype is CCZ_BF16 or CCZ_F16 (anything else: CCZ_EUNSUP); the
 * argument checks and the stream semantics are ccz_transform's.  CCZ_BF16 rows with 1 <= k <= 64, d % 16 == 0, ld % 8 == 0 and a
 * 16-byte aligned X_dev are multiplied as they lie on the bf16 matrix pipe (csrc/project_bf16.hip: a bf16 element is an exact
 * MFMA operand; W enters as three bf16 planes hi + mid + lo = fl32(W), every product is exact in float32; two calls give the
 * same bits).  Everything else -- CCZ_F16, other shapes, CCZ_PROJECT_BF16=0 -- is widened exactly into float32 scratch and
 * takes the CCZ_F32 projection of ccz_transform, written straight into out_dev.  Columns k .. ldo - 1 of out_dev are not
 * touched. */
CCZ_API int ccz_transform_wide(ccz_handle h, int dtype, const void* X_dev, int64_t n, int64_t d, int64_t ld,
                               const double* mean_dev, const double* W_dev, int64_t k, float* out_dev, int64_t ldo);
/* *route = what the last ccz_transform_wide on this handle did: 0 none yet, 1 the bf16 MFMA kernel, 2 the widening adapter. */
CCZ_API int ccz_transform_last_route(ccz_handle h, int* route);

/* Batched Cholesky factor + triangular inverse (building block of the loss and of the blocked solves; exported
 * for tests): `count` <= 8 SPD matrices A_dev[b] (d[b] x d[b], ld d[b], destroyed), L_dev[b] <- lower factor (the
 * part above the diagonal is left untouched), X_dev[b] <- L^-1 (lower; blocks of 64 columns strictly above the
 * diagonal blocks are left untouched -- zero X first if they are read).  X_dev may be NULL (factor only).  All matrices
 * advance together, d_max / 64 + 1 launches in total.  Pointer arrays are HOST arrays of device pointers.
 * torch.linalg.eigh + clamp + V diag(L^-1/2) V' in _inv_sqrtm, deep/objectives.py:9-21, as used by :94-97 */
CCZ_API int ccz_cholinv(ccz_handle h, int count, double* const* A_dev, const int64_t* d, double* const* L_dev,
                        double* const* X_dev);

/* Counter-based standard normals written straight into HBM (the at-scale JointData inputs):
 *   out[r][c] = (accumulate ? out[r][c] : 0) + scale * N(seed, (row0 + r) * row_stride + c)
 * with N(seed, i) a pure function of its arguments (csrc/rng_hash.h::hash_normal_pair; NumPy restatement in
 * oracle/rng.py), so any row range can be regenerated anywhere.  row_stride even and >= cols; dtype CCZ_F32 / CCZ_F64.
 * cca_zoo/datasets/_simulated.py:116-130 (rng.standard_normal for z and the per-view noise) */
CCZ_API int ccz_randn_fill(ccz_handle h, int dtype, void* out_dev, int64_t rows, int64_t cols, int64_t ld, uint64_t seed,
                           int64_t row0, int64_t row_stride, double scale, int accumulate);

/* Factor loadings of ONE view from its second moments (ccz_moments on that view alone, d x d + d):
 * out (d x k, device, float64) = corr(feature j, variate t) = (C W)_jt / (std_x_j std_z_t) with C the centred
 * covariance, std_z^2 = diag(W'CW), and the reference's guards max(std, 1e-12).  W (d x k) device float64.
 * cca_zoo/_base.py:208-234 (get_factor_loadings: n x d x k products on the host) */
CCZ_API int ccz_factor_loadings(ccz_handle h, const double* moments_dev, int64_t n_rows, int64_t d,
                                const double* W_dev, int64_t k, double* out_dev);

/* ---- nonparametric models: kernel matrices, KCCA / KGCCA (csrc/kernel_matrix.hip, csrc/kcca.cpp) ----------------
 * Kernel kinds: scikit-learn's pairwise_kernels(..., filter_params=True).  gamma is always explicit here (the
 * estimators resolve None to 1 / n_features); degree is a real exponent; parameters a kind does not take are ignored. */
#define CCZ_KERNEL_LINEAR 0   /* <a, b>                                                     */
#define CCZ_KERNEL_POLY 1     /* (gamma <a, b> + coef0)^degree                              */
#define CCZ_KERNEL_RBF 2      /* exp(-gamma max(||a||^2 + ||b||^2 - 2 <a, b>, 0))           */
#define CCZ_KERNEL_SIGMOID 3  /* tanh(gamma <a, b> + coef0)                                 */
#define CCZ_KERNEL_COSINE 4   /* <a, b> / (||a|| ||b||), 0 for a zero row                   */

/* K (na x nb, device float64, ld ldk) = f(a_i - meanA, b_j - meanB) over the rows of A (na x d, ld lda) and B (nb x d,
 * ld ldb), both CCZ_F32 or both CCZ_F64 (fp32 is widened exactly; all products on the fp64 matrix pipe).  meanA /
 * meanB (d, device float64) are optional and independent: each is subtracted on load when non-NULL.  A_dev == B_dev
 * with the same shape, ld and mean is the symmetric case: only tiles on and above the diagonal are computed and then
 * mirrored, and the rbf distance on the diagonal is exactly 0 (K_ii = 1).  Enqueue-only on the handle's stream.
 * cca_zoo/nonparametric/_kcca.py:195-196 (pairwise_kernels in _compute_kernels), _kgcca.py:120-127 */
CCZ_API int ccz_pairwise_kernel(ccz_handle h, int dtype, const void* A_dev, int64_t na, int64_t lda, const double* meanA_dev,
                                const void* B_dev, int64_t nb, int64_t ldb, const double* meanB_dev, int64_t d, int kind,
                                double gamma, double degree, double coef0, double* K_dev, int64_t ldk);

/* out (nb x k, device float64, ld ldo) = K(A, B)' W with K as in ccz_pairwise_kernel and W (na x k, device float64,
 * ld ldw) -- K is never written: each 64 x 64 tile lives in registers between the two products.  Any k (64 columns
 * per pass).  Enqueue-only on the handle's stream.
 * cca_zoo/nonparametric/_kcca.py:119-148 (transform: pairwise_kernels(train, test).T @ weights), _kgcca.py:136-165 */
CCZ_API int ccz_kernel_project(ccz_handle h, int dtype, const void* A_dev, int64_t na, int64_t lda, const double* meanA_dev,
                               const void* B_dev, int64_t nb, int64_t ldb, const double* meanB_dev, int64_t d, int kind,
                               double gamma, double degree, double coef0, const double* W_dev, int64_t k, int64_t ldw,
                               double* out_dev, int64_t ldo);

/* KCCA on n_views >= 2 training kernel matrices K_dev[i] (n x n, ld n, device float64, symmetric; DESTROYED: each
 * is overwritten by its eigenvectors).  Solves the reference's  A v = lambda B v,  v'Bv = 1  with
 *   A = (cov(hstack K) - blockdiag cov(K_i)) / M,   B = (blockdiag(c_i K_i + (1 - c_i) K_i^2) + shift I) / M,
 *   shift = max(0, eps - lambda_min(blockdiag)),
 * through one eigendecomposition K_i = U diag(l) U' per view (B_i is a polynomial in K_i): two views take the top-k
 * SVD of  D_1^-1/2 U_1' Kc_1' Kc_2 U_2 D_2^-1/2 / (n - 1)  (Kc: column-centred), more views a dense EVD of the
 * whitened (M n)-sized A.  weights_dev: n_views consecutive n x k_out blocks (row-major, device float64); vals_host:
 * k_out eigenvalues (descending).  k <= n.  Ordered with the host on return.
 * cca_zoo/nonparametric/_kcca.py:82-117 (fit), :214 (_build_A / _build_B), cca_zoo/_utils/_linalg.py:gevp */
CCZ_API int ccz_kcca_solve(ccz_handle h, double* const* K_dev, int n_views, int64_t n, const double* c, double eps, int k,
                           double* weights_dev, double* vals_host, int* k_out);

/* KGCCA on n_views >= 1 kernel matrices (as in ccz_kcca_solve, destroyed):
 *   Q = sum_i mu_i K_i B_i^-1 K_i,  B_i = c_i K_i + (1 - c_i) K_i^2 + shift_i I,  shift_i = max(0, eps - lambda_min(B_i)),
 * T = top-k eigenvectors of Q (view_weights mu_i >= 0: the top-k left singular vectors of [sqrt(mu_i) U_i diag(l / sqrt(b))]),
 * weights_i = pinv(K_i) T with NumPy's cutoff (|l| <= 1e-15 max|l| counts as zero).  Outputs as ccz_kcca_solve; vals_host:
 * the top-k eigenvalues of Q.
 * cca_zoo/nonparametric/_kgcca.py:80-134 (fit) */
CCZ_API int ccz_kgcca_solve(ccz_handle h, double* const* K_dev, int n_views, int64_t n, const double* c,
                            const double* view_weights, double eps, int k, double* weights_dev, double* vals_host, int* k_out);

/* ---- gradient models: CCA_EY / PLS_EY / MCCA_EY (csrc/ey.hip) ------------------------------------------------------
 * Mini-batch momentum SGD on the Eckart-Young objective, four launches per step, no host wait inside a chunk of steps.
 * A fit state (opaque, out-parameter) holds W (double-buffered), the velocity, the per-step scratch, the stop word and two
 * pinned index slots.  Views are ccz_view's of DEVICE rows (all CCZ_F32 or all CCZ_F64); means_dev[i] (device, the views'
 * dtype, or a NULL array / entry: no centring) is subtracted on load in the input precision.  W blocks: view i's p_i x k
 * row-major weights, views back to back (float64).  fp64 views: fp64 arithmetic throughout.  fp32 views: the two
 * products per step on the fp32 matrix pipe (centred fp32 rows times W or T rounded to fp32, fp32 within a stage of at
 * most 1024 features / 32 rows, fp64 across stages); W, velocity and all k x k algebra in fp64.  Measured per-step
 * relative error against float64 on the same rows (max abs error / max abs value): Z 3.5e-7, one update 3.6e-7.
 * cca_zoo/linear/gradient/_base.py:101-130, _cca_ey.py:134-225, _pls_ey.py:56-104, _mcca_ey.py:46-61,
 * cca_zoo/_utils/_ey.py:36-61 (C, V), :85-96 (B), :98-127 (PLS init), :129-185 (CCA init) */

/* Create a fit state: n_views (1..16) views of widths p[i] >= k, k in 1..128, batch_rows rows per step, up to
 * chunk_steps steps per ccz_ey_steps call; c, learning_rate, momentum and tol as in the reference. */
CCZ_API int ccz_ey_create(ccz_handle h, int dtype, int n_views, const int64_t* p, int64_t k, int64_t batch_rows,
                          int64_t chunk_steps, double c, double learning_rate, double momentum, double tol, void** state_out);

/* Free a fit state (synchronises the handle's stream).  NULL is a no-op. */
CCZ_API int ccz_ey_destroy(ccz_handle h, void* state);

/* Upload initial weights (host, float64, W blocks): velocity <- 0, B <- sum_i W_i'W_i / M, steps <- 0, objective <- inf. */
CCZ_API int ccz_ey_set_weights(ccz_handle h, void* state, const double* W_host);

/* Z (host, float64, n_views consecutive batch_rows x k blocks) = (X_i[idx] - mu_i) W_i with the weights of the last
 * ccz_ey_set_weights; idx_host: batch_rows row indices in [0, n_rows) (NULL: rows 0 .. batch_rows - 1, then n_rows must
 * equal batch_rows).  The initial projection z0 of CCA_EY (cca_zoo/_utils/_ey.py:177-184).  Ordered with the host on return. */
CCZ_API int ccz_ey_project(ccz_handle h, void* state, const ccz_view* views, const void* const* means_dev, int64_t n_rows,
                           const int64_t* idx_host, double* Z_host);

/* Enqueue n_steps (<= chunk_steps) steps.  idx_host: n_steps x batch_rows row indices (host; copied into a pinned slot
 * and uploaded asynchronously), NULL = full batch (identity; n_rows == batch_rows).  Returns without waiting for the
 * device; the only host wait is for the chunk that used the same slot two calls earlier, whose status is returned in
 * steps_known / stopped_known (-1 / 0 when there is none yet).  Steps after the stop are no-ops on the device. */
CCZ_API int ccz_ey_steps(ccz_handle h, void* state, const ccz_view* views, const void* const* means_dev, int64_t n_rows,
                         const int64_t* idx_host, int64_t n_steps, int64_t* steps_known, int* stopped_known);

/* Steps applied so far, whether the tol test stopped the fit, and the last objective.  Synchronises. */
CCZ_API int ccz_ey_status(ccz_handle h, void* state, int64_t* steps_done, int* stopped, double* last_objective);

/* Copy the current weights (W blocks, float64) to the host.  Synchronises. */
CCZ_API int ccz_ey_get_weights(ccz_handle h, void* state, double* W_host);

/* ---- ALS models with deflation: PLS_ALS / SCCA_PMD / ParkhomenkoCCA / SCCA_Span / SCCA_ADMM (csrc/als.hip) -------------
 * Whole Gauss-Seidel sweeps on the device, no host wait inside a chunk of sweeps.  For every view i of a sweep:
 * t = normalise(sum_{j != i} X_j w_j), raw = X_i' t, w_i = rule(raw); after the sweep delta = max_i |w_i - w_i_old|_2 and
 * the dimension ends when delta < tol or after max_iter sweeps.  The views are never copied or written: the deflated view
 * of dimension d is (I - Q_i Q_i') (X_i - mu_i) with Q_i the normalised scores of the earlier dimensions, applied to the
 * n-vectors of an update (DESIGN.md "ALS models").  Views are ccz_view's of DEVICE rows (all CCZ_F32 or all CCZ_F64);
 * means_dev as for ccz_ey_steps.  x - mu is rounded in the views' precision, everything after it is float64.
 * Rules: CCZ_ALS_NORMALISE raw / |raw|_2; CCZ_ALS_SOFT_FIXED soft(raw, rule_param[i]); CCZ_ALS_SOFT_L1 raw / |raw|_2 when
 * |raw|_1 <= rule_param[i], else soft(raw, level) at the level 50 halvings of [0, max |raw|] end on; CCZ_ALS_TOP_S entries
 * with |raw| >= the rule_param[i]-th largest magnitude (ties kept).  Results are normalised when their norm exceeds 1e-12.
 * cca_zoo/linear/_iterative.py:38-158, :166-223, :231-380, :631-722, :839-930, cca_zoo/_utils/_linalg.py:76-116 */
#define CCZ_ALS_NORMALISE 0
#define CCZ_ALS_SOFT_FIXED 1
#define CCZ_ALS_SOFT_L1 2
#define CCZ_ALS_TOP_S 3
/* SCCA_ADMM (cca_zoo/linear/_iterative.py:388-514), rule_param[i] = tau_i.  Its iteration is Jacobi in the scores: every
 * view's target comes from the vectors the iteration started with.  Per view: w' = w_i - (X_d'(X_d w_i - t_i) + mu eta_i) /
 * L_i, z_i = soft(w' + eta_i, tau_i / mu) over its norm when that exceeds 1, eta_i += w' - z_i, w_i = z_i, with
 * L_i = |X_d' X_d|_F / n + mu taken at the first iteration of each dimension from the Gram of the centred view on its
 * smaller side.  min(n_rows, p[i]) <= 16384 for every view; ccz_als_admm_setup must precede the first ccz_als_sweeps. */
#define CCZ_ALS_ADMM 4
/* SCCA_IPLS and ElasticCCA (cca_zoo/linear/_iterative.py:522-623, :730-831, :938-982): each update is the elastic-net
 * regression argmin_c 1/2 |X_d c - t|^2 + a_i |c|_1 + b_i/2 |c|^2 of the target on the deflated view, solved by blocked
 * cyclic coordinate descent on G_i = X_d' X_d (formed once on the p side, deflated in place) under scikit-learn's stop rule
 * (coordinate change, then duality gap < tol t't; at most 1000 CD sweeps).  rule_param is ignored.  p[i] <= 16384 for every
 * view; ccz_als_enet_setup must precede ccz_als_set_init of every fit.  What ccz_als_sweeps enqueues for this rule is not a
 * sweep but a UNIT, a fixed kernel sequence that advances the sweep as far as up to 16 CD sweeps per view take it (csrc/als.hip);
 * a sweep needs one unit or more, so the caller enqueues units until the stop is reported. */
#define CCZ_ALS_ENET 5

/* Create a fit state: n_views (1..8) views of widths p[i] and n_rows rows, k (1..32) latent dimensions, the rule and its
 * per-view parameter (NULL for CCZ_ALS_NORMALISE), tol and max_iter per dimension as in the reference
 * (cca_zoo/linear/_iterative.py:52-63), up to chunk_sweeps sweeps per ccz_als_sweeps call. */
CCZ_API int ccz_als_create(ccz_handle h, int dtype, int n_views, const int64_t* p, int64_t n_rows, int64_t k, int rule,
                           const double* rule_param, double tol, int64_t max_iter, int64_t chunk_sweeps, void** state_out);

/* Free a fit state (synchronises the handle's stream).  NULL is a no-op. */
CCZ_API int ccz_als_destroy(ccz_handle h, void* state);

/* Upload the initial vectors of all dimensions (host, float64, k x sum p: dimension d's vectors of all views back to
 * back) and reset the fit (cca_zoo/linear/_iterative.py:80-89: the draws do not depend on results). */
CCZ_API int ccz_als_set_init(ccz_handle h, void* state, const double* w0_host);

/* CCZ_ALS_ADMM only: set the penalty mu (> 0) and form, for every view, the float64 Gram of fl(X_i - mu_i) on its smaller
 * side ((X - mu)(X - mu)' when n_rows <= p[i], else (X - mu)'(X - mu)) in the state.  views / means_dev as for
 * ccz_als_sweeps, and the same rows must be passed there.  Asynchronous on the handle's stream. */
CCZ_API int ccz_als_admm_setup(ccz_handle h, void* state, const ccz_view* views, const void* const* means_dev, double mu);

/* CCZ_ALS_ENET only.  Per view: a[i] = n alpha l1_ratio, b[i] = n alpha (1 - l1_ratio); ridge[i] != 0 (the reference's
 * Ridge, l1_ratio = 0): a[i] = 0, b[i] = alpha, and the solve stops on the coordinate change alone.  target_all: the target
 * is the normalised sum of EVERY view's score (ElasticCCA), else of the other views' (SCCA_IPLS).  post_std: w_i is the
 * coefficient vector over the population standard deviation of its score when that exceeds 1e-12 (SCCA_IPLS), else the
 * coefficient vector (ElasticCCA).  Forms G_i = fl(X_i - mu_i)' fl(X_i - mu_i) in float64 for every view.  The fit deflates
 * G_i, so every fit needs its own setup.  Asynchronous on the handle's stream. */
CCZ_API int ccz_als_enet_setup(ccz_handle h, void* state, const ccz_view* views, const void* const* means_dev, const double* a,
                               const double* b, const int* ridge, int target_all, int post_std);

/* CCZ_ALS_ENET only, after the setup: one solve of view `view` outside a fit, for tests of the kernels.  G_host (p x p
 * row-major symmetric float64; NULL keeps the view's G), q_host and the starting coefficients c0_host (p each), tt = t't.
 * Enqueues r = q - G c0 and n_sweeps (<= 1000) CD sweeps under the stop rule of the state's tol; read the result with
 * ccz_als_peek.  A fit on the state must begin again with ccz_als_enet_setup and ccz_als_set_init. */
CCZ_API int ccz_als_enet_solve(ccz_handle h, void* state, int view, const double* G_host, const double* q_host,
                               const double* c0_host, double tt, int64_t n_sweeps);

/* CCZ_ALS_ENET only: CD sweeps taken per dimension (k entries) and the number of solves that ended on the cap of 1000
 * sweeps without meeting the stop rule.  Synchronises. */
CCZ_API int ccz_als_enet_status(ccz_handle h, void* state, int64_t* cd_sweeps_per_dim, int64_t* capped);

/* Enqueue n_sweeps (<= chunk_sweeps) sweeps (cca_zoo/linear/_iterative.py:86-117).  Returns without waiting for the
 * device; the only host wait is for the chunk that used the same status slot two calls earlier, whose state is returned
 * in sweeps_known / stopped_known (-1 / 0 when there is none yet).  Sweeps after the last dimension are no-ops. */
CCZ_API int ccz_als_sweeps(ccz_handle h, void* state, const ccz_view* views, const void* const* means_dev, int64_t n_sweeps,
                           int64_t* sweeps_known, int* stopped_known);

/* Dimensions finished, whether the fit is complete, and per dimension (k entries each) the sweeps taken and the delta
 * of the last sweep.  Synchronises. */
CCZ_API int ccz_als_status(ccz_handle h, void* state, int* dims_done, int* stopped, int64_t* sweeps_per_dim,
                           double* last_delta);

/* mean_dev (device, the view's dtype, cols entries) = the column means of one view of DEVICE rows exactly as NumPy's
 * v.mean(axis=0) forms them: the rows added in order in the view's own precision, then divided by n_rows
 * (cca_zoo/_base.py:97-99).  A tree-ordered float32 mean differs from it by up to ~1e-6 relative, which would move the
 * centred rows and with them the trajectory.  Asynchronous on the handle's stream. */
CCZ_API int ccz_als_colmeans(ccz_handle h, int dtype, const ccz_view* view, int64_t n_rows, void* mean_dev);

/* ---- sparse views of the four plain rules (CCZ_ALS_NORMALISE .. CCZ_ALS_TOP_S) ------------------------------------------
 * A sparse view lives on the device in BOTH compressed forms, because the two passes of an update want opposite
 * orientations and a scatter would need floating-point atomics: CSR for the score X w, CSC for X' t and the means.  Each form
 * holds the values in the fit's dtype (CCZ_F32 / CCZ_F64), int32 minor indices and int64 pointers (rows + 1 / cols + 1
 * entries).  Both must be CANONICAL: indices sorted within a line, no duplicates.  The indices are trusted: the caller checks
 * them before the upload (the Python side runs scipy's full format check); an out-of-range index is an out-of-range read.
 * A form that a call does not read may be left NULL; with nnz = 0 the value and index arrays may be NULL.
 *
 * Semantics.  A sparse view is never densified and never rewritten.  Centring is implicit:
 *   (X - 1 mu') w = X w - (mu' w) 1        (X - 1 mu')' t = X' t - mu (1' t)
 * so no x - mu element is formed and there is NO fl32(x - mu) rounding on this path (the stated difference from dense
 * float32 views): a stored value is widened exactly on load, every product and sum is float64, and a CCZ_F32 and a CCZ_F64
 * sparse view holding the same numbers give the same bits.  The means of a sparse view are float64,
 * mu_j = (sum_i x_ij) / n_rows over the stored entries of column j.  A line (a row of the CSR form, a column of the CSC
 * form) is summed by a group of G lanes, G = ccz_sparse_group(nnz, lines): lane l takes entries l, l + G, ... in order and
 * the lanes combine by a fixed butterfly; mu' w and 1' t are summed in a fixed order too.  No floating-point atomics: two
 * fits give the same bits whatever the chunk length.  The comparator of a sparse fit is the dense float64 fit of the same
 * numbers. */
typedef struct ccz_sparse_view {
  const void* csr_val;    /* nnz values, the row-major order of the entries   */
  const int32_t* csr_col; /* nnz column indices                                */
  const int64_t* csr_ptr; /* rows + 1                                          */
  const void* csc_val;    /* nnz values, the column-major order of the entries */
  const int32_t* csc_row; /* nnz row indices                                   */
  const int64_t* csc_ptr; /* cols + 1                                          */
  int64_t rows, cols, nnz; /* each below 2^31                                  */
} ccz_sparse_view;

/* The lanes per line for `lines` lines holding nnz stored entries in all: the smallest power of two that is not below
 * nnz / lines, within [4, 64].  A function of the matrix alone.  Host only; CCZ_EINVAL for nnz < 0 or lines < 1. */
CCZ_API int ccz_sparse_group(int64_t nnz, int64_t lines);

/* Mark view `view` of a fit state as sparse (device arrays, both forms; they must outlive the fit), or as dense again with
 * sparse = NULL.  rows / cols must be the state's n_rows / p[view].  CCZ_EUNSUP for CCZ_ALS_ADMM and CCZ_ALS_ENET, which
 * need the Gram of a view.  Afterwards ccz_als_sweeps ignores views[view].data and .ld (cols must still match) and reads
 * means_dev[view] as FLOAT64 whatever the fit's dtype; the other views keep their arithmetic bit for bit. */
CCZ_API int ccz_als_set_sparse(ccz_handle h, void* state, int view, const ccz_sparse_view* sparse);

/* mean_dev (device, float64, cols entries) = the column means of a sparse view from its CSC form.  Asynchronous on the
 * handle's stream. */
CCZ_API int ccz_sparse_colmeans(ccz_handle h, int dtype, const ccz_sparse_view* view, double* mean_dev);

/* out_dev (device, rows x k row-major float64) = X W - 1 (mu' W) from the CSR form: W_dev cols x k row-major float64,
 * k <= 32, mean_dev float64 or NULL for no centring.  Asynchronous on the handle's stream. */
CCZ_API int ccz_sparse_project(ccz_handle h, int dtype, const ccz_sparse_view* view, const double* mean_dev, const double* W_dev,
                               int k, double* out_dev);

/* Copy one working buffer of view `view` to the host (float64) -- what the kernel tests compare with NumPy one kernel at
 * a time: the current vector w_i (p_i), raw_i = X_d' t of its last update (p_i), its uncorrected score (X_i - mu_i) w_i
 * (n_rows), the corrected target t~ of the LAST update of any view (n_rows), Q_i (k x n_rows, column a at a n_rows:
 * the normalised scores of the finished dimensions, cca_zoo/_utils/_linalg.py:108-116), the level of its last update (2:
 * the level the bisection of cca_zoo/linear/_iterative.py:245-254 ended on or the s-th largest magnitude of :717, then
 * 1.0 when that level was applied and 0.0 when the rule has no level or |raw|_1 was within the bound).  Synchronises. */
#define CCZ_ALS_PEEK_W 0
#define CCZ_ALS_PEEK_RAW 1
#define CCZ_ALS_PEEK_SCORE 2
#define CCZ_ALS_PEEK_TARGET 3
#define CCZ_ALS_PEEK_Q 4
#define CCZ_ALS_PEEK_LEVEL 5
/* CCZ_ALS_ADMM: RAW holds w' of the view's last update and TARGET the n-vector (s_i - t_i) - Q_i Q_i' (s_i - t_i) of the
 * last view updated; Z is z_i (p_i; it coincides with w_i between iterations), ETA the scaled dual eta_i (p_i), LIPSCHITZ
 * L_i of the current dimension (1 number). */
#define CCZ_ALS_PEEK_Z 6
#define CCZ_ALS_PEEK_ETA 7
#define CCZ_ALS_PEEK_LIPSCHITZ 8
/* CCZ_ALS_ENET: RAW holds q = X_d' t of the view's last solve; GRAM is G_i (p_i x p_i, deflated by the finished dimensions),
 * RESIDUAL r = q - G c of the LAST solve of any view (p_i), COEF the view's coefficients (p_i), ENET four numbers: t't, the
 * last duality gap computed, the score's standard deviation, the CD sweeps of the view's last solve. */
#define CCZ_ALS_PEEK_GRAM 9
#define CCZ_ALS_PEEK_RESIDUAL 10
#define CCZ_ALS_PEEK_COEF 11
#define CCZ_ALS_PEEK_ENET 12
CCZ_API int ccz_als_peek(ccz_handle h, void* state, int what, int view, double* out_host);

/* Copy the finished columns (W blocks as in ccz_ey_get_weights: view i's p_i x k row-major float64 weights, views back
 * to back; unfinished columns are zero) to the host (cca_zoo/linear/_iterative.py:91-92).  Synchronises. */
CCZ_API int ccz_als_get_weights(ccz_handle h, void* state, double* W_host);

/* ---- GFA: group factor analysis, Bayesian CCA with per-view ARD (csrc/gfa.hip) -----------------------------------------
 * Whole coordinate-ascent iterations of mean-field variational Bayes on the device, no host wait inside a chunk of
 * iterations.  One iteration, in the reference's order: per view cov_w, w = (X'z) cov_w tau, ww = w'w + p cov_w; cov_z =
 * inv(I + sum tau ww); z = (sum tau X w) cov_z, zz = z'z + n cov_z; alpha, tau; columns whose mean z^2 is at most 1e-7 are
 * dropped (drop_k, when some but not all are kept; the kept ones stay in order); the fit stops after 1000 consecutive
 * iterations without a prune whose relative change of z stayed below tol, or after max_iter.  Views, means_dev, rounding
 * (x - mu in the views' precision, everything after it float64) as for ccz_als_sweeps.  k x k results are packed to the
 * ACTIVE k (k_active of ccz_gfa_status), row-major.
 * cca_zoo/probabilistic/_gfa.py:184-204 (initialisation), :217-286 (iteration) */

/* Create a fit state: n_views (1..8) views of widths p[i] and n_rows (>= 2) rows, k (1..32) latent dimensions at the start,
 * up to chunk_iters iterations per ccz_gfa_iterations call. */
CCZ_API int ccz_gfa_create(ccz_handle h, int dtype, int n_views, const int64_t* p, int64_t n_rows, int64_t k, double tol,
                           int64_t max_iter, int drop_k, int64_t chunk_iters, void** state_out);

/* Free a fit state (synchronises the handle's stream).  NULL is a no-op. */
CCZ_API int ccz_gfa_destroy(ccz_handle h, void* state);

/* Upload the initial z (host, float64, n_rows x k row-major: default_rng(random_state).standard_normal((n, k)),
 * cca_zoo/probabilistic/_gfa.py:184).  Must precede every ccz_gfa_setup. */
CCZ_API int ccz_gfa_set_init(ccz_handle h, void* state, const double* z0_host);

/* One pass per view: y_const = sum fl(x - mu)^2 and datavar = the sum of the ddof = 1 column variances of fl(x - mu)
 * (re-centred by the float64 column mean, as np.var does), then the initial alpha, tau = 1e3, cov_z = cov_w = I, w = 0, ww,
 * zz, and the status word.  Asynchronous on the handle's stream; the same rows must be passed to ccz_gfa_iterations. */
CCZ_API int ccz_gfa_setup(ccz_handle h, void* state, const ccz_view* views, const void* const* means_dev);

/* Enqueue n_iters (<= chunk_iters) iterations.  Returns without waiting for the device; the only host wait is for the
 * chunk that used the same status slot two calls earlier, whose state is returned in iters_known / stopped_known (-1 / 0
 * when there is none yet).  Iterations after the stop are no-ops. */
CCZ_API int ccz_gfa_iterations(ccz_handle h, void* state, const ccz_view* views, const void* const* means_dev, int64_t n_iters,
                               int64_t* iters_known, int* stopped_known);

/* Iterations done, whether the fit has stopped, the active k, the stable counter, the last relative change of z, and the
 * prunes so far: their number and, per prune (k entries suffice), the 1-based iteration and the active k after it.
 * Synchronises. */
CCZ_API int ccz_gfa_status(ccz_handle h, void* state, int64_t* iters, int* stopped, int* k_active, int* stable, double* rel_change,
                           int* n_prunes, int64_t* prune_iters, int* prune_k);

/* Copy one quantity to the host (float64, packed to the active k) -- what the kernel tests compare with NumPy term by term:
 * z (n x k), view's w (p x k), XW = (X - mu) w (n x k), cov_z, view's cov_w, ww, zz (k x k), view's alpha, b_ard (k), tau,
 * b_tau (n_views each), SETUP: view's y_const and datavar (2).  Synchronises. */
#define CCZ_GFA_PEEK_Z 0
#define CCZ_GFA_PEEK_W 1
#define CCZ_GFA_PEEK_XW 2
#define CCZ_GFA_PEEK_COV_Z 3
#define CCZ_GFA_PEEK_COV_W 4
#define CCZ_GFA_PEEK_WW 5
#define CCZ_GFA_PEEK_ZZ 6
#define CCZ_GFA_PEEK_ALPHA 7
#define CCZ_GFA_PEEK_TAU 8
#define CCZ_GFA_PEEK_B_TAU 9
#define CCZ_GFA_PEEK_B_ARD 10
#define CCZ_GFA_PEEK_SETUP 11
CCZ_API int ccz_gfa_peek(ccz_handle h, void* state, int what, int view, double* out_host);

/* Everything the posterior draws need (cca_zoo/probabilistic/_gfa.py:301-352), packed to the active k written to
 * *k_active: z (n x k), cov_z (k x k), w of all views back to back (sum p x k), cov_w (n_views x k x k), alpha and b_ard
 * (n_views x k), tau and b_tau (n_views).  Size the outputs for the k of ccz_gfa_status or of ccz_gfa_create; NULL outputs
 * are skipped.  Synchronises. */
CCZ_API int ccz_gfa_get_result(ccz_handle h, void* state, int* k_active, double* z_host, double* cov_z_host, double* w_host,
                               double* cov_w_host, double* alpha_host, double* b_ard_host, double* tau_host, double* b_tau_host);

/* *sumsq_host = sum over all entries of fl(x - mean)^2 of one view of DEVICE rows, in float64 (mean_dev: the view's dtype,
 * NULL for none): the setup pass alone, for the marginal log-likelihood (cca_zoo/probabilistic/_utils.py:102-103 with a
 * noise variance that is constant within a view).  Synchronises. */
CCZ_API int ccz_gfa_sumsq(ccz_handle h, int dtype, const ccz_view* view, int64_t n_rows, const void* mean_dev, double* sumsq_host);

/* ---- VariationalBayesCCA: mean-field stochastic variational inference (csrc/svi.hip) --------------------------------------
 * Whole SVI steps on the device, no host wait inside a chunk of steps.  The model is that of
 * cca_zoo/probabilistic/_vbcca.py:108-159; the reference fits it with numpyro (AutoNormal, Trace_ELBO, Adam), which this
 * library cannot call, so the algorithm is written out here and restated in NumPy in tests/vbcca_restatement.py.  These are
 * NOT numpyro's bits: its PRNG differs.
 *
 * Model, in unconstrained sites, a0 = b0 = 1e-3, K latent dimensions, M views of p_i columns, n rows, P = sum p_i:
 *   a = log alpha (K)       alpha_k ~ Gamma(a0, b0) (rate b0), Jacobian + a_k
 *   W_i (p_i x K)           W_i[j, k] ~ N(0, 1 / alpha_k)
 *   s_i = log psi_i (p_i)   s_i[j] ~ N(0, 1)
 *   Z (n x K)               Z[r, k] ~ N(0, 1)
 *   x_i[r, j] ~ N((Z W_i')[r, j], exp(s_i[j])): exp(s) is the STANDARD DEVIATION of the likelihood, as in the reference.
 * Guide: every element an independent normal, loc and scale = softplus(rho); scale starts at 0.1, loc is uploaded.
 * The flat parameter vector of N = K + P K + P + n K doubles is [ a | W_0 .. W_{M-1} (row-major, back to back) |
 * s_0 .. s_{M-1} | Z (row-major) ]; loc, rho, the Adam moments, theta, eps and the gradient all use it.
 * Sites are numbered 0: a, 1 + 2 i: W_i, 2 + 2 i: s_i, 1 + 2 M: Z.  With splitmix64 of csrc/rng_hash.h and 64-bit wrap-around,
 *   stream(seed, t, site) = splitmix64(splitmix64(splitmix64(seed) + t) + site)
 * Step t = 0, 1, ..:
 *   eps[e] = hash_normal(stream(seed, t, site of e), row-major index of e within its site); theta = loc + scale eps
 *   R_i = fl(X_i - mu_i) - Z W_i' (x - mu rounded in the views' dtype, everything after it float64), D_i = R_i o exp(-2 s_i)
 *   loss_t = -(log p(x, theta) + sum_k a_k - log q(theta)), every normalising constant included
 *   d W_i = D_i' Z - alpha o W_i;  d Z = sum_i D_i W_i - Z;  d s_i[j] = sum_r R_i[r, j]^2 exp(-2 s_i[j]) - n - s_i[j]
 *   d a_k = a0 - b0 alpha_k + P / 2 - alpha_k / 2 sum_{i, j} W_i[j, k]^2
 *   d loc = d theta;  d rho = (d theta eps + 1 / scale) sigmoid(rho)
 *   Adam on the loss (gradient -d): b1 = 0.9, b2 = 0.999, eps = 1e-8, m^ = m / (1 - b1^(t+1)), v^ = v / (1 - b2^(t+1)),
 *   x -= lr m^ / (sqrt(v^) + eps)
 * A step whose loss is not finite stops the fit (the parameters have taken that step); later steps are no-ops.
 * No floating-point atomics: two fits give the same bits, whatever the chunk length. */

/* Create a fit state: n_views (2..8) views of widths p[i] >= 1, n_rows (>= 2) rows, k (1..32) latent dimensions, num_steps steps
 * in all, up to chunk_steps per ccz_svi_steps call.  Refusals come before any device work. */
CCZ_API int ccz_svi_create(ccz_handle h, int dtype, int n_views, const int64_t* p, int64_t n_rows, int64_t k, int64_t num_steps,
                           double learning_rate, uint64_t seed, int64_t chunk_steps, void** state_out);

/* Free a fit state (synchronises the handle's stream).  NULL is a no-op. */
CCZ_API int ccz_svi_destroy(ccz_handle h, void* state);

/* Upload the initial loc (host, float64, N entries in the flat layout) and reset rho, the moments, the losses and the status:
 * starts a new fit on the state. */
CCZ_API int ccz_svi_set_init(ccz_handle h, void* state, const double* loc_host);

/* Enqueue n_steps (<= chunk_steps) steps.  Returns without waiting for the device; the only host wait is for the chunk that
 * used the same status slot two calls earlier, whose state is returned in steps_known / stopped_known (-1 / 0 when there is
 * none yet).  Views and means_dev (NULL, or NULL entries, for no centring) as for ccz_gfa_iterations. */
CCZ_API int ccz_svi_steps(ccz_handle h, void* state, const ccz_view* views, const void* const* means_dev, int64_t n_steps,
                          int64_t* steps_known, int* stopped_known);

/* Steps done, whether the fit has stopped (all steps done, or a non-finite loss), and the step of the non-finite loss (-1 when
 * there was none).  Synchronises. */
CCZ_API int ccz_svi_status(ccz_handle h, void* state, int64_t* steps, int* stopped, int64_t* bad_step);

/* Copy one buffer to the host (float64) -- what the kernel tests compare with NumPy term by term.  LOC .. GRAD hold N entries
 * in the flat layout (THETA, EPS and GRAD = d theta are those of the last step), LOSS num_steps, PLAN the planned launch of the
 * fused kernel: row chunks, rows per chunk, strips in all, then the strips of every view.  Synchronises. */
#define CCZ_SVI_PEEK_LOC 0
#define CCZ_SVI_PEEK_RHO 1
#define CCZ_SVI_PEEK_M_LOC 2
#define CCZ_SVI_PEEK_V_LOC 3
#define CCZ_SVI_PEEK_M_RHO 4
#define CCZ_SVI_PEEK_V_RHO 5
#define CCZ_SVI_PEEK_THETA 6
#define CCZ_SVI_PEEK_EPS 7
#define CCZ_SVI_PEEK_GRAD 8
#define CCZ_SVI_PEEK_LOSS 9
#define CCZ_SVI_PEEK_PLAN 10
CCZ_API int ccz_svi_peek(ccz_handle h, void* state, int what, double* out_host);

/* loc and rho (N each, flat layout) and the losses (num_steps; zero for steps not taken).  NULL outputs are skipped.
 * Synchronises. */
CCZ_API int ccz_svi_get_result(ccz_handle h, void* state, double* loc_host, double* rho_host, double* losses_host);

/* *out_host = sum_j weights_host[j] sum_rows fl(x - mean)[row, j]^2 of one view of DEVICE rows, in float64 (mean_dev: the
 * view's dtype, NULL for none): x' Psi^-1 x of the marginal log-likelihood with one noise variance per feature
 * (cca_zoo/probabilistic/_utils.py:102-103).  Synchronises. */
CCZ_API int ccz_colsumsq_weighted(ccz_handle h, int dtype, const ccz_view* view, int64_t n_rows, const void* mean_dev,
                                  const double* weights_host, double* out_host);

/* ---- ProbabilisticCCA: the No-U-Turn sampler (csrc/nuts.hip) ------------------------------------------------------------------
 * Whole leapfrog steps on the device; the tree and the adaptation scalars on the host, which reads one small record per
 * leapfrog (the tree is data-dependent).  The model is that of cca_zoo/probabilistic/_pcca.py:90-131; the reference samples it
 * with numpyro (NUTS, MCMC with their defaults), which this library cannot call, so the sampler is written out here and
 * restated in NumPy in tests/pcca_restatement.py, which is the specification.  These are NOT numpyro's bits: the random
 * numbers are this library's.
 *
 * Model (VariationalBayesCCA's without the ARD site), K latent dimensions, M views of p_i columns, n rows, P = sum p_i:
 *   W_i[j, k] ~ N(0, 1);  s_i = log psi_i, s_i[j] ~ N(0, 1);  Z[r, k] ~ N(0, 1)
 *   x_i[r, j] ~ N((Z W_i')[r, j], exp(s_i[j])): exp(s) is the STANDARD DEVIATION of the likelihood, as in the reference.
 * State: one flat vector of N = P K + P + n K doubles, q = [ W_0 .. W_{M-1} (row-major, back to back) | s_0 .. s_{M-1} |
 * Z (row-major) ]; the momentum p, the gradient g, minv and the Welford vectors all use it.
 * Potential, every normalising constant included, with R_i = fl(X_i - mu_i) - Z W_i' (x - mu rounded in the views' dtype,
 * everything after it float64) and D_i = R_i o exp(-2 s_i):
 *   U = |W|^2 / 2 + |s|^2 / 2 + |Z|^2 / 2 + sum_ij (n s_ij + exp(-2 s_ij) sum_r R_rj^2 / 2) + log(2 pi) (N + n P) / 2
 *   dU/dW_i = W_i - D_i' Z;  dU/dZ = Z - sum_i D_i W_i;  dU/ds_ij = s_ij + n - exp(-2 s_ij) sum_r R_rj^2
 * Leapfrog with the diagonal inverse mass minv (initially 1) and the step eps (negative: backwards in time):
 *   p -= (eps / 2) g;  q += eps minv o p;  g = dU(q);  p -= (eps / 2) g;  kinetic energy sum minv p^2 / 2
 * Sites are numbered 2 i: W_i, 2 i + 1: s_i, 2 M: Z, and 2 M + 1 is the tree's stream.  With splitmix64 / hash_normal of
 * csrc/rng_hash.h, stream(seed, t, site) = splitmix64(splitmix64(splitmix64(seed) + t) + site) as for ccz_svi_*:
 *   p[e] = hash_normal(stream(seed, t, site of e), row-major index of e within its site) / sqrt(minv[e])
 *   u_j = (splitmix64(stream(seed, t, 2 M + 1) ^ splitmix64(j)) >> 11) 2^-53, used in order: the direction coin of a doubling
 *   (u < 1/2: forwards), the selections of its leaves 1 .., the tree's selection
 * Transition t: multinomial NUTS, built iteratively.  H0 = U + kinetic at the start.  A doubling at depth d adds 2^d leaves at
 * one end; leaf i: one leapfrog; dH = H - H0 (NaN is +inf); statistic min(1, exp(-dH)); dH > 1000 is a divergence and ends the
 * transition; the subtree's proposal is leaf 0, then leaf i with probability w_i / (w_before + w_i), w = exp(-dH); rsum += p;
 * an even leaf is checkpoint c = popcount(i >> 1), keeping (p, rsum); an odd leaf closes one subtree per trailing one-bit of i
 * (checkpoints c, c - 1, ..): rho = rsum - rsum_c + p_c, rho~ = rho - (p_c + p) / 2, turning when (minv o p_c) . rho~ <= 0 or
 * (minv o p) . rho~ <= 0, which ends the transition.  A whole subtree: the tree takes its proposal with probability
 * min(1, w_sub / w_tree), w_tree += w_sub, rho_tree += rsum, and the whole tree is tested the same way with its two ends'
 * momenta; up to max_tree_depth doublings.  accept_prob is the mean statistic of all leaves.
 * Warm-up: dual averaging of log eps (t0 = 10, kappa = 0.75, gamma = 0.05, mu = log(10 eps), eps_0 = 1, no step-size
 * heuristic); Stan's windows as numpyro builds them (below 20 transitions one window; else 75 / 50 / 25 doubling, or
 * 15 % / 10 % / the rest); in the MIDDLE windows a Welford mean / M2 of q, and at such a window's end (count c)
 * minv = (c / (c + 5)) M2 / (c - 1) + 1e-3 (5 / (c + 5)), the Welford state reset, dual averaging restarted at
 * mu = log(10 eps); after the last warm-up transition eps = exp(averaged log eps).
 * No floating-point atomics: two fits give the same bits.  A leapfrog is M + 3 launches.
 * Limits: 2..8 views, k 1..32, n_rows >= 2, max_tree_depth 1..10, and the 15 + 2 max_tree_depth slots of N doubles may not
 * exceed 2^33 doubles (64 GiB): CCZ_EUNSUP before any device work. */

/* Create a fit state.  Refusals come before any device work. */
CCZ_API int ccz_nuts_create(ccz_handle h, int dtype, int n_views, const int64_t* p, int64_t n_rows, int64_t k, int64_t num_warmup,
                            int64_t num_samples, int max_tree_depth, double target_accept_prob, uint64_t seed, void** state_out);

/* Free a fit state (synchronises the handle's stream).  NULL is a no-op. */
CCZ_API int ccz_nuts_destroy(ccz_handle h, void* state);

/* Upload the initial point q (host, float64, N entries), evaluate U and g there and reset the chain (eps = 1, minv = 1, no
 * transitions done).  *potential_out = U; when U is not finite the fit is stopped (every kernel becomes a no-op,
 * ccz_nuts_run refuses) and *potential_out is NaN.  Views and means_dev as for ccz_svi_steps.  Synchronises. */
CCZ_API int ccz_nuts_set_init(ccz_handle h, void* state, const ccz_view* views, const void* const* means_dev, const double* q_host,
                              double* potential_out);

/* Test seam: set eps (dual averaging restarts from it) and, unless NULL, minv (host, N entries). */
CCZ_API int ccz_nuts_set_adapt(ccz_handle h, void* state, double step_size, const double* minv_host);

/* Test seam: leaf `leaf` (0 .. 2^depth - 1) of a doubling at `depth` in `direction` (+1: the right end forwards, -1: the left
 * end backwards), as ccz_nuts_run would take it; with `begin` the momentum of `transition` is drawn first (both ends = the
 * chain's point).  Every intermediate stays in its slot for ccz_nuts_peek.  record_host (27 doubles): U, kinetic, H, the
 * dots (2 l, 2 l + 1: the l-th closed subtree, smallest first; 20, 21: the whole tree), finite, the kinetic energy of the
 * drawn momentum (0 without `begin`).  Dots of tests the leaf does not close are 0.  Synchronises. */
CCZ_API int ccz_nuts_leapfrog(ccz_handle h, void* state, const ccz_view* views, const void* const* means_dev, int64_t transition,
                              int begin, int direction, int64_t leaf, int depth, double* record_host);

/* Run the next n_transitions (warm-up first, with its adaptation).  The q of kept draw d (transition num_warmup + d) is
 * written to draws_host + d N as its transition ends (NULL: not fetched).  Synchronises. */
CCZ_API int ccz_nuts_run(ccz_handle h, void* state, const ccz_view* views, const void* const* means_dev, int64_t n_transitions,
                         double* draws_host);

/* Transitions done, whether the fit has stopped (a non-finite initial potential: bad = 0, else -1).  Synchronises. */
CCZ_API int ccz_nuts_status(ccz_handle h, void* state, int64_t* transitions, int* stopped, int64_t* bad);

/* Copy one slot (N doubles) or one small table to the host -- what the kernel tests compare with NumPy term by term.
 * Slots: the tree's left / right end q, p, g; the chain's point q, g; the subtree's proposal q, g; the momentum sum of the
 * tree and of the subtree; minv; the Welford mean and M2; checkpoint c at CKPT + 2 c (p) and CKPT + 2 c + 1 (sum).
 * PLAN: row chunks, rows per chunk, strips in all, workgroups of the passes over N, slots, then the strips of every view.
 * RECORD: the last record (26 doubles, as ccz_nuts_leapfrog).  SCALARS: U of the chain's point, eps, the Welford count, the
 * window index.  PLAN is known from ccz_nuts_create on; the rest needs ccz_nuts_set_init.  Synchronises. */
#define CCZ_NUTS_PEEK_LEFT_Q 0
#define CCZ_NUTS_PEEK_LEFT_P 1
#define CCZ_NUTS_PEEK_LEFT_G 2
#define CCZ_NUTS_PEEK_RIGHT_Q 3
#define CCZ_NUTS_PEEK_RIGHT_P 4
#define CCZ_NUTS_PEEK_RIGHT_G 5
#define CCZ_NUTS_PEEK_Q 6
#define CCZ_NUTS_PEEK_G 7
#define CCZ_NUTS_PEEK_SUB_Q 8
#define CCZ_NUTS_PEEK_SUB_G 9
#define CCZ_NUTS_PEEK_RHO 10
#define CCZ_NUTS_PEEK_RSUM 11
#define CCZ_NUTS_PEEK_MINV 12
#define CCZ_NUTS_PEEK_WELFORD_MEAN 13
#define CCZ_NUTS_PEEK_WELFORD_M2 14
#define CCZ_NUTS_PEEK_CKPT 15
#define CCZ_NUTS_PEEK_PLAN 100
#define CCZ_NUTS_PEEK_RECORD 101
#define CCZ_NUTS_PEEK_SCALARS 102
CCZ_API int ccz_nuts_peek(ccz_handle h, void* state, int what, double* out_host);

/* Per transition done so far (T of them, warm-up included), six arrays of T doubles back to back: tree_depth, n_leapfrog,
 * accept_prob, diverging, potential_energy, step_size (the one the transition used); the current step size; minv (N).
 * NULL outputs are skipped.  Synchronises. */
CCZ_API int ccz_nuts_get_stats(ccz_handle h, void* state, double* stats_host, double* step_size, double* minv_host);

/* ---- Khatri-Rao moment and its adjoint (tensor CCA) -------------------------------------------------------------------
 * Views are float64 DEVICE matrices H_i (n x d_i), 2..8 of them, prod d_i <= 2^24.  Tensors are row-major, the last view's
 * index fastest.  Both run on the handle's stream without a host wait and use no floating-point atomics: two calls give the
 * same bits.  CCZ_EINVAL: n_views outside 2..8, prod d_i > 2^24, mode out of range, a bad view. */

/* M[r_1 .. r_V] = scale * sum_s prod_i H_i[s, r_i]: the cross-moment tensor, as the product (H_1 (.) .. (.) H_{V-1})' H_V
 * whose Khatri-Rao operand is formed in registers.  Replaces the n x d_1 x .. x d_V outer-product tensor and its mean over
 * the batch: cca_zoo/deep/objectives.py:279-288, cca_zoo/linear/_tcca.py:99-109 */
CCZ_API int ccz_kr_moment(ccz_handle h, const ccz_view* H_dev, int n_views, int64_t n, double scale, double* M_dev);

/* out[s, a] = scale * sum_{r : r_mode = a} T[r] * prod_{i != mode} H_i[s, r_i]   (n x d_mode, row stride ldo): the adjoint of
 * ccz_kr_moment with respect to view `mode` -- what autograd computes through the broadcast products of
 * cca_zoo/deep/objectives.py:280-288 by keeping the n x prod d tensor alive. */
CCZ_API int ccz_kr_apply(ccz_handle h, const ccz_view* H_dev, int n_views, int64_t n, const double* T_dev, int mode, double scale,
                         double* out_dev, int64_t ldo);

/* ---- CP-ALS of a dense float64 tensor (csrc/cp_als.hip): the factor step of TCCA / KTCCA ------------------------------------
 * The tensor M lies in DEVICE memory in ccz_kr_moment's layout (row-major, the last mode's index fastest): order V = 2..8,
 * prod d_i <= 2^24, rank k = 1..32, k <= min d_i.  The algorithm is tensorly's documented parafac with the defaults the
 * reference calls it with (init="svd", n_iter_max=100, tol=1e-8, no normalisation, stop on the absolute change of the
 * reconstruction error), written out:
 *   unfold(T, m) = moveaxis(T, m, 0).reshape(d_m, -1)
 *   init: A_m = the k leading left singular vectors of unfold(M, m), every column's entry of largest magnitude positive
 *   iteration t, for m = 0 .. V-1 in turn: P = Hadamard product over i != m of A_i'A_i, G = unfold(M, m) khatri_rao(A_i, i != m),
 *     A_m = G P^-1; then F2 = sum of the Hadamard product of all A_i'A_i, ip = sum G o A_m of the last mode,
 *     e_t = sqrt|normM^2 + F2 - 2 ip| / normM; the fit stops after iteration t when t >= 1 and |e_{t-1} - e_t| < tol, after
 *     max_iter iterations, or when a pivot of P is zero or not finite ("singular").
 * Whole iterations run on the device behind a status word, in chunks without a host wait; every sum has a fixed order (two fits
 * give the same bits, whatever the chunk length).  k > min d_i is refused (tensorly would pad the init with random columns).
 * cca_zoo/linear/_tcca.py:111-117, cca_zoo/nonparametric/_ktcca.py:130-136 */
#define CCZ_CP_RUNNING 0
#define CCZ_CP_TOL 1
#define CCZ_CP_MAXITER 2
#define CCZ_CP_SINGULAR 3

/* Create a fit state for tensors of `order` modes of widths dims[i], rank k, up to chunk_iters iterations per
 * ccz_cp_iterations call.  CCZ_EUNSUP: order outside 2..8, k outside 1..32, prod dims > 2^24.  CCZ_EINVAL: k > min dims, an
 * empty mode, tol < 0 or NaN, max_iter or chunk_iters < 1.  (_tcca.py:111-117, _ktcca.py:130-136) */
CCZ_API int ccz_cp_create(ccz_handle h, int order, const int64_t* dims, int64_t k, double tol, int64_t max_iter,
                          int64_t chunk_iters, void** state_out);

/* Free a fit state (synchronises the handle's stream).  NULL is a no-op.  (_tcca.py:111-117, _ktcca.py:130-136) */
CCZ_API int ccz_cp_destroy(ccz_handle h, void* state);

/* A new fit of the tensor at M_dev: its unfoldings (made once), ||M||_F, the SVD init, the status word.  M_dev is read by
 * every later ccz_cp_iterations of this fit and must stay unchanged until they have run.  May wait for the device (the
 * symmetric EVD behind the init reads its eigenvalues on the host).  (_tcca.py:111-117, _ktcca.py:130-136) */
CCZ_API int ccz_cp_setup(ccz_handle h, void* state, const double* M_dev);

/* Restart the fit of the tensor of the last ccz_cp_setup from the given factors (host, float64, A_m as d_m x k row-major,
 * modes back to back) instead of the SVD init.  (_tcca.py:111-117, _ktcca.py:130-136) */
CCZ_API int ccz_cp_set_init(ccz_handle h, void* state, const double* factors_host);

/* Enqueue n_iters (<= chunk_iters) iterations.  Returns without waiting for the device; the only host wait is for the chunk
 * that used the same status slot two calls earlier, whose state is returned in iters_known / stopped_known (-1 / 0 when
 * there is none yet).  Iterations after the stop are no-ops.  (_tcca.py:111-117, _ktcca.py:130-136) */
CCZ_API int ccz_cp_iterations(ccz_handle h, void* state, int64_t n_iters, int64_t* iters_known, int* stopped_known);

/* Iterations done, whether the fit has stopped and why (CCZ_CP_*), the last error e_t and the last |e_{t-1} - e_t|.
 * Synchronises.  (_tcca.py:111-117, _ktcca.py:130-136) */
CCZ_API int ccz_cp_status(ccz_handle h, void* state, int64_t* iters, int* stopped, int* reason, double* err, double* decrease);

/* The factors (layout of ccz_cp_set_init) and the error trace e_0 .. e_{iters-1} (size it for max_iter) to the host; NULL
 * outputs are skipped.  Synchronises.  (_tcca.py:111-117, _ktcca.py:130-136) */
CCZ_API int ccz_cp_get_result(ccz_handle h, void* state, double* factors_host, double* trace_host, int64_t* n_trace);

/* ---- Row-sparse reduced-rank regression by ADMM (csrc/rrr.hip): the coefficient step of CCAR3 ------------------------------
 * With M = (Sxx + (rho + eps) I)^-1 (p x p) and P = Sxy Sy^-1/2 (p x q), both float64 in DEVICE memory, from Z = U = 0:
 *   B = M (P + rho (Z - U));  Z_old = Z;  Z = B + U, every row scaled by max(0, 1 - (lambda_ / rho) / |row|) (a zero row stays
 *   zero);  U += B - Z;  the fit stops after the iteration whose max(|Z - B|_F, |Z_old - Z|_F) / sqrt(p) < tol, or after
 *   max_iter.  The result is Z, which has exact zero rows.
 * The reference solves with the Cholesky factor every iteration; M is the explicit inverse (condition number at most
 * (lambda_max + rho) / rho).  Whole iterations run on the device behind a status word, two launches each, in chunks without
 * a host wait; every sum has a fixed order (two fits give the same bits, whatever the chunk length).
 * cca_zoo/linear/_ccar3.py:37-80 (_admm_row_sparse_rrr) */
#define CCZ_RRR_RUNNING 0
#define CCZ_RRR_TOL 1
#define CCZ_RRR_MAXITER 2

/* Create a fit state for a p x q coefficient matrix, up to chunk_iters iterations per ccz_rrr_iterations call.  CCZ_EUNSUP:
 * p + q > 16384, q > 1024.  CCZ_EINVAL: p or q < 1, lambda_ < 0, rho <= 0, tol < 0, a NaN, max_iter or chunk_iters < 1.
 * (_ccar3.py:37-54) */
CCZ_API int ccz_rrr_create(ccz_handle h, int64_t p, int64_t q, double lambda_, double rho, double tol, int64_t max_iter,
                           int64_t chunk_iters, void** state_out);

/* Free a fit state (synchronises the handle's stream).  NULL is a no-op.  (_ccar3.py:37-80) */
CCZ_API int ccz_rrr_destroy(ccz_handle h, void* state);

/* A new fit on M (Minv_dev, p x p) and P (P_dev, p x q): Z = U = 0, the status word.  Both matrices are read by every later
 * ccz_rrr_iterations of this fit and must stay unchanged until they have run.  Does not wait for the device.
 * (_ccar3.py:48-54) */
CCZ_API int ccz_rrr_setup(ccz_handle h, void* state, const double* Minv_dev, const double* P_dev);

/* Enqueue n_iters (<= chunk_iters) iterations.  Returns without waiting for the device; the only host wait is for the chunk
 * that used the same status slot two calls earlier, whose state is returned in iters_known / stopped_known (-1 / 0 when
 * there is none yet).  Iterations after the stop are no-ops.  (_ccar3.py:55-70) */
CCZ_API int ccz_rrr_iterations(ccz_handle h, void* state, int64_t n_iters, int64_t* iters_known, int* stopped_known);

/* Iterations done, whether the fit has stopped and why (CCZ_RRR_*), and the two residuals of the last iteration.
 * Synchronises.  (_ccar3.py:67-70) */
CCZ_API int ccz_rrr_status(ccz_handle h, void* state, int64_t* iters, int* stopped, int* reason, double* primal, double* dual);

/* Z (p x q row-major) to the host and / or to another device buffer; NULL outputs are skipped.  Synchronises when Z_host is
 * given.  (_ccar3.py:71-80: Z, not B, is returned) */
CCZ_API int ccz_rrr_get_result(ccz_handle h, void* state, double* Z_host, double* Z_dev);

/* *out_host = sum over the rows of (sum_j (y_ij - mean_j)^2)^2 of one view of DEVICE rows: rows read in `dtype`, arithmetic in
 * float64, per-workgroup partials folded in index order (two calls give the same bits).  mean_dev: float64, NULL for none.
 * The one quantity of sklearn's Ledoit-Wolf shrinkage that the second moments do not hold (beta_ = sum (X^2)'(X^2)).
 * Synchronises.  cca_zoo/linear/_ccar3.py:258 (LedoitWolf().fit(Y)) */
CCZ_API int ccz_rownorm4(ccz_handle h, int dtype, const ccz_view* view, int64_t n_rows, const double* mean_dev, double* out_host);

/* out (rows x cols, row stride ldo) = (G[r0 + i][c0 + j] - (center ? s[r0 + i] s[c0 + j] / n_rows : 0)) / n_rows, plus `shift`
 * on the diagonal (a diagonal block only), from the moments [G | s] of ccz_moments (upper triangle authoritative): X'X / n,
 * X'Y / n and Y'Y / n of the centred views as dense matrices, without a pass over the data.
 * cca_zoo/linear/_ccar3.py:48-50, 273-274 */
CCZ_API int ccz_moments_block(ccz_handle h, const double* moments_dev, int64_t D, int64_t n_rows, int center, int64_t r0,
                              int64_t rows, int64_t c0, int64_t cols, double shift, double* out_dev, int64_t ldo);

/* ---- TreeCCA (csrc/tree.hip): boosted-tree CCA, histogram tree growth on the device ---------------------------------------
 * The booster is the one tests/treecca_restatement.py specifies: 256 bins per feature from the sorted column of at most 8192
 * sampled rows, gradients in fixed point (q = rint(g 2^S), |q| <= 2^30, node sums exact integers), gain in float64 with every
 * operation rounded once, ties to the lowest feature, then the lowest bin.  A tree is a heap of 2^(max_depth + 1) - 1 nodes
 * (children of i: 2 i + 1 and 2 i + 2): feature (-1: not a split), bin, threshold (float32 cut), leaf (float32, 0 on a split),
 * gain (float64, 0 on a leaf).  Limits: 2..8 views, 1 <= k <= 32 and k <= every p_i, 1 <= max_depth <= 8, p_i <= 32768,
 * n < 2^31; the histogram workspace is 64 MiB (the features of a level are tiled to fit it).
 *   create         a fit state for n_rounds rounds; subsample in (0, 1], seed the hash seed of the row samples
 *   setup          cuts and bins of every view from DEVICE rows (dtype CCZ_F32 / CCZ_F64, means_dev of the same dtype or null);
 *                  sample_rows (host) are the min(n, 8192) rows the cuts are taken from
 *   project        Z0_i = (X_i - mean_i) W_i (W_host: the p_i x k blocks one after another, float64) kept on the device;
 *                  sumsq_host (n_views x k) receives the column sums of squares
 *   set_margin     base margin = float32(Z0 / scale) (scale_host: n_views x k), tree sums zero, the round counter zero
 *   set_features   per view n_selected[i] ascending feature indices for every round (lists_host: view after view, round after
 *                  round)
 *   rounds         enqueues n_rounds (at most chunk_rounds) whole rounds: per view in turn the EY gradient of all views, the shared
 *                  rescale to std 0.1, one tree per component, and with gauss_seidel a fresh gradient before the next view; no
 *                  host wait but for the status of the chunk two calls back (rounds_known: -1 while unknown)
 *   get_bins       bins (p x n, feature-major), cuts (p x 256, unused entries +inf) and cut counts of a view, to the host
 *   get_trees      the trees of a view, rounds x k x nodes each, to the host
 *   get_embedding  double(base margin) + double(float32 tree sum), n x k float64, to the host and / or the device
 *   grow           TEST SEAM: the k trees of one view from caller-supplied HOST bins (p x n), cuts (p x 256), cut counts,
 *                  quantised gradients (k x n, int32), shifts (k), row mask (n) and ascending feature list; hist_bytes > 0
 *                  replaces the workspace bound (to force feature tiling).  Returns k x nodes heap arrays and node_out (k x n):
 *                  a row's position in the last level, a leaf above it continued to the left (pos -> 2 pos).
 *   predict        out_dev (n x k, float64) = (X - mean) P (proj_dev: p x k float64, null: 0) + the float32 leaves of n_trees
 *                  trees ([n_trees][k][nodes] DEVICE arrays) summed in tree order; left iff float32(x - mean) < threshold */
CCZ_API int ccz_tree_create(ccz_handle h, int n_views, const int64_t* p, int64_t n_rows, int64_t k, int64_t max_depth, int64_t n_rounds,
                            double learning_rate, double min_child_weight, int gauss_seidel, double subsample, uint64_t seed,
                            int64_t chunk_rounds, void** state_out);
CCZ_API int ccz_tree_destroy(ccz_handle h, void* state);
CCZ_API int ccz_tree_setup(ccz_handle h, void* state, int dtype, const ccz_view* views, const void* const* means_dev,
                           const int64_t* sample_rows, int64_t n_sample);
CCZ_API int ccz_tree_project(ccz_handle h, void* state, int dtype, const ccz_view* views, const void* const* means_dev, const double* W_host,
                             double* sumsq_host);
CCZ_API int ccz_tree_set_margin(ccz_handle h, void* state, const double* scale_host);
CCZ_API int ccz_tree_set_features(ccz_handle h, void* state, const int* n_selected, const int* lists_host);
CCZ_API int ccz_tree_rounds(ccz_handle h, void* state, int64_t n_rounds, int64_t* rounds_known, int* stopped_known);
CCZ_API int ccz_tree_status(ccz_handle h, void* state, int64_t* rounds, int* stopped);
CCZ_API int ccz_tree_get_bins(ccz_handle h, void* state, int view, uint8_t* bins_host, float* cuts_host, int* ncuts_host);
CCZ_API int ccz_tree_get_trees(ccz_handle h, void* state, int view, int* feature_host, int* bin_host, float* threshold_host,
                               float* leaf_host, double* gain_host);
CCZ_API int ccz_tree_get_embedding(ccz_handle h, void* state, int view, double* Z_host, double* Z_dev);
CCZ_API int ccz_tree_grow(ccz_handle h, int64_t n_rows, int64_t p, int64_t k, int64_t max_depth, const uint8_t* bins_host,
                          const float* cuts_host, const int* ncuts_host, const int* q_host, const int* shift_host, const uint8_t* mask_host,
                          const int* features_host, int64_t n_features, double learning_rate, double min_child_weight, int64_t hist_bytes,
                          int* feature_out, int* bin_out, float* threshold_out, float* leaf_out, double* gain_out, uint8_t* node_out);
CCZ_API int ccz_tree_predict(ccz_handle h, int dtype, const ccz_view* view, int64_t n_rows, const void* mean_dev, const double* proj_dev,
                             int64_t k, int64_t n_trees, int64_t max_depth, const int* feature_dev, const float* threshold_dev,
                             const float* leaf_dev, double* out_dev, int64_t ldo);

/* ---- permutation null of the two-view singular values (csrc/perm.hip) ------
 * sv_dev[b, :] (nperm x r, r = min(p1, p2), float64, descending) = the singular values of
 *   scale * Z_1' Z_2[pi_b]        Z_i: n x p_i float64, row-major, ld = p_i, device;
 * pi_b = perms_dev[b * n .. b * n + n) (int32, device), perms_dev NULL = the identity (nperm must then be 1).  The rows of
 * Z_1 are read in order, those of Z_2 gathered by index; many permutations share one launch (grid: row split x permutation).
 * The rows are cut into splits of CCZ_PERM_ROWS -- a function of n alone -- whose partial products (fp64 MFMA) go to pooled
 * scratch and are folded in split order, then one workgroup per permutation runs a one-sided Jacobi SVD.  No floating-point
 * atomics: the bits of sv_dev[b, :] depend on (Z_1, Z_2, pi_b, scale) only -- not on nperm, on b, or on how a caller cuts
 * its permutations into calls.  Indices are trusted like sparse indices (an index outside [0, n) reads row 0 or n - 1).
 * A row of NaN in sv_dev: the Jacobi sweeps did not settle (non-finite input).  Enqueue-only on the handle's stream.
 * CCZ_EUNSUP: p_i > 64 or n >= 2^31;  CCZ_EINVAL: n, p_i, nperm < 1, a null pointer, or nperm != 1 without perms_dev. */
#define CCZ_PERM_ROWS 4096
#define CCZ_PERM_MAXP 64
CCZ_API int ccz_perm_singular_values(ccz_handle h, int64_t n, int64_t p1, int64_t p2, const double* Z1_dev, const double* Z2_dev,
                                     const int32_t* perms_dev, int64_t nperm, double scale, double* sv_dev);

/* ---- bootstrap refits of the two-view ridge CCA (csrc/boot.hip) -----------
 * Resample b is its multiplicity vector m_b = counts_dev[b * n .. b * n + n) (int32, device: how often row s was drawn);
 * counts_dev NULL = all ones (nboot must then be 1).  With x_s = [x1_s, x2_s] (X_i: n x p_i float64, row-major, ld = p_i,
 * device) and N_b = sum_s m_b[s]:
 *   G_b = sum_s m_b[s] x_s x_s',  s_b = sum_s m_b[s] x_s,  C = (G_b - s_b s_b' / N_b) / (N_b - 1)  (center = 0: G_b / (N_b - 1))
 *   R_i = (1 - c_i) C_ii + c_i I = L_i L_i',   T = L_1^-1 C_12 L_2^-T = U S V',   W_1 = L_1^-T U_k,  W_2 = L_2^-T V_k.
 * sv_dev[b, :] (nboot x r, r = min(p1, p2), descending) = S;  W_dev[b] ((p1 + p2) x k row-major, the rows of view 1 first) =
 * [W_1; W_2], column j in the coupled sign of the pair (u_j, v_j) -- no other sign rule;  info_dev[b]: 0, or CCZ_BOOT_INFO_*
 * (the resample's rows of sv_dev and W_dev are then NaN).  The divisor is N_b, not n: 0/1 counts give subsampling.  The rows
 * are read in their stored order (no gather; a staged chunk whose counts are all zero is skipped), in splits of CCZ_PERM_ROWS
 * rows -- a function of n alone -- whose partial moments (fp64 MFMA; the 11 and 22 blocks on and above the diagonal only) go
 * to pooled scratch and are folded in split order; one workgroup per resample then factors, solves and runs a one-sided
 * Jacobi SVD that accumulates the right vectors.  No floating-point atomics: the bits of resample b depend on (X, m_b, c, center, k)
 * only -- not on nboot, on b, or on how a caller cuts its resamples into calls.  Counts are trusted (nothing is dereferenced
 * through them).  With center set, pass views whose column means are near zero (the covariance does not change under a shift;
 * G_b - s_b s_b' / N_b cancels otherwise).  Enqueue-only on the handle's stream.
 * CCZ_EUNSUP: p_i > 64 or n >= 2^31;  CCZ_EINVAL: n, p_i, nboot, k < 1, k > r, a null pointer, or nboot != 1 without counts_dev. */
#define CCZ_BOOT_INFO_R1 1       /* R_1 has a non-positive or non-finite pivot */
#define CCZ_BOOT_INFO_R2 2       /* R_2 has a non-positive or non-finite pivot */
#define CCZ_BOOT_INFO_N 3        /* N_b < 2 */
#define CCZ_BOOT_INFO_JACOBI 4   /* the Jacobi sweeps did not settle */
CCZ_API int ccz_boot_rcca(ccz_handle h, int64_t n, int64_t p1, int64_t p2, const double* X1_dev, const double* X2_dev,
                          const int32_t* counts_dev, int64_t nboot, double c1, double c2, int center, int64_t k, double* sv_dev,
                          double* W_dev, int32_t* info_dev);

/* ---- delete-group jackknife of the same fit (csrc/boot.hip) ----------------
 * Replicate g in [g0, g0 + ng) is the fit above on all rows EXCEPT those with s % ngroups == g (ngroups == n: leave-one-out).
 * The groups are interleaved, so rows sorted by class do not put a whole stratum into one group; group sizes differ by at
 * most 1.  In exact arithmetic replicate g equals ccz_boot_rcca with the 0/1 counts m[s] = (s % ngroups != g); here its moments
 * are the full-sample moments (one pass per call, the all-ones resample of ccz_boot_rcca) minus those of the rows left out,
 *   G_(g) = G - sum_{s in g} x_s x_s',   s_(g) = s - sum_{s in g} x_s,   N_(g) = n - |g|,
 * one workgroup per replicate (plain fp64 FMAs in row order, subtracted once), then the solve of ccz_boot_rcca unchanged: no
 * count matrix, and the whole jackknife reads the data twice.  sv_dev (ng x r), W_dev (ng x (p1 + p2) x k), info_dev (ng): row i
 * is replicate g0 + i; layouts, the coupled sign, CCZ_BOOT_INFO_* and NaN rows as above.  No floating-point atomics and every
 * sum in a fixed order: the bits of replicate g depend on (X, ngroups, g, c, center, k) only -- not on g0 or ng.  With center
 * set, pass views whose column means are near zero, as above.  Enqueue-only on the handle's stream.
 * CCZ_EUNSUP: p_i > 64 or n >= 2^31;  CCZ_EINVAL: n, p_i, ng, k < 1, k > r, a null pointer, ngroups < 2, ngroups > n, g0 < 0 or
 * g0 + ng > ngroups. */
CCZ_API int ccz_jack_rcca(ccz_handle h, int64_t n, int64_t p1, int64_t p2, const double* X1_dev, const double* X2_dev,
                          int64_t ngroups, int64_t g0, int64_t ng, double c1, double c2, int center, int64_t k, double* sv_dev,
                          double* W_dev, int32_t* info_dev);

/* ---- the draws of ccz_perm_singular_values and ccz_boot_rcca, made on the device (csrc/draw.hip) ---
 * Pure functions of (seed, b, n), b = the resample's index in the whole call (row i of a call is resample first + i), on
 * the stream convention of the ccz_svi_* and ccz_nuts_* sections (all arithmetic uint64, wrapping):
 *   stream(seed, b, site) = splitmix64(splitmix64(splitmix64(seed) + b) + site)
 *   key(seed, b, site, j) = splitmix64(stream(seed, b, site) ^ splitmix64(j))                            j = 0 .. n - 1
 * ccz_draw_permutations: perms_dev (nperm x n, int32) row i = pi_{first + i} = argsort_j key(seed, first + i, CCZ_DRAW_SITE_PERM, j),
 *   i.e. pi[rank] = j.  splitmix64 is a bijection of the 64-bit words, so the n keys of one stream are pairwise distinct:
 *   the order is total and no tie rule exists.  The keys are never stored: a one-level bucket sort (count, scan, scatter,
 *   sort in LDS) recomputes them from j.  bucket_rows = expected rows per bucket (0: CCZ_DRAW_BUCKET_ROWS); the result does
 *   not depend on it by a bit -- it exists so that tests reach the scan over many buckets and, with more than
 *   CCZ_DRAW_SORT_CAP rows in a bucket, the slower path that ranks an oversize bucket by counting.
 * ccz_draw_counts: counts_dev (nboot x n, int32) row i = m_{first + i}, m_b[s] = #{j < n : idx_j = s} with
 *   idx_j = (key(seed, b, CCZ_DRAW_SITE_BOOT, j) * n) >> 64, the high word of the 128-bit product (multiply-shift, no
 *   rejection): a row is drawn with probability within n / 2^64 of 1 / n (some rows own one more of the 2^64 keys than
 *   others), below 1.2e-10 relative at n = 2^31 and below anything a test can see.
 * Integer arithmetic and integer atomics only: the bits depend on (seed, first + i, n) alone -- not on nperm / nboot, on
 * how a caller cuts its resamples into calls, or on bucket_rows.  Scratch (bucket cursors, rows in bucket order) is pooled
 * in the handle and sized per launch group.  Enqueue-only on the handle's stream.
 * CCZ_EINVAL: n < 1, nperm / nboot < 1, first < 0, bucket_rows < 0 or a null pointer;  CCZ_EUNSUP: n >= 2^31.  A refused call
 * writes nothing. */
#define CCZ_DRAW_SITE_PERM 0x5045524Dull   /* "PERM" */
#define CCZ_DRAW_SITE_BOOT 0x424F4F54ull   /* "BOOT" */
#define CCZ_DRAW_BUCKET_ROWS 1024
#define CCZ_DRAW_SORT_CAP 2048             /* rows of one bucket that the sort pass holds in LDS */
CCZ_API int ccz_draw_permutations(ccz_handle h, int64_t n, int64_t nperm, uint64_t seed, int64_t first, int64_t bucket_rows,
                                  int32_t* perms_dev);
CCZ_API int ccz_draw_counts(ccz_handle h, int64_t n, int64_t nboot, uint64_t seed, int64_t first, int32_t* counts_dev);

#ifdef __cplusplus
}
#endif
#endif /* CCZ_H */
