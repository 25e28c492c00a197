/*
 * gnnx.h -- C-ABI of the MI355X (gfx950) backend for the walexi/gnn.cpp GCN hot path.
 *
 * This is the drop-in boundary.  The reference has no FFI: its device hook is
 * the empty include/device.cuh + the commented call `device::add(out_data, lhs_data, rhs_data)`
 * (reference include/functional.h:174,180) -- free functions on raw buffers called from
 * functional::<op>.  These entry points sit exactly there: plain pointers and sizes, int status
 * returns, an explicit stream, no C++/torch types.  The C++ mirror of the reference API
 * (gnn.cpp_amd/host/) and the ctypes binding (gnn.cpp_amd/capi.py) are the two callers.
 *
 * Conventions
 *   - every pointer named d_* is DEVICE memory (hipMalloc'd, e.g. torch.Tensor.data_ptr() or gnnx_malloc);
 *   - dense matrices are row-major fp32 with an explicit leading dimension in ELEMENTS (ld >= cols),
 *     exactly the reference's contiguous std::valarray<float> layout (reference include/tensor.h:825)
 *     when ld == cols;
 *   - CSR indices are int32 (rowptr has n_rows+1 entries; nnz < 2^31), columns ASCENDING in a row
 *     (the row-major scan order of reference src/graph.cpp:52-60);
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); calls are asynchronous on
 *     it unless stated; nothing is allocated or synchronised inside a compute call;
 *   - return 0 (GNNX_OK) or a negative gnnx_status; gnnx_last_error() gives the message of the
 *     calling thread's last failure.  The C++ wrapper maps them to std::runtime_error with the
 *     reference's ERROR_* texts (reference include/utils.h:19-30).
 *   - threads: every entry point may be called from any host thread; a call works on the stream it is given and keeps no state of
 *     its own between calls beyond what its handles (plans, communicators) own -- one thread drives one handle at a time.  Host
 *     threads that run ranks of an in-process group each use a stream of their OWN (gnnx_stream_create; the C++ layer does this
 *     by itself), never the NULL stream; what crosses threads is ordered by the collectives (gnnx_comm.hip) and nothing else
 *     needs to be.  Process-wide state is immutable once built (the libm table of the degree block, kernel attribute opt-ins).
 */
#ifndef GNNX_H
#define GNNX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNNX_VERSION 100

typedef enum gnnx_status {
    GNNX_OK = 0,
    GNNX_ERR_INVALID_ARG = -1,  /* null pointer / negative size / ld < cols / misaligned */
    GNNX_ERR_SHAPE = -2,        /* operand shapes do not agree (reference CHECK_MM_DIMS, utils.cpp:8-78) */
    GNNX_ERR_INDEX_RANGE = -3,  /* an edge endpoint is outside [0, n_nodes) (reference graph.cpp:89) */
    GNNX_ERR_WORKSPACE = -4,    /* caller-provided workspace too small */
    GNNX_ERR_HIP = -5,          /* a HIP runtime call failed (message in gnnx_last_error) */
    GNNX_ERR_NO_DEVICE = -6,    /* no gfx950 device visible */
    GNNX_ERR_UNSUPPORTED = -7
} gnnx_status;

int gnnx_version(void);
const char *gnnx_status_string(int status);
const char *gnnx_last_error(void);

/* ------------------------------------------------------------------ runtime plumbing ------------- */
/* Thin HIP wrappers so that host code above this ABI needs no HIP headers. */
int gnnx_device_count(int *count);
int gnnx_set_device(int device);
int gnnx_device_name(int device, char *buf, size_t buflen);
int gnnx_malloc(void **d_ptr, size_t bytes);
int gnnx_free(void *d_ptr);
int gnnx_memset(void *d_ptr, int value, size_t bytes, void *stream);
int gnnx_memcpy_h2d(void *d_dst, const void *h_src, size_t bytes, void *stream);
int gnnx_memcpy_d2h(void *h_dst, const void *d_src, size_t bytes, void *stream); /* synchronises `stream` */
int gnnx_memcpy_d2d(void *d_dst, const void *d_src, size_t bytes, void *stream);
/* rows x width_bytes between two pitched device buffers (stream-ordered) */
int gnnx_memcpy2d_d2d(void *d_dst, size_t dst_pitch_bytes, const void *d_src, size_t src_pitch_bytes, size_t width_bytes, size_t rows,
                      void *stream);
int gnnx_stream_create(void **stream);
int gnnx_stream_destroy(void *stream);
int gnnx_stream_sync(void *stream);
int gnnx_device_sync(void);
int gnnx_event_create(void **event);
int gnnx_event_destroy(void *event);
int gnnx_event_record(void *event, void *stream);
int gnnx_event_sync(void *event);
int gnnx_event_elapsed_ms(void *start, void *stop, float *ms);
int gnnx_stream_wait_event(void *stream, void *event); /* work queued on `stream` after this call waits for `event` */

/* ------------------------------------------------------------------ graph build ------------------ */
/*
 * COO [2,E] -> CSR with the reference's adjacency semantics:
 *   A[src][dst] = 1 by assignment  => duplicate edges collapse   (reference graph.cpp:21-44, line 40)
 *   diagonal zeroed                => self loops are REMOVED     (graph.cpp:68-75 with fillValue 0, called
 *                                                                 from GCNConv::forward graph.cpp:172)
 *   row-major scan                 => entries ordered by (src,dst) (graph.cpp:46-67)
 * Replaces the dense round trip edge_to_adj_mat -> fill_diagonal_ -> adj_to_edge_list.
 * Pass (d_dst, d_src) to get the CSR of A^T (what MatMul::_backward's dense transpose,
 * reference operation.h:524-527, becomes).
 *
 * d_rowptr: n_nodes+1 int32.  d_colidx: capacity n_edges int32.  *nnz_out: host int64, valid on return
 * (this call synchronises `stream`).  Workspace: gnnx_csr_from_coo_workspace() bytes of device memory.
 * flags: bit0 keep self loops, bit1 keep duplicates (both 0 = reference semantics).
 * Errors: GNNX_ERR_INDEX_RANGE if any endpoint is outside [0,n_nodes) (the reference would write out
 * of bounds at graph.cpp:40; its Data ctor throws at graph.cpp:89).
 */
#define GNNX_CSR_KEEP_SELF_LOOPS 1u
#define GNNX_CSR_KEEP_DUPLICATES 2u
int gnnx_csr_from_coo_workspace(int64_t n_edges, int32_t n_nodes, size_t *bytes);
int gnnx_csr_from_coo(const int32_t *d_src, const int32_t *d_dst, int64_t n_edges, int32_t n_nodes, uint32_t flags,
                      int32_t *d_rowptr, int32_t *d_colidx, int64_t *nnz_out, void *d_workspace,
                      size_t workspace_bytes, void *stream);

/* The SpMM entry points TRUST the CSR they are given (column ids index X without a bounds check: a check per gathered row would
 * sit in the hottest loop).  A CSR made by gnnx_csr_from_coo / gnnx_halo_plan_create is valid by construction; validate one from
 * anywhere else once, before its first use: rowptr[0] == 0, monotone, every column id in [0, n_cols).  Synchronises `stream`;
 * GNNX_ERR_INDEX_RANGE otherwise. */
int gnnx_csr_validate(const int32_t *d_rowptr, const int32_t *d_colidx, int32_t n_rows, int32_t n_cols, void *stream);

/* *equal_out = 1 iff the two device arrays hold the same n int32 values (synchronises `stream`).  The host layer compares an
 * incoming edge_index with the copy its cached adjacency was built from, so an edge list edited in place -- or a new one that
 * happens to be allocated at the old address -- never hits a stale CSR / norm. */
int gnnx_equal_i32(const int32_t *d_a, const int32_t *d_b, int64_t n, int *equal_out, void *stream);

/* Weighted adjacency (edge_attr, reference graph.h:35): A[r][c] = w by assignment, so of duplicate (r, c) pairs the LAST one
 * in the list wins (edge_to_adj_mat, graph.cpp:38-40).  diag_mode:
 *   GNNX_DIAG_KEEP   self loops stay as given                         (edge_to_adj_mat alone)
 *   GNNX_DIAG_STRIP  self loops are removed                           (add_self_loops(..., fillValue 0), graph.cpp:72)
 *   GNNX_DIAG_FILL   every (i, i) becomes diag_value, given or not    (add_self_loops(..., fillValue v))
 * flags: GNNX_CSR_KEEP_DUPLICATES keeps every entry of a run of equal (r, c) pairs, in list order, each with its own weight;
 * GNNX_CSR_DROP_TRUNCATED_ZERO drops entries whose value truncates to the integer 0 -- adj_to_edge_list's `int(data[i]) != 0` test
 * (graph.cpp:54), through which |w| < 1 vanishes on the add_self_loops round trip.  The contract: an entry is dropped iff
 * -1 < w < 1; NaN, +-inf and every |w| >= 1 stay (the test is two compares, never a float-to-int cast, so host and device agree on
 * every value).  It applies to the entry that survived its run -- a pair whose LAST weight is dropped vanishes entirely -- and to
 * diag_value.  Without the flag explicit zeros stay as entries (they add +-0 in a product, like the dense matrix).
 * Output: rowptr[N+1], colidx[nnz], vals[nnz] sorted by (row, column); capacity n_edges (+ n_nodes with GNNX_DIAG_FILL). */
enum { GNNX_DIAG_KEEP = 0, GNNX_DIAG_STRIP = 1, GNNX_DIAG_FILL = 2 };
#define GNNX_CSR_DROP_TRUNCATED_ZERO 4u
int gnnx_csr_from_coo_weighted_workspace(int64_t n_edges, int32_t n_nodes, size_t *bytes);
int gnnx_csr_from_coo_weighted(const int32_t *d_src, const int32_t *d_dst, const float *d_weights, int64_t n_edges, int32_t n_nodes,
                               uint32_t flags, int diag_mode, float diag_value, int32_t *d_rowptr, int32_t *d_colidx, float *d_vals,
                               int64_t *nnz_out, void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * Degree / symmetric-normalisation block of GCNConv::forward (reference graph.cpp:177-185):
 *   deg_i = 1 + sum_j A_ij        (adj_mat->sum(-1,true) + 1;  the "+1" stays although self loops were removed)
 *   s_i   = deg_i ^ (-1/2)        (deg->pow(-0.5))
 *   norm_i = s_i * sum_j A_ij s_j (adj_mat->mm(deg); norm *= deg), inner sum in the reference's matmul
 *            order (descending j, see DESIGN.md "summation order").
 * d_s and d_norm: n_rows fp32 each (the reference's [N,1] tensors).  Either may be NULL.
 * For a row block of a sharded graph pass d_s_cols (the s values indexed by COLUMN id, i.e. [local|halo])
 * and d_s is written for the block's own rows only; with d_s_cols == NULL columns index d_s itself.
 * s written here is LOOKED UP in a table of the host libm's powf(k, -0.5f), k = 1 .. 1 + max degree -- functional.h:253 is that call,
 * and glibc's powf is 1 ulp away from the correctly rounded value for 9 685 of the 2^24 degrees (the smallest 1058) -- so s, norm and
 * both aggregations carry the reference's bits at every size (test_headline_config_whole_graph_vs_oracle).  Writing d_s costs one
 * host synchronisation (the maximum degree); a caller may still pass its own s through d_s_cols with d_s == NULL.
 */
int gnnx_degree_norm_f32(const int32_t *d_rowptr, const int32_t *d_colidx, int32_t n_rows, float *d_s,
                         const float *d_s_cols, float *d_norm, void *stream);

/* ------------------------------------------------------------------ hot path: aggregation -------- */
/*
 * CSR SpMM with fused prologue/epilogue -- replaces functional::matmul on the dense N x N adjacency
 * (reference functional.h:399-441 called from graph.cpp:208), the broadcast multiply by norm
 * (graph.cpp:209 -> functional.h:190-213) and the bias add (graph.cpp:188 -> functional.h:163-187):
 *
 *   Y[i,:] = beta * Y[i,:] + rowscale[i] * ( sum_{p in row i, DESCENDING column} vals[p] * colscale[c_p] * X[c_p,:] ) + bias
 *
 *   forward  (graph.cpp:204-212,188):  vals=NULL colscale=NULL rowscale=norm bias=bias|NULL  on CSR(A)
 *   backward (operation.h:144-167 then :524-531):  dH = A^T . (norm (.) G):
 *                                      vals=NULL colscale=norm rowscale=NULL bias=NULL      on CSR(A^T)
 *   Mode SYM (textbook D^-1/2 A D^-1/2): colscale=s rowscale=s.
 * Every product/add is separately rounded fp32 in the reference's order -- ONE accumulator per output element, whatever the
 * row's degree -- so the result is bit-identical to the reference CPU path (modulo the sign of 0), with or without a plan.
 * vals, colscale, rowscale, bias may each be NULL.  beta is 0 or 1 (1 = the reference's `_grad +=`,
 * tensor.h:268-271).  X: [n_cols, F] ld ldx.  Y: [n_rows, F] ld ldy.  X and Y must not alias.
 *
 * `plan` (optional, from gnnx_spmm_plan_create) load-balances power-law rows without touching the arithmetic: rows longer
 * than `chunk` (the hub rows) are summed by wavefronts of their own -- one per (row, 64-feature slab), the neighbour rows in
 * flight in an LDS ring, still one accumulator per feature in descending column order (functional.h:433-439) -- and the other
 * rows are cut into non-zero-balanced blocks.  Planned and unplanned results are the same bits; the plan only changes the
 * time (RMAT 10M / 100M, F = 256: 18.0 -> 13.6 ms).  max_feat is ignored (kept for source compatibility).
 * gnnx_spmm_plan_info: number of hub rows and their non-zeros.
 */
typedef struct gnnx_spmm_plan gnnx_spmm_plan; /* opaque, device-resident work list */
int gnnx_spmm_plan_create(const int32_t *d_rowptr, int32_t n_rows, int32_t chunk, int32_t max_feat,
                          gnnx_spmm_plan **plan, void *stream);
int gnnx_spmm_plan_destroy(gnnx_spmm_plan *plan);
/* GNNX_OK, or GNNX_ERR_HIP when a completed launch of the plan's producer / consumer kernel gave up one of its bounded waits (the
 * rows it owned were then NOT written: nothing is ever summed from a slot that did not land).  One read of pinned host memory, no
 * synchronisation; every planned aggregation call makes the same check on entry and returns the error instead of launching. */
int gnnx_spmm_plan_status(const gnnx_spmm_plan *plan);
int gnnx_spmm_plan_info(const gnnx_spmm_plan *plan, int64_t *n_hub_rows, int64_t *n_hub_nnz);
/* The longest hub rows are summed by the producer / consumer hub kernel -- a CU per (row, 64-feature slab): one wavefront adds in
 * the reference's order, three keep the row's slices coming through a 128 KiB LDS ring -- because their time is their own chain of
 * dependent adds, not their bytes.  By default the library picks them per call (rows whose chain in the plain hub kernel would
 * exceed half of what all hub rows' bytes take: a handful on a whole 10 M / 100 M graph, the rows beyond ~18 k non-zeros on an
 * eighth of it).  threshold >= 0 fixes the cut (rows longer than it; tests pass 0: every hub row), < 0 restores the default.  Same
 * bits for every choice. */
int gnnx_spmm_plan_set_big_row_threshold(gnnx_spmm_plan *plan, int32_t threshold);
/* *structured = 1 when the plan's hub rows sit on vertex ids with few one-bits (non-zero-weighted mean popcount well below half the id
 * width) and are not one dense block of consecutive ids -- what R-MAT and other generators that draw the bits of an id independently
 * produce; ids spread at random, or hubs sorted to the front, do not.  The hub rows of CSR(A) are the rows the aggregation over
 * CSR(A^T) gathers most, and vice versa: with such ids the gathered matrix wants the padded row pitch of gnnx_gather_row_stride. */
int gnnx_spmm_plan_hub_ids_structured(const gnnx_spmm_plan *plan, int *structured);

int gnnx_spmm_csr_f32(int32_t n_rows, int32_t n_cols, int32_t n_feat, const int32_t *d_rowptr,
                      const int32_t *d_colidx, const float *d_vals, const float *d_colscale,
                      const float *d_rowscale, const float *d_bias, const float *d_X, int64_t ldx, float beta,
                      float *d_Y, int64_t ldy, const gnnx_spmm_plan *plan, void *stream);

/* The same SpMM with the modules that GCNConv::forward runs either side of the aggregation folded in, so the
 * normalised / rectified activations never make their own trip through HBM:
 *   prologue, applied to every gathered row of X before it is added (forward mode only: vals = colscale = NULL):
 *     bn_mean/bn_var != NULL : x <- ((x - mean) / (var + eps)^0.5) * gamma + beta   (nn.cpp:285-330 BatchNorm::forward with
 *                              the batch statistics of gnnx_bn_stats_f32; gamma / beta NULL = 1 / 0)
 *     relu_in  != 0          : x <- where(x > 0, x, 0)                              (nn.cpp:229-237, graph.cpp:174-175)
 *   epilogue: relu_out != 0  : Y <- where(Y > 0, Y, 0) after rowscale / bias / beta (the ReLU between two stacked layers).
 * Separately rounded ops in the order of gnnx_bn_relu_fwd_f32: fused and unfused results are the same bits.
 * fusion == NULL is gnnx_spmm_csr_f32. */
typedef struct gnnx_spmm_fusion {
    const float *bn_mean, *bn_var, *bn_gamma, *bn_beta; /* [F] device pointers, or NULL */
    float bn_eps;
    int relu_in;
    int relu_out;
} gnnx_spmm_fusion;
int gnnx_spmm_csr_fused_f32(int32_t n_rows, int32_t n_cols, int32_t n_feat, const int32_t *d_rowptr,
                            const int32_t *d_colidx, const float *d_vals, const float *d_colscale,
                            const float *d_rowscale, const float *d_bias, const float *d_X, int64_t ldx, float beta,
                            float *d_Y, int64_t ldy, const gnnx_spmm_fusion *fusion, const gnnx_spmm_plan *plan,
                            void *stream);

/* Backward aggregation of a layer whose forward fused BatchNorm + ReLU into the gather (gnnx_spmm_csr_fused_f32): dY = A^T . (vals (.) G)
 * on CSR(A^T) as gnnx_spmm_csr_f32 computes it (same bits), PLUS the two column sums BatchNorm's backward needs before it can
 * produce dX -- dbeta = sum_i g_i and dgamma = sum_i g_i xhat_i with g = dY where relu(BN(h)) > 0 (the mask recomputed from H
 * with the forward's arithmetic; relu = 0: g = dY), xhat = (h - mean) * (var + eps)^-1/2 -- accumulated by the wavefronts that
 * store the rows of dY (the row of dY comes back from L2, the row of H is the one extra read) and reduced in a fixed order: the
 * separate sums pass over dY and H (gnnx_bn_relu_bwd_sums_f32: 8 F bytes per node) disappears.  Follow with
 * gnnx_bn_relu_bwd_apply_f32.  Same summands as gnnx_bn_relu_bwd_sums_f32 in another (fixed) order: rounding-level agreement.
 * Shapes: n_feat % 4 == 0, n_feat > 64, 16-byte aligned rows; GNNX_ERR_UNSUPPORTED otherwise (use the two separate calls). */
int gnnx_spmm_csr_bn_sums_workspace(int32_t n_rows, int32_t n_feat, const gnnx_spmm_plan *plan, size_t *bytes);
int gnnx_spmm_csr_bn_sums_f32(int32_t n_rows, int32_t n_cols, int32_t n_feat, const int32_t *d_rowptr, const int32_t *d_colidx,
                              const float *d_vals, const float *d_G, int64_t ldg, float *d_dY, int64_t ldy, const float *d_H, int64_t ldh,
                              const float *d_mean, const float *d_var, float eps, const float *d_gamma, const float *d_beta, int relu,
                              float *d_dgamma, float *d_dbeta, void *d_workspace, size_t workspace_bytes, const gnnx_spmm_plan *plan,
                              void *stream);

/* Opt-in bf16 FEATURE STORAGE: the same SpMM gathering rows of X stored as bf16 -- 2 bytes per
 * feature instead of 4, i.e. about half the algorithmic bytes of the aggregation -- widened exactly to f32 in registers and
 * accumulated in f32 in the same order.  NOT the parity path: rounding X to bf16 (gnnx_f32_to_bf16, round to nearest even)
 * costs up to 2^-8 relative per element, far outside the 1e-5 bar; if X is exactly representable in bf16 the result is the f32
 * path's, bit for bit.  No fusion with this entry.  ldx in bf16 elements. */
int gnnx_f32_to_bf16(const float *d_X, int64_t ldx, int64_t n_rows, int32_t n_cols, uint16_t *d_Y_bf16, int64_t ldy, void *stream);
int gnnx_spmm_csr_bf16_f32(int32_t n_rows, int32_t n_cols, int32_t n_feat, const int32_t *d_rowptr, const int32_t *d_colidx,
                           const float *d_vals, const float *d_colscale, const float *d_rowscale, const float *d_bias,
                           const uint16_t *d_X_bf16, int64_t ldx, float beta, float *d_Y, int64_t ldy,
                           const gnnx_spmm_plan *plan, void *stream);
/* H = X . W^T (X [M,K], W [N,K]: the layer's transform, nn.cpp:205-211) written as bf16 by the product's own epilogue -- the same
 * round-to-nearest-even as gnnx_f32_to_bf16, so the result equals gnnx_gemm_f32 followed by gnnx_f32_to_bf16 bit for bit, without
 * the 4 M N-byte f32 round trip.  LDS-DMA kernel shapes only (K % 64 == 0, N % 4 == 0, N >= 64, M >= 2048, 16-byte aligned rows):
 * GNNX_ERR_SHAPE otherwise.  ldh in bf16 elements. */
int gnnx_gemm_nt_bf16out_workspace(int64_t M, int64_t N, int64_t K, size_t *bytes);
int gnnx_gemm_nt_bf16out_f32(int64_t M, int64_t N, int64_t K, const float *d_X, int64_t ldx, const float *d_W, int64_t ldw,
                             uint16_t *d_H_bf16, int64_t ldh, void *d_workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ hot path: transform ---------- */
/*
 * fp32 GEMM on the MFMA units (v_mfma_f32_32x32x2_f32, exact f32) -- replaces functional::matmul for the
 * dense products of the path (reference functional.h:399-441):
 *   C[M,N] = alpha * op(A)[M,K] . op(B)[K,N] + beta * C         row-major, ld in elements
 *   forward   H  = X . W^T      (nn.cpp:205-211)        transA=0 transB=1  A=X[N,Fin]   B=W[Fout,Fin]
 *   backward  dX = dH . W       (operation.h:516-523)   transA=0 transB=0  A=dH[N,Fout] B=W[Fout,Fin]
 *             dW = dH^T . X     (operation.h:524-531 + Transpose::_backward :416-433)
 *                                                       transA=1 transB=0  A=dH[N,Fout] B=X[N,Fin]
 * The big operands (X, dH, the outputs) are never transposed in memory (the reference materialises W^T, nn.cpp:207, and a
 * clone of each operand's transpose in backward).  transA=1 (reduction over the node dimension) runs split-K over workgroups
 * into the caller's workspace and reduces slabs in a fixed order (deterministic).  Tall products with whole 256-row tiles,
 * N % 128 == 0 and K % 64 == 0 take the LDS-DMA kernels; for X . W^T those want the small W k-major, so
 * gnnx_gemm_workspace() asks for K * N floats and the call transposes W into them first (same products, same order).  Every
 * kernel computes an output element as the same k-ascending fmaf chain: which kernel ran never changes a bit.
 * Workspace: gnnx_gemm_workspace() bytes (split-K slabs for transA=1; W^T for the tall transB=1 case; else 0).  The W^T
 * workspace is optional: a tall transB=1 call with less (or none) still works, on the register-staged kernels, and gives the
 * same bits.  The split-K slabs are required, and the required size is gnnx_gemm_workspace()'s figure, not the slabs a given call
 * happens to fill: a transA=1 call for which that figure is not 0 and that passes less returns GNNX_ERR_WORKSPACE and leaves C
 * untouched (one workgroup per output tile over millions of rows would be far slower, silently).
 * Epilogue, the same in every kernel: v = fl(alpha * acc), then, only if beta != 0, fl(v + fl(beta * C)) -- three separately
 * rounded float32 operations, nothing fused; with beta == 0, C is never read (it may hold NaN).  K == 0 gives C = beta * C;
 * M == 0 or N == 0 returns GNNX_OK and writes nothing.  ldc < N is GNNX_ERR_INVALID_ARG; lda or ldb below the operand's row
 * length (K, or M resp. N for a k-major operand) is GNNX_ERR_SHAPE.
 */
int gnnx_gemm_workspace(int transA, int transB, int64_t M, int64_t N, int64_t K, size_t *bytes);
int gnnx_gemm_f32(int transA, int transB, int64_t M, int64_t N, int64_t K, float alpha, const float *d_A,
                  int64_t lda, const float *d_B, int64_t ldb, float beta, float *d_C, int64_t ldc,
                  void *d_workspace, size_t workspace_bytes, void *stream);

/* The backward GEMM of a stacked layer with its two followers fused into the epilogue:
 *   C[M,N] = (A[M,K] . B[K,N]) masked by the ReLU of the layer below: C[m][n] is kept where Ymask[m][n] > 0 (IEEE: NaN drops, as
 *            -0 and -inf do; a positive denormal and +inf keep) and is +0 elsewhere, whatever the product   (Mask::_backward,
 *            reference operation.h:557-562; Ymask = that layer's stored forward output)
 *   colsum[n] = sum_m C[m][n]                                                 (its bias gradient: Add::_backward -> sum_to_size,
 *            operation.h:114-128, tensor.h:618-638)
 * i.e. G_{l-1} = (dH_l . W_l) (.) (Y_{l-1} > 0) and db_{l-1} in ONE pass over the output: the unmasked gradient is never written,
 * the mask pass (read Y, read G, write G) and the column-sum pass (read G) disappear.  C holds the same bits as gnnx_gemm_f32
 * followed by the mask; colsum is summed per workgroup then over workgroups in a fixed order (deterministic; a different order
 * than gnnx_colsum_f32, so equal within rounding).  Any shape: what the fused kernel does not cover runs as three plain passes. */
int gnnx_gemm_relu_colsum_workspace(int64_t M, int64_t N, int64_t K, size_t *bytes);
int gnnx_gemm_relu_colsum_f32(int64_t M, int64_t N, int64_t K, const float *d_A, int64_t lda, const float *d_B, int64_t ldb,
                              const float *d_Ymask, int64_t ldy, float *d_C, int64_t ldc, float *d_colsum, void *d_workspace,
                              size_t workspace_bytes, void *stream);

/* OPT-IN (never the default; the parity path uses gnnx_gemm_f32 + gnnx_bn_stats_f32): H = X[M,K] . W[N,K]^T together with the
 * BatchNorm batch statistics of H's columns in ONE pass over H -- SURVEY.md 2b "BN statistics as the GEMM epilogue".  H holds the
 * same bits as gnnx_gemm_f32.  mean / var (biased) come from per-lane sums of d = h - shift[n] and d^2, shift = row 0 of H (a
 * sample value, so Q/M - (S/M)^2 cancels mildly), finished in double: a single-pass variance, within rounding of -- not bit-equal
 * to -- the exact two-pass statistics (x->mean(-2), x->var(-2, 0); reference nn.cpp:303,312).  Saves the two reads of H that
 * gnnx_bn_stats_f32 makes.  Shapes the fused kernel does not cover fall back to the exact pair of calls. */
int gnnx_gemm_bn_stats_workspace(int64_t M, int64_t N, int64_t K, size_t *bytes);
int gnnx_gemm_bn_stats_f32(int64_t M, int64_t N, int64_t K, const float *d_X, int64_t ldx, const float *d_W, int64_t ldw, float *d_H,
                           int64_t ldh, float *d_mean, float *d_var, void *d_workspace, size_t workspace_bytes, void *stream);

/* OPT-IN split-precision GEMM -- never the default, not used by any parity-graded call.  C[M,N] = A[M,K] . op(B)
 * (transB: B is [N,K], else [K,N]) on the bf16 matrix cores: every f32 operand is split exactly into three bf16 pieces
 * (8 + 8 + 8 significand bits: x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1), round to nearest even, subtractions in
 * f32) and the six piece products with i + j <= 2 are accumulated in f32, smallest first, at several times the f32 MFMA rate.
 * Not the reference's arithmetic.  What holds (tests/test_gpu_gemm_split.py):
 *   - accuracy: per element |C - A.op(B)| <= K * 2^-24 * sum_k |a_ik||b_kj| against float64, the worst case of an f32 chain of
 *     K roundings (measured worst: 1.2 .. 3.3 times 2^-24 * sum_k |a_ik||b_kj| for K = 16 .. 1024).  When every piece product
 *     and every partial sum of them is exact in f32 (integers with sum_k |a_ik||b_kj| < 2^24) the result is the exact product.
 *     A power-of-two scale of A or B scales C by the same factor, bit for bit, while operands, pieces, piece products and sums
 *     stay in the normal range.  transB = 0 and transB = 1 on the transposed B give the same bits.
 *   - range: finite operands below 2^127 * (2 - 2^-8).  A larger finite operand rounds to a bf16 infinity and behaves like one.
 *     An Inf or NaN in A makes exactly its row of C non-finite, one in B exactly its column (the split of an Inf has NaN pieces:
 *     whether such an element is NaN or Inf is unspecified); every other element is what it would be with that entry zero.
 *     An operand below 2^-103 in magnitude can have a subnormal second or third piece and may lose it: whether the bf16 matrix
 *     cores keep subnormal inputs has not been measured, and nothing is asserted about it.
 *   - status, checked in this order: a negative size GNNX_ERR_INVALID_ARG; M == 0 or N == 0 GNNX_OK with nothing read or written
 *     (null operands allowed); a null A, B or C GNNX_ERR_INVALID_ARG; K == 0, K % 16 != 0, N % 128 != 0, N or K >= 2^31, lda < K,
 *     lda % 4 != 0 or A not 16-byte aligned GNNX_ERR_UNSUPPORTED; ldb < K (transB) / ldb < N (else) or ldc < N GNNX_ERR_SHAPE; a
 *     workspace that is null, below gnnx_gemm_split_workspace() bytes (6 N K: the split copy of B) or not 16-byte aligned
 *     GNNX_ERR_WORKSPACE.  A refused call writes nothing.  B and C need no more than their 4-byte alignment, ldb and ldc may
 *     exceed their minimum by any amount; pad elements are neither read (A, B) nor written (C), nor are rows of C behind M. */
int gnnx_gemm_split_workspace(int64_t M, int64_t N, int64_t K, size_t *bytes);
int gnnx_gemm_split_bf16_f32(int transB, int64_t M, int64_t N, int64_t K, const float *d_A, int64_t lda, const float *d_B,
                             int64_t ldb, float *d_C, int64_t ldc, void *d_workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ small ops on the path -------- */
/* dbias: out[f] = beta*out[f] + sum_i G[i,f]  (Add::_backward -> sum_to_size, reference operation.h:114-128,
 * tensor.h:618-638).  Two-stage deterministic tree (fixed grid); workspace gnnx_colsum_workspace() bytes. */
int gnnx_colsum_workspace(int64_t n_rows, int32_t n_feat, size_t *bytes);
/* gnnx_colsum_copy_f32: the same sums (same bits) and, from the same pass, a copy of G's rows on another row stride: d_copy[i * ldc + f]
 * = G[i * ldg + f] -- the upstream gradient laid out for the backward aggregation's gather (gnnx_gather_row_stride).
 * gnnx_gather_row_stride: the row pitch (in floats) a matrix whose rows are GATHERED by the aggregation should be stored on:
 * n_feat, or n_feat + 64 when a row is a multiple of 512 bytes and the matrix is large -- with a power-of-two pitch the hub rows of
 * a synthetic power-law graph (vertex ids with few one-bits) pile onto a few memory channels (forward aggregation of RMAT 10 M /
 * 100 M, F = 256, vertices as generated: 17.8 ms on pitch 256, 13.9 ms on pitch 320; 13.8 ms after relabelling the vertices). */
/* gnnx_rows_to_slots_f32: the halo pack driven from the PRODUCER's side (the sharded step): d_slots[row][8] lists the
 * positions of `row` in the send buffer (packed to the front, -1 behind; a row goes to at most world - 1 <= 7 peers); every row is
 * read once and written to each of its slots: d_send[slot * ld_send + f] = d_X[row * ldx + f] -- the same send buffer the gather
 * pack (gnnx_gather_rows_f32 by the send list) fills.  d_colsum != NULL: the column sums of ALL rows from the same pass (out[f] =
 * beta * out[f] + sum_i X[i, f], the bits of gnnx_colsum_f32; workspace gnnx_colsum_workspace() bytes) -- the layer's dbias and the
 * pack of the upstream gradient in one read.  Rows of 16-byte pieces (n_feat % 4 == 0, n_feat / 4 a divisor of 256). */
int gnnx_rows_to_slots_f32(const float *d_X, int64_t ldx, int64_t n_rows, int32_t n_feat, const int32_t *d_slots, float *d_send,
                           int64_t ld_send, float *d_colsum, float beta, void *d_workspace, size_t workspace_bytes, void *stream);

/* gnnx_gemm_nt_rows_to_slots_f32: the sharded step's transform with the halo pack in the product's epilogue (the product
 * replaces nn::Linear::forward, /root/reference/src/nn.cpp:205-211, as gnnx_gemm_f32(0, 1, ...) does).  H[M][N] = X[M][K] . W[N][K]^T,
 * and every row of H listed in d_slots ([M][8], gnnx_rows_to_slots_f32's table) is ALSO stored to its send-buffer rows from the
 * registers the epilogue stores H from: the same bits in H and in d_send as gnnx_gemm_f32 followed by gnnx_rows_to_slots_f32, without
 * the pass that reads H back.  Shapes off the LDS-DMA kernel's grid (and the ragged last rows) run exactly those two calls.  Rows of
 * 16-byte pieces, as gnnx_rows_to_slots_f32.  Workspace: gnnx_gemm_nt_rows_to_slots_workspace() bytes (W^T).  As there, every listed
 * slot must be a row of d_send (the table is the caller's: gnnx_halo_plan_slot_table, or built like it) -- the kernels do not check. */
int gnnx_gemm_nt_rows_to_slots_workspace(int64_t M, int64_t N, int64_t K, size_t *bytes);
int gnnx_gemm_nt_rows_to_slots_f32(int64_t M, int64_t N, int64_t K, const float *d_X, int64_t ldx, const float *d_W, int64_t ldw,
                                   float *d_H, int64_t ldh, const int32_t *d_slots, float *d_send, int64_t ld_send,
                                   void *d_workspace, size_t workspace_bytes, void *stream);
int gnnx_gather_row_stride(int64_t n_rows, int32_t n_feat, int64_t *ld_out);
int gnnx_colsum_copy_f32(const float *d_G, int64_t ldg, int64_t n_rows, int32_t n_feat, float beta, float *d_out, float *d_copy,
                         int64_t ldc, void *d_workspace, size_t workspace_bytes, void *stream);
int gnnx_colsum_f32(const float *d_G, int64_t ldg, int64_t n_rows, int32_t n_feat, float beta, float *d_out,
                    void *d_workspace, size_t workspace_bytes, void *stream);

/* Unfused forms of the epilogues, for callers that go op by op through the tensor API:
 *   rowscale: Y[i,:] = X[i,:] * v[i]      ([N,F] (.) [N,1], reference functional.h:190-213 + utils.h:181-228)
 *   bias    : Y[i,:] = X[i,:] + b[:]      ([N,F] + [F],     reference functional.h:163-187)
 *   axpy    : y += a * x                  (tensor.h:268-271 `_grad +=`, a = 1)
 * X and Y may alias. */
int gnnx_rowscale_f32(const float *d_X, int64_t ldx, const float *d_v, int64_t n_rows, int32_t n_feat, float *d_Y,
                      int64_t ldy, void *stream);
int gnnx_bias_add_f32(const float *d_X, int64_t ldx, const float *d_b, int64_t n_rows, int32_t n_feat, float *d_Y,
                      int64_t ldy, void *stream);
int gnnx_axpy_f32(int64_t n, float a, const float *d_x, float *d_y, void *stream);

/* General 2-D broadcast of the API's elementwise operators (operator+ - * / on tensors: reference tensor.h:30-77 ->
 * functional.h:163-239, broadcast rule utils.h:181-228):  Y[r][c] = A[r*a_row_stride + c*a_col_stride] (op)
 * B[r*b_row_stride + c*b_col_stride], a stride of 0 broadcasts that dimension ([N,F] op [N,1], [N,F] op [F],
 * [N,F] op scalar, either side).  Each element is rounded once (IEEE add / sub / mul / div).  Y may alias A or B when
 * the aliased operand is not broadcast.  rowsum is the reduction that undoes a column broadcast in backward
 * (sum_to_size to [N,1], tensor.h:618-638): out[r] = sum_c X[r][c]. */
enum { GNNX_OP_ADD = 0, GNNX_OP_SUB = 1, GNNX_OP_MUL = 2, GNNX_OP_DIV = 3 };
int gnnx_binary_bcast_f32(int op, int64_t n_rows, int64_t n_cols, const float *d_A, int64_t a_row_stride, int64_t a_col_stride,
                          const float *d_B, int64_t b_row_stride, int64_t b_col_stride, float *d_Y, int64_t ldy, void *stream);
int gnnx_rowsum_f32(const float *d_X, int64_t ldx, int64_t n_rows, int32_t n_cols, float *d_out, void *stream);

/* Elementwise helpers behind the tensor API mirror (gnn.cpp_amd/host/):
 *   fill      : x[i] = value                                   (tensor(dims, value) ctor, reference tensor.h:106)
 *   pow       : y[i] = pow(x[i], e).  The reference's pow is the HOST libm's powf (functional.h:253) and its one use on the path is
 *               deg->pow(-0.5) on the degrees (graph.cpp:183): when every x[i] is an integer in [0, 2^24] the result is looked up in a
 *               table of that libm call (table[k] = powf(k, e), built on the host: one synchronisation, a graph-build call) -- the
 *               reference's bits; any other argument vector is evaluated on the device (e == -0.5: correctly rounded 1/sqrt)
 *   csr_rowsum: out[i] = sum_j A_ij = rowptr[i+1]-rowptr[i] (vals == NULL) -- adj_mat->sum(-1,true), reference
 *               graph.cpp:178 -> functional.h:267-296, without the dense N x N matrix
 *   transpose : Y[c,r] = X[r,c]  (materialises a 2-D transpose only when a caller insists on the data;
 *               the GEMM never needs it).  X and Y must not alias.  Tall and wide matrices alike: all 32 x 32 tiles ride on grid.x;
 *               more than 2^31 - 1 tiles (over 8 TB of floats) is GNNX_ERR_UNSUPPORTED. */
int gnnx_fill_f32(float *d_x, int64_t n, float value, void *stream);
int gnnx_pow_f32(const float *d_x, int64_t n, float exponent, float *d_y, void *stream);
int gnnx_csr_rowsum_f32(const int32_t *d_rowptr, const float *d_vals, int32_t n_rows, float *d_out, void *stream);
int gnnx_transpose_f32(const float *d_X, int64_t ldx, int64_t n_rows, int64_t n_cols, float *d_Y, int64_t ldy, void *stream);

/* ------------------------------------------------------------------ next row: BatchNorm + ReLU ---- */
/*
 * The pair that sits between transform and aggregation inside GCNConv::forward (reference graph.cpp:174-175):
 *   BatchNorm::forward (nn.cpp:301-330, training mode): mean = x->mean(-2,true); var = x->var(-2, 0, true);
 *       y = ((x - mean) / (var + eps)->pow(0.5)) * gammas + betas     (running stats are never really updated in the
 *       reference: they are assigned to temporaries, nn.cpp:323-324)
 *   ReLU::forward (nn.cpp:229-237): where(x > 0, x, 0)
 * stats : d_mean[F], d_var[F] (biased variance).   fwd: d_mean/d_var may both be NULL (ReLU only); gamma / beta may be NULL.
 * bwd   : mathematically correct gradients (the reference's own drop fan-in contributions, operation.h:82-86):
 *         g = dY (.) (Y > 0);  dbeta = colsum g;  dgamma = colsum g (.) xhat;  dX = gamma/sigma (.) (g - dbeta/N - xhat (.) dgamma/N).
 *         d_Y (the forward output) is only read when relu != 0; d_Y == NULL with relu != 0 redoes the forward arithmetic on
 *         x (with d_beta) to find the sign -- the backward of a fused forward (gnnx_spmm_csr_fused_f32), where the rectified
 *         activations were never stored.  d_beta is read for that only.  Workspace: gnnx_bn_workspace() bytes.
 */
int gnnx_bn_workspace(int64_t n_rows, int32_t n_feat, size_t *bytes);
int gnnx_bn_stats_f32(const float *d_X, int64_t ldx, int64_t n_rows, int32_t n_feat, float *d_mean, float *d_var,
                      void *d_workspace, size_t workspace_bytes, void *stream);
int gnnx_bn_relu_fwd_f32(const float *d_X, int64_t ldx, int64_t n_rows, int32_t n_feat, const float *d_mean, const float *d_var,
                         float eps, const float *d_gamma, const float *d_beta, int relu, float *d_Y, int64_t ldy, void *stream);
int gnnx_bn_relu_bwd_f32(const float *d_X, int64_t ldx, const float *d_Y, int64_t ldy, const float *d_dY, int64_t ldd, int64_t n_rows,
                         int32_t n_feat, const float *d_mean, const float *d_var, float eps, const float *d_gamma, const float *d_beta,
                         int relu, float *d_dX, int64_t ldo, float *d_dgamma, float *d_dbeta, void *d_workspace,
                         size_t workspace_bytes, void *stream);
/* Cross-shard BatchNorm: the batch is the whole graph, a rank holds n_rows of its n_total rows.
 *   partial : d_out[f] = scale * sum_i x_if (d_mean == NULL), or scale * sum_i (x_if - d_mean[f])^2.  With scale = 1 / n_total an
 *             all-reduce of the first gives the global mean, then an all-reduce of the second (against the GLOBAL mean) the global
 *             biased variance: the exact two-pass arithmetic of gnnx_bn_stats_f32, two [F] vectors on the wire per layer.
 *   bwd_sums / bwd_apply : the two halves of gnnx_bn_relu_bwd_f32 -- local dgamma / dbeta sums, then (after the caller's
 *             all-reduce of those two [F] vectors) dX with the global sums and n_total. */
/* OPT-IN reference-quirk backward: dgamma / dbeta as above, dX = (g * gamma) / (var + eps)^0.5 with the batch statistics treated
 * as constants.  That is what the REFERENCE's own backward delivers through BatchNorm: an op that has completed its backward drops
 * every later arrival (operation.h:80-88) and BatchNorm's input has three consumers (x - mean, mean, var; nn.cpp:301-316), so only
 * the first, direct path (Mul::_backward operation.h:159-164 -> Div::_backward :192-198) reaches the transform.  Pinned against
 * the reference's through-layer gradients (tests/golden ref_full_*); exists only to compare with them, never the default. */
int gnnx_bn_relu_bwd_quirk_f32(const float *d_X, int64_t ldx, const float *d_Y, int64_t ldy, const float *d_dY, int64_t ldd,
                               int64_t n_rows, int32_t n_feat, const float *d_mean, const float *d_var, float eps, const float *d_gamma,
                               const float *d_beta, int relu, float *d_dX, int64_t ldo, float *d_dgamma, float *d_dbeta,
                               void *d_workspace, size_t workspace_bytes, void *stream);
int gnnx_bn_partial_f32(const float *d_X, int64_t ldx, int64_t n_rows, int32_t n_feat, const float *d_mean, float scale, float *d_out,
                        void *d_workspace, size_t workspace_bytes, void *stream);
int gnnx_bn_relu_bwd_sums_f32(const float *d_X, int64_t ldx, const float *d_Y, int64_t ldy, const float *d_dY, int64_t ldd,
                              int64_t n_rows, int32_t n_feat, const float *d_mean, const float *d_var, float eps, const float *d_gamma,
                              const float *d_beta, int relu, float *d_dgamma, float *d_dbeta, void *d_workspace, size_t workspace_bytes,
                              void *stream);
int gnnx_bn_relu_bwd_apply_f32(const float *d_X, int64_t ldx, const float *d_Y, int64_t ldy, const float *d_dY, int64_t ldd,
                               int64_t n_rows, int32_t n_feat, const float *d_mean, const float *d_var, float eps, const float *d_gamma,
                               const float *d_beta, int relu, const float *d_dgamma, const float *d_dbeta, int64_t n_total, float *d_dX,
                               int64_t ldo, void *d_workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ next row: loss + optimiser ---- */
/*
 * Softmax cross-entropy on the last layer's logits and the SGD update, so a multi-layer GCN runs as a whole training
 * step on the device.
 *   loss    = mean_i -log( exp(x_i[t_i]) / (sum_c exp(x_ic) + 1e-20) )     the reference's forward, nn.cpp:442-453
 *             (no max-subtraction, like the reference); d_loss: one float on the device (may be NULL)
 *   dlogits = (softmax(x_i) - onehot(t_i)) / N                             textbook (the reference's backward throws);
 *             may be NULL.  Synchronises `stream` (validates the targets: GNNX_ERR_INDEX_RANGE).
 *   One kernel set serves these calls and gnnx_softmax_ce_rows_f32 below (the loss over a row list); each *_workspace query is the
 *   layout its call then uses, and the workspace pointer may have any alignment -- for gnnx_softmax_ce_f32, _colsum_f32, _partial_f32
 *   and gnnx_softmax_ce_rows_f32 (the query includes the room to round the pointer up; no byte outside the queried size is touched).
 *   gnnx_bce_logits_f32 takes its workspace pointer as it is: 4-byte aligned.
 *   Non-finite logits (there is no max-subtraction, so x >= 89 overflows expf like +inf): no error status.  The row's own
 *   gradient row and the loss become non-finite (the column sums of the classes it poisons too); every other gradient row has the bits
 *   it has without the poisoned row.  A -inf logit off the target is an ordinary dead class (probability 0, gradient +0).  A row whose
 *   target's exp is 0 has an infinite row loss and the gradient p - onehot as usual; a FULLY dead row (every exp 0: the sum is 0, the
 *   denominator 1e-20) gives exactly -onehot / n_total.
 *   Error bounds against float64, u = 2^-24, p = softmax, d = onehot (tests/test_gpu_loss.py holds every form to them):
 *     gradient     |dlogits - (p - d) / n_total| <= (S + 8) u (p + d) / n_total
 *     column sums  |colsum - exact|              <= (S + 8 + n_listed) u sum_i (p + d) / n_total
 *     loss         |loss - exact|                <= u [(S + 4) n_listed + (ceil(n_listed / 65536) + 266) sum_i |l_i|] / n_total
 *   S = additions on the path of a row sum: 4 ceil(C / 256) + 6 on the vector form (C % 4 == 0, C <= 1024, ldx % 4 == 0, ldd % 4 == 0,
 *   logits and dlogits 16-byte aligned), ceil(C / 64) + 6 otherwise.  Worst ratios error / (u * scale) observed on an MI355X: gradient
 *   5.3 (vector) / 5.4 (generic) against S + 8 >= 15; column sums 5.4 / 4.4; loss 3.5 / 3.2 times u sum |l_i| / n_total, 1.3 % of its bound.
 *   On inputs where nothing rounds (logits 0 or dead, 1 / 2 / 4 / 8 live classes a row, n_total a power of two) dlogits and the column
 *   sums are exact on every path.
 *   sgd     : p -= lr * (g + weight_decay * p)                             textbook (nn.cpp:395-421 indexes an empty vector)
 */
int gnnx_softmax_ce_workspace(int64_t n_rows, size_t *bytes);
int gnnx_softmax_ce_f32(const float *d_logits, int64_t ldx, const int32_t *d_target, int64_t n_rows, int32_t n_classes, float *d_loss,
                        float *d_dlogits, int64_t ldd, void *d_workspace, size_t workspace_bytes, void *stream);
/* The same with the column sums of dlogits -- the last layer's bias gradient (operation.h:114-128 sum_to_size on the Add node's
 * bias operand, reached with dlogits as the incoming gradient) -- accumulated by the kernel that writes dlogits instead of one more
 * pass over them.  d_colsum [n_classes] may be NULL (then exactly gnnx_softmax_ce_f32).  Deterministic (fixed summation order);
 * the order differs from gnnx_colsum_f32's, so the two agree to rounding. */
int gnnx_softmax_ce_colsum_workspace(int64_t n_rows, int32_t n_classes, size_t *bytes);
int gnnx_softmax_ce_colsum_f32(const float *d_logits, int64_t ldx, const int32_t *d_target, int64_t n_rows, int32_t n_classes,
                               float *d_loss, float *d_dlogits, int64_t ldd, float *d_colsum, void *d_workspace,
                               size_t workspace_bytes, void *stream);
/* A shard's share (1-D vertex partition): n_rows local rows of a batch of n_total; d_loss is this rank's term of the mean (the caller
 * sums the ranks' terms), dlogits and the column sums carry 1 / n_total.  n_total == n_rows is gnnx_softmax_ce_colsum_f32. */
int gnnx_softmax_ce_partial_f32(const float *d_logits, int64_t ldx, const int32_t *d_target, int64_t n_rows, int32_t n_classes,
                                int64_t n_total, float *d_loss, float *d_dlogits, int64_t ldd, float *d_colsum, void *d_workspace,
                                size_t workspace_bytes, void *stream);
int gnnx_sgd_step_f32(float *d_param, const float *d_grad, int64_t n, float lr, float weight_decay, void *stream);
/* Binary cross-entropy on logits -- the loss over scored pairs (link prediction: the inner-product decoder of the graph
 * auto-encoder scores a pair with gnnx_sddmm_csr_f32; the reference has no counterpart, its one loss is nn.cpp:442-453):
 *   loss       = (1 / n_total) sum_p [ max(x_p, 0) - x_p y_p + log1p(exp(-|x_p|)) ]    the stable form: no inf / NaN for any finite x
 *   dscores[p] = (sigmoid(x_p) - y_p) / n_total
 * d_target is float: soft labels are allowed.  n_total >= n is the divisor (n on one GPU).  d_loss (one device float) and d_dscores
 * [n] may each be NULL.  The sum is two-stage on a fixed grid in a fixed order (as gnnx_colsum_f32): the same bits on every run.
 * Asynchronous.  n == 0 is GNNX_ERR_INVALID_ARG, never a NaN loss (as gnnx_softmax_ce_rows_f32).  Workspace:
 * gnnx_bce_logits_workspace() bytes, 4-byte aligned, needed only with d_loss; both outputs NULL: GNNX_OK, nothing is touched.
 * Against float64 (tests/test_gpu_loss.py): |dscores - exact| <= 6 * 2^-24 (sigmoid + y) / n_total (observed 3.4) wherever sigmoid(x)
 * is a normal f32 number; exact on scores of +-128 / +-256 with targets 0, 1, 0.25 and n_total a power of two, loss included. */
int gnnx_bce_logits_workspace(int64_t n, size_t *bytes);
int gnnx_bce_logits_f32(const float *d_scores, const float *d_target, int64_t n, int64_t n_total, float *d_loss, float *d_dscores,
                        void *d_workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ optimisers over a parameter table ---- */
/*
 * Adam / AdamW, SGD with momentum and the global gradient norm (clipping) for ALL parameter tensors of a model in one launch.  A
 * model's parameters are many small tensors; a launch per tensor is what a step costs, so the tensors are listed once in a TABLE
 * in device memory and a step is one workgroup of 256 threads per chunk of 1024 elements, whatever the number of tensors.
 *
 *   gnnx_optim_table_bytes   size of the table for n_tensors tensors.
 *   gnnx_optim_table_build   fills d_table (8-byte aligned, >= the queried size: GNNX_ERR_WORKSPACE) from HOST arrays of n_tensors
 *                       device pointers (parameter, gradient; 4-byte aligned) and element counts; copies it to the device and
 *                       synchronises `stream` (a build call).  Per tensor the table holds the two pointers, the count and the offset
 *                       of the tensor's state in ONE flat state arena of *state_elems_out floats that the caller owns (zeroed before
 *                       the first step; Adam has two such arenas, m and v); offsets are rounded up to 4 elements, so on a 16-byte
 *                       aligned arena every tensor's state is 16-byte aligned.  Behind the entries: int32 first[n_tensors + 1], the
 *                       running chunk count (a workgroup finds its tensor by binary search).  A tensor of size 0 is legal and has no
 *                       chunk (its pointers may be NULL).  *n_chunks_out = the total chunk count = the grid of a step; 2^31 chunks or
 *                       more: GNNX_ERR_UNSUPPORTED.  Every check precedes the first HIP call.  The table stays valid while the
 *                       tensors stay where they are.
 *   gnnx_adam_step_f32 / gnnx_momentum_step_f32   one launch, n_chunks workgroups (n_chunks: what the build returned; workgroups
 *                       past the table's own count return at once, a smaller count leaves the last chunks alone).  A chunk runs on
 *                       16-byte lanes where its parameter, gradient and state addresses are all 16-byte aligned and on scalar lanes
 *                       otherwise, its tail on scalar lanes either way.  No host synchronisation, no copy, no atomics: capturable.
 *                       d_gscale (may be NULL): one device float every gradient is multiplied with -- gnnx_grad_sqnorm_f32's.
 *   gnnx_grad_sqnorm_f32     *d_sqnorm = sum of g^2 over every gradient of the table: a fixed grid of 256 workgroups strides the
 *                       chunks, thread i adds elements i, i + 256, i + 512, i + 768 of each of its chunks in that order (scalar loads
 *                       whatever the alignment), a fixed tree folds the workgroup, a second stage adds the 256 partials in order: the
 *                       same bits on every run.  The second stage also writes *d_gscale = min(1, max_norm / (sqrtf(sq) + 1e-6f))
 *                       (torch's clip_grad_norm_): clipping never visits the host.  Either output may be NULL.  Workspace:
 *                       gnnx_grad_sqnorm_workspace() bytes, 4-byte aligned.
 *   gnnx_adam_bias_corrections   HOST only, no device: *c = (float)(1.0 - pow((double)b, (double)t)) for both betas, t >= 1 the number
 *                       of the step about to be taken.  Every caller gets its two floats here; the step is a pure function of its
 *                       arguments.
 *
 * The arithmetic is the contract: every line is ONE float32 operation with one rounding (nothing is contracted to an fma), division
 * and sqrtf correctly rounded, float32 denormals kept.
 *     g1 = g * s                       only with d_gscale (s = *d_gscale)
 *     g2 = g1 + wd * p                 only when wd != 0 and the decay is coupled (product rounded, then the sum; as gnnx_sgd_step_f32)
 *   Adam:      m' = b1 * m + (1.0f - b1) * g2
 *              v' = b2 * v + ((1.0f - b2) * g2) * g2
 *              u  = (m' / c1) / (sqrtf(v' / c2) + eps)
 *              p1 = p - (lr * wd) * p          only when decoupled and wd != 0 (AdamW)
 *              p' = p1 - lr * u
 *   momentum:  buf' = g2 if first else momentum * buf + (1.0f - dampening) * g2
 *              d    = g2 + momentum * buf' if nesterov else buf'
 *              p'   = p - lr * d
 * With momentum == 0, dampening == 0 and no scale the momentum call gives the bits of gnnx_sgd_step_f32 (g = -0, an infinite p and
 * wd == 0, where the decay term is skipped, included) -- with `first` for every input; without it on a +0 buffer for every input but
 * p = -0 with g2 = -0 (0 * buf + g2 is +0 there: p' = -0 where gnnx_sgd_step_f32 gives +0).  Subnormal intermediates are outside the
 * contract.  A zero gradient on zero state leaves p as it is and m, v at +0 (zero pad columns stay zero without weight decay, and
 * with it: wd * 0 = 0).
 * Non-finite gradients: no error status.  Without a scale a NaN or Inf gradient element changes its own element of p, m and v (or
 * buf) and no other bit.  With clipping it poisons the norm: a NaN makes the scale NaN and with it every element; an Inf makes the
 * scale 0, so every finite gradient counts as 0 and the infinite one as NaN.
 * GNNX_ERR_INVALID_ARG before any HIP call: a null table / arena / output, a negative count, b1 or b2 outside [0, 1), eps <= 0,
 * c1 or c2 <= 0, t < 1, a negative max_norm.
 */
int gnnx_optim_table_bytes(int32_t n_tensors, size_t *bytes);
int gnnx_optim_table_build(int32_t n_tensors, float *const *h_params, const float *const *h_grads, const int64_t *h_sizes, void *d_table,
                           size_t table_bytes, int64_t *n_chunks_out, int64_t *state_elems_out, void *stream);
int gnnx_adam_bias_corrections(float b1, float b2, int64_t t, float *c1, float *c2);
int gnnx_adam_step_f32(const void *d_table, int32_t n_tensors, int64_t n_chunks, float *d_m, float *d_v, float lr, float b1, float b2,
                       float eps, float c1, float c2, float weight_decay, int decoupled, const float *d_gscale, void *stream);
int gnnx_momentum_step_f32(const void *d_table, int32_t n_tensors, int64_t n_chunks, float *d_buf, float lr, float momentum, float dampening,
                           int nesterov, int first, float weight_decay, const float *d_gscale, void *stream);
int gnnx_grad_sqnorm_workspace(size_t *bytes);
int gnnx_grad_sqnorm_f32(const void *d_table, int32_t n_tensors, float max_norm, float *d_sqnorm, float *d_gscale, void *d_workspace,
                         size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ semi-supervised training: masks ---- */
/*
 * Node classification with a label mask (reference include/graph.h:86-94 / src/graph.cpp:130-151: Data::set_mask with a train, a
 * validation and a test mask over the vertices; functional.h:59-61: argmax).  A mask is one byte per vertex (non-zero = in the set);
 * the compute calls take the set as an ascending list of row ids.
 *
 *   gnnx_mask_to_rows   d_rows[k] = the k-th non-zero position of d_mask[0..n), ascending (capacity n int32); *n_rows_out: HOST, valid
 *                       on return (synchronises `stream`).
 *   gnnx_csr_restrict   the CSR with the SAME number of rows that keeps entry (r, c) iff d_row_keep[r] != 0 (when given) and
 *                       d_col_keep[c] != 0 (when given); rows that lose everything become empty; surviving entries keep their STORED
 *                       ORDER inside the row -- the summation order of the aggregation, also on a relabelled graph whose rows are
 *                       sorted by original column id.  nnz = rowptr[n_rows] (checked); d_colidx_out / d_vals_out have capacity nnz;
 *                       d_vals / d_vals_out both or neither; both masks NULL is a copy; not in place.  *nnz_out: HOST, valid on
 *                       return (synchronises).  GNNX_ERR_INDEX_RANGE: a column id outside [0, n_cols) met under a column mask.
 *                       With a train mask the last GCN layer aggregates on the row-restricted CSR(A) forward and on the
 *                       column-restricted CSR(A^T) backward: every dropped term of a kept accumulator is norm * 0, so the kept rows
 *                       and the whole backward product have the bits of the full aggregation.
 *   gnnx_softmax_ce_rows_f32  the loss of gnnx_softmax_ce_f32 (reference forward nn.cpp:442-453) over the listed rows:
 *                       loss = (sum_{i in rows} -log(exp(x_i[t_i]) / (sum_c exp(x_ic) + 1e-20))) / n_total;
 *                       dlogits[i,:] = (softmax(x_i) - onehot(t_i)) / n_total for LISTED rows only -- every other row of the buffer
 *                       is left as it is (the caller zeroes it once); d_colsum [n_classes] (may be NULL) = column sums of those
 *                       gradient rows, fixed order.  n_total >= n_listed is the divisor (n_listed on one GPU; the labelled count of
 *                       the whole batch on a shard).  d_rows: ascending, no repeats, each in [0, n_rows).  Targets are read at listed
 *                       rows only (-1 elsewhere is fine).  The kernels, grids and summation orders of gnnx_softmax_ce_colsum_f32
 *                       behind the list: listing every row gives its loss, dlogits and column-sum bits.  Cost O(n_listed), not
 *                       O(n_rows).
 *                       Synchronises.  GNNX_ERR_INDEX_RANGE: a target outside [0, n_classes) at a listed row, or a listed row
 *                       outside [0, n_rows); GNNX_ERR_INVALID_ARG: n_listed == 0 (never a NaN loss).
 *   gnnx_argmax_rows_f32      d_pred[i] = the FIRST index of the maximum of row i (functional.h:59-61), every row.
 *   gnnx_accuracy_rows_f32    *correct_out (HOST) = number of listed rows (d_rows NULL: all n_rows rows, n_listed == n_rows) whose
 *                       argmax equals the target (a target outside the classes never matches); d_pred (may be NULL): the class of
 *                       the k-th listed row at d_pred[k].  Both synchronise.  A row with a NaN gives some in-range class
 *                       (unspecified which).
 */
int gnnx_mask_to_rows_workspace(int64_t n, size_t *bytes);
int gnnx_mask_to_rows(const uint8_t *d_mask, int64_t n, int32_t *d_rows, int32_t *n_rows_out, void *d_workspace, size_t workspace_bytes,
                      void *stream);
int gnnx_csr_restrict_workspace(int32_t n_rows, int64_t nnz, size_t *bytes);
int gnnx_csr_restrict(int32_t n_rows, int32_t n_cols, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx, const float *d_vals,
                      const uint8_t *d_row_keep, const uint8_t *d_col_keep, int32_t *d_rowptr_out, int32_t *d_colidx_out,
                      float *d_vals_out, int64_t *nnz_out, void *d_workspace, size_t workspace_bytes, void *stream);
int gnnx_softmax_ce_rows_workspace(int64_t n_listed, int32_t n_classes, size_t *bytes);
int gnnx_softmax_ce_rows_f32(const float *d_logits, int64_t ldx, const int32_t *d_target, const int32_t *d_rows, int64_t n_listed,
                             int64_t n_rows, int32_t n_classes, int64_t n_total, float *d_loss, float *d_dlogits, int64_t ldd,
                             float *d_colsum, void *d_workspace, size_t workspace_bytes, void *stream);
int gnnx_argmax_rows_workspace(size_t *bytes);
int gnnx_argmax_rows_f32(const float *d_logits, int64_t ldx, int64_t n_rows, int32_t n_classes, int32_t *d_pred, void *d_workspace,
                         size_t workspace_bytes, void *stream);
int gnnx_accuracy_rows_f32(const float *d_logits, int64_t ldx, const int32_t *d_target, const int32_t *d_rows, int64_t n_listed,
                           int64_t n_rows, int32_t n_classes, int32_t *d_pred, int64_t *correct_out, void *d_workspace,
                           size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ query inference: receptive fields ---- */
/*
 * Logits for a vertex set from its L-hop field instead of a forward over every vertex.  The reference's layer (src/graph.cpp:170-191) is
 * Y_l = act(norm (.) (A . (Y_{l-1} W_l^T)) + b_l) with the diagonal of A zeroed (graph.cpp:68-75, :172: a vertex is not its own
 * neighbour), so rows Q_l of Y_l need Y_{l-1} only on Q_{l-1} = the columns stored in rows Q_l of CSR(A); Q_L is the query -- e.g. a
 * validation or test mask (graph.cpp:130-151 Data::set_mask) evaluated every epoch.  Layer l then runs on compact matrices: the block
 * of A with rows Q_l and columns Q_{l-1}, norm on Q_l, and X rows Q_0 as the only input read.  Every Q_l is an ASCENDING row list and a
 * row's compact id is its position in the list; a block keeps each row's entries in STORED ORDER, every aggregation kernel walks a
 * row in stored order with one accumulator per output element, and every row-parallel product is one k-ascending fmaf chain per
 * output element: the compact layers give the bits of the full forward on the listed rows.
 *
 *   gnnx_frontier_mark      d_mark[c] = 1 for every column c stored in the listed rows (one byte per column, n_cols bytes; bytes of
 *                           other columns are left as they are: the caller zeroes the mask, or keeps marks to form a union).
 *                           *nnz_listed_out (HOST) = the number of entries of the listed rows.  gnnx_mask_to_rows turns the mask into
 *                           the ascending list Q_{l-1}.
 *   gnnx_rows_to_positions  d_pos[0..n) = -1 ("not in the set"), then d_pos[d_rows[k]] = k.
 *   gnnx_csr_extract_rows   the CSR of the n_listed listed rows: d_rowptr_out [n_listed + 1] = exclusive scan of their lengths;
 *                           d_colidx_out[p] = d_col_pos[c] for the entries' columns c in stored order (d_col_pos NULL: c itself; else
 *                           a position table over [0, n_cols)); d_vals_out carried along when d_vals is given (both or neither).
 *                           *nnz_out (HOST) = the entries of the listed rows -- set even when nnz_capacity (the capacity of
 *                           d_colidx_out / d_vals_out in entries) is too small, which is GNNX_ERR_INVALID_ARG with nothing written,
 *                           never a truncated CSR.  n_listed == 0 is a valid result: d_rowptr_out = [0].
 *
 * d_rows: ascending, no repeats, each in [0, n_rows) -- checked on the device, GNNX_ERR_INDEX_RANGE otherwise.  A stored column outside
 * [0, n_cols), or one whose position is "not in the set", is GNNX_ERR_INDEX_RANGE, never a wrong index.  Negative sizes are
 * GNNX_ERR_INVALID_ARG before any device is touched.  Work is dealt in the non-zero domain of the LISTED rows (scan of the listed
 * lengths, 64 entries per wavefront, owning row by search): a hub row is spread over many wavefronts.  Cost O(n_listed + entries of
 * the listed rows), plus the O(n) fill of gnnx_rows_to_positions; nothing is O(nnz of the graph).  All three synchronise `stream`.
 */
int gnnx_frontier_mark_workspace(int64_t n_listed, size_t *bytes);
int gnnx_frontier_mark(const int32_t *d_rowptr, const int32_t *d_colidx, int32_t n_rows, int32_t n_cols, const int32_t *d_rows,
                       int64_t n_listed, uint8_t *d_mark, int64_t *nnz_listed_out, void *d_workspace, size_t workspace_bytes,
                       void *stream);
int gnnx_rows_to_positions_workspace(size_t *bytes);
int gnnx_rows_to_positions(const int32_t *d_rows, int64_t n_listed, int64_t n, int32_t *d_pos, void *d_workspace, size_t workspace_bytes,
                           void *stream);
int gnnx_csr_extract_rows_workspace(int64_t n_listed, size_t *bytes);
int gnnx_csr_extract_rows(int32_t n_rows, int32_t n_cols, const int32_t *d_rowptr, const int32_t *d_colidx, const float *d_vals,
                          const int32_t *d_rows, int64_t n_listed, const int32_t *d_col_pos, int32_t *d_rowptr_out,
                          int32_t *d_colidx_out, float *d_vals_out, int64_t nnz_capacity, int64_t *nnz_out, void *d_workspace,
                          size_t workspace_bytes, void *stream);
/* gnnx_csr_renumber_cols: d_colidx[q] = d_pos[d_colidx[q]] IN PLACE for q in [0, nnz) -- the columns of a block that was made with
 * original column ids (gnnx_csr_sample_rows) become positions in a row list through its position table (gnnx_rows_to_positions over
 * [0, n_cols)).  A column outside [0, n_cols), or one whose position is -1, is GNNX_ERR_INDEX_RANGE; such entries are then -1, every
 * other entry is renumbered: never a wrong index.  The workspace is a fixed 256 bytes at any address (no query, as for
 * gnnx_csr_sample_negatives); nnz == 0 returns GNNX_OK and touches nothing.  Synchronises `stream`. */
int gnnx_csr_renumber_cols(int64_t nnz, int32_t *d_colidx, const int32_t *d_pos, int64_t n_cols, void *d_workspace, size_t workspace_bytes,
                           void *stream);

/* ------------------------------------------------------------------ edge scores (SDDMM) ---------- */
/*
 * A value per STORED entry from the two endpoint rows -- the other half of message passing (the aggregation is a row per vertex from
 * its entries):
 *   out[p] = (dot_p * rowscale[i]) * colscale[c_p],   dot_p = <L[i,:], R[c_p,:]>   for entry p of row i of the CSR pattern.
 * Each scale is skipped when NULL; each multiply is rounded on its own.  L: [n_rows, F] ld ldl.  R: [n_cols, F] ld ldr.  out: [nnz].
 * Asynchronous on `stream`; nothing is allocated or synchronised.  The CSR and nnz (= rowptr[n_rows]) are TRUSTED, as the
 * aggregation trusts its CSR (gnnx_csr_validate is the check).  d_out aliases nothing; L == R is allowed (link scores <z_i, z_c>).
 * n_feat == 0 writes +0 to d_out; nnz == 0 is GNNX_OK with no launch.  Null pointers, negative sizes and ld < F are
 * GNNX_ERR_INVALID_ARG before any device call.
 *
 * The ORDER of dot_p is a function of F alone (every operation separately rounded fp32; -ffp-contract=off):
 *   - Split the row into Q = ceil(F/4) chunks.  Chunk q holds features 4q .. min(4q+3, F-1).
 *   - G is the smallest power of two with G >= Q, capped at 64 (F <= 4 gives G = 1).
 *   - Lane l < G starts from +0.  For q = l, l+G, l+2G, ... < Q, and within a chunk in ascending f, it does
 *     acc_l = acc_l + (L[i,f] * R[c,f]).  The product is rounded first, then the sum.
 *   - A lane with no chunk holds +0.
 *   - For s = 1, 2, 4, ..., G/2, every lane does acc_l = acc_l + acc_{l xor s}.  IEEE addition is commutative, so all lanes end
 *     with the same bits.
 *   - dot_p = acc_0.
 * This is a vec4 lane group: F = 256 is one wavefront per entry with one 16-byte load per lane, F = 128 two entries per wavefront.
 * The order does not depend on alignment: rows that fail the vec4 conditions (F % 4 != 0, a pointer or ld not 16-byte aligned) take
 * scalar loads with the same feature-to-lane assignment and give the same bits.  tests/sddmm_ref.py restates the order in NumPy and
 * the GPU tests hold the kernel to it bit for bit.  Work is dealt in the non-zero domain (a fixed number of entries per wavefront,
 * the owning row by a search in rowptr): a hub row spreads over the device, no plan.
 *
 * Second use -- the gradient of the aggregation's per-entry values: for Y = rowscale (.) sum_p vals[p] * colscale[c_p] * X[c_p,:]
 * (gnnx_spmm_csr_f32) with upstream gradient G,
 *   dL/dvals = gnnx_sddmm_csr_f32(L = G, R = X, rowscale, colscale).
 * The reference computes this gradient as the dense N x N product G . X^T (MatMul::_backward, reference operation.h:516-523); on a CSR
 * adjacency only the stored entries exist, and the product restricted to them is this call.
 *
 * gnnx_csr_transpose_map: for entry q = (c, r) of CSR(A^T), map_t[q] = the position p of (r, c) in CSR(A), found by binary search
 * in row r.  Both CSRs must have ascending columns and no duplicates (what the COO builds produce).  Built once per pattern;
 * synchronises `stream`.  GNNX_ERR_INDEX_RANGE -- never a wrong index -- when an entry has no partner, a row is not strictly ascending
 * (e.g. a relabelled graph stored in original-id order), or rowptr[n_rows], rowptr_t[n_cols] and nnz disagree.  Per-entry values move
 * to the transposed order with a 1-column gather: gnnx_gather_rows_f32(vals as [nnz, 1], map_t, n_feat = 1).
 */
int gnnx_sddmm_csr_f32(int32_t n_rows, int32_t n_cols, int32_t n_feat, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx,
                       const float *d_L, int64_t ldl, const float *d_R, int64_t ldr, const float *d_rowscale, const float *d_colscale,
                       float *d_out, void *stream);
int gnnx_csr_transpose_map(int32_t n_rows, int32_t n_cols, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx,
                           const int32_t *d_rowptr_t, const int32_t *d_colidx_t, int32_t *d_map_t, void *stream);

/* ------------------------------------------------------------------ edge softmax ----------------- */
/*
 * A softmax over the STORED entries of each row of a CSR pattern, forward and backward: the one step of a graph-attention layer that
 * is not a composition of the calls above (scores: gnnx_sddmm_csr_f32 or two per-vertex terms; aggregation with vals = alpha:
 * gnnx_spmm_csr_f32; gradient of vals: gnnx_sddmm_csr_f32; transposed order: gnnx_csr_transpose_map).  The reference has no
 * attention layer: the contract is this comment, restated in NumPy by tests/edge_softmax_ref.py.
 *
 * Forward, for entry p of row i with column c = colidx[p]; every operation is a separately rounded fp32 operation:
 *   t_p     = (scores[p] + rowterm[i * rowterm_stride]) + colterm[c * colterm_stride]
 *             A NULL operand is skipped; at least one of the three must be given.  Strides are in elements (>= 1), so the two
 *             terms can be the two columns of one [N, 2] matrix.
 *   e_p     = t_p > 0 ? t_p : t_p * negative_slope          (slope 1: the identity -- scaled dot-product attention is
 *                                                            scores = sddmm(Q, K, rowscale = 1/sqrt(d)) and no terms)
 *   m_i     = max_p e_p                                      (exact; a maximum has no order)
 *   x_p     = expf(e_p - m_i)                                (the subtraction rounded once; expf is the device library's)
 *   z_i     = the row sum of x_p in the ROW ORDER below
 *   alpha_p = x_p / z_i                                      (one correctly rounded IEEE division, not a multiply by 1 / z_i)
 *   d_out[p] = alpha_p, or x_p with flags & GNNX_EDGE_SOFTMAX_UNNORMALISED (what a sharded softmax would exchange);
 *   d_rowmax[i] = m_i and d_rowsum[i] = z_i when those pointers are given.
 * An empty row writes no entry, rowmax = -inf and rowsum = +0.  Inputs are finite; NaN and inf give unspecified values but never an
 * out-of-bounds access.  d_out aliases no input.
 *
 * ROW ORDER -- of every row sum of both calls, a function of the row length d alone.  Entries are numbered k = 0 .. d-1 in stored
 * order; S = 4096 is a fixed segment length.
 *   d <= S:  G is the smallest power of two with G >= d, capped at 64.  Virtual lane l < G starts from +0 and does
 *            acc_l = acc_l + v_k for k = l, l+G, l+2G, ... ascending; a lane with no entry holds +0.  For s = 1, 2, ..., G/2 every
 *            lane does acc_l = acc_l + acc_{l xor s}.  The sum is acc_0.
 *   d > S:   the row is cut into segments of S consecutive entries (the last may be short); each segment is summed by the rule
 *            above with G = 64; the row sum is ((seg_0 + seg_1) + seg_2) + ... in ascending segment order.
 * The lanes are virtual: how rows, segments and lanes map to wavefronts does not appear in the result.  The segment rule lets a hub
 * row of 10^5 .. 10^6 entries spread over many wavefronts: the segments' partial sums go to the workspace and are combined in the
 * fixed order.
 *
 * Backward (no transcendental: restatable bit for bit), from alpha (the normalised forward output) and dalpha = dL/dalpha:
 *   w_p   = alpha_p * dalpha_p;   dot_i = the row sum of w_p in the row order
 *   de_p  = alpha_p * (dalpha_p - dot_i)
 *   dt_p  = t_p > 0 ? de_p : de_p * negative_slope           (t_p recomputed from the same three inputs with the forward's additions)
 *   d_dt[p] = dt_p -- the gradient of scores[p];  d_drowterm[i] (when given) = the row sum of dt_p in the row order, +0 on an empty
 *   row -- the gradient of rowterm[i].  d_dt aliases nothing.  The gradient of colterm is not this call's job: it is
 *   gnnx_csr_rowsum_f32(rowptr_t, vals = dt[map_t]) on the transposed pattern (gnnx_csr_transpose_map); no atomics anywhere.
 *
 * Both calls are asynchronous on `stream` (a chain of launches on that one stream); they allocate nothing and synchronise nothing and
 * TRUST the CSR and nnz (= rowptr[n_rows]) as the aggregation does.  Null pointers, negative sizes, a stride < 1, all three operands
 * NULL and nnz >= 2^31 are GNNX_ERR_INVALID_ARG before any device call; a workspace smaller than gnnx_edge_softmax_workspace() bytes
 * is GNNX_ERR_WORKSPACE.  nnz == 0 still writes the per-row outputs.  The workspace (lists of the rows longer than 16 and than S
 * entries, one value per segment) serves either call and holds nothing between calls.
 */
#define GNNX_EDGE_SOFTMAX_UNNORMALISED 1u
int gnnx_edge_softmax_workspace(int32_t n_rows, int64_t nnz, size_t *bytes);
int gnnx_edge_softmax_csr_f32(int32_t n_rows, int32_t n_cols, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx,
                              const float *d_scores, const float *d_rowterm, int64_t rowterm_stride, const float *d_colterm,
                              int64_t colterm_stride, float negative_slope, uint32_t flags, float *d_out, float *d_rowmax,
                              float *d_rowsum, void *d_workspace, size_t workspace_bytes, void *stream);
int gnnx_edge_softmax_bwd_csr_f32(int32_t n_rows, int32_t n_cols, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx,
                                  const float *d_scores, const float *d_rowterm, int64_t rowterm_stride, const float *d_colterm,
                                  int64_t colterm_stride, float negative_slope, const float *d_alpha, const float *d_dalpha,
                                  float *d_dt, float *d_drowterm, void *d_workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ multi-head attention --------- */
/*
 * The three calls of a graph-attention layer -- aggregation, edge scores, edge softmax -- for H heads at once.  Feature matrices are
 * [rows, n_heads * head_dim]; head h owns columns h D .. h D + D - 1 (D = head_dim).  Every per-entry, per-head array is ENTRY-MAJOR:
 * a[p * ld + h], h < n_heads, ld >= n_heads in elements, so that the H values of one entry are one contiguous piece.
 *
 * THE CONTRACT of every call below is one sentence: head h of the result carries the bits that the single-head call above gives on slab
 * h of the feature matrices and column h of the per-entry arrays.  Every order stays the one already documented: the aggregation's ONE
 * accumulator per output element in descending column order (gnnx_spmm_csr_f32), the SDDMM lane-group order with F := head_dim
 * (gnnx_sddmm_csr_f32), the edge softmax's ROW ORDER with S = 4096 (gnnx_edge_softmax_csr_f32).  How heads, entries and rows map to
 * lanes never shows in the result; tests/heads_ref.py restates the calls in NumPy and the GPU tests hold the kernels to it bit for bit.
 * What the calls change is the memory traffic: the pattern (colidx) is read once for all heads, and a gathered row is one piece of
 * H D floats (8 heads of 8 features: one 256-byte row instead of eight 32-byte slices).
 *
 * gnnx_spmm_csr_heads_f32 -- the aggregation with one value per entry AND head:
 *   Y[i, h D + j] = beta * Y[i, h D + j] + ( sum_{p in row i, DESCENDING column} vals[p * ldv + h] * X[c_p, h D + j] ) + bias[h D + j]
 *   then where(Y > 0, Y, 0) with relu_out != 0.  The product is rounded, then the add; after the row the bias, then beta (0 or 1), then
 *   the ReLU -- the epilogue order of gnnx_spmm_csr_fused_f32.  There is no colscale / rowscale.  bias: [H D] or NULL.  X: [n_cols, H D]
 *   ld ldx.  Y: [n_rows, H D] ld ldy; columns of Y beyond H D are not touched.  X and Y must not alias.  Any head_dim >= 1 and n_heads >= 1.
 *   head_dim % 4 == 0 with 16-byte aligned rows (X, Y, bias, ldx, ldy) takes one 16-byte load per lane, the lane's head being f0 / head_dim;
 *   everything else (a 4-float piece that would straddle two heads, e.g. D = 6; unaligned pointers or leading dimensions) takes scalar
 *   lanes with the same bits.  head_dim == 1 over a matrix of ones is the per-head row sum of vals (the gradient of the softmax's column
 *   term on the transposed pattern).  There is NO PLAN: a row is one lane group's chain of adds, a hub row included (DESIGN.md 5.3:
 *   4.8 ms on R-MAT 1 M / 10 M whose longest row has 26 763 entries, whatever the width).  The CSR is trusted as in gnnx_spmm_csr_f32.
 *
 * gnnx_sddmm_csr_heads_f32 -- a score per entry and head:
 *   out[p * ldo + h] = <L[i, h D .. h D + D - 1], R[c_p, h D .. h D + D - 1]>      in the SDDMM order for F = head_dim; no scales.
 *   Work is dealt in the non-zero domain (a hub row spreads over the device); colidx and both rows are read once per entry for all
 *   heads.  L == R is allowed; out aliases nothing.  nnz == 0 is GNNX_OK with no launch.  Second use: dL/dvals of the heads aggregation
 *   is gnnx_sddmm_csr_heads_f32(L = G, R = X).
 *
 * gnnx_edge_softmax_csr_heads_f32 / gnnx_edge_softmax_bwd_csr_heads_f32 -- the edge softmax per head: scores [nnz, H] ld lds, out ld ldo,
 *   alpha / dalpha / dt ld lda / ldd / ldt.  Term operand h is rowterm[i * rowterm_stride + h] / colterm[c * colterm_stride + h], strides
 *   >= n_heads: the two halves of one [N, 2H] matrix serve as the two terms.  rowmax / rowsum are [n_rows, H] contiguous;
 *   drowterm[i * drowterm_stride + h] (stride >= n_heads) lets the row term's gradient land in the left half of an [N, 2H] buffer.  The
 *   segment rule and everything else of the single-head contract hold per head; the workspace of gnnx_edge_softmax_heads_workspace
 *   serves either call.  n_heads == 1 with unit leading dimensions IS the single-head call.
 *
 * gnnx_csr_rowsum_heads_f32 -- out[i * ldo + h] = the sum of vals[p * ldv + h] over the entries p of row i, ONE accumulator from +0 in
 *   ASCENDING p: column h carries the bits of gnnx_csr_rowsum_f32 on column h of vals (the reference's functional::sum walks up, where the
 *   aggregation walks down: the two orders differ in the last bit).  It is the gradient of the softmax's column term on the transposed
 *   pattern -- out the right half of the [N, 2H] gradient buffer.  An empty row writes +0.
 *
 * All entries: null pointers, negative sizes, n_heads < 1, head_dim < 1, a leading dimension or stride below its minimum and
 * nnz >= 2^31 are GNNX_ERR_INVALID_ARG before any device call (p * ld + h is formed in 64 bits); a small workspace is GNNX_ERR_WORKSPACE;
 * nnz == 0 still writes the per-row outputs.  Asynchronous on `stream`; nothing is allocated or synchronised; no atomics on any value.
 */
int gnnx_spmm_csr_heads_f32(int32_t n_rows, int32_t n_cols, int32_t n_heads, int32_t head_dim, const int32_t *d_rowptr,
                            const int32_t *d_colidx, const float *d_vals, int64_t ldv, const float *d_bias, const float *d_X, int64_t ldx,
                            float beta, int relu_out, float *d_Y, int64_t ldy, void *stream);
int gnnx_sddmm_csr_heads_f32(int32_t n_rows, int32_t n_cols, int32_t n_heads, int32_t head_dim, int64_t nnz, const int32_t *d_rowptr,
                             const int32_t *d_colidx, const float *d_L, int64_t ldl, const float *d_R, int64_t ldr, float *d_out, int64_t ldo,
                             void *stream);
int gnnx_csr_rowsum_heads_f32(const int32_t *d_rowptr, const float *d_vals, int64_t ldv, int32_t n_rows, int32_t n_heads, float *d_out,
                              int64_t ldo, void *stream);
int gnnx_edge_softmax_heads_workspace(int32_t n_rows, int64_t nnz, int32_t n_heads, size_t *bytes);
int gnnx_edge_softmax_csr_heads_f32(int32_t n_rows, int32_t n_cols, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx,
                                    int32_t n_heads, const float *d_scores, int64_t lds, const float *d_rowterm, int64_t rowterm_stride,
                                    const float *d_colterm, int64_t colterm_stride, float negative_slope, uint32_t flags, float *d_out,
                                    int64_t ldo, float *d_rowmax, float *d_rowsum, void *d_workspace, size_t workspace_bytes, void *stream);
int gnnx_edge_softmax_bwd_csr_heads_f32(int32_t n_rows, int32_t n_cols, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx,
                                        int32_t n_heads, const float *d_scores, int64_t lds, const float *d_rowterm, int64_t rowterm_stride,
                                        const float *d_colterm, int64_t colterm_stride, float negative_slope, const float *d_alpha,
                                        int64_t lda, const float *d_dalpha, int64_t ldd, float *d_dt, int64_t ldt, float *d_drowterm,
                                        int64_t drowterm_stride, void *d_workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ dynamic attention scores (GATv2) ---- */
/*
 * The score of GATv2 (Brody, Alon, Yahav, ICLR 2022): e(i, c) = a^T leaky_relu(W_l h_i + W_r h_c), the non-linearity INSIDE the sum.  The
 * GAT score leaky_relu(el_i + er_c) is monotone in er_c, so every row that stores the same columns ranks them alike; this one does not.
 * It is not a composition of the calls above (the SDDMM is a plain dot product, the softmax's terms are one scalar per vertex and head):
 * a per-entry, per-feature non-linearity is a kernel with the memory traffic of an aggregation -- one gathered H D row per stored entry.
 * Everything around it exists: the softmax over given scores with slope 1 (gnnx_edge_softmax_csr_heads_f32), the aggregation with vals =
 * alpha, its value gradient, gnnx_csr_transpose_map.  The conventions are the multi-head section's: feature matrices [rows, H D], head h
 * in columns h D .. h D + D - 1; per-entry arrays entry-major [nnz, H] with a leading dimension.  Every operation is a separately rounded
 * fp32 operation (-ffp-contract=off); tests/gatv2_ref.py restates both calls in NumPy and the GPU tests hold the kernels to it bit for bit.
 *
 * gnnx_gatv2_scores_csr_f32 -- for entry p of row i with column c = colidx[p], head h, feature f = h D + k:
 *   u_f    = L[i, f] + R[c, f]
 *   e_f    = u_f > 0 ? u_f : u_f * negative_slope          (u_f == 0 takes the slope branch)
 *   term_f = a[f] * e_f
 *   out[p * ldo + h] = the sum over k of term_f in the SDDMM lane-group order of gnnx_sddmm_csr_f32 with F := head_dim: the chunk step is
 *   acc = acc + term_f, term_f in the place of the product and rounded before the add; chunks, lanes and the butterfly as documented there.
 *   L: [n_rows, H D] ld ldl.  R: [n_cols, H D] ld ldr.  a: [H D] contiguous, a head's slice is its attention vector.  out: [nnz, H] ld ldo.
 *   Work is dealt in the non-zero domain (a fixed number of entries per lane group, the row by a search in rowptr: a hub row spreads
 *   over the device, no plan); the lane's pieces of L and a stay in registers while the row lasts.  The result does not depend on
 *   alignment: head_dim % 4 != 0, or a pointer (L, R, a) or leading dimension (ldl, ldr) that is not 16-byte aligned, takes scalar loads
 *   with the same feature-to-lane assignment and the same bits.  L == R is allowed; out aliases nothing.  nnz == 0 is GNNX_OK with no
 *   launch.
 *
 * gnnx_gatv2_scores_bwd_csr_f32 -- the gradient to the ROW-SIDE operand of whichever pattern it is handed.  For row i and feature
 *   f = h D + k: ONE accumulator from +0 over the row's entries p in DESCENDING stored position (the order of gnnx_spmm_csr_heads_f32):
 *     m   = entry_map ? entry_map[p] : p
 *     u   = Own[i, f] + Other[c_p, f]
 *     w   = u > 0 ? a[f] : a[f] * negative_slope           (rounded once)
 *     acc = acc + (de[m * ldd + h] * w)                    (the product rounded, then the sum)
 *   dOwn[i, f] = beta ? dOwn[i, f] + acc : acc             (beta is 0 or 1)
 *   With d_T != NULL a second accumulator runs in the same order:
 *     e    = u > 0 ? u : u * negative_slope
 *     tacc = tacc + (de[m * ldd + h] * e);                 T[i, f] = tacc
 *   and the gradient of the attention vector is da = gnnx_colsum_f32(T), a call with a fixed order: no atomics anywhere on the path.
 *   On the forward pattern with Own = L, Other = R, entry_map = NULL the call gives dL and T.  On the transposed pattern with Own = R,
 *   Other = L, entry_map = map_t (gnnx_csr_transpose_map: de stays in the forward order), T = NULL and beta = 1 it adds dR onto the buffer
 *   that already holds the aggregation's gradient; IEEE addition commutes, so u has the forward's bits in both passes.
 *   de: [nnz, H] ld ldd.  Own: [n_rows, H D] ld ld_own.  Other: [n_cols, H D] ld ld_other.  dOwn: [n_rows, H D] ld ld_down.  T: [n_rows, H D]
 *   ld ldt or NULL.  Columns beyond H D of dOwn and T are never touched.  An empty row writes +0 (T too), or leaves dOwn unchanged with
 *   beta = 1.  dOwn and T alias nothing.  There is NO PLAN, as in gnnx_spmm_csr_heads_f32: a row is one lane group's chain whatever its
 *   length, G lanes per row with a 4-float (or 1-float) piece per lane, the Own and a pieces in registers for the whole row, several
 *   Other rows in flight.  The alignment rule is the forward's, over Own, Other, a, dOwn, T and their leading dimensions.
 *
 * Both: null pointers, negative sizes, n_heads < 1, head_dim < 1, a leading dimension below its minimum (H D, or H for out / de), beta
 * other than 0 or 1 and nnz >= 2^31 are GNNX_ERR_INVALID_ARG before any device call.  Asynchronous on `stream`; nothing is allocated or
 * synchronised; the CSR and nnz (= rowptr[n_rows]) are trusted as in the aggregation.
 */
int gnnx_gatv2_scores_csr_f32(int32_t n_rows, int32_t n_cols, int32_t n_heads, int32_t head_dim, int64_t nnz, const int32_t *d_rowptr,
                              const int32_t *d_colidx, const float *d_L, int64_t ldl, const float *d_R, int64_t ldr, const float *d_a,
                              float negative_slope, float *d_out, int64_t ldo, void *stream);
int gnnx_gatv2_scores_bwd_csr_f32(int32_t n_rows, int32_t n_cols, int32_t n_heads, int32_t head_dim, int64_t nnz, const int32_t *d_rowptr,
                                  const int32_t *d_colidx, const float *d_de, int64_t ldd, const int32_t *d_entry_map, const float *d_Own,
                                  int64_t ld_own, const float *d_Other, int64_t ld_other, const float *d_a, float negative_slope, float beta,
                                  float *d_dOwn, int64_t ld_down, float *d_T, int64_t ldt, void *stream);

/* ------------------------------------------------------------------ neighbourhood reductions ---- */
/*
 * The reduce operators of message passing that are not a sum: an element-wise MAX / MIN over the stored entries of each row of a CSR
 * pattern, with its arg, and the backward that routes every gradient element to the one entry that won -- what a GraphSAGE pooling
 * layer, PNA or a graph max-pool needs.  The reference's MessagePassing base declares the hook (message / aggregate_and_update,
 * reference graph.h:114-115) and implements only GCN's sum; the contract is this comment, restated in NumPy by tests/reduce_ref.py.
 *
 * Forward, gnnx_spmm_csr_reduce_f32, for entry p of row i with column c_p = colidx[p]:
 *   t_p,f     = vals[p] * X[c_p, f]        ONE rounded fp32 multiply; with vals == NULL t_p,f = X[c_p, f] with its own bits.
 *   arg[i, f] = the SMALLEST position p of row i such that no entry q of the row has t_q,f > t_p,f  (GNNX_REDUCE_MIN: <): an ABSOLUTE
 *               entry position in [rowptr[i], rowptr[i+1]).
 *   Y[i, f]   = t_arg,f with that entry's bits: where +0 and -0 tie the earlier entry wins and keeps its sign.
 * An empty row writes Y = +0 and arg = -1.  A non-empty row ALWAYS gets a valid position, also when every t is -inf (MIN: +inf): there
 * is no sentinel that a strict compare can never beat.  With a NaN among the t the value and the arg are unspecified; no out-of-range
 * access ever happens.  d_arg may be NULL.  X: [n_cols, n_feat] ld ldx; Y (float) ld ldy and arg (int32) ld lda: [n_rows, n_feat];
 * columns beyond n_feat are not touched.  X aliases no output.  A maximum has no order: the result is a function of the inputs alone,
 * however a row is split or mapped to lanes.
 *
 * Backward, gnnx_spmm_csr_reduce_bwd_f32: the gradient with respect to X (vals are constants; their gradient is not this call's job).
 * It runs on the TRANSPOSED pattern, as every backward here does: entry q of row c of CSR(A^T) is the stored entry (i, c) of A with
 * i = colidx_t[q] and p = map_t[q] its position in CSR(A) (gnnx_csr_transpose_map).  Entry q contributes vals[p] * G[i, f] (the product
 * rounded first; G[i, f] with vals == NULL) iff arg[i, f] == p, and nothing otherwise.
 *   ORDER of the sum, with S = 4096: row c is cut into segments of S consecutive entries (the last may be short); a segment is summed
 *   by ONE accumulator per feature starting from +0 and walking the segment from its LAST entry to its FIRST; the row sum is
 *   ((seg_0 + seg_1) + seg_2) + ... in ascending segment order.  A row of at most S entries is therefore the aggregation's own
 *   descending one-accumulator chain (gnnx_spmm_csr_f32 with the 0/1 match folded into the values); a hub column of 10^4 .. 10^6
 *   entries spreads over d / S lane groups instead of one.
 *   dX[c, f] = acc with beta == 0 (dX is never read), dX[c, f] + acc with beta == 1.
 * d_dX: [n_rows_t, n_feat] ld ldx; d_G (float, ld ldg) and d_arg (int32, ld lda): [n_cols_t, n_feat].  d_vals is indexed by the
 * positions of CSR(A).  No atomics on any value: the bits are the same on every run.
 *
 * Both calls are asynchronous on `stream` (a chain of launches on that one stream); they allocate nothing and synchronise nothing and
 * TRUST the CSR and nnz (= rowptr[n_rows]).  Negative sizes, a leading dimension < n_feat, an op outside the enum, a beta other than 0
 * or 1 and nnz >= 2^31 are GNNX_ERR_INVALID_ARG before any device call, and so is a null pointer (d_vals and the forward's d_arg may be
 * NULL; d_colidx / d_colidx_t / d_map_t may be NULL with nnz == 0).  n_feat == 0 or n_rows == 0 returns GNNX_OK and writes nothing;
 * nnz == 0 still writes the per-row outputs.  A workspace that is NULL or smaller than gnnx_spmm_csr_reduce_workspace() bytes is
 * GNNX_ERR_WORKSPACE with nothing written.  The workspace serves either call (the backward passes n_rows_t), holds nothing between
 * calls and may sit at any address.  Its size is a function of (n_rows, nnz, n_feat) alone:
 *   hubs = min(nnz / (S + 1), n_rows)   rows can be longer than S;   segs = nnz / S + hubs   bounds the sum of their ceil(d / S);
 *   bytes = 256 + round_up_256( 4 * (16 + 2 * hubs + segs + 2 * segs * n_feat) )
 * -- 16 counter words, the hub list with each hub's first segment slot, the hub of each slot, and per (slot, feature) the segment's
 * value and position (forward) or its sum (backward).
 *
 * Kernels (gnnx_reduce.hip): rows of at most S entries take the lane-group shape of gnnx_spmm_csr_heads_f32 (4 .. 64 lanes per row, one
 * 16-byte piece per lane, feature tiles in the grid's y); n_feat % 4 != 0, or an X / Y / arg / G / dX pointer or leading dimension
 * that is not 16-byte aligned, takes scalar lanes with the same bits.  Longer rows are listed in the workspace by the row kernel (a
 * counter atomic reserves slots, never an atomic on a value), a fixed grid strides over their segments and a combine kernel finishes
 * each row: the better value wins and on equal values the smaller position (forward); ascending segment order (backward).
 */
enum { GNNX_REDUCE_MAX = 0, GNNX_REDUCE_MIN = 1 };
int gnnx_spmm_csr_reduce_workspace(int32_t n_rows, int64_t nnz, int32_t n_feat, size_t *bytes);
int gnnx_spmm_csr_reduce_f32(int op, int32_t n_rows, int32_t n_cols, int32_t n_feat, int64_t nnz, const int32_t *d_rowptr,
                             const int32_t *d_colidx, const float *d_vals, const float *d_X, int64_t ldx, float *d_Y, int64_t ldy,
                             int32_t *d_arg, int64_t lda, void *d_workspace, size_t workspace_bytes, void *stream);
int gnnx_spmm_csr_reduce_bwd_f32(int32_t n_rows_t, int32_t n_cols_t, int32_t n_feat, int64_t nnz, const int32_t *d_rowptr_t,
                                 const int32_t *d_colidx_t, const int32_t *d_map_t, const float *d_vals, const int32_t *d_arg,
                                 int64_t lda, const float *d_G, int64_t ldg, float beta, float *d_dX, int64_t ldx, void *d_workspace,
                                 size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ graph readout --------------- */
/*
 * One row of output per GRAPH of a batch: the SUM, MEAN or MAX of each segment of consecutive rows of X, and the backward that hands a
 * segment's gradient back to its rows -- the readout of graph classification and regression.  The reference declares the batch
 * (graph::DataBatch, reference graph.h:104-109) and leaves it without a body; the contract is this comment, restated in NumPy by
 * tests/pool_ref.py.
 *
 * Segment b is the rows [segptr[b], segptr[b+1]) of X; segptr has n_seg + 1 entries and is TRUSTED to be non-decreasing with
 * segptr[0] == 0 and segptr[n_seg] == n_rows.  X and dX: [n_rows, n_feat]; Y (float), arg (int32) and G (float): [n_seg, n_feat]; every
 * matrix has its own leading dimension and columns beyond n_feat are never touched.  len = segptr[b+1] - segptr[b].
 *
 * Forward, gnnx_segment_pool_f32:
 *   GNNX_POOL_SUM   With T = GNNX_POOL_CHUNK a segment is cut into chunks of T consecutive rows counted from the segment's OWN first
 *                   row (the last chunk may be short).  A chunk is summed by ONE accumulator per feature that starts at +0 and walks the
 *                   chunk's rows in ASCENDING order; the segment's sum is ((c_0 + c_1) + c_2) + ... in ascending chunk order.  A graph's
 *                   readout is therefore a function of that graph's rows alone: the same bits whether the graph is pooled by itself or
 *                   at any position of any batch, and however chunks are mapped to lanes, workgroups or XCDs.
 *   GNNX_POOL_MEAN  Y = sum / (float)len with the sum above and ONE correctly rounded fp32 division (no reciprocal multiply).
 *   GNNX_POOL_MAX   arg[b, f] = the SMALLEST row i of the segment such that no row q of it has X[q, f] > X[i, f]: an ABSOLUTE row index.
 *                   Y[b, f] = X[arg, f] with that row's bits: between +0 and -0 the earlier row wins and keeps its sign.  A non-empty
 *                   segment ALWAYS gets a valid row, also when every value is -inf.  With a NaN in the segment the value and the arg
 *                   are unspecified; no access is ever out of range.
 *   An empty segment writes Y = +0 for every op and arg = -1 for MAX.  d_arg may be NULL; SUM and MEAN never write it.
 *
 * Backward, gnnx_segment_pool_bwd_f32, for row i of segment b:
 *   t = G[b, f] (SUM);  t = G[b, f] / (float)len (MEAN, the same single division);  t = G[b, f] if arg[b, f] == i and +0 otherwise (MAX);
 *   dX[i, f] = t with beta == 0 -- dX is never read, a NaN already in it vanishes -- and dX[i, f] + t (one rounded add) with beta == 1.
 *   Every row of dX is written.
 *
 * Both calls are asynchronous on `stream` (a chain of launches on that one stream); they allocate nothing, synchronise nothing and use
 * no atomics on any value: the bits are the same on every run.  All element offsets are 64-bit.  GNNX_ERR_INVALID_ARG before any device
 * call for: a negative size, a leading dimension < n_feat (lda only where the op is MAX), an op outside the enum, a beta other than 0 or 1, n_seg == 0 with
 * n_rows != 0, and a null pointer (the forward's d_arg may be NULL, MAX backward requires it, SUM / MEAN backward ignore it; d_X / d_dX
 * may be NULL with n_rows == 0).  n_feat == 0 or n_seg == 0 returns GNNX_OK and writes nothing; n_rows == 0 with n_seg > 0 still writes
 * the per-segment outputs.  A workspace that is NULL or smaller than gnnx_segment_pool_workspace() bytes is GNNX_ERR_WORKSPACE with
 * nothing written; it holds nothing between calls and may sit at any address.  Its size is a function of the sizes alone (n_seg does
 * not enter):
 *   tiles = n_rows / T + 1 (integer division);   bytes = 256 + round_up_256( 4 * tiles * (4 * n_feat + 1) )
 * -- per tile of T rows two chunk partials, each a value and a position per feature, and the long segment that starts in the tile.
 *
 * Kernels (gnnx_pool.hip): the work unit is a (segment, chunk) pair.  The grid is dealt over global tiles of T rows; a lane group of
 * 4 .. 64 lanes (one 16-byte piece of the feature row per lane, feature tiles in the grid's y) finds by binary search in segptr the
 * chunks that START inside its tile -- any segment has at most one, and at most two of them belong to segments longer than T -- and
 * reads their rows with no index array, the loads of sixteen rows issued ahead of the dependent chain.  A segment of at most T rows
 * writes Y directly; a longer one writes chunk partials and a combine kernel finishes it in ascending chunk order (MAX: the better
 * value wins and on equal values the smaller row).  n_feat % 4 != 0, or a pointer or leading dimension that is not 16-byte aligned,
 * takes scalar lanes with the same bits.  The backward is one streaming pass over the rows of dX, each lane group finding its segment
 * in segptr.
 */
enum { GNNX_POOL_SUM = 0, GNNX_POOL_MEAN = 1, GNNX_POOL_MAX = 2 };
#define GNNX_POOL_CHUNK 256
int gnnx_segment_pool_workspace(int32_t n_seg, int32_t n_rows, int32_t n_feat, size_t *bytes);
int gnnx_segment_pool_f32(int op, int32_t n_seg, int32_t n_rows, int32_t n_feat, const int32_t *d_segptr, const float *d_X, int64_t ldx,
                          float *d_Y, int64_t ldy, int32_t *d_arg, int64_t lda, void *d_workspace, size_t workspace_bytes, void *stream);
int gnnx_segment_pool_bwd_f32(int op, int32_t n_seg, int32_t n_rows, int32_t n_feat, const int32_t *d_segptr, const int32_t *d_arg,
                              int64_t lda, const float *d_G, int64_t ldg, float beta, float *d_dX, int64_t ldx, void *stream);

/* ------------------------------------------------------------------ neighbour sampling ---------- */
/*
 * A fixed fanout of k neighbours per vertex, drawn afresh from a seed: the other half of GraphSAGE (Hamilton et al. 2017).  The sample
 * of a CSR is a CSR on the same rows and columns; everything downstream (gnnx_csr_from_coo for the transpose, gnnx_degree_norm_f32, the
 * plans, gnnx_csr_transpose_map, every aggregation) takes it as it takes any other.  The contract is this comment, restated in NumPy by
 * tests/sample_ref.py.
 *
 * Selection: uniformly without replacement.  Take row i with d = rowptr[i+1] - rowptr[i] entries, numbered j = 0 .. d-1 in stored order.
 *   h_j = splitmix64( splitmix64(seed) ^ (((uint64)i << 32 | (uint64)j) * 0x9E3779B97F4A7C15) )   the finaliser of gnnx_rmat_edges /
 *                                                                                                 gnnx_uniform_pm1_f32; the product
 *                                                                                                 wraps in 64 bits
 *   u_j = (h_j >> 32) << 32 | j                                                                   a 32-bit random key above the
 *                                                                                                 entry's own offset
 * The u_j of a row are pairwise different by construction: there is no tie and no tie rule; u is compared as ONE 64-bit value.  A row
 * with d <= k keeps all its entries; a longer row keeps the k entries with the smallest u_j.  Kept entries stay in STORED ORDER
 * (ascending j), the order every aggregation here sums in.  The key depends on the offset j, never on the column id: the selection
 * reads no colidx.  A selection of the k smallest has no order: the result is a function of (seed, i, d, k) alone, however rows,
 * segments and lanes are mapped.  A different seed gives an independent draw; a caller uses one seed per epoch or layer.
 *
 * Outputs:
 *   d_rowptr_out    n_rows + 1 values, the exclusive scan of min(d_i, k).
 *   d_colidx_out[q] the column of kept entry q.
 *   d_pos_out[q]    (may be NULL) the ABSOLUTE position of kept entry q in the input CSR: a per-entry array (edge weights, attention
 *                   values) follows the sample by a gather through it.
 *   d_rowid_out[q]  (may be NULL) the row of kept entry q: with d_colidx_out the COO that gnnx_csr_from_coo takes to build the
 *                   transposed CSR.
 *   *nnz_out        (HOST) = rowptr_out[n_rows], valid on return: the call synchronises `stream`, as gnnx_csr_extract_rows does.
 *
 * Statuses.  GNNX_ERR_INVALID_ARG before any device call: negative sizes, k < 1, nnz >= 2^31, a null rowptr / rowptr_out / colidx_out /
 * nnz_out, a null colidx with nnz > 0.  GNNX_ERR_UNSUPPORTED: k > 64 (one wavefront holds a row's running selection; fanouts in use
 * are 5 to 50).  GNNX_ERR_WORKSPACE with nothing written: a workspace that is NULL or smaller than the query.  GNNX_ERR_INVALID_ARG
 * with nothing written and *nnz_out still set: nnz_capacity (the capacity of d_colidx_out / d_pos_out / d_rowid_out in entries) is
 * smaller than the result -- never a truncated CSR, the convention of gnnx_csr_extract_rows.  n_rows == 0 is a valid result:
 * rowptr_out = [0].
 *
 * The CSR and nnz (= rowptr[n_rows]) are TRUSTED, as everywhere else.  The workspace holds nothing between calls, may sit at any
 * address, and its size is a function of (n_rows, nnz, k) alone, with S = 4096:
 *   tiles = n_rows / 1024 + 1          the scan of min(d, k) works on tiles of 1024 rows;
 *   hubs = min(nnz / (S + 1), n_rows)  rows can be longer than S;   segs = nnz / S + hubs   bounds the sum of their ceil(d / S);
 *   longs = min(nnz / 257, n_rows)     rows can be longer than 256;
 *   bytes = 256 + round_up_256( 4 * (16 + tiles + 2 * hubs + segs + segs * k + longs) )
 * -- 16 counter words, a sum per tile, the hub list with each hub's first segment slot, the hub of each slot, per slot the k
 * candidates of the segment, and the list of long rows.  A counter atomic reserves a listed row's slots; no other atomic is used: the same bits on every run.
 *
 * Kernels (gnnx_sample.hip): min(d, k) is scanned into rowptr_out and the total copied to the host.  Rows of at most 256 entries take a
 * lane group (4 .. 64 lanes by the mean row length, several short rows per wavefront): d <= k is a copy; otherwise a radix select on
 * the 64-bit key from the top bit down, which stops as soon as as many candidates are left as are still needed (keys are recomputed
 * per pass, never stored), and a ballot-prefix compaction that writes the kept entries in ascending j.  Longer rows are listed in the
 * workspace by the row kernel: a row of at most S entries gets a wavefront of its own from a fixed grid that strides over the list (on a
 * power-law graph these rows sit next to each other and would otherwise keep a few narrow lane groups busy long after the rest is
 * done); for a row of more than S entries a fixed grid strides over its segments of S consecutive entries, each segment writes the offsets of
 * its min(k, len) smallest keys to its slot, and a combine step per hub row picks the k smallest of the candidates and writes the row.
 */
int gnnx_csr_sample_workspace(int32_t n_rows, int64_t nnz, int32_t k, size_t *bytes);
int gnnx_csr_sample_neighbors(int32_t n_rows, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx, int32_t k, uint64_t seed,
                              int32_t *d_rowptr_out, int32_t *d_colidx_out, int32_t *d_pos_out, int32_t *d_rowid_out,
                              int64_t nnz_capacity, int64_t *nnz_out, void *d_workspace, size_t workspace_bytes, void *stream);
/*
 * gnnx_csr_sample_rows: the same sample for a LIST of rows -- the sampler of a mini-batch, whose cost is O(n_listed + entries of the
 * listed rows) and reads nothing else of the graph.  d_rows [n_listed] holds row ids of the CSR in any order, repeats allowed.
 * Output row x is, entry for entry, row d_rows[x] of what gnnx_csr_sample_neighbors(..., k, seed) writes for the whole graph: the key
 * is formed from the CSR's row id i = d_rows[x], never from x, and a repeated row gives the same sample twice.
 *   d_rowptr_out    n_listed + 1 values, the exclusive scan of min(d_{rows[x]}, k).
 *   d_colidx_out[q] the ORIGINAL column id of kept entry q (gnnx_csr_renumber_cols makes it a position in a row list).
 *   d_pos_out[q]    (may be NULL) the absolute position of kept entry q in the input CSR.
 *   d_rowid_out[q]  (may be NULL) x, the LIST position of kept entry q: (colidx_out, rowid_out) is the COO of the transposed block.
 *   d_col_mark      (may be NULL) one byte per column, n_cols bytes: byte c is set to 1 for every kept entry of column c and no other
 *                   byte is written -- the frontier of the sampled block, as gnnx_frontier_mark marks that of the full rows.  The
 *                   caller zeroes or presets the array; many lanes storing the same 1 is the only race.  (A stored column outside
 *                   [0, n_cols) is not marked; gnnx_csr_renumber_cols refuses it.)
 *   *nnz_out        (HOST) = rowptr_out[n_listed], valid on return.
 * Statuses, capacity, k <= 64 and synchronisation are those of gnnx_csr_sample_neighbors; in addition a negative n_cols or n_listed,
 * n_listed >= 2^31 and a null d_rows with n_listed > 0 are GNNX_ERR_INVALID_ARG before any device call, and an id of d_rows outside
 * [0, n_rows) is GNNX_ERR_INDEX_RANGE with nothing written to any output.  n_listed == 0 is a valid result: rowptr_out = [0].
 *
 * Workspace: there is no query of its own.  The call carves as the whole-graph call does, with the list's length in the place of the
 * row count: at least gnnx_csr_sample_workspace(n_listed, nnz, k) bytes, nnz that of the whole CSR.  The range flag is one of the 16
 * counter words.  The lists of long rows are sized for rows met once each; a list that repeats rows of more than 256 entries more
 * often than they hold has the surplus rows selected by the row kernel's own lane group: slower, and the same entries.
 *
 * Kernels: those of gnnx_csr_sample_neighbors with a row indirection (CSR row = d_rows[x], output row = x; the long-row and hub lists
 * hold x).  The lane-group width comes from nnz / n_rows of the CSR; the result does not depend on it.
 */
int gnnx_csr_sample_rows(int32_t n_rows, int32_t n_cols, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx,
                         const int32_t *d_rows, int64_t n_listed, int32_t k, uint64_t seed, int32_t *d_rowptr_out, int32_t *d_colidx_out,
                         int32_t *d_pos_out, int32_t *d_rowid_out, uint8_t *d_col_mark, int64_t nnz_capacity, int64_t *nnz_out,
                         void *d_workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ negative sampling, ranking --- */
/*
 * The negative half of link prediction: for every stored entry of a POSITIVES pattern, m columns drawn uniformly from the columns its
 * row does NOT hold in an EXCLUDED pattern (normally the whole graph), and the per-positive counts that MRR, Hits@K and AUC are made
 * of.  The contract is this comment, restated with Python sets and integers by tests/negative_ref.py.
 *
 * gnnx_csr_sample_negatives.  The positives pattern is (d_rowptr_pos, nnz_pos) on n_rows rows: only its row structure is read.  The
 * excluded pattern (d_rowptr_ex, d_colidx_ex) has the same n_rows rows, n_cols columns, and STRICTLY ASCENDING rows (what every
 * gnnx_csr_from_coo build gives).  Take entry j (offset within its row) of row i of the positives -- entry p = rowptr_pos[i] + j --
 * and a draw t < m:
 *   S_i   = row i of the excluded pattern, d = |S_i|;   E = S_i, plus {i} when flags has GNNX_NEG_EXCLUDE_SELF and i < n_cols
 *   count = n_cols - |E|
 *   s     = splitmix64(seed ^ 0x6E65676174697665)                 a domain constant: independent of the neighbour sampler's draw
 *                                                                 under the same seed
 *   h     = splitmix64( splitmix64( s ^ (((uint64)i << 32 | (uint64)j) * 0x9E3779B97F4A7C15) ) ^ ((uint64)t * 0x9E3779B97F4A7C15) )
 *                                                                 the finaliser of the neighbour sampler; products wrap in 64 bits
 *   r     = floor(h * count / 2^64)                               the high 64 bits of the 128-bit product: bias <= count / 2^64
 *   d_neg[p * m + t] = the r-th smallest element (from 0) of [0, n_cols) \ E
 * Exact and bounded: there is no rejection loop and no spin.  count == 0 (a complete row): d_neg[p * m + t] = -1 for every t, and the
 * positive adds m to the unfilled counter -- a counter atomic on an integer, the only atomic: the same bits on every run.  The m draws
 * of one positive are independent and may repeat.  The result is a function of (seed, i, j, t, S_i, n_cols, flags) alone, however
 * positives and draws are mapped to lanes.  A different seed gives an independent draw; a caller uses one seed per epoch.
 *
 * The selection needs no list of non-members.  For the ascending c_0 < .. < c_{d-1} of S_i, g(x) = c_x - x is non-decreasing, and
 * with J(r) = #{x : g(x) <= r} (one upper-bound search) the r-th non-member of S_i is r + J(r).  With the self flag set, i < n_cols
 * and i not in S_i (one lower-bound search): if r + J(r) >= i the answer is (r + 1) + J(r + 1), otherwise r + J(r).  O(log d)
 * dependent loads per negative.
 *
 * Outputs: d_neg [nnz_pos, m] int32, entry-major like the per-head arrays; *n_unfilled_out (HOST) = the number of -1 entries, valid
 * on return: the call synchronises `stream`, as gnnx_csr_sample_neighbors does.
 *
 * Statuses.  GNNX_ERR_INVALID_ARG before any device call: negative sizes, m < 1, nnz_pos * m >= 2^31, nnz_ex >= 2^31, a null
 * rowptr_pos / rowptr_ex / n_unfilled_out, a null d_neg with nnz_pos > 0, a null colidx_ex with nnz_ex > 0.  GNNX_ERR_WORKSPACE with
 * nothing written: a workspace that is NULL or smaller than GNNX_NEG_WORKSPACE_BYTES (it holds the counter, keeps nothing between
 * calls and may sit at any address).  n_rows == 0 or nnz_pos == 0 is a valid empty result (*n_unfilled_out = 0, no device call).
 * Both patterns, nnz_pos (= rowptr_pos[n_rows]) and nnz_ex are TRUSTED, as everywhere else: with an excluded column outside
 * [0, n_cols) or a row that is not strictly ascending the values of that row's draws are unspecified; no access is ever out of range.
 *
 * Kernel (gnnx_negative.hip): work is dealt in the entry domain, as in gnnx_sddmm_csr_f32: a wavefront owns GNNX_NEG_RUN consecutive
 * positives and finds the rows of its first and last one in rowptr_pos, so a hub row spreads over the device without a plan; the
 * (positive, draw) items of the run go to the lanes draw-fastest, so the m draws of a positive sit on adjacent lanes, search the same
 * row and share the loads of the search's top levels.  Offsets are 64-bit.
 *
 * gnnx_rank_counts_f32.  For positive scores s[n_pos] and negative scores q[n_pos, m] (entry-major), with an optional d_neg[n_pos, m]
 * whose entries < 0 mark draws to SKIP (NULL: none is skipped):
 *   greater[p] = #{t : q[p,t] >  s[p]}     equal[p] = #{t : q[p,t] == s[p]}     valid[p] = #{t : q[p,t] <, == or > s[p]}
 * over the draws that are not skipped.  Comparisons are IEEE: -0 == +0, and a NaN on either side is counted in none of the three --
 * valid[p] - greater[p] - equal[p] is exactly #{t : q[p,t] < s[p]}.  One streaming pass of m loads per positive (a lane group of
 * 1 .. 64 lanes by m), integer sums, no atomics; asynchronous on `stream`.  Every metric is a function of these integers, so it is exact in any
 * summation order.  GNNX_ERR_INVALID_ARG: negative n_pos, n_pos >= 2^31, m < 1, a null pointer among s, q, greater, equal, valid
 * with n_pos > 0.
 */
#define GNNX_NEG_EXCLUDE_SELF 1u
#define GNNX_NEG_RUN 64
#define GNNX_NEG_WORKSPACE_BYTES 256
int gnnx_csr_sample_negatives(int32_t n_rows, int32_t n_cols, int64_t nnz_pos, const int32_t *d_rowptr_pos, int64_t nnz_ex,
                              const int32_t *d_rowptr_ex, const int32_t *d_colidx_ex, int32_t m, uint64_t seed, uint32_t flags,
                              int32_t *d_neg, int64_t *n_unfilled_out, void *d_workspace, size_t workspace_bytes, void *stream);
int gnnx_rank_counts_f32(int64_t n_pos, int32_t m, const float *d_pos_scores, const float *d_neg_scores, const int32_t *d_neg,
                         int32_t *d_greater, int32_t *d_equal, int32_t *d_valid, void *stream);

/* ------------------------------------------------------------------ random walks ---------------- */
/*
 * Seeded random walks on a CSR: uniform (DeepWalk, Perozzi et al. 2014) and second-order (node2vec, Grover & Leskovec 2016) -- the
 * sampler of the unsupervised objectives (co-occurrence pairs within a window; the loss of GraphSAGE section 3.2).  The contract is this
 * comment, restated with Python integers and plain loops by tests/walk_ref.py.
 *
 * gnnx_csr_random_walk.  The CSR (d_rowptr, d_colidx; n_rows rows, nnz entries) is SQUARE: its columns index its rows.  d_starts
 * [n_walks] holds the start vertices, any order, repeats allowed.  d_walks is walk-major: row x (ldw >= walk_length + 1 elements; all
 * offsets are 64-bit) holds the walk_length + 1 vertices of walk x and nothing behind them is written.  Position 0 is d_starts[x], or
 * -1 when that is outside [0, n_rows); position t + 1 is the result of step t, t = 0 .. walk_length - 1.
 *
 * Random numbers.  fin = splitmix64, the finaliser of the other samplers; G = 0x9E3779B97F4A7C15; products wrap in 64 bits.
 *   s          = fin(seed ^ 0x77616C6B73746570)       "walkstep", a domain constant: independent of the neighbour and the negative
 *                                                     sampler's draws under the same seed
 *   w          = walk_base + x                        the GLOBAL walk number
 *   h(w, t, a) = fin( fin( s ^ (((uint64)w << 32 | (uint64)t) * G) ) ^ ((uint64)a * G) )
 * The key holds w, never the start vertex: repeated starts give independent walks, and a list walked in slices, walk_base set to each
 * slice's offset, gives the slices of one call.
 *
 * Ending.  A step from the current vertex v with d = rowptr[v+1] - rowptr[v]: if v < 0, v >= n_rows or d == 0 the walk has ended and
 * the step's result and every later position are -1 (-1 is absorbing).  So a start outside [0, n_rows) gives a row of -1 from position 0
 * on, a start without neighbours the start followed by -1.  No access is out of range.
 *
 * Uniform step -- step 0 of every walk, and every step when p == 1 && q == 1:
 *   r = floor(h(w, t, 0) * d / 2^64)  (the high 64 bits of the product),   next = colidx[rowptr[v] + r].
 *
 * node2vec step -- otherwise (t >= 1, previous vertex u).  Rows must be STRICTLY ASCENDING, as gnnx_csr_from_coo builds them.  A
 * candidate x of row v belongs to one of three classes with the weights of the paper, turned into integer thresholds on the HOST from
 * doubles:
 *   wa = 1 / p  (x == u)      wb = 1  (x != u and x stored in row u: ONE binary search)      wc = 1 / q  (otherwise)
 *   M = max(wa, wb, wc)       thr_k = min(2^32, (uint64)floor(w_k / M * 4294967296.0))        the largest class gets exactly 2^32
 * Rejection (KnightKing, Yang et al. 2019), attempts a = 0 .. GNNX_WALK_TRIES - 1:
 *   x = colidx[rowptr[v] + floor(h(w, t, 2a) * d / 2^64)],   accepted iff (h(w, t, 2a + 1) >> 32) < thr_class(x);
 * the first accepted candidate is the step.  If none is accepted, the exact fallback -- bounded, no spin:
 *   W = sum over the row's entries j of thr_class(colidx_j), in uint64;
 *   W == 0: the uniform formula with a = 2 * GNNX_WALK_TRIES;
 *   else r = floor(h(w, t, 2 * GNNX_WALK_TRIES) * W / 2^64) and the step is the first entry whose prefix sum of thresholds exceeds r.
 * Both samplers draw from the node2vec distribution up to the 2^-32 quantum of the thresholds, so the trade between them is cost alone.
 * The result is a function of (seed, w, start, graph, p, q) alone, however walks map to lanes.  With p = q = 1 every threshold is 2^32,
 * attempt 0 always accepts and its candidate is the uniform step's: the same bits.
 *
 * Cost.  A uniform step is three dependent loads.  An attempt adds a search of O(log d_u) loads unless wb == wc (q == 1: skipped, the
 * result cannot depend on it).  With min(w) / max(w) >= 1/4 (p, q in [0.5, 2]) a step reaches the fallback with probability
 * <= 0.75^64 ~ 1e-8; at p = 0.25, q = 4 on a sparse graph (most candidates at weight 1/16) it is about (15/16)^64 ~ 1.6 % of the steps,
 * and each such step costs O(d log d_u): the wavefront of the walk stops and scans the row together, 64 entries per pass, one pending
 * walk at a time -- on a power-law graph these steps, not the attempts, set the time.  Results stay exact;
 * scripts/bench_walks.py reports the rate.
 *
 * Statuses.  GNNX_ERR_INVALID_ARG before any device call: negative sizes, walk_length < 0, ldw < walk_length + 1, walk_base < 0 or
 * walk_base + n_walks > 2^32, nnz >= 2^31, p or q not finite or <= 0 (or so small that the reciprocal is not finite), a null rowptr, a
 * null starts or walks with n_walks > 0, a null colidx with nnz > 0.  n_walks == 0 is a valid empty result with no launch;
 * walk_length == 0 copies the starts (those outside [0, n_rows) become -1).  The CSR and nnz (= rowptr[n_rows]) are TRUSTED, as
 * everywhere else.  Asynchronous on `stream`; no workspace, no atomics: the same bits on every run.
 *
 * Kernel (gnnx_walk.hip): one lane per walk, one wavefront per 64 consecutive walks, a grid-stride loop over the walk blocks.  The
 * wavefront stages GNNX_WALK_CHUNK positions of its 64 walks in LDS and stores each walk's piece with adjacent lanes on adjacent words.
 * The attempts run lane by lane; the fallback scans of a step run after them, by all 64 lanes on one walk's row at a time.
 */
#define GNNX_WALK_TRIES 64
#define GNNX_WALK_CHUNK 16
int gnnx_csr_random_walk(int32_t n_rows, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_colidx, const int32_t *d_starts,
                         int64_t n_walks, int64_t walk_base, int32_t walk_length, double p, double q, uint64_t seed, int32_t *d_walks,
                         int64_t ldw, void *stream);

/* ------------------------------------------------------------------ nearest neighbours ---------- */
/*
 * The k nearest neighbours of every query among the candidates of its segment, by exact all-pairs squared Euclidean distances -- the
 * edges of data that arrives as coordinates or features (point clouds; the per-layer graphs of DGCNN, Wang et al. 2019).  The contract is
 * this comment, restated with NumPy float32 steps and Python integer keys by tests/knn_ref.py.
 *
 * gnnx_knn_f32.  Candidates d_X [n, ldx], n_feat used columns.  Queries d_Q [m, ldq]; d_Q == NULL: the queries are the candidates
 * (m == n required, ldq and d_qsegptr ignored).  d_segptr [n_seg + 1] splits the candidates into consecutive groups (the graph_ptr of
 * a graph batch), d_qsegptr [n_seg + 1] the queries; a query of segment b sees the candidates of segment b only.  Both NULL with
 * n_seg == 1: one segment that covers everything.  The arrays are TRUSTED to be non-decreasing from 0 to n (m), like every CSR here.
 *
 * Distance.  Every operation rounded once to float32, ascending feature order, no fused multiply-add (the unit switches contraction
 * off itself, whatever the build's flags):
 *   acc = +0;   for f = 0 .. n_feat - 1:   t = q[f] - c[f];   p = t * t;   acc = acc + p
 * The chain cannot give a negative value or -0.
 *
 * Order.  ukey(d) = 0xFFFFFFFF for a NaN d, else the bit pattern of d;  key(d, c) = (uint64)ukey(d) << 32 | c  with c the candidate's
 * GLOBAL row.  A query keeps the L = min(k, the candidates of its segment -- one fewer with GNNX_KNN_EXCLUDE_SELF when the query's own
 * index lies in the candidate segment) candidates with the smallest keys: a total order, equal distances go to the smaller index, NaN
 * distances come last.  GNNX_KNN_EXCLUDE_SELF drops the candidate whose row equals the query's row; it is meant for d_Q == NULL
 * (pointer identity is not checked).
 *
 * Output.  Row i of d_idx (ldi >= k) holds the L kept rows at positions 0 .. L - 1 and -1 behind them up to k - 1; row i of d_dist
 * (optional, ldd >= k) their distances -- the bits of acc, a NaN as 0x7FC00000 -- and +inf behind them.  Nothing behind position k - 1
 * is written.  The kept entries stand in ASCENDING INDEX order (flattened: a strictly ascending CSR row, what csr_transpose_map and the
 * node2vec step need); with GNNX_KNN_NEAREST_FIRST in ascending key order.  The result is a function of the inputs alone, bit for bit.
 *
 * Statuses.  GNNX_ERR_INVALID_ARG before any device call: negative n or m, n_feat < 1, k < 1 or k > GNNX_KNN_MAX_K, n_seg < 1, unknown
 * flag bits, ldx < n_feat, ldq < n_feat (d_Q given), ldi < k, ldd < k (d_dist given), exactly one segment array NULL while d_Q is given,
 * NULL segment arrays with n_seg != 1, d_Q == NULL with m != n, a NULL d_X with n > 0, a NULL d_idx with m > 0.  m == 0 is a valid
 * empty result with no launch; n == 0 (or an empty segment) fills the rows with -1 / +inf.  Asynchronous on `stream`; no workspace, no
 * atomics.
 *
 * Kernel and dispatch (gnnx_knn.hip) -- a function of the call's arguments alone:
 *   form   n_feat <= GNNX_KNN_REG_FEAT: the query row in NF registers, NF the smallest of {2, 3, 4, 8, 16, 32, 64} >= n_feat, candidate
 *          tiles of GNNX_KNN_TILE rows in LDS.  Beyond: the LDS form, tiles of GNNX_KNN_TILE_LDS rows, 64 features of the tile and of
 *          the queries staged at a time.
 *   group  G lanes per query, each taking every G-th row of a tile, their lists merged at the end:
 *            G = min(Gm, Gs, Gw)   Gm = the smallest power of two <= 64 with m * Gm >= GNNX_KNN_FULL_LANES (four wavefronts per SIMD)
 *                                  Gs = the largest power of two <= 64 with Gs * 2k <= n / n_seg (integer division), at least 1
 *                                  Gw = the largest power of two <= 64 with Gw * NF <= GNNX_KNN_GROUP_FLOATS (NF = 64 in the LDS form)
 *          Gw is a measured bound: only G = 1 reads a tile row as a broadcast, and rows of 64 features are bound by those reads
 *          (G = 2 is the best there, G = 8 slower than G = 1; at n_feat = 3 the best G is Gm's: DESIGN.md section 5.12).
 *   LDS    k * 512 bytes of lists (64 lanes, k keys of 8 bytes) + the tile: (NF + 4) * 256 bytes (NF * 256 below NF = 4), or 21 kB
 *          in the LDS form -- at most 52.5 KiB, checked against the device at the first launch.
 * One wavefront per workgroup and 64 / G consecutive queries; queries of one workgroup in different segments are served one segment
 * after the other.  Numbers: DESIGN.md section 5.12, scripts/bench_knn.py.
 */
#define GNNX_KNN_MAX_K 64
#define GNNX_KNN_EXCLUDE_SELF 1u
#define GNNX_KNN_NEAREST_FIRST 2u
#define GNNX_KNN_REG_FEAT 64
#define GNNX_KNN_TILE 64
#define GNNX_KNN_TILE_LDS 16
#define GNNX_KNN_FULL_LANES 262144
#define GNNX_KNN_GROUP_FLOATS 128
int gnnx_knn_f32(int32_t n, int32_t m, int32_t n_feat, int32_t n_seg, const float *d_X, int64_t ldx, const int32_t *d_segptr,
                 const float *d_Q, int64_t ldq, const int32_t *d_qsegptr, int32_t k, uint32_t flags, int32_t *d_idx, int64_t ldi,
                 float *d_dist, int64_t ldd, void *stream);

/* ------------------------------------------------------------------ halo (multi-GPU) ------------- */
/* Pack rows for the all-to-all-v send buffer: out[k,:] = X[idx[k],:]; and the reverse for backward:
 * Y[idx[k],:] += in[k,:] (idx may repeat across calls but NOT within one call => no atomics, deterministic). */
int gnnx_gather_rows_f32(const float *d_X, int64_t ldx, const int32_t *d_idx, int64_t n_idx, int32_t n_feat,
                         float *d_out, int64_t ldo, void *stream);
int gnnx_scatter_add_rows_f32(const float *d_in, int64_t ldi, const int32_t *d_idx, int64_t n_idx, int32_t n_feat,
                              float *d_Y, int64_t ldy, void *stream);

/* The exchange itself.  Two transports behind one handle:
 *   RCCL  (gnnx_comm_init): one process per GPU; librccl is bound with dlopen at first use.  Every rank creates the
 *         communicator from the same 128-byte id (rank 0 calls gnnx_comm_unique_id and ships it to the others by whatever
 *         channel the host program has).
 *   local (gnnx_comm_init_local): the `world` ranks are threads of ONE process; handles for all ranks are created by one call
 *         and handed to the threads.  Collectives rendezvous on host memory and move data with device copies on each rank's
 *         stream (they synchronise that stream).  Rank threads may drive different GPUs: the all-to-all-v uses device-to-device
 *         copies, the all-reduce reads every peer's buffer from a kernel and enables peer access between the ranks' devices on
 *         first use (GNNX_ERR_UNSUPPORTED where the topology has none: use the RCCL transport there).  Destroying a handle while
 *         peers wait in a collective fails their call instead of hanging it; a collective that completed is never failed by a
 *         peer's later destroy.
 * gnnx_halo_exchange_f32 is the all-to-all-v of the halo step: rows for peer p are send_rows[p] consecutive rows of d_send
 * (peer-major, as gnnx_gather_rows_f32 packs them with the peer-major send list), rows from peer p land as recv_rows[p]
 * consecutive rows of d_recv (the [halo] tail of the feature buffer, halo ids being grouped by owner).  On RCCL: one group of
 * ncclSend/ncclRecv pairs, each pair of GPUs uses its own xGMI link; a failed Send/Recv still closes the group before the
 * error is returned.  send_rows / recv_rows are HOST arrays of `world` entries. */
typedef struct gnnx_comm gnnx_comm;
int gnnx_comm_unique_id(void *id_out_128_bytes);
int gnnx_comm_init(gnnx_comm **comm, int world, int rank, const void *id_128_bytes);
int gnnx_comm_init_local(gnnx_comm **comms_out /* [world] */, int world);
int gnnx_comm_info(const gnnx_comm *comm, int *world, int *rank);
int gnnx_comm_destroy(gnnx_comm *comm);
int gnnx_halo_exchange_f32(gnnx_comm *comm, const float *d_send, const int64_t *send_rows, float *d_recv, const int64_t *recv_rows,
                           int32_t n_feat, void *stream);
int gnnx_allreduce_sum_f32(gnnx_comm *comm, float *d_buf, int64_t n, void *stream);

/* ------------------------------------------------------------------ partition + halo plan -------- */
/*
 * 1-D vertex partition and the halo plan of a shard, built on the device (SURVEY.md 8(b) `gnnx_halo_plan`, 8(e)).  The
 * reference is a single process on a dense N x N matrix and has no counterpart; what these calls must preserve is its
 * SUMMATION ORDER: a row's entries stay sorted by ORIGINAL column id (the CSR build sees original ids) and are renumbered
 * value by value, so a shard's SpMM adds the same terms in the same order as the unsharded one (bit-identical rows).
 *
 *   gnnx_vertex_weights     w[v] = out-degree + in-degree + row_weight (the cost model: one unit per incident edge for the two
 *                           aggregations, row_weight ~ 0.08 F for the three GEMM passes over the row).  Synchronises.
 *   gnnx_partition_deal     vertices in stable descending-weight order (ties: ascending id) are dealt to the ranks in snake
 *                           order (0..P-1, P-1..0, ...): every rank gets n/P +- 1 rows with the same degree mix => equal GEMM
 *                           rows, non-zeros and per-link halo volume.  d_owner[v] = rank; d_nid[v] = new id, rank p owning the
 *                           contiguous new-id range [cuts[p], cuts[p+1]) in ascending original id.  cuts: HOST, world+1
 *                           entries.  world == 1 is the identity.  Synchronises.
 *   gnnx_partition_scramble a second relabelling INSIDE every rank's range: position k of rank p's n_p vertices moves to
 *                           (k * 2654435761) mod n_p (a bijection: the multiplier is a prime above every n_p).  Synthetic power-law
 *                           generators (R-MAT) put the hubs on the ids with few one-bits, i.e. feature rows whose addresses have few
 *                           one-bits: the address bits that select the memory channel / cache slice are mostly zero and the hottest rows pile onto a few
 *                           (10 M / 100 M, F = 256: aggregation 19.0 -> 13.7 ms once the labels are scrambled).  world == 1 with
 *                           d_nid = 0..n-1 gives the single-GPU relabelling (d_owner may be NULL for one rank, and every
 *                           device pointer when n_nodes == 0).  Row contents and summation order are untouched
 *                           (see above): every vertex's result has the same bits, stored at row nid[v].  Synchronises.
 *   gnnx_shard_select_edges the edges rank `rank` owns (owner[src] == rank; transpose != 0: owner[dst] == rank, roles swapped),
 *                           self loops dropped on ORIGINAL ids: d_rows = local row id (nid - lo), d_cols = ORIGINAL column id;
 *                           capacity n_edges each.  Feed them to gnnx_csr_from_coo (n_nodes = max(n_local, n_nodes),
 *                           GNNX_CSR_KEEP_SELF_LOOPS: a local row id may equal an unrelated original column id).  Synchronises.
 *   gnnx_halo_plan_create   from the shard's CSR columns (ORIGINAL ids): halo = sorted new ids of the remote columns (grouped by
 *                           owner), d_colidx_local[p] = column in [local rows | halo rows] numbering (may alias
 *                           d_colidx_orig), recv_rows[q] = halo rows owned by q.  Synchronises.
 *   gnnx_halo_plan_exchange_requests  tells every owner which rows this rank reads (all-to-all of counts, then of the halo
 *                           ids) and stores the peer-major send list; gnnx_halo_plan_set_send_list does the same from ids the
 *                           host program moved itself (d_want_new_ids: peer-major new ids requested by the peers).
 *   gnnx_halo_plan_info     any out pointer may be NULL; recv_rows / send_rows: HOST arrays of `world` entries; d_halo_ids /
 *                           d_send_idx: device pointers owned by the plan.
 *   gnnx_halo_exchange_rows_f32  the per-aggregation step: pack rows [send list] of d_buf[:n_local] into d_send_buf
 *                           ([n_send, n_feat]) and exchange into d_buf[n_local:] (d_buf: [n_local + n_halo, n_feat]).
 */
typedef struct gnnx_halo_plan gnnx_halo_plan;
int gnnx_vertex_weights(const int32_t *d_src, const int32_t *d_dst, int64_t n_edges, int32_t n_nodes, int32_t row_weight,
                        int32_t *d_weight, void *stream);
int gnnx_partition_deal(const int32_t *d_weight, int32_t n_nodes, int world, int32_t *d_owner, int32_t *d_nid, int64_t *cuts_out,
                        void *stream);
int gnnx_partition_scramble(const int32_t *d_owner, int32_t n_nodes, int world, const int64_t *cuts, int32_t *d_nid, void *stream);
int gnnx_shard_select_edges(const int32_t *d_src, const int32_t *d_dst, int64_t n_edges, const int32_t *d_owner, const int32_t *d_nid,
                            int rank, int64_t lo, int transpose, int32_t *d_rows, int32_t *d_cols, int64_t *n_selected, void *stream);
int gnnx_halo_plan_create(const int32_t *d_colidx_orig, int64_t nnz, const int32_t *d_nid, int32_t n_nodes, int world, int rank,
                          const int64_t *cuts, int32_t *d_colidx_local, gnnx_halo_plan **plan, void *stream);
int gnnx_halo_plan_destroy(gnnx_halo_plan *plan);
int gnnx_halo_plan_info(const gnnx_halo_plan *plan, int64_t *n_local, int64_t *n_halo, int64_t *n_send, int64_t *recv_rows,
                        int64_t *send_rows, const int32_t **d_halo_ids, const int32_t **d_send_idx);
int gnnx_halo_plan_set_send_list(gnnx_halo_plan *plan, const int32_t *d_want_new_ids, const int64_t *send_rows, void *stream);
int gnnx_halo_plan_exchange_requests(gnnx_halo_plan *plan, gnnx_comm *comm, void *stream);
/* (the pack inside gnnx_halo_exchange_rows_f32 runs from the producer's side -- gnnx_rows_to_slots_f32 on the plan's own slot table,
 * built by gnnx_halo_plan_set_send_list -- whenever the rows are 16-byte pieces; the gather by the send list otherwise: same buffer) */
int gnnx_halo_exchange_rows_f32(const gnnx_halo_plan *plan, gnnx_comm *comm, float *d_buf, int64_t ldb, int32_t n_feat,
                                float *d_send_buf, void *stream);
/* A producer that packs while it produces (gnnx_gemm_nt_rows_to_slots_f32: the transform's epilogue; gnnx_rows_to_slots_f32 with the
 * column sums: the upstream gradient's dbias pass) takes the plan's slot table ([n_local][8]: a row's slots ascending, packed to the front,
 * -1 behind them; NULL when the plan has none: some local row has more than 7 slots, i.e. more than 7 peers read it -- whatever the
 * number of ranks --, or no send list yet, or no rows to send) and hands the filled send buffer ([n_send][n_feat], dense) to gnnx_halo_exchange_packed_f32 -- the
 * exchange step of gnnx_halo_exchange_rows_f32 without its pack. */
int gnnx_halo_plan_slot_table(const gnnx_halo_plan *plan, const int32_t **d_slots);
int gnnx_halo_exchange_packed_f32(const gnnx_halo_plan *plan, gnnx_comm *comm, float *d_buf, int64_t ldb, int32_t n_feat,
                                  const float *d_send_buf, void *stream);

/* ------------------------------------------------------------------ synthetic inputs ------------- */
/* Counter-based SplitMix64 generators, bit-identical to gnn.cpp_amd/synth.py. */
int gnnx_rmat_edges(uint64_t seed, int32_t n_nodes, int64_t n_edges, int64_t first_edge, double a, double b,
                    double c, int32_t *d_src, int32_t *d_dst, void *stream);
int gnnx_uniform_pm1_f32(uint64_t seed, int64_t n, float scale, float *d_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNX_H */
