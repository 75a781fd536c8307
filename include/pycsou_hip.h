/*
 * pycsou_hip.h -- C ABI of libpycsou_hip.so, the gfx950 (MI355X) engine behind
 * the pycsou PrimalDualSplitting / APGD hot path.
 *
 * Conventions
 *  - Buffers are caller-allocated DEVICE pointers, contiguous, C order (the
 *    flat-vector layout pycsou uses: a d-dimensional image of `shape` is the
 *    C-order ravel; a gradient is the concatenation [d_0 x; d_1 x; (d_2 x)],
 *    pycsou/linop/diff.py:855-875).
 *  - `dtype` is PCS_F32 or PCS_F64.  Scalars are passed as double and rounded
 *    to `dtype` inside, exactly as NumPy does for `array * python_float`.
 *  - Every entry point returns PCS_OK (0) or a negative status; nothing is
 *    thrown across the ABI.  No entry point allocates, frees or synchronises:
 *    all of them are hipGraph-capturable on `stream`.
 *  - Workspaces (`ws`) are caller-allocated device buffers of the size the
 *    matching *_ws_bytes() query returns.
 *  - Caller-owned scratch (ws, partials, the control block, the history): the
 *    advertised size is all a call touches -- nothing is read or written past
 *    it -- and every such argument says what its contents on entry mean:
 *    "contents on entry: arbitrary" (every slot a call reads it has written
 *    first; the buffer may be shared by successive calls on one stream) or
 *    "zeroed once before first use" (the call keeps counters there and leaves
 *    them at zero).  Contents on return are unspecified unless stated.
 *    INTEGRATION.md lists every such buffer with size, alignment and contents.
 *
 * Each entry point names the reference interface it replaces (file:line in
 * dhamm97/pycsou; PyLops 1.x for the operators pycsou delegates to it).
 */
#ifndef PYCSOU_HIP_H
#define PYCSOU_HIP_H

#include <stdint.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { PCS_F32 = 0, PCS_F64 = 1 };
enum { PCS_OK = 0, PCS_EINVAL = -1, PCS_ELAUNCH = -2, PCS_EUNSUPPORTED = -3 };
/* derivative kinds (pycsou/linop/diff.py:24 `kind`) */
enum { PCS_FORWARD = 0, PCS_BACKWARD = 1, PCS_CENTERED = 2 };
/* H functional kinds in the fused step */
enum { PCS_H_L1 = 0, PCS_H_L21 = 1 };
/* G functional kinds in the fused step */
enum { PCS_G_NULL = 0, PCS_G_NONNEG = 1, PCS_G_SEGMENT = 2 };
/* F kinds in the fused step */
enum { PCS_F_NULL = 0, PCS_F_DENOISE = 1, PCS_F_SEPCONV = 2, PCS_F_GRADBUF = 3, PCS_F_CONV2D = 4, PCS_F_CONV0 = 5 };
/* finite-difference K of the fused 2-D steps */
enum { PCS_K_GRAD_FORWARD = 0, PCS_K_GRAD_BACKWARD = 1, PCS_K_GRAD_CENTERED = 2, PCS_K_LAPLACIAN = 3 };

int pcs_abi_version(void);

/* ---------------------------------------------------------------- operators */

/* FirstDerivative along `axis` (pycsou/linop/diff.py:24-130 -> pylops.FirstDerivative):
 * out = D_axis x.  ndim in 1..32, dims[ndim], step = sampling. */
int pcs_deriv1_fwd(int dtype, const void* x, void* out, int ndim, const int64_t* dims, int axis, double step,
                   int kind, int edge, hipStream_t stream);
/* Adjoint of the above (pylops FirstDerivative.rmatvec). */
int pcs_deriv1_adj(int dtype, const void* y, void* out, int ndim, const int64_t* dims, int axis, double step,
                   int kind, int edge, hipStream_t stream);

/* SecondDerivative along `axis` (pycsou/linop/diff.py:133-219 -> pylops.SecondDerivative):
 * out[i] = (x[i+1] - 2 x[i] + x[i-1]) / step^2 inside; ends 0, or the one-sided second-order
 * stencils with `edge`.  ndim in 1..32. */
int pcs_deriv2_fwd(int dtype, const void* x, void* out, int ndim, const int64_t* dims, int axis, double step,
                   int edge, hipStream_t stream);
int pcs_deriv2_adj(int dtype, const void* y, void* out, int ndim, const int64_t* dims, int axis, double step,
                   int edge, hipStream_t stream);

/* Gradient (pycsou/linop/diff.py:777-882 -> pylops.Gradient = VStack of FirstDerivative):
 * out[k*N:(k+1)*N] = D_k x for k < ndim (1..32; one launch per axis beyond 3).  steps[ndim]. */
int pcs_grad_fwd(int dtype, const void* x, void* out, int ndim, const int64_t* dims, const double* steps,
                 int kind, int edge, hipStream_t stream);
/* Gradient.adjoint: out = sum_k D_k^T z_k (accumulated in axis order, pylops VStack.rmatvec). */
int pcs_grad_adj(int dtype, const void* z, void* out, int ndim, const int64_t* dims, const double* steps,
                 int kind, int edge, hipStream_t stream);

/* Laplacian 2-D (pycsou/linop/diff.py:885-957 -> pylops.Laplacian):
 * out = w0 * D2_0 x + w1 * D2_1 x.  dims[2], weights[2], steps[2]. */
int pcs_lap_fwd(int dtype, const void* x, void* out, const int64_t* dims, const double* weights,
                const double* steps, int edge, hipStream_t stream);
int pcs_lap_adj(int dtype, const void* y, void* out, const int64_t* dims, const double* weights,
                const double* steps, int edge, hipStream_t stream);

/* FirstDirectionalDerivative (pycsou/linop/diff.py:380-486 -> pylops 1.x Sum(axis 0) * Diagonal(v) *
 * Gradient), one launch: out[p] = scale * ((v_0[p] (D_0 x)[p] + v_1[p] (D_1 x)[p]) + v_2[p] (D_2 x)[p]),
 * ndim in 1..3, steps[ndim].  `v` is a device buffer of dtype: ndim scalars (v_is_field == 0) or ndim * N
 * values in [k][p] order.  `kill` is 0 or 2: outputs within `kill` samples of either end of any axis are
 * written as 0 (the kill-edge mask of SecondDirectionalDerivative, diff.py:598-605; an axis shorter than
 * 2 * kill zeroes everything).  The adjoint is out = scale * sum_k D_k^T (v_k . y), accumulated in axis
 * order as pcs_grad_adj, with the same `kill` on its output.  With them SecondDirectionalDerivative
 * = mask . (-Dv^T Dv) is pcs_dirderiv_fwd followed by pcs_dirderiv_adj(scale = -1, kill = 2).
 * x == out is rejected; a negative dim is PCS_EINVAL, a zero dim an empty array (0, no launch).
 * Arguments are checked before any device call; nothing allocates or synchronises. */
int pcs_dirderiv_fwd(int dtype, const void* x, const void* v, int v_is_field, void* out, int ndim,
                     const int64_t* dims, const double* steps, int kind, int edge, double scale, int kill,
                     hipStream_t stream);
int pcs_dirderiv_adj(int dtype, const void* y, const void* v, int v_is_field, void* out, int ndim,
                     const int64_t* dims, const double* steps, int kind, int edge, double scale, int kill,
                     hipStream_t stream);

/* Integration1D (pycsou/linop/diff.py:1071-1137 -> pylops 1.x CausalIntegration, halfcurrent=False):
 * out[i] = step * sum_{j <= i} x[j] along `axis` of a C-order array (ndim in 1..32), or with
 * reverse != 0 the adjoint step * sum_{j >= i} x[j] (indexed backwards, no flipped copy).  Sums are
 * carried in fp64 for both dtypes and multiplied by `step` last.  The axis is seen as the middle of
 * (outer, n, inner): inner > 1 marches threads along n with coalesced loads across inner; inner == 1
 * scans each line with wave-level shuffles and a carried prefix.  When there are too few lines to fill
 * the device a line is cut into segments of at least PCS_CUMSUM_SPAN (inner == 1) or
 * PCS_CUMSUM_SPAN_STRIDED (inner > 1) samples and handled reduce-then-scan in three launches (segment
 * totals into ws, a scan of the totals, the offset scan); no workgroup ever waits for another.  ws then
 * holds pcs_cumsum_ws_bytes(ndim, dims, axis) bytes, 8-byte aligned (the function returns 0 when no
 * workspace is needed -- ws may then be NULL --, -1 on bad arguments, and never decreases in the axis
 * length; it stays below PCS_CUMSUM_WS_MAX for any shape; contents on entry: arbitrary).  x == out is allowed: every sample is read and written by the same
 * thread.  A negative dim is PCS_EINVAL, a zero dim an empty array (0, no launch). */
#define PCS_CUMSUM_SPAN 2048
#define PCS_CUMSUM_SPAN_STRIDED 64
#define PCS_CUMSUM_WS_MAX (2 * 1024 * 1024 + 64 * 1024)
int64_t pcs_cumsum_ws_bytes(int ndim, const int64_t* dims, int axis);
int pcs_cumsum(int dtype, const void* x, void* out, int ndim, const int64_t* dims, int axis, double step,
               int reverse, void* ws, hipStream_t stream);

/* Convolve2D (pycsou/linop/conv.py:167-295 -> pylops Convolve2D, 'same', zero boundary):
 * out[i] = sum_j h[j] x[i + off - j] (+ beta * b[i] if b != NULL).  `psf` is a device
 * buffer kh*kw of dtype.  The adjoint (correlation) is this call with the flipped PSF
 * and offsets (kh-1-off0, kw-1-off1). */
int pcs_conv2d(int dtype, const void* x, void* out, int64_t n0, int64_t n1, const void* psf, int kh, int kw,
               int off0, int off1, const void* b, double beta, hipStream_t stream);
/* x == out is rejected (PCS_EINVAL); b == out is allowed.  Odd square PSFs centred at
 * (kh/2, kw/2) of size 3..15 or 31 run the register-blocked marching kernel (corr2d.hip);
 * other shapes run the LDS-tiled kernel, or use the plan entry points below. */

/* Convolve2D through a packed plan (same operator, any PSF up to 31 x 31): every call is
 * one correlation with a K x K window centred at K/2, K = the "tier" (odd, 3..15 or 31)
 * returned by pcs_conv2d_plan_tier (< 0: unsupported).  pcs_conv2d_plan_pack is a HOST
 * function: it writes the forward (adjoint = 0) or adjoint (adjoint = 1) window of the
 * fp64 host PSF into a host buffer of pcs_conv2d_plan_bytes bytes of `dtype`, which the
 * caller copies to the device once.  pcs_conv2d_planned then computes
 *   out = Conv(x) (+ beta * b)  (plan of adjoint = 0)  or  Conv^T(x) (+ beta * b)  (adjoint = 1)
 * Same arithmetic as pcs_conv2d up to floating-point summation order.  x != out. */
int pcs_conv2d_plan_tier(int kh, int kw, int off0, int off1);
int64_t pcs_conv2d_plan_bytes(int dtype, int kh, int kw, int off0, int off1);
int pcs_conv2d_plan_pack(int dtype, const double* psf, int kh, int kw, int off0, int off1, int adjoint,
                         void* plan_host);
int pcs_conv2d_planned(int dtype, const void* x, void* out, int64_t n0, int64_t n1, const void* plan, int tier,
                       const void* b, double beta, hipStream_t stream);

/* Convolve1D along `axis` of a 1..32-D array (pycsou/linop/conv.py:20-164 -> pylops Convolve1D):
 * out[i] = sum_t h[t] x[i + (off - t) e_axis].  Adjoint = flipped taps, off' = k-1-off. */
int pcs_conv1d(int dtype, const void* x, void* out, int ndim, const int64_t* dims, int axis, const void* taps,
               int k, int off, hipStream_t stream);

/* Two Convolve1D of a 3-D array's planes in one pass (pycsou/linop/conv.py:20-164 along axes 1
 * and 2): C_a along axis 1 (taps ha, ka, offa), C_b along axis 2 (taps hb, kb, offb), both with
 * pcs_conv1d's definition; out = C_b(C_a(in)) if vfirst else C_a(C_b(in)) (the two pcs_conv1d
 * calls in that order, same per-output sums to rounding).  in != out, 16-B aligned; ka, kb <= 15. */
int pcs_conv2d_sep_planes(int dtype, const void* in, void* out, int64_t nplanes, int64_t n1, int64_t n2,
                          const void* ha, int ka, int offa, const void* hb, int kb, int offb, int vfirst,
                          hipStream_t stream);

/* In-plane normal operator of a separable blur, every plane in one pass (pycsou/linop/conv.py:20-164
 * along axes 1 and 2; the in-plane half of grad F = C^T (C x - y), core/map.py:609-610):
 *   out = C_a^T C_b^T C_b C_a in   (C_a along axis 1: ha, ka, offa; C_b along axis 2: hb, kb, offb;
 *                                   zero boundary between the passes, as the four pcs_conv1d calls)
 * in != out, 16-B aligned, ka, kb <= 15.  PCS_EUNSUPPORTED when n2 % 4 != 0 or the horizontal
 * offset cannot be fitted to the strip layout (15-tap filter with offb % 4 == 1); nplanes == 0
 * only validates. */
int pcs_conv2d_sep_ata_planes(int dtype, const void* in, void* out, int64_t nplanes, int64_t n1, int64_t n2,
                              const void* ha, int ka, int offa, const void* hb, int kb, int offb, hipStream_t stream);

/* FFT-domain Convolve2D (pycsou/linop/conv.py:167-295, method='fft': scipy.signal.fftconvolve,
 * mode 'same' at pycsou's offset), for PSFs of any size at a cost independent of the PSF:
 *   forward out[i] = sum_j h[j] x[i + off - j] (+ beta b[i]);  adjoint out[i] = sum_j h[j] x[i - off + j]
 * (zero boundary; kh x kw PSF h in host fp64, row-major; offsets off0 < kh, off1 < kw).  Overlap-add
 * over blocks of at most 2048 x 2048 samples: the plan holds batched rocFFT R2C / C2R plans on a
 * zero-padded P0 x P1 grid per block (P = pcs_fftconv2d_grid(n, k): the smallest even 2-3-5-7-smooth
 * size >= block + k - 1, so the circular transforms are exact linear ones), their work buffer and
 * the PSF spectrum (formed at creation; create synchronises).
 * pcs_fftconv2d_apply: x != out, device arrays of n0*n1 (b may be NULL); stream-ordered, no
 * allocation (graph-capturable).  One plan per (dtype, shape, PSF); not thread-safe per plan. */
int64_t pcs_fftconv2d_grid(int64_t n, int k);
int pcs_fftconv2d_create(int dtype, int64_t n0, int64_t n1, const double* h, int kh, int kw, int off0, int off1,
                         void** handle);
int pcs_fftconv2d_apply(void* handle, const void* x, void* out, int adjoint, const void* b, double beta,
                        hipStream_t stream);
int pcs_fftconv2d_destroy(void* handle);

/* The axis-0 stage of grad F = C^T (C x - y) for a 3-D Convolve1D chain, in one pass
 * (pycsou/linop/conv.py:20-164 along axis 0, residual of core/map.py:609-610): on sub-volumes
 * of nsub planes of `plane` elements,
 *   r[p] = sum_t h[t] t[p + off - t] - y[p]  for p in [img_lo, img_hi) n [0, nsub) (0 elsewhere;
 *          t = 0 outside [0, nsub)),
 *   s[q] = sum_t h[k-1-t] r[q + k-1-off - t]  written for q in [q0, q1) only.
 * = pcs_conv1d(axis 0) + pcs_axpby(1, -1) + pcs_conv1d(axis 0, flipped) with 3 instead of 7
 * sub-volume passes.  k <= 15. */
int pcs_conv0_residual_adjoint(int dtype, const void* t, const void* y, void* s, int64_t nsub, int64_t plane,
                               const void* taps, int k, int off, int64_t img_lo, int64_t img_hi, int64_t q0,
                               int64_t q1, hipStream_t stream);

/* Masking / DownSampling / SubSampling (pycsou/linop/sampling.py:25-391).
 * pcs_gather:          out[i] = x[idx[i]], i < m         (Masking.__call__, sampling.py:192-193)
 * pcs_gather_or_zero:  out[p] = inv[p] >= 0 ? y[inv[p]] : 0, p < n
 *                      = (x = 0; x[idx] = y) with inv the inverse index map (Masking.adjoint,
 *                      sampling.py:195-198).  Indices are int32 (n < 2^31). */
int pcs_gather(int dtype, const void* x, const int32_t* idx, void* out, int64_t m, hipStream_t stream);
int pcs_gather_or_zero(int dtype, const void* y, const int32_t* inv, void* out, int64_t n, hipStream_t stream);

/* CSR sparse matrix-vector product out = A x (SparseLinearOperator, pycsou/linop/base.py:121-137 ->
 * csr_matrix.dot; the sparse MappedDistanceMatrix, sampling.py:975-1007; the adjoint of NNSampling,
 * sampling.py:680-687).  A is nrows x ncols with nnz entries: rowptr[nrows + 1] int64, colind[nnz] int32
 * (ncols < 2^31), vals[nnz] and x[ncols] of `dtype`; out[nrows] must not overlap x.  A transposed product is
 * this entry point on the CSR of A^T, which the caller builds once.
 *  - `lanes` (a power of two in 1..64, chosen once per matrix from nnz / nrows) lanes serve one row of at
 *    most PCS_SPMV_LONG_ROW entries: lane j adds entries j, j + lanes, ... in order, then a fixed xor tree.
 *  - Every longer row is cut by the caller into chunks of PCS_SPMV_CHUNK entries (the last one shorter), listed
 *    row by row: chunk c covers entries chunk_start[c] .. of row chunk_row[c]; long row i is long_row[i] and
 *    owns chunks long_first[i] .. long_first[i + 1] - 1 (long_first has nlong + 1 entries, all four lists are
 *    int64 device arrays).  One workgroup sums one chunk into partials[c] (nchunks doubles, 8-byte aligned,
 *    contents on entry: arbitrary), then one thread per long row adds its partials in chunk order.  A row of more than PCS_SPMV_LONG_ROW
 *    entries that is not listed is left unwritten.
 * Sums are carried in fp64 and rounded once.  The order of every sum depends on (rowptr, lanes) alone, so two
 * calls return the same bits; there are no atomics.  Empty matrices and empty rows are legal (an empty row
 * gives 0); colind, vals and x may be null when nnz == 0.  PCS_EINVAL before any device call for a null
 * pointer, a negative size, ncols >= 2^31, lanes not a power of two in 1..64, an unknown dtype, chunk lists
 * that cannot belong to nnz entries, or out overlapping x.  The device arrays are trusted: the caller
 * validates rowptr, colind and the chunk lists on the host when it builds them. */
#define PCS_SPMV_LONG_ROW 4096
#define PCS_SPMV_CHUNK 4096
int pcs_csr_spmv(int dtype, int64_t nrows, int64_t ncols, int64_t nnz, const int64_t* rowptr, const int32_t* colind,
                 const void* vals, const void* x, void* out, int lanes, int64_t nchunks, const int64_t* chunk_row,
                 const int64_t* chunk_start, int64_t nlong, const int64_t* long_row, const int64_t* long_first,
                 void* partials, hipStream_t stream);

/* CSR matrix times a row-major dense matrix along one of its axes (csrc/spmm.hip; the sparse factors of
 * KroneckerProduct / KroneckerSum, pycsou/linop/base.py:715-886).  A and its chunk lists are those of
 * pcs_csr_spmv; nb is the length of the other axis of X.
 *   axis 0:  out (nrows x nb) = A X,    X (ncols x nb): min(64, nb rounded up to a power of two) lanes across the columns of one row,
 *            each walking the row's entries in order (rows of any length; the chunk lists are not used).
 *   axis 1:  out (nb x nrows) = X A^T,  X (nb x ncols): the kernels of pcs_csr_spmv with the batch on grid y;
 *            partials holds nb * nchunks doubles (partials_len >= that; 8-byte aligned, contents on entry:
 *            arbitrary), batch row b the bits of pcs_csr_spmv.  Axis 0 with nb > 1 does not touch partials.
 *   nb == 1: either axis is that vector product, bit for bit pcs_csr_spmv (and needs its partials).
 * accumulate = 1: out = out + ..., rounded once ((T)((double)out + sum)).  Sums in fp64, no atomics, every order
 * a function of (rowptr, lanes, axis, nb == 1) alone.  PCS_EINVAL before any device call for what pcs_csr_spmv
 * rejects, an axis or accumulate outside {0, 1}, a negative nb, a partials workspace too small for nb rows, or
 * out overlapping X.  nrows == 0 or nb == 0 is an empty product (0, no launch). */
int pcs_csr_spmm(int dtype, int axis, int accumulate, int64_t nrows, int64_t ncols, int64_t nnz, const int64_t* rowptr,
                 const int32_t* colind, const void* vals, const void* X, void* out, int64_t nb, int lanes,
                 int64_t nchunks, const int64_t* chunk_row, const int64_t* chunk_start, int64_t nlong,
                 const int64_t* long_row, const int64_t* long_first, void* partials, int64_t partials_len,
                 hipStream_t stream);

/* Khatri-Rao product of two dense row-major factors A (k x l) and B (n x l) (csrc/khatri_rao.hip;
 * KhatriRaoProduct, pycsou/linop/base.py:889-989):
 *   pcs_khatri_rao_fwd:  out (n x k, row-major) = (B * x[None, :]) A^T
 *   pcs_khatri_rao_adj:  out[c] = B[:, c]^T Y A[:, c],  Y (n x k, row-major)
 * for k * n <= PCS_KR_MAX_NK and k + n <= PCS_KR_MAX_ROWS (the LDS and register budget derived in the source
 * file); the caller composes larger products.  The forward cuts the l columns into slabs of PCS_KR_SLAB;
 * workgroup g of `ngroups` = ceil(nslabs / spg) <= PCS_KR_MAX_GROUPS sums `spg` consecutive slabs in column
 * order into partials[g * n k ..] (ngroups * n * k doubles, partials_len >= that; 8-byte aligned, contents on
 * entry: arbitrary), and a second kernel adds the groups in order.  Sums in fp64, rounded once, no atomics; the bits depend on (k, n, l, spg) alone.
 * PCS_EINVAL before any device call for an unknown dtype, a negative size, a shape past the limits, a plan that
 * does not tile l, a null or misaligned or short workspace, a null array, or out overlapping an input. */
#define PCS_KR_SLAB 64
#define PCS_KR_MAX_NK 1024
#define PCS_KR_MAX_ROWS 120
#define PCS_KR_MAX_GROUPS 512
int pcs_khatri_rao_fwd(int dtype, const void* A, const void* B, const void* x, void* out, int64_t k, int64_t n,
                       int64_t l, int64_t spg, int64_t ngroups, void* partials, int64_t partials_len,
                       hipStream_t stream);
int pcs_khatri_rao_adj(int dtype, const void* A, const void* B, const void* Y, void* out, int64_t k, int64_t n,
                       int64_t l, hipStream_t stream);

/* Green functions (pycsou/math/green.py) and the matrix-free MappedDistanceMatrix built on them
 * (csrc/green_core.hpp, csrc/mdm.hip; pycsou/linop/sampling.py:772-1058).  A function is (kind, k, p0, p1):
 *   PCS_GREEN_MATERN / PCS_GREEN_WENDLAND   k in 0..3, p0 = epsilon > 0
 *   PCS_GREEN_SUBGAUSSIAN                   p0 = alpha in (0, 2), p1 = epsilon > 0 (k unused)
 *   PCS_GREEN_CAUSAL_ITER                   k >= 1:  t^(k-1) [t >= 0]
 *   PCS_GREEN_CAUSAL_EXP                    k >= 1, p0 = alpha > 0:  t^(k-1) exp(-alpha t) [t >= 0]
 * Negative arguments as NumPy: the causal mask gives 0, SubGaussian NaN, Matern and Wendland their formulas.
 *   pcs_green_eval:  out[i] = phi(r[i])  (out == r allowed).
 *   pcs_mdm_apply:   out[i] = sum_j phi(d(P_i, Q_j)) x[j],  P (nrows x dim), Q (ncols x dim) row-major,
 *                    dim in 1..PCS_MDM_MAX_DIM; the adjoint is the same call with P and Q exchanged.
 *                    PCS_MDM_RADIAL: d = ||P_i - Q_j||_ord, any ord > 0 (1, 2 and +inf have fast paths, otherwise
 *                    (sum |.|^ord)^(1/ord));  PCS_MDM_ZONAL: d = clip(<P_i, Q_j>, -1, 1), ord ignored.
 * fp32: d and phi in fp32 with sqrtf / expf / powf; fp64: in fp64.  In both every product phi * x and every sum is
 * carried in fp64 and rounded once at the store.  nrows > PCS_MDM_SMALL_ROWS: the row form (a 256-thread
 * workgroup owns PCS_MDM_ROWS rows, lane = row, columns staged in LDS PCS_MDM_SLAB at a time); otherwise the column
 * form (lane = column, one fp64 accumulator per row and lane).  The max(ceil(ncols / PCS_MDM_SLAB), 1) slabs are
 * split into `ngroups` <= PCS_MDM_MAX_GROUPS groups of `spg` consecutive slabs, ngroups = ceil(slabs / spg) (the
 * caller's plan).  ngroups == 1 stores directly and does not touch partials; otherwise group g writes
 * partials[g * nrows + i] (pcs_mdm_partials_len doubles, partials_len >= that; 8-byte aligned, contents on entry:
 * arbitrary) and a second kernel adds the groups in group order.  No atomics; the bits depend on (nrows, ncols,
 * dim, spg, ngroups) and the data alone.  pcs_mdm_partials_len: ngroups * nrows, 0 for ngroups == 1, -1 for sizes
 * or a group count pcs_mdm_apply rejects.
 * PCS_EINVAL before any device call for an unknown dtype, kind or mode, parameters outside the ranges above, ord <= 0
 * or NaN in radial mode, dim outside 1..PCS_MDM_MAX_DIM, a negative size or one of 2^31 or more, a plan that does
 * not tile the slabs or has more than PCS_MDM_MAX_GROUPS groups, a null or misaligned or short partials when
 * ngroups > 1, a null array, or out (or partials) overlapping an input.  nrows == 0 is a no-op; ncols == 0 writes
 * zeros. */
#define PCS_GREEN_MATERN 0
#define PCS_GREEN_WENDLAND 1
#define PCS_GREEN_SUBGAUSSIAN 2
#define PCS_GREEN_CAUSAL_ITER 3
#define PCS_GREEN_CAUSAL_EXP 4
#define PCS_MDM_RADIAL 0
#define PCS_MDM_ZONAL 1
#define PCS_MDM_MAX_DIM 4        /* a row's point lives in registers */
#define PCS_MDM_ROWS 64          /* rows per workgroup, row form: one lane per row */
#define PCS_MDM_SLAB 256         /* columns staged in LDS at a time */
#define PCS_MDM_SMALL_ROWS 16    /* at most this many rows: column form */
#define PCS_MDM_MAX_GROUPS 1024
int pcs_green_eval(int dtype, int kind, int k, double p0, double p1, const void* r, void* out, int64_t n,
                   hipStream_t stream);
int pcs_mdm_apply(int dtype, int kind, int k, double p0, double p1, int mode, double ord, int dim, const void* P,
                  int64_t nrows, const void* Q, int64_t ncols, const void* x, void* out, int64_t spg, int64_t ngroups,
                  void* partials, int64_t partials_len, hipStream_t stream);
int64_t pcs_mdm_partials_len(int64_t nrows, int64_t ncols, int64_t ngroups);

/* Block pooling of a C-order array of ndim in 1..3 axes (Pooling, pycsou/linop/sampling.py:394-536 ->
 * skimage.measure.block_reduce with cval = 0) and its unpooling (Pooling.adjoint, np.repeat and crop).
 * dims[ndim] is the shape of the UNPOOLED array in both calls, block[ndim] >= 1 the block sizes; the pooled
 * array has ceil(dims[k] / block[k]) entries per axis.
 *   pcs_pool_fwd:  out[b] = scale * (sum of x over the real cells of block b)   -- a ragged block is zero padded
 *   pcs_pool_adj:  out[p] = scale * y[block of p]
 * Fixed summation order in fp64, no atomics; a block may be wider than a workgroup or larger than its axis.
 * x == out is rejected; a negative dim or a block < 1 is PCS_EINVAL, a zero dim an empty array (0, no launch). */
int pcs_pool_fwd(int dtype, const void* x, void* out, int ndim, const int64_t* dims, const int64_t* block,
                 double scale, hipStream_t stream);
int pcs_pool_adj(int dtype, const void* y, void* out, int ndim, const int64_t* dims, const int64_t* block,
                 double scale, hipStream_t stream);

/* ---------------------------------------------------------------- prox / functionals */

/* L1Norm.prox (pycsou/func/penalty.py:194-245 via LpNorm.prox, func/base.py:239-240):
 * out = x - tau*clip(x/tau, -1, 1). */
int pcs_prox_l1(int dtype, const void* x, void* out, int64_t n, double tau, hipStream_t stream);
/* (lam*L1Norm).fenchel_prox (core/functional.py:207, 264-265):
 * out = w - sigma * prox_l1(w/sigma, (1/sigma)*lam). */
int pcs_fenchel_l1(int dtype, const void* w, void* out, int64_t n, double sigma, double lam, hipStream_t stream);
/* L21Norm.prox with pixel groups tile(arange(npix), d) (func/penalty.py:551-557):
 * out_g = max(1 - tau/||x_g||, 0) x_g. */
int pcs_prox_l21_pixel(int dtype, const void* x, void* out, int64_t npix, int d, double tau, hipStream_t stream);
int pcs_fenchel_l21_pixel(int dtype, const void* w, void* out, int64_t npix, int d, double sigma, double lam,
                          hipStream_t stream);
/* L21Norm.prox with arbitrary labels: `gid[n]` = index of the element's group in
 * [0, ngroups) (np.unique order); ws = ngroups doubles (8-byte aligned, contents on entry: arbitrary -- the
 * call clears it). */
int pcs_prox_l21_labels(int dtype, const void* x, void* out, int64_t n, const int32_t* gid, int64_t ngroups,
                        double tau, void* ws, hipStream_t stream);
/* The same prox with run-to-run identical group sums (ABI 10; replaces pcs_prox_l21_labels in
 * L21Norm.prox, func/penalty.py:525-560): `order[n]` lists the elements group by group (a stable
 * argsort of gid), `off[ngroups + 1]` the group boundaries in it, `maxlen` the largest group; each
 * group's sum of squares is taken in ascending element order (fp64) without atomics.  ws = ngroups doubles
 * (8-byte aligned, contents on entry: arbitrary). */
int pcs_prox_l21_groups(int dtype, const void* x, void* out, int64_t n, const int32_t* gid, int64_t ngroups,
                        const int32_t* order, const int64_t* off, int64_t maxlen, double tau, void* ws,
                        hipStream_t stream);
/* L2Norm.prox (func/penalty.py:23-70 via LpNorm.prox + proj_l2_ball, math/prox.py:207-210):
 * v = x/tau; out = x - tau*(||v|| <= 1 ? v : v/||v||), with ||x||^2 read from the device
 * double `sumsq_dev` (pcs_reduce kind 0). */
int pcs_prox_l2(int dtype, const void* x, void* out, int64_t n, double tau, const double* sumsq_dev,
                hipStream_t stream);
/* SquaredL2Norm prox (new API, core/functional.py:100-103): out = x / (1 + 2 tau). */
int pcs_prox_sql2(int dtype, const void* x, void* out, int64_t n, double tau, hipStream_t stream);
/* NonNegativeOrthant / Segment projections (math/prox.py:295-297, 340-343). */
int pcs_proj_nonneg(int dtype, const void* x, void* out, int64_t n, hipStream_t stream);
int pcs_proj_segment(int dtype, const void* x, void* out, int64_t n, double a, double b, hipStream_t stream);
/* KLDivergence.prox (pycsou/func/loss.py:682): out = (d + sqrt(d^2 + 4 tau y)) / 2, d = x - tau; for d < 0
 * the same root as 2 tau y / (sqrt(.) - d), which does not cancel -- more accurate than the reference
 * there, and exactly 0 for y = 0, d <= 0 as in the reference.  fp64 arithmetic for both dtypes; tau > 0. */
int pcs_prox_kl(int dtype, const void* x, const void* y, void* out, int64_t n, double tau, hipStream_t stream);
/* LogBarrier.prox (func/penalty.py:840): out = (x + sqrt(x^2 + 4 tau)) / 2, for x < 0 as
 * 2 tau / (sqrt(.) - x) (more accurate than the reference there).  tau > 0. */
int pcs_prox_logbarrier(int dtype, const void* x, void* out, int64_t n, double tau, hipStream_t stream);
/* ShannonEntropy.prox (func/penalty.py:921-922): out = tau W0(exp(x / tau - 1) / tau), evaluated in the log
 * domain: out = tau w with w + ln w = x / tau - 1 - ln tau.  Underflows to 0 like the reference for very
 * negative x / tau.  Deliberate deviation: stays finite where the reference's exp overflows to inf
 * (x / tau >~ 709).  tau > 0. */
int pcs_prox_entropy(int dtype, const void* x, void* out, int64_t n, double tau, hipStream_t stream);

/* One global threshold (pycsou/math/prox.py:158-164 proj_l1_ball, func/base.py:239-240 with it for
 * LInftyNorm.prox, func/penalty.py:296-316 SquaredL1Norm.prox; the reference searches on the host with
 * brentq or a full sort):
 *   t = 0 if sum |x_i| <= a, else the root t > 0 of sum max(|x_i| - t, 0) = a + b t
 *   (a >= 0, b >= 0, not both 0), i.e. t = (S_k - a) / (k + b) over the k elements above the crossing;
 *   mode PCS_THRESH_SOFT: out = sign(x) max(|x| - t, 0)   (t = 0: a bitwise copy of x)
 *   mode PCS_THRESH_CLIP: out = clip(x, -t, t)            (t = 0: zeros)
 * L1Ball(r).prox: a = r, b = 0, SOFT.  LInftyNorm.prox(x, tau): a = tau, b = 0, CLIP.
 * SquaredL1Norm.prox(x, tau): a = 0, b = 1 / (2 tau), SOFT (the 'sort' threshold 2 tau / (1 + 2 tau k) S_k).
 * The crossing is located exactly, by 32-section of the ordered bit patterns of |x| down to two adjacent
 * representable values (7 passes fp32, 13 fp64), not to a tolerance in value; all sums are fp64 in a fixed
 * order, so two calls agree bitwise.  19 (fp32) / 31 (fp64) plain launches whatever the data, no host
 * read-back, no atomics: capturable in a hipGraph.  t_dev (device double, may be NULL) receives t.
 * ws >= pcs_thresh_ws_bytes(n) (which never decreases in n), 8-byte aligned, contents on entry: arbitrary.  x == out is allowed.  Arguments are checked before any
 * device call; n = 0 is a no-op. */
enum { PCS_THRESH_SOFT = 0, PCS_THRESH_CLIP = 1 };
#define PCS_THRESH_PIVOTS 31
int64_t pcs_thresh_ws_bytes(int64_t n);
int pcs_thresh_l1(int dtype, const void* x, void* out, int64_t n, double a, double b, int mode, double* t_dev,
                  void* ws, hipStream_t stream);
/* Host-only: one bracket selection of pcs_thresh_l1's stage 2 (the same __host__ __device__ code).  The
 * bracket [lo, hi] of keys (bit patterns of |x| in `dtype`) has pivots j = 1 .. PCS_THRESH_PIVOTS at
 * lo + j ceil((hi - lo) / 32), clamped to hi; pivots_out (may be NULL) receives their values.  With
 * sums[j - 1] = sum max(|x| - pivot_j, 0): returns 0 and bracket_out = {0, 0} if sum_abs <= a (t = 0),
 * else PCS_THRESH_PIVOTS and bracket_out = {pivot k - 1, pivot k}, k the first pivot with
 * sums - a - b pivot <= 0 (pivot 0 = lo, pivot 32 = hi).  sums == NULL: pivots only. */
int pcs_thresh_pick_host(int dtype, uint64_t lo, uint64_t hi, double sum_abs, const double* sums, double a,
                         double b, double* pivots_out, uint64_t* bracket_out);

/* ---------------------------------------------------------------- algebra / reductions */

/* out = a*x + b*y (y may be NULL -> out = a*x).  Numpy-order: (a*x) + (b*y). */
int pcs_axpby(int dtype, const void* x, const void* y, void* out, int64_t n, double a, double b,
              hipStream_t stream);
/* out = (x - a*y) - b*w  (the PDS primal argument, proxalgs.py:348). */
int pcs_sub2(int dtype, const void* x, const void* y, const void* w, void* out, int64_t n, double a, double b,
             hipStream_t stream);
/* out = d * x elementwise (DiagonalOperator with a vector diagonal, pycsou/linop/base.py:551-579). */
int pcs_mul(int dtype, const void* x, const void* d, void* out, int64_t n, hipStream_t stream);
/* The two sums of one relative improvement ||old - new|| / ||old|| (proxalgs.py:370-383) in one
 * pass, fixed order: out_dev[0] = sum (old - new)^2, out_dev[1] = sum old^2 (the layout
 * pcs_pds_finalize reads).  ws >= pcs_reduce_ws_bytes(), 8-byte aligned, contents on entry: arbitrary. */
int pcs_rel_sums(int dtype, const void* old, const void* nw, int64_t n, double* out_dev, void* ws,
                 hipStream_t stream);
/* Deterministic fp64 reductions into out_dev[0]: kind 0 = sum x^2, 1 = sum |x|,
 * 2 = sum (x-y)^2, 3 = sum x*y.  ws >= pcs_reduce_ws_bytes(), 8-byte aligned, contents on entry: arbitrary.
 * pcs_reduce_ws_bytes() serves every entry point that names it: 2 doubles for each of at most 1024 workgroups;
 * pcs_apgd_step and pcs_mcmc_accumulate reach its last double once n > 256 * 1023. */
int64_t pcs_reduce_ws_bytes(void);
int pcs_reduce(int dtype, int kind, const void* x, const void* y, int64_t n, double* out_dev, void* ws,
               hipStream_t stream);

/* One fused AcceleratedProximalGradientDescent.update_iterand + update_diagnostics
 * (pycsou/opt/proxalgs.py:586-601 and 612-622), given g = grad F(x):
 *   x_t = G.prox(x - tau g, tau)   gkind PCS_G_NULL / PCS_G_NONNEG / PCS_G_SEGMENT [seg_a, seg_b] /
 *                                  PCS_APGD_G_L1 (lam * L1Norm: soft threshold tau*lam)
 *   x'  = x_t + a (x_t - aux)      aux = the previous x_t ('past_aux'), a = (t_old - 1) / t
 * writes x' -> xn, x_t -> aux_n (no aliasing) and sums_dev[0..1] = ||x - x'||^2, ||x||^2 (fp64,
 * fixed order).  ws >= pcs_reduce_ws_bytes(), 8-byte aligned, contents on entry: arbitrary. */
enum { PCS_APGD_G_L1 = 3 };
int pcs_apgd_step(int dtype, const void* x, const void* g, const void* aux, void* xn, void* aux_n, int64_t n,
                  double tau, double a, int gkind, double lam, double seg_a, double seg_b, double* sums_dev,
                  void* ws, hipStream_t stream);

/* ---------------------------------------------------------------- PMYULA sampler, P2 streaming quantiles */

/* State of K <= PCS_P2_MAX_K P-square estimators (pycsou/util/stats.py) over n pixels, structure of arrays:
 *   heights[K][5][n]  marker heights in `dtype`, ascending over the middle index
 *   pos[K][3][n]      int32 positions of markers 1..3 (marker 0 is at 1, marker 4 at `count`)
 * `count` is the number of samples including the one being added (1 <= count < 2^31).  Samples 1..5 are the
 * warm-up (sorted insertion; sample 5 sets the positions to 1..5); from the sixth on `desired` (host, 5
 * doubles per p-value: the desired marker positions after this sample's increment, accumulated by repeated
 * addition as P2Algorithm.add_sample does) is passed to the kernel by value.  The update follows
 * stats.py:97-132 operation for operation, uncontracted, so fp64 states equal the reference's bit for bit.
 * Any n; 16-B accesses when n is a multiple of 16 / sizeof(dtype) and the arrays are 16-B aligned.
 * PCS_EINVAL: null pointer, n < 0, K outside 1..PCS_P2_MAX_K (0 allowed for pcs_mcmc_accumulate), bad dtype. */
#define PCS_P2_MAX_K 8
int pcs_p2_update(int dtype, const void* x, void* heights, int32_t* pos, int64_t n, int K, int64_t count,
                  const double* desired, hipStream_t stream);
/* Host-only twin of pcs_p2_update (the same __host__ __device__ element update) on host arrays. */
int pcs_p2_update_host(int dtype, const void* x, void* heights, int32_t* pos, int64_t n, int K, int64_t count,
                       const double* desired);
/* One retained sample of PMYULA (pycsou/opt/mcmc.py:125-129 and 197-208), reading x once:
 *   sums_dev[0] = sum x^2, sums_dev[1] = sum S_old^2   (fp64, fixed order, no atomics: the reference's
 *                 diagnostic ||old_sum - new_sum|| / ||old_sum||, the difference being x)
 *   sum += x ; sumsq += x * x ; the K P2 states take x (K = 0: no quantiles, heights / pos / desired unused).
 * ws >= pcs_reduce_ws_bytes(), 8-byte aligned, contents on entry: arbitrary.  x, sum and sumsq are distinct
 * arrays. */
int pcs_mcmc_accumulate(int dtype, const void* x, void* sum, void* sumsq, void* heights, int32_t* pos, int64_t n,
                        int K, int64_t count, const double* desired, double* sums_dev, void* ws, hipStream_t stream);

/* One Langevin step (mcmc.py:112-118) with g = grad F(x), summed left to right:
 *   PCS_MYULA_P_NONE  xn = (x - gamma g) + sqrt(2 gamma) z                                  (G null, mcmc.py:114)
 *   otherwise         xn = (((1 - gamma/tau) x - gamma g) + (gamma/tau) p) + sqrt(2 gamma) z
 *     PCS_MYULA_P_BUF   p read from the buffer `p` (= G.prox(x, tau) computed by the caller)
 *     PCS_MYULA_P_KIND  p = G.prox(x, tau) in the kernel, gkind as in pcs_apgd_step (PCS_G_NULL: p = x)
 * z: a buffer of n normals, or NULL for in-kernel noise: Philox4x32-10 with key (seed low, seed high) and
 * counter (element / 4, iter, stream_id, 0), Box-Muller in fp32 on 24-bit uniforms (the mapping is stated in
 * csrc/mcmc_core.hpp and is part of this contract); the value of an element depends on seed, iter, stream_id
 * and its index alone.  xn aliases no input. */
enum { PCS_MYULA_P_NONE = 0, PCS_MYULA_P_BUF = 1, PCS_MYULA_P_KIND = 2 };
int pcs_myula_step(int dtype, const void* x, const void* g, const void* p, const void* z, void* xn, int64_t n,
                   double tau, double gamma, int pmode, int gkind, double lam, double seg_a, double seg_b,
                   uint64_t seed, uint32_t iter, uint32_t stream_id, hipStream_t stream);
/* out[0..n) = the normals pcs_myula_step generates for (seed, iter, stream_id), in `dtype`. */
int pcs_mcmc_normal(int dtype, void* out, int64_t n, uint64_t seed, uint32_t iter, uint32_t stream_id,
                    hipStream_t stream);
/* out[4 b .. 4 b + 3] = the raw Philox words of block b < nblocks for (seed, iter, stream_id). */
int pcs_mcmc_philox(uint32_t* out, int64_t nblocks, uint64_t seed, uint32_t iter, uint32_t stream_id,
                    hipStream_t stream);
/* Host-only twins (no GPU): one Philox4x32-10 block, and the fp32 normals of pcs_mcmc_normal. */
int pcs_mcmc_philox_host(const uint32_t* ctr, const uint32_t* key, uint32_t* out);
int pcs_mcmc_normal_host(uint64_t seed, uint32_t iter, uint32_t stream_id, int64_t n, float* out);

/* ---------------------------------------------------------------- fused PDS iteration */

/* One fused PrimalDualSplitting.update_iterand + update_diagnostics
 * (pycsou/opt/proxalgs.py:343-394) for 2-D images, K = Gradient(kind='forward'):
 *   g   = grad F(x)           (F kind: 0, x - y, Conv^T(Conv x - y) separable, or read from gbuf)
 *   x_t = prox_G((x - tau g) - tau K^T z)
 *   u   = 2 x_t - x
 *   z_t = H.fenchel_prox(z + sigma K u, sigma)      (H = lam*L1 or lam*L21 pixel groups)
 *   z'  = rho z_t + (1-rho) z ;  x' = rho x_t + (1-rho) x
 * plus per-block partials of ||x-x'||^2, ||x||^2, ||z-z'||^2, ||z||^2.
 * Slab form: the local arrays hold rows [row0 - halo, row0 + rows + halo) of a
 * global n0 x n1 image (halo rows of x >= pcs_pds2d_halo_x(half), of each z component >= 1,
 * of y >= (pcs_pds2d_halo_x(half) - 1)/2 + 1); only the slab's own rows of xn/zn are written. */
typedef struct {
  int dtype;          /* PCS_F32 / PCS_F64 */
  int fkind;          /* PCS_F_* */
  int hkind;          /* PCS_H_* */
  int gkind;          /* PCS_G_* */
  int64_t n0, n1;     /* global image */
  int64_t row0, rows; /* this slab: global rows [row0, row0+rows) */
  int halo_x, halo_z, halo_y; /* halo rows stored above/below the slab in x/xn, z/zn, y/gbuf */
  int half;           /* separable conv half width H (taps 2H+1, centred) */
  const void* taps0;  /* 2H+1 taps along axis 0 (rows), device */
  const void* taps1;  /* 2H+1 taps along axis 1 (cols), device */
  double tau, sigma, rho, lam, step0, step1, seg_a, seg_b;
  const void* x; void* xn; const void* z; void* zn; const void* y; const void* gbuf;
  double* partials;       /* [nblocks][4] (pcs_pds2d_nblocks; for pcs_pds2d_run pcs_pds2d_run_nblocks); 16-byte
                             aligned with hist or sums_out; contents on entry: arbitrary */
  void* ctrl;             /* device control block (pcs_ctrl_*): pcs_ctrl_bytes() bytes, contents arbitrary
                             before pcs_ctrl_init / pcs_ctrl_init2 ; NULL = always run */
  double* hist;           /* non-NULL: reduce the partials and run pcs_pds_finalize inside the
                             step launch (single GPU); NULL: only write `partials`.  Ctrl.hist_len doubles
                             (8-byte aligned); contents on entry: arbitrary -- rows [0, Ctrl.it) are written,
                             the rest is never read or written */
  void* ws;               /* with hist or sums_out: pcs_pds2d_ws_bytes() bytes, 16-byte aligned, zeroed once
                             before first use: every counter is reset by its last arriver, so a loop that
                             stopped, naturally or not, leaves it ready for the next one */
  double* sums_out;       /* hist NULL, sums_out non-NULL (slab mode): the last workgroups reduce the
                             partials, then add pre_partials, into sums_out[4] (no loop control) */
  const double* pre_partials; /* [n_pre][4] partials of an earlier launch of the same iteration */
  int64_t n_pre;
  /* optional, fkind PCS_F_SEPCONV (fp32, half <= 7): grad F = N x - cty with N = Conv^T Conv
   * applied as two (4 tier + 1)-tap passes (the normal-operator row-marching kernel).  cty: Conv^T y
   * in y's layout (halo_y rows); ntaps: pcs_pds2d_ntaps_len(half) fp32 values, the window taps of
   * N along axis 0 and axis 1 and their exact rows on the tier rows / columns nearest each image
   * edge (layout in pds_nmarch.hpp; pycsou_amd.opt.engine.nmarch_taps builds it).  NULL: grad F
   * = Conv^T (Conv x - y) as four (2 tier + 1)-tap passes. */
  const void* cty;
  const void* ntaps;
  /* K (appended in ABI 2; all zero = the forward Gradient of the fields above).  kkind
   * PCS_K_GRAD_{FORWARD,BACKWARD,CENTERED}: K = Gradient(kind, edge, step0/1), z = [D0 x; D1 x];
   * PCS_K_LAPLACIAN: K = w0 D2_0 + w1 D2_1 (Laplacian(weights, step, edge), z has rows*n1
   * elements, H = lam*L1).  Non-forward K: the general-stencil row-marching kernel (fp32, F = NULL /
   * DENOISE / GRADBUF / SEPCONV with cty (grad F = N x - cty, N x into gbuf first) / CONV2D,
   * n1 % 4 == 0, 16-B aligned, at least two 64-column strips; slabs need halo rows x >= 2,
   * y >= 2, z >= 4); PCS_EUNSUPPORTED otherwise (pcs_pds2d_stencil_step covers the rest). */
  int kkind, edge;
  double w0, w1;
  /* fkind PCS_F_CONV2D (ABI 3): a general (non-separable) Convolve2D in F, grad F = Conv^T (Conv x - y)
   * by two pcs_conv2d_planned passes (conv_fwd / conv_adj: packed windows of tier conv_tier) over
   * the stored rows of x clipped to the image, into rbuf (the residual) and gbuf, inside this call
   * before the step (any K).  y, rbuf and gbuf share x's layout (halo_y == halo_x); a slab needs
   * halo_x >= conv_tier + 1 so that the rows the step reads are exact.  With fkind PCS_F_SEPCONV,
   * cty and a non-forward K, N x goes to gbuf the same way (halo_y == halo_x, halo_x >= 2 + 2 tier).
   * Neither runs banded (pcs_pds2d_step_bands: PCS_EUNSUPPORTED). */
  const void* conv_fwd;
  const void* conv_adj;
  int conv_tier, pad3;
  void* rbuf;
  /* ABI 6: a masked data-fidelity block (mkind PCS_M_L1LOSS), the reference notebook's TV-LAD
   * inpainting solved by ChambollePockSplitting (pycsou/opt/proxalgs.py:628-716):
   *   K = LinOpVStack(Masking(mask), K_s)  (linop/base.py:259-279, linop/sampling.py:125-196),
   *   H = ProxFuncHStack(L1Loss(dim=m, data=y), lam * L1Norm | lam * L21Norm on K_s x)
   *       (func/base.py:21-89, func/loss.py:222-268), K_s the kkind stencil above, F = 0 (fkind
   *       PCS_F_NULL), whole images only (rows == n0), the general-stencil row march (n1 % 4 == 0,
   *       at least two 64-column strips).
   * The masked dual block z_m is held EXPANDED to the image: zm / zmn are n0*n1 arrays (0 where the
   * mask is False, the sampled entries in image order elsewhere); ym is y expanded the same way
   * with NaN where the mask is False.  z / zn hold the K_s block only.  pcs_pds2d_run swaps zm / zmn
   * with x / xn.  The partials' z sums cover both blocks (= the reference's ||z|| over [z_m; z_s]). */
  int mkind, pad4;
  const void* ym;
  const void* zm;
  void* zmn;
  /* ABI 8: deferred finalization (with hist; NULL = finalize inside the launch).  The launch stores
   * its partials into `partials` without reducing them and finalizes the PREVIOUS launch's partials,
   * `fin_partials` (the other of two [nblocks][4] arrays, swapped with the iterate parity -- as
   * pcs_pds2d_run does), in a workgroup of its own while its tasks run: the reduction leaves the
   * critical path of every launch.  The stopping rule then acts one launch later (the extra iterate
   * goes to the buffer the engine does not select: the iterate after Ctrl.it iterations), and the
   * last launch's partials are finalized by pcs_pds_finalize_pending at the end of a run.  Sized and
   * aligned as `partials`; contents on entry: arbitrary (Ctrl.pend says whether they are meaningful). */
  const double* fin_partials;
} pcs_pds2d_args;
enum { PCS_M_NONE = 0, PCS_M_L1LOSS = 1 };
/* 1 if pcs_pds2d_step runs these arguments (0: PCS_EUNSUPPORTED / invalid). */
int pcs_pds2d_supported(const pcs_pds2d_args* a);
/* Which kernel family pcs_pds2d_step runs for these arguments (-1: none), so an engine can tell the fused
 * normal-operator marches (one launch per iteration) from the split forms: */
enum {
  PCS_PATH_TILE = 1,      /* the tile kernel (pds_tile.hpp)                                         */
  PCS_PATH_MARCH = 2,     /* fp32 separable PSF, four-pass row march (pds_march.hpp)                */
  PCS_PATH_NMARCH = 3,    /* fp32 separable PSF, normal-operator march (pds_nmarch.hpp)             */
  PCS_PATH_PT = 4,        /* fp32 pointwise grad F, forward K (pds_pt.hpp)                          */
  PCS_PATH_SMARCH = 5,    /* general-stencil march, pointwise grad F (pds_smarch.hpp)               */
  PCS_PATH_SMARCH_NX = 6, /* N x pass into gbuf, then the general-stencil march (two launches)      */
  PCS_PATH_NM64 = 7,      /* fp64 separable PSF, fused normal-operator march (pds_nm64.hip)         */
  PCS_PATH_CONV2D = 8     /* two correlation passes, then the step with grad F from gbuf            */
};
int pcs_pds2d_path(const pcs_pds2d_args* a);
int pcs_pds2d_ntaps_len(int half); /* 64 + 32 * tier(half); -1 beyond tier 7 */

int pcs_pds2d_halo_x(int half);
int64_t pcs_pds2d_nblocks(const pcs_pds2d_args* a);
int64_t pcs_pds2d_ws_bytes(const pcs_pds2d_args* a);
/* One iteration (x, z -> xn, zn).  With fin_partials the launch finalizes the previous launch's
 * partials, not its own: see pcs_pds2d_run for the stop semantics and pcs_pds_finalize_pending. */
int pcs_pds2d_step(const pcs_pds2d_args* a, hipStream_t stream);
/* pcs_pds2d_step restricted to the slab's own rows [ra0, rb0) u [ra1, rb1)
 * (0 <= ra0 <= rb0 <= ra1 <= rb1 <= rows): writes x', z' on those rows and one partials row per
 * block (pcs_pds2d_nblocks_bands of them); hist must be NULL.  Same arithmetic per pixel as the
 * whole-slab step, so any split of the rows into launches gives bitwise the same x', z'.  The
 * multi-GPU loop runs the boundary bands and the interior band as separate launches so that the
 * halo exchange overlaps the interior.  Row-marching kernels only (fp32, L1/L21; F separable
 * conv of half width <= 7, or pointwise): PCS_EUNSUPPORTED otherwise. */
int64_t pcs_pds2d_nblocks_bands(const pcs_pds2d_args* a, int64_t ra0, int64_t rb0, int64_t ra1, int64_t rb1);
int pcs_pds2d_step_bands(const pcs_pds2d_args* a, int64_t ra0, int64_t rb0, int64_t ra1, int64_t rb1,
                         hipStream_t stream);
/* n iterations of pcs_pds2d_step launched back to back, ping-ponging (x, z) <-> (xn, zn) (and
 * partials <-> fin_partials); requires hist/ctrl/ws (in-kernel loop control).  The host-side form of
 * GenericIterativeAlgorithm.iterate's loop (pycsou/core/solver.py:55-76).
 * Without fin_partials an even n leaves the iterate in (x, z).  With fin_partials (deferred
 * finalization) the stopping rule acts one launch late: after a natural stop at iteration j the
 * next launch has already written iterate j + 1 into the other buffer pair, and the stop flag is
 * written mid-launch by that launch's finalizer workgroup.  The caller must then (1) call
 * pcs_pds_finalize_pending once the run is done, before reading ctrl or hist, and (2) select the
 * result by the parity of Ctrl.it (iterations done: even -> x, z; odd -> xn, zn), not by n. */
int pcs_pds2d_run(const pcs_pds2d_args* a, int64_t n, hipStream_t stream);
/* The band-paired schedule of pcs_pds2d_run (deferred finalization only).  A whole image whose seven
 * step arrays exceed the Infinity Cache runs every iteration as two row-band launches T = [0, m) and
 * B = [m, rows), T first in even iterations and B first in odd ones, so that every second band launch
 * rereads the previous iteration's output of its own band on-die.  x, z and the iteration count are
 * those of the single launch bit for bit; the partials of an iteration are T's tasks then B's, reduced
 * in that order by the first band launch of the next iteration, so the diagnostics are reproducible and
 * differ from the single launch's only in the fp64 summation order.  Off unless PCS_RUN_BANDS asks for
 * it (on the C3 step it measured slower than the single launch): 1 pairs any problem that
 * pcs_pds2d_step_bands takes, auto pairs where the size rule of csrc/pds.hip says so, 0 or unset keeps
 * the single launch.  `mode`: -1 = as pcs_pds2d_run will decide, 0 / 1 / 2 = as if PCS_RUN_BANDS were
 * 0 / 1 / auto.
 * pcs_pds2d_run_nblocks: partials rows per iteration (size both partials arrays, and call
 * pcs_pds_finalize_pending, with it).  pcs_pds2d_run_plan: out[6] = {paired, m, tasks of T, tasks of B,
 * rows lo, hi of the first launch of iteration i}; nothing is launched. */
int64_t pcs_pds2d_run_nblocks(const pcs_pds2d_args* a, int mode);
int pcs_pds2d_run_plan(const pcs_pds2d_args* a, int mode, int64_t i, int64_t* out);

/* ---------------------------------------------------------------- fused APGD iteration */

/* One fused AcceleratedProximalGradientDescent.update_iterand + update_diagnostics + loop test
 * (pycsou/opt/proxalgs.py:586-622, pycsou/core/solver.py:65-66) in ONE launch, for a whole 2-D image and
 * F = (1/2) ||Conv x - y||^2 with a separable Conv of half width <= 7:
 *   g    = N x - cty              N = Conv^T Conv as two 29-tap passes (exact zero-boundary edge rows)
 *   x_t  = G.prox(x - tau g, tau) gkind PCS_G_NULL / PCS_G_NONNEG / PCS_G_SEGMENT [seg_a, seg_b] /
 *                                 PCS_APGD_G_L1 (lam * L1Norm: soft threshold tau*lam)
 *   x'   = x_t + a (x_t - aux)    aux = the previous x_t ('past_aux'), a = (t_old - 1) / t
 * writes x' -> xn, x_t -> aux_n, reduces ||x - x'||^2 and ||x||^2 inside the launch and runs the loop
 * control of pcs_pds_finalize on them (the dual pair of `hist` reads inf; init the control block with
 * has_dual = 0).  A launch that finds the stop flag set stores nothing.  Per element the arithmetic is
 * pcs_apgd_step's; only grad F is formed differently (N x - Conv^T y instead of Conv^T (Conv x - y)).
 * Takes n0, n1 >= 16, n1 % 4 == 0, half <= 7, n0 * n1 * sizeof(T) < 2^30, every array n0 * n1 elements
 * and 16-B aligned, x / aux / cty distinct from xn / aux_n (a workgroup reads rows of x that its
 * neighbours write in xn): pcs_apgd2d_supported is 0 and the calls return PCS_EUNSUPPORTED otherwise. */
typedef struct {
  int dtype;          /* PCS_F32 / PCS_F64 */
  int gkind;          /* PCS_G_* / PCS_APGD_G_L1 */
  int64_t n0, n1;     /* image */
  int half;           /* separable conv half width H (taps 2H+1, centred) */
  int pad;
  const void* taps0;  /* 2H+1 taps along axis 0 (rows), device */
  const void* taps1;  /* 2H+1 taps along axis 1 (cols), device */
  double tau, lam, seg_a, seg_b;
  const void* x; void* xn; const void* aux; void* aux_n;
  const void* cty;    /* Conv^T y, formed once by the caller */
  double* partials;   /* [pcs_apgd2d_nblocks()][4], 16-byte aligned; contents on entry: arbitrary */
  void* ctrl;         /* device control block (pcs_ctrl_init2, has_dual 0) */
  double* hist;       /* 2 doubles per iteration: the relative improvement, inf; Ctrl.hist_len doubles,
                         contents on entry: arbitrary */
  void* ws;           /* pcs_apgd2d_ws_bytes() bytes, 16-byte aligned, zeroed once before first use (counters
                         reset by their last arriver, as pcs_pds2d_args.ws) */
} pcs_apgd2d_args;
int pcs_apgd2d_supported(const pcs_apgd2d_args* a);
int64_t pcs_apgd2d_nblocks(const pcs_apgd2d_args* a);
int64_t pcs_apgd2d_ws_bytes(const pcs_apgd2d_args* a);
/* One iteration (x, aux -> xn, aux_n) with momentum coefficient a. */
int pcs_apgd2d_step(const pcs_apgd2d_args* a, double a_coef, hipStream_t stream);
/* n iterations launched back to back, ping-ponging (x, aux) <-> (xn, aux_n); launch i uses a_host[i]
 * (host memory, read before the call returns).  The coefficients depend on the iteration index alone, so
 * the host always knows them, and once the loop has stopped every later launch is a no-op: the iterate
 * after Ctrl.it iterations is in (x, aux) when Ctrl.it - (Ctrl.it at the call) is even, else in (xn, aux_n). */
int pcs_apgd2d_run(const pcs_apgd2d_args* a, const double* a_host, int64_t n, hipStream_t stream);

/* One fused PrimalDualSplitting.update_iterand + update_diagnostics (pycsou/opt/proxalgs.py:343-394)
 * for a 2-D image with a general finite-difference K (single GPU, whole image):
 *   kkind PCS_K_GRAD_{FORWARD,BACKWARD,CENTERED}: K = Gradient(kind, edge, step)  (diff.py:777-882),
 *         z = [D0 x; D1 x] (2 N), H = lam*L1 or lam*L21 over the two components;
 *   kkind PCS_K_LAPLACIAN: K = w0 D2_0 + w1 D2_1 (Laplacian(weights, step, edge), diff.py:885-957),
 *         z has N elements, H = lam*L1.
 *   fkind PCS_F_NULL: grad F = 0; PCS_F_DENOISE: grad F = x - g (g holds y); PCS_F_GRADBUF: g.
 * Same update and partials as pcs_pds2d_step (x_t = prox_G((x - tau g) - tau K^T z), ...); the
 * stencils are the standalone operators' (pcs_grad_fwd/adj, pcs_lap_fwd/adj) per element.  With
 * hist/ctrl/ws the last workgroups reduce the partials and run the stopping rule (as
 * pcs_pds2d_step); else only `partials` ([nblocks][4]) is written. */
typedef struct {
  int dtype, kkind, fkind, hkind, gkind, edge;
  int64_t n0, n1;
  double tau, sigma, rho, lam, step0, step1, w0, w1, seg_a, seg_b;
  const void* x; void* xn; const void* z; void* zn; const void* g;
  double* partials; /* [pcs_pds2d_stencil_nblocks()][4], 16-byte aligned with hist; contents on entry: arbitrary */
  void* ctrl;       /* as pcs_pds2d_args.ctrl */
  double* hist;     /* as pcs_pds2d_args.hist */
  void* ws; /* pcs_pds2d_stencil_ws_bytes() bytes, 16-byte aligned, zeroed once before first use (as pcs_pds2d_args.ws) */
} pcs_pds2d_stencil_args;
int64_t pcs_pds2d_stencil_nblocks(const pcs_pds2d_stencil_args* a);
int64_t pcs_pds2d_stencil_ws_bytes(const pcs_pds2d_stencil_args* a);
int pcs_pds2d_stencil_step(const pcs_pds2d_stencil_args* a, hipStream_t stream);
/* n steps back to back, ping-ponging (x, z) <-> (xn, zn); requires hist/ctrl/ws. */
int pcs_pds2d_stencil_run(const pcs_pds2d_stencil_args* a, int64_t n, hipStream_t stream);

/* ---------------------------------------------------------------- multi-GPU row slabs
 * Native per-rank loop of the row-slab 2-D PDS (one process per GPU, RCCL over xGMI):
 * GenericIterativeAlgorithm.iterate (pycsou/core/solver.py:55-76) around
 * PrimalDualSplitting.update_iterand / update_diagnostics (pycsou/opt/proxalgs.py:343-394) for an
 * image split into contiguous row slabs.  Per iteration: the fused slab step, the four norm sums
 * all-gathered (4 doubles per rank, added in rank order, so every rank takes the same stop
 * decision) and the boundary rows of x', z' exchanged with the two neighbour ranks.
 * RCCL is bound at run time (dlopen librccl.so.1); pcs_comm_available() says whether it was. */
int pcs_comm_available(void);
int pcs_comm_id_bytes(void); /* size of the opaque unique id (ncclUniqueId) */
int pcs_comm_unique_id(void* id);                               /* rank 0; broadcast id to the others */
int pcs_comm_init(const void* id, int world, int rank, void** comm); /* collective over the ranks */
int pcs_comm_destroy(void* comm);

/* Halo buffers written by one parity of the ping-pong (up to 4 arrays, e.g. x', z0', z1'):
 * send_lo[k] (own first rows) goes to rank-1's recv_hi[k]; send_hi[k] (own last rows) to
 * rank+1's recv_lo[k]; bytes[k] bytes each.  Pointers toward a missing neighbour may be NULL. */
typedef struct {
  int nbuf;
  int pad;
  void* send_lo[4];
  void* recv_lo[4];
  void* send_hi[4];
  void* recv_hi[4];
  int64_t bytes[4];
} pcs_halo_set;

/* One grouped RCCL send/recv of the halo rows/planes with the two neighbour ranks on `stream`
 * (the exchange step of SURVEY 8(e)): send_lo -> rank-1's recv_hi, send_hi -> rank+1's recv_lo.
 * world == 1: no-op.  Graph-capturable (no allocation, no host synchronisation). */
int pcs_halo_exchange(void* comm, int rank, int world, const pcs_halo_set* h, hipStream_t stream);
/* dst[r * count .. (r + 1) * count) = src of rank r (RCCL all-gather over `comm` on `stream`; the
 * norm-sums step of SURVEY 8(e)); comm NULL (world 1 only): a device copy.  Graph-capturable. */
int pcs_allgather_f64(void* comm, int world, const double* src, double* dst, int64_t count, hipStream_t stream);

typedef struct {
  int world, rank;
  pcs_pds2d_args step[2]; /* parity p: x = X[p] -> xn = X[1-p] (hist/ws ignored, partials owned by the plan) */
  pcs_halo_set halo[2];   /* halo[p]: the buffers step[p] writes (X[1-p], Z[1-p]) */
  void* ctrl;             /* loop control block (pcs_ctrl_init2), identical on every rank */
  double* hist;
  int64_t band;           /* boundary band rows (>= the x halo depth) for the overlapped schedule */
  int overlap;            /* 1: boundary bands, then the halo exchange on a side stream while the
                             interior band runs (row-marching kernels only; else the serial schedule) */
  int pad2;
} pcs_slab2d_desc;

/* comm may be NULL when world == 1.  The plan owns its partials/sums buffers, a side stream and
 * events (allocated here, not in pcs_slab2d_run). */
int pcs_slab2d_create(const pcs_slab2d_desc* d, void* comm, void** plan);
int pcs_slab2d_overlapped(const void* plan);
/* n iterations starting at parity p0 (no host synchronisation; the stop flag in ctrl makes the
 * iterations after the reference loop's exit return at once). */
int pcs_slab2d_run(void* plan, int64_t n, int p0, hipStream_t stream);
int pcs_slab2d_destroy(void* plan);

/* Communication-avoiding form of the row-slab loop (ABI 9; the same iteration as pcs_slab2d_run,
 * GenericIterativeAlgorithm.iterate of pycsou/core/solver.py:55-76 across ranks): the halos of x, z, y
 * are stored `depth` iterations deep and exchanged once per chunk of `depth` iterations.  Iteration j of
 * a chunk computes the own rows plus (m - j) * reach redundant rows of each halo (clipped at the image),
 * so the own rows after the chunk are bitwise the single-GPU iterate; the m x 4 norm sums of a chunk are
 * all-gathered once and pcs_pds_reduce_finalize_k runs the loop control over them in iteration order.
 * Buffers rotate through nbuf sets (step[b]: X[b] -> X[(b + 1) % nbuf]); after n iterations from set 0
 * the iterate is set n % nbuf, and after a natural stop set (Ctrl.it % nbuf).  Needs the banded
 * (row-marching) step: PCS_EUNSUPPORTED at create otherwise. */
#define PCS_DEEP_MAX 8
typedef struct {
  int world, rank;
  int depth;              /* 1 <= depth <= PCS_DEEP_MAX: iterations per exchange */
  int nbuf;               /* buffer sets in the rotation, >= max(2, depth) */
  int reach;              /* even, >= the rows one iteration reads past its own (x and z) */
  int local;              /* 1: no communicator -- the plan runs only under pcs_slab2d_deep_run_local */
  pcs_pds2d_args step[PCS_DEEP_MAX]; /* plain slabs with the deep halos (>= (depth - 1) reach + 1 rows) */
  pcs_halo_set halo[PCS_DEEP_MAX];   /* the deep halos of X[b], Z[b] */
  void* ctrl;
  double* hist;
} pcs_slab2d_deep_desc;
int pcs_slab2d_deep_create(const pcs_slab2d_deep_desc* d, void* comm, void** plan);
/* n iterations from buffer set b0: chunks of depth (the last one shorter), each followed by the
 * all-gather, the loop control and the deep-halo exchange. */
int pcs_slab2d_deep_run(void* plan, int64_t n, int b0, hipStream_t stream);
/* The same chunks for all `nplans` ranks of one image in ONE process (plans[i] of ranks 0..nplans-1,
 * one stream): the all-gather and the halo exchange as device copies -- the parity tests' transport. */
int pcs_slab2d_deep_run_local(void* const* plans, int nplans, int64_t n, int b0, hipStream_t stream);
int pcs_slab2d_deep_destroy(void* plan);
/* Loop control over k iterations' sums gathered as [world][k][4] (rank r's k rows of 4 sums, each summed
 * across ranks in the order pcs_pds_reduce_finalize uses), in iteration order. */
int pcs_pds_reduce_finalize_k(const double* gathered, int world, int k, void* ctrl_dev, double* hist,
                              hipStream_t stream);

/* One fused PrimalDualSplitting.update_iterand + update_diagnostics for 3-D volumes
 * (pycsou/opt/proxalgs.py:343-394), K = Gradient(kind='forward') in 3-D
 * (pycsou/linop/diff.py:777-882): the same update as pcs_pds2d_step with three gradient
 * components (z = [D0 x; D1 x; D2 x]) and grad F taken from `g`:
 *   fkind PCS_F_NULL: 0;  PCS_F_DENOISE: x - g (g holds y);  PCS_F_GRADBUF: g.
 * Volume n0 x n1 x n2 (C order, n2 % 4 == 0); slab form as in 2-D along axis 0: the local
 * arrays hold planes [plane0 - halo, plane0 + planes + halo); `g` must supply planes
 * [0, planes] (one past the slab) when planes < n0 -- [-1, planes] for the backward / centred
 * kinds (kkind), which also need halo_z >= 2 (K^T z at plane p reads z0 of p - 1 .. p + 1). */
typedef struct {
  int dtype, fkind, hkind, gkind;
  int64_t n0, n1, n2;
  int64_t plane0, planes;
  int halo_x, halo_z, halo_g;
  int pad;
  double tau, sigma, rho, lam, step0, step1, step2, seg_a, seg_b;
  const void* x; void* xn; const void* z; void* zn; const void* g;
  double* partials;       /* [nblocks][4] (pcs_pds3d_nblocks / pcs_pds3d_nblocks_bands), 16-byte aligned with hist;
                             contents on entry: arbitrary */
  void* ctrl;             /* device control block; NULL = always run */
  double* hist;           /* non-NULL: in-launch reduce + loop control (single GPU); as pcs_pds2d_args.hist */
  void* ws;               /* with hist: pcs_pds3d_ws_bytes() bytes, 16-byte aligned, zeroed once before first use
                             (as pcs_pds2d_args.ws) */
  int kkind;              /* PCS_FORWARD (0), PCS_BACKWARD or PCS_CENTERED: Gradient(kind) */
  int edge;               /* Gradient(edge=...): the centred kind's one-sided end samples */
  /* fkind PCS_F_CONV0 (ABI 5; fp32, forward K): the axis-0 Convolve1D of a separable 3-D PSF inside
   * the step, grad F = C0^T (C0 g - conv0_w) along axis 0 with `g` holding the in-plane normal
   * operator C12^T C12 x and conv0_w = C12^T y (both with halo_g planes; halo_g >= conv0_k when
   * planes < n0); conv0_taps: conv0_k <= 15 device taps, conv0_off the Convolve1D offset.  Replaces
   * the pcs_conv0_residual_adjoint pass (pycsou/linop/conv.py:20-164 along axis 0). */
  const void* conv0_w;
  const void* conv0_taps;
  int conv0_k, conv0_off;
} pcs_pds3d_args;

int64_t pcs_pds3d_nblocks(const pcs_pds3d_args* a);
int64_t pcs_pds3d_ws_bytes(const pcs_pds3d_args* a);
int pcs_pds3d_step(const pcs_pds3d_args* a, hipStream_t stream);
/* pcs_pds3d_step restricted to the slab's own planes [a0, b0) u [a1, b1)
 * (0 <= a0 <= b0 <= a1 <= b1 <= planes): writes x', z' on those planes and one partials row per
 * block (pcs_pds3d_nblocks_bands of them); hist must be NULL.  Per-voxel arithmetic is that of
 * the whole-slab step (bitwise the same x', z' for any split).  The multi-GPU loop updates the
 * boundary bands first, starts their halo exchange, and updates the interior meanwhile. */
int64_t pcs_pds3d_nblocks_bands(const pcs_pds3d_args* a, int64_t a0, int64_t b0, int64_t a1, int64_t b1);
int pcs_pds3d_step_bands(const pcs_pds3d_args* a, int64_t a0, int64_t b0, int64_t a1, int64_t b1,
                         hipStream_t stream);

/* Device control block for the hipGraph-captured loop:
 * int32 [0]=it (next iteration), [1]=stopped, [2]=min_iter, [3]=max_iter, [4]=has_dual,
 * [5]=hist_len, [6]=pend (deferred finalization: the last launch's partials wait); double at byte 32:
 * accuracy_threshold.  pcs_ctrl_bytes() bytes, 8-byte aligned; contents on entry to pcs_ctrl_init /
 * pcs_ctrl_init2: arbitrary (every field is written).
 * hist: double[2*(max(min_iter,max_iter)+1)+2] = (primal, dual) relative improvement per iteration; the loop
 * stops before a row would pass hist_len, the two doubles after the last row are never written. */
int64_t pcs_ctrl_bytes(void);
int pcs_ctrl_init(void* ctrl_dev, int min_iter, int max_iter, double thr, int has_dual, hipStream_t stream);
/* Reduce [nparts][4] partials (fixed order, fp64) into sums[4]. */
int pcs_reduce_partials(const double* partials, int64_t nparts, double* sums, hipStream_t stream);
/* From sums[4] (global), write hist[it], advance it, set stopped per
 * GenericIterativeAlgorithm.iterate's loop condition (pycsou/core/solver.py:65-66). */
int pcs_pds_finalize(const double* sums, void* ctrl_dev, double* hist, hipStream_t stream);
/* Single-GPU shortcut: pcs_reduce_partials + pcs_pds_finalize in one launch. */
int pcs_pds_reduce_finalize(const double* partials, int64_t nparts, void* ctrl_dev, double* hist,
                            hipStream_t stream);
/* End of a deferred-finalization run (pcs_pds2d_args.fin_partials): finalize the last launch's
 * [nparts][4] partials if they are pending and the loop has not stopped (a no-op otherwise), in the
 * summation order of the in-launch finalizer. */
int pcs_pds_finalize_pending(const double* partials, int64_t nparts, void* ctrl_dev, double* hist,
                             hipStream_t stream);
/* pcs_ctrl_init with an explicit history length (doubles in `hist`). */
int pcs_ctrl_init2(void* ctrl_dev, int min_iter, int max_iter, double thr, int has_dual, int hist_len,
                   hipStream_t stream);

/* ---------------------------------------------------------------- pseudo-inverse: batched conjugate gradients */

/* The solver between two operator applications of LinearOperator.pinv / LinOpPinv (pycsou/core/linop.py:397-420,
 * 618-629 -> pylops NormalEquationsInversion(Op, None, y, epsI=eps) -> scipy.sparse.linalg.cg on
 * (A^T A + eps^2 I) x = A^T y; SciPy 1.15: x0 = 0 unless given, stop when ||r|| < max(atol, rtol ||b||),
 * rtol = 1e-5, maxiter = 10 n).  PyLops only forwards; the contract restated here is SciPy's cg.
 *
 * nb >= 1 independent systems; system j is row j of contiguous (nb, n) arrays x, r, p, q, b.  One iteration:
 *   pcs_cg_dir     p_j = beta_j p_j + r_j              (p_j = r_j while the control block's it == 0)
 *   caller         q = A^T (A p)                       (rows of p -> rows of q)
 *   pcs_cg_dot     pq_j = sum p (q + eps2 p),  alpha_j = rho_j / pq_j
 *   pcs_cg_update  x_j += alpha_j p_j,  r_j -= alpha_j (q_j + eps2 p_j),  rho' = sum r_j r_j,
 *                  beta_j = rho' / rho_j,  rho_j = rho',  active_j &= !(sqrt(rho') < tol_j),  it += 1,
 *                  stopped when no system is active or it == max_iter (or the history is full),
 *                  hist[2 it], hist[2 it + 1] = max_j ||r_j|| / ||b_j|| (0 where b_j = 0), active systems
 * SciPy's recurrences operation for operation (no contraction into fma), so an fp64 run differs from SciPy by
 * the summation order alone.  Vectors in `dtype`; sums and scalars in fp64, scalars rounded to `dtype` where
 * they multiply a vector; eps2 = eps^2 is applied on the fly, q is never rewritten.  Traffic per system and
 * iteration: dir 2n + n, dot 2n, update 4n + 2n words.
 * An inactive system is not written at all (x, r, p keep their bits); once the control block's `stopped` is
 * set every launch returns without writing, so replays of a captured chunk past the stop change nothing.
 * Breakdown: pq_j not > 0 or not finite sets breakdown_j = 1 and active_j = 0 (SciPy goes on and returns
 * inf / NaN there).
 * Sums: per-workgroup partials, then a finalising launch adds a system's partials in a fixed order; no
 * atomics, the bits depend on n and on the access path alone (16-byte loads and stores when n sizeof(dtype) is
 * a multiple of 16 and every base is 16-byte aligned, element-wise otherwise), not on nb or the run.
 * Grid: blockIdx.y = system, min(ceil(n / 256), PCS_CG_MAX_BLOCKS) workgroups per system, grid-stride over n.
 *
 * state:    pcs_cg_state_bytes(nb) bytes, 8-byte aligned: per system 8 doubles rho, pq, alpha, beta, tol, ||b||,
 *           active, breakdown.  Contents on entry to pcs_cg_init: arbitrary (it writes every field); the other
 *           entries read what pcs_cg_init and they have written.
 * partials: pcs_cg_nblocks(n, nb) doubles ([nb][workgroups per system]), 8-byte aligned; contents on entry:
 *           arbitrary (a finalising launch reads only what the launch before it has written).
 * ctrl:     the control block above (pcs_ctrl_bytes()); pcs_cg_init writes every field (it = 0, min_iter = 0,
 *           max_iter, hist_len, stopped when no system is active or max_iter == 0).
 * hist:     hist_len doubles, rows of 2; never written past hist_len (pcs_cg_init does not write it).
 * pcs_cg_init: on entry r holds the initial residual (b, or b - (A^T A + eps^2 I) x0); writes ||b_j||,
 *           tol_j = max(atol, rtol ||b_j||), rho_j = r_j . r_j, active_j = ||b_j|| > 0 and not ||r_j|| < tol_j.
 * PCS_EINVAL before any device call: null pointer, n < 0, nb < 1, unknown dtype, max_iter < 0, hist_len < 2,
 * negative or non-finite rtol / atol / eps2, overlap among x, r, p, q.  PCS_EUNSUPPORTED: nb > 65535 (split the
 * batch).  pcs_cg_state_bytes / pcs_cg_nblocks return PCS_EINVAL for n < 0 or nb < 1. */
#define PCS_CG_MAX_BLOCKS 1024
int64_t pcs_cg_state_bytes(int64_t nb);
int64_t pcs_cg_nblocks(int64_t n, int64_t nb);
int pcs_cg_init(int dtype, const void* b, const void* r, int64_t n, int64_t nb, double rtol, double atol, int max_iter,
                void* state, double* partials, void* ctrl, double* hist, int hist_len, hipStream_t stream);
int pcs_cg_dir(int dtype, const void* r, void* p, int64_t n, int64_t nb, const void* state, const void* ctrl,
               hipStream_t stream);
int pcs_cg_dot(int dtype, const void* p, const void* q, int64_t n, int64_t nb, double eps2, void* state,
               double* partials, const void* ctrl, hipStream_t stream);
int pcs_cg_update(int dtype, void* x, void* r, const void* p, const void* q, int64_t n, int64_t nb, double eps2,
                  void* state, double* partials, void* ctrl, double* hist, hipStream_t stream);

/* ---------------------------------------------------------------- eigenvalues: re-orthogonalised Lanczos steps */

/* The vector work of one step of the thick-restart Lanczos behind LinearOperator.eigenvals / singularvals
 * (pycsou/core/linop.py:208-219 -> scipy.sparse.linalg.eigsh / svds -> ARPACK) between two applications of the
 * operator.  Everything is fp64.  V: m + 1 rows of n elements, row stride ldv >= n elements; at step s (0 <= s < m)
 * rows 0..s are orthonormal and w (n contiguous elements, outside V) holds A V_s.  Classical Gram-Schmidt twice:
 *   pcs_orth_dots    h[i] = <V_i, w> for i <= s,  h[s+1] = <w, w>        (w is read once per group of
 *                    PCS_ORTH_GROUP rows)
 *   pcs_orth_update  w -= sum_{i<=s} h_in[i] V_i in place (rows in the order 0..s, one fma each), then, in the
 *                    same launch, h_out[i] = <V_i, w_new> for i <= s and h_out[s+1] = <w_new, w_new>.  Up to
 *                    PCS_ORTH_REG_ROWS rows (s < 24) a thread keeps its elements of every row in registers
 *                    between the two, so the basis is read once (instantiations of 8, 16 and 24 rows);
 *                    above, the rows are read a second time, in groups of PCS_ORTH_GROUP.
 *   one step         dots(h1), update(h1 -> h2), update(h2 -> h3); h3 is what is left after two passes
 *   pcs_orth_commit  H[i][s] = H[s][i] = h1[i] + h2[i] for i <= s;  beta[s] = sqrt(h3[s+1]);
 *                    omega[s] = max_{i<=s} |h3[i]| / beta[s];  row s + 1 of V = w / beta[s].
 *                    Breakdown: if beta_s <= brk sqrt(h1[s+1]) (an invariant subspace or w = 0; the caller passes
 *                    brk, 0 <= brk < inf) row s + 1 is written as zeros, beta[s] = omega[s] = 0 and `breakdown`
 *                    keeps the first such s.  The steps after it then see w = 0 and break down the same way:
 *                    no division by zero, every value finite, the first index kept.
 * V and w are only read by dots; update writes w alone; commit writes row s + 1 of V and the state alone.
 * Sums: per-workgroup partials, then a finalising launch adds a row's partials in a fixed order; no atomics, the
 * bits depend on n, s and the access path alone (16-byte loads when V and w are 16-byte aligned and ldv is even,
 * element-wise otherwise).  Grid: min(ceil(n / 512), PCS_ORTH_MAX_BLOCKS) workgroups of 256 threads over the
 * columns, grid-stride; for dots times the row groups.
 *
 * h, h_in, h_out, h1..h3: s + 2 doubles each (m + 1 serve every step); h_in != h_out.
 * partials: pcs_orth_nblocks(n, rows) doubles for rows >= s + 1 ([s + 2][workgroups]; pcs_orth_nblocks(n, m)
 *           serves every step), 8-byte aligned; contents on entry: arbitrary.
 * state:    pcs_orth_state_bytes(m) bytes = m m + 2 m + 1 doubles, 8-byte aligned: H (m x m, row-major), beta[m],
 *           omega[m], breakdown (the index of the first step that broke down, as a double; -1: none).  Contents on
 *           entry to pcs_orth_state_init: arbitrary (H, beta, omega = 0, breakdown = -1); pcs_orth_commit writes
 *           row and column s of H (entries i <= s), beta[s], omega[s] and the breakdown index.
 * PCS_EINVAL before any device call: null pointer, n < 0, s < 0, s >= m (commit), m < 1, ldv < n, w overlapping
 * rows 0..s+1 of V, h_in == h_out, brk negative or not finite.  PCS_EUNSUPPORTED: m > PCS_ORTH_MAX_M (for dots and
 * update: s >= PCS_ORTH_MAX_M).  The size functions return the same statuses (rows, m < 1: PCS_EINVAL). */
#define PCS_ORTH_MAX_M 256
#define PCS_ORTH_GROUP 8
#define PCS_ORTH_REG_ROWS 24
#define PCS_ORTH_MAX_BLOCKS 1024
int64_t pcs_orth_state_bytes(int64_t m);
int64_t pcs_orth_nblocks(int64_t n, int64_t rows);
int pcs_orth_state_init(void* state, int64_t m, hipStream_t stream);
int pcs_orth_dots(const double* V, int64_t ldv, int64_t s, const double* w, int64_t n, double* h, double* partials,
                  hipStream_t stream);
int pcs_orth_update(const double* V, int64_t ldv, int64_t s, double* w, int64_t n, const double* h_in, double* h_out,
                    double* partials, hipStream_t stream);
int pcs_orth_commit(double* V, int64_t ldv, int64_t s, int64_t m, const double* w, int64_t n, const double* h1,
                    const double* h2, const double* h3, double brk, void* state, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PYCSOU_HIP_H */
