/* maxent_hip.h -- C-ABI of libmaxent_hip.so (MI355X / gfx950)
 *
 * Drop-in boundary for the alpha-scan inner solver of TRIQS/maxent.
 * The reference (pure Python, /root/reference/python) has no FFI; the natural
 * hook for a batched device solver is the body of
 *     MaxEntLoop.run                      maxent_loop.py:144-302  (one alpha scan)
 *     ElementwiseMaxEnt.run_diagonal /
 *                       run_offdiagonal   elementwise_maxent.py:223-268 (all elements)
 * i.e. everything between "K.reduce_singular_space()" (maxent_loop.py:184) and
 * "result.add_result(...)" (maxent_loop.py:258-266).  The entry points below
 * replace exactly that span:
 *
 *   reference                                              | this library
 *   -------------------------------------------------------+---------------------------
 *   KernelSVD.U/.S/.V after reduce_singular_space          | mxe_ctx_create(U,S,V)
 *     kernels.py:53-122                                    |
 *   NormalChi2(K, G, err)            functions.py:336-377  | mxe_dataset_add (U,err) +
 *   TauMaxEnt.set_cov rotation       tau_maxent.py:253-325 |   mxe_elements_set (G, D, kind)
 *   NormalEntropy / PlusMinusEntropy functions.py:491-564  |
 *   NormalH_of_v / PlusMinusH_of_v   functions.py:720-796  |
 *   for alpha in alpha_mesh:                               | mxe_solve_chains
 *      cost_function.set_alpha       maxent_loop.py:243    |   (one chain = one element's
 *      minimizer.minimize            maxent_loop.py:245    |    warm-started alpha scan)
 *        LevenbergMinimizer.minimize levenberg_minimizer.py:123-248
 *        MaxEntCostFunction.f/d/dd   maxent_cost_function.py:68-165
 *        BryanCostFunction.f/d/dd    bryan_cost_function.py:57-128
 *      Q_min = cost_function(v)      maxent_loop.py:246    | out_v/out_H/out_chi2/out_S/out_Q
 *      minimizer.n_iter_last/.converged  maxent_loop.py:254-256 | out_niter/out_converged
 *      self.probability(Q_min)       maxent_loop.py:258-264 | mxe_logdet (the determinant of
 *        NormalLogProbability        probabilities.py:60-85 |   the posterior curvature)
 *   PreblurA_of_H.f  A = B H         functions.py:999-1001 | mxe_apply_output_map
 *   result.analyze(analyzers): LineFitAnalyzer,            | mxe_select3_launch / mxe_select3_fetch
 *     Chi2CurvatureAnalyzer, EntropyAnalyzer               |   (alpha_index and the H row of each,
 *     maxent_result.py:793-822, analyzers/               |    for every scan of the launch)
 *   CostFunction.__call__ / .f / .d / .dd at a given v     | mxe_eval_batch, mxe_entropy, mxe_audit
 *     cost_function.py:73-85, maxent_cost_function.py:68-165
 *   TauKernel / PreblurKernel fill + KernelSVD.svd         | mxe_kernel_svd (optional: the host
 *     kernels.py:53-122,244-271,384-393                    |   numpy path stays the default)
 *   IOmegaKernel fill (stacked real [Re K ; Im K])         | mxe_kernel_svd_iw (the same, for
 *     + KernelSVD.svd   kernels.py:283-346                 |   Matsubara data)
 *   BosonicTauKernel / BosonicIOmegaKernel fill + SVD      | mxe_kernel_svd_boson / mxe_kernel_svd_boson_iw
 *     (chi(tau), chi(i nu_n); not in the reference)        |
 *   LegendreKernel fill + SVD (G_l; not in the reference)  | mxe_kernel_svd_legendre
 *   DataKernel (a caller's matrix) + KernelSVD.svd         | mxe_kernel_svd_data
 *     kernels.py:183-207                                   |
 *   get_G_w_from_A_w  maxent_util.py:43-132                | mxe_kramers_kronig (also get_chi_w_from_A_w)
 *   (nothing: the reference gives no error bars)           | mxe_posterior_var (posterior variances of
 *                                                          |   integrated quantities, diagonal of the covariance)
 *   (nothing: the reference draws no spectra)              | mxe_posterior_sample (draws of H from the same
 *                                                          |   Gaussian posterior), mxe_normals (its generator)
 *   (nothing: the reference gives no fit diagnostics)      | mxe_fit_diagnostics (leverages, number of good
 *                                                          |   data, whitened residuals of a fit)
 *   (nothing: the reference gives chi2(alpha) only)        | mxe_response (resolution operator of a fit, its
 *                                                          |   response to the data and to the default model)
 *   (nothing: users loop run() over their resamples)       | mxe_bins_resample (the rotated data of every
 *                                                          |   jackknife / bootstrap resample of the bins),
 *                                                          |   mxe_resample_reduce (mean, spread and functional
 *                                                          |   covariances of the H rows they were continued to)
 *   (nothing: users loop run() over mock data by hand)     | mxe_mock_data (mock data drawn from continued spectra
 *                                                          |   with the noise of the job), mxe_resample_quantiles
 *                                                          |   (percentile bands of the H rows of resamples or mocks)
 *   (nothing: no rule for alpha looks at held-out data)    | mxe_cv_score (out-of-sample chi2 of the training scans
 *                                                          |   of a k-fold split of the bins, for every alpha)
 *   (nothing: users rebin by hand until the errors settle) | mxe_bins_check (blocking ladder, skewness and
 *                                                          |   kurtosis of the block means of the bins)
 *   (nothing: few bins give a biased covariance)           | mxe_bins_eig_shrunk (shrinkage intensity from the
 *                                                          |   bins, eigenbasis of the shrunk covariance)
 *   (nothing: users loop run() over their default models)  | mxe_evidence_reduce (evidence of every default
 *                                                          |   model, model-averaged image, spread between models)
 *   (nothing: positivity of the matrix is not checked)     | mxe_hermitian_eig (eigenvalues of A(w) as a matrix,
 *                                                          |   its nearest positive semi-definite matrix)
 *   (nothing: "FullMatrixMaxEnt" is announced, not shipped) | mxe_fullmatrix_solve (the matrix A(w) as one unknown,
 *                                                          |   positive semi-definite by construction),
 *                                                          |   mxe_fullmatrix_solve_metric (the same with one
 *                                                          |   error bar per matrix element)
 *   the arrays of MaxEntResult (numpy allocations)         | mxe_host_alloc / mxe_host_free (optional:
 *     maxent_result.py:835-967                             |   page-locked destinations, one DMA per fetch)
 *
 * Conventions: plain C, no C++ types; every function returns 0 (MXE_OK) or a
 * negative error code and never throws or aborts; the caller owns every host
 * buffer (C-contiguous, row-major); the library owns device memory inside
 * mxe_ctx.  Calls on one ctx are not re-entrant; different ctxs (devices) may
 * be driven from different threads.  All arithmetic is IEEE binary64 unless
 * mxe_opts.precision asks for the binary32 streaming variant.
 */
#ifndef MAXENT_HIP_H
#define MAXENT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MXE_OK               0
#define MXE_ERR_ARG         -1   /* bad argument (NULL, size, index)          */
#define MXE_ERR_HIP         -2   /* a HIP runtime call failed (mxe_last_hip_error) */
#define MXE_ERR_NODEVICE    -3   /* no usable gfx950 device                   */
#define MXE_ERR_STATE       -4   /* call order (e.g. solve before elements)   */
#define MXE_ERR_LIMIT       -5   /* n_s > 128 (fp32: > 64); mxe_eval_batch / mxe_audit: w and H of a problem
                                     exceed the LDS next to the n_s x n_s matrix (n_omega > 7680 for n_s <= 64,
                                     n_omega > 1408 for 64 < n_s <= 128); the alpha scans themselves take any
                                     n_omega (state in device memory where the LDS does not hold it) */
#define MXE_ERR_NUMERIC     -6   /* whitening failed (non-positive error bar) / SVD sweeps exhausted or matrix not finite */
#define MXE_ERR_NOMEM       -7   /* host allocation failed                     */

#define MXE_PRECISION_F64      0 /* all arithmetic IEEE binary64 (default)      */
#define MXE_PRECISION_F32      1 /* omega-space streaming arithmetic in binary32 */

#define MXE_ENTROPY_NORMAL     0 /* NormalEntropy + NormalH_of_v              */
#define MXE_ENTROPY_PLUSMINUS  1 /* PlusMinusEntropy + PlusMinusH_of_v        */

typedef struct mxe_ctx mxe_ctx;

/* Options of the per-alpha minimiser.  Fill with mxe_opts_default() first.
 * Counterparts: LevenbergMinimizer.__init__ (levenberg_minimizer.py:92-121)
 * and convergence_methods.py:81-122. */
typedef struct mxe_opts {
    int32_t maxiter;      /* max Newton iterations per alpha (reference: 1000)            */
    int32_t miniter;      /* reference: 0                                                 */
    double  tol_h;        /* converged when the Newton correction satisfies
                             ||dH||_2 / ||H||_2 < tol_h   (0 = off); with stop_estimate
                             the ESTIMATED next correction is tested as well             */
    double  tol_d;        /* MaxDerivativeConvergenceMethod: max|W g| < tol_d (0 = off; reference default
                             1e-4).  The maximum runs over the coupled block (rows and columns of the
                             directions with c_k^2 max(w) > decouple_tol * alpha): the gradient
                             components of the decoupled directions are zeroed by their own diagonal
                             Newton step to relative decouple_tol and add nothing at that level; with
                             decouple_tol = 0 it is the reference's max over all n_s              */
    double  tol_relq;     /* RelativeFunctionChangeConvergenceMethod: |Q0-Q1|/|Q1| <
                             tol_relq (0 = off; reference default 1e-16)                  */
    double  step_max;     /* step bound  delta^T W delta <= step_max * sum(D)  (0.2)      */
    double  mu_first;     /* first non-zero damping, in units of alpha (1e-3)             */
    double  mu_grow;      /* growth factor of the damping on a rejected step (4)          */
    double  mu_max;       /* give up on the alpha when mu/alpha exceeds this (1e20)       */
    double  decouple_tol; /* theta: singular directions with c_k^2 max(w) <= theta*alpha
                             take the diagonal Newton step (1e-5; 0 = full n_s block)      */
    int32_t waves_per_chain; /* one-chain-per-workgroup layout: wavefronts per chain;
                                0 = choose from the chain count; else 1,2,4,8             */
    int32_t chains_per_wg;   /* 0 = auto; 1 = one chain per workgroup; 4 = four chains of
                                one data set per workgroup in lock-step (shared V loads)   */
    int32_t alpha_split;     /* cut every alpha scan into this many cold-started pieces
                                (more chains to fill the GPU; results are path independent);
                                0 = auto: about two pieces per chain slot of the GPU, a piece
                                of a normal-entropy scan counting twice, none shorter than two
                                alphas (binary32 variant: at most 16, none shorter than six);
                                1 = never.  In either case a piece of a normal-entropy scan
                                that would start among the scan's smallest alphas (the last 6 %
                                of its logarithmic range, where a cold start from the default
                                model can take hundreds of iterations) solves the last alpha above
                                that range cold instead and walks down the mesh to its own alpha with a
                                loose tolerance (lock-step layout: every alpha of that range is a piece
                                of its own; one-chain layout: joined to the piece before) */
    int32_t stop_estimate;   /* 1 (default): after a full (undamped) Newton step the next
                                correction is estimated as (expm1(max|du|) + decouple_tol) * ||dH||/||H||
                                (the relative change of the weights w bounds the relative
                                change of the Jacobian) and tol_h is applied to it, which
                                saves the last, verifying iteration; 0: tol_h is applied to
                                the correction just taken only                              */
    int32_t precision;       /* MXE_PRECISION_F64 (default) or MXE_PRECISION_F32: V, u = V v, w, H,
                                exp, h = V^T H and the Gram matrix in binary32 (the Gram matrix by split-f16
                                MFMA in the lock-step kernel, from V^T in the LDS as binary32 in chain_kernel_lv); the
                                n_act x n_act Newton system, the residual and all scalars stay
                                binary64.  An alpha also stops when its Newton correction has
                                reached the rounding floor (it no longer shrinks).  n_s <= 64.
                                Where V^T fits the LDS as binary32 the launch runs in the lock-step
                                kernel chain_kernel_lv (mxe_opts.lds_basis), else one chain per
                                workgroup.  A request, not a promise: binary32 is asked for as the cheaper
                                arithmetic, and a launch for which it is not is PROMOTED to binary64 -- a
                                job with an alpha that couples more than 32 directions (error bars far
                                below the noise of the data: the lock-step build with the 64-row block),
                                and, with wg_per_cu = 0, a batch that fills the GPU at two workgroups per
                                CU (the binary64 kernel that runs that way: 0.81 against 1.24 ms on the
                                16 x 16 x 100 batch; wg_per_cu = 1 keeps chain_kernel_lv), and a frequency
                                mesh whose basis does not fit the LDS as binary32 (n_omega > 512: one chain
                                per workgroup in binary32 takes 3.6-7.8 ms where the binary64 lock-step
                                kernel takes 0.5-1.7; lds_basis = 2 or chains_per_wg = 1 keep that kernel);
                                mxe_last_launch_info names the kernel that ran.  For the fp32-vs-fp64 tolerance sweep of BASELINE config 5
                                (tools/cfg5_tolerance_sweep.py)                                 */
    int32_t wg_per_cu;       /* lock-step layout: workgroups per CU.  0 = auto (2 where the kernel has a
                                build for it: n_s <= 64 active block 32, n_omega <= 512 -- u then lives in
                                registers and two workgroups of 73 KB share a CU, so that the serial
                                sections of one overlap the streaming passes of the other), 1, 2   */
    double  chi2_factor;     /* eta in Q = eta chi2 / 2 - alpha S (CostFunction(chi2_factor=...),
                                cost_function.py:60, bryan_cost_function.py:71); default 1       */
    int32_t lds_basis;       /* lock-step layout with V^T resident in the LDS as binary32 (chain_kernel_lv; it needs
                                n_s * (n_omega_pad + 4) * 4 B + 47 KB <= 160 KB: the BASELINE grids just fit).
                                0 = auto: it IS the launch for precision = MXE_PRECISION_F32 (where the basis fits) and is
                                NOT used by binary64 launches;
                                1 = opt-in: also the first pass of every binary64 launch (every alpha to 1e-5 in binary32,
                                then one binary64 Newton step per alpha in the lock-step kernel, all alphas side by side) --
                                correct, measured NOT faster than the plain binary64 launch, hence not auto;
                                2 = never                                                                        */
    int32_t in_flight;       /* batches of this size the caller keeps in flight on the GPU (launches of several
                                contexts enqueued without waiting in between): 0 or 1 = one -- the scans are cut into
                                enough cold-started pieces to fill the GPU on their own --, n > 1: into 1 / n as many
                                (a cold start costs 4-17 evaluations: with n batches side by side the GPU is full
                                without them; bench.py --in-flight 4: 0.83 -> 0.65 ms per batch of 25 600 alpha-solves).
                                The latency of ONE batch grows (1.7 ms for n = 4)                                */
} mxe_opts;

/* ---- library / device ------------------------------------------------- */
const char* mxe_version(void);
/* first 16 hex digits of the SHA-256 over the library's sources (the .hip and .hip.h files of csrc/, this header) as the Makefile
   saw them when it built this binary: bench.py only trusts a counter profile under profiles/ that records the same hash */
const char* mxe_source_hash(void);
/* Page-locked host memory for result arrays (the destination of mxe_chains_fetch / mxe_fetch_rows / mxe_select3_fetch may be
   any host memory; into a block of this call the copy is one DMA at the rate of the link -- all H of the BASELINE batch,
   102 MB: 3 ms against 11-22 ms into pageable memory).  The library keeps a few freed blocks for the next call.  NULL when
   the runtime cannot pin that much.  What they replace in the reference: numpy's allocation of MaxEntResult's arrays
   (maxent_result.py:835-967). */
void* mxe_host_alloc(size_t bytes);
void  mxe_host_free(void* block);
const char* mxe_strerror(int code);
int  mxe_device_count(int* n_devices);
void mxe_opts_default(mxe_opts* opts);

/* ---- context: one per device; holds the truncated SVD of the kernel ---- */
/* U: n_tau x n_s, S: n_s, V: n_omega x n_s (row-major, as KernelSVD.U/.S/.V
 * return them, kernels.py:66-94).  U is only used as the default data set 0
 * together with `err` given to mxe_dataset_add; it may be NULL if every data
 * set brings its own (rotated) U. */
int  mxe_ctx_create(int device, int n_tau, int n_omega, int n_s,
                    const double* U, const double* S, const double* V,
                    mxe_ctx** out);
void mxe_ctx_destroy(mxe_ctx* ctx);
const char* mxe_last_hip_error(mxe_ctx* ctx);

/* ---- data sets: a (U, err) pair = one whitened singular basis ---------- */
/* U_rot: n_rows x n_s left factor in the (possibly covariance-rotated) data
 * space (Kernel.transform, kernels.py:160-180); NULL = the ctx's U (then
 * n_rows must equal n_tau).  err: n_rows standard deviations
 * (TauMaxEnt.set_error / set_cov, tau_maxent.py:227-288).
 * Returns the data-set id (>= 0) in *id. */
int  mxe_dataset_add(mxe_ctx* ctx, int n_rows, const double* U_rot,
                     const double* err, int* id);
int  mxe_dataset_clear(mxe_ctx* ctx);

/* ---- elements: the matrix elements of G that will be continued -------- */
/* dataset_of_elem[e]: data-set id; G: concatenated data vectors, element e
 * has n_rows(dataset) entries starting at G_offset[e] (already rotated into
 * the data set's space); D: n_elem x n_omega default models INCLUDING
 * delta-omega (default_models.py:61-63); entropy[e]: MXE_ENTROPY_*. */
int  mxe_elements_set(mxe_ctx* ctx, int n_elem, const int32_t* dataset_of_elem,
                      const double* G, const int64_t* G_offset,
                      const double* D, const int32_t* entropy);
/* New DATA for the elements that are set (same number, same data sets, default models and entropies): G as above.  Only the
 * projections of the data change on the device; the staged chains (mxe_chains_upload: their cut into pieces, the start
 * states) do not depend on G and stay ready -- what every iteration of a self-consistency loop does to an
 * ElementwiseMaxEnt on fixed grids (reference: set_G_tau_data again, elementwise_maxent.py:373-395, then run()).
 * MXE_ERR_STATE when no elements are set, MXE_ERR_ARG when n_elem differs. */
int  mxe_elements_update_data(mxe_ctx* ctx, int n_elem, const double* G, const int64_t* G_offset);

/* ---- the hot path ------------------------------------------------------ */
/* n_chain warm-started alpha scans of n_alpha values each.
 *   elem_of_chain[c]          element index
 *   alpha_scaled[c*n_alpha+i] alpha * scale_alpha (maxent_loop.py:216-243),
 *                             in the order they are to be visited
 *   v0[c*n_s + k]             start vector in the caller's singular basis
 *                             (maxent_loop.py:196-203)
 * Outputs (host pointers, any may be NULL), problem p = c*n_alpha + i:
 *   out_v[p*n_s+k]  optimum in the caller's singular basis
 *   out_H[p*n_omega+j] hidden image H(v)   out_chi2/out_S/out_Q[p]
 *   out_niter[p] iterations (minimizer.n_iter_last)   out_converged[p] 0/1
 *   (an alpha whose minimisation FAILED -- damping exhausted, nothing finite to evaluate: converged 0
 *    before maxiter -- reports v, chi2, S, Q of its last accepted iterate and H = NaN)
 *   out_nevals[p] cost evaluation passes spent on p
 * Blocking: returns after the results are in the host buffers. */
int  mxe_solve_chains(mxe_ctx* ctx, int n_chain, int n_alpha,
                      const int32_t* elem_of_chain, const double* alpha_scaled,
                      const double* v0, const mxe_opts* opts,
                      double* out_v, double* out_H, double* out_chi2,
                      double* out_S, double* out_Q, int32_t* out_niter,
                      int32_t* out_converged, int32_t* out_nevals);

/* Device-resident variant used by bench.py and by multi-GPU drivers:
 * mxe_chains_upload stages the chain description once; mxe_chains_launch
 * enqueues one pass of the solver on the ctx stream (inputs already in HBM),
 * bracketed by HIP events; mxe_sync waits for it; mxe_chains_fetch copies the
 * results to host buffers (same layout as mxe_solve_chains).
 * mxe_result_device_ptrs exposes the device result buffers (for an RCCL
 * gather driven by the caller); layouts as above except v, which is in the
 * whitened basis with row stride mxe_ns_padded() (use mxe_chains_fetch for
 * caller-basis v).  H, chi2, S, Q are contiguous in that order in ONE
 * allocation of P*n_omega + 3*P doubles starting at d_H, so that one
 * collective moves all per-alpha results.
 * A lock-step launch (chain_kernel_mc) whose pieces come off a queue puts NO reset of the queue counter in front of the
 * kernel: the counter is a pair of words, launch k of a context draws from word k & 1, and its first thread stores the
 * start value of launch k + 1 into the other word, which launch k - 1 has finished with (the launches of a context are
 * ordered by its stream).  mxe_chains_upload sets both words and starts at word 0; a launch that could not be enqueued
 * does not advance the turn.  The two passes of a launch that starts in chain_kernel_lv keep two words of their own and
 * their reset.  mxe_chains_upload also tabulates log and log10 of the staged alphas on the device for mxe_select_launch /
 * mxe_select3_launch (it is the only writer of the staged alphas, so the table cannot go stale). */
int  mxe_chains_upload(mxe_ctx* ctx, int n_chain, int n_alpha,
                       const int32_t* elem_of_chain, const double* alpha_scaled,
                       const double* v0, const mxe_opts* opts);
int  mxe_chains_launch(mxe_ctx* ctx);
int  mxe_sync(mxe_ctx* ctx);
/* Blocking.  After a launch in the lock-step layout: the alphas that did not converge there are solved again in
 * the one-chain layout, from the state they were left in, and their records are overwritten (iteration and
 * evaluation counts: both passes).  The lock-step kernel forms its Gram matrices from binary16 products (21 bits):
 * an inexact Newton matrix that is harmless where the system is well conditioned and stalls where it is not (few
 * data points, small alpha); it gives an alpha up after 32 iterations, and the one-chain kernel (binary64 Gram
 * matrix) takes it from there with the rest of mxe_opts.maxiter.  n_resolved (may be NULL): how many alphas that
 * was.  Alphas that couple more than the 32 directions the lock-step kernel has a build for (error bars far below
 * 1e-5 of the data: the smallest alphas of a scan) are not in its pieces at all when they are the smaller part of the
 * batch: after mxe_chains_launch their records read NaN / not converged / 0 iterations, and this call solves them
 * as one warm chain per scan from the last alpha before them -- a launch is complete after mxe_chains_finish, not
 * before.  A no-op after a launch in the one-chain layout or when everything converged.  mxe_solve_chains calls it;
 * what it replaces in the reference is nothing but the remaining iterations of levenberg_minimizer.py:155-243. */
int  mxe_chains_finish(mxe_ctx* ctx, int32_t* n_resolved);
int  mxe_chains_fetch(mxe_ctx* ctx, double* out_v, double* out_H,
                      double* out_chi2, double* out_S, double* out_Q,
                      int32_t* out_niter, int32_t* out_converged,
                      int32_t* out_nevals);
/* The two blocks of per-alpha scalars queued behind the launch on the context's stream, so that a caller with jobs in flight on
 * several contexts finds them in its memory when the kernel has finished instead of copying them out, job after job, when all
 * kernels are done: out_chi2_S_Q [3][P] (chi2 | S | Q), out_niter_converged_nevals [3][P].  Both should be page-locked
 * (mxe_host_alloc), or the runtime stages them.  mxe_chains_fetch given exactly these destinations waits for the stream and
 * copies nothing; mxe_chains_finish, when it solves anything again, makes the next fetch copy afresh.  The destinations must
 * stay allocated until a call that waits for the stream has returned.  Replaces nothing of the reference (its per-alpha
 * scalars are Python floats as they are made, maxent_loop.py:330-353): plumbing of the asynchronous boundary. */
int  mxe_chains_prefetch(mxe_ctx* ctx, double* out_chi2_S_Q, int32_t* out_niter_converged_nevals);
/* log det(I + M W / alpha~) at the returned point of every problem of the last launch,
 * [n_chain][n_alpha], over all n_s kept singular directions (M = S U^T diag(1/err^2) U S,
 * W = V^T diag(w) V).  It is the only expensive term of NormalLogProbability
 * (probabilities.py:60-85: two n_omega x n_omega slogdet per alpha in the reference):
 * log p = -1/2 logdet - Q - log(alpha~) with the default norm and prior. */
int  mxe_logdet(mxe_ctx* ctx, double* out_logdet);
/* diagnostic: size of the coupled (active) block of the last Newton iteration of
 * every problem, [n_chain][n_alpha] (see mxe_opts.decouple_tol) */
int  mxe_chains_fetch_nact(mxe_ctx* ctx, int32_t* out_nact);
int  mxe_result_device_ptrs(mxe_ctx* ctx, void** d_H, void** d_chi2,
                            void** d_S, void** d_Q, void** d_v,
                            void** d_niter, void** d_converged);
int  mxe_ns_padded(mxe_ctx* ctx);
/* two result allocations (0, 1): the next launches / fetches / pointer queries use
 * `which`, so that a driver can gather buffer k while the solver fills buffer 1-k */
int  mxe_set_result_buffer(mxe_ctx* ctx, int which);
/* duration of the last mxe_chains_launch in ms (HIP events on the ctx stream) */
int  mxe_last_kernel_ms(mxe_ctx* ctx, float* ms);
/* mxe_timing_mark records an event on the ctx stream; mxe_ms_since_mark waits for the end of the
 * last launch and returns the device time from the mark to it: the duration of a run of launches
 * that were enqueued back to back, without a host synchronisation in between */
int  mxe_timing_mark(mxe_ctx* ctx);
int  mxe_ms_since_mark(mxe_ctx* ctx, float* ms);
/* the HIP stream (hipStream_t) the ctx launches on, for callers that order their own device work
 * (an RCCL gather of the result buffers) against it with events instead of host synchronisation */
void* mxe_stream(mxe_ctx* ctx);
/* name of the kernel instantiation the last mxe_chains_launch ran, as a profiler shows it
 * (e.g. "mxe::chain_kernel_mc<32, 4>"); owned by the ctx */
const char* mxe_last_kernel_name(mxe_ctx* ctx);
/* kernel geometry of the last launch: waves per chain, workgroups, LDS bytes */
int  mxe_last_launch_info(mxe_ctx* ctx, int* waves_per_chain, int* n_workgroups,
                          int* lds_bytes);
/* Depth of the last lock-step launch in ROUNDS (one Newton iteration of the four chain slots of a workgroup): maximum and mean over
 * its workgroups.  The reference's scan is one serial chain of n_alpha x ~16 iterations (maxent_loop.py:241-245 around
 * levenberg_minimizer.py:155); here a launch that does not fill the GPU is as long as its deepest workgroup, and this is that depth
 * as the kernel counted it (bench.py: scaling_projection.bound divides the measured time by it).  [0]: the launch, or the binary32
 * first pass of a two-pass launch (mxe_opts.lds_basis); [1]: the second pass (0 when there is none).  One-chain layout: zeros.
 * Blocking. */
int  mxe_launch_depth(mxe_ctx* ctx, int32_t* max_rounds /*[2]*/, double* mean_rounds /*[2]*/);
/* The schedule of the staged chains (after mxe_chains_upload): n_solo = workgroups of a two-per-CU lock-step launch that get a CU to
 * themselves for the longest pieces (the tails of the normal-entropy scans; the serial alpha loop they replace: maxent_loop.py:241-245).
 * That schedule rests on which workgroups share a CU -- b and b + gridDim / 2 --, an observed placement that HIP does not promise: the
 * library probes it once per device (a 25 us kernel that records XCC_ID / HW_ID) and drops the solo workgroups where it does not
 * hold.  placement_rule: 0 = the upload wanted none, 1 = probed and holds, 2 = does not hold (n_solo = 0).  Results never depend
 * on it; MXE_FORCE_NO_SOLO_RULE in the environment forces 2. */
int  mxe_schedule_info(mxe_ctx* ctx, int* n_solo, int* placement_rule);

/* ---- the cost function and its derivatives at caller-supplied points --- */
/* Device side of CostFunction.__call__ / f / d / dd (cost_function.py:73-85),
 * MaxEntCostFunction.f/dH/d/ddH/dd (maxent_cost_function.py:68-165), BryanCostFunction.f/d/dd
 * (bryan_cost_function.py:57-128) and of the component functions NormalChi2, NormalEntropy /
 * PlusMinusEntropy, NormalH_of_v / PlusMinusH_of_v (functions.py:336-796), for a batch of P points.
 *   elem_of_problem[p]  element (its G, err, D, entropy) the point belongs to
 *   alpha_scaled[p]     alpha * scale_alpha (>= 0)
 *   x                   input_is_H = 0: v, [P][n_s], the caller's singular basis
 *                       input_is_H = 1: the hidden image H itself, [P][n_omega] (the component functions
 *                       chi2(H), S(H) and H_of_v.inv: u = log(H/D) | log((H + sqrt(H^2 + 4 D^2)) / 2D))
 *   chi2_factor         eta in Q = eta chi2 / 2 - alpha S
 * Outputs (host, any may be NULL):
 *   out_Q, out_chi2, out_S [P];  out_H, out_u (= V v), out_w (= dH/du), out_q (= V g = dQ/dH) [P][n_omega];
 *   out_h = V^T H, out_g = eta (M h - b) + alpha v  [P][n_s]     (input_is_H: no alpha v term)
 *   out_W  = V^T diag(w) V,  out_W2 = V^T diag((V g) H) V        [P][n_s][n_s]
 * from which every derivative of the reference follows with M = S U^T diag(1/err^2) U S:
 *   default (dA_projection = 2):  d = W g        dd = W M' W + alpha W       (M' = eta M)
 *   dA_projection = 1:            d = g          dd = M' W + alpha I
 *   dA_projection = 0:            d = V g        dd = V M' W + alpha V       (n_omega rows)
 *   d_dv = True:                  d = W g        dd = W M' W + alpha W + W2
 *   BryanCostFunction:            d = g          dd = M' W
 *   dQ/dH = V g;  dchi2/dH = 2 V (M h - b);  dS/dH = -u;  d2S/dH2 = -diag(1/w);  dH/dv = diag(w) V */
int  mxe_eval_batch(mxe_ctx* ctx, int P, const int32_t* elem_of_problem, const double* alpha_scaled,
                    const double* x, int input_is_H, double chi2_factor,
                    double* out_Q, double* out_chi2, double* out_S,
                    double* out_H, double* out_u, double* out_w, double* out_q,
                    double* out_h, double* out_g, double* out_W, double* out_W2);
/* Posterior error bars in the Gaussian approximation around the minimiser (Bryan 1990; Jarrell & Gubernatis 1996,
 * section 5).  Replaces nothing of the reference, which offers none.  With w = H (normal entropy) or sqrt(H^2 + 4 D^2)
 * (plus-minus), the whitened basis K^T Sigma^-1 K = V' c^2 V'^T and a = alpha~ / eta the covariance of H is
 *   Gamma = (eta K^T Sigma^-1 K + alpha~ diag(1/w))^-1 = (1/alpha~) [diag(w) - diag(w) V' c B^-1 c V'^T diag(w)],
 *   B = c W c + a I,  W = V'^T diag(w) V',  B = L L^T  (the matrix and the factor of mxe_logdet), so that
 *   out_var[p][j]   = f_j^T Gamma f_j = (1/alpha~) [sum_i w_i f_ji^2 - |L^-1 y|^2],  y = c o V'^T (w o f_j)
 *   out_prior[p][j] = f_j^T diag(w) f_j / alpha~     (what the entropy alone would leave: var <= prior)
 *   out_diag[p][i]  = Gamma_ii = (w_i / alpha~) [1 - w_i |L^-1 (c o V'_i)|^2]
 * for P problems on the staged elements of ctx (data set, entropy and D of elem_of_problem[p], as mxe_eval_batch) at
 * alpha_scaled[p] > 0 and the hidden images
 *   H != NULL:  H [P][n_omega], host (results outlive launches);
 *   H == NULL:  rows of the last launch, read where they lie on the device: row problem_index[p] = chain * n_alpha +
 *               alpha index (problem_index == NULL: row p).  MXE_ERR_STATE when nothing was launched.
 * F: n_f x n_omega weights on H (host, finite; n_f may be 0 with F == NULL when only out_diag is wanted); out_prior and
 * out_diag may be NULL.  The differences are formed as written, never through B^-1; one that rounding makes negative
 * is returned as 0 (a NaN stays a NaN).  A problem whose H row is not finite or whose B is not positive definite gets NaN in all its
 * outputs, the others are not touched by it and the call returns MXE_OK.  The bits of a value do not depend on the
 * other problems or functionals of the call (fixed summation order, no atomics).  out_ms: device time of the kernel
 * (may be NULL).  MXE_ERR_LIMIT when B and w exceed 160 KB of LDS (n_omega > 15872 with n_s <= 64,
 * > 3584 with n_s <= 128; the right-hand sides live in the part of B that its factor leaves free). */
int  mxe_posterior_var(mxe_ctx* ctx, int P, const int32_t* elem_of_problem, const double* alpha_scaled,
                       const double* H, const int32_t* problem_index, double chi2_factor,
                       int n_f, const double* F, double* out_var, double* out_diag, double* out_prior,
                       float* out_ms);
/* Draws from the Gaussian posterior that mxe_posterior_var integrates, for error bars of what is not linear in A (a peak
 * position, a gap edge, Sigma(omega)).  Replaces nothing of the reference.  In the notation above (w, V', c, a = alpha~ /
 * eta, B = c W c + a I = L L^T), with z1 [n_omega] and z2 [n_s] independent standard normals:
 *   q_i     = sqrt(a w_i) z1_i + w_i V'_i . (c o z2)        (q = w o r, cov r = a diag(1/w) + V' c^2 V'^T; no division by w)
 *   y       = c o V'^T q
 *   x       = L^-T L^-1 y                                     (forward, then backward substitution; B^-1 is never formed)
 *   delta_i = (1/a) [q_i - w_i V'_i . (c o x)] / sqrt(eta)
 * so that cov delta = Gamma exactly; w_i = 0 gives delta_i = 0.  out_dH [P][n_samples][n_omega] (host) receives delta:
 * a sample of H is the minimiser plus its row.  elem_of_problem, alpha_scaled, H, problem_index and chi2_factor as in
 * mxe_posterior_var (also the rows of the last launch with H == NULL, and MXE_ERR_STATE).
 *   z == NULL:  the normals are generated on the device, see mxe_normals: problem p draws from (seed, stream[p]), its
 *               sample s uses the normals 0 .. n_omega-1 as z1 and n_omega .. n_omega+n_s-1 as z2 (n_s: the kept rank);
 *   z != NULL:  z [P][n_samples][n_omega + n_s] on the host, finite, used as given (seed and stream are ignored).
 * A problem whose H row is not finite or whose B is not positive definite gets NaN in all its samples, the others are
 * not touched and the call returns MXE_OK.  No atomics, fixed summation order: the bits of sample s of a problem depend on
 * neither the other problems of the call nor on n_samples.  MXE_ERR_ARG: n_samples < 1, P n_samples (n_omega + n_s) >
 * 2^31 - 1, a z that is not finite.  MXE_ERR_LIMIT as mxe_posterior_var.  out_ms: device time (may be NULL). */
int  mxe_posterior_sample(mxe_ctx* ctx, int P, const int32_t* elem_of_problem, const double* alpha_scaled,
                          const double* H, const int32_t* problem_index, double chi2_factor,
                          int n_samples, uint64_t seed, const uint64_t* stream, const double* z,
                          double* out_dH, float* out_ms);
/* Diagnostics of a fit from its hat matrix, the derivative of the fitted whitened data Sigma^-1/2 K H with respect to
 * the whitened data Sigma^-1/2 G (exact at the minimiser).  Replaces nothing of the reference.  In the notation above
 * (w, V', c, a = alpha~ / eta, B = c W c + a I = L L^T) and with Sigma^-1/2 K = U^ c V'^T, g^ = U^^T G~, G~ = Sigma^-1/2 G:
 *   Hat             = U^ (I - a B^-1) U^^T
 *   out_lev[p][i]   = h_i = |U^_i|^2 - a |L^-1 U^_i^T|^2                  (leverage of data point i, 0 <= h_i <= |U^_i|^2)
 *   out_ngood[p]    = N_g = sum_i h_i = sum_k lambda_k / (lambda_k + a)   (number of good data; lambda: eigenvalues of c W c)
 *   out_resid[p][i] = r_i = sum_k U^_ik rho_k - rperp_i = [Sigma^-1/2 (K H - G)]_i,
 *                     rho = c o V'^T H - g^,  rperp = G~ - U^ g^          (the part of the data outside the singular space)
 *   out_chi2[p]     = sum_i r_i^2 = |rho|^2 + c_perp                      (the chi2 of the solver)
 * The rows i are those of the problem's data set (tau points, the 2 n_iw stacked real Matsubara values, the kept
 * eigen-directions of a covariance).  out_resid and out_lev are [P][ld] with ld at least the largest row count among the
 * data sets of the problems named (else MXE_ERR_ARG); entries behind a data set's rows are written as 0.
 * elem_of_problem, alpha_scaled, H, problem_index and chi2_factor as in mxe_posterior_var (also the rows of the last launch
 * with H == NULL, and MXE_ERR_STATE); only a = alpha~ / chi2_factor enters.  Every output pointer may be NULL.  The
 * leverage is formed as written, never through B^-1; a difference that rounding makes negative is returned as 0 (a NaN
 * stays a NaN).  A problem whose H row is not finite or whose B is not positive definite gets NaN in all its outputs,
 * the others are not touched by it and the call returns MXE_OK.  No atomics, fixed summation order (N_g and chi2 are added
 * in index order): the bits of a problem do not depend on the other problems of the call.  U^ of the data sets and rperp
 * of the elements go to the device at the first call and after any change of data sets or elements
 * (mxe_elements_update_data keeps rperp current).  MXE_ERR_LIMIT as mxe_posterior_var.  out_ms: device time of the kernel
 * (may be NULL). */
int  mxe_fit_diagnostics(mxe_ctx* ctx, int P, const int32_t* elem_of_problem, const double* alpha_scaled,
                         const double* H, const int32_t* problem_index, double chi2_factor, int ld,
                         double* out_ngood, double* out_chi2, double* out_resid, double* out_lev, float* out_ms);
/* The linear response of the minimiser: what the continuation does to a feature that is really there.  Replaces nothing
 * of the reference.  Differentiating the stationarity condition of Q = eta chi2 / 2 - alpha~ S gives, in the notation
 * above (w, V', c, a = alpha~ / eta, B = c W c + a I = L L^T, Sigma^-1/2 K = U^ c V'^T), exactly at the minimiser
 *   space 1 (data):   dH = diag(w) V' c B^-1 U^^T dG~            dG~ = Sigma^-1/2 dG in the rows of the problem's data set
 *   space 0 (model):  dH = R f,  R = diag(w) S,  S = V' c B^-1 c V'^T = S^T     (f: a perturbation of the true H, dG = K f)
 *                     R = I - alpha~ Gamma diag(1/w),  tr R = sum_k lambda_k / (lambda_k + a) = N_g of mxe_fit_diagnostics
 *   default model:    dH = (I - R)(H o dlnD)  for both entropies (the caller subtracts)
 * out_X[p][j] = [diag(w)] V' c B^-1 y_j with y_j = c o V'^T F[p][j] (space 0) or U^^T F[p][j] (space 1); diag(w) only when
 * weighted != 0 (weighted == 0 in space 0 gives the rows of the symmetric S: column j of it is row j, so
 * w_j S_j. is the averaging kernel of the value returned at omega_j).  Only a enters: eta scales nothing.
 * F [P][n_rhs][ld], host, finite: ld >= n_omega in space 0 (the first n_omega entries of a row are used), in space 1 at
 * least the largest row count among the data sets of the problems named; entries behind a data set's rows do not enter
 * the result, but like every entry of F they must be finite (the check covers all P n_rhs ld values).
 * out_X [P][n_rhs][n_omega], host.  elem_of_problem, alpha_scaled, H, problem_index and chi2_factor as in
 * mxe_posterior_var (also the rows of the last launch with H == NULL, and MXE_ERR_STATE).  x = L^-T L^-1 y by a forward
 * and a backward substitution; B^-1 is never formed.  A problem whose H row is not finite or whose B is not positive
 * definite gets NaN in all its outputs, the others are not touched by it and the call returns MXE_OK.  No atomics, fixed
 * summation order: the bits of a column depend on neither the other problems of the call, nor on n_rhs, nor on the
 * column's place among the right-hand sides.  MXE_ERR_ARG: n_rhs < 1, space other than 0 or 1, ld too small, an F that is
 * not finite, P n_rhs max(ld, n_omega) > 2^31 - 1.  MXE_ERR_LIMIT as mxe_posterior_var.  out_ms: device time of the kernel
 * (may be NULL). */
int  mxe_response(mxe_ctx* ctx, int P, const int32_t* elem_of_problem, const double* alpha_scaled,
                  const double* H, const int32_t* problem_index, double chi2_factor,
                  int space, int weighted, int n_rhs, int ld, const double* F, double* out_X, float* out_ms);
/* The standard normals of mxe_posterior_sample, out_z [n_samples][n] (host), by the same device function.  Philox4x32-10
 * (Salmon et al. 2011; multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9, 0xBB67AE85) with the key (seed low,
 * seed high) and the counter (j, s, stream low, stream high): s the sample, j the pair of normals.  From the output
 * words x0..x3:  u1 = (((x0 2^32 + x1) >> 11) + 0.5) 2^-53, u2 likewise from x2, x3,
 *   z_2j = sqrt(-2 ln u1) cos(2 pi u2),  z_2j+1 = sqrt(-2 ln u1) sin(2 pi u2)      (|z| < 8.7).
 * A sample's normals depend on (seed, stream, s) alone.  maxent_amd.posterior.sample_normals is the host mirror. */
int  mxe_normals(int device, uint64_t seed, uint64_t stream, int n_samples, int n, double* out_z);
/* NormalEntropy / PlusMinusEntropy as functions of a hidden image given directly (functions.py:508-520,
 * 544-564): S, dS/dH and the diagonal of d2S/dH2 for P images H [P][n_omega] and one default model D
 * [n_omega] (including delta-omega).  No context needed; outputs may be NULL. */
int  mxe_entropy(int device, int kind, int n_omega, int P, const double* H, const double* D,
                 double* out_S, double* out_dS, double* out_ddS);
/* Audit of the last launch, every problem, binary64, all n_s directions (no active-subspace cut, no
 * binary16 tiles): at the returned v the exact Newton correction delta of Bryan's system is computed and
 *   out_corr[p] = ||w * V delta||_2 / ||H||_2   -- to first order the relative L2 distance of the
 *                 returned H from the minimiser (the quantity mxe_opts.tol_h bounds by an estimate)
 *   out_gmax[p] = max_k |g_k| / (|eta c_k rho_k| + |alpha v_k|),  g = eta c rho + alpha v  -- the gradient
 *                 against its cancelling terms, in the whitened basis of the problem's data set (the audit
 *                 itself runs with eta = 1 on the alpha / eta the chains iterated on)
 * [n_chain][n_alpha]; either may be NULL. */
int  mxe_audit(mxe_ctx* ctx, double* out_corr, double* out_gmax);

/* ---- the default analyzer's alpha on the device; selected rows ---------- */
/* LineFitAnalyzer (analyzers/linefit_analyzer.py:28-87,151-183: the kink of log chi2 over log alpha,
 * linefit_deg = p2_deg) for every scan of the last launch, enqueued on the ctx stream behind it; the H
 * of the chosen alpha is copied next to chi2 / S / Q, which makes the COMPACT result pack
 *     chi2 [P] | S [P] | Q [P] | H_selected [n_chain][n_omega] | index [n_chain] (as doubles)
 * contiguous on the device (P = n_chain * n_alpha).  index = -1: no fit (fewer than five alphas, chi2 NaN). */
int  mxe_select_launch(mxe_ctx* ctx, int p2_deg);
int  mxe_select_fetch(mxe_ctx* ctx, int32_t* out_index, double* out_H_selected);
/* The three default analyzers of the reference in one launch (it also fills the compact pack like mxe_select_launch):
 *   0  LineFitAnalyzer (as above),
 *   1  Chi2CurvatureAnalyzer (analyzers/chi2_curvature_analyzer.py:25-49,101-131): the alpha of the largest curvature
 *      y'' / (1 + y'^2)^(3/2) of y = log10 chi2 over x = gamma log10 alpha, NaN ignored, the first of equal maxima,
 *   2  EntropyAnalyzer (analyzers/entropy_analyzer.py:72-103): the alpha where (dS / dlog alpha)^2 is smallest;
 * mxe_select3_fetch: out_index [3][n_chain] (-1: nothing to choose from), out_H_selected [3][n_chain][n_omega] (may be
 * NULL), both in ONE device-to-host copy. */
int  mxe_select3_launch(mxe_ctx* ctx, int p2_deg, double gamma);
int  mxe_select3_fetch(mxe_ctx* ctx, int32_t* out_index, double* out_H_selected);
/* The same, the rows of the analyzers first .. first + count - 1 only (out_H_selected [count][n_chain][n_omega]; out_index
 * [3][n_chain] or NULL): a caller whose default analyzer is the line fit takes its row behind the launch and those of the
 * other two when somebody looks at them (result.analyzer_results[...]['A_out'], maxent_result.py:600-640 of the reference
 * reads one analyzer's A_out at a time).  The rows stay valid until the next mxe_select3_launch / mxe_chains_upload. */
int  mxe_select3_fetch_rows(mxe_ctx* ctx, int32_t* out_index, int first, int count, double* out_H_selected);
/* The copies of mxe_select3_fetch_rows queued behind the selection kernel (see mxe_chains_prefetch): the indices into memory of
 * the context, the rows into out_H_selected (page-locked; to stay allocated until a call that waits for the stream has
 * returned).  mxe_select3_fetch_rows with the same first / count / out_H_selected then waits and converts the indices. */
int  mxe_select3_prefetch_rows(mxe_ctx* ctx, int first, int count, double* out_H_selected);
/* n_rows hidden images of the last launch by problem index (chain * n_alpha + i), [n_rows][n_omega]:
 * what an analyzer needs (one row per scan) without moving all of H */
int  mxe_fetch_rows(mxe_ctx* ctx, int n_rows, const int32_t* problem_index, double* out_H);

/* ---- several GPUs: shard by matrix element, one gather ------ */
/* The (element, alpha) problems are independent given U, S, V: element e goes to rank e mod n_ranks
 * (mxe_shard_plan), every rank stages the basis itself and solves its shard with the same entry points;
 * afterwards ONE gather brings the result packs to the root's device (and, if asked, to its host):
 * RCCL send / recv over xGMI, called directly from this library (librccl.so.1 is loaded on first use).
 *   ranks in separate processes:  rank 0 calls mxe_comm_unique_id and hands the 128 bytes to the others
 *                                 (file, socket, environment: the caller's business); every rank calls
 *                                 mxe_comm_init(ctx, n_ranks, rank, id) and, per step, mxe_gather.
 *   ranks in one process:         mxe_comm_init_local(ctxs, n) (rank = position; contexts on the same
 *                                 device -- used for tests on one GPU -- gather with device copies
 *                                 instead of RCCL) and, per step, mxe_gather_local.
 * what: MXE_GATHER_COMPACT (the pack above; needs mxe_select_launch first) or MXE_GATHER_FULL (all H
 * in front of it).  counts[r]: doubles rank r contributes (checked against the rank's own launch).
 * The gather is enqueued on the ctx streams; with recv_host != NULL the root copies the gathered packs,
 * rank after rank, to the host and waits for it.  recv_host may be NULL on the other ranks. */
#define MXE_GATHER_COMPACT 0
#define MXE_GATHER_FULL    1
int  mxe_shard_plan(int n_elem, int n_ranks, int32_t* rank_of_elem, int32_t* local_index, int32_t* n_local);
int  mxe_comm_unique_id(char* out_id128);
int  mxe_comm_init(mxe_ctx* ctx, int n_ranks, int rank, const char* id128);
int  mxe_comm_init_local(mxe_ctx** ctxs, int n);
int  mxe_comm_destroy(mxe_ctx* ctx);
/* test plumbing for a one-GPU box (communicators of mxe_comm_init): with on != 0 the root's own pack goes through
   ncclGroupStart / ncclSend / ncclRecv (to itself) / ncclGroupEnd instead of a device copy, and mxe_comm_allreduce
   runs ncclAllReduce with the single rank -- the RCCL calls of the multi-GPU path execute on one device */
int  mxe_comm_set_loopback(mxe_ctx* ctx, int on);
int  mxe_gather(mxe_ctx* ctx, int root, int what, const int64_t* counts, double* recv_host);
/* sum (op = 0) or maximum (op = 1) of n <= 64 doubles over the ranks, result on every rank; with it the
 * ranks of separate processes agree on a timing or wait for each other (a barrier is a sum of zeros) */
int  mxe_comm_allreduce(mxe_ctx* ctx, double* inout_host, int n, int op);
int  mxe_gather_local(mxe_ctx** ctxs, int n, int root, int what, const int64_t* counts, double* recv_host);

/* ---- output map A = B H (PreblurA_of_H.f, functions.py:999-1001) ------- */
/* B: n_omega x n_omega row-major.  Applies to the device-resident H of the
 * last solve; result n_problem x n_omega to host. */
int  mxe_apply_output_map(mxe_ctx* ctx, const double* B, double* out_A);

/* ---- kernel matrix staging on the device ------------- */
/* TauKernel._fill_values (kernels.py:244-271), get_preblur (preblur.py:31-58),
 * PreblurKernel._fill_values (kernels.py:384-393: K' = K diag(delta) B), KernelSVD.svd
 * and reduce_singular_space (kernels.py:53-122) for a batch of n_b blur widths in one
 * go (a b-scan; preblur_b[ib] <= 0: the plain TauKernel).  tau: n_tau, omega / delta:
 * n_omega (delta = the trapezoid weights of the mesh, omega_meshes.py:54-62).
 * The decomposition is a pivoted-QR preconditioned one-sided Jacobi SVD in binary64
 * (one workgroup per blur width); singular values S >= threshold (ABSOLUTE, as in the
 * reference) are kept, at most ns_max (<= 128).  Outputs, host, row-major, per item ib:
 *   out_K [ib][n_tau][n_omega]   the (blurred) kernel matrix; may be NULL
 *   out_U [ib][n_tau][ns_max], out_S [ib][ns_max], out_V [ib][n_omega][ns_max]
 *         (columns >= out_ns[ib] are zero), out_ns [ib]
 *   out_info [ib][3]: rank kept by the QR stage, Jacobi sweeps, status (may be NULL); status: 0 ok,
 *         1 Jacobi sweeps exhausted or a matrix that is not finite, 2 more than ns_max values pass
 *         the threshold, 3 the QR stage kept its 128 rows and columns above its stop cut
 *         (eps x the largest column norm) were left: K has more than 128 significant directions
 *         and U, S, V are those of a rank-128 approximation, not the leading triplets of K
 *   out_ms: device time of the whole batch (may be NULL)
 * Returns MXE_ERR_LIMIT if more than ns_max singular values pass the threshold (status 2) or
 * the numerical rank of K is above 128 (status 3: only a host SVD decomposes such a matrix),
 * MXE_ERR_NUMERIC if the Jacobi sweeps did not converge, if K holds a NaN or an Inf or its
 * squared column norms overflow (status 1), or if a NaN came out in out_S. */
int  mxe_kernel_svd(int device, int n_tau, int n_omega, const double* tau,
                    const double* omega, const double* delta, double beta,
                    int n_b, const double* preblur_b, double threshold, int ns_max,
                    double* out_K, double* out_U, double* out_S, double* out_V,
                    int32_t* out_ns, int32_t* out_info, float* out_ms);

/* IOmegaKernel (reference kernels.py:283-346, K(i w_n, w) = 1 / (i w_n - w)) as the stacked real
 * matrix of 2 n_iw rows: rows 0..n_iw-1 = Re K = -w / (w_n^2 + w^2), rows n_iw..2 n_iw-1 = Im K
 * = -w_n / (w_n^2 + w^2).  iomega: the n_iw real Matsubara frequencies w_n.  Everything else --
 * preblur widths, threshold, ns_max, outputs (with n_tau -> 2 n_iw), error codes -- as
 * mxe_kernel_svd.  MXE_ERR_LIMIT also when 2 n_iw rows exceed the decomposition's LDS
 * (n_iw > ~3700). */
int  mxe_kernel_svd_iw(int device, int n_iw, int n_omega, const double* iomega,
                       const double* omega, const double* delta,
                       int n_b, const double* preblur_b, double threshold, int ns_max,
                       double* out_K, double* out_U, double* out_S, double* out_V,
                       int32_t* out_ns, int32_t* out_info, float* out_ms);

/* Bosonic kernels (no counterpart in the reference), for A(w) = Im chi(w) / (pi w):
 *   mxe_kernel_svd_boson     K(tau, w) = w e^{-tau w} / (1 - e^{-beta w}), K(tau, 0) = 1/beta, n_tau rows.
 *       symmetric != 0: K(tau, w) + K(tau, -w) = w (e^{-tau w} + e^{-(beta - tau) w}) / (1 - e^{-beta w}) on a mesh
 *       w >= 0 (2/beta at w = 0).  Filled without overflow on either half-axis, by a series below
 *       |beta w| = 1e-5, and with the rounding of the arguments of exp compensated: a few ulp everywhere.
 *   mxe_kernel_svd_boson_iw  K(i nu_n, w) = w / (w - i nu_n), 1 at w = nu_n = 0, as the stacked real matrix of
 *       2 n_inu rows: Re K = w^2 / (w^2 + nu_n^2) above Im K = w nu_n / (w^2 + nu_n^2) (the zero row Im K(i nu_0 = 0)
 *       is kept).  symmetric != 0: the real 2 w^2 / (w^2 + nu_n^2) of n_inu rows (2 at w = nu_n = 0).
 * inu: the n_inu real bosonic Matsubara frequencies nu_n.  A symmetric kernel on a mesh with a negative point is
 * MXE_ERR_ARG.  Everything else -- preblur widths, threshold, ns_max, outputs, error codes, the LDS limit on the
 * rows -- as mxe_kernel_svd / mxe_kernel_svd_iw. */
int  mxe_kernel_svd_boson(int device, int n_tau, int n_omega, const double* tau,
                          const double* omega, const double* delta, double beta, int symmetric,
                          int n_b, const double* preblur_b, double threshold, int ns_max,
                          double* out_K, double* out_U, double* out_S, double* out_V,
                          int32_t* out_ns, int32_t* out_info, float* out_ms);
int  mxe_kernel_svd_boson_iw(int device, int n_inu, int n_omega, const double* inu,
                             const double* omega, const double* delta, int symmetric,
                             int n_b, const double* preblur_b, double threshold, int ns_max,
                             double* out_K, double* out_U, double* out_S, double* out_V,
                             int32_t* out_ns, int32_t* out_info, float* out_ms);

/* DataKernel (reference kernels.py:183-207): the same preblur products and decomposition for a matrix the caller
 * filled.  K: n_rows x n_omega, host, row-major; it is transposed into the column-major working layout on the
 * device.  omega and delta serve the preblur (and are required).  Outputs as mxe_kernel_svd with n_tau -> n_rows;
 * MXE_ERR_LIMIT also when n_rows exceed the decomposition's LDS (n_rows > 7464).  A matrix with a NaN or an Inf is
 * refused before anything is launched (MXE_ERR_NUMERIC); a well-conditioned matrix of more than 128 rows and columns
 * is MXE_ERR_LIMIT (status 3 above). */
int  mxe_kernel_svd_data(int device, int n_rows, int n_omega, const double* K,
                         const double* omega, const double* delta,
                         int n_b, const double* preblur_b, double threshold, int ns_max,
                         double* out_K, double* out_U, double* out_S, double* out_V,
                         int32_t* out_ns, int32_t* out_info, float* out_ms);

/* LegendreKernel (no counterpart in the reference; its documentation anticipates it): G given as Legendre coefficients
 * in TRIQS's GfLegendre normalisation, G(tau) = sum_l sqrt(2l+1)/beta P_l(2 tau/beta - 1) G_l, G_l = int dw K(l, w) A(w),
 *     K(l, w) = -beta sqrt(2l+1) (-sgn w)^l i_l(beta |w| / 2) / (2 cosh(beta w / 2))
 * (i_l: modified spherical Bessel function of the first kind): K(0, w) = -tanh(beta w / 2) / w; at w = 0 the row l = 0
 * is -beta/2 and every other row 0.  Real, n_l rows.  l: the n_l orders as integer-valued doubles, in any order (a
 * subset is fine); beta is required.  Filled column by column from the ratios i_{k+1}/i_k (backward recurrence) and the
 * scaled e^{-a} i_0(a), a = beta |w| / 2: no positive exponent, no overflow for any beta w, small entries underflow
 * to 0; relative error below (8 + l) 2^-52.  MXE_ERR_ARG, before anything is launched: an order that is negative, not
 * integer-valued, above 4096 or there twice; beta <= 0 or not finite; beta |w| / 2 above 1e6 or a NaN in omega (the work of a column
 * grows like max(l_max, beta |w| / 2)).  Everything else as mxe_kernel_svd, with n_tau -> n_l. */
int  mxe_kernel_svd_legendre(int device, int n_l, int n_omega, const double* l,
                             const double* omega, const double* delta, double beta,
                             int n_b, const double* preblur_b, double threshold, int ns_max,
                             double* out_K, double* out_U, double* out_S, double* out_V,
                             int32_t* out_ns, int32_t* out_info, float* out_ms);

/* ---- Kramers-Kronig: G(w) from A(w) (get_G_w_from_A_w, maxent_util.py:43-132) ---- */
/* The broadened Cauchy / Hilbert sum, for every spectrum s and output point o:
 *     G[s][o] = sum_j A[s][j] * weight[j] / (w_out[o] - w[j] + i eta[j])
 * w, weight, eta: n_w; w_out: n_out; A: n_spec x n_w (real; a complex spectrum is two rows, the caller
 * recombines them); out_G: n_spec x n_out x 2 (interleaved complex), host, row-major.  get_G_w_from_A_w
 * passes weight = the half-width of each point's neighbourhood and eta = broadening_factor * weight.
 * The bits of one spectrum's G do not depend on n_spec or on its place in the batch: each sum runs over
 * j in a fixed order (slices of 256 values, added in slice order), with no atomics.  out_ms: device
 * time of the sum (may be NULL).  MXE_ERR_ARG also when n_spec * n_out or n_spec * n_w exceed 2^31 - 1,
 * MXE_ERR_LIMIT when n_out > 65535 * 256. */
int  mxe_kramers_kronig(int device, int n_w, const double* w, const double* weight, const double* eta,
                        int n_out, const double* w_out, int n_spec, const double* A,
                        double* out_G, float* out_ms);

/* ---- binned Monte Carlo data: the covariance eigenbasis of every set (no counterpart in the reference) ---- */
/* bins: n_sets x n_bins x n_data, host, C order: n_bins independent estimates of the n_data values of each set.  Per
 * set, all sets in one launch (one workgroup each): the mean over the bins (double-double sums in a fixed order: the
 * error does not grow with n_bins), X = (bins - mean) / sqrt(n_bins (n_bins - 1)), and the eigen-decomposition of the
 * covariance of the mean C = X^T X as the one-sided Jacobi SVD of X (pivoted Householder QR first when
 * n_bins > n_data; the n_bins rows of X themselves otherwise) -- C is never formed, eigenvalues are resolved down to
 * (eps s_max)^2 instead of eps lambda_max.
 *   threshold   absolute cut on the eigenvalues (cov_threshold).  Kept: lambda_k >= threshold and
 *               lambda_k > (max(n_bins, n_data) eps)^2 lambda_max (the noise floor of a null direction).
 *   out_mean    n_sets x n_data
 *   out_var     n_sets x n_data: the kept eigenvalues, ASCENDING like eigh, in the first out_rank[s] entries (0 behind)
 *   out_T       n_sets x n_data x n_data: row k = the eigenvector of out_var[k], its component of largest magnitude
 *               (lowest index on ties) positive (zero rows behind the kept ones)
 *   out_rank    n_sets: eigenvalues kept;  out_sweeps  n_sets: Jacobi sweeps taken
 * A set's output does not depend on the other sets of the launch and repeats bit for bit.  MXE_ERR_ARG: n_sets < 1,
 * n_bins < 2, n_data < 1 or > 512, n_bins * n_data > 2^31 - 1, a threshold that is negative or not finite, a NaN or an
 * Inf anywhere in bins (nothing is launched in any of these cases); MXE_ERR_NUMERIC: a set whose Jacobi iteration did
 * not converge in 60 sweeps, or whose squares overflow. */
int  mxe_bins_eig(int device, int n_sets, int n_bins, int n_data, const double* bins, double threshold,
                  double* out_mean, double* out_var, double* out_T, int32_t* out_rank, int32_t* out_sweeps);

/* ---- few bins: the shrinkage covariance of the mean (no counterpart in the reference) ---- */
/* mxe_bins_eig with the covariance of the mean replaced by the shrinkage estimator of Schaefer & Strimmer (2005), target
 * "diagonal, unequal variances":  C* = (1 - lambda) X^T X + lambda diag(c),  c_j = (X^T X)_jj  -- the variances are kept,
 * the correlations shrunk towards zero.  With x = bins - mean, s_j^2 = sum_k x_kj^2 / (m - 1), z = x / s (columns with
 * s_j = 0 left out), w_ij = sum_k z_ki z_kj / m, r_ij = m / (m - 1) w_ij (m = n_bins):
 *   lambda_raw = sum_{i != j} Var(r_ij) / sum_{i != j} r_ij^2,   Var(r_ij) = m / (m - 1)^3 sum_k (z_ki z_kj - w_ij)^2,
 *   lambda     = min(1, max(0, lambda_raw));  a zero denominator (one column, no correlation at all): lambda = 1 and
 *                lambda_raw = NaN (C* = C whatever lambda).
 * The two Gram matrices behind the sums run as v_mfma_f64_16x16x4_f64 tiles, every sum over the bins in index order inside
 * one wavefront, the tile sums added in tile order: no atomics.  C* is never formed: it is Y^T Y of
 * Y = [sqrt(1 - lambda) X ; sqrt(lambda) diag(sqrt(c))], which goes through the pivoted QR and the one-sided Jacobi SVD of
 * mxe_bins_eig; lambda is read from device memory, there is no host round trip between the kernels.
 *   bins, threshold, out_mean, out_var, out_T, out_rank, out_sweeps   as for mxe_bins_eig (out_mean: the same bits); the
 *               noise floor of the selection is ((n_bins + n_data) eps)^2 lambda_max, Y having n_bins + n_data rows.
 *   lambda_in   < 0: lambda is estimated per set;  0 <= lambda_in <= 1: it is that value for every set
 *   out_lambda      n_sets: the intensity used
 *   out_lambda_raw  n_sets: the unclipped estimate (NaN with a fixed lambda_in)
 *   out_diag    n_sets x n_data: c_j, the variances of the mean
 *   out_ms      device time of all kernels of the call (may be NULL)
 * A set's output does not depend on the other sets of the launch and repeats bit for bit.  MXE_ERR_ARG (nothing is
 * launched): what mxe_bins_eig refuses, lambda_in > 1 or NaN, n_bins < 4 with lambda_in < 0, a NULL out_lambda,
 * out_lambda_raw or out_diag;  MXE_ERR_NUMERIC as for mxe_bins_eig. */
int  mxe_bins_eig_shrunk(int device, int n_sets, int n_bins, int n_data, const double* bins, double threshold,
                         double lambda_in, double* out_mean, double* out_var, double* out_T, int32_t* out_rank,
                         int32_t* out_sweeps, double* out_lambda, double* out_lambda_raw, double* out_diag, float* out_ms);

/* ---- jackknife / bootstrap resampling of the bins (no counterpart in the reference) ---- */
/* The rotated data of every resample of every set, one launch (one workgroup per set).
 *   bins        n_sets x n_bins x n_data, as for mxe_bins_eig
 *   counts      n_res x n_bins: counts[r][b] >= 0 is the multiplicity of bin b in resample r, N_r = sum_b counts[r][b] > 0.
 *               One table for every set of the call: bins are joint measurements, all sets see the same resample.
 *   T, rank     n_sets x n_data x n_data and n_sets: out_T and out_rank of mxe_bins_eig
 *   out_mean    n_sets x n_data: the mean over the bins, formed by the code mxe_bins_eig runs -- the same bits
 *   out_dev     n_sets x n_res x n_data (may be NULL): out_dev[r][k] = sum_j T[k][j] D[r][j] with the deviation of the
 *               resampled mean D[r] = sum_b counts[r][b] (bins[b] - mean) / N_r.  A resampled mean is never formed as a
 *               sum of raw bins: the deviations are ~1/n_bins of the data and keep their own relative accuracy.
 *   out_G       n_sets x n_res x n_data: out_G[r][k] = sum_j T[k][j] mean[j] + out_dev[r][k], the data of resample r in
 *               the eigenbasis.  Rows k >= rank of out_G and out_dev are zeros.
 *   out_ms      device time of the kernel (may be NULL)
 * Both products run as v_mfma_f64_16x16x4_f64 tiles, every sum over all bins (all data points) in index order inside one
 * wavefront: no atomics, a set's output does not depend on the other sets and repeats bit for bit.  MXE_ERR_ARG (nothing
 * is launched): what mxe_bins_eig refuses in its sizes and bins, n_res < 1, n_res * n_bins or n_res * n_data > 2^31 - 1, a
 * negative count, a row of counts that sums to 0, a rank outside 0 .. n_data, a NaN or an Inf in bins or T. */
int  mxe_bins_resample(int device, int n_sets, int n_bins, int n_data, const double* bins,
                       int n_res, const int32_t* counts, const double* T, const int32_t* rank,
                       double* out_mean, double* out_G, double* out_dev, float* out_ms);

/* Mean, spread and functional covariances of groups of hidden images (the resamples of one matrix element each), one
 * launch (one workgroup per group).  Group g owns the rows group_offset[g] .. group_offset[g + 1] - 1 (group_offset[0] = 0,
 * not decreasing; a group may be empty), rows = group_offset[n_groups].
 *   H           rows x n_omega on the host, or NULL: row r is problem problem_index[r] (chain * n_alpha + alpha index; NULL:
 *               r itself) of the last launch on ctx, read where it lies on the device -- no H row crosses to the host
 *   scale       n_groups: the factor on the centred sums of squares ((n - 1) / n jackknife, 1 / (n - 1) bootstrap)
 *   F           n_f x n_omega weights on H (n_f may be 0)
 *   out_fval    rows x n_f: F H_row of every row
 *   out_used    n_groups: the rows of the group that are finite.  A failed alpha leaves H = NaN; such a row is left out of
 *               everything below.
 *   out_mean    n_groups x n_omega: the mean over the used rows, added in row order
 *   out_var     n_groups x n_omega: scale * sum (H_r - mean)^2, a second pass in row order
 *   out_fmean   n_groups x n_f, out_fcov n_groups x n_f x n_f: the same of the functional values (scaled centred covariance)
 *   out_ms      device time of the kernel (may be NULL)
 * Every output pointer may be NULL.  A group with fewer than two used rows has NaN in out_var and out_fcov (and in its means
 * when it has none); the other groups are not touched by it.  Fixed summation order, no atomics: a group's bits do not depend
 * on the other groups and repeat.  MXE_ERR_STATE: H == NULL and nothing was launched.  MXE_ERR_ARG: n_groups < 1, offsets
 * that decrease or do not start at 0, a problem_index outside the last launch, a scale or an F that is not finite, sizes
 * whose products exceed 2^31 - 1. */
int  mxe_resample_reduce(mxe_ctx* ctx, int n_groups, const int32_t* group_offset, const double* H,
                         const int32_t* problem_index, const double* scale, int n_f, const double* F,
                         double* out_mean, double* out_var, double* out_fval, double* out_fmean, double* out_fcov,
                         int32_t* out_used, float* out_ms);

/* Quantiles over the rows of groups of hidden images, per omega point: the percentile bands of a bootstrap.  The groups,
 * H and problem_index are those of mxe_resample_reduce (also the rows of the last launch with H == NULL, read where they
 * lie, and MXE_ERR_STATE).  Two launches on the stream of ctx: one wavefront per row (is it finite), then one workgroup
 * per (group, tile of 16 omega points), which sorts its tile in LDS by a bitonic network.
 *   q           n_q probabilities in [0, 1]
 *   out_used    n_groups: the rows of the group that are finite -- the rule and the numbers of mxe_resample_reduce; the
 *               others are left out
 *   out_q       n_groups x n_q x n_omega: per omega point the type-7 quantile (numpy's default, method='linear') of the
 *               n = out_used[g] values x_0 <= ... <= x_(n-1): h = (n - 1) q, lo = floor(h), t = h - lo, d = x_(lo+1) - x_lo,
 *               x_lo + t d for t < 1/2 and x_(lo+1) - (1 - t) d from there on, every operation rounded on its own: the
 *               order statistic itself where h is an integer (q = 0: the smallest, q = 1: the largest value).  NaN for a
 *               group without a used row.
 *   out_ms      device time of the two kernels (may be NULL)
 * out_q and out_used may be NULL.  A fixed sequence of compare-exchanges, no atomics: a group's bits do not depend on the
 * other groups and repeat.  MXE_ERR_ARG: n_groups < 1, n_q < 1, offsets that decrease or do not start at 0, a problem_index
 * outside the last launch, a q outside [0, 1] or NaN, sizes whose products exceed 2^31 - 1.  MXE_ERR_LIMIT: a group of more
 * than MXE_QUANTILE_MAX_ROWS rows (16 columns of them fill 128 KB of the 160 KB of LDS; the network needs a power of two).
 * Nothing is written in either case. */
#define MXE_QUANTILE_MAX_ROWS 1024
int  mxe_resample_quantiles(mxe_ctx* ctx, int n_groups, const int32_t* group_offset, const double* H,
                            const int32_t* problem_index, int n_q, const double* q,
                            double* out_q, int32_t* out_used, float* out_ms);

/* ---- parametric bootstrap: mock data (no counterpart in the reference) ---- */
/* Mock data drawn from continued spectra with the noise of the job, all sets in one launch (one workgroup per tile of 16
 * sets and chunk of mocks).  What is sampled is N(K H0, diag(err^2)) in the data space of the job, not a posterior.
 *   K           n_data x n_omega: the job's kernel (rotated / stacked / pre-blurred as the job has it), shared by the sets
 *   H0          n_sets x n_omega: the hidden image the mocks of a set are drawn from
 *   err         n_sets x n_data: the error bar of every data row (> 0, finite; also behind rank, where it is not used)
 *   T, rank     both NULL, or n_sets x n_data x n_data and n_sets: a rotation per set applied to K H0 (out_T and out_rank
 *               of mxe_bins_eig: rows >= rank are zero)
 *   seed, stream   stream[s] (n_sets) names the stream of set s of the generator of mxe_normals
 *   out_model   n_sets x n_data: m_s = K H0_s, or T_s K H0_s
 *   out_G       n_sets x n_mock x n_data: out_G[s][k][i] = m_s[i] + err[s][i] z, one fused multiply-add, z the standard
 *               normal number i of sample k of the stream (seed, stream[s]): what mxe_normals(seed, stream[s], n_mock,
 *               n_data) returns.  With T, rows i >= rank[s] of out_model and out_G are zeros.
 *   out_ms      device time of the kernel (may be NULL)
 * K H0 runs as v_mfma_f64_16x16x4_f64 tiles, every sum over all omega in index order inside one wavefront; T m one
 * wavefront per row.  No atomics: a set's output depends on nothing but its own H0, err, T, rank and stream and on K, it
 * is the same bits alone or in a batch, for any n_mock, and from call to call.  MXE_ERR_ARG (nothing is launched, nothing is
 * written): a size below 1, n_mock < 1, exactly one of T and rank NULL, a rank outside 0 .. n_data, a NaN or an Inf in K,
 * H0, err or T, an err <= 0, sizes whose products exceed 2^31 - 1.  MXE_ERR_NODEVICE: no device. */
int  mxe_mock_data(int device, int n_sets, int n_mock, int n_data, int n_omega,
                   const double* K, const double* H0, const double* err, const double* T, const int32_t* rank,
                   uint64_t seed, const uint64_t* stream, double* out_model, double* out_G, float* out_ms);

/* ---- k-fold cross-validation of alpha over the bins (no counterpart in the reference) ---- */
/* The out-of-sample chi2 of hidden images against held-out data, all groups in one launch (one workgroup per tile of 16
 * rows of a group), then one small launch that counts the finite rows.  The groups, H and problem_index are those of
 * mxe_resample_reduce (also the rows of the last launch with H == NULL, read where they lie, and MXE_ERR_STATE).  A group is
 * one (matrix element, fold); its rows are the alphas of that fold's training scan.
 *   n_data, n_omega   the sizes of K; with H == NULL n_omega must be that of ctx
 *   K           n_data x n_omega: the job's kernel as mxe_mock_data takes it (not rotated by a covariance; stacked or
 *               pre-blurred as the job has it), shared by the groups
 *   T, rank     both NULL (the identity, n_data), or n_groups x n_data x n_data and n_groups: out_T and out_rank of
 *               mxe_bins_eig; rows k >= rank do not count
 *   Gval        n_groups x n_data: the validation data in the rotated basis (a row of out_G of mxe_bins_resample)
 *   w           n_groups x n_data: weights >= 0, finite (the inverse variance of the validation data)
 *   out_z       rows x n_data: out_z[r][k] = sqrt(w[g][k]) (sum_j T[g][k][j] (sum_i K[j][i] H[r][i]) - Gval[g][k]) for
 *               k < rank[g], 0 behind it.  May be NULL.
 *   out_score   rows: sum_k out_z[r][k]^2
 *   out_used    n_groups: the rows of the group that are finite (may be NULL).  A failed alpha leaves H = NaN; such a row
 *               has NaN in out_score and in all of its out_z and does not touch its neighbours.
 *   out_ms      device time of the two kernels (may be NULL)
 * K H runs as v_mfma_f64_16x16x4_f64 tiles (16 data rows x 16 H rows, one wavefront per tile, the omega sum in index order
 * inside one chain, zeros beyond the edges), T (K H) as the same tiles over the n_data sum in index order; the sum of
 * squares is taken by lane l over k = l, l + 64, ... and a butterfly over the 64 lanes, an order that depends on n_data
 * alone.  No atomics: a row's bits do not depend on the other rows of its group, on the other groups or on H being on the
 * host or on the device, and repeat.  MXE_ERR_ARG (nothing is launched, nothing is written): a size below 1, offsets that
 * decrease or do not start at 0, a problem_index outside the last launch, exactly one of T and rank NULL, a rank outside
 * 0 .. n_data, a w that is negative or not finite, a NaN or an Inf in K, T or Gval, sizes whose products exceed 2^31 - 1,
 * with H == NULL an n_omega that is not the launch's. */
int  mxe_cv_score(mxe_ctx* ctx, int n_groups, const int32_t* group_offset, const double* H,
                  const int32_t* problem_index, int n_data, int n_omega, const double* K,
                  const double* T, const int32_t* rank, const double* Gval, const double* w,
                  double* out_score, double* out_z, int32_t* out_used, float* out_ms);

/* ---- default-model scans: evidence and model averages (no counterpart in the reference) ---- */
/* The same data continued under a family of default models: the alpha-integrated evidence of every scan, the row it stands
 * for, and per group of scans (the models of one matrix element) the evidence weights of the models, the model-averaged
 * hidden image and the spread between the models.  Two launches on the stream of ctx: one workgroup per scan, then one
 * per group.  Group g owns the scans group_offset[g] .. group_offset[g + 1] - 1 (group_offset[0] = 0, not decreasing; a
 * group may be empty), n_scan = group_offset[n_groups].
 *   H           n_scan x n_alpha x n_omega on the host, or NULL: scan s is chain chain_index[s] (NULL: s) of the last
 *               launch on ctx, its rows read where they lie on the device -- no H row crosses to the host
 *   logp        n_scan x n_alpha: log p(alpha, D | G) (NormalLogProbability.from_logdet).  NaN and +-inf are data: an
 *               alpha is GOOD when its logp is finite and, in row_mode 0, its H row is finite (a failed alpha leaves NaN)
 *   log_quad    n_alpha: log |get_delta(alpha~)|, the measure of the evidence integral
 *   log_mix     n_alpha: the measure of the mixture over alpha: zeros (BryanAnalyzer) or log_quad (average_by_integration)
 *   log_prior   n_scan: log P(model), NULL: equal.  -inf switches a model off
 *   row_mode    0: the Bryan mixture over alpha, 1: the row at the largest logp (classic), 2: the row pick[s]
 *   F           n_f x n_omega weights on H (n_f may be 0)
 * Per scan:
 *   out_logZ    m + log sum_good exp(logp[k] + log_quad[k] - m), m the largest exponent, the terms added in k order
 *   out_kmax    the first index of the largest logp among the good alphas, -1 when there is none;  out_ngood  their number
 *   out_walpha  n_scan x n_alpha: exp(logp[k] + log_mix[k] - m') / their sum in k order over the good alphas, 0 elsewhere
 *   out_row     n_scan x n_omega: sum_k walpha[k] H[k] in k order (mode 0), H[kmax] (mode 1), H[pick[s]] (mode 2)
 *   out_fval    n_scan x n_f: F row (lanes over omega, butterfly sum)
 *               A scan with no good alpha, a chosen row that is not finite or pick[s] < 0 is left out of its group: its
 *               out_logZ is -inf, its out_row and out_fval NaN, its out_wmodel 0.
 * Per group:
 *   out_wmodel  n_scan: u_s = exp(logZ_s + log_prior_s - max) / their sum in s order over the usable scans of the group
 *               (NaN when every usable scan of the group is switched off)
 *   out_mean    n_groups x n_omega: sum_s u_s row_s in s order
 *   out_between n_groups x n_omega: sum_s u_s (row_s - mean)^2, a second pass on the explicit difference
 *   out_fmean   n_groups x n_f, out_fcov n_groups x n_f x n_f: the same sums of the functional values
 *   out_used    n_groups: the usable scans.  A group with none has NaN means.
 *   out_ms      device time of the two kernels (may be NULL)
 * Every output pointer may be NULL.  Fixed summation order, no atomics: a scan's bits depend on nothing but its own rows,
 * a group's on nothing but its own scans, and both repeat.  MXE_ERR_STATE: H == NULL and nothing was launched.
 * MXE_ERR_ARG (nothing is launched, no output is touched): n_groups < 1, n_alpha < 1, offsets that decrease or do not
 * start at 0, with H == NULL a chain_index outside the last launch or an n_alpha that is not the launch's, a row_mode
 * outside 0 .. 2, row_mode 2 without pick, a pick >= n_alpha, a log_quad, log_mix or F that is not finite, a log_prior that
 * is NaN or +inf, sizes whose products exceed 2^31 - 1. */
int  mxe_evidence_reduce(mxe_ctx* ctx, int n_groups, const int32_t* group_offset, int n_alpha, const double* H,
                         const int32_t* chain_index, const double* logp, const double* log_quad, const double* log_mix,
                         const double* log_prior, int row_mode, const int32_t* pick, int n_f, const double* F,
                         double* out_logZ, int32_t* out_kmax, int32_t* out_ngood, double* out_walpha,
                         double* out_row, double* out_fval, double* out_wmodel, double* out_mean, double* out_between,
                         double* out_fmean, double* out_fcov, int32_t* out_used, float* out_ms);

/* ---- bin checks: blocking ladder and normality of the block means (no counterpart in the reference) ---- */
/* May the bins be used as they are?  The covariance of the mean of mxe_bins_eig assumes bins that are uncorrelated and
 * normally distributed.  Per set, all sets in one launch (one workgroup each), per column c and level k = 0 .. L - 1,
 * L = floor(log2 n_bins): the bins are cut into n_k = floor(n_bins / 2^k) blocks of 2^k successive bins (a trailing
 * remainder is dropped at that level only; every n_k >= 2), B_q is the mean of block q, Bbar their mean, and
 * mu_p = (1 / n_k) sum_q (B_q - Bbar)^p, p = 2, 3, 4 (two passes: Bbar first, then powers of the explicit difference).
 *   bins        n_sets x n_bins x n_data, as for mxe_bins_eig.  The bin index is Monte Carlo time: here, unlike everywhere
 *               else, the order of the bins matters.
 *   T, rank     both NULL: the columns are the data values, y[b][c] = bins[b][c] - mean[c].  Both given (n_sets x n_data x
 *               n_data and n_sets: out_T and out_rank of mxe_bins_eig): the columns are the eigen-directions chi^2 sums,
 *               y[b][k] = sum_j T[k][j] (bins[b][j] - mean[j]) for k < rank (v_mfma_f64_16x16x4_f64 tiles, every inner
 *               product in index order), zeros for k >= rank.
 *   out_mean    n_sets x n_data: the mean over the bins, formed by the code mxe_bins_eig runs -- the same bits
 *   out_err2    n_sets x L x n_data: mu_2 / (n_k - 1), the squared error of the mean as estimated at block length 2^k.
 *               Level 0 is C_cc in the data basis and the eigenvalue out_var[c] of mxe_bins_eig in the eigen basis; the
 *               ratio to level 0 estimates 2 tau_int and levels off once the blocks are uncorrelated.
 *   out_skew    n_sets x L x n_data: mu_3 / mu_2^(3/2);   out_kurt: mu_4 / mu_2^2 - 3 (both 0 for normal block means)
 *               Where mu_2 == 0 -- a constant column, a column k >= rank -- out_err2 is 0 and both are NaN.
 *   out_levels  one value: L
 *   out_ms      device time of the kernel (may be NULL)
 * The block sums of level k + 1 are sums of two block sums of level k (a halving tree over a work array of the set in
 * device memory); every sum over blocks runs as 16 chunks in chunk order: no atomics, a set's output does not depend on the
 * other sets and repeats bit for bit.  MXE_ERR_ARG (nothing is launched): what mxe_bins_eig refuses in its sizes and bins,
 * exactly one of T and rank NULL, a rank outside 0 .. n_data, a NaN or an Inf in bins or T. */
int  mxe_bins_check(int device, int n_sets, int n_bins, int n_data, const double* bins,
                    const double* T, const int32_t* rank,
                    double* out_mean, double* out_err2, double* out_skew, double* out_kurt,
                    int32_t* out_levels, float* out_ms);

/* ---- positivity of a matrix-valued A: batched Hermitian eigenproblems (no counterpart in the reference) ---- */
/* A physical spectral function matrix is Hermitian and positive semi-definite at every frequency; one continued element by
 * element usually is not (the reference's guide says so and offers no check).  Per matrix, all matrices in one launch: the
 * eigen-decomposition of Herm(A) = (A + A^H) / 2, formed on the device, by a parallel two-sided cyclic Jacobi iteration
 * (round-robin ordering, A and V in the LDS; one wavefront per matrix and four matrices per workgroup for m <= 16, one
 * workgroup per matrix above), its projection onto the cone of matrices with eigenvalues >= floor, and what that costs.
 *   A           n_mat x m x m row-major; is_complex = 1: interleaved (re, im).  It need not be Hermitian.
 *   floor       eigenvalues below it are raised to it in out_proj (0: the positive semi-definite cone)
 *   out_lambda  n_mat x m: the eigenvalues, ascending (by index on ties)
 *   out_vec     n_mat x m x m (complex: x 2): column k is the eigenvector of out_lambda[k], of unit norm, its component of
 *               largest magnitude (lowest index on ties) real and positive
 *   out_proj    n_mat x m x m (x 2): V max(Lambda, floor) V^H, the nearest such matrix in the Frobenius norm; the upper
 *               triangle is computed, the lower is its conjugate and the diagonal is real: exactly Hermitian
 *   out_neg     n_mat: sum over lambda < floor of (floor - lambda)
 *   out_dist    n_mat: || out_proj - Herm(A) ||_F = sqrt(sum over the same of (floor - lambda)^2)
 *   out_pair    n_mat: max over i < j of |h_ij| - sqrt(max(h_ii, 0) max(h_jj, 0)), h = Herm(A): positive where the
 *               reference's necessary condition |A_ij| <= sqrt(A_ii A_jj) fails; 0 for m = 1
 *   out_asym    n_mat: || A - A^H ||_F of the input
 *   out_info    n_mat: the sweeps that rotated (>= 0; 0: the matrix was diagonal), -1: the matrix holds a NaN or an Inf,
 *               -2: MXE_HERMEIG_MAX_SWEEPS sweeps did not end the iteration
 *   out_ms      device time of the kernel (may be NULL)
 * Every output pointer may be NULL.  A pair (p, q) is rotated when |a_pq| > 2^-53 || Herm(A) ||_F / m -- a threshold that does
 * not look at the diagonal, which may vanish --, and a sweep without a rotation ends the solve.  A matrix with a NaN or an
 * Inf gets info -1 and NaN in all its outputs; the other matrices of the call are not touched by it.  No atomics: a
 * matrix's bits depend on nothing but the matrix, they are the same alone or in a batch, and from call to call.
 * MXE_ERR_ARG (nothing is launched, nothing is written): n_mat < 1, m < 1, A == NULL, is_complex outside {0, 1}, a floor
 * that is not finite, sizes whose products exceed 2^31 - 1.  MXE_ERR_LIMIT (likewise): m > MXE_HERMEIG_MAX_M -- two padded
 * 64 x 64 complex matrices fill 133 KB of the 160 KB of LDS.  MXE_ERR_NODEVICE: no device. */
#define MXE_HERMEIG_MAX_M      64
#define MXE_HERMEIG_MAX_SWEEPS 30
int  mxe_hermitian_eig(int device, int n_mat, int m, int is_complex, const double* A, double floor,
                       double* out_lambda, double* out_vec, double* out_proj, double* out_neg, double* out_dist,
                       double* out_pair, double* out_asym, int32_t* out_info, float* out_ms);

/* Whole-matrix continuation (no counterpart in the reference: its guide announces a FullMatrixMaxEnt, its FAQ says it is
 * not implemented).  The unknown is the Hermitian matrix H_i = D_i exp(Gamma_i) at every frequency, Gamma_i = sum_p
 * (V' u)_ip E_p with E_p an orthonormal basis of the Hermitian m x m matrices (P = m (m + 1) / 2 of them for real symmetric
 * data, m^2 with is_complex: the diagonal units, (e_ab + e_ba) / sqrt 2 for a < b in row order, then i (e_ab - e_ba) /
 * sqrt 2); x_p = Tr(E_p X) are the coordinates of a Hermitian X.  Minimised is Q = chi2 / 2 - alpha S with
 * chi2 = sum_p | c o V'^T H_p - g^_p |^2 + c_perp and the matrix entropy S = sum_i Tr[H_i - D_i - H_i log(H_i / D_i)]:
 * H is Hermitian and positive semi-definite at every frequency and alpha.  n_prob problems share V', c, D and the alpha
 * mesh; one workgroup per problem walks the mesh in order, warm-started, by a damped Newton iteration on
 * F = alpha u + c o (c o V'^T H_p - g^_p): a step is taken only if Q does not rise (a Q that is not finite counts as a
 * rise), a step that makes Q rise is halved up to three times before the damping grows, the damping grows and shrinks
 * geometrically, an alpha ends converged when a full undamped step was taken whose first-order change of H,
 * || L V' delta ||_F / || H ||_F, is below tol_h, and unconverged after maxiter trial points.
 *   V           n_omega x n_s row-major, the (whitened) right singular basis;  c  n_s, > 0: S / sigma
 *   D           n_omega, > 0: the default model (times delta omega), the same for every diagonal element
 *   alpha       n_alpha, > 0, already scaled by the number of data of ONE matrix element
 *   ghat        n_prob x P x n_s: U^T G_p / sigma of the coordinates G_p of the data;  cperp  n_prob: chi2 outside U
 *   u0          n_prob x P x n_s: the start of the first alpha (NULL: zeros, H = D 1)
 *   out_u       n_prob x n_alpha x P x n_s
 *   out_H       n_prob x n_alpha x (is_complex ? 2 : 1) x m x m x n_omega: the real part and (is_complex) the imaginary part
 *               of every matrix element; the upper triangle is computed, the lower is its conjugate: exactly Hermitian
 *   out_chi2, out_S, out_Q   n_prob x n_alpha: one cost for the whole matrix
 *   out_niter   n_prob x n_alpha: the trial points evaluated;  out_conv  n_prob x n_alpha: 1 converged, 0 not
 *   out_ms      device time of the kernel (may be NULL)
 * No atomics, fixed summation order: the bits of a problem do not depend on the other problems of the call.
 * MXE_ERR_ARG (nothing is launched, nothing is written): a size < 1, maxiter < 0, tol_h <= 0, a NULL among the arrays
 * other than u0 and out_ms, a NaN or an Inf in an input, a c, D or alpha that is not positive, sizes whose products exceed
 * 2^31 - 1.  MXE_ERR_LIMIT (likewise): m > MXE_FULLMATRIX_MAX_M or n_s > MXE_FULLMATRIX_MAX_NS (the Newton matrix has order
 * P n_s <= 1024: its panel of 16 columns fills 139 KB of the 160 KB of LDS); cut the singular space.
 * MXE_ERR_NODEVICE: no device. */
#define MXE_FULLMATRIX_MAX_M   4
#define MXE_FULLMATRIX_MAX_NS  64
int  mxe_fullmatrix_solve(int device, int n_prob, int m, int is_complex, int n_omega, int n_s, int n_alpha,
                          const double* V, const double* c, const double* D, const double* alpha,
                          const double* ghat, const double* cperp, const double* u0, int maxiter, double tol_h,
                          double* out_u, double* out_H, double* out_chi2, double* out_S, double* out_Q,
                          int32_t* out_niter, int32_t* out_conv, float* out_ms);

/* The same continuation with one error bar per matrix element: sigma_ab(t) = sigma_ba(t) is the standard deviation of the
 * real and of the imaginary part of the symmetrised G_ab(t).  In the coordinates of E_p the misfit stays a sum over the
 * components, chi2 = sum_p sum_t (g_p - (K h_p))_t^2 / sigma_p(t)^2 with sigma_p = sigma_aa for a diagonal unit and
 * sigma_ab for both components of a pair a < b, and the diagonal metric c, shared by all components, becomes a dense
 * n_s x n_s factor per component: diag(1 / sigma_p) U S = Q^_p R_p (thin, any sign convention), A_p = R_p^T R_p,
 *   rho_p = R_p V^T H_p - g^_p    chi2 = sum_p |rho_p|^2 + c_perp    F_p = alpha u_p + R_p^T rho_p
 *   J = alpha I + blockdiag_p(A_p) W
 * V is not rotated and u stays in its basis.  The iteration, the outputs and their layouts are those of
 * mxe_fullmatrix_solve; block row p of J - alpha I is formed as A_p W[(p, .), :] by a phase of its own, in a fixed order.
 *   V           n_omega x n_s row-major, the right singular basis itself
 *   R, A        P x n_s x n_s row-major, shared by the problems: R_p and A_p = R_p^T R_p (finite; no sign is asked for)
 *   ghat        n_prob x P x n_s: Q^_p^T (G_p / sigma_p);  cperp  n_prob: sum_p (|G_p / sigma_p|^2 - |ghat_p|^2), >= 0
 * Everything else, the return codes and the limits as for mxe_fullmatrix_solve (with R, A in the place of c). */
int  mxe_fullmatrix_solve_metric(int device, int n_prob, int m, int is_complex, int n_omega, int n_s, int n_alpha,
                                 const double* V, const double* R, const double* A, const double* D, const double* alpha,
                                 const double* ghat, const double* cperp, const double* u0, int maxiter, double tol_h,
                                 double* out_u, double* out_H, double* out_chi2, double* out_S, double* out_Q,
                                 int32_t* out_niter, int32_t* out_conv, float* out_ms);

/* Posterior (Gaussian) variances of the whole-matrix continuation with one error for all matrix elements, around the u of
 * mxe_fullmatrix_solve (the same V', c, D, scaled alpha and basis E_p).  In the coordinates h_p,i = Tr(E_p H_i) the matrix
 * entropy has the Hessian -L^-1, L_i (P x P) the Frechet derivative of D exp at Gamma_i, and the covariance of h is
 *   Gamma = (alpha L^-1 + (V' c^2 V'^T) (x) 1_P)^-1,   B = alpha I + c W c = L_B L_B^T of order d = P n_s (W: the solver's Gram matrix)
 *   var(x)     = (1 / alpha) [ sum_i f_i^T L_i f_i - |L_B^-1 y|^2 ],  y_(p,s) = c_s sum_i V'_is (L_i f_i)_p,  x = sum_p,i f_p,i h_p,i
 *   var(h_p,i) = (1 / alpha) [ L_i,pp - |L_B^-1 y|^2 ],               y_(q,s) = c_s V'_is L_i,qp
 * formed as written (differences of sums of non-negative terms; a negative difference is returned as 0, a NaN stays one).
 * One workgroup per job, a job being one (u, alpha) pair; jobs share V', c, D and F.  For m = 1 this is mxe_posterior_var
 * with w = H.
 *   alpha       n_job, > 0;   u  n_job x P x n_s
 *   F           n_f x P x n_omega: the coordinates f_p,i = Tr(E_p F_i) of Hermitian weights on H (NULL with n_f == 0)
 *   want_diag   1: also the variance of every coordinate
 *   out_value, out_var, out_prior   n_job x n_f: x, var(x), and the variance sum_i f_i^T L_i f_i / alpha the entropy alone leaves
 *   out_diag_var, out_diag_prior, out_h   n_job x P x n_omega (want_diag): var(h_p,i), L_i,pp / alpha, h_p,i
 *   out_ms      device time of the kernel (may be NULL)
 * A job whose u or H is not finite, or whose B is not positive definite in binary64, gets NaN in all its outputs; the other
 * jobs are not touched.  No atomics, fixed summation order: the bits of a job do not depend on the batch, on n_f or on a
 * functional's place in F.  The device scratch is one slice per workgroup; the workgroups take the jobs in strides over as
 * many slices as fit below MXE_FULLMATRIX_POSTVAR_SCRATCH_BYTES (one at least); results do not depend on their number.
 * MXE_ERR_ARG (nothing is launched): a size < 1, n_f < 0, nothing asked for (n_f == 0 without want_diag), a NULL among the
 * arrays that are needed, a NaN or an Inf in V, c, D, alpha or F, a c, D or alpha that is not positive, sizes whose products
 * exceed 2^31 - 1.  MXE_ERR_LIMIT: m > MXE_FULLMATRIX_MAX_M, n_s > MXE_FULLMATRIX_MAX_NS, or more than 160 KB of LDS (a block
 * of 16 right-hand sides of order d <= 1024 fills 141 KB).  MXE_ERR_NODEVICE: no device. */
#define MXE_FULLMATRIX_POSTVAR_SCRATCH_BYTES  (1ull << 30)
int  mxe_fullmatrix_posterior_var(int device, int n_job, int m, int is_complex, int n_omega, int n_s, int n_f,
                                  const double* V, const double* c, const double* D, const double* alpha,
                                  const double* u, const double* F, int want_diag,
                                  double* out_value, double* out_var, double* out_prior,
                                  double* out_diag_var, double* out_diag_prior, double* out_h, float* out_ms);

/* The evidence of alpha of the whole-matrix continuation with one error for all matrix elements, around the u of
 * mxe_fullmatrix_solve (the same V', c, D, scaled alpha and basis E_p as mxe_fullmatrix_posterior_var).  With
 * B = alpha I + c W c = L_B L_B^T of order d = P n_s, l_jj the diagonal of L_B:
 *   out_logdet  n_job: log det(I_d + c W c / alpha) = sum_j log(l_jj^2 / alpha), summed pivot by pivot (no term is negative
 *               but for the rounding of a pivot; nothing cancels at large alpha);
 *               log p(alpha | G) = -1/2 logdet - Q - log alpha, as from mxe_logdet for a scalar problem
 *   want_ngood  1: also out_ngood
 *   out_ngood   n_job (want_ngood; may be NULL otherwise): the number of good data N_g = tr(c W c B^-1)
 *               = d - alpha |L_B^-1|_F^2, the identity through the forward substitution of the variance kernel (a negative
 *               difference is returned as 0, a NaN stays one)
 *   out_ms      device time of the kernel (may be NULL)
 * One workgroup per job, a job being one (u, alpha) pair.  A job whose u or H is not finite, or whose B is not positive
 * definite in binary64, gets NaN in its outputs; the other jobs are not touched.  No atomics, fixed summation order: the bits
 * of a job do not depend on the batch or on the number of scratch slices, those of out_logdet not on want_ngood.  The
 * scratch is cut as for mxe_fullmatrix_posterior_var, below the same MXE_FULLMATRIX_POSTVAR_SCRATCH_BYTES (the environment
 * variable MXE_FULLMATRIX_LOGDET_SLICES = n caps the number of slices further; a test aid).
 * MXE_ERR_ARG (nothing is launched): a size < 1, want_ngood neither 0 nor 1, a NULL among the arrays that are needed, a NaN or
 * an Inf in V, c, D or alpha, a c, D or alpha that is not positive, sizes whose products exceed 2^31 - 1.  MXE_ERR_LIMIT:
 * m > MXE_FULLMATRIX_MAX_M, n_s > MXE_FULLMATRIX_MAX_NS, or more than 160 KB of LDS.  MXE_ERR_NODEVICE: no device. */
int  mxe_fullmatrix_logdet(int device, int n_job, int m, int is_complex, int n_omega, int n_s,
                           const double* V, const double* c, const double* D, const double* alpha, const double* u,
                           int want_ngood, double* out_logdet, double* out_ngood, float* out_ms);

#ifdef __cplusplus
}
#endif
#endif /* MAXENT_HIP_H */
