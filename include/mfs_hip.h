/*
 * mfs_hip.h -- C ABI of libmfs_hip.so: the MI355X (gfx950) moment-filter hot path of zgbkdlm/mfs.
 *
 * This is the drop-in boundary.  The reference is pure Python/JAX and has no FFI of its own; the entry points
 * below are what a ctypes binding for its filter loop binds (INTEGRATION.md shows the stub).  Each entry point
 * names the reference interface it replaces (paths relative to the reference repository root).
 *
 * Conventions
 *   - plain C, plain pointers and sizes; all floating point is IEEE fp64 (the reference sets jax_enable_x64).
 *   - every function returns MFS_OK (0) or a negative MFS_E* code; mfs_last_error() gives the message of the
 *     calling thread's last failure.  Numerical failure is NEVER an error code: a non-positive-definite moment
 *     matrix poisons that replicate with NaN in-band, exactly as the reference's XLA Cholesky does, and the first
 *     poisoned step is reported in out_first_nan.
 *   - "host" entry points take host pointers and stage through device buffers owned by the library;
 *     "_dev" entry points take device pointers (inputs already resident in HBM) and only enqueue work on `stream`.
 *   - batch axis: B independent replicates (Monte-Carlo keys / parameter points; the reference runs these as
 *     separate calls, dardel/benes_bernoulli/mf.py:70-92).  Layouts are row-major with the replicate axis first.
 */
#ifndef MFS_HIP_H
#define MFS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MFS_ABI_VERSION 2   /* 2: mfs_model_nd carries likelihood factors, ny and per-replicate tables; staging pool */

/* return codes */
#define MFS_OK 0
#define MFS_EINVAL (-1)   /* bad argument (mirrors the reference's only raise, multi_dims/filtering.py:159-161) */
#define MFS_EUNSUPPORTED (-2) /* N / degree / model outside what the kernels are compiled for */
#define MFS_EHIP (-3)     /* a HIP runtime call failed (message in mfs_last_error) */
#define MFS_ENOMEM (-4)
#define MFS_ERCCL (-5)

/* moment representation, mfs/one_dim/filtering.py:32 / :92 / :164 */
#define MFS_MODE_RAW 0
#define MFS_MODE_CENTRAL 1
#define MFS_MODE_SCALED 2
/* OR-ed into `mode`: the moment vectors carry 2N + 1 entries instead of 2N.  The reference warns about an odd count and
 * proceeds (mfs/one_dim/filtering.py:65-66): N = floor(M / 2) (mfs/one_dim/quadtures.py:122), every rule is built from
 * the first 2N entries, and the last entry of each output row is the N-node rule's value of the order-2N moment.  m0 and
 * out_moments then have rows of 2N + 1 doubles; the run uses the dense kernel in one launch. */
#define MFS_MODE_ODD_TAIL 0x100

/* how the transition moments E[(X_k - c)^n | X_{k-1} = x] are produced on the device */
#define MFS_TRANS_OPERATOR 0 /* TME without closure: sum_{k<=K} Q_k(u(x)) n!/(n-k)! (x - c)^(n-k);
                                replaces sde_cond_moments_tme, mfs/one_dim/moments.py:141-179 */
#define MFS_TRANS_GAUSSIAN 1 /* normal closure from (mu(x), var(x)): TME-normal (:182-219), Euler (:222-255), or an
                                exact linear-Gaussian step (dardel/convergence/convergence_mf.py:86-107) */

/* the variable the coefficient tables are polynomials in */
#define MFS_U_IDENTITY 0 /* u = x        (polynomial drift, e.g. well_poisson, OU) */
#define MFS_U_TANH 1     /* u = tanh(x)  (benes_bernoulli, mfs/one_dim/ss_models.py:37-38) */

/* measurement likelihood p(y | x) */
#define MFS_LIK_BERNOULLI_LOGISTIC 0 /* p = 1/(1+exp(-(l0 + l1 x + l2 x^2 + l3 x^3))), pmf(y; p), y in {0,1}
                                        (ss_models.py:43-47; multi_dims/ss_models.py:63-67 on x_0) */
#define MFS_LIK_POISSON_SOFTPLUS 1   /* rate = log(1 + exp(l0 x)), Poisson pmf(y; rate) (ss_models.py:80-84) */
#define MFS_LIK_GAUSSIAN 2           /* y ~ N(l0 x + l1, l2) (l2 = variance) (convergence_mf.py:58-61) */
#define MFS_LIK_BEARING_GAUSSIAN 3   /* N-D only, a factor of BOTH state components (fac_component = 2): y ~ N(atan2(x_1, x_0), l0),
                                        l0 = variance (examples/2d_bearing_only.ipynb cell 7); not with TME-order-3 operator tables */

#define MFS_MAX_N 32       /* quadrature order N (2N moments) */
#define MFS_MAX_TERMS 8    /* K <= 2 * tme_order */
#define MFS_MAX_DEGREE 15  /* polynomial degree of a coefficient row */
#define MFS_MAX_LIK 4

/*
 * 1-D model descriptor.  Replaces the Python callables the reference's filters take
 * (state_cond_*_moments, state_cond_mean[_var], measurement_cond_pdf; mfs/one_dim/filtering.py:32-36,92-98,164-172):
 * callables cannot cross a C ABI, so the host side reduces a model to coefficient tables (mfs_amd/tme_poly.py).
 *
 * coef is [n_rows][degree + 1] (ascending powers of u), or [B][n_rows][degree + 1] when coef_batched:
 *   MFS_TRANS_OPERATOR: rows 0..K-1 = Q_1..Q_K (Q_0 = 1 is implicit); row K = conditional variance polynomial
 *                       (tme.mean_and_cov, used by the scaled mode only).  Conditional mean = x + Q_1(u).
 *                       n_rows = K + 1.
 *   MFS_TRANS_GAUSSIAN: row 0 = P_m, row 1 = P_v with mu(x) = mean_x_coef * x + P_m(u), var(x) = P_v(u).
 *                       n_rows = 2.
 */
typedef struct mfs_model_1d {
    int32_t trans_kind;   /* MFS_TRANS_* */
    int32_t umap;         /* MFS_U_* */
    int32_t n_terms;      /* K (MFS_TRANS_OPERATOR); 0 otherwise */
    int32_t degree;       /* J <= MFS_MAX_DEGREE */
    int32_t n_rows;       /* rows per table */
    int32_t coef_batched; /* 0: one table for all replicates; 1: one per replicate */
    int32_t lik_kind;     /* MFS_LIK_* */
    int32_t n_lik;        /* <= MFS_MAX_LIK */
    int32_t lik_batched;  /* 0 / 1 */
    int32_t reserved;
    double mean_x_coef;   /* MFS_TRANS_GAUSSIAN only */
    const double* coef;
    const double* lik;    /* [n_lik] or [B][n_lik] */
} mfs_model_1d;

/* ---- library / device management --------------------------------------------------------------------------- */
int mfs_version(void);                 /* MFS_ABI_VERSION */
const char* mfs_last_error(void);      /* thread-local message of the last failing call ("" if none) */
int mfs_device_count(int* count);
int mfs_set_device(int device);
int mfs_device_synchronize(void);
int mfs_device_name(int device, char* buf, int buflen);

/* device memory and streams for callers that keep data resident (bench harness, sharded driver) */
int mfs_malloc(void** dptr, uint64_t bytes);
int mfs_free(void* dptr);
int mfs_memcpy_h2d(void* dst, const void* src, uint64_t bytes, void* stream);
int mfs_memcpy_d2h(void* dst, const void* src, uint64_t bytes, void* stream);
int mfs_memset(void* dst, int value, uint64_t bytes, void* stream);
int mfs_stream_create(void** stream);
int mfs_stream_destroy(void* stream);
int mfs_stream_synchronize(void* stream);
/*
 * The library's staging pool (SURVEY.md section 8b "Ownership": the caller owns what it passes; the library stages
 * through its own device buffers and pinned pool, reused across calls).  The host-pointer entry points below borrow
 * their device buffers, streams and events from per-device caches, so a steady-state call makes no hipMalloc / hipFree.
 * mfs_host_alloc hands out page-locked host memory from the same pool: results written into it (e.g. out_moments)
 * travel at the PCIe rate instead of the pageable-copy rate, and a block given back with mfs_host_free is reused by
 * the next request of similar size.  mfs_pool_trim returns every unused block (device, pinned, streams) to the driver;
 * mfs_pool_stats reports bytes held and the number of driver allocations made so far (NULL = not wanted).
 */
int mfs_host_alloc(void** ptr, uint64_t bytes, int device);
int mfs_host_free(void* ptr);
int mfs_pool_trim(int device);
int mfs_pool_stats(int device, uint64_t* device_bytes, uint64_t* pinned_bytes, uint64_t* device_allocs,
                   uint64_t* pinned_allocs);
/* HIP-event timing on `stream` (bench.py's live per-launch kernel time) */
int mfs_event_create(void** event);
int mfs_event_destroy(void* event);
int mfs_event_record(void* event, void* stream);
int mfs_event_elapsed_ms(void* start, void* stop, float* ms); /* synchronises on `stop` */

/*
 * ---- 1-D moment filter, host pointers ------------------------------------------------------------------------
 * Replaces moment_filter_rms / moment_filter_cms / moment_filter_scms (mfs/one_dim/filtering.py:32-89, 92-161,
 * 164-240) for B replicates at once.
 *
 *   mode        MFS_MODE_*
 *   N           quadrature order; the moment vectors have 2N entries (orders 0..2N-1), 2 <= N <= MFS_MAX_N
 *   T, B        time steps, replicates
 *   m0          initial moments, [2N] (m0_batched = 0) or [B][2N]
 *   mean0       [1] or [B] (same batching as m0); ignored in raw mode (may be NULL)
 *   scale0      likewise; scaled mode only
 *   ys          [B][T], measurements as doubles (Bernoulli y in {0., 1.})
 *   stable      0 = Cholesky; 1 = LDL^T completion (mfs/utils.py:495-538), on the same register-resident kernel (the completed
 *               rule stays tridiagonal)
 *   out_moments [B][T][2N]   out_means [B][T] (NULL in raw mode)   out_scales [B][T] (scaled mode, else NULL)
 *   out_nell    [B]          out_first_nan [B]: first step whose outputs are non-finite, -1 if none (may be NULL)
 *   device      HIP device ordinal; stream: hipStream_t or NULL (a stream of the library's).  Returns after the
 *               results are in the host buffers.
 * When out_moments is requested and large, the run is split into T-chunks (carry state in HBM, bit-identical to one
 * launch) and each chunk's slice of the moments is copied out while the next chunk computes (MFS_HOST_CHUNKS=n
 * overrides the chunk count, 1 = no pipelining).  Per-replicate parameters theta arrive as
 * batched model tables (model->coef_batched / lik_batched), not as a separate argument.
 */
int mfs_filter_1d(const mfs_model_1d* model, int mode, int N, int T, int B,
                  const double* m0, int m0_batched, const double* mean0, const double* scale0,
                  const double* ys, int stable,
                  double* out_moments, double* out_means, double* out_scales, double* out_nell,
                  int32_t* out_first_nan, int device, void* stream);

/*
 * ---- 1-D moment filter, device-resident plan -----------------------------------------------------------------
 * The same computation with every buffer already in HBM.  A plan uploads the model tables once, owns the carry
 * state, splits T into chunks of `chunk` steps (0 = whole T in one launch) and captures the chunk launches into a
 * hipGraph so that a run is one graph launch.  All pointers passed to mfs_plan_1d_run are DEVICE pointers with the
 * layouts documented for mfs_filter_1d; out_moments may be NULL ("NLL only", the parameter-estimation grid of
 * dardel/parameter_estimation/mf.py:37-54 needs nothing else).
 */
typedef struct mfs_plan_1d mfs_plan_1d;

int mfs_plan_1d_create(mfs_plan_1d** plan, const mfs_model_1d* model /* host pointers inside */, int mode, int N,
                       int T, int B, int stable, int chunk, int device);
int mfs_plan_1d_run(mfs_plan_1d* plan, const double* d_m0, int m0_batched, const double* d_mean0,
                    const double* d_scale0, const double* d_ys, double* d_out_moments, double* d_out_means,
                    double* d_out_scales, double* d_out_nell, int32_t* d_out_first_nan, void* stream);
int mfs_plan_1d_destroy(mfs_plan_1d* plan);
/* launch geometry actually used (for DESIGN.md / the bench JSON): lanes per filter, filters per block, grid size */
int mfs_plan_1d_geometry(const mfs_plan_1d* plan, int* lanes_per_filter, int* filters_per_block, int* grid,
                         int* lds_bytes_per_block);
/* which build of the 1-D filter kernel the plan launches, decided at plan creation.  The specialised one-wave build keeps
 * the model's coefficient table in registers and runs the two halves of a step as straight-line code; it exists for the
 * orders with a one-wave build (N = 14..16), operator tables of 2 / 4 / 6 terms and normal closures of polynomial degree
 * <= 3, and computes bit for bit what the generic build computes (MFS_FAST_BUILD=generic keeps the generic one).  A
 * specialised build that also has the model's step switches compiled in (mfs_plan_1d_kernel_traits below) reports the same
 * code, MFS_BUILD_FAST_ONE_WAVE_SPEC. */
#define MFS_BUILD_DENSE 0
#define MFS_BUILD_FAST 1
#define MFS_BUILD_FAST_ONE_WAVE 2
#define MFS_BUILD_FAST_ONE_WAVE_SPEC 3
int mfs_plan_1d_kernel_build(const mfs_plan_1d* plan, int* build);
/* the step traits of the plan's kernel build.  MFS_TRAITS_RUNTIME: moment mode, u-map and likelihood law are run-time values
 * of the launch (every build but the ones below).  Otherwise the plan runs a specialised one-wave build with the three
 * compiled in, the likelihood parameters in registers and the output stores decided before the time loop; it exists for the
 * combinations named here, central mode only, and computes bit for bit what the run-time-traits build computes
 * (MFS_FAST_TRAITS=runtime, read at plan creation, keeps that one). */
#define MFS_TRAITS_RUNTIME 0
#define MFS_TRAITS_CENTRAL_TANH_BERNOULLI 1      /* operator table of 6 terms (TME-3) or normal closure */
#define MFS_TRAITS_CENTRAL_IDENTITY_GAUSSIAN 2   /* normal closure */
int mfs_plan_1d_kernel_traits(const mfs_plan_1d* plan, int* traits);
/* 1: the plan runs the partner-wave variant of its fixed-traits build (N = 14, 15): 512-thread workgroups in which four main
 * waves run the step's critical path and four partner waves, one beside each on its SIMD, form the posterior moments, decide
 * the poisoning and accumulate the likelihood.  Bit for bit the one-wave build's outputs (MFS_FAST_PARTNER=0, read at plan
 * creation, keeps that one; a run under MFS_PREDICT_RULE=recompute takes it as well).  mfs_plan_1d_kernel_build and
 * mfs_plan_1d_kernel_traits report what they report for the one-wave build; mfs_plan_1d_geometry reports the variant's. */
int mfs_plan_1d_kernel_partner(const mfs_plan_1d* plan, int* partner);
/* placement record of the partner-wave variant, over the launches of this process on the current device: the workgroups
 * whose prologue compared the SIMDs of its waves, and those among them in which a main wave and its partner did not share one.
 * Sums over every order that has the variant.  A profile record: nothing but speed depends on the placement. */
int mfs_partner_placement(uint64_t* workgroups, uint64_t* mismatches);

/*
 * ---- negative log-likelihood and its gradient, forward mode inside the time loop ------------------------------------
 * Replaces what dardel/parameter_estimation/mf.py:37-54,70-73 obtains by differentiating obj_func (moment_filter_cms
 * under jax.jit) through the lax.scan with JAX autodiff for jaxopt.ScipyMinimize(L-BFGS-B): the filter's state -- moments,
 * mean, scale, nell -- is carried as dual numbers (value + n_par tangents) through every Cholesky pivot, eigenvalue,
 * weight and quadrature sum (mfs_amd/csrc/filter1d_grad.hpp); no reverse pass.
 *
 *   model       the value tables, as for mfs_filter_1d (coef_batched / lik_batched: one parameter point per replicate)
 *   dcoef       d coef / d theta_p: [n_par][n_rows][degree + 1], or [B][n_par][n_rows][degree + 1] when coef_batched
 *   dlik        d lik / d theta_p:  [n_par][n_lik], or [B][n_par][n_lik] when lik_batched
 *   n_par       1 .. 4;  N  2 .. 16;  m0, mean0, scale0, ys as for mfs_filter_1d (the initial law does not depend on theta)
 *   out_nell    [B];  out_grad [B][n_par] = d nell / d theta_p;  out_first_nan [B] or NULL.  Host pointers.
 * A replicate that NaN-poisons returns NaN in both, as the reference's objective would.
 */
int mfs_filter_1d_grad(const mfs_model_1d* model, const double* dcoef, const double* dlik, int n_par, int mode, int N,
                       int T, int B, const double* m0, int m0_batched, const double* mean0, const double* scale0,
                       const double* ys, double* out_nell, double* out_grad, int32_t* out_first_nan, int device,
                       void* stream);

/*
 * ---- quadrature only -----------------------------------------------------------------------------------------
 * Replaces moment_quadrature (mfs/one_dim/quadtures.py:83-133) for B moment vectors: ms [B][2N], mean/scale [B] or
 * NULL (0 / 1), out weights/nodes [B][N].  Host pointers.  Used by the parity tests to check the Cholesky /
 * triangular-solve / eigensolve stage in isolation, and by characteristic-function post-processing
 * (mfs/one_dim/moments.py:309-337).
 */
int mfs_quadrature_1d(int N, int B, const double* ms, const double* mean, const double* scale, int stable,
                      double* out_weights, double* out_nodes, int device, void* stream);

/*
 * ---- characteristic function from moments ------------------------------------------------------------------------
 * Replaces characteristic_fn (mfs/one_dim/moments.py:309-337) as the post-processing drivers call it
 * (dardel/benes_bernoulli/post_processing_mf.py:37-60: vmapped over the z grid and over every filtering step):
 * out[c][k] = sum_n w_n exp(i zs[k] x_n) with (w, x) the quadrature of ms[c] (mean / scale [count] or NULL).
 * ms [count][2N]; zs [nz]; out [count][nz][2] = (re, im) pairs, i.e. a C-contiguous complex128 array.  Host pointers.
 */
int mfs_characteristic_1d(int N, int count, const double* ms, const double* mean, const double* scale, int nz,
                          const double* zs, double* out, int device, void* stream);

/*
 * ---- diagnostic: the kernels' own elementary functions -------------------------------------------------------------
 * The 1-D kernel evaluates exp / tanh / log with short in-line routines instead of the ocml ones (the reference uses
 * jnp.exp / jnp.tanh / jnp.log inside its model callables, mfs/one_dim/ss_models.py:37-47).  This entry point applies
 * them to an array so that the tests can bound their error against libm.  which: 0 exp, 1 tanh, 2 log.  Host pointers.
 */
int mfs_elementary(int which, int n, const double* x, double* out, int device);

/*
 * ---- diagnostic: the shared device math and the likelihood forms ---------------------------------------------------
 * Every routine of csrc/device_util.hpp and csrc/likelihood.hpp that the kernel families share, one thread per element,
 * from a translation unit of its own (csrc/device_math_inst.hip), so that the tests can compare each with exact
 * arithmetic.  in is [n_in][n], out is [n_out][n] (argument j of element i at in[j * n + i]); integer arguments (kind,
 * degree, D) travel as doubles.  n_in and n_out must be the routine's own (below), n >= 1.  Host pointers.
 *
 *   fn                              inputs                                       outputs
 *   MFS_DM_EXP / _EXP_SC            y                                            fast_exp<false / true>
 *   MFS_DM_TANH                     x                                            fast_tanh
 *   MFS_DM_LOG / _LOG_SC            v                                            fast_log<false / true>
 *   MFS_DM_RCP_NR / _RCP_SAT / _RSQ_NR   v                                       the Newton-refined 1 / v, 1 / v, 1 / sqrt(v)
 *   MFS_DM_LOG_FACTORIAL            y                                            log(y!)
 *   MFS_DM_HORNER                   degree, u, row[MFS_MAX_DEGREE + 1]           sum_j row[j] u^j
 *   MFS_DM_POLY2                    D, x0, x1, c[HI * HI] (HI = MFS_ND_MAX_EXTENT_HI; the D x D table is c[a * D + b])
 *                                                                                sum c[a][b] x0^a x1^b
 *   MFS_DM_POLY2_GRAD               the same                                     value, d / dx0, d / dx1
 *   MFS_DM_CHOL2                    p00, p01, p11                                l00, l10, l11, ok (1 / 0)
 *   MFS_DM_LIKELIHOOD               kind, lp[MFS_MAX_LIK], y, x                  likelihood (libm form)
 *   MFS_DM_LIKELIHOOD_ND            the same                                     likelihood_nd
 *   MFS_DM_LIK_DENSITY / _SC        kind, eta, var, y                            lik_density<false / true>
 *   MFS_DM_LIKELIHOOD_JOINT_ND      kind, lp[MFS_MAX_LIK], y, x0, x1             likelihood_joint_nd
 *   MFS_DM_LIKELIHOOD_FAST / _REGS  kind, lp[MFS_MAX_LIK], y, x                  likelihood_fast with the parameters behind a
 *                                                                                pointer / in LikRegs; the log(y!) table in LDS
 *   MFS_DM_LFAC_TABLE               y (an integer in [0, 32])                    the entry of that table
 */
#define MFS_DM_EXP 0
#define MFS_DM_EXP_SC 1
#define MFS_DM_TANH 2
#define MFS_DM_LOG 3
#define MFS_DM_LOG_SC 4
#define MFS_DM_RCP_NR 5
#define MFS_DM_RCP_SAT 6
#define MFS_DM_RSQ_NR 7
#define MFS_DM_LOG_FACTORIAL 8
#define MFS_DM_HORNER 9
#define MFS_DM_POLY2 10
#define MFS_DM_POLY2_GRAD 11
#define MFS_DM_CHOL2 12
#define MFS_DM_LIKELIHOOD 13
#define MFS_DM_LIKELIHOOD_ND 14
#define MFS_DM_LIK_DENSITY 15
#define MFS_DM_LIK_DENSITY_SC 16
#define MFS_DM_LIKELIHOOD_JOINT_ND 17
#define MFS_DM_LIKELIHOOD_FAST 18
#define MFS_DM_LIKELIHOOD_FAST_REGS 19
#define MFS_DM_LFAC_TABLE 20
#define MFS_DM_COUNT 21
int mfs_device_math(int fn, int n, int n_in, const double* in, int n_out, double* out, int device);

/*
 * ---- N-D moment filter (d = 2), host pointers ------------------------------------------------------------------
 * Replaces moment_filter_nd_rms / moment_filter_nd_cms / moment_filter_nd_scms (mfs/multi_dims/filtering.py:283-344,
 * 210-280, 33-207) for B replicates, with either transition family the reference offers.
 *
 * MFS_ND_TRANS_OPERATOR ('multi-index' signature, sde_cond_moments_tme, mfs/multi_dims/moments.py:414-479):
 * polynomial drift / dispersion reduced on the host to the operator table Q_kappa(x), 1 <= |kappa| <= 2 M for TME order
 * M <= 3, dense per-variable extent D, in graded-lex kappa order (0,1),(1,0),(0,2),(1,1),(2,0),(0,3),..., zeros where the
 * model has no term.  Conditional mean_k = x_k + Q_{e_k}.  Two layouts, chosen by n_terms (MFS_ND_TABLE_ROWS):
 *   n_terms <= MFS_ND_TERMS (|kappa| <= 4, TME order <= 2): coef [16][D][D], rows 14, 15 the conditional variances of
 *     X'_0, X'_1 (diagonal of tme.mean_and_cov, moments.py:469-476; read in scaled mode only);
 *   n_terms <= MFS_ND_TERMS_MAX (|kappa| <= 6, TME order 3): coef [29][D][D], rows 27, 28 the variances.
 *
 * MFS_ND_TRANS_GAUSSIAN ('index' signature, the Normal closures sde_cond_moments_tme_normal / _euler_maruyama,
 * mfs/multi_dims/moments.py:340-411, 257-337, whose moments the reference takes from Kan's formula, :110-154):
 * X' | x ~ N(mu(x), S(x)); rows 0..4 of coef hold the polynomials mu_0, mu_1, S_00, S_01, S_11 (n_terms = 5), the
 * other rows are ignored.  The kernel evaluates E[(X'_0-c_0)^a (X'_1-c_1)^b] by the Stein recursion, which is the
 * same polynomial in (mu - c, S) as Kan's sum.
 * The likelihood is a product of up to MFS_ND_MAX_FACTORS factors, each a function of ONE state component and one
 * column of the measurement: p(y | x) = prod_f lik(kind_f, params_f, y[ycol_f], x[component_f]).  One factor on x_0 is the
 * prey--predator model (mfs/multi_dims/ss_models.py:63-67); two Gaussian factors, one per component, are the reference's
 * measurement_cond_pdf_2d (tests/test_filtering.py:36-46: ys_2d of shape (T, 2), prod(norm.pdf(y, x, sd))).
 *
 *   N              quadrature order per dimension: s = N(N+1)/2 Gram size, z = N(2N+1) moments (|n| <= 2N-1), 2..7
 *   multi_indices  [z][2] int32, must equal the graded-lex table (checked: MFS_EINVAL otherwise, mirroring the
 *                  reference's only raise, multi_dims/filtering.py:238-239)
 *   inds           [3][s][s] int32 Gram / Hankel gather tables (gram_and_hankel_indices_graded_lexico)
 *   m0 [z] or [B][z]; mean0 [2] or [B][2] (central, scaled); scale0 likewise (scaled); ys [B][T][ny]
 *   out_moments [B][T][z]; out_means [B][T][2] (central, scaled; NULL in raw mode); out_scales [B][T][2] (scaled);
 *   out_nell [B]; out_first_nan [B]
 */
#define MFS_ND_TERMS 14     /* kappa terms with |kappa| <= 4 */
#define MFS_ND_TERMS_MAX 27 /* ... with |kappa| <= 6 */
#define MFS_ND_ROWS 16      /* coefficient blocks of the short layout: MFS_ND_TERMS operator terms + 2 variance rows */
#define MFS_ND_ROWS_MAX 29
#define MFS_ND_TABLE_ROWS(n_terms) ((n_terms) > MFS_ND_TERMS ? MFS_ND_ROWS_MAX : MFS_ND_ROWS)
#define MFS_ND_MAX_EXTENT 6    /* per-variable extent (degree + 1) of the coefficient blocks, short layout */
#define MFS_ND_MAX_EXTENT_HI 7 /* ... long layout (TME order 3 of a quadratic drift reaches degree 6) */
#define MFS_ND_MAX_FACTORS 2
#define MFS_ND_TRANS_OPERATOR 0
#define MFS_ND_TRANS_GAUSSIAN 1
typedef struct mfs_model_nd {
    int32_t d;             /* 2 (d = 1 problems go through the 1-D entry points, which the reference guarantees equal:
                              tests/test_filtering.py:304-329; mfs_amd.multi_dims.filtering routes them) */
    int32_t trans_kind;    /* MFS_ND_TRANS_* */
    int32_t n_terms;       /* MFS_ND_TABLE_ROWS(n_terms) blocks are passed; operator terms >= n_terms are known to be zero */
    int32_t extent;        /* D <= MFS_ND_MAX_EXTENT (MFS_ND_MAX_EXTENT_HI with the long layout) */
    int32_t n_factors;     /* 1 .. MFS_ND_MAX_FACTORS likelihood factors */
    int32_t ny;            /* measurement columns per step (1 or 2) */
    int32_t fac_kind[MFS_ND_MAX_FACTORS];      /* MFS_LIK_* */
    int32_t fac_component[MFS_ND_MAX_FACTORS]; /* state component the factor reads */
    int32_t fac_ycol[MFS_ND_MAX_FACTORS];      /* measurement column the factor reads (< ny) */
    int32_t fac_n_par[MFS_ND_MAX_FACTORS];     /* parameters used (<= MFS_MAX_LIK) */
    int32_t coef_batched;  /* 0: one table; 1: one per replicate (per-replicate drift / dispersion parameters) */
    int32_t lik_batched;   /* likewise for the likelihood parameters */
    const double* coef;    /* [rows][D][D] or [B][rows][D][D], rows = MFS_ND_TABLE_ROWS(n_terms) */
    const double* lik;     /* [n_factors][MFS_MAX_LIK] or [B][n_factors][MFS_MAX_LIK], unused entries 0 */
} mfs_model_nd;

int mfs_filter_nd(const mfs_model_nd* model, int mode, int N, int T, int B, int z, const int32_t* multi_indices,
                  const int32_t* inds, const double* m0, int m0_batched, const double* mean0, const double* scale0,
                  const double* ys, int stable, double* out_moments, double* out_means, double* out_scales,
                  double* out_nell, int32_t* out_first_nan, int device, void* stream);

/*
 * ---- N-D plan: device pointers ------------------------------------------------------------------------------------
 * The same filter for callers that keep data resident in HBM (benchmark harness, repeated calls of a jitted filter as
 * in dardel/prey_predator/mf.py:54-65): model tables and gather indices are uploaded once at create; run() only
 * enqueues the kernel on `stream`.  Device buffers have the layouts documented for mfs_filter_nd; d_out_moments,
 * d_out_means, d_out_scales, d_out_first_nan may be NULL.
 */
typedef struct mfs_plan_nd mfs_plan_nd;

int mfs_plan_nd_create(mfs_plan_nd** plan, const mfs_model_nd* model /* host pointers inside */, int mode, int N,
                       int T, int B, int z, const int32_t* multi_indices, const int32_t* inds, int stable, int device);
int mfs_plan_nd_run(mfs_plan_nd* plan, const double* d_m0, int m0_batched, const double* d_mean0,
                    const double* d_scale0, const double* d_ys, double* d_out_moments, double* d_out_means,
                    double* d_out_scales, double* d_out_nell, int32_t* d_out_first_nan, void* stream);
int mfs_plan_nd_destroy(mfs_plan_nd* plan);
/* launch geometry: threads per filter (one workgroup each), grid size, dynamic LDS bytes per workgroup */
int mfs_plan_nd_geometry(const mfs_plan_nd* plan, int* threads_per_filter, int* grid, int* lds_bytes_per_block);

/*
 * ---- N-D moment filter for three-dimensional states (d = 3), host pointers ----------------------------------------
 * The same three filters (mfs/multi_dims/filtering.py:33-344) for d = 3 (Lorenz-63, three-species Lotka--Volterra, 3-D OU),
 * on a kernel of its own (mfs_amd/csrc/filternd3_kernel.hpp).  Gram size s = C(N + 2, 3), z = C(2N + 2, 3) moments
 * (|n| <= 2N - 1), s^3 tensor nodes; MFS_ND3_MIN_N <= N <= MFS_ND3_MAX_N (s = 4, 10, 20; z = 20, 56, 120).
 *
 * mfs_model_nd3.coef is [MFS_ND3_ROWS][D][D][D] (or [B][MFS_ND3_ROWS][D][D][D] when coef_batched), D = extent, entry
 * [row][a][b][c] the coefficient of x0^a x1^b x2^c:
 *   MFS_ND_TRANS_OPERATOR: rows 0..33 the operator table Q_kappa, 1 <= |kappa| <= 4 (TME order <= 2), in graded-lex kappa
 *     order (0,0,1),(0,1,0),(1,0,0),(0,0,2),(0,1,1),(0,2,0),(1,0,1),(1,1,0),(2,0,0),(0,0,3),... -- the row of kappa is its
 *     position in the graded-lex multi-index table minus one; zeros where the model has no term.  Rows 34..36: the
 *     conditional variances of X'_0, X'_1, X'_2 (scaled mode).  Conditional mean_k = x_k + Q_{e_k}.
 *   MFS_ND_TRANS_GAUSSIAN: rows 0..8 = mu_0, mu_1, mu_2, S_00, S_01, S_02, S_11, S_12, S_22 of X' | x ~ N(mu(x), S(x))
 *     (Euler--Maruyama, TME-normal, exact linear-Gaussian steps); the other rows are ignored.
 * Likelihood: a product of up to MFS_ND3_MAX_FACTORS factors, each a function of one state component (fac_component 0..2) and
 * one measurement column (fac_ycol < ny <= 3); kinds Bernoulli-logistic, Poisson-softplus, Gaussian.  Factors of several
 * components: mfs_joint_nd3 below.
 *
 *   multi_indices  [z][3] int32, the graded-lex table (checked);  inds [4][s][s] int32, the Gram / Hankel gather tables (checked)
 *   m0 [z] or [B][z]; mean0, scale0 [3] or [B][3]; ys [B][T][ny]
 *   out_moments [B][T][z]; out_means [B][T][3] (central, scaled); out_scales [B][T][3] (scaled); out_nell [B]; out_first_nan [B]
 * A replicate whose moment matrix is not positive definite is NaN-poisoned from that step on, and only that replicate.
 */
#define MFS_ND3_MIN_N 2
#define MFS_ND3_MAX_N 4
#define MFS_ND3_TERMS 34      /* kappa terms with 1 <= |kappa| <= 4 in three variables */
#define MFS_ND3_ROWS 37       /* coefficient blocks: MFS_ND3_TERMS operator terms + 3 variance rows */
#define MFS_ND3_GAUSS_TERMS 9 /* mu_0..2 and the 6 covariance polynomials */
#define MFS_ND3_MAX_EXTENT 6  /* per-variable extent (degree + 1) of the coefficient blocks */
#define MFS_ND3_MAX_FACTORS 3
typedef struct mfs_model_nd3 {
    int32_t trans_kind;    /* MFS_ND_TRANS_* */
    int32_t n_terms;       /* MFS_ND3_TERMS (operator) or MFS_ND3_GAUSS_TERMS (Gaussian) */
    int32_t extent;        /* D <= MFS_ND3_MAX_EXTENT */
    int32_t n_factors;     /* 1 .. MFS_ND3_MAX_FACTORS */
    int32_t ny;            /* measurement columns per step (1 .. 3) */
    int32_t fac_kind[MFS_ND3_MAX_FACTORS];      /* MFS_LIK_* (not MFS_LIK_BEARING_GAUSSIAN) */
    int32_t fac_component[MFS_ND3_MAX_FACTORS]; /* 0 .. 2 */
    int32_t fac_ycol[MFS_ND3_MAX_FACTORS];      /* < ny */
    int32_t fac_n_par[MFS_ND3_MAX_FACTORS];     /* <= MFS_MAX_LIK */
    int32_t coef_batched;
    int32_t lik_batched;
    const double* coef;    /* [MFS_ND3_ROWS][D][D][D] or [B][MFS_ND3_ROWS][D][D][D] */
    const double* lik;     /* [n_factors][MFS_MAX_LIK] or [B][n_factors][MFS_MAX_LIK], unused entries 0 */
} mfs_model_nd3;

int mfs_filter_nd3(const mfs_model_nd3* model, int mode, int N, int T, int B, int z, const int32_t* multi_indices,
                   const int32_t* inds, const double* m0, int m0_batched, const double* mean0, const double* scale0,
                   const double* ys, int stable, double* out_moments, double* out_means, double* out_scales,
                   double* out_nell, int32_t* out_first_nan, int device, void* stream);

/* d = 3 plan, device pointers: as mfs_plan_nd (tables uploaded at create, run() only enqueues the kernel on `stream`;
 * d_out_moments, d_out_means, d_out_scales, d_out_first_nan may be NULL).  mfs_filter_nd3 runs the same launch. */
typedef struct mfs_plan_nd3 mfs_plan_nd3;

int mfs_plan_nd3_create(mfs_plan_nd3** plan, const mfs_model_nd3* model /* host pointers inside */, int mode, int N,
                        int T, int B, int z, const int32_t* multi_indices, const int32_t* inds, int stable, int device);
int mfs_plan_nd3_run(mfs_plan_nd3* plan, const double* d_m0, int m0_batched, const double* d_mean0,
                     const double* d_scale0, const double* d_ys, double* d_out_moments, double* d_out_means,
                     double* d_out_scales, double* d_out_nell, int32_t* d_out_first_nan, void* stream);
int mfs_plan_nd3_destroy(mfs_plan_nd3* plan);
int mfs_plan_nd3_geometry(const mfs_plan_nd3* plan, int* threads_per_filter, int* grid, int* lds_bytes_per_block);

/*
 * ---- d = 3: joint likelihood factors (functions of all three state components) -------------------------------------
 * A joint factor is kind(y ; u(x), par) with kind one of MFS_LIK_BERNOULLI_LOGISTIC (p = logistic(u)),
 * MFS_LIK_POISSON_SOFTPLUS (rate = softplus(u)), MFS_LIK_GAUSSIAN (y ~ N(u, par), par the variance), and u a scalar link of
 * at most two trivariate polynomials p, q:
 *   MFS_ND3_LINK_POLY        u = p(x)                     y ~ N(x0 x1, var); Poisson(softplus(x0 + x1 + x2))
 *   MFS_ND3_LINK_SQRT        u = sqrt(p(x))               range |x - s|
 *   MFS_ND3_LINK_ATAN2       u = atan2(p(x), q(x))        azimuth atan2(x1 - s1, x0 - s0); no angle wrapping of y - u
 *   MFS_ND3_LINK_ATAN2_SQRT  u = atan2(p(x), sqrt(q(x)))  elevation atan2(x2 - s2, hypot(x0 - s0, x1 - s1))
 * coef is [n_joint][2][E][E][E] (or [B][n_joint][2][E][E][E] when batched): block [f][0] is p, [f][1] is q (zeros where the
 * link has no q), entry [a][b][c] the coefficient of x0^a x1^b x2^c, E = extent <= MFS_ND3_JOINT_MAX_EXTENT (degree 3).
 * par is [n_joint] (or [B][n_joint]): the Gaussian variance, ignored by the other kinds.  `batched` covers coef and par.
 * The factors multiply the single-component factors of mfs_model_nd3, whose n_factors may then be 0 (lik may be NULL) and
 * whose ny may reach MFS_ND3_JOINT_MAX_NY; every ycol, single or joint, is < ny.  sqrt of a negative value and any
 * non-finite u NaN-poison the replicate from that step on, as a non-finite posterior does.
 * mfs_plan_nd3_create_joint makes an ordinary mfs_plan_nd3 (run / destroy / geometry as above); joint == NULL or
 * n_joint == 0 is refused -- such a model goes through mfs_plan_nd3_create and runs the kernel it always ran.
 */
#define MFS_ND3_MAX_JOINT 3
#define MFS_ND3_JOINT_MAX_EXTENT 4 /* per-variable extent (degree + 1) of p and q */
#define MFS_ND3_JOINT_MAX_NY 6
#define MFS_ND3_LINK_POLY 0
#define MFS_ND3_LINK_SQRT 1
#define MFS_ND3_LINK_ATAN2 2
#define MFS_ND3_LINK_ATAN2_SQRT 3
typedef struct mfs_joint_nd3 {
    int32_t n_joint;                       /* 1 .. MFS_ND3_MAX_JOINT */
    int32_t extent;                        /* E, 1 .. MFS_ND3_JOINT_MAX_EXTENT */
    int32_t batched;                       /* coef and par carry a leading [B] */
    int32_t kind[MFS_ND3_MAX_JOINT];       /* MFS_LIK_BERNOULLI_LOGISTIC / _POISSON_SOFTPLUS / _GAUSSIAN */
    int32_t link[MFS_ND3_MAX_JOINT];       /* MFS_ND3_LINK_* */
    int32_t ycol[MFS_ND3_MAX_JOINT];       /* < ny of the model */
    const double* coef;                    /* [n_joint][2][E][E][E] or [B][...] */
    const double* par;                     /* [n_joint] or [B][n_joint] */
} mfs_joint_nd3;

int mfs_filter_nd3_joint(const mfs_model_nd3* model, const mfs_joint_nd3* joint, int mode, int N, int T, int B, int z,
                         const int32_t* multi_indices, const int32_t* inds, const double* m0, int m0_batched,
                         const double* mean0, const double* scale0, const double* ys, int stable, double* out_moments,
                         double* out_means, double* out_scales, double* out_nell, int32_t* out_first_nan, int device,
                         void* stream);
int mfs_plan_nd3_create_joint(mfs_plan_nd3** plan, const mfs_model_nd3* model, const mfs_joint_nd3* joint /* host pointers */,
                              int mode, int N, int T, int B, int z, const int32_t* multi_indices, const int32_t* inds,
                              int stable, int device);

/*
 * ---- brute-force grid filter: the true 1-D filtering densities, host pointers ---------------------------------------
 * Replaces brute_force_filter (mfs/classical_filters_smoothers/brute_force.py:26-136, Chapman--Kolmogorov branches
 * 'chapman-euler' / 'chapman-tme-k') as the driver runs it (dardel/benes_bernoulli/brute_force.py: 2000 grid points, 100
 * sub-steps per measurement, chapman-tme-3), for B replicates on one shared grid.  The transition density over one sub-step
 * is Normal, N(x'; trans_mean(x), trans_sd(x)^2) (tme.mean_and_cov at :74-78, Euler at :70); the caller evaluates the two
 * on the grid, so no model struct crosses here.  Per measurement: `substeps` applications of
 *   p(x_i) <- sum_j w_j N(x_i; trans_mean_j, trans_sd_j^2) p(x_j)        (w = the weights of jnp.trapz(., xs), :86)
 * then p <- lik(y, x) p / z with z = sum_i w_i lik(y, x_i) p(x_i) (:133), out_nell -= log z.
 *
 *   n, T, B      grid points (2 .. MFS_GRID_MAX_N), measurements, replicates
 *   substeps     >= 1, integration_steps of the reference
 *   use_power    1: form the n x n matrix of `substeps` sub-steps once (binary exponentiation), one product per measurement;
 *                0: apply the one-sub-step matrix `substeps` times per measurement.  Same result up to rounding: every entry
 *                is non-negative, so the products are componentwise forward-stable whatever the association
 *   xs           [n] strictly increasing (uneven spacing allowed);  trans_mean, trans_sd [n], trans_sd finite and > 0
 *   lik_kind     MFS_LIK_BERNOULLI_LOGISTIC / _POISSON_SOFTPLUS / _GAUSSIAN; lik [n_lik] or [B][n_lik] (lik_batched)
 *   init_ps      [n] or [B][n] (init_batched): the initial density on the grid;  ys [B][T]
 *   out_pdfs     [B][T][n] or NULL: with NULL nothing of that size exists on the device either
 *   out_means, out_vars [B][T]: trapezoid mean and central variance of each posterior (may be NULL)
 *   out_nell [B];  out_first_nan [B] or NULL: the first step whose normaliser is zero or not finite, -1 if none.  That
 *                replicate is NaN from that step on, in-band, and only that replicate.
 * Two calls with the same inputs return the same bits.  MFS_EINVAL: n < 2, T < 1, B < 1, substeps < 1, xs not strictly
 * increasing, trans_sd not finite or not > 0, lik_kind not one of the three, a NULL required buffer.  MFS_EUNSUPPORTED:
 * n > MFS_GRID_MAX_N (the power route holds three padded n x n buffers: 1.6 GB at 8192).
 */
#define MFS_GRID_MAX_N 8192
int mfs_grid_filter_1d(int n, int T, int B, int substeps, int use_power,
                       const double* xs, const double* trans_mean, const double* trans_sd,
                       int lik_kind, int n_lik, const double* lik, int lik_batched,
                       const double* init_ps, int init_batched, const double* ys,
                       double* out_pdfs, double* out_means, double* out_vars,
                       double* out_nell, int32_t* out_first_nan, int device, void* stream);
/*
 * The same filter, and on request the characteristic function of every posterior: the `true_filtering_cfs` that
 * dardel/benes_bernoulli/post_processing_brute_force.py:27-50 takes with characteristic_from_pdf (mfs/one_dim/moments.py:340-343)
 * of the downloaded pdfs, the ground truth of the cf errors of dardel/benes_bernoulli/compute_errs.py:103-113:
 *   out_cfs[b][t][k] = sum_i w_i exp(i zs[k] x_i) p_{b,t}(x_i)                  (w = the weights of jnp.trapz(., xs))
 * as one more product per measurement on the matrix core, with a table of w_i cos(zs[k] x_i) and w_i sin(zs[k] x_i) built
 * once per call from fp64 sincos of the rounded product (any finite zs: no spacing is assumed).
 *   nz, zs       frequencies, 0 .. MFS_GRID_MAX_NZ of them; zs [nz], finite.  nz = 0: zs and out_cfs may be NULL, and the
 *                call is mfs_grid_filter_1d (which forwards here), bit for bit
 *   out_cfs      [B][T][nz][2] = (re, im) pairs, i.e. a C-contiguous complex128 array.  Nothing of that size exists on the
 *                device: the pairs leave in blocks of a few steps while the next steps are computed
 *   every other argument as in mfs_grid_filter_1d; the other outputs do not depend on nz.
 * A replicate whose normaliser was zero or not finite at step t has NaN in both parts from step t on (out_first_nan), and only
 * that replicate.  The sum over i runs in ascending order in one wave: two calls return the same bits, and a replicate's cfs
 * do not depend on the batch it is in.  MFS_EINVAL, besides those of mfs_grid_filter_1d: nz < 0, nz > 0 with zs or out_cfs
 * NULL, a zs entry that is not finite.  MFS_EUNSUPPORTED: nz > MFS_GRID_MAX_NZ (the table is 2 nz n doubles, padded: 1 GB at
 * 8192 x 8192).
 */
#define MFS_GRID_MAX_NZ 8192
int mfs_grid_filter_1d_cf(int n, int T, int B, int substeps, int use_power,
                          const double* xs, const double* trans_mean, const double* trans_sd,
                          int lik_kind, int n_lik, const double* lik, int lik_batched,
                          const double* init_ps, int init_batched, const double* ys,
                          int nz, const double* zs,
                          double* out_pdfs, double* out_means, double* out_vars, double* out_cfs /* [B][T][nz][2] */,
                          double* out_nell, int32_t* out_first_nan, int device, void* stream);
/*
 * characteristic_from_pdf (mfs/one_dim/moments.py:340-343) on its own, for densities that did not come from the filter (a saved
 * run, a reconstructed pdf): out[c][k] = sum_i w_i exp(i zs[k] xs[i]) ps[c][i], the trapezoid rule on xs.  Same table kernel and
 * same GEMM as mfs_grid_filter_1d_cf, with the table transposed so that the densities are used as they lie.
 *   n, xs        grid points (2 .. MFS_GRID_MAX_N), [n] finite and strictly increasing (uneven spacing allowed)
 *   count, ps    densities, [count][n];  nz, zs as above;  out [count][nz][2] = (re, im) pairs
 * Host pointers; the densities are staged in chunks of rows, so the device holds the table and one chunk whatever `count` is.
 * Rows are independent: a NaN in ps[c] makes out[c] NaN and nothing else.  Two calls return the same bits.  count = 0 or nz = 0
 * returns at once.  MFS_EINVAL: n < 2, count < 0, nz < 0, a NULL buffer, xs not strictly increasing, a zs entry that is not
 * finite.  MFS_EUNSUPPORTED: n > MFS_GRID_MAX_N, nz > MFS_GRID_MAX_NZ.
 */
int mfs_cf_from_pdf_1d(int n, int count, int nz, const double* xs, const double* zs, const double* ps /* [count][n] */,
                       double* out /* [count][nz][2] */, int device, void* stream);
/* diagnostic: the filter's fp64 matrix-core GEMM on its own, C[M][N] = A[M][K] B[K][N], row-major DEVICE pointers, enqueued
 * on `stream`.  M and N must be multiples of 64 and K of 16 (the filter pads its buffers to that), C distinct from A and B:
 * MFS_EINVAL otherwise.  The sum over k runs in ascending order in one wave: bit-reproducible. */
int mfs_grid_gemm_dev(int M, int N, int K, const double* d_A, const double* d_B, double* d_C, void* stream);

/*
 * ---- bootstrap particle filter, 1-D, host pointers ------------------------------------------------------------------
 * Replaces bootstrap_filter (mfs/classical_filters_smoothers/smc.py:26-84) with the resamplers stratified / systematic
 * (mfs/classical_filters_smoothers/resampling.py:43-59) as the drivers run it (dardel/benes_bernoulli/pf.py: 10 000 particles,
 * proposal tme.mean_and_cov; dardel/convergence/convergence_pf.py: 100 000), for B replicates at once, and the empirical
 * characteristic function the driver takes of every step's samples (pf.py:58-75).  The two sampler callables of the reference
 * become descriptors: the transition is the Normal closure of a mfs_model_1d (MFS_TRANS_GAUSSIAN: mu(x), var(x)), the initial
 * law a mixture of at most MFS_PF_MAX_MIX Normals, or explicit samples.  Per measurement t (kernels: particle_kernel.hpp):
 *   x_i <- mu(x_i) + sqrt(var(x_i)) z_i (var <= 0 or not finite: NaN);  w_i = lik(y_t, x_i);  nell -= log(mean_i w_i)   (:66-69)
 *   cs = inclusive prefix sums of w / sum w;  v_i = (i + u_i) / n (stratified: one u per particle, systematic: one for all);
 *   idx_i = the first j with cs[j] >= v_i (searchsorted, side left), clamped to [0, n - 1];  x'_i = x[idx_i]              (:76)
 *   out_means, out_vars: mean and population variance (about that mean) of x';  out_cfs[k] = mean_i exp(i zs[k] x'_i).
 *
 * The random stream is part of the interface.  Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9,
 * 0xBB67AE85 after every round), key = (low, high 32 bits of seeds[b]), counter = (particle i, step t, tag, draw); of the
 * four output words r0..r3
 *   uniform  U(a, b) = ((a >> 6) 2^26 + (b >> 6) + 1/2) 2^-52, strictly inside (0, 1);  a draw's uniform is U(r0, r1)
 *   normal   z = sqrt(-2 ln U(r0, r1)) cos(2 pi U(r2, r3))
 *   tag 0 (t = 0): the initial draw: draw 0 gives z, draw 1 the component uniform u_c; component c = #{k : mix_cumw[k] <= u_c}
 *                  clamped to n_mix - 1;  x_i = mix_mean[c] + sqrt(mix_var[c]) z
 *   tag 1: the propagation normal of step t (draw 0);  tag 2: the resampling uniform of step t (draw 0; systematic: particle 0's)
 * A draw depends on (seed, i, t, tag, draw) alone, not on the launch geometry or the batch.
 *
 *   model        trans_kind MFS_TRANS_GAUSSIAN; coef_batched / lik_batched give one table per replicate (a theta grid)
 *   n, T, B      particles (1 .. MFS_PF_MAX_PARTICLES), measurements, replicates;  resampling MFS_RESAMPLE_*
 *   seeds [B];  n_mix 1 .. MFS_PF_MAX_MIX with mix_cumw (cumulative weights), mix_mean, mix_var [n_mix] each, or n_mix = 0 and
 *   init_samples [n] or [B][n] (init_batched);  ys [B][T];  zs [nz] or NULL with nz = 0
 *   out_samples  [B][T][n] or NULL: with NULL nothing of that size exists on the device either
 *   out_means, out_vars [B][T];  out_cfs [B][T][nz][2] = (re, im), i.e. complex128, or NULL;  out_nell [B]
 *   out_first_nan [B] or NULL: the first step whose sum of weights is zero or not finite, -1 if none.  That replicate is NaN
 *                from that step on -- samples, summaries, cf and nell -- and only that replicate; no index leaves [0, n - 1].
 * Every sum runs in an order fixed by n alone (block totals are combined in index order, no atomics): two calls with the same
 * inputs return the same bits, and replicate b of a batch returns the bits of a B = 1 call with seeds[b].  On a uniformly
 * spaced zs the cf takes one true sincos per particle and 8 frequencies and rotates by exp(i dz x) in between.
 * MFS_EINVAL: n, T or B < 1, an unknown resampling code, a model that is not MFS_TRANS_GAUSSIAN, n_mix outside 0 .. 8, n_mix = 0
 * without init_samples, mixture variances not finite and > 0, nz > 0 with a NULL zs or out_cfs, a NULL required buffer.
 * MFS_EUNSUPPORTED: n > MFS_PF_MAX_PARTICLES.  MFS_ENOMEM: the work buffers cannot be had.
 */
#define MFS_PF_MAX_PARTICLES (1 << 20)
#define MFS_PF_MAX_MIX 8
#define MFS_RESAMPLE_STRATIFIED 0
#define MFS_RESAMPLE_SYSTEMATIC 1
int mfs_particle_filter_1d(const mfs_model_1d* model, int n, int T, int B, int resampling, const uint64_t* seeds,
                           int n_mix, const double* mix_cumw, const double* mix_mean, const double* mix_var,
                           const double* init_samples, int init_batched, const double* ys, int nz, const double* zs,
                           double* out_samples, double* out_means, double* out_vars, double* out_cfs, double* out_nell,
                           int32_t* out_first_nan, int device, void* stream);
/* diagnostic, like mfs_elementary: the stream's draws (seed, i, t, tag, draw) for particles i = 0 .. count - 1, computed on the
 * device: out_uniform[i] = U(r0, r1), out_normal[i] = z.  Host pointers, [count] each. */
int mfs_pf_draws(uint64_t seed, int t, int tag, int draw, int count, double* out_uniform, double* out_normal, int device);
/* diagnostic for the benchmark tool: with MFS_PF_SPLIT=1 in the environment mfs_particle_filter_1d records an event after every
 * launch and waits once per step; this returns the summed time in ms of the calling thread's last call per kernel, out[5] =
 * propagate (with the block scan), offsets, resample, cf (with the variance), finalize.  Zeros without the switch.
 * mfs_particle_filter_nd honours the same switch; its fourth kernel is the covariance pass. */
int mfs_pf_last_split_ms(double* out);

/*
 * ---- bootstrap particle filter, d = 2, host pointers ----------------------------------------------------------------
 * bootstrap_filter (mfs/classical_filters_smoothers/smc.py:26-84) as dardel/prey_predator/pf.py runs it: 10 000 particles of a
 * two-dimensional state, Normal proposal N(mu(x), S(x)) with a Cholesky factor per particle, stratified resampling, T = 2000;
 * for B replicates at once.  The transition is the Normal closure of a mfs_model_nd (MFS_ND_TRANS_GAUSSIAN: blocks 0..4 of
 * coef = mu_0, mu_1, S_00, S_01, S_11), the likelihood its 1..MFS_ND_MAX_FACTORS single-component factors, the initial law a
 * mixture of at most MFS_PF_MAX_MIX bivariate Normals given by their lower Cholesky factors, or explicit samples.  Per
 * measurement t (kernels: particle_nd_kernel.hpp; the particles are held as [B][2][n], component-major):
 *   L = lower Cholesky factor of S(x_i) in closed form: l_00 = sqrt(S_00), l_10 = S_01 / l_00, l_11 = sqrt(S_11 - l_10^2);
 *   x'_i0 = mu_0(x_i) + l_00 z_i0,  x'_i1 = mu_1(x_i) + l_10 z_i0 + l_11 z_i1;  a pivot (S_00, S_11 - l_10^2) that is negative
 *   or not finite makes both components NaN (zero is legal), as jnp.linalg.cholesky does;
 *   w_i = prod_f lik(kind_f, params_f, y_t[ycol_f], x'_i[component_f]);  nell -= log(mean_i w_i);
 *   cs, v_i, idx_i as in mfs_particle_filter_1d; the one ancestor index gathers both components: x''_i = x'[idx_i];
 *   out_means: mean of x'';  out_covs: population covariance about that mean, entries (0,1) and (1,0) both written.
 *
 * The random stream extends the 1-D statement above: counter = (particle i, step t, tag, draw), key = the halves of seeds[b];
 *   tag 0 (t = 0): draws 0, 1 give the normals z_0, z_1, draw 2 the component uniform u_c; c = #{k : mix_cumw[k] <= u_c} clamped
 *                  to n_mix - 1;  x_i = mix_mean[c] + mix_chol[c] (z_0, z_1)^T
 *   tag 1: draw k is the propagation normal of component k at step t;  tag 2: draw 0 the resampling uniform, as in 1-D.
 * Every normal is z = sqrt(-2 ln U(r0, r1)) cos(2 pi U(r2, r3)) of its own Philox block, so mfs_pf_draws reproduces each one.
 *
 *   model        d = 2, trans_kind MFS_ND_TRANS_GAUSSIAN, 1..MFS_ND_MAX_FACTORS factors of kind Bernoulli-logistic,
 *                Poisson-softplus or Gaussian, ny 1 or 2; coef_batched / lik_batched give one table per replicate
 *   n, T, B      particles (1 .. MFS_PF_MAX_PARTICLES), measurements, replicates;  resampling MFS_RESAMPLE_*
 *   seeds [B];  n_mix 1 .. MFS_PF_MAX_MIX with mix_cumw [n_mix], mix_mean [n_mix][2], mix_chol [n_mix][2][2] (lower factors,
 *   computed on the host; entry [0][1] is not read), or n_mix = 0 and init_samples [n][2] or [B][n][2] (init_batched);
 *   ys [B][T][ny]
 *   out_samples  [B][T][n][2] or NULL: with NULL nothing of size B T n exists on the device either
 *   out_means [B][T][2];  out_covs [B][T][2][2];  out_nell [B]
 *   out_first_nan [B] or NULL: the first step whose sum of weights is zero or not finite, -1 if none.  A NaN particle makes the
 *                sum NaN.  That replicate is NaN from that step on -- samples, summaries and nell -- and only that replicate;
 *                no index leaves [0, n - 1].
 * At most five launches per step and no atomics: every sum runs in an order fixed by n alone (block totals in index order,
 * covariance partials per segment of 4096 particles in index order), so two calls with the same inputs return the same bits,
 * and replicate b of a batch returns the bits of a B = 1 call with seeds[b].
 * MFS_EINVAL: a model that is not MFS_ND_TRANS_GAUSSIAN, n, T or B < 1, an unknown resampling code, n_factors, ny, a factor's
 * kind, component or column out of range, n_mix outside 0 .. 8, n_mix = 0 without init_samples, a mixture factor whose diagonal
 * is not finite and > 0, a NULL required buffer.  MFS_EUNSUPPORTED: n > MFS_PF_MAX_PARTICLES, d != 2.  MFS_ENOMEM: the work
 * buffers cannot be had.
 */
int mfs_particle_filter_nd(const mfs_model_nd* model, int n, int T, int B, int resampling, const uint64_t* seeds,
                           int n_mix, const double* mix_cumw, const double* mix_mean /* [n_mix][2] */,
                           const double* mix_chol /* [n_mix][2][2], lower factor, computed on the host */,
                           const double* init_samples /* [n][2] or [B][n][2] */, int init_batched,
                           const double* ys /* [B][T][ny] */,
                           double* out_samples /* [B][T][n][2] or NULL */, double* out_means /* [B][T][2] */,
                           double* out_covs /* [B][T][2][2] */, double* out_nell /* [B] */,
                           int32_t* out_first_nan /* [B] */, int device, void* stream);

/*
 * ---- Gaussian filters: Gauss--Hermite / cubature sigma-point filter and extended Kalman filter, host pointers ----------
 * Replaces sgp_filter and ekf (mfs/classical_filters_smoothers/gfs.py:503-551, 317-362) as the drivers run them
 * (dardel/benes_bernoulli, dardel/parameter_estimation/ghf_ekf.py, dardel/prey_predator/ghf_ekf.py), for B replicates at once
 * and a scalar measurement (dy = 1).  The two callables of the reference become descriptors: state_cond_m_cov is the Normal
 * closure of the model (MFS_TRANS_GAUSSIAN: mu(x), var(x); MFS_ND_TRANS_GAUSSIAN: mu(x), S(x)), measurement_cond_m_cov the mean
 * h(x) and variance Xi(x) of the likelihood kind: Bernoulli-logistic (p, p (1 - p)), Poisson-softplus (rate, rate), Gaussian
 * (l0 x + l1, l2).  The whole time loop is one launch (kernels: gaussfilter_kernel.hpp).  Per measurement y_t:
 *
 *   MFS_GF_SIGMA_POINT, with points xi_i and weights w_i (SigmaPoints of the reference; any rule of 1 .. MFS_GF_MAX_POINTS points):
 *     chi_i = m + L xi_i, L the lower Cholesky factor of P;  mp = sum w_i mu(chi_i);
 *     Pp = sum w_i (mu mu^T + S(chi_i)) - mp mp^T;  chi_i = mp + Lp xi_i redrawn from (mp, Pp);
 *     pred = sum w h;  S = sum w (h^2 + Xi) - pred^2;  C = sum w chi h - mp pred;  K = C / S
 *   MFS_GF_EKF (xi, w, n_points ignored), with analytic Jacobians F = d mu / d x at m and H = d h / d x at mp:
 *     mp = mu(m);  Pp = F P F^T + S(m);  pred = h(mp);  S = H Pp H^T + Xi(mp);  K = Pp H^T / S
 *   both:  m = mp + K (y - pred);  P = Pp - K K^T S;  nell += ((y - pred)^2 / S + log(2 pi S)) / 2
 *
 *   model        1-D: trans_kind MFS_TRANS_GAUSSIAN; coef_batched / lik_batched give one table per replicate (a theta grid).
 *                d = 2: d = 2, trans_kind MFS_ND_TRANS_GAUSSIAN, one likelihood factor on one state component, ny = 1;
 *                lik_batched allowed, coef_batched not
 *   xi, w        [n_points] ([n_points][2] for d = 2), [n_points];  T, B measurements, replicates
 *   m0, v0       [1] or [B] (init_batched);  d = 2: m0 [2], P0 [2][2] or [B][2], [B][2][2] (the lower triangle of P0 is read)
 *   ys           [B][T]
 *   out_means    [B][T] ([B][T][2]);  out_vars [B][T] (out_covs [B][T][2][2]);  either may be NULL
 *   out_nells    [B][T]: the running sum, as the reference's scan returns it
 *   out_first_nan [B] or NULL.  The reference's Cholesky of a matrix that is not positive definite is NaN: a replicate whose
 *                Cholesky pivot is negative or not finite (zero is legal), or whose S is not finite and > 0, is NaN in every
 *                output from that step on, and that step is its first_nan (-1 if none).  Only that replicate.  The EKF takes
 *                no Cholesky, so only the rule on S applies to it.  A measurement y_t that is not finite (NaN or +-inf) poisons
 *                its replicate at step t in the same way, in both methods.  At d = 2 the zero that is legal is the second
 *                pivot (P = diag(v, 0)): a zero first pivot divides P01 by zero, and that step is the replicate's first_nan.
 * A group of L lanes owns a replicate, L the smallest power of two >= n_points, at most 64 (one lane for the EKF); the sums are
 * butterfly reductions in an order fixed by n_points alone and there are no atomics: two calls with the same inputs return the
 * same bits, and replicate b of a batch returns the bits of a B = 1 call.
 * MFS_EINVAL: a model outside the Gaussian family, an unknown method, T or B < 1, a NULL required buffer, an unknown u-map or
 * likelihood kind.  MFS_EUNSUPPORTED: n_points outside 1 .. MFS_GF_MAX_POINTS (sigma-point method), d != 2, more than one
 * likelihood factor, a factor of both components, ny != 1, coef_batched at d = 2.
 */
#define MFS_GF_SIGMA_POINT 0
#define MFS_GF_EKF 1
#define MFS_GF_MAX_POINTS 256
int mfs_gaussian_filter_1d(const mfs_model_1d* model, int method, int n_points, const double* xi, const double* w, int T, int B,
                           const double* m0, const double* v0, int init_batched, const double* ys, double* out_means,
                           double* out_vars, double* out_nells, int32_t* out_first_nan, int device, void* stream);
int mfs_gaussian_filter_nd(const mfs_model_nd* model, int method, int n_points, const double* xi, const double* w, int T, int B,
                           const double* m0, const double* P0, int init_batched, const double* ys, double* out_means,
                           double* out_covs, double* out_nells, int32_t* out_first_nan, int device, void* stream);

/*
 * ---- multi-GPU: one process per GPU, replicates sharded, NLL all-gather over RCCL / xGMI -----------------------
 * The reference has no multi-device code (its Monte-Carlo runs are separate OS processes,
 * dardel/run_benes_bernoulli_mf.sh:26-31); replicates share nothing, so the data path needs no collective and the
 * only exchange is one ncclAllGather of the per-replicate negative log-likelihoods after the kernel
 * (SURVEY.md section 8e).  Rank 0 creates an id, the host side distributes its 128 bytes by any means
 * (mfs_amd/dist.py sends it over its TCP control plane, mfs_amd/rdzv.py), every rank calls mfs_comm_init.
 */
typedef struct mfs_rccl_id { char bytes[128]; } mfs_rccl_id; /* = ncclUniqueId */
int mfs_comm_unique_id(mfs_rccl_id* id);
int mfs_comm_init(void** comm, const mfs_rccl_id* id, int nranks, int rank, int device);
/* d_send [count], d_recv [nranks * count], DEVICE pointers, rank-major; enqueued on `stream` */
int mfs_allgather_nell(void* comm, const double* d_send, double* d_recv, uint64_t count, void* stream);
int mfs_comm_destroy(void* comm);
int mfs_memcpy_d2d(void* dst, const void* src, uint64_t bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MFS_HIP_H */
