/*
 * nngp.h -- C-ABI of libnngp_hip.so, the MI355X (gfx950) hot path of nnGParareal.
 *
 * The reference (Python + jax, /root/reference) has no native code: its hot path is three
 * duck-typed Python plugin calls that a process pool fans out:
 *
 *   1. propagator  SolverAbstr.run_F/run_G(t0, t1, u0) -> u1      solver.py:29-69, 86-107
 *                  (Parareal fans run_F over slices: parareal.py:310-315)
 *   2. model       NNGP_p.predict(new_x, ...) -> preds[d]          models.py:171-226
 *                  (kNN :177-179, n*9*R Nelder-Mead fits of the -LML :185-202, 228-260,
 *                   argmin :207-215, posterior mean :162-168, 217)
 *   3. executor    pool.map(fn, *iterables)                        parareal.py:16-24, 58-64
 *
 * Each entry point below replaces one of those call sites with ONE stream-ordered launch
 * sequence on the GPU.  Python binds them through ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - All array arguments are DEVICE pointers (hipMalloc / torch.cuda memory) unless the
 *     parameter name ends in `_host`.  Layouts are row-major: states are [n_slices][d], which
 *     is exactly the reference's u[i, :, k] slice for consecutive i.
 *   - Every call is asynchronous on `stream` (a hipStream_t; NULL = default stream) and
 *     returns 0 on success, a negative NNGP_E_* code otherwise; nngp_last_error() gives a
 *     thread-local message.  Nothing here allocates per call except the library's own
 *     grow-only device workspace (nngp_predict), so steady-state calls never hit hipMalloc.
 *   - Arithmetic is IEEE fp64 throughout (the reference runs jax with x64 enabled,
 *     e.g. models.py:8, RK.py:13).  Kernels are built with -ffp-contract=off so that every
 *     add/mul rounds exactly where the reference's does.
 */
#ifndef NNGP_H_
#define NNGP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NNGP_ABI_VERSION 1

/* error codes */
#define NNGP_OK 0
#define NNGP_E_ARG (-1)       /* invalid argument (shape, enum, null pointer)            */
#define NNGP_E_HIP (-2)       /* a HIP runtime call failed                               */
#define NNGP_E_UNSUPPORTED (-3) /* valid in the reference but not (yet) on this path     */

/* Vector fields.  Reference: systems.py (modern) and new_lib.Systems (legacy twin). */
enum nngp_system_kind {
    NNGP_SYS_LORENZ = 0,            /* systems.py:225-247                                  */
    NNGP_SYS_HOPF = 1,              /* systems.py:140-172 (non-autonomous Hopf), param[0]=maxtime */
    NNGP_SYS_THOMAS_LABYRINTH = 2,  /* systems.py:250-288                                  */
    NNGP_SYS_FHN_ODE = 3,           /* systems.py:80-106                                   */
    NNGP_SYS_ROSSLER = 4,           /* systems.py:109-137                                  */
    NNGP_SYS_BRUSSELATOR = 5,       /* systems.py:202-222                                  */
    NNGP_SYS_DBL_PEND = 6,          /* systems.py:175-199                                  */
    NNGP_SYS_BURGERS = 7,           /* systems.py:402-459, nx = d, param[0] = nu           */
    NNGP_SYS_FHN_PDE = 8,           /* systems.py:291-398, nx = d_x, d = 2*d_x*d_x         */
    NNGP_SYS_DIFFREACT = 9,         /* systems.py:463-577, nx = d_x (3..32), d = 2*nx*nx, state u | v,
                                       param[0..2] = Du, Dv, k; zero-flux walls             */
    NNGP_SYS_POLY = 10,             /* a caller-defined polynomial field (the reference's extension point,
                                       a subclass of ODE: systems.py:23-61), nx = the table's handle
                                       from nngp_poly_create, 1 <= d <= 2048                  */
    NNGP_SYS_FUNC = 11              /* a caller-defined field of monomials over the state and over
                                       elementary-function atoms of it (sin, cos, exp, log, 1/x, sqrt),
                                       nx = the table's handle from nngp_func_create, 1 <= d <= 2048 */
};

/* Explicit Runge-Kutta tableaux, RK.py:30-48 (value = order). */
enum nngp_tableau { NNGP_RK1 = 1, NNGP_RK2 = 2, NNGP_RK4 = 4, NNGP_RK8 = 8 };

/* Step-size convention.
 *   FIXED:    h = (t1 - t0)/steps for every step          RK.run_get_last, RK.py:101-109
 *   LINSPACE: h_n = t[n+1] - t[n], t = np.linspace(t0, t1, steps+1)
 *             RK.run / legacy new_lib.RK (RK.py:91-99, new_lib.py:87-137) -- the convention
 *             of every published scalability run.
 * NNGP_STEP_CONTRACT (a flag OR-ed onto either mode; opt-in, not a reference behaviour): run the
 *   propagator's second code object, compiled with a*b+c contracted to fma.  Fewer fp64
 *   instructions per step (the fine sweep is instruction-issue-bound), results no longer bitwise
 *   the reference's rounding order: per-slice end states agree to <= 1e-12 relative on the
 *   test schedules (tests/test_gpu_contract.py).  Every other entry point ignores it.        */
enum nngp_step_mode { NNGP_STEP_FIXED = 0, NNGP_STEP_LINSPACE = 1, NNGP_STEP_CONTRACT = 16 };

/* One ODE/PDE right-hand side, optionally wrapped by the '-11' normalisation of
 * ODE.get_vector_field (systems.py:32-44, utils.py:14-33):
 *     f_n(u) = f((u+1)/2*(mx-mn) + mn) * (2/(mx-mn))                                       */
typedef struct nngp_system {
    int32_t kind;        /* enum nngp_system_kind                                         */
    int32_t d;           /* state dimension                                               */
    int32_t nx;          /* grid points per axis (Burgers: d; FHN_PDE, DIFFREACT: d_x); POLY, FUNC:
                            the table's handle; else 0                                    */
    int32_t normalized;  /* 0: identity, 1: '-11' wrapper                                 */
    double param[4];     /* HOPF: [0]=maxtime (tspan[1]); BURGERS: [0]=nu; DIFFREACT: [0..2]=Du, Dv, k;
                            else unused                                                   */
    const double *norm;  /* DEVICE [3*d] = mn | (mx-mn) | 2/(mx-mn), or NULL if identity   */
} nngp_system;

/* ---- library ---------------------------------------------------------------------------- */
int nngp_abi_version(void);
const char *nngp_last_error(void);
/* Number of visible HIP devices (0 when no GPU); never fails. */
int nngp_device_count(void);

/* ---- 1. fine / coarse propagator --------------------------------------------------------
 * Replaces: SolverRK.run_F / run_G for every slice of one Parareal iteration
 *           (solver.py:86-107 via RK.run_get_last RK.py:101-109 / _RK_jax_last RK.py:146-174),
 *           as fanned out by pool.map(solver.run_F_timed, ...) at parareal.py:310-315, and the
 *           legacy RK_last (new_lib.py:57-69, 939-945).
 * Integrates n_slices independent initial values u0[i] from t0[i] to t1[i] with `steps`
 * steps of tableau `tableau`; writes the end states to uF[i].  The paging quirk of
 * solver.py:86-99 is a host-side loop over pages calling this once per page.
 * t0, t1: DEVICE [n_slices]; u0, uF: DEVICE [n_slices][sys->d]; uF may alias u0.          */
int nngp_rk_batch(const nngp_system *sys, int tableau, int step_mode, int n_slices,
                  const double *t0, const double *t1, int64_t steps, const double *u0,
                  double *uF, void *stream);

/* Legacy global-grid variant (the legacy driver's initial coarse sweep, new_lib.py:902-906,
 * integrates ONE np.linspace(g0, g1, gsteps+1) grid and sub-samples it at slice boundaries).
 * Slice i performs grid steps j0[i] .. j0[i]+steps-1 of the grid (g0[i], g1[i], gsteps):
 * t[j] = j*((g1-g0)/gsteps) + g0, t[gsteps] = g1, h = t[j+1]-t[j].  j0: DEVICE int64 [n].  */
int nngp_rk_batch_grid(const nngp_system *sys, int tableau, int n_slices, const double *g0,
                       const double *g1, int64_t gsteps, const int64_t *j0, int64_t steps,
                       const double *u0, double *uF, void *stream);

/* Sampled trajectory of every slice in ONE launch (replaces SolverRK.run_F_full / run_G_full,
 * solver.py:109-113 -> RK.run RK.py:91-99, as called per slice by Parareal._build_cont_traj,
 * parareal.py:500-508).  Slice i integrates `steps` steps from u0[i] exactly as nngp_rk_batch
 * would with the same tableau and step_mode, and writes
 *     traj[i][0] = u0[i],   traj[i][p] = state after min(p*every, steps) steps,  p = 1..n_out-1,
 *     n_out = 1 + ceil(steps / every)
 * so every row is bitwise what nngp_rk_batch returns after that many steps of the same grid, and
 * with NNGP_STEP_FIXED the last row is bitwise its end state.  Both step modes, with and without
 * NNGP_STEP_CONTRACT; the paging quirk does not apply (RK.run never pages).  Each shape runs on
 * the kernel form its nngp_rk_batch launch would use.
 * traj: DEVICE [n_slices][n_out][sys->d], must not alias u0.  every >= 1. */
int nngp_rk_traj(const nngp_system *sys, int tableau, int step_mode, int n_slices,
                 const double *t0, const double *t1, int64_t steps, int64_t every,
                 const double *u0, double *traj, void *stream);

/* Adaptive fine propagator (replaces SolverScipy.run_F -> scipy.integrate.solve_ivp(f, [t0, t1],
 * u0, method, t_eval=(t1,), max_step=(t1-t0)/Nf, **kwargs), solver.py:138-145, for every slice of
 * one Parareal iteration).  Slice i integrates u0[i] from t0[i] to t1[i] (forward only) with the
 * embedded pair `method` under scipy's step-size control -- rtol, atol scalars, max_step =
 * (t1[i]-t0[i])/nf, first_step = 0 to select the initial step as scipy does (a first_step beyond
 * a slice's length is the caller's to refuse, as validate_first_step does; here it is clipped to
 * max_step) -- and writes y_new of its last accepted step to uF[i].  The arithmetic is a fully
 * specified operation order (tests/adaptive_ref.py), not scipy's BLAS / libm one:
 * step counts equal scipy's on the recorded cases and end states agree to ~1e-13 relative.
 * A slice stops after max_attempts attempted steps, whatever its arithmetic does.
 * stats: DEVICE int64 [n_slices][4] = status, nfev, accepted steps, rejected steps, or NULL;
 *   status 0 = reached t1, 1 = step size below min_step = 10*|nextafter(t, inf) - t|,
 *   2 = max_attempts reached.  On a non-zero status uF[i] is the last accepted state.  A slice
 *   with t1 <= t0 takes no step (uF[i] = u0[i], status 0).
 * Stream-ordered, no host synchronisation; uF may alias u0; n_slices = 0 is a no-op.  Exact build
 * only: there is no NNGP_STEP_CONTRACT form.  Field systems take d <= 2048.
 * NNGP_E_ARG before any HIP call: unknown method; nf < 1; rtol <= 0, atol < 0 or a non-finite
 * tolerance; first_step < 0; max_attempts < 1; an unknown or destroyed NNGP_SYS_POLY or
 * NNGP_SYS_FUNC handle.
 * t0, t1: DEVICE [n_slices]; u0, uF: DEVICE [n_slices][sys->d].                              */
enum nngp_adaptive_method { NNGP_RK23 = 23, NNGP_RK45 = 45 };
int nngp_rk_adaptive(const nngp_system *sys, int method, int n_slices,
                     const double *t0, const double *t1, int64_t nf,   /* max_step = (t1-t0)/nf */
                     double rtol, double atol, double first_step,      /* 0 = choose */
                     int64_t max_attempts, const double *u0, double *uF,
                     int64_t *stats /* DEVICE [n][4] = status, nfev, accepted, rejected; or NULL */,
                     void *stream);

/* Vector field evaluation f_n(u) for n states (what ODE.get_vector_field() returns as a
 * callable, systems.py:32-44).  u, out: DEVICE [n][sys->d].                                 */
int nngp_rhs_batch(const nngp_system *sys, int n, const double *u, double *out, void *stream);

/* Polynomial vector fields (NNGP_SYS_POLY): the right-hand side as data, for systems that are not
 * one of the compiled kinds (the reference's user subclasses ODE and writes _f_np / _f_jax,
 * systems.py:23-61).  A table has d rows; row c is the ordered list of the terms
 * row_ptr[c] .. row_ptr[c+1]-1, term t = coef[t] * u[idx[t][0]] * u[idx[t][1]] * u[idx[t][2]] with
 * -1 for a factor that is not there (only after the real ones: degree 0..3).  The arithmetic is
 * fixed: a term is coef times its factors left to right, one rounding per
 * multiply; a row is its first term plus the following ones in list order; a row without terms is
 * +0.0.  All arguments are HOST arrays, copied; nothing is launched.
 *   Checked here, before any HIP call (the kernels trust a registered table): 1 <= d <= 2048,
 *   0 <= n_terms <= 1048576, row_ptr[0] = 0, non-decreasing, row_ptr[d] = n_terms, every index -1 or
 *   in [0, d) with no -1 before a real index, every coefficient finite.
 * *handle_out >= 1 goes into nngp_system.nx of a system of kind NNGP_SYS_POLY with the same d
 * (param is unused; the '-11' wrapper applies as to every kind).  Every propagator entry point
 * and nngp_rhs_batch refuses an unknown or destroyed handle and another d with NNGP_E_ARG.  The
 * device copy is uploaded per device on first use and kept.  nngp_poly_destroy frees a table (its
 * slot may be handed out again); nngp_shutdown frees all of them.                             */
int nngp_poly_create(int d, int n_terms, const int32_t *row_ptr_host, const double *coef_host,
                     const int16_t *idx_host, int32_t *handle_out);
int nngp_poly_destroy(int32_t handle);

/* Fields with elementary-function atoms (NNGP_SYS_FUNC): a polynomial table whose monomials range
 * over the extended vector w = [u_0 .. u_{d-1}, atom_0 .. atom_{n_atoms-1}].  Atom q is fn(x) of
 *     x = a*u[i];   if j >= 0: x = x + c*u[j];   if has_b: x = x + b
 * one rounding per operation in that order (an absent part is not an added 0.0), with fn one of
 * enum nngp_func_fn: the library's own sine (the one NNGP_SYS_THOMAS_LABYRINTH uses), cosine, exp
 * and log -- fully specified routines, the same bits on every device -- and the IEEE 1.0/x and
 * sqrt(x).  Atoms read the state only.  A domain error gives what the routine gives (NaN, inf).
 * Terms, rows and their arithmetic are nngp_poly_create's, the term indices in [0, d + n_atoms);
 * with n_atoms = 0 the kind is NNGP_SYS_POLY bit for bit.  The contracted build
 * (NNGP_STEP_CONTRACT) may fuse the atom's argument and the row sum.  Restated in
 * tests/func_ref.py.  All arguments are HOST arrays, copied; nothing is launched.
 *   Checked here, before any HIP call (the kernels trust a registered table): 1 <= d <= 2048,
 *   0 <= n_atoms <= 2048, 0 <= n_terms <= 1048576; per atom fn in 1..6, i in [0, d), j = -1 or in
 *   [0, d), has_b 0 or 1, a, c and b finite; row_ptr as for nngp_poly_create; every term index -1
 *   or in [0, d + n_atoms) with no -1 before a real index; every coefficient finite.
 * *handle_out >= 1 goes into nngp_system.nx of a system of kind NNGP_SYS_FUNC with the same d.
 * Every propagator entry point and nngp_rhs_batch refuses an unknown or destroyed handle and
 * another d with NNGP_E_ARG.  The device copy is uploaded per device on first use and kept.
 * nngp_func_destroy frees a table (its slot may be handed out again); nngp_shutdown frees all. */
enum nngp_func_fn { NNGP_FN_SIN = 1, NNGP_FN_COS = 2, NNGP_FN_EXP = 3, NNGP_FN_LOG = 4, NNGP_FN_RECIP = 5,
                    NNGP_FN_SQRT = 6 };
typedef struct nngp_func_atom {
    int32_t fn;          /* enum nngp_func_fn                                             */
    int32_t i, j;        /* state indices; j = -1: no second component                    */
    int32_t has_b;       /* 1: the offset b is added, 0: it is absent                     */
    double a, c, b;      /* c is unused when j = -1, b when has_b = 0 (both still finite) */
} nngp_func_atom;
int nngp_func_create(int d, int n_atoms, const nngp_func_atom *atoms_host, int n_terms,
                     const int32_t *row_ptr_host, const double *coef_host, const int16_t *idx_host,
                     int32_t *handle_out);
int nngp_func_destroy(int32_t handle);

/* Elementwise  out = (a - b) + c   (c may be NULL: out = a - b), n doubles, DEVICE.
 *   Parareal update with the classic model: u = (uF_prev - uG_prev) + uG_new
 *   (models.py:82-83 + parareal.py:382); training targets D = uF - uG (parareal.py:337).     */
int nngp_parareal_update(int64_t n, const double *a, const double *b, const double *c,
                         double *out, void *stream);

/* ---- 2. nnGP correction -----------------------------------------------------------------
 * kNN (models.py:177-179): indices of the m rows of X[rows][d] nearest to q[d] in squared
 * euclidean distance, ascending, ties broken by row index.  idx_out: DEVICE int32 [m];
 * dist_out: DEVICE [m] or NULL.  Requires 1 <= m <= rows.                                   */
int nngp_knn(const double *X, int64_t rows, int d, const double *q, int m, int32_t *idx_out,
             double *dist_out, void *stream);

/* Batched hyper-parameter fits, replacing pool.map(NNGP_p._get_opt_par, ...) at
 * models.py:197-202 -> opt_theta (models.py:254-260) -> scipy Nelder-Mead on log_lik
 * (models.py:240-252).  Fit f minimises -LML(theta | xm, ym[:, coord[f]], 10**jitter) with
 * jitter = jitter_exp_host[jitter_idx[f]], starting from theta0[f], by the rules of scipy's
 * _minimize_neldermead (rho=1, chi=2, psi=0.5, sigma=0.5, 5% initial simplex, xatol/fatol stop,
 * maxiter = maxfev).  A NaN -LML (failed Cholesky) counts as +inf (models.py:250-251).
 *   xm, ym: DEVICE [m][d]; coord, jitter_idx: DEVICE int32 [n_fits]; theta0: DEVICE [n_fits][2];
 *   jitter_exp_host: HOST [n_jitter] exponents (e.g. -20..-12, models.py:186);
 *   theta_out: DEVICE [n_fits][2]; fval_out: DEVICE [n_fits]; nfev_out: DEVICE int32 or NULL.
 * Requires 1 <= m <= 64 (fits padded to 8/16/20/24/32/48/64 rows; m > 32 runs 3-4 kernel rows
 * per lane, one wave per workgroup).                                                        */
int nngp_nm_fit_batch(int m, int d, const double *xm, const double *ym, int n_fits,
                      const int32_t *coord, const int32_t *jitter_idx, int n_jitter,
                      const double *jitter_exp_host, const double *theta0, double fatol,
                      double xatol, int maxfev, double *theta_out, double *fval_out,
                      int32_t *nfev_out, void *stream);

/* Posterior mean K(xm, new_x)^T alpha per coordinate c with hyper-parameters theta[c] and
 * jitter 10**jitter_exp_host[jitter_idx[c]] (models.py:162-168, 217).  NaN if the Cholesky
 * fails (jax semantics).  theta: DEVICE [d][2]; jitter_idx: DEVICE int32 [d]; out: DEVICE [d]. */
int nngp_gp_mean(int m, int d, const double *xm, const double *ym, const double *new_x,
                 const double *theta, const int32_t *jitter_idx, int n_jitter,
                 const double *jitter_exp_host, double *out, void *stream);

/* One full correction for one slice = NNGP_p.predict (models.py:171-226) fused:
 * kNN over the training set X/Y[rows][d] at new_x[d], d*n_jitter*n_restarts fits in the
 * reference's product(coord, jitter, restart) order (models.py:186-192) starting from
 * theta0[d*n_jitter*n_restarts][2] (the host replays rng.integers(-8, 0, 2) in that order),
 * per-coordinate first-argmin of fval (models.py:207-215) and the posterior mean.
 *   preds_out = mean;  if bias != NULL also out = preds + bias (parareal.py:382).
 *   fits_out: DEVICE [n_fits][4] = (theta_x, theta_y, fval, nfev) or NULL.
 *   jitter_exp_host: HOST [n_jitter]. All other arrays DEVICE.  Requires 1 <= m <= 64.   */
int nngp_predict(const double *X, const double *Y, int64_t rows, int d, const double *new_x,
                 int m, int n_jitter, const double *jitter_exp_host, int n_restarts,
                 const double *theta0, double fatol, double xatol, int maxfev,
                 double *preds_out, const double *bias, double *out, double *fits_out,
                 void *stream);

/* nngp_predict_batch: n_q INDEPENDENT predictions over one training set as one launch set -- the
 * comparison nnGPs of Figure 2 at every slice's start value, or the learned correction on a grid
 * of states.  Query q is nngp_predict(X, Y, rows, d, Q + q*d, m, ..., theta0 + q*n_fits*2, ...)
 * bit for bit, n_fits = d*n_jitter*n_restarts: one kNN-distance launch, one select (a workgroup
 * per query: the ordered list, y_m, D2 and kd2), all n_q*n_fits fits as one packed launch (the
 * sweep's speculative batch, throughput-shaped) and one launch for every (query, coordinate)
 * arg-min and posterior mean.  A query's bits depend neither on the queries beside it nor on the
 * chunking: the host walks the queries in chunks of
 *     min(65535, max(1, NNGP_PREDICT_BATCH_MAX_FITS / n_fits))
 * on the stream, and the grow-only workspace (dist[nq][rows] | D2 | y_m | kd2 | fits) is sized by
 * the chunk, never by n_q.  No host synchronisation beyond that workspace; n_q = 0 is a no-op.
 *   Q: [n_q][d];  theta0: [n_q][n_fits][2] (query q's draws, nngp_predict's order);
 *   preds_out: [n_q][d] = mean;  bias: [n_q][d] or NULL, out: [n_q][d] = preds + bias -- both or
 *   neither; out may alias bias;
 *   idx_out: int32 [n_q][m], query q's ordered list as nngp_knn gives it, or NULL;
 *   fits_out: [n_q][n_fits][4] = (theta_x, theta_y, fval, nfev), nngp_predict's layout, or NULL.
 *   jitter_exp_host: HOST [n_jitter].  All other arrays DEVICE.
 * NNGP_E_ARG before any HIP call: a NULL required pointer, n_q < 0, m outside 1..min(64, rows),
 * d < 1, n_jitter outside 1..16, n_restarts < 1, maxfev < 1, bias / out given singly.       */
#define NNGP_PREDICT_BATCH_MAX_FITS 262144   /* fits per internal chunk; the sweep's speculation bound */
int nngp_predict_batch(const double *X, const double *Y, int64_t rows, int d,
                       const double *Q, int n_q, int m, int n_jitter, const double *jitter_exp_host,
                       int n_restarts, const double *theta0, double fatol, double xatol, int maxfev,
                       double *preds_out, const double *bias, double *out,
                       int32_t *idx_out, double *fits_out, void *stream);

/* nngp_predict_listed: nngp_predict_batch with each query's kNN replaced by a PRESCRIBED ordered
 * neighbour list, lists_host[q][0..m) (the nntype variants of the reference's NNGP_alt,
 * nnGPara_with_time.py:50-171, choose neighbours by their place in the (interval, iteration) table
 * instead of by distance).  No distance launch and no select: one gather of y_m^T per query, D2 and
 * kd2 per query (a wave per pair where nngp_predict's dispatch uses waves, else a thread per pair;
 * every form gives the same bits), all n_q*n_fits fits as one packed launch and one launch for every
 * (query, coordinate) arg-min and posterior mean, in nngp_predict_batch's chunks.
 *   lists_host: HOST int32 [n_q][m].  Every entry is checked against [0, rows) before any HIP call
 *   and the library uploads the lists itself, so a bad list is NNGP_E_ARG, never a device fault (in
 *   pinned memory the upload is asynchronous: keep it until the stream has passed the call).  A row
 *   may appear more than once; the fits then see what the reference's see on a duplicated row.
 *   Q, theta0, preds_out, bias, out, fits_out and the refusals: as nngp_predict_batch.
 * Contract: where lists_host[q] is what nngp_knn returns for Q[q], query q's preds_out, out and
 * fits_out are nngp_predict's bit for bit. */
int nngp_predict_listed(const double *X, const double *Y, int64_t rows, int d, const double *Q, int n_q,
                        const int32_t *lists_host, int m, int n_jitter, const double *jitter_exp_host,
                        int n_restarts, const double *theta0, double fatol, double xatol, int maxfev,
                        double *preds_out, const double *bias, double *out, double *fits_out,
                        void *stream);

/* nngp_listed_sweep: the sequential sweep of one iteration on prescribed lists: for i = I .. N-1
 *     UG1[i+1] = G(t[i], t[i+1], U1[i])
 *     U1[i+1]  = mean_i(U1[i]) + UG1[i+1],   preds_out[i-I] = mean_i(U1[i])
 * with mean_i the listed prediction on lists_host[i-I] with the draws theta0[i-I].  A list does not
 * depend on the query, so nothing of a fit does: before the chain, for all N-I slices at once, the
 * gather and D2, ONE packed fits launch and ONE launch that prepares every (slice, coordinate)
 * (alpha, the kernel scalars, the factorisation's success).  What is left per slice is G, m
 * distances, d short dot products and the add:
 *   - one-wave form (every ODE kind; Burgers with d = 64k <= 256; exact G): the whole chain is ONE
 *     launch of one 64-lane workgroup.  *g_ms_out is 0 in this form: the G time is not separated.
 *   - launch form (everything else: field kernels, tables, larger Burgers, NNGP_STEP_CONTRACT): per
 *     slice the G launch and one mean launch (for d > 128 a kd2 launch between them); *g_ms_out as
 *     in nngp_elm_sweep.
 * Both forms give the bits of a per-slice loop of nngp_rk_batch, nngp_predict_listed with n_q = 1
 * and the update.  All on `stream`, no host synchronisation beyond the grow-only workspace.
 *   t, U1, UG1 as in nngp_correction_sweep; lists_host: HOST int32 [N-I][m], checked and uploaded as
 *   in nngp_predict_listed; theta0: DEVICE [N-I][n_fits][2]; preds_out: DEVICE [N-I][d] or NULL;
 *   g_ms_out: HOST or NULL.  N <= I is a no-op.  Refusals as nngp_predict_listed. */
int nngp_listed_sweep(const nngp_system *sys, int g_tableau, int g_step_mode, int64_t g_steps,
                      const double *t, int I, int N, double *U1, double *UG1, const double *X,
                      const double *Y, int64_t rows, const int32_t *lists_host, int m, int n_jitter,
                      const double *jitter_exp_host, int n_restarts, const double *theta0, double fatol,
                      double xatol, int maxfev, double *preds_out, float *g_ms_out, void *stream);

/* nngp_predict_range: the coordinates [c0, c1) of nngp_predict (their fits, in the same
 * product order with their own rows of theta0 = the FULL [d*n_jitter*n_restarts][2] draws, and
 * their means) into preds_out [c1-c0]: a rank's share of one prediction when the multi-GPU
 * sweep shards the d*9*R fits by coordinate (parareal.correction_sweep_sharded).
 * Concatenating the ranges gives nngp_predict's preds bit for bit. */
int nngp_predict_range(const double *X, const double *Y, int64_t rows, int d, const double *new_x,
                       int m, int n_jitter, const double *jitter_exp_host, int n_restarts,
                       const double *theta0, int c0, int c1, double fatol, double xatol, int maxfev,
                       double *preds_out, void *stream);

/* ---- 3. the sequential correction sweep of one Parareal iteration ------------------------
 * Replaces the loop parareal.py:359-382 (legacy new_lib.py:990-1012): for i = I .. N-1
 *     UG1[i+1] = G(t[i], t[i+1], U1[i])                     run_G_timed, parareal.py:361
 *     U1[i+1]  = correction(U1[i]) + UG1[i+1]                  parareal.py:367-368, 382
 * with correction = (UF[i+1] - UG[i+1]) for NNGP_MODEL_PARAREAL (models.py:82-83) or the
 * nnGP prediction for NNGP_MODEL_NNGP (= nngp_predict on X/Y[rows][d] with m neighbours,
 * theta0 = the (N-I) predictions' initial thetas back to back, [(N-I)][d*n_jitter*n_restarts][2]).
 * All slice launches are queued on `stream` without host synchronisation.
 *   t: DEVICE [N+1]; U1, UG1: DEVICE [N+1][d] (rows I.. read, rows I+1.. written);
 *   UF, UG: DEVICE [N+1][d] (parareal model; for nngp they enable speculation);
 *   preds_scratch: DEVICE [d] (nngp only);
 *   speculate (nngp): -1 auto, 0 off, 1 on.  Every slice's query is guessed by the classic
 *     Parareal update along the coarse chain and all their fits run as ONE batched launch; a
 *     slice whose actual ordered kNN list equals its guess reuses those fits (bitwise identical:
 *     a fit depends only on the ordered neighbours, coordinate, jitter and theta0), the others
 *     are recomputed in the sweep.  Auto speculates while (N-I)*d*n_jitter*n_restarts <= 262144.
 *     The batch's fits overlap the sweep on a side stream (a hit waits for its own prediction's
 *     fits; NNGP_SPEC_OVERLAP=0 serialises them); the call returns after both have drained.
 *   spec_hits_out: HOST, number of slices served by the speculative batch, or NULL;
 *   g_ms_out: HOST, total device time of the G launches (ms), or NULL (no timing events).
 * With NNGP_CHAIN=1, speculation on, an ODE or Burgers (d = 64k <= 256) system, exact G and m <= 24, the runs
 * of hit slices go through ONE persistent cooperative kernel (G, kNN, hit check, arg-min, mean
 * and update per slice, grid barriers between the phases; the host takes over at each miss):
 * bitwise the launch chain.  Opt-in (NNGP_CHAIN=1): measured not faster than the launch chain
 * on MI355X, so the launch chain stays the default.                        */
#define NNGP_MODEL_PARAREAL 0
#define NNGP_MODEL_NNGP 1
/* NNGP_MODEL_GPFULL: the full-data GP posterior mean (GPjax_p.predict, models.py:456-462) with
 * Y = alpha DEVICE [d][rows] and theta0 = coefficients DEVICE [d][2] = (-0.5/sigma_x^2, sigma_y^2)
 * from nngp_gpfull_fit/nngp_gpfull_lml; m, n_jitter, jitter_exp_host, n_restarts, fatol, xatol,
 * maxfev, preds_scratch and speculate are unused. */
#define NNGP_MODEL_GPFULL 2
int nngp_correction_sweep(const nngp_system *sys, int g_tableau, int g_step_mode, int64_t g_steps,
                          const double *t, int I, int N, double *U1, double *UG1, const double *UF,
                          const double *UG, int model, const double *X, const double *Y, int64_t rows,
                          int m, int n_jitter, const double *jitter_exp_host, int n_restarts,
                          const double *theta0, double fatol, double xatol, int maxfev,
                          double *preds_scratch, int speculate, int32_t *spec_hits_out, float *g_ms_out,
                          void *stream);

/* Counters of the fused correction chain since the library was loaded (this process): kernel
 * launches, and slices it completed (G through the update) -- the rest of the sweep's slices were
 * misses finished by the host's fits.  Returns launches; *slices_out (HOST, optional). */
int64_t nngp_chain_stats(int64_t *slices_out);

/* Sweeps (this process) that were run a second time with the speculative batch serialised
 * because a hit slice's wait for the overlapped batch timed out (NNGP_SPEC_WAIT_US, default 2 s;
 * the first pass wrote nothing for that slice, and the rerun gives the same bits).            */
int64_t nngp_sweep_late_reruns(void);

/* Drains the device and releases every resource the library holds (workspaces, side streams,
 * events, host-mapped flags); the next call re-creates what it needs.  Registered with atexit
 * by the Python package, so none of them is left to the HIP runtime's process-exit teardown.
 * (No reference counterpart: the reference holds no device resources.)  Returns 0.
 * Threading: the library serves one host thread per process (the reference's host loop is
 * single-threaded, parareal.py); nngp_shutdown must not run while another thread is inside a
 * library call. */
int nngp_shutdown(void);

/* ---- 4. full-data GParareal (models.GPjax_p, models.py:273-473) ------------------------------
 * The training set X, Y: DEVICE [rows][d], 1 <= rows <= 46 000 (32-bit offsets inside a matrix;
 * the scratch is rows^2 doubles for D^2 plus (rows+1)^2 per point factored together, in slabs of
 * <= NNGP_GPF_SLAB_MB, default 32 GB, but at least one point; up to 7 936 rows the alpha solve
 * keeps its vector in LDS, past that in its output row).  The factor is a left-looking Cholesky
 * on 64-column panels.  K = sigma_y^2 exp(-0.5/sigma_x^2 D^2) + 10^jitter I over
 * ALL rows (kernel_np / _fit_gp_np, models.py:300-312), theta = (sigma_x, sigma_y) in linear
 * units.  Points and fits are batched: one blocked Cholesky per point.
 *
 * nngp_gpfull_lml: -LML of n_pts points (GPjax_p.log_lik, models.py:321-327; +inf when the
 * Cholesky fails).  coord, jitter_exp, theta [n_pts][2], fval_out: HOST.  alpha_out: DEVICE
 * [n_pts][rows] = L^-T L^-1 y (the posterior weights _predict uses, models.py:446-451) or NULL. */
int nngp_gpfull_lml(const double *X, int64_t rows, int d, const double *Y, int n_pts,
                    const int32_t *coord, const double *jitter_exp, const double *theta,
                    double *fval_out, double *alpha_out, void *stream);

/* nngp_gpfull_factor: a TEST AND DIAGNOSTIC entry with no reference call site (the reference never
 * exposes its Cholesky factor).  nngp_gpfull_lml's arguments and results, computed by the same
 * launches under the same knobs and slab chunking (no kernel and no arithmetic of its own), plus
 * copies of what they leave behind, all DEVICE:
 *   factor_out [n_pts][rows+1][rows+1]: per point the factored matrix [K; y^T].  ONLY the lower
 *              triangle of rows 0..rows-1 (L, diagonal included) and columns 0..rows-1 of row
 *              `rows` (z^T = (L^-1 y)^T) are defined; everything else, and every entry of a point
 *              whose fail flag is set, is unspecified.
 *   fail_out   [n_pts] int32: 1 where a pivot was not > 0 (fval_out is then +inf), else 0.
 *   d2_out     [rows][rows] = cdist(X, X, 'sqeuclidean'), or NULL. */
int nngp_gpfull_factor(const double *X, int64_t rows, int d, const double *Y, int n_pts,
                       const int32_t *coord, const double *jitter_exp, const double *theta,
                       double *fval_out, double *alpha_out, double *factor_out, int32_t *fail_out,
                       double *d2_out, void *stream);

/* nngp_gpfull_fit: n_fit Nelder-Mead fits (GPjax_p.opt_theta, models.py:329-335: scipy NM,
 * fatol/xatol, maxiter = maxfev) of -LML for (coord[f], jitter_exp[f]) from theta0[f], all fits
 * advancing together, one batched evaluation per round; replaces pool.map(_get_opt_par, ...)
 * in GPjax_p._train (models.py:376-407) and _train_coord_rnd (:352-374).  All arrays HOST
 * except X, Y.  theta_out [n_fit][2], fval_out [n_fit], nfev_out [n_fit] or NULL, rounds_out
 * (number of evaluation rounds) or NULL. */
int nngp_gpfull_fit(const double *X, int64_t rows, int d, const double *Y, int n_fit,
                    const int32_t *coord, const double *jitter_exp, const double *theta0,
                    double fatol, double xatol, int maxfev, double *theta_out, double *fval_out,
                    int32_t *nfev_out, int32_t *rounds_out, void *stream);

/* nngp_gpfull_mean: posterior means of all d coordinates at q (GPjax_p.predict -> _predict,
 * models.py:441-462): out[j] = sum_i sigma_y^2 exp(c cdist(x_i, q)) alpha[j][i] (+ bias[j]).
 * coef DEVICE [d][2] = (-0.5/sigma_x^2, sigma_y^2), alpha DEVICE [d][rows]; bias may be NULL. */
int nngp_gpfull_mean(const double *X, int64_t rows, int d, const double *q, const double *coef,
                     const double *alpha, const double *bias, double *out, void *stream);

/* ---- 5. multi-GPU: one RCCL communicator per process (one process per GPU) -------------------
 * Replaces the reference's task farm across MPI ranks (parareal.py:310-315, F over slices;
 * models.py:197-202, fits over the pool; launched as `srun ... mpi4py.futures`, Hopf.py:43-46) with
 * the two exchanges of SURVEY.md §8e.  RCCL is resolved at run time (the process's loaded
 * librccl.so.1 -- torch's -- else the system's), so the library loads without it; every call
 * below returns NNGP_E_UNSUPPORTED when it is absent.
 * nngp_comm_unique_id: rank 0 creates the id (NNGP_COMM_UID_BYTES bytes, HOST), the caller
 *   broadcasts it (e.g. torch.distributed.broadcast_object_list); nngp_comm_init: every rank, on
 *   its device (collective); nngp_comm_size: (ranks, rank) of the live communicator, (0, -1) if
 *   none, and NNGP_E_HIP once the watchdog has aborted it; nngp_comm_destroy: releases it
 *   (nngp_shutdown does too); nngp_comm_available: resolves RCCL only (NNGP_OK or
 *   NNGP_E_UNSUPPORTED) -- the every-rank check before rank 0 alone creates the id.
 * Deadline (NNGP_COMM_TIMEOUT_S, default 600 s): nngp_comm_init is RCCL's non-blocking init polled
 *   to the deadline -- a rank whose peers never arrive aborts (ncclCommAbort) and returns
 *   NNGP_E_HIP; every collective is bracketed by two events that a watchdog thread checks, and one
 *   that has not finished the deadline after its stream reached it aborts the communicator (RCCL's
 *   kernels return, the stream drains, later calls return NNGP_E_HIP).                          */
#define NNGP_COMM_UID_BYTES 128
int nngp_comm_available(void);
int nngp_comm_unique_id(void *uid_out);
int nngp_comm_init(int nranks, int rank, const void *uid);
int nngp_comm_size(int *nranks_out, int *rank_out);
int nngp_comm_destroy(void);

/* All-gather of equal [per_rank_elems] fp64 blocks in rank order, recv = [nranks][per_rank_elems]
 * (DEVICE; send may be recv + rank*per_rank_elems, in place): the ONE collective of a Parareal
 * iteration -- the fine end states of every rank's contiguous slice block (parareal.py:310-315's
 * gather), stream-ordered on `stream`.                                                          */
int nngp_allgather_states(const double *send, double *recv, size_t per_rank_elems, void *stream);

/* nngp_correction_sweep for NNGP_MODEL_NNGP with every prediction's d*n_jitter*n_restarts fits
 * sharded by coordinate over the communicator's ranks (rank r fits coordinates
 * [r*chunk, min((r+1)*chunk, d)), chunk = ceil(d/nranks)): per slice G (replicated), this rank's
 * coordinates (nngp_predict_range), one in-place all-gather of the predictions, and
 * U1[i+1] = preds + UG1[i+1] -- all on `stream`, no host synchronisation.  Bitwise the unsharded
 * sweep on every rank (same inputs, same theta0 draws).  gather: DEVICE [nranks*chunk] scratch.
 * No speculation (every rank would need the whole batch).                                       */
int nngp_correction_sweep_sharded(const nngp_system *sys, int g_tableau, int g_step_mode, int64_t g_steps,
                                  const double *t, int I, int N, double *U1, double *UG1, const double *X,
                                  const double *Y, int64_t rows, int m, int n_jitter,
                                  const double *jitter_exp_host, int n_restarts, const double *theta0,
                                  double fatol, double xatol, int maxfev, double *gather, float *g_ms_out,
                                  void *stream);

/* Test entry (one GPU): nngp_correction_sweep_sharded on a ONE-rank communicator with this process
 * playing the emulate_ranks >= 1 ranks of the coordinate split in turn (each rank's coordinates into
 * its gather block, no collective).  gather_elems: the length of gather, checked against
 * emulate_ranks * ceil(d / emulate_ranks) before any launch.                                      */
int nngp_correction_sweep_sharded_emulated(const nngp_system *sys, int g_tableau, int g_step_mode,
                                           int64_t g_steps, const double *t, int I, int N, double *U1,
                                           double *UG1, const double *X, const double *Y, int64_t rows, int m,
                                           int n_jitter, const double *jitter_exp_host, int n_restarts,
                                           const double *theta0, double fatol, double xatol, int maxfev,
                                           double *gather, size_t gather_elems, int emulate_ranks,
                                           float *g_ms_out, void *stream);

/* ---- 6. ELM correction (RandNet-Parareal; models.ELM / ELM_base, models.py:476-554) -----------
 * A random-weights network on the m nearest neighbours.  Weights (drawn on the host exactly as
 * ELM_base.__init__ / _init_obj do, models.py:481-504, C already multiplied by R, :524):
 *   bias_h DEVICE [res_size], C DEVICE [res_size][n_poly], n_poly = 1 + d + (degree == 2 ? d(d+1)/2 : 0),
 *   the columns in sklearn's PolynomialFeatures(degree) order: 1, x_0 .. x_{d-1}, x_i x_j for i <= j.
 * Supported: degree 1 or 2, 1 <= res_size <= 1024, 1 <= d <= 8192, relu, alpha = 0.  The arithmetic
 * (summation orders, the Gram-Schmidt solve and its threshold) is the contract of DESIGN.md 3.6,
 * restated in tests/elm_ref.py.
 *
 * nngp_elm_hidden: hidden features of a batch of rows,
 *     H[row][r] = max(0, bias_h[r] + sum_f C[r][f] phi_f(X[row]))    self.loss(bias + C @ x.T),
 *                                                                    models.py:507-508 and :530-531
 * X DEVICE [rows][d], H DEVICE [rows][res_size].  A row's bits do not depend on the rows it is
 * batched with.  rows = 0 is a no-op. */
int nngp_elm_hidden(const double *X, int64_t rows, int d, int degree, int res_size,
                    const double *bias_h, const double *C, double *H, void *stream);

/* nngp_elm_predict: one prediction = ELM_base.predict (models.py:521-535), enqueued on `stream`
 * with no host synchronisation: nngp_knn's m nearest rows of X at new_x (:526-528), their cached
 * hidden rows H[rows][res_size] (nngp_elm_hidden of X) and targets Y[rows][d], the query's hidden
 * row (:530-531), and the min-norm interpolation with a free intercept through them
 * (Ridge(alpha=0).fit / predict, :510-511 and :533-534) evaluated at the query.
 *   preds_out = the prediction [d] (or NULL);  if bias != NULL also out = preds + bias
 *   (parareal.py:382).  Requires 1 <= m <= min(16, rows).                                      */
int nngp_elm_predict(const double *X, const double *Y, const double *H, int64_t rows, int d,
                     const double *new_x, int m, int degree, int res_size, const double *bias_h,
                     const double *C, double *preds_out, const double *bias, double *out,
                     void *stream);

/* nngp_elm_sweep: the sequential sweep of one iteration with the ELM model (parareal.py:359-382),
 * like nngp_correction_sweep without speculation: for i = I .. N-1
 *     UG1[i+1] = G(t[i], t[i+1], U1[i])             (nngp_rk_batch, the sweep's own G launch)
 *     U1[i+1]  = nngp_elm_predict(U1[i]) + UG1[i+1]
 * all on `stream`.  t, U1, UG1 as in nngp_correction_sweep; g_ms_out: HOST, total device time of
 * the G launches (ms), or NULL.                                                                */
int nngp_elm_sweep(const nngp_system *sys, int g_tableau, int g_step_mode, int64_t g_steps,
                   const double *t, int I, int N, double *U1, double *UG1, const double *X,
                   const double *Y, const double *H, int64_t rows, int m, int degree, int res_size,
                   const double *bias_h, const double *C, float *g_ms_out, void *stream);

/* ---- 7. k-NN Parareal correction (Figure_2.py:455-475, NN.predict) ------------------------
 * The plain average of the m nearest neighbours' targets (restated in
 * tests/knnmean_ref.py): the neighbours i_0 .. i_{m-1} are nngp_knn's ordered list; per coordinate
 * s = Y[i_0][c], s = s + Y[i_r][c] for r = 1 .. m-1 in that order, mean = s / (double)m.
 *
 * nngp_knn_mean: the means of the m_j nearest rows for every query and every count, as one
 * distance launch and one select-and-mean launch on `stream`, with no host synchronisation.  The
 * neighbours are selected once at max(m_j); the mean for m_j is the running sum after m_j rows
 * over m_j, bitwise what a call with that count alone gives, and a query's bits do not depend on
 * the queries it is batched with.
 *   X, Y DEVICE [rows][d];  Q DEVICE [n_q][d], 0 <= n_q <= 65535 (0 is a no-op);
 *   m_host HOST [n_m], 1 <= n_m <= 16, each 1 <= m_j <= min(64, rows), any order, repeats allowed;
 *   out DEVICE [n_m][n_q][d];  idx_out DEVICE int32 [n_q][max m_j] or NULL;
 *   bias / out_biased DEVICE [d], both or neither, n_q == n_m == 1 only: out_biased = out + bias. */
int nngp_knn_mean(const double *X, const double *Y, int64_t rows, int d, const double *Q, int n_q,
                  const int32_t *m_host, int n_m, double *out, int32_t *idx_out, const double *bias,
                  double *out_biased, void *stream);

/* nngp_knn_mean_sweep: the sequential sweep of one iteration with the k-NN model, shaped like
 * nngp_elm_sweep: for i = I .. N-1
 *     UG1[i+1] = G(t[i], t[i+1], U1[i])             (nngp_rk_batch)
 *     U1[i+1]  = mean + UG1[i+1],  preds[i-I] = mean  (preds DEVICE [N-I][d] or NULL)
 * two launches per slice, all on `stream`.  N <= I is a no-op.  g_ms_out as in nngp_elm_sweep.   */
int nngp_knn_mean_sweep(const nngp_system *sys, int g_tableau, int g_step_mode, int64_t g_steps,
                        const double *t, int I, int N, double *U1, double *UG1, const double *X,
                        const double *Y, int64_t rows, int m, double *preds, float *g_ms_out,
                        void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NNGP_H_ */
