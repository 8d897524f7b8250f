/*
 * nngp_oracle.c -- CPU RESTATEMENT of the reference's hot path.  TEST INFRASTRUCTURE ONLY.
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this library,
 * and only as the checker / the timed CPU baseline -- never as the product path.  The product
 * (nearest-neighbors-gparareal_amd/) never links or calls it.
 *
 * What it restates (all fp64, /root/reference file:line):
 *   RHS + '-11' wrapper   systems.py:32-44 (wrapper), utils.py:14-33, and the vector fields
 *                         Lorenz 232-238, Hopf 148-154, ThomasLabyrinth 257-271, FHN_ODE 87-95,
 *                         Rossler 116-125, Brusselator 209-214, DblPend 182-189,
 *                         Burgers 421-446, FHN_PDE 321-368
 *   RK stepping           RK.py:30-48 (tableaux), 146-174 (_RK_jax_last: fixed dt),
 *                         91-99 + 178-203 (linspace grid, = new_lib.RK 87-137)
 *   -LML                  models.py:86-92 (_fit_gp_jit), 145-155 (kernel), 240-252 (log_lik,
 *                         NaN -> +inf)
 *   Nelder-Mead           models.py:254-260 -> scipy.optimize._minimize_neldermead (scipy
 *                         1.12/1.15; third-party, restated rule by rule in nm_fit below)
 *   predict               models.py:171-226 (kNN 177-179, fan-out 185-202, argmin 207-215,
 *                         posterior mean 162-168)
 *
 * Parity is pinned against fixtures produced by running the reference itself
 * (tests/golden/gen_golden.py).  Where the reference's arithmetic order is owned by a
 * third-party kernel we cannot reproduce (XLA reductions, OpenBLAS SIMD dot/gemv inside
 * potrf/trsv), this file fixes ONE documented order -- the same one the HIP kernels use -- so
 * GPU-vs-oracle parity is (near) bitwise and oracle-vs-reference is within a stated tolerance:
 *   - sum over d of squared differences in the GP kernel: numpy pairwise_sum order
 *   - kNN distance: sequential (scipy cdist sqeuclidean, transform_reduce_2d_)
 *   - Cholesky: OpenBLAS dpotf2_L's structure (pivot = a_jj - ddot, column = dgemv_n then scale by
 *     the reciprocal; the kernels' accumulation order, see potf2_dot / potf2_gemv_row)
 *   - triangular solves: successive subtraction (OpenBLAS trsv column sweeps)
 *   - y^T alpha, sum(log diag L), K*^T alpha: per lane l the rows l, l+16, l+32, l+48 summed
 *     left to right, then a balanced binary tree over the 16 lanes, = the GPU's xor-butterfly
 *     reduction
 *   - x**3 = x*(x*x) (jax integer_pow), x**2 = x*x
 * Build: oracle/Makefile (gcc -O2 -fopenmp -ffp-contract=off).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#include "../include/nngp.h"

#define MAXS 11

/* ------------------------------------------------------------------------------------------ */
/* Tableaux, RK.py:30-48                                                                      */
/* ------------------------------------------------------------------------------------------ */
typedef struct {
    int S;
    double a[MAXS][MAXS];
    double b[MAXS];
} tableau_t;

/* fully specified sin/cos (defined below, restating csrc/nngp_math.h) */
void nn_sincos(double x, double *sn, double *cs);
double nn_sin(double x);
double nn_sin_pi(double x);
double nn_cos(double x);

static void make_tableau(int order, tableau_t *T) {
    memset(T, 0, sizeof(*T));
    if (order == 1) {
        T->S = 1;
        T->b[0] = 1.0;
    } else if (order == 2) {
        T->S = 2;
        T->a[1][0] = 0.5;
        T->b[1] = 1.0;
    } else if (order == 4) {
        T->S = 4;
        T->a[1][0] = 0.5;
        T->a[2][1] = 0.5;
        T->a[3][2] = 1.0;
        T->b[0] = 1.0 / 6;
        T->b[1] = 1.0 / 3;
        T->b[2] = 1.0 / 3;
        T->b[3] = 1.0 / 6;
    } else { /* Cooper-Verner RK8, RK.py:42-46 */
        const double s = sqrt(21.0);
        T->S = 11;
        double (*a)[MAXS] = T->a;
        a[1][0] = 1.0 / 2;
        a[2][0] = 1.0 / 4; a[2][1] = 1.0 / 4;
        a[3][0] = 1.0 / 7; a[3][1] = (-7 - 3 * s) / 98; a[3][2] = (21 + 5 * s) / 49;
        a[4][0] = (11 + s) / 84; a[4][2] = (18 + 4 * s) / 63; a[4][3] = (21 - s) / 252;
        a[5][0] = (5 + s) / 48; a[5][2] = (9 + s) / 36; a[5][3] = (-231 + 14 * s) / 360;
        a[5][4] = (63 - 7 * s) / 80;
        a[6][0] = (10 - s) / 42; a[6][2] = (-432 + 92 * s) / 315; a[6][3] = (633 - 145 * s) / 90;
        a[6][4] = (-504 + 115 * s) / 70; a[6][5] = (63 - 13 * s) / 35;
        a[7][0] = 1.0 / 14; a[7][4] = (14 - 3 * s) / 126; a[7][5] = (13 - 3 * s) / 63;
        a[7][6] = 1.0 / 9;
        a[8][0] = 1.0 / 32; a[8][4] = (91 - 21 * s) / 576; a[8][5] = 11.0 / 72;
        a[8][6] = (-385 - 75 * s) / 1152; a[8][7] = (63 + 13 * s) / 128;
        a[9][0] = 1.0 / 14; a[9][4] = 1.0 / 9; a[9][5] = (-733 - 147 * s) / 2205;
        a[9][6] = (515 + 111 * s) / 504; a[9][7] = (-51 - 11 * s) / 56;
        a[9][8] = (132 + 28 * s) / 245;
        a[10][4] = (-42 + 7 * s) / 18; a[10][5] = (-18 + 28 * s) / 45;
        a[10][6] = (-273 - 53 * s) / 72; a[10][7] = (301 + 53 * s) / 72;
        a[10][8] = (28 - 28 * s) / 45; a[10][9] = (49 - 7 * s) / 18;
        T->b[0] = 1.0 / 20; T->b[7] = 49.0 / 180; T->b[8] = 16.0 / 45; T->b[9] = 49.0 / 180;
        T->b[10] = 1.0 / 20;
    }
}

/* ------------------------------------------------------------------------------------------ */
/* Vector fields                                                                              */
/* ------------------------------------------------------------------------------------------ */
static inline double cube(double x) { return x * (x * x); } /* jax integer_pow(x, 3) */

/* dense-row dot of a periodic 1-D tridiagonal operator in ascending column order
 * (the non-zeros of row i of Burgers' Dxx / Dx, systems.py:421-442)                         */
static void burgers_rhs(int d, double nu, const double *u, double *out) {
    const double dx = (1.0 - (-1.0)) / (d - 1);
    const double cxx = nu / (dx * dx);      /* Dxx = (nu/dx^2) * Txx                       */
    const double cdg = cxx * -2.0;          /* diagonal entry                              */
    const double q = 1.0 / (2 * dx);        /* Dx = (1/(2 dx)) * Tx                        */
    {   /* row 0: columns 0, 1, d-1; row d-1: columns 0, d-2, d-1 */
        const double lap0 = (cdg * u[0] + cxx * u[1]) + cxx * u[d - 1];
        const double grad0 = q * u[1] + (-q) * u[d - 1];
        const double lapn = (cxx * u[0] + cxx * u[d - 2]) + cdg * u[d - 1];
        const double gradn = q * u[0] + (-q) * u[d - 2];
        out[0] = lap0 - u[0] * grad0;   /* Dxx@u - u*(Dx@u), systems.py:446 */
        out[d - 1] = lapn - u[d - 1] * gradn;
    }
    for (int i = 1; i < d - 1; i++) {
        const double lap = (cxx * u[i - 1] + cdg * u[i]) + cxx * u[i + 1];
        const double grad = (-q) * u[i - 1] + q * u[i + 1];
        out[i] = lap - u[i] * grad;
    }
}

/* FHN-PDE, systems.py:355-368.  (a*(DXX+DYY))@u1: the scalar multiplies the matrix first
 * (Python: `a*(DXX + DYY)@u1` == `(a*(DXX+DYY)) @ u1`).  5 non-zeros per row summed in
 * ascending column order.                                                                   */
static double fhn_lap_row(int nx, double cdiag, double cx, double cy, const double *v, int y,
                          int x) {
    int cols[5];
    double coef[5];
    const int ym = (y == 0) ? nx - 1 : y - 1, yp = (y == nx - 1) ? 0 : y + 1;
    const int xm = (x == 0) ? nx - 1 : x - 1, xp = (x == nx - 1) ? 0 : x + 1;
    cols[0] = ym * nx + x; coef[0] = cy;
    cols[1] = y * nx + xm; coef[1] = cx;
    cols[2] = y * nx + x;  coef[2] = cdiag;
    cols[3] = y * nx + xp; coef[3] = cx;
    cols[4] = yp * nx + x; coef[4] = cy;
    /* sort the 5 (col, coef) pairs by column (insertion sort) */
    for (int i = 1; i < 5; i++) {
        int c = cols[i];
        double k = coef[i];
        int j = i - 1;
        while (j >= 0 && cols[j] > c) {
            cols[j + 1] = cols[j];
            coef[j + 1] = coef[j];
            j--;
        }
        cols[j + 1] = c;
        coef[j + 1] = k;
    }
    double s = coef[0] * v[cols[0]];
    for (int i = 1; i < 5; i++) s = s + coef[i] * v[cols[i]];
    return s;
}

static void fhn_pde_rhs(int nx, const double *u, double *out) {
    const int h = nx * nx;
    const double dx = (1.0 - (-1.0)) / (nx - 1);
    const double c1 = 1 / (dx * dx);                 /* Dxx = (1/dx^2) Txx (= Dyy)         */
    const double ldiag = c1 * -2.0 + c1 * -2.0;       /* (DXX + DYY) diagonal               */
    const double a = 2.8E-4, b = 5E-3, k = -5E-3, tau = 0.1;
    const double ad = a * ldiag, ax = a * c1, ay = a * c1;
    const double bd = b * ldiag, bx = b * c1, by = b * c1;
    const double itau = 1 / tau;
    const double *u1 = u, *u2 = u + h;
    for (int y = 0; y < nx; y++)
        for (int x = 0; x < nx; x++) {
            const int i = y * nx + x;
            double lu, lv;
            if (y > 0 && y < nx - 1 && x > 0 && x < nx - 1) {   /* no wrap: columns already ascending */
                lu = (((ay * u1[i - nx] + ax * u1[i - 1]) + ad * u1[i]) + ax * u1[i + 1]) + ay * u1[i + nx];
                lv = (((by * u2[i - nx] + bx * u2[i - 1]) + bd * u2[i]) + bx * u2[i + 1]) + by * u2[i + nx];
            } else {
                lu = fhn_lap_row(nx, ad, ax, ay, u1, y, x);
                lv = fhn_lap_row(nx, bd, bx, by, u2, y, x);
            }
            out[i] = (((lu + u1[i]) - cube(u1[i])) - u2[i]) + k * 1.0;
            out[h + i] = itau * ((lv + u1[i]) - u2[i]);
        }
}

/* ------------------------------------------------------------------------------------------ */
/* The reference's DENSE formulation of the PDE fields (the timed "reference formulation" CPU  */
/* leg): Burgers Dxx@u - u*(Dx@u) with the d x d matrices (systems.py:421-446),  */
/* FHN-PDE (a(DXX+DYY))@u1, (b(DXX+DYY))@u2 with the h x h Laplacian (systems.py:321-368), as    */
/* XLA evaluates them: every matrix entry multiplied, zeros included.  Each y_i is summed over   */
/* j ascending (column sweeps, vectorised across i without reassociation), so the non-zero      */
/* terms add in the stencil's order and the result equals the stencil RHS bit for bit (up to the */
/* sign of an exact zero); only the cost differs: 2d^2 (Burgers) / h^2 per matvec.              */
/* ------------------------------------------------------------------------------------------ */
typedef struct {
    int n;             /* matrix order: d (Burgers), h = nx^2 (FHN-PDE)                          */
    double *A1T, *A2T; /* column-major: Dxx, Dx (Burgers) / a*L, b*L (FHN-PDE)                   */
} dense_ctx;

static void dense_free(dense_ctx *c) {
    if (!c) return;
    free(c->A1T);
    free(c->A2T);
    free(c);
}

static dense_ctx *dense_build(const nngp_system *sys) {
    dense_ctx *c = (dense_ctx *)calloc(1, sizeof(dense_ctx));
    if (!c) return NULL;
    if (sys->kind == NNGP_SYS_BURGERS) {
        const int d = sys->d;
        const double dx = (1.0 - (-1.0)) / (d - 1), nu = sys->param[0];
        const double cxx = nu / (dx * dx), q = 1.0 / (2 * dx);
        c->n = d;
        c->A1T = (double *)calloc((size_t)d * d, sizeof(double));
        c->A2T = (double *)calloc((size_t)d * d, sizeof(double));
        if (!c->A1T || !c->A2T) { dense_free(c); return NULL; }
#define AT(M, i, j) (M)[(size_t)(j) * d + (i)]
        for (int i = 0; i < d; i++) {       /* Txx: -2 diagonal, 1 off; Tx: +1 above, -1 below */
            AT(c->A1T, i, i) = cxx * -2.0;
            if (i + 1 < d) {
                AT(c->A1T, i, i + 1) = cxx * 1.0;
                AT(c->A1T, i + 1, i) = cxx * 1.0;
                AT(c->A2T, i, i + 1) = q * 1.0;
                AT(c->A2T, i + 1, i) = q * -1.0;
            }
        }
        AT(c->A1T, 0, d - 1) = 1 * cxx;      /* periodic corners, Burgers.py:53-56 / systems.py */
        AT(c->A1T, d - 1, 0) = 1 * cxx;
        AT(c->A2T, 0, d - 1) = -1 * q;
        AT(c->A2T, d - 1, 0) = 1 * q;
#undef AT
    } else if (sys->kind == NNGP_SYS_FHN_PDE) {
        const int nx = sys->nx, h = nx * nx;
        const double dx = (1.0 - (-1.0)) / (nx - 1);
        const double c1 = 1 / (dx * dx);
        const double ldiag = c1 * -2.0 + c1 * -2.0;
        const double a = 2.8E-4, b = 5E-3;
        c->n = h;
        c->A1T = (double *)calloc((size_t)h * h, sizeof(double));
        c->A2T = (double *)calloc((size_t)h * h, sizeof(double));
        if (!c->A1T || !c->A2T) { dense_free(c); return NULL; }
        for (int y = 0; y < nx; y++)
            for (int x = 0; x < nx; x++) {
                const int i = y * nx + x;
                const int ym = (y == 0) ? nx - 1 : y - 1, yp = (y == nx - 1) ? 0 : y + 1;
                const int xm = (x == 0) ? nx - 1 : x - 1, xp = (x == nx - 1) ? 0 : x + 1;
                const int cols[4] = {ym * nx + x, y * nx + xm, y * nx + xp, yp * nx + x};
                c->A1T[(size_t)i * h + i] = a * ldiag;
                c->A2T[(size_t)i * h + i] = b * ldiag;
                for (int t = 0; t < 4; t++) {
                    c->A1T[(size_t)cols[t] * h + i] = a * c1;
                    c->A2T[(size_t)cols[t] * h + i] = b * c1;
                }
            }
    } else {
        dense_free(c);
        return NULL;
    }
    return c;
}

/* y = A x, y_i = sum_j A_ij x_j over j ascending (AT column-major)                           */
static void matvec_cols(int n, const double *restrict AT, const double *restrict x, double *restrict y) {
    const double x0 = x[0];
    for (int i = 0; i < n; i++) y[i] = AT[i] * x0;
    for (int j = 1; j < n; j++) {
        const double xj = x[j];
        const double *restrict col = AT + (size_t)j * n;
        for (int i = 0; i < n; i++) y[i] = y[i] + col[i] * xj;
    }
}

static void rhs_dense(const nngp_system *sys, const dense_ctx *c, const double *u, double *out) {
    const int n = c->n;
    double *y1 = (double *)__builtin_alloca(sizeof(double) * 2 * (size_t)n), *y2 = y1 + n;
    if (sys->kind == NNGP_SYS_BURGERS) {
        matvec_cols(n, c->A1T, u, y1);
        matvec_cols(n, c->A2T, u, y2);
        for (int i = 0; i < n; i++) out[i] = y1[i] - u[i] * y2[i];   /* systems.py:446 */
    } else {
        const double *u1 = u, *u2 = u + n;
        const double k = -5E-3, itau = 1 / 0.1;
        matvec_cols(n, c->A1T, u1, y1);
        matvec_cols(n, c->A2T, u2, y2);
        for (int i = 0; i < n; i++) {
            out[i] = (((y1[i] + u1[i]) - cube(u1[i])) - u2[i]) + k * 1.0;
            out[n + i] = itau * ((y2[i] + u1[i]) - u2[i]);
        }
    }
}

static void rhs_raw(const nngp_system *sys, const double *u, double *out) {
    switch (sys->kind) {
    case NNGP_SYS_LORENZ:
        out[0] = 10 * (u[1] - u[0]);
        out[1] = (28 * u[0] - u[1]) - u[0] * u[2];
        out[2] = u[0] * u[1] - (8.0 / 3) * u[2];
        break;
    case NNGP_SYS_HOPF: {
        const double mt = sys->param[0];
        const double g = ((u[2] / mt) - u[0] * u[0]) - u[1] * u[1];
        out[0] = -u[1] + u[0] * g;
        out[1] = u[0] + u[1] * g;
        out[2] = 1;
        break;
    }
    case NNGP_SYS_THOMAS_LABYRINTH: {
        const double a = 0.5, b = 10.0;
        out[0] = -a * u[0] + b * nn_sin_pi(u[1]);
        out[1] = -a * u[1] + b * nn_sin_pi(u[2]);
        out[2] = -a * u[2] + b * nn_sin_pi(u[0]);
        break;
    }
    case NNGP_SYS_FHN_ODE: {
        const double a = 0.2, b = 0.2, c = 3;
        out[0] = c * ((u[0] - (cube(u[0]) / 3)) + u[1]);
        out[1] = -(1 / c) * ((u[0] - a) + b * u[1]);
        break;
    }
    case NNGP_SYS_ROSSLER: {
        const double a = 0.2, b = 0.2, c = 5.7;
        out[0] = -u[1] - u[2];
        out[1] = u[0] + (a * u[1]);
        out[2] = b + u[2] * (u[0] - c);
        break;
    }
    case NNGP_SYS_BRUSSELATOR:
        out[0] = (1 + (u[0] * u[0]) * u[1]) - (3 + 1) * u[0];
        out[1] = 3 * u[0] - (u[0] * u[0]) * u[1];
        break;
    case NNGP_SYS_DBL_PEND: {
        double s, c;
        nn_sincos(u[0] - u[2], &s, &c);
        const double s0 = nn_sin(u[0]), s2 = nn_sin(u[2]);
        const double pre = -1 / (2 - c * c);
        out[0] = u[1];
        out[1] = pre * ((((u[1] * u[1]) * c) * s + (u[3] * u[3]) * s) + 2 * s0 - c * s2);
        out[2] = u[3];
        out[3] = pre * ((((-2 * (u[1] * u[1])) * s - ((u[3] * u[3]) * s) * c) - (2 * c) * s0) + 2 * s2);
        break;
    }
    case NNGP_SYS_BURGERS:
        burgers_rhs(sys->d, sys->param[0], u, out);
        break;
    case NNGP_SYS_FHN_PDE:
        fhn_pde_rhs(sys->nx, u, out);
        break;
    }
}

/* systems.py:36-40 + utils.py:24,31: f_n(u) = f(inverse(u)) * scale                         */
static void rhs_ex(const nngp_system *sys, const dense_ctx *dc, const double *u, double *out, double *scratch) {
    const int d = sys->d;
    if (sys->normalized) {
        const double *mn = sys->norm, *w = sys->norm + d;
        for (int i = 0; i < d; i++) scratch[i] = ((u[i] + 1) / 2) * w[i] + mn[i];
        u = scratch;
    }
    if (dc) rhs_dense(sys, dc, u, out);
    else rhs_raw(sys, u, out);
    if (sys->normalized) {
        const double *sc = sys->norm + 2 * d;
        for (int i = 0; i < d; i++) out[i] = out[i] * sc[i];
    }
}

void orc_rhs(const nngp_system *sys, const double *u, double *out, double *scratch) {
    rhs_ex(sys, NULL, u, out, scratch);
}

/* ------------------------------------------------------------------------------------------ */
/* RK propagation, one slice.  RK.py:146-174 (FIXED) / RK.py:178-203 (LINSPACE)               */
/* ------------------------------------------------------------------------------------------ */
/* general form: FIXED uses h = (t1-t0)/steps; LINSPACE walks steps j0..j0+steps-1 of the grid
 * np.linspace(t0, t1, gsteps+1) (gsteps = steps, j0 = 0: the per-slice grid of RK.run)     */
static int rk_core(const nngp_system *sys, const dense_ctx *dc, int order, int mode, double t0, double t1,
                   int64_t gsteps, int64_t j0, int64_t steps, const double *u0, double *u1) {
    tableau_t T;
    make_tableau(order, &T);
    const int d = sys->d, S = T.S;
    double *buf = (double *)malloc(sizeof(double) * (size_t)d * (S + 3));
    if (!buf) return -1;
    double *u = buf, *tmp = buf + d, *scr = buf + 2 * d, *k = buf + 3 * d;
    memcpy(u, u0, sizeof(double) * d);
    const double dt = (t1 - t0) / steps;          /* RK.py:103                               */
    const double lstep = (t1 - t0) / gsteps;      /* numpy linspace: step = delta/div        */
    for (int64_t n = 0; n < steps; n++) {
        double h;
        if (mode == NNGP_STEP_FIXED) {
            h = dt;
        } else { /* h = t[j+1] - t[j], t[j] = j*step + t0, t[gsteps] = t1 (linspace)         */
            const int64_t j = j0 + n;
            const double tn = (double)j * lstep + t0;
            const double tn1 = (j + 1 == gsteps) ? t1 : (double)(j + 1) * lstep + t0;
            h = tn1 - tn;
        }
        /* k_0 = h*f(u); k_i = h*f(u + sum_{j<i} a_ij k_j)                                  */
        rhs_ex(sys, dc, u, k, scr);
        for (int c = 0; c < d; c++) k[c] = h * k[c];
        for (int i = 1; i < S; i++) {
            /* the reference sums from temp = 0 (RK.py:153-166); starting from the first non-zero
             * term is identical up to the sign of an exact zero (the HIP kernels do the same).
             * Each element's terms are added in ascending j; the loops run j outer, c inner so
             * the per-element sums vectorise across c without reassociation.                   */
            if (d <= 8) {   /* small systems: per-element scalar sums (same order) */
                for (int c = 0; c < d; c++) {
                    double t = 0.0;
                    int first = 1;
                    for (int j = 0; j < i; j++) {
                        if (T.a[i][j] == 0.0) continue;
                        const double v = T.a[i][j] * k[(size_t)j * d + c];
                        t = first ? v : t + v;
                        first = 0;
                    }
                    tmp[c] = first ? u[c] : u[c] + t;
                }
                double *ki = k + (size_t)i * d;
                rhs_ex(sys, dc, tmp, ki, scr);
                for (int c = 0; c < d; c++) ki[c] = h * ki[c];
                continue;
            }
            int first = 1;
            for (int j = 0; j < i; j++) {
                const double a = T.a[i][j];
                if (a == 0.0) continue;
                const double *kj = k + (size_t)j * d;
                if (first)
                    for (int c = 0; c < d; c++) tmp[c] = a * kj[c];
                else
                    for (int c = 0; c < d; c++) tmp[c] = tmp[c] + a * kj[c];
                first = 0;
            }
            if (first)
                memcpy(tmp, u, sizeof(double) * d);
            else
                for (int c = 0; c < d; c++) tmp[c] = u[c] + tmp[c];
            double *ki = k + (size_t)i * d;
            rhs_ex(sys, dc, tmp, ki, scr);
            for (int c = 0; c < d; c++) ki[c] = h * ki[c];
        }
        /* u += sum_s b_s k_s  (jnp.sum(b*k,1); zeros in b are exact no-ops)                */
        if (d <= 8) {
            for (int c = 0; c < d; c++) {
                double acc = 0.0;
                int first = 1;
                for (int s2 = 0; s2 < S; s2++) {
                    if (T.b[s2] == 0.0) continue;
                    const double v = T.b[s2] * k[(size_t)s2 * d + c];
                    acc = first ? v : acc + v;
                    first = 0;
                }
                u[c] = u[c] + acc;
            }
        } else {
            int first = 1;
            for (int s2 = 0; s2 < S; s2++) {
                const double b = T.b[s2];
                if (b == 0.0) continue;
                const double *ks = k + (size_t)s2 * d;
                if (first)
                    for (int c = 0; c < d; c++) tmp[c] = b * ks[c];
                else
                    for (int c = 0; c < d; c++) tmp[c] = tmp[c] + b * ks[c];
                first = 0;
            }
            for (int c = 0; c < d; c++) u[c] = u[c] + tmp[c];
        }
    }
    memcpy(u1, u, sizeof(double) * d);
    free(buf);
    return 0;
}

int orc_rk_grid(const nngp_system *sys, int order, int mode, double t0, double t1, int64_t gsteps,
                int64_t j0, int64_t steps, const double *u0, double *u1) {
    return rk_core(sys, NULL, order, mode, t0, t1, gsteps, j0, steps, u0, u1);
}

int orc_rk(const nngp_system *sys, int order, int mode, double t0, double t1, int64_t steps,
           const double *u0, double *u1) {
    return rk_core(sys, NULL, order, mode, t0, t1, steps, 0, steps, u0, u1);
}

/* dense != 0: the PDE fields in the reference's dense-matrix formulation (see rhs_dense)    */
int orc_rk_batch_ex(const nngp_system *sys, int order, int mode, int n_slices, const double *t0,
                    const double *t1, int64_t steps, const double *u0, double *uF, int nthreads, int dense) {
    int err = 0;
    dense_ctx *dc = NULL;
    if (dense) {
        dc = dense_build(sys);
        if (!dc) return -1;
    }
#ifdef _OPENMP
    if (nthreads > 0) omp_set_num_threads(nthreads);
#pragma omp parallel for schedule(dynamic, 1) reduction(| : err)
#endif
    for (int i = 0; i < n_slices; i++)
        err |= rk_core(sys, dc, order, mode, t0[i], t1[i], steps, 0, steps,
                       u0 + (size_t)i * sys->d, uF + (size_t)i * sys->d);
    dense_free(dc);
    return err ? -1 : 0;
}

int orc_rk_batch(const nngp_system *sys, int order, int mode, int n_slices, const double *t0,
                 const double *t1, int64_t steps, const double *u0, double *uF, int nthreads) {
    return orc_rk_batch_ex(sys, order, mode, n_slices, t0, t1, steps, u0, uF, nthreads, 0);
}

/* ------------------------------------------------------------------------------------------ */
/* exp / 10^x / log with a fully specified operation order -- the same algorithm and constants  */
/* as the GPU's csrc/nngp_math.h, so the -LML (and every Nelder-Mead branch on it) is bitwise   */
/* identical on both sides.  <= 2 ulp vs glibc (tests/test_oracle_golden.py::test_math_accuracy), */
/* <= 1 ulp of the true value (::test_math_true_error, 200-bit mpmath: exp 0.81, 10^x 0.93,      */
/* log 0.62; sin / cos <= 2 with an absolute floor of 2^-62 on |x| <= 1e4).                      */
/* ------------------------------------------------------------------------------------------ */
static const double NN_INV_LN2 = 0x1.71547652b82fep+0;
static const double NN_LN2_HI = 0x1.62e42fefa3800p-1;
static const double NN_LN2_LO = 0x1.ef35793c76730p-45;
static const double NN_LN10 = 0x1.26bb1bbb55516p+1;
static const double NN_LN10_LO = -0x1.f48ad494ea3e9p-53;

static double nn_exp_dd(double hi, double lo) {
    if (hi != hi) return hi;
    if (hi > 709.782712893384) return INFINITY;
    if (hi < -745.1332191019412) return 0.0;
    const double n = rint(hi * NN_INV_LN2);
    double r = fma(-n, NN_LN2_HI, hi);
    r = fma(-n, NN_LN2_LO, r);
    r = r + lo;
    double p = 1.0 / 6227020800.0;
    p = fma(p, r, 1.0 / 479001600.0);
    p = fma(p, r, 1.0 / 39916800.0);
    p = fma(p, r, 1.0 / 3628800.0);
    p = fma(p, r, 1.0 / 362880.0);
    p = fma(p, r, 1.0 / 40320.0);
    p = fma(p, r, 1.0 / 5040.0);
    p = fma(p, r, 1.0 / 720.0);
    p = fma(p, r, 1.0 / 120.0);
    p = fma(p, r, 1.0 / 24.0);
    p = fma(p, r, 1.0 / 6.0);
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return ldexp(p, (int)n);
}

double nn_exp(double x) { return nn_exp_dd(x, 0.0); }

/* elementwise nn_exp / nn_log over arrays (tools/fit_agreement.py)                          */
void orc_exp_array(int64_t n, const double *x, double *out) {
    for (int64_t i = 0; i < n; i++) out[i] = nn_exp(x[i]);
}

double nn_log(double x);

void orc_log_array(int64_t n, const double *x, double *out) {
    for (int64_t i = 0; i < n; i++) out[i] = nn_log(x[i]);
}

/* the other shared routines over arrays (tests/test_gpu_math_probe.py: the device's copy against
 * these, bit for bit); the exp of a double-double is the static nn_exp_dd above                 */
double nn_pow10(double x);

void orc_exp_dd_array(int64_t n, const double *hi, const double *lo, double *out) {
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; i++) out[i] = nn_exp_dd(hi[i], lo[i]);
}

void orc_pow10_array(int64_t n, const double *x, double *out) {
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; i++) out[i] = nn_pow10(x[i]);
}

void orc_sincos_array(int64_t n, const double *x, double *sn, double *cs) {
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; i++) nn_sincos(x[i], sn + i, cs + i);
}

void orc_sin_pi_array(int64_t n, const double *x, double *out) {
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; i++) out[i] = nn_sin_pi(x[i]);
}

double nn_pow10(double x) {
    const double hi = x * NN_LN10;
    const double lo = fma(x, NN_LN10, -hi) + x * NN_LN10_LO;
    return nn_exp_dd(hi, lo);
}

double nn_log(double x) {   /* fdlibm e_log.c */
    if (!(x > 0.0)) return x == 0.0 ? -INFINITY : NAN;
    if (x == INFINITY) return x;
    const double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01,
                 Lg3 = 2.857142874366239149e-01, Lg4 = 2.222219843214978396e-01,
                 Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
                 Lg7 = 1.479819860511658591e-01;
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
    int k;
    double m = frexp(x, &k);
    if (m < 0.70710678118654752440) {
        m = m * 2.0;
        k -= 1;
    }
    const double f = m - 1.0;
    const double dk = (double)k;
    const double s = f / (2.0 + f);
    const double z = s * s;
    const double w = z * z;
    const double t1 = w * (Lg2 + w * (Lg4 + w * Lg6));
    const double t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)));
    const double R = t2 + t1;
    const double hfsq = 0.5 * f * f;
    return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f);
}

/* sin / cos, restating csrc/nngp_math.h nn_sincos bit for bit (fdlibm pieces, fma reduction).  */
static const double TR_INVPIO2 = 6.36619772367581382433e-01, TR_PIO2_1 = 1.57079632673412561417e+00,
                    TR_PIO2_2 = 6.07710050630396597660e-11, TR_PIO2_3 = 2.02226624871116645580e-21;
static const double TR_S1 = -1.66666666666666324348e-01, TR_S2 = 8.33333333332248946124e-03,
                    TR_S3 = -1.98412698298579493134e-04, TR_S4 = 2.75573137070700676789e-06,
                    TR_S5 = -2.50507602534068634195e-08, TR_S6 = 1.58969099521155010221e-10;
static const double TR_C1 = 4.16666666666666019037e-02, TR_C2 = -1.38888888888741095749e-03,
                    TR_C3 = 2.48015872894767294178e-05, TR_C4 = -2.75573143513906633035e-07,
                    TR_C5 = 2.08757232129817482790e-09, TR_C6 = -1.13596475577881948265e-11;

void nn_sincos(double x, double *sn, double *cs) {
    const int fin = (x - x) == 0.0;
    const double xf = fin ? x : 0.0;
    const double n = rint(xf * TR_INVPIO2);
    double r = fma(-n, TR_PIO2_1, xf);
    r = fma(-n, TR_PIO2_2, r);
    r = fma(-n, TR_PIO2_3, r);
    const double z = r * r;
    const double v = z * r;
    const double ps = TR_S2 + z * (TR_S3 + z * (TR_S4 + z * (TR_S5 + z * TR_S6)));
    const double ks = r + v * (TR_S1 + z * ps);
    const double pc = z * (TR_C1 + z * (TR_C2 + z * (TR_C3 + z * (TR_C4 + z * (TR_C5 + z * TR_C6)))));
    const double hz = 0.5 * z;
    const double w = 1.0 - hz;
    const double kc = w + (((1.0 - w) - hz) + z * pc);
    /* quadrant from the bit pattern of n + 1.5*2^52 (= n mod 4 for |n| < 2^51), as the kernel */
    const double nq = n + 6755399441055744.0;
    uint64_t nb;
    memcpy(&nb, &nq, sizeof nb);
    const int q = (int)(nb & 3u);
    double s_ = (q & 1) ? kc : ks;
    double c_ = (q & 1) ? ks : kc;
    s_ = (q & 2) ? -s_ : s_;
    c_ = ((q + 1) & 2) ? -c_ : c_;
    const double nanv = x - x;
    *sn = fin ? s_ : nanv;
    *cs = fin ? c_ : nanv;
}

/* sin alone, restating csrc/nngp_math.h nn_sin_pi bit for bit (ThomasLabyrinth): x = n pi + r,
 * |r| <= pi/2, one odd polynomial, sign (-1)^n. */
static const double SP_INVPI = 0x1.45f306dc9c883p-2;
static const double SP_PI_1 = 2 * 1.57079632673412561417e+00, SP_PI_2 = 2 * 6.07710050630396597660e-11,
                    SP_PI_3 = 2 * 2.02226624871116645580e-21;
static const double SP_S1 = -0x1.5555555555555p-3, SP_S2 = 0x1.11111111110c1p-7, SP_S3 = -0x1.a01a01a0148bbp-13,
                    SP_S4 = 0x1.71de3a5287c12p-19, SP_S5 = -0x1.ae6454cb54cccp-26, SP_S6 = 0x1.6123cb28741dap-33,
                    SP_S7 = -0x1.ae431d76c3814p-41, SP_S8 = 0x1.88299fb2db5f9p-49;

double nn_sin_pi(double x) {   /* inf / NaN: n = +-inf or NaN, so r = NaN and the result is NaN */
    const double n = rint(x * SP_INVPI);
    double r = fma(-n, SP_PI_1, x);
    r = fma(-n, SP_PI_2, r);
    r = fma(-n, SP_PI_3, r);
    const double z = r * r;
    double p = fma(SP_S8, z, SP_S7);
    p = fma(p, z, SP_S6);
    p = fma(p, z, SP_S5);
    p = fma(p, z, SP_S4);
    p = fma(p, z, SP_S3);
    p = fma(p, z, SP_S2);
    p = fma(p, z, SP_S1);
    double s = fma(r * z, p, r);
    const double nq = n + 6755399441055744.0;
    uint64_t nb, sb;
    memcpy(&nb, &nq, sizeof nb);
    memcpy(&sb, &s, sizeof sb);
    sb ^= (nb & 1u) << 63;
    memcpy(&s, &sb, sizeof s);
    return s;
}

double nn_sin(double x) {
    double s, c;
    nn_sincos(x, &s, &c);
    return s;
}

double nn_cos(double x) {
    double s, c;
    nn_sincos(x, &s, &c);
    return c;
}

/* ------------------------------------------------------------------------------------------ */
/* GP pieces                                                                                  */
/* ------------------------------------------------------------------------------------------ */
/* numpy pairwise_sum (numpy/_core/src/umath/loops_utils.h.src), used by jnp/np.sum          */
static double pairwise_sum(const double *a, int n) {
    if (n < 8) {
        double res = 0.;
        for (int i = 0; i < n; i++) res += a[i];
        return res;
    } else if (n <= 128) {
        double r[8];
        int i;
        for (int j = 0; j < 8; j++) r[j] = a[j];
        for (i = 8; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; j++) r[j] += a[i + j];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; i++) res += a[i];
        return res;
    } else {
        int n2 = n / 2;
        n2 -= n2 % 8;
        return pairwise_sum(a, n2) + pairwise_sum(a + n2, n - n2);
    }
}

double orc_sqdist_pairwise(const double *a, const double *b, int d, double *scratch) {
    for (int i = 0; i < d; i++) {
        const double t = a[i] - b[i];
        scratch[i] = t * t;
    }
    return pairwise_sum(scratch, d);
}

/* Cross-lane sum of the GPU's 16-lane group (one DPP row): lane l holds rows l, l+16, l+32,
 * l+48 (as many as ceil(n/16)), which it adds first, left to right; then xor-butterfly levels
 * 1, 2, 4, 8 -- lane 0 pairs (0,1),(2,3),... first, then (0,2),... -- a balanced tree.  Rows >= n
 * contribute 0.0.                                                                            */
static double butterfly_sum(const double *v, int n) {
    double buf[16];
    for (int i = 0; i < 16; i++) {
        buf[i] = i < n ? v[i] : 0.0;
        for (int s = 1; 16 * s < n; s++) buf[i] = buf[i] + (i + 16 * s < n ? v[i + 16 * s] : 0.0);
    }
    for (int s = 1; s < 16; s <<= 1)
        for (int i = 0; i < 16; i += 2 * s) buf[i] = buf[i] + buf[i + s];
    return buf[0];
}

/* The reference's Cholesky is LAPACK dpotrf (jax.numpy.linalg.cholesky on CPU -> OpenBLAS; for
 * n <= 32 its unblocked dpotf2_L):  ajj = a_jj - ddot(row j);  column j below the diagonal
 * = (a_ij - A[j+1:, :j] @ L[j, :j]) via dgemv_n, then scaled by 1/ajj.  Its pass/fail bit on
 * near-singular kernels (duplicated training rows: a jitter below psy*2^-53 is lost and K is
 * psy*ones) steers Nelder-Mead -- a spurious pass yields a hugely negative -LML that wins the
 * arg-min -- so the sums follow OpenBLAS's structure (x86_64 kernels; fma where its gcc build
 * contracts), which agrees with numpy's LAPACK on pass/fail for ~99.6 % of duplicated-row kernels
 * against ~89 % for subtracting the products one at a time:
 *   diagonal  ddot over a strided row: two accumulators over groups of 4, t1 += fma(x0, x0, x2^2),
 *             t2 += fma(x1, x1, x3^2), tail t1 = fma(x, x, t1); ddot = t1 + t2;
 *   below     dgemv_n: rows in whole groups of 4 ("vector rows") add each 4-column block as
 *             y -= fma(a3,x3, fma(a2,x2, fma(a1,x1, a0*x0))) and each leftover column as
 *             y -= a*x; the last (n-j-1) & 3 rows ("tail rows") take y -= one fma chain over
 *             all columns.                                                                  */
static double potf2_dot(const double *x, int n) {
    double t1 = 0.0, t2 = 0.0;
    int i = 0;
    for (; i + 4 <= n; i += 4) {
        t1 = t1 + fma(x[i], x[i], x[i + 2] * x[i + 2]);
        t2 = t2 + fma(x[i + 1], x[i + 1], x[i + 3] * x[i + 3]);
    }
    for (; i < n; i++) t1 = fma(x[i], x[i], t1);
    return t1 + t2;
}

static double potf2_gemv_row(double y, const double *a, const double *x, int n, int vector_row) {
    if (vector_row) {
        int k = 0;
        for (; k + 4 <= n; k += 4) {
            double t = a[k] * x[k];
            t = fma(a[k + 1], x[k + 1], t);
            t = fma(a[k + 2], x[k + 2], t);
            t = fma(a[k + 3], x[k + 3], t);
            y = y - t;
        }
        for (; k < n; k++) y = y - a[k] * x[k];
        return y;
    }
    double t = 0.0;
    for (int k = 0; k < n; k++) t = fma(a[k], x[k], t);
    return y - t;
}

/* Roundoff-sensitivity experiment only (tests/golden/gen_oracle_loops.py *_sumorder): 1 switches
 * the GP solves and the -LML's two sums to another, equally valid summation order (dot products
 * accumulated with fma in the opposite direction and subtracted once; sequential instead of
 * pairwise sums) -- the kind of last-ulp difference between the restatement and XLA/OpenBLAS.
 * The default 0 is the oracle.                                                               */
static int g_sum_order = 0;
void orc_set_sum_order(int o) { g_sum_order = o; }

/* Cholesky + solves for K = psy*exp(c*D2) + jit*I.  Returns 0 ok, 1 if potrf fails.
 * The factorisation follows OpenBLAS dpotf2_L (potf2_dot / potf2_gemv_row above); on the
 * reference's own LML fixtures (tests/golden/lml.npz) its pass/fail bit agrees on 99.8 % of the
 * duplicated-row grid, and on 99.6 % of random duplicated / clustered kernels against numpy's
 * LAPACK (89-97 % for subtracting the products one at a time, round 1's order, whose spurious
 * passes on exactly duplicated neighbours -- FHN-PDE at its steady state -- derailed the run).
 * The solves: forward z_i (k ascending), back alpha_i (k descending), successive subtraction,
 * each division the Markstein-corrected x*RN(1/L_ii) (bitwise the IEEE quotient).            */
/* the factorisation and the two solves on a built K (lower triangle of L, in place), exported as
 * orc_potf2 / orc_solves for the fit-level attribution (tools/fit_agreement.py)                */
int orc_potf2(int m, double *L /*m*m, lower = K on entry*/, double *rinv_d) {
    for (int j = 0; j < m; j++) {
        const double t = L[j * m + j] - potf2_dot(L + j * m, j);
        if (!(t > 0.0)) return 1;           /* ajj <= 0 or NaN: jax -> NaN -> +inf          */
        const double ljj = sqrt(t);
        const double rinv = 1.0 / ljj;
        L[j * m + j] = ljj;
        rinv_d[j] = rinv;
        const int mm = m - 1 - j, m1 = mm & -4;
        for (int i = j + 1; i < m; i++)
            L[i * m + j] = potf2_gemv_row(L[i * m + j], L + i * m, L + j * m, j, i - j - 1 < m1) * rinv;
    }
    return 0;
}

static void gp_solves(int m, const double *L, const double *rinv_d, const double *y, double *alpha);

void orc_solves(int m, const double *L, const double *rinv_d, const double *y, double *alpha) {
    gp_solves(m, L, rinv_d, y, alpha);
}

static int gp_factor(int m, const double *D2, const double *y, double c, double psy, double jit,
                     double *L /*m*m*/, double *alpha) {
    /* build lower triangle (models.py:146-155, 88) */
    for (int r = 0; r < m; r++)
        for (int j = 0; j <= r; j++) {
            double v = psy * nn_exp(c * D2[r * m + j]);
            if (j == r) v = v + jit;
            L[r * m + j] = v;
        }
    double rinv_d[64];
    if (orc_potf2(m, L, rinv_d)) return 1;
    gp_solves(m, L, rinv_d, y, alpha);
    return 0;
}

static void gp_solves(int m, const double *L, const double *rinv_d, const double *y, double *alpha) {
    double z[64];
    for (int i = 0; i < m; i++) {
        double s = y[i];
        if (g_sum_order) {   /* experiment: BLAS-style dot first, reversed, then one subtraction */
            double d = 0.0;
            for (int k = i - 1; k >= 0; k--) d = fma(L[i * m + k], z[k], d);
            s = s - d;
        } else
            for (int k = 0; k < i; k++) s = s - L[i * m + k] * z[k];
        const double q = s * rinv_d[i];
        z[i] = fma(fma(-q, L[i * m + i], s), rinv_d[i], q);
    }
    for (int i = m - 1; i >= 0; i--) {
        double s = z[i];
        if (g_sum_order) {
            double d = 0.0;
            for (int k = i + 1; k < m; k++) d = fma(L[k * m + i], alpha[k], d);
            s = s - d;
        } else
            for (int k = m - 1; k > i; k--) s = s - L[k * m + i] * alpha[k];
        const double q = s * rinv_d[i];
        alpha[i] = fma(fma(-q, L[i * m + i], s), rinv_d[i], q);
    }
}

static const double LOG_2PI = 1.8378770664093453; /* np.log(2*np.pi) */

/* -LML, models.py:240-252 (NaN -> +inf).  jit = 10**jitter (host pow).                       */
double orc_nlml(int m, const double *D2, const double *y, double sx, double sy, double jit) {
    double L[64 * 64], alpha[64], tmp[64] = {0};
    const double c = -0.5 * (1 / nn_pow10(sx));
    const double psy = nn_pow10(sy);
    if (gp_factor(m, D2, y, c, psy, jit, L, alpha)) return INFINITY;
    for (int i = 0; i < m; i++) tmp[i] = y[i] * alpha[i];
    double ydot = butterfly_sum(tmp, m);
    for (int i = 0; i < m; i++) tmp[i] = nn_log(L[i * m + i]);
    double slog = butterfly_sum(tmp, m);
    if (g_sum_order) {   /* experiment: sequential sums */
        ydot = 0.0;
        slog = 0.0;
        for (int i = 0; i < m; i++) {
            ydot = fma(y[i], alpha[i], ydot);
            slog += nn_log(L[i * m + i]);
        }
    }
    const double res = -(((-0.5 * ydot) - slog) - ((double)m / 2) * LOG_2PI);
    if (isnan(res)) return INFINITY;
    return res;
}

/* posterior mean K(xm, new_x)^T alpha, models.py:162-168                                     */
double orc_gp_mean_one(int m, const double *D2, const double *kd2, const double *y, double sx,
                       double sy, double jit) {
    double L[64 * 64], alpha[64], tmp[64] = {0};
    const double c = -0.5 * (1 / nn_pow10(sx));
    const double psy = nn_pow10(sy);
    if (gp_factor(m, D2, y, c, psy, jit, L, alpha)) return NAN;
    for (int i = 0; i < m; i++) tmp[i] = (psy * nn_exp(c * kd2[i])) * alpha[i];
    return butterfly_sum(tmp, m);
}

/* numpy's small-array argsort is insertion sort (stable); NaN sort last                      */
static inline int nm_less(double a, double b) { return a < b || (b != b && a == a); }

static void nm_sort(double sim[3][2], double fsim[3]) {
    for (int i = 1; i < 3; i++) {
        double f = fsim[i], x0 = sim[i][0], x1 = sim[i][1];
        int j = i - 1;
        while (j >= 0 && nm_less(f, fsim[j])) {
            fsim[j + 1] = fsim[j];
            sim[j + 1][0] = sim[j][0];
            sim[j + 1][1] = sim[j][1];
            j--;
        }
        fsim[j + 1] = f;
        sim[j + 1][0] = x0;
        sim[j + 1][1] = x1;
    }
}

/* scipy.optimize._optimize._minimize_neldermead, N = 2, adaptive=False, no bounds:
 * rho=1, chi=2, psi=0.5, sigma=0.5; nonzdelt=0.05, zdelt=0.00025; maxiter=maxfun=200*N.
 * A call beyond maxfun raises _MaxFuncCallError, which aborts the current iteration
 * (the `finally` still sorts).  Returns sim[0], min(fsim), nfev.                             */
typedef double (*nm_fn_t)(const double *x, void *ctx);

typedef struct {
    nm_fn_t fn;
    void *ctx;
    int fcalls;
    int maxfun;
} nm_obj_t;

static int nm_eval(nm_obj_t *o, const double x[2], double *f) {
    if (o->fcalls >= o->maxfun) return 1; /* _MaxFuncCallError */
    o->fcalls++;
    *f = o->fn(x, o->ctx);
    return 0;
}

/* Nelder-Mead core on an arbitrary objective (exported so tests can pin it against scipy
 * with the very same Python objective).                                                     */
void orc_nm_core(nm_fn_t fn, void *ctx, const double th0[2], double fatol, double xatol,
                 int maxfev, double th_out[2], double *fval, int *nfev) {
    nm_obj_t o = {fn, ctx, 0, maxfev};
    const int maxiter = maxfev; /* both default to 200*N (models.py passes neither)          */
    double sim[3][2], fsim[3] = {INFINITY, INFINITY, INFINITY};
    sim[0][0] = th0[0];
    sim[0][1] = th0[1];
    for (int k = 0; k < 2; k++) {
        double yk[2] = {th0[0], th0[1]};
        yk[k] = (yk[k] != 0) ? (1 + 0.05) * yk[k] : 0.00025;
        sim[k + 1][0] = yk[0];
        sim[k + 1][1] = yk[1];
    }
    for (int k = 0; k < 3; k++)
        if (nm_eval(&o, sim[k], &fsim[k])) break;
    nm_sort(sim, fsim);
    int iterations = 1;
    while (o.fcalls < o.maxfun && iterations < maxiter) {
        /* convergence test: max|sim[1:]-sim[0]| <= xatol and max|fsim[0]-fsim[1:]| <= fatol */
        int xok = 1, fok = 1;
        for (int i = 1; i < 3; i++)
            for (int k = 0; k < 2; k++)
                if (!(fabs(sim[i][k] - sim[0][k]) <= xatol)) xok = 0;
        for (int i = 1; i < 3; i++)
            if (!(fabs(fsim[0] - fsim[i]) <= fatol)) fok = 0;
        if (xok && fok) break;

        double xbar[2], xr[2], fxr;
        for (int k = 0; k < 2; k++) xbar[k] = (sim[0][k] + sim[1][k]) / 2;
        for (int k = 0; k < 2; k++) xr[k] = 2 * xbar[k] - 1 * sim[2][k];
        int aborted = nm_eval(&o, xr, &fxr);
        if (!aborted) {
            int doshrink = 0;
            if (fxr < fsim[0]) {
                double xe[2], fxe;
                for (int k = 0; k < 2; k++) xe[k] = 3 * xbar[k] - 2 * sim[2][k];
                aborted = nm_eval(&o, xe, &fxe);
                if (!aborted) {
                    if (fxe < fxr) {
                        sim[2][0] = xe[0]; sim[2][1] = xe[1]; fsim[2] = fxe;
                    } else {
                        sim[2][0] = xr[0]; sim[2][1] = xr[1]; fsim[2] = fxr;
                    }
                }
            } else {
                if (fxr < fsim[1]) {
                    sim[2][0] = xr[0]; sim[2][1] = xr[1]; fsim[2] = fxr;
                } else {
                    if (fxr < fsim[2]) {
                        double xc[2], fxc;
                        for (int k = 0; k < 2; k++) xc[k] = 1.5 * xbar[k] - 0.5 * sim[2][k];
                        aborted = nm_eval(&o, xc, &fxc);
                        if (!aborted) {
                            if (fxc <= fxr) {
                                sim[2][0] = xc[0]; sim[2][1] = xc[1]; fsim[2] = fxc;
                            } else {
                                doshrink = 1;
                            }
                        }
                    } else {
                        double xcc[2], fxcc;
                        for (int k = 0; k < 2; k++) xcc[k] = 0.5 * xbar[k] + 0.5 * sim[2][k];
                        aborted = nm_eval(&o, xcc, &fxcc);
                        if (!aborted) {
                            if (fxcc < fsim[2]) {
                                sim[2][0] = xcc[0]; sim[2][1] = xcc[1]; fsim[2] = fxcc;
                            } else {
                                doshrink = 1;
                            }
                        }
                    }
                    if (!aborted && doshrink) {
                        for (int j = 1; j < 3 && !aborted; j++) {
                            for (int k = 0; k < 2; k++)
                                sim[j][k] = sim[0][k] + 0.5 * (sim[j][k] - sim[0][k]);
                            aborted = nm_eval(&o, sim[j], &fsim[j]);
                        }
                    }
                }
            }
            if (!aborted) iterations += 1;
        }
        nm_sort(sim, fsim);
    }
    th_out[0] = sim[0][0];
    th_out[1] = sim[0][1];
    /* np.min(fsim): the sorted head, NaN-propagating (log_lik never returns NaN)         */
    *fval = (isnan(fsim[1]) || isnan(fsim[2])) ? NAN : fsim[0];
    *nfev = o.fcalls;
}

typedef struct {
    int m;
    const double *D2;
    const double *y;
    double jit;
} nlml_ctx_t;

static double nlml_fn(const double *x, void *vctx) {
    const nlml_ctx_t *c = (const nlml_ctx_t *)vctx;
    return orc_nlml(c->m, c->D2, c->y, x[0], x[1], c->jit);
}

/* one hyper-parameter fit: NNGP_p._get_opt_par / opt_theta (models.py:228-260)              */
void orc_nm_fit(int m, const double *D2, const double *y, const double th0[2], double jit,
                double fatol, double xatol, int maxfev, double th_out[2], double *fval,
                int *nfev) {
    nlml_ctx_t ctx = {m, D2, y, jit};
    orc_nm_core(nlml_fn, &ctx, th0, fatol, xatol, maxfev, th_out, fval, nfev);
}

/* kNN: sequential squared distance (scipy cdist sqeuclidean), ascending (dist, index).      */
void orc_knn(const double *X, int64_t rows, int d, const double *q, int m, int32_t *idx,
             double *dist_out) {
    double *dist = (double *)malloc(sizeof(double) * rows);
    for (int64_t r = 0; r < rows; r++) {
        double s = 0.0;
        for (int c = 0; c < d; c++) {
            const double t = q[c] - X[r * d + c];
            s = s + t * t;
        }
        dist[r] = s;
    }
    double pd = -INFINITY;
    int64_t pi = -1;
    for (int k = 0; k < m; k++) {
        double bd = 0;
        int64_t bi = -1;
        for (int64_t r = 0; r < rows; r++) {
            const double v = dist[r];
            /* strictly after (pd, pi) in (dist, index) order; NaN sorts last               */
            int after = (v > pd) || (v == pd && r > pi) || (isnan(v) && !isnan(pd)) ||
                        (isnan(v) && isnan(pd) && r > pi);
            if (!after) continue;
            if (bi < 0 || v < bd || (v == bd && r < bi) || (isnan(bd) && !isnan(v))) {
                bd = v;
                bi = r;
            }
        }
        idx[k] = (int32_t)bi;
        if (dist_out) dist_out[k] = bd;
        pd = bd;
        pi = bi;
    }
    free(dist);
}

/* One NNGP_p.predict (models.py:171-226).  theta0: [d*nj*R][2] in product(coord, jitter,
 * restart) order; jit_exp: [nj] exponents.  fits_out: [n_fits][4] or NULL.                 */
int orc_predict(const double *X, const double *Y, int64_t rows, int d, const double *q, int m,
                int nj, const double *jit_exp, int R, const double *theta0, double fatol,
                double xatol, int maxfev, double *preds, double *fits_out, int nthreads) {
    if (m < 1 || m > 64 || m > rows) return -1;   /* the GPU path's bound (m <= 64) */
    int32_t *idx = (int32_t *)malloc(sizeof(int32_t) * m);
    double *xm = (double *)malloc(sizeof(double) * m * d);
    double *ymT = (double *)malloc(sizeof(double) * m * d); /* [d][m] */
    double *D2 = (double *)malloc(sizeof(double) * m * m);
    double *kd2 = (double *)malloc(sizeof(double) * m);
    double *scr = (double *)malloc(sizeof(double) * d);
    const int nf = d * nj * R;
    double *fits = (double *)malloc(sizeof(double) * nf * 4);
    orc_knn(X, rows, d, q, m, idx, NULL);
    for (int r = 0; r < m; r++)
        for (int c = 0; c < d; c++) {
            xm[r * d + c] = X[(int64_t)idx[r] * d + c];
            ymT[c * m + r] = Y[(int64_t)idx[r] * d + c];
        }
    for (int r = 0; r < m; r++)
        for (int j = 0; j < m; j++) D2[r * m + j] = orc_sqdist_pairwise(xm + r * d, xm + j * d, d, scr);
    for (int r = 0; r < m; r++) kd2[r] = orc_sqdist_pairwise(xm + r * d, q, d, scr);
    double jit[64];
    for (int a = 0; a < nj; a++) jit[a] = pow(10.0, jit_exp[a]);
#ifdef _OPENMP
    if (nthreads > 0) omp_set_num_threads(nthreads);
#pragma omp parallel for schedule(dynamic, 4)
#endif
    for (int f = 0; f < nf; f++) {
        const int c = f / (nj * R), a = (f / R) % nj;
        double th[2], fv;
        int ne;
        orc_nm_fit(m, D2, ymT + c * m, theta0 + 2 * f, jit[a], fatol, xatol, maxfev, th, &fv, &ne);
        fits[4 * f + 0] = th[0];
        fits[4 * f + 1] = th[1];
        fits[4 * f + 2] = fv;
        fits[4 * f + 3] = ne;
    }
    for (int c = 0; c < d; c++) {
        int best = c * nj * R;
        for (int f = best + 1; f < (c + 1) * nj * R; f++)
            if (fits[4 * f + 2] < fits[4 * best + 2]) best = f;
        const int a = (best / R) % nj;
        preds[c] = orc_gp_mean_one(m, D2, kd2, ymT + c * m, fits[4 * best], fits[4 * best + 1], jit[a]);
    }
    if (fits_out) memcpy(fits_out, fits, sizeof(double) * nf * 4);
    free(idx); free(xm); free(ymT); free(D2); free(kd2); free(scr); free(fits);
    return 0;
}

/* helper for tests: D2 of a given xm with the oracle's pairwise order                       */
void orc_d2(const double *xm, int m, int d, double *D2) {
    double *scr = (double *)malloc(sizeof(double) * d);
    for (int r = 0; r < m; r++)
        for (int j = 0; j < m; j++) D2[r * m + j] = orc_sqdist_pairwise(xm + r * d, xm + j * d, d, scr);
    free(scr);
}

int orc_max_threads(void) {
#ifdef _OPENMP
    return omp_get_max_threads();
#else
    return 1;
#endif
}
