// nngp_rk_adapt.hip -- batched adaptive Runge-Kutta fine propagator (RK23 / RK45) for gfx950.
//
// Replaces the reference's SolverScipy.run_F -> scipy.integrate.solve_ivp(f, [t0, t1], u0,
// method, t_eval=(t1,), max_step=(t1-t0)/Nf, **kwargs) (solver.py:138-145), fanned over the
// unconverged slices by pool.map at parareal.py:310-315.  One launch integrates ALL slices; every
// slice runs its own step-size control.
//
// The arithmetic is the contract of DESIGN.md 3.2d, whose normative text is tests/adaptive_ref.py:
// scipy 1.15's RungeKutta._step_impl / rk_step / select_initial_step / norm for the forward
// direction with every sum in a fixed order, the two powers as nn_exp(e * nn_log(x)) (nngp_math.h),
// IEEE division and square root.  Both kernel forms below hold it bit for bit.  Exact build only
// (-ffp-contract=off): there is no contracted form of this file.
//
// Two kernel shapes, chosen as nngp_rk_batch chooses (nngp_rk_kernels.h), on the same right-hand
// sides:
//   * lane kernel  (the seven ODEs; PolyODE with d <= 4 and at most 16 terms; FuncODE with at most 4 atoms besides): one lane = one
//     slice, y, y_new and the S + 1 stage derivatives in VGPRs, no LDS, no barriers.  The lanes
//     of a wave take different numbers of steps and reject independently (divergent control flow
//     under the exec mask); a finished lane idles until its wave's last lane ends.
//   * field kernel (Burgers, FHN-PDE, DiffReact, PolyODE and FuncODE up to d = 2048): one workgroup = one
//     slice, thread t owns elements t, t + BT, ... (at most 4 per thread), stage images in a
//     double-buffered LDS array exactly as rk_field_kernel.  The error norm is reduced by wave 0
//     from an LDS array of squares; thread 0 alone runs the controller and publishes the next
//     attempt's step, the accept flag and the exit code through LDS, so every thread of the
//     workgroup takes the same branch at every barrier by construction (uniformity, below).
//
// Termination: every pass of a slice's loop either leaves it or counts one attempted step, and
// the loop is left once max_attempts steps have been attempted -- whatever the arithmetic does
// (NaN included: a NaN error norm fails `norm < 1`, shrinks h by MIN_FACTOR and ends in status 1
// after a few dozen attempts; a NaN step size is clipped to max_step first).

#include <algorithm>
#include <cmath>
#include <type_traits>

#include "common.h"
#include "nngp_math.h"
#include "tableau.h"

#define NNGP_RK_VARIANT exact

namespace nngp {
inline namespace NNGP_RK_VARIANT {

#include "nngp_rk_dev.h"
// the fixed-step dispatch's own thread choice (pick_threads) is not used here: adapt_threads below
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"
#include "nngp_rk_kernels.h"
#pragma clang diagnostic pop

// ---------------------------------------------------------------------------------------------
// Embedded pairs: the published rationals evaluated in double (the same expressions as
// tests/adaptive_ref.py).  A: stage coefficients, B: the propagated solution, E: the error
// estimate over K_0 .. K_S (K_S = f(y_new), first-same-as-last).
// ---------------------------------------------------------------------------------------------
template <int METHOD> struct AdTab;

template <> struct AdTab<NNGP_RK23> {    // Bogacki-Shampine 3(2)
    static constexpr int S = 3;
    static constexpr int ERR_ORDER = 2;
    static constexpr double A[3][3] = {{0.0, 0.0, 0.0}, {1.0 / 2, 0.0, 0.0}, {0.0, 3.0 / 4, 0.0}};
    static constexpr double B[3] = {2.0 / 9, 1.0 / 3, 4.0 / 9};
    static constexpr double E[4] = {5.0 / 72, -1.0 / 12, -1.0 / 9, 1.0 / 8};
};
template <> struct AdTab<NNGP_RK45> {    // Dormand-Prince 5(4)
    static constexpr int S = 6;
    static constexpr int ERR_ORDER = 4;
    static constexpr double A[6][6] = {
        {0.0, 0.0, 0.0, 0.0, 0.0, 0.0},
        {1.0 / 5, 0.0, 0.0, 0.0, 0.0, 0.0},
        {3.0 / 40, 9.0 / 40, 0.0, 0.0, 0.0, 0.0},
        {44.0 / 45, -56.0 / 15, 32.0 / 9, 0.0, 0.0, 0.0},
        {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0.0, 0.0},
        {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656, 0.0}};
    static constexpr double B[6] = {35.0 / 384, 0.0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84};
    static constexpr double E[7] = {-71.0 / 57600, 0.0, 71.0 / 16695, -71.0 / 1920, 17253.0 / 339200,
                                    -22.0 / 525, 1.0 / 40};
};

constexpr double AD_SAFETY = 0.9, AD_MIN_FACTOR = 0.2, AD_MAX_FACTOR = 10.0;

// sum_j coef_j K_j over the non-zero coef_j in ascending j, the first term starting the sum
// (stage_input's convention); K is indexed k[j * KS + c], s a compile-time constant after unrolling
template <typename T, int KS>
__device__ __forceinline__ double ad_sum_a(int s, const double *k, int c) {
    double t = 0.0;
    bool first = true;
#pragma unroll
    for (int j = 0; j < T::S; j++) {
        if (j >= s || T::A[s][j] == 0.0) continue;
        const double v = T::A[s][j] * k[j * KS + c];
        t = first ? v : t + v;
        first = false;
    }
    return t;
}
template <typename T, int KS>
__device__ __forceinline__ double ad_sum_b(const double *k, int c) {
    double t = 0.0;
    bool first = true;
#pragma unroll
    for (int j = 0; j < T::S; j++) {
        if (T::B[j] == 0.0) continue;
        const double v = T::B[j] * k[j * KS + c];
        t = first ? v : t + v;
        first = false;
    }
    return t;
}
template <typename T, int KS>
__device__ __forceinline__ double ad_sum_e(const double *k, int c) {
    double t = 0.0;
    bool first = true;
#pragma unroll
    for (int j = 0; j <= T::S; j++) {
        if (T::E[j] == 0.0) continue;
        const double v = T::E[j] * k[j * KS + c];
        t = first ? v : t + v;
        first = false;
    }
    return t;
}

// Python's min / max of two: the first unless the second compares less / greater (a NaN never does)
__device__ __forceinline__ double py_min(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double py_max(double a, double b) { return b > a ? b : a; }

// np.maximum(|a|, |b|): a NaN on either side comes through (fmax would drop it)
__device__ __forceinline__ double ad_max_abs(double a, double b) {
    const double x = fabs(a), y = fabs(b);
    return (x != x) ? x : ((y > x || y != y) ? y : x);
}

// x ** e of the contract
__device__ __forceinline__ double ad_pow(double x, double e) { return nn_exp(e * nn_log(x)); }

// 10 * |nextafter(t, inf) - t|
__device__ __forceinline__ double ad_min_step(double t) {
    const long long b = __double_as_longlong(t);
    const double nx = (t == 0.0) ? __longlong_as_double(1LL) : __longlong_as_double(t > 0.0 ? b + 1 : b - 1);
    return 10 * fabs(nx - t);
}

// ---------------------------------------------------------------------------------------------
// The controller of one slice: scipy's _step_impl around the Runge-Kutta attempt, restated so
// that one loop pass is one attempted step.  The lane form holds one per lane, the field form
// one in thread 0 of the slice's workgroup.
// ---------------------------------------------------------------------------------------------
enum { AD_GO = 0, AD_TOO_SMALL = 1, AD_CAP = 2, AD_DONE = 3 };

template <typename T> struct AdCtl {
    double t, t1, h_abs, max_step, min_step, t_new;
    int64_t attempts, max_attempts, nfev, acc, rej;
    bool fresh, rejected;

    __device__ __forceinline__ void init(double T0, double T1, int64_t nf, int64_t cap) {
        t = T0;
        t1 = T1;
        max_step = (T1 - T0) / (double)nf;
        h_abs = min_step = t_new = 0.0;
        attempts = nfev = acc = rej = 0;
        max_attempts = cap;
        fresh = true;
        rejected = false;
    }
    // select_initial_step's two ends around the evaluation of f(y0 + h0 f0)
    __device__ __forceinline__ double first_guess(double d0, double d1) const {
        const double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
        return py_min(h0, t1 - t);
    }
    __device__ __forceinline__ void initial_step(double h0, double d1, double d2_sum_norm) {
        const double d2 = d2_sum_norm / h0;
        double h1;
        if (d1 <= 1e-15 && d2 <= 1e-15)
            h1 = py_max(1e-6, h0 * 1e-3);
        else
            h1 = ad_pow(0.01 / py_max(d1, d2), 1.0 / (T::ERR_ORDER + 1));
        h_abs = py_min(py_min(py_min(100 * h0, h1), t1 - t), max_step);
    }
    // the head of an attempted step: AD_GO and its h, or the slice's exit code
    __device__ __forceinline__ int attempt(double &h) {
        if (fresh) {   // the start of _step_impl
            min_step = ad_min_step(t);
            if (!(h_abs <= max_step))   // > max_step, or NaN (scipy keeps a NaN and never ends)
                h_abs = max_step;
            else if (h_abs < min_step)
                h_abs = min_step;
            rejected = false;
            fresh = false;
        }
        if (h_abs < min_step) return AD_TOO_SMALL;
        if (attempts >= max_attempts) return AD_CAP;
        attempts++;
        t_new = t + h_abs;
        if (t_new - t1 > 0) t_new = t1;
        h = t_new - t;
        h_abs = fabs(h);
        nfev += T::S;
        return AD_GO;
    }
    // the tail: whether the attempt is accepted; AD_DONE once an accepted step has reached t1
    __device__ __forceinline__ bool judge(double en, int &code) {
        const double expo = -1.0 / (T::ERR_ORDER + 1);
        code = AD_GO;
        if (en < 1) {
            double factor = (en == 0) ? AD_MAX_FACTOR : py_min(AD_MAX_FACTOR, AD_SAFETY * ad_pow(en, expo));
            if (rejected) factor = py_min(1.0, factor);
            h_abs = h_abs * factor;
            acc++;
            t = t_new;
            fresh = true;
            if (!(t < t1)) code = AD_DONE;
            return true;
        }
        h_abs = h_abs * py_max(AD_MIN_FACTOR, AD_SAFETY * ad_pow(en, expo));
        rejected = true;
        rej++;
        return false;
    }
    __device__ __forceinline__ void write_stats(int64_t *row, int code) const {
        row[0] = (code == AD_TOO_SMALL || code == AD_CAP) ? code : 0;
        row[1] = nfev;
        row[2] = acc;
        row[3] = rej;
    }
};

// the contract's sum of squares for d <= 4: columns (x0 + x2) + (x1 + x3), absent ones +0.0
template <int D>
__device__ __forceinline__ double lane_rms(const double *v) {
    double x[D];
#pragma unroll
    for (int c = 0; c < D; c++) x[c] = v[c] * v[c];
    double s;
    if constexpr (D == 1) s = x[0];
    else if constexpr (D == 2) s = x[0] + x[1];
    else if constexpr (D == 3) s = (x[0] + x[2]) + x[1];
    else s = (x[0] + x[2]) + (x[1] + x[3]);
    return sqrt(s / (double)D);
}

// ---------------------------------------------------------------------------------------------
// lane form
// ---------------------------------------------------------------------------------------------
struct AdArgs {
    int n_slices;
    const double *t0, *t1;
    int64_t nf;
    double rtol, atol, first_step;
    int64_t max_attempts;
    const double *u0;   // may alias uF: a slice reads its row before it writes it
    double *uF;
    int64_t *stats;     // [n][4] or null
};

template <int SYS, int METHOD, bool NORM, class A>
__device__ __forceinline__ void ad_lane_slice(A args, const AdArgs &a, int i) {
    using T = AdTab<METHOD>;
    constexpr int S = T::S;
    constexpr int D = LaneSys<SYS>::D;
    if constexpr (NORM) {
#pragma unroll
        for (int c = 0; c < D; c++) {
            args.mn[c] = args.norm[c];
            args.hw[c] = 0.5 * args.norm[D + c];
            args.sc[c] = args.norm[2 * D + c];
        }
    }
    double y[D], yn[D], K[(S + 1) * D], tmp[D];
#pragma unroll
    for (int c = 0; c < D; c++) y[c] = a.u0[(size_t)i * D + c];
    AdCtl<T> ctl;
    ctl.init(a.t0[i], a.t1[i], a.nf, a.max_attempts);
    int code = AD_DONE;
    if (ctl.t < ctl.t1) {
        lane_rhs<SYS, NORM>(y, K, args);
        ctl.nfev = 1;
        if (a.first_step == 0.0) {   // select_initial_step
            double sc[D];
#pragma unroll
            for (int c = 0; c < D; c++) {
                sc[c] = a.atol + fabs(y[c]) * a.rtol;
                tmp[c] = y[c] / sc[c];
            }
            const double d0 = lane_rms<D>(tmp);
#pragma unroll
            for (int c = 0; c < D; c++) tmp[c] = K[c] / sc[c];
            const double d1 = lane_rms<D>(tmp);
            const double h0 = ctl.first_guess(d0, d1);
#pragma unroll
            for (int c = 0; c < D; c++) tmp[c] = y[c] + h0 * K[c];
            lane_rhs<SYS, NORM>(tmp, K + S * D, args);
            ctl.nfev = 2;
#pragma unroll
            for (int c = 0; c < D; c++) tmp[c] = (K[S * D + c] - K[c]) / sc[c];
            ctl.initial_step(h0, d1, lane_rms<D>(tmp));
        } else {
            ctl.h_abs = a.first_step;
        }
        for (;;) {
            double h;
            code = ctl.attempt(h);
            if (code != AD_GO) break;
#pragma unroll
            for (int s = 1; s < S; s++) {
#pragma unroll
                for (int c = 0; c < D; c++) tmp[c] = y[c] + ad_sum_a<T, D>(s, K, c) * h;
                lane_rhs<SYS, NORM>(tmp, K + s * D, args);
            }
#pragma unroll
            for (int c = 0; c < D; c++) yn[c] = y[c] + h * ad_sum_b<T, D>(K, c);
            lane_rhs<SYS, NORM>(yn, K + S * D, args);
#pragma unroll
            for (int c = 0; c < D; c++) {
                const double scale = a.atol + ad_max_abs(y[c], yn[c]) * a.rtol;
                tmp[c] = ad_sum_e<T, D>(K, c) * h / scale;
            }
            if (ctl.judge(lane_rms<D>(tmp), code)) {
#pragma unroll
                for (int c = 0; c < D; c++) {
                    y[c] = yn[c];
                    K[c] = K[S * D + c];
                }
            }
            if (code != AD_GO) break;
        }
    }
#pragma unroll
    for (int c = 0; c < D; c++) a.uF[(size_t)i * D + c] = y[c];
    if (a.stats) ctl.write_stats(a.stats + (size_t)i * 4, code);
}

template <int SYS, int METHOD, bool NORM>
__global__ void __launch_bounds__(64) rk_adapt_lane_kernel(LaneArgs args, AdArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_slices) return;
    ad_lane_slice<SYS, METHOD, NORM>(args, a, i);
}

template <int D, int METHOD, bool NORM>
__global__ void __launch_bounds__(64) rk_adapt_poly_lane_kernel(PolyLaneArgs args, AdArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_slices) return;
    ad_lane_slice<NNGP_SYS_POLY_LANE + D, METHOD, NORM>(args, a, i);
}

template <int D, int METHOD, bool NORM>
__global__ void __launch_bounds__(64) rk_adapt_func_lane_kernel(FuncLaneArgs args, AdArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_slices) return;
    ad_lane_slice<NNGP_SYS_FUNC_LANE + D, METHOD, NORM>(args, a, i);
}

// ---------------------------------------------------------------------------------------------
// field form
//
// LDS: [2][d] stage images (NNGP_SYS_FUNC: [2][d + n_atoms], and a second barrier per evaluation of
// f, behind the atoms: func_atoms_stage) | sq[EPT * BT] squares | ctl[2] = the next attempt's h, 8 * accept +
// exit code.  Barriers per attempted step: one per evaluation of f (S of them) and the two of the
// norm -- after the squares are written, and after thread 0 has published ctl.
//
// Uniformity: t, h_abs, the accept flag, the exit code and the attempt count exist in thread 0
// only.  What the other threads branch on -- h, accept, code -- they read from ctl after the
// barrier that follows thread 0's write, and the next write lies behind the next attempt's
// barriers, so all threads of the workgroup read the same words and reach every __syncthreads()
// together or not at all.  The only branches around a barrier are on those words, on kernel
// arguments and on t0 < t1 (the slice's, loaded by every thread from the same address).
// ---------------------------------------------------------------------------------------------
template <int SYS, int EPT, bool NORM> struct AdField {
    const FieldArgs &fa;
    int d, half, buf, W;   // W: doubles per image
    double *img;
    int e_[EPT];
    double mn[EPT], w[EPT], sc[EPT];
    Nbr5 nb[(SYS == NNGP_SYS_FHN_PDE) ? EPT : 1];
    DrNbr rnb[(SYS == NNGP_SYS_DIFFREACT) ? EPT : 1];
    int pb[table_sys(SYS) ? EPT : 1], pe[table_sys(SYS) ? EPT : 1];
    int tid_, BT_;
    const nngp_func_atom *fatoms;

    __device__ __forceinline__ AdField(const FieldArgs &fa_, double *img_, int tid, int BT)
        : fa(fa_), d(fa_.d), half(fa_.d / 2), buf(0), W(image_doubles<SYS>(fa_)), img(img_), tid_(tid), BT_(BT), fatoms(nullptr) {
        if constexpr (SYS == NNGP_SYS_FUNC) fatoms = func_atoms_of(fa_);
#pragma unroll
        for (int r = 0; r < EPT; r++) {
            const int e = tid + r * BT;
            e_[r] = e;
            const bool ok = e < d;
            if constexpr (table_sys(SYS)) {
                pb[r] = ok ? fa.p_row[e] : 0;
                pe[r] = ok ? fa.p_row[e + 1] : 0;
            }
            if (NORM && ok) {
                mn[r] = fa.norm[e];
                w[r] = 0.5 * fa.norm[d + e];   // (mx-mn)/2, see lane_rhs
                sc[r] = fa.norm[2 * d + e];
            } else {
                mn[r] = 0.0; w[r] = 1.0; sc[r] = 1.0;
            }
            if constexpr (SYS == NNGP_SYS_FHN_PDE) nb[r] = fhn_neighbours(fa.nx, ok ? (e % half) : 0);
            if constexpr (SYS == NNGP_SYS_DIFFREACT) rnb[r] = dr_neighbours(fa, ok ? (e % half) : 0, ok);
        }
    }
    // f_n(x) of the thread's elements: one stage of rk_field_kernel without the h (one barrier)
    __device__ __forceinline__ void rhs(const double *x, double *out) {
        double *V = img + buf * W;
#pragma unroll
        for (int r = 0; r < EPT; r++)
            if (e_[r] < d) V[e_[r]] = NORM ? (x[r] + 1) * w[r] + mn[r] : x[r];
        __syncthreads();
        if constexpr (SYS == NNGP_SYS_FUNC) func_atoms_stage(V, fa, fatoms, tid_, BT_);
#pragma unroll
        for (int r = 0; r < EPT; r++) {
            const int e = e_[r];
            double f = 0.0;
            if (e < d) {
                if constexpr (SYS == NNGP_SYS_BURGERS) {
                    f = burgers_elem(V, e, d, fa);
                } else if constexpr (SYS == NNGP_SYS_DIFFREACT) {
                    f = dr_elem(V, e, half, rnb[r], fa);
                } else if constexpr (table_sys(SYS)) {
                    f = poly_elem(V, pb[r], pe[r], fa.p_terms);
                } else {   // FHN_PDE, systems.py:365-366
                    if (e < half) {
                        const double lu = fhn_lap(V, nb[r], fa.a_off, fa.a_diag);
                        const double u1 = V[e], u1c = u1 * (u1 * u1);
                        f = (((lu + u1) - u1c) - V[half + e]) + -5E-3 * 1.0;
                    } else {
                        const double lv = fhn_lap(V + half, nb[r], fa.b_off, fa.b_diag);
                        f = (1 / 0.1) * ((lv + V[e - half]) - V[e]);
                    }
                }
                if (NORM) f = f * sc[r];
            }
            out[r] = f;
        }
        buf ^= 1;
    }
};

// the first half of a norm: every thread stores its elements' squares (+0.0 past d) and, behind
// the barrier, wave 0 forms the contract's sum -- column l = lane l's sequential sum over the
// elements l, l + 64, ..., then the stride-halving tree -- valid in thread 0.  The caller's thread
// 0 uses it, publishes what follows from it, and closes with the norm's second barrier.
template <int EPT>
__device__ __forceinline__ double field_sumsq(double *sq, const double *v, const int *e_, int d, int tid, int npad) {
#pragma unroll
    for (int r = 0; r < EPT; r++) sq[e_[r]] = (e_[r] < d) ? v[r] * v[r] : 0.0;
    __syncthreads();
    double s = 0.0;
    if (tid < 64) {
        s = sq[tid];
        for (int e = tid + 64; e < npad; e += 64) s = s + sq[e];
#pragma unroll
        for (int w = 32; w >= 1; w >>= 1) s = s + __shfl_down(s, w, 64);
    }
    return s;
}

template <int SYS, int METHOD, int EPT, bool NORM>
__global__ void __launch_bounds__(EPT == 1 ? 256 : 512) rk_adapt_field_kernel(FieldArgs fa, AdArgs a) {
    using T = AdTab<METHOD>;
    constexpr int S = T::S;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int slice = blockIdx.x;
    const int tid = threadIdx.x, BT = blockDim.x;
    const int d = fa.d, npad = EPT * BT;
    double *sq = smem + 2 * image_doubles<SYS>(fa);
    double *pub = sq + npad;   // ctl[2]
    AdField<SYS, EPT, NORM> F(fa, smem, tid, BT);

    double y[EPT], yn[EPT], K[(S + 1) * EPT], tmp[EPT];
#pragma unroll
    for (int r = 0; r < EPT; r++) y[r] = (F.e_[r] < d) ? a.u0[(size_t)slice * d + F.e_[r]] : 0.0;
    AdCtl<T> ctl;   // thread 0's; the other threads' copies are never read
    ctl.init(a.t0[slice], a.t1[slice], a.nf, a.max_attempts);
    int code = AD_DONE;
    if (ctl.t < ctl.t1) {   // workgroup-uniform: the slice's own t0, t1
        const double dd = (double)d;
        F.rhs(y, K);
        ctl.nfev = 1;
        if (a.first_step == 0.0) {   // select_initial_step (a kernel argument: uniform)
            double scl[EPT];
#pragma unroll
            for (int r = 0; r < EPT; r++) {
                scl[r] = a.atol + fabs(y[r]) * a.rtol;
                tmp[r] = y[r] / scl[r];
            }
            double s = field_sumsq<EPT>(sq, tmp, F.e_, d, tid, npad);
            const double d0 = sqrt(s / dd);
            __syncthreads();
#pragma unroll
            for (int r = 0; r < EPT; r++) tmp[r] = K[r] / scl[r];
            s = field_sumsq<EPT>(sq, tmp, F.e_, d, tid, npad);
            const double d1 = sqrt(s / dd);
            if (tid == 0) pub[0] = ctl.first_guess(d0, d1);
            __syncthreads();
            const double h0 = pub[0];
#pragma unroll
            for (int r = 0; r < EPT; r++) tmp[r] = y[r] + h0 * K[r];
            F.rhs(tmp, K + S * EPT);
            ctl.nfev = 2;
#pragma unroll
            for (int r = 0; r < EPT; r++) tmp[r] = (K[S * EPT + r] - K[r]) / scl[r];
            s = field_sumsq<EPT>(sq, tmp, F.e_, d, tid, npad);
            if (tid == 0) ctl.initial_step(h0, d1, sqrt(s / dd));
        } else if (tid == 0) {
            ctl.h_abs = a.first_step;
        }
        if (tid == 0) {
            double h = 0.0;
            const int c = ctl.attempt(h);
            pub[0] = h;
            pub[1] = (double)c;
        }
        __syncthreads();
        double h = pub[0];
        code = (int)pub[1];
        while (code == AD_GO) {
#pragma unroll
            for (int s = 1; s < S; s++) {
#pragma unroll
                for (int r = 0; r < EPT; r++) tmp[r] = y[r] + ad_sum_a<T, EPT>(s, K, r) * h;
                F.rhs(tmp, K + s * EPT);
            }
#pragma unroll
            for (int r = 0; r < EPT; r++) yn[r] = y[r] + h * ad_sum_b<T, EPT>(K, r);
            F.rhs(yn, K + S * EPT);
#pragma unroll
            for (int r = 0; r < EPT; r++) {
                const double scale = a.atol + ad_max_abs(y[r], yn[r]) * a.rtol;
                tmp[r] = ad_sum_e<T, EPT>(K, r) * h / scale;
            }
            const double s = field_sumsq<EPT>(sq, tmp, F.e_, d, tid, npad);   // the norm's first barrier
            if (tid == 0) {
                int c;
                const bool ok = ctl.judge(sqrt(s / dd), c);
                double hn = 0.0;
                if (c == AD_GO) c = ctl.attempt(hn);
                pub[0] = hn;
                pub[1] = (double)(c + (ok ? 8 : 0));
            }
            __syncthreads();   // the norm's second barrier
            h = pub[0];
            const int word = (int)pub[1];
            code = word & 7;
            if (word & 8) {
#pragma unroll
                for (int r = 0; r < EPT; r++) {
                    y[r] = yn[r];
                    K[r] = K[S * EPT + r];
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < EPT; r++)
        if (F.e_[r] < d) a.uF[(size_t)slice * d + F.e_[r]] = y[r];
    if (a.stats && tid == 0) ctl.write_stats(a.stats + (size_t)slice * 4, code);
}

// ---------------------------------------------------------------------------------------------
// host dispatch
// ---------------------------------------------------------------------------------------------
template <int SYS, int METHOD>
static int adapt_lane(const nngp_system *sys, const AdArgs &a, hipStream_t st) {
    LaneArgs la{};
    constexpr int D = LaneSys<SYS>::D;
    NNGP_REQUIRE(sys->d == D, "system kind %d has d=%d, got d=%d", SYS, D, sys->d);
    NNGP_REQUIRE(!sys->normalized || sys->norm != nullptr, "normalized system needs norm[3d]");
    la.normalized = sys->normalized;
    for (int c = 0; c < 4; c++) la.param[c] = sys->param[c];
    la.rparam0 = 1.0 / sys->param[0];
    la.norm = sys->norm;
    const dim3 grid((a.n_slices + 63) / 64);
    if (sys->normalized)
        hipLaunchKernelGGL((rk_adapt_lane_kernel<SYS, METHOD, true>), grid, dim3(64), 0, st, la, a);
    else
        hipLaunchKernelGGL((rk_adapt_lane_kernel<SYS, METHOD, false>), grid, dim3(64), 0, st, la, a);
    NNGP_LAUNCH_CHECK();
    return NNGP_OK;
}

// threads per slice and elements per thread of the field form, by d alone: one element per thread
// up to 256 threads, two up to 512 threads (d <= 1024), four beyond (d <= 2048)
constexpr int AD_FIELD_MAX_D = 2048;
static void adapt_threads(int d, int &bt, int &ept) {
    ept = d <= 256 ? 1 : (d <= 1024 ? 2 : 4);
    bt = ((d + 64 * ept - 1) / (64 * ept)) * 64;
}

template <int SYS, int METHOD, int EPT>
static int adapt_field_ept(const FieldArgs &fa, int bt, const AdArgs &a, hipStream_t st) {
    const size_t lds = sizeof(double) * (2 * (size_t)image_doubles<SYS>(fa) + (size_t)EPT * bt + 2);
    if (fa.normalized)
        hipLaunchKernelGGL((rk_adapt_field_kernel<SYS, METHOD, EPT, true>), dim3(a.n_slices), dim3(bt), lds, st, fa, a);
    else
        hipLaunchKernelGGL((rk_adapt_field_kernel<SYS, METHOD, EPT, false>), dim3(a.n_slices), dim3(bt), lds, st, fa,
                           a);
    NNGP_LAUNCH_CHECK();
    return NNGP_OK;
}

template <int SYS, int METHOD>
static int adapt_field(const nngp_system *sys, const AdArgs &a, hipStream_t st) {
    NNGP_REQUIRE(sys->d >= 1 && sys->d <= AD_FIELD_MAX_D, "the adaptive field kernel takes d <= %d (got d=%d)",
                 AD_FIELD_MAX_D, sys->d);
    FieldArgs fa;
    int rc = field_args(sys, fa);
    if (rc) return rc;
    int bt, ept;
    adapt_threads(sys->d, bt, ept);
    if (ept == 1) return adapt_field_ept<SYS, METHOD, 1>(fa, bt, a, st);
    if (ept == 2) return adapt_field_ept<SYS, METHOD, 2>(fa, bt, a, st);
    return adapt_field_ept<SYS, METHOD, 4>(fa, bt, a, st);
}

template <int KIND, int D, int METHOD, bool NORM>
static auto adapt_table_lane_kernel() {
    if constexpr (KIND == NNGP_SYS_POLY) return &rk_adapt_poly_lane_kernel<D, METHOD, NORM>;
    else return &rk_adapt_func_lane_kernel<D, METHOD, NORM>;
}

template <int KIND, int D, int METHOD>
static int adapt_table_lane(const nngp_system *sys, const Table &tb, const AdArgs &a, hipStream_t st) {
    TableLaneArgs<KIND> la{};
    la.normalized = sys->normalized;
    la.norm = sys->norm;
    lane_tab(tb, la.tab);
    const dim3 grid((a.n_slices + 63) / 64);
    if (sys->normalized)
        hipLaunchKernelGGL((adapt_table_lane_kernel<KIND, D, METHOD, true>()), grid, dim3(64), 0, st, la, a);
    else
        hipLaunchKernelGGL((adapt_table_lane_kernel<KIND, D, METHOD, false>()), grid, dim3(64), 0, st, la, a);
    NNGP_LAUNCH_CHECK();
    return NNGP_OK;
}

// NNGP_SYS_POLY / NNGP_SYS_FUNC: the lane form while the table fits the kernel arguments, else the
// field form (launch_table); tb is the table nngp_rk_adaptive looked up
template <int KIND, int METHOD>
static int adapt_table(const nngp_system *sys, const Table &tb, const AdArgs &a, hipStream_t st) {
    NNGP_REQUIRE(!sys->normalized || sys->norm != nullptr, "normalized system needs norm[3d]");
    if (!lane_fits(tb)) return adapt_field<KIND, METHOD>(sys, a, st);
    switch (tb.d) {
    case 1: return adapt_table_lane<KIND, 1, METHOD>(sys, tb, a, st);
    case 2: return adapt_table_lane<KIND, 2, METHOD>(sys, tb, a, st);
    case 3: return adapt_table_lane<KIND, 3, METHOD>(sys, tb, a, st);
    default: return adapt_table_lane<KIND, 4, METHOD>(sys, tb, a, st);
    }
}

// tb: the table of a table-backed kind, unused by the others
template <int METHOD>
static int adapt_sys(const nngp_system *s, const Table &tb, const AdArgs &a, hipStream_t st) {
    switch (s->kind) {
    case NNGP_SYS_LORENZ: return adapt_lane<NNGP_SYS_LORENZ, METHOD>(s, a, st);
    case NNGP_SYS_HOPF: return adapt_lane<NNGP_SYS_HOPF, METHOD>(s, a, st);
    case NNGP_SYS_THOMAS_LABYRINTH: return adapt_lane<NNGP_SYS_THOMAS_LABYRINTH, METHOD>(s, a, st);
    case NNGP_SYS_FHN_ODE: return adapt_lane<NNGP_SYS_FHN_ODE, METHOD>(s, a, st);
    case NNGP_SYS_ROSSLER: return adapt_lane<NNGP_SYS_ROSSLER, METHOD>(s, a, st);
    case NNGP_SYS_BRUSSELATOR: return adapt_lane<NNGP_SYS_BRUSSELATOR, METHOD>(s, a, st);
    case NNGP_SYS_DBL_PEND: return adapt_lane<NNGP_SYS_DBL_PEND, METHOD>(s, a, st);
    case NNGP_SYS_BURGERS: return adapt_field<NNGP_SYS_BURGERS, METHOD>(s, a, st);
    case NNGP_SYS_FHN_PDE: return adapt_field<NNGP_SYS_FHN_PDE, METHOD>(s, a, st);
    case NNGP_SYS_DIFFREACT: return adapt_field<NNGP_SYS_DIFFREACT, METHOD>(s, a, st);
    case NNGP_SYS_POLY: return adapt_table<NNGP_SYS_POLY, METHOD>(s, tb, a, st);
    case NNGP_SYS_FUNC: return adapt_table<NNGP_SYS_FUNC, METHOD>(s, tb, a, st);
    default: set_error("unknown system kind %d", s->kind); return NNGP_E_ARG;
    }
}

}  // namespace NNGP_RK_VARIANT
}  // namespace nngp

extern "C" int nngp_rk_adaptive(const nngp_system *sys, int method, int n_slices, const double *t0,
                                const double *t1, int64_t nf, double rtol, double atol, double first_step,
                                int64_t max_attempts, const double *u0, double *uF, int64_t *stats,
                                void *stream) {
    using namespace nngp;
    // every argument check comes before any HIP call
    NNGP_REQUIRE(sys != nullptr, "sys is NULL");
    NNGP_REQUIRE(method == NNGP_RK23 || method == NNGP_RK45, "unknown adaptive method %d (NNGP_RK23 = 23, "
                 "NNGP_RK45 = 45)", method);
    NNGP_REQUIRE(n_slices >= 0, "n_slices < 0");
    NNGP_REQUIRE(nf >= 1, "nf must be >= 1 (got %lld)", (long long)nf);
    NNGP_REQUIRE(std::isfinite(rtol) && rtol > 0, "rtol must be finite and > 0 (got %g)", rtol);
    NNGP_REQUIRE(std::isfinite(atol) && atol >= 0, "atol must be finite and >= 0 (got %g)", atol);
    NNGP_REQUIRE(std::isfinite(first_step) && first_step >= 0, "first_step must be finite and >= 0, 0 = choose "
                 "(got %g)", first_step);
    NNGP_REQUIRE(max_attempts >= 1, "max_attempts must be >= 1 (got %lld)", (long long)max_attempts);
    Table tb{};
    if (table_sys(sys->kind)) {
        int rc = table_lookup(sys, &tb);   // an unknown or destroyed handle, or another d
        if (rc) return rc;
    }
    if (n_slices == 0) return NNGP_OK;
    NNGP_REQUIRE(t0 && t1 && u0 && uF, "null array argument");
    const AdArgs a{n_slices, t0, t1, nf, rtol, atol, first_step, max_attempts, u0, uF, stats};
    hipStream_t st = (hipStream_t)stream;
    if (method == NNGP_RK23) return adapt_sys<NNGP_RK23>(sys, tb, a, st);
    return adapt_sys<NNGP_RK45>(sys, tb, a, st);
}
