// nngp_rk.hip -- batched fine/coarse Runge-Kutta propagator for gfx950 (MI355X).
//
// Replaces the reference's per-slice fine solve SolverRK.run_F -> RK.run_get_last ->
// _RK_jax_last (solver.py:86-107, RK.py:101-109, 146-174), fanned over the unconverged slices by
// pool.map at parareal.py:310-315 (legacy: RK_last / RK_jax_, new_lib.py:57-137, 939-945).
//
// One launch integrates ALL slices of one Parareal iteration.  Two kernel shapes:
//   * lane kernel  (ODEs, d <= 4): one lane = one slice, state + all S stage vectors in VGPRs,
//     no LDS, no barriers.  The RHS is a handful of dependent fp64 ops, so a slice is a serial
//     chain of 10^3..10^9 RK steps: this shape is latency-bound by construction.
//   * field kernel (Burgers d=nx, FHN-PDE and DiffReact d=2 nx^2): one workgroup = one slice,
//     thread t owns elements t, t+BT, ... (EPT per thread, u and the S stage vectors in VGPRs;
//     from 16x16 points the two 2-D fields run one thread per grid point).  The stage input
//     is staged (already inverse-normalised) in a double-buffered LDS image so the stencil reads
//     neighbours from LDS; exactly one __syncthreads per stage.
// HBM traffic is 16*d bytes per slice per launch (read u0, write uF); everything else stays on
// chip, so the roofline is FP64 VALU, not HBM.
//
// Numerics: compiled with -ffp-contract=off; every add/mul is rounded in the order of the
// reference expression it restates (cited inline).  Zero tableau entries are skipped at compile
// time, which is exact for finite stages (t + 0*k == t).
//
// The kernels and their host dispatch live in nngp_rk_kernels.h, which nngp_rk_traj.hip (the
// sampled-trajectory entry, nngp_rk_traj) instantiates a second time with sampling compiled in;
// this file instantiates the end-state propagators and holds the rest of the RK C-ABI.
//
// This file is compiled TWICE (csrc/Makefile): the exact build above, and -- with NNGP_RK_FMA
// defined and -ffp-contract=fast -- the opt-in contracted propagator (NNGP_STEP_CONTRACT,
// include/nngp.h): the same kernels with every a*b+c fused, in the inline namespace `contracted`
// so the two code objects' kernels never share a symbol.  Only the exact build exports the C-ABI;
// the contracted one exports nngp_rk_dispatch_contracted, which nngp_rk_batch calls.

#include <algorithm>
#include <type_traits>

#include "common.h"
#include "nngp_math.h"
#include "tableau.h"

#ifdef NNGP_RK_FMA
#define NNGP_RK_VARIANT contracted
#else
#define NNGP_RK_VARIANT exact
#endif

namespace nngp {
inline namespace NNGP_RK_VARIANT {

#include "nngp_rk_dev.h"
#include "nngp_rk_kernels.h"

// ---------------------------------------------------------------------------------------------
// single RHS evaluations (ODE.get_vector_field()(t, u)) and the elementwise Parareal update
// ---------------------------------------------------------------------------------------------
template <int SYS>
__global__ void __launch_bounds__(64) rhs_lane_kernel(LaneArgs args, int n, const double *__restrict__ u,
                                                      double *__restrict__ out) {
    constexpr int D = LaneSys<SYS>::D;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (args.normalized)
        for (int c = 0; c < D; c++) {
            args.mn[c] = args.norm[c];
            args.hw[c] = 0.5 * args.norm[D + c];
            args.sc[c] = args.norm[2 * D + c];
        }
    double x[D], o[D];
    for (int c = 0; c < D; c++) x[c] = u[(size_t)i * D + c];
    if (args.normalized)
        lane_rhs<SYS, true>(x, o, args);
    else
        lane_rhs<SYS, false>(x, o, args);
    for (int c = 0; c < D; c++) out[(size_t)i * D + c] = o[c];
}

template <int SYS>
__global__ void __launch_bounds__(256) rhs_field_kernel(FieldArgs fa, const double *__restrict__ u,
                                                        double *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double V[];
    const int d = fa.d, half = d / 2, s = blockIdx.x;
    for (int e = threadIdx.x; e < d; e += blockDim.x) {
        const double x = u[(size_t)s * d + e];
        V[e] = fa.normalized ? ((x + 1) / 2) * fa.norm[d + e] + fa.norm[e] : x;
    }
    __syncthreads();
    if constexpr (SYS == NNGP_SYS_FUNC) func_atoms_stage(V, fa, func_atoms_of(fa), threadIdx.x, blockDim.x);
    for (int e = threadIdx.x; e < d; e += blockDim.x) {
        double f;
        if constexpr (SYS == NNGP_SYS_BURGERS) {
            f = burgers_elem(V, e, d, fa);
        } else if constexpr (SYS == NNGP_SYS_DIFFREACT) {
            f = dr_elem(V, e, half, dr_neighbours(fa, e < half ? e : e - half, true), fa);
        } else if constexpr (table_sys(SYS)) {
            f = poly_elem(V, fa.p_row[e], fa.p_row[e + 1], fa.p_terms);
        } else if (e < half) {
            const Nbr5 nb = fhn_neighbours(fa.nx, e);
            const double u1 = V[e];
            f = (((fhn_lap(V, nb, fa.a_off, fa.a_diag) + u1) - u1 * (u1 * u1)) - V[half + e]) + -5E-3 * 1.0;
        } else {
            const Nbr5 nb = fhn_neighbours(fa.nx, e - half);
            f = (1 / 0.1) * ((fhn_lap(V + half, nb, fa.b_off, fa.b_diag) + V[e - half]) - V[e]);
        }
        out[(size_t)s * d + e] = fa.normalized ? f * fa.norm[2 * d + e] : f;
    }
}

__global__ void __launch_bounds__(256) update_kernel(int64_t n, const double *__restrict__ a,
                                                     const double *__restrict__ b,
                                                     const double *__restrict__ c,
                                                     double *__restrict__ out) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const double p = a[i] - b[i];
        out[i] = c ? p + c[i] : p;
    }
}


template <int SYS>
static int launch_rhs_lane(const nngp_system *sys, int n, const double *u, double *out, hipStream_t st) {
    LaneArgs a{};
    NNGP_REQUIRE(sys->d == LaneSys<SYS>::D, "system kind %d has d=%d, got d=%d", SYS, LaneSys<SYS>::D, sys->d);
    NNGP_REQUIRE(!sys->normalized || sys->norm != nullptr, "normalized system needs norm[3d]");
    a.normalized = sys->normalized;
    a.norm = sys->norm;
    for (int c = 0; c < 4; c++) a.param[c] = sys->param[c];
    a.rparam0 = 1.0 / sys->param[0];
    hipLaunchKernelGGL(rhs_lane_kernel<SYS>, dim3((n + 63) / 64), dim3(64), 0, st, a, n, u, out);
    NNGP_LAUNCH_CHECK();
    return NNGP_OK;
}

template <int SYS>
static int launch_rhs_field(const nngp_system *sys, int n, const double *u, double *out, hipStream_t st) {
    FieldArgs fa;
    int rc = field_args(sys, fa);
    if (rc) return rc;
    hipLaunchKernelGGL(rhs_field_kernel<SYS>, dim3(n), dim3(256), sizeof(double) * image_doubles<SYS>(fa), st, fa, u,
                       out);
    NNGP_LAUNCH_CHECK();
    return NNGP_OK;
}

}  // namespace NNGP_RK_VARIANT
}  // namespace nngp

#ifdef NNGP_RK_FMA
// the contracted code object's one entry (not part of include/nngp.h): same arguments as the exact
// build's dispatch below
extern "C" __attribute__((visibility("hidden"))) int nngp_rk_dispatch_contracted(
    const nngp_system *sys, int tableau, int linspace, int n_slices, const double *t0, const double *t1,
    int64_t steps, int64_t gsteps, const int64_t *j0, const double *u0, double *uF, void *stream) {
    using namespace nngp;
    hipStream_t st = (hipStream_t)stream;
    if (linspace) return dispatch_tab<true, false>(sys, tableau, n_slices, t0, t1, steps, gsteps, j0, u0, uF, st);
    return dispatch_tab<false, false>(sys, tableau, n_slices, t0, t1, steps, gsteps, j0, u0, uF, st);
}
#else
extern "C" int nngp_rk_dispatch_contracted(const nngp_system *sys, int tableau, int linspace, int n_slices,
                                           const double *t0, const double *t1, int64_t steps, int64_t gsteps,
                                           const int64_t *j0, const double *u0, double *uF, void *stream);

extern "C" int nngp_rhs_batch(const nngp_system *sys, int n, const double *u, double *out, void *stream) {
    using namespace nngp;
    NNGP_REQUIRE(sys != nullptr && n >= 0, "bad sys / n");
    if (n == 0) return NNGP_OK;
    NNGP_REQUIRE(u && out, "null array argument");
    hipStream_t st = (hipStream_t)stream;
    switch (sys->kind) {
    case NNGP_SYS_LORENZ: return launch_rhs_lane<NNGP_SYS_LORENZ>(sys, n, u, out, st);
    case NNGP_SYS_HOPF: return launch_rhs_lane<NNGP_SYS_HOPF>(sys, n, u, out, st);
    case NNGP_SYS_THOMAS_LABYRINTH: return launch_rhs_lane<NNGP_SYS_THOMAS_LABYRINTH>(sys, n, u, out, st);
    case NNGP_SYS_FHN_ODE: return launch_rhs_lane<NNGP_SYS_FHN_ODE>(sys, n, u, out, st);
    case NNGP_SYS_ROSSLER: return launch_rhs_lane<NNGP_SYS_ROSSLER>(sys, n, u, out, st);
    case NNGP_SYS_BRUSSELATOR: return launch_rhs_lane<NNGP_SYS_BRUSSELATOR>(sys, n, u, out, st);
    case NNGP_SYS_DBL_PEND: return launch_rhs_lane<NNGP_SYS_DBL_PEND>(sys, n, u, out, st);
    case NNGP_SYS_BURGERS: return launch_rhs_field<NNGP_SYS_BURGERS>(sys, n, u, out, st);
    case NNGP_SYS_FHN_PDE: return launch_rhs_field<NNGP_SYS_FHN_PDE>(sys, n, u, out, st);
    case NNGP_SYS_DIFFREACT: return launch_rhs_field<NNGP_SYS_DIFFREACT>(sys, n, u, out, st);
    // one evaluation has no step loop to keep the table in registers for: the field form at every d
    case NNGP_SYS_POLY: return launch_rhs_field<NNGP_SYS_POLY>(sys, n, u, out, st);
    case NNGP_SYS_FUNC: return launch_rhs_field<NNGP_SYS_FUNC>(sys, n, u, out, st);
    default: set_error("unknown system kind %d", sys->kind); return NNGP_E_ARG;
    }
}

extern "C" int nngp_parareal_update(int64_t n, const double *a, const double *b, const double *c,
                                    double *out, void *stream) {
    using namespace nngp;
    NNGP_REQUIRE(n >= 0, "n < 0");
    if (n == 0) return NNGP_OK;
    NNGP_REQUIRE(a && b && out, "null array argument");
    const int64_t blocks = std::min<int64_t>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(update_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, n, a, b, c, out);
    NNGP_LAUNCH_CHECK();
    return NNGP_OK;
}

extern "C" int nngp_rk_batch(const nngp_system *sys, int tableau, int step_mode, int n_slices,
                             const double *t0, const double *t1, int64_t steps, const double *u0,
                             double *uF, void *stream) {
    using namespace nngp;
    NNGP_REQUIRE(sys != nullptr, "sys is NULL");
    NNGP_REQUIRE(n_slices >= 0, "n_slices < 0");
    NNGP_REQUIRE(steps >= 1, "steps must be >= 1 (got %lld)", (long long)steps);
    if (n_slices == 0) return NNGP_OK;
    NNGP_REQUIRE(t0 && t1 && u0 && uF, "null array argument");
    hipStream_t st = (hipStream_t)stream;
    const int mode = step_mode & ~NNGP_STEP_CONTRACT;
    NNGP_REQUIRE(mode == NNGP_STEP_FIXED || mode == NNGP_STEP_LINSPACE, "unknown step_mode %d", step_mode);
    if (step_mode & NNGP_STEP_CONTRACT)
        return nngp_rk_dispatch_contracted(sys, tableau, mode == NNGP_STEP_LINSPACE, n_slices, t0, t1, steps,
                                           steps, nullptr, u0, uF, stream);
    if (mode == NNGP_STEP_FIXED)
        return dispatch_tab<false, false>(sys, tableau, n_slices, t0, t1, steps, steps, nullptr, u0, uF, st);
    return dispatch_tab<true, false>(sys, tableau, n_slices, t0, t1, steps, steps, nullptr, u0, uF, st);
}

extern "C" int nngp_rk_batch_grid(const nngp_system *sys, int tableau, int n_slices,
                                  const double *g0, const double *g1, int64_t gsteps,
                                  const int64_t *j0, int64_t steps, const double *u0, double *uF,
                                  void *stream) {
    using namespace nngp;
    NNGP_REQUIRE(sys != nullptr, "sys is NULL");
    NNGP_REQUIRE(n_slices >= 0 && steps >= 1 && gsteps >= 1, "bad n_slices / steps / gsteps");
    if (n_slices == 0) return NNGP_OK;
    NNGP_REQUIRE(g0 && g1 && j0 && u0 && uF, "null array argument");
    return dispatch_tab<true, false>(sys, tableau, n_slices, g0, g1, steps, gsteps, j0, u0, uF,
                              (hipStream_t)stream);
}
#endif  // NNGP_RK_FMA
