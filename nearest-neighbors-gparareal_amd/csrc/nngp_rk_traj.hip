// nngp_rk_traj.hip -- sampled trajectories of every slice in one launch (nngp_rk_traj,
// include/nngp.h) for gfx950 (MI355X).
//
// Replaces the reference's SolverRK.run_F_full / run_G_full (solver.py:109-113 -> RK.run,
// RK.py:91-99) as Parareal._build_cont_traj calls them slice by slice (parareal.py:500-508): the
// whole solution between the slice boundaries, here every `every`-th state of it.
//
// The kernels are the propagators of nngp_rk.hip (nngp_rk_kernels.h) instantiated with TRAJ = true:
// the same step, the same expression order, and a store of the state from inside the step loop
// whenever a per-slice countdown runs out (TrajOut, nngp_rk_dev.h).  A trajectory row is therefore
// bitwise what nngp_rk_batch returns after that many steps.  The host dispatch is the same
// template too, so every shape runs on the kernel form its end-state launch uses and the knobs
// (NNGP_RK_GROUP, NNGP_BURGERS_LDS, NNGP_RK_THREADS, NNGP_FHN_PAIR) and refusals keep their meaning.
// The instantiations live in this translation unit so that they compile beside nngp_rk.hip's.
//
// Like nngp_rk.hip this file is compiled TWICE (csrc/Makefile): exact, and with NNGP_RK_FMA and
// -ffp-contract=fast for NNGP_STEP_CONTRACT.  Only the exact build exports the C-ABI; the
// contracted one exports nngp_rk_traj_dispatch_contracted, which nngp_rk_traj calls.

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

// the TRAJ kernels take `every` in the gsteps argument and no j0 (nngp_rk_kernels.h)
static int traj_dispatch(const nngp_system *sys, int tableau, bool linspace, int n_slices, const double *t0,
                         const double *t1, int64_t steps, int64_t every, const double *u0, double *traj,
                         hipStream_t st) {
    if (linspace) return dispatch_tab<true, true>(sys, tableau, n_slices, t0, t1, steps, every, nullptr, u0, traj, st);
    return dispatch_tab<false, true>(sys, tableau, n_slices, t0, t1, steps, every, nullptr, u0, traj, st);
}

}  // namespace NNGP_RK_VARIANT
}  // namespace nngp

#ifdef NNGP_RK_FMA
// the contracted code object's one entry (not part of include/nngp.h)
extern "C" __attribute__((visibility("hidden"))) int nngp_rk_traj_dispatch_contracted(
    const nngp_system *sys, int tableau, int linspace, int n_slices, const double *t0, const double *t1,
    int64_t steps, int64_t every, const double *u0, double *traj, void *stream) {
    return nngp::traj_dispatch(sys, tableau, linspace != 0, n_slices, t0, t1, steps, every, u0, traj,
                               (hipStream_t)stream);
}
#else
extern "C" int nngp_rk_traj_dispatch_contracted(const nngp_system *sys, int tableau, int linspace, int n_slices,
                                                const double *t0, const double *t1, int64_t steps, int64_t every,
                                                const double *u0, double *traj, void *stream);

extern "C" int nngp_rk_traj(const nngp_system *sys, int tableau, int step_mode, int n_slices, const double *t0,
                            const double *t1, int64_t steps, int64_t every, const double *u0, double *traj,
                            void *stream) {
    using namespace nngp;
    NNGP_REQUIRE(sys != nullptr, "sys is NULL");
    NNGP_REQUIRE(n_slices >= 0, "n_slices < 0");
    NNGP_REQUIRE(steps >= 1 && every >= 1, "steps and every must be >= 1 (got steps=%lld, every=%lld)",
                 (long long)steps, (long long)every);
    const int mode = step_mode & ~NNGP_STEP_CONTRACT;
    NNGP_REQUIRE(mode == NNGP_STEP_FIXED || mode == NNGP_STEP_LINSPACE, "unknown step_mode %d", step_mode);
    if (n_slices == 0) return NNGP_OK;
    NNGP_REQUIRE(t0 && t1 && u0 && traj, "null array argument");
    NNGP_REQUIRE(traj != u0, "traj must not alias u0");
    every = std::min(every, steps);   // the same rows (u0 and the end), and steps + every cannot overflow
    if (step_mode & NNGP_STEP_CONTRACT)
        return nngp_rk_traj_dispatch_contracted(sys, tableau, mode == NNGP_STEP_LINSPACE, n_slices, t0, t1, steps,
                                                every, u0, traj, stream);
    return traj_dispatch(sys, tableau, mode == NNGP_STEP_LINSPACE, n_slices, t0, t1, steps, every, u0, traj,
                         (hipStream_t)stream);
}
#endif  // NNGP_RK_FMA
