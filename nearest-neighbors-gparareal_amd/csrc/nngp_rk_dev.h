// nngp_rk_dev.h -- device building blocks of the RK propagators, shared by nngp_rk_kernels.h (the
// batched F/G kernels of nngp_rk.hip and nngp_rk_traj.hip, exact and contracted builds) and nngp_gp.hip (the fused correction chain,
// whose in-kernel G step must be bitwise the G launch).  Included INSIDE
// `namespace nngp { inline namespace <variant> {`; needs common.h, nngp_math.h and tableau.h.
#pragma once

// ---------------------------------------------------------------------------------------------
// ODE right-hand sides (systems.py), one lane = one state
// ---------------------------------------------------------------------------------------------
struct LaneArgs {
    double mn[4], hw[4], sc[4];  // '-11' wrapper: mn, (mx-mn)/2, 2/(mx-mn)   (utils.py:14-33)
    double param[4];
    double rparam0;              // RN(1/param[0]) for the Markstein division below
    int normalized;
    const double *norm;          // device [3D], loaded into the fields above by each lane
};

// x / b for a constant divisor b with r = RN(1/b) precomputed: q = x*r corrected by one fma
// (Markstein's theorem: r within 1/2 ulp of 1/b => RN(q + r*(x - q*b)) == RN(x/b)); bitwise the
// IEEE quotient (checked on 2e8 random operands), 3 dependent ops instead of the ~10-op
// v_div_scale/v_rcp/v_div_fmas/v_div_fixup sequence on the RK critical path.
__device__ __forceinline__ double div_const(double x, double b, double r) {
    const double q = x * r;
    return fma(fma(-q, b, x), r, q);
}

template <int SYS> struct LaneSys;

template <> struct LaneSys<NNGP_SYS_LORENZ> {   // systems.py:232-238
    static constexpr int D = 3;
    __device__ static void f(const double *u, double *o, const LaneArgs &) {
        o[0] = 10 * (u[1] - u[0]);
        o[1] = (28 * u[0] - u[1]) - u[0] * u[2];
        o[2] = u[0] * u[1] - (8.0 / 3) * u[2];
    }
};
template <> struct LaneSys<NNGP_SYS_HOPF> {     // systems.py:148-154
    static constexpr int D = 3;
    __device__ static void f(const double *u, double *o, const LaneArgs &a) {
        const double g = (div_const(u[2], a.param[0], a.rparam0) - u[0] * u[0]) - u[1] * u[1];
        o[0] = -u[1] + u[0] * g;
        o[1] = u[0] + u[1] * g;
        o[2] = 1.0;
    }
};
template <> struct LaneSys<NNGP_SYS_THOMAS_LABYRINTH> {   // systems.py:257-271
    static constexpr int D = 3;
    __device__ static void f(const double *u, double *o, const LaneArgs &) {
        o[0] = -0.5 * u[0] + 10.0 * nn_sin_pi(u[1]);
        o[1] = -0.5 * u[1] + 10.0 * nn_sin_pi(u[2]);
        o[2] = -0.5 * u[2] + 10.0 * nn_sin_pi(u[0]);
    }
};
template <> struct LaneSys<NNGP_SYS_FHN_ODE> {  // systems.py:87-95 (u**3 = u*(u*u), jax)
    static constexpr int D = 2;
    __device__ static void f(const double *u, double *o, const LaneArgs &) {
        const double c = 3;
        o[0] = c * ((u[0] - div_const(u[0] * (u[0] * u[0]), 3.0, 1.0 / 3)) + u[1]);
        o[1] = -(1 / c) * ((u[0] - 0.2) + 0.2 * u[1]);
    }
};
template <> struct LaneSys<NNGP_SYS_ROSSLER> {  // systems.py:116-125
    static constexpr int D = 3;
    __device__ static void f(const double *u, double *o, const LaneArgs &) {
        o[0] = -u[1] - u[2];
        o[1] = u[0] + (0.2 * u[1]);
        o[2] = 0.2 + u[2] * (u[0] - 5.7);
    }
};
template <> struct LaneSys<NNGP_SYS_BRUSSELATOR> {  // systems.py:209-214
    static constexpr int D = 2;
    __device__ static void f(const double *u, double *o, const LaneArgs &) {
        o[0] = (1 + (u[0] * u[0]) * u[1]) - (3 + 1) * u[0];
        o[1] = 3 * u[0] - (u[0] * u[0]) * u[1];
    }
};
template <> struct LaneSys<NNGP_SYS_DBL_PEND> {  // systems.py:182-189
    static constexpr int D = 4;
    __device__ static void f(const double *u, double *o, const LaneArgs &) {
        double s, c;
        nn_sincos(u[0] - u[2], s, c);
        const double s0 = nn_sin(u[0]), s2 = nn_sin(u[2]);
        const double pre = -1 / (2 - c * c);
        o[0] = u[1];
        o[1] = pre * ((((u[1] * u[1]) * c) * s + (u[3] * u[3]) * s) + 2 * s0 - c * s2);
        o[2] = u[3];
        o[3] = pre * ((((-2 * (u[1] * u[1])) * s - ((u[3] * u[3]) * s) * c) - (2 * c) * s0) + 2 * s2);
    }
};

// ---------------------------------------------------------------------------------------------
// Polynomial field, lane form (NNGP_SYS_POLY with d <= 4 and at most 16 terms).
// Every lane evaluates the same table, so the table is wave-uniform: it travels by value in the
// kernel arguments -- in its own argument type, LaneArgs is what it was -- and lives in scalar
// registers; the step loop reads no memory.  The 16 terms are unrolled, a term past the table's
// count leaves the body by one uniform branch, and the factors are picked from the state by a
// uniform index.  The arithmetic is the contract's: coef times the factors left to right, the
// row's first term, then acc + term in list order; a row without terms is +0.0.
// LaneSys<NNGP_SYS_POLY_LANE + D> is the D-component form (D is a compile-time constant so that
// the state stays in registers and the slice's row stride is the system's d).
// ---------------------------------------------------------------------------------------------
struct PolyLaneTab {
    double coef[POLY_LANE_TERMS];
    // per term: bits 0-1 the number of factors, 2-3 / 5-6 / 8-9 their indices, 11-12 the row,
    // 13 first term of its row, 14 last term of its row
    uint16_t desc[POLY_LANE_TERMS];
    int n;
};
struct PolyLaneArgs : LaneArgs {
    PolyLaneTab tab;
};
constexpr int NNGP_SYS_POLY_LANE = 64;   // + D: not a value of enum nngp_system_kind

// keeps a uniform `if` a scalar branch: without it the compiler turns the skipped work into
// per-lane selects (two v_cndmask per fp64 value), which cost more than the work they skip
#define NNGP_POLY_KEEP_BRANCH() asm volatile("")

// eight slots so that x[uniform index] is one indexed register move per half (s_set_gpr_idx) and
// not a chain of selects over the components (which LLVM makes of up to five fp64 slots); the
// slots past D are never selected by a table's indices (< D)
constexpr int POLY_LANE_SLOTS = 8;

// terms T.. of the table, nested: term T + 1 lies inside term T's `if`, so the first term past the
// table's count leaves all the remaining bodies by ONE taken branch (16 separate `if`s cost a taken
// branch per missing term; a loop with an early exit is re-rolled by the compiler and then reads
// the table from the argument segment, memory, inside the step)
template <int D, int T>
__device__ __forceinline__ void poly_lane_terms(const PolyLaneTab &tab, int n, const double (&x)[POLY_LANE_SLOTS],
                                                double (&r)[POLY_LANE_D], double acc) {
    if constexpr (T < POLY_LANE_TERMS) {
        if (T < n) {
            // the descriptor is re-read as a value the compiler cannot trace (also keeps this `if` a
            // branch): else every field and comparison of all 16 terms is hoisted out of the step
            // loop into a scalar-register pair each, far more than there are, and comes back into
            // the loop as v_readlane from spill registers
            unsigned ds = tab.desc[T];
            asm volatile("" : "+s"(ds));
            const unsigned p = ds & 3u;
            double v = tab.coef[T];
            if (p >= 1) {
                NNGP_POLY_KEEP_BRANCH();
                v = v * x[(ds >> 2) & 3u];
                if (p >= 2) {
                    NNGP_POLY_KEEP_BRANCH();
                    v = v * x[(ds >> 5) & 3u];
                    if (p >= 3) {
                        NNGP_POLY_KEEP_BRANCH();
                        v = v * x[(ds >> 8) & 3u];
                    }
                }
            }
            // the row's first term: -0.0 + v is v bit for bit (zeros of either sign and NaN included),
            // so the sum still does not start from 0.0; a select instead of a taken branch
            const double before = (ds & (1u << 13)) ? -0.0 : acc;
            acc = before + v;
            if (__builtin_expect((ds & (1u << 14)) != 0, 0)) {   // the row's last term, out of line
                NNGP_POLY_KEEP_BRANCH();
                const unsigned row = (ds >> 11) & 3u;
#pragma unroll
                for (int c = 0; c < D; c++)
                    if (row == (unsigned)c) r[c] = acc;
            }
            poly_lane_terms<D, T + 1>(tab, n, x, r, acc);
        }
    }
}

template <int D_> struct PolyLane {
    static constexpr int D = D_;
    __device__ __forceinline__ static void f(const double *u, double *o, const PolyLaneArgs &a) {
        double x[POLY_LANE_SLOTS], r[POLY_LANE_D];
#pragma unroll
        for (int c = 0; c < POLY_LANE_SLOTS; c++) x[c] = c < D ? u[c] : 1.0;
#pragma unroll
        for (int c = 0; c < POLY_LANE_D; c++) r[c] = 0.0;   // a row without terms: +0.0
        int n = a.tab.n;
        asm volatile("" : "+s"(n));   // as the descriptors: compared inside the step, not hoisted
        poly_lane_terms<D, 0>(a.tab, n, x, r, 0.0);
#pragma unroll
        for (int c = 0; c < D; c++) o[c] = r[c];
    }
};
#undef NNGP_POLY_KEEP_BRANCH
template <> struct LaneSys<NNGP_SYS_POLY_LANE + 1> : PolyLane<1> {};
template <> struct LaneSys<NNGP_SYS_POLY_LANE + 2> : PolyLane<2> {};
template <> struct LaneSys<NNGP_SYS_POLY_LANE + 3> : PolyLane<3> {};
template <> struct LaneSys<NNGP_SYS_POLY_LANE + 4> : PolyLane<4> {};

// ---------------------------------------------------------------------------------------------
// Fields with elementary-function atoms (NNGP_SYS_FUNC): monomials over the
// extended vector [u_0 .. u_{d-1}, atom_0 .. atom_{n_atoms-1}], atom q = fn(a u[i] (+ c u[j]) (+ b)).
// The six functions are the project's own routines (nngp_math.h, pinned to the oracle bit for bit)
// and the IEEE 1.0/x and sqrt.
// ---------------------------------------------------------------------------------------------
// keeps a uniform `if` a scalar branch (see NNGP_POLY_KEEP_BRANCH above)
#define NNGP_FUNC_KEEP_BRANCH() asm volatile("")

// fn(x), fn in 1..6 (checked when the table was registered).  UNIFORM: fn is the same in every lane
// (the lane form, the table in the kernel arguments), and each function stands behind a scalar
// branch of its own, so a step pays for the functions its table names and for no other; a per-lane
// select over six results would run all six.  The field form's threads hold different atoms and
// diverge here by exec mask.
template <bool UNIFORM>
__device__ __forceinline__ double func_apply(unsigned fn, double x) {
    double r;
    if (fn == NNGP_FN_SIN) {
        if constexpr (UNIFORM) NNGP_FUNC_KEEP_BRANCH();
        r = nn_sin_pi(x);
    } else if (fn == NNGP_FN_COS) {
        if constexpr (UNIFORM) NNGP_FUNC_KEEP_BRANCH();
        r = nn_cos(x);
    } else if (fn == NNGP_FN_EXP) {
        if constexpr (UNIFORM) NNGP_FUNC_KEEP_BRANCH();
        r = nn_exp(x);
    } else if (fn == NNGP_FN_LOG) {
        if constexpr (UNIFORM) NNGP_FUNC_KEEP_BRANCH();
        r = nn_log(x);
    } else if (fn == NNGP_FN_RECIP) {
        if constexpr (UNIFORM) NNGP_FUNC_KEEP_BRANCH();
        r = 1.0 / x;
    } else {
        if constexpr (UNIFORM) NNGP_FUNC_KEEP_BRANCH();
        r = sqrt(x);
    }
    return r;
}

// field form: atom A from the state part of the stage image V (the de-normalised state); the
// argument in the contract's order, an absent part not replaced by + 0.0
__device__ __forceinline__ double func_atom_value(const nngp_func_atom &A, const double *__restrict__ V) {
    double x = A.a * V[A.i];
    if (A.j >= 0) x = x + A.c * V[A.j];
    if (A.has_b) x = x + A.b;
    return func_apply<false>((unsigned)A.fn, x);
}

// Lane form (d <= 4, at most 4 atoms and 16 terms): the polynomial lane form's scheme -- the table
// wave-uniform, by value in the kernel arguments, the 16 terms and the 4 atoms unrolled and nested so
// that the first one past the table's count leaves by one taken branch -- with the atoms in slots
// D .. D + n_atoms - 1 of the same 8-slot register array, hence 3-bit indices in the term
// descriptors and a table type of its own (PolyLaneTab is what it was).
struct FuncLaneTab {
    double coef[POLY_LANE_TERMS];
    // per term: bits 0-1 the number of factors, 2-4 / 5-7 / 8-10 their indices, 11-12 the row,
    // 13 first term of its row, 14 last term of its row
    uint16_t desc[POLY_LANE_TERMS];
    int n;
    double a[FUNC_LANE_ATOMS], c[FUNC_LANE_ATOMS], b[FUNC_LANE_ATOMS];
    // per atom: bits 0-2 the function, 3-4 i, 5-6 j, 7 a second component is present, 8 b is present
    uint16_t adesc[FUNC_LANE_ATOMS];
    int n_atoms;
};
struct FuncLaneArgs : LaneArgs {
    FuncLaneTab tab;
};
constexpr int NNGP_SYS_FUNC_LANE = 80;   // + D: not a value of enum nngp_system_kind

// the atoms, into slots D .. D + n_atoms - 1: unrolled and nested like the terms, so the table stays
// in scalar registers and an atom past the table's count leaves by one taken branch.  (A rolled loop
// over the atoms was tried for its smaller code: a uniform index into the table moves the whole
// argument struct to private memory, and with scalar selects instead the loop inside the stage loop
// keeps the compiler from unrolling the stages at all from D = 2 on -- DESIGN.md 3.2e.)
template <int D, int Q>
__device__ __forceinline__ void func_lane_atoms(const FuncLaneTab &tab, int na, double (&x)[POLY_LANE_SLOTS]) {
    if constexpr (Q < FUNC_LANE_ATOMS) {
        if (Q < na) {
            unsigned ds = tab.adesc[Q];
            asm volatile("" : "+s"(ds));   // as the term descriptors: decoded inside the step
            double v = tab.a[Q] * x[(ds >> 3) & 3u];
            if (ds & (1u << 7)) {
                NNGP_FUNC_KEEP_BRANCH();
                v = v + tab.c[Q] * x[(ds >> 5) & 3u];
            }
            if (ds & (1u << 8)) {
                NNGP_FUNC_KEEP_BRANCH();
                v = v + tab.b[Q];
            }
            x[D + Q] = func_apply<true>(ds & 7u, v);
            func_lane_atoms<D, Q + 1>(tab, na, x);
        }
    }
}

// poly_lane_terms with 3-bit factor indices
template <int D, int T>
__device__ __forceinline__ void func_lane_terms(const FuncLaneTab &tab, int n, const double (&x)[POLY_LANE_SLOTS],
                                                double (&r)[POLY_LANE_D], double acc) {
    if constexpr (T < POLY_LANE_TERMS) {
        if (T < n) {
            unsigned ds = tab.desc[T];
            asm volatile("" : "+s"(ds));
            const unsigned p = ds & 3u;
            double v = tab.coef[T];
            if (p >= 1) {
                NNGP_FUNC_KEEP_BRANCH();
                v = v * x[(ds >> 2) & 7u];
                if (p >= 2) {
                    NNGP_FUNC_KEEP_BRANCH();
                    v = v * x[(ds >> 5) & 7u];
                    if (p >= 3) {
                        NNGP_FUNC_KEEP_BRANCH();
                        v = v * x[(ds >> 8) & 7u];
                    }
                }
            }
            const double before = (ds & (1u << 13)) ? -0.0 : acc;   // -0.0 + v is v bit for bit
            acc = before + v;
            if (__builtin_expect((ds & (1u << 14)) != 0, 0)) {
                NNGP_FUNC_KEEP_BRANCH();
                const unsigned row = (ds >> 11) & 3u;
#pragma unroll
                for (int c = 0; c < D; c++)
                    if (row == (unsigned)c) r[c] = acc;
            }
            func_lane_terms<D, T + 1>(tab, n, x, r, acc);
        }
    }
}

template <int D_> struct FuncLane {
    static constexpr int D = D_;
    __device__ __forceinline__ static void f(const double *u, double *o, const FuncLaneArgs &a) {
        double x[POLY_LANE_SLOTS], r[POLY_LANE_D];
#pragma unroll
        for (int c = 0; c < POLY_LANE_SLOTS; c++) x[c] = c < D ? u[c] : 1.0;
#pragma unroll
        for (int c = 0; c < POLY_LANE_D; c++) r[c] = 0.0;   // a row without terms: +0.0
        int na = a.tab.n_atoms, n = a.tab.n;
        asm volatile("" : "+s"(na), "+s"(n));
        func_lane_atoms<D, 0>(a.tab, na, x);
        func_lane_terms<D, 0>(a.tab, n, x, r, 0.0);
#pragma unroll
        for (int c = 0; c < D; c++) o[c] = r[c];
    }
};
#undef NNGP_FUNC_KEEP_BRANCH
template <> struct LaneSys<NNGP_SYS_FUNC_LANE + 1> : FuncLane<1> {};
template <> struct LaneSys<NNGP_SYS_FUNC_LANE + 2> : FuncLane<2> {};
template <> struct LaneSys<NNGP_SYS_FUNC_LANE + 3> : FuncLane<3> {};
template <> struct LaneSys<NNGP_SYS_FUNC_LANE + 4> : FuncLane<4> {};

// f_n(u) = f(inverse(u)) * scale   (systems.py:36-40), inverse(u) = ((u+1)/2)*(mx-mn) + mn
// (utils.py:24) evaluated as (u+1)*((mx-mn)/2) + mn: halving is exact for normal numbers, so
// RN(RN(u+1)/2 * w) == RN(RN(u+1) * (w/2)) bit for bit, one multiply fewer per component.  NORM is a template parameter so the RK
// step loop carries no branches: the lane kernel is VALU-issue-bound (one wave per SIMD, ~4.5
// cycles per fp64 instruction, dependent or not -- tools/ubench_fp64.hip), so every instruction
// and every taken scalar branch inside the step is paid in full on the critical path.
// (A: LaneArgs, or the polynomial field's PolyLaneArgs)
template <int SYS, bool NORM, class A>
__device__ __forceinline__ void lane_rhs(const double *u, double *o, const A &a) {
    constexpr int D = LaneSys<SYS>::D;
    if constexpr (NORM) {
        double v[D];
#pragma unroll
        for (int c = 0; c < D; c++) v[c] = (u[c] + 1) * a.hw[c] + a.mn[c];
        LaneSys<SYS>::f(v, o, a);
#pragma unroll
        for (int c = 0; c < D; c++) o[c] = o[c] * a.sc[c];
    } else {
        LaneSys<SYS>::f(u, o, a);
    }
}

// stage input  u + sum_{j<s} a_sj k_j  over the non-zero a_sj in ascending j (RK.py:153-166).
// The reference starts the sum from 0.0 (`temp = jnp.zeros(dim)`); starting from the first term
// instead is identical up to the sign of an exact zero and saves one dependent add per stage.
// k is indexed k[j*KS + c]; s is a compile-time constant after unrolling.
template <typename T, int KS>
__device__ __forceinline__ double stage_input(int s, double u, const double *k, int c) {
    double t = 0.0;
    bool first = true;
#pragma unroll
    for (int j = 0; j < T::S; j++) {
        if (j >= s || T::A[s][j] == 0.0) continue;
        const double v = T::A[s][j] * k[j * KS + c];
        t = first ? v : t + v;
        first = false;
    }
    return first ? u : u + t;
}

// stage_input split at j = s - 1, for kernels that form the terms not involving k_{s-1} early:
// stage_partial = the sum over the non-zero a_sj with j < s - 1 (0.0 if none), stage_finish adds
// a_{s,s-1} k_{s-1} and u -- the same additions in the same order as stage_input.
template <typename T>
__host__ __device__ constexpr bool stage_has_partial(int s) {
    for (int j = 0; j + 1 < s; j++)
        if (T::A[s][j] != 0.0) return true;
    return false;
}
template <typename T, int KS>
__device__ __forceinline__ double stage_partial(int s, const double *k, int c) {
    double t = 0.0;
    bool first = true;
#pragma unroll
    for (int j = 0; j < T::S; j++) {
        if (j + 1 >= s || T::A[s][j] == 0.0) continue;
        const double v = T::A[s][j] * k[j * KS + c];
        t = first ? v : t + v;
        first = false;
    }
    return t;
}
template <typename T, int KS>
__device__ __forceinline__ double stage_finish(int s, double u, double partial, const double *k, int c) {
    const bool hp = stage_has_partial<T>(s), hl = s >= 1 && T::A[s][s - 1] != 0.0;
    if (!hp && !hl) return u;
    double t = partial;
    if (hl) {
        const double v = T::A[s][s - 1] * k[(s - 1) * KS + c];
        t = hp ? t + v : v;
    }
    return u + t;
}
// step_update accumulated stage by stage: acc after stage s (the same order, non-zero b_s only;
// acc is unset until the first non-zero b_s, which every tableau has at s = 0 or 1)
template <typename T>
__device__ __forceinline__ void step_accumulate(int s, double &acc, double ks) {
    if (T::B[s] == 0.0) return;
    bool first = true;
#pragma unroll
    for (int j = 0; j < T::S; j++)
        if (j < s && T::B[j] != 0.0) first = false;
    const double v = T::B[s] * ks;
    acc = first ? v : acc + v;
}

// u + sum_s b_s k_s over the non-zero b_s in ascending s (jnp.sum(b*k, 1), RK.py:170)
template <typename T, int KS>
__device__ __forceinline__ double step_update(double u, const double *k, int c) {
    double acc = 0.0;
    bool first = true;
#pragma unroll
    for (int s = 0; s < T::S; s++) {
        if (T::B[s] == 0.0) continue;
        const double v = T::B[s] * k[s * KS + c];
        acc = first ? v : acc + v;
        first = false;
    }
    return u + acc;
}

// The lane-group kernel's folded tableau (rk_group_kernel only; the lane, field and pair kernels
// keep stage_input and step_update above).  Where some row's single non-zero entry is a power of
// two a = A[s][j] != 1 (RK4: u + 0.5 k0, u + 0.5 k1), column j's k is stored pre-scaled,
// k'_j = (a h) o_j -- the one multiply h o_j costs -- and that stage's input is u + k'_j, an add
// instead of a multiply and an add.  Scaling by a power of two commutes with rounding,
// RN(a RN(h o)) = RN((a h) o), whenever the products are normal or exact zeros (signs included),
// so k'_j is bitwise a k_j; every other coefficient on column j, B[j] included, is divided by a
// at compile time (an exact rescaling), so each term c k_j = (c/a) k'_j has the same real product
// and the same rounding, and the sums keep stage_input's and step_update's order.  Where h o is
// subnormal (|k| < 2^-1022) the two forms can differ in the last denormal bit.
// The contracted build keeps the unfolded tableau: there u + k' with k' = (a h) o would contract to
// fma(a h, o, u) and skip k's rounding, where u + a k contracts to fma(a, k, u) and keeps it --
// another result (TomLab N = 256 converges in another K, tests/test_gpu_contract.py).
#ifdef NNGP_RK_FMA
constexpr bool FOLD_TABLEAU = false;
#else
constexpr bool FOLD_TABLEAU = true;
#endif
__host__ __device__ constexpr bool fold_pow2(double a) {
    if (!(a > 0.0)) return false;
    while (a < 1.0) a *= 2.0;
    while (a >= 2.0) a *= 0.5;
    return a == 1.0;
}
template <typename T>
__host__ __device__ constexpr double fold_col_scale(int j) {
    for (int s = j + 1; s < T::S; s++) {
        int nz = 0;
        for (int q = 0; q < s; q++) nz += T::A[s][q] != 0.0;
        const double a = T::A[s][j];
        if (nz == 1 && a != 0.0 && a != 1.0 && fold_pow2(a)) return a;
    }
    return 1.0;
}
template <typename T>
__host__ __device__ constexpr double fold_a(int s, int j) { return T::A[s][j] / fold_col_scale<T>(j); }
template <typename T>
__host__ __device__ constexpr double fold_b(int j) { return T::B[j] / fold_col_scale<T>(j); }
static_assert(fold_col_scale<Tableau<1>>(0) == 1.0, "RK1: nothing to fold");
static_assert(fold_col_scale<Tableau<2>>(0) == 0.5 && fold_col_scale<Tableau<2>>(1) == 1.0 &&
              fold_a<Tableau<2>>(1, 0) == 1.0 && fold_b<Tableau<2>>(0) == 0.0, "RK2: k0 halved");
static_assert(fold_col_scale<Tableau<4>>(0) == 0.5 && fold_col_scale<Tableau<4>>(1) == 0.5 &&
              fold_col_scale<Tableau<4>>(2) == 1.0 && fold_col_scale<Tableau<4>>(3) == 1.0 &&
              fold_a<Tableau<4>>(1, 0) == 1.0 && fold_a<Tableau<4>>(2, 1) == 1.0 &&
              fold_a<Tableau<4>>(3, 2) == 1.0 && fold_b<Tableau<4>>(0) == 2 * Tableau<4>::B[0] &&
              fold_b<Tableau<4>>(1) == 2 * Tableau<4>::B[1] && fold_b<Tableau<4>>(2) == Tableau<4>::B[2],
              "RK4: k0 and k1 halved, their update weights doubled");
static_assert(fold_col_scale<Tableau<8>>(0) == 0.5 && fold_col_scale<Tableau<8>>(1) == 1.0 &&
              fold_a<Tableau<8>>(1, 0) == 1.0 && fold_a<Tableau<8>>(2, 0) == 0.5 &&
              fold_a<Tableau<8>>(3, 0) == 2 * Tableau<8>::A[3][0] && fold_b<Tableau<8>>(0) == 2 * Tableau<8>::B[0],
              "RK8: k0 halved (row 1), column 0's other entries and B[0] doubled");

// stage s's step size: (a h) for a pre-scaled column (loop-invariant in fixed-step mode), else h
template <typename T>
__device__ __forceinline__ double fold_h(int s, double h) {
    return fold_col_scale<T>(s) == 1.0 ? h : fold_col_scale<T>(s) * h;
}
// one term c k' of a folded sum: no multiply where the rescaled coefficient is 1
__device__ __forceinline__ double fold_term(double c, double kp) { return c == 1.0 ? kp : c * kp; }
// stage_input and step_update on the pre-scaled k' (one component per lane: k[j])
template <typename T>
__device__ __forceinline__ double fold_stage_input(int s, double u, const double *k) {
    double t = 0.0;
    bool first = true;
#pragma unroll
    for (int j = 0; j < T::S; j++) {
        if (j >= s || T::A[s][j] == 0.0) continue;
        const double v = fold_term(fold_a<T>(s, j), k[j]);
        t = first ? v : t + v;
        first = false;
    }
    return first ? u : u + t;
}
// (fold_step_sum: the step's increment alone, for a component whose k are known beforehand)
template <typename T>
__device__ __forceinline__ double fold_step_sum(const double *k) {
    double acc = 0.0;
    bool first = true;
#pragma unroll
    for (int s = 0; s < T::S; s++) {
        if (T::B[s] == 0.0) continue;
        const double v = fold_term(fold_b<T>(s), k[s]);
        acc = first ? v : acc + v;
        first = false;
    }
    return acc;
}
template <typename T>
__device__ __forceinline__ double fold_step_update(double u, const double *k) {
    return u + fold_step_sum<T>(k);
}

// FIXED:   h = dt = (t1-t0)/steps (RK.py:103).
// LINSPACE: step n of slice i is step j = j0 + n of the grid np.linspace(t0, t1, gsteps+1):
//           t[j] = j*gstep + t0 (gstep = (t1-t0)/gsteps), t[gsteps] = t1, h = t[j+1]-t[j]
//           (RK.py:91-99, 121; new_lib.py:87-137).  j0 = 0, gsteps = steps is the per-slice grid;
//           j0 > 0 walks one global grid (the legacy initial coarse sweep, new_lib.py:902-906).
// The grid is walked with loop-carried state: jd = (double)j is bumped by an exact +1.0 (j < 2^53)
// and t[j+1] of one step is t[j] of the next, so a step costs one grid point (add, mul, add, the
// last-point select, sub) instead of two int64 -> double conversions and two grid points -- the
// same values bit for bit, off the lane/group kernels' issue-bound step (TomLab RK4 267 -> 256
// VALU per step).
struct LinGrid {
    double jd, tn;     // (double)j, t[j]
    int64_t nlast;     // the step n with j + 1 == gsteps (its right end is t1 itself)
    __device__ __forceinline__ void init(int64_t j0, int64_t gsteps, double t0, double dt) {
        jd = (double)j0;
        tn = jd * dt + t0;
        nlast = gsteps - 1 - j0;
    }
    __device__ __forceinline__ double next(int64_t n, double t0, double t1, double dt) {
        jd = jd + 1.0;
        const double tn1 = (n == nlast) ? t1 : jd * dt + t0;
        const double h = tn1 - tn;
        tn = tn1;
        return h;
    }
};

// ---------------------------------------------------------------------------------------------
// PDE fields
// ---------------------------------------------------------------------------------------------
struct FieldArgs {
    int d, nx, normalized;
    const double *norm;   // device [3d] = mn | w | sc, or nullptr
    double c_off, c_diag, c_grad;   // Burgers: nu/dx^2, -2 nu/dx^2, 1/(2dx)
    // FHN-PDE: a*L and b*L entries.  The polynomial field (NNGP_SYS_POLY) keeps the device copy of
    // its table in the first two's bytes -- no kind uses both -- so the argument block, and with it
    // every other kernel's code, is what it was.
    union {
        struct {
            double a_off, a_diag;
        };
        struct {
            const int32_t *p_row;     // DEVICE [d+1]
            const PolyTerm *p_terms;  // DEVICE [n_terms]
        };
    };
    // (NNGP_SYS_FUNC is a polynomial table too; its atom records lie between the terms and the row
    // pointers of the same device block -- func_atoms_of -- and `nx` holds their count)
    double b_off, b_diag;
    // DiffReact: 1/dx^2, 1/dy^2, the main diagonal -(a)/dx^2 - (b)/dy^2 with a (b) = 2 inside a
    // row (column) and 1 at its two ends (m_ab), and Du, Dv, k
    double r_cx, r_cy, r_m22, r_m12, r_m21, r_m11, r_du, r_dv, r_k;
};

// NNGP_SYS_FUNC: the device block is terms [n_terms] | atoms [nx] | row_ptr [d+1] (nngp_table.hip),
// and row_ptr[d] = n_terms
__device__ __forceinline__ const nngp_func_atom *func_atoms_of(const FieldArgs &fa) {
    return (const nngp_func_atom *)(fa.p_terms + fa.p_row[fa.d]);
}

__device__ __forceinline__ double wave_prev(double v) {   // lane i <- lane i-1 (lane 0 <- 63)
    return __builtin_amdgcn_mov_dpp(v, 0x13C, 0xF, 0xF, false);
}
__device__ __forceinline__ double wave_next(double v) {   // lane i <- lane i+1 (lane 63 <- 0)
    return __builtin_amdgcn_mov_dpp(v, 0x134, 0xF, 0xF, false);
}

// ---------------------------------------------------------------------------------------------
// Sampled trajectories (nngp_rk_traj, include/nngp.h): the TRAJ instantiation of a propagator
// writes its slice's rows
//     out[0] = u0,  out[p] = state after min(p*every, steps) steps,  p = 1 .. n_out-1,
//     n_out = 1 + ceil(steps / every)
// instead of the end state alone.  The step loop keeps a countdown (a scalar decrement and branch
// per step, no modulo), the threads that hold the state in registers store it when the countdown
// runs out, and the state after the last step goes to row n_out-1 unconditionally after the loop
// (again, bitwise the same, when every divides steps).  TRAJ is a compile-time parameter: the
// end-state instantiations contain none of this.
// ---------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ int64_t traj_rows(int64_t steps, int64_t every) {
    return 1 + (steps + every - 1) / every;
}

struct TrajOut {
    double *next, *last;   // the row of the next sample, row n_out-1
    size_t stride;         // doubles per row (the system's d)
    int64_t every, left;
    // base: the slice's [n_out][d] block, whose row 0 the caller writes from the loaded u0
    __device__ __forceinline__ void init(double *base, int64_t steps, int64_t every_, int d) {
        stride = (size_t)d;
        every = left = every_;
        next = base + stride;
        last = base + (size_t)(traj_rows(steps, every_) - 1) * stride;
    }
    // once after every step: whether that step's state is a sample (wave-uniform: a scalar
    // countdown and branch); if so, take() is the row to store it to
    // Marked unlikely so that the store lies out of line and the usual step falls through: with
    // one wave per SIMD a taken branch is paid in full.
    __device__ __forceinline__ bool due() {
        if (__builtin_expect(--left != 0, 1)) return false;
        left = every;
        return true;
    }
    __device__ __forceinline__ double *take() {
        double *row = next;
        next += stride;
        return row;
    }
};

// ---------------------------------------------------------------------------------------------
// Per-slice bodies.  The batched kernels (nngp_rk.hip) call them with their slice's row; the
// correction chain (nngp_gp.hip) calls them for its in-kernel G step, so both are the same code.
// ---------------------------------------------------------------------------------------------

// one lane integrates one ODE slice (rk_lane_kernel): u0/uF are the slice's [D] rows; TRAJ: uF is
// the slice's [n_out][D] block, sampled every `every` steps (TrajOut)
template <int SYS, int ORDER, bool LINSPACE, bool NORM, bool TRAJ = false, class A = LaneArgs>
__device__ __forceinline__ void lane_slice(A args, double T0, double T1, int64_t steps, int64_t gsteps,
                                           int64_t j0, const double *__restrict__ u0, double *__restrict__ uF,
                                           int64_t every = 0) {
    using T = Tableau<ORDER>;
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
    double u[D], k[S * D], tmp[D];
#pragma unroll
    for (int c = 0; c < D; c++) u[c] = u0[c];
    TrajOut tr;
    if constexpr (TRAJ) {
        tr.init(uF, steps, every, D);
#pragma unroll
        for (int c = 0; c < D; c++) uF[c] = u[c];
        uF = tr.last;
    }
    const double dt = (T1 - T0) / (double)(LINSPACE ? gsteps : steps);
    LinGrid grid;
    if constexpr (LINSPACE) grid.init(j0, gsteps, T0, dt);
    for (int64_t n = 0; n < steps; n++) {
        const double h = LINSPACE ? grid.next(n, T0, T1, dt) : dt;
        // k_0 = h f(u); k_s = h f(u + sum_{j<s} a_sj k_j)     (RK.py:153-170)
#pragma unroll
        for (int s = 0; s < S; s++) {
#pragma unroll
            for (int c = 0; c < D; c++) tmp[c] = stage_input<T, D>(s, u[c], k, c);
            lane_rhs<SYS, NORM>(tmp, k + s * D, args);
#pragma unroll
            for (int c = 0; c < D; c++) k[s * D + c] = h * k[s * D + c];
        }
#pragma unroll
        for (int c = 0; c < D; c++) u[c] = step_update<T, D>(u[c], k, c);   // RK.py:170
        if constexpr (TRAJ) {
            if (tr.due()) {
                double *row = tr.take();
#pragma unroll
                for (int c = 0; c < D; c++) row[c] = u[c];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < D; c++) uF[c] = u[c];
}

// one wave integrates one Burgers slice, d = 64*EPT (rk_burgers_wave_kernel): lane l owns the
// contiguous elements l*EPT .. l*EPT+EPT-1; u0/uF are the slice's [d] rows.  Every lane of the
// wave must be active (the stencil's outer neighbours are wave_ror/wave_rol DPP moves).
// TRAJ: uF is the slice's [n_out][d] block, sampled every `every` steps (TrajOut).
template <int ORDER, bool LINSPACE, int EPT, bool NORM, bool TRAJ = false>
__device__ __forceinline__ void burgers_wave_slice(const FieldArgs &fa, int l, double T0, double T1, int64_t steps,
                                                   int64_t gsteps, int64_t j0, const double *__restrict__ u0,
                                                   double *__restrict__ uF, int64_t every = 0) {
    using T = Tableau<ORDER>;
    constexpr int S = T::S;
    constexpr int d = 64 * EPT;
    double u[EPT], k[S * EPT], mn[EPT], w[EPT], sc[EPT];
#pragma unroll
    for (int r = 0; r < EPT; r++) {
        const int e = l * EPT + r;
        u[r] = u0[e];
        mn[r] = NORM ? fa.norm[e] : 0.0;
        w[r] = NORM ? 0.5 * fa.norm[d + e] : 1.0;   // (mx-mn)/2, see lane_rhs
        sc[r] = NORM ? fa.norm[2 * d + e] : 1.0;
    }
    TrajOut tr;
    if constexpr (TRAJ) {
        tr.init(uF, steps, every, d);
#pragma unroll
        for (int r = 0; r < EPT; r++) uF[l * EPT + r] = u[r];
        uF = tr.last;
    }
    const bool first = l == 0, last = l == 63;     // rows 0 and d-1 live in lanes 0 and 63
    const double cxx = fa.c_off, cdg = fa.c_diag, q = fa.c_grad;
    const double dt = (T1 - T0) / (double)(LINSPACE ? gsteps : steps);
    LinGrid grid;
    if constexpr (LINSPACE) grid.init(j0, gsteps, T0, dt);
    for (int64_t n = 0; n < steps; n++) {
        const double h = LINSPACE ? grid.next(n, T0, T1, dt) : dt;
#pragma unroll
        for (int s = 0; s < S; s++) {
            double V[EPT];
#pragma unroll
            for (int r = 0; r < EPT; r++) {
                const double x = stage_input<T, EPT>(s, u[r], k, r);
                V[r] = NORM ? (x + 1) * w[r] + mn[r] : x;
            }
            const double Vl = wave_prev(V[EPT - 1]);   // element l*EPT - 1
            const double Vr = wave_next(V[0]);         // element l*EPT + EPT
#pragma unroll
            for (int r = 0; r < EPT; r++) {
                const double L = r > 0 ? V[r - 1] : Vl;
                const double C = V[r];
                const double R = r < EPT - 1 ? V[r + 1] : Vr;
                const double pL = cxx * L, pC = cdg * C, pR = cxx * R;
                // row 0: (cdg C + cxx R) + cxx L; row d-1: (cxx R + cxx L) + cdg C; else
                // (cxx L + cdg C) + cxx R
                const bool b0 = (r == 0) && first, b1 = (r == EPT - 1) && last;
                const double a1 = b0 ? pC : (b1 ? pR : pL);
                const double a2 = b0 ? pR : (b1 ? pL : pC);
                const double a3 = b0 ? pL : (b1 ? pC : pR);
                const double lap = (a1 + a2) + a3;
                const double grad = (-q) * L + q * R;
                double f = lap - C * grad;
                if (NORM) f = f * sc[r];
                k[s * EPT + r] = h * f;
            }
        }
#pragma unroll
        for (int r = 0; r < EPT; r++) u[r] = step_update<T, EPT>(u[r], k, r);   // RK.py:170
        if constexpr (TRAJ) {
            if (tr.due()) {
                double *row = tr.take();
#pragma unroll
                for (int r = 0; r < EPT; r++) row[l * EPT + r] = u[r];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < EPT; r++) uF[l * EPT + r] = u[r];
}
