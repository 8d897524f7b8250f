// nngp_rk_kernels.h -- the batched propagator kernels and their host dispatch, shared by
// nngp_rk.hip (end states: nngp_rk_batch, nngp_rk_batch_grid) and nngp_rk_traj.hip (sampled
// trajectories: nngp_rk_traj), each compiled exact and contracted.  Included INSIDE
// `namespace nngp { inline namespace <variant> {` after nngp_rk_dev.h.
//
// Every kernel and every launch_* / dispatch_* function takes `bool TRAJ` as its last template
// parameter.  TRAJ = false is the end-state propagator, with the code it has always had.  TRAJ =
// true samples the state from inside the step loop (TrajOut, nngp_rk_dev.h); it goes through the
// same dispatch, so a shape runs on the kernel form its end-state launch uses.  A trajectory walks
// the per-slice grid only (gsteps == steps, j0 == 0: RK.run never pages), so the TRAJ kernels
// read `every` from the `gsteps` argument and ignore `j0s`, `uF` is the [n_slices][n_out][d]
// trajectory, and the argument lists -- hence the end-state instantiations -- stay what they were.
#pragma once

// the slice's trajectory block and the arguments of its per-slice grid (TRAJ kernels)
__device__ __forceinline__ double *traj_block(double *traj, int slice, int64_t steps, int64_t every, int d) {
    return traj + (size_t)slice * (size_t)traj_rows(steps, every) * (size_t)d;
}

template <int SYS, int ORDER, bool LINSPACE, bool NORM, bool TRAJ>
__global__ void __launch_bounds__(64) rk_lane_kernel(LaneArgs args, int n_slices,
                                                     const double *__restrict__ t0,
                                                     const double *__restrict__ t1, int64_t steps,
                                                     int64_t gsteps, const int64_t *__restrict__ j0s,
                                                     const double *__restrict__ u0,
                                                     double *__restrict__ uF) {
    constexpr int D = LaneSys<SYS>::D;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_slices) return;
    if constexpr (TRAJ)
        lane_slice<SYS, ORDER, LINSPACE, NORM, true>(args, t0[i], t1[i], steps, steps, 0, u0 + (size_t)i * D,
                                                     traj_block(uF, i, steps, gsteps, D), gsteps);
    else
        lane_slice<SYS, ORDER, LINSPACE, NORM>(args, t0[i], t1[i], steps, gsteps, j0s ? j0s[i] : 0,
                                               u0 + (size_t)i * D, uF + (size_t)i * D);
}

// The lane kernel of the polynomial field (d = D <= 4, at most 16 terms): rk_lane_kernel's body --
// the same lane_slice -- on LaneSys<NNGP_SYS_POLY_LANE + D>, with the table in its own argument
// type (PolyLaneArgs), so rk_lane_kernel's argument block and symbols stay what they were.  There is
// no group form of it.
template <int D, int ORDER, bool LINSPACE, bool NORM, bool TRAJ>
__global__ void __launch_bounds__(64) rk_poly_lane_kernel(PolyLaneArgs args, int n_slices,
                                                          const double *__restrict__ t0,
                                                          const double *__restrict__ t1, int64_t steps,
                                                          int64_t gsteps, const int64_t *__restrict__ j0s,
                                                          const double *__restrict__ u0,
                                                          double *__restrict__ uF) {
    constexpr int SYS = NNGP_SYS_POLY_LANE + D;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_slices) return;
    if constexpr (TRAJ)
        lane_slice<SYS, ORDER, LINSPACE, NORM, true>(args, t0[i], t1[i], steps, steps, 0, u0 + (size_t)i * D,
                                                     traj_block(uF, i, steps, gsteps, D), gsteps);
    else
        lane_slice<SYS, ORDER, LINSPACE, NORM>(args, t0[i], t1[i], steps, gsteps, j0s ? j0s[i] : 0,
                                               u0 + (size_t)i * D, uF + (size_t)i * D);
}

// The lane kernel of a field with atoms (NNGP_SYS_FUNC with d = D <= 4, at most 4 atoms and 16 terms):
// as rk_poly_lane_kernel, on LaneSys<NNGP_SYS_FUNC_LANE + D> with its table in FuncLaneArgs.  No
// group form either.
template <int D, int ORDER, bool LINSPACE, bool NORM, bool TRAJ>
__global__ void __launch_bounds__(64) rk_func_lane_kernel(FuncLaneArgs args, int n_slices,
                                                          const double *__restrict__ t0,
                                                          const double *__restrict__ t1, int64_t steps,
                                                          int64_t gsteps, const int64_t *__restrict__ j0s,
                                                          const double *__restrict__ u0,
                                                          double *__restrict__ uF) {
    constexpr int SYS = NNGP_SYS_FUNC_LANE + D;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_slices) return;
    if constexpr (TRAJ)
        lane_slice<SYS, ORDER, LINSPACE, NORM, true>(args, t0[i], t1[i], steps, steps, 0, u0 + (size_t)i * D,
                                                     traj_block(uF, i, steps, gsteps, D), gsteps);
    else
        lane_slice<SYS, ORDER, LINSPACE, NORM>(args, t0[i], t1[i], steps, gsteps, j0s ? j0s[i] : 0,
                                               u0 + (size_t)i * D, uF + (size_t)i * D);
}

// ---------------------------------------------------------------------------------------------
// Lane-group kernel: one slice = one group of G lanes, each component on its own lanes: G = 16
// (components in DPP banks, below) for every ODE but Thomas labyrinth, G = 4 (lane c = component c,
// lane 3 padding) for Thomas labyrinth's rotation.
// The lane kernel above runs every component's stage sums, (de)normalisation, h*k and final update
// in one lane; here each of those is one instruction per step-part for all components at once, and
// only the RHS coupling crosses lanes: `v_mov_b64_dpp row_newbcast` (gfx950's 64-bit DPP, one VALU
// op) for G = 16, or a quad_perm rotation (two 32-bit DPP ops) for G = 4.
// At few slices the step is one wave's instruction issue (a wave with 1 active
// lane costs the same as 64), so fewer instructions per step is the whole gain, measured on the
// box (tools/lane_group_probe.py): Hopf RK4 119 -> 97 VALU, 0.250 -> 0.201
// us/step; Lorenz 0.29 -> 0.19; Thomas labyrinth one sin per lane instead of three, 1.45 -> 0.47;
// double pendulum one sincos per bank instead of three, 1.82 -> 0.91.
// Hopf since then (GroupSys<HOPF> below): registers carried across stages (85
// VALU), one fused `v_fmac_f64_dpp` per RHS and RK4's third stage re-using the second's u2/mu
// (78), and two steps per loop iteration (the taken branch of a one-step loop is paid in full
// with one wave per SIMD): 0.1725 -> 0.158 us/step (profiles/r07/bench_before_after.txt); then
// RK4's three u2/mu divisions per step as one, in spare lanes of the component's bank (73), and
// four steps per iteration: 0.143 us/step (profiles/r08/bench_before_after.txt).
// Every group kernel since round 9: the tableau's power-of-two entry folded into h (k'_j = (a h) o_j
// stored, u + k'_j used, the column's other coefficients rescaled at compile time: fold_* in
// nngp_rk_dev.h; two VALU fewer per RK4 step, Hopf 71) and sixteen steps per iteration for the
// tableaux of up to four stages (profiles/r09/bench_before_after.txt).
// Hopf RK4 in fixed-step mode since round 13: the time track (GroupSys<HOPF>::track_div, f_take).
// u2 advances by the same INC every step, so the u2/mu quotients of four steps -- twelve of them,
// one per lane of a register of its own -- come from one de-normalisation and one division per
// four steps, formed a pass ahead from instructions that read nothing of the u0/u1 chain and
// stand in its wait states; every stage, stage 0 included, takes its quotient with the move it
// issues anyway, and the sixteen-step loop ends on a scalar compare (69.75 VALU per step, round
// 9: 71.06).  With the track's instructions as the fillers round 9 lacked, three stages per four
// steps fuse the second subtraction of g as well (f_take2): 69.19 (profiles/r13/).
// Since round 14 the sixteen-step loop in normalised coordinates is four asm statements, one per
// pass of four steps, in an order of their own (GroupSys<HOPF>::pass_asm): the update's terms and
// the track's instructions stand in the wait states of the fused ops, so fifteen of a pass's
// sixteen stages fuse both subtractions, and no copy or `s_nop` is left: 66.0 (profiles/r14/).
// Bitwise the lane kernel: each component is rounded by the same expression in the same order
// (the fold: by an expression with the same real value at every rounding, for normal products).
// ---------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ double quad_mov(double v) {
    return __builtin_amdgcn_mov_dpp(v, CTRL, 0xF, 0xF, false);
}
constexpr int QROT = 0xC9;   // quad_perm [1,2,0,3]: lane c reads lane c+1 mod 3

// G = 16: component c lives in DPP bank c (lanes 4c..4c+3 of the row hold the same value; lane 4c
// writes it), so every cross-lane step is one 64-bit `v_mov_b64_dpp row_newbcast` -- the only DPP
// control gfx950 allows on 64-bit operands:
//   bcast<c>(v)            component c's value in every lane;
//   take<L, BANKS>(o, v)   lanes of the banks in BANKS take lane L's v, the others keep o -- a
//                          per-component select in one op (bank_mask), where a 64-bit v_cndmask
//                          is two.
template <int C>
__device__ __forceinline__ double bcast(double v) {
    return __builtin_amdgcn_mov_dpp(v, 0x150 + 4 * C, 0xF, 0xF, false);
}
template <int L, int BANKS>
__device__ __forceinline__ double take(double old, double v) {
    return __builtin_amdgcn_update_dpp(old, v, 0x150 + L, 0xF, BANKS, false);
}

// f(x = own de-normalised component, c = its index, one = 1.0) -> own component of f.  G16 (bank
// layout above) for the broadcast-coupled fields, G4 (lane c = component c) for Thomas
// labyrinth's rotation (quad_perm, two 32-bit DPP ops).
template <int SYS> struct GroupSys;

template <> struct GroupSys<NNGP_SYS_LORENZ> {   // systems.py:232-238, as LaneSys<LORENZ>
    static constexpr int G = 16;
    __device__ static double f(double x, int, double, const LaneArgs &) {
        const double A = bcast<0>(x), B = bcast<1>(x), C = bcast<2>(x);
        const double o0 = 10 * (B - A);
        const double o1 = (28 * A - B) - A * C;
        const double o2 = A * B - (8.0 / 3) * C;
        return take<8, 0x4>(take<4, 0x2>(o0, o1), o2);
    }
};
template <> struct GroupSys<NNGP_SYS_HOPF> {     // systems.py:148-154, as LaneSys<HOPF>
    static constexpr int G = 16;
    // g = (u2/mu - u0*u0) - u1*u1; component 0: -u1 + u0*g, component 1: u0 + u1*g, component 2: 1.
    // Fewer ops than broadcasting u0, u1, u2 and squaring the broadcasts: every lane squares its
    // own component (sq = x*x, the same rounded products) and divides its own component by mu
    // (q = x/mu, div_const; only bank 2's is used), and bank-masked DPP ops into registers carried
    // from stage to stage move only what banks 0 and 1 need -- u2/mu into Q, u1^2 into B2 and the
    // coupling term P (bank 0: u1, bank 1: u0) -- while bank 2's lanes keep what `init` put there:
    // 0 in Q, A2, B2, so g = +-0 and x*g = +-0 (u2 is always finite), and 1.0 in P.
    // The sum p + x*g is one fma(S, P, x*g) with S = -1 in bank 0 and +1 elsewhere: S*P is exact,
    // so the fma is the correctly rounded x*g -+ P, bitwise the reference's addition (signed zeros
    // included: the fma's exact-sum rule is the addition's); bank 2: +-0 + 1 = 1.
    // By the same argument q - u0^2 is ONE `v_fmac_f64_dpp row_newbcast:0`: Q <- fma(bcast(sq), M,
    // Q) with M = -1.0 (in a VGPR: the DPP form takes no inline constant) is the correctly rounded
    // subtraction, in place of a broadcast move plus an add.  12 VALU per RHS.
    //
    // Why only one of the four additions is fused, and why this is inline asm: LLVM does not form
    // v_fmac_f64_dpp, and a DPP op needs EVERY VGPR it reads -- the DPP source, but also the
    // accumulator and the old value of a bank-masked move -- written at least two wait states
    // earlier (tools/ubench_dpp_fma.hip: a fused op right behind the op that wrote its
    // accumulator returns wrong values).  A wait state spent in s_nop costs
    // more than the move it saves, so a fused op pays only where two useful instructions fit
    // between it and its accumulator's writer: here the moves of B2 and P.  Each RHS is ONE asm
    // statement whose order meets every wait state by construction, whatever precedes it: the
    // first DPP op comes after four plain ops (x is read through DPP no sooner), and between any
    // write and a DPP read of the same register stand two instructions (or one and `s_nop 0`).
    //
    // `repeat`: this stage's u2 input is bitwise the previous stage's (bank 2's f is the constant 1,
    // so every k_s[2] is the same h*sc2, and the tableau adds the same multiple of it:
    // group_stage_repeats below), hence so is q = u2/mu: the division and its move are skipped
    // and Q is used again.  The stage before (`keep`) must then leave Q intact, so it subtracts
    // u0^2 with a move into A2 and an add (13 VALU); the repeating stage has 8 (+ s_nop 0: nothing
    // else is left to put between x*x and the first DPP read of x).  RK4: 12 + 13 + 8 + 12.
    // (The contracted build keeps the broadcast form, whose p + x*g contracts to one fma there.)
#ifdef NNGP_RK_FMA
    __device__ static double f(double x, int c, double one, const LaneArgs &a) {
        const double A = bcast<0>(x), B = bcast<1>(x), C = bcast<2>(x);
        const double g = (div_const(C, a.param[0], a.rparam0) - A * A) - B * B;
        const double p = c == 0 ? -B : A;
        return take<8, 0x4>(p + x * g, one);
    }
#else
    struct St {
        double Q, A2, B2, P, S, M;
    };
    __device__ static St init(int c) {
        return St{0.0, 0.0, 0.0, c == 2 ? 1.0 : 0.0, c == 0 ? -1.0 : 1.0, -1.0};
    }
    // q = x/mu (div_const) and sq = x*x in every lane, then P, Q, B2 in an order that leaves two
    // instructions between each register's write and its DPP read: q -> (sq, P) -> Q;
    // sq -> (P, Q) -> B2; P -> (Q, B2) -> P; Q -> (B2, P) -> the op after this block
#define NNGP_HOPF_HEAD                                                        \
    "v_mul_f64 %[q], %[x], %[r]\n\t"                                          \
    "v_fma_f64 %[e], -%[q], %[b], %[x]\n\t"                                   \
    "v_fma_f64 %[q], %[e], %[r], %[q]\n\t"                                    \
    "v_mul_f64 %[sq], %[x], %[x]\n\t"                                         \
    "v_mov_b64_dpp %[P], %[x] row_newbcast:4 row_mask:0xf bank_mask:0x1\n\t"   \
    "v_mov_b64_dpp %[Q], %[q] row_newbcast:8 row_mask:0xf bank_mask:0x3\n\t"   \
    "v_mov_b64_dpp %[B2], %[sq] row_newbcast:4 row_mask:0xf bank_mask:0x3\n\t" \
    "v_mov_b64_dpp %[P], %[x] row_newbcast:0 row_mask:0xf bank_mask:0x2\n\t"
    // g = (q - u0^2) - u1^2 from FROM = q - u0^2, then x*g and fma(S, P, x*g)
#define NNGP_HOPF_TAIL(FROM)                        \
    "v_add_f64 %[t], %[" FROM "], -%[B2]\n\t"       \
    "v_mul_f64 %[t], %[x], %[t]\n\t"                \
    "v_fma_f64 %[o], %[S], %[P], %[t]"
    __device__ static double f(double x, St &s, bool repeat, bool keep, const LaneArgs &a) {
        double o, sq, e, q, t;
        if (repeat) {   // Q is the previous stage's and is used up here: P -> (B2, fused) -> P
            asm("v_mul_f64 %[sq], %[x], %[x]\n\t"
                "s_nop 0\n\t"
                "v_mov_b64_dpp %[P], %[x] row_newbcast:4 row_mask:0xf bank_mask:0x1\n\t"
                "v_mov_b64_dpp %[B2], %[sq] row_newbcast:4 row_mask:0xf bank_mask:0x3\n\t"
                "v_fmac_f64_dpp %[Q], %[sq], %[M] row_newbcast:0 row_mask:0xf bank_mask:0x3\n\t"
                "v_mov_b64_dpp %[P], %[x] row_newbcast:0 row_mask:0xf bank_mask:0x2\n\t"
                NNGP_HOPF_TAIL("Q")
                : [o] "=&v"(o), [sq] "=&v"(sq), [t] "=&v"(t), [Q] "+v"(s.Q), [B2] "+v"(s.B2), [P] "+v"(s.P)
                : [x] "v"(x), [S] "v"(s.S), [M] "v"(s.M));
        } else if (keep) {   // Q stays q for the next stage
            asm(NNGP_HOPF_HEAD
                "v_mov_b64_dpp %[A2], %[sq] row_newbcast:0 row_mask:0xf bank_mask:0x3\n\t"
                "v_add_f64 %[t], %[Q], -%[A2]\n\t" NNGP_HOPF_TAIL("t")
                : [o] "=&v"(o), [sq] "=&v"(sq), [t] "=&v"(t), [e] "=&v"(e), [q] "=&v"(q), [Q] "+v"(s.Q),
                  [A2] "+v"(s.A2), [B2] "+v"(s.B2), [P] "+v"(s.P)
                : [x] "v"(x), [S] "v"(s.S), [b] "v"(a.param[0]), [r] "v"(a.rparam0));
        } else {
            asm(NNGP_HOPF_HEAD
                "v_fmac_f64_dpp %[Q], %[sq], %[M] row_newbcast:0 row_mask:0xf bank_mask:0x3\n\t"
                NNGP_HOPF_TAIL("Q")
                : [o] "=&v"(o), [sq] "=&v"(sq), [t] "=&v"(t), [e] "=&v"(e), [q] "=&v"(q), [Q] "+v"(s.Q),
                  [B2] "+v"(s.B2), [P] "+v"(s.P)
                : [x] "v"(x), [S] "v"(s.S), [M] "v"(s.M), [b] "v"(a.param[0]), [r] "v"(a.rparam0));
        }
        return o;
    }
    // The time track (RK4 in fixed-step mode: group_tracks below).
    // Bank 2's f is the constant 1, so in fixed-step mode its four k are the same constants at every
    // step of the slice and u2 advances by the same INC = RN(sum b k) per step, whatever u0 and u1
    // do: every time input of the next four steps -- u2_j at stage 0, u2_j + RN(a k2) at the later
    // stages, two distinct a in RK4 -- is known before those steps start.  A register of its own,
    // the track, holds them for four steps at once: lane 4j + r of a slice's 16 carries step j's u2
    // (j = 0..3, the same in the four lanes of a j) and, after one add of the per-lane constant OFFr
    // (-0.0, RN(a0 k2), RN(a1 k2) for r = 0, 1, 2; x + (-0.0) is x bit for bit, zeros of either sign
    // included), one de-normalisation with component 2's constants and ONE Markstein division, the
    // quotient of step j's stage 0 (r = 0), stages 1 and 2 (r = 1) and stage 3 (r = 2): the roundings
    // the reference performs on that stage's time input, 12 of them in one pass.  Every stage of
    // the four steps, stage 0 included, is a take stage: it fetches its u2/mu with the bank-masked
    // `row_newbcast:L` move it needs anyway and divides nothing.  The track advances by four
    // dependent adds of INC per batch, the sequential roundings lane 8 performs on u, so it reads
    // nothing of the u0/u1 chain inside the loop and its 11 instructions per four steps (8 without
    // de-normalisation) are free to stand wherever that chain leaves a wait state.  The state u is
    // advanced in bank 2 as ever (P = 1, Q = B2 = 0 there).
    // Wait states of a take stage (every VGPR a DPP op reads written at least two instructions
    // earlier): x may be written by the instruction before the statement, so its first DPP read is
    // the third op, behind x*x and the move of the quotient; the quotient register is written by
    // the first instruction of track_div's statement, whose second (one of the track's adds)
    // follows it, and x*x stands in front of the move that reads it; Q was written by the previous
    // statement's fused op, which its three-op tail follows (before the first statement:
    // track_settle), and nothing between two statements writes Q, B2 or P (no other code names
    // them); sq -> (Q, P) -> B2; Q -> (P, B2) -> fused; P -> (B2, fused) -> P.
    static constexpr int TC = 2;   // the time component
    // the last op of the track's division and one of its adds: a quotient register is never
    // written by the instruction in front of a take statement
    // x/mu as div_const forms it, q = RN(x r), fma(fma(-q, mu, x), r, q); tu advances by inc
    __device__ static double track_div(double x, double &tu, double inc, const LaneArgs &a) {
        const double q = x * a.rparam0, e = fma(-q, a.param[0], x);
        double o;
        asm("v_fma_f64 %[o], %[e], %[r], %[q]\n\t"
            "v_add_f64 %[tu], %[tu], %[inc]"
            : [o] "=&v"(o), [tu] "+v"(tu)
            : [e] "v"(e), [q] "v"(q), [r] "v"(a.rparam0), [inc] "v"(inc));
        return o;
    }
    // before the first take statement: whatever initialised the carried registers is two wait
    // states away
    __device__ static void track_settle(St &s) {
        asm volatile("s_nop 1" : "+v"(s.Q), "+v"(s.B2), "+v"(s.P), "+v"(s.S), "+v"(s.M));
    }
    // lane L of the track's quotients qt into Q, then the round-7 right-hand side
    template <int L>
    __device__ static double f_take(double x, St &s, double qt) {
        double o, sq, t;
        asm("v_mul_f64 %[sq], %[x], %[x]\n\t"
            "v_mov_b64_dpp %[Q], %[q] row_newbcast:%[L] row_mask:0xf bank_mask:0x3\n\t"
            "v_mov_b64_dpp %[P], %[x] row_newbcast:4 row_mask:0xf bank_mask:0x1\n\t"
            "v_mov_b64_dpp %[B2], %[sq] row_newbcast:4 row_mask:0xf bank_mask:0x3\n\t"
            "v_fmac_f64_dpp %[Q], %[sq], %[M] row_newbcast:0 row_mask:0xf bank_mask:0x3\n\t"
            "v_mov_b64_dpp %[P], %[x] row_newbcast:0 row_mask:0xf bank_mask:0x2\n\t"
            NNGP_HOPF_TAIL("Q")
            : [o] "=&v"(o), [sq] "=&v"(sq), [t] "=&v"(t), [Q] "+v"(s.Q), [B2] "+v"(s.B2), [P] "+v"(s.P)
            : [x] "v"(x), [q] "v"(qt), [S] "v"(s.S), [M] "v"(s.M), [L] "n"(L));
        return o;
    }
    // A take stage with BOTH subtractions of g fused: Q <- fma(bcast(u1^2), M, Q) by a second
    // `v_fmac_f64_dpp row_newbcast:4` on the same square, in place of B2's move and the add -- the
    // correctly rounded (q - u0^2) - u1^2 by the argument above (bank 2 keeps Q = +0, the 0 - 0 of
    // the unfused form).  Each fused op needs its accumulator written two instructions earlier,
    // and the chain has nothing of its own to put there (rounds 7 and 9): the
    // two slots F1 and F2 take two instructions of the track, which read nothing of the chain and
    // are written to tk, a register set no DPP op reads.  8 chain ops instead of 9.
    // Wait states: sq -> (Q, P, F1) -> fused; Q -> (P, F1) -> fused -> (P, F2) -> fused; P ->
    // (F1, fused) -> P; x and the quotient as in f_take; B2 is not touched.  The statement ends
    // with two plain ops behind its last write of Q, so the next statement's move into Q is safe.
    struct Tk { double x, q, e; };   // the track's division in flight: its input, RN(x r), the residual
#define NNGP_HOPF_TAKE2(F1, F2)                                                       \
    asm("v_mul_f64 %[sq], %[x], %[x]\n\t"                                             \
        "v_mov_b64_dpp %[Q], %[q] row_newbcast:%[L] row_mask:0xf bank_mask:0x3\n\t"   \
        "v_mov_b64_dpp %[P], %[x] row_newbcast:4 row_mask:0xf bank_mask:0x1\n\t"      \
        F1 "\n\t"                                                                     \
        "v_fmac_f64_dpp %[Q], %[sq], %[M] row_newbcast:0 row_mask:0xf bank_mask:0x3\n\t" \
        "v_mov_b64_dpp %[P], %[x] row_newbcast:0 row_mask:0xf bank_mask:0x2\n\t"      \
        F2 "\n\t"                                                                     \
        "v_fmac_f64_dpp %[Q], %[sq], %[M] row_newbcast:4 row_mask:0xf bank_mask:0x3\n\t" \
        "v_mul_f64 %[t], %[x], %[Q]\n\t"                                              \
        "v_fma_f64 %[o], %[S], %[P], %[t]"                                            \
        : [o] "=&v"(o), [sq] "=&v"(sq), [t] "=&v"(t), [Q] "+v"(s.Q), [P] "+v"(s.P),   \
          [tx] "+v"(tk.x), [tq] "+v"(tk.q), [te] "+v"(tk.e)                           \
        : [x] "v"(x), [q] "v"(qt), [S] "v"(s.S), [M] "v"(s.M), [L] "n"(L), [tu] "v"(tu), \
          [offr] "v"(offr), [hw2] "v"(hw2), [mn2] "v"(mn2), [r] "v"(a.rparam0), [b] "v"(a.param[0]))
    // K: which two of the track's instructions the statement carries.  Normalised: 1 = tu + OFFr
    // and + 1, 2 = * hw and + mn, 3 = x r and the residual.  Identity: 4 = tu + OFFr and x r.
    template <int L, int K>
    __device__ static double f_take2(double x, St &s, double qt, Tk &tk, double tu, double offr, double hw2,
                                     double mn2, const LaneArgs &a) {
        static_assert(K >= 1 && K <= 4, "one of the four pairs");
        double o, sq, t;
        if constexpr (K == 1) NNGP_HOPF_TAKE2("v_add_f64 %[tx], %[tu], %[offr]", "v_add_f64 %[tx], %[tx], 1.0");
        else if constexpr (K == 2) NNGP_HOPF_TAKE2("v_mul_f64 %[tx], %[tx], %[hw2]", "v_add_f64 %[tx], %[tx], %[mn2]");
        else if constexpr (K == 3) NNGP_HOPF_TAKE2("v_mul_f64 %[tq], %[tx], %[r]", "v_fma_f64 %[te], -%[tq], %[b], %[tx]");
        else NNGP_HOPF_TAKE2("v_add_f64 %[tx], %[tu], %[offr]", "v_mul_f64 %[tq], %[tx], %[r]");
        return o;
    }
    // the end of the division the fused take stages left in tk, and one of the track's adds (as
    // track_div: the quotient register is not written by the last instruction of the statement)
    __device__ static double track_fin(const Tk &tk, double &tu, double inc, const LaneArgs &a) {
        double o;
        asm("v_fma_f64 %[o], %[e], %[r], %[q]\n\t"
            "v_add_f64 %[tu], %[tu], %[inc]"
            : [o] "=&v"(o), [tu] "+v"(tu)
            : [e] "v"(tk.e), [q] "v"(tk.q), [r] "v"(a.rparam0), [inc] "v"(inc));
        return o;
    }
    // A whole pass of the time track -- four RK4 steps in normalised coordinates, the next pass's
    // quotients and the track's four adds -- as ONE asm statement (the sixteen-step loop of
    // rk_group_kernel).  The compiler cannot see which
    // instruction of an asm statement wrote an output, so it puts a wait state in front of
    // whatever reads one next and fills it with the update's terms; with a statement per RHS those
    // terms were spent on its padding.  Inside one statement nothing is inserted and the order is
    // ours, so the update's terms and the track's instructions stand in the two slots F1 and F2
    // of the doubly fused stage (f_take2's order), and fifteen of the sixteen stages of a pass
    // subtract both squares by `v_fmac_f64_dpp`.  Every value is rounded by the expression the
    // C++ form rounds it by, in the same order: x = ((u + k') + 1) hw + mn, the take stage,
    // o sc, (a h) o, and u + (((b0 k'0 + b1 k'1) + b2 k2) + b3 k3) (fold_step_update).
    // Fillers, per step j of the pass (T1..T7: + OFFr, + 1, hw2, + mn2, x r, the residual, the
    // quotient; TA: tu + INC):
    //   stage 0:  two of the track's      j = 0: T1 T2,  1: T4 T5,  2: T7 TA,  3: TA TA
    //   stage 1:  b0 k'0, one of the track's      0: T3,     1: T6,     2: TA,     3: none
    //   stage 2:  b1 k'1, the sum of the two
    //   stage 3:  b2 k2, the next sum
    // The track has eleven instructions for twelve slots, so stage 1 of step 3 keeps the singly
    // fused form (f_take's: u1^2 through B2 and an add), which needs no filler: 4 x 63 + 1 + 11 =
    // 264 VALU per pass.
    // Wait states (every VGPR a DPP op reads written at least two instructions earlier), stage by
    // stage as in f_take2: x -> (x x, Q) -> P; sq -> (Q, P, F1) -> fused; Q -> (P, F1) -> fused ->
    // (P, F2) -> fused; P -> (F1, fused) -> P, and in the singly fused stage sq -> (Q, P) -> B2,
    // Q -> (P, B2) -> fused, P -> (B2, fused) -> P.  No filler writes a register a DPP op reads
    // but T7, the next pass's quotients QN: never the register this pass takes from (QT; the two
    // alternate between consecutive passes through the operand bindings, so no copy is issued),
    // and written in stage 0 of step 2, a step and a half before the statement ends.  From one
    // stage to the next, Q, P and B2 are read no sooner than four plain ops after the stage's last
    // fused op (x Q, the fma, sc, (a h), then the next stage's input).  Pass -> next pass, the
    // loop's back edge included: the statement ends with the update's three plain ops and starts
    // with x's three and x x, so its first DPP op is seven instructions from any write of the
    // statement before, whatever the compiler puts between the two.
    struct PassC {   // what a pass reads and does not write
        double hw, mn, sc, h[4], b[4], inc, offr, hw2, mn2, r, mu;   // r, mu: div_const's 1/mu and mu
    };
#define NNGP_HOPF_T1 "v_add_f64 %[tx], %[tu], %[offr]"
#define NNGP_HOPF_T2 "v_add_f64 %[tx], %[tx], 1.0"
#define NNGP_HOPF_T3 "v_mul_f64 %[tx], %[tx], %[hw2]"
#define NNGP_HOPF_T4 "v_add_f64 %[tx], %[tx], %[mn2]"
#define NNGP_HOPF_T5 "v_mul_f64 %[tq], %[tx], %[r]"
#define NNGP_HOPF_T6 "v_fma_f64 %[te], -%[tq], %[b], %[tx]"
#define NNGP_HOPF_T7 "v_fma_f64 %[QN], %[te], %[r], %[tq]"
#define NNGP_HOPF_TA "v_add_f64 %[tu], %[tu], %[inc]"
#define NNGP_HOPF_U1 "v_mul_f64 %[a0], %[b0], %[k0]"
#define NNGP_HOPF_U2 "v_mul_f64 %[a1], %[b1], %[k1]"
#define NNGP_HOPF_U3 "v_add_f64 %[a0], %[a0], %[a1]"
#define NNGP_HOPF_U4 "v_mul_f64 %[a1], %[b2], %[k2]"
#define NNGP_HOPF_U5 "v_add_f64 %[a0], %[a0], %[a1]"
    // the stage's input, de-normalised: stage 0 from u, a later stage from u + k' of the stage before
#define NNGP_HOPF_IN0 "v_add_f64 %[x], %[u], 1.0\n\t"
#define NNGP_HOPF_IN(K) "v_add_f64 %[x], %[u], %[" K "]\n\tv_add_f64 %[x], %[x], 1.0\n\t"
    // x, the take stage with both subtractions fused (lane L of QT), then k'_s = (a h)(o sc) into K
#define NNGP_HOPF_STAGE2(L, F1, F2, K, H)                                                \
    "v_mul_f64 %[x], %[x], %[hw]\n\t"                                                    \
    "v_add_f64 %[x], %[x], %[mn]\n\t"                                                    \
    "v_mul_f64 %[sq], %[x], %[x]\n\t"                                                    \
    "v_mov_b64_dpp %[Q], %[QT] row_newbcast:" L " row_mask:0xf bank_mask:0x3\n\t"        \
    "v_mov_b64_dpp %[P], %[x] row_newbcast:4 row_mask:0xf bank_mask:0x1\n\t"             \
    F1 "\n\t"                                                                            \
    "v_fmac_f64_dpp %[Q], %[sq], %[M] row_newbcast:0 row_mask:0xf bank_mask:0x3\n\t"     \
    "v_mov_b64_dpp %[P], %[x] row_newbcast:0 row_mask:0xf bank_mask:0x2\n\t"             \
    F2 "\n\t"                                                                            \
    "v_fmac_f64_dpp %[Q], %[sq], %[M] row_newbcast:4 row_mask:0xf bank_mask:0x3\n\t"     \
    "v_mul_f64 %[t], %[x], %[Q]\n\t"                                                     \
    "v_fma_f64 %[t], %[S], %[P], %[t]\n\t"                                               \
    "v_mul_f64 %[t], %[t], %[sc]\n\t"                                                    \
    "v_mul_f64 %[" K "], %[" H "], %[t]\n\t"
    // the same with f_take's singly fused stage, which has no slot to fill
#define NNGP_HOPF_STAGE1(L, K, H)                                                        \
    "v_mul_f64 %[x], %[x], %[hw]\n\t"                                                    \
    "v_add_f64 %[x], %[x], %[mn]\n\t"                                                    \
    "v_mul_f64 %[sq], %[x], %[x]\n\t"                                                    \
    "v_mov_b64_dpp %[Q], %[QT] row_newbcast:" L " row_mask:0xf bank_mask:0x3\n\t"        \
    "v_mov_b64_dpp %[P], %[x] row_newbcast:4 row_mask:0xf bank_mask:0x1\n\t"             \
    "v_mov_b64_dpp %[B2], %[sq] row_newbcast:4 row_mask:0xf bank_mask:0x3\n\t"           \
    "v_fmac_f64_dpp %[Q], %[sq], %[M] row_newbcast:0 row_mask:0xf bank_mask:0x3\n\t"     \
    "v_mov_b64_dpp %[P], %[x] row_newbcast:0 row_mask:0xf bank_mask:0x2\n\t"             \
    "v_add_f64 %[t], %[Q], -%[B2]\n\t"                                                   \
    "v_mul_f64 %[t], %[x], %[t]\n\t"                                                     \
    "v_fma_f64 %[t], %[S], %[P], %[t]\n\t"                                               \
    "v_mul_f64 %[t], %[t], %[sc]\n\t"                                                    \
    "v_mul_f64 %[" K "], %[" H "], %[t]\n\t"
    // stages 2 and 3 and the end of the update, the same in every step; L1, L3: the lanes of the
    // quotients of stages 1 and 2, and of stage 3
#define NNGP_HOPF_STEP_END(L1, L3)                                                       \
    NNGP_HOPF_IN("k1") NNGP_HOPF_STAGE2(L1, NNGP_HOPF_U2, NNGP_HOPF_U3, "k2", "h2")      \
    NNGP_HOPF_IN("k2") NNGP_HOPF_STAGE2(L3, NNGP_HOPF_U4, NNGP_HOPF_U5, "k3", "h3")      \
    "v_mul_f64 %[a1], %[b3], %[k3]\n\t"                                                  \
    "v_add_f64 %[a0], %[a0], %[a1]\n\t"                                                  \
    "v_add_f64 %[u], %[u], %[a0]\n\t"
    // a step whose stages 0 and 1 carry the track's TA, TB and TC
#define NNGP_HOPF_STEP(L0, L1, L3, TA_, TB_, TC_)                                        \
    NNGP_HOPF_IN0 NNGP_HOPF_STAGE2(L0, TA_, TB_, "k0", "h0")                             \
    NNGP_HOPF_IN("k0") NNGP_HOPF_STAGE2(L1, NNGP_HOPF_U1, TC_, "k1", "h1")               \
    NNGP_HOPF_STEP_END(L1, L3)
    __device__ static void pass_asm(double &u, St &s, double qt, double &qn, double &tu, const PassC &c) {
        double x, sq, t, k0, k1, k2, k3, a0, a1, tx, tq, te;
        asm(NNGP_HOPF_STEP("0", "1", "2", NNGP_HOPF_T1, NNGP_HOPF_T2, NNGP_HOPF_T3)
            NNGP_HOPF_STEP("4", "5", "6", NNGP_HOPF_T4, NNGP_HOPF_T5, NNGP_HOPF_T6)
            NNGP_HOPF_STEP("8", "9", "10", NNGP_HOPF_T7, NNGP_HOPF_TA, NNGP_HOPF_TA)
            NNGP_HOPF_IN0 NNGP_HOPF_STAGE2("12", NNGP_HOPF_TA, NNGP_HOPF_TA, "k0", "h0")
            NNGP_HOPF_U1 "\n\t"
            NNGP_HOPF_IN("k0") NNGP_HOPF_STAGE1("13", "k1", "h1")
            NNGP_HOPF_STEP_END("13", "14")
            : [u] "+v"(u), [tu] "+v"(tu), [Q] "+v"(s.Q), [P] "+v"(s.P), [B2] "+v"(s.B2), [QN] "=&v"(qn),
              [x] "=&v"(x), [sq] "=&v"(sq), [t] "=&v"(t), [k0] "=&v"(k0), [k1] "=&v"(k1), [k2] "=&v"(k2),
              [k3] "=&v"(k3), [a0] "=&v"(a0), [a1] "=&v"(a1), [tx] "=&v"(tx), [tq] "=&v"(tq), [te] "=&v"(te)
            : [QT] "v"(qt), [S] "v"(s.S), [M] "v"(s.M), [hw] "v"(c.hw), [mn] "v"(c.mn), [sc] "v"(c.sc),
              [h0] "v"(c.h[0]), [h1] "v"(c.h[1]), [h2] "v"(c.h[2]), [h3] "v"(c.h[3]), [b0] "v"(c.b[0]),
              [b1] "v"(c.b[1]), [b2] "v"(c.b[2]), [b3] "v"(c.b[3]), [inc] "v"(c.inc), [offr] "v"(c.offr),
              [hw2] "v"(c.hw2), [mn2] "v"(c.mn2), [r] "v"(c.r), [b] "v"(c.mu));
    }
#undef NNGP_HOPF_STEP
#undef NNGP_HOPF_STEP_END
#undef NNGP_HOPF_STAGE1
#undef NNGP_HOPF_STAGE2
#undef NNGP_HOPF_IN
#undef NNGP_HOPF_IN0
#undef NNGP_HOPF_U5
#undef NNGP_HOPF_U4
#undef NNGP_HOPF_U3
#undef NNGP_HOPF_U2
#undef NNGP_HOPF_U1
#undef NNGP_HOPF_TA
#undef NNGP_HOPF_T7
#undef NNGP_HOPF_T6
#undef NNGP_HOPF_T5
#undef NNGP_HOPF_T4
#undef NNGP_HOPF_T3
#undef NNGP_HOPF_T2
#undef NNGP_HOPF_T1
#undef NNGP_HOPF_TAKE2
#undef NNGP_HOPF_HEAD
#undef NNGP_HOPF_TAIL
#endif
};
template <> struct GroupSys<NNGP_SYS_THOMAS_LABYRINTH> {   // systems.py:257-271
    static constexpr int G = 4;
    __device__ static double f(double x, int, double, const LaneArgs &) {
        const double sn = quad_mov<QROT>(nn_sin_pi(x));   // sin(u[c+1 mod 3])
        return -0.5 * x + 10.0 * sn;
    }
};
template <> struct GroupSys<NNGP_SYS_ROSSLER> {  // systems.py:116-125
    static constexpr int G = 16;
    __device__ static double f(double x, int, double, const LaneArgs &) {
        const double A = bcast<0>(x), B = bcast<1>(x), C = bcast<2>(x);
        return take<8, 0x4>(take<4, 0x2>(-B - C, A + (0.2 * B)), 0.2 + C * (A - 5.7));
    }
};

template <> struct GroupSys<NNGP_SYS_FHN_ODE> {  // systems.py:87-95, as LaneSys<FHN_ODE>
    static constexpr int G = 16;
    __device__ static double f(double x, int, double, const LaneArgs &) {
        const double A = bcast<0>(x), B = bcast<1>(x);
        const double c = 3;
        const double o0 = c * ((A - div_const(A * (A * A), 3.0, 1.0 / 3)) + B);
        const double o1 = -(1 / c) * ((A - 0.2) + 0.2 * B);
        return take<4, 0x2>(o0, o1);
    }
};
template <> struct GroupSys<NNGP_SYS_BRUSSELATOR> {  // systems.py:209-214, as LaneSys<BRUSSELATOR>
    static constexpr int G = 16;
    __device__ static double f(double x, int, double, const LaneArgs &) {
        const double A = bcast<0>(x), B = bcast<1>(x);
        const double o0 = (1 + (A * A) * B) - (3 + 1) * A;
        const double o1 = 3 * A - (A * A) * B;
        return take<4, 0x2>(o0, o1);
    }
};
template <> struct GroupSys<NNGP_SYS_DBL_PEND> {  // systems.py:182-189, as LaneSys<DBL_PEND>
    static constexpr int G = 16;
    __device__ static double f(double x, int, double, const LaneArgs &) {
        const double A = bcast<0>(x), B = bcast<1>(x), C = bcast<2>(x), D = bcast<3>(x);
        // the lane kernel's three sincos (of u0-u2, u0, u2) as one per bank: bank 0 takes u0-u2,
        // bank 1 u0 (lane 0's x), bank 2 u2 (lane 8's x)
        const double arg = take<8, 0x4>(take<0, 0x2>(A - C, x), x);
        double sn, cs;
        nn_sincos(arg, sn, cs);
        const double s = bcast<0>(sn), c = bcast<0>(cs), s0 = bcast<1>(sn), s2 = bcast<2>(sn);
        const double pre = -1 / (2 - c * c);
        const double o1 = pre * ((((B * B) * c) * s + (D * D) * s) + 2 * s0 - c * s2);
        const double o3 = pre * ((((-2 * (B * B)) * s - ((D * D) * s) * c) - (2 * c) * s0) + 2 * s2);
        // component 0: u1, 1: o1, 2: u3 (lane 12's x), 3: o3
        return take<12, 0x8>(take<12, 0x4>(take<4, 0x2>(B, o1), x), o3);
    }
};

// Per-lane state a group RHS carries from stage to stage (GroupSys<SYS>::St, made by its init(c));
// a field without one gets its component index.
template <class GS, class = void> struct GroupState {
    using T = int;
    __device__ static int init(int c) { return c; }
};
template <class GS> struct GroupState<GS, std::void_t<typename GS::St>> {
    using T = typename GS::St;
    __device__ static T init(int c) { return GS::init(c); }
};

// Stage s adds to u exactly what stage s-1 added, taken one stage later: rows s and s-1 of the
// tableau each have a single non-zero entry, of the same value, on k_{s-1} and k_{s-2}.  A
// component whose f is the same constant at every stage (all its k_j bitwise equal) then has the
// same stage input at s as at s-1, and a group RHS may carry what it derived from it (RK4: s = 2,
// u + k0/2 and u + k1/2; no stage of RK1, RK2 or RK8).
template <typename T>
__host__ __device__ constexpr bool group_stage_repeats(int s) {
    if (s < 2 || s >= T::S) return false;
    for (int j = 0; j < s; j++) {
        if ((T::A[s][j] != 0.0) != (j == s - 1)) return false;
        if (j < s - 1 && (T::A[s - 1][j] != 0.0) != (j == s - 2)) return false;
    }
    return T::A[s][s - 1] == T::A[s - 1][s - 2];
}
template <typename T>
constexpr int group_repeat_count() {   // -1: two repeating stages in a row
    int n = 0;
    for (int s = 0; s <= T::S; s++) {
        if (group_stage_repeats<T>(s) && group_stage_repeats<T>(s + 1)) return -1;
        n += group_stage_repeats<T>(s);
    }
    return n;
}
static_assert(group_stage_repeats<Tableau<4>>(2) && group_repeat_count<Tableau<4>>() == 1,
              "RK4: the third stage, and only it, repeats");
static_assert(group_repeat_count<Tableau<1>>() == 0 && group_repeat_count<Tableau<2>>() == 0 &&
              group_repeat_count<Tableau<8>>() == 0, "RK1, RK2, RK8: no stage repeats");

// Lane batching of a component whose f is the same constant at every stage (all its k_j bitwise
// equal, k): its input at stage 0 is u, and at a stage whose tableau row has a single non-zero
// entry a it is u + RN(a*k) whichever k_j the entry is on, so what a group RHS derives from those
// inputs can be computed for all of them at once, in lanes of their own (slot = the index of a
// among the tableau's distinct such entries, in order of appearance; a repeating stage has its
// predecessor's).  group_batch_slot: -1 for stage 0, the slot, or -2 where the input has another
// form (a later row with none or several entries).  The time track (group_tracks below) is built
// for exactly two slots: RK4 (a = 1/2 at stages 1 and 2, a = 1 at stage 3); not RK1 and RK2 (no
// and one slot) nor RK8 (row 2 has two entries), which keep the form above.
template <typename T>
__host__ __device__ constexpr double group_batch_entry(int s) {   // the single entry of row s, or 0.0
    double a = 0.0;
    for (int j = 0; j < s; j++) {
        if (T::A[s][j] == 0.0) continue;
        if (a != 0.0) return 0.0;
        a = T::A[s][j];
    }
    return a;
}
template <typename T>
__host__ __device__ constexpr int group_batch_slot(int s) {
    if (s == 0) return -1;
    const double a = group_batch_entry<T>(s);
    if (a == 0.0) return -2;
    int slot = 0;   // the distinct entries of the rows before a's first
    for (int r = 1; group_batch_entry<T>(r) != a; r++) {
        bool seen = false;
        for (int q = 1; q < r; q++) seen = seen || group_batch_entry<T>(q) == group_batch_entry<T>(r);
        slot += !seen;
    }
    return slot;
}
template <typename T>
__host__ __device__ constexpr int group_batch_slots() {   // how many slots, -1: not of this form
    int n = 0;
    for (int s = 1; s < T::S; s++) {
        const int slot = group_batch_slot<T>(s);
        if (slot == -2) return -1;
        n = slot + 1 > n ? slot + 1 : n;
    }
    return n;
}
template <typename T>
__host__ __device__ constexpr double group_batch_coef(int slot) {   // the entry a of a slot
    for (int s = 1; s < T::S; s++)
        if (group_batch_slot<T>(s) == slot) return group_batch_entry<T>(s);
    return 0.0;
}
static_assert(group_batch_slots<Tableau<4>>() == 2 && group_batch_slot<Tableau<4>>(1) == 0 &&
              group_batch_slot<Tableau<4>>(2) == 0 && group_batch_slot<Tableau<4>>(3) == 1 &&
              group_batch_coef<Tableau<4>>(0) == 0.5 && group_batch_coef<Tableau<4>>(1) == 1.0,
              "RK4: u + k/2 at stages 1 and 2, u + k at stage 3");
static_assert(group_batch_slots<Tableau<1>>() == 0 && group_batch_slots<Tableau<2>>() == 1 &&
              group_batch_slots<Tableau<8>>() == -1, "RK1, RK2, RK8: not lane-batched");
// The time track: a group RHS with a track_div keeps the constant component's inputs of four steps
// at once (GroupSys<HOPF>) when the tableau has exactly the two slots the form is built for, so
// that lane 4j + slot + 1 of the track holds step j's stage input of that slot (slot -1: stage 0).
template <typename T>
__host__ __device__ constexpr bool group_track_tableau() { return group_batch_slots<T>() == 2; }
static_assert(group_track_tableau<Tableau<4>>(), "RK4: the time track applies");
static_assert(!group_track_tableau<Tableau<1>>() && !group_track_tableau<Tableau<2>>() &&
              !group_track_tableau<Tableau<8>>(), "RK1, RK2, RK8: no time track");
constexpr int TRACK_STEPS = 4;   // steps per pass of the track: 4 lanes per step, 16 per slice
template <class GS, typename T, class = void> struct group_tracks {
    static constexpr bool value = false;
};
template <class GS, typename T> struct group_tracks<GS, T, std::void_t<decltype(&GS::track_div)>> {
    static constexpr bool value = group_track_tableau<T>();
};

// stage s of the group RHS: a field with carried state (St) is told whether the stage repeats and
// whether the next one will (never both: what a stage keeps, the next uses up)
template <int SYS, typename T, typename G>
__device__ __forceinline__ double group_f(int s, double x, G &gst, double one, const LaneArgs &args) {
    if constexpr (std::is_same_v<G, int>) return GroupSys<SYS>::f(x, gst, one, args);
    else return GroupSys<SYS>::f(x, gst, group_stage_repeats<T>(s), group_stage_repeats<T>(s + 1), args);
}
// stage s of step J of a pass of the time track: the RHS takes lane 4 J + slot + 1 of the quotients
template <typename T> struct GroupBatchSlots {
    int slot[T::S];
};
template <typename T>
constexpr GroupBatchSlots<T> group_batch_table() {
    GroupBatchSlots<T> t{};
    for (int s = 0; s < T::S; s++) t.slot[s] = group_batch_slot<T>(s);
    return t;
}
template <int SYS, typename T, int J, typename G>
__device__ __forceinline__ double group_f_track(int s, double x, G &gst, double qt) {
    static_assert(J >= 0 && J < TRACK_STEPS, "a pass of the track holds TRACK_STEPS steps");
    constexpr GroupBatchSlots<T> tab = group_batch_table<T>();   // a constant once s is unrolled
    const int slot = tab.slot[s];
    if (slot < 0) return GroupSys<SYS>::template f_take<4 * J>(x, gst, qt);
    if (slot == 0) return GroupSys<SYS>::template f_take<4 * J + 1>(x, gst, qt);
    return GroupSys<SYS>::template f_take<4 * J + 2>(x, gst, qt);
}

template <int SYS> struct has_group { static constexpr bool value = false; };
template <> struct has_group<NNGP_SYS_LORENZ> { static constexpr bool value = true; };
template <> struct has_group<NNGP_SYS_HOPF> { static constexpr bool value = true; };
template <> struct has_group<NNGP_SYS_THOMAS_LABYRINTH> { static constexpr bool value = true; };
template <> struct has_group<NNGP_SYS_ROSSLER> { static constexpr bool value = true; };
template <> struct has_group<NNGP_SYS_FHN_ODE> { static constexpr bool value = true; };
template <> struct has_group<NNGP_SYS_BRUSSELATOR> { static constexpr bool value = true; };
template <> struct has_group<NNGP_SYS_DBL_PEND> { static constexpr bool value = true; };

template <int SYS, int ORDER, bool LINSPACE, bool NORM, bool TRAJ>
__global__ void __launch_bounds__(64) rk_group_kernel(LaneArgs args, int n_slices,
                                                     const double *__restrict__ t0,
                                                     const double *__restrict__ t1, int64_t steps,
                                                     int64_t gsteps_, const int64_t *__restrict__ j0s,
                                                     const double *__restrict__ u0,
                                                     double *__restrict__ uF) {
    const int64_t gsteps = TRAJ ? steps : gsteps_;   // TRAJ: gsteps_ is `every`
    using T = Tableau<ORDER>;
    constexpr int S = T::S;
    constexpr int D = LaneSys<SYS>::D;
    static_assert(D <= (GroupSys<SYS>::G == 16 ? 4 : 3), "group kernel: one DPP bank (G=16) or lane (G=4) per component");
    constexpr int G = GroupSys<SYS>::G;
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = tid / G, c = (G == 16) ? (tid % 16) >> 2 : tid % G;   // component of this lane
    if (i >= n_slices) return;   // group-uniform: the DPP partners of a live lane are live
    const bool own = c < D;
    const bool writer = own && (G != 16 || (tid & 3) == 0);
    const double one = 1.0;
    typename GroupState<GroupSys<SYS>>::T gst = GroupState<GroupSys<SYS>>::init(c);
    double mn = 0, hw = 0, sc = 0;
    if constexpr (NORM) {
        if (own) {
            mn = args.norm[c];
            hw = 0.5 * args.norm[D + c];
            sc = args.norm[2 * D + c];
        }
    }
    double u = own ? u0[(size_t)i * D + c] : 0.0, k[S];
    const double T0 = t0[i], T1 = t1[i];
    const double dt = (T1 - T0) / (double)(LINSPACE ? gsteps : steps);
    const int64_t j0 = (!TRAJ && j0s) ? j0s[i] : 0;
    LinGrid grid;
    if constexpr (LINSPACE) grid.init(j0, gsteps, T0, dt);
    // TRAJ: the writer lanes store their component of row 0 now and of every sample as it falls due
    TrajOut tr;
    if constexpr (TRAJ) {
        double *base = traj_block(uF, i, steps, gsteps_, D);
        tr.init(base, steps, gsteps_, D);
        if (writer) base[c] = u;
    }
    auto sample = [&]() __attribute__((always_inline)) {
        if constexpr (TRAJ) {
            if (tr.due()) {
                double *row = tr.take();
                if (writer) row[c] = u;
            }
        }
    };
    // The tableau is folded (nngp_rk_dev.h, fold_*): k[j] holds k'_j = (a_j h) o_j, the one multiply
    // h o_j costs, and the stage inputs and the update take the rescaled coefficients (RK4:
    // u + k'0, u + k'1, u + k2 and (1/3) k'0 + (2/3) k'1 + (1/3) k2 + (1/6) k3).  (Exact build
    // only: the contracted build keeps stage_input and step_update, FOLD_TABLEAU in nngp_rk_dev.h.)
    // UNROLL steps per iteration and a remainder loop: the step is one wave's instruction issue with
    // no other wave on the SIMD to cover the loop's taken branch.  Sixteen
    // for the tableaux of up to four stages (RK4: about 10 KB of loop body, inside the instruction
    // cache); RK8's eleven stay at two (code size).
    constexpr int UNROLL = S <= 4 ? 16 : 2;
    // The time track (group_tracks above): fixed-step mode only, where the constant component's k
    // are the same at every step.  (Linspace mode has another h at every step and keeps the form
    // below, as do the tableaux and the systems the track is not built for.)
    constexpr bool TRACK = !LINSPACE && FOLD_TABLEAU && group_tracks<GroupSys<SYS>, T>::value;
    if constexpr (TRACK) {
        using GS = GroupSys<SYS>;
        constexpr int TC = GS::TC;
        static_assert(G == 16 && UNROLL % TRACK_STEPS == 0 && TC < D, "four lanes per step of a pass");
        // Component TC's constants in every lane, and its k, INC and offsets from the step's own
        // expressions: o = 1 * sc, k'_s = fold_h(s) * o, INC = their sum in fold_step_update's
        // order, and the offsets a*RN(dt*o), the values the reference forms.
        double mn2 = 0, hw2 = 0, o2 = one;
        if constexpr (NORM) {
            mn2 = args.norm[TC];
            hw2 = 0.5 * args.norm[D + TC];
            o2 = one * args.norm[2 * D + TC];
        }
        double kk[S];
#pragma unroll
        for (int s = 0; s < S; s++) kk[s] = fold_h<T>(s, dt) * o2;
        double inc = fold_step_sum<T>(kk);
        const double kc = dt * o2;
        const int r = tid & 3;   // the lane's role; its step of the pass is c
        double offr = r == 1 ? group_batch_coef<T>(0) * kc : r == 2 ? group_batch_coef<T>(1) * kc : -0.0;
        double m1 = c >= 1 ? inc : -0.0, m2 = c >= 2 ? inc : -0.0, m3 = c >= 3 ? inc : -0.0;
        // opaque from here on, so that every add of a per-lane constant stays one add: x + (-0.0) -> x
        // is a legal fold that would move the add into the select
        asm("" : "+v"(offr), "+v"(inc), "+v"(m1), "+v"(m2), "+v"(m3));
        // tu: lane 4j + r holds u2 at step j of the pass, spread by the sequential roundings lane
        // 4 TC performs on u
        double tu = ((bcast<TC>(u) + m1) + m2) + m3;
        // the pass's quotients from tu; tu advances by one of the pass's TRACK_STEPS steps
        auto quot = [&]() __attribute__((always_inline)) {
            double x = tu + offr;
            if constexpr (NORM) x = (x + 1) * hw2 + mn2;
            return GS::track_div(x, tu, inc, args);
        };
        auto advance = [&]() __attribute__((always_inline)) {
#pragma unroll
            for (int j = 1; j < TRACK_STEPS; j++) tu = tu + inc;
        };
        // step J of the pass whose quotients qt holds
        auto step = [&](auto J, double qt) __attribute__((always_inline)) {
#pragma unroll
            for (int s = 0; s < S; s++) {
                const double tmp = fold_stage_input<T>(s, u, k);
                double o;
                if constexpr (NORM)
                    o = group_f_track<SYS, T, decltype(J)::value>(s, (tmp + 1) * hw + mn, gst, qt) * sc;
                else o = group_f_track<SYS, T, decltype(J)::value>(s, tmp, gst, qt);
                k[s] = fold_h<T>(s, dt) * o;
            }
            u = fold_step_update<T>(u, k);
            sample();
        };
        // One pass: the next pass's quotients are formed while this one's are used (they read
        // nothing the steps write), so qt is always ready, for the remainder too.
        double qt = quot();
        advance();
        GS::track_settle(gst);
        // Inside a pass the second stage of its first steps is the doubly fused take stage
        // (GroupSys<HOPF>::f_take2), which carries two instructions of the next pass's division
        // each (pair K, from tu0 = the track at the start of the pass): three such stages in
        // normalised coordinates, one in identity coordinates, as many as leave the track enough
        // free instructions for the wait states behind the stage-0 statements.
        typename GS::Tk tk{0.0, 0.0, 0.0};
        auto step2 = [&](auto J, auto K, double qt, double tu0) __attribute__((always_inline)) {
            constexpr int j = decltype(J)::value, kf = decltype(K)::value;
            static_assert(group_batch_slot<T>(1) == 0, "stage 1 takes lane 4 j + 1");
#pragma unroll
            for (int s = 0; s < S; s++) {
                const double tmp = fold_stage_input<T>(s, u, k);
                double x = tmp;
                if constexpr (NORM) x = (tmp + 1) * hw + mn;
                double o;
                if (s == 1) o = GS::template f_take2<4 * j + 1, kf>(x, gst, qt, tk, tu0, offr, hw2, mn2, args);
                else o = group_f_track<SYS, T, j>(s, x, gst, qt);
                if constexpr (NORM) o = o * sc;
                k[s] = fold_h<T>(s, dt) * o;
            }
            u = fold_step_update<T>(u, k);
            sample();
        };
        auto pass = [&]() __attribute__((always_inline)) {
            const double tu0 = tu;
            if constexpr (NORM) {
                step2(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{}, qt, tu0);
                step2(std::integral_constant<int, 1>{}, std::integral_constant<int, 2>{}, qt, tu0);
                step2(std::integral_constant<int, 2>{}, std::integral_constant<int, 3>{}, qt, tu0);
            } else {
                step2(std::integral_constant<int, 0>{}, std::integral_constant<int, 4>{}, qt, tu0);
                tk.e = fma(-tk.q, args.param[0], tk.x);
                step(std::integral_constant<int, 1>{}, qt);
                step(std::integral_constant<int, 2>{}, qt);
            }
            const double next = GS::track_fin(tk, tu, inc, args);
            advance();
            step(std::integral_constant<int, 3>{}, qt);
            qt = next;
        };
        static_assert(TRACK_STEPS == 4, "pass: four steps");
        // (the long loop ends on n != full, a scalar compare: n + UNROLL - 1 < steps is a 64-bit
        // signed one, which gfx950 has as a VALU op only)
        const int64_t full = steps > 0 ? steps - steps % UNROLL : 0;
        int64_t n = 0;
        if constexpr (NORM && !TRAJ) {
            // The long loop in normalised coordinates: each pass is one asm statement in an order
            // of its own (GroupSys<HOPF>::pass_asm), fifteen of its sixteen stages doubly fused.
            // The quotients alternate between two registers, so a pass writes the one the next
            // reads without a copy; an iteration holds an even number of passes and ends on qt.
            static_assert(S == 4 && (UNROLL / TRACK_STEPS) % 2 == 0, "pass_asm: RK4, passes in pairs");
            typename GS::PassC pc{hw, mn, sc,
                                  {fold_h<T>(0, dt), fold_h<T>(1, dt), fold_h<T>(2, dt), fold_h<T>(3, dt)},
                                  {fold_b<T>(0), fold_b<T>(1), fold_b<T>(2), fold_b<T>(3)},
                                  inc, offr, hw2, mn2, args.rparam0, args.param[0]};
            // the wave-uniform ones in VGPRs once, in front of the loop: left to itself the
            // compiler moves them there from their SGPRs again in every iteration
            asm("" : "+v"(pc.b[0]), "+v"(pc.b[1]), "+v"(pc.b[2]), "+v"(pc.b[3]), "+v"(pc.hw2), "+v"(pc.mn2),
                     "+v"(pc.r), "+v"(pc.mu));
            double qo;
            for (; n != full; n += UNROLL) {
#pragma unroll
                for (int j = 0; j < UNROLL / TRACK_STEPS / 2; j++) {
                    GS::pass_asm(u, gst, qt, qo, tu, pc);
                    GS::pass_asm(u, gst, qo, qt, tu, pc);
                }
            }
        } else {
            for (; n != full; n += UNROLL) {
#pragma unroll
                for (int j = 0; j < UNROLL / TRACK_STEPS; j++) pass();
            }
        }
#pragma unroll 1
        for (; n + (TRACK_STEPS - 1) < steps; n += TRACK_STEPS) pass();
        if (n < steps) step(std::integral_constant<int, 0>{}, qt);
        if (n + 1 < steps) step(std::integral_constant<int, 1>{}, qt);
        if (n + 2 < steps) step(std::integral_constant<int, 2>{}, qt);
    } else {
        auto step = [&](int64_t n) __attribute__((always_inline)) {
            const double h = LINSPACE ? grid.next(n, T0, T1, dt) : dt;
#pragma unroll
            for (int s = 0; s < S; s++) {
                double tmp;
                if constexpr (FOLD_TABLEAU) tmp = fold_stage_input<T>(s, u, k);
                else tmp = stage_input<T, 1>(s, u, k, 0);
                double o;
                if constexpr (NORM) o = group_f<SYS, T>(s, (tmp + 1) * hw + mn, gst, one, args) * sc;
                else o = group_f<SYS, T>(s, tmp, gst, one, args);
                if constexpr (FOLD_TABLEAU) k[s] = fold_h<T>(s, h) * o;
                else k[s] = h * o;
            }
            if constexpr (FOLD_TABLEAU) u = fold_step_update<T>(u, k);
            else u = step_update<T, 1>(u, k, 0);
        };
        int64_t n = 0;
        for (; n + (UNROLL - 1) < steps; n += UNROLL) {
#pragma unroll
            for (int j = 0; j < UNROLL; j++) {
                step(n + j);
                sample();
            }
        }
#pragma unroll 1
        for (; n < steps; n++) {
            step(n);
            sample();
        }
    }
    if constexpr (TRAJ) {
        if (writer) tr.last[c] = u;
    } else {
        if (writer) uF[(size_t)i * D + c] = u;
    }
}

// ---------------------------------------------------------------------------------------------
// PDE right-hand sides (Burgers, FHN-PDE), one workgroup = one slice
// ---------------------------------------------------------------------------------------------

// Burgers row i: (Dxx@u)_i - u_i (Dx@u)_i with non-zeros summed in ascending column order
// (systems.py:421-446)
__device__ __forceinline__ double burgers_elem(const double *__restrict__ V, int i, int d,
                                               const FieldArgs &fa) {
    const double cxx = fa.c_off, cdg = fa.c_diag, q = fa.c_grad;
    double lap, grad;
    if (i == 0) {
        lap = (cdg * V[0] + cxx * V[1]) + cxx * V[d - 1];
        grad = q * V[1] + (-q) * V[d - 1];
    } else if (i == d - 1) {
        lap = (cxx * V[0] + cxx * V[d - 2]) + cdg * V[d - 1];
        grad = q * V[0] + (-q) * V[d - 2];
    } else {
        lap = (cxx * V[i - 1] + cdg * V[i]) + cxx * V[i + 1];
        grad = (-q) * V[i - 1] + q * V[i + 1];
    }
    return lap - V[i] * grad;
}

// 5-point periodic neighbourhood of grid point p = y*nx + x with its columns in ascending order
// and a flag for the diagonal slot; precomputed once per element (a 9-comparator sorting
// network on named registers -- no runtime-indexed arrays, so nothing spills to scratch).
struct Nbr5 {
    int c0, c1, c2, c3, c4;
    bool d0, d1, d2, d3, d4;
};

__device__ __forceinline__ void cswap(int &a, bool &fa, int &b, bool &fb) {
    if (a > b) {
        const int t = a; a = b; b = t;
        const bool u = fa; fa = fb; fb = u;
    }
}

__device__ inline Nbr5 fhn_neighbours(int nx, int p) {
    const int y = p / nx, x = p - y * nx;
    const int ym = (y == 0) ? nx - 1 : y - 1, yp = (y == nx - 1) ? 0 : y + 1;
    const int xm = (x == 0) ? nx - 1 : x - 1, xp = (x == nx - 1) ? 0 : x + 1;
    Nbr5 r{ym * nx + x, y * nx + xm, p, y * nx + xp, yp * nx + x, false, false, true, false, false};
    // optimal 5-input sorting network
    cswap(r.c0, r.d0, r.c1, r.d1); cswap(r.c3, r.d3, r.c4, r.d4);
    cswap(r.c2, r.d2, r.c4, r.d4); cswap(r.c2, r.d2, r.c3, r.d3);
    cswap(r.c0, r.d0, r.c3, r.d3); cswap(r.c0, r.d0, r.c2, r.d2);
    cswap(r.c1, r.d1, r.c4, r.d4); cswap(r.c1, r.d1, r.c3, r.d3);
    cswap(r.c1, r.d1, r.c2, r.d2);
    return r;
}

// ((a L)@v)_p with the 5 terms in ascending column order (systems.py:365-366: `a*(DXX+DYY)@u1`
// multiplies the matrix by a first)
__device__ __forceinline__ double fhn_lap(const double *__restrict__ V, const Nbr5 &nb, double off,
                                          double diag) {
    double s = (nb.d0 ? diag : off) * V[nb.c0];
    s = s + (nb.d1 ? diag : off) * V[nb.c1];
    s = s + (nb.d2 ? diag : off) * V[nb.c2];
    s = s + (nb.d3 ? diag : off) * V[nb.c3];
    s = s + (nb.d4 ? diag : off) * V[nb.c4];
    return s;
}

// DiffReact (systems.py:463-577): zero-flux 5-point Laplacian of grid point p = y*nx + x.  The
// reference stores it as DIA with offsets [0, -1, 1, -nx, nx] (systems.py:528-530) and scipy's
// DIA product adds the diagonals in that order, so row p is
//     main_p w[p] + cx w[p-1] + cx w[p+1] + cy w[p-nx] + cy w[p+nx]
// summed left to right, a neighbour across a wall giving no term.  Here a wall neighbour is the
// point itself with coefficient 0.0: adding 0.0*w[p] changes at most the sign of an exact zero
// (scipy does the same for the in-row wraps, whose stored entries are 0), and every lane runs the
// same five products.  Chosen once per point, before the step loop: the four neighbour indices,
// the four "has a neighbour" flags and the main-diagonal entry (one of four values).
struct DrNbr {
    int l, r, dn, up;       // p-1, p+1, p-nx, p+nx, or p at a wall
    bool hl, hr, hd, hu;
    double main;
};

__device__ __forceinline__ DrNbr dr_neighbours(const FieldArgs &fa, int p, bool live) {
    const int nx = fa.nx;
    const int y = p / nx, x = p - y * nx;
    DrNbr n;
    n.hl = live && x > 0;
    n.hr = live && x < nx - 1;
    n.hd = live && y > 0;
    n.hu = live && y < nx - 1;
    n.l = n.hl ? p - 1 : p;
    n.r = n.hr ? p + 1 : p;
    n.dn = n.hd ? p - nx : p;
    n.up = n.hu ? p + nx : p;
    const bool ex = !(n.hl && n.hr), ey = !(n.hd && n.hu);   // first/last of its row / column
    n.main = ex ? (ey ? fa.r_m11 : fa.r_m12) : (ey ? fa.r_m21 : fa.r_m22);
    return n;
}

// (lap @ w)_p from the point's own value and its four neighbours', in the DIA order
__device__ __forceinline__ double dr_lap(double c, double wl, double wr, double wd, double wu, double main,
                                         double kl, double kr, double kd, double ku) {
    double s = main * c;
    s = s + kl * wl;
    s = s + kr * wr;
    s = s + kd * wd;
    s = s + ku * wu;
    return s;
}

// systems.py:558-563 (u**3 = u*(u*u)): u_t = (((u - u^3) - k) - v) + Du*lap(u)
__device__ __forceinline__ double dr_fu(double u, double v, double lap, const FieldArgs &fa) {
    return (((u - u * (u * u)) - fa.r_k) - v) + fa.r_du * lap;
}
// v_t = (u - v) + Dv*lap(v)
__device__ __forceinline__ double dr_fv(double u, double v, double lap, const FieldArgs &fa) {
    return (u - v) + fa.r_dv * lap;
}

// element e of the state u | v from the image V[d] (rk_field_kernel, rhs_field_kernel); nb is the
// stencil of its grid point (e, or e - d/2 for a v element)
__device__ __forceinline__ double dr_elem(const double *__restrict__ V, int e, int half, const DrNbr &nb,
                                          const FieldArgs &fa) {
    const bool isv = e >= half;
    const double *W = V + (isv ? half : 0);
    const int p = isv ? e - half : e;
    const double lap = dr_lap(W[p], W[nb.l], W[nb.r], W[nb.dn], W[nb.up], nb.main, nb.hl ? fa.r_cx : 0.0,
                              nb.hr ? fa.r_cx : 0.0, nb.hd ? fa.r_cy : 0.0, nb.hu ? fa.r_cy : 0.0);
    return isv ? dr_fv(V[p], V[e], lap, fa) : dr_fu(V[e], V[half + e], lap, fa);
}

// Polynomial field (NNGP_SYS_POLY): row e of the table from the image V, its terms
// b .. en-1 walked in list order from device memory -- one 16-byte record, one global_load_dwordx4,
// per term (wave-divergent where the rows of a wave differ in length; the table of every slice is
// the same, so it stays in cache).  coef times the factors left to right, the first term, then
// acc + term; no terms: +0.0.  The indices were checked when the table was registered.
__device__ __forceinline__ double poly_elem(const double *__restrict__ V, int b, int en,
                                            const PolyTerm *__restrict__ terms) {
    double acc = 0.0;
    for (int t = b; t < en; t++) {
        const PolyTerm T = terms[t];
        double v = T.coef;
        if (T.i >= 0) v = v * V[T.i];
        if (T.j >= 0) v = v * V[T.j];
        if (T.k >= 0) v = v * V[T.k];
        acc = (t == b) ? v : acc + v;
    }
    return acc;
}

// the kinds whose rows are a term table in device memory (FieldArgs::p_row / p_terms)
__host__ __device__ constexpr bool table_sys(int sys) { return sys == NNGP_SYS_POLY || sys == NNGP_SYS_FUNC; }

// doubles per stage image: the state, and for NNGP_SYS_FUNC the atoms behind it
template <int SYS>
__host__ __device__ __forceinline__ int image_doubles(const FieldArgs &fa) {
    if constexpr (SYS == NNGP_SYS_FUNC) return fa.d + fa.nx;   // nx: the number of atoms
    else return fa.d;
}

// Field with atoms (NNGP_SYS_FUNC): once the state part V[0 .. d) of the image is
// written and the stage's barrier passed, thread t evaluates atoms t, t + BT, ... from it into the
// image's tail V[d + q]; behind a second barrier poly_elem walks the rows over the extended image.
// Atoms read the state part only, so the two parts never race; the double buffering argument of
// rk_field_kernel holds for the tail as for the state (the tail written in stage s was last read
// before the second barrier of stage s - 1 ... of the other image: two barriers earlier at least).
__device__ __forceinline__ void func_atoms_stage(double *__restrict__ V, const FieldArgs &fa,
                                                 const nngp_func_atom *__restrict__ atoms, int tid, int BT) {
    for (int q = tid; q < fa.nx; q += BT) V[fa.d + q] = func_atom_value(atoms[q], V);
    __syncthreads();
}

// <= 256 threads per slice leaves ~170 VGPRs for u, the S stage vectors and the neighbour table
template <int SYS, int ORDER, bool LINSPACE, int EPT, bool NORM, bool TRAJ>
__global__ void __launch_bounds__(EPT == 1 ? 1024 : (EPT == 2 ? 512 : 256)) rk_field_kernel(FieldArgs fa, int n_slices,
                                                        const double *__restrict__ t0,
                                                        const double *__restrict__ t1,
                                                        int64_t steps, int64_t gsteps_,
                                                        const int64_t *__restrict__ j0s,
                                                        const double *__restrict__ u0,
                                                        double *__restrict__ uF) {
    const int64_t gsteps = TRAJ ? steps : gsteps_;   // TRAJ: gsteps_ is `every`
    using T = Tableau<ORDER>;
    constexpr int S = T::S;
    extern __shared__ __attribute__((aligned(16))) double smem[];   // [2][d]
    const int slice = blockIdx.x;
    const int tid = threadIdx.x, BT = blockDim.x;
    const int d = fa.d;
    const int half = d / 2;   // FHN-PDE: u1 | u2

    double u[EPT], k[S * EPT], mn[EPT], w[EPT], sc[EPT];
    int e_[EPT];
    Nbr5 nb[(SYS == NNGP_SYS_FHN_PDE) ? EPT : 1];
    DrNbr rnb[(SYS == NNGP_SYS_DIFFREACT) ? EPT : 1];
    int pb[table_sys(SYS) ? EPT : 1], pe[table_sys(SYS) ? EPT : 1];   // the rows' term ranges
    const int W = image_doubles<SYS>(fa);
    const nngp_func_atom *fatoms = nullptr;
    if constexpr (SYS == NNGP_SYS_FUNC) fatoms = func_atoms_of(fa);
#pragma unroll
    for (int r = 0; r < EPT; r++) {
        const int e = tid + r * BT;
        e_[r] = e;
        const bool ok = e < d;
        if constexpr (table_sys(SYS)) {
            pb[r] = ok ? fa.p_row[e] : 0;
            pe[r] = ok ? fa.p_row[e + 1] : 0;
        }
        u[r] = ok ? u0[(size_t)slice * d + e] : 0.0;
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
    const double T0 = t0[slice], T1 = t1[slice];
    const double dt = (T1 - T0) / (double)(LINSPACE ? gsteps : steps);
    const int64_t j0 = (!TRAJ && j0s) ? j0s[slice] : 0;
    int buf = 0;
    LinGrid grid;
    if constexpr (LINSPACE) grid.init(j0, gsteps, T0, dt);
    // TRAJ: every thread stores the elements it holds (u lives in VGPRs: no barrier needed)
    TrajOut tr;
    auto store_row = [&](double *row) __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < EPT; r++)
            if (e_[r] < d) row[e_[r]] = u[r];
    };
    if constexpr (TRAJ) {
        double *base = traj_block(uF, slice, steps, gsteps_, d);
        tr.init(base, steps, gsteps_, d);
        store_row(base);
    }
    for (int64_t n = 0; n < steps; n++) {
        const double h = LINSPACE ? grid.next(n, T0, T1, dt) : dt;
#pragma unroll
        for (int s = 0; s < S; s++) {
            double *V = smem + buf * W;
#pragma unroll
            for (int r = 0; r < EPT; r++) {
                if (e_[r] < d) {
                    const double x = stage_input<T, EPT>(s, u[r], k, r);
                    V[e_[r]] = NORM ? (x + 1) * w[r] + mn[r] : x;
                }
            }
            __syncthreads();
            if constexpr (SYS == NNGP_SYS_FUNC) func_atoms_stage(V, fa, fatoms, tid, BT);
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
                k[s * EPT + r] = h * f;
            }
            buf ^= 1;
        }
#pragma unroll
        for (int r = 0; r < EPT; r++) u[r] = step_update<T, EPT>(u[r], k, r);   // RK.py:170
        if constexpr (TRAJ) {
            if (tr.due()) store_row(tr.take());
        }
    }
    if constexpr (TRAJ) {
        store_row(tr.last);
    } else {
#pragma unroll
        for (int r = 0; r < EPT; r++)
            if (e_[r] < d) uF[(size_t)slice * d + e_[r]] = u[r];
    }
}

// ---------------------------------------------------------------------------------------------
// FHN-PDE with one thread per grid point: thread p owns u[p] and v[p] (elements p and half + p)
// with all their stage values.  The reaction terms couple u and v at the SAME point and the
// Laplacian's centre is the point itself, so a stage reads from LDS only the two 5-point
// Laplacians (the own and partner values come from registers): 1 write + 10 reads per point
// instead of the element-per-thread kernel's 2 writes + 14 reads.  Same expressions, same order
// (systems.py:365-366) -- bitwise rk_field_kernel<FHN_PDE>.  d = 2 nx^2 <= 2048.
//
// LDS layout: FhnPairImages::N images of [point][u, v] (below), and a stage's image fixed at
// compile time (stage s of every step uses image s & 1, the last of an odd stage count image 2, so
// the image a stage writes was last read two barriers earlier).  Every LDS access of the step loop
// is then one of five per-thread neighbour addresses plus an immediate offset: no address
// arithmetic per stage.  Threads past the grid (the last wave's idle lanes) compute point 0's
// stencil on their own zeros and write their garbage to the images' padding, so the step loop has
// no branch either.
// ---------------------------------------------------------------------------------------------
template <int S> struct FhnPairImages {
    static constexpr int N = (S % 2 == 1 && S > 1) ? 3 : 2;
    // image of stage s (S == 1 alternates at run time)
    static constexpr int of(int s) { return (S % 2 == 1 && s == S - 1) ? 2 : (s & 1); }
};

// ((a L)@v)_p as fhn_lap, from the five neighbour values (ascending column order) and the five
// coefficients selected once per thread
__device__ __forceinline__ double fhn_sum5(const double (&v)[5], double k0, double k1, double k2, double k3,
                                           double k4) {
    double s = k0 * v[0];
    s = s + k1 * v[1];
    s = s + k2 * v[2];
    s = s + k3 * v[3];
    s = s + k4 * v[4];
    return s;
}

// Images interleaved [point][u, v], 16 bytes per point: a neighbour's u and v arrive by ONE
// ds_read_b128 (4 LDS-array cycles per wave-instruction, 256 B/clk) and a point's two stage inputs
// leave by one ds_write_b128.  Round 3's split [u | v] images needed a ds_read2st64_b64 (8 cycles,
// 128 B/clk) per neighbour; PMC at 512 slices (profiles/r04/pmc_fhn_pair_r4c.txt) had the CU's LDS
// ~70 % busy under it (66 LDS instructions per wave per RK8 step, 20 % of their cycles bank
// conflicts) beside a 64 % busy VALU.  Measured (profiles/r04/fhn_pair_il_r4d.txt), us per RK8
// step at d = 800: 512 slices 5.54 -> 4.91, 64 slices 3.53 -> 2.98; bitwise unchanged.  The image
// stride is the block size (points past the grid write their own padding slots).
template <int ORDER, bool LINSPACE, bool NORM, bool TRAJ>
__global__ void __launch_bounds__(1024) rk_fhn_pair_kernel(FieldArgs fa, int n_slices,
                                                           const double *__restrict__ t0,
                                                           const double *__restrict__ t1, int64_t steps,
                                                           int64_t gsteps_, const int64_t *__restrict__ j0s,
                                                           const double *__restrict__ u0,
                                                           double *__restrict__ uF) {
    const int64_t gsteps = TRAJ ? steps : gsteps_;   // TRAJ: gsteps_ is `every`
    using T = Tableau<ORDER>;
    using IM = FhnPairImages<T::S>;
    constexpr int S = T::S;
    extern __shared__ __attribute__((aligned(16))) double smem[];   // [IM::N][blockDim.x][2]
    const int slice = blockIdx.x;
    const int p = threadIdx.x;
    const int d = fa.d, half = d / 2;
    const bool ok = p < half;
    double u[2], k[S * 2], mn[2], w[2], sc[2];
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const int e = p + r * half;
        u[r] = ok ? u0[(size_t)slice * d + e] : 0.0;
        if (NORM && ok) {
            mn[r] = fa.norm[e];
            w[r] = 0.5 * fa.norm[d + e];   // (mx-mn)/2, see lane_rhs
            sc[r] = fa.norm[2 * d + e];
        } else {
            mn[r] = 0.0; w[r] = 1.0; sc[r] = 1.0;
        }
    }
    const Nbr5 nb = fhn_neighbours(fa.nx, ok ? p : 0);   // the same stencil for u and v
    const double ka0 = nb.d0 ? fa.a_diag : fa.a_off, ka1 = nb.d1 ? fa.a_diag : fa.a_off,
                 ka2 = nb.d2 ? fa.a_diag : fa.a_off, ka3 = nb.d3 ? fa.a_diag : fa.a_off,
                 ka4 = nb.d4 ? fa.a_diag : fa.a_off;
    const double kb0 = nb.d0 ? fa.b_diag : fa.b_off, kb1 = nb.d1 ? fa.b_diag : fa.b_off,
                 kb2 = nb.d2 ? fa.b_diag : fa.b_off, kb3 = nb.d3 ? fa.b_diag : fa.b_off,
                 kb4 = nb.d4 ? fa.b_diag : fa.b_off;
    const double T0 = t0[slice], T1 = t1[slice];
    const double dt = (T1 - T0) / (double)(LINSPACE ? gsteps : steps);
    const int64_t j0 = (!TRAJ && j0s) ? j0s[slice] : 0;
    LinGrid grid;
    if constexpr (LINSPACE) grid.init(j0, gsteps, T0, dt);
    // TRAJ: every live thread stores its point's u and v (registers: no barrier needed)
    TrajOut tr;
    auto store_row = [&](double *row) __attribute__((always_inline)) {
        if (ok) {
            row[p] = u[0];
            row[half + p] = u[1];
        }
    };
    if constexpr (TRAJ) {
        double *base = traj_block(uF, slice, steps, gsteps_, d);
        tr.init(base, steps, gsteps_, d);
        store_row(base);
    }
    // stage 0's input is u itself (RK.py:153-166: no a_0j terms)
    double xw[2];
#pragma unroll
    for (int r = 0; r < 2; r++) xw[r] = NORM ? (u[r] + 1) * w[r] + mn[r] : u[r];
    const int ISTR = 2 * (int)blockDim.x;   // doubles per image
    for (int64_t n = 0; n < steps; n++) {
        const double h = LINSPACE ? grid.next(n, T0, T1, dt) : dt;
        double acc[2];   // sum_s b_s k_s, accumulated as the stages finish (step_update's order)
#pragma unroll
        for (int s = 0; s < S; s++) {
            const int img = (S == 1) ? (int)(n & 1) : IM::of(s);
            double va[5], vb[5];
            double2 *V2 = reinterpret_cast<double2 *>(smem + img * ISTR);
            V2[p] = make_double2(xw[0], xw[1]);
            __syncthreads();
            const double2 w0 = V2[nb.c0], w1 = V2[nb.c1], w2 = V2[nb.c2], w3 = V2[nb.c3], w4 = V2[nb.c4];
            va[0] = w0.x; va[1] = w1.x; va[2] = w2.x; va[3] = w3.x; va[4] = w4.x;
            vb[0] = w0.y; vb[1] = w1.y; vb[2] = w2.y; vb[3] = w3.y; vb[4] = w4.y;
            // the next stage's input terms that do not involve this stage's k, computed while the
            // neighbour reads are in flight (pinned before the stencil: the reads' results pass
            // through the same empty asm, so LLVM can neither sink these sums past the stencil
            // nor start the stencil before them; profiles/r03: 47 % of a 64-slice step's wave
            // cycles were spent waiting, mostly on these reads and the barrier)
            double pn[2] = {0.0, 0.0};
            if (s + 1 < S) {
#pragma unroll
                for (int r = 0; r < 2; r++) pn[r] = stage_partial<T, 2>(s + 1, k, r);
            }
            // systems.py:365-366, as rk_field_kernel with V[e] / V[half+e] / V[e-half] in registers
            const double lu = fhn_sum5(va, ka0, ka1, ka2, ka3, ka4);
            const double u1 = xw[0], u1c = u1 * (u1 * u1);
            double fu = (((lu + u1) - u1c) - xw[1]) + -5E-3 * 1.0;
            const double lv = fhn_sum5(vb, kb0, kb1, kb2, kb3, kb4);
            double fv = (1 / 0.1) * ((lv + xw[0]) - xw[1]);
            if (NORM) {
                fu = fu * sc[0];
                fv = fv * sc[1];
            }
            k[s * 2 + 0] = h * fu;
            k[s * 2 + 1] = h * fv;
#pragma unroll
            for (int r = 0; r < 2; r++) {
                step_accumulate<T>(s, acc[r], k[s * 2 + r]);   // RK.py:170, in its order
                if (s + 1 < S) {
                    const double x = stage_finish<T, 2>(s + 1, u[r], pn[r], k, r);
                    xw[r] = NORM ? (x + 1) * w[r] + mn[r] : x;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 2; r++) {
            u[r] = u[r] + acc[r];   // RK.py:170
            xw[r] = NORM ? (u[r] + 1) * w[r] + mn[r] : u[r];
        }
        if constexpr (TRAJ) {
            if (tr.due()) store_row(tr.take());
        }
    }
    if constexpr (TRAJ) {
        store_row(tr.last);
    } else {
        if (ok) {
            uF[(size_t)slice * d + p] = u[0];
            uF[(size_t)slice * d + half + p] = u[1];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// DiffReact with one thread per grid point, as rk_fhn_pair_kernel: thread p owns u[p] and v[p] with
// all their stage values, the images are interleaved [point][u, v] with FhnPairImages' stage
// schedule, and a stage is one 128-bit LDS write, one barrier and FOUR 128-bit reads (the centre
// comes from registers).  The stencil does not wrap, so there is no column order to sort: the
// four neighbour slots are p-1, p+1, p-nx, p+nx, and at a wall the thread's own slot with
// coefficient 0.0 (dr_neighbours) -- both chosen once per thread, so the step loop has no branch.
// Threads past the grid are "all walls": they read and write only their own slot p < blockDim.x,
// which lies in the images' padding (the image stride is the block size), never a live point.
// Same expressions in the same order as dr_elem -- bitwise rk_field_kernel<DIFFREACT>.
// nx <= 32: at most 1024 points = the launch bound; LDS 16 B * blockDim.x * 3 images <= 48 KiB.
// ---------------------------------------------------------------------------------------------
template <int ORDER, bool LINSPACE, bool NORM, bool TRAJ>
__global__ void __launch_bounds__(1024) rk_dr_pair_kernel(FieldArgs fa, int n_slices,
                                                          const double *__restrict__ t0,
                                                          const double *__restrict__ t1, int64_t steps,
                                                          int64_t gsteps_, const int64_t *__restrict__ j0s,
                                                          const double *__restrict__ u0,
                                                          double *__restrict__ uF) {
    const int64_t gsteps = TRAJ ? steps : gsteps_;   // TRAJ: gsteps_ is `every`
    using T = Tableau<ORDER>;
    using IM = FhnPairImages<T::S>;
    constexpr int S = T::S;
    extern __shared__ __attribute__((aligned(16))) double smem[];   // [IM::N][blockDim.x][2]
    const int slice = blockIdx.x;
    const int p = threadIdx.x;
    const int d = fa.d, half = d / 2;
    const bool ok = p < half;
    double u[2], k[S * 2], mn[2], w[2], sc[2];
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const int e = p + r * half;
        u[r] = ok ? u0[(size_t)slice * d + e] : 0.0;
        if (NORM && ok) {
            mn[r] = fa.norm[e];
            w[r] = 0.5 * fa.norm[d + e];   // (mx-mn)/2, see lane_rhs
            sc[r] = fa.norm[2 * d + e];
        } else {
            mn[r] = 0.0; w[r] = 1.0; sc[r] = 1.0;
        }
    }
    const DrNbr nb = dr_neighbours(fa, p, ok);   // the same stencil for u and v
    const double kl = nb.hl ? fa.r_cx : 0.0, kr = nb.hr ? fa.r_cx : 0.0, kd = nb.hd ? fa.r_cy : 0.0,
                 ku = nb.hu ? fa.r_cy : 0.0, km = nb.main;
    const double T0 = t0[slice], T1 = t1[slice];
    const double dt = (T1 - T0) / (double)(LINSPACE ? gsteps : steps);
    const int64_t j0 = (!TRAJ && j0s) ? j0s[slice] : 0;
    LinGrid grid;
    if constexpr (LINSPACE) grid.init(j0, gsteps, T0, dt);
    // TRAJ: every live thread stores its point's u and v (registers: no barrier needed)
    TrajOut tr;
    auto store_row = [&](double *row) __attribute__((always_inline)) {
        if (ok) {
            row[p] = u[0];
            row[half + p] = u[1];
        }
    };
    if constexpr (TRAJ) {
        double *base = traj_block(uF, slice, steps, gsteps_, d);
        tr.init(base, steps, gsteps_, d);
        store_row(base);
    }
    // stage 0's input is u itself (RK.py:153-166: no a_0j terms)
    double xw[2];
#pragma unroll
    for (int r = 0; r < 2; r++) xw[r] = NORM ? (u[r] + 1) * w[r] + mn[r] : u[r];
    const int ISTR = 2 * (int)blockDim.x;   // doubles per image
    for (int64_t n = 0; n < steps; n++) {
        const double h = LINSPACE ? grid.next(n, T0, T1, dt) : dt;
        double acc[2];   // sum_s b_s k_s, accumulated as the stages finish (step_update's order)
#pragma unroll
        for (int s = 0; s < S; s++) {
            const int img = (S == 1) ? (int)(n & 1) : IM::of(s);
            double2 *V2 = reinterpret_cast<double2 *>(smem + img * ISTR);
            V2[p] = make_double2(xw[0], xw[1]);
            __syncthreads();
            const double2 wl = V2[nb.l], wr = V2[nb.r], wd = V2[nb.dn], wu = V2[nb.up];
            // the next stage's input terms that do not involve this stage's k (as rk_fhn_pair_kernel)
            double pn[2] = {0.0, 0.0};
            if (s + 1 < S) {
#pragma unroll
                for (int r = 0; r < 2; r++) pn[r] = stage_partial<T, 2>(s + 1, k, r);
            }
            const double lu = dr_lap(xw[0], wl.x, wr.x, wd.x, wu.x, km, kl, kr, kd, ku);
            const double lv = dr_lap(xw[1], wl.y, wr.y, wd.y, wu.y, km, kl, kr, kd, ku);
            double fu = dr_fu(xw[0], xw[1], lu, fa);
            double fv = dr_fv(xw[0], xw[1], lv, fa);
            if (NORM) {
                fu = fu * sc[0];
                fv = fv * sc[1];
            }
            k[s * 2 + 0] = h * fu;
            k[s * 2 + 1] = h * fv;
#pragma unroll
            for (int r = 0; r < 2; r++) {
                step_accumulate<T>(s, acc[r], k[s * 2 + r]);   // RK.py:170, in its order
                if (s + 1 < S) {
                    const double x = stage_finish<T, 2>(s + 1, u[r], pn[r], k, r);
                    xw[r] = NORM ? (x + 1) * w[r] + mn[r] : x;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 2; r++) {
            u[r] = u[r] + acc[r];   // RK.py:170
            xw[r] = NORM ? (u[r] + 1) * w[r] + mn[r] : u[r];
        }
        if constexpr (TRAJ) {
            if (tr.due()) store_row(tr.take());
        }
    }
    if constexpr (TRAJ) {
        store_row(tr.last);
    } else {
        if (ok) {
            uF[(size_t)slice * d + p] = u[0];
            uF[(size_t)slice * d + half + p] = u[1];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Burgers with d = 64*EPT: ONE WAVE per slice, no LDS, no barriers.
// Lane l owns the contiguous elements l*EPT .. l*EPT+EPT-1; the periodic stencil's outer
// neighbours come from lanes l-1 / l+1 by `wave_ror:1` / `wave_rol:1` DPP moves, which wrap around
// the wave exactly like the periodic boundary wraps around the grid.  The general kernel above
// pays an LDS round trip and a workgroup barrier per stage instead (11 per RK8 step).
// Summation order = burgers_elem (systems.py:421-446, non-zeros in ascending column order): the
// three Laplacian terms of rows 0 and d-1 associate differently from the interior rows, so the
// operands are selected per element; the two gradient terms commute (a+b == b+a bitwise).
// ---------------------------------------------------------------------------------------------

template <int ORDER, bool LINSPACE, int EPT, bool NORM, bool TRAJ>
__global__ void __launch_bounds__(64) rk_burgers_wave_kernel(FieldArgs fa, int n_slices,
                                                              const double *__restrict__ t0,
                                                              const double *__restrict__ t1,
                                                              int64_t steps, int64_t gsteps,
                                                              const int64_t *__restrict__ j0s,
                                                              const double *__restrict__ u0,
                                                              double *__restrict__ uF) {
    constexpr int d = 64 * EPT;
    const int slice = blockIdx.x;
    if constexpr (TRAJ)   // gsteps is `every`
        burgers_wave_slice<ORDER, LINSPACE, EPT, NORM, true>(fa, threadIdx.x, t0[slice], t1[slice], steps, steps, 0,
                                                             u0 + (size_t)slice * d,
                                                             traj_block(uF, slice, steps, gsteps, d), gsteps);
    else
        burgers_wave_slice<ORDER, LINSPACE, EPT, NORM>(fa, threadIdx.x, t0[slice], t1[slice], steps, gsteps,
                                                       j0s ? j0s[slice] : 0, u0 + (size_t)slice * d,
                                                       uF + (size_t)slice * d);
}
// ---------------------------------------------------------------------------------------------
// host dispatch
// ---------------------------------------------------------------------------------------------
template <int SYS, int ORDER, bool LIN, bool TRAJ>
static int launch_lane(const nngp_system *sys, int n, const double *t0, const double *t1,
                       int64_t steps, int64_t gsteps, const int64_t *j0, const double *u0, double *uF,
                       hipStream_t st) {
    LaneArgs a{};
    constexpr int D = LaneSys<SYS>::D;
    NNGP_REQUIRE(sys->d == D, "system kind %d has d=%d, got d=%d", SYS, D, sys->d);
    a.normalized = sys->normalized;
    for (int c = 0; c < 4; c++) a.param[c] = sys->param[c];
    a.rparam0 = 1.0 / sys->param[0];
    a.norm = sys->norm;
    NNGP_REQUIRE(!sys->normalized || sys->norm != nullptr, "normalized system needs norm[3d]");
    const int bs = 64;
    if constexpr (has_group<SYS>::value) {
        // group kernel while all slices' lane groups fit one wave per SIMD (G*n <= 64 * 1024): there
        // the step time is one wave's issue and the group form issues fewer instructions per step;
        // beyond it waves share SIMDs and the lane kernel's G-fold fewer waves win.
        // NNGP_RK_GROUP=0 forces the lane kernel (A/B tool, tests).
        const char *ge = getenv("NNGP_RK_GROUP");
        const int group_on = ge ? atoi(ge) : 1;
        constexpr int G = GroupSys<SYS>::G;
        if (group_on && (int64_t)n * G <= 64 * 1024) {
            const int nb = (int)(((int64_t)G * n + bs - 1) / bs);
            if (sys->normalized)
                hipLaunchKernelGGL((rk_group_kernel<SYS, ORDER, LIN, true, TRAJ>), dim3(nb), dim3(bs), 0, st,
                                   a, n, t0, t1, steps, gsteps, j0, u0, uF);
            else
                hipLaunchKernelGGL((rk_group_kernel<SYS, ORDER, LIN, false, TRAJ>), dim3(nb), dim3(bs), 0, st,
                                   a, n, t0, t1, steps, gsteps, j0, u0, uF);
            NNGP_LAUNCH_CHECK();
            return NNGP_OK;
        }
    }
    if (sys->normalized)
        hipLaunchKernelGGL((rk_lane_kernel<SYS, ORDER, LIN, true, TRAJ>), dim3((n + bs - 1) / bs), dim3(bs), 0, st,
                           a, n, t0, t1, steps, gsteps, j0, u0, uF);
    else
        hipLaunchKernelGGL((rk_lane_kernel<SYS, ORDER, LIN, false, TRAJ>), dim3((n + bs - 1) / bs), dim3(bs), 0,
                           st, a, n, t0, t1, steps, gsteps, j0, u0, uF);
    NNGP_LAUNCH_CHECK();
    return NNGP_OK;
}

template <int SYS, int ORDER, bool LIN, int EPT, bool TRAJ>
static int launch_field_ept(const FieldArgs &fa, int bt, int n, const double *t0,
                            const double *t1, int64_t steps, int64_t gsteps, const int64_t *j0,
                            const double *u0, double *uF, hipStream_t st) {
    const size_t lds = sizeof(double) * 2 * (size_t)image_doubles<SYS>(fa);
    if (fa.normalized)
        hipLaunchKernelGGL((rk_field_kernel<SYS, ORDER, LIN, EPT, true, TRAJ>), dim3(n), dim3(bt), lds, st, fa, n,
                           t0, t1, steps, gsteps, j0, u0, uF);
    else
        hipLaunchKernelGGL((rk_field_kernel<SYS, ORDER, LIN, EPT, false, TRAJ>), dim3(n), dim3(bt), lds, st, fa, n,
                           t0, t1, steps, gsteps, j0, u0, uF);
    NNGP_LAUNCH_CHECK();
    return NNGP_OK;
}

// threads per slice: env NNGP_RK_THREADS overrides (tuning), else the fewest whole waves that
// keep EPT <= 4 (d=128 -> 64 threads x 2, d=800 -> 256 threads x 4)
static int pick_threads(int d, int n_slices) {
    const char *env = getenv("NNGP_RK_THREADS");
    if (env) {
        int v = atoi(env);
        if (v >= 64 && v <= 1024 && v % 64 == 0) return v;
    }
    int bt = 64;
    while (bt < 256 && (d + bt - 1) / bt > 4) bt += 64;
    // up to 1024 elements: one element per thread while all slices' waves fit ~4 per SIMD (few
    // slices: the per-step latency is the stage chain, FHN-PDE d=800 at 64 slices 5.2 -> 4.0
    // us/step), else <= 2 per thread in 512 threads (512 slices: 8.6 -> 6.7 us/step)
    if ((d + bt - 1) / bt > 2 && d <= 1024) {
        const int64_t waves1 = (int64_t)n_slices * ((d + 63) / 64);
        bt = (waves1 <= 4 * 1024) ? ((d + 63) / 64) * 64 : 512;
    }
    return bt;
}

static int field_args(const nngp_system *sys, FieldArgs &fa) {
    fa = FieldArgs{};
    fa.d = sys->d;
    fa.nx = sys->nx;
    fa.normalized = sys->normalized;
    fa.norm = sys->norm;
    int n_atoms = 0;   // of a table; behind the state in the stage image
    NNGP_REQUIRE(!sys->normalized || sys->norm, "normalized system needs norm[3d]");
    if (sys->kind == NNGP_SYS_BURGERS) {
        NNGP_REQUIRE(sys->nx == sys->d && sys->d >= 3, "Burgers needs nx == d >= 3");
        const double dx = (1.0 - (-1.0)) / (sys->d - 1);
        const double nu = sys->param[0];
        fa.c_off = nu / (dx * dx);   // (nu/dx**2)*Txx
        fa.c_diag = fa.c_off * -2.0;
        fa.c_grad = 1 / (2 * dx);    // (1/(2*dx))*Tx
    } else if (sys->kind == NNGP_SYS_DIFFREACT) {
        // one workgroup per slice, at most one thread per grid point: 32 x 32 points is the launch
        // bound (d <= 2048, the FHN-PDE paths' ceiling)
        NNGP_REQUIRE(sys->nx >= 3 && sys->nx <= 32, "DiffReact needs 3 <= nx <= 32 (got nx=%d): larger grids "
                     "need a multi-workgroup propagator", sys->nx);
        NNGP_REQUIRE(sys->d == 2 * sys->nx * sys->nx, "DiffReact needs d = 2 nx^2 (got d=%d, nx=%d)", sys->d,
                     sys->nx);
        // systems.py:496-522, in double exactly as the Python expressions (dx**2 = dx*dx)
        const double dx = (1.0 - (-1.0)) / sys->nx, dy = (1.0 - (-1.0)) / sys->nx;
        const double dx2 = dx * dx, dy2 = dy * dy;
        fa.r_cx = 1.0 / dx2;
        fa.r_cy = 1.0 / dy2;
        fa.r_m22 = -2.0 / dx2 - 2.0 / dy2;
        fa.r_m12 = -1.0 / dx2 - 2.0 / dy2;   // first/last point of a row
        fa.r_m21 = -2.0 / dx2 - 1.0 / dy2;   // first/last row
        fa.r_m11 = -1.0 / dx2 - 1.0 / dy2;   // corners
        fa.r_du = sys->param[0];
        fa.r_dv = sys->param[1];
        fa.r_k = sys->param[2];
    } else if (table_sys(sys->kind)) {
        // the handle and d are checked on the host first; only then the device copy (uploaded on
        // this device's first use).  The atoms lie behind the terms in the same block: func_atoms_of
        int rc = table_device(sys, &fa.p_row, &fa.p_terms, &n_atoms);
        if (rc) return rc;
        // the kernels of NNGP_SYS_FUNC read the number of atoms here; those of NNGP_SYS_POLY read
        // nothing, and their argument block keeps the handle it has always carried
        if (sys->kind == NNGP_SYS_FUNC) fa.nx = n_atoms;
    } else {
        NNGP_REQUIRE(sys->nx >= 3 && sys->d == 2 * sys->nx * sys->nx, "FHN_PDE needs d = 2 nx^2, nx >= 3");
        const double dx = (1.0 - (-1.0)) / (sys->nx - 1);
        const double c1 = 1 / (dx * dx);
        const double ldiag = c1 * -2.0 + c1 * -2.0;   // (DXX + DYY) diagonal
        fa.a_off = 2.8E-4 * c1;
        fa.a_diag = 2.8E-4 * ldiag;
        fa.b_off = 5E-3 * c1;
        fa.b_diag = 5E-3 * ldiag;
    }
    NNGP_REQUIRE(sizeof(double) * 2 * ((size_t)sys->d + n_atoms) <= 160 * 1024, "LDS image too large");
    return NNGP_OK;
}

template <int ORDER, bool LIN, int EPT, bool TRAJ>
static int launch_burgers_wave(const FieldArgs &fa, int n, const double *t0, const double *t1, int64_t steps,
                               int64_t gsteps, const int64_t *j0, const double *u0, double *uF, hipStream_t st) {
    if (fa.normalized)
        hipLaunchKernelGGL((rk_burgers_wave_kernel<ORDER, LIN, EPT, true, TRAJ>), dim3(n), dim3(64), 0, st, fa, n, t0,
                           t1, steps, gsteps, j0, u0, uF);
    else
        hipLaunchKernelGGL((rk_burgers_wave_kernel<ORDER, LIN, EPT, false, TRAJ>), dim3(n), dim3(64), 0, st, fa, n, t0,
                           t1, steps, gsteps, j0, u0, uF);
    NNGP_LAUNCH_CHECK();
    return NNGP_OK;
}

template <int SYS, int ORDER, bool LIN, bool TRAJ>
static int launch_field(const nngp_system *sys, int n, const double *t0, const double *t1,
                        int64_t steps, int64_t gsteps, const int64_t *j0, const double *u0, double *uF,
                        hipStream_t st) {
    FieldArgs fa;
    int rc = field_args(sys, fa);
    if (rc) return rc;
    if (SYS == NNGP_SYS_BURGERS && sys->d % 64 == 0 && sys->d <= 256 && !getenv("NNGP_BURGERS_LDS")) {
        const int e = sys->d / 64;
        if (e == 1) return launch_burgers_wave<ORDER, LIN, 1, TRAJ>(fa, n, t0, t1, steps, gsteps, j0, u0, uF, st);
        if (e == 2) return launch_burgers_wave<ORDER, LIN, 2, TRAJ>(fa, n, t0, t1, steps, gsteps, j0, u0, uF, st);
        if (e == 3) return launch_burgers_wave<ORDER, LIN, 3, TRAJ>(fa, n, t0, t1, steps, gsteps, j0, u0, uF, st);
        return launch_burgers_wave<ORDER, LIN, 4, TRAJ>(fa, n, t0, t1, steps, gsteps, j0, u0, uF, st);
    }
    // FHN-PDE from 16x16 grid points: one thread per point (u and v of the point) unless
    // NNGP_FHN_PAIR=0 or a thread count is forced.  Measured (tools/contract_probe.py): d = 800 at
    // 512 slices 7.50 -> 6.75 us/step, at 64 slices unchanged; d = 200 (100 points: 28 of 128
    // lanes idle) 3.65 -> 4.25, so small grids keep the element kernel's 64 threads x 4
    if (SYS == NNGP_SYS_FHN_PDE && sys->d / 2 >= 256 && sys->d / 2 <= 1024 && !getenv("NNGP_RK_THREADS")) {
        const char *pe = getenv("NNGP_FHN_PAIR");
        if (!pe || atoi(pe) != 0) {
            const int bt = ((sys->d / 2 + 63) / 64) * 64;
            const size_t lds = sizeof(double) * 2 * bt * FhnPairImages<Tableau<ORDER>::S>::N;
            if (fa.normalized)
                hipLaunchKernelGGL((rk_fhn_pair_kernel<ORDER, LIN, true, TRAJ>), dim3(n), dim3(bt), lds, st, fa, n, t0, t1,
                                   steps, gsteps, j0, u0, uF);
            else
                hipLaunchKernelGGL((rk_fhn_pair_kernel<ORDER, LIN, false, TRAJ>), dim3(n), dim3(bt), lds, st, fa, n, t0, t1,
                                   steps, gsteps, j0, u0, uF);
            NNGP_LAUNCH_CHECK();
            return NNGP_OK;
        }
    }
    // DiffReact from 16x16 grid points (nx 16..32): one thread per point, as FHN-PDE above; a forced
    // thread count (NNGP_RK_THREADS) selects the element kernel
    if (SYS == NNGP_SYS_DIFFREACT && sys->d / 2 >= 256 && sys->d / 2 <= 1024 && !getenv("NNGP_RK_THREADS")) {
        const int bt = ((sys->d / 2 + 63) / 64) * 64;
        const size_t lds = sizeof(double) * 2 * bt * FhnPairImages<Tableau<ORDER>::S>::N;
        if (fa.normalized)
            hipLaunchKernelGGL((rk_dr_pair_kernel<ORDER, LIN, true, TRAJ>), dim3(n), dim3(bt), lds, st, fa, n, t0, t1,
                               steps, gsteps, j0, u0, uF);
        else
            hipLaunchKernelGGL((rk_dr_pair_kernel<ORDER, LIN, false, TRAJ>), dim3(n), dim3(bt), lds, st, fa, n, t0, t1,
                               steps, gsteps, j0, u0, uF);
        NNGP_LAUNCH_CHECK();
        return NNGP_OK;
    }
    const int bt = pick_threads(sys->d, n);
    const int ept = (sys->d + bt - 1) / bt;
    NNGP_REQUIRE(ept <= 8, "d=%d with %d threads per slice exceeds the field kernel's 8 elements per thread",
                 sys->d, bt);
    // each EPT variant is compiled for at most 1024 / 512 / 256 / 256 threads (launch bounds): a
    // larger block (only reachable through NNGP_RK_THREADS) would fail to launch
    const int bound = ept <= 1 ? 1024 : (ept <= 2 ? 512 : 256);
    NNGP_REQUIRE(bt <= bound, "%d threads per slice exceed the field kernel's bound %d at %d elements per thread "
                 "(d=%d)", bt, bound, ept <= 2 ? ept : (ept <= 4 ? 4 : 8), sys->d);
    if (ept <= 1) return launch_field_ept<SYS, ORDER, LIN, 1, TRAJ>(fa, bt, n, t0, t1, steps, gsteps, j0, u0, uF, st);
    if (ept <= 2) return launch_field_ept<SYS, ORDER, LIN, 2, TRAJ>(fa, bt, n, t0, t1, steps, gsteps, j0, u0, uF, st);
    if (ept <= 4) return launch_field_ept<SYS, ORDER, LIN, 4, TRAJ>(fa, bt, n, t0, t1, steps, gsteps, j0, u0, uF, st);
    return launch_field_ept<SYS, ORDER, LIN, 8, TRAJ>(fa, bt, n, t0, t1, steps, gsteps, j0, u0, uF, st);
}

// The lane form of the table-backed kinds (NNGP_SYS_POLY, NNGP_SYS_FUNC): the table by value in the
// kernel arguments, built here from the registered one.
// the descriptors of the terms, the same bits in PolyLaneTab and FuncLaneTab (nngp_rk_dev.h; the
// indices of a table with atoms reach 7 and take the third bit its layout leaves them)
static void lane_terms(const Table &tb, double *coef, uint16_t *desc) {
    for (int c = 0; c < tb.d; c++)
        for (int t = tb.row_ptr[c]; t < tb.row_ptr[c + 1]; t++) {
            const PolyTerm &T = tb.terms[t];
            const unsigned p = (T.i >= 0) + (T.j >= 0) + (T.k >= 0);
            coef[t] = T.coef;
            desc[t] = (uint16_t)(p | (unsigned)(T.i >= 0 ? T.i : 0) << 2 | (unsigned)(T.j >= 0 ? T.j : 0) << 5 |
                                 (unsigned)(T.k >= 0 ? T.k : 0) << 8 | (unsigned)c << 11 |
                                 (unsigned)(t == tb.row_ptr[c]) << 13 | (unsigned)(t + 1 == tb.row_ptr[c + 1]) << 14);
        }
}
static void lane_tab(const Table &tb, PolyLaneTab &tab) {
    tab = PolyLaneTab{};
    tab.n = tb.n_terms;
    lane_terms(tb, tab.coef, tab.desc);
}
static void lane_tab(const Table &tb, FuncLaneTab &tab) {
    tab = FuncLaneTab{};
    tab.n = tb.n_terms;
    tab.n_atoms = tb.n_atoms;
    for (int q = 0; q < tb.n_atoms; q++) {
        const nngp_func_atom &A = tb.atoms[q];
        tab.a[q] = A.a;
        tab.c[q] = A.c;
        tab.b[q] = A.b;
        tab.adesc[q] = (uint16_t)((unsigned)A.fn | (unsigned)A.i << 3 | (unsigned)(A.j >= 0 ? A.j : 0) << 5 |
                                  (unsigned)(A.j >= 0) << 7 | (unsigned)(A.has_b != 0) << 8);
    }
    lane_terms(tb, tab.coef, tab.desc);
}
// whether a table takes the lane form: d <= 4, at most 16 terms and at most 4 atoms (so d + n_atoms
// <= 8 slots and 3-bit indices; a polynomial table has none); anything larger takes the field form
// (one workgroup per slice, the table in device memory)
static bool lane_fits(const Table &tb) {
    return tb.d <= POLY_LANE_D && tb.n_atoms <= FUNC_LANE_ATOMS && tb.n_terms <= POLY_LANE_TERMS;
}
// what KIND (NNGP_SYS_POLY or NNGP_SYS_FUNC) selects: the argument type and the kernel
template <int KIND> using TableLaneArgs = std::conditional_t<KIND == NNGP_SYS_POLY, PolyLaneArgs, FuncLaneArgs>;
template <int KIND, int D, int ORDER, bool LIN, bool NORM, bool TRAJ>
static auto table_lane_kernel() {
    if constexpr (KIND == NNGP_SYS_POLY) return &rk_poly_lane_kernel<D, ORDER, LIN, NORM, TRAJ>;
    else return &rk_func_lane_kernel<D, ORDER, LIN, NORM, TRAJ>;
}

template <int KIND, int D, int ORDER, bool LIN, bool TRAJ>
static int launch_table_lane(const nngp_system *sys, const Table &tb, int n, const double *t0, const double *t1,
                             int64_t steps, int64_t gsteps, const int64_t *j0, const double *u0, double *uF,
                             hipStream_t st) {
    TableLaneArgs<KIND> a{};
    a.normalized = sys->normalized;
    a.norm = sys->norm;
    lane_tab(tb, a.tab);
    const int bs = 64;
    if (sys->normalized)
        hipLaunchKernelGGL((table_lane_kernel<KIND, D, ORDER, LIN, true, TRAJ>()), dim3((n + bs - 1) / bs), dim3(bs), 0,
                           st, a, n, t0, t1, steps, gsteps, j0, u0, uF);
    else
        hipLaunchKernelGGL((table_lane_kernel<KIND, D, ORDER, LIN, false, TRAJ>()), dim3((n + bs - 1) / bs), dim3(bs), 0,
                           st, a, n, t0, t1, steps, gsteps, j0, u0, uF);
    NNGP_LAUNCH_CHECK();
    return NNGP_OK;
}

// NNGP_SYS_POLY / NNGP_SYS_FUNC: the lane form while the table fits the kernel arguments, else the
// field form
template <int KIND, int ORDER, bool LIN, bool TRAJ>
static int launch_table(const nngp_system *sys, int n, const double *t0, const double *t1, int64_t steps,
                        int64_t gsteps, const int64_t *j0, const double *u0, double *uF, hipStream_t st) {
    Table tb;
    int rc = table_lookup(sys, &tb);   // host checks, before any HIP call
    if (rc) return rc;
    NNGP_REQUIRE(!sys->normalized || sys->norm != nullptr, "normalized system needs norm[3d]");
    if (!lane_fits(tb)) return launch_field<KIND, ORDER, LIN, TRAJ>(sys, n, t0, t1, steps, gsteps, j0, u0, uF, st);
    switch (tb.d) {
    case 1: return launch_table_lane<KIND, 1, ORDER, LIN, TRAJ>(sys, tb, n, t0, t1, steps, gsteps, j0, u0, uF, st);
    case 2: return launch_table_lane<KIND, 2, ORDER, LIN, TRAJ>(sys, tb, n, t0, t1, steps, gsteps, j0, u0, uF, st);
    case 3: return launch_table_lane<KIND, 3, ORDER, LIN, TRAJ>(sys, tb, n, t0, t1, steps, gsteps, j0, u0, uF, st);
    default: return launch_table_lane<KIND, 4, ORDER, LIN, TRAJ>(sys, tb, n, t0, t1, steps, gsteps, j0, u0, uF, st);
    }
}

template <int ORDER, bool LIN, bool TRAJ>
static int dispatch_sys(const nngp_system *s, int n, const double *t0, const double *t1,
                        int64_t steps, int64_t gsteps, const int64_t *j0, const double *u0,
                        double *uF, hipStream_t st) {
    switch (s->kind) {
    case NNGP_SYS_LORENZ: return launch_lane<NNGP_SYS_LORENZ, ORDER, LIN, TRAJ>(s, n, t0, t1, steps, gsteps, j0, u0, uF, st);
    case NNGP_SYS_HOPF: return launch_lane<NNGP_SYS_HOPF, ORDER, LIN, TRAJ>(s, n, t0, t1, steps, gsteps, j0, u0, uF, st);
    case NNGP_SYS_THOMAS_LABYRINTH:
        return launch_lane<NNGP_SYS_THOMAS_LABYRINTH, ORDER, LIN, TRAJ>(s, n, t0, t1, steps, gsteps, j0, u0, uF, st);
    case NNGP_SYS_FHN_ODE: return launch_lane<NNGP_SYS_FHN_ODE, ORDER, LIN, TRAJ>(s, n, t0, t1, steps, gsteps, j0, u0, uF, st);
    case NNGP_SYS_ROSSLER: return launch_lane<NNGP_SYS_ROSSLER, ORDER, LIN, TRAJ>(s, n, t0, t1, steps, gsteps, j0, u0, uF, st);
    case NNGP_SYS_BRUSSELATOR:
        return launch_lane<NNGP_SYS_BRUSSELATOR, ORDER, LIN, TRAJ>(s, n, t0, t1, steps, gsteps, j0, u0, uF, st);
    case NNGP_SYS_DBL_PEND: return launch_lane<NNGP_SYS_DBL_PEND, ORDER, LIN, TRAJ>(s, n, t0, t1, steps, gsteps, j0, u0, uF, st);
    case NNGP_SYS_BURGERS: return launch_field<NNGP_SYS_BURGERS, ORDER, LIN, TRAJ>(s, n, t0, t1, steps, gsteps, j0, u0, uF, st);
    case NNGP_SYS_FHN_PDE: return launch_field<NNGP_SYS_FHN_PDE, ORDER, LIN, TRAJ>(s, n, t0, t1, steps, gsteps, j0, u0, uF, st);
    case NNGP_SYS_DIFFREACT:
        return launch_field<NNGP_SYS_DIFFREACT, ORDER, LIN, TRAJ>(s, n, t0, t1, steps, gsteps, j0, u0, uF, st);
    case NNGP_SYS_POLY: return launch_table<NNGP_SYS_POLY, ORDER, LIN, TRAJ>(s, n, t0, t1, steps, gsteps, j0, u0, uF, st);
    case NNGP_SYS_FUNC: return launch_table<NNGP_SYS_FUNC, ORDER, LIN, TRAJ>(s, n, t0, t1, steps, gsteps, j0, u0, uF, st);
    default: set_error("unknown system kind %d", s->kind); return NNGP_E_ARG;
    }
}

template <bool LIN, bool TRAJ>
static int dispatch_tab(const nngp_system *s, int tab, int n, const double *t0, const double *t1,
                        int64_t steps, int64_t gsteps, const int64_t *j0, const double *u0,
                        double *uF, hipStream_t st) {
    switch (tab) {
    case NNGP_RK1: return dispatch_sys<1, LIN, TRAJ>(s, n, t0, t1, steps, gsteps, j0, u0, uF, st);
    case NNGP_RK2: return dispatch_sys<2, LIN, TRAJ>(s, n, t0, t1, steps, gsteps, j0, u0, uF, st);
    case NNGP_RK4: return dispatch_sys<4, LIN, TRAJ>(s, n, t0, t1, steps, gsteps, j0, u0, uF, st);
    case NNGP_RK8: return dispatch_sys<8, LIN, TRAJ>(s, n, t0, t1, steps, gsteps, j0, u0, uF, st);
    default: set_error("unknown tableau %d (RK1/2/4/8)", tab); return NNGP_E_ARG;
    }
}
