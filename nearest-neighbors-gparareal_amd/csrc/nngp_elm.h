// nngp_elm.h -- the constants of the ELM arithmetic contract, restated in
// tests/elm_ref.py.
#pragma once

namespace nngp {

// A Gram-Schmidt row is kept iff |r|^2 > NNGP_ELM_TAU * |z|^2 (r: z after the projections).
// Below 2^-52 on the squared norm the reference's Gram arithmetic (cond^2) has no correct bit; the
// value is that raised by factors of 2^4 until the Lorenz N = 32 and FHN-ODE N = 40 runs converge no
// later than classic Parareal to within 10 eps of the serial fine solution: a
// neighbour whose part outside the span of the nearer ones is under 1/16 of its length is dropped.
constexpr double NNGP_ELM_TAU = 0x1p-8;

constexpr int ELM_CHUNK = 1024;    // features per partial sum: 16 per lane of one wave
constexpr int ELM_ROW_TILE = 4;    // rows that share one read of a chunk of C
constexpr int ELM_MAX_M = 16;      // neighbours
constexpr int ELM_MAX_RES = 1024;  // hidden units
constexpr int ELM_MAX_D = 8192;    // a row tile of x in LDS: ELM_ROW_TILE * d doubles <= 64 KB at d <= 2048,
                                   // one row per tile past that

}  // namespace nngp
