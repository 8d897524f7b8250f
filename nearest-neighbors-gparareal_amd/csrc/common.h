// common.h -- shared host/device helpers of libnngp_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../include/nngp.h"

namespace nngp {

// integer tuning/test knob from the environment (read on every call: tests toggle them in-process)
inline int env_int(const char *name, int dflt) {
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}

// attributes of the CURRENT device (hipGetDevice), cached per device: compute units, and the
// rate of the 100 MHz wall clock the kernels read (wall_clock64) in kHz
int device_cus();
double device_wallclock_khz();

// thread-local last error, returned by nngp_last_error()
void set_error(const char *fmt, ...);

#define NNGP_HIP_CHECK(expr)                                                                 \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            ::nngp::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),         \
                              __FILE__, __LINE__);                                           \
            return NNGP_E_HIP;                                                               \
        }                                                                                    \
    } while (0)

#define NNGP_REQUIRE(cond, ...)                                                              \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            ::nngp::set_error(__VA_ARGS__);                                                  \
            return NNGP_E_ARG;                                                               \
        }                                                                                    \
    } while (0)

// launch-error check right after a <<<>>> launch
#define NNGP_LAUNCH_CHECK()                                                                  \
    do {                                                                                     \
        hipError_t _e = hipGetLastError();                                                   \
        if (_e != hipSuccess) {                                                              \
            ::nngp::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(_e),     \
                              __FILE__, __LINE__);                                           \
            return NNGP_E_HIP;                                                               \
        }                                                                                    \
    } while (0)

// Grow-only device scratch owned by the library (per device and slot), so that steady-state
// calls never allocate.  Slot 0: per-call scratch (nngp_knn / nngp_predict / ...); slot 1: the
// speculative sweep's batch buffers, which must outlive the per-slice calls.  Growing a slot
// frees the old buffer after hipFree's implicit device synchronisation.  Not thread-safe across
// host threads sharing a device.
constexpr int N_WS_SLOTS = 15;   // slot 2: the sweep's speculation buffers; 3: full-GP factors; 4: fit queues; 5: parked fits;
                                // 6: the re-speculation window's batch (slot 1 may still be read by an overlapped batch);
                                // 7 / 8: the fit queues of the overlapped batch / of the re-speculation window;
                                // 9: the sharded sweep's zeros (nngp_comm.hip);
                                // 10 / 11: the ELM prediction's scratch / nngp_elm_hidden's partial sums (nngp_elm.hip)
                                // 12 / 13: nngp_predict_batch's and nngp_predict_listed's chunk workspace / fit queues
                                // 14: nngp_listed_sweep's prepared coordinates, lists and kd2 (live through the sweep)
constexpr int WS_PREDICT_BATCH = 12, WS_PREDICT_BATCH_QUEUE = 13, WS_LISTED_SWEEP = 14;
void *workspace(size_t bytes, int *err, int slot = 0);

// Table-backed vector fields: the library's registry of term tables (nngp_table.hip).
// Polynomial fields (NNGP_SYS_POLY): d rows of ordered terms, one 16-byte record per
// term -- coef and the state indices of its up to three factors in multiplication order, -1 = no
// factor (only after the real ones).
struct alignas(16) PolyTerm {
    double coef;
    int16_t i, j, k, pad;
};
constexpr int POLY_MAX_D = 2048;             // one workgroup per slice, as every field kernel
constexpr int POLY_MAX_TERMS = 1 << 20;
constexpr int POLY_LANE_D = 4;               // lane form: d <= 4 and at most 16 terms in total
constexpr int POLY_LANE_TERMS = 16;
// Fields with elementary-function atoms (NNGP_SYS_FUNC): the same term records, their
// indices over the extended vector [u_0 .. u_{d-1}, atom_0 .. atom_{n_atoms-1}], and n_atoms records
// of nngp_func_atom (include/nngp.h), which the kernels read as they were registered.  A polynomial
// table is one with n_atoms = 0.
constexpr int FUNC_MAX_ATOMS = 2048;         // with d <= 2048: a stage image [2][d + n_atoms] of 64 KB
constexpr int FUNC_LANE_ATOMS = 4;           // lane form: d <= 4, at most 4 atoms and 16 terms
struct Table {                 // a registered table of either kind as the host holds it
    int d, n_atoms, n_terms;
    const int32_t *row_ptr;         // HOST [d+1]
    const PolyTerm *terms;          // HOST [n_terms]
    const nngp_func_atom *atoms;    // HOST [n_atoms]
};
// the table of sys->nx (a handle of nngp_poly_create or nngp_func_create, by sys->kind: the two
// handle spaces are separate) after checking it against sys->d: NNGP_E_ARG for an unknown or
// destroyed handle or another d.  Makes no HIP call.
int table_lookup(const nngp_system *sys, Table *out);
// the CURRENT device's copy of that table after the same checks, uploaded on first use and kept
// until the handle is destroyed or nngp_shutdown (so steady-state calls never allocate): one block
// terms | atoms | row_ptr, the atoms found from the other two (func_atoms_of, nngp_rk_dev.h)
int table_device(const nngp_system *sys, const int32_t **row_ptr, const PolyTerm **terms, int *n_atoms);
void table_release();   // nngp_shutdown's part: every table of both kinds, host and device

// A prepared coordinate of gp_pre_kernel: alpha rows 0..maxm-1 | c | psy | ok
__host__ __device__ constexpr int HM_STRIDE(int maxm) { return maxm + 3; }

// The sweep's split prediction (nngp_sweep.hip): a select whose ordered list hits a speculative
// prediction that gp_pre_kernel has already prepared (done[0] == target) finishes the slice's
// posterior mean itself -- from the prepared coordinates and the query's kd2, gp_mean_finish --
// and reports hit + 2 to the host, which then launches no mean kernel for the slice.
struct HitMean {
    const double *AP1, *AP2;          // the slice's prepared coordinates for hit 1 / hit 2 (or null)
    const int32_t *done1, *done2;     // their gp_pre workgroup counters (the slice's entry)
    int target;                       // gp_pre workgroups per prediction
    int maxm;                         // the padded fit size the coordinates were prepared at
    const double *bias;               // UG1[i+1]
    double *out, *preds;              // U1[i+1] = mean + bias, preds = mean
    // profiling (NNGP_SEL_PROF=1, any select of predict_impl): wall-clock sums, relative to each
    // launch's start, at the select's marks (rounds | merges | gathers | D2) and its end, + launches
    uint64_t *marks;
};
// the select-profile buffer (uint64_t[6]) when NNGP_SEL_PROF=1, else null; sel_prof_report prints
// and clears it (the correction sweep, at its end)
uint64_t *sel_prof_marks();
void sel_prof_report(const char *what);

// ---- the correction sweeps' argument bundles (plain aggregates; passed by const reference) ----
struct Coarse {     // the coarse propagator G and its time grid: slice i runs t[i] -> t[i+1]
    const nngp_system *sys; int tableau, step_mode; int64_t steps; const double *t;
    int run(int i, const double *u, double *ug, hipStream_t st) const {   // ug = G(t[i], t[i+1], u)
        return nngp_rk_batch(sys, tableau, step_mode, 1, t + i, t + i + 1, steps, u, ug, st);
    }
};
struct TrainSet {   // the training set: X[rows][d] -> Y[rows][d]
    const double *X, *Y; int64_t rows; int d;
};
struct FitSet {     // the Nelder-Mead fit settings of one prediction
    int m, n_jitter; const double *jitter_exp_host; int n_restarts; double fatol, xatol; int maxfev;
    int64_t n_fits(int d) const { return (int64_t)d * n_jitter * n_restarts; }
};
// The speculative references a prediction may be given (all null: no speculation): the ordered
// neighbour list a speculative batch assumed for this query, that batch's fits and the device hit
// flag; the same of the re-speculation window (hit 2); the host-mapped copy of the hit code; and the
// completion counter (and error word) of a batch whose fits may still be running.
struct SpecRefs {
    const int32_t *spec_idx; const double *spec_fits; int32_t *hit_flag;
    const int32_t *spec2_idx; const double *spec2_fits; int32_t *host_flag;
    const int32_t *wait_done; int32_t *wait_err;
};
struct PredOut {    // a prediction's outputs: preds = mean, out = mean + bias (or null), every fit (or null)
    double *preds; const double *bias; double *out, *fits_out;
};

// ---- workspace layouts: pure functions of sizes and a base pointer (no HIP call).  A null base is
// the sizing pass: every pointer null, .bytes what workspace() is asked for.
struct Carver {
    char *base;
    size_t off = 0;
    template <class T> T *take(size_t n) {
        T *p = base ? (T *)(base + off) : nullptr;
        off += sizeof(T) * n;
        return p;
    }
};
// slot 0, one prediction: what the kNN, the select, the fits and the mean hand to each other (also the
// fused chain's select and gdist): dist[rows] | D2[m*m] | kd2[m] | ymT[d*m] | idx[64] | fits[n_fits][4]
struct PredWs {
    double *dist, *D2, *kd2, *ymT; int32_t *idx; double *fits; size_t bytes;
};
inline PredWs pred_ws_carve(char *base, int64_t rows, int d, int m, int64_t n_fits) {
    Carver c{base};   // (a braced list is evaluated in order)
    PredWs w{c.take<double>((size_t)rows), c.take<double>((size_t)m * m), c.take<double>((size_t)m),
             c.take<double>((size_t)d * m), c.take<int32_t>(64), c.take<double>(4 * (size_t)n_fits), 0};
    w.bytes = c.off;
    return w;
}
// slot 2, the speculative sweep (nq slices, window W, hst HitMean doubles per slice or 0):
//   Qg[nq][d] | gtmp[d] | spec_fits[nq][n_fits][4] | W > 0: Qr[W][d] | gtmp2[d] | spec2_fits[nq][n_fits][4]
//   | spec_idx[nq][m] | flags[nq] | done[nq] | W > 0: spec2_idx[nq][m]
//   | hst > 0, 8-byte aligned: AP1[nq][hst] | AP2[nq][hst] | pre1[nq] | pre2[nq]
struct SpecWs {
    double *Qg, *gtmp, *spec_fits, *Qr, *gtmp2, *spec2_fits;
    int32_t *spec_idx, *flags, *done, *spec2_idx;
    double *AP1, *AP2; int32_t *pre1, *pre2; size_t bytes;
};
inline SpecWs spec_ws_carve(char *base, int64_t nq, int d, int m, int64_t n_fits, int W, size_t hst) {
    Carver c{base};
    SpecWs w{};
    const size_t q = (size_t)nq, fits = q * (size_t)n_fits * 4;
    w.Qg = c.take<double>(q * d);
    w.gtmp = c.take<double>((size_t)d);
    w.spec_fits = c.take<double>(fits);
    if (W > 0) {
        w.Qr = c.take<double>((size_t)W * d);
        w.gtmp2 = c.take<double>((size_t)d);
        w.spec2_fits = c.take<double>(fits);
    }
    w.spec_idx = c.take<int32_t>(q * m);
    w.flags = c.take<int32_t>(q);
    w.done = c.take<int32_t>(q);
    if (W > 0) w.spec2_idx = c.take<int32_t>(q * m);
    if (hst > 0) {
        const size_t pad = ((c.off + 7) & ~(size_t)7) - c.off;
        c.off += pad;
        w.AP1 = c.take<double>(q * hst);
        w.AP2 = c.take<double>(q * hst);
        w.pre1 = c.take<int32_t>(q);
        w.pre2 = c.take<int32_t>(q);
        c.off += sizeof(double) - pad;   // a whole double is reserved for the alignment step
    }
    w.bytes = c.off;
    return w;
}

// predict_impl's launches in parts (the speculative sweep issues the select, reads its hit flag on
// the host, and then launches the fits only on a miss): all | kNN + select | fits + mean | mean only
enum { PREDICT_ALL = 0, PREDICT_SELECT = 1, PREDICT_FITS_MEAN = 2, PREDICT_MEAN = 3, PREDICT_SELECT_ONLY = 4 };
// the slice head G(U1[i]) + the query's distances as one launch (gdist_kernel): PREDICT_SELECT_ONLY
// then launches the select alone.  gdist_supported: systems with an in-kernel G (NNGP_GDIST=0: off)
bool gdist_supported(const nngp_system *sys, int g_step_mode);
bool g_side_supported(const nngp_system *sys, int g_step_mode);
int gdist(const Coarse &G, int i, const TrainSet &T, const FitSet &F, const double *ui, double *ug_next,
          hipStream_t st);
// one prediction at new_x with its theta0 draws; coordinates [c0, c1) (c1 < 0: d)
int predict_impl(const TrainSet &T, const FitSet &F, const double *new_x, const double *theta0, const PredOut &O,
                 const SpecRefs &S, hipStream_t st, int c0 = 0, int c1 = -1, int phase = PREDICT_ALL,
                 const HitMean *hm = nullptr, hipEvent_t bias_ready = nullptr);
int gpfull_mean(const double *X, int64_t rows, int d, const double *q, const double *coef, const double *alpha,
                const double *bias, double *out, hipStream_t st);
// bo: the queries are independent predictions to finish here (nngp_predict_batch) -- the select also
// writes each query's kd2, and one more launch gives every (query, coordinate) arg-min and mean;
// idx_out / fits_out may then be null (the slot's workspace holds them)
struct BatchOut {   // [nq][d] each: preds = mean, out = mean + bias (both or neither; out may alias bias)
    double *preds; const double *bias; double *out;
};
int spec_batch(const TrainSet &T, const FitSet &F, const double *Q, int nq, const double *theta0, int32_t *idx_out,
               double *fits_out, bool latency, hipStream_t st, int slot = 1, int32_t *done = nullptr,
               hipEvent_t ev_select = nullptr, double *pre_AP = nullptr, int32_t *pre_done = nullptr,
               const BatchOut *bo = nullptr);
// gp_pre_kernel's workgroups per prediction (the HitMean target) for d coordinates at fit size m
int pre_target(int d, int m);
int pre_maxm(int m);   // the padded fit size of m
// the fused correction chain (nngp_gp.hip): one persistent kernel per run of hit slices
void chain_release();   // nngp_shutdown's parts (nngp_gp.hip / nngp_sweep.hip / nngp_comm.hip)
void sweep_release();
void comm_release();
// The G time of a sweep (g_ms_out) without host synchronisation in the loop: event pairs around the
// G launch of every stride-th slice, summed and scaled to all slices once the sweep has drained.
// Each event record costs the host ~3 us on a chain whose hit slices are host-bound
// (profiles/r05/sweep/), hence the stride (NNGP_G_TIME_EVERY, default 8; 1 = every slice).
inline int g_time_stride() {
    const int e = env_int("NNGP_G_TIME_EVERY", 8);
    return e > 1 ? e : 1;
}
struct GTimer {
    hipEvent_t *ev = nullptr; float *out = nullptr; int64_t slices = 0; int stride = 1;
    // *g_ms_out = 0; no events for a null g_ms_out or an empty (or negative) slice count
    int begin(float *g_ms_out, int64_t n_slices, int every);
    bool timed(size_t j) const { return ev && j % (size_t)stride == 0; }
    // G of slice i (the sweep's j-th): u -> ug on st, inside its event pair when the slice is timed
    int launch(const Coarse &G, int i, size_t j, const double *u, double *ug, hipStream_t st) const {
        if (!timed(j)) return G.run(i, u, ug, st);
        NNGP_HIP_CHECK(hipEventRecord(ev[2 * j], st));
        const int rc = G.run(i, u, ug, st);
        if (rc) return rc;
        NNGP_HIP_CHECK(hipEventRecord(ev[2 * j + 1], st));
        return NNGP_OK;
    }
    void drop() { ev = nullptr; }   // the time comes from elsewhere (the fused chain's clock)
    // waits for the last timed pair; *g_ms_out = the pairs' sum, scaled by slices / timed slices
    int finish() const;
};
bool chain_supported(const nngp_system *sys, int g_step_mode, int m);
bool guess_chain_supported(const nngp_system *sys, int g_step_mode);
int guess_chain(const Coarse &G, int I, int nq, const double *UF, const double *UG, double *Q, double *gtmp,
                hipStream_t st);
// S: the batch's references at slice I (hit_flag = the sweep's flags[nq]; no host flag, no wait)
int chain_sweep(const Coarse &G, int I, int N, int i0, double *U1, double *UG1, const TrainSet &T, const FitSet &F,
                const SpecRefs &S, double *preds, int *stop_out, float *g_ms_out, hipStream_t st);
int chain_miss_fits(const TrainSet &T, const FitSet &F, const double *theta0, const PredOut &O, hipStream_t st);

}  // namespace nngp
