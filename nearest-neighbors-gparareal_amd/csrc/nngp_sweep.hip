// nngp_sweep.hip -- the sequential correction sweep of one Parareal iteration, driven natively.
//
// Reference: parareal.py:359-382 (modern) / new_lib.py:990-1012 (legacy).  For i = I .. N-1:
//     uG[i+1, :, k+1] = run_G(t[i], t[i+1], u[i, :, k+1])                 (:361-363)
//     preds           = model.predict(u[i, :, k+1], uF[i+1, :, k], uG[i+1, :, k])   (:367-368)
//     u[i+1, :, k+1]  = preds + uG[i+1, :, k+1]                            (:382)
// Slice i+1 depends on slice i, so the sweep is a chain of small launches (G: one RK launch;
// nnGP: kNN distance, kNN select, fused fits + arg-min + mean + update).  Driving that chain from
// Python costs tens of microseconds of interpreter/ctypes work per launch; here the loop issues the
// launches back to back on one stream, so the GPU never waits for the host.
#include <algorithm>
#include <atomic>
#include <mutex>
#include <vector>

#include "common.h"

namespace nngp {
// grow-only pool of timing events (G time per slice without host synchronisation in the loop)
static std::vector<hipEvent_t> g_events;
static std::mutex g_events_mu;

static int timing_events(size_t n, hipEvent_t **out) {   // *out = n events
    std::lock_guard<std::mutex> lk(g_events_mu);
    while (g_events.size() < n) {
        hipEvent_t e;
        NNGP_HIP_CHECK(hipEventCreate(&e));
        g_events.push_back(e);
    }
    *out = g_events.data();
    return NNGP_OK;
}

int GTimer::begin(float *g_ms_out, int64_t n_slices, int every) {
    *this = GTimer{};
    if (g_ms_out) *g_ms_out = 0.f;
    if (!g_ms_out || n_slices <= 0) return NNGP_OK;
    out = g_ms_out; slices = n_slices; stride = every;
    return timing_events(2 * (size_t)n_slices, &ev);
}

int GTimer::finish() const {
    if (!ev) return NNGP_OK;
    const int64_t ns = (slices - 1) / stride + 1;   // timed slices j = 0, stride, 2 stride, ...
    NNGP_HIP_CHECK(hipEventSynchronize(ev[2 * (size_t)(ns - 1) * stride + 1]));
    float total = 0.f;
    for (int64_t k = 0; k < ns; k++) {
        const size_t j = (size_t)k * stride;
        float ms = 0.f;
        NNGP_HIP_CHECK(hipEventElapsedTime(&ms, ev[2 * j], ev[2 * j + 1]));
        total += ms;
    }
    // every G launch of a sweep is the same work; with every slice timed the sum is the answer
    *out = ns == slices ? total : total * (float)slices / (float)ns;
    return NNGP_OK;
}

// nngp_shutdown: the sweep's timing events (re-created on next use)
static void events_release() {
    std::lock_guard<std::mutex> lk(g_events_mu);
    for (hipEvent_t e : g_events) (void)hipEventDestroy(e);
    g_events.clear();
}

// re-speculation resources (per process; one device per process): a side stream, the events
// that order it against the sweep's stream, and host-mapped hit flags the select kernel writes
struct Respec {
    int dev = -1;
    hipStream_t st2 = nullptr;
    hipEvent_t ev_g = nullptr, ev_r = nullptr;
    hipStream_t st3 = nullptr;      // the overlapped speculative batch
    hipEvent_t ev_pre = nullptr, ev_sel = nullptr, ev_b = nullptr;
    int32_t *herr = nullptr;        // host-mapped: a mean kernel's wait timed out
    int32_t *hflags = nullptr;   // host-mapped, fine-grained
    size_t nflags = 0;
};
static Respec g_respec;
static std::mutex g_respec_mu;

static int respec_resources(size_t nflags, Respec **out) {
    std::lock_guard<std::mutex> lk(g_respec_mu);
    Respec &r = g_respec;
    int dev = 0;
    NNGP_HIP_CHECK(hipGetDevice(&dev));
    if (r.dev != dev) {   // first use (or another device): fresh stream / events / flags
        if (r.st2) (void)hipStreamDestroy(r.st2);
        if (r.ev_g) (void)hipEventDestroy(r.ev_g);
        if (r.ev_r) (void)hipEventDestroy(r.ev_r);
        if (r.st3) (void)hipStreamDestroy(r.st3);
        for (hipEvent_t e : {r.ev_pre, r.ev_sel, r.ev_b})
            if (e) (void)hipEventDestroy(e);
        if (r.herr) (void)hipHostFree(r.herr);
        if (r.hflags) (void)hipHostFree(r.hflags);
        r = Respec{};
        NNGP_HIP_CHECK(hipStreamCreateWithFlags(&r.st2, hipStreamNonBlocking));
        NNGP_HIP_CHECK(hipEventCreateWithFlags(&r.ev_g, hipEventDisableTiming));
        NNGP_HIP_CHECK(hipEventCreateWithFlags(&r.ev_r, hipEventDisableTiming));
        NNGP_HIP_CHECK(hipStreamCreateWithFlags(&r.st3, hipStreamNonBlocking));
        NNGP_HIP_CHECK(hipEventCreateWithFlags(&r.ev_pre, hipEventDisableTiming));
        NNGP_HIP_CHECK(hipEventCreateWithFlags(&r.ev_sel, hipEventDisableTiming));
        NNGP_HIP_CHECK(hipEventCreateWithFlags(&r.ev_b, hipEventDisableTiming));
        NNGP_HIP_CHECK(hipHostMalloc((void **)&r.herr, 64, hipHostMallocMapped | hipHostMallocCoherent));
        r.dev = dev;
    }
    if (r.nflags < nflags) {
        if (r.hflags) (void)hipHostFree(r.hflags);
        r.hflags = nullptr;
        r.nflags = 0;
        NNGP_HIP_CHECK(hipHostMalloc((void **)&r.hflags, sizeof(int32_t) * nflags,
                                     hipHostMallocMapped | hipHostMallocCoherent));
        r.nflags = nflags;
    }
    *out = &r;
    return NNGP_OK;
}

// G beside the prediction (g_side_supported): a side stream and its two ordering events
struct GSide {
    int dev = -1;
    hipStream_t st = nullptr;
    hipEvent_t ev_u = nullptr, ev_g = nullptr;   // U1[i] ready (sweep stream) / G(U1[i]) done (side)
};
static GSide g_gside;

static int gside_resources(GSide **out) {
    std::lock_guard<std::mutex> lk(g_respec_mu);
    int dev = 0;
    NNGP_HIP_CHECK(hipGetDevice(&dev));
    if (g_gside.dev != dev) {
        if (g_gside.st) (void)hipStreamDestroy(g_gside.st);
        for (hipEvent_t e : {g_gside.ev_u, g_gside.ev_g})
            if (e) (void)hipEventDestroy(e);
        g_gside = GSide{};
        NNGP_HIP_CHECK(hipStreamCreateWithFlags(&g_gside.st, hipStreamNonBlocking));
        NNGP_HIP_CHECK(hipEventCreateWithFlags(&g_gside.ev_u, hipEventDisableTiming));
        NNGP_HIP_CHECK(hipEventCreateWithFlags(&g_gside.ev_g, hipEventDisableTiming));
        g_gside.dev = dev;
    }
    *out = &g_gside;
    return NNGP_OK;
}

// nngp_shutdown: the side streams, events and host-mapped flags (re-created on next use)
void sweep_release() {
    events_release();
    std::lock_guard<std::mutex> lk(g_respec_mu);
    Respec &r = g_respec;
    if (r.st2) (void)hipStreamDestroy(r.st2);
    if (r.st3) (void)hipStreamDestroy(r.st3);
    for (hipEvent_t e : {r.ev_g, r.ev_r, r.ev_pre, r.ev_sel, r.ev_b})
        if (e) (void)hipEventDestroy(e);
    if (r.herr) (void)hipHostFree(r.herr);
    if (r.hflags) (void)hipHostFree(r.hflags);
    r = Respec{};
    if (g_gside.st) (void)hipStreamDestroy(g_gside.st);
    for (hipEvent_t e : {g_gside.ev_u, g_gside.ev_g})
        if (e) (void)hipEventDestroy(e);
    g_gside = GSide{};
}

// wait for the select kernel's host-mapped hit flag (-1 = not yet written); a stream that has
// drained (or failed) without writing it is an error, never a hang
static int wait_flag(const int32_t *flag, hipStream_t st, int32_t *out) {
    for (uint64_t spin = 1;; spin++) {
        const int32_t v = __atomic_load_n(flag, __ATOMIC_ACQUIRE);
        if (v >= 0) {
            *out = v;
            return NNGP_OK;
        }
        if ((spin & 1023) == 0) {
            const hipError_t q = hipStreamQuery(st);
            if (q == hipSuccess && __atomic_load_n(flag, __ATOMIC_ACQUIRE) < 0) {
                set_error("correction sweep: speculation flag was not written");
                return NNGP_E_HIP;
            }
            if (q != hipSuccess && q != hipErrorNotReady) {
                set_error("correction sweep: %s", hipGetErrorString(q));
                return NNGP_E_HIP;
            }
        }
    }
}

// Speculation policy: worth it while the batch of every slice's fits is a throughput-shaped
// launch much cheaper than the latency-bound sweep it shortens (Burgers N=128: 146k fits; not
// FHN-PDE d=800 N=512: 3.7M).  NNGP_SPEC_MAX_FITS overrides the bound (0 disables).
static bool speculate_ok(int speculate, int64_t nq, int64_t n_fits) {
    if (speculate == 0 || nq < 2) return false;
    if (speculate > 0) return true;
    const char *e = getenv("NNGP_SPEC_MAX_FITS");
    const int64_t bound = e ? atoll(e) : 262144;
    return nq * n_fits <= bound;
}

// sweeps rerun with the batch serialised because a hit's wait timed out (nngp_sweep_late_reruns)
static std::atomic<int64_t> g_late_reruns{0};

// nngp_correction_sweep's arguments; T.d = sys->d.  U1 / UG1: the iterate being written, UF / UG: the
// previous iterate's fine and coarse results
struct SweepArgs {
    Coarse G; int I, N; double *U1, *UG1; const double *UF, *UG; int model; TrainSet T; FitSet F;
    const double *theta0; double *preds_scratch; int speculate; int32_t *spec_hits_out; float *g_ms_out;
    hipStream_t st;
    double *u1(int i) const { return U1 + (size_t)i * T.d; }
    double *ug1(int i) const { return UG1 + (size_t)i * T.d; }
    const double *uf(int i) const { return UF + (size_t)i * T.d; }
    const double *ug(int i) const { return UG + (size_t)i * T.d; }
};

// The speculation plan (nnGP).  Speculation: guess every slice's query along the coarse chain from
// U1[I] (reguess) and run all of their fits as one batch; the sweep then only recomputes the slices
// whose actual ordered neighbour list differs from the guessed one.
struct SpecPlan {
    bool spec = false;
    // the fused chain (nngp_gp.hip chain_kernel) instead of the launch chain
    bool chained = false;
    // overlapped batch (NNGP_SPEC_OVERLAP, default 1; launch chain only): the batch's fits run on a
    // side stream while the sweep starts as soon as the batch's neighbour lists exist; a hit slice's
    // mean waits for that slice's fits only (per-prediction completion counters, b.done)
    bool overlap = false;
    // hit means finished in the select (NNGP_HIT_MEAN, default 1; launch chain with host flags only):
    // every prediction of the batch (AP1) and of each re-speculation window (AP2) prepared by
    // gp_pre_kernel after its fits, pre1 / pre2 counting the prepared workgroups per slice
    bool hitmean = false;
    // re-speculation: the chain guesses drift; when slice i misses, the next W slices are guessed
    // again, restarted from the actual U1[i], and their fits run as one launch on a side stream while
    // slice i's own fits run.  Their lists / fits form a second candidate set (hit = 2).
    int W = 0;
    size_t hst = 0;   // HitMean doubles per slice
    SpecWs b{};       // the slot-2 buffers
    Respec *rs = nullptr;
    bool respec_pending = false;   // a window was issued on rs->st2 and the sweep has not waited for ev_r
};

static int sweep_check(const SweepArgs &a) {
    NNGP_REQUIRE(a.G.sys != nullptr && a.G.t && a.U1 && a.UG1, "null argument");
    NNGP_REQUIRE(0 <= a.I && a.I <= a.N, "need 0 <= I <= N (I=%d N=%d)", a.I, a.N);
    NNGP_REQUIRE(a.model == NNGP_MODEL_PARAREAL || a.model == NNGP_MODEL_NNGP || a.model == NNGP_MODEL_GPFULL,
                 "unknown model %d", a.model);
    if (a.model == NNGP_MODEL_PARAREAL) NNGP_REQUIRE(a.UF && a.UG, "parareal model needs UF and UG");
    if (a.model == NNGP_MODEL_NNGP)
        NNGP_REQUIRE(a.T.X && a.T.Y && a.theta0 && a.preds_scratch && a.T.rows >= a.F.m && a.F.m >= 1,
                     "nngp model arguments");
    if (a.model == NNGP_MODEL_GPFULL)
        NNGP_REQUIRE(a.T.X && a.T.Y && a.theta0 && a.T.rows >= 1, "full-GP model arguments (X, alpha, coefficients)");
    return NNGP_OK;
}

// w guesses along the coarse chain by the classic Parareal update (models.py:82-83),
//     g[s+1] = G(g[s]) + (UF[s+1] - UG[s+1]),
// Q[q] for slice i+q+1, from the state u of slice i -- or from g0 = G(u) where the sweep has it
// already; tmp[d] takes every other G
static int reguess(const SweepArgs &a, int i, int w, const double *u, const double *g0, double *Q, double *tmp,
                   hipStream_t st) {
    const int d = a.T.d;
    int rc = NNGP_OK;
    for (int q = 0; q < w && rc == NNGP_OK; q++) {
        const int s = i + q;
        const double *g = g0;
        if (q > 0 || !g0) {
            rc = a.G.run(s, q > 0 ? Q + (size_t)(q - 1) * d : u, tmp, st);
            g = tmp;
        }
        if (rc == NNGP_OK) rc = nngp_parareal_update(d, a.uf(s + 1), a.ug(s + 1), g, Q + (size_t)q * d, st);
    }
    return rc;
}

// the plan's flags and resources, the carve of its buffers, the guesses and the batch
static int spec_plan(const SweepArgs &a, bool allow_overlap, bool allow_chain, SpecPlan &p) {
    const int d = a.T.d, m = a.F.m;
    const int64_t nq = a.N - a.I, nf = a.F.n_fits(d);
    hipStream_t st = a.st;
    p.spec = a.model == NNGP_MODEL_NNGP && a.UF && a.UG && speculate_ok(a.speculate, nq, nf);
    if (!p.spec) return NNGP_OK;
    p.W = (int)std::min<int64_t>(std::max(0, env_int("NNGP_RESPEC_W", 4)), nq - 1);   // (0 disables)
    int rc = respec_resources((size_t)nq, &p.rs);
    if (rc) return rc;
    Respec *rs = p.rs;
    p.chained = allow_chain && chain_supported(a.G.sys, a.G.step_mode, m);
    p.overlap = !p.chained && allow_overlap && env_int("NNGP_SPEC_OVERLAP", 1) != 0;
    p.hitmean = !p.chained && p.W > 0 && env_int("NNGP_HIT_MEAN", 1) != 0;
    p.hst = p.hitmean ? (size_t)d * HM_STRIDE(pre_maxm(m)) : 0;
    int err = 0;
    char *ws = (char *)workspace(spec_ws_carve(nullptr, nq, d, m, nf, p.W, p.hst).bytes, &err, 2);
    if (err) return err;
    const SpecWs &b = p.b = spec_ws_carve(ws, nq, d, m, nf, p.W, p.hst);
    if (p.W > 0) {
        NNGP_HIP_CHECK(hipMemsetAsync(b.spec2_idx, 0xFF, sizeof(int32_t) * (size_t)nq * m, st));   // -1: none
        for (int64_t j = 0; j < nq; j++) rs->hflags[j] = -1;
    }
    if (p.hitmean) NNGP_HIP_CHECK(hipMemsetAsync(b.pre1, 0, sizeof(int32_t) * 2 * (size_t)nq, st));   // pre1 | pre2
    NNGP_HIP_CHECK(hipMemcpyAsync(b.Qg, a.u1(a.I), sizeof(double) * d, hipMemcpyDeviceToDevice, st));
    if (guess_chain_supported(a.G.sys, a.G.step_mode))   // one launch for the whole chain (bitwise)
        rc = guess_chain(a.G, a.I, (int)nq, a.UF, a.UG, b.Qg, b.gtmp, st);
    else
        rc = reguess(a, a.I, (int)nq - 1, b.Qg, nullptr, b.Qg + d, b.gtmp, st);
    if (rc) return rc;
    if (p.overlap) {
        *rs->herr = 0;
        NNGP_HIP_CHECK(hipEventRecord(rs->ev_pre, st));             // the guesses Qg
        NNGP_HIP_CHECK(hipStreamWaitEvent(rs->st3, rs->ev_pre, 0));
    }
    rc = spec_batch(a.T, a.F, b.Qg, (int)nq, a.theta0, b.spec_idx, b.spec_fits, false, p.overlap ? rs->st3 : st, 1,
                    p.overlap ? b.done : nullptr, p.overlap ? rs->ev_sel : nullptr, b.AP1, b.pre1);
    if (rc || !p.overlap) return rc;
    NNGP_HIP_CHECK(hipEventRecord(rs->ev_b, rs->st3));
    NNGP_HIP_CHECK(hipStreamWaitEvent(st, rs->ev_sel, 0));   // lists ready; fits may run on
    return NNGP_OK;
}

// After a miss at slice s: re-guess slices s+1 .. s+w from the actual U1[s] (its G is the sweep's own
// UG1[s+1]) on the side stream, and their lists and fits there as one latency-shaped launch (a wave
// per fit: the sweep waits on this window's fits); ev_r marks them ready.  AP2 / pre2: the window's
// HitMean coordinates and counters (or null).
static int respec_issue(const SweepArgs &a, SpecPlan &p, int s, double *AP2, int32_t *pre2) {
    const size_t j1 = (size_t)(s - a.I) + 1;
    const size_t nf = (size_t)a.F.n_fits(a.T.d);
    const int w = (int)std::min<int64_t>(p.W, a.N - 1 - s);
    hipStream_t s2 = p.rs->st2;
    int rc = reguess(a, s, w, nullptr, a.ug1(s + 1), p.b.Qr, p.b.gtmp2, s2);
    if (rc == NNGP_OK)
        rc = spec_batch(a.T, a.F, p.b.Qr, w, a.theta0 + j1 * nf * 2, p.b.spec2_idx + j1 * a.F.m,
                        p.b.spec2_fits + j1 * nf * 4, true, s2, 6, nullptr, nullptr, AP2, pre2);
    if (rc) return rc;
    NNGP_HIP_CHECK(hipEventRecord(p.rs->ev_r, s2));
    p.respec_pending = true;
    return NNGP_OK;
}

// The fused chain: runs of hit slices as one persistent kernel; the host takes over at each miss
// (that slice's fits, the re-speculation), then resumes it.  The G time is the chain's own clock.
static int sweep_chain(const SweepArgs &a, SpecPlan &p, int *late) {
    const SpecWs &b = p.b;
    const SpecRefs S{b.spec_idx, b.spec_fits, b.flags, b.spec2_idx, b.spec2_fits, nullptr, nullptr, nullptr};
    const size_t nf = (size_t)a.F.n_fits(a.T.d);
    float g_ms = 0.f;
    int rc = NNGP_OK;
    for (int i = a.I; i < a.N && rc == NNGP_OK;) {
        if (p.respec_pending) NNGP_HIP_CHECK(hipStreamWaitEvent(a.st, p.rs->ev_r, 0));   // lists/fits ready
        p.respec_pending = false;
        int s = a.N;
        rc = chain_sweep(a.G, a.I, a.N, i, a.U1, a.UG1, a.T, a.F, S, a.preds_scratch, &s, &g_ms, a.st);
        if (rc && s == -2) *late = 1;   // a grid barrier timed out: rerun on the launch chain
        if (rc || s >= a.N) break;
        // miss at slice s: G(U1[s]) and its select are done (the chain kernel has drained)
        rc = chain_miss_fits(a.T, a.F, a.theta0 + (size_t)(s - a.I) * nf * 2,
                             {a.preds_scratch, a.ug1(s + 1), a.u1(s + 1), nullptr}, a.st);
        if (rc == NNGP_OK && p.W > 0 && s + 1 < a.N) rc = respec_issue(a, p, s, nullptr, nullptr);
        i = s + 1;
    }
    if (a.g_ms_out && rc == NNGP_OK) *a.g_ms_out = g_ms;
    return rc;
}

// The launch chain.  With a host flag (W > 0, not the last slice: split_at) the prediction is issued
// in two parts: the kNN + select, then -- once the host has read the select's hit code -- the mean
// alone on a hit (the fits are the batch's) or the fits and the mean on a miss.  The fits launch a hit
// would have skipped on the device is never issued: its waves (191 VGPRs) could only be dispatched
// once the overlapped batch's waves drained a SIMD.  With HitMean the select finishes a hit's mean
// itself once the prediction is prepared (host code 3 / 4), and no mean launch follows.
//
// Look-ahead (HitMean only): once the batch's predictions are all prepared, a hit finishes in its
// select, so slice i+1's head is queued behind slice i's select before the host reads slice i's
// code.  On a miss or a hit that still needs the mean kernel, the early head read a U1[i+1] that
// was not written yet: the host waits for its select's host flag, resets it, redoes slice i's
// distances and select (the workspace the fits / mean read), and slice i+1's head follows later --
// every value the early launches wrote is written again.  (Before the batch is prepared, queueing
// slice i's mean kernel first and the head behind it measured no gain: those slices wait on the
// batch's fits, profiles/r05/sweep/host_path_ab.txt.)
static int sweep_launches(const SweepArgs &a, SpecPlan &p, const GTimer &gt, GSide *gs, int64_t hit_codes[5]) {
    const int d = a.T.d, m = a.F.m, I = a.I, N = a.N, W = p.W;
    const size_t nf = (size_t)a.F.n_fits(d), hst = p.hst;
    const SpecWs &b = p.b;
    Respec *rs = p.rs;
    hipStream_t st = a.st;
    const bool nngp_model = a.model == NNGP_MODEL_NNGP;
    const bool gdist_ok = gdist_supported(a.G.sys, a.G.step_mode);
    const bool ahead_on = env_int("NNGP_SWEEP_AHEAD", 1) != 0;
    auto split_at = [&](int i) { return p.spec && W > 0 && i + 1 < N; };
    auto predict_at = [&](int i, int phase, bool host_flag, hipEvent_t bias_ready = nullptr) {
        const size_t j = (size_t)(i - I);
        const bool hf = host_flag && split_at(i);   // every written flag is awaited
        HitMean hm{};
        if (p.hitmean && hf)
            hm = HitMean{b.AP1 + j * hst, b.AP2 + j * hst, b.pre1 + j, b.pre2 + j, pre_target(d, m), pre_maxm(m),
                         a.ug1(i + 1), a.u1(i + 1), a.preds_scratch};
        SpecRefs S{};
        if (p.spec) S.spec_idx = b.spec_idx + j * m, S.spec_fits = b.spec_fits + j * nf * 4, S.hit_flag = b.flags + j;
        if (W > 0) S.spec2_idx = b.spec2_idx + j * m, S.spec2_fits = b.spec2_fits + j * nf * 4;
        if (hf) S.host_flag = rs->hflags + j;
        if (p.overlap) S.wait_done = b.done + j, S.wait_err = rs->herr;
        return predict_impl(a.T, a.F, a.u1(i), a.theta0 + j * nf * 2, {a.preds_scratch, a.ug1(i + 1), a.u1(i + 1), nullptr},
                            S, st, 0, -1, phase, hm.out ? &hm : nullptr, bias_ready);
    };
    // slice i's head: G(U1[i]) (with the kNN distances as one launch, gdist, on the untimed split
    // slices), the re-speculation window's lists, and the select (or the whole prediction)
    auto head = [&](int i) -> int {
        const size_t j = (size_t)(i - I);
        const bool fused = nngp_model && split_at(i) && gdist_ok && !gt.timed(j);
        // an unsplit prediction's G on the side stream: only the mean needs G(U1[i]) (its bias)
        const bool side = nngp_model && !split_at(i) && gs && !gt.timed(j);
        int r;
        if (fused) {
            r = gdist(a.G, i, a.T, a.F, a.u1(i), a.ug1(i + 1), st);
        } else if (side) {
            NNGP_HIP_CHECK(hipEventRecord(gs->ev_u, st));   // U1[i] (the previous slice's mean)
            NNGP_HIP_CHECK(hipStreamWaitEvent(gs->st, gs->ev_u, 0));
            r = gt.launch(a.G, i, j, a.u1(i), a.ug1(i + 1), gs->st);   // (untimed)
            if (r == NNGP_OK) NNGP_HIP_CHECK(hipEventRecord(gs->ev_g, gs->st));
        } else {
            r = gt.launch(a.G, i, j, a.u1(i), a.ug1(i + 1), st);
        }
        if (r) return r;
        if (a.model == NNGP_MODEL_PARAREAL)   // (uF - uG_prev) + uG_new, models.py:82-83
            return nngp_parareal_update(d, a.uf(i + 1), a.ug(i + 1), a.ug1(i + 1), a.u1(i + 1), st);
        if (a.model == NNGP_MODEL_GPFULL)     // GPjax_p.predict + uG (models.py:456-462)
            return gpfull_mean(a.T.X, a.T.rows, d, a.u1(i), a.theta0, a.T.Y, a.ug1(i + 1), a.u1(i + 1), st);
        if (W > 0) {
            if (p.respec_pending) NNGP_HIP_CHECK(hipStreamWaitEvent(st, rs->ev_r, 0));   // lists/fits ready
            p.respec_pending = false;
        }
        return predict_at(i, split_at(i) ? (fused ? PREDICT_SELECT_ONLY : PREDICT_SELECT) : PREDICT_ALL, true,
                          side ? gs->ev_g : nullptr);
    };
    bool pre_ready = !p.overlap;   // serialised batch: prepared before the sweep
    bool issued = false;           // slice i's head was queued by slice i-1's look-ahead
    int rc = NNGP_OK;
    for (int i = I; i < N && rc == NNGP_OK; i++) {
        const size_t j = (size_t)(i - I);
        if (!issued) rc = head(i);
        issued = false;
        if (rc) break;
        if (!nngp_model || !split_at(i)) continue;
        if (p.hitmean && !pre_ready) pre_ready = hipEventQuery(rs->ev_b) == hipSuccess;
        const bool ahead = ahead_on && p.hitmean && pre_ready && split_at(i + 1);
        if (ahead && (rc = head(i + 1)) != NNGP_OK) break;
        int32_t hit = 0;
        rc = wait_flag(rs->hflags + j, st, &hit);
        // a mean that gave up waiting for the overlapped batch: stop issuing, the caller reruns
        if (rc == NNGP_OK && p.overlap && __atomic_load_n(rs->herr, __ATOMIC_ACQUIRE) != 0) break;
        if (rc) break;
        // a miss's re-speculation window starts from G(U1[i]): the event is recorded only on a miss,
        // behind the select the host has just seen finish (so behind G), before the slice's fits
        if (hit == 0) NNGP_HIP_CHECK(hipEventRecord(rs->ev_g, st));
        hit_codes[std::min(hit, 4)]++;
        if (hit >= 3) {   // the select finished the mean (HitMean)
            issued = ahead;
            continue;
        }
        if (ahead) {   // undo the look-ahead (above)
            int32_t early = 0;
            if ((rc = wait_flag(rs->hflags + j + 1, st, &early)) != NNGP_OK) break;
            __atomic_store_n(rs->hflags + j + 1, -1, __ATOMIC_RELEASE);
            if ((rc = predict_at(i, PREDICT_SELECT, false)) != NNGP_OK) break;
        }
        rc = predict_at(i, hit != 0 ? PREDICT_MEAN : PREDICT_FITS_MEAN, true);
        if (rc || hit != 0) continue;
        NNGP_HIP_CHECK(hipStreamWaitEvent(rs->st2, rs->ev_g, 0));   // miss: the window, from G(U1[i])
        rc = respec_issue(a, p, i, p.hitmean ? b.AP2 + (j + 1) * hst : nullptr, p.hitmean ? b.pre2 + j + 1 : nullptr);
    }
    return rc;
}

// the side streams never outlive the sweep (also on an error path: their buffers are reused); then
// the hit count, the reports and the G time
static int sweep_drain(const SweepArgs &a, SpecPlan &p, const GTimer &gt, int rc, const int64_t hit_codes[5],
                       int *late) {
    hipStream_t st = a.st;
    if (p.respec_pending) NNGP_HIP_CHECK(hipStreamWaitEvent(st, p.rs->ev_r, 0));
    if (p.overlap) {
        NNGP_HIP_CHECK(hipStreamWaitEvent(st, p.rs->ev_b, 0));
        NNGP_HIP_CHECK(hipStreamSynchronize(st));
        if (rc == NNGP_OK && __atomic_load_n(p.rs->herr, __ATOMIC_ACQUIRE) != 0) {
            // a hit slice's mean gave up waiting for the batch's fits (bounded spin; e.g. a GPU
            // shared by several ranks) and wrote nothing: the caller redoes the sweep serially
            set_error("correction sweep: a speculative fit count was not reached in time");
            *late = 1;
            rc = NNGP_E_HIP;
        }
    }
    if (a.spec_hits_out && rc == NNGP_OK) {   // speculation hits (0 when not speculating)
        *a.spec_hits_out = 0;
        if (p.spec) {
            const int64_t nq = a.N - a.I;
            std::vector<int32_t> h((size_t)nq);
            NNGP_HIP_CHECK(hipMemcpyAsync(h.data(), p.b.flags, sizeof(int32_t) * nq, hipMemcpyDeviceToHost, st));
            NNGP_HIP_CHECK(hipStreamSynchronize(st));
            for (int32_t v : h) *a.spec_hits_out += v != 0;
        }
    }
    sel_prof_report("sweep");
    if (env_int("NNGP_SWEEP_STATS", 0))   // the host-flag codes seen
        fprintf(stderr, "sweep I=%d N=%d: miss %lld, hit (mean kernel) %lld / %lld, hit (mean in select) %lld / %lld\n",
                a.I, a.N, (long long)hit_codes[0], (long long)hit_codes[1], (long long)hit_codes[2],
                (long long)hit_codes[3], (long long)hit_codes[4]);
    if (rc == NNGP_OK) return gt.finish();   // the G launches' time once the sweep has drained
    return rc;
}

static int correction_sweep(const SweepArgs &a, bool allow_overlap, bool allow_chain, int *late) {
    *late = 0;
    int rc = sweep_check(a);
    if (rc) return rc;
    GSide *gs = nullptr;
    if (a.model == NNGP_MODEL_NNGP && g_side_supported(a.G.sys, a.G.step_mode) && (rc = gside_resources(&gs)) != NNGP_OK)
        return rc;
    GTimer gt;
    if ((rc = gt.begin(a.g_ms_out, (int64_t)a.N - a.I, g_time_stride())) != NNGP_OK) return rc;
    SpecPlan p;
    if ((rc = spec_plan(a, allow_overlap, allow_chain, p)) != NNGP_OK) return rc;
    int64_t hit_codes[5] = {0, 0, 0, 0, 0};
    if (p.chained) {
        rc = sweep_chain(a, p, late);
        gt.drop();
    } else {
        rc = sweep_launches(a, p, gt, gs, hit_codes);
    }
    return sweep_drain(a, p, gt, rc, hit_codes, late);
}

}  // namespace nngp

extern "C" int nngp_correction_sweep(const nngp_system *sys, int g_tableau, int g_step_mode,
                                     int64_t g_steps, const double *t, int I, int N, double *U1,
                                     double *UG1, const double *UF, const double *UG, int model,
                                     const double *X, const double *Y, int64_t rows, int m,
                                     int n_jitter, const double *jitter_exp_host, int n_restarts,
                                     const double *theta0, double fatol, double xatol, int maxfev,
                                     double *preds_scratch, int speculate, int32_t *spec_hits_out,
                                     float *g_ms_out, void *stream) {
    using namespace nngp;
    const SweepArgs a{{sys, g_tableau, g_step_mode, g_steps, t}, I, N, U1, UG1, UF, UG, model,
                      {X, Y, rows, sys ? sys->d : 0}, {m, n_jitter, jitter_exp_host, n_restarts, fatol, xatol, maxfev},
                      theta0, preds_scratch, speculate, spec_hits_out, g_ms_out, (hipStream_t)stream};
    // The sweep writes UG1[i+1] and U1[i+1] for i >= I only and reads none of them before writing,
    // so a sweep whose overlapped batch fell behind, or whose fused chain's grid barrier timed out
    // (see sweep_drain / sweep_chain), is simply run again with the batch serialised on the launch
    // chain: the same bits, later.
    int late = 0;
    int rc = correction_sweep(a, true, true, &late);
    if (rc != NNGP_OK && late) {
        g_late_reruns.fetch_add(1);
        rc = correction_sweep(a, false, false, &late);
    }
    return rc;
}

extern "C" int64_t nngp_sweep_late_reruns(void) { return nngp::g_late_reruns.load(); }
