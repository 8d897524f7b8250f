// nngp_poly.hip -- registry of the polynomial vector fields (NNGP_SYS_POLY, include/nngp.h;
// DESIGN.md 3.2c): nngp_poly_create / nngp_poly_destroy and the lookups the propagator dispatch
// uses (common.h).  Host code only: the kernels that evaluate a table are the lane and field
// propagators of nngp_rk_kernels.h.
//
// The reference's extension point is a subclass of ODE with its own _f_np / _f_jax
// (systems.py:23-61).  Here the right-hand side is data: d rows of ordered terms
// (coef, up to three state indices).  The kernels trust a registered table -- they index the
// state with its indices and walk its rows without a bound check -- so everything is checked
// here, on the host, before any HIP call.
#include <cmath>
#include <mutex>
#include <vector>

#include "common.h"

namespace nngp {

struct PolyDev {
    int dev;
    void *block;   // terms [n_terms] (16-byte records first, for their alignment) | row_ptr [d+1]
};
struct PolyEntry {
    bool live = false;
    int d = 0;
    std::vector<int32_t> row_ptr;
    std::vector<PolyTerm> terms;
    std::vector<PolyDev> devs;
};
static std::vector<PolyEntry> g_poly;   // handle = index + 1
static std::mutex g_poly_mu;

static void poly_free_devs(PolyEntry &e) {
    for (PolyDev &p : e.devs)
        if (p.block) (void)hipFree(p.block);   // implicit device synchronisation: no launch still reads it
    e.devs.clear();
}

static PolyEntry *poly_entry(const nngp_system *sys) {
    const int h = sys->nx;
    if (h < 1 || h > (int)g_poly.size() || !g_poly[h - 1].live) {
        set_error("poly: unknown or destroyed table handle %d (nngp_system.nx holds the handle of nngp_poly_create)", h);
        return nullptr;
    }
    PolyEntry *e = &g_poly[h - 1];
    if (sys->d != e->d) {
        set_error("poly: system has d=%d but table %d was created with d=%d", sys->d, h, e->d);
        return nullptr;
    }
    return e;
}

int poly_table(const nngp_system *sys, PolyTable *out) {
    std::lock_guard<std::mutex> lk(g_poly_mu);
    PolyEntry *e = poly_entry(sys);
    if (!e) return NNGP_E_ARG;
    out->d = e->d;
    out->n_terms = (int)e->terms.size();
    out->row_ptr = e->row_ptr.data();
    out->terms = e->terms.data();
    return NNGP_OK;
}

int poly_device(const nngp_system *sys, const int32_t **row_ptr, const PolyTerm **terms) {
    std::lock_guard<std::mutex> lk(g_poly_mu);
    PolyEntry *e = poly_entry(sys);
    if (!e) return NNGP_E_ARG;
    int dev = 0;
    NNGP_HIP_CHECK(hipGetDevice(&dev));
    void *block = nullptr;
    for (const PolyDev &p : e->devs)
        if (p.dev == dev) block = p.block;
    const size_t tbytes = sizeof(PolyTerm) * e->terms.size(), rbytes = sizeof(int32_t) * e->row_ptr.size();
    if (!block) {
        NNGP_HIP_CHECK(hipMalloc(&block, tbytes + rbytes));
        hipError_t err = hipSuccess;
        if (tbytes) err = hipMemcpy(block, e->terms.data(), tbytes, hipMemcpyHostToDevice);
        if (err == hipSuccess)
            err = hipMemcpy((char *)block + tbytes, e->row_ptr.data(), rbytes, hipMemcpyHostToDevice);
        if (err != hipSuccess) {
            (void)hipFree(block);
            set_error("poly: upload of table %d failed: %s", sys->nx, hipGetErrorString(err));
            return NNGP_E_HIP;
        }
        e->devs.push_back(PolyDev{dev, block});
    }
    *terms = (const PolyTerm *)block;
    *row_ptr = (const int32_t *)((const char *)block + tbytes);
    return NNGP_OK;
}

void poly_release() {
    std::lock_guard<std::mutex> lk(g_poly_mu);
    for (PolyEntry &e : g_poly) poly_free_devs(e);
    g_poly.clear();
}

}  // namespace nngp

extern "C" int nngp_poly_create(int d, int n_terms, const int32_t *row_ptr_host, const double *coef_host,
                                const int16_t *idx_host, int32_t *handle_out) {
    using namespace nngp;
    NNGP_REQUIRE(handle_out != nullptr, "poly: handle_out is NULL");
    NNGP_REQUIRE(d >= 1 && d <= POLY_MAX_D, "poly: d=%d outside 1..%d", d, POLY_MAX_D);
    NNGP_REQUIRE(n_terms >= 0 && n_terms <= POLY_MAX_TERMS, "poly: n_terms=%d outside 0..%d", n_terms,
                 POLY_MAX_TERMS);
    NNGP_REQUIRE(row_ptr_host != nullptr, "poly: row_ptr is NULL");
    NNGP_REQUIRE(n_terms == 0 || (coef_host != nullptr && idx_host != nullptr), "poly: coef / idx is NULL");
    NNGP_REQUIRE(row_ptr_host[0] == 0, "poly: row_ptr[0] = %d, must be 0", row_ptr_host[0]);
    for (int c = 0; c < d; c++)
        NNGP_REQUIRE(row_ptr_host[c + 1] >= row_ptr_host[c] && row_ptr_host[c + 1] <= n_terms,
                     "poly: row_ptr must be non-decreasing and end at n_terms=%d (row_ptr[%d] = %d, row_ptr[%d] = %d)",
                     n_terms, c, row_ptr_host[c], c + 1, row_ptr_host[c + 1]);
    NNGP_REQUIRE(row_ptr_host[d] == n_terms, "poly: row_ptr[d] = %d, must be n_terms = %d", row_ptr_host[d], n_terms);
    std::vector<PolyTerm> terms((size_t)n_terms);
    for (int t = 0; t < n_terms; t++) {
        NNGP_REQUIRE(std::isfinite(coef_host[t]), "poly: coefficient of term %d is not finite", t);
        const int16_t *ix = idx_host + 3 * (size_t)t;
        bool ended = false;
        for (int q = 0; q < 3; q++) {
            NNGP_REQUIRE(ix[q] == -1 || (ix[q] >= 0 && ix[q] < d), "poly: term %d has index %d outside [0, d=%d) "
                         "(-1 = no factor)", t, (int)ix[q], d);
            NNGP_REQUIRE(!(ended && ix[q] != -1), "poly: term %d has a factor after a -1 (the real indices come first)", t);
            ended = ended || ix[q] == -1;
        }
        terms[t] = PolyTerm{coef_host[t], ix[0], ix[1], ix[2], 0};
    }
    std::lock_guard<std::mutex> lk(g_poly_mu);
    size_t slot = 0;
    while (slot < g_poly.size() && g_poly[slot].live) slot++;   // a freed slot is reused
    if (slot == g_poly.size()) g_poly.emplace_back();
    PolyEntry &e = g_poly[slot];
    e.live = true;
    e.d = d;
    e.row_ptr.assign(row_ptr_host, row_ptr_host + d + 1);
    e.terms.swap(terms);
    *handle_out = (int32_t)slot + 1;
    return NNGP_OK;
}

extern "C" int nngp_poly_destroy(int32_t handle) {
    using namespace nngp;
    std::lock_guard<std::mutex> lk(g_poly_mu);
    NNGP_REQUIRE(handle >= 1 && handle <= (int32_t)g_poly.size() && g_poly[handle - 1].live,
                 "poly: unknown or destroyed table handle %d", (int)handle);
    PolyEntry &e = g_poly[handle - 1];
    poly_free_devs(e);
    e = PolyEntry{};
    return NNGP_OK;
}
