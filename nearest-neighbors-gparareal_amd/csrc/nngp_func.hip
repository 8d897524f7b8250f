// nngp_func.hip -- registry of the fields with elementary-function atoms (NNGP_SYS_FUNC,
// include/nngp.h): nngp_func_create / nngp_func_destroy and the lookups the
// propagator dispatch uses (common.h).  Host code only, as nngp_poly.hip: the kernels that evaluate
// a table are the lane and field propagators of nngp_rk_kernels.h.
//
// A table is the polynomial field's d rows of ordered terms, their indices over the extended vector
// [u_0 .. u_{d-1}, atom_0 .. atom_{n_atoms-1}], and n_atoms atom records fn(a u[i] (+ c u[j]) (+ b)).
// The kernels trust a registered table -- they index the state and the image with its indices and
// switch on its function ids without a check -- so everything is checked here, on the host, before
// any HIP call.
#include <cmath>
#include <mutex>
#include <vector>

#include "common.h"

namespace nngp {

struct FuncDev {
    int dev;
    void *block;   // terms [n_terms] (16-byte records first) | atoms [n_atoms] (8-byte aligned) | row_ptr [d+1]
};
struct FuncEntry {
    bool live = false;
    int d = 0;
    std::vector<int32_t> row_ptr;
    std::vector<PolyTerm> terms;
    std::vector<nngp_func_atom> atoms;
    std::vector<FuncDev> devs;
};
static std::vector<FuncEntry> g_func;   // handle = index + 1
static std::mutex g_func_mu;

static void func_free_devs(FuncEntry &e) {
    for (FuncDev &p : e.devs)
        if (p.block) (void)hipFree(p.block);   // implicit device synchronisation: no launch still reads it
    e.devs.clear();
}

static FuncEntry *func_entry(const nngp_system *sys) {
    const int h = sys->nx;
    if (h < 1 || h > (int)g_func.size() || !g_func[h - 1].live) {
        set_error("func: unknown or destroyed table handle %d (nngp_system.nx holds the handle of nngp_func_create)", h);
        return nullptr;
    }
    FuncEntry *e = &g_func[h - 1];
    if (sys->d != e->d) {
        set_error("func: system has d=%d but table %d was created with d=%d", sys->d, h, e->d);
        return nullptr;
    }
    return e;
}

int func_table(const nngp_system *sys, FuncTable *out) {
    std::lock_guard<std::mutex> lk(g_func_mu);
    FuncEntry *e = func_entry(sys);
    if (!e) return NNGP_E_ARG;
    out->d = e->d;
    out->n_atoms = (int)e->atoms.size();
    out->n_terms = (int)e->terms.size();
    out->row_ptr = e->row_ptr.data();
    out->terms = e->terms.data();
    out->atoms = e->atoms.data();
    return NNGP_OK;
}

int func_device(const nngp_system *sys, const int32_t **row_ptr, const PolyTerm **terms,
                const nngp_func_atom **atoms) {
    std::lock_guard<std::mutex> lk(g_func_mu);
    FuncEntry *e = func_entry(sys);
    if (!e) return NNGP_E_ARG;
    int dev = 0;
    NNGP_HIP_CHECK(hipGetDevice(&dev));
    void *block = nullptr;
    for (const FuncDev &p : e->devs)
        if (p.dev == dev) block = p.block;
    const size_t tbytes = sizeof(PolyTerm) * e->terms.size(), abytes = sizeof(nngp_func_atom) * e->atoms.size(),
                 rbytes = sizeof(int32_t) * e->row_ptr.size();
    if (!block) {
        NNGP_HIP_CHECK(hipMalloc(&block, tbytes + abytes + rbytes));
        hipError_t err = hipSuccess;
        if (tbytes) err = hipMemcpy(block, e->terms.data(), tbytes, hipMemcpyHostToDevice);
        if (err == hipSuccess && abytes)
            err = hipMemcpy((char *)block + tbytes, e->atoms.data(), abytes, hipMemcpyHostToDevice);
        if (err == hipSuccess)
            err = hipMemcpy((char *)block + tbytes + abytes, e->row_ptr.data(), rbytes, hipMemcpyHostToDevice);
        if (err != hipSuccess) {
            (void)hipFree(block);
            set_error("func: upload of table %d failed: %s", sys->nx, hipGetErrorString(err));
            return NNGP_E_HIP;
        }
        e->devs.push_back(FuncDev{dev, block});
    }
    *terms = (const PolyTerm *)block;
    *atoms = (const nngp_func_atom *)((const char *)block + tbytes);
    *row_ptr = (const int32_t *)((const char *)block + tbytes + abytes);
    return NNGP_OK;
}

void func_release() {
    std::lock_guard<std::mutex> lk(g_func_mu);
    for (FuncEntry &e : g_func) func_free_devs(e);
    g_func.clear();
}

}  // namespace nngp

extern "C" int nngp_func_create(int d, int n_atoms, const nngp_func_atom *atoms_host, int n_terms,
                                const int32_t *row_ptr_host, const double *coef_host, const int16_t *idx_host,
                                int32_t *handle_out) {
    using namespace nngp;
    static_assert(sizeof(nngp_func_atom) == 40, "nngp_func_atom is 4 int32 + 3 doubles, no padding");
    NNGP_REQUIRE(handle_out != nullptr, "func: handle_out is NULL");
    NNGP_REQUIRE(d >= 1 && d <= POLY_MAX_D, "func: d=%d outside 1..%d", d, POLY_MAX_D);
    NNGP_REQUIRE(n_atoms >= 0 && n_atoms <= FUNC_MAX_ATOMS, "func: n_atoms=%d outside 0..%d", n_atoms,
                 FUNC_MAX_ATOMS);
    NNGP_REQUIRE(n_terms >= 0 && n_terms <= POLY_MAX_TERMS, "func: n_terms=%d outside 0..%d", n_terms,
                 POLY_MAX_TERMS);
    NNGP_REQUIRE(n_atoms == 0 || atoms_host != nullptr, "func: atoms is NULL");
    NNGP_REQUIRE(row_ptr_host != nullptr, "func: row_ptr is NULL");
    NNGP_REQUIRE(n_terms == 0 || (coef_host != nullptr && idx_host != nullptr), "func: coef / idx is NULL");
    for (int q = 0; q < n_atoms; q++) {
        const nngp_func_atom &A = atoms_host[q];
        NNGP_REQUIRE(A.fn >= NNGP_FN_SIN && A.fn <= NNGP_FN_SQRT, "func: atom %d has function id %d outside 1..6 "
                     "(sin, cos, exp, log, recip, sqrt)", q, (int)A.fn);
        NNGP_REQUIRE(A.i >= 0 && A.i < d, "func: atom %d has state index i=%d outside [0, d=%d)", q, (int)A.i, d);
        NNGP_REQUIRE(A.j == -1 || (A.j >= 0 && A.j < d), "func: atom %d has state index j=%d outside [0, d=%d) "
                     "(-1 = no second component)", q, (int)A.j, d);
        NNGP_REQUIRE(A.has_b == 0 || A.has_b == 1, "func: atom %d has has_b=%d (0 or 1)", q, (int)A.has_b);
        NNGP_REQUIRE(std::isfinite(A.a) && std::isfinite(A.c) && std::isfinite(A.b),
                     "func: atom %d has a coefficient (a, c or b) that is not finite", q);
    }
    NNGP_REQUIRE(row_ptr_host[0] == 0, "func: row_ptr[0] = %d, must be 0", row_ptr_host[0]);
    for (int c = 0; c < d; c++)
        NNGP_REQUIRE(row_ptr_host[c + 1] >= row_ptr_host[c] && row_ptr_host[c + 1] <= n_terms,
                     "func: row_ptr must be non-decreasing and end at n_terms=%d (row_ptr[%d] = %d, row_ptr[%d] = %d)",
                     n_terms, c, row_ptr_host[c], c + 1, row_ptr_host[c + 1]);
    NNGP_REQUIRE(row_ptr_host[d] == n_terms, "func: row_ptr[d] = %d, must be n_terms = %d", row_ptr_host[d], n_terms);
    const int nw = d + n_atoms;
    std::vector<PolyTerm> terms((size_t)n_terms);
    for (int t = 0; t < n_terms; t++) {
        NNGP_REQUIRE(std::isfinite(coef_host[t]), "func: coefficient of term %d is not finite", t);
        const int16_t *ix = idx_host + 3 * (size_t)t;
        bool ended = false;
        for (int q = 0; q < 3; q++) {
            NNGP_REQUIRE(ix[q] == -1 || (ix[q] >= 0 && ix[q] < nw), "func: term %d has index %d outside "
                         "[0, d + n_atoms = %d) (-1 = no factor)", t, (int)ix[q], nw);
            NNGP_REQUIRE(!(ended && ix[q] != -1), "func: term %d has a factor after a -1 (the real indices come first)", t);
            ended = ended || ix[q] == -1;
        }
        terms[t] = PolyTerm{coef_host[t], ix[0], ix[1], ix[2], 0};
    }
    std::lock_guard<std::mutex> lk(g_func_mu);
    size_t slot = 0;
    while (slot < g_func.size() && g_func[slot].live) slot++;   // a freed slot is reused
    if (slot == g_func.size()) g_func.emplace_back();
    FuncEntry &e = g_func[slot];
    e.live = true;
    e.d = d;
    e.row_ptr.assign(row_ptr_host, row_ptr_host + d + 1);
    e.terms.swap(terms);
    e.atoms.assign(atoms_host, atoms_host + n_atoms);
    *handle_out = (int32_t)slot + 1;
    return NNGP_OK;
}

extern "C" int nngp_func_destroy(int32_t handle) {
    using namespace nngp;
    std::lock_guard<std::mutex> lk(g_func_mu);
    NNGP_REQUIRE(handle >= 1 && handle <= (int32_t)g_func.size() && g_func[handle - 1].live,
                 "func: unknown or destroyed table handle %d", (int)handle);
    FuncEntry &e = g_func[handle - 1];
    func_free_devs(e);
    e = FuncEntry{};
    return NNGP_OK;
}
