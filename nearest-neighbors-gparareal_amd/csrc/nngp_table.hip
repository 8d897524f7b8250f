// nngp_table.hip -- registry of the table-backed vector fields: the polynomial fields (NNGP_SYS_POLY,
// DESIGN.md 3.2c) and the fields with elementary-function atoms (NNGP_SYS_FUNC).
// nngp_poly_create / nngp_func_create, their destroy calls, and the lookups the propagator dispatch
// uses (common.h).  Host code only: the kernels that evaluate a table are the lane and field
// propagators of nngp_rk_kernels.h.
//
// The reference's extension point is a subclass of ODE with its own _f_np / _f_jax
// (systems.py:23-61).  Here the right-hand side is data: d rows of ordered terms (coef, up to three
// indices) over the extended vector [u_0 .. u_{d-1}, atom_0 .. atom_{n_atoms-1}], and n_atoms atom
// records fn(a u[i] (+ c u[j]) (+ b)).  A polynomial table is one without atoms; the two kinds share
// everything here but their handle spaces, which are two instances of one registry.  The kernels
// trust a registered table -- they index the state and the image with its indices, walk its rows and
// switch on its function ids without a check -- so everything is checked here, on the host, before
// any HIP call.
#include <cmath>
#include <mutex>
#include <vector>

#include "common.h"

namespace nngp {

struct TableDev {
    int dev;
    // terms [n_terms] (16-byte records first, for their alignment) | atoms [n_atoms] (8-byte aligned) |
    // row_ptr [d+1]; without atoms the polynomial field's terms | row_ptr
    void *block;
};
struct TableEntry {
    bool live = false;
    int d = 0;
    std::vector<int32_t> row_ptr;
    std::vector<PolyTerm> terms;
    std::vector<nngp_func_atom> atoms;
    std::vector<TableDev> devs;

    void free_devs() {
        for (TableDev &p : devs)
            if (p.block) (void)hipFree(p.block);   // implicit device synchronisation: no launch still reads it
        devs.clear();
    }
};
struct Registry {
    const char *tag;                  // "poly" / "func": of the messages, and of nngp_<tag>_create
    std::mutex mu;
    std::vector<TableEntry> slots;    // handle = index + 1

    TableEntry *live(int h) { return h >= 1 && h <= (int)slots.size() && slots[h - 1].live ? &slots[h - 1] : nullptr; }
    // the entry of sys->nx after checking it against sys->d (mu held)
    TableEntry *entry(const nngp_system *sys) {
        TableEntry *e = live(sys->nx);
        if (!e)
            set_error("%s: unknown or destroyed table handle %d (nngp_system.nx holds the handle of nngp_%s_create)",
                      tag, sys->nx, tag);
        else if (sys->d != e->d) {
            set_error("%s: system has d=%d but table %d was created with d=%d", tag, sys->d, sys->nx, e->d);
            e = nullptr;
        }
        return e;
    }
    void release() {
        std::lock_guard<std::mutex> lk(mu);
        for (TableEntry &e : slots) e.free_devs();
        slots.clear();
    }
};
static Registry g_poly{"poly"}, g_func{"func"};
static Registry &registry_of(const nngp_system *sys) { return sys->kind == NNGP_SYS_FUNC ? g_func : g_poly; }

int table_lookup(const nngp_system *sys, Table *out) {
    Registry &R = registry_of(sys);
    std::lock_guard<std::mutex> lk(R.mu);
    TableEntry *e = R.entry(sys);
    if (!e) return NNGP_E_ARG;
    *out = Table{e->d, (int)e->atoms.size(), (int)e->terms.size(), e->row_ptr.data(), e->terms.data(), e->atoms.data()};
    return NNGP_OK;
}

int table_device(const nngp_system *sys, const int32_t **row_ptr, const PolyTerm **terms, int *n_atoms) {
    Registry &R = registry_of(sys);
    std::lock_guard<std::mutex> lk(R.mu);
    TableEntry *e = R.entry(sys);
    if (!e) return NNGP_E_ARG;
    int dev = 0;
    NNGP_HIP_CHECK(hipGetDevice(&dev));
    void *block = nullptr;
    for (const TableDev &p : e->devs)
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
            set_error("%s: upload of table %d failed: %s", R.tag, sys->nx, hipGetErrorString(err));
            return NNGP_E_HIP;
        }
        e->devs.push_back(TableDev{dev, block});
    }
    *terms = (const PolyTerm *)block;
    *row_ptr = (const int32_t *)((const char *)block + tbytes + abytes);
    *n_atoms = (int)e->atoms.size();
    return NNGP_OK;
}

void table_release() {
    g_poly.release();
    g_func.release();
}

// validates a table and registers it in R; n_atoms = 0 and atoms_host = NULL for a polynomial field
static int table_create(Registry &R, int d, int n_atoms, const nngp_func_atom *atoms_host, int n_terms,
                        const int32_t *row_ptr_host, const double *coef_host, const int16_t *idx_host,
                        int32_t *handle_out) {
    static_assert(sizeof(nngp_func_atom) == 40, "nngp_func_atom is 4 int32 + 3 doubles, no padding");
    const char *tag = R.tag;
    NNGP_REQUIRE(handle_out != nullptr, "%s: handle_out is NULL", tag);
    NNGP_REQUIRE(d >= 1 && d <= POLY_MAX_D, "%s: d=%d outside 1..%d", tag, d, POLY_MAX_D);
    NNGP_REQUIRE(n_atoms >= 0 && n_atoms <= FUNC_MAX_ATOMS, "%s: n_atoms=%d outside 0..%d", tag, n_atoms,
                 FUNC_MAX_ATOMS);
    NNGP_REQUIRE(n_terms >= 0 && n_terms <= POLY_MAX_TERMS, "%s: n_terms=%d outside 0..%d", tag, n_terms,
                 POLY_MAX_TERMS);
    NNGP_REQUIRE(n_atoms == 0 || atoms_host != nullptr, "%s: atoms is NULL", tag);
    NNGP_REQUIRE(row_ptr_host != nullptr, "%s: row_ptr is NULL", tag);
    NNGP_REQUIRE(n_terms == 0 || (coef_host != nullptr && idx_host != nullptr), "%s: coef / idx is NULL", tag);
    for (int q = 0; q < n_atoms; q++) {
        const nngp_func_atom &A = atoms_host[q];
        NNGP_REQUIRE(A.fn >= NNGP_FN_SIN && A.fn <= NNGP_FN_SQRT, "%s: atom %d has function id %d outside 1..6 "
                     "(sin, cos, exp, log, recip, sqrt)", tag, q, (int)A.fn);
        NNGP_REQUIRE(A.i >= 0 && A.i < d, "%s: atom %d has state index i=%d outside [0, d=%d)", tag, q, (int)A.i, d);
        NNGP_REQUIRE(A.j == -1 || (A.j >= 0 && A.j < d), "%s: atom %d has state index j=%d outside [0, d=%d) "
                     "(-1 = no second component)", tag, q, (int)A.j, d);
        NNGP_REQUIRE(A.has_b == 0 || A.has_b == 1, "%s: atom %d has has_b=%d (0 or 1)", tag, q, (int)A.has_b);
        NNGP_REQUIRE(std::isfinite(A.a) && std::isfinite(A.c) && std::isfinite(A.b),
                     "%s: atom %d has a coefficient (a, c or b) that is not finite", tag, q);
    }
    NNGP_REQUIRE(row_ptr_host[0] == 0, "%s: row_ptr[0] = %d, must be 0", tag, row_ptr_host[0]);
    for (int c = 0; c < d; c++)
        NNGP_REQUIRE(row_ptr_host[c + 1] >= row_ptr_host[c] && row_ptr_host[c + 1] <= n_terms,
                     "%s: row_ptr must be non-decreasing and end at n_terms=%d (row_ptr[%d] = %d, row_ptr[%d] = %d)",
                     tag, n_terms, c, row_ptr_host[c], c + 1, row_ptr_host[c + 1]);
    NNGP_REQUIRE(row_ptr_host[d] == n_terms, "%s: row_ptr[d] = %d, must be n_terms = %d", tag, row_ptr_host[d],
                 n_terms);
    const int nw = d + n_atoms;
    std::vector<PolyTerm> terms((size_t)n_terms);
    for (int t = 0; t < n_terms; t++) {
        NNGP_REQUIRE(std::isfinite(coef_host[t]), "%s: coefficient of term %d is not finite", tag, t);
        const int16_t *ix = idx_host + 3 * (size_t)t;
        bool ended = false;
        for (int q = 0; q < 3; q++) {
            NNGP_REQUIRE(ix[q] == -1 || (ix[q] >= 0 && ix[q] < nw), "%s: term %d has index %d outside "
                         "[0, d + n_atoms = %d) (-1 = no factor)", tag, t, (int)ix[q], nw);
            NNGP_REQUIRE(!(ended && ix[q] != -1), "%s: term %d has a factor after a -1 (the real indices come first)",
                         tag, t);
            ended = ended || ix[q] == -1;
        }
        terms[t] = PolyTerm{coef_host[t], ix[0], ix[1], ix[2], 0};
    }
    std::lock_guard<std::mutex> lk(R.mu);
    size_t slot = 0;
    while (slot < R.slots.size() && R.slots[slot].live) slot++;   // a freed slot is reused
    if (slot == R.slots.size()) R.slots.emplace_back();
    TableEntry &e = R.slots[slot];
    e.live = true;
    e.d = d;
    e.row_ptr.assign(row_ptr_host, row_ptr_host + d + 1);
    e.terms.swap(terms);
    e.atoms.assign(atoms_host, atoms_host + n_atoms);
    *handle_out = (int32_t)slot + 1;
    return NNGP_OK;
}

static int table_destroy(Registry &R, int32_t handle) {
    std::lock_guard<std::mutex> lk(R.mu);
    TableEntry *e = R.live(handle);
    NNGP_REQUIRE(e != nullptr, "%s: unknown or destroyed table handle %d", R.tag, (int)handle);
    e->free_devs();
    *e = TableEntry{};
    return NNGP_OK;
}

}  // namespace nngp

extern "C" int nngp_poly_create(int d, int n_terms, const int32_t *row_ptr_host, const double *coef_host,
                                const int16_t *idx_host, int32_t *handle_out) {
    return nngp::table_create(nngp::g_poly, d, 0, nullptr, n_terms, row_ptr_host, coef_host, idx_host, handle_out);
}

extern "C" int nngp_func_create(int d, int n_atoms, const nngp_func_atom *atoms_host, int n_terms,
                                const int32_t *row_ptr_host, const double *coef_host, const int16_t *idx_host,
                                int32_t *handle_out) {
    return nngp::table_create(nngp::g_func, d, n_atoms, atoms_host, n_terms, row_ptr_host, coef_host, idx_host,
                              handle_out);
}

extern "C" int nngp_poly_destroy(int32_t handle) { return nngp::table_destroy(nngp::g_poly, handle); }
extern "C" int nngp_func_destroy(int32_t handle) { return nngp::table_destroy(nngp::g_func, handle); }
