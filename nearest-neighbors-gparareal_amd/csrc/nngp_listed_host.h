// nngp_listed_host.h -- the host side of the prescribed-list entries (nngp_predict_listed,
// nngp_listed_sweep; kernels and launches in nngp_gp.hip) that touches caller memory before any HIP
// call: the argument checks, the walk over lists_host, and the workspace layouts the lists are
// uploaded into.  No HIP call and no device code here, so the same functions run in a stand-alone
// host program under -fsanitize=address,undefined (tests/host/listed_host_check.cpp, `make check-listed`).
#pragma once

#include "common.h"

namespace nngp {

// every entry of lists_host[n][m] is a training row: checked on the host, so a bad list is an
// argument error and never a device fault
inline int check_lists(const int32_t *lists_host, int64_t n, int m, int64_t rows) {
    for (int64_t q = 0; q < n; q++)
        for (int r = 0; r < m; r++) {
            const int32_t v = lists_host[q * m + r];
            NNGP_REQUIRE(v >= 0 && v < rows, "lists_host[%lld][%d] = %d is not a training row (rows=%lld)",
                         (long long)q, r, (int)v, (long long)rows);
        }
    return NNGP_OK;
}

// the argument checks the two listed entries share (nngp_predict_batch's), then the n lists;
// max_m / max_jit: the fit kernels' bounds (64 neighbours, 16 jitters)
inline int listed_check(const double *X, const double *Y, int64_t rows, int d, const int32_t *lists_host, int64_t n,
                        int m, int n_jitter, const double *jitter_exp_host, int n_restarts, const double *theta0,
                        int maxfev, int max_m, int max_jit) {
    NNGP_REQUIRE(X != nullptr, "X is NULL");
    NNGP_REQUIRE(Y != nullptr, "Y is NULL");
    NNGP_REQUIRE(lists_host != nullptr, "lists_host is NULL");
    NNGP_REQUIRE(jitter_exp_host != nullptr, "jitter_exp_host is NULL");
    NNGP_REQUIRE(theta0 != nullptr, "theta0 is NULL");
    NNGP_REQUIRE(d >= 1, "d must be >= 1 (got %d)", d);
    NNGP_REQUIRE(m >= 1 && m <= max_m && m <= rows, "need 1 <= m <= min(%d, rows) (m=%d rows=%lld)", max_m, m,
                 (long long)rows);
    NNGP_REQUIRE(n_jitter >= 1 && n_jitter <= max_jit, "n_jitter must be in [1, %d] (got %d)", max_jit, n_jitter);
    NNGP_REQUIRE(n_restarts >= 1, "n_restarts must be >= 1 (got %d)", n_restarts);
    NNGP_REQUIRE(maxfev >= 1, "maxfev must be >= 1 (got %d)", maxfev);
    NNGP_REQUIRE((int64_t)d * n_jitter * n_restarts <= INT32_MAX / 4,
                 "d * n_jitter * n_restarts = %lld fits per query is too many", (long long)d * n_jitter * n_restarts);
    return check_lists(lists_host, n, m, rows);
}

// the chunk workspace of nq listed predictions (slot WS_PREDICT_BATCH):
// D2[nq][m*m] | ymT[nq][d*m] | kd2[nq][m] | fits[nq][n_fits][4] | lists[nq][m]
struct ListedWs {
    double *D2, *ymT, *kd2, *fits; int32_t *lists; size_t bytes;
};
inline ListedWs listed_ws_carve(char *base, int64_t nq, int d, int m, int64_t n_fits) {
    Carver c{base};
    const size_t q = (size_t)nq;
    ListedWs w{c.take<double>(q * m * m), c.take<double>(q * d * m), c.take<double>(q * m),
               c.take<double>(q * (size_t)n_fits * 4), c.take<int32_t>(q * m), 0};
    w.bytes = c.off;
    return w;
}

// the sweep's own slot (WS_LISTED_SWEEP), live from the batched fits to the last slice:
// AP[nq][d][HM_STRIDE(maxm)] | kd2[m] | pre_done[nq] | lists[nq][m]
struct ListedSweepWs {
    double *AP, *kd2; int32_t *pre_done, *lists; size_t bytes;
};
inline ListedSweepWs listed_sweep_ws_carve(char *base, int64_t nq, int d, int m, int maxm) {
    Carver c{base};
    const size_t q = (size_t)nq;
    ListedSweepWs w{c.take<double>(q * d * HM_STRIDE(maxm)), c.take<double>((size_t)m), c.take<int32_t>(q),
                    c.take<int32_t>(q * m), 0};
    w.bytes = c.off;
    return w;
}

}  // namespace nngp
