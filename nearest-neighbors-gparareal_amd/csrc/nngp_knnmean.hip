// nngp_knnmean.hip -- the k-NN Parareal correction: the plain average of the m nearest neighbours'
// F - G rows.
//
// Reference: Figure_2.py:455-475 (NN.predict): argsort of cdist(new_x, x, 'sqeuclidean'), the first
// nn rows of y, ym.mean(axis=0).  Here (restated in tests/knnmean_ref.py):
//   knn_dist_kernel      nngp_gp.hip's kernel (declared in nngp_knn_dev.h), batched over queries by
//                        blockIdx.y: the batched entry point's distances, spread over the device;
//   knnmean_kernel<K, FUSED>  one workgroup of 256 threads per query (blockIdx.y): the ordered select
//                        (knn_select_dev<K>, nngp_knn's own device code and LDS key cache, so the
//                        neighbour list is nngp_knn's by construction), then thread c walks the
//                        selected rows once for the coordinates c, c + 256, ..: s = Y[i_0][c],
//                        s = s + Y[i_r][c] in list order, and s / m_j is stored whenever the row count
//                        reaches one of the requested counts m_j (kernel arguments, no table).
// The sweep's form (FUSED) computes its one query's distances in the same launch, which keeps a
// slice at two launches: G, then this kernel.  The grid then has one workgroup per 64 rows; each
// computes its rows' distances (knn_dist_kernel's shape), counts itself on a device counter, and the
// workgroup that arrives last -- after every other's distances are visible -- runs the select and the
// mean.  No workgroup waits for another, so the launch needs no co-residency.  (One workgroup
// computing all distances itself was tried first: at d = 800, rows = 1 024 a slice took 306 us with
// the loads straight from memory and 478 us through LDS tiles, against 77 us in this form -- a single
// CU's loads in flight bound it.  Development runs, not kept in a profile file.)  The batched form is
// its own instantiation, so it does not carry the distance body's registers.
#include <algorithm>

#include "common.h"
#include "nngp_knn_dev.h"

namespace nngp {

constexpr int KNNMEAN_MAX_M = 64;        // the select's bound (SelShm)
constexpr int KNNMEAN_MAX_COUNTS = 16;
constexpr int KNNMEAN_MAX_Q = 65535;     // gridDim.y

struct KnnMeanArgs {
    const double *X, *Y;       // [rows][d]
    int64_t rows;
    int d;
    const double *Q;           // [n_q][d]
    int n_q;
    double *dist;              // workspace [n_q][rows]
    int32_t *idx;              // [n_q][m_max]: the caller's idx_out or workspace
    int m_max;
    double *out;               // [n_m][n_q][d] or null
    const double *bias;        // [d] or null (n_q == n_m == 1)
    double *out_biased;        // [d] = mean + bias
    int key_lds;               // K = 0: the keys staged in the dynamic LDS
    unsigned *counter;         // FUSED: workgroups that have finished their distances (0 between launches)
    uint64_t want;             // bit r: some count equals r + 1
    int n_m;
    int32_t m[KNNMEAN_MAX_COUNTS];
};

// FUSED: the launch computes its (one) query's distances itself, 64 rows per workgroup
template <int K, bool FUSED>
__global__ void __launch_bounds__(256) knnmean_kernel(const KnnMeanArgs a) {
    __shared__ SelShm sh;
    const int qy = blockIdx.y, tid = threadIdx.x;
    const int d = a.d, m_max = a.m_max;
    const double *q = a.Q + (size_t)qy * d;
    double *dist = a.dist + (size_t)qy * a.rows;
    if constexpr (FUSED) {
        __shared__ int s_last;
        const int64_t r = (int64_t)blockIdx.x * 64 + tid;
        if (tid < 64 && r < a.rows) dist[r] = knn_dist_row(a.X, d, q, r);
        __threadfence();   // this thread's distances, device-wide, before the workgroup is counted
        __syncthreads();
        if (tid == 0) {
            const unsigned prev = __hip_atomic_fetch_add(a.counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            s_last = prev + 1 == gridDim.x;
            if (s_last) __hip_atomic_store(a.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // for the next launch
        }
        __syncthreads();
        if (!s_last) return;   // uniform
        __threadfence();       // the other workgroups' distances before the select reads them
    }
    knn_select_dev<K, false>(sh, dist, a.rows, m_max, a.X, nullptr, d, q, a.idx + (size_t)qy * m_max, nullptr, nullptr,
                             nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr,
                             K == 0 && a.key_lds != 0);
    // the select ends on a barrier with the ordered list in sh.sel[0 .. m_max)
    constexpr int RB = 8;   // rows whose loads are in flight together
    const size_t qd = (size_t)a.n_q * d;
    for (int c = tid; c < d; c += 256) {
        double s = 0.0;
        for (int r0 = 0; r0 < m_max; r0 += RB) {
            double y[RB];
#pragma unroll
            for (int u = 0; u < RB; u++)
                if (r0 + u < m_max) y[u] = a.Y[(int64_t)sh.sel[r0 + u] * d + c];
#pragma unroll
            for (int u = 0; u < RB; u++) {
                const int r = r0 + u;
                if (r >= m_max) break;
                s = r == 0 ? y[u] : s + y[u];
                if ((a.want >> r) & 1) {   // uniform
                    const double mean = s / (double)(r + 1);
                    for (int j = 0; j < a.n_m; j++)
                        if (a.m[j] == r + 1) {
                            if (a.out) a.out[(size_t)j * qd + (size_t)qy * d + c] = mean;
                            if (a.out_biased) a.out_biased[c] = mean + a.bias[c];
                        }
                }
            }
        }
    }
}

template <bool FUSED>
static void knnmean_launch(const KnnMeanArgs &a, hipStream_t st) {
    // the select's form by ceil(rows / 256), as nngp_knn's launcher picks it
    const int64_t per = (a.rows + 255) / 256;
    const dim3 grid(FUSED ? (unsigned)((a.rows + 63) / 64) : 1u, (unsigned)a.n_q);
    const size_t shmem = a.key_lds ? (size_t)a.rows * sizeof(uint64_t) : 0;
    if (per <= 2)
        hipLaunchKernelGGL((knnmean_kernel<2, FUSED>), grid, dim3(256), shmem, st, a);
    else if (per <= 4)
        hipLaunchKernelGGL((knnmean_kernel<4, FUSED>), grid, dim3(256), shmem, st, a);
    else if (per <= 8)
        hipLaunchKernelGGL((knnmean_kernel<8, FUSED>), grid, dim3(256), shmem, st, a);
    else if (per <= 16)
        hipLaunchKernelGGL((knnmean_kernel<16, FUSED>), grid, dim3(256), shmem, st, a);
    else
        hipLaunchKernelGGL((knnmean_kernel<0, FUSED>), grid, dim3(256), shmem, st, a);
}

static int knnmean_check(const double *X, const double *Y, int64_t rows, int d) {
    NNGP_REQUIRE(X != nullptr, "X is NULL");
    NNGP_REQUIRE(Y != nullptr, "Y is NULL");
    NNGP_REQUIRE(d >= 1, "d must be >= 1 (got %d)", d);
    NNGP_REQUIRE(rows >= 1, "rows must be >= 1 (got %lld)", (long long)rows);
    return NNGP_OK;
}

static int knnmean_check_m(int m, int64_t rows) {
    NNGP_REQUIRE(m >= 1 && m <= KNNMEAN_MAX_M && m <= rows, "m must be in 1..min(%d, rows) (m=%d rows=%lld)",
                 KNNMEAN_MAX_M, m, (long long)rows);
    return NNGP_OK;
}

// the counts into the kernel's arguments, and the form of the select
static void knnmean_counts(KnnMeanArgs &a, const int32_t *m_host, int n_m) {
    a.n_m = n_m;
    a.m_max = 0;
    a.want = 0;
    for (int j = 0; j < KNNMEAN_MAX_COUNTS; j++) a.m[j] = 0;
    for (int j = 0; j < n_m; j++) {
        a.m[j] = m_host[j];
        a.m_max = std::max(a.m_max, (int)m_host[j]);
        a.want |= 1ull << (m_host[j] - 1);
    }
    const int64_t per = (a.rows + 255) / 256;
    a.key_lds = (per > 16 && a.rows <= KEY_LDS_ROWS && env_int("NNGP_KEY_LDS", 1) != 0) ? 1 : 0;
}

}  // namespace nngp

using namespace nngp;

extern "C" int nngp_knn_mean(const double *X, const double *Y, int64_t rows, int d, const double *Q, int n_q,
                             const int32_t *m_host, int n_m, double *out, int32_t *idx_out, const double *bias,
                             double *out_biased, void *stream) {
    int rc = knnmean_check(X, Y, rows, d);
    if (rc) return rc;
    NNGP_REQUIRE(Q != nullptr, "Q is NULL");
    NNGP_REQUIRE(m_host != nullptr, "m_host is NULL");
    NNGP_REQUIRE(out != nullptr, "out is NULL");
    NNGP_REQUIRE(n_m >= 1 && n_m <= KNNMEAN_MAX_COUNTS, "n_m must be in 1..%d (got %d)", KNNMEAN_MAX_COUNTS, n_m);
    for (int j = 0; j < n_m; j++)
        if ((rc = knnmean_check_m(m_host[j], rows)) != NNGP_OK) return rc;
    NNGP_REQUIRE(n_q >= 0 && n_q <= KNNMEAN_MAX_Q, "n_q must be in 0..%d (got %d)", KNNMEAN_MAX_Q, n_q);
    NNGP_REQUIRE((bias == nullptr) == (out_biased == nullptr), "bias and out_biased go together");
    NNGP_REQUIRE(!bias || (int64_t)n_q * n_m == 1, "bias needs n_q == n_m == 1 (n_q=%d n_m=%d)", n_q, n_m);
    if (n_q == 0) return NNGP_OK;
    hipStream_t st = (hipStream_t)stream;
    KnnMeanArgs a;
    a.X = X; a.Y = Y; a.rows = rows; a.d = d; a.Q = Q; a.n_q = n_q;
    knnmean_counts(a, m_host, n_m);
    // slot-0 workspace: dist [n_q][rows] | idx [n_q][m_max] (when the caller wants no list)
    int err = 0;
    const size_t dist_bytes = sizeof(double) * (size_t)n_q * (size_t)rows;
    char *ws = (char *)workspace(dist_bytes + sizeof(int32_t) * (size_t)n_q * KNNMEAN_MAX_M, &err);
    if (err) return err;
    a.dist = (double *)ws;
    a.idx = idx_out ? idx_out : (int32_t *)(ws + dist_bytes);
    a.out = out; a.bias = bias; a.out_biased = out_biased;
    a.counter = nullptr;
    hipLaunchKernelGGL(knn_dist_kernel, dim3((unsigned)((rows + 63) / 64), (unsigned)n_q), dim3(64), 0, st, X, rows,
                       d, Q, a.dist);
    NNGP_LAUNCH_CHECK();
    knnmean_launch<false>(a, st);
    NNGP_LAUNCH_CHECK();
    return NNGP_OK;
}

extern "C" int nngp_knn_mean_sweep(const nngp_system *sys, int g_tableau, int g_step_mode, int64_t g_steps,
                                   const double *t, int I, int N, double *U1, double *UG1, const double *X,
                                   const double *Y, int64_t rows, int m, double *preds, float *g_ms_out,
                                   void *stream) {
    NNGP_REQUIRE(sys != nullptr, "sys is NULL");
    NNGP_REQUIRE(t != nullptr, "t is NULL");
    NNGP_REQUIRE(U1 != nullptr, "U1 is NULL");
    NNGP_REQUIRE(UG1 != nullptr, "UG1 is NULL");
    const int d = sys->d;
    int rc = knnmean_check(X, Y, rows, d);
    if (rc) return rc;
    if ((rc = knnmean_check_m(m, rows)) != NNGP_OK) return rc;
    NNGP_REQUIRE(I >= 0, "I must be >= 0 (got %d)", I);
    GTimer gt;   // (N < I: an empty sweep)
    if ((rc = gt.begin(g_ms_out, (int64_t)N - I, g_time_stride())) != NNGP_OK) return rc;
    if (N <= I) return NNGP_OK;
    const Coarse G{sys, g_tableau, g_step_mode, g_steps, t};
    hipStream_t st = (hipStream_t)stream;
    KnnMeanArgs a;
    a.X = X; a.Y = Y; a.rows = rows; a.d = d; a.n_q = 1;
    const int32_t m32 = m;
    knnmean_counts(a, &m32, 1);
    int err = 0;
    const size_t dist_bytes = sizeof(double) * (size_t)rows;
    // slot-0 workspace: dist [rows] | idx [64] | the workgroup counter
    char *ws = (char *)workspace(dist_bytes + sizeof(int32_t) * (KNNMEAN_MAX_M + 1), &err);
    if (err) return err;
    a.dist = (double *)ws;
    a.idx = (int32_t *)(ws + dist_bytes);
    a.counter = (unsigned *)(a.idx + KNNMEAN_MAX_M);
    NNGP_HIP_CHECK(hipMemsetAsync(a.counter, 0, sizeof(unsigned), st));   // once per sweep: every launch leaves 0
    for (int i = I; i < N; i++) {
        const size_t j = (size_t)(i - I);
        const double *ui = U1 + (size_t)i * d;
        double *ug_next = UG1 + (size_t)(i + 1) * d;
        if ((rc = gt.launch(G, i, j, ui, ug_next, st)) != NNGP_OK) return rc;
        a.Q = ui;
        a.out = preds ? preds + j * (size_t)d : nullptr;
        a.bias = ug_next;
        a.out_biased = U1 + (size_t)(i + 1) * d;
        knnmean_launch<true>(a, st);
        NNGP_LAUNCH_CHECK();
    }
    return gt.finish();
}
