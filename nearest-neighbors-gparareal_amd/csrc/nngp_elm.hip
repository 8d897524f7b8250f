// nngp_elm.hip -- the ELM (RandNet-Parareal) correction: a random-weights network on the m nearest
// neighbours.
//
// Reference: models.py:476-554 (ELM_base / ELM).  ELM_base.predict (:521-535) takes the m rows of
// the training set nearest to new_x (:526-528), maps them and new_x through
//     X = relu(bias + C @ PolynomialFeatures(degree)(x).T)                 (:507-508, :530-531)
// and fits Ridge(alpha=0) with an intercept on the m hidden rows (:510-511, :533-534): the min-norm
// interpolation through the neighbours.  Here (restated in tests/elm_ref.py):
//   elm_hidden_kernel   the feature map, phi generated on the fly, a chunk of C read once per tile
//                       of rows, in a summation order that depends on nothing but the feature index;
//   elm_solve_kernel    one wave: modified Gram-Schmidt over the neighbours' differences and the
//                       d-long combination of their targets, coalesced over coordinates.
// Training rows get their hidden features once (nngp_elm_hidden, when ELM.fit appends them); a
// prediction computes only the query's row.
#include <algorithm>

#include "common.h"
#include "nngp_elm.h"

namespace nngp {

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double readlane_f64(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// The fixed butterfly of the contract: v = v + v[lane ^ off] for off = 1, 2, 4, 8, 16, 32.  fp64 add
// commutes, so after each level every lane of an aligned block holds the same bits and a mirror
// reaches the partner block like the xor does; the last two levels are (R0 + R1) + (R2 + R3) of the
// four 16-lane row sums.
__device__ __forceinline__ double wave_sum(double v) {
    v = v + dpp_f64<0xB1>(v);    // quad_perm [1,0,3,2]
    v = v + dpp_f64<0x4E>(v);    // quad_perm [2,3,0,1]
    v = v + dpp_f64<0x141>(v);   // row_half_mirror
    v = v + dpp_f64<0x140>(v);   // row_mirror
    const double s01 = readlane_f64(v, 0) + readlane_f64(v, 16);
    const double s23 = readlane_f64(v, 32) + readlane_f64(v, 48);
    return s01 + s23;
}

// start of row i of the degree-2 block: pairs (i, i) .. (i, d-1)
__device__ __forceinline__ int64_t pair_row_start(int64_t i, int64_t d) { return i * d - i * (i - 1) / 2; }

// Partial sums of one chunk of features for one tile of RT rows:
//   part[chunk][row][r] = butterfly over lanes of (sum over the lane's features f = base + lane + 64 k,
//   k ascending, of C[r][f] * phi_f(x_row), starting from 0.0).
// Block = 4 waves; every wave holds phi of its lanes' 16 features for the RT rows in registers (from
// the x rows in LDS) and takes the hidden units r = wave, wave + 4, ..: C[r][chunk] is read once,
// coalesced, for the RT rows.  blockIdx.x = tile + ntiles * chunk: the tiles of a chunk are adjacent
// in dispatch order, so its C lines are shared in L2.  gridDim.y splits the hidden units over more
// workgroups when the rows are few (a prediction's single query row): each recomputes phi.
template <int RT>
__global__ void __launch_bounds__(256) elm_hidden_kernel(const double *__restrict__ X, int64_t rows, int d,
                                                         int degree, int64_t F, const double *__restrict__ C,
                                                         int res, int ntiles, double *__restrict__ part) {
    extern __shared__ double xs[];   // [RT][d]
    const int tile = blockIdx.x % ntiles, chunk = blockIdx.x / ntiles;
    const int64_t row0 = (int64_t)tile * RT;
    const int nr = (int)min((int64_t)RT, rows - row0);
    for (int e = threadIdx.x; e < RT * d; e += 256) {
        const int t = e / d;
        xs[e] = t < nr ? X[(size_t)row0 * d + e] : 0.0;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int KPL = ELM_CHUNK / 64;   // features per lane
    const int64_t f0 = (int64_t)chunk * ELM_CHUNK + lane;
    double phi[KPL][RT];
    int pi = -1, pj = 0;   // the (i, j) of the lane's previous pair feature
#pragma unroll
    for (int k = 0; k < KPL; k++) {
        const int64_t f = f0 + 64 * k;
        if (f >= F) {
#pragma unroll
            for (int t = 0; t < RT; t++) phi[k][t] = 0.0;
        } else if (f == 0) {
#pragma unroll
            for (int t = 0; t < RT; t++) phi[k][t] = 1.0;
        } else if (f <= d) {
#pragma unroll
            for (int t = 0; t < RT; t++) phi[k][t] = xs[t * d + (int)(f - 1)];
        } else {
            if (pi < 0) {   // closed form, then an exact integer fix-up (index arithmetic only)
                const int64_t p = f - 1 - d;
                const double b = 2.0 * d + 1.0;
                int64_t i = (int64_t)((b - sqrt(b * b - 8.0 * (double)p)) * 0.5);
                i = max((int64_t)0, min(i, (int64_t)d - 1));
                while (i + 1 < d && pair_row_start(i + 1, d) <= p) i++;
                while (i > 0 && pair_row_start(i, d) > p) i--;
                pi = (int)i;
                pj = (int)(i + (p - pair_row_start(i, d)));
            } else {        // 64 features on
                pj += 64;
                while (pj >= d) {
                    pj = pj - d + pi + 1;
                    pi++;
                }
            }
#pragma unroll
            for (int t = 0; t < RT; t++) phi[k][t] = xs[t * d + pi] * xs[t * d + pj];
        }
    }
    for (int r = wave + 4 * blockIdx.y; r < res; r += 4 * gridDim.y) {
        const double *Cr = C + (size_t)r * F;
        double acc[RT];
#pragma unroll
        for (int t = 0; t < RT; t++) acc[t] = 0.0;
#pragma unroll
        for (int k = 0; k < KPL; k++) {
            const int64_t f = f0 + 64 * k;
            if (f < F) {
                const double c = Cr[f];
#pragma unroll
                for (int t = 0; t < RT; t++) acc[t] = acc[t] + c * phi[k][t];
            }
        }
#pragma unroll
        for (int t = 0; t < RT; t++) {
            const double v = wave_sum(acc[t]);
            if (lane == 0 && t < nr) part[((size_t)chunk * rows + row0 + t) * res + r] = v;
        }
    }
}

// H[row][r] = relu(bias[r] + (part[0] + part[1] + ..)): the chunk sums in ascending order, left to right
__global__ void __launch_bounds__(256) elm_combine_kernel(const double *__restrict__ part, int nch, int64_t rows,
                                                          int res, const double *__restrict__ bias,
                                                          double *__restrict__ H) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= rows * res) return;
    double tot = part[e];
    for (int c = 1; c < nch; c++) tot = tot + part[(size_t)c * rows * res + e];
    const double pre = bias[e % res] + tot;
    H[e] = pre > 0.0 ? pre : 0.0;
}

// The same sum with a wave per element, for few elements (a prediction's query row: res_size threads
// would each wait for nch dependent loads): the lanes load 64 chunk sums at once, then they are added
// in ascending chunk order.
__global__ void __launch_bounds__(64) elm_combine_wave_kernel(const double *__restrict__ part, int nch, int64_t rows,
                                                              int res, const double *__restrict__ bias,
                                                              double *__restrict__ H) {
    const int64_t e = blockIdx.x;
    const int lane = threadIdx.x;
    const size_t stride = (size_t)rows * res;
    double tot = 0.0;
    for (int c0 = 0; c0 < nch; c0 += 64) {
        const double v = c0 + lane < nch ? part[(size_t)(c0 + lane) * stride + e] : 0.0;
        const int n = min(64, nch - c0);
        for (int u = 0; u < n; u++) {
            const double x = __shfl(v, u);
            tot = (c0 + u == 0) ? x : tot + x;
        }
    }
    const double pre = bias[e % res] + tot;
    if (lane == 0) H[e] = pre > 0.0 ? pre : 0.0;
}

// products in sp[0 .. res), summed in ascending index, left to right, by every lane (LDS broadcast
// reads), so every lane holds the same sum
__device__ __forceinline__ double serial_sum(const double *sp, int res) {
    double s = sp[0];
    for (int k = 1; k < res; k++) s = s + sp[k];
    return s;
}

// One wave: the contract's steps 1-3.  Qw: [m-1][res] scratch for the kept directions q_i.
__global__ void __launch_bounds__(64) elm_solve_kernel(const int32_t *__restrict__ idx, const double *__restrict__ H,
                                                       const double *__restrict__ Y, const double *__restrict__ hq,
                                                       int m, int res, int d, double *__restrict__ Qw,
                                                       const double *__restrict__ bias, double *__restrict__ preds,
                                                       double *__restrict__ out) {
    __shared__ double sr[ELM_MAX_RES], sv[ELM_MAX_RES], sp[ELM_MAX_RES];
    __shared__ double cm[ELM_MAX_M][ELM_MAX_M], ssq[ELM_MAX_M], sw[ELM_MAX_M], gl[ELM_MAX_M][64];
    __shared__ int skept[ELM_MAX_M];
    const int lane = threadIdx.x;
    const int64_t i0 = idx[0];
    const double *h0 = H + (size_t)i0 * res;
    for (int k = lane; k < res; k += 64) sv[k] = hq[k] - h0[k];
    int nk = 0;
    for (int j = 1; j < m; j++) {
        const double *hj = H + (size_t)idx[j] * res;
        __syncthreads();
        for (int k = lane; k < res; k += 64) {
            const double z = hj[k] - h0[k];
            sr[k] = z;
            sp[k] = z * z;
        }
        __syncthreads();
        const double zz = serial_sum(sp, res);
        for (int i = 0; i < nk; i++) {
            const double *qi = Qw + (size_t)i * res;
            __syncthreads();
            for (int k = lane; k < res; k += 64) sp[k] = qi[k] * sr[k];
            __syncthreads();
            const double c = serial_sum(sp, res);
            for (int k = lane; k < res; k += 64) sr[k] = sr[k] - c * qi[k];
            if (lane == 0) cm[j][i] = c;
        }
        __syncthreads();
        for (int k = lane; k < res; k += 64) sp[k] = sr[k] * sr[k];
        __syncthreads();
        const double s = serial_sum(sp, res);
        if (s > NNGP_ELM_TAU * zz) {   // uniform: every lane holds the same s and zz
            const double sq = sqrt(s);
            for (int k = lane; k < res; k += 64) Qw[(size_t)nk * res + k] = sr[k] / sq;
            if (lane == 0) {
                ssq[nk] = sq;
                skept[nk] = j;
            }
            nk++;
        }
    }
    for (int i = 0; i < nk; i++) {
        const double *qi = Qw + (size_t)i * res;
        __syncthreads();   // (also orders the Qw writes above before these reads, block scope)
        for (int k = lane; k < res; k += 64) sp[k] = qi[k] * sv[k];
        __syncthreads();
        const double w = serial_sum(sp, res);
        if (lane == 0) sw[i] = w;
    }
    __syncthreads();
    // the d-long pass, a coordinate per lane: g_s = (dy_j - sum_{i<s} c_ji g_i) / sqrt(s_j), then
    // pred = y_0 + w_0 g_0 + w_1 g_1 + .., left to right
    for (int c0 = 0; c0 < d; c0 += 64) {
        const int c = c0 + lane;
        if (c >= d) break;
        const double y0 = Y[(size_t)i0 * d + c];
        double pred = y0;
        for (int s = 0; s < nk; s++) {
            const int j = skept[s];
            double g = Y[(size_t)idx[j] * d + c] - y0;
            for (int i = 0; i < s; i++) g = g - cm[j][i] * gl[i][lane];
            g = g / ssq[s];
            gl[s][lane] = g;
            pred = pred + sw[s] * g;
        }
        if (preds) preds[c] = pred;
        if (out) out[c] = pred + bias[c];
    }
}

static int64_t elm_n_poly(int d, int degree) {
    return 1 + (int64_t)d + (degree == 2 ? (int64_t)d * (d + 1) / 2 : 0);
}

static int elm_check(int d, int degree, int res, const double *bias_h, const double *C) {
    NNGP_REQUIRE(bias_h && C, "null weight argument (bias_h, C)");
    NNGP_REQUIRE(d >= 1 && d <= ELM_MAX_D, "ELM supports 1 <= d <= %d (got %d)", ELM_MAX_D, d);
    NNGP_REQUIRE(degree == 1 || degree == 2, "ELM supports degree 1 or 2 (got %d)", degree);
    NNGP_REQUIRE(res >= 1 && res <= ELM_MAX_RES, "ELM supports 1 <= res_size <= %d (got %d)", ELM_MAX_RES, res);
    return NNGP_OK;
}

// hidden rows of X[rows][d] into H[rows][res]; part: scratch of nch * max_rows * res doubles, the
// rows go through it in batches of max_rows (the sums of a row do not depend on its batch)
static int hidden_launch(const double *X, int64_t rows, int d, int degree, int res, const double *bias_h,
                         const double *C, double *H, double *part, int64_t max_rows, hipStream_t st) {
    const int64_t F = elm_n_poly(d, degree);
    const int nch = (int)((F + ELM_CHUNK - 1) / ELM_CHUNK);
    const int rt = d <= 2048 ? ELM_ROW_TILE : 1;
    for (int64_t r0 = 0; r0 < rows; r0 += max_rows) {
        const int64_t nb = std::min(max_rows, rows - r0);
        const int ntiles = (int)((nb + rt - 1) / rt);
        // few workgroups (a query row): split the hidden units over gridDim.y, up to one group of 4 each
        const int64_t nwg = (int64_t)ntiles * nch;
        const int ysplit = nwg >= 2048 ? 1 : (int)std::min<int64_t>((res + 3) / 4, (2048 + nwg - 1) / nwg);
        const dim3 grid((unsigned)nwg, (unsigned)ysplit);
        const size_t lds = sizeof(double) * (size_t)rt * d;
        if (rt == ELM_ROW_TILE)
            hipLaunchKernelGGL(elm_hidden_kernel<ELM_ROW_TILE>, grid, dim3(256), lds, st, X + (size_t)r0 * d, nb, d,
                               degree, F, C, res, ntiles, part);
        else
            hipLaunchKernelGGL(elm_hidden_kernel<1>, grid, dim3(256), lds, st, X + (size_t)r0 * d, nb, d, degree, F,
                               C, res, ntiles, part);
        NNGP_LAUNCH_CHECK();
        if (nb * res <= 4096)
            hipLaunchKernelGGL(elm_combine_wave_kernel, dim3((unsigned)(nb * res)), dim3(64), 0, st, part, nch, nb, res,
                               bias_h, H + (size_t)r0 * res);
        else
            hipLaunchKernelGGL(elm_combine_kernel, dim3((unsigned)((nb * res + 255) / 256)), dim3(256), 0, st, part,
                               nch, nb, res, bias_h, H + (size_t)r0 * res);
        NNGP_LAUNCH_CHECK();
    }
    return NNGP_OK;
}

// the per-prediction scratch (workspace slot 10): idx [16] | hq [res] | part [nch][res] | Qw [m-1][res]
struct ElmScratch {
    int32_t *idx;
    double *hq, *part, *Qw;
};

static int elm_scratch(int d, int degree, int res, ElmScratch *s) {
    const int64_t F = elm_n_poly(d, degree);
    const size_t nch = (size_t)((F + ELM_CHUNK - 1) / ELM_CHUNK);
    int err = 0;
    char *ws = (char *)workspace(128 + sizeof(double) * (size_t)res * (1 + nch + ELM_MAX_M), &err, 10);
    if (err) return err;
    s->idx = (int32_t *)ws;
    s->hq = (double *)(ws + 128);
    s->part = s->hq + res;
    s->Qw = s->part + nch * res;
    return NNGP_OK;
}

static int elm_predict_impl(const double *X, const double *Y, const double *H, int64_t rows, int d,
                            const double *new_x, int m, int degree, int res, const double *bias_h, const double *C,
                            double *preds_out, const double *bias, double *out, const ElmScratch &s, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    int rc = nngp_knn(X, rows, d, new_x, m, s.idx, nullptr, stream);
    if (rc) return rc;
    rc = hidden_launch(new_x, 1, d, degree, res, bias_h, C, s.hq, s.part, 1, st);
    if (rc) return rc;
    hipLaunchKernelGGL(elm_solve_kernel, dim3(1), dim3(64), 0, st, s.idx, H, Y, s.hq, m, res, d, s.Qw, bias, preds_out,
                       bias ? out : nullptr);
    NNGP_LAUNCH_CHECK();
    return NNGP_OK;
}

}  // namespace nngp

using namespace nngp;

extern "C" int nngp_elm_hidden(const double *X, int64_t rows, int d, int degree, int res_size,
                               const double *bias_h, const double *C, double *H, void *stream) {
    const int rc0 = elm_check(d, degree, res_size, bias_h, C);
    if (rc0) return rc0;
    NNGP_REQUIRE(rows >= 0, "rows must be >= 0 (got %lld)", (long long)rows);
    if (rows == 0) return NNGP_OK;
    NNGP_REQUIRE(X && H, "null array argument (X, H)");
    const int64_t F = elm_n_poly(d, degree);
    const int64_t nch = (F + ELM_CHUNK - 1) / ELM_CHUNK;
    // batches of rows whose partial sums fit 64 MB (a multiple of the row tile, at least one tile)
    int64_t max_rows = ((int64_t)64 << 20) / (int64_t)(sizeof(double) * nch * res_size);
    max_rows = std::max<int64_t>(ELM_ROW_TILE, max_rows / ELM_ROW_TILE * ELM_ROW_TILE);
    max_rows = std::min(max_rows, (rows + ELM_ROW_TILE - 1) / ELM_ROW_TILE * ELM_ROW_TILE);
    int err = 0;
    double *part = (double *)workspace(sizeof(double) * (size_t)nch * max_rows * res_size, &err, 11);
    if (err) return err;
    return hidden_launch(X, rows, d, degree, res_size, bias_h, C, H, part, max_rows, (hipStream_t)stream);
}

static int elm_predict_check(const double *X, const double *Y, const double *H, int64_t rows, int m) {
    NNGP_REQUIRE(X && Y && H, "null array argument (X, Y, H)");
    NNGP_REQUIRE(m >= 1 && m <= ELM_MAX_M && m <= rows, "ELM needs 1 <= m <= min(%d, rows) (m=%d rows=%lld)",
                 ELM_MAX_M, m, (long long)rows);
    return NNGP_OK;
}

extern "C" int nngp_elm_predict(const double *X, const double *Y, const double *H, int64_t rows, int d,
                                const double *new_x, int m, int degree, int res_size, const double *bias_h,
                                const double *C, double *preds_out, const double *bias, double *out,
                                void *stream) {
    int rc = elm_check(d, degree, res_size, bias_h, C);
    if (rc) return rc;
    if ((rc = elm_predict_check(X, Y, H, rows, m)) != NNGP_OK) return rc;
    NNGP_REQUIRE(new_x && (preds_out || (bias && out)), "need new_x and preds_out or (bias, out)");
    NNGP_REQUIRE(!out || bias, "out needs bias");
    ElmScratch s;
    if ((rc = elm_scratch(d, degree, res_size, &s)) != NNGP_OK) return rc;
    return elm_predict_impl(X, Y, H, rows, d, new_x, m, degree, res_size, bias_h, C, preds_out, bias, out, s, stream);
}

extern "C" int nngp_elm_sweep(const nngp_system *sys, int g_tableau, int g_step_mode, int64_t g_steps,
                              const double *t, int I, int N, double *U1, double *UG1, const double *X,
                              const double *Y, const double *H, int64_t rows, int m, int degree, int res_size,
                              const double *bias_h, const double *C, float *g_ms_out, void *stream) {
    NNGP_REQUIRE(sys != nullptr && t && U1 && UG1, "null argument");
    NNGP_REQUIRE(0 <= I && I <= N, "need 0 <= I <= N (I=%d N=%d)", I, N);
    const int d = sys->d;
    int rc = elm_check(d, degree, res_size, bias_h, C);
    if (rc) return rc;
    if ((rc = elm_predict_check(X, Y, H, rows, m)) != NNGP_OK) return rc;
    GTimer gt;
    if ((rc = gt.begin(g_ms_out, (int64_t)N - I, g_time_stride())) != NNGP_OK) return rc;
    if (N == I) return NNGP_OK;
    const Coarse G{sys, g_tableau, g_step_mode, g_steps, t};
    ElmScratch s;
    if ((rc = elm_scratch(d, degree, res_size, &s)) != NNGP_OK) return rc;
    for (int i = I; i < N; i++) {
        const double *ui = U1 + (size_t)i * d;
        double *ug_next = UG1 + (size_t)(i + 1) * d;
        if ((rc = gt.launch(G, i, (size_t)(i - I), ui, ug_next, (hipStream_t)stream)) != NNGP_OK) return rc;
        rc = elm_predict_impl(X, Y, H, rows, d, ui, m, degree, res_size, bias_h, C, nullptr, ug_next,
                              U1 + (size_t)(i + 1) * d, s, stream);
        if (rc) return rc;
    }
    return gt.finish();
}
