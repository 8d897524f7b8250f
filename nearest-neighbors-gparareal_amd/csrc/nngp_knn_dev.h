// nngp_knn_dev.h -- the device code of the ordered kNN select (the select): the distance
// row body, the (distance, index) keys and their DPP minima, numpy's pairwise sums, the select itself
// (knn_select_dev) and its LDS.  Shared by nngp_gp.hip (nngp_knn, the nnGP prediction, the fused
// chain) and nngp_knnmean.hip (the k-NN mean), so that every caller selects with the same code.
#pragma once

#include "common.h"
#include "nngp_math.h"
#include "nngp_gpeval.h"

namespace nngp {

// squared distance of every training row to the query; blockIdx.y = query (query y is q + y*d, its
// distances dist + y*rows).  Defined in nngp_gp.hip, launched from there and from nngp_knnmean.hip.
__global__ void knn_dist_kernel(const double *__restrict__ X, int64_t rows, int d, const double *__restrict__ q,
                                double *__restrict__ dist);

// (value, index) order of numpy argsort with NaN last, on the squared distances the kNN selects
// from (always >= +0 or NaN): the IEEE bit pattern of a non-negative double orders like its value,
// and every NaN maps to one key above +inf, so a (u64 key, index) pair compares with integer ops.
__device__ __forceinline__ uint64_t dist_key(double v) {
    return (v != v) ? 0x7FF8000000000000ull : (uint64_t)__double_as_longlong(v);
}

__device__ __forceinline__ bool key_less(uint64_t a, int ai, uint64_t b, int bi) {
    return (a < b) | ((a == b) & (ai < bi));
}

// take (k, r) as the running minimum when it is a candidate (r >= 0) ahead of the current one
__device__ __forceinline__ void key_take(uint64_t &bk, int &bi, uint64_t k, int r) {
    const bool t = (r >= 0) & ((bi < 0) | key_less(k, r, bk, bi));
    bk = t ? k : bk;
    bi = t ? r : bi;
}

// numpy pairwise_sum of (a[i]-b[i])^2, i < n (numpy/_core/src/umath/loops_utils.h.src)
__device__ double pw_leaf(const double *__restrict__ a, const double *__restrict__ b, int n) {
    if (n < 8) {
        double res = 0.;
        for (int i = 0; i < n; i++) {
            const double t = a[i] - b[i];
            res += t * t;
        }
        return res;
    }
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const double t = a[j] - b[j];
        r[j] = t * t;
    }
    int i;
    for (i = 8; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const double t = a[i + j] - b[i + j];
            r[j] += t * t;
        }
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; i++) {
        const double t = a[i] - b[i];
        res += t * t;
    }
    return res;
}

// numpy's pairwise recursion over n terms (split at n2 = n/2 - (n/2)%8 until n <= 128) as a
// post-order walk: leaf(off, len) gives a leaf's value, the walk combines them as the recursion does
template <typename Leaf>
__device__ __forceinline__ double pw_walk(int n, Leaf &&leaf) {
    if (n <= 128) return leaf(0, n);
    int off[32], len[32], stage[32];
    double left[32];
    int sp = 1;
    off[0] = 0; len[0] = n; stage[0] = 0;
    double ret = 0.0;
    bool have = false;
    while (sp > 0) {
        const int t = sp - 1;
        if (have) {
            if (stage[t] == 1) {
                left[t] = ret;
                stage[t] = 2;
                have = false;
                int n2 = len[t] / 2;
                n2 -= n2 % 8;
                off[sp] = off[t] + n2; len[sp] = len[t] - n2; stage[sp] = 0; sp++;
            } else {   // stage 2: combine
                ret = left[t] + ret;
                sp--;
            }
            continue;
        }
        if (len[t] <= 128) {
            ret = leaf(off[t], len[t]);
            have = true;
            sp--;
            continue;
        }
        int n2 = len[t] / 2;
        n2 -= n2 % 8;
        stage[t] = 1;
        off[sp] = off[t]; len[sp] = n2; stage[sp] = 0; sp++;
    }
    return ret;
}

__device__ double pw_sqdiff(const double *__restrict__ a, const double *__restrict__ b, int n) {
    return pw_walk(n, [&](int o, int l) { return pw_leaf(a + o, b + o, l); });
}

// ---------------------------------------------------------------------------------------------
// kNN
// ---------------------------------------------------------------------------------------------
// blockIdx.y = query (batched: query y is q + y*d, its distances dist + y*rows).
// One lane per training row: the row is read with 16-byte vector loads that are all in flight at
// once (no LDS staging, no barriers), then summed sequentially in column order (scipy cdist).
// squared distance of training row r to q (the kernel's and the correction chain's row body)
__device__ __forceinline__ double knn_dist_row(const double *__restrict__ X, int d, const double *__restrict__ q,
                                               int64_t r) {
    const double *xr = X + r * d;
    double acc = 0.0;
    int c = 0;
    if ((((uintptr_t)xr | (uintptr_t)q) & 15) == 0) {   // 16-byte aligned rows: double2 loads
        // 16 double2 loads in flight per lane: 74 VGPRs, so a sweep's kNN launch fits beside the
        // overlapped batch's fit waves (2 per SIMD at 192 VGPRs); at 32 in flight (139 VGPRs) it
        // waited ~3 ms for a SIMD to drain at the start of each Burgers iteration
        constexpr int B = 16;
        for (; c + 2 * B <= d; c += 2 * B) {
            double2 v[B];
#pragma unroll
            for (int j = 0; j < B; j++) v[j] = *(const double2 *)(xr + c + 2 * j);
#pragma unroll
            for (int j = 0; j < B; j++) {
                const double t0 = q[c + 2 * j] - v[j].x;
                acc = acc + t0 * t0;
                const double t1 = q[c + 2 * j + 1] - v[j].y;
                acc = acc + t1 * t1;
            }
        }
    }
    for (; c < d; c++) {
        const double t = q[c] - xr[c];
        acc = acc + t * t;
    }
    return acc;
}

__device__ __forceinline__ double wave_lane_double(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// Wave-wide minimum of the (key, index) pair (index -1 = no candidate) with DPP moves inside each
// 16-lane row (quad_perm 1,0,3,2 / 2,3,0,1, row_half_mirror, row_mirror: after each level every
// lane of the aligned block holds the block's minimum, so a mirror reaches the partner block) and
// v_readlane across the four rows.  The order is total, so every lane ends with the same pair.
template <int CTRL>
__device__ __forceinline__ void key_min_dpp(uint64_t &bk, int &bi) {
    const uint32_t lo = __builtin_amdgcn_mov_dpp((int)(uint32_t)bk, CTRL, 0xF, 0xF, false);
    const uint32_t hi = __builtin_amdgcn_mov_dpp((int)(uint32_t)(bk >> 32), CTRL, 0xF, 0xF, false);
    const int oi = __builtin_amdgcn_mov_dpp(bi, CTRL, 0xF, 0xF, false);
    key_take(bk, bi, ((uint64_t)hi << 32) | lo, oi);
}

__device__ __forceinline__ void wave_key_min(uint64_t &bk, int &bi) {
    key_min_dpp<0xB1>(bk, bi);    // quad_perm [1,0,3,2]
    key_min_dpp<0x4E>(bk, bi);    // quad_perm [2,3,0,1]
    key_min_dpp<0x141>(bk, bi);   // row_half_mirror
    key_min_dpp<0x140>(bk, bi);   // row_mirror
    uint64_t rk = 0;
    int ri = -1;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)bk, 16 * r);
        const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(bk >> 32), 16 * r);
        key_take(rk, ri, ((uint64_t)hi << 32) | lo, __builtin_amdgcn_readlane(bi, 16 * r));
    }
    bk = rk;
    bi = ri;
}

// total order of doubles as u64 keys (NaN above everything, -0.0 == +0.0) for arg-min reductions
__device__ __forceinline__ uint64_t fval_key(double v) {
    if (v != v) return ~0ull;
    if (v == 0.0) return 0x8000000000000000ull;
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// minimum over each 16-lane row only (the 4 DPP levels of wave_key_min)
__device__ __forceinline__ void row_key_min(uint64_t &bk, int &bi) {
    key_min_dpp<0xB1>(bk, bi);
    key_min_dpp<0x4E>(bk, bi);
    key_min_dpp<0x141>(bk, bi);
    key_min_dpp<0x140>(bk, bi);
}

// Merge 4 ascending lists of m (key, index) pairs (lists k[0..3][*], index -1 = empty slot) into
// the m smallest in order: a wave's lane t < 4m ranks its pair against all 4m, and a valid pair
// of rank < m lands at that position (ok[]/oi[], or as index + value into oi32/od when ok null).
template <typename KI>
__device__ __forceinline__ void rank_merge(const uint64_t (*k)[64], const int (*ki)[64], int m, int lane, KI *ok,
                                           int *oi, double *od = nullptr) {
    const int n = 4 * m;
    for (int t = lane; t < n; t += 64) {
        const int tl = t / m, tq = t - tl * m;
        const uint64_t ck = k[tl][tq];
        const int ci = ki[tl][tq];
        if (ci < 0) continue;
        int rank = 0;
#pragma unroll
        for (int L = 0; L < 4; L++)
            for (int q = 0; q < m; q++) {
                const int ui = ki[L][q];
                rank += (ui >= 0) & key_less(k[L][q], ui, ck, ci);
            }
        if (rank < m) {
            if (ok) ok[rank] = ck;
            oi[rank] = ci;
            if (od) od[rank] = __longlong_as_double((long long)ck);
        }
    }
}

// LDS of one select (the caller's: a kernel-level __shared__ object, one per kernel)
static constexpr int SEL_CAND = 256;   // candidates the threshold select ranks exactly
struct SelShm {
    int32_t sel[64];
    double seld[64];
    uint32_t hist[256];
    uint64_t ck[SEL_CAND];
    int ci[SEL_CAND];
    int nc, digit, need;
    uint64_t rk[16][64];   // m <= 64
    int ri[16][64];
    uint64_t wk[4][64];
    int wi[4][64];
};

// K = 0 (rows > 4 096): up to this many rows the keys are staged once in the dynamic LDS (which
// the launcher sizes for them; the y_m / D2 staging reuses it afterwards) instead of being re-read
// from L2 on each of the radix passes (TomLab N = 256: ~20 of a select's ~24 us at 5 000 rows)
static constexpr int64_t KEY_LDS_ROWS = 14336;

// pw_leaf (8 <= n <= 128) on the 8 lanes of an aligned octet, lane j = lane & 7: lane j sums the
// elements i = j (mod 8) below n - n%8 in ascending order (pw_leaf's r[j]); the octet combines
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) with DPP moves (lane^1, lane^2, then the mirrored 4-block;
// a+b == b+a, so every lane holds the same bits); the n%8 tail follows in ascending order.
// Bitwise pw_leaf, with 8 lanes on one pair instead of one.  All 8 lanes must be active.
__device__ __forceinline__ double pw_leaf_octet(const double *__restrict__ a, const double *__restrict__ b, int n,
                                                int j) {
    const int nb = n - (n % 8);
    double av[16], bv[16];   // all loads in flight before the sum (n <= 128: <= 16 per lane)
#pragma unroll
    for (int u = 0; u < 16; u++) {
        const int i = j + 8 * u;
        av[u] = i < nb ? a[i] : 0.0;
        bv[u] = i < nb ? b[i] : 0.0;
    }
    double t = av[0] - bv[0];
    double r = t * t;
#pragma unroll
    for (int u = 1; u < 16; u++) {
        if (8 * u < nb) {   // nb is a multiple of 8: the same trip count on every lane
            t = av[u] - bv[u];
            r += t * t;
        }
    }
    r = r + __builtin_amdgcn_mov_dpp(r, 0xB1, 0xF, 0xF, false);    // quad_perm [1,0,3,2]
    r = r + __builtin_amdgcn_mov_dpp(r, 0x4E, 0xF, 0xF, false);    // quad_perm [2,3,0,1]
    r = r + __builtin_amdgcn_mov_dpp(r, 0x141, 0xF, 0xF, false);   // row_half_mirror
    for (int i = nb; i < n; i++) {
        t = a[i] - b[i];
        r += t * t;
    }
    return r;
}

// one workgroup of 256 threads per query (blockIdx.y; batched outputs at query-strided offsets).
// spec_idx / hit_flag (single query): hit_flag = 1 iff the selected ordered neighbour list equals
// spec_idx, else 2 iff it equals spec2_idx (when given), else 0 -- the speculative sweep then
// reuses the fits it computed for that list.  host_flag (host-mapped, optional) gets the same value.
template <int K, bool GENERIC_D2 = true>
__device__ __forceinline__ void knn_select_dev(
    SelShm &sh, const double *__restrict__ dist, int64_t rows, int m, const double *__restrict__ X,
    const double *__restrict__ Y, int d, const double *__restrict__ q, int32_t *__restrict__ idx_out,
    double *__restrict__ dist_out, double *__restrict__ ymT, double *__restrict__ D2,
    double *__restrict__ kd2, const int32_t *__restrict__ spec_idx, int32_t *__restrict__ hit_flag,
    int xs_doubles, const int32_t *__restrict__ spec2_idx, int32_t *host_flag, uint64_t *marks = nullptr,
    const HitMean *hm = nullptr, bool key_lds = false) {
    // marks (profiling, thread 0's clock): after the rounds | the merges | the gathers | D2
#define SEL_MARK(k) \
    if (marks && tid == 0) marks[k] += wall_clock64();
    int32_t *sel = sh.sel;
    double *seld = sh.seld;
    uint64_t(*rk)[64] = sh.rk;
    int(*ri)[64] = sh.ri;
    uint64_t(*wk)[64] = sh.wk;
    int(*wi)[64] = sh.wi;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    // K > 0: the thread's K keys (rows tid + 256*j) stay in registers
    uint64_t kv[K > 0 ? K : 1];
    int kr[K > 0 ? K : 1];
    if constexpr (K > 0) {
#pragma unroll
        for (int j = 0; j < K; j++) {
            const int r = tid + 256 * j;
            kr[j] = r < rows ? r : -1;
            kv[j] = r < rows ? dist_key(dist[r]) : 0;
        }
    }
    // 0) threshold select: the m-th smallest high word T of the keys by a 4-pass radix select
    //    (8-bit digits, LDS histograms), then every row with high word <= T -- a superset of the
    //    m nearest, usually m plus a few -- is ranked exactly by (key, row) against the others.
    //    Bitwise the rounds below (the ordered m smallest pairs are unique); they remain the path
    //    when more than SEL_CAND rows tie at or below T (duplicated training rows).  K > 0: the
    //    thread's keys from registers; K = 0 (rows > 4 096): re-read from dist (L2-resident) on
    //    each of the 5 passes -- against the rounds' m passes over all rows (TomLab N = 256 late
    //    in its run: ~25 000 rows, m = 18, 172 us per select with the rounds alone).
    bool done = false;
    // K = 0 with key_lds: the keys staged once in the dynamic LDS (KEY_LDS_ROWS)
    extern __shared__ __attribute__((aligned(16))) double sel_dyn[];
    uint64_t *kc = reinterpret_cast<uint64_t *>(sel_dyn);
    if constexpr (K == 0) {
        if (key_lds) {
#pragma unroll 8
            for (int r = tid; r < rows; r += 256) kc[r] = dist_key(dist[r]);
            __syncthreads();
        }
    }
    auto for_keys = [&](auto &&f) {
        if constexpr (K > 0) {
#pragma unroll
            for (int j = 0; j < K; j++)
                if (kr[j] >= 0) f(kv[j], kr[j]);
        } else if (key_lds) {
#pragma unroll 8
            for (int r = tid; r < rows; r += 256) f(kc[r], r);
        } else {
#pragma unroll 8
            for (int r = tid; r < rows; r += 256) f(dist_key(dist[r]), r);
        }
    };
    {
        uint32_t prefix = 0;
        int need = m;
        for (int pass = 0; pass < 4; pass++) {
            const int shift = 24 - 8 * pass;
            sh.hist[tid] = 0;   // 256 threads = 256 bins
            __syncthreads();
            for_keys([&](uint64_t key, int) {
                const uint32_t hk = (uint32_t)(key >> 32);
                const bool in = pass == 0 || (hk >> (shift + 8)) == (prefix >> (shift + 8));
                if (in) atomicAdd(&sh.hist[(hk >> shift) & 255], 1u);
            });
            __syncthreads();
            if (wid == 0) {   // the digit whose bin holds the need-th smallest: lane l scans bins 4l..4l+3
                const uint32_t h0 = sh.hist[4 * lane], h1 = sh.hist[4 * lane + 1], h2 = sh.hist[4 * lane + 2],
                               h3 = sh.hist[4 * lane + 3];
                const int own = (int)(h0 + h1 + h2 + h3);
                int incl = own;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int v = __shfl_up(incl, o, 64);
                    if (lane >= o) incl += v;
                }
                const int excl = incl - own;
                if (excl < need && need <= incl) {
                    int c = excl, b = 0;
                    const int hb[4] = {(int)h0, (int)h1, (int)h2, (int)h3};
#pragma unroll
                    for (int u = 0; u < 3; u++)
                        if (b == u && c + hb[u] < need) {
                            c += hb[u];
                            b = u + 1;
                        }
                    sh.digit = 4 * lane + b;
                    sh.need = need - c;
                }
            }
            __syncthreads();
            prefix |= (uint32_t)sh.digit << shift;
            need = sh.need;
        }
        if (tid == 0) sh.nc = 0;
        __syncthreads();
        for_keys([&](uint64_t key, int row) {
            if ((uint32_t)(key >> 32) <= prefix) {
                const int p = atomicAdd(&sh.nc, 1);
                if (p < SEL_CAND) {
                    sh.ck[p] = key;
                    sh.ci[p] = row;
                }
            }
        });
        __syncthreads();
        const int L = sh.nc;
        if (L <= SEL_CAND) {   // uniform
            for (int t = tid; t < L; t += 256) {
                const uint64_t k0 = sh.ck[t];
                const int i0 = sh.ci[t];
                int rank = 0;
#pragma unroll 8
                for (int u = 0; u < L; u++) rank += key_less(sh.ck[u], sh.ci[u], k0, i0);
                if (rank < m) {
                    sel[rank] = i0;
                    seld[rank] = __longlong_as_double((long long)k0);
                }
            }
            done = true;
        }
    }
    // 1) each 16-lane row of the workgroup: its m best (key, index) pairs among its lanes' rows
    //    (row r of the training set belongs to thread r % 256), in ascending order, by m rounds of
    //    "smallest pair strictly after the previous pick" with a 4-level DPP row minimum
    if (!done) {
        const int grp = tid >> 4;
        if constexpr (K > 0) {
            // sort the thread's K pairs once (odd-even transposition; an empty slot, row -1, sorts
            // last), then every round only the lanes' heads compete: the 16-lane minimum is the
            // row's next pick and its owner pops its head (~3x fewer instructions per round than
            // rescanning all K keys against the previous pick)
#pragma unroll
            for (int p = 0; p < K; p++) {
#pragma unroll
                for (int j = p & 1; j + 1 < K; j += 2) {
                    const bool sw = (kr[j + 1] >= 0) & ((kr[j] < 0) | key_less(kv[j + 1], kr[j + 1], kv[j], kr[j]));
                    const uint64_t tk = kv[j];
                    const int ti = kr[j];
                    kv[j] = sw ? kv[j + 1] : kv[j];
                    kr[j] = sw ? kr[j + 1] : kr[j];
                    kv[j + 1] = sw ? tk : kv[j + 1];
                    kr[j + 1] = sw ? ti : kr[j + 1];
                }
            }
            for (int k = 0; k < m; k++) {
                uint64_t bk = kv[0];
                int bi = kr[0];
                row_key_min(bk, bi);
                if ((tid & 15) == 0) {
                    rk[grp][k] = bk;
                    ri[grp][k] = bi;
                }
                const bool pop = (bi >= 0) & (kr[0] == bi);   // rows are distinct: one owner
#pragma unroll
                for (int j = 0; j + 1 < K; j++) {
                    kv[j] = pop ? kv[j + 1] : kv[j];
                    kr[j] = pop ? kr[j + 1] : kr[j];
                }
                kv[K - 1] = pop ? 0 : kv[K - 1];
                kr[K - 1] = pop ? -1 : kr[K - 1];
            }
        } else {
            uint64_t pk = 0;   // (0, -1) precedes every (key, row >= 0)
            int pi = -1;
            for (int k = 0; k < m; k++) {
                uint64_t bk = 0;
                int bi = -1;
                for (int r = tid; r < rows; r += 256) {
                    const uint64_t v = dist_key(dist[r]);
                    key_take(bk, bi, v, key_less(pk, pi, v, r) ? r : -1);
                }
                row_key_min(bk, bi);
                if ((tid & 15) == 0) {
                    rk[grp][k] = bk;
                    ri[grp][k] = bi;
                }
                if (bi >= 0) {   // an exhausted row keeps its last pick (no re-picking from the start)
                    pk = bk;
                    pi = bi;
                }
            }
        }
    }
    __syncthreads();
    SEL_MARK(0);
    // 2) each wave merges its 4 row lists by rank (a pair's rank = how many valid pairs precede
    //    it; pairs are distinct, so ranks are too), 3) wave 0 merges the 4 wave lists the same way
    if (!done) {   // uniform
        for (int t = lane; t < m; t += 64) wi[wid][t] = -1;
        rank_merge(&rk[4 * wid], &ri[4 * wid], m, lane, wk[wid], wi[wid]);
        __syncthreads();
        if (wid == 0) rank_merge(wk, wi, m, lane, (uint64_t *)nullptr, sel, seld);
        __syncthreads();
    }
    for (int k = tid; k < m; k += 256) {
        idx_out[k] = sel[k];
        if (dist_out) dist_out[k] = seld[k];
    }
    SEL_MARK(1);
    // the hit code; with hm, whether this select also finishes the mean (the prediction it hit is
    // prepared).  Without it the host flag is written here; with it, after the mean.
    __shared__ int s_hm;
    if (hit_flag && wid == 0) {   // lane k compares entry k of the lists: one round trip, not m
        bool ne1 = false, ne2 = spec2_idx == nullptr;
        for (int k = lane; k < m; k += 64) {
            const int v = sel[k];
            ne1 |= v != spec_idx[k];
            if (spec2_idx) ne2 |= v != spec2_idx[k];
        }
        const bool hit1 = __ballot(ne1) == 0, hit2 = __ballot(ne2) == 0;
        const int hit = hit1 ? 1 : (hit2 ? 2 : 0);
        if (lane == 0) {
            *hit_flag = hit;
            int hmv = 0;
            if (hm && hit != 0) {
                const double *ap = hit == 1 ? hm->AP1 : hm->AP2;
                const int32_t *dn = hit == 1 ? hm->done1 : hm->done2;
                if (ap && __hip_atomic_load(dn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= hm->target) {
                    __threadfence();   // the prepared coordinates before their count
                    hmv = hit;
                }
            }
            s_hm = hmv;
            // a select that finishes the mean says so on the device too (code 3 / 4): it computes no
            // y_m / D2, so a mean kernel queued behind it (the look-ahead's form 1) must not run
            if (hmv != 0) *hit_flag = hmv + 2;
            if (host_flag && hmv == 0) __hip_atomic_store(host_flag, hit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    } else if (tid == 0) {
        s_hm = 0;
    }
    __syncthreads();
    const int hm_hit = s_hm;   // uniform: 1 / 2 = finish the mean from AP1 / AP2 below
    // the gathers of the m selected rows: SG loads in flight per thread before their stores (a
    // load -> store per trip would wait out one memory latency per element)
    constexpr int SG = 8;
    const int md = m * d;
    if (ymT && hm_hit == 0) {   // coalesced row reads, transposed writes (a finished hit reads none)
        for (int t0 = tid; t0 < md; t0 += 256 * SG) {
            double v[SG];
#pragma unroll
            for (int u = 0; u < SG; u++) {
                const int t = t0 + 256 * u, r = t / d, c = t - r * d;
                if (t < md) v[u] = Y[(int64_t)sel[r] * d + c];
            }
#pragma unroll
            for (int u = 0; u < SG; u++) {
                const int t = t0 + 256 * u, r = t / d, c = t - r * d;
                if (t < md) ymT[c * m + r] = v[u];
            }
        }
    }
    if (D2) {
        // lower triangle incl. diagonal, mirrored ((a-b)^2 == (b-a)^2 bitwise); the m neighbour
        // rows are staged in LDS with coalesced loads when they fit (xs_doubles), at a row stride
        // of d+1 doubles so that lanes reading different rows hit different banks
        extern __shared__ __attribute__((aligned(16))) double xs[];
        const int ds = d + 1;
        const bool staged = (int64_t)m * ds <= xs_doubles;
        if (staged)
            for (int t0 = tid; t0 < md; t0 += 256 * SG) {
                double v[SG];
#pragma unroll
                for (int u = 0; u < SG; u++) {
                    const int t = t0 + 256 * u, r = t / d, c = t - r * d;
                    if (t < md) v[u] = X[(int64_t)sel[r] * d + c];
                }
#pragma unroll
                for (int u = 0; u < SG; u++) {
                    const int t = t0 + 256 * u, r = t / d, c = t - r * d;
                    if (t < md) xs[r * ds + c] = v[u];
                }
            }
        __syncthreads();
        SEL_MARK(2);
        // the pairs, then kd2 on the next tasks
        const int npairs = m * (m + 1) / 2;
        const int ntask = npairs + (kd2 ? m : 0);
        if (staged && d >= 8 && d <= 128) {   // an octet of lanes per pair (pw_leaf_octet)
            const int j8 = tid & 7;
            // a finished hit needs kd2 only (its D2 is the prepared prediction's): tasks npairs..
            const int t0 = hm_hit != 0 ? npairs : 0;
            const int nrnd = (ntask - t0 + 31) / 32;   // whole octets iterate together
            for (int rd = 0; rd < nrnd; rd++) {
                const int t = t0 + rd * 32 + (tid >> 3);
                const bool valid = t < ntask;
                const bool is_kd = valid && t >= npairs;
                int r = 0, jj = 0;
                if (valid && !is_kd) {
                    while ((r + 1) * (r + 2) / 2 <= t) r++;
                    jj = t - r * (r + 1) / 2;
                } else if (is_kd) {
                    r = t - npairs;
                }
                const double *xr = xs + (size_t)r * ds;
                const double *xj = is_kd ? q : xs + (size_t)jj * ds;
                const double v = pw_leaf_octet(xr, xj, d, j8);
                if (valid && j8 == 0) {
                    if (is_kd) {
                        kd2[r] = v;
                    } else {
                        D2[r * m + jj] = v;
                        D2[jj * m + r] = v;
                    }
                }
            }
        } else if constexpr (GENERIC_D2) {   // the fused chain: any d, staged or not
        for (int t = tid; t < ntask; t += 256) {
            if (t >= npairs) {
                const int r = t - npairs;
                kd2[r] = pw_sqdiff(staged ? xs + (size_t)r * ds : X + (int64_t)sel[r] * d, q, d);
                continue;
            }
            int r = 0;
            while ((r + 1) * (r + 2) / 2 <= t) r++;
            const int j = t - r * (r + 1) / 2;
            const double *xr = staged ? xs + (size_t)r * ds : X + (int64_t)sel[r] * d;
            const double *xj = staged ? xs + (size_t)j * ds : X + (int64_t)sel[j] * d;
            const double v = pw_sqdiff(xr, xj, d);
            D2[r * m + j] = v;
            D2[j * m + r] = v;
        }
        } else {   // d < 8, staged (the host's contract for this kernel): pw_leaf's sequential branch
        for (int t = tid; t < ntask; t += 256) {
            int r = 0, j = 0;
            const double *xj = q;
            if (t >= npairs) {
                r = t - npairs;
            } else {
                while ((r + 1) * (r + 2) / 2 <= t) r++;
                j = t - r * (r + 1) / 2;
                xj = xs + (size_t)j * ds;
            }
            const double *xr = xs + (size_t)r * ds;
            double res = 0.;
            for (int i = 0; i < d; i++) {
                const double u = xr[i] - xj[i];
                res += u * u;
            }
            if (t >= npairs) {
                kd2[r] = res;
            } else {
                D2[r * m + j] = res;
                D2[j * m + r] = res;
            }
        }
        }
    }
    __syncthreads();
    SEL_MARK(3);
#undef SEL_MARK
    if (hm_hit != 0) {   // gp_mean_dev's output for every coordinate, from the prepared halves
        const double *AP = hm_hit == 1 ? hm->AP1 : hm->AP2;
        const int l = tid & 15, grp = tid >> 4, maxm = hm->maxm, rpl = (maxm + 15) / 16, st = HM_STRIDE(maxm);
        const bool big = maxm > 32;
        double kd[4];
#pragma unroll
        for (int s = 0; s < 4; s++) kd[s] = kd2[l + 16 * s < m ? l + 16 * s : 0];
        // CH coordinates per group at a time, all their loads issued before the sums; every group
        // runs every trip (the DPP row sums)
        constexpr int CH = 4;
        for (int c0 = 0; c0 < d; c0 += 16 * CH) {
            double al[CH][4], cq[CH], ps[CH], okv[CH];
#pragma unroll
            for (int u = 0; u < CH; u++) {
                const int c = c0 + 16 * u + grp;
                const double *ap = AP + (int64_t)(c < d ? c : 0) * st;
#pragma unroll
                for (int s = 0; s < 4; s++) {
                    const int row = l + 16 * s;
                    al[u][s] = (s < rpl && row < maxm) ? ap[row] : 0.0;
                }
                cq[u] = ap[maxm];
                ps[u] = ap[maxm + 1];
                okv[u] = ap[maxm + 2];
            }
#pragma unroll
            for (int u = 0; u < CH; u++) {
                const int c = c0 + 16 * u + grp;
                const double mean = gp_mean_finish<4>(m, l, rpl, big, kd, cq[u], ps[u], al[u], okv[u] != 0.0);
                if (c < d && l == 0) {
                    hm->preds[c] = mean;
                    hm->out[c] = mean + hm->bias[c];
                }
            }
        }
        __syncthreads();
        if (tid == 0 && host_flag) {   // the mean is in U1[i+1] (stream-ordered for the next slice)
            __threadfence();
            __hip_atomic_store(host_flag, hm_hit + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

}  // namespace nngp
