// ubench_dpp_fma.hip -- cost and value check of gfx950's `v_fmac_f64_dpp row_newbcast` (one wave).
// Informs the Hopf lane-group RHS: acc +- bcast(v) as ONE fused DPP multiply-add
// with a +-1.0 multiplier in a VGPR, instead of `v_mov_b64_dpp row_newbcast` + `v_add_f64`.
//   timing: one wave, 8 x unrolled asm blocks, cycles per chain step (s_memtime) for
//     (a) v_mov_b64_dpp + v_add_f64          (b) v_fmac_f64_dpp          (c) v_add_f64
//     each on an accumulator chain (the DPP source is loop-invariant), and (a2)/(b2) with the DPP
//     source on the chain itself (x += m * bcast(x), `s_nop 1` for the VALU-write -> DPP-read hazard);
//   values: lanes of a masked-off bank keep their accumulator, lanes of an enabled bank get
//     fma(v[row lane N], m, acc) bit for bit (host fma), bank masks 0x1 0x2 0x3, source lanes 0 4 8;
//     with m = +-1.0 that is the host's acc +- v, signed zeros included;
//   back-to-back chain: fused ops right behind the op that wrote their accumulator, no wait states.
// Result on MI355X (profiles/r07/ubench_dpp_fma.txt): a single fused op is bitwise the host's fma and
// issues at an add's cost (4.9 cycles against 9.4 for mov + add), but the back-to-back chain
// MISMATCHES (hence the NO-GO verdict for fusing every addition): the accumulator of a DPP op
// needs its two wait states like the DPP source, and `s_nop 1` in a chain costs 7.7 cycles.
// Build: hipcc -O3 --offload-arch=gfx950 tools/ubench_dpp_fma.hip -o tools/_ubench_dpp_fma
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#define REP 4096
#define CK(x)                                                              \
    do {                                                                   \
        hipError_t e_ = (x);                                               \
        if (e_ != hipSuccess) {                                            \
            printf("%s: %s\n", #x, hipGetErrorString(e_));                 \
            return 2;                                                      \
        }                                                                  \
    } while (0)

#define R8(x) x x x x x x x x

// MODE 0: (a) mov_dpp + add, 1: (b) fmac_dpp, 2: (c) add, 3: (a2) source on the chain, mov_dpp + fma,
// 4: (b2) source on the chain, fmac_dpp
template <int MODE>
__global__ void chain(double *out, long long *cyc, double v0, double m0) {
    double acc = threadIdx.x * 1e-3 + 1.0, v = v0 + threadIdx.x * 1e-6, m = m0, t = 0.0;
    asm volatile("" : "+v"(acc), "+v"(v), "+v"(m), "+v"(t));
    __syncthreads();
    long long t0 = clock64();
    for (int r = 0; r < REP; r += 8) {
        if constexpr (MODE == 0)
            asm volatile(R8("v_mov_b64_dpp %1, %2 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
                            "v_add_f64 %0, %0, %1\n\t")
                         : "+v"(acc), "+v"(t) : "v"(v));
        if constexpr (MODE == 1)
            asm volatile(R8("v_fmac_f64_dpp %0, %1, %2 row_newbcast:0 row_mask:0xf bank_mask:0x3\n\t")
                         : "+v"(acc) : "v"(v), "v"(m));
        if constexpr (MODE == 2)
            asm volatile(R8("v_add_f64 %0, %0, %1\n\t") : "+v"(acc) : "v"(v));
        if constexpr (MODE == 3)
            asm volatile(R8("s_nop 1\n\t"
                            "v_mov_b64_dpp %1, %0 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
                            "v_fma_f64 %0, %1, %2, %0\n\t")
                         : "+v"(acc), "+v"(t) : "v"(m));
        if constexpr (MODE == 4)
            asm volatile(R8("s_nop 1\n\t"
                            "v_fmac_f64_dpp %0, %0, %1 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t")
                         : "+v"(acc) : "v"(m));
    }
    long long t1 = clock64();
    out[threadIdx.x] = acc + t;
    if (threadIdx.x == 0) cyc[0] = t1 - t0;
}

template <int MODE>
static double run(const char *name, int per) {
    double *o;
    long long *c, h = 0;
    CK(hipMalloc(&o, 64 * 8));
    CK(hipMalloc(&c, 8));
    chain<MODE><<<1, 64>>>(o, c, 1e-9, MODE >= 3 ? 1e-6 : 1.0);
    chain<MODE><<<1, 64>>>(o, c, 1e-9, MODE >= 3 ? 1e-6 : 1.0);
    CK(hipMemcpy(&h, c, 8, hipMemcpyDeviceToHost));
    const double step = (double)h / REP;
    printf("%-44s : %6.2f cycles per chain step, %d VALU -> %.2f per VALU\n", name, step, per, step / per);
    CK(hipFree(o));
    CK(hipFree(c));
    return step;
}

// one fused op per lane: acc <- fmac_dpp(acc, v, m) row_newbcast:N bank_mask:M
template <int N, int M>
__global__ void fused(const double *acc, const double *v, const double *m, double *out) {
    double a = acc[threadIdx.x], x = v[threadIdx.x], mm = m[threadIdx.x];
    asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:%4"
                 : "+v"(a) : "v"(x), "v"(mm), "n"(N), "n"(M));
    out[threadIdx.x] = a;
}

// the RHS's pattern: a plain VALU op writes the accumulator and two fused ops follow it back to
// back with NO wait states (the accumulator is an ordinary, interlocked dependency; only the DPP
// source operand needs its two wait states, and v and m are old here)
__global__ void fused_chain(const double *acc, const double *v, const double *m, double *out) {
    double a = acc[threadIdx.x], x = v[threadIdx.x], mm = m[threadIdx.x];
    asm volatile("s_nop 1\n\t"
                 "v_fma_f64 %0, %0, %2, %0\n\t"
                 "v_fmac_f64_dpp %0, %1, %2 row_newbcast:0 row_mask:0xf bank_mask:0x3\n\t"
                 "v_fmac_f64_dpp %0, %1, %2 row_newbcast:4 row_mask:0xf bank_mask:0x3\n\t"
                 "v_fma_f64 %0, %1, %0, %2\n\t"
                 "v_fmac_f64_dpp %0, %1, %2 row_newbcast:4 row_mask:0xf bank_mask:0x1\n\t"
                 "v_fmac_f64_dpp %0, %1, %2 row_newbcast:0 row_mask:0xf bank_mask:0x2"
                 : "+v"(a) : "v"(x), "v"(mm));
    out[threadIdx.x] = a;
}

static uint64_t bits(double x) {
    uint64_t b;
    memcpy(&b, &x, 8);
    return b;
}

template <int N, int M>
static int check(const double *acc, const double *v, const double *m, const char *what) {
    double *da, *dv, *dm, *dout, out[64];
    CK(hipMalloc(&da, 512)); CK(hipMalloc(&dv, 512)); CK(hipMalloc(&dm, 512)); CK(hipMalloc(&dout, 512));
    CK(hipMemcpy(da, acc, 512, hipMemcpyHostToDevice));
    CK(hipMemcpy(dv, v, 512, hipMemcpyHostToDevice));
    CK(hipMemcpy(dm, m, 512, hipMemcpyHostToDevice));
    fused<N, M><<<1, 64>>>(da, dv, dm, dout);
    CK(hipMemcpy(out, dout, 512, hipMemcpyDeviceToHost));
    int bad = 0, kept = 0, fusedn = 0;
    for (int l = 0; l < 64; l++) {
        const int bank = (l % 16) / 4, src = (l / 16) * 16 + N;
        double want;
        if ((M >> bank) & 1) {
            want = fma(v[src], m[l], acc[l]);
            if (m[l] == 1.0 && bits(want) != bits(acc[l] + v[src]) && !std::isnan(want)) bad++;
            if (m[l] == -1.0 && bits(want) != bits(acc[l] - v[src]) && !std::isnan(want)) bad++;
            fusedn++;
        } else {
            want = acc[l];
            kept++;
        }
        const bool same = std::isnan(want) ? std::isnan(out[l]) : bits(want) == bits(out[l]);
        if (!same) {
            bad++;
            printf("  MISMATCH %s newbcast:%d bank_mask:0x%x lane %d: got %a want %a\n", what, N, M, l, out[l], want);
        }
    }
    printf("values %-10s row_newbcast:%d bank_mask:0x%x : %2d lanes fused, %2d kept, %s\n", what, N, M, fusedn, kept,
           bad ? "MISMATCH" : "bitwise the host fma");
    CK(hipFree(da)); CK(hipFree(dv)); CK(hipFree(dm)); CK(hipFree(dout));
    return bad;
}

static int check_chain(const double *acc, const double *v, const double *m) {
    double *da, *dv, *dm, *dout, out[64];
    CK(hipMalloc(&da, 512)); CK(hipMalloc(&dv, 512)); CK(hipMalloc(&dm, 512)); CK(hipMalloc(&dout, 512));
    CK(hipMemcpy(da, acc, 512, hipMemcpyHostToDevice));
    CK(hipMemcpy(dv, v, 512, hipMemcpyHostToDevice));
    CK(hipMemcpy(dm, m, 512, hipMemcpyHostToDevice));
    fused_chain<<<1, 64>>>(da, dv, dm, dout);
    CK(hipMemcpy(out, dout, 512, hipMemcpyDeviceToHost));
    int bad = 0;
    for (int l = 0; l < 64; l++) {
        const int bank = (l % 16) / 4, row = (l / 16) * 16;
        double a = fma(acc[l], m[l], acc[l]);
        if (bank < 2) a = fma(v[row + 0], m[l], a);
        if (bank < 2) a = fma(v[row + 4], m[l], a);
        a = fma(v[l], a, m[l]);
        if (bank == 0) a = fma(v[row + 4], m[l], a);
        if (bank == 1) a = fma(v[row + 0], m[l], a);
        const bool same = std::isnan(a) ? std::isnan(out[l]) : bits(a) == bits(out[l]);
        if (!same) {
            bad++;
            printf("  MISMATCH back-to-back chain lane %d: got %a want %a\n", l, out[l], a);
        }
    }
    printf("values back-to-back chain (fma, 2 fused, fma, 2 fused; no wait states) : %s\n",
           bad ? "MISMATCH" : "bitwise the host");
    CK(hipFree(da)); CK(hipFree(dv)); CK(hipFree(dm)); CK(hipFree(dout));
    return bad;
}

template <int N>
static int check_masks(const double *acc, const double *v, const double *m, const char *what) {
    return check<N, 0x1>(acc, v, m, what) + check<N, 0x2>(acc, v, m, what) + check<N, 0x3>(acc, v, m, what);
}

int main() {
    const double ta = run<0>("(a)  v_mov_b64_dpp + v_add_f64", 2);
    const double tb = run<1>("(b)  v_fmac_f64_dpp", 1);
    const double tc = run<2>("(c)  v_add_f64", 1);
    const double ta2 = run<3>("(a2) s_nop 1 + v_mov_b64_dpp(chain) + v_fma_f64", 2);
    const double tb2 = run<4>("(b2) s_nop 1 + v_fmac_f64_dpp(chain)", 1);
    // values: a deterministic mix of ordinary numbers and edge cases in every operand
    const double edge[] = {0.0, -0.0, 5e-324, -5e-324, 1e200, -1e200, 0.3, -0.3, 1.0, 0x1.fffffffffffffp+1023,
                           0x1p-1022, 1e-300, 3.0, -1e308, 0x1.0000000000001p+0, 0x1.fffffffffffffp-1};
    double acc[64], v[64], m[64], pm[64];
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        return (double)(int64_t)s * 0x1p-63;
    };
    int bad = 0;
    for (int round = 0; round < 4; round++) {
        for (int l = 0; l < 64; l++) {
            acc[l] = (round & 1) ? edge[(l * 7 + round) % 16] : rnd();
            v[l] = (round & 2) ? edge[(l * 5 + 3 * round) % 16] : rnd();
            m[l] = (l % 3 == 0) ? rnd() : edge[(l + round) % 16];
            pm[l] = ((l + round) & 1) ? -1.0 : 1.0;
        }
        bad += check_masks<0>(acc, v, m, "m any") + check_masks<4>(acc, v, m, "m any") +
               check_masks<8>(acc, v, m, "m any");
        bad += check_chain(acc, v, m) + check_chain(acc, v, pm);
        bad += check_masks<0>(acc, v, pm, "m +-1") + check_masks<4>(acc, v, pm, "m +-1") +
               check_masks<8>(acc, v, pm, "m +-1");
    }
    const bool go = !bad && tb < ta && tb2 < ta2;
    printf("value mismatches: %d\n", bad);
    printf("(b)/(a) = %.3f, (b)/(c) = %.3f, (b2)/(a2) = %.3f\n", tb / ta, tb / tc, tb2 / ta2);
    printf("verdict: %s\n", go ? "GO (fused op returns the expected bits and costs less than mov + add)" : "NO-GO");
    return bad ? 1 : 0;
}
