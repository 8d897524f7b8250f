// ws_layout_check.cpp -- the two workspace carves of csrc/common.h (pred_ws_carve, spec_ws_carve) against
// the layouts written out as literal formulas: every sub-buffer's byte offset and the total size.
// Host only, no HIP call; built with the host compiler under -fsanitize=address,undefined and run by
// `make -C nearest-neighbors-gparareal_amd/csrc check-layout`.
#include <cinttypes>
#include <cstdio>

#include "common.h"

using namespace nngp;

static int g_bad = 0;
static char *const BASE = (char *)(uintptr_t)0x7f0000001000;   // never dereferenced

static void expect(const char *what, const void *p, size_t want) {
    const size_t got = (size_t)((const char *)p - BASE);
    printf("    %-10s %12zu%s\n", what, got, got == want ? "" : "   MISMATCH");
    if (got != want) {
        printf("    %-10s %12zu expected\n", "", want);
        g_bad++;
    }
}

static void expect_null(const char *what, const void *p) {
    if (p) {
        printf("    %-10s not null   MISMATCH\n", what);
        g_bad++;
    }
}

struct Case {
    const char *name;
    size_t rows, d, m, n_jitter, n_restarts, nq, W, maxm;   // maxm: the padded fit size; 0 = no HitMean
};

static void check(const Case &c) {
    const FitSet F{(int)c.m, (int)c.n_jitter, nullptr, (int)c.n_restarts, 0.1, 0.1, 400};
    const TrainSet T{nullptr, nullptr, (int64_t)c.rows, (int)c.d};
    const size_t rows = c.rows, d = c.d, m = c.m, nq = c.nq, W = c.W;
    const size_t nf = d * c.n_jitter * c.n_restarts;
    const size_t hst = c.maxm ? d * (size_t)HM_STRIDE((int)c.maxm) : 0;
    printf("%s: rows=%zu d=%zu m=%zu n_jitter=%zu n_restarts=%zu nq=%zu W=%zu hst=%zu\n", c.name, rows, d, m,
           c.n_jitter, c.n_restarts, nq, W, hst);
    if ((size_t)F.n_fits(T.d) != nf) {
        printf("  n_fits MISMATCH\n");
        g_bad++;
    }

    // slot 0: dist[rows] | D2[m*m] | kd2[m] | ymT[d*m] | idx[64] (int32) | fits[n_fits][4]
    printf("  prediction workspace\n");
    const PredWs p = pred_ws_carve(BASE, T.rows, T.d, F.m, F.n_fits(T.d));
    const size_t nd = rows + m * m + m + d * m;
    expect("dist", p.dist, 0);
    expect("D2", p.D2, 8 * rows);
    expect("kd2", p.kd2, 8 * (rows + m * m));
    expect("ymT", p.ymT, 8 * (rows + m * m + m));
    expect("idx", p.idx, 8 * nd);
    expect("fits", p.fits, 8 * nd + 4 * 64);
    expect("bytes", BASE + p.bytes, 8 * nd + 4 * 64 + 8 * 4 * nf);
    const PredWs p0 = pred_ws_carve(nullptr, T.rows, T.d, F.m, F.n_fits(T.d));
    expect("bytes (0)", BASE + p0.bytes, p.bytes);
    expect_null("dist (0)", p0.dist);
    expect_null("fits (0)", p0.fits);

    // slot 2: Qg | gtmp | spec_fits | [Qr | gtmp2 | spec2_fits] | spec_idx | flags | done | [spec2_idx]
    //         | [AP1 | AP2 | pre1 | pre2] after rounding the offset up to 8 bytes
    printf("  speculation buffers\n");
    const SpecWs s = spec_ws_carve(BASE, (int64_t)nq, T.d, F.m, F.n_fits(T.d), (int)W, hst);
    size_t o = 0;
    expect("Qg", s.Qg, o);
    expect("gtmp", s.gtmp, o += 8 * nq * d);
    expect("spec_fits", s.spec_fits, o += 8 * d);
    o += 8 * nq * nf * 4;
    if (W > 0) {
        expect("Qr", s.Qr, o);
        expect("gtmp2", s.gtmp2, o += 8 * W * d);
        expect("spec2_fits", s.spec2_fits, o += 8 * d);
        o += 8 * nq * nf * 4;
    } else {
        expect_null("Qr", s.Qr);
        expect_null("gtmp2", s.gtmp2);
        expect_null("spec2_fits", s.spec2_fits);
    }
    expect("spec_idx", s.spec_idx, o);
    expect("flags", s.flags, o += 4 * nq * m);
    expect("done", s.done, o += 4 * nq);
    o += 4 * nq;
    if (W > 0) {
        expect("spec2_idx", s.spec2_idx, o);
        o += 4 * nq * m;
    } else {
        expect_null("spec2_idx", s.spec2_idx);
    }
    if (hst > 0) {
        o = (o + 7) & ~(size_t)7;
        expect("AP1", s.AP1, o);
        expect("AP2", s.AP2, o += 8 * nq * hst);
        expect("pre1", s.pre1, o += 8 * nq * hst);
        expect("pre2", s.pre2, o += 4 * nq);
    } else {
        expect_null("AP1", s.AP1);
        expect_null("AP2", s.AP2);
        expect_null("pre1", s.pre1);
        expect_null("pre2", s.pre2);
    }
    const size_t bytes = 8 * (nq * d + d + nq * nf * 4) + 4 * (nq * m + nq + nq) +
                         (W > 0 ? 8 * (W * d + d + nq * nf * 4) + 4 * nq * m : 0) +
                         (hst > 0 ? 8 * (2 * nq * hst + 1) + 4 * 2 * nq : 0);
    expect("bytes", BASE + s.bytes, bytes);
    expect("bytes (0)", BASE + spec_ws_carve(nullptr, (int64_t)nq, T.d, F.m, F.n_fits(T.d), (int)W, hst).bytes, bytes);
}

int main() {
    // HitMean needs a window (W > 0), and then the int32 arrays hold 2 nq (m + 1) entries: an odd
    // nq * m leaves spec_idx's end off an 8-byte boundary, but AP1's offset is on one already.
    const Case cases[] = {
        {"smallest", 1, 1, 1, 1, 1, 2, 0, 0},
        {"smallest, window and HitMean", 1, 1, 1, 1, 1, 2, 1, 8},
        {"odd nq * m", 40, 3, 5, 9, 1, 3, 2, 8},
        {"odd nq * m, no HitMean", 40, 3, 5, 9, 1, 3, 2, 0},
        {"W = nq - 1", 57, 3, 7, 9, 2, 5, 4, 8},
        {"Burgers N = 128", 1280, 128, 18, 9, 1, 128, 4, 18},
    };
    for (const Case &c : cases) check(c);
    printf("%d mismatches\n", g_bad);
    return g_bad ? 1 : 0;
}
