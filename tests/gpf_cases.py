"""Shared by tests/test_gpf_cases_host.py (CPU) and tests/test_gpu_gpfull_factor.py (GPU): the
backward-error bounds that pin the full-GP factor of csrc/nngp_gpfull.hip itself (not only its
-LML), the case table, and a plain numpy restatement of the blocked left-looking order with the
mutants that show the bounds have teeth.  Host only: nothing here imports the GPU package.

Notation.  u = 2^-53, gamma_k = k u / (1 - k u).  F is the returned (n+1) x n lower-trapezoidal
factor: rows 0..n-1 are L, row n is z^T = (L^-1 y)^T.  M = [K; y^T].  Every reference value is
computed in np.longdouble (64-bit significand on x86-64).  None of the bounds depends on cond(K)
or on the summation order, and none holds a measured number:

  factor  |F F[:n]^T - M|_ij <= 2 gamma_{n+1} (|F| |F[:n]|^T)_ij + (3 + |c D2_ij|) u |K_ij|
          for every lower-triangle entry and every entry of row n (Higham, Accuracy and Stability
          of Numerical Algorithms, 2nd ed., Thm 10.3 for the Cholesky rows, Thm 8.5 for row n, a
          forward substitution).  M is psy exp(c D2) (+ 10^jitter on the diagonal) in longdouble
          from the D2 the factor itself used; the second term is the device's rounding of c D2
          (|c D2| u relative through exp), a 1-ulp exp (2u) and the product (u) -- on the diagonal
          c D2 = 0 and the jitter's addition is the one rounding.  The factor 2 covers multiplying
          by 1/L_jj instead of dividing and the FMA variant.  Row n of M is y itself: no 2nd term.
          Underflow: both theorems assume none, and the d = 1 cases cannot avoid it (321 points on
          a line are factorable at jitter -20 only with sigma_x near their spacing, so exp(c D2)
          leaves the normal range for the far pairs; LAPACK's factor is outside the two terms
          there by 1e13).  Each of the <= n + 1 products of an entry, the entry of K and the
          reciprocal multiply may then be off by up to the smallest normal 2^-1022 (gradual or
          flushed), scaled by entries <= max(1, psy + 10^jitter): the bound carries the absolute
          term (n + 4) max(1, psy + 10^jitter) 2^-1022 ~ 1e-305, far below u times any entry
          that did not underflow.
  -LML    |fval - (0.5 z.z + sum log L_ii + (n/2) log 2pi)| <= gamma_{n+2} (0.5 sum z^2 +
          sum |log L_ii| + (n/2) log 2pi), from the returned F (log 2pi: the double constant).
  alpha   |L^T alpha - z|_i <= gamma_n (|L^T| |alpha|)_i (Higham Thm 8.5), from the returned L, z.
  mean    |out_j - (sum_i psy exp(c dist_i) alpha_i + bias_j)| <= gamma_{n+2} sum |term_i| +
          sum (3 + |c dist_i|) u |term_i| (+ u |out_j| for the bias addition's one rounding),
          dist_i the sequential double sum the kernel states (scipy's order, as D2).
  D2      bitwise scipy's cdist(x, x, 'sqeuclidean'); d2_fallback_ratio holds it to gamma_{d+1}
          relative of the longdouble sum should that ever not hold.
"""
import functools

import numpy as np
import scipy.linalg
import scipy.spatial.distance

LD = np.longdouble
U = LD(2.0) ** -53
TINY = LD(2.0) ** -1022              # the smallest normal double: the underflow threshold
LOG_2PI = float(np.log(2 * np.pi))   # GPF_LOG_2PI of csrc/nngp_gpfull.hip, the same double
LB = 64                              # panel width of the left-looking order
assert np.finfo(LD).nmant >= 63, 'the reference arithmetic needs an extended-precision long double'


def gamma(k):
    return k * U / (1 - k * U)


# ----------------------------------------------------------------------------------- the inputs
def data(n, d):
    """x uniform in [-1, 1]^d, y = sin(2x) + 0.01 noise (tests/test_gpu_gpfull.py's recipe)."""
    rng = np.random.default_rng([n, d])
    x = rng.uniform(-1, 1, (n, d))
    y = np.sin(2 * x) + 0.01 * rng.standard_normal((n, d))
    return x, y


def gp_point(sx, sy, jit):
    """(c, psy, jp) as csrc/nngp_gpfull.hip gp_point rounds them (sigma_x = 0: c = -inf)."""
    with np.errstate(all='ignore'):
        sx, sy = np.float64(sx), np.float64(sy)
        return float(-0.5 * (1 / (sx * sx))), float(sy * sy), float(10.0 ** float(jit))


def d2_ref(x):
    return scipy.spatial.distance.cdist(x, x, 'sqeuclidean')


def dist_seq(x, q):
    """sum_k (x_ik - q_k)^2 in double, k ascending (gpf_mean_kernel's and scipy's loop)."""
    acc = np.zeros(x.shape[0])
    for k in range(x.shape[1]):
        t = x[:, k] - q[k]
        acc = acc + t * t
    return acc


def d2_fallback_ratio(D2, x):
    """max |D2 - longdouble sum| / (gamma_{d+1} longdouble sum): the bound D2 is held to should
    the bitwise claim fail (the difference, the square and the d - 1 additions each round once)."""
    xl = x.astype(LD)
    t = xl[:, None, :] - xl[None, :, :]
    s = (t * t).sum(-1)
    b = gamma(x.shape[1] + 1) * s
    with np.errstate(all='ignore'):
        return float(np.max(np.where(b > 0, np.abs(D2.astype(LD) - s) / b, np.where(D2 == s, 0, np.inf))))


def kernel_double(D2, pt):
    """K in double, kernel_np's order (gpf_entry): psy * exp(c * D2), + jp on the diagonal."""
    c, psy, jp = pt
    with np.errstate(all='ignore'):
        K = psy * np.exp(c * D2)
        K[np.diag_indices_from(K)] = K.diagonal() + jp
    return K


def kernel_long(D2, pt):
    c, psy, jp = pt
    K = LD(psy) * np.exp(LD(c) * D2.astype(LD))
    K[np.diag_indices_from(K)] = K.diagonal() + LD(jp)
    return K


def cond_of(x, theta, jit):
    with np.errstate(all='ignore'):
        K = kernel_double(d2_ref(x), gp_point(theta[0], theta[1], jit))
        return float(np.linalg.cond(K)) if np.all(np.isfinite(K)) else np.inf


# ----------------------------------------------------------------------------------- the bounds
def trapezoid(A, n):
    """The defined part of one returned (n+1) x (n+1) slab as F: L's lower triangle and row n."""
    F = np.array(A[:, :n], dtype=np.float64)
    F[:n] = np.tril(F[:n])
    return F


def _products(F):
    """F F[:n]^T and |F| |F[:n]|^T in longdouble on the lower trapezoid (64-row blocks: only the
    columns and the k range a block's rows reach, a third of the full product)."""
    n = F.shape[1]
    Fl = F.astype(LD)
    Al = np.abs(Fl)
    P = np.zeros((n + 1, n), dtype=LD)
    Q = np.zeros((n + 1, n), dtype=LD)
    for r0 in range(0, n + 1, 64):
        r1 = min(r0 + 64, n + 1)
        m = min(r1, n)
        P[r0:r1, :m] = Fl[r0:r1, :m] @ Fl[:m, :m].T
        Q[r0:r1, :m] = Al[r0:r1, :m] @ Al[:m, :m].T
    return P, Q


def factor_check(F, D2, pt, yv):
    """The factor bound on every lower-triangle entry and every entry of row n.  Returns a dict:
    ratio = max |R| / bound (<= 1: inside), at = its (i, j), ratio_g = max |R| / (2 gamma_{n+1}
    (|F||F[:n]|^T)), the part of the bound that belongs to the factorisation alone."""
    n = F.shape[1]
    c = pt[0]
    K = kernel_long(D2, pt)
    M = np.vstack([K, yv.astype(LD)[None, :]])
    P, Q = _products(F)
    mask = np.vstack([np.tril(np.ones((n, n), dtype=bool)), np.ones((1, n), dtype=bool)])
    R = np.abs(P - M)
    second = np.vstack([(3 + np.abs(LD(c) * D2.astype(LD))) * U * np.abs(K), np.zeros((1, n), dtype=LD)])
    first = 2 * gamma(n + 1) * Q
    with np.errstate(all='ignore'):
        B = first + second + (n + 4) * max(LD(1), LD(pt[1]) + LD(pt[2])) * TINY
        ratio = np.where(B > 0, R / B, np.where(R == 0, 0, np.inf))   # a zero bound admits only R = 0
        ratio = np.where(mask, np.where(np.isnan(ratio), np.inf, ratio), 0)
        rg = np.where(mask & (first > TINY / U), R / first, 0)   # (entries that underflowed: no scale)
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    worst = float(ratio[at])
    if not np.all(np.isfinite(F)):
        worst = np.inf
    return {'ratio': worst, 'at': (int(at[0]), int(at[1])), 'ratio_g': float(np.max(rg)),
            'where': failure_map(at[0], at[1], n)}


def failure_map(i, j, n):
    """Names the panel and tile of entry (i, j) in the left-looking order's terms."""
    p, t = j // LB, (i - LB * (j // LB)) // LB
    return (f'entry ({i}, {j}){" (row n = z)" if i == n else ""}: panel {p} (columns {LB * p}..), '
            f'row tile {t} of the panel, 16x16 sub-tile ({(i - LB * p) % LB // 16}, {j % LB // 16})')


def lml_check(F, fval):
    """|fval - recomputed| / bound from the returned F."""
    n = F.shape[1]
    z = F[n].astype(LD)
    lg = np.log(np.diagonal(F[:n]).astype(LD))
    half = LD(n) / 2 * LD(LOG_2PI)
    ref = LD(0.5) * (z * z).sum() + lg.sum() + half
    bound = gamma(n + 2) * (LD(0.5) * (z * z).sum() + np.abs(lg).sum() + half)
    return float(abs(LD(fval) - ref) / bound)


def alpha_check(F, alpha):
    """max_i |L^T alpha - z|_i / (gamma_n (|L^T| |alpha|)_i)."""
    n = F.shape[1]
    Lt = F[:n].astype(LD).T
    a = alpha.astype(LD)
    r = np.abs(Lt @ a - F[n].astype(LD))
    b = gamma(n) * (np.abs(Lt) @ np.abs(a))
    with np.errstate(all='ignore'):
        q = np.where(r <= b, np.where(b > 0, r / b, 0), np.inf)
    return float(np.max(q)) if np.all(np.isfinite(alpha)) else np.inf


def mean_reference(x, q, coef, alpha, bias):
    """(reference out [d], bound [d]) of nngp_gpfull_mean in longdouble."""
    n = x.shape[0]
    dist = dist_seq(x, q).astype(LD)
    ref, bnd = [], []
    for j in range(coef.shape[0]):
        c, psy = LD(coef[j, 0]), LD(coef[j, 1])
        term = psy * np.exp(c * dist) * alpha[j].astype(LD)
        m = term.sum()
        b = gamma(n + 2) * np.abs(term).sum() + ((3 + np.abs(c * dist)) * U * np.abs(term)).sum()
        if bias is not None:
            m = m + LD(bias[j])
            b = b + U * abs(m)
        ref.append(m)
        bnd.append(b)
    return np.array(ref, dtype=LD), np.array(bnd, dtype=LD)


# -------------------------------------------------------------------------------- the case table
ORDERS = {'ll64': {'NNGP_GPF_ORDER': '0', 'NNGP_GPF_FMA': '0'},
          'll64_fma': {'NNGP_GPF_ORDER': '0', 'NNGP_GPF_FMA': '1'},
          'rl32': {'NNGP_GPF_ORDER': '1', 'NNGP_GPF_FMA': '0'}}
SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257, 319, 320, 321)
BIG = 600
JITTERS = np.arange(-20, -11, dtype=float)
# sigma_x of the ill-conditioned point per n (jitter -12, sigma_y 1.3): the shortest of a sqrt(2)
# ladder with cond(K) >= 3e10; from n = 257 up tests/test_gpu_gpfull.py's own (0.7, 1.3).  n = 1
# has cond(K) = 1 whatever theta is.
HI_SX = {2: 9.2e4, 31: 5.6, 32: 4.0, 33: 4.0, 63: 2.0, 64: 2.0, 65: 2.0, 127: 1.4, 128: 1.0, 129: 1.4,
         191: 1.0, 192: 1.0, 193: 1.0}
LO_SX = {BIG: 0.12}   # the well-conditioned point is (0.2, 0.5) / -14 elsewhere
# sigma_x per (n, d) of the dimension cases: cond(K) >= 3e10 already at jitter -20, and small
# enough (< 1e12) that LAPACK factors every jitter of arange(-20, -11)
DIM_SX = {(65, 1): 0.0226, (65, 3): 1.58, (65, 200): 7.98e4, (130, 1): 0.016, (130, 3): 1.02,
          (130, 200): 2.59e4, (321, 1): 0.00617, (321, 3): 0.609, (321, 200): 680.0}
DIM_NS, DIM_DS = (65, 130, 321), (1, 3, 200)
BATCH_N, BATCH_NBS = 65, (1, 2, 3, 7, 8, 9)
NAN_POINT = (0.0, 1.0, -16.0, 0)   # sigma_x = 0: a NaN kernel, the factor must fail


def size_points(n):
    """[(sigma_x, sigma_y, jitter, coord)]: the cond >= 1e10 point, then the cond <= 1e4 point."""
    return [(HI_SX.get(n, 0.7), 1.3, -12.0, 0), (LO_SX.get(n, 0.2), 0.5, -14.0, 1)]


def dim_points(n, d):
    """The nine jitters at the (n, d) pair's sigma_x, over coordinates 0, d - 1 and d // 2."""
    co = (0, d - 1, d // 2)
    return [(DIM_SX[n, d], 1.3, float(j), co[i % 3]) for i, j in enumerate(JITTERS)]


def batch_points(nb):
    """nb distinct points at n = BATCH_N, ill- and well-conditioned ones interleaved."""
    hi, lo = size_points(BATCH_N)
    pool = [hi, lo, (1.0, 0.9, -13.0, 2), (0.5, 1.1, -15.0, 0), (1.58, 1.3, -20.0, 1), (0.3, 0.7, -12.0, 2),
            (1.2, 2.0, -18.0, 0), (0.9, 0.4, -16.0, 1), (2.0, 1.3, -14.0, 2)]
    return pool[:nb]


def duplicate_case(n=65):
    """Row 1 duplicates row 0, jitter -20: the second pivot is rounding noise, so either outcome
    of the factor is legitimate and only its self-consistency is asserted."""
    x, y = data(n, 3)
    x[1] = x[0]
    return x, y, [(0.7, 1.3, -20.0, 0)]


MEAN_NS, MEAN_DS = (1, 255, 256, 257, 600), (1, 3, 200)


def mean_case(n, d):
    """(x, q, coef [d][2], alpha [d][n], bias [d]): weights of magnitude 1e-3..1e10 with mixed
    signs, length scales that keep the kernel values away from underflow."""
    rng = np.random.default_rng([7, n, d])
    x = rng.uniform(-1, 1, (n, d))
    q = rng.uniform(-1, 1, d)
    sx = rng.uniform(0.5, 2.0, d) * np.sqrt(d)
    sy = rng.uniform(0.3, 2.0, d)
    coef = np.stack([-0.5 * (1 / (sx * sx)), sy * sy], axis=1)
    alpha = rng.choice([-1.0, 1.0], (d, n)) * 10.0 ** rng.uniform(-3, 10, (d, n))
    bias = rng.standard_normal(d)
    return x, q, coef, alpha, bias


# ------------------------------------------------------- the reference and the restated factors
def lapack_factor(D2, pt, yv):
    """[L; z^T] by LAPACK (np.linalg.cholesky / solve_triangular, as oracle/gpfull.py) and
    alpha = L^-T z; None when the Cholesky fails."""
    K = kernel_double(D2, pt)
    try:
        L = np.linalg.cholesky(K)
    except np.linalg.LinAlgError:
        return None, None
    z = scipy.linalg.solve_triangular(L, yv, lower=True)
    alpha = scipy.linalg.solve_triangular(L.T, z, lower=False)
    return np.vstack([L, z[None, :]]), alpha


def lml_double(F):
    """gpf_lml_kernel's expression in double."""
    n = F.shape[1]
    z = F[n]
    return float(-(((-0.5 * (z @ z)) - np.sum(np.log(np.diagonal(F[:n])))) - (n / 2) * LOG_2PI))


def _msub(x, a, b, fma):
    """x - a b; fma: one rounding, emulated through the longdouble product and difference."""
    if fma:
        return (x.astype(LD) - a.astype(LD) * b.astype(LD)).astype(np.float64)
    return x - a * b


MUTANTS = ('drop_kblock', 'skip_y_update', 'last_col_unsolved', 'ljj_early')
FATAL_MUTANT = 'drop_kblock_mid'


def restated_ll64(D2, pt, yv, fma=False, mutant=None):
    """The blocked left-looking order of csrc/nngp_gpfull.hip in plain numpy: per 64-column panel
    the update A[c0.., panel] -= L[c0.., :c0] L[panel, :c0]^T accumulated from zero in k blocks of
    4 (the MFMA's depth) and subtracted once, then the panel's columns right-looking: L_jj =
    sqrt(a_jj), L_ij = a_ij * (1 / L_jj), a_ik -= L_ij L_kj (one FMA when fma); row n = y^T rides
    along.  Returns F, or None on a pivot that is not > 0.

    mutant: one of MUTANTS, the subtle errors the bound must catch (placed in panel 0 / 1 and at
    k = 0, where the dropped terms are of the entries' own size; with a short length scale
    L[i, 0] ~ 0 for most rows and dropping it would be legitimately invisible):
      drop_kblock        the k block 0..3 missing from the first 16x16 sub-tile of the last panel's
                         update when that panel is short (n = 129, 321: the last pivot and z's last
                         entry).  It sits there because a dropped diagonal term only raises the
                         pivot; FATAL_MUTANT, the same block missing from panel 1's sub-tile (rows
                         96.., columns 64..), turns a later pivot negative at cond >= 1e10 whichever
                         k block it is, so the factor fails outright and there is no F to measure
      skip_y_update      row n not updated in panel 1
      last_col_unsolved  the last panel's last column left as the update wrote it (pb < 64 only)
      ljj_early          L_22 stored from a_22 before column 1's update"""
    n = D2.shape[0]
    A = np.vstack([kernel_double(D2, pt), yv[None, :]])
    assert mutant is None or mutant in MUTANTS or mutant == FATAL_MUTANT
    pre22 = None
    for c0 in range(0, n, LB):
        pb = min(LB, n - c0)
        c1 = c0 + pb
        acc = np.zeros((n + 1 - c0, pb))
        for k0 in range(0, c0, 4):
            blk = A[c0:, k0:k0 + 4] @ A[c0:c1, k0:k0 + 4].T
            if mutant == 'drop_kblock' and c1 == n and pb < LB and k0 == 0:
                blk[0:16, 0:16] = 0.0
            if mutant == FATAL_MUTANT and c0 == LB and k0 == 0:
                blk[32:48, 0:16] = 0.0
            acc = acc + blk
        if mutant == 'skip_y_update' and c0 == LB:
            acc[-1, :] = 0.0
        A[c0:, c0:c1] = A[c0:, c0:c1] - acc
        for j in range(pb):
            cj = c0 + j
            if mutant == 'last_col_unsolved' and pb < LB and c1 == n and j == pb - 1:
                continue
            if not A[cj, cj] > 0.0:
                return None
            ljj = np.sqrt(A[cj, cj])
            rj = 1.0 / ljj
            A[cj, cj] = ljj
            A[cj + 1:, cj] = A[cj + 1:, cj] * rj
            if cj == 1:
                pre22 = A[2, 2] if n > 2 else None
            if cj == 2 and mutant == 'ljj_early':
                A[cj, cj] = np.sqrt(pre22)
            if cj + 1 < c1:
                A[cj + 1:, cj + 1:c1] = _msub(A[cj + 1:, cj + 1:c1], A[cj + 1:, cj][:, None],
                                              A[cj + 1:c1, cj][None, :], fma)
    return trapezoid(A, n)


def perturbed(F, i, j, mult=64):
    """F with entry (i, j) moved by mult gamma_{n+1} (|F| |F[:n]|^T)_ij / L_jj: the residual at
    (i, j) moves by mult gamma_{n+1} of its own |L||L^T| scale."""
    n = F.shape[1]
    s = float(np.abs(F[i]) @ np.abs(F[j]))
    G = F.copy()
    G[i, j] = G[i, j] + float(mult * gamma(n + 1)) * s / F[j, j]
    return G


@functools.lru_cache(maxsize=None)
def host_case(n, d=3):
    """(x, y, D2) of one (n, d), computed once per process."""
    x, y = data(n, d)
    return x, y, d2_ref(x)
