"""NumPy restatement of the DiffReact arithmetic contract (DiffReact) and of the RK
step in the operation order of csrc/nngp_rk_dev.h (stage_input / step_update / LinGrid): the
bitwise yardstick of tests/test_gpu_diffreact.py, itself checked on the CPU by
tests/test_diffreact_host.py.  NumPy's elementwise fp64 add/sub/mul is IEEE, one rounding per
operation, so this is bit-reproducible.  Not a test module (no test_ prefix)."""
import numpy as np

# csrc/tableau.h: RK1 (Euler) and RK4 (classic); zero entries are skipped, as in the kernels
TABLEAUX = {
    1: ([[0.0]], [1.0]),
    4: ([[0.0, 0.0, 0.0, 0.0], [0.5, 0.0, 0.0, 0.0], [0.0, 0.5, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]],
        [1.0 / 6, 1.0 / 3, 1.0 / 3, 1.0 / 6]),
}


def rk_np(f, order, t0, t1, steps, u0, mode='fixed', gsteps=None, j0=0):
    """`steps` steps of tableau `order` from t0 to t1; mode 'fixed': h = (t1-t0)/steps, 'linspace':
    h_n = t[n+1]-t[n] on t[j] = j*dt + t0, t[steps] = t1 (LinGrid).  With gsteps (linspace only):
    steps j0 .. j0+steps-1 of the global grid of gsteps steps over [t0, t1] (nngp_rk_batch_grid)."""
    A, B = TABLEAUX[order]
    S = len(B)
    t0, t1 = np.float64(t0), np.float64(t1)
    if gsteps is None:
        gsteps = steps
    else:
        assert mode == 'linspace'
    dt = (t1 - t0) / np.float64(gsteps)
    u = np.array(u0, dtype=np.float64)
    jd = np.float64(j0)
    tn = jd * dt + t0
    for n in range(steps):
        if mode == 'linspace':
            jd = jd + np.float64(1.0)
            tn1 = t1 if n == gsteps - 1 - j0 else jd * dt + t0
            h = tn1 - tn
            tn = tn1
        else:
            h = dt
        k = []
        for s in range(S):
            t = None
            for j in range(s):
                if A[s][j] != 0.0:
                    v = A[s][j] * k[j]
                    t = v if t is None else t + v
            x = u if t is None else u + t
            k.append(h * f(x))
        acc = None
        for s in range(S):
            if B[s] != 0.0:
                v = B[s] * k[s]
                acc = v if acc is None else acc + v
        u = u + acc
    return u


def lorenz_np(u):
    """csrc LaneSys<LORENZ>, identity normalisation."""
    return np.array([10 * (u[1] - u[0]), (28 * u[0] - u[1]) - u[0] * u[2], u[0] * u[1] - (8.0 / 3) * u[2]])


class DiffReactNP:
    """f_n(u) of DiffReact(d_x=nx, Du, Dv, k), optionally inside the '-11' wrapper on [-4, 4]."""

    def __init__(self, nx, Du=1e-3, Dv=5e-3, k=5e-3, normalized=False):
        self.nx, self.n = nx, nx * nx
        self.Du, self.Dv, self.k = Du, Dv, k
        self.normalized = normalized
        dx = (1.0 - (-1.0)) / nx
        dy = (1.0 - (-1.0)) / nx
        self.cx, self.cy = 1 / dx**2, 1 / dy**2
        a = np.full(nx, 2.0)
        a[0] = a[-1] = 1.0
        # main[y][x] = -(a_x)/dx**2 - (a_y)/dy**2
        self.main = (-a[None, :] / dx**2) - (a[:, None] / dy**2)
        mn, mx = -4.0, 4.0
        self.mn, self.hw, self.sc = mn, 0.5 * (mx - mn), 2 / (mx - mn)

    def lap(self, w):
        """DIA order [0, -1, 1, -nx, nx]; a neighbour across a wall contributes no term."""
        W = w.reshape(self.nx, self.nx)   # [y][x], p = y*nx + x
        s = self.main * W
        s[:, 1:] = s[:, 1:] + self.cx * W[:, :-1]
        s[:, :-1] = s[:, :-1] + self.cx * W[:, 1:]
        s[1:, :] = s[1:, :] + self.cy * W[:-1, :]
        s[:-1, :] = s[:-1, :] + self.cy * W[1:, :]
        return s.reshape(-1)

    def raw(self, y):
        u, v = y[:self.n], y[self.n:]
        u_t = (((u - u * (u * u)) - self.k) - v) + self.Du * self.lap(u)
        v_t = (u - v) + self.Dv * self.lap(v)
        return np.concatenate([u_t, v_t])

    def __call__(self, y):
        y = np.asarray(y, dtype=np.float64)
        if not self.normalized:
            return self.raw(y)
        return self.raw((y + 1) * self.hw + self.mn) * self.sc
