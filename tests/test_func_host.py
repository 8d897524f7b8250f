"""FuncODE without a GPU: the NumPy yardstick of tests/test_gpu_func.py (tests/func_ref.py) against
the CPU oracle -- ThomasLabyrinth written as three sine atoms is bit for bit the oracle's built-in
one, a system without atoms is bit for bit the polynomial restatement -- and against the reference's
recorded outputs (tests/golden/func.npz, written by gen_func.py from subclasses of the reference's
ODE); the library's refusals, every one made before any HIP call; the table handles; the Python
surface.

The fixture bound.  The reference evaluates the same equations with NumPy's sin / cos / exp / log and
in its own association, so per row the two sides differ by at most
    (16 + n_terms) eps sum|term|,   eps = 2^-52,
which covers, on both sides, <= 2 ulp per atom, three roundings per term and one per addition.  End
states after 32 steps are held to 64 times that bound on the step's terms |u_c| + h sum|term| (two
such errors per step, the steps' errors carried with gain ~1 over these short spans), taken at the
larger of the start and end state."""
import ctypes

import numpy as np
import pytest

import oracle as O
from conftest import golden
from adaptive_ref import solve
from func_ref import (GOLDEN_SYSTEMS, THOMAS_ATOMS, THOMAS_BOUNDS, THOMAS_ROWS, THOMAS_U0, FuncNP, n_terms, parse_atom,
                      synthetic)
from poly_ref import BRUS, PolyNP, lorenz96, rk_np

EPS = 2.0 ** -52
ORDERS = [1, 2, 4, 8]
SPANS = [(7, 0.3, 0.41), (1, 0.0, 0.01), (12, 1.7, 1.9)]


def _thomas(norm):
    return FuncNP(THOMAS_ATOMS, THOMAS_ROWS, *THOMAS_BOUNDS) if norm else FuncNP(THOMAS_ATOMS, THOMAS_ROWS)


# ------------------------------------------------------------------------------------------------
# the yardstick
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('norm', [False, True])
def test_thomas_rows_are_bitwise_the_oracle_rhs(norm):
    so = O.System('tomlab', normalized=norm)
    rng = np.random.default_rng(3)
    U = rng.uniform(-20, 20, (2000, 3))
    if norm:
        U = so.fit(U)
    ref = np.array([so.rhs(u) for u in U])
    f = _thomas(norm)
    assert np.array_equal(f(U), ref)
    assert np.array_equal(f(U[5]), ref[5])


@pytest.mark.parametrize('norm', [False, True])
@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('mode', ['fixed', 'linspace'])
def test_thomas_rows_are_bitwise_the_oracle_rk(norm, order, mode):
    so = O.System('tomlab', normalized=norm)
    f = _thomas(norm)
    m = O.STEP_FIXED if mode == 'fixed' else O.STEP_LINSPACE
    rng = np.random.default_rng(order)
    for steps, t0, t1 in SPANS:
        u0 = so.fit(np.array(THOMAS_U0) + rng.standard_normal(3))
        assert np.array_equal(rk_np(f, order, t0, t1, steps, u0, mode), so.rk(order, t0, t1, steps, u0, m)), steps


@pytest.mark.parametrize('rows,centre,bounds', [(BRUS, [1.0, 3.07], ([0.4, 0.9], [4.0, 5.0])),
                                                (lorenz96(40), [2.0] * 40, (-12.0, 16.0))])
def test_zero_atoms_is_bitwise_the_polynomial_restatement(rows, centre, bounds):
    rng = np.random.default_rng(5)
    U = np.array(centre) + rng.uniform(-1, 1, (200, len(centre)))
    assert np.array_equal(FuncNP([], rows)(U), PolyNP(rows)(U))
    Un = rng.uniform(-0.9, 0.9, (200, len(centre)))
    f, p = FuncNP([], rows, *bounds), PolyNP(rows, *bounds)
    assert np.array_equal(f(Un), p(Un))
    assert np.array_equal(rk_np(f, 4, 0.0, 0.05, 7, Un[:5], 'linspace'), rk_np(p, 4, 0.0, 0.05, 7, Un[:5], 'linspace'))


def test_atom_argument_order_and_absent_parts():
    """x = a u[i], then + c u[j], then + b, one rounding each; an absent b is not an added 0.0:
    recip(1.0 * -0.0) is -inf, recip(1.0 * -0.0 + 0.0) would be +inf"""
    f = FuncNP([('recip', (1.0, 0)), ('recip', (1.0, 0), 0.0), ('sqrt', (0.1, 0), (0.2, 1), 0.3)],
               [[(1.0, (2,))], [(1.0, (3,))]])
    v = f.atom_values(np.array([-0.0, 3.0]))
    assert v[0] == -np.inf and v[1] == np.inf
    v = f.atom_values(np.array([7.0, 3.0]))
    assert v[2] == np.sqrt((0.1 * 7.0 + 0.2 * 3.0) + 0.3)
    assert parse_atom(('sin', (1, 2), 4)) == ('sin', (1.0, 2), None, 4.0)
    assert parse_atom(('sin', (1, 2), (3, 0))) == ('sin', (1.0, 2), (3.0, 0), None)


def test_domain_errors_are_what_the_routines_give():
    f = FuncNP([('log', (1.0, 0)), ('sqrt', (1.0, 0)), ('recip', (1.0, 1))], [[(1.0, (2,))], [(1.0, (3,)), (1.0, (4,))]])
    out = f(np.array([-1.0, 0.0]))
    assert np.isnan(out[0]) and np.isnan(out[1])


def test_synthetic_systems_cover_every_function_and_argument_shape():
    for d, na in ((5, 1), (40, 130), (1025, 1025)):
        S = synthetic(d, na)
        kinds = {(a[0], len(a)) for a in S['atoms']}
        assert len(S['atoms']) == na and len(S['rows']) == d
        if na >= 24:
            assert {k[0] for k in kinds} == {'sin', 'cos', 'exp', 'log', 'recip', 'sqrt'}
    lane = [synthetic(D, 4, shift=s) for D in (1, 2, 3, 4) for s in (0, 2)]
    assert {a[0] for S in lane for a in S['atoms']} == {'sin', 'cos', 'exp', 'log', 'recip', 'sqrt'}
    shapes = {(len(a), np.isscalar(a[-1])) for S in lane for a in S['atoms']}
    assert shapes == {(2, False), (3, False), (3, True), (4, True)}


# ------------------------------------------------------------------------------------------------
# against the reference's recorded outputs
# ------------------------------------------------------------------------------------------------
def _system(key):
    S = GOLDEN_SYSTEMS[key]()
    return S, FuncNP(S['atoms'], S['rows'])


def _row_bound(f, S, U):
    return (16 + n_terms(S['rows'])) * EPS * f.term_magnitudes(U)


@pytest.mark.parametrize('key', list(GOLDEN_SYSTEMS))
def test_rhs_against_the_reference(key):
    R = golden('func.npz')
    S, f = _system(key)
    U, ref = R[f'rhs__{key}__u'], R[f'rhs__{key}__f']
    assert U.shape == (16, len(S['u0']))
    err, bound = np.abs(f(U) - ref), _row_bound(f, S, U)
    print(key, 'rhs worst error / bound', float(np.max(err / bound)))
    assert np.all(err <= bound)


def test_the_fixture_covers_all_six_functions():
    fns = {parse_atom(a)[0] for key in GOLDEN_SYSTEMS for a in GOLDEN_SYSTEMS[key]()['atoms']}
    assert fns == {'sin', 'cos', 'exp', 'log', 'recip', 'sqrt'}
    assert len(GOLDEN_SYSTEMS['kuramoto']()['atoms']) == 56 and len(GOLDEN_SYSTEMS['sinegordon']()['u0']) == 64
    assert len(GOLDEN_SYSTEMS['bratu']()['u0']) == 40


@pytest.mark.parametrize('key', list(GOLDEN_SYSTEMS))
@pytest.mark.parametrize('order', [1, 4, 8])
def test_rk_against_the_reference(key, order):
    R = golden('func.npz')
    S, f = _system(key)
    k = f'rk__{key}__RK{order}'
    t0, t1, steps = R[k + '__span']
    assert steps == 32
    h = (t1 - t0) / steps
    u0 = R[k + '__u0']
    for mode in ('fixed', 'linspace'):
        ref = R[k + '__' + mode]
        got = rk_np(f, order, t0, t1, int(steps), u0, mode)
        mag = np.maximum(np.abs(u0) + h * f.term_magnitudes(u0), np.abs(ref) + h * f.term_magnitudes(ref))
        bound = 64 * (16 + n_terms(S['rows'])) * EPS * mag
        err = np.abs(got - ref)
        print(key, order, mode, 'end state worst error / bound', float(np.max(err / bound)))
        assert np.all(err <= bound)


def test_adaptive_restatement_takes_the_func_rhs():
    """adaptive_ref.solve on the pendulum: reaches t1, and a tighter tolerance moves the end state by
    less than the looser tolerance's own error scale"""
    S, f = _system('pendulum')
    a = solve(f, 'RK45', 0.0, 1.0, 4, np.array(S['u0']), rtol=1e-6, atol=1e-9)
    b = solve(f, 'RK45', 0.0, 1.0, 4, np.array(S['u0']), rtol=1e-9, atol=1e-12)
    assert a[4] == 0 and b[4] == 0 and np.max(np.abs(a[0] - b[0])) < 1e-5


# ------------------------------------------------------------------------------------------------
# the library: tables, handles, refusals (no HIP call is reached)
# ------------------------------------------------------------------------------------------------
def _create(L, d, atoms, row_ptr, coef, idx):
    from nngp_amd import _lib
    recs = (_lib.CFuncAtom * max(len(atoms), 1))(*[_lib.CFuncAtom(*a) for a in atoms])
    rp = np.ascontiguousarray(row_ptr, dtype=np.int32)
    cf = np.ascontiguousarray(coef, dtype=np.float64)
    ix = np.ascontiguousarray(idx, dtype=np.int16).reshape(-1)
    h = ctypes.c_int32(0)
    rc = L.nngp_func_create(d, len(atoms), recs, len(cf), rp.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                            cf.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                            ix.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)), ctypes.byref(h))
    return rc, h.value


# atoms as (fn, i, j, has_b, a, c, b); term indices 2 and 3 are the atoms
GOOD = dict(d=2, atoms=[(1, 0, -1, 0, 1.0, 0.0, 0.0), (3, 1, 0, 1, 0.5, 0.25, 1.0)], row_ptr=[0, 1, 2],
            coef=[1.0, -2.0], idx=[[0, 2, -1], [3, -1, -1]])


def _atom(**kw):
    a = dict(fn=1, i=0, j=-1, has_b=0, a=1.0, c=0.0, b=0.0)
    a.update(kw)
    return [(a['fn'], a['i'], a['j'], a['has_b'], a['a'], a['c'], a['b']), GOOD['atoms'][1]]


@pytest.mark.parametrize('change,word', [
    (dict(d=0), 'd=0'), (dict(d=2049), 'd=2049'),
    (dict(atoms=_atom(fn=0)), 'function id 0'), (dict(atoms=_atom(fn=7)), 'function id 7'),
    (dict(atoms=_atom(i=2)), 'i=2'), (dict(atoms=_atom(i=-1)), 'i=-1'),
    (dict(atoms=_atom(j=2)), 'j=2'), (dict(atoms=_atom(j=-2)), 'j=-2'),
    (dict(atoms=_atom(has_b=2)), 'has_b=2'),
    (dict(atoms=_atom(a=np.inf)), 'finite'), (dict(atoms=_atom(c=np.nan)), 'finite'), (dict(atoms=_atom(b=-np.inf)), 'finite'),
    (dict(row_ptr=[1, 1, 2]), 'row_ptr[0]'), (dict(row_ptr=[0, 2, 1]), 'non-decreasing'),
    (dict(row_ptr=[0, 1, 1]), 'row_ptr[d]'), (dict(row_ptr=[0, 1, 3]), 'n_terms'),
    (dict(idx=[[0, 4, -1], [1, -1, -1]]), 'index 4'), (dict(idx=[[0, -2, -1], [1, -1, -1]]), 'index -2'),
    (dict(idx=[[-1, 0, -1], [1, -1, -1]]), 'after a -1'),
    (dict(coef=[np.inf, 1.0]), 'finite'), (dict(coef=[1.0, np.nan]), 'finite'),
])
def test_create_refuses_a_bad_table(change, word):
    from nngp_amd import _lib
    L = _lib.lib()
    rc, h = _create(L, **dict(GOOD, **change))
    msg = L.nngp_last_error().decode()
    assert rc == -1 and h == 0 and 'func' in msg and word in msg, msg


def test_create_refuses_counts_out_of_range_and_null_arguments():
    from nngp_amd import _lib
    L = _lib.lib()
    h = ctypes.c_int32(0)
    rp = (ctypes.c_int32 * 3)(0, 1, 2)
    one = (_lib.CFuncAtom * 1)(_lib.CFuncAtom(1, 0, -1, 0, 1.0, 0.0, 0.0))

    def refused(word, *args):
        assert L.nngp_func_create(*args) == -1
        msg = L.nngp_last_error().decode()
        assert 'func' in msg and word in msg, msg

    refused('n_atoms', 2, 2049, one, 0, rp, None, None, ctypes.byref(h))
    refused('n_atoms', 2, -1, one, 0, rp, None, None, ctypes.byref(h))
    refused('n_terms', 2, 0, None, 1048577, rp, None, None, ctypes.byref(h))
    refused('n_terms', 2, 0, None, -1, rp, None, None, ctypes.byref(h))
    refused('atoms is NULL', 2, 1, None, 0, rp, None, None, ctypes.byref(h))
    refused('coef / idx', 2, 0, None, 2, rp, None, None, ctypes.byref(h))
    refused('row_ptr is NULL', 2, 0, None, 0, None, None, None, ctypes.byref(h))
    refused('handle_out', 2, 0, None, 0, (ctypes.c_int32 * 3)(0, 0, 0), None, None, None)
    assert h.value == 0


def test_the_largest_table_is_accepted():
    from nngp_amd import _lib
    L = _lib.lib()
    atoms = [(1 + q % 6, q, -1, 0, 1.0, 0.0, 0.0) for q in range(2048)]
    rc, h = _create(L, d=2048, atoms=atoms, row_ptr=list(range(2049)), coef=[1.0] * 2048,
                    idx=[[2048 + c, -1, -1] for c in range(2048)])
    assert rc == 0 and h >= 1 and L.nngp_func_destroy(h) == 0


def test_handles_are_created_destroyed_and_reused():
    from nngp_amd import _lib
    L = _lib.lib()
    rc, a = _create(L, **GOOD)
    rc2, b = _create(L, **GOOD)
    assert rc == 0 and rc2 == 0 and a >= 1 and b >= 1 and a != b
    rc, empty = _create(L, d=3, atoms=[], row_ptr=[0, 0, 0, 0], coef=[], idx=[])   # no atoms, no terms: valid
    assert rc == 0 and empty not in (a, b)
    assert L.nngp_func_destroy(a) == 0
    assert L.nngp_func_destroy(a) == -1 and 'func' in L.nngp_last_error().decode()   # twice
    rc, c = _create(L, **GOOD)
    assert rc == 0 and c == a                        # the freed slot is handed out again
    for h in (b, c, empty):
        assert L.nngp_func_destroy(h) == 0
    for h in (0, -1, 10 ** 6):
        assert L.nngp_func_destroy(h) == -1


def test_func_and_poly_handles_are_separate_registries():
    from nngp_amd import _lib
    L = _lib.lib()
    rc, h = _create(L, **GOOD)
    assert rc == 0
    try:
        cs = _lib.CSystem(_lib.SYS_POLY, 2, h + 500, 0, (ctypes.c_double * 4)(), None)
        buf = (ctypes.c_double * 16)()
        assert L.nngp_rhs_batch(ctypes.byref(cs), 1, ctypes.addressof(buf), ctypes.addressof(buf), None) == -1
        assert 'poly' in L.nngp_last_error().decode()
    finally:
        L.nngp_func_destroy(h)


def test_equal_func_and_poly_handles_name_different_tables():
    """A func table (d = 2) and a poly table (d = 3) under the same handle number: each kind resolves
    its own table and is refused the other's d, and destroying one leaves the other.  (n_slices = 0:
    nngp_rk_adaptive returns right after the table lookup, before any HIP call.)"""
    from nngp_amd import _lib
    L = _lib.lib()
    rc, h = _create(L, **GOOD)
    assert rc == 0 and h >= 1
    rp = (ctypes.c_int32 * 4)(0, 0, 0, 0)   # d = 3, no terms: valid
    made, same, func_live = [], None, True

    def lookup(kind, d):
        cs = _lib.CSystem(kind, d, h, 0, (ctypes.c_double * 4)(), None)
        rc = L.nngp_rk_adaptive(ctypes.byref(cs), 45, 0, None, None, 4, 1e-3, 1e-6, 0.0, 100, None, None, None, None)
        return rc, L.nngp_last_error().decode()

    try:
        for _ in range(4096):   # each registry hands out its lowest free slot: h comes within h creations
            p = ctypes.c_int32(0)
            assert L.nngp_poly_create(3, 0, rp, None, None, ctypes.byref(p)) == 0
            made.append(p.value)
            if p.value == h:
                same = p.value
                break
        assert same == h, f'no poly table with handle {h} after {len(made)} creations'
        assert lookup(_lib.SYS_POLY, 3)[0] == 0
        assert lookup(_lib.SYS_FUNC, 2)[0] == 0
        rc, msg = lookup(_lib.SYS_POLY, 2)
        assert rc == -1 and 'poly' in msg and 'd=2' in msg, msg
        rc, msg = lookup(_lib.SYS_FUNC, 3)
        assert rc == -1 and 'func' in msg and 'd=3' in msg, msg
        assert L.nngp_func_destroy(h) == 0
        func_live = False
        assert lookup(_lib.SYS_POLY, 3)[0] == 0
        assert lookup(_lib.SYS_FUNC, 2)[0] == -1
    finally:
        for p in made:
            L.nngp_poly_destroy(p)
        if func_live:
            L.nngp_func_destroy(h)


@pytest.mark.parametrize('case', ['unknown', 'destroyed', 'zero', 'other_d'])
def test_library_refuses_bad_descriptors_without_a_gpu(case):
    """NNGP_E_ARG from the host-side lookup, before any HIP call (the pointers are placeholders that
    are never dereferenced): every tableau and step mode, the trajectory, the adaptive propagator
    and the right-hand side."""
    from nngp_amd import _lib
    L = _lib.lib()
    rc, live = _create(L, **GOOD)
    assert rc == 0
    try:
        d, word = 2, 'handle'
        if case == 'unknown':
            h = live + 1000
        elif case == 'zero':
            h = 0
        elif case == 'destroyed':
            rc, h = _create(L, **GOOD)
            assert L.nngp_func_destroy(h) == 0
        else:
            h, d, word = live, 3, 'd=3'
        cs = _lib.CSystem(_lib.SYS_FUNC, d, h, 0, (ctypes.c_double * 4)(), None)
        buf = (ctypes.c_double * 16)()
        ptr = ctypes.addressof(buf)

        def refused(rc):
            msg = L.nngp_last_error().decode()
            assert rc == -1 and 'func' in msg and word in msg, msg

        for tab in (1, 2, 4, 8):
            for mode in (_lib.STEP_FIXED, _lib.STEP_LINSPACE, _lib.STEP_FIXED | _lib.STEP_CONTRACT,
                         _lib.STEP_LINSPACE | _lib.STEP_CONTRACT):
                refused(L.nngp_rk_batch(ctypes.byref(cs), tab, mode, 1, ptr, ptr, 3, ptr, ptr, None))
                refused(L.nngp_rk_traj(ctypes.byref(cs), tab, mode, 1, ptr, ptr, 3, 1, ptr, ptr + 64, None))
            refused(L.nngp_rk_batch_grid(ctypes.byref(cs), tab, 1, ptr, ptr, 3, ptr, 3, ptr, ptr, None))
        for method in (23, 45):
            refused(L.nngp_rk_adaptive(ctypes.byref(cs), method, 1, ptr, ptr, 4, 1e-3, 1e-6, 0.0, 100, ptr, ptr, None,
                                       None))
        refused(L.nngp_rhs_batch(ctypes.byref(cs), 1, ptr, ptr, None))
    finally:
        L.nngp_func_destroy(live)


# ------------------------------------------------------------------------------------------------
# the Python surface
# ------------------------------------------------------------------------------------------------
PEND = dict(atoms=[('sin', (1.0, 0))], terms=[[(1.0, (1,))], [(-1.0, (2,)), (-0.1, (1,))]], u0=[1.0, 0.0])


def test_funcode_is_exported():
    import nngp_amd
    from nngp_amd import _lib
    assert 'FuncODE' in nngp_amd.__all__ and issubclass(nngp_amd.FuncODE, nngp_amd.ODE)
    assert _lib.SYS_FUNC == 11 and nngp_amd.FuncODE.kind == 11
    assert _lib.FUNC_FN == {'sin': 1, 'cos': 2, 'exp': 3, 'log': 4, 'recip': 5, 'sqrt': 6}
    assert ctypes.sizeof(_lib.CFuncAtom) == 40


def test_funcode_descriptor_fields():
    import nngp_amd
    from nngp_amd import _lib
    ode = nngp_amd.FuncODE(**PEND)
    assert ode.name == 'FuncODE' and ode.d == 2 and ode.get_dim() == 2 and not ode.normalized and ode.param == ()
    assert ode.atoms == [('sin', (1.0, 0), None, None)]
    assert ode._handle is None                      # made on first use of the descriptor
    f = ode.get_vector_field()
    assert isinstance(f, nngp_amd.VectorField) and ode._handle is None
    cs = f.csystem('cpu')
    assert (cs.kind, cs.d, cs.normalized, cs.norm) == (11, 2, 0, None) and cs.nx == ode._handle >= 1
    assert ode.get_vector_field().csystem('cpu').nx == cs.nx       # one table per object
    assert np.array_equal(ode.get_init_cond(), [1.0, 0.0])
    h = ode._handle
    ode.destroy()
    assert _lib.lib().nngp_func_destroy(h) == -1     # gone
    other = nngp_amd.FuncODE(atoms=[('exp', (1.0, 0), (0.5, 0), -0.25)], terms=[[(1.0, (1,))]], u0=[0.5], name='growth')
    assert other.nx == h and other.name == 'growth'  # the slot is reused
    rec = other._atoms[0]
    assert (rec.fn, rec.i, rec.j, rec.has_b, rec.a, rec.c, rec.b) == (3, 0, 0, 1, 1.0, 0.5, -0.25)
    del other
    assert _lib.lib().nngp_func_destroy(h) == -1     # destroyed with the object


def test_funcode_normalisation_needs_bounds():
    import nngp_amd
    with pytest.raises(ValueError, match='FuncODE.*mn and mx'):
        nngp_amd.FuncODE(normalization='-11', **PEND)
    ode = nngp_amd.FuncODE(mn=THOMAS_BOUNDS[0], mx=THOMAS_BOUNDS[1], normalization='-11', atoms=THOMAS_ATOMS,
                           terms=THOMAS_ROWS, u0=THOMAS_U0)
    ref = nngp_amd.ThomasLabyrinth(normalization='-11')
    assert ode.normalized and np.array_equal(ode.get_init_cond(), ref.get_init_cond())
    assert np.array_equal(ode.normalizer.device_table(3), ref.normalizer.device_table(3))


@pytest.mark.parametrize('atoms,terms,u0,word', [
    ([], [[(1.0, (0,))]], [1.0, 2.0], 'rows'),
    ([], [[(1.0, (0,))]], [[1.0]], 'u0'),
    ([], [[(1.0, (0, 0, 0, 0))]], [1.0], 'row 0.*degree'),
    ([('sin', (1.0, 0))], [[(1.0, (2,))]], [1.0], 'row 0.*index'),
    ([], [[(1.0, (-1,))]], [1.0], 'row 0.*index'),
    ([], [[(np.nan, ())]], [1.0], 'row 0.*finite'),
    ([], [[]] * 2049, np.ones(2049), '2048'),
    ([('sin', (1.0, 0))] * 2049, [[]], [1.0], '2049 atoms'),
    ([('tan', (1.0, 0))], [[]], [1.0], "atom 0.*'tan'"),
    ([('sin', (1.0, 0)), ('sin', (1.0, 1))], [[]], [1.0], 'atom 1.*state index'),
    ([('sin', (1.0, 0), (1.0, -1))], [[]], [1.0], 'atom 0.*state index'),
    ([('sin', (np.inf, 0))], [[]], [1.0], 'atom 0.*finite'),
    ([('sin', (1.0, 0), np.nan)], [[]], [1.0], 'atom 0.*b that is not finite'),
    ([('sin',)], [[]], [1.0], 'atom 0 must be'),
    ([('sin', 1.0)], [[]], [1.0], 'atom 0 must be'),
    ([('sin', (1.0, 0), (1.0, 0), (1.0, 0))], [[]], [1.0], 'atom 0 must be'),
    ([('sin', (1.0, 0, 0))], [[]], [1.0], 'atom 0.*pair'),
    (['sin'], [[]], [1.0], 'atom 0 must be'),
])
def test_funcode_refuses_bad_input(atoms, terms, u0, word):
    import nngp_amd
    with pytest.raises(ValueError, match='FuncODE.*' + word):
        nngp_amd.FuncODE(atoms=atoms, terms=terms, u0=u0)


def test_solvers_accept_a_funcode_unchanged():
    import nngp_amd
    ode = nngp_amd.FuncODE(mn=[-2.0, -2.0], mx=[2.0, 2.0], normalization='-11', **PEND)
    s = nngp_amd.SolverRK(ode.get_vector_field(), Ng=4, Nf=40, F='RK4', G='RK1')
    p = nngp_amd.Parareal(ode, s, [0, 8], 16, verbose=None)
    assert p.N == 16 and s.step_mode == 0
    assert nngp_amd.SolverRK(ode.get_vector_field(), 4, 40, 'RK8', 'RK2', step_mode='linspace', fma=True).step_mode == 17
    sc = nngp_amd.SolverScipy(ode.get_vector_field(), Ng=4, Nf=40, F='RK45', G='RK4')
    assert nngp_amd.PararealLight is not None and sc is not None
    with pytest.raises(nngp_amd.NNGPError) if not _has_gpu() else _null():
        s.run_F(0.0, 0.5, ode.get_init_cond())


def _has_gpu():
    import torch
    return torch.cuda.is_available()


class _null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False
