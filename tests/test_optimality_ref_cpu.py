"""The definition of the path and bound multipliers and of H_y, H_u, checked without a GPU.

1. The identity, on the restatement (tests/optimality_ref.py).  The dual residual of the scaled NLP from the oracle's own
   G~ and grad J~, r~ = grad J~ + G~^T lam~ + z~, against the right-hand sides
       control b, weighted nodes:   w V_b stretch omega_j (H_u[b](j) + zeta_u[b](j))
       state a, interior nodes:     w V_a (stretch omega_j (H_y[a](j) + zeta_y[a](j)) + D_a(j))
   entry by entry: |lhs - rhs| <= 1e-10 |rhs| + 64 eps (|G~|^T |lam~| + |z~|), the magnitudes from ``G_mag``.  Cases: every
   case of ``test_gpu_costate.CASES`` with a control or a path row, Radau included; random lam~, z~, W in [0.5, 2],
   w = 0.7.
2. End to end on the host: hypersensitive, final time 10, order 8, K = 8, u in [-0.2, 50], solved by the host
   interior-point solver on the oracle's functions (``propagate_ref.cpu_solve``), tol 1e-10.  The lower control bound is
   active over part of the mesh: |H_u| is large there and H_u + zeta_u is zero to the solver's tolerance.
3. Argument errors of ``Solution`` raise ``ValueError`` before any device call.
"""
import numpy as np
import pytest

import optimality_ref as oref
from conftest import golden_tables
from oracle.ref_numpy import OracleNlp
from pycollo_amd import problems
from test_gpu_costate import CASES, W_J

EPS = np.finfo(float).eps


def _method(prob):
    return getattr(prob, "quadrature_method", "lobatto") or "lobatto"


def random_point(prob, seed=41):
    """(oracle with a random W in [0.5, 2] and w = W_J, tables, x~, lam~, z~)"""
    tables = golden_tables(_method(prob))
    base = OracleNlp(prob, tables)
    rng = np.random.default_rng(seed)
    ora = OracleNlp(prob, tables, V_ocp=base.V_ocp, r_ocp=base.r_ocp, W_ocp=rng.uniform(0.5, 2.0, base.num_ocp_c), w_J=W_J)
    x = rng.uniform(-0.2, 0.2, ora.num_x)
    for P in ora.P:
        x[P.q_off:P.q_off + P.n_q + P.n_t] = rng.uniform(0.1, 0.3, P.n_q + P.n_t)
    return ora, tables, x, 0.1 * rng.normal(size=ora.num_c), 0.1 * rng.normal(size=ora.num_x)


def assert_identity(cols, lhs, rhs, scale, what):
    assert len(cols) > 0
    ratio = np.abs(lhs - rhs) / (1e-10 * np.abs(rhs) + 64 * EPS * scale)
    print(f"{what}: {len(cols)} columns, largest |lhs - rhs| / bound = {np.max(ratio):.3e}, "
          f"largest |lhs - rhs| / max |rhs| = {np.max(np.abs(lhs - rhs)) / np.max(np.abs(rhs)):.3e}")
    assert np.all(ratio <= 1.0), f"{what}: column {cols[int(np.argmax(ratio))]} misses the identity by {np.max(ratio):.3e} x its bound"


@pytest.mark.parametrize("name", list(CASES))
def test_identity_on_the_restatement(name):
    prob = CASES[name]()
    ora, tables, x, lam, z = random_point(prob)
    assert any(P.n_u > 0 or P.n_p > 0 for P in ora.P), "every case of the list has a control or a path row"
    cols, lhs, rhs, scale = oref.identity_sides(ora, tables, x, lam, z, W_J)
    n_cols = sum(P.n_u * int(np.count_nonzero(oref.NodeReference(ora, tables, x, lam, z, ip, w_J=W_J).weighted))
                 + P.n_y * (P.N - 2) for ip, P in enumerate(ora.P))
    assert len(cols) == n_cols                 # every control column at a weighted node, every interior state column
    assert_identity(cols, lhs, rhs, scale, name)


def test_identity_needs_every_term():
    """the check is not vacuous: without the path term or without zeta the identity fails by orders of magnitude on a
    problem with a path row"""
    ora, tables, x, lam, z = random_point(CASES["two_phase_transfer_K6"]())
    assert any(P.n_p > 0 for P in ora.P)
    cols, lhs, rhs, scale = oref.identity_sides(ora, tables, x, lam, z, W_J)
    bound = 1e-10 * np.abs(rhs) + 64 * EPS * scale
    lam0 = lam.copy()
    for P in ora.P:
        lam0[P.c_path:P.c_int] = 0.0
    for other in (oref.identity_sides(ora, tables, x, lam0, z, W_J)[2], oref.identity_sides(ora, tables, x, lam, 0 * z, W_J)[2]):
        assert np.max(np.abs(lhs - other) / bound) > 1e6


def test_interpolant_derivative_restatement():
    """SectionInterpolant reproduces a polynomial and its derivative (the helper the GPU tests lean on)"""
    from pycollo_amd.solution import exact_tables, section_points
    from pycollo_amd.quadrature import QuadratureTables
    for method, n in (("lobatto", 7), ("radau", 5)):
        pts = section_points(QuadratureTables(method), n)
        poly = np.polynomial.Polynomial([0.3, -1.0, 0.5, 2.0])
        s = oref.SectionInterpolant(exact_tables(method, n)[1], poly(pts)[None, :])
        for c in (-1.0, -0.3, 0.0, 0.77, 1.0):
            assert abs(s.value(c)[0] - poly(c)) <= 1e-14 and abs(s.derivative(c)[0] - poly.deriv()(c)) <= 1e-13


# ---- end to end on the host -----------------------------------------------------------------------------------
def bounded_hypersensitive(K=8):
    """hypersensitive, final time 10, order 8, u in [-0.2, 50] (an upper bound of 3 makes it infeasible)"""
    prob = problems.hypersensitive(K=K, order=8)
    ph = prob.phases[0]
    ph.bounds.final_time = 10.0
    ph.guess.time = ph.guess.time * 1e-3
    ph.bounds.control_variables = [[-0.2, 50]]
    return prob


@pytest.fixture(scope="module")
def host_solution():
    prob = bounded_hypersensitive()
    tables = golden_tables("lobatto")
    ora, res = oref.cpu_solve_with_multipliers(prob, tables, tol=1e-10)
    return prob, tables, ora, res


def test_bounded_hypersensitive_on_the_host(host_solution):
    prob, tables, ora, res = host_solution
    assert res.success, res.status
    x, lam, z = np.asarray(res.x, float), np.asarray(res.lam, float), np.asarray(res.zu, float) - np.asarray(res.zl, float)
    ref = oref.NodeReference(ora, tables, x, lam, z, 0)
    P = ora.P[0]
    u = ora._unpack(P, x)[0][P.n_y]
    H_u, zeta_u = ref.H_z[P.n_y].astype(float), ref.zeta[P.n_y].astype(float)
    active = np.abs(H_u) >= 0.1
    mid = oref.host_section_costate_residual(ora, tables, x, lam, z, k=P.mesh.K // 2)
    print(f"bounded hypersensitive on the host, K = 8: {res.iterations} iterations; max |H_u| = {np.max(np.abs(H_u)):.4e} "
          f"({int(active.sum())} of {P.N} nodes >= 0.1); max |H_u + zeta_u| = {np.max(np.abs(H_u + zeta_u)):.3e}; "
          f"max zeta_u = {np.max(zeta_u):.3e}; max |zeta_u| (u + 0.2) = {np.max(np.abs(zeta_u) * (u + 0.2)):.3e}; "
          f"mid-section max |dp + H_y + zeta_y| = {mid:.4e}")
    assert int(active.sum()) >= 1
    assert np.max(np.abs(H_u + zeta_u)) <= 1e-6          # the solver's acceptable tolerance
    assert np.all(zeta_u <= 0.0)
    assert np.all(np.abs(zeta_u) * (u + 0.2) <= 1e-6)
    # the costate equation as the NLP discretises it holds at the interior nodes to the same tolerance
    cd = ref.costate_defect().astype(float)
    assert np.nanmax(np.abs(cd)) <= 1e-6 * max(1.0, float(np.max(np.abs(ref.p))))


# ---- argument errors: ValueError before any device call ------------------------------------------------------
class _NoDeviceEngine:
    """stands in for an engine: any use beyond the sizes is a device call the check should have come before"""
    num_x, num_c = 30, 25

    def __getattr__(self, name):
        raise AssertionError(f"Solution touched engine.{name} before refusing its arguments")


@pytest.mark.parametrize("bad", [
    np.zeros(29), np.zeros(31), np.zeros(30, dtype=np.float32), np.zeros((1, 30)), np.zeros(60)[::2],
    (np.zeros(30), np.zeros(29)), (np.zeros(30),), (np.zeros(30), np.zeros(30), np.zeros(30)),
    (np.zeros(30, dtype=np.int64), np.zeros(30)),
])
def test_refused_bound_multipliers(bad):
    from pycollo_amd.solution import Solution
    with pytest.raises(ValueError, match="bound_multipliers"):
        Solution(_NoDeviceEngine(), np.zeros(30), multipliers=np.zeros(25), bound_multipliers=bad)


def test_bound_multipliers_need_multipliers():
    from pycollo_amd.solution import Solution, signed_bound_multipliers
    with pytest.raises(ValueError, match="need multipliers"):
        Solution(_NoDeviceEngine(), np.zeros(30), bound_multipliers=np.zeros(30))
    zl, zu = np.arange(30.0), np.ones(30)
    np.testing.assert_array_equal(signed_bound_multipliers((zl, zu), 30, True), zu - zl)
    z = np.linspace(-1, 1, 30)
    assert signed_bound_multipliers(z, 30, True) is z and signed_bound_multipliers(None, 30, False) is None


def _detached_solution(closed):
    """a Solution with one phase and no device behind it"""
    from pycollo_amd.solution import Solution
    s = object.__new__(Solution)
    s.state = (np.zeros((1, 3)),)
    s.costate = (np.zeros((1, 3)),)
    s.initial_time, s.final_time = (0.0,), (1.0,)
    s._h = None if closed else 1
    s._optimality = None
    s._z = None
    s.engine = _NoDeviceEngine()
    return s


@pytest.mark.parametrize("phase", [-1, 1, 7])
def test_phase_out_of_range(phase):
    s = _detached_solution(closed=False)
    with pytest.raises(ValueError, match="out of range"):
        s.sample_optimality(phase, tau=np.array([0.0]))
    with pytest.raises(ValueError, match="out of range"):
        s.optimality_report(phase)
    with pytest.raises(ValueError, match="out of range"):
        s.multiplier_coefficients(phase)
    s._h = None


def test_closed_solution():
    s = _detached_solution(closed=True)
    with pytest.raises(ValueError, match="closed"):
        s.sample_optimality(0, tau=np.array([0.0]))
    with pytest.raises(ValueError, match="closed"):
        s.optimality_report(0)
    for name in ("path_multiplier", "hamiltonian_gradient", "control_stationarity", "costate_defect", "bound_multiplier"):
        with pytest.raises(ValueError, match="closed"):
            getattr(s, name)
    s.costate = None                                  # made without multipliers: None, as costate is
    assert s.path_multiplier is None and s.control_stationarity is None and s.hamiltonian_gradient is None
    with pytest.raises(ValueError, match="without multipliers"):
        s.sample_optimality(0, tau=np.array([0.0]))
