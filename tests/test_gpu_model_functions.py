"""Generated model math on the device, function family by function family (run with -m gpu on an MI355X): the
evaluation kernels on pycollo_amd.problems.function_family against the mpmath oracle -- every model function and
partial evaluated at 60 digits and rounded once (OracleNlp(fn_modules="mpmath")), assembled by the fp64 code every
other parity test trusts.  Tolerance as everywhere: index arrays equal, every entry of c~ / G~ / H~ within
1e-10 |ref| + 64 eps mag of the oracle (conftest.entry_err), no entry skipped.

Node functions run one node per lane, so a mesh only has to supply interior nodes, section-boundary nodes and a partly
filled tile: K = 5, order 4 (16 nodes, the order-4 build) and one ragged mesh of orders 2..10 (any-order build, a full
64-node tile and a partial one).

Kink margin: at the random points every kink argument (model_function_cases.kink_arguments) at every node is at least
1e-6 from its tie -- the device's x = V x~ + r may differ from the oracle's in the last bit, which must not change
sides.  This is a condition on the inputs (counted on the reference side, required to be 0), not a tolerance.  The edge
test plants exact ties with ``scaling_method = None`` (x~ is the variable itself), where both sides see the same inputs.
"""
import numpy as np
import pytest

from conftest import entry_err, golden_tables, vec_err
from model_function_cases import FAMILIES, family_problem, kink_violations, plant_edges, ragged_mesh
from oracle.ref_numpy import OracleNlp

pytestmark = pytest.mark.gpu
TOL = 1e-10
SEEDS = {"powers": 1, "trig": 1, "special": 1, "kinks": 1}     # (kinks: checked to leave the margin on both meshes)


@pytest.fixture(scope="module")
def tab():
    return golden_tables("lobatto")


def _engine(prob, **kw):
    from pycollo_amd.engine import NlpEngine
    return NlpEngine(prob, device=0, **kw)


def _check_all(eng, ora, x, lam, sigma=0.6):
    c, G, H = eng.evaluate_all(x, sigma, lam)
    cr, Gr, Hr = ora.c(x), ora.G(x), ora.H(x, sigma, lam)
    Gm, Hm, cm = ora.G_mag(x), ora.H_mag(x, sigma, lam), ora.c_mag(x)
    for got, ref in ((eng.evaluate_G_structure(), ora.G_structure()), (eng.evaluate_H_structure(), ora.H_structure())):
        np.testing.assert_array_equal(got[0], ref[0])
        np.testing.assert_array_equal(got[1], ref[1])
    errs = {"c": entry_err(c, cr, cm, expect_unscaled=0), "G": entry_err(G, Gr, Gm, expect_unscaled=0),
            "H": entry_err(H, Hr, Hm, expect_unscaled=0)}
    print("fused call, ratio to the bound:", {k: f"{v:.3g}" for k, v in errs.items()})
    assert errs["c"] <= 1.0 and errs["G"] <= 1.0 and errs["H"] <= 1.0, errs
    # the separate callbacks
    assert entry_err(eng.evaluate_c(x), cr, cm, expect_unscaled=0) <= 1.0
    assert entry_err(eng.evaluate_G_nonzeros(x, new_x=False), Gr, Gm, expect_unscaled=0) <= 1.0
    assert entry_err(eng.evaluate_H_nonzeros(x, sigma, lam), Hr, Hm, expect_unscaled=0) <= 1.0
    assert abs(eng.evaluate_J(x) - ora.J(x)) <= TOL * max(1.0, abs(ora.J(x)))
    assert vec_err(eng.evaluate_g(x), ora.grad_J(x)) <= 1.0


def _scaled_pair(prob, tab, tpb, **kw):
    eng = _engine(prob, threads_per_block=tpb, **kw)
    rng = np.random.default_rng(11)
    W = rng.uniform(0.5, 2.0, eng.layout.num_ocp_c)
    eng.set_scaling(eng.V_ocp, eng.r_ocp, W, 1.7)
    ora = OracleNlp(prob, tab, V_ocp=eng.V_ocp, r_ocp=eng.r_ocp, W_ocp=W, w_J=1.7, fn_modules="mpmath")
    return eng, ora


def _random_point(eng, family, salt=0):
    rng = np.random.default_rng(SEEDS[family] + salt)
    return rng.uniform(-0.45, 0.45, eng.num_x), rng.normal(size=eng.num_c)


@pytest.mark.parametrize("tpb", [64, 256])
@pytest.mark.parametrize("family", FAMILIES)
def test_family_small_mesh(built, tab, family, tpb):
    prob = family_problem(family, K=5, order=4)
    eng, ora = _scaled_pair(prob, tab, tpb)
    assert eng.orders == (4,) and ora.P[0].N == 16
    x, lam = _random_point(eng, family)
    assert kink_violations(ora, x) == 0
    _check_all(eng, ora, x, lam)
    eng.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_family_ragged_mesh(built, tab, family):
    prob = ragged_mesh(family_problem(family))
    eng, ora = _scaled_pair(prob, tab, 64)
    N = ora.P[0].N
    assert eng.orders == (0,) and not any(eng.mixed) and 65 <= N <= 130
    x, lam = _random_point(eng, family, salt=100)
    assert kink_violations(ora, x) == 0
    _check_all(eng, ora, x, lam)
    eng.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_family_exact_edge_points(built, tab, family):
    """Planted values where the correct result is finite and a special-cased formula goes wrong: powers at base exactly 1,
    at base exactly 0 (integer exponents >= 3, half-integer exponents >= 5/2) and at negative bases, atan2(0, x < 0),
    every kink function at an exact tie (model_function_cases.EDGE_NODES); all in one evaluation."""
    prob = family_problem(family, K=5, order=4, scaling=None)
    eng = _engine(prob, threads_per_block=64)
    assert np.all(eng.V_ocp == 1) and np.all(eng.r_ocp == 0)
    rng = np.random.default_rng(11)
    W = rng.uniform(0.5, 2.0, eng.layout.num_ocp_c)
    eng.set_scaling(eng.V_ocp, eng.r_ocp, W, 1.7)
    ora = OracleNlp(prob, tab, V_ocp=eng.V_ocp, r_ocp=eng.r_ocp, W_ocp=W, w_J=1.7, fn_modules="mpmath")
    P = ora.P[0]
    # a point of the bounds box (x~ is x here), then the edge nodes
    lo, hi = ora.bounds[:, 0], ora.bounds[:, 1]
    u01 = np.random.default_rng(SEEDS[family] + 200).uniform(0.05, 0.95, eng.num_x)
    x = np.empty(eng.num_x)
    for j in range(P.n_z):
        x[P.x_off + j * P.N:P.x_off + (j + 1) * P.N] = lo[j] + (hi[j] - lo[j]) * u01[P.x_off + j * P.N:P.x_off + (j + 1) * P.N]
    rest = np.arange(P.q_off, eng.num_x)
    x[rest] = lo[P.n_z:] + (hi[P.n_z:] - lo[P.n_z:]) * u01[rest]
    x = plant_edges(family, x, P.N, P.n_z, P.x_off)
    lam = rng.normal(size=eng.num_c)
    assert kink_violations(ora, x, exact_ties_ok=True) == 0
    if family == "kinks":
        assert kink_violations(ora, x) >= 10       # the planted ties are there
    _check_all(eng, ora, x, lam)
    eng.close()
