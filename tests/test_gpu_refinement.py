"""Row N2: the ph mesh-error estimate on the GPU against an exact (mpmath) restatement of
pycollo/mesh_refinement.py:63-240, at points on trajectories where the estimate is near the 1e-7 tolerance the
refinement decision is taken at, and the refine -> re-solve loop.

Tolerance: entry-wise |got - ref| <= 1e-10 |ref| + 32 eps mag through conftest.entry_err, mag the
first-order running-error magnitude of the entry (oracle.ref_refine.mesh_error_mp); ``max_rel`` per section, ``max_abs``
per section and state, no entry skipped.  tests/test_refinement_cpu.py holds two float64 restatements to the same
bound at the same points."""
import warnings

import numpy as np
import pytest

import mesh_error_cases as mc
from conftest import golden_tables
from oracle.ref_numpy import OracleNlp
from oracle.ref_refine import mesh_error_mp
from pycollo_amd import problems
from pycollo_amd.quadrature import QuadratureTables

pytestmark = pytest.mark.gpu


def _assert_within_bound(got, ref, label):
    r = mc.ratios(got, ref)
    print(f"{label}: kernel: max_rel / max_abs ratio to the bound per phase {[(float(f'{a:.3g}'), float(f'{b:.3g}')) for a, b in r]}")
    for ip, (a, b) in enumerate(r):
        assert a <= 1.0, f"{label}: max_rel of phase {ip} is {a:.3g} x its bound off the exact reference"
        assert b <= 1.0, f"{label}: max_abs (per section and state) of phase {ip} is {b:.3g} x its bound off the exact reference"


@pytest.mark.parametrize("name,kw,ragged", [("hypersensitive", dict(K=40, order=5), False),
                                            ("cart_pole", dict(K=300, order=4), False),
                                            ("shuttle", dict(K=12, order=6), False),
                                            ("two_phase_transfer", dict(K=6, order=4), False),
                                            ("time_coupled_transfer", dict(K=6, order=4), False),
                                            ("cart_pole", dict(K=10, order=4), True),
                                            ("double_pendulum", dict(K=10, order=4), True)])
def test_mesh_error_matches_oracle(built, name, kw, ragged):
    """The shapes of the row's first parity test (a random cubic in tau per variable: no trajectory, estimates of
    O(1) and more), now against the exact reference, per section and state."""
    from pycollo_amd.engine import NlpEngine
    from pycollo_amd.refinement import mesh_error
    i = mc.CUBIC_CASES.index((name, kw, ragged))
    eng = NlpEngine(mc.cubic_problem(name, kw, ragged), device=0)
    ora, x, ref = mc.cubic(i, eng)
    np.testing.assert_array_equal(ora.V_ocp, eng.V_ocp)
    _assert_within_bound(mesh_error(eng, x), ref, name)
    eng.close()


def _device_engine(p):
    from pycollo_amd.engine import NlpEngine
    eng = NlpEngine(p.spec["build"](), device=0, **p.spec["engine_kw"])
    np.testing.assert_array_equal(p.V, eng.V_ocp)
    np.testing.assert_array_equal(p.r, eng.r_ocp)
    return eng


@pytest.mark.parametrize("name", list(mc.CASES))
def test_mesh_error_on_a_trajectory(built, name):
    """The kernel against mesh_error_mp at a point on a trajectory (tests/mesh_error_cases.py): ragged orders 2..10
    over four tiles, one filled to exactly 256 lanes and one closed early; every order 2..19 on its own; free t0, two
    phases, static parameters; a phase without controls; K = 1; Delta III's seven states.  From the reference alone
    the test first asserts that the case is where it is meant to be -- estimates on both sides of 1e-7 -- and that the
    bound is <= 1e-3 of every section's estimate, so that a wrong kernel cannot hide inside it.

    The two ``high_orders`` cases (hypersensitive, T = 10 000, orders 11..19) are exempt from the latter: they are
    ill-conditioned by construction (stretch h in the thousands: the bound reaches 20 times a section's estimate for
    orders 11..15, where 29 of 30 sections lie at or below their rounding bound, and 3.6 times for orders 16..19;
    profiles/mesh_error_parity.txt) and guard the INDEXING at high orders -- table offsets, lanes, tiles -- not the accuracy near the
    tolerance.  The fraction of every section is printed."""
    from pycollo_amd.refinement import mesh_error
    p = mc.point(name)
    est, frac = mc.assert_regime(name, p.ref)
    print(f"{name}: estimates {est.min():.1e}..{est.max():.1e}, bound / estimate up to {frac.max():.1e}")
    if not p.spec["sharp"]:
        print(f"{name}: bound as a fraction of the estimate, per section: {np.array2string(frac, precision=1)}")
    eng = _device_engine(p)
    _assert_within_bound(mesh_error(eng, p.x), p.ref, name)
    eng.close()


def test_mesh_error_is_reproducible(built):
    """The ragged four-tile case twice on one engine and once on a fresh one: the same bits."""
    from pycollo_amd.refinement import mesh_error
    p = mc.point("ragged_multitile")
    eng = _device_engine(p)
    (rel1, ab1), = mesh_error(eng, p.x)
    (rel2, ab2), = mesh_error(eng, p.x)
    eng.close()
    eng = _device_engine(p)
    (rel3, ab3), = mesh_error(eng, p.x)
    eng.close()
    for rel, ab in ((rel2, ab2), (rel3, ab3)):
        np.testing.assert_array_equal(rel1, rel)
        np.testing.assert_array_equal(ab1, ab)


@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_non_finite_node_poisons_its_section_only(built, value):
    """One interior node's angle set to NaN / +inf (cart-pole: sin and cos of it are NaN): the owning section's max_rel
    and the max_abs of every state the NaN reaches are NaN, as np.max gives in the restatement -- fmax would return 0
    or the largest finite entry, and ``not max > tol`` would read that as "tolerance met".  Every other section keeps
    the bits of the finite run."""
    from pycollo_amd.refinement import mesh_error
    p = mc.point("ragged_multitile")
    P = p.ora.P[0]
    k = int(np.flatnonzero(P.mesh.nodes >= 5)[7])             # a section with interior nodes
    node = int(P.mesh.bnd[k]) + 2
    x = p.x.copy()
    x[P.x_off + 1 * P.N + node] = value                       # state 1 (the pendulum's angle) at an interior node
    eng = _device_engine(p)
    (rel0, ab0), = mesh_error(eng, p.x)
    (rel, ab), = mesh_error(eng, x)
    eng.close()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        (ref_rel, ref_ab), = mc.table_form(p.ora, x, QuadratureTables("lobatto"))
    assert np.isnan(ref_rel[k]) and np.isnan(ref_ab[k, 1]) and np.sum(np.isnan(ref_rel)) == 1
    assert np.isnan(rel[k]), f"max_rel of the poisoned section is {rel[k]}"
    np.testing.assert_array_equal(np.isnan(ab), np.isnan(ref_ab))
    np.testing.assert_array_equal(np.isnan(rel), np.isnan(ref_rel))
    others = np.arange(P.mesh.K) != k
    np.testing.assert_array_equal(rel[others], rel0[others])
    np.testing.assert_array_equal(ab[others], ab0[others])
    fin = ~np.isnan(ref_ab[k])
    np.testing.assert_array_equal(ab[k][fin], ab0[k][fin])


@pytest.mark.parametrize("K", [5, 10])
def test_mesh_error_at_a_solved_point(built, K):
    """The only points that come from a solver: the iterate of the project's own interior-point solve on the
    brachistochrone meshes of ``test_refine_and_resolve_brachistochrone`` (K = 5 misses the tolerance, K = 10 meets
    it).  Kernel, float64 oracle and table form against the exact reference, bound <= 1e-3 of every estimate."""
    from pycollo_amd.iteration import MeshIteration
    from pycollo_amd.refinement import mesh_error
    it = MeshIteration(problems.brachistochrone(K=K, order=4))
    res = it.solve_with_ipm(tol=1e-10)
    assert res.success
    np.testing.assert_allclose(it.objective, 0.82434, rtol=1e-4)
    eng = it.engine
    ora = OracleNlp(problems.brachistochrone(K=K, order=4), golden_tables("lobatto"), V_ocp=eng.V_ocp, r_ocp=eng.r_ocp,
                    W_ocp=eng.W_ocp)
    x = np.array(it.x_tilde, float)
    ref = mesh_error_mp(ora, x)
    est, frac = ref[0]["max_rel"], mc.sharpness(ref)[0]
    print(f"solved K={K}: estimates {est.min():.1e}..{est.max():.1e}, bound / estimate up to {frac.max():.1e}")
    assert np.all(frac <= 1e-3)
    assert (np.max(est) > mc.TOL) == (K == 5)
    for what, got in (("float64 oracle", mc.oracle_maxima(ora, x)), ("table form", mc.table_form(ora, x, QuadratureTables("lobatto")))):
        r = mc.ratios(got, ref)
        print(f"solved K={K}: {what}: ratio to the bound {r}")
        assert max(r[0]) <= 1.0
    _assert_within_bound(mesh_error(eng, x), ref, f"solved K={K}")
    eng.close()


def test_refine_and_resolve_brachistochrone(built):
    """solve -> estimate -> refine -> carry the solution over: a coarse mesh (K = 5) converges to the known
    objective but misses the 1e-7 mesh tolerance, the rules ask for more nodes, the reference's default mesh
    (K = 10) meets the tolerance, and the carried-over solution is a far better starting point than the user
    guess.  (scipy's trust-constr stands in for IPOPT; it is only asked to solve meshes it is known to handle.)"""
    from pycollo_amd.iteration import MeshIteration
    from pycollo_amd.refinement import mesh_error, next_phase_mesh
    it5 = MeshIteration(problems.brachistochrone(K=5, order=4))
    res5 = it5.solve_with_scipy(maxiter=600)
    assert res5.constr_violation < 1e-8
    np.testing.assert_allclose(it5.objective, 0.82434, rtol=1e-4)     # tests/integration/test_brachistochrone.py:159-166
    (rel5, _), = mesh_error(it5.engine, it5.x_tilde)
    assert rel5.shape == (5,) and np.all(rel5 >= 0) and np.max(rel5) > 1e-7
    sizes, nodes, done = next_phase_mesh(it5.meshes[0].sizes, it5.meshes[0].n, rel5)
    assert not done and abs(sizes.sum() - 1) < 1e-12 and nodes.min() >= 4 and nodes.max() <= 10
    assert nodes.sum() > it5.meshes[0].n.sum()
    it10 = MeshIteration(problems.brachistochrone())
    it10.solve_with_scipy(maxiter=600)
    (rel10, _), = mesh_error(it10.engine, it10.x_tilde)
    assert np.max(rel10) < 1e-7 < np.max(rel5)
    assert next_phase_mesh(it10.meshes[0].sizes, it10.meshes[0].n, rel10)[2]
    np.testing.assert_allclose(it10.objective, 0.82434, rtol=1e-4)
    # carry the K = 5 solution to the refined mesh (iteration.py:528-583 -> 86-194)
    x = it5.V * it5.x_tilde + it5.r
    pl = it5.layout.phases[0]
    prev = ([it5.meshes[0].tau], [x[pl.x_off:pl.x_off + 3 * pl.N].reshape(3, -1)], [x[pl.x_off + 3 * pl.N:pl.q_off].reshape(1, -1)],
            [np.zeros(0)], [x[pl.t_off:pl.t_off + 1]], np.zeros(0))
    prob2 = problems.brachistochrone()
    prob2.phases[0].mesh.number_mesh_sections = len(nodes)
    prob2.phases[0].mesh.mesh_section_sizes = sizes
    prob2.phases[0].mesh.number_mesh_section_nodes = nodes
    warm = MeshIteration(prob2, prev=prev)
    cold = MeshIteration(prob2)
    viol_warm = np.max(np.abs(warm.engine.evaluate_c(warm.guess_x_tilde)))
    viol_cold = np.max(np.abs(cold.engine.evaluate_c(cold.guess_x_tilde)))
    assert viol_warm < 1e-2 * viol_cold
    assert abs(warm.engine.evaluate_J(warm.guess_x_tilde) - 0.82434) < 1e-4
