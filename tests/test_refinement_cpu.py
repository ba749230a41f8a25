"""Host side of row N2 (no GPU): the ph tables, the float64 restatements of the estimate against the exact reference at
every point the GPU tests use, the guards of ``mesh_error`` and the next-mesh rules."""
import os
import warnings

import numpy as np
import pytest

import mesh_error_cases as mc
from conftest import GOLDEN, golden_tables
from pycollo_amd.quadrature import QuadratureTables
from pycollo_amd.refinement import ph_tables

EPS = np.finfo(float).eps


def test_ph_tables_equal_the_reference_polynomial_fits():
    """B / E reproduce Legendre.fit(...).integ(k=y0) and Polynomial.fit(...) of solution_abc.py:70-100."""
    q = QuadratureTables("lobatto")
    for n in (3, 4, 6, 8):
        B, E, A = ph_tables(q, n)
        assert B.shape == E.shape == (n - 1, n) and A.shape == (n, n + 1)
        c = 0.5 * (q.points(n) + 1)
        cp = 0.5 * (q.points(n + 1)[1:-1] + 1)
        rng = np.random.default_rng(n)
        f, u = rng.normal(size=n), rng.normal(size=n)
        yref = np.polynomial.Legendre.fit(c, f, deg=n - 1, window=[0, 1]).integ(k=0.3)(cp)
        uref = np.polynomial.Polynomial.fit(c, u, deg=n - 1, window=[0, 1])(cp)
        np.testing.assert_allclose(0.3 + B @ f, yref, atol=1e-11)
        np.testing.assert_allclose(E @ u, uref, atol=1e-10)
        np.testing.assert_allclose(E.sum(axis=1), 1.0, atol=1e-12)       # partition of unity
        np.testing.assert_allclose(B.sum(axis=1), cp, atol=1e-12)        # integral of 1 up to c


def test_next_mesh_rules():
    from pycollo_amd.refinement import next_phase_mesh
    sizes, nodes, done = next_phase_mesh(np.full(4, 0.25), np.full(4, 4), [1e-9, 1e-8, 1e-10, 5e-8])
    assert done and np.array_equal(nodes, [4, 4, 4, 4])
    sizes, nodes, done = next_phase_mesh(np.full(4, 0.25), np.full(4, 4), [1e-9, 1e-5, 1e-3, 1e-1])
    assert not done
    assert np.array_equal(nodes, [4, 8, 4, 4, 4, 4, 4, 4, 4])          # +4 nodes; 11 -> 3 sections; 14 -> 4 sections
    np.testing.assert_allclose(sizes, [0.25, 0.25] + [0.25 / 3] * 3 + [0.0625] * 4)


def test_merge_runs_of_over_resolved_sections():
    """mesh_refinement.py:339-347,354-372: MERGE_TOLERANCE_FACTOR = 0 zeroes the threshold, it does not disable the
    branch -- sections whose predicted order P + n is negative are merged (:252-285).  Expected values worked from the
    reference's formulas by hand:
    n = 4, tol = 1e-7, e = 1e-13: P = ceil(log(1e-6) / log 4) = -9 -> -9 + ceil(log 10) = -6, predicted -2 < 0;
    merge ratio 4 / (4 + 6) = 0.4 per section, two neighbours -> ceil(0.8) = 1 section of their joint width."""
    from pycollo_amd.refinement import next_phase_mesh
    sizes, nodes, done = next_phase_mesh(np.full(4, 0.25), np.full(4, 4), [1e-5, 1e-13, 1e-13, 1e-6])
    assert not done
    assert np.array_equal(nodes, [8, 4, 6])                     # +4 nodes | merged pair at n_min | +2 nodes
    np.testing.assert_allclose(sizes, [0.25, 0.5, 0.25])
    # a run that needs two sections (order 6, uneven widths and errors): P = [-7, -8, -7], ratios 6/11, 6/12, 6/11
    # -> ceil(1.59) = 2; knots at [1/6, 1/2, 1] carry the densities [0.16176471, 0.51470588, 1], the new knots are the
    # density function evaluated at [0.5, 1] -> widths 0.6 * [0.51470588, 0.48529412]; then +3 nodes; then a section
    # predicted at 4 + 9 = 13 >= 10 nodes, cut into ceil(13 / 4) = 4
    sizes, nodes, done = next_phase_mesh([0.1, 0.2, 0.3, 0.25, 0.15], [6, 6, 6, 6, 4],
                                         [9.2e-16, 1.5e-16, 9.2e-16, 50e-7, 1e-2])
    assert np.array_equal(nodes, [4, 4, 9, 4, 4, 4, 4])
    np.testing.assert_allclose(sizes, [0.6 * 0.5147058823529411, 0.6 * 0.4852941176470589, 0.25] + [0.0375] * 4, rtol=1e-12)
    # a merge run at the end of the mesh and one at the start
    sizes, nodes, _ = next_phase_mesh(np.full(4, 0.25), np.full(4, 4), [1e-13, 1e-13, 1e-5, 1e-13])
    assert np.array_equal(nodes, [4, 8, 4])
    np.testing.assert_allclose(sizes, [0.5, 0.25, 0.25])


@pytest.mark.parametrize("n", range(2, 20))
def test_ph_tables_against_exact_lagrange_tables(n):
    """B, E of every order the kernel accepts, entry by entry against the Lagrange basis of the golden points
    integrated / evaluated with 70 digits, and A against the golden A(n + 1).  An entry is a sum of n <= 19 products on
    a Legendre Vandermonde matrix of condition O(n), so it is held to 32 eps of its row's sum of magnitudes (measured
    worst: 5.3 eps for B at n = 18, 7.4 eps for E at n = 18; at most 2.1 eps up to n = 11)."""
    from oracle.ref_refine import lagrange_tables_mp
    g = golden_tables("lobatto")
    B, E, A = ph_tables(QuadratureTables("lobatto"), n)
    Bx, Ex = (np.array([[float(v) for v in row] for row in T]).reshape(n - 1, n)
              for T in lagrange_tables_mp(g.points(n), g.points(n + 1)[1:-1]))
    assert B.shape == E.shape == (n - 1, n) and A.shape == (n, n + 1)
    for got, ref, what in ((B, Bx, "B"), (E, Ex, "E")):
        worst = np.max(np.abs(got - ref) / np.abs(ref).sum(axis=1)[:, None]) / EPS
        print(f"order {n}: {what} differs from the exact table by {worst:.2f} eps of the row sum")
        assert worst <= 32.0
    np.testing.assert_allclose(A, g.A(n + 1), rtol=0, atol=4 * EPS * np.max(np.abs(g.A(n + 1))))


def _check_restatements(ora, x, ref, label):
    oracle, table = mc.oracle_maxima(ora, x), mc.table_form(ora, x, QuadratureTables("lobatto"))
    for what, got in (("float64 oracle", oracle), ("table form", table)):
        r = mc.ratios(got, ref)
        print(f"{label}: {what}: max_rel / max_abs ratio to the bound per phase {[(float(f'{a:.3g}'), float(f'{b:.3g}')) for a, b in r]}")
        assert max(max(pair) for pair in r) <= 1.0, f"{what} misses the tolerance the kernel is held to"


@pytest.mark.parametrize("name", list(mc.CASES))
def test_float64_restatements_meet_the_gpu_tolerance(name):
    """(Cost: most cases take a second or less.  Three take longer, for what is built once per process and shared with
    every other test of the model: Delta III about 25 s, of which 20 s are the oracle's symbolic derivatives of its
    model; the ragged cart-pole case about 18 s -- its oracle, 780 integration legs and the 40-digit reference; the
    double pendulum about 7 s, its oracle.  tests/test_gpu_refinement.py pays the same once in its own process.)

    oracle.ref_refine.mesh_error and a NumPy restatement of the kernel's table form, each on its own, against
    mesh_error_mp at the trajectory points of tests/test_gpu_refinement.py, within the bound the kernel is held to
    (mc.ULPS = 32 leaves the worse of the two a factor 4.04: the oracle at the no-control point is at 0.2475 of the
    bound, the table form nowhere above 0.035): the tolerance of the GPU tests is achievable in fp64.  The
    sharpness of the bound (<= 1e-3 of every section's estimate, from the reference alone) and the regime of the case
    (estimates on both sides of 1e-7) are asserted here as they are on the GPU."""
    p = mc.point(name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        _check_restatements(p.ora, p.x, p.ref, name)
    mc.assert_regime(name, p.ref)


@pytest.mark.parametrize("i", range(len(mc.CUBIC_CASES)))
def test_float64_restatements_at_the_cubic_points(i):
    ora, x, ref = mc.cubic(i)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        _check_restatements(ora, x, ref, mc.CUBIC_CASES[i][0])


def test_ragged_case_fills_and_closes_tiles_as_intended():
    """The ragged multi-tile case by the host code's greedy rule (section k takes n_k + 1 of 256 lanes): about four
    tiles, the first filled to exactly 256 lanes, the second closed with >= 5 lanes free because the next section has
    order 10 (11 lanes); and every call of every case stays under 64 KiB of LDS except Delta III's (7 states)."""
    nodes = mc.point("ragged_multitile").ora.P[0].mesh.nodes
    used, first = mc.tile_lanes(nodes)
    assert len(nodes) == 120 and nodes.min() == 2 and nodes.max() == 10 and len(used) == 4
    assert used[0] == 256
    assert 5 <= 256 - used[1] < 11 and nodes[first[2]] == 10
    for name in mc.CASES:
        for P in mc.point(name).ora.P:
            assert name == "delta_iii" or mc.lds_bytes(P.mesh.nodes, P.n_y, P.n_u) < 64 * 1024


def test_mesh_error_guards_radau_and_order_20():
    """Radau tables: NotImplementedError that names the method (only the Lobatto branch of solution_abc.py:70-107 is
    restated; with Radau points the last "point" is a placeholder).  A section of order 20 needs the quadrature rule of
    order 21, which nobody has: a ValueError from Python that says so, before any table is built; 19 works."""
    from types import SimpleNamespace
    from pycollo_amd.refinement import mesh_error
    with pytest.raises(NotImplementedError, match="radau"):
        ph_tables(QuadratureTables("radau"), 4)
    calls = []
    fake = lambda orders, method="lobatto": SimpleNamespace(
        quad=QuadratureTables(method), meshes=[SimpleNamespace(n=np.asarray(orders))],
        mesh_error=lambda ip, x, od, B, E, A: calls.append((od, B.size, E.size, A.size)) or "ran")
    with pytest.raises(NotImplementedError, match="radau"):
        mesh_error(fake([4, 4], "radau"), np.zeros(3))
    for bad in (20, 1):
        with pytest.raises(ValueError, match=rf"order {bad}, outside \[2, 19\]"):
            mesh_error(fake([4, bad, 5]), np.zeros(3))
        with pytest.raises(ValueError, match="outside"):
            ph_tables(QuadratureTables("lobatto"), bad)
    assert not calls
    assert mesh_error(fake([19, 2, 19]), np.zeros(3)) == ["ran"]
    assert calls == [([2, 19], 2 + 18 * 19, 2 + 18 * 19, 6 + 19 * 20)]


def test_next_mesh_refuses_a_non_finite_error():
    """A NaN estimate (f not finite somewhere) compares false with the tolerance: ``not max > tol`` read it as
    "tolerance met".  It is an error instead, wherever the NaN sits and whatever the other sections say."""
    from pycollo_amd.refinement import next_phase_mesh
    sizes, nodes = np.full(4, 0.25), np.full(4, 4)
    for err in ([np.nan, 1e-9, 1e-9, 1e-9], [1e-9, 1e-9, 1e-9, np.nan], [1e-3, np.nan, 1e-9, 1e-9], [np.nan] * 4,
                [1e-9, np.inf, 1e-9, 1e-9]):
        with pytest.raises(ValueError, match="not finite"):
            next_phase_mesh(sizes, nodes, err)
    assert next_phase_mesh(sizes, nodes, [1e-9] * 4)[2]


def test_next_mesh_equals_the_reference_function_on_recorded_cases():
    """300 seeded inputs of the reference's own ``next_iteration_phase_mesh`` (tests/golden/make_golden.py runs it on
    stand-in objects and records what it hands to PhaseMesh): K in 1..30, orders within (4, 10) and (2, 20), tolerances
    1e-7 and 1e-5, errors log-uniform in 1e-17..1, and forced structure -- merge runs at the start, in the middle, at
    the end, a run that needs >= 3 merged sections, an error equal to the tolerance, an error of 0, all below.  Node
    counts equal as integers, sizes (normalised as PhaseMesh normalises them) to 1e-14 relative."""
    from pycollo_amd.refinement import next_phase_mesh
    z = np.load(os.path.join(GOLDEN, "next_mesh_cases.npz"))
    status = z["status"]
    assert len(status) == 300 and set(z["tags"]) >= {"random", "run_start", "run_middle", "run_end", "run_long",
                                                      "equal_tol", "zero", "all_below", "zero_only", "equal_tol_only"}
    seen_long_merge = False
    for i, st in enumerate(status):
        a, b = z["in_off"][i:i + 2]
        oa, ob = z["out_off"][i:i + 2]
        tol, n_min, n_max = z["in_par"][i]
        args = (z["in_h"][a:b], z["in_nodes"][a:b], z["in_err"][a:b])
        kw = dict(mesh_tol=tol, n_min=int(n_min), n_max=int(n_max))
        label = f"case {i} ({z['tags'][i]})"
        if st >= 2:     # the reference itself raised or produced non-finite sizes: no mesh may come back silently
            with pytest.raises((ValueError, FloatingPointError, ZeroDivisionError)):
                next_phase_mesh(*args, **kw)
            continue
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            sizes, nodes, done = next_phase_mesh(*args, **kw)
        if st == 1:     # the reference kept the mesh
            assert done and np.array_equal(nodes, args[1]), label
            np.testing.assert_allclose(sizes, args[0] / args[0].sum(), rtol=1e-15, err_msg=label)
            continue
        ref_sizes, ref_nodes = z["out_sizes"][oa:ob], z["out_nodes"][oa:ob]
        assert not done, label
        assert nodes.dtype.kind == "i" and np.array_equal(nodes, ref_nodes), label
        np.testing.assert_allclose(sizes, ref_sizes / ref_sizes.sum(), rtol=1e-14, atol=0, err_msg=label)
        if z["tags"][i] == "run_long":
            seen_long_merge = seen_long_merge or np.any(np.convolve(ref_nodes == int(n_min), np.ones(3), "valid") == 3)
    assert seen_long_merge and np.sum(status == 1) >= 10 and np.sum(status == 0) >= 250


def test_solve_ocp_stops_on_a_non_finite_estimate(monkeypatch):
    """A NaN estimate in ANY phase ends the mesh loop with ``mesh_tolerance_met = False`` and a warning, and no next
    mesh is asked for (the NLP solve and the estimate are stand-ins; the loop is solve_ocp's own)."""
    from types import SimpleNamespace
    import pycollo_amd.solve as solve
    made = []

    class FakeIteration:
        def __init__(self, prob, **kw):
            made.append(self)
            self.engine, self.x_tilde, self.objective, self.scaling_record = None, np.zeros(3), 1.25, None
            self.meshes = [SimpleNamespace(K=4, sizes=np.full(4, 0.25), n=np.full(4, 4))] * 2
            self.layout = SimpleNamespace(phases=[SimpleNamespace(N=13)] * 2)

        def solve_with_ipm(self, **kw):
            return SimpleNamespace(status="solved", success=True, iterations=7, seconds=0.0, evaluations={}, inf_pr=0.0, inf_du=0.0)

    monkeypatch.setattr(solve, "MeshIteration", FakeIteration)
    monkeypatch.setattr(solve, "mesh_error", lambda eng, x: [(np.array([1e-9, np.nan, 1e-9, 1e-9]), None),
                                                             (np.full(4, 1e-9), None)])
    monkeypatch.setattr(solve, "next_phase_mesh", lambda *a, **k: pytest.fail("a next mesh was asked for"))
    with pytest.warns(RuntimeWarning, match="not finite"):
        res = solve.solve_ocp(SimpleNamespace(phases=[]), max_mesh_iterations=3)
    assert res.mesh_tolerance_met is False and res.mesh_iterations == 1 and len(made) == 1
    assert np.isnan(res.iterations[0]["max_rel_err"])
