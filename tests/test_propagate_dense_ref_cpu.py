"""The restatement of the propagation with integrals and dense output (tests/propagate_dense_ref.py), checked on
the CPU before tests/test_gpu_propagate_dense.py holds the kernel to it.

* P is ``scipy.integrate.RK45.P`` to the last bit, and b_i(1) = b_i as an identity of fractions.
* On the smooth hypersensitive case of tests/test_propagate_ref_cpu.py the integrals converge at order 5 at least and
  the dense values at order 4 at least (lower limits only).  Measured, m = 2 -> 4 and 4 -> 8: integrals at the nodes 95
  and 53 (still above 2^5 at these widths: the integrand's error changes sign along the phase), dense states 40 and
  30, dense integrals 45 and 30: an interpolant of order 4 has a local error O(h^5) that is not carried along, so
  beside the steps' own O(h^5) a halving gains nearly 2^5.
* Without ``integral_atol`` the states and the step counts are ``propagate_ref.propagate_f64``'s bit for bit.
* The float64 restatement stays inside the parity bound 1e-10 |ref| + 64 eps n M against the 60-digit one, entry by
  entry, on every case the GPU test uses: what entitles the kernel to that bound.  The largest ratio measured is 7.6e-4
  (cart_pole_ragged_K23; the other cases stay below 7e-5).
* The C++ plan's ``q_order`` / ``node_q0`` equal the NumPy restatement, and that restatement equals the definition
  applied query by query.
* Bad arguments raise.
"""
import numpy as np
import pytest

import propagate_dense_ref as pd
import propagate_ref as pr
from conftest import golden_tables
from oracle.ref_numpy import OracleNlp
from pycollo_amd import problems
from pycollo_amd.solution import check_integral_atol, dense_query_tau
from test_propagate_dense_plan_sanitize import harness, run_plan_cases   # noqa: F401  (the fixture)

RESTARTS = ("nodes", "sections", "phase")
# the cases of the GPU test: propagate_ref.CASES' small meshes, and a phase without integrals
DENSE_CASES = dict((k, pr.CASES[k]) for k in ("hypersensitive_K5_n4", "hypersensitive_radau_K7_n5", "cart_pole_ragged_K23",
                                              "two_phase_transfer_K6", "hypersensitive_no_control"))
DENSE_CASES["sliding_mass_n4"] = lambda: problems.sliding_mass(order=4)


def _method(prob):
    return getattr(prob, "quadrature_method", None) or "lobatto"


_data = {}


def phase_data(name):
    """[DenseData per phase] of a case at the smooth point, from the oracle alone"""
    if name not in _data:
        prob = DENSE_CASES[name]()
        ora = OracleNlp(prob, golden_tables(_method(prob)))
        x = pr.smooth_x_oracle(ora)
        _data[name] = [pd.DenseData.from_oracle(ora, ip, x, _method(prob)) for ip in range(len(ora.P))]
    return _data[name]


def test_P_equals_scipy_rk45():
    from scipy.integrate._ivp.rk import RK45
    assert pd.P.shape == np.asarray(RK45.P).shape == (7, 4)
    assert pd.P.tobytes() == np.asarray(RK45.P, dtype=np.float64).tobytes()
    assert pd.P_ROWS == [0, 2, 3, 4, 5, 6]


def test_b_of_one_is_b():
    for i, row in enumerate(pd.P_FR):
        assert sum(row) == (pr._B[i] if i < 6 else 0), i
    assert sum(sum(row) for row in pd.P_FR) == 1


def _smooth_hypersensitive():
    """the case of test_propagate_ref_cpu.py's order check: hypersensitive (K = 10, order 4), final time 10, y = 1 + 0.2 tau
    at the nodes and the cubic control 0.5 + 0.3 tau - 0.2 tau^2 + 0.1 tau^3"""
    prob = pr._final_time(problems.hypersensitive(K=10, order=4), 10.0)
    ora = OracleNlp(prob, golden_tables("lobatto"))
    P = ora.P[0]
    tau, V, r = P.mesh.tau, ora.V_ocp, ora.r_ocp
    x = np.zeros(ora.num_x)
    x[P.x_off:P.x_off + P.N] = ((1.0 + 0.2 * tau) - r[P.ox]) / V[P.ox]
    x[P.x_off + P.N:P.x_off + 2 * P.N] = ((0.5 + 0.3 * tau - 0.2 * tau**2 + 0.1 * tau**3) - r[P.ox + 1]) / V[P.ox + 1]
    return pd.DenseData.from_oracle(ora, 0, x, "lobatto")


def test_integrals_converge_at_order_5_and_dense_values_at_order_4():
    d = _smooth_hypersensitive()
    seg = pr.segments("phase", d.s, d.N)
    rng = np.random.default_rng(1)
    tq = np.concatenate([d.tau[j] + rng.uniform(0.1, 0.9, 2) * (d.tau[j + 1] - d.tau[j]) for j in range(d.N - 1)])
    run = {m: pd.propagate_dense_f64(d, seg, tq, substeps=m) for m in (2, 4, 8, 64)}
    err_I = {m: np.max(np.abs(run[m]["q_arrive"] - run[64]["q_arrive"])) for m in (2, 4, 8)}                 # over the nodes
    err_y = {m: np.max(np.abs(run[m]["y_dense"] - run[64]["y_dense"])) for m in (2, 4, 8)}
    err_q = {m: np.max(np.abs(run[m]["q_dense"] - run[64]["q_dense"])) for m in (2, 4, 8)}
    for a, b in ((2, 4), (4, 8)):
        rI, ry, rq = err_I[a] / err_I[b], err_y[a] / err_y[b], err_q[a] / err_q[b]
        print(f"m = {a} -> {b}: integral at the nodes {err_I[a]:.3e} -> {err_I[b]:.3e}, ratio {rI:.2f}; dense y {err_y[a]:.3e} -> "
              f"{err_y[b]:.3e}, ratio {ry:.2f}; dense integral {err_q[a]:.3e} -> {err_q[b]:.3e}, ratio {rq:.2f}")
        assert rI >= 24.0                          # (2^5 less a quarter, the margin of test_propagate_ref_cpu.py's order check)
        assert ry >= 12.0 and rq >= 12.0           # (2^4 less a quarter)


@pytest.mark.parametrize("name", ["hypersensitive_K5_n4", "two_phase_transfer_K6", "sliding_mass_n4"])
def test_without_integral_atol_the_steps_are_propagate_f64s(name):
    for d in phase_data(name):
        V = np.maximum(np.max(np.abs(d.node_y), axis=1), 1.0)
        tq = pd.sample_queries(d)
        for restart in RESTARTS:
            seg = pr.segments(restart, d.s, d.N)
            for kw in (dict(substeps=1), dict(substeps=3), dict(rtol=1e-6, atol=1e-6 * V), dict(rtol=1e-10, atol=1e-10 * V)):
                y, acc, rej, st = pr.propagate_f64(d, seg, **kw)
                for q in ((), tq):
                    got = pd.propagate_dense_f64(d, seg, q, **kw)
                    assert got["y_arrive"].tobytes() == y.tobytes()
                    for a, b in ((got["accepted"], acc), (got["rejected"], rej), (got["status"], st)):
                        np.testing.assert_array_equal(a, b)


def _ratio(got, ref):
    val, n, M = ref
    b = pd.parity_bound(val, n, M)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(np.abs(got - val) == 0.0, 0.0, np.abs(got - val) / b)
    return float(np.max(r)) if r.size else 0.0


@pytest.mark.parametrize("name", list(DENSE_CASES))
def test_float64_restatement_within_the_parity_bound(name):
    """the condition DESIGN 8g sets for holding the kernel to 1e-10 |ref| + 64 eps n M; no entry is left out"""
    worst = 0.0
    for ip, d in enumerate(phase_data(name)):
        ref = pd.DenseFixedReference(d)
        tq = pd.sample_queries(d)
        for m in (1, 3):
            for restart in RESTARTS:
                seg = pr.segments(restart, d.s, d.N)
                want = ref.run(seg, m, tq)
                got = pd.propagate_dense_f64(d, seg, tq, substeps=m)
                for key in ("y_arrive", "q_arrive", "y_dense", "q_dense"):
                    assert np.all(np.isfinite(want[key][0])) and np.all(np.isfinite(want[key][2])) and np.all(np.isfinite(got[key]))
                    ratio = _ratio(got[key], want[key])
                    worst = max(worst, ratio)
                    print(f"{name} phase {ip} m = {m} {restart} {key}: largest |f64 - ref| / bound = {ratio:.3e}")
                    assert ratio <= 1.0
    print(f"{name}: largest ratio {worst:.3e}")


def test_nodes_are_answered_with_the_arrivals():
    d = phase_data("hypersensitive_K5_n4")[0]
    for restart in RESTARTS:
        seg = pr.segments(restart, d.s, d.N)
        for kw in (dict(substeps=2), dict(rtol=1e-8, atol=np.array([1e-8]))):
            got = pd.propagate_dense_f64(d, seg, d.tau, **kw)
            assert got["y_dense"].tobytes() == got["y_arrive"].tobytes()
            assert got["q_dense"].tobytes() == got["q_arrive"].tobytes()
            assert np.all(got["q_arrive"][:, 0] == 0.0)


def test_query_plan_restatement_and_the_cpp_plan(harness, tmp_path):   # noqa: F811
    rng = np.random.default_rng(4)
    n_k = np.array([4, 3, 6, 2, 5])
    sec_s = np.concatenate(([0], np.cumsum(n_k - 1)))
    N = int(sec_s[-1]) + 1
    tau = np.sort(np.concatenate(([-1.0, 1.0], rng.uniform(-1, 1, N - 2))))
    inner = rng.uniform(-1, 1, 40)
    lists = [np.zeros(0), tau.copy(), tau[::-1].copy(), np.concatenate([inner, inner[:5], tau[[3, 3, 0, N - 1]]]), inner[:1]]
    cases = [dict(n_k=n_k, tau=tau, seg=np.array([0, N - 1]), tq=tq, NQ=1, iatol=None) for tq in lists]
    got = run_plan_cases(harness, cases, tmp_path)
    for tq, g in zip(lists, got):
        order, q0 = pd.query_plan(tau, tq)
        np.testing.assert_array_equal(g[0], order)
        np.testing.assert_array_equal(g[1], q0)
        # the definition, query by query: slot 0 = tau_0, slot j = (tau_{j-1}, tau_j]; equal queries in the caller's order
        slot = [0 if t == tau[0] else next(j for j in range(1, N) if tau[j - 1] < t <= tau[j]) for t in tq]
        want = sorted(range(len(tq)), key=lambda i: (tq[i], i))
        np.testing.assert_array_equal(order, want)
        np.testing.assert_array_equal(np.diff(q0), np.bincount(slot, minlength=N) if len(tq) else np.zeros(N))


def test_bad_arguments_raise():
    tau = np.linspace(-1, 1, 7)
    for bad in ([np.nan], [0.0, np.inf], [np.nextafter(1.0, 2.0)], [-1.5]):
        with pytest.raises(ValueError):
            pd.query_plan(tau, bad)
        with pytest.raises(ValueError):
            dense_query_tau(None, np.array(bad), 0.0, 2.0)
    for bad_t in ([np.nan], [-0.1], [2.1]):
        with pytest.raises(ValueError):
            dense_query_tau(np.array(bad_t), None, 0.0, 2.0)
    with pytest.raises(ValueError):
        dense_query_tau(np.array([0.5]), np.array([0.0]), 0.0, 2.0)             # both
    with pytest.raises(ValueError):
        dense_query_tau(np.zeros((2, 2)), None, 0.0, 2.0)
    assert dense_query_tau(None, None, 0.0, 2.0).shape == (0,)
    # a time within a few ulp of the phase's end is the end
    np.testing.assert_array_equal(dense_query_tau(np.array([0.0, 2.0, np.nextafter(2.0, 3.0), 1.0]), None, 0.0, 2.0), [-1.0, 1.0, 1.0, 0.0])
    for bad in (0.0, -1e-9, np.nan, np.inf, [1e-9, 0.0], [1e-9, 1e-9, 1e-9]):
        with pytest.raises(ValueError):
            check_integral_atol(bad, 2)
    assert check_integral_atol(None, 2) is None
    np.testing.assert_array_equal(check_integral_atol(1e-9, 2), [1e-9, 1e-9])
    assert check_integral_atol([], 0).shape == (0,)


# ---- end to end ------------------------------------------------------------------------------------------------------
# hypersensitive (K = 10, order 4; the brachistochrone carries no integral), NLP tolerance 1e-10, propagated at rtol 1e-10
# (DESIGN 8g): |integral_defect| of the open-loop pass and of the restart at every node, and the largest |y_dense - y(t)|
# over 33 points per section of the open-loop pass.  Ten sections of order 4 over 10 000 time units resolve neither
# boundary layer: the figures say how far the transcription's integral (633.95) and curve are from the dynamics.
CPU_INTEGRAL_DEFECT_PHASE = 618.86
CPU_INTEGRAL_DEFECT_NODES = 607.06
CPU_DENSE_GAP = 7.251


def test_end_to_end_figures_on_the_cpu():
    ora, x = pr.cpu_solve(problems.hypersensitive(K=10, order=4), golden_tables("lobatto"))
    d = pd.DenseData.from_oracle(ora, 0, x, "lobatto")
    phase, nodes, gap = pd.end_to_end_figures(d, "lobatto", ora.V_ocp[:d.n_y])
    print(f"hypersensitive on the CPU: objective {ora.J(x):.10f}; |integral_defect| (phase) {phase[0]:.5e}, (nodes) {nodes[0]:.5e}; "
          f"largest |y_dense - y(t)| {gap:.4e}")
    assert abs(phase[0] - CPU_INTEGRAL_DEFECT_PHASE) <= 0.02 * CPU_INTEGRAL_DEFECT_PHASE
    assert abs(nodes[0] - CPU_INTEGRAL_DEFECT_NODES) <= 0.02 * CPU_INTEGRAL_DEFECT_NODES
    assert abs(gap - CPU_DENSE_GAP) <= 0.02 * CPU_DENSE_GAP
    # the interpolant's restatement returns the NLP's node values up to the defects the solve left
    assert np.max(np.abs(pd.sample_y_f64(d, "lobatto", d.tau) - d.node_y)) <= 1e-9 * np.max(np.abs(d.node_y))


# ---- the adaptive mode's integral bound (what test 4 of the GPU file asks of the kernel) ---------------------------------
@pytest.mark.parametrize("name", ["hypersensitive_K5_n4", "hypersensitive_radau_K7_n5", "two_phase_transfer_K6"])
def test_adaptive_restatement_meets_the_integral_bound(name):
    """with integral_atol = rtol the float64 restatement's integrals are within a (integral_atol + rtol max|I|) of the
    60-digit fixed-mode truth at every combination (largest ratio 0.26), and its steps are no fewer than without"""
    from test_propagate_ref_cpu import TRUTH_M
    for ip, d in enumerate(phase_data(name)):
        ref = pd.DenseFixedReference(d)
        V = np.maximum(np.max(np.abs(d.node_y), axis=1), 1.0)
        for restart in RESTARTS:
            seg = pr.segments(restart, d.s, d.N)
            truth = ref.run(seg, TRUTH_M[name])["q_arrive"][0]
            for rtol in (1e-6, 1e-10):
                loose = pd.propagate_dense_f64(d, seg, rtol=rtol, atol=rtol * V)
                tight = pd.propagate_dense_f64(d, seg, rtol=rtol, atol=rtol * V, integral_atol=rtol)
                assert np.all(tight["status"] == -1)
                bound = pd.integral_adaptive_bound(seg, truth, tight["accepted"], rtol, rtol)
                ratio = float(np.max(np.abs(tight["q_arrive"] - truth)[:, 1:] / bound[:, 1:]))
                n0, n1 = (int(r["accepted"].sum() + r["rejected"].sum()) for r in (loose, tight))
                print(f"{name} phase {ip} {restart} rtol {rtol:g}: integral error / bound = {ratio:.3e}; steps {n0} -> {n1}")
                assert ratio <= 1.0 and n1 >= n0
