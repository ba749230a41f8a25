"""The tests' own restatement of the forward propagation (tests/propagate_ref.py), checked on the CPU, so that
tests/test_gpu_propagate.py compares the kernel against something itself checked; and the host-side argument handling
of ``Solution.propagate`` (pycollo_amd/solution.py), which needs no device.

* the tableau equals scipy's ``RK45`` to the last bit;
* the fixed mode converges at order 5;
* one fixed step is exact on the sliding mass (a quintic);
* the float64 restatement stays within the parity bound of the 60-digit one on every case of the GPU tests -- the
  condition for using that bound on the kernel;
* the adaptive restatement against the textbook bound a (atol + rtol max|y|) exp(L T), and the truth it is measured
  against (the combinations that do not meet it are listed in ``ADAPTIVE_DROPPED`` and are not asked of the kernel);
* the premises of the cap test;
* the end-to-end figures quoted in DESIGN 8e.
"""
import numpy as np
import pytest

import propagate_ref as pr
from conftest import golden_tables
from oracle.ref_numpy import OracleNlp
from pycollo_amd import problems
from pycollo_amd.solution import check_propagate_tolerances, propagation_segments

RESTARTS = ("nodes", "sections", "phase", "irregular")


def _method(prob):
    return getattr(prob, "quadrature_method", None) or "lobatto"


_data = {}


def phase_data(name):
    """[PhaseData per phase] of a case at the smooth point, from the oracle alone"""
    if name not in _data:
        prob = pr.CASES[name]()
        ora = OracleNlp(prob, golden_tables(_method(prob)))
        x = pr.smooth_x_oracle(ora)
        _data[name] = [pr.PhaseData.from_oracle(ora, ip, x, _method(prob)) for ip in range(len(ora.P))], ora
    return _data[name]


def test_tableau_equals_scipy_rk45():
    from scipy.integrate._ivp.rk import RK45
    for mine, theirs in ((pr.A, RK45.A), (pr.B, RK45.B), (pr.C, RK45.C), (pr.E, RK45.E)):
        assert mine.shape == np.asarray(theirs).shape
        assert mine.tobytes() == np.asarray(theirs, dtype=np.float64).tobytes()
    assert pr.ROWS[6] == list(pr.B) and pr.CS == list(pr.C) + [1.0]


def _smooth_hypersensitive():
    """hypersensitive (K = 10, order 4), final time 10, y(0) = 1 and the cubic control 0.5 + 0.3 tau - 0.2 tau^2 + 0.1 tau^3"""
    prob = pr._final_time(problems.hypersensitive(K=10, order=4), 10.0)
    ora = OracleNlp(prob, golden_tables("lobatto"))
    P = ora.P[0]
    tau, V, r = P.mesh.tau, ora.V_ocp, ora.r_ocp
    x = np.zeros(ora.num_x)
    x[P.x_off:P.x_off + P.N] = ((1.0 + 0.2 * tau) - r[P.ox]) / V[P.ox]
    x[P.x_off + P.N:P.x_off + 2 * P.N] = ((0.5 + 0.3 * tau - 0.2 * tau**2 + 0.1 * tau**3) - r[P.ox + 1]) / V[P.ox + 1]
    return pr.PhaseData.from_oracle(ora, 0, x, "lobatto")


def test_fixed_mode_converges_at_order_5():
    d = _smooth_hypersensitive()
    ref = pr.FixedReference(d)
    end = {m: ref._extend(0, m, d.N - 1)["y"][-1][0] for m in (2, 4, 8, 64)}      # y(tF) of one pass over the phase
    err = {m: abs(end[m] - end[64]) for m in (2, 4, 8)}
    for a, b in ((2, 4), (4, 8)):
        ratio = float(err[a] / err[b])
        print(f"m = {a} -> {b}: error {float(err[a]):.3e} -> {float(err[b]):.3e}, ratio {ratio:.2f}")
        assert 24.0 <= ratio <= 40.0


def _sliding_mass_data():
    prob = problems.sliding_mass(order=4)
    ora = OracleNlp(prob, golden_tables("lobatto"))
    x = pr.smooth_x_oracle(ora)
    return [pr.PhaseData.from_oracle(ora, ip, x, "lobatto") for ip in range(len(ora.P))]


def test_one_fixed_step_is_exact_on_the_sliding_mass():
    for d in _sliding_mass_data():
        seg = pr.segments("sections", d.s, d.N)
        exact = pr.sliding_mass_exact(d)
        y, steps, M = pr.FixedReference(d).arrivals(seg, 1)
        bound = pr.parity_bound(exact, steps, M)
        assert np.all(np.abs(y - exact)[:, 1:] <= bound[:, 1:])                 # the 60-digit restatement (exact up to its rounding to double)
        g = pr.propagate_f64(d, seg, substeps=1)[0]
        assert np.all(np.abs(g - exact)[:, 1:] <= bound[:, 1:])                 # the float64 one
        assert np.max(np.abs(exact - d.node_y)) > 1e-3                          # (the point is no solution: the arrivals differ from the nodes)


@pytest.mark.parametrize("name", list(pr.CASES))
def test_float64_restatement_within_the_parity_bound(name):
    """the condition DESIGN 8e sets for holding the kernel to 1e-10 |ref| + 64 eps n M"""
    for ip, d in enumerate(phase_data(name)[0]):
        ref = pr.FixedReference(d)
        for m in (1, 3):
            for restart in RESTARTS:
                seg = pr.segments(restart, d.s, d.N)
                y, steps, M = ref.arrivals(seg, m)
                assert np.all(np.isfinite(y)) and np.all(np.isfinite(M))
                g, acc, rej, st = pr.propagate_f64(d, seg, substeps=m)
                ratio = np.max(np.abs(g - y)[:, 1:] / pr.parity_bound(y, steps, M)[:, 1:])
                print(f"{name} phase {ip} m = {m} {restart}: largest |f64 - ref| / bound = {ratio:.3e}")
                assert ratio <= 1.0
                assert np.all(st == -1) and np.all(acc[1:] == m) and np.all(rej == 0)


def test_final_time_10_overflows_the_fixed_mode():
    """why the hypersensitive cases last 0.02 time units (propagate_ref.CASES): at the smooth point |y| reaches 15,
    and one step over a node interval of the final-time-10 mesh leaves the stability region"""
    prob = pr._final_time(problems.hypersensitive(K=5, order=4), 10.0)
    ora = OracleNlp(prob, golden_tables("lobatto"))
    d = pr.PhaseData.from_oracle(ora, 0, pr.smooth_x_oracle(ora), "lobatto")
    with np.errstate(all="ignore"):
        y = pr.propagate_f64(d, pr.segments("phase", d.s, d.N), substeps=1)[0]
    assert not np.all(np.isfinite(y))


# ---- adaptive ----------------------------------------------------------------------------------------------------
ADAPTIVE_CASES = ("hypersensitive_K5_n4", "hypersensitive_radau_K7_n5", "two_phase_transfer_K6")
ADAPTIVE_RESTARTS = ("nodes", "sections", "phase")
# substeps of the 60-digit truth: doubling them moves no arrival by 1e-14 of the state's largest magnitude
TRUTH_M = {"hypersensitive_K5_n4": 64, "hypersensitive_radau_K7_n5": 64, "two_phase_transfer_K6": 32}
# (case, restart, rtol) at which the float64 restatement itself misses a (atol + rtol max|y|) exp(L T): one step over a
# whole node interval with h |df/dy| ~ 2 is accepted by the embedded estimate with a true error of three tolerances.
# Not asked of the kernel.
ADAPTIVE_DROPPED = {("hypersensitive_K5_n4", "nodes", 1e-6), ("hypersensitive_K5_n4", "sections", 1e-6),
                    ("hypersensitive_radau_K7_n5", "nodes", 1e-6)}


def adaptive_truth(d, ref, seg, m):
    return ref.arrivals(seg, m)[0]


@pytest.mark.parametrize("name", ADAPTIVE_CASES)
def test_adaptive_restatement_meets_the_textbook_bound(name):
    data, ora = phase_data(name)
    for ip, d in enumerate(data):
        V = ora.V_ocp[ora.P[ip].ox:ora.P[ip].ox + d.n_y]
        ref = pr.FixedReference(d)
        for restart in ADAPTIVE_RESTARTS:
            seg = pr.segments(restart, d.s, d.N)
            truth = adaptive_truth(d, ref, seg, TRUTH_M[name])
            twice = adaptive_truth(d, ref, seg, 2 * TRUTH_M[name])
            scale = np.max(np.abs(truth), axis=1, keepdims=True)
            assert np.max(np.abs(twice - truth) / scale) <= 1e-14
            L = pr.lipschitz(d, truth)
            if name.startswith("hypersensitive"):
                assert L == 0.0                                  # df/dy = -3 y^2
            for rtol in (1e-6, 1e-10):
                atol = rtol * V
                y, acc, rej, st = pr.propagate_f64(d, seg, rtol=rtol, atol=atol)
                assert np.all(st == -1) and np.all(acc[1:] >= 1) and np.all(rej >= 0)
                ratio = np.max(np.abs(y - truth)[:, 1:] / pr.adaptive_bound(d, seg, truth, acc, atol, rtol, L)[:, 1:])
                print(f"{name} phase {ip} {restart} rtol {rtol:g}: L = {L:.3g}, largest error / bound = {ratio:.3e}")
                if (name, restart, rtol) in ADAPTIVE_DROPPED:
                    assert ratio > 1.0, "a dropped combination meets the bound: take it off ADAPTIVE_DROPPED"
                else:
                    assert ratio <= 1.0


# ---- the cap -------------------------------------------------------------------------------------------------------
def test_premises_of_the_cap_test():
    # final time 10 000, max_steps = 1: every segment fails at its first interval, at rtol 1e-13 and at any other
    prob = problems.hypersensitive(K=5, order=4)
    ora = OracleNlp(prob, golden_tables("lobatto"))
    d = pr.PhaseData.from_oracle(ora, 0, pr.smooth_x_oracle(ora), "lobatto")
    seg = pr.segments("sections", d.s, d.N)
    for rtol in (1e-13, 1e-6, 1.0, 1e6):
        with np.errstate(all="ignore"):
            y, acc, rej, st = pr.propagate_f64(d, seg, rtol=rtol, atol=rtol * ora.V_ocp[:1], max_steps=1)
        np.testing.assert_array_equal(st, seg[:-1])
        assert np.all(np.isnan(y[:, 1:]))
    # final time 0.02, rtol 1e-6, max_steps = 1: some first intervals pass in one step, some intervals do not
    d = phase_data("hypersensitive_K5_n4")[0][0]
    y, acc, rej, st = pr.propagate_f64(d, seg, rtol=1e-6, atol=1e-6 * ora.V_ocp[:1], max_steps=1)
    failed = st >= 0
    assert failed.any() and not failed.all()
    assert any(st[i] > seg[i] for i in np.nonzero(failed)[0]) or any(not f for f in failed)


# ---- the host-side argument handling of Solution.propagate ---------------------------------------------------------
def test_segment_lists_and_refusals_of_the_python_layer():
    s, N = np.array([0, 3, 6, 9, 12, 15]), 16
    for restart in ("nodes", "sections", "phase"):
        got = propagation_segments(restart, s, N)
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, pr.segments(restart, s, N))
    irregular = pr.segments("irregular", s, N)
    np.testing.assert_array_equal(propagation_segments(irregular, s, N), irregular)
    for bad in ([0, 4, 4, 15], [0, 5, 4, 15], [1, 4, 15], [0, 4, 14], [0, 4, 16], [0], [[0, 15]], [0.0, 15.0]):
        with pytest.raises(ValueError):
            propagation_segments(np.array(bad), s, N)
    with pytest.raises(ValueError):
        propagation_segments("mesh", s, N)
    ok = np.array([1e-9, 2e-9])
    check_propagate_tolerances(None, 1e-9, ok, 4096)
    check_propagate_tolerances(3, float("nan"), ok, 1)                 # fixed: rtol is not read
    check_propagate_tolerances(1 << 20, 1e-9, ok, 1 << 20)
    for args in ((-1, 1e-9, ok, 4096), (0, 1e-9, ok, 4096), (2.5, 1e-9, ok, 4096), ((1 << 20) + 1, 1e-9, ok, 4096),
                 (None, 0.0, ok, 4096), (None, -1e-9, ok, 4096), (None, float("nan"), ok, 4096), (None, float("inf"), ok, 4096),
                 (None, 1e-9, np.array([1e-9, 0.0]), 4096), (None, 1e-9, np.array([-1.0, 1e-9]), 4096),
                 (2, 1e-9, np.array([np.nan, 1e-9]), 4096), (None, 1e-9, np.array([np.inf, 1e-9]), 4096),
                 (None, 1e-9, ok, 0), (None, 1e-9, ok, (1 << 20) + 1), (None, 1e-9, ok, 2.5)):
        with pytest.raises(ValueError):
            check_propagate_tolerances(*args)


# ---- end to end ------------------------------------------------------------------------------------------------------
# the largest relative defect at tF of one pass over the phase, and the largest over the nodes restarted at every node:
# brachistochrone (K = 10, order 4), NLP tolerance 1e-10, propagation rtol 1e-10
CPU_TERMINAL_PHASE = 6.4e-12
CPU_MAX_NODES = 1.37e-8


def test_end_to_end_figures_on_the_cpu():
    ora, x = pr.cpu_solve(problems.brachistochrone(K=10, order=4), golden_tables("lobatto"))
    d = pr.PhaseData.from_oracle(ora, 0, x, "lobatto")
    V = ora.V_ocp[:d.n_y]
    fig = {}
    for restart in ("phase", "nodes"):
        y, acc, rej, st = pr.propagate_f64(d, pr.segments(restart, d.s, d.N), rtol=1e-10, atol=1e-10 * V)
        assert np.all(st == -1)
        fig[restart] = np.abs((y - d.node_y) / V[:, None])
    terminal, nodes = float(np.max(fig["phase"][:, -1])), float(np.max(fig["nodes"]))
    print(f"brachistochrone on the CPU: objective {ora.J(x):.10f}; relative defect at tF (phase) {terminal:.3e}, "
          f"largest over the nodes (nodes) {nodes:.3e}")
    assert abs(nodes - CPU_MAX_NODES) <= 0.02 * CPU_MAX_NODES
    assert terminal <= 1e-10               # (at the level the NLP tolerance leaves undetermined: see DESIGN 8e)
