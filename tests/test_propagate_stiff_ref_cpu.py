"""CPU checks of the tests' restatement of the implicit propagation (tests/propagate_stiff_ref.py), which
tests/test_gpu_propagate_stiff.py then holds the kernel to.

1. The tableau, in exact rationals: row sums, the eight order conditions through order 4 for b, order 3 and the four
   order-4 residuals of the embedded weights, R(inf) = 0 and R^(inf) = 10/3.
2. The fixed mode converges at order 4 against the existing 60-digit Dormand-Prince truth.
3. The float64 restatement against the exact step of the method (60 digits, every stage equation solved to 1e-40):
   |f64 - exact| <= n (atol_a + rtol max|y_a|) exp(L T), n the steps taken in the segment up to the node.  This is the
   bound the kernel inherits.
4. The adaptive mode on the stiff relaxation phase (rate 1e4) against its exact flow:
   |got - exact| <= a (atol_a + rtol max|y_a|), a the accepted steps up to the node; the explicit pair's restatement
   under max_steps = 256 fails its first interval there.
5. The headline phase at its own final time of 10 000, rtol 1e-6, default max_steps: every segment of ``nodes`` and
   ``sections`` completes, within a (atol_a + rtol max|y_a|) exp(L T) (L = 0) of the 60-digit truth: the method's fixed
   mode with m doubled until no arrival moves by 1e-3 (atol + rtol |y|), which took m = 512 and minutes, so it is a
   fixture (tests/golden/propagate_stiff_headline.npz, made by tools/make_propagate_stiff_golden.py) of which one
   segment is recomputed here.
6. Near-threshold decisions: in the adaptive cases the GPU file uses, at most 1 interval in 20 has a decision within
   relative 1e-6 of its threshold.
"""
import os
from fractions import Fraction as Fr

import numpy as np
import pytest

import propagate_ref as pr
import propagate_stiff_ref as ps
from conftest import ROOT, golden_tables
from oracle.ref_numpy import OracleNlp
from pycollo_amd import problems
from test_propagate_ref_cpu import TRUTH_M

RESTARTS = ("nodes", "sections", "phase", "irregular")
CASES = dict(pr.CASES)
CASES[ps.STIFF_CASE] = ps.stiff_case
# The inputs of the fixed-mode comparison: rtol 1e-6 (atol = rtol V) and newton_max = 16.  At the defaults (rtol 1e-9,
# newton_max = 8) the restatement's Newton iteration, which keeps the Jacobian of the step's start, runs out on the
# hypersensitive meshes with h |df/dy| ~ 3 (one interval of hypersensitive_K5_n4); at rtol 1e-6 and newton_max = 8 one
# interval of order_extremes_2_and_20 still does at m = 1 (the failure-convention test of the GPU file uses it).  The
# inputs were changed, not the bound.
FIXED_RTOL = 1e-6
FIXED_NEWTON_MAX = 16
# (case, m, restart) at which the float64 restatement itself misses the bound of 3, each with its own ratio
FIXED_DROPPED = {}
ADAPTIVE_RESTARTS = ("nodes", "sections", "phase")
ADAPTIVE_RTOLS = (1e-6, 1e-10)
# (restart, rtol) on the stiff relaxation phase at which the float64 restatement itself misses the bound of 4
ADAPTIVE_DROPPED = {}
NEAR = 1e-6
FAILURE_CASE = "order_extremes_2_and_20"


def _method(prob):
    return getattr(prob, "quadrature_method", None) or "lobatto"


_data = {}


def phase_data(name):
    """([PhaseData per phase], oracle) of a case at the smooth point, from the oracle alone"""
    if name not in _data:
        prob = CASES[name]()
        ora = OracleNlp(prob, golden_tables(_method(prob)))
        x = pr.smooth_x_oracle(ora)
        _data[name] = [pr.PhaseData.from_oracle(ora, ip, x, _method(prob)) for ip in range(len(ora.P))], ora
    return _data[name]


def state_scale(ora, ip, d):
    return np.asarray(ora.V_ocp[ora.P[ip].ox:ora.P[ip].ox + d.n_y], dtype=np.float64)


# ---- 1. the tableau --------------------------------------------------------------------------------------------------
def _order_sums(b):
    """the left sides of the eight order conditions through order 4, in the order 1, c, c^2, Ac, c^3, c.Ac, Ac^2, AAc"""
    A = [[row[j] if j < len(row) else Fr(0) for j in range(5)] for row in ps.A_FR]
    c = ps.C_FR
    Ac = [sum(A[i][j] * c[j] for j in range(5)) for i in range(5)]
    Ac2 = [sum(A[i][j] * c[j] ** 2 for j in range(5)) for i in range(5)]
    AAc = [sum(A[i][j] * Ac[j] for j in range(5)) for i in range(5)]
    dot = lambda v: sum(bi * vi for bi, vi in zip(b, v))
    return [dot([Fr(1)] * 5), dot(c), dot([v ** 2 for v in c]), dot(Ac), dot([v ** 3 for v in c]),
            dot([ci * v for ci, v in zip(c, Ac)]), dot(Ac2), dot(AAc)]


ORDER_RHS = [Fr(1), Fr(1, 2), Fr(1, 3), Fr(1, 6), Fr(1, 4), Fr(1, 8), Fr(1, 12), Fr(1, 24)]


def _r_inf(b):
    import sympy as sym
    A = sym.Matrix(5, 5, lambda i, j: sym.Rational(ps.A_FR[i][j].numerator, ps.A_FR[i][j].denominator) if j <= i else 0)
    bb = sym.Matrix([[sym.Rational(v.numerator, v.denominator) for v in b]])
    return 1 - (bb * A.inv() * sym.ones(5, 1))[0, 0]


def test_tableau_in_exact_rationals():
    import sympy as sym
    for i, row in enumerate(ps.A_FR):
        assert len(row) == i + 1 and row[-1] == ps.GAMMA and sum(row) == ps.C_FR[i]
    assert ps.B_FR == ps.A_FR[4] and ps.C_FR[4] == 1                                   # stiffly accurate
    assert _order_sums(ps.B_FR) == ORDER_RHS
    hat = [s - r for s, r in zip(_order_sums(ps.BHAT_FR), ORDER_RHS)]
    assert hat[:4] == [0, 0, 0, 0]
    assert hat[4:] == [Fr(-27, 1280), Fr(-9, 1280), Fr(5, 768), Fr(7, 768)] and all(v != 0 for v in hat[4:])
    assert ps.E_FR == [Fr(-3, 16), Fr(-27, 32), Fr(25, 32), Fr(0), Fr(1, 4)]
    assert _r_inf(ps.B_FR) == 0 and _r_inf(ps.BHAT_FR) == sym.Rational(10, 3)
    assert ps.A[4] == ps.B and ps.G == 0.25 and [float(v) for v in ps.E_FR] == ps.E


# ---- 2. order --------------------------------------------------------------------------------------------------------
def test_fixed_mode_converges_at_order_4():
    name = "hypersensitive_K5_n4"
    d = phase_data(name)[0][0]
    seg = pr.segments("phase", d.s, d.N)
    truth = pr.FixedReference(d).arrivals(seg, TRUTH_M[name])[0]
    ex = ps.ExactFixed(d)
    size = float(np.max(np.abs(truth)))
    err = {m: float(np.max(np.abs(ex.arrivals(seg, m)[0] - truth))) for m in (1, 2, 4, 8, 16, 32)}
    pairs = [(m, 2 * m) for m in (1, 2, 4, 8, 16) if err[2 * m] > 1e-13 * size][-2:]
    assert len(pairs) == 2
    for a, b in pairs:
        ratio = err[a] / err[b]
        print(f"m = {a} -> {b}: error {err[a]:.3e} -> {err[b]:.3e}, ratio {ratio:.2f}")
        assert 2 ** 3.5 <= ratio <= 2 ** 4.5


# ---- 3. the float64 restatement against the exact step ---------------------------------------------------------------
_exact = {}


def exact_fixed(name, ip):
    if (name, ip) not in _exact:
        _exact[name, ip] = ps.ExactFixed(phase_data(name)[0][ip])
    return _exact[name, ip]


def fixed_lipschitz(name, d, exact):
    """``propagate_ref.lipschitz``; 0 on the stiff relaxation phase, as in 4: y2 is integrated exactly and y1 contracts
    (the symmetric part of its Jacobian, with rate cos y2 off the diagonal, would give exp(L T) = inf and no check)"""
    return 0.0 if name == ps.STIFF_CASE else pr.lipschitz(d, exact)


@pytest.mark.parametrize("name", list(CASES))
def test_float64_restatement_within_the_fixed_bound(name):
    data, ora = phase_data(name)
    for ip, d in enumerate(data):
        atol = FIXED_RTOL * state_scale(ora, ip, d)
        for m in (1, 3):
            for restart in RESTARTS:
                seg = pr.segments(restart, d.s, d.N)
                exact = exact_fixed(name, ip).arrivals(seg, m)[0]
                L = fixed_lipschitz(name, d, exact)
                R = ps.propagate_f64(d, seg, substeps=m, rtol=FIXED_RTOL, atol=atol, newton_max=FIXED_NEWTON_MAX)
                assert np.all(R.status == -1) and np.all(R.accepted[1:] == m) and not R.rejected.any()
                bound = ps.fixed_bound(d, seg, exact, m, atol, FIXED_RTOL, L)
                ratio = float(np.max(np.abs(R.y - exact)[:, 1:] / bound[:, 1:]))
                print(f"{name} phase {ip} m = {m} {restart}: L = {L:.3g}, |f64 - exact| / bound = {ratio:.3e}, "
                      f"{int(R.newton_iterations.sum())} Newton iterations")
                if (name, m, restart) in FIXED_DROPPED:
                    assert ratio > 1.0, "a dropped combination meets the bound: take it off FIXED_DROPPED"
                else:
                    assert ratio <= 1.0
    assert 8 * len(FIXED_DROPPED) <= len(CASES) * 2 * len(RESTARTS)


# ---- 4. adaptive mode on the stiff relaxation phase -------------------------------------------------------------------
def adaptive_stiff(restart, rtol, **kw):
    data, ora = phase_data(ps.STIFF_CASE)
    d = data[0]
    seg = pr.segments(restart, d.s, d.N)
    atol = rtol * state_scale(ora, 0, d)
    return d, seg, atol, ps.propagate_f64(d, seg, rtol=rtol, atol=atol, **kw)


@pytest.mark.parametrize("restart", ADAPTIVE_RESTARTS)
def test_adaptive_mode_on_the_stiff_relaxation_phase(restart):
    for rtol in ADAPTIVE_RTOLS:
        d, seg, atol, R = adaptive_stiff(restart, rtol)
        exact = ps.relaxation_exact(d, seg)
        assert np.all(R.status == -1) and np.all(R.accepted[1:] >= 1)
        bound = pr.adaptive_bound(d, seg, exact, R.accepted, atol, rtol, 0.0)
        ratio = float(np.max(np.abs(R.y - exact)[:, 1:] / bound[:, 1:]))
        print(f"stiff relaxation {restart} rtol {rtol:g}: error / bound = {ratio:.3e}; {int(R.accepted.sum())} accepted, "
              f"{int(R.rejected.sum())} rejected ({int(R.newton_rejected.sum())} by Newton), "
              f"{int(R.newton_iterations.sum())} Newton iterations")
        if (restart, rtol) in ADAPTIVE_DROPPED:
            assert ratio > 1.0, "a dropped combination meets the bound: take it off ADAPTIVE_DROPPED"
        else:
            assert ratio <= 1.0
    assert 8 * len(ADAPTIVE_DROPPED) <= len(ADAPTIVE_RESTARTS) * len(ADAPTIVE_RTOLS)


@pytest.mark.parametrize("restart", ADAPTIVE_RESTARTS)
def test_the_explicit_pair_fails_its_first_interval_there(restart):
    data, ora = phase_data(ps.STIFF_CASE)
    d = data[0]
    seg = pr.segments(restart, d.s, d.N)
    for rtol in ADAPTIVE_RTOLS:
        with np.errstate(all="ignore"):
            y, acc, rej, st = pr.propagate_f64(d, seg, rtol=rtol, atol=rtol * state_scale(ora, 0, d), max_steps=256)
        np.testing.assert_array_equal(st, seg[:-1])
        assert np.all(np.isnan(y[:, 1:]))


# ---- 5. the headline phase at its own final time ---------------------------------------------------------------------
HEADLINE_RTOL = 1e-6


def headline_data():
    if "headline" not in _data:
        prob = problems.hypersensitive(K=5, order=4)
        ora = OracleNlp(prob, golden_tables("lobatto"))
        _data["headline"] = [pr.PhaseData.from_oracle(ora, 0, pr.smooth_x_oracle(ora), "lobatto")], ora
    return _data["headline"]


HEADLINE_GOLDEN = os.path.join(ROOT, "tests", "golden", "propagate_stiff_headline.npz")
# restarts at which the float64 restatement itself misses the bound of 5
HEADLINE_DROPPED = {}


def headline_truth(restart):
    """(arrivals [n_y][N], m) of the fixture"""
    with np.load(HEADLINE_GOLDEN) as g:
        return g[f"y_{restart}"].copy(), int(g[f"m_{restart}"])


def test_headline_fixture_is_what_its_generator_makes():
    data, ora = headline_data()
    d = data[0]
    with np.load(HEADLINE_GOLDEN) as g:
        assert float(g["rtol"]) == HEADLINE_RTOL
        np.testing.assert_array_equal(g["atol"], HEADLINE_RTOL * state_scale(ora, 0, d))
        np.testing.assert_array_equal(g["node_y"], d.node_y)                # the same doubles went in
        np.testing.assert_array_equal(g["coef_u"], d.coef_u)
        np.testing.assert_array_equal(g["tau"], d.tau)
        assert float(g["moved_nodes"]) <= 1e-3 and float(g["moved_sections"]) <= 1e-3
    for restart in ("nodes", "sections"):
        y, m = headline_truth(restart)
        assert y.shape == d.node_y.shape and np.all(np.isfinite(y)) and m >= 128
        print(f"headline truth, {restart}: m = {m}")
    # one segment again: the last node interval, from its own node
    y, m = headline_truth("nodes")
    ch = ps.ExactFixed(d)._extend(d.N - 2, m, d.N - 1)
    np.testing.assert_array_equal(np.array([float(v) for v in ch[1]]), y[:, -1])


@pytest.mark.parametrize("restart", ("nodes", "sections"))
def test_headline_phase_completes_at_final_time_10000(restart):
    data, ora = headline_data()
    d = data[0]
    seg = pr.segments(restart, d.s, d.N)
    atol = HEADLINE_RTOL * state_scale(ora, 0, d)
    R = ps.propagate_f64(d, seg, rtol=HEADLINE_RTOL, atol=atol)
    truth = headline_truth(restart)[0]
    L = pr.lipschitz(d, truth)
    assert L == 0.0                                                        # df/dy = -3 y^2
    ratio = float(np.max(np.abs(R.y - truth)[:, 1:] / pr.adaptive_bound(d, seg, truth, R.accepted, atol, HEADLINE_RTOL, L)[:, 1:]))
    print(f"hypersensitive T = 10000 {restart}: error / bound = {ratio:.3e}")
    if restart in HEADLINE_DROPPED:
        assert ratio > 1.0, "a dropped restart meets the bound: take it off HEADLINE_DROPPED"
    else:
        assert ratio <= 1.0
    print(f"hypersensitive T = 10000 {restart}: {int(R.accepted.sum())} accepted, {int(R.rejected.sum())} rejected "
          f"({int(R.newton_rejected.sum())} by Newton), {int(R.newton_iterations.sum())} Newton iterations")
    assert np.all(R.status == -1) and np.all(np.isfinite(R.y))
    # the explicit pair's restatement under the same cap does not get through
    with np.errstate(all="ignore"):
        st = pr.propagate_f64(d, seg, rtol=HEADLINE_RTOL, atol=atol)[3]
    print(f"  the explicit pair completes {int(np.sum(st == -1))} of {len(st)} segments")
    assert np.any(st >= 0)


# ---- 6. near-threshold decisions ---------------------------------------------------------------------------------------
def test_newton_max_8_fails_one_interval_of_the_order_extremes_mesh():
    # the premise of the GPU file's failure-convention test: fixed mode, m = 1, restart at every node, rtol 1e-6
    data, ora = phase_data(FAILURE_CASE)
    d = data[0]
    seg = pr.segments("nodes", d.s, d.N)
    atol = FIXED_RTOL * state_scale(ora, 0, d)
    short = ps.propagate_f64(d, seg, substeps=1, rtol=FIXED_RTOL, atol=atol, newton_max=8)
    full = ps.propagate_f64(d, seg, substeps=1, rtol=FIXED_RTOL, atol=atol, newton_max=FIXED_NEWTON_MAX)
    failed = short.status >= 0
    assert np.all(full.status == -1) and failed.any() and not failed.all()
    np.testing.assert_array_equal(short.status[failed], seg[:-1][failed])
    np.testing.assert_array_equal(short.y[:, 1:][:, ~failed], full.y[:, 1:][:, ~failed])      # the same bits elsewhere
    assert np.all(np.isnan(short.y[:, 1:][:, failed]))
    np.testing.assert_array_equal(short.rejected[1:], failed.astype(int))
    np.testing.assert_array_equal(short.newton_rejected[1:], failed.astype(int))
    assert np.all(short.newton_iterations[1:][failed] <= 5 * 8)


def test_few_decisions_fall_near_their_threshold():
    total = near = 0
    for restart in ADAPTIVE_RESTARTS:
        for rtol in ADAPTIVE_RTOLS:
            R = adaptive_stiff(restart, rtol)[3]
            total += len(R.near) - 1
            near += int(np.sum(R.near[1:] < NEAR))
    for restart in ("nodes", "sections"):
        data, ora = headline_data()
        d = data[0]
        R = ps.propagate_f64(d, pr.segments(restart, d.s, d.N), rtol=HEADLINE_RTOL, atol=HEADLINE_RTOL * state_scale(ora, 0, d))
        total += len(R.near) - 1
        near += int(np.sum(R.near[1:] < NEAR))
    print(f"{near} of {total} intervals have a decision within relative {NEAR:g} of its threshold")
    assert 20 * near <= total
