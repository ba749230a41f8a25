"""The NumPy restatement of the derivative check's report (tests/deriv_restate.py: errors, expected_report, sum_keys) on
hand-made inputs, against literal expected values: what tests/test_gpu_deriv_report.py holds the device's report to is
itself pinned here, without a GPU."""
from types import SimpleNamespace

import numpy as np

from deriv_restate import errors, expected_report, sum_keys

INF, NAN = float("inf"), float("nan")

# 5 columns of colours 0 1 0 1 2; G~: 9 entries in 4 rows, three (row, colour) sums of two terms; H~: 3 entries; grad J~: 2
PLAN = SimpleNamespace(colour=np.array([0, 1, 0, 1, 2]), jac_located=np.array([1, 1, 0, 0, 1, 0, 0, 0, 0], bool))
G_STRUCT = (np.array([0, 0, 1, 1, 1, 2, 2, 3, 3]), np.array([0, 1, 0, 2, 4, 1, 3, 0, 2]))
H_STRUCT = (np.array([0, 2, 4]), np.array([0, 1, 4]))
JCOLS = np.array([4, 1])
STRUCT = (G_STRUCT, H_STRUCT, JCOLS)
# positions: G~ 0..8, sums 9..11, H~ 12..14, grad J~ 15..16


def test_sums_are_numbered_colour_by_colour():
    assert sum_keys(G_STRUCT, PLAN) == [(1, 0), (3, 0), (2, 1)]


def test_errors_of_located_entries_sums_and_non_finite_values():
    G = np.array([2.0, 0.5, 1.0, 2.0, INF, NAN, 1.0, 1.0, -0.5])
    fdG = np.array([1.0, 0.25, NAN, NAN, 1.0, NAN, NAN, NAN, NAN])
    sums = {(1, 0): ([2, 3], 1.0, [0.5, 0.25]),    # 1 * 0.5 + 2 * 0.25 = 1: clean
            (3, 0): ([7, 8], 0.0, [0.5, 0.5]),     # 0.5 - 0.25 = 0.25 against 0, largest term 0.5
            (2, 1): ([5, 6], 0.5, [0.5, 0.5])}     # a NaN term
    H, fdH = np.array([1.0, -4.0, 0.0]), np.array([1.0, -2.0, NAN])
    Jv, fdJ = np.array([-INF, 3.0]), np.array([1.0, 3.0])
    err = errors(G, H, Jv, fdG, fdH, fdJ, sums, G_STRUCT, PLAN)
    assert err.tolist() == [0.5, 0.25, -1.0, -1.0, INF, -1.0, -1.0, -1.0, -1.0, 0.0, 0.5, INF, 0.0, 0.5, INF, INF, 0.0]
    # an infinite FD value, and a quotient that overflows
    err = errors(np.array([1.0, 1e308] + [0.0] * 7), H, Jv, np.array([INF, -1e308] + [0.0] * 7), fdH, fdJ,
                 {(1, 0): ([2, 3], INF, [0.5, 0.25]), (3, 0): ([7, 8], 0.0, [0.5, 0.5]), (2, 1): ([5, 6], 0.0, [0.5, 0.5])},
                 G_STRUCT, PLAN)
    assert err[:2].tolist() == [INF, INF] and err[9:12].tolist() == [INF, 0.0, 0.0]


def _err(**at):
    e = np.array([0.0, 0.0, -1.0, -1.0, 0.0, -1.0, -1.0, -1.0, -1.0] + [0.0] * 8)
    for t, v in at.items():
        e[int(t[1:])] = v
    return e


def test_all_clean():
    rep = expected_report(_err(), 1e-4, 20, STRUCT, PLAN)
    assert rep == dict(n_fail=dict(jac=0, hess=0, grad=0), max_err=dict(jac=0.0, hess=0.0, grad=0.0),
                       worst=dict(jac=("jac", 0, 0, 0), hess=("hess", 0, 0, 0), grad=("grad", 0, -1, 4)), failures=[])
    # an error equal to tol passes: the comparison is strict
    rep = expected_report(_err(t1=1e-4), 1e-4, 20, STRUCT, PLAN)
    assert rep["n_fail"]["jac"] == 0 and rep["failures"] == [] and rep["max_err"]["jac"] == 1e-4
    assert rep["worst"]["jac"] == ("jac", 1, 0, 1)
    assert expected_report(_err(t1=1e-4), np.nextafter(1e-4, 0), 20, STRUCT, PLAN)["failures"] == [("jac", 1, 0, 1)]


def test_ties_go_to_the_lowest_position():
    rep = expected_report(_err(t1=0.5, t4=0.5, t10=0.5, t13=0.25, t14=0.25, t16=0.125), 1e-4, 20, STRUCT, PLAN)
    assert rep["n_fail"] == dict(jac=3, hess=2, grad=1)
    assert rep["max_err"] == dict(jac=0.5, hess=0.25, grad=0.125)
    assert rep["worst"] == dict(jac=("jac", 1, 0, 1), hess=("hess", 1, 2, 1), grad=("grad", 1, -1, 1))
    assert rep["failures"] == [("jac", 1, 0, 1), ("jac", 4, 1, 4), ("jac_sum", 1, 3, 0), ("hess", 1, 2, 1),
                               ("hess", 2, 4, 4), ("grad", 1, -1, 1)]
    # a sum is the worst only when it is strictly larger than every located entry
    assert expected_report(_err(t4=0.5, t9=0.75, t11=0.75), 1e-4, 20, STRUCT, PLAN)["worst"]["jac"] == ("jac_sum", 0, 1, 0)


def test_cap_and_max_report_zero():
    e = _err(t0=1.0, t1=2.0, t4=3.0, t9=4.0, t12=5.0, t16=6.0)
    full = [("jac", 0, 0, 0), ("jac", 1, 0, 1), ("jac", 4, 1, 4), ("jac_sum", 0, 1, 0), ("hess", 0, 0, 0), ("grad", 1, -1, 1)]
    for max_report, n in ((0, 0), (1, 1), (4, 4), (6, 6), (1000, 6), (-3, 0)):
        rep = expected_report(e, 1e-4, max_report, STRUCT, PLAN)
        assert rep["failures"] == full[:n]
        assert rep["n_fail"] == dict(jac=4, hess=1, grad=1)
        assert rep["worst"] == dict(jac=("jac_sum", 0, 1, 0), hess=("hess", 0, 0, 0), grad=("grad", 1, -1, 1))
    # more failures than the cap of 64: 100 located entries in one row, all failing
    gs = (np.zeros(100, int), np.arange(100))
    plan = SimpleNamespace(colour=np.arange(100), jac_located=np.ones(100, bool))
    rep = expected_report(np.full(100, 1.0), 0.5, 1000, (gs, (np.zeros(0, int), np.zeros(0, int)), np.zeros(0, int)), plan)
    assert rep["n_fail"]["jac"] == 100 and rep["failures"] == [("jac", i, 0, i) for i in range(64)]


def test_a_kind_without_entries():
    gs = (np.array([0, 1]), np.array([1, 0]))
    plan = SimpleNamespace(colour=np.array([0, 1]), jac_located=np.array([True, True]))
    none = (np.zeros(0, int), np.zeros(0, int))
    rep = expected_report(np.array([0.0, 0.5]), 1e-4, 20, (gs, none, np.zeros(0, int)), plan)
    assert rep == dict(n_fail=dict(jac=1, hess=0, grad=0), max_err=dict(jac=0.5, hess=0.0, grad=0.0),
                       worst=dict(jac=("jac", 1, 1, 0), hess=None, grad=None), failures=[("jac", 1, 1, 0)])
    assert sum_keys(gs, plan) == []


def test_inf_is_the_largest_and_negative_maxima_become_zero():
    rep = expected_report(_err(t4=INF, t0=INF, t1=1e300, t11=INF, t14=INF), 1e-4, 20, STRUCT, PLAN)
    assert rep["max_err"] == dict(jac=INF, hess=INF, grad=0.0)
    assert rep["worst"]["jac"] == ("jac", 0, 0, 0) and rep["worst"]["hess"] == ("hess", 2, 4, 4)
    assert [f[:2] for f in rep["failures"]] == [("jac", 0), ("jac", 1), ("jac", 4), ("jac_sum", 2), ("hess", 2)]
    # the -1 of sum terms never is a maximum: G~ of two terms of one clean sum
    gs = (np.array([0, 0]), np.array([0, 1]))
    plan = SimpleNamespace(colour=np.array([0, 0]), jac_located=np.array([False, False]))
    none = (np.zeros(0, int), np.zeros(0, int))
    rep = expected_report(np.array([-1.0, -1.0, 0.0]), 1e-4, 20, (gs, none, np.zeros(0, int)), plan)
    assert rep["max_err"]["jac"] == 0.0 and rep["n_fail"]["jac"] == 0 and rep["worst"]["jac"] == ("jac_sum", 0, 0, 0)
    # a kind whose maximum is negative reports 0
    assert expected_report(np.array([-1.0, -1.0, -0.5]), 1e-4, 20, (gs, none, np.zeros(0, int)), plan)["max_err"]["jac"] == 0.0
