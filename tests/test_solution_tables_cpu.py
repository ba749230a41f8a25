"""The coefficient tables of the dense output (pycollo_amd/solution.py::solution_tables) against an mpmath inverse of
the Legendre Vandermonde at the project's own quadrature points, and the argument errors of ``Solution.sample`` that
need no device."""
import mpmath as mp
import numpy as np
import pytest

from pycollo_amd.quadrature import QuadratureTables
from pycollo_amd.solution import Solution, check_queries, normalise_query, section_points, solution_tables

EPS = np.finfo(float).eps


def _exact_inverse(points, deg):
    """inverse of V[i][k] = P_k(x_i) with mpmath's own Legendre polynomials, 60 digits"""
    n = len(points)
    assert n == deg + 1
    V = mp.matrix(n, n)
    for i, x in enumerate(points):
        for k in range(n):
            V[i, k] = mp.legendre(k, mp.mpf(float(x)))
    return mp.inverse(V)


@pytest.mark.parametrize("method", ["lobatto", "radau"])
@pytest.mark.parametrize("n", range(2, 21))
def test_tables_are_the_exact_ones_rounded(method, n):
    with mp.workdps(60):
        quad = QuadratureTables(method)
        x = section_points(quad, n)
        if method == "lobatto":
            np.testing.assert_array_equal(x, quad.points(n))
        else:   # the rule's n-1 points and the section's end
            np.testing.assert_array_equal(x[:-1], quad.points(n)[:-1])
            assert x[-1] == 1.0
        Cd, Cu = solution_tables(method, n)
        assert Cd.shape == Cu.shape == (n, n)
        exact_u = _exact_inverse(x, n - 1)
        if method == "lobatto":
            exact_d = exact_u
        else:
            inner = _exact_inverse(x[:-1], n - 2)
            exact_d = mp.zeros(n, n)
            for i in range(n - 1):
                for j in range(n - 1):
                    exact_d[i, j] = inner[i, j]
        for got, ref in ((Cd, exact_d), (Cu, exact_u)):
            for i in range(n):
                row_max = max(abs(ref[i, j]) for j in range(n))
                for j in range(n):
                    err = abs(mp.mpf(float(got[i, j])) - ref[i, j])
                    assert err <= EPS * row_max, (method, n, i, j, float(err / (EPS * row_max)) if row_max else err)
        # the interpolant reproduces its node values (a table indexed the wrong way round does not)
        f = np.cos(1.3 * x) + 0.2 * x
        np.testing.assert_allclose(np.polynomial.legendre.legval(x, Cu @ f), f, rtol=0, atol=1e-12)
        m = n if method == "lobatto" else n - 1
        np.testing.assert_allclose(np.polynomial.legendre.legval(x[:m], Cd @ f), f[:m], rtol=0, atol=1e-12)


def test_tables_are_cached():
    assert solution_tables("lobatto", 7)[0] is solution_tables("lobatto", 7)[0]
    with pytest.raises(ValueError):
        solution_tables("lobatto", 7)[0][0, 0] = 1.0     # read-only: the cache cannot be damaged through a result


def _bare_solution():
    """a Solution with the host-side state ``sample`` reads before it needs the device"""
    s = Solution.__new__(Solution)
    s.state = (np.zeros((2, 5)),)
    s.initial_time, s.final_time = (0.5,), (2.5,)
    s._h = None
    s.engine = None
    return s


def test_sample_argument_errors_without_a_device():
    s = _bare_solution()
    with pytest.raises(ValueError, match="either t or tau"):
        s.sample(0)
    with pytest.raises(ValueError, match="either t or tau"):
        s.sample(0, np.zeros(3), tau=np.zeros(3))
    with pytest.raises(ValueError, match="one-dimensional"):
        s.sample(0, np.zeros((2, 2)))
    with pytest.raises(ValueError, match="phase 1 out of range"):
        s.sample(1, np.array([1.0]))
    with pytest.raises(ValueError, match="outside the phase"):
        s.sample(0, np.array([1.0, 2.5000001]))
    with pytest.raises(ValueError, match="outside the phase"):
        s.sample(0, np.array([0.4999999, 1.0]))
    with pytest.raises(ValueError, match="outside the phase"):
        s.sample(0, tau=np.array([-1.0, 1.0000001]))
    with pytest.raises(ValueError, match="NaN"):
        s.sample(0, np.array([1.0, np.nan]), extrapolate=True)
    # in range / extrapolating: the next thing it needs is the device
    for kw in (dict(t=np.array([0.5, 2.5])), dict(tau=np.array([-1.0, 1.0])), dict(t=np.array([9.0]), extrapolate=True)):
        with pytest.raises(ValueError, match="closed"):
            s.sample(0, **kw)


def test_query_helpers():
    q, is_tau = normalise_query(None, [0.0, 0.5])
    assert is_tau and q.dtype == np.float64 and q.shape == (2,)
    check_queries(-1.0, 1.0, False, False)
    with pytest.raises(ValueError):
        check_queries(-1.0, 1.0 + 4 * EPS, False, False)            # tau itself: no slack
    check_queries(-1.0 - 4 * EPS, 1.0 + 4 * EPS, False, False, 8 * EPS)   # a time a few ulp past the end is the end
    with pytest.raises(ValueError):
        check_queries(-1.0, 1.0 + 16 * EPS, False, False, 8 * EPS)
    check_queries(-1.5, 0.5, False, True)
    # a phase run backwards in time (tF < t0): the range is the same in tau
    s = _bare_solution()
    s.initial_time, s.final_time = (2.5,), (0.5,)
    with pytest.raises(ValueError, match="closed"):
        s.sample(0, np.array([0.5, 2.5]))
    with pytest.raises(ValueError, match="outside the phase"):
        s.sample(0, np.array([0.4]))
