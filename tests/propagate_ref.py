"""The tests' own host restatement of the forward propagation (pycollo_amd/csrc/pc_solution.hpp,
pc_sol_propagate_p<i>).  TEST INFRASTRUCTURE: nothing here shares code with the kernel or with ``Solution.propagate``.

Per phase: N nodes at ``tau``, K sections, section k with n_k nodes from node ``s[k]``, width w_k = tau[s[k+1]] -
tau[s[k]]; the position of node j in section k is c_j = 2 (tau_j - tau_{s_k}) / w_k - 1 (float64, in this order).  Inside
section k

    dy/dc = stretch (w_k / 2) f(y, u(c), q, t0, tF, s),     u(c) = sum_m e_m P_m(c),

e the section's ``coef_u``.  A segment [j0, j1] starts from ``node_y[:, j0]`` and crosses the node intervals in order.

* :func:`propagate_f64`: float64 NumPy, both modes, the kernel's arithmetic step by step.
* :func:`FixedReference`: the fixed mode in mpmath at 60 digits.  The doubles it is fed (node values, coefficients,
  c_j, the step starts c_j + i h and widths h, the rounded tableau) are taken as exact; everything from there is exact
  to 60 digits.  With every arrival it returns the rounding scale of the project's parity rule carried through an RK
  step: n, the number of steps taken in the segment up to that node, and M_a, the largest value over those steps of
  |y_a| + |h g| sum_i |b_i| F_a,i, where F_a,i is stage i's f_a with every term taken in absolute value
  (``oracle.ref_numpy._mag_expr``) and g = stretch w_k / 2.
"""
from fractions import Fraction as Fr

import mpmath as mp
import numpy as np
import sympy as sym

from oracle.ref_numpy import _mag_expr

DPS = 60
EPS = np.finfo(float).eps

# Dormand-Prince 5(4) (Dormand & Prince 1980), as exact fractions; rounded once
_A = [[],
      [Fr(1, 5)],
      [Fr(3, 40), Fr(9, 40)],
      [Fr(44, 45), Fr(-56, 15), Fr(32, 9)],
      [Fr(19372, 6561), Fr(-25360, 2187), Fr(64448, 6561), Fr(-212, 729)],
      [Fr(9017, 3168), Fr(-355, 33), Fr(46732, 5247), Fr(49, 176), Fr(-5103, 18656)]]
_B = [Fr(35, 384), Fr(0), Fr(500, 1113), Fr(125, 192), Fr(-2187, 6784), Fr(11, 84)]
_C = [Fr(0), Fr(1, 5), Fr(3, 10), Fr(4, 5), Fr(8, 9), Fr(1)]
_E = [Fr(-71, 57600), Fr(0), Fr(71, 16695), Fr(-71, 1920), Fr(17253, 339200), Fr(-22, 525), Fr(1, 40)]
A = np.zeros((6, 5))
for _i, _row in enumerate(_A):
    A[_i, :len(_row)] = [float(v) for v in _row]
B = np.array([float(v) for v in _B])
C = np.array([float(v) for v in _C])
E = np.array([float(v) for v in _E])
# rows of the seven stages' states: rows 0 .. 5 of A, then b; abscissae; 7 entries each
ROWS = [list(A[i, :i]) for i in range(6)] + [list(B)]
CS = list(C) + [1.0]


def legendre_f64(cf, c):
    """sum_j cf[j] P_j(c) by Clenshaw's recurrence, float64, the kernel's operation order"""
    u1 = u2 = 0.0
    for j in range(len(cf) - 1, -1, -1):
        al, be = float(2 * j + 1) / float(j + 1) * c, float(j + 1) / float(j + 2)
        u1, u2 = cf[j] + (al * u1 - be * u2), u1
    return u1


def legendre_mp(cf, c):
    p0, p1, acc = mp.mpf(1), c, mp.mpf(0)
    for j, v in enumerate(cf):
        acc += v * p0
        p0, p1 = p1, ((2 * j + 3) * c * p1 - (j + 1) * p0) / (j + 2)
    return acc


def _guard(fn, a):
    """fn(*a) in Python floats; an overflow is inf and an invalid operation NaN, as in IEEE arithmetic"""
    try:
        return float(fn(*a))
    except OverflowError:
        return float("inf")
    except (ValueError, ZeroDivisionError):
        return float("nan")


class PhaseData:
    """One phase's inputs of a propagation.  ``P``: the oracle's phase record (``OracleNlp.P[ip]``: the expressions f
    and their arguments); ``tau`` [N]; ``s`` [K+1]; ``node_y`` [n_y][N]; ``coef_u`` [n_u][N + K - 1]; ``w``: the
    unscaled [q | free t | s] arguments of f."""

    def __init__(self, P, tau, s, node_y, coef_u, t0, tF, w):
        self.P = P
        self.tau = np.asarray(tau, dtype=np.float64)
        self.s = np.asarray(s, dtype=np.int64)
        self.N, self.K = len(self.tau), len(self.s) - 1
        self.n_y, self.n_u = P.n_y, P.n_u
        self.node_y = np.asarray(node_y, dtype=np.float64).reshape(self.n_y, self.N)
        self.coef_u = np.asarray(coef_u, dtype=np.float64).reshape(self.n_u, self.N + self.K - 1)
        self.t0, self.tF = float(t0), float(tF)
        self.stretch = 0.5 * (self.tF - self.t0)
        self.w = [float(v) for v in w]
        assert len(self.w) == P.n_w
        self.sec_of = np.repeat(np.arange(self.K), np.diff(self.s))       # section of interval (j, j + 1)
        csyms = list(P.consts)
        args = list(P.v) + csyms
        self._cvals = [P.consts[k] for k in csyms]
        self._f64 = [sym.lambdify(args, e, modules="math") for e in P.f]
        self._fmp = [sym.lambdify(args, e, modules="mpmath") for e in P.f]
        real = [{"re": lambda z: z, "im": lambda z: 0.0}, "math"]          # (Abs of a function prints re / im of its argument)
        self._fmag = [sym.lambdify(args, _mag_expr(e), modules=real) for e in P.f]
        self._dfdy = [[sym.lambdify(args, sym.diff(e, v), modules="math") for v in P.v[:P.n_y]] for e in P.f]
        self._ucache = {}

    @classmethod
    def from_oracle(cls, ora, ip, x, method):
        """CPU only: node values by the oracle's unscaling, control coefficients by the rounded exact C_u tables"""
        from pycollo_amd.solution import solution_tables
        P = ora.P[ip]
        z, _, _, _, w = ora._unpack(P, np.asarray(x, dtype=np.float64))
        mesh = P.mesh
        s = np.asarray(mesh.bnd, dtype=np.int64)
        NC = mesh.N + mesh.K - 1
        coef = np.zeros((P.n_u, NC))
        for k in range(mesh.K):
            n = int(mesh.nodes[k])
            Cu = solution_tables(method, n)[1]
            for b in range(P.n_u):
                for j in range(n):
                    acc = 0.0
                    for i in range(n):
                        acc += Cu[j, i] * z[P.n_y + b, s[k] + i]
                    coef[b, s[k] + k + j] = acc
        t, j = [], 0
        V, r = ora.V_ocp, ora.r_ocp
        to = P.ox + P.n_z + P.n_q
        tt = x[P.t_off:P.t_off + P.n_t]
        for e in (0, 1):
            if P.t_free[e]:
                t.append(V[to + j] * tt[j] + r[to + j])
                j += 1
            else:
                t.append(P.t_fixed[e])
        return cls(P, mesh.tau, s, z[:P.n_y], coef, t[0], t[1], w)

    @classmethod
    def from_solution(cls, sol, ora, ip):
        """the kernel's own node values and coefficient arrays (``Solution.coefficients``)"""
        P = ora.P[ip]
        mesh = sol.engine.meshes[ip]
        w = np.concatenate([sol.integral[ip], sol.time[ip], sol.parameter])
        return cls(P, sol.tau[ip], mesh.s, sol.state[ip], sol.coefficients(ip)[1], sol.initial_time[ip], sol.final_time[ip], w)

    # ---- where interval (j, j + 1) lies --------------------------------------------------------------------
    def interval(self, j):
        """(k, coefficient slice, c_j, c_{j+1}, g) of the interval from node j, float64 as the kernel forms them"""
        k = int(self.sec_of[j])
        sk, n = int(self.s[k]), int(self.s[k + 1] - self.s[k] + 1)
        ta = self.tau[sk]
        w = self.tau[int(self.s[k + 1])] - ta
        ca = 2.0 * (self.tau[j] - ta) / w - 1.0
        cb = 2.0 * (self.tau[j + 1] - ta) / w - 1.0
        return k, slice(sk + k, sk + k + n), float(ca), float(cb), float(self.stretch * (0.5 * w))

    # ---- f -------------------------------------------------------------------------------------------------
    def f64(self, y, sl, c):
        u = [legendre_f64(self.coef_u[b, sl], c) for b in range(self.n_u)]
        a = [float(v) for v in y] + u + self.w + self._cvals
        return np.array([_guard(fn, a) for fn in self._f64])

    def u_mp(self, sl, c):
        key = (sl.start, float(c))
        if key not in self._ucache:
            self._ucache[key] = [legendre_mp([mp.mpf(float(v)) for v in self.coef_u[b, sl]], mp.mpf(float(c)))
                                 for b in range(self.n_u)]
        return self._ucache[key]

    def fmp(self, y, u):
        a = list(y) + list(u) + [mp.mpf(v) for v in self.w] + [mp.mpf(float(v)) for v in self._cvals]
        return [mp.mpf(fn(*a)) for fn in self._fmp]

    def fmag(self, y, u):
        a = [float(v) for v in y] + [float(v) for v in u] + self.w + self._cvals
        return np.array([_guard(fn, a) for fn in self._fmag])

    def jac_y(self, y, u):
        a = [float(v) for v in y] + [float(v) for v in u] + self.w + self._cvals
        return np.array([[float(fn(*a)) for fn in row] for row in self._dfdy]).reshape(self.n_y, self.n_y)

    def node_time(self, j):
        return self.tau[j] * self.stretch + 0.5 * (self.t0 + self.tF)


# ---- float64: the kernel's arithmetic -----------------------------------------------------------------------------
def step_f64(d, y, sl, c, h, g, want_err, atol=None, rtol=None):
    """one Dormand-Prince step of width h from (c, y): (ynew, err); err None unless ``want_err``"""
    Ks = []
    ys = y
    for s in range(7):
        if s:
            acc = np.zeros(d.n_y)
            for i, wgt in enumerate(ROWS[s]):
                if wgt != 0.0:
                    acc = acc + wgt * Ks[i]
            ys = y + h * acc
        if s < 6 or want_err:
            cc = c if s == 0 else c + CS[s] * h
            Ks.append(g * d.f64(ys, sl, cc))
    ynew = ys
    if not want_err:
        return ynew, None
    e = np.zeros(d.n_y)
    for i, wgt in enumerate(E):
        if wgt != 0.0:
            e = e + wgt * Ks[i]
    with np.errstate(all="ignore"):
        r = np.abs(h * e) / (atol + rtol * np.maximum(np.abs(y), np.abs(ynew)))
    if not np.all(np.isfinite(r)):
        return ynew, float("nan")
    return ynew, float(np.max(r)) if d.n_y else 0.0


def propagate_f64(d, seg, *, substeps=0, rtol=1e-9, atol=None, max_steps=4096):
    """(y_arrive [n_y][N], accepted [N], rejected [N], seg_status [n_seg]) by the definition, in float64"""
    N = d.N
    y_arr = np.full((d.n_y, N), np.nan)
    acc, rej = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    status = np.full(len(seg) - 1, -1, dtype=np.int64)
    y_arr[:, 0] = d.node_y[:, 0]
    atol = None if atol is None else np.asarray(atol, dtype=np.float64)
    for i in range(len(seg) - 1):
        y = d.node_y[:, int(seg[i])].copy()
        for j in range(int(seg[i]), int(seg[i + 1])):
            if status[i] >= 0:
                continue                                   # NaN arrival, zero counts
            _, sl, ca, cb, g = d.interval(j)
            if substeps > 0:
                h = (cb - ca) / float(substeps)
                for q in range(substeps):
                    c = ca + float(q) * h
                    y, _ = step_f64(d, y, sl, c, cb - c if q == substeps - 1 else h, g, False)
                acc[j + 1] = substeps
            else:
                c, h = ca, cb - ca
                last, after_reject, done = True, False, False
                while not done and acc[j + 1] + rej[j + 1] < max_steps:
                    ynew, err = step_f64(d, y, sl, c, h, g, True, atol, rtol)
                    bad = not np.isfinite(err)
                    factor = 0.2
                    if not bad:
                        factor = 5.0 if err == 0.0 else min(5.0, max(0.2, 0.9 * err ** -0.2))
                    if not bad and err <= 1.0:
                        acc[j + 1] += 1
                        y = ynew
                        c = cb if last else c + h
                        if after_reject:
                            factor = min(factor, 1.0)
                        after_reject = False
                        rest = cb - c
                        if last or not rest > 0.0:
                            done = True
                        else:
                            h = h * factor
                            last = h >= rest
                            if last:
                                h = rest
                    else:
                        rej[j + 1] += 1
                        h = h * factor
                        last, after_reject = False, True
                if not done:
                    status[i] = j
                    continue
            y_arr[:, j + 1] = y
    return y_arr, acc, rej, status


# ---- 60 digits: the fixed mode --------------------------------------------------------------------------------------
class FixedReference:
    """The fixed mode at 60 digits.  ``arrivals(seg, m)`` -> (y [n_y][N], steps [N], M [n_y][N]); column 0 is y(0) with
    steps 0.  Chains are kept per (start node, m): a segment is a prefix of the chain from its start, so the modes
    of a test share their work."""

    def __init__(self, data):
        self.d = data
        self._chain = {}

    def _step(self, y, sl, c, h, g):
        d = self.d
        hm, gm = mp.mpf(h), mp.mpf(g)
        Ks, mags = [], np.zeros(d.n_y)
        for s in range(6):
            ys = y if s == 0 else [y[a] + hm * sum(mp.mpf(wgt) * Ks[i][a] for i, wgt in enumerate(ROWS[s]) if wgt != 0.0)
                                    for a in range(d.n_y)]
            cc = mp.mpf(c) if s == 0 else mp.mpf(c) + mp.mpf(CS[s]) * hm
            u = d.u_mp(sl, float(cc)) if s == 0 else [legendre_mp([mp.mpf(float(v)) for v in d.coef_u[b, sl]], cc)
                                                       for b in range(d.n_u)]
            Ks.append([gm * v for v in d.fmp(ys, u)])
            mags += abs(B[s]) * d.fmag(ys, u)
        ynew = [y[a] + hm * sum(mp.mpf(B[i]) * Ks[i][a] for i in range(6) if B[i] != 0.0) for a in range(d.n_y)]
        M = np.array([abs(float(v)) for v in y]).reshape(d.n_y) + abs(h * g) * mags
        return ynew, M

    def _extend(self, j0, m, upto):
        d = self.d
        ch = self._chain.setdefault((j0, m), dict(y=[[mp.mpf(float(v)) for v in d.node_y[:, j0]]], M=[np.zeros(d.n_y)]))
        with mp.workdps(DPS):
            while len(ch["y"]) - 1 < upto - j0:
                j = j0 + len(ch["y"]) - 1
                _, sl, ca, cb, g = d.interval(j)
                y, M = ch["y"][-1], ch["M"][-1].copy()
                h = (cb - ca) / float(m)
                for q in range(m):
                    c = ca + float(q) * h
                    y, Ms = self._step(y, sl, c, cb - c if q == m - 1 else h, g)
                    M = np.maximum(M, Ms)
                ch["y"].append(y)
                ch["M"].append(M)
        return ch

    def arrivals(self, seg, m):
        d = self.d
        y, steps, M = np.zeros((d.n_y, d.N)), np.zeros(d.N), np.zeros((d.n_y, d.N))
        y[:, 0] = d.node_y[:, 0]
        for i in range(len(seg) - 1):
            j0, j1 = int(seg[i]), int(seg[i + 1])
            ch = self._extend(j0, m, j1)
            for j in range(j0 + 1, j1 + 1):
                y[:, j] = [float(v) for v in ch["y"][j - j0]]
                steps[j] = m * (j - j0)
                M[:, j] = ch["M"][j - j0]
        return y, steps, M


def parity_bound(ref, steps, M):
    """1e-10 |ref| + 64 eps n M, entry by entry"""
    return 1e-10 * np.abs(ref) + 64 * EPS * steps[None, :] * M


def segments(restart, s, N):
    """the segment lists of the tests: "nodes", "sections", "phase", "irregular" (restarts at nodes 0, 1, then roughly
    every 2.5 nodes, so segments start inside sections and straddle section boundaries)"""
    if restart == "nodes":
        return np.arange(N)
    if restart == "sections":
        return np.asarray(s, dtype=np.int64)
    if restart == "phase":
        return np.array([0, N - 1])
    if restart == "irregular":
        cut = sorted({0, 1, N - 1} | {int(v) for v in np.arange(3, N - 1, 2.5)})
        return np.array(cut)
    raise ValueError(restart)


# ---- the cases of the tests ------------------------------------------------------------------------------------------
def _final_time(prob, T):
    ph = prob.phases[0]
    ph.bounds.final_time = float(T)
    ph.guess.time = np.array([0.0, float(T)])
    return prob


def _ragged(prob, seed=3, K=23):
    """the ragged pattern of test_gpu_refinement.py / test_gpu_solution.py"""
    rng = np.random.default_rng(seed)
    ph = prob.phases[0]
    ph.mesh.number_mesh_sections = K
    ph.mesh.mesh_section_sizes = rng.uniform(0.3, 1.0, K)
    ph.mesh.number_mesh_section_nodes = rng.integers(3, 9, K)
    return prob


def _extremes():
    from pycollo_amd import problems
    prob = problems.hypersensitive(K=5, order=4)
    ph = prob.phases[0]
    ph.mesh.mesh_section_sizes = np.array([0.1, 0.3, 0.15, 0.25, 0.2])
    ph.mesh.number_mesh_section_nodes = np.array([2, 20, 3, 20, 2])
    return prob


def _radau():
    from pycollo_amd import problems
    prob = problems.hypersensitive(K=7, order=5)
    prob.quadrature_method = "radau"
    return prob


def _p():
    from pycollo_amd import problems
    return problems


# the meshes of test_gpu_solution.py's CASES, and a phase without controls.  The hypersensitive phases last HYPER_T =
# 0.02 time units, not 10 000 and not 10: the smooth test point is drawn in scaled variables and the state's scale is
# 100, so |y| reaches 15 and df/dy = -3 y^2 reaches -675.  With a final time of 10 one step of the 21-node mesh has
# h |df/dy| ~ 450, far outside the method's stability region: the fixed mode overflows (checked on the CPU), and no
# rounding bound without a growth factor holds over such a segment.  At 0.02 the longest node interval of these meshes
# (0.004 time units, the two-node sections of the order-extremes mesh) has h |df/dy| < 3.
HYPER_T = 0.02
CASES = {
    "hypersensitive_K5_n4": lambda: _final_time(_p().hypersensitive(K=5, order=4), HYPER_T),
    "cart_pole_ragged_K23": lambda: _ragged(_p().cart_pole(K=10, order=4)),
    "cart_pole_ragged_K60": lambda: _ragged(_p().cart_pole(K=10, order=4), K=60),
    "order_extremes_2_and_20": lambda: _final_time(_extremes(), HYPER_T),
    "two_phase_transfer_K6": lambda: _p().two_phase_transfer(K=6, order=4),
    "time_coupled_transfer_K6": lambda: _p().time_coupled_transfer(K=6, order=4),
    "hypersensitive_radau_K7_n5": lambda: _final_time(_radau(), HYPER_T),
    "hypersensitive_no_control": lambda: _final_time(_p().hypersensitive(K=5, order=4, fixed_control=0.0), HYPER_T),
}


def smooth_x_oracle(ora):
    """the smooth random point of test_gpu_solution.py (``_smooth_x``), from the oracle's own offsets"""
    rng = np.random.default_rng(5)
    x = np.zeros(ora.num_x)
    for P in ora.P:
        for b in range(P.n_z):
            cf = rng.uniform(-0.15, 0.15, 4)
            x[P.x_off + b * P.N:P.x_off + (b + 1) * P.N] = np.polynomial.polynomial.polyval(P.mesh.tau, cf)
        x[P.q_off:P.q_off + P.n_q + P.n_t] = rng.uniform(0.1, 0.3, P.n_q + P.n_t)
    x[ora.s_off:] = rng.uniform(-0.2, 0.2, ora.n_s)
    return x


# ---- the adaptive mode's bound ---------------------------------------------------------------------------------------
def lipschitz(d, y_nodes):
    """L >= 0: the largest one-sided Lipschitz constant of f in y (the largest eigenvalue of the symmetric part of
    df/dy, per unit time) over the nodes, at the states ``y_nodes`` [n_y][N] and the interpolated node controls"""
    L = 0.0
    for j in range(d.N):
        jj = min(j, d.N - 2)
        _, sl, ca, cb, _ = d.interval(jj)
        u = [legendre_f64(d.coef_u[b, sl], ca if j == jj else cb) for b in range(d.n_u)]
        J = d.jac_y(y_nodes[:, j], u)
        L = max(L, float(np.max(np.linalg.eigvalsh(0.5 * (J + J.T)))))
    return L


def adaptive_bound(d, seg, truth, accepted, atol, rtol, L):
    """a (atol_a + rtol max |y_a|) exp(L T) per entry [n_y][N]: a the accepted steps in the segment up to the node,
    max |y_a| over the truth from the segment's start to the node, T the time from the segment's start to the node --
    the textbook global bound of error-per-step control"""
    b = np.zeros((d.n_y, d.N))
    for i in range(len(seg) - 1):
        j0, j1 = int(seg[i]), int(seg[i + 1])
        for j in range(j0 + 1, j1 + 1):
            a = float(np.sum(accepted[j0 + 1:j + 1]))
            ymax = np.max(np.abs(np.concatenate([d.node_y[:, [j0]], truth[:, j0 + 1:j + 1]], axis=1)), axis=1)
            T = abs(d.stretch * (d.tau[j] - d.tau[j0]))
            b[:, j] = a * (atol + rtol * ymax) * np.exp(L * T)
    return b


# ---- sliding mass: the exact solution under a polynomial control ----------------------------------------------------
def _leg_monomials(n):
    """monomial coefficients (ascending) of P_0 .. P_{n-1}, mpmath"""
    P = [[mp.mpf(1)], [mp.mpf(0), mp.mpf(1)]]
    for m in range(1, n):
        a = [mp.mpf(0)] + [(2 * m + 1) * v for v in P[m]]
        b = P[m - 1] + [mp.mpf(0)] * (len(a) - len(P[m - 1]))
        P.append([(x - m * y) / (m + 1) for x, y in zip(a, b)])
    return P[:n]


def _integrate_from_minus_one(p):
    """monomial coefficients of int_{-1}^{c} p"""
    q = [mp.mpf(0)] + [v / (i + 1) for i, v in enumerate(p)]
    q[0] = -sum(v * (-1) ** i for i, v in enumerate(q))
    return q


def _polyval(p, c):
    return sum(v * c ** i for i, v in enumerate(p))


def sliding_mass_exact(d):
    """x' = v, v' = f with f the section's control polynomial: the exact (x, v) [2][N] arriving at every node from its
    section's first node (for a section's first node: from the previous section's), 60 digits, rounded once.  Column 0
    is the node value."""
    out = np.zeros((2, d.N))
    out[:, 0] = d.node_y[:, 0]
    with mp.workdps(DPS):
        for k in range(d.K):
            sk, n = int(d.s[k]), int(d.s[k + 1] - d.s[k] + 1)
            g = mp.mpf(d.interval(sk)[4])
            mono = _leg_monomials(n)
            cf = [mp.mpf(float(v)) for v in d.coef_u[0, sk + k:sk + k + n]]
            u = [sum(cf[m] * (mono[m][i] if i < len(mono[m]) else 0) for m in range(n)) for i in range(n)]
            x0, v0 = (mp.mpf(float(v)) for v in d.node_y[:, sk])
            vel = _integrate_from_minus_one(u)                              # v = v0 + g int u
            vel = [v0 + g * vel[0]] + [g * v for v in vel[1:]]
            pos = _integrate_from_minus_one(vel)                            # x = x0 + g int v
            pos = [x0 + g * pos[0]] + [g * v for v in pos[1:]]
            for j in range(sk, int(d.s[k + 1])):
                c = mp.mpf(d.interval(j)[3])
                out[0, j + 1], out[1, j + 1] = float(_polyval(pos, c)), float(_polyval(vel, c))
    return out


# ---- the end-to-end figures on the CPU --------------------------------------------------------------------------------
class _OracleProblem:
    """the cyipopt protocol over the oracle (host arrays)"""

    def __init__(self, ora):
        import scipy.sparse as sp
        self.ora, self.n, self.m = ora, ora.num_x, ora.num_c
        self._sp = sp

    def objective(self, x):
        return float(self.ora.J(x))

    def gradient(self, x):
        return np.asarray(self.ora.grad_J(x), dtype=float)

    def constraints(self, x):
        return np.asarray(self.ora.c(x), dtype=float)

    def jacobian(self, x):
        return np.asarray(self.ora.G(x), dtype=float)

    def jacobianstructure(self):
        return self.ora.G_structure()

    def hessian(self, x, lagrange, obj_factor):
        return np.asarray(self.ora.H(x, obj_factor, lagrange), dtype=float)

    def hessianstructure(self):
        return self.ora.H_structure()

    def intermediate(self, *a):
        pass


def cpu_solve(prob, tables, tol=1e-10):
    """Solve the NLP of ``prob`` on the host: the oracle's functions, the host ``InteriorPointSolver``, the user guess
    interpolated linearly.  Returns (oracle, x~)."""
    from oracle.ref_numpy import OracleNlp, _bnds, _pair, _same
    from pycollo_amd.ipm import InteriorPointSolver
    ora = OracleNlp(prob, tables)
    V, r = ora.V_ocp, ora.r_ocp
    x0 = np.zeros(ora.num_x)
    xl, xu = np.zeros(ora.num_x), np.zeros(ora.num_x)
    for ph, P in zip(prob.phases, ora.P):
        ys, us = list(ph.state_variables), list(ph.control_variables)
        y_b, u_b = _bnds(ys, ph.bounds.state_variables), _bnds(us, ph.bounds.control_variables)
        q_b = _bnds(list(ph.integral_variables), ph.bounds.integral_variables)
        t_b = [_pair(ph.bounds.initial_time), _pair(ph.bounds.final_time)]
        time = np.asarray(ph.guess.time, dtype=float)
        tg = (time - 0.5 * (time[0] + time[-1])) / (0.5 * (time[-1] - time[0]))
        yg = np.asarray(ph.guess.state_variables, dtype=float).reshape(len(ys), -1)
        ug = np.asarray(ph.guess.control_variables, dtype=float).reshape(len(us), -1)

        def ends(spec, i, b):
            if spec is None:
                return b
            if isinstance(spec, dict):
                return _pair(spec[ys[i]]) if ys[i] in spec else b
            return _pair(list(spec)[i])
        rows = [(yg[i], b, ends(ph.bounds.initial_state_constraints, i, b), ends(ph.bounds.final_state_constraints, i, b))
                for i, b in enumerate(y_b) if not _same(*b)]
        rows += [(ug[i], b, b, b) for i, b in enumerate(u_b) if not _same(*b)]
        for j, (g, b, b0, bF) in enumerate(rows):
            sl = slice(P.x_off + j * P.N, P.x_off + (j + 1) * P.N)
            sc, sh = V[P.ox + j], r[P.ox + j]
            x0[sl] = (np.interp(P.mesh.tau, tg, g) - sh) / sc
            xl[sl], xu[sl] = (b[0] - sh) / sc, (b[1] - sh) / sc
            xl[sl.start], xu[sl.start] = (b0[0] - sh) / sc, (b0[1] - sh) / sc
            xl[sl.stop - 1], xu[sl.stop - 1] = (bF[0] - sh) / sc, (bF[1] - sh) / sc
        rest = [(g, b) for g, b in zip(np.atleast_1d(ph.guess.integral_variables if ph.guess.integral_variables is not None else []), q_b)
                if not _same(*b)]
        rest += [(g, b) for g, b in zip((time[0], time[-1]), t_b) if not _same(*b)]
        for j, (g, b) in enumerate(rest):
            col, o = P.q_off + j, P.ox + P.n_z + j
            x0[col], xl[col], xu[col] = (g - r[o]) / V[o], (b[0] - r[o]) / V[o], (b[1] - r[o]) / V[o]
    assert ora.n_s == 0 and ora.n_b == 0 and all(P.n_p == 0 for P in ora.P), "cpu_solve: only defect and integral rows"
    zero = np.zeros(ora.num_c)
    pobj = _OracleProblem(ora)
    res = InteriorPointSolver(pobj, pobj.n, pobj.m, xl, xu, zero, zero, tol=tol, max_iter=500).solve(np.clip(x0, xl, xu))
    assert res.success, res.status
    return ora, np.asarray(res.x, dtype=float)
