"""Test points of the ph mesh-error estimate (row N2), shared by tests/test_refinement_cpu.py (float64 restatements
against the exact reference, no GPU) and tests/test_gpu_refinement.py (the kernel against the same reference).

A point lies ON A TRAJECTORY of its model, without a solve: smooth scaled controls (a constant plus two low-frequency
sinusoids), a drawn initial state, q, free times and static parameters, and the states integrated through
``y' = stretch f`` over tau in [-1, 1] (DOP853, rtol 1e-13) at the mesh's nodes.  There the estimate is what it is at
an NLP solution -- the small difference of two O(|y|) numbers -- and the section widths of every case are chosen so
that its estimates straddle the 1e-7 tolerance the refinement decision is taken at."""
import numpy as np

from conftest import entry_err, golden_tables
from oracle.ref_numpy import OracleNlp
from oracle.ref_refine import mesh_error as oracle_mesh_error
from oracle.ref_refine import mesh_error_mp
from pycollo_amd import problems

ULPS = 32          # the smallest power of two that leaves the float64 restatements a factor 4
TOL = 1e-7         # refinement.MESH_TOLERANCE
TB = 256           # lanes of a mesh-error tile (pc_mesh_error)


def tile_lanes(nodes):
    """Lanes used by every tile, by the host code's greedy rule: section k occupies n_k + 1 lanes of a 256-lane tile,
    a section that does not fit opens the next tile.  Returns (lanes used per tile, first section of every tile)."""
    used, first, lanes = [], [0], 0
    for k, n in enumerate(nodes):
        if lanes + int(n) + 1 > TB:
            used.append(lanes)
            first.append(k)
            lanes = 0
        lanes += int(n) + 1
    used.append(lanes)
    return used, first


def lds_bytes(nodes, n_y, n_u):
    """Dynamic LDS of one call, by the host code's formula (tables of the orders in use + the per-lane arrays)."""
    orders = sorted({int(n) for n in nodes})
    be = sum((n - 1) * n for n in orders)
    a = sum(n * (n + 1) for n in orders)
    return 8 * (2 * be + a + TB * (5 * n_y + max(1, n_u) + 1)) + 1024


def _set_mesh(prob, meshes):
    for ph, (sizes, nodes) in zip(prob.phases, meshes):
        sizes = np.asarray(sizes, float)
        ph.mesh.number_mesh_sections = len(nodes)
        ph.mesh.mesh_section_sizes = sizes / sizes.sum()
        ph.mesh.number_mesh_section_nodes = np.asarray(nodes, dtype=np.int64)
    return prob


# width of a cart-pole section of order n relative to its neighbours: a section's estimate falls like (h / ell)^n, so
# equal widths would put the high orders many decades below the rounding of the estimate's own terms.  Found by
# iterating the float64 oracle's estimates of every order towards 1e-7; the draw around them makes the case straddle it.
RAGGED_WIDTH = {2: 1.0, 3: 8.848, 4: 20.83, 5: 38.48, 6: 51.58, 7: 71.89, 8: 86.86, 9: 98.64, 10: 121.9}


def _widths(nodes, rng, spread=0.1):
    return np.array([RAGGED_WIDTH[int(n)] for n in nodes]) * rng.uniform(1.0 - spread, 1.0 + spread, len(nodes))


def _ragged_multitile():
    """cart-pole, K = 120, orders 2..10 from a seeded draw, then adjusted by hand (the lane counts are asserted by
    test_ragged_case_fills_and_closes_tiles_as_intended in tests/test_refinement_cpu.py):
    tile 0 ends with exactly 256 lanes used, tile 1 is closed with >= 5 lanes free because the next section has order 10."""
    rng = np.random.default_rng(11)
    nodes = rng.integers(2, 11, 120)
    used, first = tile_lanes(nodes)
    # tile 0: trim / pad its last sections so that it holds exactly 256 lanes
    k1 = first[1]
    nodes[k1 - 1] += TB - used[0]
    assert 2 <= nodes[k1 - 1] <= 10
    # tile 1: its last section shrinks until >= 5 lanes stay free, and the section after it has order 10
    used, first = tile_lanes(nodes)
    k2 = first[2]
    nodes[k2] = 10
    while True:
        used, first = tile_lanes(nodes)
        free = TB - used[1]
        if first[2] == k2 and 5 <= free < 11:
            break
        nodes[k2 - 1] = nodes[k2 - 1] + (1 if free >= 11 else -1)
        assert 2 <= nodes[k2 - 1] <= 10
    return nodes


CASES = {}


def _case(name, build, *, seed, engine_kw=None, sharp=True, freq=(1.0, 2.3), times=None, amp=0.08, start="draw",
          ctrl0=None, paths=()):
    """Register a case.  ``build``: the problem with its mesh; ``seed``: of every draw of the point; ``engine_kw``: for
    NlpEngine; ``sharp``: the bound must be <= 1e-3 of every section's estimate.  The trajectory (trajectory_point):
    ``freq``: the two control frequencies (rad per unit tau); ``amp``: the largest scaled amplitude of either;
    ``ctrl0``: the scaled constant of every control instead of a draw; ``times``: scaled free times instead of a draw;
    ``start``: "draw" -- scaled initial states from (-0.2, 0.2); "guess" -- the problem's initial guess, each state up
    to 1 % (and 1e-4 of its range) larger; "chain" -- as "guess" in the first phase, the others continue it.
    ``paths``: kernel paths the case exists for, asserted on the oracle's model when the point is built:
    "no_control" (n_u = 0 in every phase), "free_t0" (some phase has a free initial time)."""
    CASES[name] = dict(build=build, seed=seed, engine_kw=engine_kw or {}, sharp=sharp, freq=freq, times=times, amp=amp, start=start, ctrl0=ctrl0,
                       paths=tuple(paths))


def _cart_ragged():
    nodes = _ragged_multitile()
    return _set_mesh(problems.cart_pole(), [(_widths(nodes, np.random.default_rng(12)), nodes)])


def _hyper_high(lo, hi, seed):
    def build():
        rng = np.random.default_rng(seed)
        nodes = rng.integers(lo, hi + 1, 30)
        nodes[:hi - lo + 1] = np.arange(lo, hi + 1)          # every order of the range is present
        return _set_mesh(problems.hypersensitive(test_fixture_bounds=True), [(rng.uniform(0.5, 1.0, 30), nodes)])
    return build


def _uniform(n):
    """K = 3 sections of one order, widths 1 : g : g^2 with g^n = 10^1.2: the estimates span two to three decades."""
    g = 10.0 ** (1.2 / n)
    return lambda: _set_mesh(problems.brachistochrone(K=3, order=n), [([1.0, g, g * g], [n] * 3)])


_case("ragged_multitile", _cart_ragged, seed=21, freq=(100.0, 230.0), amp=0.3)
_case("high_orders_11_15", _hyper_high(11, 15, 31), seed=32, sharp=False, ctrl0=-0.37, amp=0.008)
_case("high_orders_16_19", _hyper_high(16, 19, 33), seed=34, sharp=False, ctrl0=-0.37, amp=0.008)
# control frequencies that put the middle section of the order's case at 1e-7 (bisection on the float64 oracle's estimates).
# Orders 16..19 cannot get there: whatever the controls, their estimates stay at 2e-7..1e-5 on this mesh.
UNIFORM_FREQ = {2: (0.02, 0.038), 3: (0.099, 0.188), 4: (0.158, 0.301), 5: (0.304, 0.578), 6: (1.061, 2.016),
                7: (1.732, 3.29), 8: (1.283, 2.437), 9: (2.414, 4.587), 10: (2.618, 4.974), 11: (3.81, 7.24),
                12: (3.7, 7.03), 13: (3.818, 7.254), 14: (4.748, 9.021), 15: (4.875, 9.262)}
for _n in range(2, 20):
    _case(f"uniform_n{_n}", _uniform(_n), seed=40 + _n, engine_kw=dict(specialise=False),
          freq=UNIFORM_FREQ.get(_n, (0.5, 0.95)), times=[-0.46] if _n < 4 else None)


def _ragged_small(make, orders, grade=1.0):
    """Every phase on sections of the given orders, widths proportional to order^grade."""
    def build():
        prob = make()
        return _set_mesh(prob, [(np.asarray(orders, float) ** grade, orders) for _ in prob.phases])
    return build


_case("time_coupled_transfer", _ragged_small(problems.time_coupled_transfer, [5, 6, 7, 8]), seed=51, freq=(2.403, 5.408),
      engine_kw=dict(specialise=False), paths=("free_t0",))
_case("sliding_mass", _ragged_small(lambda: problems.sliding_mass(num_phases=2), [5, 6, 7, 8]), seed=52, freq=(3.673, 8.265),
      engine_kw=dict(specialise=False), paths=("free_t0",))
_case("double_pendulum", _ragged_small(problems.double_pendulum, [5, 6, 7, 8, 6, 7, 8, 7]), seed=53, freq=(3.0, 7.0),
      engine_kw=dict(specialise=False), start="guess", times=[-0.5])


def _no_control():
    """y' = -5000 y^3 decays like (tau + 1)^(-1/2) and never settles: sections growing geometrically away from the
    start keep h / (tau + 1), and with it the estimate, of one size along the whole phase."""
    rng = np.random.default_rng(57)
    return _set_mesh(problems.hypersensitive(fixed_control=0.0), [(NO_CONTROL_GROWTH ** np.arange(24) * rng.uniform(0.7, 1.3, 24),
                                                                   [6] * 24)])


NO_CONTROL_GROWTH = 1.35
_case("no_control", _no_control, seed=54, engine_kw=dict(specialise=False), paths=("no_control",))
_case("single_section", lambda: problems.brachistochrone(K=1, order=7), seed=55, engine_kw=dict(specialise=False),
      freq=(4.0, 9.0))
_case("delta_iii", lambda: problems.delta_iii(K=4, order=4), seed=56, start="chain", ctrl0=0.3)


class Point:
    """A case's problem, scaling, oracle and x~ (built once per session)."""

    def __init__(self, name, engine):
        spec = CASES[name]
        self.name, self.spec = name, spec
        self.prob = spec["build"]()
        self.V, self.r, self.W = np.array(engine.V_ocp), np.array(engine.r_ocp), np.array(engine.W_ocp)
        self.ora = OracleNlp(self.prob, golden_tables("lobatto"), V_ocp=self.V, r_ocp=self.r, W_ocp=self.W)
        if "no_control" in spec["paths"]:       # the kernel's NU > 0 ? NU : 1 path
            assert all(P.n_u == 0 for P in self.ora.P), f"{name}: a control is left in the model"
        if "free_t0" in spec["paths"]:          # the kernel's T0_FREE path
            assert any(P.t_free[0] for P in self.ora.P), f"{name}: no phase has a free initial time"
        self.x = trajectory_point(self.ora, spec["seed"], spec["freq"], spec["times"], spec["amp"], spec["start"], spec["ctrl0"])
        self._mp = None

    @property
    def ref(self):
        if self._mp is None:
            self._mp = mesh_error_mp(self.ora, self.x)
        return self._mp


_POINTS = {}


def point(name, engine=None):
    """The case's test point; the scaling comes from ``engine`` (a structure-only engine is built when none is given:
    V, r, W depend on the problem alone)."""
    if name not in _POINTS:
        if engine is None:
            from pycollo_amd.engine import NlpEngine
            engine = NlpEngine(CASES[name]["build"](), device=None, **CASES[name]["engine_kw"])
        _POINTS[name] = Point(name, engine)
    return _POINTS[name]


_RHS_CACHE = {}


def _scalar_f(P):
    """The oracle's state equations as one scalar callable (the integrator calls it a million times on the stiff
    models; the oracle's vectorised F_fn cost ten times as much per call)."""
    import sympy as sym
    if P.key not in _RHS_CACHE:
        fn = sym.lambdify(list(P.v) + list(P.consts), list(P.f), modules="math", cse=True)
        cv = [float(v) for v in P.consts.values()]
        _RHS_CACHE[P.key] = lambda *a: fn(*a, *cv)
    return _RHS_CACHE[P.key]


def trajectory_point(ora, seed, freq=(1.0, 2.3), times=None, amp_max=0.08, start="draw", ctrl0=None):
    """x~ on a trajectory of every phase (module docstring).  The integration stops at every mesh node: the dense
    output that ``t_eval`` reads is of lower order than the steps and leaves a 1e-7 roughness at the nodes, which
    sections of order 16 and more resolve -- their estimates then sit on that floor whatever the mesh."""
    from scipy.integrate import solve_ivp
    rng = np.random.default_rng(seed)
    V, r = ora.V_ocp, ora.r_ocp
    x = np.zeros(ora.num_x)
    x[ora.s_off:] = rng.uniform(-0.2, 0.2, ora.n_s)
    for P, ph in zip(ora.P, ora.prob.phases):
        N, n_y, n_u, n_z = P.N, P.n_y, P.n_u, P.n_z
        x[P.q_off:P.t_off] = rng.uniform(-0.2, 0.2, P.n_q)
        x[P.t_off:P.t_off + P.n_t] = np.sort(rng.uniform(-0.2, 0.2, P.n_t))
        if times is not None:
            x[P.t_off:P.t_off + P.n_t] = times[:P.n_t]
        c0 = rng.uniform(-0.15, 0.15, n_u)
        if ctrl0 is not None:
            c0 = np.full(n_u, float(ctrl0))
        amp = amp_max * rng.uniform(0.4, 1.0, (2, n_u))
        om = np.array(freq)[:, None] * rng.uniform(0.8, 1.2, (2, n_u))
        phi = rng.uniform(0, 2 * np.pi, (2, n_u))
        ut = lambda tau: c0 + np.sum(amp * np.sin(om * tau + phi), axis=0)            # scaled controls at one tau
        Vy, ry = V[P.ox:P.ox + n_y], r[P.ox:P.ox + n_y]
        Vu, ru = V[P.ox + n_y:P.ox + n_z], r[P.ox + n_y:P.ox + n_z]
        y0 = Vy * rng.uniform(-0.2, 0.2, n_y) + ry
        if start == "chain" and P is not ora.P[0]:
            # a later phase goes on where the previous one ended, except in the states its own guess starts
            # differently (Delta III: the mass after a stage is dropped)
            g0 = np.asarray(ora.prob.phases[0].guess.state_variables, float)[:, 0]
            g = np.asarray(ph.guess.state_variables, float)[:, 0]
            y0 = np.where(g != g0, g, ys[:, -1])
        elif start in ("guess", "chain"):
            assert n_y == len(ph.state_variables)
            # (a little off the guess itself: models have kinks there, Delta III's sqrt of a relative velocity of 0)
            y0 = np.asarray(ph.guess.state_variables, float)[:, 0] * (1.0 + rng.uniform(0.0, 0.01, n_y)) \
                + Vy * rng.uniform(0.0, 1e-4, n_y)
        _, _, stretch, _, w = ora._unpack(P, x)
        f = _scalar_f(P)

        def rhs(tau, y):
            return stretch * np.array(f(*y, *(Vu * ut(tau) + ru), *w), float)
        tau = P.mesh.tau
        ys = np.empty((n_y, N))
        ys[:, 0] = y0
        for i in range(1, N):
            sol = solve_ivp(rhs, (tau[i - 1], tau[i]), ys[:, i - 1], method="DOP853", rtol=1e-13, atol=1e-14)
            assert sol.success
            ys[:, i] = sol.y[:, -1]
        yt = (ys - ry[:, None]) / Vy[:, None]
        utn = np.array([ut(t) for t in tau]).reshape(N, n_u).T
        x[P.x_off:P.q_off] = np.vstack([yt, utn]).ravel()
    return x


def table_form(ora, xt, quad):
    """NumPy restatement of the kernel's table form (pc::mesh_error): y_ph = y_start + stretch (h (B f)), u_ph = E u,
    Y_ph = y_start + stretch (h (A f_ph)) with the product's own ``ph_tables``; (max_rel [K], max_abs [K][n_y]) per phase."""
    from pycollo_amd.refinement import ph_tables
    out = []
    for P in ora.P:
        mesh = P.mesh
        z, _, stretch, _, w = ora._unpack(P, np.asarray(xt, float))
        n_y, n_z, K = P.n_y, P.n_z, mesh.K
        f = np.array([P.F_fn[i](*ora._args(P, z, w)) for i in range(n_y)]).reshape(n_y, P.N)
        rel, ab = np.zeros(K), np.zeros((K, n_y))
        for k in range(K):
            n, i0, h = int(mesh.nodes[k]), int(mesh.bnd[k]), mesh.h[k]
            B, E, A = ph_tables(quad, n)
            zp = np.zeros((n_z, n + 1))
            zp[:, 0], zp[:, n] = z[:, i0], z[:, i0 + n - 1]
            zp[:n_y, 1:n] = z[:n_y, i0][:, None] + stretch * (h * (f[:, i0:i0 + n] @ B.T))
            zp[n_y:, 1:n] = z[n_y:, i0:i0 + n] @ E.T
            ap = [zp[b] for b in range(n_z)] + [np.full(n + 1, w[i]) for i in range(P.n_w)]
            fp = np.array([P.F_fn[i](*ap) for i in range(n_y)]).reshape(n_y, n + 1)
            Y = zp[:n_y, 0][:, None] + stretch * (h * (fp @ A.T))
            err = np.abs(Y - zp[:n_y, 1:])
            ab[k] = np.max(err, axis=1)
            rel[k] = np.max(err / (1.0 + (np.max(np.abs(zp[:n_y, 1:]), axis=1) + 1.0))[:, None])
        out.append((rel, ab))
    return out


def oracle_maxima(ora, xt):
    """(max_rel [K], max_abs [K][n_y]) per phase of the float64 oracle (oracle.ref_refine.mesh_error)."""
    return [(rel, ab.max(axis=2)) for ab, rel in oracle_mesh_error(ora, xt)]


def ratios(got, ref, ulps=ULPS):
    """Per phase the entry_err ratio (<= 1 passes) of max_rel per section and of max_abs per section AND state against
    the exact reference, no entry skipped."""
    out = []
    for (rel, ab), R in zip(got, ref):
        out.append((entry_err(rel, R["max_rel"], R["mag_max_rel"], ulps=ulps, expect_unscaled=0),
                    entry_err(ab, R["max_abs"], R["mag_max_abs"], ulps=ulps, expect_unscaled=0)))
    return out


def sharpness(ref, ulps=ULPS):
    """Per phase and section: the bound on max_rel as a fraction of the reference estimate (from the reference alone)."""
    eps = np.finfo(float).eps
    return [(1e-10 * R["max_rel"] + ulps * eps * R["mag_max_rel"]) / R["max_rel"] for R in ref]


# ------------------------------------------------------------------------------------------------------------------
# the points of the first parity test of this row: a random cubic in tau per variable, which is no trajectory -- the
# estimates are O(1) (cart-pole) to 1e14 (hypersensitive).  Kept for their shapes (K = 300 uniform, the shuttle, two
# phases) and held to the same entry-wise tolerance.
CUBIC_CASES = [("hypersensitive", dict(K=40, order=5), False), ("cart_pole", dict(K=300, order=4), False),
               ("shuttle", dict(K=12, order=6), False), ("two_phase_transfer", dict(K=6, order=4), False),
               ("time_coupled_transfer", dict(K=6, order=4), False), ("cart_pole", dict(K=10, order=4), True),
               ("double_pendulum", dict(K=10, order=4), True)]


def cubic_problem(name, kw, ragged):
    prob = problems.REGISTRY[name](**kw)
    if ragged:
        rng = np.random.default_rng(3)
        ph = prob.phases[0]
        ph.mesh.number_mesh_sections = 23
        ph.mesh.mesh_section_sizes = rng.uniform(0.3, 1.0, 23)
        ph.mesh.number_mesh_section_nodes = rng.integers(3, 9, 23)
    return prob


def cubic_point(eng):
    rng = np.random.default_rng(5)
    x = np.zeros(eng.num_x)
    for pl, mesh in zip(eng.layout.phases, eng.meshes):
        for b in range(pl.n_z):
            cf = rng.uniform(-0.15, 0.15, 4)
            x[pl.x_off + b * pl.N:pl.x_off + (b + 1) * pl.N] = np.polynomial.polynomial.polyval(mesh.tau, cf)
        x[pl.q_off:pl.q_off + pl.n_q + pl.n_t] = rng.uniform(0.1, 0.3, pl.n_q + pl.n_t)
    x[eng.layout.s_off:] = rng.uniform(-0.2, 0.2, eng.layout.n_s)
    return x


_CUBIC = {}


def cubic(i, engine=None):
    """(oracle, x~, exact reference) of CUBIC_CASES[i]."""
    if i not in _CUBIC:
        name, kw, ragged = CUBIC_CASES[i]
        prob = cubic_problem(name, kw, ragged)
        if engine is None:
            from pycollo_amd.engine import NlpEngine
            engine = NlpEngine(prob, device=None)
        ora = OracleNlp(prob, golden_tables("lobatto"), V_ocp=engine.V_ocp, r_ocp=engine.r_ocp, W_ocp=engine.W_ocp)
        x = cubic_point(engine)
        _CUBIC[i] = (ora, x, mesh_error_mp(ora, x))
    return _CUBIC[i]


# cases whose estimates lie on both sides of the tolerance: the others cannot (orders 16..19: the reference's own
# A(n + 1) integrates a constant with an error of 5e-8..1e-5 there, which is the floor of the estimate; the single
# section has one estimate; Delta III's mesh is fixed at K = 4, n = 4 per phase and its phase times are fixed by the
# problem, and on any flown trajectory 19..175 s per order-4 section leave 1e-6..1e-4)
STRADDLING = ({"ragged_multitile", "high_orders_11_15", "high_orders_16_19", "time_coupled_transfer", "sliding_mass",
               "double_pendulum", "no_control"} | {f"uniform_n{n}" for n in range(2, 16)})


def assert_regime(name, ref, ulps=ULPS):
    """From the reference alone: the case's estimates straddle the tolerance (where the case is built to), and the
    bound is <= 1e-3 of every section's estimate (all cases but the ill-conditioned high-order ones)."""
    est = np.concatenate([R["max_rel"] for R in ref])
    if name in STRADDLING:
        assert np.any(est > TOL) and np.any(est < TOL), f"{name}: the estimates {est.min():.1e}..{est.max():.1e} do not straddle {TOL}"
    frac = np.concatenate(sharpness(ref, ulps))
    if CASES[name]["sharp"]:
        assert np.all(frac <= 1e-3), f"{name}: the bound is {frac.max():.1e} of a section's estimate"
    return est, frac
