"""Every ``pc_ipm_*`` call (pycollo_amd/csrc/pc_ipm.hpp) on its own against the reference statement of the step
(``StepRef``, tests/test_ipm_steps_ref.py), given the device's own inputs to that call: the state comes from
``pc_ipm_get_state``, the solved step from ``pc_ipm_get_step``, c~ / grad J / J^T lambda from ``OracleNlp`` at the same
point -- so the KKT solve's own error stays out of the vector-kernel checks (tests/test_gpu_kkt_conditions.py holds
the solve).  The bounds are the derived ones stated in test_ipm_steps_ref.py; the non-finite counter must be 0, two
``pc_ipm_errors`` calls in a row must return the same bits, and the exact statements (zero steps of fixed unknowns, zero
multipliers of unbounded ones, the Newton step back after ``pc_ipm_soc_restore``) are asserted as such."""
import numpy as np
import pytest

from conftest import entry_err, golden_tables, vec_err
from pycollo_amd import problems
from test_ipm_steps_ref import EPS, K_ENTRY, LD, StepRef, attained, static_of
from test_ipm_steps_ref import ratio as _ratio

_LARGEST = {}      # the largest ratio to a StepRef bound seen per call since the last report (printed under -s)
_CALL = ["set_state / eval_point"]


def ratio(got, ref, bound):
    r = _ratio(got, ref, bound)
    _LARGEST[_CALL[0]] = max(_LARGEST.get(_CALL[0], 0.0), r)
    return r


def _report(tag):
    print(f"{tag}: largest |got - ref| / bound per call: " + ", ".join(f"{k} {v:.3f}" for k, v in _LARGEST.items()))
    _LARGEST.clear()

pytestmark = pytest.mark.gpu


def _probe_class():
    from pycollo_amd.ipm import ResidentInteriorPointSolver

    class Probe(ResidentInteriorPointSolver):
        """The resident solver with its device state kept after ``solve`` returns (``close`` releases it)."""

        def _release(self):
            pass

        def close(self):
            ResidentInteriorPointSolver._release(self)

    return Probe


def _problem(name, kw):
    prob = problems.REGISTRY[name](**kw)
    if name == "two_phase_transfer":
        # (the registry's problem carries no guess: it is only ever evaluated at given points elsewhere) straight lines
        # between the pinned initial and final states, the linkage point halfway
        A, B = prob.phases
        A.guess.time, B.guess.time = np.array([0.0, 1.0]), np.array([1.0, 3.0])
        A.guess.state_variables, B.guess.state_variables = np.array([[0.0, 0.5], [0.0, 0.5]]), np.array([[0.5, 1.0], [0.5, 0.0]])
        A.guess.control_variables, B.guess.control_variables = np.array([[0.5, 0.5]]), np.array([[0.0, 0.0]])
        A.guess.integral_variables, B.guess.integral_variables = np.array([1.0]), np.array([2.0, 0.0])
        prob.guess.parameter_variables = np.array([1.0])
    return prob


class _Case:
    """A problem's mesh iteration, its oracle and a probe stopped at the pushed-interior start."""

    def __init__(self, name, kw, lower_free=False):
        from oracle.ref_numpy import OracleNlp
        from pycollo_amd.engine import PycolloGpuProblem
        from pycollo_amd.iteration import MeshIteration
        self.it = it = MeshIteration(_problem(name, kw), device=0)
        eng = it.engine
        self.ora = OracleNlp(it.problem, golden_tables(it.model.quadrature_method), V_ocp=eng.V_ocp, r_ocp=eng.r_ocp,
                             W_ocp=eng.W_ocp, w_J=eng.w_J)
        self.pobj = PycolloGpuProblem(eng)
        lb, cl = it.x_bnd_l, it.c_bnd_l
        if lower_free:
            lb, cl = np.full_like(lb, -np.inf), np.full_like(cl, -np.inf)
        self.bounds = (lb, it.x_bnd_u, cl, it.c_bnd_u)
        self.captured = []

    def capture(self, max_iter):
        """Every accepted iterate of a ``linear_solver="gpu"`` run, slacks included (IpmResult drops them)."""
        from pycollo_amd.ipm import GpuInteriorPointSolver
        g = GpuInteriorPointSolver(self.pobj, self.pobj.n, self.pobj.m, *self.bounds, tol=1e-8, max_iter=max_iter)
        accept = g._accept

        def _accept(alpha, a_z, mu):
            accept(alpha, a_z, mu)
            self.captured.append((g.st.v.copy(), g.st.lam.copy(), g.st.zl.copy(), g.st.zu.copy(), float(mu)))
        g._accept = _accept
        g.solve(self.it.guess_x_tilde)
        assert len(self.captured) >= 4
        self.scaling = (g.sf, g.sc.copy())

    def start(self):
        """(a): the probe after the start of ``solve`` (scaling, pushed-interior point, least-squares multipliers)."""
        self.probe = p = _probe_class()(self.pobj, self.pobj.n, self.pobj.m, *self.bounds, tol=1e-8, max_iter=0)
        res = p.solve(self.it.guess_x_tilde)
        assert res.iterations == 0
        self.it.engine.set_prefetch_jac(False)        # (G~ is consumed where it is produced, as inside solve)
        if self.captured:
            assert p.sf == self.scaling[0] and np.array_equal(p.sc, self.scaling[1])
        v, lam, zl, zu, _, _ = p._get_state()
        return (v, lam, zl, zu), p.mu_init

    def close(self):
        self.probe.close()
        self.it.engine.close()


def _near_converged(p, state, mu=1e-9):
    """(c): ``state`` with a few unknowns 1e-12 max(1, |bound|) from a bound and z on the central path there, one
    multiplier far below and one far above its central-path value (both arms of the clip in ipm_accept_kernel)."""
    v, lam, zl, zu = (a.copy() for a in state)
    L, U = np.nonzero(p.hasl)[0], np.nonzero(p.hasu)[0]
    assert len(L) + len(U) >= 4
    close_l = L[:: max(1, len(L) // 5)][:5]
    close_u = np.setdiff1d(U[:: max(1, len(U) // 5)][:5], close_l)
    for i in close_l:
        v[i] = p.vl[i] + 1e-12 * max(1.0, abs(p.vl[i]))
        zl[i] = mu / (v[i] - p.vl[i])
    for i in close_u:
        v[i] = p.vu[i] - 1e-12 * max(1.0, abs(p.vu[i]))
        zu[i] = mu / (p.vu[i] - v[i])
    # the two out-of-band multipliers: unknowns well inside their bounds
    far = [(i, "l", v[i] - p.vl[i]) for i in np.setdiff1d(L, close_l)] + [(i, "u", p.vu[i] - v[i]) for i in np.setdiff1d(U, close_u)]
    far.sort(key=lambda t: -t[2])
    (i0, s0, d0), (i1, s1, d1) = far[0], far[1]
    (zl if s0 == "l" else zu)[i0] = 1e-25 * mu / d0
    (zl if s1 == "l" else zu)[i1] = 1e15 * mu / d1
    return (v, lam, zl, zu), mu


def _jt_lambda(ora, p, x, lam):
    """J^T lambda over v = [x ; s] from the oracle's G~ in long double, and what entry_err's rule allows it: every entry
    of G~ its 64 eps mag, the product one rounding per term of the column in an order not stated."""
    rows, cols = ora.G_structure()
    G, Gm = np.asarray(ora.G(x), LD), np.asarray(ora.G_mag(x), LD)
    sc, lam = np.asarray(p.sc, LD), np.asarray(lam, LD)
    jtl, mag, cnt = np.zeros(p.nv, LD), np.zeros(p.nv, LD), np.zeros(p.nv)
    np.add.at(jtl, cols, sc[rows] * G * lam[rows])
    np.add.at(mag, cols, sc[rows] * Gm * np.abs(lam[rows]))
    np.add.at(cnt, cols, 1.0)
    if p.ns:
        jtl[p.n:] = -lam[p.ineq]
    return jtl, mag * (64 + cnt) / 64


def _c_oracle(ora, p, ref, v):
    """(c at v from the oracle's c~, the entry_err magnitude that goes with it)."""
    x = np.asarray(v[:p.n], float)
    c_ref, _ = ref.scaled_c(ora.c(x), v)
    _, mag = ref.scaled_c(ora.c_mag(x), v)
    return c_ref.astype(float), mag.astype(float)


def _scalar(got, ref, bound, what):
    assert np.isfinite(bound) or (np.isinf(ref) and got == ref), (what, "no bound", got, ref)
    assert ratio(got, ref, bound) <= 1.0, (what, got, ref, bound, ratio(got, ref, bound))


def _check_step(p, ref, step, out, mu, tau, what):
    """What ipm_step_kernel left (dv in sol, dzl, dzu) and returned, against the reference for the device's own sol."""
    sol, dzl, dzu = step[0], step[1], step[2]
    a_max, a_z = out
    (dv, _), (a, a_b), (b, b_b), sv, sb = ref.step(sol, mu, tau)
    assert np.all(sol[:p.nv][p.fixed] == 0.0) and np.all(dzl[p.fixed] == 0.0) and np.all(dzu[p.fixed] == 0.0), what
    assert np.all(dzl[~p.hasl] == 0.0) and np.all(dzu[~p.hasu] == 0.0), what
    assert sv[5] == 0.0, (what, "non-finite entries in the step")
    assert ratio(dzl, a, a_b) <= 1.0, (what, "dzl", ratio(dzl, a, a_b))
    assert ratio(dzu, b, b_b) <= 1.0, (what, "dzu", ratio(dzu, b, b_b))
    _scalar(a_max, sv[0], sb[0], what + " alpha_max")
    _scalar(a_z, *attained([sv[1], sv[2]], [sb[1], sb[2]], "min"), what + " alpha_z")
    if not p.hasl.any():
        assert sv[1] == 1.0 and sb[1] == 0.0          # no lower bounds: a_zl is the identity
    return sv, sb


def check_iteration(p, ora, state, mu, a_z_accept=None, expect_arms=False, tag=""):
    """One iteration's calls in order, each held to StepRef.  Returns nothing; asserts."""
    n, nv, m = p.n, p.nv, p.m
    tau = max(0.99, 1.0 - mu)
    _CALL[0] = "set_state / eval_point"
    # ---- pc_ipm_set_state / pc_ipm_eval_point -------------------------------------------------------------------
    p._set_state(*state)
    f, theta = p._eval_point()
    max_c = float(p._r3[2])
    v, lam, zl, zu, c, g = p._get_state()
    for got, sent in zip((v, lam, zl, zu), state):
        np.testing.assert_array_equal(got, sent)
    x = v[:n].copy()
    jtl, jtl_mag = _jt_lambda(ora, p, x, lam)
    ref = StepRef(static_of(p), v=v, lam=lam, zl=zl, zu=zu, JTlam=jtl, JTlam_mag=jtl_mag)
    c_ref, c_mag = _c_oracle(ora, p, ref, v)
    assert entry_err(c, c_ref, c_mag) <= 1.0, "scaled c differs from the oracle's"
    g_ref = ref.scaled_g(ora.grad_J(x)).astype(float)
    assert vec_err(g[:n], g_ref[:n]) <= 1.0 and np.all(g[n:] == 0.0), "g differs from the oracle's"
    assert abs(f - float(p.sf) * ora.J(x)) <= 1e-10 * abs(f) + 1e-290
    ref.c, ref.g = np.asarray(c, LD), np.asarray(g, LD)              # from here on: the device's own c and g
    (th, th_b), (mc, _) = ref.theta(c)
    _scalar(theta, th, th_b, "theta")
    assert max_c == mc
    _CALL[0] = 'errors'
    # ---- pc_ipm_errors (twice: the reduction counter is re-armed) ---------------------------------------------------
    e1 = p._errors()
    e2 = p._errors()
    assert e1.tobytes() == e2.tobytes(), ("pc_ipm_errors twice", e1, e2)
    val, bnd = ref.errors()
    for q in range(10):
        _scalar(e1[q], val[q], bnd[q], f"error scalar {q}")
    if not p.hasl.any():
        assert e1[3] == -np.inf and e1[4] == np.inf
    if not p.hasu.any():
        assert e1[5] == -np.inf and e1[6] == np.inf
    _CALL[0] = 'newton'
    # ---- pc_ipm_newton ----------------------------------------------------------------------------------------------
    dw, a_max, a_z, dphi, mub = p._newton(mu, tau, 0.0)
    assert dw >= 0.0 and p._r8[7] == 0.0
    newton = p._get_step()
    sol, dzl, dzu, rhs, _, dvec_true = newton
    (Sigma, Sigma_b), _, (rhs_ref, rhs_b) = ref.newton_setup(mu)
    assert ratio(rhs, rhs_ref, rhs_b) <= 1.0, ("rhs", ratio(rhs, rhs_ref, rhs_b))
    np.testing.assert_array_equal(rhs[nv:], -c)
    assert np.all(rhs[:nv][p.fixed] == 0.0)
    assert ratio(dvec_true[:nv], Sigma + LD(dw), Sigma_b + K_ENTRY * EPS * (np.abs(Sigma) + dw)) <= 1.0, "Sigma + dw"
    assert np.all(dvec_true[nv:] == 0.0)
    sv, sb = _check_step(p, ref, newton, (a_max, a_z), mu, tau, "newton")
    _scalar(dphi, sv[3], sb[3], "grad phi . dv")
    _scalar(mub, mu * sv[4], mu * sb[4] + EPS * abs(mu * sv[4]), "mu x barrier sum")
    _CALL[0] = 'trial'
    # ---- pc_ipm_trial -----------------------------------------------------------------------------------------------
    alpha = 0.5 * a_max

    def check_trial(a, dv):
        ft, th_t, mub_t = p._trial(a, mu)
        vt = p._get_step()[4]
        vt_ref, vt_b = ref.trial(a, dv)
        assert ratio(vt, vt_ref, vt_b) <= 1.0, ("trial point", ratio(vt, vt_ref, vt_b))
        bar, bar_b = ref.barrier(vt)
        _scalar(mub_t, mu * bar, mu * bar_b + EPS * abs(mu * bar), "mu x barrier sum at the trial point")
        assert abs(ft - float(p.sf) * ora.J(vt[:n])) <= 1e-10 * abs(ft) + 1e-290
        return vt, th_t

    vt, th_t = check_trial(alpha, sol[:nv])
    # c at the trial point, bit for bit: a correction with alpha = 0 has it as its right-hand side (0 c + ct), put back at once
    p._soc(0.0, True, mu, tau)
    ct = -p._get_step()[3][nv:]
    p._soc_restore(mu, tau)
    for got, kept in zip(p._get_step()[:4], newton[:4]):
        np.testing.assert_array_equal(got, kept)
    ct_ref, ct_mag = _c_oracle(ora, p, ref, vt)
    assert entry_err(ct, ct_ref, ct_mag) <= 1.0, "c at the trial point differs from the oracle's"
    _scalar(th_t, *ref.theta(ct)[0], "theta at the trial point")
    _CALL[0] = 'soc / soc_restore'
    # ---- pc_ipm_soc (first, then a further one), pc_ipm_soc_restore -------------------------------------------------------
    a1, az1, failed = p._soc(alpha, True, mu, tau)
    assert not failed
    soc1 = p._get_step()
    np.testing.assert_array_equal(soc1[3][:nv], rhs[:nv])
    cs, cs_b = ref.c_soc(alpha, c, ct)
    assert ratio(-soc1[3][nv:], cs, cs_b) <= 1.0, "c_soc (first)"
    _check_step(p, ref, soc1, (a1, az1), mu, tau, "first correction")
    a2, az2, failed = p._soc(a1, False, mu, tau)
    assert not failed
    soc2 = p._get_step()
    cs, cs_b = ref.c_soc(a1, -soc1[3][nv:], ct)
    assert ratio(-soc2[3][nv:], cs, cs_b) <= 1.0, "c_soc (second)"
    _check_step(p, ref, soc2, (a2, az2), mu, tau, "second correction")
    p._soc_restore(mu, tau)
    back = p._get_step()
    for got, kept, what in zip(back[:3], newton[:3], ("sol", "dzl", "dzu")):
        np.testing.assert_array_equal(got, kept, err_msg=what + " after pc_ipm_soc_restore")
    np.testing.assert_array_equal(back[3][nv:], rhs[nv:])
    _CALL[0] = 'trial / accept'
    # ---- pc_ipm_trial again, pc_ipm_accept ----------------------------------------------------------------------------
    vt, _ = check_trial(alpha, sol[:nv])
    a_z_use = a_z if a_z_accept is None else a_z_accept
    p._accept(alpha, a_z_use, mu)
    v2, lam2, zl2, zu2, c2, g2 = p._get_state()
    (_, _), (lam_r, lam_b), (zl_r, zl_b), (zu_r, zu_b), arms = ref.accept(alpha, a_z_use, mu, vt, sol, dzl, dzu)
    np.testing.assert_array_equal(v2, vt)
    assert ratio(lam2, lam_r, lam_b) <= 1.0, ("lambda", ratio(lam2, lam_r, lam_b))
    assert ratio(zl2, zl_r, zl_b) <= 1.0, ("zl", ratio(zl2, zl_r, zl_b))
    assert ratio(zu2, zu_r, zu_b) <= 1.0, ("zu", ratio(zu2, zu_r, zu_b))
    assert np.all(zl2[~p.hasl] == 0.0) and np.all(zu2[~p.hasu] == 0.0)
    if expect_arms:
        assert arms[0] >= 1 and arms[1] >= 1, ("both arms of the clip must be taken", arms)
    assert entry_err(c2, ct_ref, ct_mag) <= 1.0
    assert vec_err(g2[:n], ref.scaled_g(ora.grad_J(vt[:n])).astype(float)[:n]) <= 1.0 and np.all(g2[n:] == 0.0)
    _report(f"{tag} nu={p.nv + p.m} mu={mu:g}")


SMALL = [("brachistochrone", {}),                               # nu = 215: one workgroup, which is also the last one
         ("hypersensitive", dict(K=1, order=2)),                 # fewer unknowns than one wave
         ("free_flying_robot", dict(K=10, order=5)),             # bounds on both sides, fixed endpoints, path inequalities
         ("two_phase_transfer", {})]                             # endpoint rows, several phases


@pytest.mark.parametrize("name,kw", SMALL)
def test_every_call_at_start_mid_and_near_converged_iterates(built, name, kw):
    case = _Case(name, kw)
    try:
        case.capture(max_iter=300)
        start, mu0 = case.start()
        p = case.probe
        if name == "brachistochrone":
            assert p.nv + p.m <= 256
        if name == "hypersensitive":
            assert p.nv + p.m < 64
        if name == "free_flying_robot":
            assert p.ns > 0 and p.fixed.any() and (p.hasl & p.hasu).any()
        check_iteration(p, case.ora, start, mu0, tag=f"{name} (a)")
        half = case.captured[len(case.captured) // 2]
        check_iteration(p, case.ora, half[:4], half[4], tag=f"{name} (b)")
        near, mu = _near_converged(p, case.captured[-1][:4])
        check_iteration(p, case.ora, near, mu, a_z_accept=1e-16, expect_arms=True, tag=f"{name} (c)")
    finally:
        case.close()


def test_every_call_past_one_pass_of_the_grid(built):
    """hypersensitive K = 3300, order 6: n + ns = 33 003 and n + ns + m = 49 504 are both past 128 x 256 = 32 768, so the
    loops over the primal unknowns and those over all unknowns each take a second, ragged pass."""
    case = _Case("hypersensitive", dict(K=3300, order=6))
    try:
        case.capture(max_iter=40)
        start, mu0 = case.start()
        p = case.probe
        assert p.nv > 32768 and p.nv + p.m > 32768 and p.nv < 2 * 32768
        check_iteration(p, case.ora, start, mu0, tag="hypersensitive K=3300 (a)")
        near, mu = _near_converged(p, case.captured[-1][:4])
        check_iteration(p, case.ora, near, mu, a_z_accept=1e-16, expect_arms=True, tag="hypersensitive K=3300 (c)")
    finally:
        case.close()


def test_every_call_without_lower_bounds(built):
    """(d): the robot with every lower bound of a variable and of a constraint row at -inf: hasl all false, slacks
    included -- the max / min over the lower side must be the reductions' identities and the lower dual limit 1."""
    case = _Case("free_flying_robot", dict(K=10, order=5), lower_free=True)
    try:
        start, mu0 = case.start()
        p = case.probe
        assert not p.hasl.any() and p.hasu.any() and p.ns == p.m
        check_iteration(p, case.ora, start, mu0, tag="free_flying_robot without lower bounds (d)")
    finally:
        case.close()
