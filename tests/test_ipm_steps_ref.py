"""The reference statement of every step of an interior-point iteration (``StepRef``), and the host steps of
``pycollo_amd.ipm.InteriorPointSolver`` held to it on two analytic NLPs.  No GPU.

``StepRef`` restates the comments of ``pycollo_amd/csrc/pc_ipm.hpp`` -- scaled c, g, the ten error scalars, Sigma,
grad phi, the right-hand side, dzl / dzu, the six step scalars, the trial point with its barrier sum, c_soc and the
accepted v, lambda, zl, zu with the 1e10 clip -- entry by entry in ``np.longdouble`` (64-bit mantissa: an entry's own
error is 2^-11 of a double's) with every sum taken exactly (``math.fsum`` over the high and low double halves of the
long-double terms, i.e. more than 30 digits for the summation).  Nothing is imported from ``ipm.py``.  Beside each
value it returns the running magnitude of the terms it is made of, in the manner of ``OracleNlp.c_mag``.

Bounds (derived, not tuned; eps = 2^-52):

* an entry computed in k roundings from terms of magnitude mag: k eps mag; the largest k is 5 (dzl), one constant
  8 eps mag is used.  The magnitude is that of the terms each rounding acts on: a difference v - vl of two given doubles
  is rounded relative to its own result.
* a max / min: the same bound on the entry that attains it (the largest bound among the entries that can attain it
  within their bounds).  A max / min over given doubles (max |c|) is exact.
* a sum of N terms: (ceil(N / 32768) + 18) eps sum(mag): the serial part of a thread of the 128 x 256 grid, two
  8-level trees, the element's own rounding.
* a barrier term -log(d), d = fl(v - vl): the device's log gets 1 ulp, and the rounding of d (relative eps / 2) moves
  the logarithm by eps / 2 absolutely: the term's magnitude is |log d| + 1.
* a step limit -tau z / dz inherits dz's error: bound 8 eps |limit| (1 + mag(dz) / |dz|); an entry whose dz is within its
  own bound of zero has no bound (and the tests require that no such entry can attain the minimum).
* what comes from the oracle (c~, grad J, J^T lambda) is held by ``conftest.entry_err``'s rule, 1e-10 |ref| + 64 eps mag.
"""
import math

import numpy as np
import pytest

LD = np.longdouble
EPS = float(np.finfo(float).eps)
assert np.finfo(LD).eps < 1e-18, "np.longdouble carries no more than a double here: StepRef needs the 64-bit mantissa"
K_ENTRY = 8.0
KS = 1e10


def exact_sum(terms):
    """The sum of long-double terms, exact until the final rounding to a double."""
    t = np.asarray(terms, LD).ravel()
    if t.size == 0:
        return 0.0
    if not np.all(np.isfinite(t)):
        return float(np.sum(t))
    hi = t.astype(np.float64)
    lo = (t - hi.astype(LD)).astype(np.float64)
    return math.fsum(np.concatenate([hi, lo]).tolist())


def sum_bound(mags, n_serial):
    return (math.ceil(max(1, n_serial) / 32768) + 18) * EPS * exact_sum(np.abs(np.asarray(mags, LD)))


def attained(vals, bnds, kind, init=None):
    """(max or min of vals, the bound it is held to): the largest bound among the entries that can attain it within
    their bounds (an entry without a bound is given as the extreme value it can take).  ``init``: the value the reduction
    starts from (takes part with bound 0)."""
    vals, bnds = np.asarray(vals, LD).ravel(), np.asarray(bnds, LD).ravel()
    if init is not None:
        vals, bnds = np.concatenate([vals, [LD(init)]]), np.concatenate([bnds, [LD(0)]])
    if vals.size == 0:
        return (-np.inf if kind == "max" else np.inf), 0.0
    with np.errstate(invalid="ignore"):
        if kind == "max":
            i = int(np.argmax(np.where(np.isfinite(bnds), vals, -np.inf)))
            can = np.where(np.isfinite(bnds), vals + bnds, vals) >= vals[i] - bnds[i]
        else:
            i = int(np.argmin(np.where(np.isfinite(bnds), vals, np.inf)))
            can = np.where(np.isfinite(bnds), vals - bnds, vals) <= vals[i] + bnds[i]
    return float(vals[i]), float(np.max(bnds[can]))


def ratio(got, ref, bound):
    """max |got - ref| / bound over the entries (0 / 0 = 0; the same infinity on both sides = 0; else inf)."""
    got, ref, bound = np.broadcast_arrays(np.asarray(got, LD), np.asarray(ref, LD), np.asarray(bound, LD))
    if ref.size == 0:
        return 0.0
    same = (np.isinf(got) & np.isinf(ref) & (np.sign(got) == np.sign(ref))) | (got == ref)
    fin = np.isfinite(got) & np.isfinite(ref)
    if not np.all(same | fin):
        return float("inf")
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        r = np.where(same, LD(0), np.abs(np.where(fin, got, 0) - np.where(fin, ref, 0)) / bound)
    return float(np.max(r))


class StepRef:
    """Static data of a solver (vl, vu, hasl, hasu, fixed, sc, rhs_c, ineq, sf) and a state (v, lam, zl, zu, c, g, JTlam
    and, for the oracle-derived J^T lambda, its magnitude JTlam_mag); every method returns what the ``pc_ipm_*`` call of
    its name must produce, as (value, bound) pairs."""

    def __init__(self, static, **state):
        s = static
        self.vl, self.vu = np.asarray(s["vl"], LD), np.asarray(s["vu"], LD)
        self.hasl, self.hasu, self.fixed = (np.asarray(s[k], bool) for k in ("hasl", "hasu", "fixed"))
        self.sc, self.rhs_c = np.asarray(s["sc"], LD), np.asarray(s["rhs_c"], LD)
        self.ineq, self.sf = np.asarray(s["ineq"], np.int64), LD(s["sf"])
        self.nv, self.m = len(self.vl), len(self.sc)
        self.n, self.nu = self.nv - len(self.ineq), self.nv + self.m
        for k in ("v", "lam", "zl", "zu", "c", "g", "JTlam", "JTlam_mag"):
            setattr(self, k, None if state.get(k) is None else np.asarray(state[k], LD))
        if self.JTlam_mag is None and self.JTlam is not None:
            self.JTlam_mag = None

    # ---- pieces --------------------------------------------------------------------------------------------------
    def _dist(self, v=None):
        v = self.v if v is None else np.asarray(v, LD)
        with np.errstate(invalid="ignore"):
            dl = np.where(self.hasl, v - self.vl, LD(1))
            du = np.where(self.hasu, self.vu - v, LD(1))
        return dl, du

    def _oracle_err(self):
        """What entry_err's rule allows J^T lambda when it comes from the oracle (0 when it is given exactly)."""
        if self.JTlam_mag is None:
            return np.zeros(self.nv, LD)
        return 1e-10 * np.abs(self.JTlam) + 64 * EPS * self.JTlam_mag

    def scaled_c(self, c_raw, v=None):
        """c = sc (c_raw - rhs_c) - [slack of the row]; its magnitude."""
        v = self.v if v is None else np.asarray(v, LD)
        c_raw = np.asarray(c_raw, LD)
        c = self.sc * (c_raw - self.rhs_c)
        mag = np.abs(self.sc) * (np.abs(c_raw) + np.abs(self.rhs_c))
        if len(self.ineq):
            c[self.ineq] -= v[self.n:]
            mag[self.ineq] += np.abs(v[self.n:])
        return c, mag

    def scaled_g(self, grad_J):
        """g = [sf grad J ; 0]."""
        return np.concatenate([self.sf * np.asarray(grad_J, LD), np.zeros(self.nv - self.n, LD)])

    def barrier(self, v, n_serial=None):
        """-sum log(v - vl) - sum log(vu - v) at the doubles v, and its bound."""
        dl, du = self._dist(v)
        terms = np.concatenate([-np.log(dl[self.hasl]), -np.log(du[self.hasu])])
        return exact_sum(terms), sum_bound(np.abs(terms) + 1, self.nv if n_serial is None else n_serial)

    # ---- pc_ipm_eval_point / the theta part of pc_ipm_trial ------------------------------------------------------
    def theta(self, c):
        c = np.abs(np.asarray(c, LD))
        return (exact_sum(c), sum_bound(c, self.m)), ((float(np.max(c)) if c.size else 0.0), 0.0)

    # ---- pc_ipm_errors ---------------------------------------------------------------------------------------------
    def errors(self):
        val, bnd = np.zeros(10), np.zeros(10)
        free = ~self.fixed
        r = self.g + self.JTlam - self.zl + self.zu
        mag = np.abs(self.g) + np.abs(self.JTlam) + np.abs(self.zl) + np.abs(self.zu)
        val[0], bnd[0] = attained(np.abs(r)[free], (K_ENTRY * EPS * mag + self._oracle_err())[free], "max", init=0.0)
        (val[2], bnd[2]), (val[1], bnd[1]) = self.theta(self.c)
        dl, du = self._dist()
        n_ser = max(self.nv, self.m)
        cl, cu = (dl * self.zl)[self.hasl], (du * self.zu)[self.hasu]
        val[3], bnd[3] = attained(cl, K_ENTRY * EPS * np.abs(cl), "max")
        val[4], bnd[4] = attained(cl, K_ENTRY * EPS * np.abs(cl), "min")
        val[5], bnd[5] = attained(cu, K_ENTRY * EPS * np.abs(cu), "max")
        val[6], bnd[6] = attained(cu, K_ENTRY * EPS * np.abs(cu), "min")
        for slot, t in ((7, np.abs(self.lam)), (8, self.zl), (9, self.zu)):
            val[slot], bnd[slot] = exact_sum(t), sum_bound(t, n_ser)
        return val, bnd

    # ---- pc_ipm_newton: before the solve ---------------------------------------------------------------------------
    def newton_setup(self, mu):
        """Sigma, grad phi, the right-hand side (each with its bound)."""
        mu = LD(mu)
        dl, du = self._dist()
        sl, su = np.where(self.hasl, self.zl / dl, LD(0)), np.where(self.hasu, self.zu / du, LD(0))
        ml, mu_ = np.where(self.hasl, mu / dl, LD(0)), np.where(self.hasu, mu / du, LD(0))
        Sigma = sl + su
        gphi = self.g - ml + mu_
        gphi_mag = np.abs(self.g) + np.abs(ml) + np.abs(mu_)
        rhs1 = np.where(self.fixed, LD(0), -(gphi + self.JTlam))
        rhs1_b = np.where(self.fixed, LD(0), K_ENTRY * EPS * (gphi_mag + np.abs(self.JTlam)) + self._oracle_err())
        self.gphi, self.gphi_mag = gphi, gphi_mag
        return ((Sigma, K_ENTRY * EPS * (np.abs(sl) + np.abs(su))), (gphi, K_ENTRY * EPS * gphi_mag),
                (np.concatenate([rhs1, -self.c]), np.concatenate([rhs1_b, np.zeros(self.m, LD)])))

    # ---- pc_ipm_newton / pc_ipm_soc / pc_ipm_soc_restore: after the solve -----------------------------------------------
    def step(self, sol, mu, tau):
        """dv, dzl, dzu (value, bound) and the six scalars of ipm_step_kernel (values, bounds) for the solution ``sol``."""
        mu, tau, sol = LD(mu), LD(tau), np.asarray(sol, LD)
        if getattr(self, "gphi", None) is None:
            self.newton_setup(mu)
        dv = np.where(self.fixed, LD(0), sol[:self.nv])
        with np.errstate(invalid="ignore"):
            dl_raw, du_raw = self.v - self.vl, self.vu - self.v
        dl, du = self._dist()
        with np.errstate(invalid="ignore", over="ignore"):
            a = np.where(self.hasl, mu / dl - self.zl - self.zl / dl * dv, LD(0))
            a_mag = np.where(self.hasl, np.abs(mu / dl) + np.abs(self.zl) + np.abs(self.zl / dl * dv), LD(0))
            b = np.where(self.hasu, mu / du - self.zu + self.zu / du * dv, LD(0))
            b_mag = np.where(self.hasu, np.abs(mu / du) + np.abs(self.zu) + np.abs(self.zu / du * dv), LD(0))
        a_b, b_b = K_ENTRY * EPS * a_mag, K_ENTRY * EPS * b_mag
        val, bnd = np.zeros(6), np.zeros(6)
        # 0: the primal limit
        kl, ku = self.hasl & (dv < 0), self.hasu & (dv > 0)
        cand = np.concatenate([-tau * dl_raw[kl] / dv[kl], tau * du_raw[ku] / dv[ku]])
        val[0], bnd[0] = attained(cand, K_ENTRY * EPS * np.abs(cand), "min", init=1.0)
        # 1 / 2: the dual limits (inherit the error of dz; no bound where the sign of dz is not decided)
        for slot, z, dz, dz_b, has in ((1, self.zl, a, a_b, self.hasl), (2, self.zu, b, b_b, self.hasu)):
            undecided = has & (np.abs(dz) <= dz_b) & (dz_b > 0)
            k = has & ((dz < 0) | undecided)
            with np.errstate(divide="ignore", invalid="ignore"):
                cand = -tau * z[k] / np.where(undecided[k], -2 * np.abs(dz_b[k]), dz[k])
                cb = np.where(undecided[k], LD(np.inf), K_ENTRY * EPS * np.abs(cand) * (1 + dz_b[k] / (K_ENTRY * EPS) / np.abs(dz[k])))
            val[slot], bnd[slot] = attained(cand, cb, "min", init=1.0)
        val[3], bnd[3] = exact_sum(self.gphi * dv), sum_bound(self.gphi_mag * np.abs(dv), self.nu)
        val[4], bnd[4] = self.barrier(self.v, self.nu)
        val[5] = float(np.sum(~np.isfinite(dv)) + np.sum(~np.isfinite(sol[self.nv:])))
        return (dv, np.zeros(self.nv, LD)), (a, a_b), (b, b_b), val, bnd

    # ---- pc_ipm_trial ----------------------------------------------------------------------------------------------
    def trial(self, alpha, dv):
        dv = np.asarray(dv, LD)
        vt = self.v + LD(alpha) * dv
        return vt, K_ENTRY * EPS * (np.abs(self.v) + np.abs(LD(alpha) * dv))

    # ---- pc_ipm_soc ------------------------------------------------------------------------------------------------
    @staticmethod
    def c_soc(alpha, c_prev, ct):
        c_prev, ct = np.asarray(c_prev, LD), np.asarray(ct, LD)
        return LD(alpha) * c_prev + ct, K_ENTRY * EPS * (np.abs(LD(alpha) * c_prev) + np.abs(ct))

    # ---- pc_ipm_accept ---------------------------------------------------------------------------------------------
    def accept(self, alpha, a_z, mu, vt, sol, dzl, dzu):
        """v, lambda, zl, zu after the acceptance (value, bound each) and how many entries took the lower / upper arm of
        the clip."""
        alpha, a_z, mu = LD(alpha), LD(a_z), LD(mu)
        vt, sol = np.asarray(vt, LD), np.asarray(sol, LD)
        lam = self.lam + alpha * sol[self.nv:]
        lam_b = K_ENTRY * EPS * (np.abs(self.lam) + np.abs(alpha * sol[self.nv:]))
        dl, du = self._dist(vt)
        out, arms = [], [0, 0]
        for z, dz, d, has in ((self.zl, np.asarray(dzl, LD), dl, self.hasl), (self.zu, np.asarray(dzu, LD), du, self.hasu)):
            a = z + a_z * dz
            a_b = K_ENTRY * EPS * (np.abs(z) + np.abs(a_z * dz))
            with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
                lo, hi = mu / (LD(KS) * d), LD(KS) * mu / d
            lo_b, hi_b = K_ENTRY * EPS * np.abs(lo), K_ENTRY * EPS * np.abs(hi)
            with np.errstate(invalid="ignore"):
                low, high = has & (a < lo), has & (a > hi)
                near_lo, near_hi = np.abs(a - lo) <= a_b + lo_b, np.abs(a - hi) <= a_b + hi_b
            arms[0] += int(np.sum(low & ~near_lo))
            arms[1] += int(np.sum(high & ~near_hi))
            val = np.where(low, lo, np.where(high, hi, a))
            bnd = np.where(low, lo_b, np.where(high, hi_b, a_b)) + np.where(near_lo, a_b + lo_b, 0) + np.where(near_hi, a_b + hi_b, 0)
            out.append((np.where(has, val, LD(0)), np.where(has, bnd, LD(0))))
        return (vt, np.zeros(self.nv, LD)), (lam, lam_b), out[0], out[1], tuple(arms)


def static_of(solver):
    """The static data ``StepRef`` takes, from a solver whose scaling has been set (after the start of ``solve``)."""
    return dict(vl=solver.vl, vu=solver.vu, hasl=solver.hasl, hasu=solver.hasu, fixed=solver.fixed, sc=solver.sc,
                rhs_c=solver.rhs_c, ineq=solver.ineq, sf=solver.sf)


# ---- the host steps held to StepRef -----------------------------------------------------------------------------------
def _problems():
    from test_ipm_cpu import HS071, WaechterBiegler
    return {"hs071": (HS071(), 4, 2, np.ones(4), 5 * np.ones(4), np.array([25.0, 40.0]), np.array([2e19, 40.0]), [1.0, 5.0, 5.0, 1.0]),
            "waechter_biegler": (WaechterBiegler(), 3, 2, [-2e19, 0.0, 0.0], [2e19, 2e19, 2e19], np.zeros(2), np.zeros(2), [0.5, 1.0, 1.0])}


def _captured(name):
    """Every accepted iterate (v, lam, zl, zu, mu) of a host solve, slacks included, the start first."""
    from pycollo_amd.ipm import InteriorPointSolver
    p, n, m, lb, ub, cl, cu, x0 = _problems()[name]
    s = InteriorPointSolver(p, n, m, lb, ub, cl, cu)
    states, mus = [], []
    newton, accept = s._newton, s._accept

    def _newton(mu, tau, dw_last):
        if not states:
            states.append((s.st.v.copy(), s.st.lam.copy(), s.st.zl.copy(), s.st.zu.copy(), mu))
        return newton(mu, tau, dw_last)

    def _accept(alpha, a_z, mu):
        accept(alpha, a_z, mu)
        states.append((s.st.v.copy(), s.st.lam.copy(), s.st.zl.copy(), s.st.zu.copy(), mu))
    s._newton, s._accept = _newton, _accept
    res = s.solve(np.array(x0, float))
    assert res.status == "optimal"
    return s, states


@pytest.mark.parametrize("name", ["hs071", "waechter_biegler"])
@pytest.mark.parametrize("where", ["start", "mid", "late"])
def test_host_steps_follow_the_reference_statement(name, where):
    s, states = _captured(name)
    v, lam, zl, zu, mu = states[{"start": 0, "mid": len(states) // 2, "late": len(states) - 2}[where]]
    n, nv = s.n, s.nv
    st = s.st
    # the state and everything the steps read at it, as _start_at would leave it (without its multiplier estimate)
    st.g = np.concatenate([s._g(v[:n]), np.zeros(s.ns)])
    st.J = s._J(v[:n])
    s._set_state(v, lam, zl, zu)
    f, theta = s._eval_point()
    J = np.asarray(st.J.todense(), LD)
    ref = StepRef(static_of(s), v=v, lam=lam, zl=zl, zu=zu, JTlam=J.T @ np.asarray(lam, LD))
    c_ref, c_mag = ref.scaled_c(s.p.constraints(v[:n]))
    assert ratio(st.c, c_ref, K_ENTRY * EPS * c_mag) <= 1.0
    assert ratio(st.g, ref.scaled_g(s.p.gradient(v[:n])), K_ENTRY * EPS * np.abs(st.g)) <= 1.0
    ref.c, ref.g = np.asarray(st.c, LD), np.asarray(st.g, LD)         # downstream: the step's own inputs
    (th, th_b), _ = ref.theta(st.c)
    assert abs(theta - th) <= th_b
    # J^T lambda of the host (a sparse product): held by the rounding of its own terms
    jtl_mag = np.abs(J).T @ np.abs(np.asarray(lam, LD))
    e = s._errors()
    assert ratio(st.JTlam, ref.JTlam, K_ENTRY * EPS * jtl_mag + 1e-300) <= 1.0
    ref.JTlam = np.asarray(st.JTlam, LD)
    val, bnd = ref.errors()
    for q in range(10):
        if (q in (3, 4) and not s.hasl.any()) or (q in (5, 6) and not s.hasu.any()):
            # no bound on that side: the reduction's identities on the device (-inf / +inf), untouched zeros on the host
            assert e[q] == 0.0 and val[q] == (-np.inf if q in (3, 5) else np.inf)
            continue
        assert ratio(e[q], val[q], bnd[q]) <= 1.0, (q, e[q], val[q], bnd[q])
    tau = max(0.99, 1.0 - mu)
    dw, a_max, a_z, dphi, mub = s._newton(mu, tau, 0.0)
    assert dw >= 0.0
    (Sigma, Sigma_b), (gphi, gphi_b), (rhs, rhs_b) = ref.newton_setup(mu)
    assert ratio(st.grad_phi, gphi, gphi_b) <= 1.0
    sol = np.concatenate([st.dv, st.dlam])
    (dv, _), (dzl, dzl_b), (dzu, dzu_b), sv, sb = ref.step(sol, mu, tau)
    assert np.all(st.dv[s.fixed] == 0.0) and np.all(st.dzl[~s.hasl] == 0.0) and np.all(st.dzu[~s.hasu] == 0.0)
    assert ratio(st.dzl, dzl, dzl_b) <= 1.0 and ratio(st.dzu, dzu, dzu_b) <= 1.0
    assert np.isfinite(sb).all()
    for got, q in ((a_max, 0), (dphi, 3)):
        assert ratio(got, sv[q], sb[q]) <= 1.0, (q, got, sv[q], sb[q])
    assert ratio(a_z, min(sv[1], sv[2]), max(sb[1], sb[2])) <= 1.0
    assert ratio(mub, mu * sv[4], mu * sb[4] + EPS * abs(mu * sv[4])) <= 1.0
    # trial point, second-order correction and back, acceptance
    alpha = 0.5 * a_max
    ft, th_t, mub_t = s._trial(alpha, mu)
    vt, vt_b = ref.trial(alpha, st.dv)
    assert ratio(st.vt, vt, vt_b) <= 1.0
    bar, bar_b = ref.barrier(st.vt)
    assert ratio(mub_t, mu * bar, mu * bar_b + EPS * abs(mu * bar)) <= 1.0
    ct_ref, ct_mag = ref.scaled_c(s.p.constraints(st.vt[:n]), st.vt)
    assert ratio(st.ct, ct_ref, K_ENTRY * EPS * ct_mag) <= 1.0
    newton_step = (st.dv.copy(), st.dlam.copy(), st.dzl.copy(), st.dzu.copy())
    a1, az1, failed = s._soc(alpha, True, mu, tau)
    assert not failed
    cs, cs_b = ref.c_soc(alpha, st.c, st.ct)
    assert ratio(st.c_soc, cs, cs_b) <= 1.0
    (_, _), (dzl, dzl_b), (dzu, dzu_b), sv, sb = ref.step(np.concatenate([st.dv, st.dlam]), mu, tau)
    assert ratio(st.dzl, dzl, dzl_b) <= 1.0 and ratio(st.dzu, dzu, dzu_b) <= 1.0
    assert ratio(a1, sv[0], sb[0]) <= 1.0 and ratio(az1, min(sv[1], sv[2]), max(sb[1], sb[2])) <= 1.0
    prev = st.c_soc.copy()
    s._trial(a1, mu)
    s._soc(a1, False, mu, tau)
    cs, cs_b = ref.c_soc(a1, prev, st.ct)
    assert ratio(st.c_soc, cs, cs_b) <= 1.0
    s._soc_restore(mu, tau)
    for got, kept in zip((st.dv, st.dlam, st.dzl, st.dzu), newton_step):
        np.testing.assert_array_equal(got, kept)
    s._trial(alpha, mu)
    vt_host = st.vt.copy()
    s._accept(alpha, 0.75 * a_z, mu)
    (v_r, _), (lam_r, lam_b), (zl_r, zl_b), (zu_r, zu_b), _ = ref.accept(alpha, 0.75 * a_z, mu, vt_host, np.concatenate([st.dv, st.dlam]),
                                                                       st.dzl, st.dzu)
    np.testing.assert_array_equal(st.v, vt_host)
    assert ratio(st.lam, lam_r, lam_b) <= 1.0
    assert ratio(st.zl, zl_r, zl_b) <= 1.0 and ratio(st.zu, zu_r, zu_b) <= 1.0
    assert np.all(st.zl[~s.hasl] == 0.0) and np.all(st.zu[~s.hasu] == 0.0)


def test_both_arms_of_the_clip_and_the_exact_sum():
    """StepRef itself: a multiplier far below / above its central-path value takes the lower / upper arm; a sum whose
    terms cancel to the last bit of a double is exact."""
    static = dict(vl=np.zeros(3), vu=np.full(3, 2e19), hasl=np.ones(3, bool), hasu=np.zeros(3, bool), fixed=np.zeros(3, bool),
                  sc=np.ones(0), rhs_c=np.zeros(0), ineq=np.zeros(0, np.int64), sf=1.0)
    ref = StepRef(static, v=np.ones(3), lam=np.zeros(0), zl=np.array([1e-30, 1.0, 1e30]), zu=np.zeros(3))
    _, _, (zl, _), (zu, _), arms = ref.accept(1.0, 0.0, 1.0, np.ones(3), np.zeros(3), np.zeros(3), np.zeros(3))
    assert arms == (1, 1)
    assert float(zl[0]) == 1e-10 and float(zl[1]) == 1.0 and float(zl[2]) == 1e10 and np.all(zu == 0)
    assert exact_sum(np.array([1e16, 1.0, -1e16], LD)) == 1.0
    assert exact_sum(np.array([LD(1) + LD(2) ** -60, -1.0], LD)) == 2.0 ** -60


def test_an_infinite_bound_is_no_bound():
    """-inf / +inf as a bound (not only IPOPT's 1e19): no variable becomes fixed and no row an equality through
    inf <= inf, the side has no barrier terms, and the problem solves as with 2e19."""
    from pycollo_amd.ipm import InteriorPointSolver
    from test_ipm_cpu import WaechterBiegler
    a = InteriorPointSolver(WaechterBiegler(), 3, 2, [-np.inf, 0.0, 0.0], [np.inf, np.inf, np.inf], np.zeros(2), np.zeros(2))
    assert not a.fixed.any() and a.eq.all() and not a.hasu.any() and list(a.hasl) == [False, True, True]
    b = InteriorPointSolver(WaechterBiegler(), 3, 2, [-np.inf] * 3, [np.inf, 5.0, 5.0], [-np.inf, -np.inf], np.zeros(2))
    assert not b.fixed.any() and not b.eq.any() and b.ns == 2 and not b.hasl.any() and b.hasu.sum() == 4
    res = a.solve(np.array([0.5, 1.0, 1.0]))
    assert res.status == "optimal"
    np.testing.assert_allclose(res.x, [1.0, 0.0, 0.5], atol=1e-6)
