"""A compact primal-dual interior-point NLP solver behind the cyipopt ``problem_obj`` protocol.

SURVEY.md section 8f row N3.  The reference hands its callbacks to IPOPT (pycollo/nlp.py:84-115, cyipopt, or
``ca.nlpsol(..., "ipopt")``, pycollo/backend.py:1681-1711); neither IPOPT nor cyipopt exists in this image, so
this module stands in for it: it drives *exactly* the callback surface IPOPT would -- ``objective``, ``gradient``,
``constraints``, ``jacobian`` / ``jacobianstructure``, ``hessian(x, lagrange, obj_factor)`` / ``hessianstructure``
of :class:`pycollo_amd.engine.PycolloGpuProblem` -- so the end-to-end ``solve()`` objectives of the reference's
integration tests can be used as tests of the GPU path.

Algorithm: the line-search filter interior-point method of Waechter & Biegler (Math. Program. 106, 2006), the
method IPOPT implements, with its second-order correction and a Gauss-Newton stand-in for its restoration phase:

  min f(x)  s.t.  c_E(x) = c_E^L,  c_I^L <= c_I(x) <= c_I^U,  x^L <= x <= x^U
  ->  slacks s for the inequality rows;  barrier  phi_mu = f - mu sum log(v - v^L) - mu sum log(v^U - v);
  Newton on the primal-dual equations with Sigma = Z^L/(v - v^L) + Z^U/(v^U - v) folded into the (1,1) block,
  inertia-free regularisation (curvature test on the step), fraction-to-the-boundary rule, filter on
  (constraint violation, barrier objective), monotone mu update.

There is one loop, :meth:`InteriorPointSolver.solve`, and it handles scalars only.  It asks an iterate for them through
the steps the C interface names (``pc_ipm_*``, include/pycollo_amd.h): ``_set_state`` / ``_get_state``, ``_eval_point``,
``_errors``, ``_newton``, ``_trial``, ``_soc`` / ``_soc_restore``, ``_accept``; only its rare restoration branch works
on vectors, which it gets and hands back through the first three.  Two layers can be swapped under it:

* the steps: :class:`InteriorPointSolver` keeps the vectors on the host (``self.st``) and builds the steps from the
  callbacks and five linear-algebra methods (``_JT``, ``_solve_kkt``, ``_resolve_kkt``, ``_ls_multipliers``, ``_gn_step``);
  :class:`ResidentInteriorPointSolver` keeps the vectors in device memory and every step is one C call;
* the linear algebra under the host-vector steps: SuperLU (``scipy.sparse.linalg.splu``) on matrices the callbacks
  delivered as host arrays in :class:`InteriorPointSolver`; the block L D L^T of ``pycollo_amd.kkt`` on G~ / H~ that never
  leave device memory in :class:`GpuInteriorPointSolver` (row N4; ``ipm_sharded`` cuts the same across ranks).

Multiplier sign convention: L = obj_factor f + lambda^T c, as IPOPT's ``eval_h`` expects.
"""
from __future__ import annotations

import ctypes as C
import time
from dataclasses import dataclass, field
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

INF = 1e19   # IPOPT's nlp_lower/upper_bound_inf


@dataclass
class IpmResult:
    x: np.ndarray
    lam: np.ndarray
    objective: float
    status: str
    iterations: int
    inf_pr: float
    inf_du: float
    mu: float
    seconds: float
    evaluations: dict = field(default_factory=dict)
    history: list = field(default_factory=list)
    zl: np.ndarray | None = None       # multipliers of the variables' lower / upper bounds (of the unscaled problem)
    zu: np.ndarray | None = None

    @property
    def success(self) -> bool:
        return self.status in ("optimal", "acceptable")


class InteriorPointSolver:
    """The loop (:meth:`solve`), and its steps on host vectors with SuperLU under them."""

    def __init__(self, problem_obj, n: int, m: int, lb, ub, cl, cu, tol: float = 1e-8, acceptable_tol: float = 1e-6,
                 max_iter: int = 300, mu_init: float = 0.1, verbose: int = 0, warm_start: bool = False,
                 gradient_scaling: bool = True, second_order_correction: bool = True):
        self.p, self.n, self.m = problem_obj, int(n), int(m)
        self.second_order_correction = bool(second_order_correction)
        # IPOPT's warm_start_init_point (the one thing pycollo's warm_start setting switches, backend.py:1703-1709):
        # the starting point is kept closer to where it was given -- bound push / fraction 1e-3 instead of 1e-2
        # (warm_start_bound_push, warm_start_bound_frac).  No multipliers are handed over: the reference passes none.
        self.warm_start = bool(warm_start)
        self.gradient_scaling = bool(gradient_scaling)   # IPOPT's nlp_scaling_method: gradient-based (default) or none
        self.lb, self.ub = np.asarray(lb, float).copy(), np.asarray(ub, float).copy()
        self.cl, self.cu = np.asarray(cl, float).copy(), np.asarray(cu, float).copy()
        self.tol, self.acceptable_tol, self.max_iter, self.mu_init, self.verbose = tol, acceptable_tol, max_iter, mu_init, verbose
        # (a bound that is infinite on one side only: without the finiteness test, -inf gives inf <= inf below and the row
        #  would count as an equality, the variable as fixed; cl = cu = the same infinity still reads as an equality)
        with np.errstate(invalid="ignore"):
            self.eq = np.isclose(self.cl, self.cu, rtol=0, atol=0) | (np.isfinite(self.cl) & np.isfinite(self.cu) & (
                np.abs(self.cu - self.cl) <= 1e-14 * np.maximum(1.0, np.abs(self.cl))))
        self.ineq = np.nonzero(~self.eq)[0]
        self.ns = len(self.ineq)
        self.nv = self.n + self.ns
        # bounds on v = [x ; s]
        self.vl = np.concatenate([self.lb, self.cl[self.ineq]])
        self.vu = np.concatenate([self.ub, self.cu[self.ineq]])
        # fixed variables (x^L = x^U: pinned initial states, fixed times) are parameters, as in IPOPT's default
        # fixed_variable_treatment = make_parameter: no barrier terms, no step components
        with np.errstate(invalid="ignore"):
            self.fixed = np.isfinite(self.vl) & np.isfinite(self.vu) & ((self.vu - self.vl) <= 1e-12 * np.maximum(1.0, np.abs(self.vl)))
        self.free = np.nonzero(~self.fixed)[0]
        self.nf = len(self.free)
        self.hasl = (self.vl > -INF) & ~self.fixed
        self.hasu = (self.vu < INF) & ~self.fixed
        jr, jc = problem_obj.jacobianstructure()
        hr, hc = problem_obj.hessianstructure()
        self.jr, self.jc = np.asarray(jr, np.int64), np.asarray(jc, np.int64)
        self.hr, self.hc = np.asarray(hr, np.int64), np.asarray(hc, np.int64)
        self.hoff = self.hr != self.hc
        # constant part of the constraint Jacobian w.r.t. the slacks
        self.Js = sp.csr_matrix((-np.ones(self.ns), (self.ineq, np.arange(self.ns))), shape=(self.m, self.ns))
        self.rhs_c = np.where(self.eq, self.cl, 0.0)
        self.sf = 1.0                       # IPOPT's gradient-based NLP scaling (set in solve())
        self.sc = np.ones(self.m)
        self.counts = {"objective": 0, "gradient": 0, "constraints": 0, "jacobian": 0, "hessian": 0, "factorisations": 0}
        self.kkt_seconds = 0.0              # wall time inside _solve_kkt (assembly, factorisations, solves, refinement)

    # ---- callbacks --------------------------------------------------------------------------------
    def _f(self, x):
        self.counts["objective"] += 1
        return self.sf * float(self.p.objective(x))

    def _g(self, x):
        self.counts["gradient"] += 1
        return self.sf * np.asarray(self.p.gradient(x), float)

    def _c(self, v):
        self.counts["constraints"] += 1
        c = self.sc * (np.asarray(self.p.constraints(v[:self.n]), float) - self.rhs_c)
        if self.ns:
            c[self.ineq] -= v[self.n:]      # slacks live in the scaled constraint's units
        return c

    def _J(self, x):
        self.counts["jacobian"] += 1
        Jx = sp.csr_matrix((np.asarray(self.p.jacobian(x), float) * self.sc[self.jr], (self.jr, self.jc)), shape=(self.m, self.n))
        return sp.hstack([Jx, self.Js], format="csr") if self.ns else Jx

    def _W(self, x, lam):
        self.counts["hessian"] += 1
        vals = np.asarray(self.p.hessian(x, self.sc * lam, self.sf), float)
        W = sp.coo_matrix((vals, (self.hr, self.hc)), shape=(self.nv, self.nv))
        Wt = sp.coo_matrix((vals[self.hoff], (self.hc[self.hoff], self.hr[self.hoff])), shape=(self.nv, self.nv))
        return (W + Wt).tocsr()

    # ---- pieces -----------------------------------------------------------------------------------
    def _push_interior(self, v, k1=1e-2, k2=1e-2):
        v = v.copy()
        both = self.hasl & self.hasu
        onlyl = self.hasl & ~self.hasu
        onlyu = self.hasu & ~self.hasl
        with np.errstate(invalid="ignore"):   # (an infinite bound gives inf - inf in entries the masks leave out)
            pl = np.minimum(k1 * np.maximum(1.0, np.abs(self.vl)), k2 * (self.vu - self.vl))
            pu = np.minimum(k1 * np.maximum(1.0, np.abs(self.vu)), k2 * (self.vu - self.vl))
            v[both] = np.clip(v[both], (self.vl + pl)[both], (self.vu - pu)[both])
            v[onlyl] = np.maximum(v[onlyl], (self.vl + k1 * np.maximum(1.0, np.abs(self.vl)))[onlyl])
            v[onlyu] = np.minimum(v[onlyu], (self.vu - k1 * np.maximum(1.0, np.abs(self.vu)))[onlyu])
        return v

    def _barrier(self, v, f, mu):
        b = 0.0
        if self.hasl.any():
            b -= np.sum(np.log((v - self.vl)[self.hasl]))
        if self.hasu.any():
            b -= np.sum(np.log((self.vu - v)[self.hasu]))
        return f + mu * b

    def _alpha_max(self, v, dv, tau):
        a = 1.0
        dl = (v - self.vl)
        du = (self.vu - v)
        neg = self.hasl & (dv < 0)
        if neg.any():
            a = min(a, float(np.min(-tau * dl[neg] / dv[neg])))
        pos = self.hasu & (dv > 0)
        if pos.any():
            a = min(a, float(np.min(tau * du[pos] / dv[pos])))
        return a

    @staticmethod
    def _alpha_dual(z, dz, tau):
        neg = dz < 0
        return min(1.0, float(np.min(-tau * z[neg] / dz[neg]))) if neg.any() else 1.0

    def _solve_kkt(self, W, Sigma, J, r1, r2, dw_last):
        """Solve [[W + Sigma + dw I, J^T], [J, -dc I]] [dv; dlam] = [r1; r2] with the inertia-free curvature test."""
        nv, m, fr = self.nf, self.m, self.free
        dw, dc = 0.0, 0.0
        base = (W + sp.diags(Sigma))[fr][:, fr]
        J = J[:, fr]
        r1 = r1[fr]
        rhs = np.concatenate([r1, r2])
        for attempt in range(40):
            # The (2,2) block always carries a tiny -dc I: the matrix is then quasi-definite whenever the (1,1) block
            # is positive definite, a symmetric-mode LU that pivots on the diagonal exists, and the signs of U's
            # diagonal are the inertia (Sylvester) -- which is what IPOPT's regularisation is driven by
            # (n positive, m negative eigenvalues).  SuperLU with diag_pivot_thresh = 0 is that factorisation as
            # long as it reports the same row and column permutation.
            dc_eff = max(dc, 1e-9)
            K = sp.bmat([[base + dw * sp.identity(nv), J.T], [J, -dc_eff * sp.identity(m)]], format="csc")
            self.counts["factorisations"] += 1
            good, sol = False, None
            try:
                with np.errstate(all="ignore"):
                    lu = spla.splu(K, permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
                    d = lu.U.diagonal()
                    sym = np.array_equal(lu.perm_r, lu.perm_c)
                    npos, nneg = int(np.sum(d > 0)), int(np.sum(d < 0))
                    if sym and npos == nv and nneg == m:
                        # refine against the system actually wanted (dc, not dc_eff): the tiny (2,2) shift only
                        # makes the factorisation exist, it must not limit the accuracy of the step
                        K0 = K if dc_eff == dc else sp.bmat([[base + dw * sp.identity(nv), J.T],
                                                             [J, -dc * sp.identity(m) if dc > 0 else None]], format="csc")
                        sol = lu.solve(rhs)
                        res = rhs - K0 @ sol
                        for _ in range(3):
                            trial = sol + lu.solve(res)
                            res_t = rhs - K0 @ trial
                            if not np.all(np.isfinite(trial)) or np.linalg.norm(res_t) >= 0.5 * np.linalg.norm(res):
                                break          # (nearly) singular unshifted system: keep the regularised step
                            sol, res = trial, res_t
                        good = bool(np.all(np.isfinite(sol)))
                    elif not sym:
                        # off-diagonal pivots were needed: fall back to the curvature test on the step
                        sol = lu.solve(rhs)
                        if np.all(np.isfinite(sol)):
                            dv = sol[:nv]
                            good = bool(dv @ (base @ dv) + dw * (dv @ dv) >= 1e-11 * (dv @ dv))
            except RuntimeError:
                dc = 1e-8 if dc == 0.0 else dc * 10.0
            if good or (dw >= 1e20 and sol is not None and np.all(np.isfinite(sol))):
                full = np.zeros(self.nv)
                full[fr] = sol[:nv]
                self._last_factor = (lu, K)      # (second-order corrections solve with it again: _resolve_kkt)
                return full, sol[nv:], dw
            # wrong inertia / curvature (or singular): raise the primal regularisation, IPOPT's delta_w schedule
            if dw == 0.0:
                dw = 1e-4 if dw_last == 0.0 else max(1e-20, dw_last / 3.0)
            else:
                dw *= 100.0 if dw_last == 0.0 else 8.0
            if dw > 1e20:
                break
        raise RuntimeError("KKT regularisation failed")

    def _resolve_kkt(self, r1, r2, v=None, lam=None):
        """Another right-hand side for the matrix ``_solve_kkt`` factorised last (second-order correction); ``v``, ``lam``:
        the point the matrix belongs to (for a subclass whose matrix lives where trial evaluations overwrite it)."""
        lu, K = self._last_factor
        rhs = np.concatenate([r1[self.free], r2])
        sol = lu.solve(rhs)
        res = rhs - K @ sol
        for _ in range(2):
            trial = sol + lu.solve(res)
            res_t = rhs - K @ trial
            if not np.all(np.isfinite(trial)) or np.linalg.norm(res_t) >= 0.5 * np.linalg.norm(res):
                break
            sol, res = trial, res_t
        full = np.zeros(self.nv)
        full[self.free] = sol[:self.nf]
        return full, sol[self.nf:]

    def _JT(self, J, lam):
        """J^T lambda over v = [x ; s]."""
        return J.T @ lam

    def _ls_multipliers(self, J, gz):
        """Least-squares multiplier estimate: lambda of  min ||gz + J^T lambda||  over the free unknowns (IPOPT's
        initial multipliers); zeros when the estimate is unusable."""
        lam = np.zeros(self.m)
        try:
            Jf = J[:, self.free]
            K = sp.bmat([[sp.identity(self.nf), Jf.T], [Jf, None]], format="csc")
            sol = spla.splu(K).solve(np.concatenate([-gz[self.free], np.zeros(self.m)]))
            if self.m and np.all(np.isfinite(sol)) and np.max(np.abs(sol[self.nf:])) <= 1e3:
                lam = sol[self.nf:]
        except RuntimeError:
            pass
        return lam

    def _gn_step(self, J, c):
        """Minimum-norm step onto the linearised constraints (restoration): dv of [[I, J^T], [J, -1e-10 I]]."""
        Jf = J[:, self.free]
        self.counts["factorisations"] += 1
        K = sp.bmat([[sp.identity(self.nf), Jf.T], [Jf, -1e-10 * sp.identity(self.m)]], format="csc")
        sol = spla.splu(K).solve(np.concatenate([np.zeros(self.nf), -c]))
        dr = np.zeros(self.nv)
        dr[self.free] = sol[:self.nf]
        return dr

    # ---- the steps of an iteration ----------------------------------------------------------------
    # What the loop asks of an iterate: scalars out, the vectors stay where they are -- here in ``self.st`` on the host,
    # in ResidentInteriorPointSolver behind the pc_ipm_* call of the same name (include/pycollo_amd.h).
    def _set_state(self, v, lam, zl, zu):
        s = self.st
        s.v, s.lam, s.zl, s.zu = v, lam, zl, zu

    def _get_state(self):
        s = self.st
        return s.v, s.lam, s.zl, s.zu, s.c, s.g

    def _eval_point(self):
        """Scaled f and sum |c| at the current v (grad f and J there are ``_start_at``'s)."""
        s = self.st
        s.f, s.c = self._f(s.v[:self.n]), self._c(s.v)
        return s.f, float(np.sum(np.abs(s.c)))

    def _errors(self):
        """max |grad L| over the free unknowns, max |c|, sum |c|, max / min of (v - vl) zl, max / min of (vu - v) zu,
        sum |lambda|, sum zl, sum zu: E_mu of Waechter & Biegler eq. (5) follows for any mu."""
        s, e = self.st, np.zeros(10)
        s.JTlam = self._JT(s.J, s.lam)
        if self.nf:
            e[0] = np.max(np.abs((s.g + s.JTlam - s.zl + s.zu)[self.free]))
        if self.m:
            e[1] = np.max(np.abs(s.c))
        e[2] = np.sum(np.abs(s.c))
        with np.errstate(invalid="ignore"):   # (inf x 0 where there is no bound: masked out)
            if self.hasl.any():
                comp = ((s.v - self.vl) * s.zl)[self.hasl]
                e[3], e[4] = np.max(comp), np.min(comp)
            if self.hasu.any():
                comp = ((self.vu - s.v) * s.zu)[self.hasu]
                e[5], e[6] = np.max(comp), np.min(comp)
        e[7], e[8], e[9] = np.sum(np.abs(s.lam)), np.sum(s.zl), np.sum(s.zu)
        return e

    def _bound_steps(self, mu, tau):
        """The bound multipliers' steps that go with the step ``st.dv``; its fraction-to-the-boundary limits alpha_max, alpha_z."""
        s = self.st
        s.dzl = np.where(self.hasl, mu / s.dlv - s.zl - s.zl / s.dlv * s.dv, 0.0)
        s.dzu = np.where(self.hasu, mu / s.duv - s.zu + s.zu / s.duv * s.dv, 0.0)
        a_z = min(self._alpha_dual(s.zl[self.hasl], s.dzl[self.hasl], tau) if self.hasl.any() else 1.0,
                  self._alpha_dual(s.zu[self.hasu], s.dzu[self.hasu], tau) if self.hasu.any() else 1.0)
        return self._alpha_max(s.v, s.dv, tau), a_z

    def _newton(self, mu, tau, dw_last):
        """The Newton step for barrier parameter mu (after ``_errors`` at this point): dw (negative: the regularisation
        failed), alpha_max, alpha_z, grad phi . dv, mu x barrier sum at v."""
        s = self.st
        s.dlv, s.duv = np.where(self.hasl, s.v - self.vl, 1.0), np.where(self.hasu, self.vu - s.v, 1.0)
        Sigma = np.where(self.hasl, s.zl / s.dlv, 0.0) + np.where(self.hasu, s.zu / s.duv, 0.0)
        W = self._W(s.v[:self.n], s.lam)
        s.grad_phi = s.g - np.where(self.hasl, mu / s.dlv, 0.0) + np.where(self.hasu, mu / s.duv, 0.0)
        t_kkt = time.perf_counter()
        try:
            s.dv, s.dlam, dw = self._solve_kkt(W, Sigma, s.J, -(s.grad_phi + s.JTlam), -s.c, dw_last)
        except RuntimeError:
            return -1.0, 0.0, 0.0, 0.0, 0.0
        finally:
            self.kkt_seconds += time.perf_counter() - t_kkt
        a_max, a_z = self._bound_steps(mu, tau)
        return dw, a_max, a_z, float(s.grad_phi @ s.dv), float(self._barrier(s.v, 0.0, mu))

    def _trial(self, alpha, mu):
        """The trial point v + alpha dv: scaled f, sum |c|, mu x barrier sum there."""
        s = self.st
        s.vt = s.v + alpha * s.dv
        with np.errstate(all="ignore"):
            s.ft, s.ct = self._f(s.vt[:self.n]), self._c(s.vt)
            return s.ft, float(np.sum(np.abs(s.ct))), float(self._barrier(s.vt, 0.0, mu))

    def _soc(self, alpha, first, mu, tau):
        """Second-order correction after ``_trial`` rejected the step of size alpha (IPOPT A-5.7 .. A-5.9): the last
        factorisation solved again for the constraint values alpha c + c(trial) (``first``) or alpha c_soc + c(trial) of
        the previous corrected trial.  The corrected step replaces the Newton step for ``_trial`` / ``_accept``.
        Returns alpha_max, alpha_z and whether the solve failed."""
        s = self.st
        if first:
            s.newton_step = (s.dv, s.dlam, s.dzl, s.dzu)
        s.c_soc = alpha * (s.c if first else s.c_soc) + s.ct
        try:
            dv, dlam = self._resolve_kkt(-(s.grad_phi + s.JTlam), -s.c_soc, s.v, s.lam)
        except RuntimeError:
            return 0.0, 0.0, True
        if not (np.all(np.isfinite(dv)) and np.all(np.isfinite(dlam))):
            return 0.0, 0.0, True
        s.dv, s.dlam = dv, dlam
        return (*self._bound_steps(mu, tau), False)

    def _soc_restore(self, mu, tau):
        """The Newton step back in place of the rejected corrections."""
        s = self.st
        s.dv, s.dlam, s.dzl, s.dzu = s.newton_step

    def _accept(self, alpha, a_z, mu):
        """Accept the last trial point: v, lambda (+= alpha), z (+= alpha_z, kept within a factor of the primal
        estimates); grad f and J at the new v."""
        s = self.st
        s.v = s.v + alpha * s.dv
        s.lam = s.lam + alpha * s.dlam
        zl, zu = s.zl + a_z * s.dzl, s.zu + a_z * s.dzu
        ks = 1e10
        dlv, duv = np.where(self.hasl, s.v - self.vl, 1.0), np.where(self.hasu, self.vu - s.v, 1.0)
        s.zl = np.where(self.hasl, np.clip(zl, mu / (ks * dlv), ks * mu / dlv), 0.0)
        s.zu = np.where(self.hasu, np.clip(zu, mu / (ks * duv), ks * mu / duv), 0.0)
        s.f, s.c = s.ft, s.ct
        s.g = np.concatenate([self._g(s.v[:self.n]), np.zeros(self.ns)])
        s.J = self._J(s.v[:self.n])

    def _start_at(self, v, zl, zu):
        """Everything anew at v (the start, after a restoration, after a barrier restart): grad f, J, the least-squares
        multipliers, then the state and its scaled f and sum |c|."""
        s = self.st
        s.g = np.concatenate([self._g(v[:self.n]), np.zeros(self.ns)])
        s.J = self._J(v[:self.n])
        self._set_state(v, self._ls_multipliers(s.J, s.g - zl + zu), zl, zu)
        return self._eval_point()

    # ---- main loop --------------------------------------------------------------------------------
    def solve(self, x0) -> IpmResult:
        t_start = time.perf_counter()
        n, m = self.n, self.m
        self.st = SimpleNamespace()
        x0 = np.asarray(x0, float)
        # gradient-based scaling at the starting point, IPOPT's default nlp_scaling_method (the reference leaves it
        # on, pycollo/backend.py:1704-1710): objective and every constraint row are scaled down so that no
        # gradient entry exceeds nlp_scaling_max_gradient = 100
        self.sf, self.sc = 1.0, np.ones(m)
        # (evaluated at the starting point as the algorithm will use it, i.e. pushed off its bounds: a guess that sits
        #  exactly where a model is not differentiable -- Delta III on the pad, zero air speed under a square root --
        #  gives NaN partials at the raw guess; entries that are not finite anyway take no part in the maxima)
        push = (1e-3, 1e-3) if self.warm_start else (1e-2, 1e-2)
        x0c = self._push_interior(np.concatenate([x0, np.zeros(self.ns)]), *push)[:n]
        x0c[self.fixed[:n]] = self.vl[:n][self.fixed[:n]]
        g0 = np.nan_to_num(np.asarray(self.p.gradient(x0c), float), nan=0.0, posinf=0.0, neginf=0.0)
        gmax = float(np.max(np.abs(g0))) if n else 0.0
        if gmax > 100.0 and self.gradient_scaling:
            self.sf = max(100.0 / gmax, 1e-8)
        if m and self.gradient_scaling:
            jv = np.abs(np.nan_to_num(np.asarray(self.p.jacobian(x0c), float), nan=0.0, posinf=0.0, neginf=0.0))
            rowmax = np.zeros(m)
            np.maximum.at(rowmax, self.jr, jv)
            big = rowmax > 100.0
            self.sc[big] = np.maximum(100.0 / rowmax[big], 1e-8)
        if self.ns:
            self.vl[n:] = np.where(self.cl[self.ineq] > -INF, self.sc[self.ineq] * self.cl[self.ineq], self.cl[self.ineq])
            self.vu[n:] = np.where(self.cu[self.ineq] < INF, self.sc[self.ineq] * self.cu[self.ineq], self.cu[self.ineq])
        v = np.concatenate([x0, np.zeros(self.ns)])
        if self.ns:
            v[n:] = (self.sc * np.asarray(self.p.constraints(x0), float))[self.ineq]
        v = self._push_interior(v, *push)
        v[self.fixed] = self.vl[self.fixed]
        mu = self.mu_init
        f, theta0 = self._start_at(v, np.where(self.hasl, 1.0, 0.0), np.where(self.hasu, 1.0, 0.0))
        filt: list[tuple[float, float]] = []
        theta_max, theta_min = 1e4 * max(1.0, theta0), 1e-4 * max(1.0, theta0)
        dw_last = 0.0
        status, hist = "max_iter", []
        k_eps, k_mu, th_mu, s_max, g_th, g_phi, eta = 10.0, 0.2, 1.5, 100.0, 1e-5, 1e-8, 1e-4
        accept_count = restarts = restorations = it = 0
        last_alpha = last_amax = 0.0
        last_tag = ""
        inf_pr = inf_du = np.inf
        nz = max(1, int(self.hasl.sum() + self.hasu.sum()))
        any_l, any_u = bool(self.hasl.any()), bool(self.hasu.any())

        def errors(e, mu_):
            sd = max(s_max, (e[7] + e[8] + e[9]) / (m + nz)) / s_max
            scz = max(s_max, (e[8] + e[9]) / nz) / s_max
            comp = 0.0
            if any_l:
                comp = max(comp, abs(e[3] - mu_), abs(e[4] - mu_))
            if any_u:
                comp = max(comp, abs(e[5] - mu_), abs(e[6] - mu_))
            e_du = float(e[0]) if self.nf else 0.0
            e_pr = float(e[1]) if m else 0.0
            return max(e_du / sd, e_pr, comp / scz), e_pr, e_du

        phase = {"setup": time.perf_counter() - t_start, "errors": 0.0, "line_search": 0.0, "newton": 0.0}
        for it in range(self.max_iter + 1):
            t_ph = time.perf_counter()
            e = self._errors()
            theta = float(e[2])
            e0, inf_pr, inf_du = errors(e, 0.0)
            phase["errors"] += time.perf_counter() - t_ph
            hist.append((it, f, inf_pr, inf_du, mu))
            if self.verbose:
                print(f"{it:4d}  f {f: .8e}  inf_pr {inf_pr:.2e}  inf_du {inf_du:.2e}  lg(mu) {np.log10(mu):5.1f}  dw {dw_last:.1e}"
                      f"  alpha {last_alpha:.2e} (max {last_amax:.2e}){last_tag}")
            if e0 <= self.tol:
                status = "optimal"
                break
            accept_count = accept_count + 1 if e0 <= self.acceptable_tol else 0
            if accept_count >= 15:
                status = "acceptable"
                break
            if it == self.max_iter:
                break
            while errors(e, mu)[0] <= k_eps * mu and mu > self.tol / 10:
                mu = max(self.tol / 10, min(k_mu * mu, mu ** th_mu))
                filt = []
            tau = max(0.99, 1.0 - mu)
            t_ph = time.perf_counter()
            dw, a_max, a_z, dphi, mub = self._newton(mu, tau, dw_last)
            phase["newton"] += time.perf_counter() - t_ph
            if dw < 0.0:
                status = "kkt_failure"
                break
            dw_last = dw
            phi = f + mub
            # filter line search
            t_ph = time.perf_counter()
            alpha, accepted = a_max, False
            a_min = 1e-12

            def acceptable(alpha_, ft_, th_t_, phi_t_):
                """The filter's verdict on a trial point reached with step size alpha_ (IPOPT A-5.4 .. A-5.8); a point
                accepted by the sufficient-decrease test augments the filter (returned as the second value)."""
                if not (np.isfinite(ft_) and np.isfinite(th_t_) and np.isfinite(phi_t_) and th_t_ <= theta_max):
                    return False, False
                if any(th_t_ >= th_f and phi_t_ >= ph_f for th_f, ph_f in filt):
                    return False, False
                if dphi < 0 and alpha_ * (-dphi) ** 2.3 > theta ** 1.1 and theta <= theta_min:
                    return phi_t_ <= phi + eta * alpha_ * dphi, False
                ok = th_t_ <= (1 - g_th) * theta or phi_t_ <= phi - g_phi * theta
                return ok, ok

            def trial(a):
                ft_, th_t_, mub_t = self._trial(a, mu)
                return ft_, th_t_, ft_ + mub_t

            first = True
            while alpha > a_min:
                ft, th_t, phi_t = trial(alpha)
                accepted, augment = acceptable(alpha, ft, th_t, phi_t)
                if self.verbose >= 2 and first:
                    print(f"      first trial: alpha {alpha:.2e} theta {theta:.3e} -> {th_t:.3e}  phi {phi:.10e} -> {phi_t:.10e}  dphi {dphi:.3e} "
                          f"switching {dphi < 0 and alpha * (-dphi) ** 2.3 > theta ** 1.1 and theta <= theta_min} theta_min {theta_min:.1e} "
                          f"in filter {any(th_t >= th_f and phi_t >= ph_f for th_f, ph_f in filt)} accepted {accepted}")
                if accepted:
                    if augment:
                        filt.append(((1 - g_th) * theta, phi - g_phi * theta))
                    break
                if first and self.second_order_correction and np.isfinite(th_t) and th_t >= theta:
                    # Second-order correction (IPOPT A-5.7 .. A-5.9): the full step was rejected and did not even reduce
                    # the violation -- the linearisation of c is what fails.  Up to four corrected steps from the same
                    # factorisation, each aimed at the violation the previous trial point was left with.
                    th_old, a_soc = theta, alpha
                    for p_soc in range(4):
                        self.counts["second_order_corrections"] = self.counts.get("second_order_corrections", 0) + 1
                        a_soc, a_z_s, failed = self._soc(a_soc, p_soc == 0, mu, tau)
                        if failed:
                            break
                        fs, th_s, phi_s = trial(a_soc)
                        ok_s, augment = acceptable(alpha, fs, th_s, phi_s)
                        if self.verbose >= 2:
                            print(f"      correction: alpha {a_soc:.2e} theta -> {th_s:.3e}  phi -> {phi_s:.10e}  accepted {ok_s}")
                        if ok_s:
                            if augment:
                                filt.append(((1 - g_th) * theta, phi - g_phi * theta))
                            accepted, alpha, a_z, ft = True, a_soc, a_z_s, fs
                            self.counts["second_order_steps"] = self.counts.get("second_order_steps", 0) + 1
                            break
                        if not np.isfinite(th_s) or th_s > 0.99 * th_old:
                            break
                        th_old = th_s
                    if accepted:
                        break
                    self._soc_restore(mu, tau)
                first = False
                alpha *= 0.5
            phase["line_search"] += time.perf_counter() - t_ph
            if not accepted and e0 <= self.acceptable_tol:
                # IPOPT's rule for a line search that fails at a point already inside the acceptable tolerances
                # (BacktrackingLineSearch -> STOP_AT_ACCEPTABLE_POINT): no restoration from a converged point whose
                # remaining error is the linear solver's floor
                status = "acceptable"
                self.counts["acceptable_after_failed_line_search"] = 1   # (surfaced by solve_ocp: not the requested tolerance)
                break
            if not accepted:
                # feasibility restoration, reduced to its core, on host vectors (rare: a resident state comes to the host
                # for it): Gauss-Newton steps on ||c||_1 (minimum-norm solution of the linearised constraints,
                # fraction-to-the-boundary, backtracking) until the violation has dropped by a tenth and the point is
                # acceptable to the filter
                v, lam, zl, zu, c, _ = self._get_state()
                filt.append(((1 - g_th) * theta, phi - g_phi * theta))
                vr, cr_, ok_r = v.copy(), c, False
                for _ in range(30):
                    th_r = float(np.sum(np.abs(cr_)))
                    # J at the restoration point: on the device-resident paths the line search's trial points (and the
                    # Newton step's Hessian) have left G~ of another point behind
                    Jr = self._J(vr[:n])
                    try:
                        dr = self._gn_step(Jr, cr_)
                    except RuntimeError:
                        break
                    if not np.all(np.isfinite(dr)):
                        break
                    a = self._alpha_max(vr, dr, tau)
                    moved = False
                    while a > 1e-10:
                        vt = vr + a * dr
                        with np.errstate(all="ignore"):
                            ct = self._c(vt)
                        if np.all(np.isfinite(ct)) and float(np.sum(np.abs(ct))) < (1 - 1e-4 * a) * th_r:
                            vr, cr_, moved = vt, ct, True
                            break
                        a *= 0.5
                    if not moved:
                        break
                    th_t = float(np.sum(np.abs(cr_)))
                    if th_t <= 0.9 * theta:
                        with np.errstate(all="ignore"):
                            ft = self._f(vr[:n])
                            phi_t = self._barrier(vr, ft, mu)
                        if np.isfinite(phi_t) and not any(th_t >= th_f and phi_t >= ph_f for th_f, ph_f in filt):
                            ok_r = True
                            break
                if ok_r:
                    restorations += 1
                    v, last_tag = vr, " R"        # (multipliers after restoration: least squares, as at the start)
                else:
                    # The Gauss-Newton restoration could not find a point the filter accepts.  Before giving the NLP up:
                    # a barrier restart from the best restoration point -- mu back up (two decades, at most mu_init), the
                    # filter emptied, multipliers re-estimated and the bound multipliers put back on the central path
                    # -- at most three times per solve.  (IPOPT recovers from the same situation inside its restoration
                    # NLP; the degenerate cases here are bang-bang solutions on coarse meshes, where the two
                    # factorisations' rounding decides which side of the filter a trial point falls on.)
                    restarts += 1
                    if restarts > 3:
                        status = "restoration_failed"
                        break
                    if float(np.sum(np.abs(cr_))) < theta:      # keep whatever feasibility the restoration did gain
                        v = vr
                    mu = min(self.mu_init, max(100.0 * mu, 1e-6))
                    filt = []
                    # the fraction-to-the-boundary steps can have left components ON a bound in floating point: back
                    # inside by the distance the new central path keeps from it, then everything at that point anew
                    v, last_tag = self._push_interior(v, min(1e-2, mu), min(1e-2, mu)), " r"
                    dlv, duv = np.where(self.hasl, v - self.vl, 1.0), np.where(self.hasu, self.vu - v, 1.0)
                    zl = np.where(self.hasl, mu / dlv, 0.0)
                    zu = np.where(self.hasu, mu / duv, 0.0)
                last_alpha, last_amax = 0.0, a_max
                f, _ = self._start_at(v, zl, zu)
                continue
            last_alpha, last_amax, last_tag = alpha, a_max, ""
            self._accept(alpha, a_z, mu)
            f = ft
        v, lam, zl, zu, _, _ = self._get_state()
        ev = dict(self.counts)
        ev["barrier_restarts"] = restarts
        ev["restorations"] = restorations                 # successful Gauss-Newton restorations
        ev["kkt_seconds"] = self.kkt_seconds
        ev["phase_seconds"] = {k: round(val, 6) for k, val in phase.items()}   # wall time by part of the loop (with kkt_seconds)
        return IpmResult(x=v[:n].copy(), lam=(self.sc * lam / self.sf).copy(), objective=f / self.sf, status=status, iterations=it, inf_pr=inf_pr,
                         inf_du=inf_du, mu=mu, seconds=time.perf_counter() - t_start, evaluations=ev, history=hist,
                         zl=(zl[:n] / self.sf).copy(), zu=(zu[:n] / self.sf).copy())


class GpuInteriorPointSolver(InteriorPointSolver):
    """The same loop with its linear algebra on the GPU.

    G~ and H~ are evaluated into device memory (``NlpEngine.evaluate_resident``) and consumed there by the block
    L D L^T of ``pycollo_amd.kkt.GpuKkt``; what crosses the bus per iteration is a handful of vectors (x~, lambda,
    Sigma, right-hand sides, the step).  ``problem_obj`` must be a :class:`pycollo_amd.engine.PycolloGpuProblem`.
    Replaces the linear solver inside IPOPT that the reference picks by name (pycollo/backend.py:1703-1711)."""

    def __init__(self, problem_obj, n, m, lb, ub, cl, cu, **kw):
        super().__init__(problem_obj, n, m, lb, ub, cl, cu, **kw)
        self.engine = problem_obj.engine
        self.kkt = None          # built in solve(), once the row scaling is known
        self.times = {"evaluate": 0.0, "factor": 0.0, "solve": 0.0, "matvec": 0.0}

    def _ensure_kkt(self):
        if self.kkt is None:
            from .kkt import GpuKkt
            t0 = time.perf_counter()
            self.kkt = GpuKkt(self.engine, self.ineq, self.fixed, self.sc)
            self.times["tables"] = self.times.get("tables", 0.0) + time.perf_counter() - t0   # once per solve
            self.times["tables_host"] = self.kkt.seconds_tables
        return self.kkt

    # G~ (and H~) live on the device; the "matrix" handed around is a token saying at which point they were evaluated
    def _J(self, x):
        self.counts["jacobian"] += 1
        t0 = time.perf_counter()
        self.engine.evaluate_resident(x, self.sf, None, want_grad=False)
        self.times["evaluate"] += time.perf_counter() - t0
        return ("resident", self.counts["jacobian"])

    def _W(self, x, lam):
        self.counts["hessian"] += 1
        t0 = time.perf_counter()
        self.engine.evaluate_resident(x, self.sf, self.sc * lam, want_grad=False)
        self.times["evaluate"] += time.perf_counter() - t0
        return ("resident", self.counts["hessian"])

    def _JT(self, J, lam):
        k = self._ensure_kkt()
        t0 = time.perf_counter()
        y = k.matvec(np.zeros(self.nv + self.m), np.concatenate([np.zeros(self.nv), lam]), use_hess=False)
        self.times["matvec"] += time.perf_counter() - t0
        return y[:self.nv]

    def _factor(self, dvec, use_hess):
        self.counts["factorisations"] += 1
        k = self._ensure_kkt()
        t0 = time.perf_counter()
        out = k.factor(dvec, use_hess)
        self.times["factor"] += time.perf_counter() - t0
        return out

    def _refined_solve(self, rhs, dvec_true, use_hess):
        """Solve with the current factors, refined against the system with ``dvec_true`` on the diagonal."""
        k = self.kkt
        t0 = time.perf_counter()
        # solve, residual and up to three corrections (each kept only while it halves the residual and stays finite) in
        # one device-side call: the vectors cross the bus once (pc_kkt_solve_refined)
        sol, n_solves = k.solve_refined(rhs, dvec_true, use_hess, max_steps=3)
        self.times["solve"] += time.perf_counter() - t0
        self.counts["kkt_solves"] = self.counts.get("kkt_solves", 0) + n_solves
        self.counts["refined_solves"] = self.counts.get("refined_solves", 0) + 1
        return sol

    def _solve_kkt(self, W, Sigma, J, r1, r2, dw_last):
        nv, m = self.nv, self.m
        rhs = np.concatenate([np.where(self.fixed, 0.0, r1), r2])
        dw, dc = 0.0, 0.0
        for attempt in range(40):
            dc_eff = max(dc, 1e-9)
            dvec = np.concatenate([Sigma + dw, np.full(m, -dc_eff)])
            npos, nneg = self._factor(dvec, True)
            sol = None
            if npos == nv and nneg == m:        # fixed unknowns are unit pivots: counted with the primal ones
                with np.errstate(all="ignore"):
                    sol = self._refined_solve(rhs, np.concatenate([Sigma + dw, np.full(m, -dc)]), True)
                if np.all(np.isfinite(sol)):
                    self._last_dvec = np.concatenate([Sigma + dw, np.full(m, -dc)])
                    return np.where(self.fixed, 0.0, sol[:nv]), sol[nv:], dw
            if dw >= 1e20:
                break
            if dw == 0.0:
                dw = 1e-4 if dw_last == 0.0 else max(1e-20, dw_last / 3.0)
            else:
                dw *= 100.0 if dw_last == 0.0 else 8.0
        raise RuntimeError("KKT regularisation failed")

    def _resolve_kkt(self, r1, r2, v=None, lam=None):
        nv = self.nv
        # the callbacks evaluate G~ with every new point (pc_engine.hip::ensure_fcG), the trial points included: the
        # refinement's matrix-vector products need G~ / H~ of the point the factors belong to again
        self.engine.evaluate_resident(v[:self.n], self.sf, self.sc * lam, want_grad=False)
        with np.errstate(all="ignore"):
            sol = self._refined_solve(np.concatenate([np.where(self.fixed, 0.0, r1), r2]), self._last_dvec, True)
        return np.where(self.fixed, 0.0, sol[:nv]), sol[nv:]

    def _ls_multipliers(self, J, gz):
        lam = np.zeros(self.m)
        nv, m = self.nv, self.m
        dvec = np.concatenate([np.ones(nv), np.full(m, -1e-10)])
        self._factor(dvec, False)
        with np.errstate(all="ignore"):
            sol = self._refined_solve(np.concatenate([np.where(self.fixed, 0.0, -gz), np.zeros(m)]), dvec, False)
        if m and np.all(np.isfinite(sol)) and np.max(np.abs(sol[nv:])) <= 1e3:
            lam = sol[nv:]
        return lam

    def _gn_step(self, J, c):
        nv, m = self.nv, self.m
        dvec = np.concatenate([np.ones(nv), np.full(m, -1e-10)])
        self._factor(dvec, False)
        sol = self._refined_solve(np.concatenate([np.zeros(nv), -c]), dvec, False)
        return np.where(self.fixed, 0.0, sol[:nv])

    def _release(self):
        if self.kkt is not None:
            self.kkt.close()
            self.kkt = None

    def solve(self, x0) -> IpmResult:
        self.engine.set_prefetch_jac(False)     # G~ is consumed where it is produced
        try:
            res = super().solve(x0)
        finally:
            self.engine.set_prefetch_jac(True)
            self._release()
        res.evaluations["gpu_seconds"] = dict(self.times)
        return res


class _IpmDesc(C.Structure):
    _fields_ = [("n", C.c_int64), ("m", C.c_int64), ("ns", C.c_int64), ("ineq_rows", C.c_void_p),
                ("vl", C.c_void_p), ("vu", C.c_void_p), ("hasl", C.c_void_p), ("hasu", C.c_void_p), ("fixed", C.c_void_p),
                ("row_scale", C.c_void_p), ("rhs_c", C.c_void_p), ("obj_scale", C.c_double)]


class ResidentInteriorPointSolver(GpuInteriorPointSolver):
    """The same loop with the ITERATE on the device as well (``csrc/pc_ipm.hpp``): v, lambda, z, the step and every
    right-hand side stay in device memory, and each step of :class:`InteriorPointSolver` is the ``pc_ipm_*`` call of
    its name -- per iteration four or five C calls (error measures; Newton step with Hessian, assembly, factorisation
    and its regularisation loop, refined solve, step limits; one call per line-search trial point; acceptance) and a
    handful of scalars read.  For the rare restoration branch the loop pulls the state to the host and pushes the
    result back.  The reference's boundary: one call into IPOPT per solve (pycollo/backend.py:1807-1827)."""

    _ipm = None

    def _check(self, ok):
        if not ok:
            raise RuntimeError(self.engine._lib.pc_last_error().decode())

    def _ensure_ipm(self):
        """The device state, made once the scaling is known (at the first ``_set_state``)."""
        if self._ipm is None:
            lib, vp, dbl = self.engine._lib, C.c_void_p, C.c_double
            for name, args in (("create", [vp] * 4), ("set_state", [vp] * 5), ("get_state", [vp] * 7), ("get_step", [vp] * 7), ("eval_point", [vp, vp]),
                               ("errors", [vp, vp]), ("newton", [vp, dbl, dbl, dbl, vp]), ("trial", [vp, dbl, dbl, vp]),
                               ("accept", [vp, dbl, dbl, dbl]), ("soc", [vp, dbl, C.c_int, dbl, dbl, vp]), ("soc_restore", [vp, dbl, dbl])):
                fn = getattr(lib, "pc_ipm_" + name)
                fn.restype, fn.argtypes = C.c_int, args
            lib.pc_ipm_destroy.restype, lib.pc_ipm_destroy.argtypes = None, [vp]
            kkt = self._ensure_kkt()
            keep = [np.ascontiguousarray(self.ineq, dtype=np.int64), np.ascontiguousarray(self.vl), np.ascontiguousarray(self.vu),
                    np.ascontiguousarray(self.hasl, dtype=np.uint8), np.ascontiguousarray(self.hasu, dtype=np.uint8),
                    np.ascontiguousarray(self.fixed, dtype=np.uint8), np.ascontiguousarray(self.sc), np.ascontiguousarray(self.rhs_c)]
            d = _IpmDesc(self.n, self.m, self.ns, *[a.ctypes.data for a in keep], float(self.sf))
            handle = vp()
            self._check(lib.pc_ipm_create(self.engine._h, kkt._h, C.byref(d), C.byref(handle)))
            self._ipm, self._lib = handle, lib
            self._r3, self._r8, self._r10 = np.empty(3), np.empty(8), np.empty(10)
        return self._ipm

    def _release(self):
        if self._ipm is not None:
            self.engine._lib.pc_ipm_destroy(self._ipm)
            self._ipm = None
        super()._release()

    def solve(self, x0) -> IpmResult:
        res = super().solve(x0)
        res.evaluations["resident_iteration"] = True
        return res

    def _set_state(self, v, lam, zl, zu):
        h = self._ensure_ipm()
        self._check(self._lib.pc_ipm_set_state(h, *(np.ascontiguousarray(a, dtype=np.float64).ctypes.data for a in (v, lam, zl, zu))))

    def _get_state(self):
        nv, m = self.nv, self.m
        out = [np.empty(nv), np.empty(m), np.empty(nv), np.empty(nv), np.empty(m), np.empty(nv)]
        self._check(self._lib.pc_ipm_get_state(self._ipm, *(a.ctypes.data for a in out)))
        return out

    def _get_step(self):
        """Read only, for tests (the loop does not call it): the last linear solve's solution [dv ; dlam], dzl, dzu, its
        right-hand side, the last trial point and the unshifted diagonal the solve was refined against."""
        nv, nu = self.nv, self.nv + self.m
        out = [np.empty(nu), np.empty(nv), np.empty(nv), np.empty(nu), np.empty(nv), np.empty(nu)]
        self._check(self._lib.pc_ipm_get_step(self._ipm, *(a.ctypes.data for a in out)))
        return out

    def _eval_point(self):
        # (grad J and G~ at this point were counted when _start_at asked for them)
        self.counts["objective"] += 1
        self.counts["constraints"] += 1
        self._check(self._lib.pc_ipm_eval_point(self._ipm, self._r3.ctypes.data))
        return float(self._r3[0]), float(self._r3[1])

    def _errors(self):
        self._check(self._lib.pc_ipm_errors(self._ipm, self._r10.ctypes.data))
        return self._r10.copy()

    def _newton(self, mu, tau, dw_last):
        r8 = self._r8
        t_kkt = time.perf_counter()
        self.counts["hessian"] += 1
        self._check(self._lib.pc_ipm_newton(self._ipm, mu, tau, dw_last, r8.ctypes.data))
        self.kkt_seconds += time.perf_counter() - t_kkt
        self.counts["factorisations"] += int(r8[5])
        self.counts["kkt_solves"] = self.counts.get("kkt_solves", 0) + int(r8[6])
        self.counts["refined_solves"] = self.counts.get("refined_solves", 0) + 1
        return float(r8[0]), float(r8[1]), float(r8[2]), float(r8[3]), float(r8[4])

    def _trial(self, alpha, mu):
        self.counts["objective"] += 1
        self.counts["constraints"] += 1
        self._check(self._lib.pc_ipm_trial(self._ipm, alpha, mu, self._r3.ctypes.data))
        return float(self._r3[0]), float(self._r3[1]), float(self._r3[2])

    def _soc(self, alpha, first, mu, tau):
        r8 = self._r8
        self._check(self._lib.pc_ipm_soc(self._ipm, alpha, 1 if first else 0, mu, tau, r8.ctypes.data))
        self.counts["kkt_solves"] = self.counts.get("kkt_solves", 0) + int(r8[6])
        return float(r8[1]), float(r8[2]), r8[7] != 0.0

    def _soc_restore(self, mu, tau):
        self._check(self._lib.pc_ipm_soc_restore(self._ipm, mu, tau))

    def _accept(self, alpha, a_z, mu):
        self.counts["gradient"] += 1
        self.counts["jacobian"] += 1
        self._check(self._lib.pc_ipm_accept(self._ipm, alpha, a_z, mu))


def solve_nlp(problem_obj, x0, lb, ub, cl, cu, **options) -> IpmResult:
    """``ipopt.problem(n, m, problem_obj, lb, ub, cl, cu).solve(x0)`` with the stand-in solver."""
    return InteriorPointSolver(problem_obj, len(x0), len(cl), lb, ub, cl, cu, **options).solve(x0)
