"""The tests' own host restatement of the propagation with integrals and dense output (DESIGN 8g;
pycollo_amd/csrc/pc_solution.hpp, pc_sol_propagate_dense_p<i>).  TEST INFRASTRUCTURE: nothing here shares code with the
kernel or with ``Solution.propagate_dense``.  It stands on tests/propagate_ref.py (the sections, the tableau, the step
control) and adds

* the integrals: I_m rides beside y with dI_m/dc = g g_m at the stage arguments of f, from 0 at every segment's first
  node, by the same rows in the same order; with ``integral_atol`` it joins the error norm;
* ``P``: Shampine's continuous extension of the pair as exact fractions, rounded once; over an accepted step from (c, y)
  of width h the value at c + theta h is y + h sum_i K_i b_i(theta), rows of P that are zero left out;
* the ownership rule: :func:`query_plan` sorts the queries (stable) and gives every node interval its slot.

:func:`propagate_dense_f64`: float64, both modes, the kernel's arithmetic step by step.  :class:`DenseFixedReference`: the
fixed mode at 60 digits; the doubles it is fed (with propagate_ref's: the queries' c_q and the rounded P) are taken as
exact.  With every value it returns the rounding scale of the project's parity rule: n, the steps taken in the segment
up to and including the one that answers, and M, the largest over those steps of |y_a| + |h g| sum_i |b_i| F_a,i (for an
integral: |I_m| + |h g| sum_i |b_i| G_m,i; for the step that answers a query inside it: b_i(theta) in place of b_i, all
seven stages), F and G with every term in absolute value.
"""
from fractions import Fraction as Fr

import mpmath as mp
import numpy as np
import sympy as sym

import propagate_ref as pr
from oracle.ref_numpy import _mag_expr

DPS, EPS = pr.DPS, pr.EPS

# Shampine (1986), the coefficients of theta^1 .. theta^4 of b_i(theta), as exact fractions
P_FR = [[Fr(1), Fr(-8048581381, 2820520608), Fr(8663915743, 2820520608), Fr(-12715105075, 11282082432)],
        [Fr(0), Fr(0), Fr(0), Fr(0)],
        [Fr(0), Fr(131558114200, 32700410799), Fr(-68118460800, 10900136933), Fr(87487479700, 32700410799)],
        [Fr(0), Fr(-1754552775, 470086768), Fr(14199869525, 1410260304), Fr(-10690763975, 1880347072)],
        [Fr(0), Fr(127303824393, 49829197408), Fr(-318862633887, 49829197408), Fr(701980252875, 199316789632)],
        [Fr(0), Fr(-282668133, 205662961), Fr(2019193451, 616988883), Fr(-1453857185, 822651844)],
        [Fr(0), Fr(40617522, 29380423), Fr(-110615467, 29380423), Fr(69997945, 29380423)]]
P = np.array([[float(v) for v in row] for row in P_FR])
P_ROWS = [i for i in range(7) if np.any(P[i] != 0.0)]
B7 = list(pr.B) + [0.0]                         # b_i of the seven stages (the seventh has none)


def b_theta(th):
    """[b_i(theta)] of the seven stages, float64, Horner from the highest power as the kernel does"""
    return [th * (P[i, 0] + th * (P[i, 1] + th * (P[i, 2] + th * P[i, 3]))) for i in range(7)]


def b_theta_mp(th):
    return [th * (mp.mpf(P[i, 0]) + th * (mp.mpf(P[i, 1]) + th * (mp.mpf(P[i, 2]) + th * mp.mpf(P[i, 3])))) for i in range(7)]


def query_plan(tau, tq):
    """(q_order [Q], node_q0 [N + 1]) of the host plan: a stable argsort of the queries; slot 0 the queries at tau_0,
    slot j >= 1 those in (tau_{j-1}, tau_j]; slot j is the sorted queries node_q0[j] .. node_q0[j + 1].  ``ValueError``
    for a query that is not finite or outside [tau_0, tau_{N-1}]."""
    tau, tq = np.asarray(tau, dtype=np.float64), np.asarray(tq, dtype=np.float64).reshape(-1)
    if not np.all(np.isfinite(tq)) or np.any(tq < tau[0]) or np.any(tq > tau[-1]):
        raise ValueError("a query is not finite or lies outside the phase")
    order = np.argsort(tq, kind="stable")
    slot = np.searchsorted(tau, tq[order], side="left")                    # the first node j with t <= tau_j
    return order, np.concatenate(([0], np.cumsum(np.bincount(slot, minlength=len(tau))))).astype(np.int64)


class DenseData(pr.PhaseData):
    """``propagate_ref.PhaseData`` with the phase's integrands (``P.g``)"""

    def __init__(self, P, *a):
        super().__init__(P, *a)
        self.n_q = P.n_q
        args = list(P.v) + list(P.consts)
        real = [{"re": lambda z: z, "im": lambda z: 0.0}, "math"]
        self._g64 = [sym.lambdify(args, e, modules="math") for e in P.g]
        self._gmp = [sym.lambdify(args, e, modules="mpmath") for e in P.g]
        self._gmag = [sym.lambdify(args, _mag_expr(e), modules=real) for e in P.g]

    def fg64(self, y, sl, c):
        u = [pr.legendre_f64(self.coef_u[b, sl], c) for b in range(self.n_u)]
        a = [float(v) for v in y] + u + self.w + self._cvals
        return np.array([pr._guard(fn, a) for fn in self._f64]), np.array([pr._guard(fn, a) for fn in self._g64])

    def gmp(self, y, u):
        a = list(y) + list(u) + [mp.mpf(v) for v in self.w] + [mp.mpf(float(v)) for v in self._cvals]
        return [mp.mpf(fn(*a)) for fn in self._gmp]

    def gmag(self, y, u):
        a = [float(v) for v in y] + [float(v) for v in u] + self.w + self._cvals
        return np.array([pr._guard(fn, a) for fn in self._gmag])

    def section(self, j):
        """(tau at the start of interval j's section, the section's width): what c is formed with"""
        k = int(self.sec_of[j])
        ta = self.tau[int(self.s[k])]
        return ta, self.tau[int(self.s[k + 1])] - ta


# ---- float64: the kernel's arithmetic -----------------------------------------------------------------------------
def stages_f64(d, y, I, sl, c, h, g, stage7):
    """(ynew, Inew, Ks, Gs) of one step; the seventh stage only with ``stage7``"""
    Ks, Gs, ys, Inew = [], [], y, I
    for s in range(7):
        if s:
            acc = np.zeros(d.n_y)
            for i, wgt in enumerate(pr.ROWS[s]):
                if wgt != 0.0:
                    acc = acc + wgt * Ks[i]
            ys = y + h * acc
        if s == 6:
            acc = np.zeros(d.n_q)
            for i, wgt in enumerate(pr.ROWS[6]):
                if wgt != 0.0:
                    acc = acc + wgt * Gs[i]
            Inew = I + h * acc
        if s < 6 or stage7:
            F, G = d.fg64(ys, sl, c if s == 0 else c + pr.CS[s] * h)
            Ks.append(g * F)
            Gs.append(g * G)
    return ys, Inew, Ks, Gs


def _err_f64(Ks, y, ynew, h, atol, rtol):
    """(max_a r_a, bad) of one group of components"""
    e = np.zeros(len(y))
    for i, wgt in enumerate(pr.E):
        if wgt != 0.0:
            e = e + wgt * Ks[i]
    with np.errstate(all="ignore"):
        r = np.abs(h * e) / (atol + rtol * np.maximum(np.abs(y), np.abs(ynew)))
    if not np.all(np.isfinite(r)):
        return 0.0, True
    return (float(np.max(r)) if len(y) else 0.0), False


def dense_f64(y, Ks, h, th):
    b = b_theta(th)
    acc = np.zeros(len(y))
    for i in P_ROWS:
        acc = acc + Ks[i] * b[i]
    return y + h * acc


def propagate_dense_f64(d, seg, tau_q=(), *, substeps=0, rtol=1e-9, atol=None, integral_atol=None, max_steps=4096):
    """dict(y_arrive [n_y][N], accepted [N], rejected [N], status [n_seg], q_arrive [n_q][N], y_dense [n_y][Q],
    q_dense [n_q][Q]) by the definition, in float64"""
    N = d.N
    tq = np.asarray(tau_q, dtype=np.float64).reshape(-1)
    order, q0 = query_plan(d.tau, tq)
    ts = tq[order]
    y_arr, q_arr = np.full((d.n_y, N), np.nan), np.full((d.n_q, N), np.nan)
    y_den, q_den = np.full((d.n_y, len(tq)), np.nan), np.full((d.n_q, len(tq)), np.nan)
    acc, rej = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    status = np.full(len(seg) - 1, -1, dtype=np.int64)
    y_arr[:, 0], q_arr[:, 0] = d.node_y[:, 0], 0.0
    for kq in range(q0[0], q0[1]):
        y_den[:, order[kq]], q_den[:, order[kq]] = d.node_y[:, 0], 0.0
    atol = None if atol is None else np.asarray(atol, dtype=np.float64)
    iatol = None if integral_atol is None else np.broadcast_to(np.asarray(integral_atol, dtype=np.float64), (d.n_q,))
    for i in range(len(seg) - 1):
        y, I = d.node_y[:, int(seg[i])].copy(), np.zeros(d.n_q)
        for j in range(int(seg[i]), int(seg[i + 1])):
            if status[i] >= 0:
                continue                                   # NaN arrivals and answers, zero counts
            _, sl, ca, cb, g = d.interval(j)
            ta, w = d.section(j)
            cur = [int(q0[j + 1])]
            kq1 = int(q0[j + 2])

            def cq_of(kq):
                return 2.0 * (ts[kq] - ta) / w - 1.0

            def answer(c, h, ce, y, I, ynew, Inew, Ks, Gs):
                while cur[0] < kq1:
                    cq = cq_of(cur[0])
                    if not cq <= ce:
                        break
                    col = order[cur[0]]
                    if cq == ce:
                        y_den[:, col], q_den[:, col] = ynew, Inew
                    else:
                        th = max((cq - c) / h, 0.0)
                        y_den[:, col], q_den[:, col] = dense_f64(y, Ks, h, th), dense_f64(I, Gs, h, th)
                    cur[0] += 1

            if substeps > 0:
                h = (cb - ca) / float(substeps)
                for q in range(substeps):
                    c = ca + float(q) * h
                    end = q == substeps - 1
                    hq, ce = (cb - c, cb) if end else (h, c + h)
                    hit = cur[0] < kq1 and cq_of(cur[0]) <= ce
                    ynew, Inew, Ks, Gs = stages_f64(d, y, I, sl, c, hq, g, hit)
                    if hit:
                        answer(c, hq, ce, y, I, ynew, Inew, Ks, Gs)
                    y, I = ynew, Inew
                acc[j + 1] = substeps
            else:
                c, h = ca, cb - ca
                last, after_reject, done = True, False, False
                while not done and acc[j + 1] + rej[j + 1] < max_steps:
                    ynew, Inew, Ks, Gs = stages_f64(d, y, I, sl, c, h, g, True)
                    err, bad = _err_f64(Ks, y, ynew, h, atol, rtol)
                    if iatol is not None:
                        e2, b2 = _err_f64(Gs, I, Inew, h, iatol, rtol)
                        err, bad = max(err, e2), bad or b2
                    factor = 0.2
                    if not bad:
                        factor = 5.0 if err == 0.0 else min(5.0, max(0.2, 0.9 * err ** -0.2))
                    if not bad and err <= 1.0:
                        acc[j + 1] += 1
                        ce = cb if last else c + h
                        answer(c, h, ce, y, I, ynew, Inew, Ks, Gs)
                        y, I, c = ynew, Inew, ce
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
            y_arr[:, j + 1], q_arr[:, j + 1] = y, I
    return dict(y_arrive=y_arr, accepted=acc, rejected=rej, status=status, q_arrive=q_arr, y_dense=y_den, q_dense=q_den)


# ---- 60 digits: the fixed mode --------------------------------------------------------------------------------------
class DenseFixedReference:
    """The fixed mode at 60 digits.  ``run(seg, m, tau_q)`` -> dict of (value, n, M) triples, float64 arrays of one
    shape each: ``y_arrive`` / ``q_arrive`` [.][N] (column 0: the start, n = 0), ``y_dense`` / ``q_dense`` [.][Q].  The
    steps are kept per (start node, m): a segment is a prefix of the chain from its start, and every query reads the
    step that answers it."""

    def __init__(self, data):
        self.d = data
        self._chain = {}

    def _step(self, y, I, sl, c, h, g):
        d = self.d
        hm, gm, cm = mp.mpf(h), mp.mpf(g), mp.mpf(c)
        Ks, Gs, Fm, Gm = [], [], [], []
        ys = y
        for s in range(7):
            if s:
                ys = [y[a] + hm * sum(mp.mpf(wgt) * Ks[i][a] for i, wgt in enumerate(pr.ROWS[s]) if wgt != 0.0) for a in range(d.n_y)]
            if s == 6:
                Inew = [I[m] + hm * sum(mp.mpf(wgt) * Gs[i][m] for i, wgt in enumerate(pr.ROWS[6]) if wgt != 0.0) for m in range(d.n_q)]
            cc = cm if s == 0 else cm + mp.mpf(pr.CS[s]) * hm
            u = [pr.legendre_mp([mp.mpf(float(v)) for v in d.coef_u[b, sl]], cc) for b in range(d.n_u)]
            Ks.append([gm * v for v in d.fmp(ys, u)])
            Gs.append([gm * v for v in d.gmp(ys, u)])
            Fm.append(d.fmag(ys, u).reshape(d.n_y))
            Gm.append(d.gmag(ys, u).reshape(d.n_q))
        return dict(c=c, h=h, g=g, y=y, I=I, ynew=ys, Inew=Inew, Ks=Ks, Gs=Gs, Fm=Fm, Gm=Gm)

    @staticmethod
    def _scale(st, b):
        """(M_y, M_q) of one step with the weights b [7]"""
        hg = abs(st["h"] * st["g"])
        My = np.array([abs(float(v)) for v in st["y"]]) + hg * sum(abs(b[i]) * st["Fm"][i] for i in range(7))
        Mq = np.array([abs(float(v)) for v in st["I"]]) + hg * sum(abs(b[i]) * st["Gm"][i] for i in range(7))
        return My, Mq

    def _extend(self, j0, m, upto):
        """the chain from node j0: per interval its m steps, and the running (M_y, M_q) behind every step"""
        d = self.d
        ch = self._chain.setdefault((j0, m), dict(steps=[], run=[], y=[mp.mpf(float(v)) for v in d.node_y[:, j0]],
                                                  I=[mp.mpf(0)] * d.n_q, My=np.zeros(d.n_y), Mq=np.zeros(d.n_q)))
        with mp.workdps(DPS):
            while len(ch["steps"]) < upto - j0:
                j = j0 + len(ch["steps"])
                _, sl, ca, cb, g = d.interval(j)
                h = (cb - ca) / float(m)
                steps, run = [], []
                for q in range(m):
                    c = ca + float(q) * h
                    st = self._step(ch["y"], ch["I"], sl, c, cb - c if q == m - 1 else h, g)
                    st["ce"] = cb if q == m - 1 else c + h
                    run.append((ch["My"], ch["Mq"]))                       # behind the steps before this one
                    My, Mq = self._scale(st, B7)
                    ch["My"], ch["Mq"] = np.maximum(ch["My"], My), np.maximum(ch["Mq"], Mq)
                    ch["y"], ch["I"] = st["ynew"], st["Inew"]
                    steps.append(st)
                run.append((ch["My"], ch["Mq"]))                           # ... and behind the interval's last
                ch["steps"].append(steps)
                ch["run"].append(run)
        return ch

    def run(self, seg, m, tau_q=()):
        d = self.d
        tq = np.asarray(tau_q, dtype=np.float64).reshape(-1)
        order, q0 = query_plan(d.tau, tq)
        ts, Q, N = tq[order], len(tq), d.N
        z = lambda r, c: [np.zeros((r, c)), np.zeros(c), np.zeros((r, c))]   # noqa: E731
        out = dict(y_arrive=z(d.n_y, N), q_arrive=z(d.n_q, N), y_dense=z(d.n_y, Q), q_dense=z(d.n_q, Q))
        out["y_arrive"][0][:, 0] = d.node_y[:, 0]
        for kq in range(q0[0], q0[1]):
            out["y_dense"][0][:, order[kq]] = d.node_y[:, 0]

        def put(name, col, val, n, M):
            out[name][0][:, col], out[name][1][col], out[name][2][:, col] = [float(v) for v in val], n, M

        with mp.workdps(DPS):
            for i in range(len(seg) - 1):
                j0, j1 = int(seg[i]), int(seg[i + 1])
                ch = self._extend(j0, m, j1)
                for j in range(j0, j1):
                    steps, run = ch["steps"][j - j0], ch["run"][j - j0]
                    n0 = m * (j - j0)
                    put("y_arrive", j + 1, steps[-1]["ynew"], n0 + m, run[m][0])
                    put("q_arrive", j + 1, steps[-1]["Inew"], n0 + m, run[m][1])
                    ta, w = d.section(j)
                    kq = int(q0[j + 1])
                    for q, st in enumerate(steps):
                        while kq < q0[j + 2]:
                            cq = 2.0 * (ts[kq] - ta) / w - 1.0
                            if not cq <= st["ce"]:
                                break
                            col = order[kq]
                            if cq == st["ce"]:
                                put("y_dense", col, st["ynew"], n0 + q + 1, run[q + 1][0])
                                put("q_dense", col, st["Inew"], n0 + q + 1, run[q + 1][1])
                            else:
                                th = max((mp.mpf(cq) - mp.mpf(st["c"])) / mp.mpf(st["h"]), mp.mpf(0))
                                b, hm = b_theta_mp(th), mp.mpf(st["h"])
                                yv = [st["y"][a] + hm * sum(st["Ks"][ii][a] * b[ii] for ii in P_ROWS) for a in range(d.n_y)]
                                qv = [st["I"][a] + hm * sum(st["Gs"][ii][a] * b[ii] for ii in P_ROWS) for a in range(d.n_q)]
                                My, Mq = self._scale(st, [float(v) for v in b])
                                put("y_dense", col, yv, n0 + q + 1, np.maximum(run[q][0], My))
                                put("q_dense", col, qv, n0 + q + 1, np.maximum(run[q][1], Mq))
                            kq += 1
                    assert kq == q0[j + 2], "a query of the interval found no step"
        return out


def parity_bound(ref, n, M):
    """1e-10 |ref| + 64 eps n M, entry by entry (n per column)"""
    return 1e-10 * np.abs(ref) + 64 * EPS * np.asarray(n)[None, :] * M


def sample_queries(d, per_interval=2, seed=0):
    """queries for the tests of a phase: every node, ``per_interval`` points inside every node interval, one node twice,
    the whole shuffled"""
    rng = np.random.default_rng(seed)
    inner = [d.tau[j] + rng.uniform(0.05, 0.95, per_interval) * (d.tau[j + 1] - d.tau[j]) for j in range(d.N - 1)]
    tq = np.concatenate([d.tau, np.concatenate(inner), d.tau[[d.N // 2]], inner[0][:1]])
    return rng.permutation(tq)



def integral_adaptive_bound(seg, truth_I, accepted, integral_atol, rtol):
    """a (integral_atol_m + rtol max |I_m|) per entry [n_q][N]: a the accepted steps in the segment up to the node, max
    |I_m| over the truth from the segment's start to the node (error-per-step control, each step's share added up)"""
    truth_I = np.asarray(truth_I)
    b = np.zeros_like(truth_I)
    ia = np.broadcast_to(np.asarray(integral_atol, dtype=np.float64), (truth_I.shape[0],))
    for i in range(len(seg) - 1):
        j0, j1 = int(seg[i]), int(seg[i + 1])
        for j in range(j0 + 1, j1 + 1):
            a = float(np.sum(accepted[j0 + 1:j + 1]))
            b[:, j] = a * (ia + rtol * np.max(np.abs(truth_I[:, j0 + 1:j + 1]), axis=1))
    return b


# ---- the end-to-end figures -------------------------------------------------------------------------------------------
def section_samples(d, m=33):
    """m equispaced points c in [-1, 1] of every section (its two ends included) as tau [K m]"""
    c = np.linspace(-1.0, 1.0, m)
    edges = d.tau[d.s]
    tq = edges[:-1, None] + 0.5 * (c[None, :] + 1.0) * (edges[1:, None] - edges[:-1, None])
    tq[:, 0], tq[:, -1] = edges[:-1], edges[1:]
    return tq.reshape(-1)


def sample_y_f64(d, method, tq):
    """the state interpolant of the solution at ``tq``, float64: y(c) = y(tau_k) + stretch (w_k / 2) int_{-1}^{c}
    ydot, ydot's Legendre coefficients the section's C_dy table times f at its nodes; a section boundary is read from
    the section on its left (the interpolant is continuous up to the NLP's defect there)"""
    from numpy.polynomial import legendre as L
    from pycollo_amd.solution import solution_tables
    out = np.empty((d.n_y, len(tq)))
    k_of = np.clip(np.searchsorted(d.tau[d.s], tq, side="left") - 1, 0, d.K - 1)
    for k in range(d.K):
        sk, n = int(d.s[k]), int(d.s[k + 1] - d.s[k] + 1)
        _, sl, _, _, g = d.interval(sk)
        ta, w = d.section(sk)
        cn = [2.0 * (d.tau[sk + i] - ta) / w - 1.0 for i in range(n)]
        F = np.array([d.f64(d.node_y[:, sk + i], sl, cn[i]) for i in range(n)])            # [n][n_y]
        coef = solution_tables(method, n)[0] @ F
        use = np.nonzero(k_of == k)[0]
        c = 2.0 * (tq[use] - ta) / w - 1.0
        for a in range(d.n_y):
            out[a, use] = d.node_y[a, sk] + g * L.legval(c, L.legint(coef[:, a], lbnd=-1.0))
    return out


def end_to_end_figures(d, method, V, rtol=1e-10):
    """(|integral_defect| of the open-loop pass [n_q], of the per-node restart [n_q], the largest |y_dense - y(t)| over 33
    points per section of the open-loop pass) by the float64 restatement"""
    q_nlp = np.array(d.w[:d.n_q])
    tq = section_samples(d)
    fig = []
    for restart in ("phase", "nodes"):
        seg = pr.segments(restart, d.s, d.N)
        r = propagate_dense_f64(d, seg, tq if restart == "phase" else (), rtol=rtol, atol=rtol * np.asarray(V))
        assert np.all(r["status"] == -1)
        total = np.zeros(d.n_q)
        for j in seg[1:]:
            total = total + r["q_arrive"][:, int(j)]
        fig.append(np.abs(total - q_nlp))
        if restart == "phase":
            gap = float(np.max(np.abs(r["y_dense"] - sample_y_f64(d, method, tq))))
    return fig[0], fig[1], gap
