"""The tests' own restatement of the path and bound multipliers, the gradients of the augmented Hamiltonian and the
dual-residual identity (pycollo_amd/solution.py, csrc/pc_solution.hpp: pc_sol_multipliers_p<i>,
pc_sol_sample_optimality_p<i>).  No GPU and no engine: everything is formed from an ``OracleNlp``, the golden
quadrature tables and the three vectors x~, lam~, z~.

Node quantities are formed in ``np.longdouble``; the model's partials are ``OracleNlp``'s ``P.dF`` (float64 callables
of SymPy derivatives), their magnitudes ``P.dF_mag``.  Interpolants and their derivatives are formed in 60-digit mpmath
from given node values, the way ``test_gpu_costate.Case.interpolant`` forms the costates'.

Notation: N nodes, section k has n_k nodes from node s_k, h_k its width in tau, omega_j the node weight from the last
rows of the A tables, stretch = (tF - t0) / 2, w the objective scaling, W / V the constraint / variable scaling.
"""
import mpmath as mp
import numpy as np

LD = np.longdouble
DPS = 60


class NodeReference:
    """Per phase of an ``OracleNlp`` at (x~, lam~, z~): ``omega`` [N]; ``p``, ``mag_p`` [n_y][N]; ``nu`` [n_q];
    ``mu``, ``mag_mu`` [n_p][N]; ``zeta``, ``mag_zeta`` [n_z][N] and ``end_z`` [n_y][2] (``None`` without z~);
    ``H_z``, ``mag_H`` [n_z][N]; ``D`` [n_y][N]; ``Lam`` [n_y][N - 1]; ``stretch``.  NaN where the definition says NaN."""

    def __init__(self, ora, tables, x, lam, z, ip, w_J=None):
        P = ora.P[ip]
        mesh, N = P.mesh, P.N
        w_J = LD(ora.w_J if w_J is None else w_J)
        W, V = ora.W_ocp.astype(LD), ora.V_ocp.astype(LD)
        lam = np.asarray(lam).astype(LD)
        self.N, self.n_y, self.n_u, self.n_p, self.n_q = N, P.n_y, P.n_u, P.n_p, P.n_q
        n_y, n_z, n_p, n_q = P.n_y, P.n_z, P.n_p, P.n_q
        Lam = np.array([W[P.oc + a] * lam[P.c_off + a * (N - 1):P.c_off + (a + 1) * (N - 1)] / w_J
                        for a in range(n_y)], dtype=LD).reshape(n_y, N - 1)
        self.Lam = Lam
        self.nu = np.array([-(W[P.oc + n_y + n_p + m] * lam[P.c_int + m] / w_J) for m in range(n_q)], dtype=LD)
        omega = np.zeros(N, dtype=LD)
        for k in range(mesh.K):
            s, n = int(mesh.bnd[k]), int(mesh.nodes[k])
            omega[s:s + n] += LD(mesh.h[k]) * tables.A(n)[n - 2].astype(LD)
        self.omega = omega
        wt = self.weighted = omega != 0
        I = mesh.I_mat.toarray().astype(LD)
        p, mag_p = np.empty((n_y, N), dtype=LD), np.empty((n_y, N), dtype=LD)
        p[:, wt], mag_p[:, wt] = (Lam @ I)[:, wt] / omega[wt], (np.abs(Lam) @ np.abs(I))[:, wt] / omega[wt]
        p[:, ~wt], mag_p[:, ~wt] = Lam[:, [N - 2]], np.abs(Lam[:, [N - 2]])
        self.p, self.mag_p = p, mag_p
        z_o, _, stretch, _, w_par = ora._unpack(P, np.asarray(x, float))
        self.stretch = stretch = LD(stretch)
        den = np.where(wt, stretch * omega, LD(1))
        nan = LD(np.nan)
        # path multipliers
        mu = np.empty((n_p, N), dtype=LD)
        for i in range(n_p):
            mu[i] = W[P.oc + n_y + i] * lam[P.c_path + i * N:P.c_path + (i + 1) * N] / w_J / den
        mu[:, ~wt] = nan
        self.mu, self.mag_mu = mu, np.abs(mu)
        # bound multipliers
        self.zeta = self.mag_zeta = self.end_z = None
        if z is not None:
            z = np.asarray(z).astype(LD)
            zs = np.array([z[P.x_off + b * N:P.x_off + (b + 1) * N] / (w_J * V[P.ox + b]) for b in range(n_z)],
                          dtype=LD).reshape(n_z, N)
            zeta = zs / den
            zeta[:, ~wt] = nan
            zeta[:n_y, 0] = zeta[:n_y, N - 1] = 0
            self.zeta, self.mag_zeta = zeta, np.abs(zeta)
            self.end_z = zs[:n_y][:, [0, N - 1]].copy()
        # gradients of the augmented Hamiltonian from the oracle's partials, mult = [p | mu | nu]
        ora._mag_fns()
        a = ora._args(P, z_o, w_par)
        # the NLP's integral rows weigh integrand m at node j with mesh.w[j]: rho_j nu_m is its weight in H_z
        rho = np.where(wt, mesh.w.astype(LD) / np.where(wt, omega, LD(1)), LD(0))
        self.rho = rho
        mult = np.concatenate([p, mu, self.nu[:, None] * rho[None, :]], axis=0) if (n_y + n_p + n_q) else np.zeros((0, N), dtype=LD)
        H_z, mag_H = np.zeros((n_z, N), dtype=LD), np.zeros((n_z, N), dtype=LD)
        for (r, cvar), (_, dfn) in P.dF.items():
            if cvar >= n_z:
                continue
            d = np.broadcast_to(np.asarray(dfn(*a), float), (N,)).astype(LD)
            dm = np.abs(np.broadcast_to(np.asarray(P.dF_mag[(r, cvar)](*a), float), (N,))).astype(LD)
            H_z[cvar] += mult[r] * d
            mag_H[cvar] += np.abs(mult[r]) * dm
        H_z[:, ~wt] = nan
        self.H_z, self.mag_H = H_z, mag_H
        # the discrete defect term
        D = np.zeros((n_y, N), dtype=LD)
        D[:, 1:] -= Lam
        for k in range(mesh.K):
            s, n = int(mesh.bnd[k]), int(mesh.nodes[k])
            D[:, s] += np.sum(Lam[:, s:s + n - 1], axis=1)
        self.D = D

    def costate_defect(self):
        """D_a / (stretch omega) + H_y (+ zeta_y) [n_y][N]; NaN at nodes 0, N - 1 and the unweighted node"""
        out = np.full((self.n_y, self.N), np.nan, dtype=LD)
        use = self.weighted.copy()
        use[0] = use[-1] = False
        out[:, use] = self.D[:, use] / (self.stretch * self.omega[use]) + self.H_z[:self.n_y, use]
        if self.zeta is not None:
            out[:, use] += self.zeta[:self.n_y, use]
        return out


def identity_sides(ora, tables, x, lam, z, w_J):
    """The dual residual of the scaled NLP, r~ = grad J~ + G~^T lam~ + z~, against the definition's right-hand side.
    Returns ``(cols, lhs, rhs, scale)``: the x columns of every control at the weighted nodes and of every state at the
    interior weighted nodes of every phase, the two sides there (float64 lhs from the oracle's own G~ and grad J~;
    rhs from :class:`NodeReference`) and ``scale`` = (|G~|^T |lam~| + |z~|) from ``G_mag``."""
    import scipy.sparse as sp
    x, lam, z = (np.asarray(v, float) for v in (x, lam, z))
    rows, cols_G = ora.G_structure()
    G = sp.coo_matrix((ora.G(x), (rows, cols_G)), shape=(ora.num_c, ora.num_x)).tocsr()
    Gm = sp.coo_matrix((ora.G_mag(x), (rows, cols_G)), shape=(ora.num_c, ora.num_x)).tocsr()
    r = ora.grad_J(x) + G.T @ lam + z
    scale = Gm.T @ np.abs(lam) + np.abs(z)
    V = ora.V_ocp.astype(LD)
    cols, rhs = [], []
    for ip, P in enumerate(ora.P):
        ref = NodeReference(ora, tables, x, lam, z, ip, w_J=w_J)
        N, n_y = P.N, P.n_y
        for b in range(P.n_z):
            fac = LD(w_J) * V[P.ox + b]
            for j in range(N):
                if not ref.weighted[j] or (b < n_y and j in (0, N - 1)):
                    continue
                val = ref.stretch * ref.omega[j] * (ref.H_z[b, j] + ref.zeta[b, j])
                if b < n_y:
                    val = val + ref.D[b, j]
                cols.append(P.x_off + b * N + j)
                rhs.append(fac * val)
    cols = np.array(cols, dtype=np.int64)
    return cols, r[cols], np.array(rhs, dtype=LD).astype(float), scale[cols]


# ---- exact interpolants of given node values -----------------------------------------------------------------
def _legendre(n, x):
    P = [mp.mpf(1), x]
    for m in range(1, n):
        P.append(((2 * m + 1) * x * P[m] - m * P[m - 1]) / (m + 1))
    return P[:n]


def _legendre_d(n, x):
    """P_m'(x), m < n, by P_(m+1)' = P_(m-1)' + (2m + 1) P_m"""
    P = _legendre(n + 1, x)
    d = [mp.mpf(0), mp.mpf(1)]
    for m in range(1, n):
        d.append(d[m - 1] + (2 * m + 1) * P[m])
    return d[:n]


class SectionInterpolant:
    """The degree n - 1 Legendre series through ``values`` [n_var][n] of one section, formed with the exact table
    ``C`` (an mpmath n x n matrix of ``pycollo_amd.solution.exact_tables``): ``value(c)`` and ``derivative(c)`` (d/dc)
    return float arrays [n_var]; ``mag`` [n_var] = sum_k sum_i |C_ki| |v_i|."""

    def __init__(self, C, values):
        values = np.asarray(values, float)
        self.n = n = values.shape[1]
        absC = np.array([[float(abs(C[i, j])) for j in range(n)] for i in range(n)])
        with mp.workdps(DPS):
            self.e = [C * mp.matrix([mp.mpf(float(v)) for v in row]) for row in values]
        self.mag = np.array([float(np.sum(absC @ np.abs(row))) for row in values])

    def value(self, c):
        with mp.workdps(DPS):
            P = _legendre(self.n, mp.mpf(float(c)))
            return np.array([float(sum(e[m] * P[m] for m in range(self.n))) for e in self.e])

    def derivative(self, c):
        with mp.workdps(DPS):
            d = _legendre_d(self.n, mp.mpf(float(c)))
            return np.array([float(sum(e[m] * d[m] for m in range(self.n))) for e in self.e])


# ---- the host solve with its multipliers, and the costate residual of one section on the host ----------------
def cpu_solve_with_multipliers(prob, tables, tol=1e-10):
    """``propagate_ref.cpu_solve`` (the host interior-point solver on the oracle's functions), returning
    ``(oracle, IpmResult)``: that helper hands back the point only, so the solver's ``solve`` is wrapped for the call
    to keep the result with its ``lam``, ``zl`` and ``zu``.  This leans on how ``cpu_solve`` is written -- it builds a
    ``pycollo_amd.ipm.InteriorPointSolver`` and calls its ``solve`` once; should that change, the assertion below says
    so instead of returning another solve's result."""
    import propagate_ref
    from pycollo_amd import ipm
    kept = {}
    solve = ipm.InteriorPointSolver.solve

    def keeping(self, x0):
        kept["res"] = solve(self, x0)
        return kept["res"]

    ipm.InteriorPointSolver.solve = keeping
    try:
        ora, x = propagate_ref.cpu_solve(prob, tables, tol=tol)
    finally:
        ipm.InteriorPointSolver.solve = solve
    assert "res" in kept and np.array_equal(np.asarray(kept["res"].x, float), x), \
        "propagate_ref.cpu_solve no longer solves through InteriorPointSolver.solve: the multipliers were not captured"
    return ora, kept["res"]


def host_section_costate_residual(ora, tables, x, lam, z, k, samples=33, ip=0):
    """max |dp/dt + H_y + zeta_y| over ``samples`` equispaced points c in [-1, 1] of section k of a Lobatto phase,
    formed on the host as the sampling kernel defines it: p, u and zeta_y are the degree n - 1 interpolants of the
    section's node values, y the integrated form of the interpolant of f at the nodes, H_y from the oracle's partials at
    (y(c), u(c)) with p(c), mu(c) and rho nu."""
    from numpy.polynomial import legendre as L
    from pycollo_amd.solution import solution_tables
    P = ora.P[ip]
    mesh, n_y, n_z = P.mesh, P.n_y, P.n_z
    assert k < mesh.K - 1, "the phase's last section forms mu and zeta with another table"
    ref = NodeReference(ora, tables, x, lam, z, ip)
    s, n = int(mesh.bnd[k]), int(mesh.nodes[k])
    Cd, Cu = solution_tables("lobatto", n)
    zo, _, stretch, _, w_par = ora._unpack(P, np.asarray(x, float))
    f_nodes = np.array([np.broadcast_to(np.asarray(fn(*ora._args(P, zo, w_par)), float), (P.N,)) for fn in P.F_fn[:n_y]])
    sl = slice(s, s + n)
    c = np.linspace(-1.0, 1.0, samples)
    h = float(mesh.h[k])
    ev = lambda vals: L.legval(c, Cu @ vals)   # noqa: E731
    y = np.array([zo[a, s] + stretch * 0.5 * h * L.legval(c, L.legint(Cd @ f_nodes[a, sl], lbnd=-1.0)) for a in range(n_y)])
    u = np.array([ev(zo[b, sl]) for b in range(n_y, n_z)])
    p = np.array([ev(ref.p[a, sl].astype(float)) for a in range(n_y)])
    dp = np.array([L.legval(c, L.legder(Cu @ ref.p[a, sl].astype(float))) * 2.0 / (h * stretch) for a in range(n_y)])
    mu = np.array([ev(ref.mu[i, sl].astype(float)) for i in range(P.n_p)]).reshape(P.n_p, samples)
    zeta_y = np.array([ev(ref.zeta[a, sl].astype(float)) for a in range(n_y)])
    rho = float(ref.rho[s + 1])
    mult = list(p) + list(mu) + [np.full(samples, rho * float(v)) for v in ref.nu]
    args = list(y) + list(u) + [np.full(samples, w_par[i]) for i in range(P.n_w)]
    H_y = np.zeros((n_y, samples))
    for (r, cvar), (_, dfn) in P.dF.items():
        if cvar < n_y:
            H_y[cvar] += mult[r] * np.broadcast_to(np.asarray(dfn(*args), float), (samples,))
    return float(np.max(np.abs(dp + H_y + zeta_y)))
