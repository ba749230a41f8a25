"""CPU oracle for the ph mesh-error estimate (TEST INFRASTRUCTURE ONLY).

NumPy restatement of ``PattersonRaoMeshRefinement.mesh_error`` / ``phase_mesh_error``
(pycollo/mesh_refinement.py:63-240) together with the per-section polynomial fits it consumes
(pycollo/solution/solution_abc.py:60-107, Lobatto branch):

1. f at the solution nodes (``dy_iter_callable``, pycollo/solution/casadi_solution.py:71);
2. per section and state a degree n_k-1 Legendre fit of (T/2) f, integrated from the section start with
   constant y[start]; per control a degree n_k-1 polynomial fit (solution_abc.py:70-100);
3. the "ph mesh": same sections, n_k + 1 nodes each (mesh_refinement.py:76-88); section boundary values are
   the solution's, interior values come from the fits (mesh_refinement.py:160-196);
4. f on the ph mesh, ``stretch * I_ph f`` added to the section start value, compared with the fitted states;
   relative to 1 + (1 + max|Y_k|) (sic, mesh_refinement.py:211,221-223); section maximum over states/nodes.

The fits are the reference's polynomials in a well-conditioned form: the reference maps every section onto the window
[0, 1] (``Legendre.fit(..., window=[0, 1])``, ``Polynomial.fit(..., window=[0, 1])``), where neither basis is
orthogonal and the least-squares fit loses digits with the order -- against the exact ``mesh_error_mp`` below that
form is 22 times its rounding bound at order 10 and 1.5e7 times at order 19 (brachistochrone, K = 3, on a
trajectory).  A degree n - 1 fit through n nodes is THE interpolant whatever the basis, so the oracle fits Legendre
series on [-1, 1] for states and controls alike, in the section's own coordinate (the quadrature points themselves,
not differences of tau, which cancel on a short section far from tau = 0: eps |tau| / h of the node positions is lost,
a factor 2000 on a section of width 5e-4) and integrates from the section start explicitly (``lbnd``).
"""
from __future__ import annotations

import numpy as np

from .ref_numpy import OracleMesh, OracleNlp


def mesh_error(ora: OracleNlp, xt):
    """Returns per phase (absolute errors [K][n_y][max m_k], max relative error [K])."""
    xt = np.asarray(xt, float)
    out = []
    for P in ora.P:
        mesh = P.mesh
        z, q, stretch, _, w = ora._unpack(P, xt)
        N, K = mesh.N, mesh.K
        y, u = z[:P.n_y], z[P.n_y:]
        a = ora._args(P, z, w)
        dy = np.array([P.F_fn[i](*a) for i in range(P.n_y)])
        tau = mesh.tau
        ph = OracleMesh(ora.tables, mesh.h / mesh.h.sum(), mesh.nodes + 1)
        y_ph = np.zeros((P.n_y, ph.N))
        u_ph = np.zeros((P.n_u, ph.N))
        y_ph[:, ph.bnd] = y[:, mesh.bnd]
        u_ph[:, ph.bnd] = u[:, mesh.bnd]
        for k in range(K):
            i0, i1 = mesh.bnd[k], mesh.bnd[k + 1]
            n_k = int(mesh.nodes[k])
            x_k, x_ph = ora.tables.points(n_k), ora.tables.points(n_k + 1)[1:-1]     # the section's own [-1, 1]
            sl = slice(ph.bnd[k] + 1, ph.bnd[k + 1])
            for iy in range(P.n_y):
                dpoly = np.polynomial.Legendre.fit(x_k, dy[iy, i0:i1 + 1] * stretch, deg=n_k - 1, domain=[-1, 1])
                y_ph[iy, sl] = y[iy, i0] + 0.5 * mesh.h[k] * dpoly.integ(lbnd=-1)(x_ph)
            for iu in range(P.n_u):
                upoly = np.polynomial.Legendre.fit(x_k, u[iu, i0:i1 + 1], deg=n_k - 1, domain=[-1, 1])
                u_ph[iu, sl] = upoly(x_ph)
        zp = np.vstack([y_ph, u_ph])
        ap = [zp[i] for i in range(P.n_z)] + [np.full(ph.N, w[i]) for i in range(P.n_w)]
        dy_ph = np.array([P.F_fn[i](*ap) for i in range(P.n_y)])           # [n_y][N_ph]
        I_dy = stretch * (ph.I_mat @ dy_ph.T)                               # [N_ph - 1][n_y]
        mmax = int(ph.nodes.max()) - 1
        abs_err = np.zeros((K, P.n_y, mmax))
        max_rel = np.zeros(K)
        for k in range(K):
            i0, m = ph.bnd[k], ph.nodes[k] - 1
            Y_ph = (y_ph[:, i0] + I_dy[i0:i0 + m]).T                         # [n_y][m]
            Y = y_ph[:, i0 + 1:i0 + 1 + m]
            err = np.abs(Y_ph - Y)
            abs_err[k, :, :m] = err
            scale = np.max(np.abs(Y), axis=1) + 1
            max_rel[k] = np.max(err / (1 + scale)[:, None])
        out.append((abs_err, max_rel))
    return out


# ------------------------------------------------------------------------------------------------
# exact restatement (mpmath) and the running-error magnitude of every entry
# ------------------------------------------------------------------------------------------------
_MP_FN_CACHE: dict = {}      # per model: f as mpmath callables
_MP_TAB_CACHE: dict = {}     # per (points, dps): exact Lagrange tables


def _mp_f(P):
    import sympy as sym
    fns = _MP_FN_CACHE.get(P.key)
    if fns is None:
        csyms = list(P.consts)
        # one callable for all state equations: they share most of their subexpressions
        fns = _MP_FN_CACHE[P.key] = sym.lambdify(list(P.v) + csyms, list(P.f), modules="mpmath", cse=True)
    return fns


_F_MAG_CACHE: dict = {}


def _f_mag(P):
    """Magnitude companions (``_mag_expr``) of the state equations alone: ``OracleNlp._mag_fns`` also builds those of
    every first and second partial, which this estimate does not use and large models pay tens of seconds for."""
    from .ref_numpy import _lam, _mag_expr
    if P.key not in _F_MAG_CACHE:
        _F_MAG_CACHE[P.key] = [_lam(P.v, _mag_expr(e), P.consts) for e in P.f]
    return _F_MAG_CACHE[P.key]


def lagrange_tables_mp(pts, pts_ph, dps=40):
    """Exact (to ``dps`` digits) tables of the interpolant through the abscissae c = (pts + 1) / 2, at cp =
    (pts_ph + 1) / 2 (``pts``, ``pts_ph``: fp64 points on [-1, 1], taken as exact): B[j][i] = int_0^cp_j l_i,
    E[j][i] = l_i(cp_j), l_i the Lagrange basis polynomial of node i.  The basis is expanded into monomials by
    polynomial multiplication and integrated term by term; the expansion runs with 30 guard digits."""
    import mpmath as mp
    key = (tuple(float(v) for v in pts), tuple(float(v) for v in pts_ph), dps)
    got = _MP_TAB_CACHE.get(key)
    if got is not None:
        return got
    with mp.workdps(dps + 30):
        c = [(mp.mpf(float(v)) + 1) / 2 for v in pts]
        cp = [(mp.mpf(float(v)) + 1) / 2 for v in pts_ph]
        n = len(c)
        B = [[None] * n for _ in cp]
        E = [[None] * n for _ in cp]
        for i in range(n):
            coef = [mp.mpf(1)]                     # ascending monomial coefficients of prod_{m != i} (x - c_m)
            den = mp.mpf(1)
            for m in range(n):
                if m == i:
                    continue
                new = [mp.mpf(0)] * (len(coef) + 1)
                for d, a in enumerate(coef):
                    new[d + 1] += a
                    new[d] -= a * c[m]
                coef = new
                den *= c[i] - c[m]
            for j, x in enumerate(cp):
                val = integ = mp.mpf(0)
                for d in range(len(coef) - 1, -1, -1):          # Horner, value and antiderivative
                    val = val * x + coef[d]
                    integ = integ * x + coef[d] / (d + 1)
                E[j][i] = val / den
                B[j][i] = integ * x / den
    _MP_TAB_CACHE[key] = (B, E)
    return B, E


def mesh_error_mp(ora: OracleNlp, xt, dps=40):
    """The estimate of ``mesh_error`` restated exactly, with a first-order running-error magnitude for every entry.

    Taken as exact: the float64 x~, V, r, the section widths of the oracle's mesh, the golden quadrature points of
    orders n and n + 1 and the golden A(n + 1).  Everything else is computed with ``dps`` digits: the affine
    unscaling, f (the oracle's own expressions, lambdified onto mpmath), the degree n - 1 interpolants of
    stretch f and of u in Lagrange form (the former integrated exactly from the section start), f on the ph mesh and
    y_start + stretch h A f.  Independent of ``ph_tables`` and of the float64 oracle's polynomial fits.

    Per phase a dict of float64 arrays: ``Y_ph``, ``y_ph``, ``abs_err`` [K][n_y][max n_k] (node j = 1..n_k of the
    ph mesh in column j - 1), ``max_rel`` [K], ``max_abs`` [K][n_y], and the magnitudes ``mag_abs`` (entry-wise),
    ``mag_max_abs``, ``mag_max_rel``: eps times a magnitude bounds, to first order and up to a small factor, what
    any fp64 evaluation order of the same formulas can differ from the exact value by.  With mag f the oracle's F_mag:
        mag y_ph = |y_start| + |stretch h| sum|B| mag f          mag u_ph = sum|E||u|
        mag f_ph = F_mag + sum_b |df/dz_b| mag z_ph,b           (the rounding of the interpolated arguments, through f)
        mag err  = |y_start| + |stretch h| sum|A| mag f_ph + mag y_ph
    A maximum moves by no more than its entries do, so a section maximum carries the largest magnitude of its
    entries; the relative error err / (2 + max|y_ph|) adds the rounding of its denominator, err mag y_ph / (2 + max|y_ph|)^2."""
    import mpmath as mp
    xt = np.asarray(xt, float)
    tables = ora.tables
    out = []
    with mp.workdps(dps):
        F = lambda v: mp.mpf(float(v))
        V, r = ora.V_ocp, ora.r_ocp
        for P in ora.P:
            mesh, N, K, n_y, n_u, n_z = P.mesh, P.N, P.mesh.K, P.n_y, P.n_u, P.n_z
            fns = _mp_f(P)
            F_mag = _f_mag(P)
            cvals = [F(v) for v in P.consts.values()]
            # 1. affine unscaling, exact
            unscale = lambda o, x: F(V[o]) * F(x) + F(r[o])
            z = [[unscale(P.ox + b, xt[P.x_off + b * N + i]) for i in range(N)] for b in range(n_z)]
            qv = [unscale(P.ox + n_z + l, xt[P.q_off + l]) for l in range(P.n_q)]
            to = P.ox + n_z + P.n_q
            t, tfree, j = [], [], 0
            for e in (0, 1):
                if P.t_free[e]:
                    t.append(unscale(to + j, xt[P.t_off + j]))
                    tfree.append(t[-1])
                    j += 1
                else:
                    t.append(F(P.t_fixed[e]))
            sv = [F(V[ora.ocp_s + l]) * F(xt[ora.s_off + l]) + F(r[ora.ocp_s + l]) for l in range(ora.n_s)]
            w = qv + tfree + sv
            stretch = (t[1] - t[0]) / 2
            f_at = lambda zcol: fns(*zcol, *w, *cvals)
            # float64 companions for the magnitudes
            z64, _, st64, _, w64 = ora._unpack(P, xt)
            a64 = ora._args(P, z64, w64)
            magf = np.array([np.abs(F_mag[i](*a64)) for i in range(n_y)]).reshape(n_y, N)
            # 2. f at the solution nodes
            fs = [f_at([z[b][i] for b in range(n_z)]) for i in range(N)]            # [N][n_y]
            mmax = int(mesh.nodes.max())
            shape = (K, n_y, mmax)
            Yph, yph, aerr, mag_abs = (np.zeros(shape) for _ in range(4))
            max_rel, mag_rel = np.zeros(K), np.zeros(K)
            max_abs, mag_max_abs = np.zeros((K, n_y)), np.zeros((K, n_y))
            for k in range(K):
                n, i0 = int(mesh.nodes[k]), int(mesh.bnd[k])
                h = F(mesh.h[k])
                B, E = lagrange_tables_mp(tables.points(n), tables.points(n + 1)[1:-1], dps)
                A = tables.A(n + 1)
                Bm = np.array([[abs(float(v)) for v in row] for row in B]).reshape(n - 1, n)
                Em = np.array([[abs(float(v)) for v in row] for row in E]).reshape(n - 1, n)
                sh = abs(float(stretch * h))
                # 3.-5. the ph nodes: boundaries from the solution, interior from the interpolants
                zp = [[None] * (n + 1) for _ in range(n_z)]
                mag_z = np.zeros((n_z, n + 1))
                for b in range(n_z):
                    zp[b][0], zp[b][n] = z[b][i0], z[b][i0 + n - 1]
                    mag_z[b, 0], mag_z[b, n] = abs(z64[b, i0]), abs(z64[b, i0 + n - 1])
                for jn in range(1, n):
                    for a in range(n_y):
                        zp[a][jn] = z[a][i0] + h * mp.fsum(B[jn - 1][i] * (stretch * fs[i0 + i][a]) for i in range(n))
                    for b in range(n_y, n_z):
                        zp[b][jn] = mp.fsum(E[jn - 1][i] * z[b][i0 + i] for i in range(n))
                mag_z[:n_y, 1:n] = np.abs(z64[:n_y, i0])[:, None] + sh * (magf[:, i0:i0 + n] @ Bm.T)
                mag_z[n_y:, 1:n] = np.abs(z64[n_y:, i0:i0 + n]) @ Em.T
                # 6. f on the ph mesh, and its magnitude with the arguments' rounding propagated through df/dz
                fp = [f_at([zp[b][jn] for b in range(n_z)]) for jn in range(n + 1)]     # [n + 1][n_y]
                zp64 = np.array([[float(v) for v in row] for row in zp]).reshape(n_z, n + 1)
                ap64 = [zp64[b] for b in range(n_z)] + [np.full(n + 1, w64[i]) for i in range(P.n_w)]
                mag_fp = np.array([np.abs(F_mag[a](*ap64)) for a in range(n_y)]).reshape(n_y, n + 1)
                for (row, col), (_, dfn) in P.dF.items():
                    if row < n_y and col < n_z:
                        mag_fp[row] += np.abs(dfn(*ap64)) * mag_z[col]
                # 7. y_start + stretch h A f, the differences and their maxima
                Am = np.abs(A)
                scale_den = np.zeros(n_y)
                rel_k = mp.mpf(0)
                for a in range(n_y):
                    ymax = max(abs(zp[a][jn]) for jn in range(1, n + 1))
                    den = 1 + (ymax + 1)
                    scale_den[a] = float(den)
                    for jn in range(1, n + 1):
                        Y = zp[a][0] + stretch * h * mp.fsum(F(A[jn - 1, i]) * fp[i][a] for i in range(n + 1))
                        e = abs(Y - zp[a][jn])
                        Yph[k, a, jn - 1], yph[k, a, jn - 1], aerr[k, a, jn - 1] = float(Y), float(zp[a][jn]), float(e)
                        rel_k = max(rel_k, e / den)
                    mag_abs[k, a, :n] = abs(z64[a, i0]) + sh * (Am @ mag_fp[a]) + mag_z[a, 1:]
                max_rel[k] = float(rel_k)
                max_abs[k] = aerr[k].max(axis=1)
                mag_max_abs[k] = mag_abs[k].max(axis=1)
                ymag = mag_z[:n_y, 1:].max(axis=1)
                mag_rel[k] = np.max(mag_abs[k, :, :n] / scale_den[:, None]
                                    + aerr[k, :, :n] * (ymag / scale_den ** 2)[:, None])
            out.append(dict(Y_ph=Yph, y_ph=yph, abs_err=aerr, max_rel=max_rel, max_abs=max_abs, mag_abs=mag_abs,
                            mag_max_abs=mag_max_abs, mag_max_rel=mag_rel))
    return out
