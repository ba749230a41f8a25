"""NumPy restatement of the derivative check (pc_check_derivatives_device) on top of any evaluator of c~, J~, G~ and grad J~:
what "located" and "sum" mean, entry by entry, independent of the device kernels.  Shared by the CPU and GPU tests."""
import numpy as np


def restate(fns, plan, g_struct, h_struct, jcols, x, sigma, lam, delta=1e-5, rounding=None):
    """``fns`` = (c(x), J(x), G(x) CSR values, grad J(x) dense); ``plan`` = NlpEngine.derivative_plan().  Returns the FD
    estimate of every G~ entry (NaN for sum terms), of every H~ entry, of every grad J~ non-zero, and the sums as
    {(row, colour): (list of G~ entries, (c+_r - c-_r) / 2, h of every entry)}.  A dict passed as ``rounding`` receives,
    per H~ entry, what bounds the rounding of its FD value in any summation order: ``n`` = the number of terms
    t_e = (G+_e - G-_e) lambda_r of the grad L row it is read from, ``mag`` = sum |t_e| / |step2|."""
    c_fn, J_fn, G_fn, gJ_fn = fns
    gr, gc = (np.asarray(a, np.int64) for a in g_struct)
    hr, hc = (np.asarray(a, np.int64) for a in h_struct)
    n = x.size
    col = plan.colour
    fdG = np.full(gr.size, np.nan)
    fdH = np.full(hr.size, np.nan)
    fdJ = np.full(len(jcols), np.nan)
    sums = {}
    for k in range(plan.n_colours):
        S = np.flatnonzero(col == k)
        if S.size == 0:
            continue
        h = delta * np.maximum(1.0, np.abs(x[S]))
        xp, xm = x.copy(), x.copy()
        xp[S] += h
        xm[S] -= h
        step2 = np.zeros(n)
        step2[S] = xp[S] - xm[S]
        cp, cm = c_fn(xp), c_fn(xm)
        Gp, Gm = G_fn(xp), G_fn(xm)
        gp, gm = gJ_fn(xp), gJ_fn(xm)
        # grad L(x+) - grad L(x-), grad L = sigma grad J + G^T lambda
        dL = sigma * (gp - gm) + np.bincount(gc, weights=(Gp - Gm) * lam[gr], minlength=n)
        inS = col[gc] == k
        loc = inS & plan.jac_located
        fdG[loc] = (cp[gr[loc]] - cm[gr[loc]]) / step2[gc[loc]]
        for e in np.flatnonzero(inS & ~plan.jac_located):
            key = (int(gr[e]), k)
            if key not in sums:
                sums[key] = ([], 0.5 * (cp[gr[e]] - cm[gr[e]]), [])
            sums[key][0].append(int(e))
            sums[key][2].append(0.5 * step2[gc[e]])
        cside = (plan.hess_flag & 1).astype(bool) & (col[hc] == k)
        rside = ~(plan.hess_flag & 1).astype(bool) & (plan.hess_flag & 2).astype(bool) & (col[hr] == k)
        fdH[cside] = dL[hr[cside]] / step2[hc[cside]]
        fdH[rside] = dL[hc[rside]] / step2[hr[rside]]
        if rounding is not None:
            if not rounding:
                rounding["n"] = np.zeros(hr.size, np.int64)
                rounding["mag"] = np.zeros(hr.size)
            mag = np.bincount(gc, weights=np.abs((Gp - Gm) * lam[gr]), minlength=n)
            per_col = np.bincount(gc, minlength=n)
            for side, q, s in ((cside, hr, hc), (rside, hc, hr)):
                rounding["n"][side] = per_col[q[side]]
                rounding["mag"][side] = mag[q[side]] / np.abs(step2[s[side]])
        jk = col[jcols] == k
        fdJ[jk] = (J_fn(xp) - J_fn(xm)) / step2[jcols[jk]]
    return fdG, fdH, fdJ, sums


def sum_keys(g_struct, plan):
    """The (row, colour) of every sum in the order of its number: colour by colour, rows ascending within a colour."""
    gr, gc = (np.asarray(a, np.int64) for a in g_struct)
    s = ~np.asarray(plan.jac_located, bool)
    return sorted({(int(r), int(k)) for r, k in zip(gr[s], np.asarray(plan.colour)[gc[s]])}, key=lambda rk: (rk[1], rk[0]))


def _finite_or_inf(e):
    """Errors are >= 0 or not finite: NaN and +-inf (of a value or of the quotient) count as +inf."""
    return np.where(np.isfinite(e), e, np.inf)


def errors(G, H, Jv, fdG, fdH, fdJ, sums, g_struct, plan):
    """The concatenated error array [G~ | sums | H~ | grad J~ non-zeros] of analytic values ``G``, ``H``, ``Jv`` against
    the FD values and ``sums`` of ``restate``: |an - fd| / max(1, |an|) per located entry, -1 for a G~ entry that is a
    term of a sum, |sum an_j h_j - (c+ - c-)/2| / max_j(|an_j| h_j, h_j) per sum (numbered as ``sum_keys``); an entry
    whose value or quotient is not finite and a sum with a non-finite analytic term get +inf."""
    G, H, Jv = (np.asarray(a, float) for a in (G, H, Jv))
    loc = np.asarray(plan.jac_located, bool)
    with np.errstate(all="ignore"):
        eG = np.where(loc, _finite_or_inf(np.abs(G - fdG) / np.maximum(1.0, np.abs(G))), -1.0)
        eH = _finite_or_inf(np.abs(H - fdH) / np.maximum(1.0, np.abs(H)))
        eJ = _finite_or_inf(np.abs(Jv - fdJ) / np.maximum(1.0, np.abs(Jv)))
        eS = []
        for key in sum_keys(g_struct, plan):
            ents, half, hs = sums[key]
            an, hs = G[np.array(ents)], np.array(hs)
            if not np.all(np.isfinite(an)):
                eS.append(np.inf)
                continue
            eS.append(float(_finite_or_inf(np.abs(np.sum(an * hs) - half) / max(np.max(np.abs(an) * hs), np.max(hs)))))
    return np.concatenate([eG, np.array(eS, float), eH, eJ])


def expected_report(err, tol, max_report, structures, plan):
    """What a check reports for the concatenated error array ``err`` (``errors``).  ``structures`` = (G~ (rows, cols),
    H~ (rows, cols), x index of every grad J~ non-zero).  Returns a dict: ``n_fail`` and ``max_err`` per kind "jac" (located
    entries and sums together), "hess", "grad" (err > tol fails; a negative maximum, or a kind without entries, gives 0);
    ``worst`` per kind as (kind, index, row, col), the lowest concatenated position on ties, None for a kind without
    entries; ``failures``: the first min(max_report, 64) failing positions in concatenated order as (kind, index, row,
    col), kind "jac_sum" with col = the colour and index = the number of the sum."""
    g_struct, h_struct, jcols = structures
    gr, gc = (np.asarray(a, np.int64) for a in g_struct)
    hr, hc = (np.asarray(a, np.int64) for a in h_struct)
    jcols = np.asarray(jcols, np.int64)
    keys = sum_keys(g_struct, plan)
    nG, nS, nH, nJ = gr.size, len(keys), hr.size, jcols.size
    err = np.asarray(err, float)
    assert err.shape == (nG + nS + nH + nJ,) and not np.any(np.isnan(err))

    def entry(t):
        t = int(t)
        if t < nG:
            return ("jac", t, int(gr[t]), int(gc[t]))
        t -= nG
        if t < nS:
            return ("jac_sum", t, keys[t][0], keys[t][1])
        t -= nS
        if t < nH:
            return ("hess", t, int(hr[t]), int(hc[t]))
        t -= nH
        return ("grad", t, -1, int(jcols[t]))

    out = dict(n_fail={}, max_err={}, worst={})
    for kind, a, b in (("jac", 0, nG + nS), ("hess", nG + nS, nG + nS + nH), ("grad", nG + nS + nH, nG + nS + nH + nJ)):
        e = err[a:b]
        out["n_fail"][kind] = int(np.count_nonzero(e > tol))
        if e.size == 0:
            out["max_err"][kind], out["worst"][kind] = 0.0, None
            continue
        i = int(np.argmax(e))   # (the first of equal maxima)
        out["max_err"][kind] = max(float(e[i]), 0.0)
        out["worst"][kind] = entry(a + i)
    out["failures"] = [entry(t) for t in np.flatnonzero(err > tol)[:max(0, min(int(max_report), 64))]]
    return out


def rel(an, fd):
    return np.abs(an - fd) / np.maximum(1.0, np.abs(an))


def sum_err(G, sums):
    """err of every sum: |sum an_j h_j - (c+ - c-)/2| / max(max_j |an_j| h_j, max_j h_j)."""
    out = {}
    for key, (ents, half, hs) in sums.items():
        an, hs = G[np.array(ents)], np.array(hs)
        out[key] = abs(np.sum(an * hs) - half) / max(np.max(np.abs(an) * hs), np.max(hs))
    return out
