"""NumPy restatement of the derivative check (pc_check_derivatives_device) on top of any evaluator of c~, J~, G~ and grad J~:
what "located" and "sum" mean, entry by entry, independent of the device kernels.  Shared by the CPU and GPU tests."""
import numpy as np


def restate(fns, plan, g_struct, h_struct, jcols, x, sigma, lam, delta=1e-5):
    """``fns`` = (c(x), J(x), G(x) CSR values, grad J(x) dense); ``plan`` = NlpEngine.derivative_plan().  Returns the FD
    estimate of every G~ entry (NaN for sum terms), of every H~ entry, of every grad J~ non-zero, and the sums as
    {(row, colour): (list of G~ entries, (c+_r - c-_r) / 2, h of every entry)}."""
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
        jk = col[jcols] == k
        fdJ[jk] = (J_fn(xp) - J_fn(xm)) / step2[jcols[jk]]
    return fdG, fdH, fdJ, sums


def rel(an, fd):
    return np.abs(an - fd) / np.maximum(1.0, np.abs(an))


def sum_err(G, sums):
    """err of every sum: |sum an_j h_j - (c+ - c-)/2| / max(max_j |an_j| h_j, max_j h_j)."""
    out = {}
    for key, (ents, half, hs) in sums.items():
        an, hs = G[np.array(ents)], np.array(hs)
        out[key] = abs(np.sum(an * hs) - half) / max(np.max(np.abs(an) * hs), np.max(hs))
    return out
