"""The reference elimination (oracle/ref_kkt.py) on the matrices an interior-point run produces
(``test_kkt_cpu.ipm_like_case``: Sigma over twenty decades and zero for unbounded unknowns, an indefinite Hessian, the
regularisation dw of the inertia loop), held to an eigenvalue inertia and to a solve refined with long-double residuals.
No GPU; tests/test_gpu_kkt_conditions.py holds the GPU kernels to this reference on the same matrices.

The errors measured here are kept in profiles/r07_kkt_conditions.txt."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

from oracle.ref_kkt import RefKkt
from pycollo_amd import kkt
from test_kkt_cpu import ipm_like_case, reference_matrix

LD = np.longdouble
EPS = float(np.finfo(float).eps)

CASES = [("free_flying_robot", dict(K=5, order=5)), ("free_flying_robot", dict(K=33, order=5)), ("shuttle", dict(K=6, order=4)),
         ("shuttle", dict(K=60, order=4)), ("brachistochrone", {}), ("hypersensitive", dict(K=30, order=6)),
         ("hypersensitive", dict(K=300, order=6)), ("two_phase_transfer", {})]
DWS = (1e-4, 1.0, 100.0)
# The reference's own error on each matrix, before / after one refinement step (max |x - x*| / max |x*|), as first recorded
# with this file's seeds (profiles/r07_kkt_conditions.txt).  The figures of the first experiment on such matrices (<= 2.6e-11
# at dw = 1e-4, <= 1.1e-13 for hypersensitive and two_phase_transfer) were taken with other random draws and do not
# reproduce with these: shuttle K=60 at dw = 1e-4 gives 3.5e-9, hypersensitive K=300 at dw = 1 gives 3.6e-12.  Every
# (case, dw) is therefore held to its own recorded value: within SLACK of it or of 64 eps (SuperLU / BLAS builds differ in
# the last bits of x*, and an error near the rounding floor moves by a small factor with them).
RECORDED = {
    ('free_flying_robot', 5, 0.0001): (3.14e-06, 1.01e-12),
    ('free_flying_robot', 5, 1): (1.64e-10, 7.06e-16),
    ('free_flying_robot', 5, 100): (1.72e-10, 3.01e-16),
    ('free_flying_robot', 33, 0.0001): (8.25e-08, 2.32e-14),
    ('free_flying_robot', 33, 1): (2.52e-10, 3.42e-16),
    ('free_flying_robot', 33, 100): (8.77e-12, 3.64e-16),
    ('shuttle', 6, 0.0001): (3.96e-07, 1.88e-13),
    ('shuttle', 6, 1): (1.50e-09, 2.03e-15),
    ('shuttle', 6, 100): (2.24e-11, 1.62e-15),
    ('shuttle', 60, 0.0001): (2.75e-05, 3.47e-09),
    ('shuttle', 60, 1): (9.51e-09, 9.55e-16),
    ('shuttle', 60, 100): (3.10e-09, 2.71e-16),
    ('brachistochrone', None, 0.0001): (1.79e-07, 1.78e-14),
    ('brachistochrone', None, 1): (5.72e-12, 1.15e-16),
    ('brachistochrone', None, 100): (2.58e-12, 9.64e-17),
    ('hypersensitive', 30, 0.0001): (5.14e-09, 6.11e-15),
    ('hypersensitive', 30, 1): (1.92e-09, 1.95e-14),
    ('hypersensitive', 30, 100): (1.88e-08, 9.95e-15),
    ('hypersensitive', 300, 0.0001): (2.60e-08, 2.43e-13),
    ('hypersensitive', 300, 1): (1.02e-08, 3.64e-12),
    ('hypersensitive', 300, 100): (9.83e-09, 1.68e-14),
    ('two_phase_transfer', None, 0.0001): (1.35e-10, 7.11e-17),
    ('two_phase_transfer', None, 1): (1.04e-13, 1.63e-16),
    ('two_phase_transfer', None, 100): (1.30e-12, 2.80e-16),
}
SLACK = 4.0


def residual_ld(K, rhs, x):
    """rhs - K x with the products and the sums in long double (K: scipy sparse)."""
    Kc = K.tocoo()
    r = np.asarray(rhs, LD).copy()
    np.subtract.at(r, Kc.row, np.asarray(Kc.data, LD) * np.asarray(x, LD)[Kc.col])
    return r


def truth(K, rhs):
    """x* = SuperLU's solve refined with long-double residuals until the residual stops shrinking."""
    lu = spla.splu(K.tocsc())
    x = np.asarray(lu.solve(np.asarray(rhs, float)), LD)
    r = residual_ld(K, rhs, x)
    for _ in range(30):
        xt = x + np.asarray(lu.solve(r.astype(float)), LD)
        rt = residual_ld(K, rhs, xt)
        if not float(np.max(np.abs(rt))) < float(np.max(np.abs(r))):
            break
        x, r = xt, rt
    return x


def rel_error(x, xstar):
    return float(np.max(np.abs(np.asarray(x, LD) - xstar)) / np.max(np.abs(xstar)))


def right_hand_side(nu, fixed, seed=1):
    rhs = np.random.default_rng(seed).normal(size=nu)
    rhs[np.nonzero(fixed)[0]] = 0.0
    return rhs


def refined_rule(solve, K_true, rhs, max_steps, resid_tol):
    """The rule of ``pc_kkt_solve_refined`` as ipm_sharded.py::solve_refined states it -- keep a correction while it
    halves the residual's 2-norm and stays finite, stop once the residual is below resid_tol of the right-hand side --
    executed with the given solve.  As stated there the residual that the corrections are solved for and the decisions are
    taken on is computed in double, the precision any fp64 implementation has; the long double of this file is kept for
    measuring the error of the result.  A decision within 2x of the halving threshold may go the other way in another
    fp64 implementation; for the last decision taken the iterate of that other outcome is returned too.  (A first edition decided on a long-double residual: it kept a correction whose
    gain lay below the rounding of a double residual, which no fp64 implementation can see, and then held the device
    to that iterate's error.)  Returns (x, back-substitutions, whether a keep / reject decision was close: a residual
    ratio within 2x of the halving threshold, every residual norm as a fraction of the right-hand side's, the iterate the
    other outcome of the last decision would have left if that decision was close, else None)."""
    sol = solve(rhs)
    solves, close = 1, False
    res = rhs - K_true @ sol
    nres, nrhs = float(res @ res), float(rhs @ rhs)
    norms = [np.sqrt(nres / nrhs)]
    other = None
    for _ in range(max_steps):
        if nres <= resid_tol ** 2 * nrhs:
            break
        other = None
        trial = sol + solve(res)
        res_t = rhs - K_true @ trial
        solves += 1
        nt = float(res_t @ res_t)
        norms.append(np.sqrt(nt / nrhs))
        q = np.sqrt(nt) / np.sqrt(nres)
        if 0.25 <= q <= 1.0:
            close, other = True, (sol if q < 0.5 else trial)
        if not (np.all(np.isfinite(trial)) and np.all(np.isfinite(res_t))) or q >= 0.5:
            break
        sol, nres, res = trial, nt, res_t
    return sol, solves, close, norms, other


def pivot_report(R, gpu_partial_counts, gpu_counts, ref_counts):
    """What can be said about a differing pivot count.  The device's interface returns counts only -- of the whole
    factorisation and, through ``pc_kkt_factor_partial``, of leaves and chain without the border -- so the node of the
    first differing pivot cannot be named: the report says whether the difference lies in the border block or in a leaf
    or chain node, and lists the reference's three nodes whose smallest pivot is closest to a change of sign (where a
    sum taken in another order flips a sign first)."""
    lines = [f"inertia: gpu {tuple(gpu_counts)} reference {tuple(ref_counts)}",
             f"leaves + chain: gpu {tuple(gpu_partial_counts)} reference {tuple(R.partial_counts)} -> "
             + ("the border block" if tuple(gpu_partial_counts) == tuple(R.partial_counts) else "a leaf or chain node")]
    small = []
    for kind, blocks, sizes in (("leaf", R.leafM, R.m_l), ("chain node", R.chainM, R.nzb)):
        for i, (M, sz) in enumerate(zip(blocks, sizes)):
            if M is None or int(sz) == 0:
                continue
            d = np.abs(np.diag(M[:int(sz), :int(sz)]))
            small.append((float(np.min(d) / np.max(d)), f"{kind} {i} (smallest |pivot| {np.min(d):.3e} of {np.max(d):.3e})"))
    d = np.abs(np.diag(R.Bd))
    if d.size:
        small.append((float(np.min(d) / np.max(d)), f"border (smallest |pivot| {np.min(d):.3e} of {np.max(d):.3e})"))
    lines += ["closest to a sign change in the reference: " + t for _, t in sorted(small)[:3]]
    return "\n".join(lines)


def with_dw(base, dw):
    """``ipm_like_case(..., dw=0)``'s tuple with the primal regularisation dw on its two diagonals (the same bits as
    building the case with that dw: Sigma + 0 is Sigma)."""
    *head, dvec, dvec_true = base
    nv = head[0].num_x + len(head[4])
    shift = np.concatenate([np.full(nv, dw), np.zeros(len(dvec) - nv)])
    return (*head, dvec + shift, dvec_true + shift)


def reference_run(base, dw, values=None, tables=None):
    """The reference on one matrix: (case tuple, (G, H), tables, K, RefKkt factorised, its inertia, rhs, x*, its error
    before / after one refinement step).  ``base``: ``ipm_like_case(name, kw, dw=0)``; ``values``: (G, H) to use instead
    of the oracle's (the device's own bits)."""
    case = with_dw(base, dw)
    eng, ora, x, lam, ineq, fixed, sc, dvec, dvec_true = case
    G, H = values if values is not None else (ora.G(x), ora.H(x, 1.0, lam))
    T = tables if tables is not None else kkt.build_tables(eng, ineq, fixed, sc, None)
    K = reference_matrix(eng, G, H, ineq, fixed, sc, dvec)
    R = RefKkt(T)
    inertia = R.factor(G, H, dvec)
    rhs = right_hand_side(T.nu, fixed)
    xstar = truth(K, rhs)
    x0 = R.solve(rhs)
    x1 = x0 + R.solve(rhs - K @ x0)
    return case, (G, H), T, K, R, inertia, rhs, xstar, (rel_error(x0, xstar), rel_error(x1, xstar))


@pytest.mark.parametrize("name,kw", CASES)
def test_reference_elimination_on_interior_point_matrices(built, name, kw):
    base = ipm_like_case(name, kw, dw=0.0)
    for dw in DWS:
        case, _, T, K, R, inertia, rhs, xstar, (e0, e1) = reference_run(base, dw)
        if T.nu <= 3000:
            ev = np.linalg.eigvalsh(K.toarray())
            assert inertia == (int((ev > 0).sum()), int((ev < 0).sum())), (dw, "pivot signs differ from the eigenvalue inertia")
        assert sum(inertia) == T.nu
        print(f"{name} {kw} dw={dw:g} nu={T.nu} inertia={inertia} wanted={(T.n_primal, T.n_dual)} "
              f"ref error before/after one step {e0:.2e} / {e1:.2e}")
        r0, r1 = RECORDED[(name, kw.get("K"), dw)]
        assert e0 <= SLACK * r0 and e1 <= SLACK * max(r1, 64 * EPS), (dw, (e0, e1), (r0, r1))
    base[0].close()


def test_the_cases_include_wrong_inertia(built):
    """With lam_scale = 100 the first factorisations of the inertia loop have the wrong inertia, as in a solver run: at
    least three (case, dw) combinations, among them ones at dw = 1."""
    wrong = []
    for name, kw in CASES:
        base = ipm_like_case(name, kw, dw=0.0)
        eng, ora, x, lam, ineq, fixed, sc, _, _ = base
        G, H, T = ora.G(x), ora.H(x, 1.0, lam), kkt.build_tables(eng, ineq, fixed, sc, None)
        for dw in DWS:
            inertia = RefKkt(T).factor(G, H, with_dw(base, dw)[7])
            if inertia != (T.n_primal, T.n_dual):
                wrong.append((name, dw))
        eng.close()
    assert len(wrong) >= 3, wrong
    assert any(dw == 1.0 for _, dw in wrong)


def test_no_regularisation_gives_exact_zero_pivots(built):
    """dw = 0: an unbounded unknown without a Hessian diagonal is an exact zero pivot of the elimination."""
    eng, ora, x, lam, ineq, fixed, sc, dvec, _ = ipm_like_case("brachistochrone", {}, dw=0.0)
    T = kkt.build_tables(eng, ineq, fixed, sc, None)
    with np.errstate(all="ignore"):
        inertia = RefKkt(T).factor(ora.G(x), ora.H(x, 1.0, lam), dvec)
    assert inertia != (T.n_primal, T.n_dual)
    eng.close()


def test_the_pivot_report_says_where_counts_differ(built):
    """The message an inertia mismatch on the device would carry, made here from the reference and counts that differ by
    one pivot in a leaf / in the border."""
    base = ipm_like_case("two_phase_transfer", {}, dw=0.0)
    _, _, T, _, R, inertia, *_ = reference_run(base, 1.0)
    p, q = R.partial_counts
    leaf = pivot_report(R, (p - 1, q + 1), (inertia[0] - 1, inertia[1] + 1), inertia)
    assert "-> a leaf or chain node" in leaf and leaf.count("closest to a sign change") == 3
    border = pivot_report(R, (p, q), (inertia[0] - 1, inertia[1] + 1), inertia)
    assert "-> the border block" in border and str(inertia) in border
    base[0].close()
