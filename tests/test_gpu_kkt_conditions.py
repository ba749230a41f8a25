"""The block L D L^T kernels (pc_kkt_*) on the matrices an interior-point run produces -- Sigma over twenty decades and
zero for unbounded unknowns, an indefinite Hessian, the regularisation dw of the inertia loop, most first
factorisations with the WRONG inertia -- held to the NumPy execution of the same elimination order (oracle/ref_kkt.py),
which tests/test_kkt_conditions_cpu.py holds to an eigenvalue inertia and a long-double-refined solve on these matrices.

1. inertia: exactly the reference's, wrong ones included (pivot signs of the same elimination order);
2. error against the long-double-refined truth, before and after one refinement step: within MARGIN of the reference's;
3. ``pc_kkt_solve_refined`` (dc = 0 in the system refined against, dc_eff = 1e-9 in the factors, as pc_ipm_newton
   calls it): the back-substitution count the stated rule gives with reference solves, the same error bound, and the
   early stop of ``PYCOLLO_AMD_KKT_RESID_TOL`` at the default, at 1e-6 and at 0;
4. a factorisation that failed (dw = 0: exact zero pivots) leaves nothing behind in the handle;
5. both chain paths (cyclic reduction and the node-by-node fallback).

The ratios e_gpu / max(e_ref, 64 eps) measured on the MI355X are kept in profiles/r07_kkt_conditions.txt."""
import os

import numpy as np
import pytest

from oracle.ref_kkt import RefKkt
from test_kkt_conditions_cpu import (CASES, DWS, EPS, pivot_report, reference_run, refined_rule, rel_error, truth, with_dw)
from test_kkt_cpu import ipm_like_case, reference_matrix

pytestmark = pytest.mark.gpu

# Both sides run the same elimination order in fp64 and differ in the order of the sums inside a block: the largest
# ratio e_gpu / max(e_ref, 64 eps) over all cases, before / after a refinement step and after pc_kkt_solve_refined, was
# measured on the MI355X (profiles/r07_kkt_conditions.txt); MARGIN is the next power of two above it (at most 64).
MARGIN = 32.0


def _device_case(name, kw):
    """The case with G~ / H~ evaluated on the device (they stay there) and host copies of the same bits."""
    base = ipm_like_case(name, kw, dw=0.0, device=0)
    eng, ora, x, lam = base[:4]
    c, G, H = eng.evaluate_all(x, 1.0, lam)
    eng.evaluate_resident(x, 1.0, lam)
    return base, (G, H)


def _pivot_report(k, R, dvec, got, inertia):
    _, p, q = k.factor_partial(dvec)
    return pivot_report(R, (p, q), got, inertia)


def _errors_of(solve, matvec, rhs, xstar):
    x0 = solve(rhs)
    x1 = x0 + solve(rhs - matvec(x0))
    return rel_error(x0, xstar), rel_error(x1, xstar)


def _check_factor_and_solve(k, base, values, dw, tag):
    """Items 1 and 2 for one matrix; returns what item 3 needs."""
    case, (G, H), T, K, R, inertia, rhs, xstar, e_ref = reference_run(base, dw, values=values, tables=k.tables)
    dvec = case[7]
    got = k.factor(dvec)
    assert got == inertia, f"{tag}\n" + _pivot_report(k, R, dvec, got, inertia)
    e_gpu = _errors_of(k.solve, lambda x: k.matvec(dvec, x), rhs, xstar)
    ratios = [eg / max(er, 64 * EPS) for eg, er in zip(e_gpu, e_ref)]
    wrong = "wrong" if inertia != (T.n_primal, T.n_dual) else "right"
    print(f"{tag} nu={T.nu} inertia {inertia} ({wrong}) e_ref {e_ref[0]:.2e} / {e_ref[1]:.2e} e_gpu {e_gpu[0]:.2e} / {e_gpu[1]:.2e} "
          f"ratio {ratios[0]:.2f} / {ratios[1]:.2f}")
    assert max(ratios) <= MARGIN, (tag, e_gpu, e_ref, ratios)
    return case, R, rhs, inertia != (T.n_primal, T.n_dual)


@pytest.fixture(scope="module")
def device_cases(built):
    """Every case once per module: the engine with G~ / H~ on the device, and the reference per dw (made when asked for)."""
    cache = {}

    def get(name, kw):
        key = (name, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = (*_device_case(name, kw), {})
        return cache[key]

    yield get
    for base, _, _ in cache.values():
        base[0].close()


@pytest.mark.parametrize("name,kw", CASES)
def test_inertia_and_solve_on_interior_point_matrices(device_cases, monkeypatch, name, kw):
    """Items 1 and 2 at every dw."""
    from pycollo_amd.kkt import GpuKkt
    monkeypatch.delenv("PYCOLLO_AMD_KKT_RESID_TOL", raising=False)
    base, values, _ = device_cases(name, kw)
    eng, _, _, _, ineq, fixed, sc = base[:7]
    k = GpuKkt(eng, ineq, fixed, sc)
    try:
        for dw in DWS:
            _check_factor_and_solve(k, base, values, dw, f"{name} {kw} dw={dw:g}")
    finally:
        k.close()


TOLS = (1e-12, 1e-6, 0.0)      # the default, one far above any rounding of the residual, none


class _DeviceMatrix:
    """K x through the device's own product (for the rule executed call by call with the device's kernels)."""

    def __init__(self, k, dvec):
        self.k, self.dvec = k, dvec

    def __matmul__(self, x):
        return self.k.matvec(self.dvec, x)


@pytest.fixture(scope="module")
def refined_runs(device_cases):
    """Item 3 for every (case, dw, tolerance), run once per module: ``solve_refined(rhs, dvec_true, max_steps=3)`` with
    dc = 0 in ``dvec_true`` and dc_eff = 1e-9 in the factors, beside the stated rule executed with reference solves."""
    from pycollo_amd.kkt import GpuKkt
    out, kept = {}, os.environ.get("PYCOLLO_AMD_KKT_RESID_TOL")
    try:
        for name, kw in CASES:
            base, values, _ = device_cases(name, kw)
            eng, _, _, _, ineq, fixed, sc = base[:7]
            for tol in TOLS:
                if tol == 1e-12:
                    os.environ.pop("PYCOLLO_AMD_KKT_RESID_TOL", None)        # the default
                else:
                    os.environ["PYCOLLO_AMD_KKT_RESID_TOL"] = repr(tol)
                k = GpuKkt(eng, ineq, fixed, sc)                              # (reads the tolerance when it is made)
                try:
                    for dw in DWS:
                        case, _, T, K, R, inertia, rhs, _, e_item2 = reference_run(base, dw, values=values, tables=k.tables)
                        K_true = reference_matrix(eng, *values, ineq, fixed, sc, case[8])
                        xstar = truth(K_true, rhs)
                        k.factor(case[7])
                        x_ref, n_ref, close, norms_ref, x_other = refined_rule(R.solve, K_true, rhs, 3, tol)
                        x_gpu, n_gpu = k.solve_refined(rhs, case[8], max_steps=3)
                        # the same rule call by call with the device's solve and product: its residual norms
                        _, n_dev, _, norms_dev, _ = refined_rule(k.solve, _DeviceMatrix(k, case[8]), rhs, 3, tol)
                        out[(name, kw.get("K"), dw, tol)] = dict(
                            n_gpu=n_gpu, n_ref=n_ref, n_dev=n_dev, close=close, e_ref=rel_error(x_ref, xstar), e_gpu=rel_error(x_gpu, xstar),
                            diff=float(np.max(np.abs(x_gpu - x_ref)) / np.max(np.abs(x_ref))), e0_ref=e_item2[0],
                            e_other=None if x_other is None else rel_error(x_other, xstar),
                            diff_other=None if x_other is None else float(np.max(np.abs(x_gpu - x_other)) / np.max(np.abs(x_other))),
                            norms_ref=norms_ref, norms_dev=norms_dev)
                finally:
                    k.close()
    finally:
        if kept is None:
            os.environ.pop("PYCOLLO_AMD_KKT_RESID_TOL", None)
        else:
            os.environ["PYCOLLO_AMD_KKT_RESID_TOL"] = kept
    return out


@pytest.mark.parametrize("tol", TOLS)
@pytest.mark.parametrize("dw", DWS)
@pytest.mark.parametrize("name,kw", CASES)
def test_refined_solve_follows_the_stated_rule(refined_runs, name, kw, dw, tol):
    """The back-substitution count of the stated rule, the error against the long-double-refined truth within MARGIN of
    the reference's, and x itself within MARGIN of the error of one unrefined reference solve on that matrix (the
    distance either side's iterate can have from the common fixed point; the truth of the dc = 0 system is far from
    both where that system is close to singular) -- or all three for the other outcome of the reference's last decision
    where that decision lay within 2x of the halving threshold (``_verdict``)."""
    r = refined_runs[(name, kw.get("K"), dw, tol)]
    fmt = lambda v: " ".join(f"{t:.1e}" for t in v)
    print(f"{name} {kw} dw={dw:g} tol={tol:g} refined: back-substitutions gpu {r['n_gpu']} reference {r['n_ref']} device call by call "
          f"{r['n_dev']} (close decision: {r['close']}) e_ref {r['e_ref']:.2e} e_gpu {r['e_gpu']:.2e} |x_gpu - x_ref| {r['diff']:.2e} "
          f"residuals / |rhs| reference [{fmt(r['norms_ref'])}] device [{fmt(r['norms_dev'])}]")
    assert _verdict(r) in ("same", "other outcome of a close decision"), r


def _verdict(r):
    """How a refined solve on the device relates to the rule executed with reference solves: "same" (count, x and error),
    "other outcome of a close decision" (the reference's last keep / reject decision lay within 2x of the halving
    threshold and the device's count, x and error are those of the other outcome: one back-substitution more or fewer, or
    the same count with the last correction kept on one side only), or what does not hold."""
    near = lambda d: d is not None and d <= MARGIN * max(r["e0_ref"], 64 * EPS)
    held = lambda e: e is not None and r["e_gpu"] <= MARGIN * max(e, 64 * EPS)
    if r["n_gpu"] == r["n_ref"] and near(r["diff"]) and held(r["e_ref"]):
        return "same"
    if not r["close"] or abs(r["n_gpu"] - r["n_ref"]) > 1:
        return "count or x differs without a close decision"
    if r["n_gpu"] == r["n_ref"] and not (near(r["diff_other"]) and held(r["e_other"])):
        return "x is neither outcome of the close decision"
    if r["n_gpu"] != r["n_ref"] and not (held(r["e_ref"]) or held(r["e_other"])):
        return "error beyond both outcomes"
    return "other outcome of a close decision"


def test_the_tolerance_stops_the_refinement_early(refined_runs):
    """``PYCOLLO_AMD_KKT_RESID_TOL`` and the early stop: with 1e-6, far above the rounding of any residual here, the device
    must take fewer back-substitutions than with 0 wherever the rule does -- which is most cases -- and never more; with
    0 it never stops early on a residual that is not 0."""
    fewer = 0
    for name, kw in CASES:
        for dw in DWS:
            loose, none = (refined_runs[(name, kw.get("K"), dw, tol)] for tol in (1e-6, 0.0))
            assert loose["n_gpu"] <= none["n_gpu"], (name, kw, dw)
            if loose["n_ref"] < none["n_ref"]:
                assert loose["n_gpu"] < none["n_gpu"], (name, kw, dw, loose, none)
                fewer += 1
    assert fewer >= len(CASES) * len(DWS) // 2, fewer


def test_few_refined_solves_needed_the_slack(refined_runs):
    """At most a quarter of the refined solves may be the other outcome of a close decision."""
    other = [key for key, r in refined_runs.items() if _verdict(r) != "same"]
    assert 4 * len(other) <= len(refined_runs), other


def test_wrong_inertia_is_among_the_cases_on_the_device(built):
    """At least three (case, dw) combinations have the wrong inertia in the reference -- and the device returns exactly
    those counts (the small cases; the parametrised test covers all)."""
    from pycollo_amd.kkt import GpuKkt
    wrong = 0
    for name, kw in [c for c in CASES if c[1].get("K", 0) <= 30]:
        base, values = _device_case(name, kw)
        eng, _, _, _, ineq, fixed, sc = base[:7]
        k = GpuKkt(eng, ineq, fixed, sc)
        R = RefKkt(k.tables)
        for dw in DWS:
            dvec = with_dw(base, dw)[7]
            inertia = R.factor(*values, dvec)
            assert k.factor(dvec) == inertia, (name, dw)
            wrong += inertia != (k.tables.n_primal, k.tables.n_dual)
        k.close()
        eng.close()
    assert wrong >= 3


@pytest.mark.parametrize("name,kw", [("brachistochrone", {}), ("free_flying_robot", dict(K=5, order=5))])
def test_a_failed_factorisation_leaves_nothing_behind(built, name, kw):
    """dw = 0 (exact zero pivots in the reference: NaN / inf in the factors), then dw = 100 on the same handle: bit-equal
    to a fresh handle's factor + solve."""
    from pycollo_amd.kkt import GpuKkt
    base, values = _device_case(name, kw)
    eng, _, _, _, ineq, fixed, sc = base[:7]
    rhs = np.random.default_rng(4).normal(size=eng.num_x + len(ineq) + eng.num_c)
    rhs[np.nonzero(fixed)[0]] = 0.0
    k = GpuKkt(eng, ineq, fixed, sc)
    failed = k.factor(with_dw(base, 0.0)[7])
    assert failed != (k.tables.n_primal, k.tables.n_dual)
    good = with_dw(base, 100.0)[7]
    inertia = k.factor(good)
    x = k.solve(rhs)
    k.close()
    fresh = GpuKkt(eng, ineq, fixed, sc)
    assert fresh.factor(good) == inertia
    np.testing.assert_array_equal(x, fresh.solve(rhs))
    assert np.all(np.isfinite(x))
    fresh.close()
    eng.close()


@pytest.mark.parametrize("name,kw", [("hypersensitive", dict(K=300, order=6)), ("two_phase_transfer", {})])
def test_the_sequential_chain_on_interior_point_matrices(built, monkeypatch, name, kw):
    """Items 1 and 2 with the chain eliminated node by node (PYCOLLO_AMD_KKT_CR=0)."""
    from pycollo_amd.kkt import GpuKkt
    monkeypatch.setenv("PYCOLLO_AMD_KKT_CR", "0")
    base, values = _device_case(name, kw)
    eng, _, _, _, ineq, fixed, sc = base[:7]
    k = GpuKkt(eng, ineq, fixed, sc)
    wrong = 0
    for dw in DWS:
        wrong += _check_factor_and_solve(k, base, values, dw, f"{name} {kw} dw={dw:g} CR=0")[3]
    assert wrong >= 1
    k.close()
    eng.close()
