"""The colouring plan of the derivative check (pycollo_amd/csrc/pc_deriv.hpp, pc_deriv_plan) on structure-only handles,
held against an independent NumPy recomputation from the CSR structures and the colours; and a NumPy restatement of the
check on the CPU oracle (tests/deriv_restate.py), which pins down what "located" and "sum" mean before any GPU is
involved.  The reference only promises the check (pycollo/settings.py:360, pycollo/iteration.py:455-458)."""
import numpy as np
import pytest

from conftest import golden_tables
from deriv_restate import rel, restate, sum_err
from oracle.ref_numpy import OracleNlp
from pycollo_amd import problems
from pycollo_amd.engine import NlpEngine


def _radau_brachistochrone():
    prob = problems.brachistochrone()
    prob.quadrature_method = "radau"
    return prob


CASES = {
    "brachistochrone": lambda: problems.brachistochrone(),
    "brachistochrone_radau": _radau_brachistochrone,
    "hypersensitive_2000x6": lambda: problems.hypersensitive(K=2000, order=6),
    "cart_pole": lambda: problems.cart_pole(),
    "shuttle": lambda: problems.shuttle(),
    "two_phase_transfer": lambda: problems.two_phase_transfer(),
    "time_coupled_transfer": lambda: problems.time_coupled_transfer(),
    "delta_iii": lambda: problems.delta_iii(),
    "sliding_mass_3": lambda: problems.sliding_mass(num_phases=3),
    "hypersensitive_refined": lambda: problems.with_refined_mesh(problems.hypersensitive(), 30000, seeds=(3,)),
}


def _recompute(eng, plan):
    """Located flags of G~ and H~ from the structures and the colours alone (NumPy)."""
    gr, gc = (a.astype(np.int64) for a in eng.evaluate_G_structure())
    hr, hc = (a.astype(np.int64) for a in eng.evaluate_H_structure())
    col = plan.colour.astype(np.int64)
    nc = plan.n_colours

    def counts(rows, cols):
        key = rows * nc + col[cols]
        u, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
        return cnt[inv], key

    gcnt, gkey = counts(gr, gc)
    g_loc = gcnt == 1
    off = hr != hc   # the full symmetric H~: every stored entry and its mirror
    fr = np.concatenate([hr, hc[off]])
    fc = np.concatenate([hc, hr[off]])
    fcnt, _ = counts(fr, fc)
    cside = fcnt[:hr.size] == 1
    rside = np.zeros(hr.size, bool)
    rside[off] = fcnt[hr.size:] == 1
    return gr, gc, g_loc, gkey, cside, rside


@pytest.mark.parametrize("name", list(CASES))
def test_plan_locates_every_entry(name):
    prob = CASES[name]()
    eng = NlpEngine(prob, device=None)
    plan = eng.derivative_plan()
    lay = eng.layout
    assert plan.colour.shape == (eng.num_x,) and plan.colour.min() == 0 and plan.colour.max() == plan.n_colours - 1
    gr, gc, g_loc, gkey, cside, rside = _recompute(eng, plan)
    np.testing.assert_array_equal(plan.jac_located, g_loc)
    np.testing.assert_array_equal(plan.hess_flag & 1, cside.astype(np.uint8))
    np.testing.assert_array_equal((plan.hess_flag & 2) > 0, rside)   # (a diagonal entry: bit 0 only)
    assert np.all(cside | rside), "an H~ entry is located from neither side"
    assert np.all(plan.jgrad_located)
    # sum terms: node columns of integral rows only, each in exactly one (row, colour) sum of at least two terms
    node = np.zeros(eng.num_x, bool)
    integral = np.zeros(eng.num_c, bool)
    for pl in lay.phases:
        node[pl.x_off:pl.x_off + pl.n_z * pl.N] = True
        integral[pl.c_int_off:pl.c_int_off + pl.n_q] = True
    s = ~plan.jac_located
    assert np.all(integral[gr[s]]) and np.all(node[gc[s]])
    _, cnt = np.unique(gkey[s], return_counts=True)
    assert np.all(cnt >= 2) and cnt.sum() == s.sum()
    # the colour count does not grow with the mesh
    n_max = max(int(np.max(m.n)) for m in eng.meshes)
    n_z = [pl.n_z for pl in lay.phases]
    n_global = sum(pl.n_q + pl.n_t for pl in lay.phases) + lay.n_s
    assert plan.n_colours <= max(n_z) * n_max + 2 * sum(n_z) + n_global


def test_colour_count_does_not_grow_with_the_mesh():
    small = NlpEngine(problems.hypersensitive(K=20, order=6), device=None).derivative_plan()
    big = NlpEngine(problems.hypersensitive(K=2000, order=6), device=None).derivative_plan()
    assert small.n_colours == big.n_colours
    assert big.colour.size > 90 * small.colour.size


@pytest.mark.parametrize("name,lo,hi", [("brachistochrone", -0.45, 0.45), ("two_phase_transfer", -0.45, 0.45)])
def test_numpy_restatement_reproduces_the_oracle(name, lo, hi):
    """Central differences of the oracle's own c~, J~ and grad L over the plan's colours recover the oracle's G~, H~ and
    grad J~: every located entry to 1e-6, every sum to 1e-6 of its largest term."""
    prob = CASES[name]()
    eng = NlpEngine(prob, device=None)
    plan = eng.derivative_plan()
    ora = OracleNlp(prob, golden_tables("lobatto"), V_ocp=eng.V_ocp, r_ocp=eng.r_ocp, W_ocp=eng.W_ocp, w_J=1.0)
    rng = np.random.default_rng(11)
    x = rng.uniform(lo, hi, eng.num_x)
    lam = rng.uniform(-1.0, 1.0, eng.num_c)
    jcols = eng.jgrad_columns()
    fdG, fdH, fdJ, sums = restate((ora.c, ora.J, ora.G, ora.grad_J), plan, eng.evaluate_G_structure(),
                                  eng.evaluate_H_structure(), jcols, x, 1.0, lam)
    G, H, gJ = ora.G(x), ora.H(x, 1.0, lam), ora.grad_J(x)[jcols]
    loc = plan.jac_located
    assert np.max(rel(G[loc], fdG[loc])) <= 1e-6
    assert np.all(np.isnan(fdG[~loc]))
    assert np.max(rel(H, fdH)) <= 1e-6
    assert np.max(rel(gJ, fdJ)) <= 1e-6
    if (~loc).any():
        assert len(sums) > 0 and max(sum_err(G, sums).values()) <= 1e-6
    # a corrupted entry is seen: one G~ entry and one H~ entry off by 1e-3
    G2, H2 = G.copy(), H.copy()
    e = int(np.flatnonzero(loc)[len(np.flatnonzero(loc)) // 2])
    G2[e] += 1e-3 * max(1.0, abs(G2[e]))
    H2[3] += 1e-3 * max(1.0, abs(H2[3]))
    assert rel(G2[e], fdG[e]) > 1e-4 and rel(H2[3], fdH[3]) > 1e-4
