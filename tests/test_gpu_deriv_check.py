"""GPU tests of the derivative check (pc_check_derivatives_device, NlpEngine.check_derivatives; run with -m gpu): clean
models pass, the FD estimates are the CPU restatement's (tests/deriv_restate.py), one corrupted entry of any category
is found and located, reports are bit-reproducible and leave the handle as it was, and solve_ocp / the pycollo backend
honour check_nlp_functions (pycollo/settings.py:360, pycollo/iteration.py:455-458).  Only builds build() makes are
loaded (PREBUILD, PREBUILD_MIXED, REFINED_MESHES)."""
import ctypes as C
import warnings

import numpy as np
import pytest

from conftest import golden_tables
from deriv_restate import restate
from oracle.ref_numpy import OracleNlp
from pycollo_amd import problems
from pycollo_amd.engine import NlpEngine
from test_gpu_mixed import mixed_problem

pytestmark = pytest.mark.gpu


def _radau_brachistochrone():
    prob = problems.brachistochrone()
    prob.quadrature_method = "radau"
    return prob


# (problem, engine keyword arguments, x~ range)
CLEAN = {
    "brachistochrone": (problems.brachistochrone, {}, (-0.45, 0.45)),
    "brachistochrone_radau": (_radau_brachistochrone, {}, (-0.45, 0.45)),
    "hypersensitive_2000x6": (lambda: problems.hypersensitive(K=2000, order=6), {}, (-0.45, 0.45)),
    "cart_pole": (problems.cart_pole, {}, (-0.45, 0.45)),
    "shuttle": (problems.shuttle, {}, (-0.45, 0.45)),
    "time_coupled_transfer_mixed": (lambda: mixed_problem("time_coupled_transfer"), {"mixed": ((4, 6), (4, 6))}, (-0.45, 0.45)),
    "sliding_mass_3": (lambda: problems.sliding_mass(num_phases=3), {}, (-0.45, 0.45)),
    "hypersensitive_refined": (lambda: problems.with_refined_mesh(problems.hypersensitive(), 30000, seeds=(3,)), {},
                               (-0.45, 0.45)),
}


def _point(eng, rng_range, seed=3):
    rng = np.random.default_rng(seed)
    return rng.uniform(*rng_range, eng.num_x), rng.uniform(-1.0, 1.0, eng.num_c)


@pytest.mark.parametrize("name", list(CLEAN))
def test_clean_models_pass(built, name):
    make, kw, rr = CLEAN[name]
    eng = NlpEngine(make(), device=0, **kw)
    x, lam = _point(eng, rr)
    chk = eng.check_derivatives(x, 1.0, lam)
    print(f"\n{name}: colours {chk.n_colours}, evaluations {chk.n_evaluations}, max err G~ {chk.max_err_jac:.2e} "
          f"H~ {chk.max_err_hess:.2e} grad J~ {chk.max_err_grad:.2e}")
    assert chk.ok, (chk.max_err_jac, chk.max_err_hess, chk.max_err_grad, chk.failures[:5])
    assert chk.n_evaluations == 1 + 2 * chk.n_colours
    assert chk.n_jac_located + chk.n_jac_sum_terms == eng.nnz_jac and chk.n_hess_located == eng.nnz_hess
    # seeded lambda (lagrange=None) passes as well
    assert eng.check_derivatives(x).ok
    eng.close()


@pytest.mark.parametrize("name", ["brachistochrone", "two_phase_transfer"])
def test_fd_estimates_match_the_cpu_restatement(built, name):
    prob = problems.REGISTRY[name]()
    eng = NlpEngine(prob, device=0)
    x, lam = _point(eng, (-0.45, 0.45), seed=11)
    chk = eng.check_derivatives(x, 1.0, lam, return_fd=True)
    assert chk.ok
    ora = OracleNlp(prob, golden_tables("lobatto"), V_ocp=eng.V_ocp, r_ocp=eng.r_ocp, W_ocp=eng.W_ocp, w_J=1.0)
    plan = eng.derivative_plan()
    fdG, fdH, fdJ, _ = restate((ora.c, ora.J, ora.G, ora.grad_J), plan, eng.evaluate_G_structure(), eng.evaluate_H_structure(),
                               eng.jgrad_columns(), x, 1.0, lam)
    loc = plan.jac_located
    assert np.all(np.isnan(chk.jac_fd[~loc]))
    for got, ref in ((chk.jac_fd[loc], fdG[loc]), (chk.hess_fd, fdH), (chk.jgrad_fd, fdJ)):
        assert np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))) <= 1e-8
    eng.close()


def _categories(eng, plan, G, H):
    """(name, kind, entry index) of the largest-magnitude located entry of every category of G~ / H~."""
    lay = eng.layout
    gr, gc = (a.astype(np.int64) for a in eng.evaluate_G_structure())
    hr, hc = (a.astype(np.int64) for a in eng.evaluate_H_structure())
    n, m = eng.num_x, eng.num_c
    rowk = np.zeros(m, np.int64)   # 0 defect, 1 path, 2 integral, 3 endpoint
    colk = np.zeros(n, np.int64)   # 0 node, 1 q, 2 t, 3 s
    interior = np.zeros(n, bool)
    node_of = np.full(n, -1, np.int64)
    for ip, pl in enumerate(lay.phases):
        rowk[pl.c_path_off:pl.c_int_off] = 1
        rowk[pl.c_int_off:pl.c_int_off + pl.n_q] = 2
        colk[pl.q_off:pl.t_off] = 1
        colk[pl.t_off:pl.t_off + pl.n_t] = 2
        for v in range(pl.n_z):
            idx = pl.x_off + v * pl.N + np.arange(pl.N)
            node_of[idx] = ip * 10 ** 7 + np.arange(pl.N)
            interior[idx[1:-1]] = True
    rowk[lay.c_end_off:] = 3
    colk[lay.s_off:] = 3
    special = ~interior
    gloc = plan.jac_located

    def pick(mask, vals):
        idx = np.flatnonzero(mask)
        assert idx.size, "category absent"
        return int(idx[np.argmax(np.abs(vals[idx]))])

    return [
        ("defect", "jac", pick(gloc & (rowk[gr] == 0), G)),
        ("path", "jac", pick(gloc & (rowk[gr] == 1), G)),
        ("endpoint row", "jac", pick(gloc & (rowk[gr] == 3), G)),
        ("t0/tF column", "jac", pick(gloc & (colk[gc] == 2), G)),
        ("parameter column", "jac", pick(gloc & (colk[gc] == 3), G)),
        ("node block", "hess", pick(interior[hr] & interior[hc] & (node_of[hr] == node_of[hc]), H)),
        ("endpoint cross block", "hess", pick(special[hr] & special[hc] & (colk[hr] == 0) & (colk[hc] == 0) & (hr != hc), H)),
        ("global row", "hess", pick(colk[hr] != 0, H)),
    ], gr, gc, hr, hc


def test_injected_errors_are_found_and_located(built):
    prob = problems.two_phase_transfer()
    eng = NlpEngine(prob, device=0)
    x, lam = _point(eng, (-0.45, 0.45), seed=5)
    _, G, H = eng.evaluate_all(x, 1.0, lam)
    plan = eng.derivative_plan()
    cats, gr, gc, hr, hc = _categories(eng, plan, G, H)
    assert eng.check_derivatives(x, 1.0, lam, jac_values=G, hess_values=H).ok
    for cat, kind, e in cats:
        G2, H2 = G.copy(), H.copy()
        v = G2 if kind == "jac" else H2
        v[e] += 1e-3 * max(1.0, abs(v[e]))   # (relative 1e-3 for |an| >= 1, where err = |an - fd| / max(1, |an|))
        chk = eng.check_derivatives(x, 1.0, lam, jac_values=G2, hess_values=H2)
        assert not chk.ok and chk.n_fail == 1 and len(chk.failures) == 1, (cat, chk.n_fail, chk.failures)
        f = chk.failures[0]
        rows, cols = (gr, gc) if kind == "jac" else (hr, hc)
        assert (f.kind, f.index, f.row, f.col) == (kind, e, rows[e], cols[e]), (cat, f)
    # one grad J~ non-zero
    _, gJ, _ = eng.evaluate_resident(x, 1.0, None)
    jcols = eng.jgrad_columns()
    jv = gJ[jcols]
    j = int(np.argmax(np.abs(jv)))
    jv2 = jv.copy()
    jv2[j] += 1e-3 * max(1.0, abs(jv2[j]))
    chk = eng.check_derivatives(x, 1.0, lam, jgrad_values=jv2)
    assert not chk.ok and chk.n_fail == 1 and chk.failures[0].kind == "grad" and chk.failures[0].col == jcols[j]
    # an integral row's node-column entry: detected as its (row, colour) sum
    s = np.flatnonzero(~plan.jac_located)
    e = int(s[np.argmax(np.abs(G[s]))])
    G2 = G.copy()
    G2[e] += 1e-3 * max(1.0, abs(G2[e]))
    chk = eng.check_derivatives(x, 1.0, lam, jac_values=G2)
    assert not chk.ok and chk.n_fail == 1
    f = chk.failures[0]
    assert f.kind == "jac_sum" and f.row == gr[e] and f.col == plan.colour[gc[e]]
    eng.close()


def _device_copy(eng, ptr, n):
    """n doubles of device memory at ptr, through the library's own run-copy kernel (pc_copy_runs)."""
    import torch
    out = torch.empty(n, dtype=torch.float64, device="cuda:0")
    L = eng._lib.pc_run_chunk()
    ch = torch.tensor([[s, s, min(L, n - s)] for s in range(0, n, L)], dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    assert eng._lib.pc_copy_runs(C.c_void_p(ptr), C.c_void_p(out.data_ptr()), C.c_void_p(ch.data_ptr()), ch.shape[0], None)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_reports_reproducible_and_handle_untouched(built):
    eng = NlpEngine(problems.two_phase_transfer(), device=0)
    x, lam = _point(eng, (-0.45, 0.45), seed=7)
    x2 = x + 0.01
    # the host path's cached point: J, grad J, c~, G~ at x2 (new_x = 1), then the resident buffers at x2
    J0, g0, c0, G0 = eng.evaluate_J(x2, True), eng.evaluate_g(x2, False), eng.evaluate_c(x2, False), eng.evaluate_G_nonzeros(x2, False)
    lib = eng._lib
    lib.pc_device_results.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]

    def results():
        p = [C.c_void_p() for _ in range(3)]
        assert lib.pc_device_results(eng._h, *[C.byref(q) for q in p])
        return [q.value for q in p]

    ptrs0 = results()
    dev0 = [_device_copy(eng, p, k) for p, k in zip(ptrs0, (eng.num_c, eng.nnz_jac, eng.nnz_hess)) if p]
    a = eng.check_derivatives(x, 1.0, lam, return_fd=True)
    b = eng.check_derivatives(x, 1.0, lam, return_fd=True)
    fd_a = (a.jac_fd, a.hess_fd, a.jgrad_fd)
    fd_b = (b.jac_fd, b.hess_fd, b.jgrad_fd)
    a.jac_fd = a.hess_fd = a.jgrad_fd = b.jac_fd = b.hess_fd = b.jgrad_fd = None
    assert a == b
    for u, v in zip(fd_a, fd_b):
        assert u.tobytes() == v.tobytes()
    # the companions (new_x = 0) still see x2's values; the device results are where and what they were
    assert eng.evaluate_J(x2, False) == J0
    for got, ref in ((eng.evaluate_g(x2, False), g0), (eng.evaluate_c(x2, False), c0), (eng.evaluate_G_nonzeros(x2, False), G0)):
        assert got.tobytes() == ref.tobytes()
    ptrs1 = results()
    assert ptrs1 == ptrs0
    dev1 = [_device_copy(eng, p, k) for p, k in zip(ptrs1, (eng.num_c, eng.nnz_jac, eng.nnz_hess)) if p]
    for u, v in zip(dev0, dev1):
        assert u.tobytes() == v.tobytes()
    # a fresh evaluation: the same bits before and after a check
    e0 = eng.evaluate_all(x2, 1.0, lam)
    eng.check_derivatives(x, 1.0, lam)
    e1 = eng.evaluate_all(x2, 1.0, lam)
    for u, v in zip(e0, e1):
        assert u.tobytes() == v.tobytes()
    # a tile-restricted handle is refused
    n_tiles = len(eng.phase_tiles(0)[0]) - 1
    eng.set_tile_range(0, 0, n_tiles - 1)
    with pytest.raises(RuntimeError, match="tile range"):
        eng.check_derivatives(x, 1.0, lam)
    eng.close()


def test_solve_ocp_checks_every_mesh_iteration(built):
    from pycollo_amd.solve import solve_ocp
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        on = solve_ocp(problems.brachistochrone(), check_nlp_functions=True)
    off = solve_ocp(problems.brachistochrone())
    assert on.mesh_iterations == off.mesh_iterations
    assert on.objective == off.objective
    for a, b in zip(on.iterations, off.iterations):
        assert a["derivative_check"].ok
        assert "derivative_check" not in b
        assert a["nlp_iterations"] == b["nlp_iterations"] and a["objective"] == b["objective"]


def test_backend_check_nlp_functions(built):
    import pycollo_stub as stub
    from pycollo_amd.iteration import MeshIteration
    from pycollo_amd.pycollo_backend import Mi355x
    ocp, counts = stub.brachistochrone()
    ocp.settings.check_nlp_functions = True
    be = Mi355x(ocp, device=0)
    mi = MeshIteration(problems.brachistochrone())
    it = stub.iteration(ocp, mi.engine.V_ocp, mi.engine.r_ocp, mi.W_ocp, mi.w)
    it.guess_x = mi.guess_x_tilde
    be.generate_nlp_function_callables(it)
    be.create_nlp_solver()
    chk = be.check_nlp_functions()
    assert chk is not None and chk.ok and be.derivative_check is chk
    ocp.settings.check_nlp_functions = False
    assert be.check_nlp_functions() is None and be.derivative_check is None
    be.engine.close()
    mi.engine.close()
