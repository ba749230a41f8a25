"""Propagation with integrals and dense output (pycollo_amd/solution.py ``Solution.propagate_dense``, csrc/pc_solution.hpp
``pc_sol_propagate_dense_p<i>``) on the GPU.

The reference is tests/propagate_dense_ref.py, the tests' own restatement of the definition, itself checked on the CPU
by tests/test_propagate_dense_ref_cpu.py.  It is fed the kernel's own node values and coefficient arrays, so only the
propagation is under test.  The cases are the small meshes of ``propagate_ref.CASES`` (the hypersensitive phases of 0.02
time units, the ragged cart pole, the two-phase transfer, the phase without controls) and the sliding mass, whose
phases have no integral.  The queries of a phase: every node, two points inside every node interval, a node and an
inner point twice, shuffled (``propagate_dense_ref.sample_queries``).

1. Without ``integral_atol``, ``y``, ``accepted``, ``rejected`` and ``status`` equal ``Solution.propagate``'s bit for
   bit: fixed m in {1, 3}, adaptive rtol in {1e-6, 1e-10}, nodes / sections / phase, with and without queries.
2. Fixed mode: ``q``, ``y_dense`` and ``q_dense`` (and ``y``) entry by entry against the 60-digit restatement,
   |got - ref| <= 1e-10 |ref| + 64 eps n M, n the steps of the segment up to the one that answers, M as
   propagate_dense_ref says (the integrand stages and h sum_i |K_i| |b_i(theta)| included).  The float64 restatement
   stays within 7.6e-4 of that bound on every case (CPU test), which is what entitles the kernel to it.
3. Queries at the node abscissae return ``y`` and ``q`` bit for bit, a query at tau_0 returns y(0) and 0, permuted
   queries give permuted values, a repeated query equal bits.
4. Adaptive mode: ``y_dense`` within 10 (atol + rtol |y|) of the float64 restatement's; with ``integral_atol`` the steps
   are no fewer, and ``q`` is within a (integral_atol + rtol max|I|) of the 60-digit fixed-mode truth (substeps
   ``TRUTH_M``), a the accepted steps in the segment up to the node.  The restatement meets that at all 18 combinations
   (CPU, largest ratio 0.26): none is dropped.
5. The cap: on the 0.02-unit phase with max_steps = 1 at rtol 1e-6 the dense values and the integrals are NaN exactly
   behind the failure and bit-equal to the uncapped run elsewhere.
6. The conventions of ``pc_solution``: host and device variants and a repeated call agree bit for bit, the handle is
   left as found, bad arguments raise ``ValueError`` before any launch and the C calls refuse them too.
7. End to end on the hypersensitive problem (K = 10, order 4, NLP tolerance 1e-10; the brachistochrone carries no
   integral), against the CPU figures of DESIGN 8g (test_propagate_dense_ref_cpu.py recomputes them): ``integral_defect``
   of the open-loop pass and of the per-node restart at rtol 1e-10 and the largest |y_dense - sample| over 33 points per
   section, each within a factor 2.  Printed, and appended to the file PYCOLLO_AMD_PROPAGATE_DENSE_REPORT names.
"""
import ctypes as C
import os

import numpy as np
import pytest

import propagate_dense_ref as pd
import propagate_ref as pr
from conftest import golden_tables
from oracle.ref_numpy import OracleNlp
from test_propagate_dense_ref_cpu import (CPU_DENSE_GAP, CPU_INTEGRAL_DEFECT_NODES, CPU_INTEGRAL_DEFECT_PHASE, DENSE_CASES,
                                          RESTARTS)
from test_propagate_ref_cpu import ADAPTIVE_CASES, TRUTH_M

pytestmark = pytest.mark.gpu


def _smooth_x(eng):
    """the smooth random point of test_gpu_solution.py / test_gpu_propagate.py"""
    rng = np.random.default_rng(5)
    x = np.zeros(eng.num_x)
    for pl, mesh in zip(eng.layout.phases, eng.meshes):
        for b in range(pl.n_z):
            cf = rng.uniform(-0.15, 0.15, 4)
            x[pl.x_off + b * pl.N:pl.x_off + (b + 1) * pl.N] = np.polynomial.polynomial.polyval(mesh.tau, cf)
        x[pl.q_off:pl.q_off + pl.n_q + pl.n_t] = rng.uniform(0.1, 0.3, pl.n_q + pl.n_t)
    x[eng.layout.s_off:] = rng.uniform(-0.2, 0.2, eng.layout.n_s)
    return x


class Case:
    def __init__(self, name):
        from pycollo_amd.engine import NlpEngine
        from pycollo_amd.solution import Solution
        self.name = name
        self.prob = DENSE_CASES[name]()
        self.eng = NlpEngine(self.prob, device=0)
        self.ora = OracleNlp(self.prob, golden_tables(self.eng.quad.method), V_ocp=self.eng.V_ocp, r_ocp=self.eng.r_ocp,
                             W_ocp=self.eng.W_ocp)
        self.x = _smooth_x(self.eng)
        self.c_before = self.eng.evaluate_c(self.x).copy()
        self.G_before = self.eng.evaluate_G_nonzeros(self.x).copy()
        self.sol = Solution(self.eng, self.x)
        self.phases = range(len(self.eng.meshes))
        self.data = [pd.DenseData.from_solution(self.sol, self.ora, ip) for ip in self.phases]
        self.ref = [pd.DenseFixedReference(d) for d in self.data]
        self.tq = [pd.sample_queries(d) for d in self.data]

    def close(self):
        self.sol.close()
        self.eng.close()


_cases = {}


@pytest.fixture(scope="module")
def case(built):
    def get(name):
        if name not in _cases:
            _cases[name] = Case(name)
        return _cases[name]
    yield get
    for c in _cases.values():
        c.close()
    _cases.clear()


def _same_bits(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), what


# ---- 1. the steps are propagate's ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DENSE_CASES))
def test_without_integral_atol_the_steps_are_propagates(case, name):
    cs = case(name)
    for ip in cs.phases:
        for restart in RESTARTS:
            for kw in (dict(substeps=1), dict(substeps=3), dict(rtol=1e-6), dict(rtol=1e-10)):
                want = cs.sol.propagate(ip, restart=restart, **kw)
                for tq in (None, cs.tq[ip]):
                    got = cs.sol.propagate_dense(ip, tau=tq, restart=restart, **kw)
                    for key in ("y", "accepted", "rejected", "status", "defect", "relative_defect", "terminal_defect", "ok"):
                        _same_bits(getattr(got, key), getattr(want, key), f"{name} phase {ip} {restart} {kw} {key}")
                    np.testing.assert_array_equal(got.segments, want.segments)


# ---- 2. fixed-mode parity ----------------------------------------------------------------------------------------------
def _assert_parity(got, ref, what):
    val, n, M = ref
    assert got.shape == val.shape, what
    assert np.all(np.isfinite(got)), f"{what}: a value is not finite"
    bound = pd.parity_bound(val, n, M)
    diff = np.abs(got - val)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(diff == 0.0, 0.0, diff / bound)                   # (bound 0: the start, which must be exact)
    worst = float(np.max(ratio)) if ratio.size else 0.0
    print(f"{what}: largest |got - ref| / bound = {worst:.3e}")
    assert worst <= 1.0, f"{what} differs from the 60-digit restatement by {worst:.3e} x its bound"


@pytest.mark.parametrize("restart", RESTARTS)
@pytest.mark.parametrize("substeps", [1, 3])
@pytest.mark.parametrize("name", list(DENSE_CASES))
def test_fixed_mode_matches_the_60_digit_restatement(case, name, substeps, restart):
    cs = case(name)
    for ip in cs.phases:
        d = cs.data[ip]
        want = cs.ref[ip].run(pr.segments(restart, d.s, d.N), substeps, cs.tq[ip])
        got = cs.sol.propagate_dense(ip, tau=cs.tq[ip], restart=restart, substeps=substeps)
        for key, arr in (("y_arrive", got.y), ("q_arrive", got.q), ("y_dense", got.y_dense), ("q_dense", got.q_dense)):
            _assert_parity(arr, want[key], f"{name} phase {ip} m = {substeps} {restart} {key}")
        assert np.all(got.ok)
        total = np.zeros(d.n_q)
        for j in got.segments[1:]:                                         # the segments' integrals, first to last
            total = total + got.q[:, j]
        np.testing.assert_array_equal(got.integral, total)
        np.testing.assert_array_equal(got.integral_defect, got.integral - cs.sol.integral[ip])
        np.testing.assert_array_equal(got.u_dense, cs.sol.sample(ip, tau=got.tau)[2])
        np.testing.assert_array_equal(got.tau, cs.tq[ip])


# ---- 3. the ownership rule -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hypersensitive_K5_n4", "cart_pole_ragged_K23", "two_phase_transfer_K6", "sliding_mass_n4"])
def test_nodes_permutations_and_repeats(case, name):
    cs = case(name)
    rng = np.random.default_rng(2)
    for ip in cs.phases:
        d = cs.data[ip]
        for restart in RESTARTS:
            for kw in (dict(substeps=2), dict(rtol=1e-8)):
                at_nodes = cs.sol.propagate_dense(ip, tau=d.tau, restart=restart, **kw)
                _same_bits(at_nodes.y_dense, at_nodes.y, "the nodes return the arrivals")
                _same_bits(at_nodes.q_dense, at_nodes.q, "the nodes return the arriving integrals")
                _same_bits(at_nodes.y_dense[:, 0], d.node_y[:, 0])
                assert np.all(at_nodes.q_dense[:, 0] == 0.0) and np.all(at_nodes.q[:, 0] == 0.0)
                tq = cs.tq[ip]
                one = cs.sol.propagate_dense(ip, tau=tq, restart=restart, **kw)
                perm = rng.permutation(len(tq))
                two = cs.sol.propagate_dense(ip, tau=tq[perm], restart=restart, **kw)
                _same_bits(two.y_dense, one.y_dense[:, perm])
                _same_bits(two.q_dense, one.q_dense[:, perm])
                _, first, count = np.unique(tq, return_index=True, return_counts=True)
                assert np.sum(count == 2) == 2                              # (sample_queries repeats a node and an inner point)
                for v in tq[first[count == 2]]:
                    i0, i1 = np.nonzero(tq == v)[0]
                    _same_bits(one.y_dense[:, i0], one.y_dense[:, i1])
                    _same_bits(one.q_dense[:, i0], one.q_dense[:, i1])


# ---- 4. adaptive mode --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("restart", RESTARTS)
@pytest.mark.parametrize("name", ADAPTIVE_CASES)
def test_adaptive_mode(case, name, restart):
    cs = case(name)
    for ip in cs.phases:
        d, tq = cs.data[ip], cs.tq[ip]
        seg = pr.segments(restart, d.s, d.N)
        V = cs.sol.state_scale(ip)
        truth_I = cs.ref[ip].run(seg, TRUTH_M[name])["q_arrive"][0]
        for rtol in (1e-6, 1e-10):
            atol = rtol * V
            res = cs.sol.propagate_dense(ip, tau=tq, restart=restart, rtol=rtol)            # atol = None: rtol V
            host = pd.propagate_dense_f64(d, seg, tq, rtol=rtol, atol=atol)
            assert np.all(res.ok) and np.all(np.isfinite(res.y_dense)) and np.all(np.isfinite(res.q_dense))
            close = float(np.max(np.abs(res.y_dense - host["y_dense"]) / (10.0 * (atol[:, None] + rtol * np.abs(host["y_dense"])))))
            tight = cs.sol.propagate_dense(ip, tau=tq, restart=restart, rtol=rtol, integral_atol=rtol)
            assert np.all(tight.ok)
            steps, steps_tight = int(res.accepted.sum() + res.rejected.sum()), int(tight.accepted.sum() + tight.rejected.sum())
            bound = pd.integral_adaptive_bound(seg, truth_I, tight.accepted, rtol, rtol)
            ratio = float(np.max(np.abs(tight.q - truth_I)[:, 1:] / bound[:, 1:]))
            print(f"{name} phase {ip} {restart} rtol {rtol:g}: dense y against the float64 restatement {close:.3e} x its allowance; "
                  f"steps {steps} -> {steps_tight} with integral_atol; integral error / bound = {ratio:.3e}")
            assert close <= 1.0
            assert steps_tight >= steps
            assert ratio <= 1.0


def test_integral_atol_has_no_effect_in_fixed_mode(case):
    cs = case("hypersensitive_K5_n4")
    a = cs.sol.propagate_dense(0, tau=cs.tq[0], substeps=2)
    b = cs.sol.propagate_dense(0, tau=cs.tq[0], substeps=2, integral_atol=1e-12)
    for key in ("y", "q", "y_dense", "q_dense", "accepted", "rejected"):
        _same_bits(getattr(a, key), getattr(b, key), key)


# ---- 5. the cap ----------------------------------------------------------------------------------------------------------
def test_the_cap_leaves_nan_exactly_behind_the_failure(case):
    cs = case("hypersensitive_K5_n4")
    d, tq = cs.data[0], cs.tq[0]
    seg = pr.segments("sections", d.s, d.N)
    free = cs.sol.propagate_dense(0, tau=tq, restart="sections", rtol=1e-6)
    capped = cs.sol.propagate_dense(0, tau=tq, restart="sections", rtol=1e-6, max_steps=1)
    plain = cs.sol.propagate(0, restart="sections", rtol=1e-6, max_steps=1)
    for key in ("y", "accepted", "rejected", "status"):
        _same_bits(getattr(capped, key), getattr(plain, key), key)
    assert np.all(free.ok) and not capped.ok.all() and capped.ok.any()
    slot = np.searchsorted(d.tau, tq, side="left")                         # the node whose interval owns the query
    for i in range(len(seg) - 1):
        j0, j1 = int(seg[i]), int(seg[i + 1])
        fail = int(capped.status[i])
        mine = (slot > j0) & (slot <= j1) if j0 else (slot <= j1)
        if fail < 0:
            good = mine
        else:
            # behind the failure: the failing interval's own queries (it has no accepted step: max_steps = 1) and later
            bad = mine & (slot > fail)
            good = mine & (slot <= fail)
            assert bad.any()
            assert np.all(np.isnan(capped.y_dense[:, bad])) and np.all(np.isnan(capped.q_dense[:, bad]))
            assert np.all(np.isnan(capped.q[:, fail + 1:j1 + 1]))
            assert capped.accepted[fail + 1] == 0 and capped.rejected[fail + 1] == 1
        _same_bits(capped.y_dense[:, good], free.y_dense[:, good])
        _same_bits(capped.q_dense[:, good], free.q_dense[:, good])
        upto = j1 if fail < 0 else fail
        _same_bits(capped.q[:, j0 + 1:upto + 1], free.q[:, j0 + 1:upto + 1])
        assert np.all(np.isfinite(capped.y_dense[:, good]))
    assert np.isnan(capped.integral).all() and np.isfinite(free.integral).all()


# ---- 6. the conventions of pc_solution -----------------------------------------------------------------------------------
def test_repeatable_and_host_and_device_variants_agree(case):
    import torch
    cs = case("cart_pole_ragged_K23")
    tq = cs.tq[0]
    keys = ("y", "defect", "relative_defect", "accepted", "rejected", "status", "ok", "terminal_defect", "q", "integral",
            "integral_defect", "y_dense", "q_dense", "u_dense")
    for kw in (dict(substeps=2), dict(rtol=1e-8), dict(rtol=1e-8, integral_atol=1e-9)):
        a = cs.sol.propagate_dense(0, tau=tq, restart="sections", **kw)
        b = cs.sol.propagate_dense(0, tau=tq, restart="sections", **kw)
        dev = cs.sol.propagate_dense(0, tau=torch.tensor(tq, dtype=torch.float64, device="cuda:0"), restart="sections", **kw)
        for name in keys:
            p, q, t = getattr(a, name), getattr(b, name), getattr(dev, name)
            _same_bits(p, q, name)
            assert isinstance(t, torch.Tensor) and t.is_cuda, name
            _same_bits(p, t.cpu().numpy(), name)
        none = cs.sol.propagate_dense(0, restart="sections", **kw)            # Q = 0: the integrals only
        assert none.y_dense.shape == (4, 0) and none.q_dense.shape == (1, 0) and none.u_dense.shape == (1, 0)
        _same_bits(none.q, a.q)
        _same_bits(none.integral, a.integral)
    t = cs.sol.initial_time[0] + 0.5 * (tq + 1.0) * (cs.sol.final_time[0] - cs.sol.initial_time[0])
    by_time = cs.sol.propagate_dense(0, t, restart="phase", substeps=2)
    by_tau = cs.sol.propagate_dense(0, tau=by_time.tau, restart="phase", substeps=2)
    _same_bits(by_time.y_dense, by_tau.y_dense)
    assert np.max(np.abs(by_time.tau - tq)) <= 8 * np.finfo(float).eps


@pytest.mark.parametrize("name", ["cart_pole_ragged_K23", "two_phase_transfer_K6"])
def test_handle_is_left_as_found(case, name):
    cs = case(name)
    eng = cs.eng
    cs.sol.propagate_dense(0, tau=cs.tq[0], restart="nodes", rtol=1e-8)
    np.testing.assert_array_equal(eng.evaluate_c(cs.x), cs.c_before)
    np.testing.assert_array_equal(eng.evaluate_G_nonzeros(cs.x), cs.G_before)
    c1 = eng.evaluate_c(cs.x, new_x=True).copy()
    last = len(cs.data) - 1
    cs.sol.propagate_dense(last, tau=cs.tq[last], restart="sections", substeps=2)
    assert eng.cache_holds(cs.x)
    np.testing.assert_array_equal(eng.evaluate_c(cs.x, new_x=False), c1)
    np.testing.assert_array_equal(eng.evaluate_G_nonzeros(cs.x), cs.G_before)


def test_bad_arguments_raise_before_any_launch(case):
    cs = case("hypersensitive_K5_n4")
    N = cs.data[0].N
    t0, tF = cs.sol.initial_time[0], cs.sol.final_time[0]
    for kw in (dict(tau=[1.5]), dict(tau=[np.nan]), dict(tau=[np.nextafter(-1.0, -2.0)]), dict(t=[tF + 1.0]), dict(t=[np.nan]),
               dict(t=[t0 - 1e-3]), dict(t=[0.0], tau=[0.0]), dict(integral_atol=0.0), dict(integral_atol=-1.0),
               dict(integral_atol=np.nan), dict(integral_atol=[1e-9, 1e-9]), dict(substeps=-1), dict(rtol=0.0), dict(atol=0.0),
               dict(max_steps=0), dict(restart="mesh"), dict(restart=np.array([0, 4, 4, N - 1]))):
        with pytest.raises(ValueError):
            cs.sol.propagate_dense(0, **kw)
    with pytest.raises(ValueError):
        cs.sol.propagate_dense(1)
    # the C calls make the same refusals themselves
    lib, h = cs.sol._lib, cs.sol._h
    y, q = np.empty((1, N)), np.empty((1, N))
    acc, rej, st = np.empty(N, np.int32), np.empty(N, np.int32), np.empty(N, np.int32)
    yd, qd = np.empty((1, 4)), np.empty((1, 4))
    seg, atol = np.array([0, N - 1], dtype=np.int32), np.array([1e-9])

    def call(n_seg=1, substeps=0, rtol=1e-9, at=atol, iat=None, max_steps=4096, tq=np.array([0.0, -1.0, 1.0, 0.0])):
        return lib.pc_solution_propagate_dense(h, 0, n_seg, seg.ctypes.data, substeps, C.c_double(rtol), at.ctypes.data,
                                               None if iat is None else iat.ctypes.data, max_steps, len(tq), tq.ctypes.data,
                                               y.ctypes.data, acc.ctypes.data, rej.ctypes.data, st.ctypes.data, q.ctypes.data,
                                               yd.ctypes.data, qd.ctypes.data)
    assert call() and call(iat=np.array([1e-9])) and call(tq=np.zeros(0))
    assert not call(tq=np.array([0.0, 1.5])) and not call(tq=np.array([np.nan])) and not call(tq=np.array([-np.inf]))
    assert b"propagate" in lib.pc_last_error()
    assert not call(iat=np.array([0.0])) and not call(iat=np.array([np.nan])) and not call(iat=np.array([-1e-9]))
    assert not call(n_seg=0) and not call(substeps=-1) and not call(rtol=0.0) and not call(at=np.array([0.0]))
    assert not call(max_steps=0)
    assert b"propagate" in lib.pc_last_error()


def test_backend_solution_propagates_densely(case):
    from pycollo_amd.pycollo_backend import Mi355x
    cs = case("hypersensitive_K5_n4")
    b = Mi355x(device=0)
    b.engine = cs.eng
    s = b.solution(cs.x)
    try:
        got, want = s.propagate_dense(0, tau=cs.tq[0], substeps=2), cs.sol.propagate_dense(0, tau=cs.tq[0], substeps=2)
        _same_bits(got.y_dense, want.y_dense)
        _same_bits(got.q, want.q)
    finally:
        s.close()
        b.engine = None


# ---- 7. end to end ---------------------------------------------------------------------------------------------------
def _report(line):
    print(line)
    path = os.environ.get("PYCOLLO_AMD_PROPAGATE_DENSE_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def test_solve_ocp_end_to_end(built):
    from pycollo_amd import problems
    from pycollo_amd.solve import solve_ocp
    result = solve_ocp(problems.hypersensitive(K=10, order=4), max_mesh_iterations=1)      # the K = 10 mesh itself, not refined
    sol = result.solution
    try:
        mesh = sol.engine.meshes[0]
        edges = np.asarray(mesh.tau)[np.asarray(mesh.s)]
        c = np.linspace(-1.0, 1.0, 33)
        tq = edges[:-1, None] + 0.5 * (c[None, :] + 1.0) * (edges[1:, None] - edges[:-1, None])
        tq[:, 0], tq[:, -1] = edges[:-1], edges[1:]
        tq = tq.reshape(-1)
        one = sol.propagate_dense(0, tau=tq, restart="phase", rtol=1e-10)
        per = sol.propagate_dense(0, restart="nodes", rtol=1e-10)
        assert one.ok.all() and per.ok.all()
        phase, nodes = float(np.max(np.abs(one.integral_defect))), float(np.max(np.abs(per.integral_defect)))
        gap = float(np.max(np.abs(one.y_dense - sol.sample(0, tau=tq)[0])))
        _report(f"hypersensitive K=10 n=4 on the GPU: objective {result.objective:.10f}; |integral_defect| (phase) {phase:.5e} "
                f"[CPU {CPU_INTEGRAL_DEFECT_PHASE:.5e}], (nodes) {nodes:.5e} [CPU {CPU_INTEGRAL_DEFECT_NODES:.5e}]; largest "
                f"|y_dense - sample| {gap:.4e} [CPU {CPU_DENSE_GAP:.4e}]; steps {int(one.accepted.sum())} + "
                f"{int(one.rejected.sum())} rejected")
        assert CPU_INTEGRAL_DEFECT_PHASE / 2 <= phase <= 2 * CPU_INTEGRAL_DEFECT_PHASE
        assert CPU_INTEGRAL_DEFECT_NODES / 2 <= nodes <= 2 * CPU_INTEGRAL_DEFECT_NODES
        assert CPU_DENSE_GAP / 2 <= gap <= 2 * CPU_DENSE_GAP
    finally:
        sol.close()
        result.final.engine.close()
