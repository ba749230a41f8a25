"""Forward propagation of a Solution under its own controls (pycollo_amd/solution.py ``Solution.propagate``,
csrc/pc_solution.hpp ``pc_sol_propagate_p<i>``) on the GPU.

The reference is tests/propagate_ref.py, the tests' own restatement of the definition, itself checked on the CPU by
tests/test_propagate_ref_cpu.py.  It is fed the kernel's own node values and coefficient arrays
(``Solution.coefficients``), so only the propagation is under test.

1. Fixed mode, every case x substeps {1, 3} x restart {nodes, sections, phase, irregular}, entry by entry against the
   60-digit restatement: |got - ref| <= 1e-10 |ref| + 64 eps n M, n the steps taken in the segment up to the node, M
   the largest |y| + |h g| sum_i |b_i| F_i over those steps (F_i: stage i's f with every term in absolute value).  The
   float64 restatement stays within that bound on every case (CPU test), which is what entitles the kernel to it.
   The meshes are those of tests/test_gpu_solution.py; the hypersensitive phases last 0.02 time units
   (propagate_ref.CASES says why: with a final time of 10 the fixed mode overflows at the smooth point).
2. Where two restarts run the same arithmetic they agree bit for bit.
3. One fixed step per interval is exact on the sliding mass (x is a quintic), by the bound of 1.
4. Adaptive mode against the 60-digit fixed-mode truth (substeps ``TRUTH_M``, converged to 1e-14 on the CPU):
   |got - truth| <= a (atol + rtol max|y|) exp(L T), a the accepted steps in the segment up to the node, L the largest
   one-sided Lipschitz constant of f along the truth, T the time since the segment's start; and within
   10 (atol + rtol |y|) of the float64 restatement.  The combinations at which that restatement itself misses the
   bound (``ADAPTIVE_DROPPED``, three of 24) are not asked.
5. The cap.  On hypersensitive_K5_n4 with its final time left at 10 000, max_steps = 1 and rtol 1e-13, every segment
   fails at its first interval, and at any other rtol too (CPU test), so "arrivals before the failure" and "the other
   segments" are empty there; the same call on the 0.02 phase at rtol 1e-6 has both, and is held to all four
   properties.
6. The conventions of ``pc_solution``.
7. End to end on the brachistochrone, against the CPU figures of DESIGN 8e (test_propagate_ref_cpu.py recomputes
   them): the GPU's two figures within a factor 2.  Printed, and appended to the file PYCOLLO_AMD_PROPAGATE_REPORT names.
"""
import os

import numpy as np
import pytest

import propagate_ref as pr
from conftest import golden_tables
from oracle.ref_numpy import OracleNlp
from pycollo_amd import problems
from test_propagate_ref_cpu import (ADAPTIVE_CASES, ADAPTIVE_DROPPED, ADAPTIVE_RESTARTS, CPU_MAX_NODES, CPU_TERMINAL_PHASE,
                                    TRUTH_M)

pytestmark = pytest.mark.gpu

RESTARTS = ("nodes", "sections", "phase", "irregular")
CASES = dict(pr.CASES)
CASES["sliding_mass_n4"] = lambda: problems.sliding_mass(order=4)
CASES["hypersensitive_K5_n4_T10000"] = lambda: problems.hypersensitive(K=5, order=4)       # the cap test only


def _report(line):
    print(line)
    path = os.environ.get("PYCOLLO_AMD_PROPAGATE_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _smooth_x(eng):
    """the smooth random point of test_gpu_solution.py / test_gpu_refinement.py"""
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
        self.prob = CASES[name]()
        self.eng = NlpEngine(self.prob, device=0)
        self.ora = OracleNlp(self.prob, golden_tables(self.eng.quad.method), V_ocp=self.eng.V_ocp, r_ocp=self.eng.r_ocp,
                             W_ocp=self.eng.W_ocp)
        self.x = _smooth_x(self.eng)
        self.c_before = self.eng.evaluate_c(self.x).copy()
        self.G_before = self.eng.evaluate_G_nonzeros(self.x).copy()
        self.sol = Solution(self.eng, self.x)
        self.phases = range(len(self.eng.meshes))
        self.data = [pr.PhaseData.from_solution(self.sol, self.ora, ip) for ip in self.phases]
        self.ref = [pr.FixedReference(d) for d in self.data]

    def segments(self, ip, restart):
        d = self.data[ip]
        return pr.segments(restart, d.s, d.N)

    def run(self, ip, restart, **kw):
        """``Solution.propagate`` with the test's name of a segment list"""
        arg = restart if restart in ("nodes", "sections", "phase") else self.segments(ip, restart)
        return self.sol.propagate(ip, restart=arg, **kw)

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


def _assert_parity(got, ref, steps, M, what):
    assert got.shape == ref.shape
    assert np.all(np.isfinite(got)), f"{what}: an arrival is not finite"
    np.testing.assert_array_equal(got[:, 0], ref[:, 0])
    ratio = float(np.max(np.abs(got - ref)[:, 1:] / pr.parity_bound(ref, steps, M)[:, 1:]))
    print(f"{what}: largest |got - ref| / bound = {ratio:.3e}")
    assert ratio <= 1.0, f"{what} differs from the 60-digit restatement by {ratio:.3e} x its bound"


# ---- 1. fixed-mode parity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("restart", RESTARTS)
@pytest.mark.parametrize("substeps", [1, 3])
@pytest.mark.parametrize("name", list(pr.CASES))
def test_fixed_mode_matches_the_60_digit_restatement(case, name, substeps, restart):
    cs = case(name)
    for ip in cs.phases:
        d, seg = cs.data[ip], cs.segments(ip, restart)
        ref, steps, M = cs.ref[ip].arrivals(seg, substeps)
        res = cs.run(ip, restart, substeps=substeps)
        _assert_parity(res.y, ref, steps, M, f"{name} phase {ip} m = {substeps} {restart}")
        np.testing.assert_array_equal(res.segments, seg)
        np.testing.assert_array_equal(res.accepted, np.r_[0, np.full(d.N - 1, substeps)])
        np.testing.assert_array_equal(res.rejected, np.zeros(d.N))
        assert res.status.shape == (len(seg) - 1,) and np.all(res.status == -1) and np.all(res.ok)
        np.testing.assert_array_equal(res.defect, res.y - cs.sol.state[ip])
        np.testing.assert_array_equal(res.relative_defect, res.defect / cs.sol.state_scale(ip)[:, None])
        np.testing.assert_array_equal(res.terminal_defect, res.defect[:, -1])


# ---- 2. the modes agree where they run the same arithmetic -----------------------------------------------------------
@pytest.mark.parametrize("name", list(pr.CASES))
def test_modes_agree_bit_for_bit(case, name):
    cs = case(name)
    for ip in cs.phases:
        d = cs.data[ip]
        for m in (1, 3):
            nodes, secs, phase = (cs.run(ip, r, substeps=m).y for r in ("nodes", "sections", "phase"))
            np.testing.assert_array_equal(phase[:, 1], nodes[:, 1])
            np.testing.assert_array_equal(secs[:, 1], nodes[:, 1])
            first = d.s[:-1] + 1                                        # node s_k + 1 of every section
            np.testing.assert_array_equal(secs[:, first], nodes[:, first])
            listed = cs.sol.propagate(ip, restart=np.asarray(d.s, dtype=np.int64), substeps=m)
            np.testing.assert_array_equal(listed.y, secs)
            if d.K > 1:
                assert not np.array_equal(phase[:, -1], secs[:, -1])     # (the restarts are really taken)


# ---- 3. the sliding mass ---------------------------------------------------------------------------------------------
def test_one_step_is_exact_on_the_sliding_mass(case):
    cs = case("sliding_mass_n4")
    for ip in cs.phases:
        d, seg = cs.data[ip], cs.segments(ip, "sections")
        exact = pr.sliding_mass_exact(d)
        _, steps, M = cs.ref[ip].arrivals(seg, 1)
        res = cs.run(ip, "sections", substeps=1)
        _assert_parity(res.y, exact, steps, M, f"sliding mass phase {ip}: arrivals against the exact quintic")


# ---- 4. adaptive mode ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("restart", ADAPTIVE_RESTARTS)
@pytest.mark.parametrize("name", ADAPTIVE_CASES)
def test_adaptive_mode_within_the_textbook_bound(case, name, restart):
    cs = case(name)
    for ip in cs.phases:
        d, seg = cs.data[ip], cs.segments(ip, restart)
        V = cs.sol.state_scale(ip)
        truth = cs.ref[ip].arrivals(seg, TRUTH_M[name])[0]
        L = pr.lipschitz(d, truth)
        for rtol in (1e-6, 1e-10):
            res = cs.run(ip, restart, rtol=rtol)                            # atol = None: rtol V
            assert np.all(res.ok) and np.all(res.status == -1)
            assert np.all(res.rejected >= 0) and np.all(res.accepted[1:] >= 1) and res.accepted[0] == 0
            atol = rtol * V
            host = pr.propagate_f64(d, seg, rtol=rtol, atol=atol)[0]
            close = float(np.max(np.abs(res.y - host) / (10.0 * (atol[:, None] + rtol * np.abs(host)))))
            err = np.abs(res.y - truth)[:, 1:]
            ratio = float(np.max(err / pr.adaptive_bound(d, seg, truth, res.accepted, atol, rtol, L)[:, 1:]))
            print(f"{name} phase {ip} {restart} rtol {rtol:g}: error / bound = {ratio:.3e}, against the float64 restatement "
                  f"{close:.3e} x its allowance, {int(res.accepted.sum())} accepted, {int(res.rejected.sum())} rejected")
            assert close <= 1.0
            if (name, restart, rtol) not in ADAPTIVE_DROPPED:
                assert ratio <= 1.0


# ---- 5. the cap ------------------------------------------------------------------------------------------------------
def test_the_cap_at_final_time_10000_every_segment_fails_at_once(case):
    cs = case("hypersensitive_K5_n4_T10000")
    d, seg = cs.data[0], cs.segments(0, "sections")
    res = cs.run(0, "sections", rtol=1e-13, max_steps=1)
    np.testing.assert_array_equal(res.status, seg[:-1])                    # the first interval of every segment
    assert not res.ok.any()
    np.testing.assert_array_equal(res.y[:, 0], d.node_y[:, 0])
    assert np.all(np.isnan(res.y[:, 1:]))
    assert np.all(res.accepted + res.rejected <= 1)
    np.testing.assert_array_equal((res.accepted + res.rejected)[seg[:-1] + 1], np.ones(len(seg) - 1))


def test_the_cap_stops_one_segment_and_leaves_the_others(case):
    cs = case("hypersensitive_K5_n4")
    d, seg = cs.data[0], cs.segments(0, "sections")
    free = cs.run(0, "sections", rtol=1e-6)
    capped = cs.run(0, "sections", rtol=1e-6, max_steps=1)
    assert np.all(free.ok)
    needs_more = free.accepted + free.rejected > 1                         # per arrival node
    assert needs_more.any()
    some_before = False
    for i in range(len(seg) - 1):
        j0, j1 = int(seg[i]), int(seg[i + 1])
        over = np.nonzero(needs_more[j0 + 1:j1 + 1])[0]
        if len(over) == 0:
            assert capped.status[i] == -1 and capped.ok[i]
            np.testing.assert_array_equal(capped.y[:, j0 + 1:j1 + 1], free.y[:, j0 + 1:j1 + 1])
            continue
        fail = j0 + int(over[0])                                           # the interval (fail, fail + 1)
        assert capped.status[i] == fail and not capped.ok[i]
        assert np.all(np.isnan(capped.y[:, fail + 1:j1 + 1]))
        assert np.all(np.isfinite(capped.y[:, j0 + 1:fail + 1]))
        np.testing.assert_array_equal(capped.y[:, j0 + 1:fail + 1], free.y[:, j0 + 1:fail + 1])
        assert capped.accepted[fail + 1] + capped.rejected[fail + 1] == 1
        some_before |= fail > j0
    assert not capped.ok.all() and capped.ok.any()
    print(f"capped segments: {np.nonzero(~capped.ok)[0].tolist()} of {len(seg) - 1}; a failure behind finite arrivals: {some_before}")


# ---- 6. the conventions of pc_solution -------------------------------------------------------------------------------
def test_repeatable_and_host_and_device_variants_agree(case):
    import torch
    cs = case("cart_pole_ragged_K60")
    for kw in (dict(substeps=2), dict(rtol=1e-8)):
        a = cs.run(0, "sections", **kw)
        b = cs.run(0, "sections", **kw)
        seg_t = torch.tensor(cs.segments(0, "sections"), dtype=torch.int64, device="cuda:0")
        dev = cs.sol.propagate(0, restart=seg_t, **kw)
        for name in ("y", "defect", "relative_defect", "accepted", "rejected", "status", "ok", "terminal_defect"):
            p, q, t = getattr(a, name), getattr(b, name), getattr(dev, name)
            np.testing.assert_array_equal(p, q, err_msg=name)
            assert isinstance(t, torch.Tensor) and t.is_cuda, name
            np.testing.assert_array_equal(p, t.cpu().numpy(), err_msg=name)
        at = torch.tensor(1e-8 * cs.sol.state_scale(0), dtype=torch.float64, device="cuda:0")
        dev2 = cs.sol.propagate(0, restart="sections", atol=at, **kw)
        assert dev2.y.is_cuda
        np.testing.assert_array_equal(dev2.y.cpu().numpy(), a.y)          # (rtol V given as a tensor is the default atol)


@pytest.mark.parametrize("name", ["cart_pole_ragged_K23", "two_phase_transfer_K6"])
def test_handle_is_left_as_found(case, name):
    cs = case(name)
    eng = cs.eng
    cs.run(0, "nodes", rtol=1e-8)
    cs.run(0, "phase", substeps=2)
    np.testing.assert_array_equal(eng.evaluate_c(cs.x), cs.c_before)
    np.testing.assert_array_equal(eng.evaluate_G_nonzeros(cs.x), cs.G_before)
    # ... and in the middle of the callback protocol: the point cached by a new_x = True call survives
    c1 = eng.evaluate_c(cs.x, new_x=True).copy()
    cs.run(len(cs.data) - 1, "sections", rtol=1e-6)
    assert eng.cache_holds(cs.x)
    np.testing.assert_array_equal(eng.evaluate_c(cs.x, new_x=False), c1)
    np.testing.assert_array_equal(eng.evaluate_G_nonzeros(cs.x), cs.G_before)
    np.testing.assert_array_equal(c1, cs.c_before)


def test_bad_arguments_raise_before_any_launch(case):
    cs = case("hypersensitive_K5_n4")
    N = cs.data[0].N
    for bad in ([0, 4, 4, N - 1], [0, 5, 4, N - 1], [1, N - 1], [0, N - 2], [0]):
        with pytest.raises(ValueError):
            cs.sol.propagate(0, restart=np.array(bad))
    for kw in (dict(substeps=-1), dict(rtol=0.0), dict(rtol=-1e-9), dict(rtol=float("nan")), dict(atol=0.0),
               dict(atol=np.array([-1e-9])), dict(atol=float("inf")), dict(max_steps=0), dict(max_steps=(1 << 20) + 1),
               dict(restart="mesh")):
        with pytest.raises(ValueError):
            cs.sol.propagate(0, **kw)
    with pytest.raises(ValueError):
        cs.sol.propagate(1)
    # the C calls make the same refusals themselves
    import ctypes as C
    lib, h = cs.sol._lib, cs.sol._h
    y, acc, rej, st = np.empty((1, N)), np.empty(N, np.int32), np.empty(N, np.int32), np.empty(N, np.int32)
    good_seg, atol = np.array([0, N - 1], dtype=np.int32), np.array([1e-9])

    def call(seg=good_seg, n_seg=1, substeps=0, rtol=1e-9, at=atol, max_steps=4096):
        return lib.pc_solution_propagate(h, 0, n_seg, seg.ctypes.data, substeps, C.c_double(rtol), at.ctypes.data, max_steps,
                                         y.ctypes.data, acc.ctypes.data, rej.ctypes.data, st.ctypes.data)
    assert call()
    assert not call(seg=np.array([0, 3, 3, N - 1], dtype=np.int32), n_seg=3)
    assert not call(seg=np.array([1, N - 1], dtype=np.int32))
    assert not call(seg=np.array([0, N], dtype=np.int32))
    assert not call(n_seg=0) and not call(substeps=-1) and not call(rtol=0.0) and not call(rtol=float("nan"))
    assert not call(at=np.array([0.0])) and not call(at=np.array([np.nan]))
    assert not call(max_steps=0) and not call(max_steps=(1 << 20) + 1)
    assert b"propagate" in lib.pc_last_error()


def test_backend_solution_propagates(case):
    from pycollo_amd.pycollo_backend import Mi355x
    cs = case("hypersensitive_K5_n4")
    b = Mi355x(device=0)
    b.engine = cs.eng
    s = b.solution(cs.x)
    try:
        np.testing.assert_array_equal(s.propagate(0, substeps=2).y, cs.run(0, "nodes", substeps=2).y)
    finally:
        s.close()
        b.engine = None


# ---- 7. end to end ---------------------------------------------------------------------------------------------------
def test_solve_ocp_end_to_end(built):
    from pycollo_amd.solve import solve_ocp
    result = solve_ocp(problems.brachistochrone(K=10, order=4))
    sol = result.solution
    try:
        one = sol.propagate(0, restart="phase", rtol=1e-10)
        per = sol.propagate(0, restart="nodes", rtol=1e-10)
        assert one.ok.all() and per.ok.all()
        terminal = float(np.max(np.abs(one.relative_defect[:, -1])))
        nodes = float(np.max(np.abs(per.relative_defect)))
        np.testing.assert_array_equal(one.terminal_defect, one.defect[:, -1])
        _report(f"brachistochrone K=10 n=4 on the GPU: objective {result.objective:.10f}; relative defect at tF (phase) "
                f"{terminal:.3e} [CPU {CPU_TERMINAL_PHASE:.3e}], largest over the nodes (nodes) {nodes:.3e} [CPU {CPU_MAX_NODES:.3e}]; "
                f"steps {int(one.accepted.sum())} + {int(one.rejected.sum())} rejected")
        assert CPU_MAX_NODES / 2 <= nodes <= 2 * CPU_MAX_NODES
        assert CPU_TERMINAL_PHASE / 2 <= terminal <= 2 * CPU_TERMINAL_PHASE
    finally:
        sol.close()
        result.final.engine.close()
