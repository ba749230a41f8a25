"""The implicit method of ``Solution.propagate`` (``method="sdirk4"``; pycollo_amd/solution.py,
csrc/pc_solution.hpp ``pc_sol_propagate_stiff_p<i>``) on the GPU.

The reference is tests/propagate_stiff_ref.py, the tests' own restatement of the definition, itself checked on the CPU
by tests/test_propagate_stiff_ref_cpu.py.  It is fed the kernel's own node values and coefficient arrays
(``Solution.coefficients``), so only the propagation is under test.  The ``Case`` pattern is that of
tests/test_gpu_propagate.py, restated.  Meshes have 5 .. 23 sections (``cart_pole_ragged_K60`` stays on the CPU).

7.  Fixed mode, every case x substeps {1, 3} x four restarts, against the exact step of the method (60 digits):
    |got - exact| <= n (atol_a + rtol max|y_a|) exp(L T), the bound the float64 restatement keeps on the CPU; at the
    inputs of that test (rtol 1e-6, newton_max = 16).
8.  Adaptive mode on the stiff relaxation phase against its exact flow, |got - exact| <= a (atol_a + rtol max|y_a|), and
    on the hypersensitive phase at its own final time of 10 000 (every segment completes) against the 60-digit truth of
    tests/golden/propagate_stiff_headline.npz by the same bound; everywhere within
    10 (atol + rtol |y|) of the float64 restatement, and the four counts equal to the restatement's in every interval
    up to the segment's first decision within relative 1e-6 of its threshold.
9.  The stiff contrast: under max_steps = 256 the implicit method completes the stiff relaxation phase and the
    explicit pair runs into the cap.
10. The failure convention: fixed mode, newton_max = 8 on the order-extremes mesh fails one interval of several (CPU
    test), and status, NaN, the other arrivals' bits and ``ok`` are the restatement's.
11. Where two restarts run the same arithmetic they agree bit for bit.
12. The conventions of ``pc_solution``.
"""
import numpy as np
import pytest

import propagate_ref as pr
import propagate_stiff_ref as ps
from conftest import golden_tables
from oracle.ref_numpy import OracleNlp
from pycollo_amd import problems
from test_propagate_stiff_ref_cpu import (ADAPTIVE_DROPPED, ADAPTIVE_RESTARTS, ADAPTIVE_RTOLS, FAILURE_CASE, FIXED_DROPPED,
                                          FIXED_NEWTON_MAX, FIXED_RTOL, HEADLINE_DROPPED, HEADLINE_RTOL, NEAR, fixed_lipschitz,
                                          headline_truth)

pytestmark = pytest.mark.gpu

RESTARTS = ("nodes", "sections", "phase", "irregular")
FIXED_CASES = [n for n in pr.CASES if n != "cart_pole_ragged_K60"] + [ps.STIFF_CASE]
CASES = dict(pr.CASES)
CASES[ps.STIFF_CASE] = ps.stiff_case
CASES["hypersensitive_K5_n4_T10000"] = lambda: problems.hypersensitive(K=5, order=4)


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
        self.exact = [ps.ExactFixed(d) for d in self.data]

    def segments(self, ip, restart):
        d = self.data[ip]
        return pr.segments(restart, d.s, d.N)

    def run(self, ip, restart, **kw):
        """``Solution.propagate(method="sdirk4")`` with the test's name of a segment list"""
        arg = restart if restart in ("nodes", "sections", "phase") else self.segments(ip, restart)
        kw.setdefault("method", "sdirk4")
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


def _counts_match(res, R, seg, what):
    """the four counts equal the restatement's in every interval up to the segment's first near-threshold decision"""
    asked = 0
    for i in range(len(seg) - 1):
        for j in range(int(seg[i]) + 1, int(seg[i + 1]) + 1):
            if R.near[j] < NEAR:
                break
            asked += 1
            got = (res.accepted[j], res.rejected[j], res.newton_rejected[j], res.newton_iterations[j])
            ref = (R.accepted[j], R.rejected[j], R.newton_rejected[j], R.newton_iterations[j])
            assert got == tuple(int(v) for v in ref), f"{what}: the counts of the interval that ends at node {j} are {got}, not {ref}"
    return asked


# ---- 7. fixed mode ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("restart", RESTARTS)
@pytest.mark.parametrize("substeps", [1, 3])
@pytest.mark.parametrize("name", FIXED_CASES)
def test_fixed_mode_matches_the_exact_step(case, name, substeps, restart):
    cs = case(name)
    for ip in cs.phases:
        d, seg = cs.data[ip], cs.segments(ip, restart)
        atol = FIXED_RTOL * cs.sol.state_scale(ip)
        exact = cs.exact[ip].arrivals(seg, substeps)[0]
        L = fixed_lipschitz(name, d, exact)
        res = cs.run(ip, restart, substeps=substeps, rtol=FIXED_RTOL, newton_max=FIXED_NEWTON_MAX)       # atol = None: rtol V
        assert np.all(res.ok) and np.all(res.status == -1) and np.all(np.isfinite(res.y))
        np.testing.assert_array_equal(res.y[:, 0], exact[:, 0])
        bound = ps.fixed_bound(d, seg, exact, substeps, atol, FIXED_RTOL, L)
        ratio = float(np.max(np.abs(res.y - exact)[:, 1:] / bound[:, 1:]))
        print(f"{name} phase {ip} m = {substeps} {restart}: |got - exact| / bound = {ratio:.3e}, "
              f"{int(res.newton_iterations.sum())} Newton iterations")
        if (name, substeps, restart) not in FIXED_DROPPED:
            assert ratio <= 1.0
        np.testing.assert_array_equal(res.segments, seg)
        np.testing.assert_array_equal(res.accepted, np.r_[0, np.full(d.N - 1, substeps)])
        np.testing.assert_array_equal(res.rejected, np.zeros(d.N))
        np.testing.assert_array_equal(res.newton_rejected, np.zeros(d.N))
        assert res.newton_iterations[0] == 0 and np.all(res.newton_iterations[1:] >= 5 * substeps)
        assert np.all(res.newton_iterations[1:] <= 5 * substeps * FIXED_NEWTON_MAX)
        np.testing.assert_array_equal(res.defect, res.y - cs.sol.state[ip])
        np.testing.assert_array_equal(res.terminal_defect, res.defect[:, -1])


# ---- 8. adaptive mode ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("restart", ADAPTIVE_RESTARTS)
def test_adaptive_mode_on_the_stiff_relaxation_phase(case, restart):
    cs = case(ps.STIFF_CASE)
    d, seg = cs.data[0], cs.segments(0, restart)
    V = cs.sol.state_scale(0)
    exact = ps.relaxation_exact(d, seg)
    for rtol in ADAPTIVE_RTOLS:
        atol = rtol * V
        res = cs.run(0, restart, rtol=rtol)
        assert np.all(res.ok) and np.all(res.status == -1)
        assert np.all(res.accepted[1:] >= 1) and res.accepted[0] == 0
        R = ps.propagate_f64(d, seg, rtol=rtol, atol=atol)
        close = float(np.max(np.abs(res.y - R.y) / (10.0 * (atol[:, None] + rtol * np.abs(R.y)))))
        ratio = float(np.max(np.abs(res.y - exact)[:, 1:] / pr.adaptive_bound(d, seg, exact, res.accepted, atol, rtol, 0.0)[:, 1:]))
        print(f"stiff relaxation {restart} rtol {rtol:g}: error / bound = {ratio:.3e}, against the float64 restatement "
              f"{close:.3e} x its allowance; {int(res.accepted.sum())} accepted, {int(res.rejected.sum())} rejected "
              f"({int(res.newton_rejected.sum())} by Newton), {int(res.newton_iterations.sum())} Newton iterations")
        assert close <= 1.0
        if (restart, rtol) not in ADAPTIVE_DROPPED:
            assert ratio <= 1.0
        _counts_match(res, R, seg, f"stiff relaxation {restart} rtol {rtol:g}")


@pytest.mark.parametrize("restart", ("nodes", "sections"))
def test_adaptive_mode_completes_the_headline_phase(case, restart):
    cs = case("hypersensitive_K5_n4_T10000")
    d, seg = cs.data[0], cs.segments(0, restart)
    rtol = HEADLINE_RTOL
    atol = rtol * cs.sol.state_scale(0)
    res = cs.run(0, restart, rtol=rtol)                                      # max_steps keeps its default
    assert np.all(res.ok) and np.all(res.status == -1) and np.all(np.isfinite(res.y))
    R = ps.propagate_f64(d, seg, rtol=rtol, atol=atol)
    close = float(np.max(np.abs(res.y - R.y) / (10.0 * (atol[:, None] + rtol * np.abs(R.y)))))
    explicit = cs.run(0, restart, rtol=rtol, method="dopri5")
    print(f"hypersensitive T = 10000 {restart}: against the float64 restatement {close:.3e} x its allowance; "
          f"{int(res.accepted.sum())} accepted, {int(res.rejected.sum())} rejected ({int(res.newton_rejected.sum())} by Newton), "
          f"{int(res.newton_iterations.sum())} Newton iterations; the explicit pair completes {int(explicit.ok.sum())} of "
          f"{len(explicit.ok)} segments in {int(explicit.accepted.sum() + explicit.rejected.sum())} steps")
    assert close <= 1.0
    truth = headline_truth(restart)[0]                                      # 60 digits, from the oracle's node values
    np.testing.assert_allclose(truth[:, 0], d.node_y[:, 0], rtol=1e-14, atol=0.0)
    ratio = float(np.max(np.abs(res.y - truth)[:, 1:] / pr.adaptive_bound(d, seg, truth, res.accepted, atol, rtol, 0.0)[:, 1:]))
    print(f"  error / bound against the 60-digit truth = {ratio:.3e}")
    if restart not in HEADLINE_DROPPED:
        assert ratio <= 1.0
    _counts_match(res, R, seg, f"hypersensitive T = 10000 {restart}")
    assert not explicit.ok.all()


# ---- 9. the stiff contrast -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("restart", ("phase", "sections"))
def test_implicit_completes_where_the_explicit_pair_hits_the_cap(case, restart):
    cs = case(ps.STIFF_CASE)
    implicit = cs.run(0, restart, rtol=1e-6, max_steps=256)
    explicit = cs.run(0, restart, rtol=1e-6, max_steps=256, method="dopri5")
    print(f"stiff relaxation {restart}, max_steps = 256: sdirk4 {int(implicit.accepted.sum() + implicit.rejected.sum())} steps, "
          f"dopri5 {int(explicit.accepted.sum() + explicit.rejected.sum())} steps before the cap")
    assert np.all(implicit.ok)
    assert np.all(explicit.status >= 0) and not explicit.ok.any()
    assert np.all(np.isnan(explicit.y[:, -1]))
    assert explicit.newton_rejected is None and explicit.newton_iterations is None


# ---- 10. the failure convention ---------------------------------------------------------------------------------------
def test_a_newton_failure_in_fixed_mode_ends_its_segment_only(case):
    cs = case(FAILURE_CASE)
    d, seg = cs.data[0], cs.segments(0, "nodes")
    atol = FIXED_RTOL * cs.sol.state_scale(0)
    short = cs.run(0, "nodes", substeps=1, rtol=FIXED_RTOL, newton_max=8)
    full = cs.run(0, "nodes", substeps=1, rtol=FIXED_RTOL, newton_max=FIXED_NEWTON_MAX)
    R = ps.propagate_f64(d, seg, substeps=1, rtol=FIXED_RTOL, atol=atol, newton_max=8)
    failed = R.status >= 0
    assert failed.any() and not failed.all() and np.all(R.near[1:] >= NEAR)
    np.testing.assert_array_equal(short.status, R.status)
    np.testing.assert_array_equal(short.ok, ~failed)
    assert np.all(full.ok)
    assert np.all(np.isnan(short.y[:, 1:][:, failed]))
    np.testing.assert_array_equal(short.y[:, 1:][:, ~failed], full.y[:, 1:][:, ~failed])
    for got, ref in ((short.accepted, R.accepted), (short.rejected, R.rejected), (short.newton_rejected, R.newton_rejected),
                     (short.newton_iterations, R.newton_iterations)):
        np.testing.assert_array_equal(got, ref)
    # ... and behind the failing interval of a longer segment: NaN and zero counts to the segment's end
    whole = cs.segments(0, "phase")
    Rp = ps.propagate_f64(d, whole, substeps=1, rtol=FIXED_RTOL, atol=atol, newton_max=8)
    one = cs.run(0, "phase", substeps=1, rtol=FIXED_RTOL, newton_max=8)
    np.testing.assert_array_equal(one.status, Rp.status)
    np.testing.assert_array_equal(np.isnan(one.y), np.isnan(Rp.y))
    for got, ref in ((one.accepted, Rp.accepted), (one.rejected, Rp.rejected), (one.newton_rejected, Rp.newton_rejected),
                     (one.newton_iterations, Rp.newton_iterations)):
        np.testing.assert_array_equal(got, ref)
    print(f"newton_max = 8: segments {np.nonzero(failed)[0].tolist()} of {len(seg) - 1} fail when restarted at every node; "
          f"the single pass has status {one.status.tolist()}")


# ---- 11. the same arithmetic, the same bits -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hypersensitive_K5_n4", "cart_pole_ragged_K23", ps.STIFF_CASE])
def test_modes_agree_bit_for_bit(case, name):
    cs = case(name)
    for ip in cs.phases:
        d = cs.data[ip]
        for kw in (dict(substeps=1, rtol=FIXED_RTOL, newton_max=FIXED_NEWTON_MAX), dict(substeps=3, rtol=FIXED_RTOL, newton_max=FIXED_NEWTON_MAX),
                   dict(rtol=1e-6)):
            nodes, secs, phase = (cs.run(ip, r, **kw).y for r in ("nodes", "sections", "phase"))
            np.testing.assert_array_equal(phase[:, 1], nodes[:, 1])
            np.testing.assert_array_equal(secs[:, 1], nodes[:, 1])
            first = d.s[:-1] + 1
            np.testing.assert_array_equal(secs[:, first], nodes[:, first])
            listed = cs.sol.propagate(ip, restart=np.asarray(d.s, dtype=np.int64), method="sdirk4", **kw)
            np.testing.assert_array_equal(listed.y, secs)


# ---- 12. the conventions of pc_solution -----------------------------------------------------------------------------
def test_repeatable_and_host_and_device_variants_agree(case):
    import torch
    cs = case("cart_pole_ragged_K23")
    for kw in (dict(substeps=2, rtol=FIXED_RTOL), dict(rtol=1e-8)):
        a = cs.run(0, "sections", **kw)
        b = cs.run(0, "sections", **kw)
        seg_t = torch.tensor(cs.segments(0, "sections"), dtype=torch.int64, device="cuda:0")
        dev = cs.sol.propagate(0, restart=seg_t, method="sdirk4", **kw)
        for name in ("y", "defect", "relative_defect", "accepted", "rejected", "status", "ok", "terminal_defect",
                     "newton_rejected", "newton_iterations"):
            p, q, t = getattr(a, name), getattr(b, name), getattr(dev, name)
            np.testing.assert_array_equal(p, q, err_msg=name)
            assert isinstance(t, torch.Tensor) and t.is_cuda, name
            np.testing.assert_array_equal(p, t.cpu().numpy(), err_msg=name)


def test_handle_is_left_as_found_and_dopri5_is_the_default(case):
    cs = case("two_phase_transfer_K6")
    eng = cs.eng
    cs.run(0, "nodes", rtol=1e-8)
    cs.run(1, "phase", substeps=2, rtol=FIXED_RTOL)
    np.testing.assert_array_equal(eng.evaluate_c(cs.x), cs.c_before)
    np.testing.assert_array_equal(eng.evaluate_G_nonzeros(cs.x), cs.G_before)
    for kw in (dict(substeps=2), dict(rtol=1e-8)):
        plain = cs.sol.propagate(0, restart="sections", **kw)
        named = cs.sol.propagate(0, restart="sections", method="dopri5", newton_max=3, **kw)
        for name in ("y", "accepted", "rejected", "status"):
            np.testing.assert_array_equal(getattr(plain, name), getattr(named, name), err_msg=name)
        assert named.newton_rejected is None and named.newton_iterations is None


def test_bad_arguments_raise_before_any_launch(case):
    cs = case("hypersensitive_K5_n4")
    N = cs.data[0].N
    for kw in (dict(method="radau"), dict(method=None), dict(newton_max=0), dict(newton_max=33), dict(newton_max=2.5),
               dict(substeps=2, rtol=0.0), dict(rtol=0.0), dict(substeps=2, rtol=float("nan")), dict(substeps=-1),
               dict(atol=0.0), dict(max_steps=0), dict(restart="mesh"), dict(restart=np.array([0, 4, 4, N - 1]))):
        kw.setdefault("method", "sdirk4")
        with pytest.raises(ValueError):
            cs.sol.propagate(0, **kw)
    # the C calls make the same refusals themselves
    import ctypes as C
    lib, h = cs.sol._lib, cs.sol._h
    y = np.empty((1, N))
    acc, rej, st, nr, ni = (np.empty(N, np.int32) for _ in range(5))
    good_seg, atol = np.array([0, N - 1], dtype=np.int32), np.array([1e-6])

    def call(seg=good_seg, n_seg=1, substeps=0, rtol=1e-6, at=atol, max_steps=4096, newton_max=8):
        return lib.pc_solution_propagate_stiff(h, 0, n_seg, seg.ctypes.data, substeps, C.c_double(rtol), at.ctypes.data, max_steps,
                                               newton_max, y.ctypes.data, acc.ctypes.data, rej.ctypes.data, st.ctypes.data,
                                               nr.ctypes.data, ni.ctypes.data)
    assert call() and call(substeps=2)
    assert not call(newton_max=0) and not call(newton_max=33)
    assert b"newton_max" in lib.pc_last_error()
    assert not call(substeps=2, rtol=0.0) and not call(rtol=0.0) and not call(substeps=2, rtol=float("inf"))
    assert not call(seg=np.array([1, N - 1], dtype=np.int32)) and not call(n_seg=0) and not call(substeps=-1)
    assert not call(at=np.array([0.0])) and not call(max_steps=0) and not call(max_steps=(1 << 20) + 1)
    assert b"propagate" in lib.pc_last_error()
