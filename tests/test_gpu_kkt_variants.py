"""The builds of the KKT solve that a block count or an environment knob selects (run with -m gpu on an MI355X): the
border sums by a grid (kkt_border_terms + kkt_border_terms_sum), kkt_leaf_forward from device memory, kkt_cr_top off or
with fewer waves, leaf factorisations with other than four waves.  Each is held to SuperLU by the method of
test_gpu_kkt.test_factor_and_solve_match_superlu, and ``GpuKkt.info`` must say that the build ran.

Inertia: the pivot signs of the same elimination order in NumPy (oracle/ref_kkt.py) -- it finishes in about two seconds
at the largest case here (25 204 unknowns); kkt_case's W + D block is not positive definite at the hypersensitive
cases, so (n_primal, n_dual) is not what to expect.
The 1e-9 bound on the solution: two SuperLU solves of these systems (COLAMD against NATURAL column order, one
refinement step each) differ by at most 7.4e-15 max|x| (profiles/kkt_variants.txt), so 1e-9 stands as it is.
"""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

from oracle.ref_kkt import RefKkt
from test_kkt_cpu import kkt_case, reference_matrix

pytestmark = pytest.mark.gpu

KNOBS = ("PYCOLLO_AMD_KKT_LEAF_FWD_LDS", "PYCOLLO_AMD_KKT_LEAF_WAVES", "PYCOLLO_AMD_KKT_CR_TOP", "PYCOLLO_AMD_KKT_CR")


class _Case:
    """One KKT system with its SuperLU solution and the reference's inertia per grouping, computed once."""

    def __init__(self, name, kw):
        self.eng, _, self.x, self.lam, self.ineq, self.fixed, self.sc, self.dvec = kkt_case(name, kw, device=0)
        eng = self.eng
        _, self.G, self.H = (a.copy() for a in eng.evaluate_all(self.x, 1.0, self.lam))   # host copies, for the reference matrix
        eng.evaluate_resident(self.x, 1.0, self.lam)                                       # the same bits stay on the device
        self.K = reference_matrix(eng, self.G, self.H, self.ineq, self.fixed, self.sc, self.dvec)
        nu = self.K.shape[0]
        self.rhs = np.random.default_rng(1).normal(size=nu)
        self.rhs[np.nonzero(self.fixed)[0]] = 0.0
        lu = spla.splu(self.K)
        xr = lu.solve(self.rhs)
        self.xr = xr + lu.solve(self.rhs - self.K @ xr)
        self.probe = np.random.default_rng(2).normal(size=nu)
        self.Kprobe = self.K @ self.probe

    def run(self, monkeypatch, env=None, group=None, ref_inertia=None):
        """Factor and solve with one build; held to the reference.  Returns (GpuKkt.info, inertia, solution)."""
        from pycollo_amd.kkt import GpuKkt
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        k = GpuKkt(self.eng, self.ineq, self.fixed, self.sc, group)
        assert k.nu == self.K.shape[0]
        assert k.info["leaf_forward_stage"] == -1          # no solve yet
        inertia = k.factor(self.dvec)
        y = k.matvec(self.dvec, self.probe)
        e_mv = np.max(np.abs(y - self.Kprobe)) / np.max(np.abs(self.Kprobe))
        xs = k.solve(self.rhs)
        xs = xs + k.solve(self.rhs - k.matvec(self.dvec, xs))
        e_x = np.max(np.abs(xs - self.xr)) / np.max(np.abs(self.xr))
        info = k.info
        print(f"\n   {env or {}} group {group}: matvec {e_mv:.2e}, solution {e_x:.2e} of max|x|, inertia {inertia}, {info}")
        assert e_mv <= 1e-12
        assert e_x <= 1e-9
        if ref_inertia is None:
            ref_inertia = RefKkt(k.tables).factor(self.G, self.H, self.dvec)
        assert inertia == ref_inertia
        k.factor(self.dvec)                                 # bit-reproducible: no atomics, fixed order
        a, b = k.solve(self.rhs), k.solve(self.rhs)
        np.testing.assert_array_equal(a, b)
        k.close()
        return info, inertia, xs

    def close(self):
        self.eng.close()


def _agree(xa, xb):
    assert np.max(np.abs(xa - xb)) <= 1e-9 * np.max(np.abs(xb))


def test_border_sums_by_a_grid_from_2048_terms(built, monkeypatch):
    """One section per leaf: 1 100 leaves + 1 101 chain nodes >= 2048 terms on a 2-wide border -- the grid; the default
    grouping of the same system keeps the border kernel's own walk."""
    case = _Case("hypersensitive", dict(K=1100, order=3))
    info1, in1, x1 = case.run(monkeypatch, group=1)
    assert info1["n_leaf"] + info1["n_chain"] >= 2048 and info1["border_blocks"] > 0
    assert info1["nb"] ** 2 * (info1["n_leaf"] + info1["n_chain"]) <= 2 ** 18     # (the count alone triggers)
    info0, in0, x0 = case.run(monkeypatch, group=None)
    assert info0["n_leaf"] + info0["n_chain"] < 2048 and info0["border_blocks"] == 0
    assert in0 == in1                                       # one matrix, two elimination orders: Sylvester
    _agree(x1, x0)
    case.close()


def test_border_sums_by_a_grid_on_a_wide_border(built, monkeypatch):
    """time_coupled_transfer, one section per leaf: a border of 20 unknowns; 4 K + 4 terms, so K = 163 is the smallest
    mesh with nb^2 (n_leaf + n_chain) > 2^18 -- far below 2048 terms -- and K = 162 stays on one workgroup."""
    for K, grid in ((163, True), (162, False)):
        case = _Case("time_coupled_transfer", dict(K=K, order=3))
        info, _, _ = case.run(monkeypatch, group=1)
        terms = info["n_leaf"] + info["n_chain"]
        print(f"   K {K}: nb {info['nb']}, terms {terms}")
        assert terms < 2048
        assert (info["nb"] ** 2 * terms > 2 ** 18) == grid
        assert (info["border_blocks"] > 0) == grid
        case.close()


def test_leaf_forward_from_device_memory_above_4096_leaves(built, monkeypatch):
    case = _Case("hypersensitive", dict(K=4200, order=3))
    info, _, _ = case.run(monkeypatch, group=1)
    assert info["n_leaf"] > 4096 and info["leaf_forward_stage"] == 0
    assert info["border_blocks"] > 0
    case.close()


SWEEP_CASES = [("hypersensitive", dict(K=300, order=6)), ("two_phase_transfer", {}), ("shuttle", dict(K=60, order=4))]


@pytest.mark.parametrize("name,kw", SWEEP_CASES)
def test_knob_sweeps_meet_the_reference(built, monkeypatch, name, kw):
    case = _Case(name, kw)
    base_info, base_inertia, base_x = case.run(monkeypatch)
    assert base_info["leaf_forward_stage"] == 2 and base_info["leaf_waves"] == 4 and base_info["chain_cr"] == 1
    assert base_info["cr_levels"] >= 1
    if kw.get("K") == 300:
        assert base_info["cr_top_levels"] > 0
    for stage in (0, 1, 2):
        info, inertia, xs = case.run(monkeypatch, {"PYCOLLO_AMD_KKT_LEAF_FWD_LDS": str(stage)}, ref_inertia=base_inertia)
        assert info["leaf_forward_stage"] == stage
        _agree(xs, base_x)
    for waves in (1, 2, 4):
        info, inertia, xs = case.run(monkeypatch, {"PYCOLLO_AMD_KKT_LEAF_WAVES": str(waves)}, ref_inertia=base_inertia)
        assert info["leaf_waves"] == waves
        _agree(xs, base_x)
    for top in (0, 2):
        info, inertia, xs = case.run(monkeypatch, {"PYCOLLO_AMD_KKT_CR_TOP": str(top)}, ref_inertia=base_inertia)
        if top == 0:
            assert info["cr_top_levels"] == 0
        else:
            assert info["cr_top_waves"] == 2 and info["cr_top_levels"] <= base_info["cr_top_levels"]
        _agree(xs, base_x)
    case.close()


@pytest.mark.parametrize("name,kw", [("hypersensitive", dict(K=8, order=3)), ("two_phase_transfer", {})])
def test_info_after_a_solve_is_what_the_host_shape_says(built, monkeypatch, name, kw):
    """``pc_kkt_shape_info`` decides on the host, without a device, what the handle then runs: field for field."""
    from pycollo_amd.kkt import GpuKkt, shape_info
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    eng, _, x, lam, ineq, fixed, sc, dvec = kkt_case(name, kw, device=0)
    eng.evaluate_resident(x, 1.0, lam)
    k = GpuKkt(eng, ineq, fixed, sc)
    k.factor(dvec)
    k.solve(np.ones(k.nu))
    assert k.info == shape_info(k.tables)
    assert k.info["leaf_forward_stage"] >= 0
    k.close()
    eng.close()
