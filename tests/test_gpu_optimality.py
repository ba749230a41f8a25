"""Path and bound multipliers, the gradients of the augmented Hamiltonian and the two Pontryagin residuals of a Solution
(pycollo_amd/solution.py, csrc/pc_solution.hpp: pc_sol_multipliers_p<i>, pc_sol_sample_optimality_p<i>) on the GPU.

Parity at arbitrary points (no solve): the cases, x, lam~, W and w of tests/test_gpu_costate.py, and z~ = 0.1 normal.
The reference is tests/optimality_ref.py (``np.longdouble`` node quantities, the oracle's partials, 60-digit mpmath
interpolants).

Bounds.  mu, zeta and the endpoint multipliers are one product and two or three divisions of the inputs:
``entry_err(rtol=1e-10, ulps=64)`` with the value's own magnitude.  H_y / H_u at the nodes and between them: 1e-8 of the
sum of the magnitudes of the terms, the bound the node-Hamiltonian test holds values to that pass through the generated
tape.  Sampled mu, zeta: against the 60-digit interpolant of the kernel's own node values, mag = sum_k sum_i |C_ki||v_i|
(a contraction and Clenshaw with |P_k| <= 1: at most 2n + 2 <= 42 roundings of mag, ulps = 64).  Sampled dp/dt: the same
``entry_err(rtol=1e-10, ulps=64)``; the differentiated recurrence carries |P_k'| <= n (n - 1) / 2, so its magnitude is
mag n (n - 1) / 2 times 2 / (h_k stretch).

The identity on the device path: r~ = grad J~ + G~^T lam~ + z~ from the engine's own ``evaluate_g``,
``evaluate_G_nonzeros`` and structure against the kernel's node outputs, |lhs - rhs| <= 1e-10 |rhs| + 64 eps (|G~|^T|lam~| +
|z~|) with ``G_mag``.

End to end: hypersensitive, final time 10, order 8, K = 8, u in [-0.2, 50] (tests/test_optimality_ref_cpu.py solves it
on the host): ``MeshIteration(prob).solve_with_ipm(tol=1e-10)`` then ``dense_solution()``.  The mid-mesh section's
max |costate_residual| of ``optimality_report`` is held within a factor 2 of the host figure 5.899e-7: both
solves stop at a tolerance, not at the same bits.  The figures are printed and appended to the file named by
PYCOLLO_AMD_OPTIMALITY_REPORT, if set."""
import os

import numpy as np
import pytest

import optimality_ref as oref
import test_gpu_costate as tc
from conftest import entry_err
from pycollo_amd import problems
from pycollo_amd.solution import exact_tables
from test_optimality_ref_cpu import bounded_hypersensitive

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
W_J = tc.W_J
HOST_MID_SECTION_RESIDUAL = 5.899e-7      # tests/test_optimality_ref_cpu.py::test_bounded_hypersensitive_on_the_host


def _report(line):
    print(line)
    path = os.environ.get("PYCOLLO_AMD_OPTIMALITY_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


class Case(tc.Case):
    """test_gpu_costate's case with bound multipliers: ``sol`` carries lam~ and z~"""

    def __init__(self, name):
        from pycollo_amd.solution import Solution
        super().__init__(name)
        self.sol.close()
        self.z = 0.1 * np.random.default_rng(43).normal(size=self.eng.num_x)
        self.sol = Solution(self.eng, self.x, multipliers=self.lam, bound_multipliers=self.z)
        self.launched_at_creation = self.sol._optimality is not None
        self._node = {}
        self._curve = {}

    def node_reference(self, ip):
        if ip not in self._node:
            self._node[ip] = oref.NodeReference(self.ora, self.tables, self.x, self.lam, self.z, ip, w_J=W_J)
        return self._node[ip]

    def curves(self, ip, k):
        """the exact interpolants of section k of the kernel's own node values: (p, mu, zeta) SectionInterpolants; the
        phase's last section forms mu and zeta with the ydot table, a node without weight staged as 0"""
        if (ip, k) not in self._curve:
            mesh = self.eng.meshes[ip]
            s, n = int(mesh.s[k]), int(mesh.n[k])
            Cd, Cu = exact_tables(self.method, n)
            T = Cd if k == mesh.K - 1 else Cu
            stage = lambda a: np.where(np.isnan(a[:, s:s + n]), 0.0, a[:, s:s + n])   # noqa: E731
            self._curve[(ip, k)] = (oref.SectionInterpolant(Cu, self.sol.costate[ip][:, s:s + n]),
                                    oref.SectionInterpolant(T, stage(self.sol.path_multiplier[ip])),
                                    oref.SectionInterpolant(T, stage(self.sol.bound_multiplier[ip])))
        return self._curve[(ip, k)]

    def sampled_reference(self, ip, tau):
        """(mu, mag_mu, zeta, mag_zeta, dp, mag_dp) at tau, from the exact interpolants"""
        mesh, pl = self.eng.meshes[ip], self.eng.layout.phases[ip]
        k, c = self.locate(ip, tau)
        stretch = 0.5 * (self.sol.final_time[ip] - self.sol.initial_time[ip])
        n_p = self.eng.model.phases[ip].n_p
        Q = len(tau)
        mu, mmu = np.zeros((n_p, Q)), np.zeros((n_p, Q))
        ze, mze = np.zeros((pl.n_y + pl.n_u, Q)), np.zeros((pl.n_y + pl.n_u, Q))
        dp, mdp = np.zeros((pl.n_y, Q)), np.zeros((pl.n_y, Q))
        for i in range(Q):
            kk = int(k[i])
            n, h = int(mesh.n[kk]), float(mesh.tau[mesh.s[kk + 1]] - mesh.tau[mesh.s[kk]])
            P, M, Z = self.curves(ip, kk)
            mu[:, i], mmu[:, i] = M.value(c[i]), M.mag
            ze[:, i], mze[:, i] = Z.value(c[i]), Z.mag
            f = 2.0 / (h * stretch)
            dp[:, i], mdp[:, i] = f * P.derivative(c[i]), abs(f) * P.mag * max(1.0, 0.5 * n * (n - 1))
        return mu, mmu, ze, mze, dp, mdp


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


def _assert_within(got, ref, mag, what, ulps=64):
    ratio = entry_err(got, ref, mag, rtol=1e-10, ulps=ulps)
    print(f"{what}: largest |got - ref| / bound = {ratio:.3e}")
    assert ratio <= 1.0, f"{what} differs from its reference by {ratio:.3e} x its bound"


def _assert_tape(got, ref, mag, what):
    """values that pass through the generated tape: 1e-8 of the sum of the term magnitudes; NaN where the reference is"""
    got, ref, mag = (np.asarray(a, float) for a in (got, ref, mag))
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN in other places than the reference"
    fin = ~np.isnan(ref)
    if not fin.any():
        return
    err = np.abs(got[fin] - ref[fin]) / (1e-8 * mag[fin] + 1e-290)
    print(f"{what}: largest |got - ref| / bound = {np.max(err):.3e}")
    assert np.all(err <= 1.0), f"{what} differs from its reference by {np.max(err):.3e} x its bound"


# ---- 5. node parity ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tc.CASES))
def test_node_multipliers_and_gradients(case, name):
    cs = case(name)
    sol, eng = cs.sol, cs.eng
    assert not cs.launched_at_creation                  # formed on first use, below
    mu_all, zeta_all, end_all = sol.path_multiplier, sol.bound_multiplier, sol.endpoint_bound_multiplier
    H_y_all, H_u_all = sol.hamiltonian_gradient
    assert len(mu_all) == len(zeta_all) == len(end_all) == len(H_y_all) == len(H_u_all) == len(eng.meshes)
    for ip, (pl, pm) in enumerate(zip(eng.layout.phases, eng.model.phases)):
        N, n_y, n_u = pl.N, pl.n_y, pl.n_u
        ref = cs.node_reference(ip)
        mu, zeta, end_z, H_y, H_u = mu_all[ip], zeta_all[ip], end_all[ip], H_y_all[ip], H_u_all[ip]
        assert mu.shape == (pm.n_p, N) and zeta.shape == (n_y + n_u, N) and end_z.shape == (n_y, 2)
        assert H_y.shape == (n_y, N) and H_u.shape == (n_u, N)
        _assert_within(mu, ref.mu.astype(float), ref.mag_mu.astype(float), f"{name} phase {ip} mu")
        _assert_within(zeta, ref.zeta.astype(float), ref.mag_zeta.astype(float), f"{name} phase {ip} zeta")
        _assert_within(end_z, ref.end_z.astype(float), np.abs(ref.end_z).astype(float), f"{name} phase {ip} endpoint multipliers")
        assert np.all(zeta[:n_y, 0] == 0.0) and np.all(zeta[:n_y, -1] == 0.0)       # exactly
        unweighted = np.zeros(N, dtype=bool)
        if cs.method == "radau":
            unweighted[-1] = True
        assert np.array_equal(np.isnan(mu), np.broadcast_to(unweighted, mu.shape))     # NaN exactly at the Radau final node
        assert np.array_equal(np.isnan(zeta[n_y:]), np.broadcast_to(unweighted, (n_u, N)))
        assert not np.any(np.isnan(zeta[:n_y]))
        _assert_tape(np.vstack([H_y, H_u]), ref.H_z.astype(float), ref.mag_H.astype(float), f"{name} phase {ip} H_y, H_u")
        # the two derived node arrays
        stat = sol.control_stationarity[ip]
        _assert_tape(stat, (ref.H_z[n_y:] + ref.zeta[n_y:]).astype(float), (ref.mag_H[n_y:] + ref.mag_zeta[n_y:]).astype(float),
                     f"{name} phase {ip} control_stationarity")
        cd_ref = ref.costate_defect()
        mag_cd = np.abs(ref.D) / np.where(ref.weighted, np.abs(ref.stretch * ref.omega), 1) + ref.mag_H[:n_y] + ref.mag_zeta[:n_y]
        _assert_tape(sol.costate_defect[ip], cd_ref.astype(float), mag_cd.astype(float), f"{name} phase {ip} costate_defect")
        assert np.all(np.isnan(sol.costate_defect[ip][:, [0, -1]]))


# ---- 6. the identity on the device path -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two_phase_transfer_K6", "time_coupled_transfer_K6", "cart_pole_ragged_K60",
                                  "order_extremes_2_and_20"])
def test_identity_on_the_device_path(case, name):
    import scipy.sparse as sp
    cs = case(name)
    eng, sol, ora = cs.eng, cs.sol, cs.ora
    rows, cols = eng.evaluate_G_structure()
    G = sp.coo_matrix((eng.evaluate_G_nonzeros(cs.x), (rows, cols)), shape=(eng.num_c, eng.num_x)).tocsr()
    r = np.asarray(eng.evaluate_g(cs.x), float) + G.T @ cs.lam + cs.z
    orow, ocol = ora.G_structure()
    scale = sp.coo_matrix((ora.G_mag(cs.x), (orow, ocol)), shape=(ora.num_c, ora.num_x)).tocsr().T @ np.abs(cs.lam) + np.abs(cs.z)
    V = eng.layout.expand_x(eng.V_ocp)
    worst, n_cols = 0.0, 0
    for ip, pl in enumerate(eng.layout.phases):
        N, n_y, n_u = pl.N, pl.n_y, pl.n_u
        omega = sol.quadrature_weights(ip)
        stretch = 0.5 * (sol.final_time[ip] - sol.initial_time[ip])
        node_res = np.vstack([sol.costate_defect[ip], sol.control_stationarity[ip]])      # [n_y + n_u][N]
        for b in range(n_y + n_u):
            js = np.arange(1, N - 1) if b < n_y else np.nonzero(omega != 0)[0]
            col = pl.x_off + b * N + js
            rhs = W_J * V[col] * stretch * omega[js] * node_res[b, js]
            assert np.all(np.isfinite(rhs))
            ratio = np.abs(r[col] - rhs) / (1e-10 * np.abs(rhs) + 64 * EPS * scale[col])
            worst, n_cols = max(worst, float(np.max(ratio))), n_cols + len(js)
    print(f"{name}: {n_cols} columns, largest |lhs - rhs| / bound = {worst:.3e}")
    assert n_cols > 0 and worst <= 1.0


# ---- 7. sampling ------------------------------------------------------------------------------------------------
def _oracle_gradients(cs, ip, y, u, p, mu):
    """(H_z, mag) [n_y + n_u][Q] from the oracle's partials at the given states, controls, costates and path multipliers"""
    P = cs.ora.P[ip]
    cs.ora._mag_fns()
    ref = cs.node_reference(ip)
    _, _, _, _, w = cs.ora._unpack(P, cs.x)
    Q = y.shape[1]
    rho = float(ref.rho[1])          # one number for the mesh (1 under Lobatto, 2 under Radau)
    a = [row for row in y] + [row for row in u] + [np.full(Q, w[i]) for i in range(P.n_w)]
    mult = [row for row in p] + [row for row in mu] + [np.full(Q, rho * float(v)) for v in ref.nu]
    H, mag = np.zeros((P.n_z, Q)), np.zeros((P.n_z, Q))
    for (r, cvar), (_, dfn) in P.dF.items():
        if cvar < P.n_z:
            H[cvar] += mult[r] * np.broadcast_to(np.asarray(dfn(*a), float), (Q,))
            mag[cvar] += np.abs(mult[r]) * np.abs(np.broadcast_to(np.asarray(P.dF_mag[(r, cvar)](*a), float), (Q,)))
    return H, mag


@pytest.mark.parametrize("name", list(tc.CASES))
def test_sampled_quantities(case, name):
    cs = case(name)
    sol = cs.sol
    for ip, pl in enumerate(cs.eng.layout.phases):
        n_y = pl.n_y
        tau = cs.base_queries(ip)
        got = sol.sample_optimality(ip, tau=tau)
        mu, mmu, ze, mze, dp, mdp = cs.sampled_reference(ip, tau)
        _assert_within(got.mu, mu, mmu, f"{name} phase {ip} mu(tau)")
        _assert_within(got.zeta, ze, mze, f"{name} phase {ip} zeta(tau)")
        _assert_within(got.dp, dp, mdp, f"{name} phase {ip} dp/dt(tau)")
        # H_y, H_u against the oracle's partials at the kernel's own sampled point
        y, _, u, _ = sol.sample_f(ip, tau=tau)
        p, _ = sol.sample_costate(ip, tau=tau)
        H, mag = _oracle_gradients(cs, ip, y, u, p, got.mu)
        _assert_tape(np.vstack([got.H_y, got.H_u]), H, mag, f"{name} phase {ip} H_y(tau), H_u(tau)")
        np.testing.assert_array_equal(got.costate_residual, got.dp + got.H_y + got.zeta[:n_y])
        np.testing.assert_array_equal(got.control_stationarity, got.H_u + got.zeta[n_y:])
        # at node queries (the first N of the base queries) the interpolants return the node values ...
        N = pl.N
        node_mu, node_zeta = sol.path_multiplier[ip], sol.bound_multiplier[ip]
        keep = ~np.isnan(node_zeta[-1]) if pl.n_u else np.ones(N, dtype=bool)      # (the Radau final node is not interpolated)
        _assert_within(got.mu[:, :N][:, keep], node_mu[:, keep], mmu[:, :N][:, keep], f"{name} phase {ip} mu at the nodes")
        _assert_within(got.zeta[:, :N][:, keep], node_zeta[:, keep], mze[:, :N][:, keep], f"{name} phase {ip} zeta at the nodes")
        # ... and where a section starts the sampled state is the node's own, so the sampled gradients are the node's
        starts = np.asarray(cs.eng.meshes[ip].s[:-1])
        H_y_n, H_u_n = sol.hamiltonian_gradient
        _assert_tape(np.vstack([got.H_y, got.H_u])[:, starts], np.vstack([H_y_n[ip], H_u_n[ip]])[:, starts], mag[:, starts],
                     f"{name} phase {ip} H_y, H_u at the section starts")


@pytest.mark.parametrize("Q", [1, 63, 64, 65, 1000])
def test_query_counts_shuffled_with_duplicates(case, Q):
    cs = case("cart_pole_ragged_K23")
    tau = cs.base_queries(0)
    idx = np.random.default_rng(Q).integers(0, len(tau), Q)
    full = cs.sol.sample_optimality(0, tau=tau)
    got = cs.sol.sample_optimality(0, tau=tau[idx])
    assert got.H_y.shape == (4, Q) and got.H_u.shape == (1, Q) and got.dp.shape == (4, Q)
    assert got.mu.shape == (0, Q) and got.zeta.shape == (5, Q)
    for a, b in ((got.H_y, full.H_y), (got.H_u, full.H_u), (got.dp, full.dp), (got.zeta, full.zeta)):
        np.testing.assert_array_equal(a, b[:, idx])       # a query gets the same bits wherever it stands


def test_repeatable_and_device_tensor_variants(case):
    import torch
    from pycollo_amd.solution import Solution
    cs = case("two_phase_transfer_K6")
    for ip in range(len(cs.eng.meshes)):
        tau = cs.base_queries(ip)
        tau = tau[np.random.default_rng(2).permutation(len(tau))]
        a = cs.sol.sample_optimality(ip, tau=tau)
        b = cs.sol.sample_optimality(ip, tau=tau)
        d = cs.sol.sample_optimality(ip, tau=torch.tensor(tau, dtype=torch.float64, device="cuda:0"))
        for f in ("H_y", "H_u", "dp", "mu", "zeta", "costate_residual", "control_stationarity"):
            np.testing.assert_array_equal(getattr(a, f), getattr(b, f))
            t = getattr(d, f)
            assert isinstance(t, torch.Tensor) and t.is_cuda
            np.testing.assert_array_equal(getattr(a, f), t.cpu().numpy())
    # the multipliers from device tensors, a (zl, zu) pair: the same bits
    dev = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda:0")   # noqa: E731
    zl, zu = np.maximum(-cs.z, 0.0), np.maximum(cs.z, 0.0)
    for lam, zb in ((dev(cs.lam), dev(cs.z)), (cs.lam.copy(), (zl, zu)), (dev(cs.lam), (dev(zl), dev(zu)))):
        other = Solution(cs.eng, cs.x, multipliers=lam, bound_multipliers=zb)
        try:
            for ip in range(len(cs.eng.meshes)):
                np.testing.assert_array_equal(other.path_multiplier[ip], cs.sol.path_multiplier[ip])
                np.testing.assert_array_equal(other.bound_multiplier[ip], cs.sol.bound_multiplier[ip])
                np.testing.assert_array_equal(other.hamiltonian_gradient[1][ip], cs.sol.hamiltonian_gradient[1][ip])
                for x, y in zip(other.multiplier_coefficients(ip), cs.sol.multiplier_coefficients(ip)):
                    np.testing.assert_array_equal(x, y)
        finally:
            other.close()


@pytest.mark.parametrize("name", ["cart_pole_ragged_K23", "hypersensitive_radau_K7_n5"])
def test_out_of_range_nan_error_and_extrapolation(case, name):
    cs = case(name)
    mesh = cs.eng.meshes[0]
    tau = np.array([-1.0 - 0.04 * mesh.h[0], 0.1, 1.0 + 0.03 * mesh.h[-1], -1.0, 1.0, np.nan])
    inside = np.array([False, True, False, True, True, False])
    got = cs.sol.sample_optimality_unchecked(0, tau, 1)            # (PC_SOLUTION_TAU): the C call as it is
    for a in (got.H_y, got.H_u, got.dp, got.mu, got.zeta):
        assert np.all(np.isnan(a[:, ~inside])) and np.all(np.isfinite(a[:, inside]))
    with pytest.raises(ValueError, match="outside the phase"):
        cs.sol.sample_optimality(0, tau=tau[:5])
    with pytest.raises(ValueError, match="NaN"):
        cs.sol.sample_optimality(0, tau=tau)
    te = tau[:5]
    ext = cs.sol.sample_optimality(0, tau=te, extrapolate=True)
    k = np.array([0, cs.locate(0, te[1:2])[0][0], mesh.K - 1, 0, mesh.K - 1])
    c = cs.c_of(0, k, te)
    stretch = 0.5 * (cs.sol.final_time[0] - cs.sol.initial_time[0])
    for i in range(5):
        P, M, Z = cs.curves(0, int(k[i]))
        n, h = int(mesh.n[k[i]]), float(mesh.tau[mesh.s[k[i] + 1]] - mesh.tau[mesh.s[k[i]]])
        grow = max(1.0, abs(c[i])) ** (n - 1)                       # |P_m(c)| outside [-1, 1]
        _assert_within(ext.zeta[:, i], Z.value(c[i]), grow * Z.mag, f"{name} extrapolated zeta {i}")
        _assert_within(ext.dp[:, i], 2.0 / (h * stretch) * P.derivative(c[i]), grow * abs(2.0 / (h * stretch)) * P.mag * 0.5 * n * (n - 1),
                       f"{name} extrapolated dp {i}")
    assert np.all(np.isfinite(ext.H_y)) and np.all(np.isfinite(ext.H_u))


# ---- 8. the handle is left as found; nothing is launched unasked -----------------------------------------------------
@pytest.mark.parametrize("name", ["cart_pole_ragged_K23", "two_phase_transfer_K6"])
def test_handle_is_left_as_found(case, name):
    from pycollo_amd.solution import Solution
    cs = case(name)
    eng = cs.eng
    _ = cs.sol.path_multiplier
    cs.sol.sample_optimality(0, tau=np.array([0.0, 0.5]))
    cs.sol.optimality_report(0, samples_per_section=5)
    np.testing.assert_array_equal(eng.evaluate_c(cs.x), cs.c_before)
    np.testing.assert_array_equal(eng.evaluate_G_nonzeros(cs.x), cs.G_before)
    # ... and in the middle of the callback protocol: the point cached by a new_x = True call survives
    c1 = eng.evaluate_c(cs.x, new_x=True).copy()
    other = Solution(eng, 0.5 * cs.x, multipliers=2.0 * cs.lam, bound_multipliers=-cs.z)
    other.sample_optimality(0, tau=np.array([-1.0, 0.3, 1.0]))
    other.close()
    assert eng.cache_holds(cs.x)
    np.testing.assert_array_equal(eng.evaluate_c(cs.x, new_x=False), c1)
    np.testing.assert_array_equal(eng.evaluate_G_nonzeros(cs.x), cs.G_before)
    np.testing.assert_array_equal(c1, cs.c_before)


def test_nothing_is_formed_until_asked_and_none_without_multipliers(case):
    from pycollo_amd.solution import Solution
    cs = case("hypersensitive_K5_n4")
    lazy = Solution(cs.eng, cs.x, multipliers=cs.lam, bound_multipliers=cs.z)
    plain = Solution(cs.eng, cs.x)
    no_z = Solution(cs.eng, cs.x, multipliers=cs.lam)
    try:
        lazy.sample(0, tau=np.array([0.0]))
        lazy.sample_costate(0, tau=np.array([0.0]))
        assert lazy._optimality is None                       # nothing of this file's has been launched for it
        np.testing.assert_array_equal(lazy.costate[0], cs.sol.costate[0])
        assert plain.path_multiplier is None and plain.bound_multiplier is None and plain.hamiltonian_gradient is None
        assert plain.control_stationarity is None and plain.costate_defect is None and plain.endpoint_bound_multiplier is None
        with pytest.raises(ValueError, match="without multipliers"):
            plain.sample_optimality(0, tau=np.array([0.0]))
        with pytest.raises(ValueError, match="out of range"):
            lazy.sample_optimality(1, tau=np.array([0.0]))
        # without bound multipliers zeta is left out and the report says so
        assert no_z.bound_multiplier is None and no_z.endpoint_bound_multiplier is None
        np.testing.assert_array_equal(no_z.path_multiplier[0], cs.sol.path_multiplier[0])
        np.testing.assert_array_equal(no_z.control_stationarity[0], cs.sol.hamiltonian_gradient[1][0])
        s = no_z.sample_optimality(0, tau=np.array([-1.0, 0.2]))
        assert s.zeta is None
        np.testing.assert_array_equal(s.control_stationarity, s.H_u)
        np.testing.assert_array_equal(s.costate_residual, s.dp + s.H_y)
        assert no_z.optimality_report(0).has_bound_multipliers is False and cs.sol.optimality_report(0).has_bound_multipliers
        lazy.close()
        with pytest.raises(ValueError, match="closed"):
            lazy.sample_optimality(0, tau=np.array([0.0]))
    finally:
        for s in (lazy, plain, no_z):
            s.close()


def test_optimality_report_reduces_the_samples(case):
    cs = case("cart_pole_ragged_K23")
    mesh = cs.eng.meshes[0]
    m = 9
    rep = cs.sol.optimality_report(0, samples_per_section=m)
    edges = mesh.tau[mesh.s]
    c = np.linspace(-1.0, 1.0, m)
    tau = edges[:-1, None] + 0.5 * (c[None, :] + 1.0) * (edges[1:, None] - edges[:-1, None])
    tau[:, 0] = edges[:-1]
    tau[:, -1] = np.nextafter(edges[1:], -2.0)
    tau[-1, -1] = edges[-1]
    smp = cs.sol.sample_optimality(0, tau=tau.reshape(-1))
    cs_ref = np.max(np.abs(smp.control_stationarity), axis=0).reshape(mesh.K, m)
    cr_ref = np.max(np.abs(smp.costate_residual), axis=0).reshape(mesh.K, m)
    np.testing.assert_array_equal(rep.control_stationarity, cs_ref.max(axis=1))
    np.testing.assert_array_equal(rep.costate_residual, cr_ref.max(axis=1))
    t0, tF = cs.sol.initial_time[0], cs.sol.final_time[0]
    time = tau * (0.5 * (tF - t0)) + 0.5 * (t0 + tF)
    np.testing.assert_allclose(rep.costate_residual_time, time[np.arange(mesh.K), cr_ref.argmax(axis=1)], rtol=0, atol=1e-12)
    assert rep.max_costate_residual == cr_ref.max() and rep.interior_max_costate_residual == cr_ref[1:-1].max()
    assert rep.max_control_stationarity == cs_ref.max() and rep.interior_max_control_stationarity == cs_ref[1:-1].max()
    with pytest.raises(ValueError, match="samples_per_section"):
        cs.sol.optimality_report(0, samples_per_section=1)


def test_backend_solution_takes_lam_x(case):
    from pycollo_amd.pycollo_backend import Mi355x
    cs = case("hypersensitive_K5_n4")
    b = Mi355x(device=0)
    b.engine = cs.eng
    s = b.solution(cs.x, lam_g=list(cs.lam), lam_x=list(cs.z))
    try:
        np.testing.assert_array_equal(s.bound_multiplier[0], cs.sol.bound_multiplier[0])
        np.testing.assert_array_equal(s.control_stationarity[0], cs.sol.control_stationarity[0])
    finally:
        s.close()
        b.engine = None


# ---- 9. end to end ----------------------------------------------------------------------------------------------
def test_bounded_hypersensitive_end_to_end(built):
    """the lower control bound is active over part of the mesh: H_u is large there, H_u + zeta_u is zero to the
    solver's tolerance, zeta_u <= 0 and complementary to u + 0.2; the mid-mesh section's costate residual is the host's"""
    from pycollo_amd.iteration import MeshIteration
    it = MeshIteration(bounded_hypersensitive())
    res = it.solve_with_ipm(tol=1e-10)
    sol = it.dense_solution()
    try:
        assert res.success, res.status
        assert sol.bound_multiplier is not None
        n_y = 1
        u = sol.control[0][0]
        H_u, zeta_u = sol.hamiltonian_gradient[1][0][0], sol.bound_multiplier[0][n_y]
        stat = sol.control_stationarity[0][0]
        rep = sol.optimality_report(0)
        K = it.meshes[0].K
        mid = float(rep.costate_residual[K // 2])
        _report(f"bounded hypersensitive tF=10 K=8 n=8, u in [-0.2, 50]: status {res.status}, iterations {res.iterations}; "
                f"max |H_u| = {np.max(np.abs(H_u)):.4e} ({int(np.sum(np.abs(H_u) >= 0.1))} nodes >= 0.1); "
                f"max |H_u + zeta_u| = {np.max(np.abs(stat)):.3e}; max zeta_u = {np.max(zeta_u):.3e}; "
                f"max |zeta_u| (u + 0.2) = {np.max(np.abs(zeta_u) * (u + 0.2)):.3e}; "
                f"max |costate_defect| = {np.nanmax(np.abs(sol.costate_defect[0])):.3e}; "
                f"mid-section max |costate_residual| = {mid:.4e} (host {HOST_MID_SECTION_RESIDUAL:.4e}); "
                f"per section {np.array2string(rep.costate_residual, precision=3, max_line_width=1000)}; "
                f"interior max {rep.interior_max_costate_residual:.3e}, stationarity {rep.max_control_stationarity:.3e}")
        assert int(np.sum(np.abs(H_u) >= 0.1)) >= 1
        assert np.max(np.abs(stat)) <= 1e-6
        assert np.all(zeta_u <= 0.0)
        assert np.all(np.abs(zeta_u) * (u + 0.2) <= 1e-6)
        assert 0.5 * HOST_MID_SECTION_RESIDUAL <= mid <= 2.0 * HOST_MID_SECTION_RESIDUAL
    finally:
        sol.close()
        it.engine.close()


def test_solve_ocp_solution_samples_optimality(built):
    from pycollo_amd.solve import solve_ocp
    result = solve_ocp(problems.brachistochrone())
    sol = result.solution
    try:
        t0, tF = sol.initial_time[0], sol.final_time[0]
        t = np.linspace(t0, tF, 17)
        s = sol.sample_optimality(0, t)
        assert s.mu.shape == (0, 17)
        for a in (s.H_y, s.H_u, s.dp, s.costate_residual, s.control_stationarity):
            assert np.all(np.isfinite(a))
        _report(f"brachistochrone through solve_ocp: max |control_stationarity| = {np.max(np.abs(s.control_stationarity)):.3e}, "
                f"max |costate_residual| = {np.max(np.abs(s.costate_residual)):.3e} at 17 equispaced times; "
                f"bound multipliers {'passed on' if s.zeta is not None else 'not reported by the solver'}")
    finally:
        sol.close()
        result.final.engine.close()
