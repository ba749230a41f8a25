"""Costates and the Hamiltonian of a Solution (pycollo_amd/solution.py, csrc/pc_solution.hpp: pc_sol_costate_p<i>,
pc_sol_sample_costate_p<i>) on the GPU.

Parity at arbitrary points (no solve): the meshes of tests/test_gpu_solution.py::CASES, a one-section mesh, an
all-order-2 mesh and a problem without integrands; that file's smooth x, lam~ = 0.1 normal(seed), a random W in
[0.5, 2] and w = 0.7 set through ``set_scaling``.  The reference restates the definition in ``np.longdouble`` from ``OracleMesh.I_mat`` and the
golden A tables.  Node costates entry by entry: ``entry_err(got, ref, mag, rtol=1e-10, ulps=64) <= 1`` with
mag = sum |Lam||h A| / omega (at most 2 (n - 1) products and one division: <= 40 roundings at n <= 20).  H at the nodes and
between them: 1e-8 of the sum of the magnitudes of its terms, f and g from the oracle's expression trees (the tolerance
f itself is held to against them).  nu: 4 eps.

Sampling: against the 60-digit mpmath interpolant of the kernel's own node costates,
``entry_err(..., rtol=1e-10, ulps=64)`` with mag = sum_k sum_i |C_ki||p_i| (a coefficient contraction and Clenshaw with
|P_k| <= 1: at most 2n + 2 <= 42 roundings of mag).

End to end: ``MeshIteration(prob).solve_with_ipm(tol=1e-10)`` then ``dense_solution()``; the bounds are the values a
host-only run gave with the margins stated there.  The figures of the GPU run are printed and appended to
the file named by PYCOLLO_AMD_COSTATE_REPORT, if set (the way to write profiles/costate_checks.txt)."""
import os

import mpmath as mp
import numpy as np
import pytest

from conftest import entry_err, golden_tables
from oracle.ref_numpy import OracleNlp
from pycollo_amd import problems
from pycollo_amd.solution import exact_tables
from test_gpu_solution import CASES as SOLUTION_CASES
from test_gpu_solution import _smooth_x

pytestmark = pytest.mark.gpu

DPS = 60
EPS = np.finfo(float).eps
W_J = 0.7
LD = np.longdouble

CASES = dict(SOLUTION_CASES)
CASES["hypersensitive_K1_n4"] = lambda: problems.hypersensitive(K=1, order=4)      # no neighbour section
CASES["hypersensitive_K7_n2"] = lambda: problems.hypersensitive(K=7, order=2)      # every interior node is shared
CASES["brachistochrone_K10_n4"] = problems.brachistochrone                         # no integrand (the others all have one)


def _report(line):
    print(line)
    path = os.environ.get("PYCOLLO_AMD_COSTATE_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


class Case:
    def __init__(self, name):
        from pycollo_amd.engine import NlpEngine
        from pycollo_amd.solution import Solution
        self.name = name
        self.prob = CASES[name]()
        self.eng = eng = NlpEngine(self.prob, device=0)
        self.method = eng.quad.method
        rng = np.random.default_rng(41)
        eng.set_scaling(eng.V_ocp, eng.r_ocp, rng.uniform(0.5, 2.0, eng.layout.num_ocp_c), W_J)
        self.tables = golden_tables(self.method)
        self.ora = OracleNlp(self.prob, self.tables, V_ocp=eng.V_ocp, r_ocp=eng.r_ocp, W_ocp=eng.W_ocp, w_J=W_J)
        self.x = _smooth_x(eng)
        self.lam = 0.1 * rng.normal(size=eng.num_c)
        self.c_before = eng.evaluate_c(self.x).copy()
        self.G_before = eng.evaluate_G_nonzeros(self.x).copy()
        self.sol = Solution(eng, self.x, multipliers=self.lam)
        self._ref = {}
        self._interp = {}

    def close(self):
        self.sol.close()
        self.eng.close()

    # ---- the definition, restated in extended precision ----------------------------------------------------
    def reference(self, ip):
        """(omega, p, mag_p, nu, f, g) of phase ip: omega [N], p / mag_p [n_y][N] (longdouble), nu [n_q], and the
        oracle's f [n_y][N], g [n_q][N] at the nodes"""
        if ip not in self._ref:
            P, ora = self.ora.P[ip], self.ora
            mesh, N = P.mesh, P.N
            W = self.eng.W_ocp.astype(LD)
            lam = self.lam.astype(LD)
            Lam = np.array([W[P.oc + a] * lam[P.c_off + a * (N - 1):P.c_off + (a + 1) * (N - 1)] / LD(W_J)
                            for a in range(P.n_y)]).reshape(P.n_y, N - 1)
            Lam_q = np.array([W[P.oc + P.n_y + P.n_p + m] * lam[P.c_int + m] / LD(W_J) for m in range(P.n_q)], dtype=LD)
            omega = np.zeros(N, dtype=LD)
            for k in range(mesh.K):
                s, n = int(mesh.bnd[k]), int(mesh.nodes[k])
                omega[s:s + n] += LD(mesh.h[k]) * self.tables.A(n)[n - 2].astype(LD)
            I = mesh.I_mat.toarray().astype(LD)            # [N - 1][N]: h_k A_k[r][j] of the row's section
            num = Lam @ I
            mag = np.abs(Lam) @ np.abs(I)
            p, mag_p = np.empty((P.n_y, N), dtype=LD), np.empty((P.n_y, N), dtype=LD)
            wt = omega != 0
            p[:, wt], mag_p[:, wt] = num[:, wt] / omega[wt], mag[:, wt] / omega[wt]
            p[:, ~wt], mag_p[:, ~wt] = Lam[:, [N - 2]], np.abs(Lam[:, [N - 2]])
            assert np.array_equal(np.nonzero(~wt)[0], [N - 1] if self.method == "radau" else [])
            zo, _, _, _, w = ora._unpack(P, self.x)
            Fv = [np.broadcast_to(np.asarray(fn(*ora._args(P, zo, w)), float), (N,)) for fn in P.F_fn]
            f = np.array(Fv[:P.n_y]).reshape(P.n_y, N)
            g = np.array(Fv[P.n_y + P.n_p:]).reshape(P.n_q, N)
            self._ref[ip] = (omega, p, mag_p, -Lam_q, f, g)
        return self._ref[ip]

    # ---- the exact interpolant of the kernel's node costates -----------------------------------------------
    def locate(self, ip, tau):
        """(section, c) of every tau as the kernel defines them: a boundary belongs to the section on its right"""
        mesh = self.eng.meshes[ip]
        edges = mesh.tau[mesh.s]
        k = np.clip(np.searchsorted(edges, tau, side="right") - 1, 0, mesh.K - 1)
        return k, self.c_of(ip, k, tau)

    def c_of(self, ip, k, tau):
        mesh = self.eng.meshes[ip]
        edges = mesh.tau[mesh.s]
        return 2.0 * (tau - edges[k]) / (edges[k + 1] - edges[k]) - 1.0

    def _section(self, ip, k):
        if (ip, k) not in self._interp:
            mesh = self.eng.meshes[ip]
            s, n = int(mesh.s[k]), int(mesh.n[k])
            _, Cu = exact_tables(self.method, n)
            absu = np.array([[float(abs(Cu[i, j])) for j in range(n)] for i in range(n)])
            p = self.sol.costate[ip]
            with mp.workdps(DPS):
                e = [Cu * mp.matrix([mp.mpf(float(v)) for v in row[s:s + n]]) for row in p]
            self._interp[(ip, k)] = (e, [float(np.sum(absu @ np.abs(row[s:s + n]))) for row in p])
        return self._interp[(ip, k)]

    def interpolant(self, ip, k, c):
        """(p, mag) [n_y][Q] at section variable c[i] of section k[i]"""
        mesh, pl = self.eng.meshes[ip], self.eng.layout.phases[ip]
        Q = len(c)
        p, mag = np.zeros((pl.n_y, Q)), np.zeros((pl.n_y, Q))
        with mp.workdps(DPS):
            for i in range(Q):
                kk = int(k[i])
                n = int(mesh.n[kk])
                e, mag_e = self._section(ip, kk)
                x = mp.mpf(float(c[i]))
                P = [mp.mpf(1), x]
                for m in range(1, n):
                    P.append(((2 * m + 1) * x * P[m] - m * P[m - 1]) / (m + 1))
                for a in range(pl.n_y):
                    p[a, i] = float(sum(e[a][m] * P[m] for m in range(n)))
                    mag[a, i] = mag_e[a]
        return p, mag

    def base_queries(self, ip):
        """tau of: every node, every interior boundary (the right-hand section owns it), +-1, random interior points"""
        mesh = self.eng.meshes[ip]
        rng = np.random.default_rng(17 + ip)
        return np.concatenate([mesh.tau, mesh.tau[mesh.s[1:-1]], [-1.0, 1.0], rng.uniform(-1.0, 1.0, 40)])

    def base_reference(self, ip):
        key = ("base", ip)
        if key not in self._interp:
            tau = self.base_queries(ip)
            k, c = self.locate(ip, tau)
            self._interp[key] = (tau, self.interpolant(ip, k, c))
        return self._interp[key]


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


def _assert_within(got, ref, mag, what):
    ratio = entry_err(got, ref, mag, rtol=1e-10, ulps=64)
    print(f"{what}: largest |got - ref| / bound = {ratio:.3e}")
    assert ratio <= 1.0, f"{what} differs from its reference by {ratio:.3e} x its bound"


def _oracle_fg(ora, ip, x, y, u):
    """the oracle's dynamics [n_y][Q] and integrands [n_q][Q] of phase ip at the states y and controls u"""
    P = ora.P[ip]
    _, _, _, _, w = ora._unpack(P, x)
    Q = y.shape[1]
    a = [row for row in y] + [row for row in u] + [np.full(Q, w[i]) for i in range(P.n_w)]
    ev = lambda i: np.broadcast_to(np.asarray(P.F_fn[i](*a), float), (Q,))   # noqa: E731
    f = np.array([ev(i) for i in range(P.n_y)]).reshape(P.n_y, Q)
    g = np.array([ev(P.n_y + P.n_p + m) for m in range(P.n_q)]).reshape(P.n_q, Q)
    return f, g


# ---- parity at arbitrary points ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_node_costates_hamiltonian_and_nu(case, name):
    cs = case(name)
    sol, eng = cs.sol, cs.eng
    assert len(sol.costate) == len(sol.hamiltonian) == len(sol.integrand_multiplier) == len(eng.meshes)
    for ip, (pl, P) in enumerate(zip(eng.layout.phases, cs.ora.P)):
        N = pl.N
        omega, p, mag_p, nu, f, g = cs.reference(ip)
        got_p, got_H, got_nu = sol.costate[ip], sol.hamiltonian[ip], sol.integrand_multiplier[ip]
        assert got_p.shape == (pl.n_y, N) and got_H.shape == (N,) and got_nu.shape == (pl.n_q,)
        _assert_within(got_p, p.astype(float), mag_p.astype(float), f"{name} phase {ip} costates")
        # the node weights: the definition's, the solution's, and under Lobatto the mesh's own
        w_sol = sol.quadrature_weights(ip)
        assert np.all(np.abs(w_sol - omega.astype(float)) <= 4 * EPS * np.abs(omega.astype(float)))
        if cs.method == "lobatto":
            assert np.all(np.abs(omega.astype(float) - P.mesh.w) <= 4 * EPS * P.mesh.w)
            assert np.all(np.abs(w_sol - P.mesh.w) <= 4 * EPS * P.mesh.w)
        assert np.all(np.abs(got_nu - nu.astype(float)) <= 4 * EPS * np.abs(nu.astype(float)))
        H_ref = (np.sum(p * f, axis=0) + nu @ g).astype(float)
        H_mag = (np.sum(np.abs(p) * np.abs(f), axis=0) + np.abs(nu) @ np.abs(g)).astype(float)
        fin = np.ones(N, dtype=bool)
        if cs.method == "radau":
            fin[-1] = False
            W = eng.W_ocp[P.oc:P.oc + pl.n_y]
            last = cs.lam[[P.c_off + a * (N - 1) + N - 2 for a in range(pl.n_y)]]
            np.testing.assert_array_equal(got_p[:, -1], W * last / W_J)         # bit-equal
            assert np.isnan(got_H[-1])
        assert np.all(np.isfinite(got_H[fin]))
        err = np.abs(got_H[fin] - H_ref[fin]) / (1e-8 * H_mag[fin])
        print(f"{name} phase {ip} H: largest |got - ref| / bound = {np.max(err):.3e}")
        assert np.all(err <= 1.0)


# ---- sampling ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_sampled_costates_match_the_exact_interpolant(case, name):
    cs = case(name)
    for ip in range(len(cs.eng.meshes)):
        tau, (p, mag) = cs.base_reference(ip)
        gp, gH = cs.sol.sample_costate(ip, tau=tau)
        assert gp.shape == p.shape and gH.shape == tau.shape
        _assert_within(gp, p, mag, f"{name} phase {ip} p(tau)")
        # the same through times instead of tau: tau = (t - shift) / stretch as the kernel forms it
        t0, tF = cs.sol.initial_time[ip], cs.sol.final_time[ip]
        stretch, shift = 0.5 * (tF - t0), 0.5 * (t0 + tF)
        t = np.concatenate([cs.sol.node_time[ip], [t0, tF], np.random.default_rng(23).uniform(min(t0, tF), max(t0, tF), 20)])
        k, c = cs.locate(ip, np.clip((t - shift) / stretch, -1.0, 1.0))
        p, mag = cs.interpolant(ip, k, c)
        gp, _ = cs.sol.sample_costate(ip, t)
        _assert_within(gp, p, mag, f"{name} phase {ip} p(t)")


@pytest.mark.parametrize("Q", [1, 63, 64, 65, 1000])
def test_query_counts_shuffled_with_duplicates(case, Q):
    cs = case("cart_pole_ragged_K23")
    tau, (p, mag) = cs.base_reference(0)
    idx = np.random.default_rng(Q).integers(0, len(tau), Q)      # any order; duplicates from Q = 63 on at the latest
    gp, gH = cs.sol.sample_costate(0, tau=tau[idx])
    assert gp.shape == (4, Q) and gH.shape == (Q,)
    _assert_within(gp, p[:, idx], mag[:, idx], f"Q={Q} p")
    first = {}
    for j, i in enumerate(idx):   # a duplicate gets the same bits wherever it stands
        if i in first:
            assert np.array_equal(gp[:, j], gp[:, first[i]]) and gH[j] == gH[first[i]]
        first.setdefault(i, j)


@pytest.mark.parametrize("name", ["brachistochrone_K10_n4", "hypersensitive_K5_n4", "time_coupled_transfer_K6"])
def test_sampled_hamiltonian(case, name):
    """H(t) = sum p(t) f(t) + sum nu g(t): p(t) from the same call, f(t) from sample_f at the same queries, g from the
    oracle at the sampled (y, u).  The brachistochrone has no integrand, the hypersensitive problem has one."""
    cs = case(name)
    n_q = [pl.n_q for pl in cs.eng.layout.phases]
    assert (name != "brachistochrone_K10_n4" or n_q == [0]) and (name != "hypersensitive_K5_n4" or n_q == [1])
    for ip in range(len(cs.eng.meshes)):
        tau = cs.base_queries(ip)
        p, H = cs.sol.sample_costate(ip, tau=tau)
        y, _, u, f = cs.sol.sample_f(ip, tau=tau)
        f_ora, g = _oracle_fg(cs.ora, ip, cs.x, y, u)
        nu = cs.sol.integrand_multiplier[ip]
        ref = np.sum(p * f, axis=0) + nu @ g
        mag = np.sum(np.abs(p * f), axis=0) + np.abs(nu) @ np.abs(g)
        err = np.abs(H - ref) / (1e-8 * mag)
        print(f"{name} phase {ip} H(t): largest |got - ref| / bound = {np.max(err):.3e}")
        assert np.all(err <= 1.0)
        np.testing.assert_allclose(f, f_ora, rtol=1e-8, atol=1e-11 * (1 + np.max(np.abs(f_ora))))


# ---- other behaviour --------------------------------------------------------------------------------------------
def test_repeatable_and_device_tensor_variants(case):
    import torch
    from pycollo_amd.solution import Solution
    cs = case("cart_pole_ragged_K60")
    tau = cs.base_queries(0)
    tau = tau[np.random.default_rng(2).permutation(len(tau))]
    a = cs.sol.sample_costate(0, tau=tau)
    b = cs.sol.sample_costate(0, tau=tau)
    for p, q in zip(a, b):
        np.testing.assert_array_equal(p, q)
    d = cs.sol.sample_costate(0, tau=torch.tensor(tau, dtype=torch.float64, device="cuda:0"))
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in d)
    for p, q in zip(a, d):
        np.testing.assert_array_equal(p, q.cpu().numpy())
    # multipliers from a device tensor, and set a second time: the same bits
    for lam in (torch.tensor(cs.lam, dtype=torch.float64, device="cuda:0"), cs.lam.copy()):
        other = Solution(cs.eng, cs.x, multipliers=lam)
        try:
            np.testing.assert_array_equal(other.costate[0], cs.sol.costate[0])
            np.testing.assert_array_equal(other.hamiltonian[0], cs.sol.hamiltonian[0])
            np.testing.assert_array_equal(other.costate_coefficients(0), cs.sol.costate_coefficients(0))
            for p, q in zip(a, other.sample_costate(0, tau=tau)):
                np.testing.assert_array_equal(p, q)
        finally:
            other.close()


@pytest.mark.parametrize("name", ["cart_pole_ragged_K23", "hypersensitive_radau_K7_n5"])
def test_out_of_range_nan_error_and_extrapolation(case, name):
    cs = case(name)
    mesh = cs.eng.meshes[0]
    tau = np.array([-1.0 - 0.04 * mesh.h[0], 0.1, 1.0 + 0.03 * mesh.h[-1], -1.0, 1.0, np.nan])
    inside = np.array([False, True, False, True, True, False])
    p, H = cs.sol.sample_costate_unchecked(0, tau, 1)            # (PC_SOLUTION_TAU): the C call as it is
    assert np.all(np.isnan(p[:, ~inside])) and np.all(np.isfinite(p[:, inside]))
    assert np.all(np.isnan(H[~inside])) and np.all(np.isfinite(H[inside]))
    with pytest.raises(ValueError, match="outside the phase"):
        cs.sol.sample_costate(0, tau=tau[:5])
    with pytest.raises(ValueError, match="NaN"):
        cs.sol.sample_costate(0, tau=tau)
    te = tau[:5]
    gp, gH = cs.sol.sample_costate(0, tau=te, extrapolate=True)
    k = np.array([0, cs.locate(0, te[1:2])[0][0], mesh.K - 1, 0, mesh.K - 1])
    rp, mag = cs.interpolant(0, k, cs.c_of(0, k, te))
    _assert_within(gp, rp, mag, f"{name} extrapolated p")
    assert np.all(np.isfinite(gH))


def test_without_multipliers_and_refused_vectors(case):
    from pycollo_amd.solution import Solution
    cs = case("hypersensitive_K5_n4")
    plain = Solution(cs.eng, cs.x)
    try:
        assert plain.costate is None and plain.hamiltonian is None and plain.integrand_multiplier is None
        with pytest.raises(ValueError, match="without multipliers"):
            plain.sample_costate(0, tau=np.array([0.0]))
        # ... and is the solution it was: the same node values and samples as the one with multipliers
        np.testing.assert_array_equal(plain.state_derivative[0], cs.sol.state_derivative[0])
        for p, q in zip(plain.sample(0, tau=np.array([-1.0, 0.3, 1.0])), cs.sol.sample(0, tau=np.array([-1.0, 0.3, 1.0]))):
            np.testing.assert_array_equal(p, q)
    finally:
        plain.close()
    m = cs.eng.num_c
    for bad in (cs.lam[:-1], np.concatenate([cs.lam, [0.0]]), np.repeat(cs.lam, 2)[::2], cs.lam.astype(np.float32),
                cs.lam.reshape(1, m)):
        with pytest.raises(ValueError, match="multipliers must be"):
            Solution(cs.eng, cs.x, multipliers=bad)


@pytest.mark.parametrize("name", ["cart_pole_ragged_K23", "two_phase_transfer_K6"])
def test_handle_is_left_as_found(case, name):
    from pycollo_amd.solution import Solution
    cs = case(name)
    eng = cs.eng
    # (the solution with its costates was created after c_before / G_before were taken)
    cs.sol.sample_costate(0, tau=np.array([0.0, 0.5]))
    np.testing.assert_array_equal(eng.evaluate_c(cs.x), cs.c_before)
    np.testing.assert_array_equal(eng.evaluate_G_nonzeros(cs.x), cs.G_before)
    # ... and in the middle of the callback protocol: the point cached by a new_x = True call survives
    c1 = eng.evaluate_c(cs.x, new_x=True).copy()
    other = Solution(eng, 0.5 * cs.x, multipliers=2.0 * cs.lam)
    other.sample_costate(0, tau=np.array([-1.0, 0.3, 1.0]))
    other.close()
    assert eng.cache_holds(cs.x)
    np.testing.assert_array_equal(eng.evaluate_c(cs.x, new_x=False), c1)
    np.testing.assert_array_equal(eng.evaluate_G_nonzeros(cs.x), cs.G_before)
    np.testing.assert_array_equal(c1, cs.c_before)


def test_backend_solution_takes_lam_g(case):
    from pycollo_amd.pycollo_backend import Mi355x
    cs = case("hypersensitive_K5_n4")
    b = Mi355x(device=0)
    b.engine = cs.eng
    s = b.solution(cs.x, lam_g=list(cs.lam))
    try:
        np.testing.assert_array_equal(s.costate[0], cs.sol.costate[0])
        assert b.solution(cs.x).costate is None
    finally:
        s.close()
        b.engine = None


# ---- end to end -------------------------------------------------------------------------------------------------
def _solve(prob):
    from pycollo_amd.iteration import MeshIteration
    it = MeshIteration(prob)
    res = it.solve_with_ipm(tol=1e-10)
    sol = it.dense_solution()
    return it, res, sol


def _weighted_mean(sol):
    w, H = sol.quadrature_weights(0), sol.hamiltonian[0]
    use = w != 0
    return float(np.sum(w[use] * H[use]) / np.sum(w[use]))


def test_brachistochrone_lobatto_end_to_end(built):
    """Free final time, J = tF: H = -1."""
    it, res, sol = _solve(problems.brachistochrone())
    try:
        p, H = sol.costate[0], sol.hamiltonian[0]
        mean = _weighted_mean(sol)
        _report(f"brachistochrone lobatto: status {res.status}, iterations {res.iterations}, inf_du {res.inf_du:.3e}; "
                f"weighted mean of H + 1 = {mean + 1:.3e}; max |H + 1| = {np.max(np.abs(H + 1)):.3e}; "
                f"spread p_x {np.ptp(p[0]):.3e}, p_y {np.ptp(p[1]):.3e}; p(tF) = ({p[0, -1]:.8f}, {p[1, -1]:.8f}, {p[2, -1]:.3e})")
        assert abs(mean + 1) <= 1e-8
        assert np.max(np.abs(H + 1)) <= 6e-5
        assert np.ptp(p[0]) <= 4e-6 and np.ptp(p[1]) <= 4e-6
        assert abs(p[2, -1]) <= 2e-5
        np.testing.assert_allclose(p[:2, -1], [-0.1491333, -0.0569514], rtol=1e-4)
    finally:
        sol.close()
        it.engine.close()


def test_brachistochrone_radau_end_to_end(built):
    prob = problems.brachistochrone()
    prob.quadrature_method = "radau"
    it, res, sol = _solve(prob)
    try:
        p, H = sol.costate[0], sol.hamiltonian[0]
        mean = _weighted_mean(sol)
        _report(f"brachistochrone radau: status {res.status}, iterations {res.iterations}, inf_du {res.inf_du:.3e}; "
                f"weighted mean of H + 1 = {mean + 1:.3e}; p(tF) = ({p[0, -1]:.8f}, {p[1, -1]:.8f}, {p[2, -1]:.3e}); "
                f"H[-1] = {H[-1]}")
        np.testing.assert_allclose(p[:2, -1], [-0.14913330, -0.05695136], rtol=1e-5)
        assert abs(p[2, -1]) <= 1e-9
        assert abs(mean + 1) <= 1e-8
        assert np.isnan(H[-1]) and np.all(np.isfinite(H[:-1]))
    finally:
        sol.close()
        it.engine.close()


def test_hypersensitive_tf10_end_to_end(built):
    """H_u = u + p = 0 at every node; the costate at both ends; H nearly constant (autonomous)."""
    prob = problems.hypersensitive(K=32, order=8)
    ph = prob.phases[0]
    ph.bounds.final_time = 10.0
    ph.guess.time = ph.guess.time * 1e-3
    it, res, sol = _solve(prob)
    try:
        p, H, u = sol.costate[0][0], sol.hamiltonian[0], sol.control[0][0]
        _report(f"hypersensitive tF=10 K=32 n=8: status {res.status}, iterations {res.iterations}, inf_du {res.inf_du:.3e}; "
                f"max |u + p| = {np.max(np.abs(u + p)):.3e}; p(0) = {p[0]:.8f}; p(tF) = {p[-1]:.8f}; "
                f"H in [{np.min(H):.3e}, {np.max(H):.3e}]; nu = {sol.integrand_multiplier[0][0]!r}")
        assert np.max(np.abs(u + p)) <= 1e-6
        assert abs(p[0] - 0.41414700) <= 1e-6
        assert abs(p[-1] - (-7.06620524)) <= 1e-5
        assert np.all((H >= -0.005) & (H <= 0.016))
    finally:
        sol.close()
        it.engine.close()


def test_solve_ocp_solution_carries_costates(built):
    from pycollo_amd.solve import solve_ocp
    result = solve_ocp(problems.brachistochrone())
    sol = result.solution
    try:
        lay = result.final.layout
        assert sol.costate[0].shape == (lay.phases[0].n_y, lay.phases[0].N) and sol.hamiltonian[0].shape == (lay.phases[0].N,)
        assert np.all(np.isfinite(sol.costate[0])) and np.all(np.isfinite(sol.hamiltonian[0]))
    finally:
        sol.close()
        result.final.engine.close()
