"""Dense output of an NLP point (pycollo_amd/solution.py, csrc/pc_solution.hpp) on the GPU.

Node values: y, u bit-equal to V x~ + r; the state derivatives against the oracle's dynamics (``OracleNlp._unpack`` /
``_args`` / ``F_fn``, as oracle/ref_refine.py uses them), rtol 1e-8, atol 1e-11 (1 + the phase's largest |f|).

Sampling: against the mpmath (60 digits) exact interpolant of *the kernel's own node values*, so that only the
interpolation is under test, entry by entry with ``conftest.entry_err(got, ref, mag, rtol=1e-10, ulps=64)``:
mag = sum_k sum_i |C_ki||v_i| for ydot and u, and |y(tau_k)| + |stretch h_k| sum_k sum_i |C_ki||f_i| for y.  A coefficient
contraction (n roundings of that magnitude per coefficient) followed by Clenshaw with |P_k| <= 1, |int P_k| <= 2 costs at
most 3n + 2 <= 62 roundings of mag at n <= 20, so the project's 64 ulps hold with nothing left out; an indexing,
ownership or factor error is O(1).  The reference takes the section variable c of a query as the kernel defines it
(c = 2 (tau - tau_k) / h_k - 1 in float64, tau = (t - shift) / stretch) and is exact from there."""
import mpmath as mp
import numpy as np
import pytest

from conftest import entry_err, golden_tables
from oracle.ref_numpy import OracleNlp
from pycollo_amd import problems
from pycollo_amd.solution import exact_tables

pytestmark = pytest.mark.gpu

DPS = 60


def _ragged(prob, seed=3, K=23):
    """the ragged pattern of test_gpu_refinement.py"""
    rng = np.random.default_rng(seed)
    ph = prob.phases[0]
    ph.mesh.number_mesh_sections = K
    ph.mesh.mesh_section_sizes = rng.uniform(0.3, 1.0, K)
    ph.mesh.number_mesh_section_nodes = rng.integers(3, 9, K)
    return prob


def _extremes():
    prob = problems.hypersensitive(K=5, order=4)
    ph = prob.phases[0]
    ph.mesh.mesh_section_sizes = np.array([0.1, 0.3, 0.15, 0.25, 0.2])
    ph.mesh.number_mesh_section_nodes = np.array([2, 20, 3, 20, 2])
    return prob


def _radau():
    prob = problems.hypersensitive(K=7, order=5)
    prob.quadrature_method = "radau"
    return prob


CASES = {
    "hypersensitive_K5_n4": lambda: problems.hypersensitive(K=5, order=4),               # 21 nodes, below one wave
    "cart_pole_ragged_K23": lambda: _ragged(problems.cart_pole(K=10, order=4)),          # ragged mesh, orders 3-8
    "cart_pole_ragged_K60": lambda: _ragged(problems.cart_pole(K=10, order=4), K=60),    # lanes pass one 256-lane workgroup
    "order_extremes_2_and_20": _extremes,                                                # n = 2 and n = 20 in one mesh
    "two_phase_transfer_K6": lambda: problems.two_phase_transfer(K=6, order=4),          # second phase's offsets
    "time_coupled_transfer_K6": lambda: problems.time_coupled_transfer(K=6, order=4),    # free times, q / t / s inside f
    "hypersensitive_radau_K7_n5": _radau,                                                # Radau
}


def _smooth_x(eng):
    """the smooth random point of test_gpu_refinement.py"""
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
        self.method = self.eng.quad.method
        self.ora = OracleNlp(self.prob, golden_tables(self.method), V_ocp=self.eng.V_ocp, r_ocp=self.eng.r_ocp,
                             W_ocp=self.eng.W_ocp)
        self.x = _smooth_x(self.eng)
        self.c_before = self.eng.evaluate_c(self.x).copy()
        self.G_before = self.eng.evaluate_G_nonzeros(self.x).copy()
        self.sol = Solution(self.eng, self.x, objective=1.25)
        self._exact = {}
        self._coef = {}

    def close(self):
        self.sol.close()
        self.eng.close()

    # ---- the exact interpolant of the kernel's node values ------------------------------------------------
    def exact(self, n):
        if n not in self._exact:
            Cd, Cu = exact_tables(self.method, n)
            absd = np.array([[float(abs(Cd[i, j])) for j in range(n)] for i in range(n)])
            absu = np.array([[float(abs(Cu[i, j])) for j in range(n)] for i in range(n)])
            self._exact[n] = (Cd, Cu, absd, absu)
        return self._exact[n]

    def section(self, ip, k):
        """exact Legendre coefficients of ydot and u of section k, and the magnitudes sum_k sum_i |C_ki||v_i|"""
        if (ip, k) not in self._coef:
            mesh = self.eng.meshes[ip]
            s, n = int(mesh.s[k]), int(mesh.n[k])
            Cd, Cu, absd, absu = self.exact(n)
            f, u = self.sol.state_derivative[ip], self.sol.control[ip]
            with mp.workdps(DPS):
                a = [Cd * mp.matrix([mp.mpf(float(v)) for v in row[s:s + n]]) for row in f] if len(f) else []
                e = [Cu * mp.matrix([mp.mpf(float(v)) for v in row[s:s + n]]) for row in u] if len(u) else []
            mag_a = [float(np.sum(absd @ np.abs(row[s:s + n]))) for row in f] if len(f) else []
            mag_e = [float(np.sum(absu @ np.abs(row[s:s + n]))) for row in u] if len(u) else []
            self._coef[(ip, k)] = (a, e, mag_a, mag_e)
        return self._coef[(ip, k)]

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

    def reference(self, ip, k, c):
        """(y, ydot, u, mag_y, mag_ydot, mag_u), each [var][Q], for queries at section variable c[i] of section k[i]"""
        mesh, pl = self.eng.meshes[ip], self.eng.layout.phases[ip]
        edges = mesh.tau[mesh.s]
        stretch = 0.5 * (self.sol.final_time[ip] - self.sol.initial_time[ip])
        Q = len(c)
        y, dy, u = np.zeros((pl.n_y, Q)), np.zeros((pl.n_y, Q)), np.zeros((pl.n_u, Q))
        my, md, mu = np.zeros((pl.n_y, Q)), np.zeros((pl.n_y, Q)), np.zeros((pl.n_u, Q))
        with mp.workdps(DPS):
            for i in range(Q):
                kk, n = int(k[i]), int(mesh.n[int(k[i])])
                a, e, mag_a, mag_e = self.section(ip, kk)
                x = mp.mpf(float(c[i]))
                P = [mp.mpf(1), x]
                for m in range(1, n + 1):
                    P.append(((2 * m + 1) * x * P[m] - m * P[m - 1]) / (m + 1))
                I = [x + 1] + [(P[m + 1] - P[m - 1]) / (2 * m + 1) for m in range(1, n)]     # int_{-1}^{c} P_m
                w = mp.mpf(float(edges[kk + 1] - edges[kk]))
                for b in range(pl.n_y):
                    y0 = float(self.sol.state[ip][b][int(mesh.s[kk])])
                    dy[b, i] = float(sum(a[b][m] * P[m] for m in range(n)))
                    y[b, i] = float(mp.mpf(y0) + mp.mpf(stretch) * (w / 2) * sum(a[b][m] * I[m] for m in range(n)))
                    md[b, i] = mag_a[b]
                    my[b, i] = abs(y0) + abs(stretch * float(w)) * mag_a[b]
                for b in range(pl.n_u):
                    u[b, i] = float(sum(e[b][m] * P[m] for m in range(n)))
                    mu[b, i] = mag_e[b]
        return y, dy, u, my, md, mu

    def base_queries(self, ip):
        """tau of: every node, every interior boundary, +-1, random interior points"""
        mesh = self.eng.meshes[ip]
        rng = np.random.default_rng(17 + ip)
        return np.concatenate([mesh.tau, mesh.tau[mesh.s[1:-1]], [-1.0, 1.0], rng.uniform(-1.0, 1.0, 40)])

    def base_reference(self, ip):
        key = ("base", ip)
        if key not in self._coef:
            tau = self.base_queries(ip)
            k, c = self.locate(ip, tau)
            self._coef[key] = (tau, self.reference(ip, k, c))
        return self._coef[key]


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
    assert ratio <= 1.0, f"{what} differs from the exact interpolant by {ratio:.3e} x its bound"


def _oracle_f(ora, ip, x, y, u):
    """the oracle's dynamics of phase ip at the states y [n_y][Q] and controls u [n_u][Q], parameters from x"""
    P = ora.P[ip]
    _, _, _, _, w = ora._unpack(P, x)
    Q = y.shape[1]
    a = [row for row in y] + [row for row in u] + [np.full(Q, w[i]) for i in range(P.n_w)]
    return np.array([np.broadcast_to(np.asarray(P.F_fn[i](*a), float), (Q,)) for i in range(P.n_y)])


@pytest.mark.parametrize("name", list(CASES))
def test_node_values(case, name):
    cs = case(name)
    eng, sol, x = cs.eng, cs.sol, cs.x
    lay = eng.layout
    xu = lay.expand_x(eng.V_ocp) * x + lay.expand_x(eng.r_ocp)
    assert len(sol.state) == len(lay.phases) and sol.objective == 1.25
    for ip, (pl, pm, mesh, P) in enumerate(zip(lay.phases, eng.model.phases, eng.meshes, cs.ora.P)):
        z = xu[pl.x_off:pl.x_off + pl.n_z * pl.N].reshape(pl.n_z, pl.N)
        np.testing.assert_array_equal(sol.state[ip], z[:pl.n_y])
        np.testing.assert_array_equal(sol.control[ip], z[pl.n_y:])
        np.testing.assert_array_equal(sol.integral[ip], xu[pl.q_off:pl.q_off + pl.n_q])
        np.testing.assert_array_equal(sol.time[ip], xu[pl.t_off:pl.t_off + pl.n_t])
        np.testing.assert_array_equal(sol.tau[ip], mesh.tau)
        zo, _, stretch, _, w = cs.ora._unpack(P, x)
        ref = np.array([np.broadcast_to(np.asarray(P.F_fn[i](*cs.ora._args(P, zo, w)), float), (pl.N,)) for i in range(P.n_y)])
        assert sol.state_derivative[ip].shape == (pl.n_y, pl.N)
        np.testing.assert_allclose(sol.state_derivative[ip], ref, rtol=1e-8, atol=1e-11 * (1 + np.max(np.abs(ref))))
        t0, tF = sol.initial_time[ip], sol.final_time[ip]
        assert abs(stretch - (tF - t0) / 2) <= 1e-14 * abs(stretch)
        np.testing.assert_array_equal(sol.node_time[ip], mesh.tau * ((tF - t0) / 2) + (t0 + tF) / 2)   # casadi_solution.py:80-83
    np.testing.assert_array_equal(sol.parameter, xu[lay.s_off:])


@pytest.mark.parametrize("name", list(CASES))
def test_sampling_matches_the_exact_interpolant(case, name):
    cs = case(name)
    for ip in range(len(cs.eng.meshes)):
        mesh = cs.eng.meshes[ip]
        tau, (y, dy, u, my, md, mu) = cs.base_reference(ip)
        gy, gd, gu = cs.sol.sample(ip, tau=tau)
        _assert_within(gy, y, my, f"{name} phase {ip} y")
        _assert_within(gd, dy, md, f"{name} phase {ip} ydot")
        _assert_within(gu, u, mu, f"{name} phase {ip} u")
        # an interior boundary belongs to the section on its right: the left-hand section's polynomial, whose y at its
        # end is the integrated form, is somewhere else
        nb = mesh.K - 1
        if nb:
            bt = tau[mesh.N:mesh.N + nb]
            kl = np.arange(nb)
            yl, _, _, myl, _, _ = cs.reference(ip, kl, cs.c_of(ip, kl, bt))
            gb = gy[:, mesh.N:mesh.N + nb]
            for j in range(nb):
                assert entry_err(gb[:, j], yl[:, j], myl[:, j], rtol=1e-10, ulps=64) > 1.0, \
                    f"boundary {j + 1}: the sample equals the left-hand section's value"
        # the same through times instead of tau: tau = (t - shift) / stretch as the kernel forms it
        t0, tF = cs.sol.initial_time[ip], cs.sol.final_time[ip]
        stretch, shift = 0.5 * (tF - t0), 0.5 * (t0 + tF)
        rng = np.random.default_rng(23)
        t = np.concatenate([cs.sol.node_time[ip], [t0, tF], rng.uniform(min(t0, tF), max(t0, tF), 20)])
        tt = np.clip((t - shift) / stretch, -1.0, 1.0)     # (a time within 8 eps of the end is the end)
        k, c = cs.locate(ip, tt)
        y, dy, u, my, md, mu = cs.reference(ip, k, c)
        gy, gd, gu = cs.sol.sample(ip, t)
        _assert_within(gy, y, my, f"{name} phase {ip} y(t)")
        _assert_within(gd, dy, md, f"{name} phase {ip} ydot(t)")
        _assert_within(gu, u, mu, f"{name} phase {ip} u(t)")
        assert k[len(cs.sol.node_time[ip])] == 0 and k[len(cs.sol.node_time[ip]) + 1] == mesh.K - 1


@pytest.mark.parametrize("Q", [1, 63, 64, 65, 257, 70000])
def test_query_counts_shuffled_with_duplicates(case, Q):
    cs = case("cart_pole_ragged_K23")
    tau, (y, dy, u, my, md, mu) = cs.base_reference(0)
    idx = np.random.default_rng(Q).integers(0, len(tau), Q)      # any order; duplicates from Q = 63 on at the latest
    gy, gd, gu = cs.sol.sample(0, tau=tau[idx])
    assert gy.shape == (4, Q) and gd.shape == (4, Q) and gu.shape == (1, Q)
    _assert_within(gy, y[:, idx], my[:, idx], f"Q={Q} y")
    _assert_within(gd, dy[:, idx], md[:, idx], f"Q={Q} ydot")
    _assert_within(gu, u[:, idx], mu[:, idx], f"Q={Q} u")
    if Q > 1:   # a duplicate gets the same bits wherever it stands
        first = {}
        for j, i in enumerate(idx[:2000]):
            if i in first:
                assert np.array_equal(gy[:, j], gy[:, first[i]]) and np.array_equal(gu[:, j], gu[:, first[i]])
            first.setdefault(i, j)


@pytest.mark.parametrize("name", ["cart_pole_ragged_K23", "time_coupled_transfer_K6", "hypersensitive_radau_K7_n5"])
def test_out_of_range_nan_error_and_extrapolation(case, name):
    cs = case(name)
    for ip in range(len(cs.eng.meshes)):
        mesh = cs.eng.meshes[ip]
        h0, hK = mesh.h[0], mesh.h[-1]
        tau = np.array([-1.0 - 0.04 * h0, 0.1, 1.0 + 0.03 * hK, -1.0, 1.0, np.nan])
        # the C call: NaN in every output of a query outside the phase, the others untouched by their neighbours
        y, dy, u, f = cs.sol.sample_f(ip, tau=tau)
        inside = np.array([False, True, False, True, True, False])
        for arr in (y, dy, u, f):
            assert np.all(np.isnan(arr[:, ~inside])) and np.all(np.isfinite(arr[:, inside]))
        t0, tF = cs.sol.initial_time[ip], cs.sol.final_time[ip]
        lo, hi = min(t0, tF), max(t0, tF)
        y, dy, u, f = cs.sol.sample_f(ip, np.array([lo - 1e-9 * (hi - lo), hi + 1e-9 * (hi - lo), lo, hi]))
        for arr in (y, dy, u, f):
            assert np.all(np.isnan(arr[:, :2])) and np.all(np.isfinite(arr[:, 2:]))
        # Python: ValueError
        with pytest.raises(ValueError, match="outside the phase"):
            cs.sol.sample(ip, tau=tau[:5])
        with pytest.raises(ValueError, match="outside the phase"):
            cs.sol.sample(ip, np.array([hi + 1e-9 * (hi - lo)]))
        # extrapolate=True: the end sections' polynomials, extended
        te = tau[:5]
        gy, gd, gu = cs.sol.sample(ip, tau=te, extrapolate=True)
        k = np.array([0, cs.locate(ip, te[1:2])[0][0], mesh.K - 1, 0, mesh.K - 1])
        ry, rd, ru, my, md, mu = cs.reference(ip, k, cs.c_of(ip, k, te))
        _assert_within(gy, ry, my, f"{name} phase {ip} extrapolated y")
        _assert_within(gd, rd, md, f"{name} phase {ip} extrapolated ydot")
        _assert_within(gu, ru, mu, f"{name} phase {ip} extrapolated u")


@pytest.mark.parametrize("name", ["cart_pole_ragged_K23", "two_phase_transfer_K6", "time_coupled_transfer_K6",
                                  "hypersensitive_radau_K7_n5"])
def test_f_output_and_residual(case, name):
    cs = case(name)
    for ip in range(len(cs.eng.meshes)):
        tau = cs.base_queries(ip)
        y, dy, u, f = cs.sol.sample_f(ip, tau=tau)
        ref = _oracle_f(cs.ora, ip, cs.x, y, u)          # at the *returned* y, u
        np.testing.assert_allclose(f, ref, rtol=1e-8, atol=1e-11 * (1 + np.max(np.abs(ref))))
        y2, dy2, u2, res = cs.sol.sample(ip, tau=tau, residual=True)
        np.testing.assert_array_equal(y2, y)
        np.testing.assert_array_equal(dy2, dy)
        np.testing.assert_array_equal(u2, u)
        np.testing.assert_array_equal(res, dy - f)
        # at a node ydot interpolates f(node values); f(y(t), u(t)) is taken at the integrated y: the residual is there
        assert np.all(np.isfinite(res))


def test_repeatable_host_and_device_tensor_variants(case):
    import torch
    cs = case("cart_pole_ragged_K60")
    tau = cs.base_queries(0)
    rng = np.random.default_rng(2)
    tau = tau[rng.permutation(len(tau))]
    a = cs.sol.sample(0, tau=tau, residual=True)
    b = cs.sol.sample(0, tau=tau, residual=True)
    for p, q in zip(a, b):
        np.testing.assert_array_equal(p, q)
    d = cs.sol.sample(0, tau=torch.tensor(tau, dtype=torch.float64, device="cuda:0"), residual=True)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in d)
    for p, q in zip(a, d):
        np.testing.assert_array_equal(p, q.cpu().numpy())
    with pytest.raises(ValueError, match="outside the phase"):
        cs.sol.sample(0, tau=torch.tensor([0.0, 1.5], dtype=torch.float64, device="cuda:0"))
    # a solution made from a device x is the same solution
    from pycollo_amd.solution import Solution
    sd = Solution(cs.eng, torch.tensor(cs.x, dtype=torch.float64, device="cuda:0"))
    try:
        np.testing.assert_array_equal(sd.state_derivative[0], cs.sol.state_derivative[0])
        for p, q in zip(sd.coefficients(0), cs.sol.coefficients(0)):
            np.testing.assert_array_equal(p, q)
        for p, q in zip(a[:3], sd.sample(0, tau=tau)):
            np.testing.assert_array_equal(p, q)
    finally:
        sd.close()


@pytest.mark.parametrize("name", ["cart_pole_ragged_K23", "two_phase_transfer_K6"])
def test_handle_is_left_as_found(case, name):
    cs = case(name)
    eng = cs.eng
    # (the solution was created and sampled after c_before / G_before were taken)
    cs.sol.sample(0, tau=np.array([0.0, 0.5]), residual=True)
    np.testing.assert_array_equal(eng.evaluate_c(cs.x), cs.c_before)
    np.testing.assert_array_equal(eng.evaluate_G_nonzeros(cs.x), cs.G_before)
    # ... and in the middle of the callback protocol: the point cached by a new_x = True call survives
    c1 = eng.evaluate_c(cs.x, new_x=True).copy()
    from pycollo_amd.solution import Solution
    other = Solution(eng, 0.5 * cs.x)
    other.sample(0, tau=np.array([-1.0, 0.3, 1.0]), residual=True)
    other.close()
    assert eng.cache_holds(cs.x)
    np.testing.assert_array_equal(eng.evaluate_c(cs.x, new_x=False), c1)
    np.testing.assert_array_equal(eng.evaluate_G_nonzeros(cs.x), cs.G_before)
    np.testing.assert_array_equal(c1, cs.c_before)


def test_polys_agree_with_sample(case):
    cs = case("cart_pole_ragged_K23")
    mesh = cs.eng.meshes[0]
    y_p, dy_p, u_p = cs.sol.polys(0)
    assert y_p.shape == dy_p.shape == (4, mesh.K) and u_p.shape == (1, mesh.K)
    tau, (_, _, _, my, md, mu) = cs.base_reference(0)
    k, _ = cs.locate(0, tau)
    gy, gd, gu = cs.sol.sample(0, tau=tau)
    py = np.array([[y_p[a, kk](t) for kk, t in zip(k, tau)] for a in range(4)])
    pd = np.array([[dy_p[a, kk](t) for kk, t in zip(k, tau)] for a in range(4)])
    pu = np.array([[u_p[0, kk](t) for kk, t in zip(k, tau)]])
    _assert_within(py, gy, my, "polys y")
    _assert_within(pd, gd, md, "polys ydot")
    _assert_within(pu, gu, mu, "polys u")
    assert dy_p[0, 3].degree() == mesh.n[3] - 1 and y_p[0, 3].degree() == mesh.n[3]
    dc, uc = cs.sol.coefficients(0)
    assert dc.shape == (4, mesh.N + mesh.K - 1) and uc.shape == (1, mesh.N + mesh.K - 1)


def test_radau_derivative_has_one_degree_less(case):
    cs = case("hypersensitive_radau_K7_n5")
    mesh = cs.eng.meshes[0]
    dc, uc = cs.sol.coefficients(0)
    top = mesh.s[:-1] + np.arange(mesh.K) + mesh.n - 1          # every section's highest coefficient
    assert np.all(dc[:, top] == 0.0) and np.all(dc[:, top - 1] != 0.0)


def test_backend_solution(case):
    from pycollo_amd.pycollo_backend import Mi355x
    cs = case("hypersensitive_K5_n4")
    b = Mi355x(device=0)
    b.engine = cs.eng
    s = b.solution(cs.x, objective=2.0)
    try:
        assert s.objective == 2.0
        np.testing.assert_array_equal(s.state_derivative[0], cs.sol.state_derivative[0])
        # the host evaluation it replaces for the node derivatives (Mi355x._dy)
        ref = b._dy(cs.x).reshape(cs.sol.state_derivative[0].shape)
        np.testing.assert_allclose(s.state_derivative[0], ref, rtol=1e-8, atol=1e-11 * (1 + np.max(np.abs(ref))))
    finally:
        s.close()
        b.engine = None


def test_solve_ocp_end_to_end(built):
    from pycollo_amd.solve import solve_ocp
    result = solve_ocp(problems.brachistochrone())
    sol = result.solution
    assert sol is result.solution                                   # built once, kept
    assert sol.objective == result.objective
    taus, ys, us, qs, ts, s = result.final.solution()
    lay = result.final.layout
    for ip, pl in enumerate(lay.phases):
        np.testing.assert_array_equal(sol.tau[ip], taus[ip])
        np.testing.assert_array_equal(sol.state[ip], ys[ip])
        np.testing.assert_array_equal(sol.control[ip], us[ip])
        np.testing.assert_array_equal(sol.integral[ip], qs[ip])
        np.testing.assert_array_equal(sol.time[ip], ts[ip])
        # the reference's shapes (casadi_solution.py:43-86)
        assert sol.state[ip].shape == sol.state_derivative[ip].shape == (pl.n_y, pl.N)
        assert sol.control[ip].shape == (pl.n_u, pl.N)
        assert sol.node_time[ip].shape == sol.tau[ip].shape == (pl.N,)
        assert sol.integral[ip].shape == (pl.n_q,) and sol.time[ip].shape == (pl.n_t,)
        assert isinstance(sol.initial_time[ip], float) and isinstance(sol.final_time[ip], float)
        assert abs(sol.node_time[ip][0] - sol.initial_time[ip]) < 1e-12 and abs(sol.node_time[ip][-1] - sol.final_time[ip]) < 1e-12
    np.testing.assert_array_equal(sol.parameter, s)
    for name in ("state", "state_derivative", "control", "integral", "time", "initial_time", "final_time", "node_time", "tau"):
        assert isinstance(getattr(sol, name), tuple) and len(getattr(sol, name)) == len(lay.phases)
    # dense output of the converged trajectory: every time of the phase is inside, node_time's own entries included
    y, dy, u, res = sol.sample(0, sol.node_time[0], residual=True)
    assert y.shape == (lay.phases[0].n_y, lay.phases[0].N) and np.all(np.isfinite(res))
    t = np.linspace(sol.initial_time[0], sol.final_time[0], 101)
    y, dy, u, res = sol.sample(0, t, residual=True)
    assert np.all(np.isfinite(y)) and np.all(np.isfinite(res))
    sol.close()
    result.final.engine.close()
