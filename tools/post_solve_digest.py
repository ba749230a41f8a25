"""One SHA-256 per output array of the kernels that read a finished NLP point (csrc/pc_solution.hpp: pc_sol_fit,
pc_sol_sample, pc_sol_costate, pc_sol_sample_costate, pc_sol_propagate, pc_mesh_err) at a seeded x and lam, on the
smallest meshes where the code the six kernels share -- the phase view, the lane map, the table contraction -- can go
wrong.  The kernels are built with -ffp-contract=off and sum in a fixed order, so two trees that compute the same thing
print the same text: run it from both and compare the outputs byte for byte.

    python tools/post_solve_digest.py --build-only     # compile the code objects the cases load (no GPU needed)
    python tools/post_solve_digest.py > digest.txt"""
import hashlib
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
import numpy as np

from pycollo_amd import problems


def _sections(prob, n_k, seed=3):
    """phase 0 of ``prob`` on sections of the orders ``n_k`` and seeded unequal widths"""
    ph, K = prob.phases[0], len(n_k)
    ph.mesh.number_mesh_sections = K
    ph.mesh.mesh_section_sizes = np.random.default_rng(seed).uniform(0.3, 1.0, K)
    ph.mesh.number_mesh_section_nodes = np.asarray(n_k)
    return prob


def _lanes(total, extra):
    """orders 3 .. 8 in turn, then two sections that share what is left, so that sum(n_k + extra) == total"""
    n_k, lanes = [], 0
    while total - lanes > 2 * (8 + extra):
        n_k.append(3 + len(n_k) % 6)
        lanes += n_k[-1] + extra
    rest = total - lanes                      # two more sections share what is left
    a = rest // 2
    return n_k + [a - extra, rest - a - extra]


def _radau():
    prob = problems.hypersensitive(K=7, order=5)
    prob.quadrature_method = "radau"
    return prob


# (name, problem, runs the mesh-error kernel): the fit and costate kernels give a section n_k lanes, the mesh-error
# kernel n_k + 1 (orders 2 .. 19, Lobatto only)
CASES = [
    ("one_section_n2", lambda: _sections(problems.hypersensitive(), [2]), True),
    ("one_section_n20", lambda: _sections(problems.hypersensitive(), [20]), False),
    ("one_section_n19", lambda: _sections(problems.hypersensitive(), [19]), True),
    ("fit_lanes_256", lambda: _sections(problems.cart_pole(), _lanes(256, 0)), True),
    ("fit_lanes_257", lambda: _sections(problems.cart_pole(), _lanes(257, 0)), True),
    ("mesh_error_lanes_256", lambda: _sections(problems.cart_pole(), _lanes(256, 1)), True),
    ("mesh_error_lanes_257", lambda: _sections(problems.cart_pole(), _lanes(257, 1)), True),
    ("radau_K7_n5", _radau, False),
    ("two_phase_K6_n4", lambda: problems.two_phase_transfer(K=6, order=4), True),
    ("no_controls_K5_n4", lambda: problems.hypersensitive(K=5, order=4, fixed_control=0.0), True),
    ("free_t0_tF_K6_n4", lambda: problems.time_coupled_transfer(K=6, order=4), True),
]


def _point(eng):
    """a smooth seeded x and seeded multipliers.  x is the scaled point: a free time drawn from [0.1, 0.3] lies inside
    its own bounds once unscaled, and the registry's free-time phases bound t0 below tF, so the stretch is positive"""
    rng = np.random.default_rng(5)
    x = np.zeros(eng.num_x)
    for pl, mesh in zip(eng.layout.phases, eng.meshes):
        for b in range(pl.n_z):
            x[pl.x_off + b * pl.N:pl.x_off + (b + 1) * pl.N] = np.polynomial.polynomial.polyval(mesh.tau, rng.uniform(-0.15, 0.15, 4))
        x[pl.q_off:pl.q_off + pl.n_q + pl.n_t] = rng.uniform(0.1, 0.3, pl.n_q + pl.n_t)
    x[eng.layout.s_off:] = rng.uniform(-0.2, 0.2, eng.layout.n_s)
    return x, rng.normal(size=eng.num_c)


def _put(label, a):
    a = np.ascontiguousarray(a)
    print(f"{label} {a.dtype.str}{list(a.shape)} {hashlib.sha256(a.tobytes()).hexdigest()}", flush=True)


def main():
    build_only = "--build-only" in sys.argv[1:]
    from pycollo_amd import codegen
    from pycollo_amd.engine import NlpEngine
    from pycollo_amd.model import compile_model
    from pycollo_amd.refinement import mesh_error
    from pycollo_amd.solution import Solution
    for name, make, with_mesh_error in CASES:
        prob = make()
        if build_only:
            model = compile_model(prob)
            print(codegen.build_code_object(model, tuple(0 for _ in model.phases)), flush=True)
            continue
        eng = NlpEngine(prob, device=0, specialise=False, build=False)
        x, lam = _point(eng)
        sol = Solution(eng, x, multipliers=lam)
        for ip, mesh in enumerate(eng.meshes):
            at = f"{name} phase{ip}"
            for what in ("node_time", "state", "state_derivative", "control", "costate", "hamiltonian", "integrand_multiplier"):
                _put(f"{at} {what}", getattr(sol, what)[ip])
            for what, a in zip(("coef_dy", "coef_u"), sol.coefficients(ip)):
                _put(f"{at} {what}", a)
            _put(f"{at} coef_p", sol.costate_coefficients(ip))
            # every node, every section boundary and seeded points between them, shuffled
            rng = np.random.default_rng(17 + ip)
            tau = rng.permutation(np.concatenate([mesh.tau, rng.uniform(-1.0, 1.0, 3 * mesh.N)]))
            for what, a in zip(("sample_y", "sample_dy", "sample_u", "sample_f"), sol.sample_f(ip, tau=tau)):
                _put(f"{at} {what}", a)
            for what, a in zip(("sample_p", "sample_H"), sol.sample_costate(ip, tau=tau)):
                _put(f"{at} {what}", a)
            for tag, kw in (("substeps3", dict(substeps=3)), ("adaptive", dict(rtol=1e-8))):
                for restart in ("nodes", "phase"):
                    pr = sol.propagate(ip, restart=restart, **kw)
                    for what in ("y", "accepted", "rejected", "status"):
                        _put(f"{at} propagate_{tag}_{restart}_{what}", getattr(pr, what))
        sol.close()
        if with_mesh_error:
            for ip, (rel, ab) in enumerate(mesh_error(eng, x)):
                _put(f"{name} phase{ip} max_rel", rel)
                _put(f"{name} phase{ip} max_abs", ab)
        eng.close()


if __name__ == "__main__":
    main()
