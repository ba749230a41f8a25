"""One SHA-256 per output array of the three propagation kernels (csrc/pc_solution.hpp: pc_sol_propagate,
pc_sol_propagate_dense, pc_sol_propagate_stiff) at a seeded x, on the smallest meshes where the walk over the node
intervals and the step control they share can go wrong: every restart, fixed and adaptive steps, with and without
queries and ``integral_atol``, and the calls in which a segment fails on purpose of the numbers (``max_steps=2``, a
Newton iteration cut to one or two rounds), so that the NaN tail, the zero counts and the Newton counters are hashed too.
The kernels are built with -ffp-contract=off and sum in a fixed order, so two trees that compute the same thing print
the same text: run it from both and compare the outputs byte for byte.  Only the public Python API is used.

    python tools/propagate_digest.py --build-only     # compile the code objects the cases load (no GPU needed)
    python tools/propagate_digest.py > digest.txt"""
import hashlib
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
import numpy as np

from pycollo_amd import problems

sys.path.insert(0, os.path.join(_R, "tools"))
from post_solve_digest import _point, _radau, _sections   # noqa: E402  (the same meshes and the same seeded point)


CASES = [
    ("one_section_n2", lambda: _sections(problems.hypersensitive(), [2])),
    ("one_section_n20", lambda: _sections(problems.hypersensitive(), [20])),
    ("radau_K7_n5", _radau),
    ("two_phase_K6_n4", lambda: problems.two_phase_transfer(K=6, order=4)),
    ("no_controls_K5_n4", lambda: problems.hypersensitive(K=5, order=4, fixed_control=0.0)),
    ("free_t0_tF_K6_n4", lambda: problems.time_coupled_transfer(K=6, order=4)),
    ("cart_pole_K6_mixed", lambda: _sections(problems.cart_pole(), [3, 7, 4, 6, 5, 8])),
    ("stiff_relaxation_K5_n4", lambda: problems.stiff_relaxation(K=5, order=4)),
]
MODES = (("substeps1", dict(substeps=1)), ("substeps3", dict(substeps=3)), ("adaptive", dict(rtol=1e-8)))


def _put(label, a):
    a = np.ascontiguousarray(a)
    print(f"{label} {a.dtype.str}{list(a.shape)} {hashlib.sha256(a.tobytes()).hexdigest()}", flush=True)


def _put_all(label, result, names):
    for what in names:
        _put(f"{label}_{what}", getattr(result, what))


def main():
    build_only = "--build-only" in sys.argv[1:]
    from pycollo_amd import codegen
    from pycollo_amd.engine import NlpEngine
    from pycollo_amd.model import compile_model
    from pycollo_amd.solution import Solution
    plain = ("y", "accepted", "rejected", "status")
    dense = plain + ("q", "integral", "y_dense", "q_dense")
    stiff = plain + ("newton_rejected", "newton_iterations")
    for name, make in CASES:
        prob = make()
        if build_only:
            model = compile_model(prob)
            print(codegen.build_code_object(model, tuple(0 for _ in model.phases)), flush=True)
            continue
        eng = NlpEngine(prob, device=0, specialise=False, build=False)
        x, _ = _point(eng)
        sol = Solution(eng, x)
        for ip, mesh in enumerate(eng.meshes):
            at, N = f"{name} phase{ip}", mesh.N
            listed = np.array(sorted({0, N // 3, (2 * N) // 3, N - 1}), dtype=np.int32)
            restarts = (("nodes", "nodes"), ("sections", "sections"), ("phase", "phase"), ("listed", listed))
            # every node, seeded points between the nodes, duplicates, shuffled
            rng = np.random.default_rng(23 + ip)
            tau = np.concatenate([mesh.tau, rng.uniform(-1.0, 1.0, 3 * N)])
            tau = rng.permutation(np.concatenate([tau, tau[::5]]))
            for tag, kw in MODES:
                for rname, restart in restarts:
                    _put_all(f"{at} propagate_{tag}_{rname}", sol.propagate(ip, restart=restart, **kw), plain)
                    _put_all(f"{at} stiff_{tag}_{rname}", sol.propagate(ip, restart=restart, method="sdirk4", **kw), stiff)
                for qname, q in (("queries", tau), ("no_queries", None)):
                    for iname, ia in (("", None), ("_iatol", 1e-8)):
                        _put_all(f"{at} dense_{tag}_{qname}{iname}",
                                 sol.propagate_dense(ip, tau=q, restart="sections", integral_atol=ia, **kw), dense)
                _put_all(f"{at} dense_{tag}_queries_phase", sol.propagate_dense(ip, tau=tau, restart="phase", **kw), dense)
            # segments that fail midway: the step cap, and a Newton iteration that is not given the rounds it needs
            for rname in ("sections", "phase"):
                cap = dict(restart=rname, rtol=1e-10, max_steps=2)
                _put_all(f"{at} propagate_cap2_{rname}", sol.propagate(ip, **cap), plain)
                _put_all(f"{at} dense_cap2_{rname}", sol.propagate_dense(ip, tau=tau, **cap), dense)
                _put_all(f"{at} stiff_cap2_{rname}", sol.propagate(ip, method="sdirk4", **cap), stiff)
                _put_all(f"{at} stiff_newton1_fixed_{rname}",
                         sol.propagate(ip, restart=rname, method="sdirk4", substeps=2, newton_max=1), stiff)
                _put_all(f"{at} stiff_newton2_adaptive_{rname}",
                         sol.propagate(ip, restart=rname, method="sdirk4", rtol=1e-8, newton_max=2), stiff)
        sol.close()
        eng.close()


if __name__ == "__main__":
    main()
