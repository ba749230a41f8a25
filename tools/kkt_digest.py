"""One SHA-256 per output of the KKT solver (csrc/pc_kkt.hip) at seeded x, lam, dvec and rhs: the inertia pair, pc_kkt_solve,
pc_kkt_matvec, pc_kkt_solve_refined with its back-substitution count and pc_kkt_info, on the smallest meshes that pick each
build of the kernels and under the knobs that switch builds off; and for a factorisation cut across ranks held by one
process (tests/test_gpu_kkt_sharded.py) every rank's border block, exported panels and right-hand sides, and its
back-substitution.  The solver has no atomics and sums in a fixed order, so two trees that compute the same thing print the
same text: run it from both and compare the outputs byte for byte.

    python tools/kkt_digest.py --build-only     # compile the code objects the cases load (no GPU needed)
    python tools/kkt_digest.py > digest.txt"""
import hashlib
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
sys.path.insert(0, os.path.join(_R, "tests"))
import numpy as np

KNOBS = ("PYCOLLO_AMD_KKT_LEAF_FWD_LDS", "PYCOLLO_AMD_KKT_LEAF_WAVES", "PYCOLLO_AMD_KKT_CR_TOP", "PYCOLLO_AMD_KKT_CR")

# (problem, kwargs, group, environment)
CASES = [
    ("hypersensitive", dict(K=8, order=3), None, {}),
    ("hypersensitive", dict(K=8, order=3), 1, {}),
    ("hypersensitive", dict(K=300, order=6), None, {}),                        # cr_top_levels > 0
    ("two_phase_transfer", {}, None, {}),
    ("shuttle", dict(K=60, order=4), None, {}),
    ("time_coupled_transfer", dict(K=163, order=3), 1, {}),                    # the border grid; long rows of the product
    ("hypersensitive", dict(K=300, order=6), None, {"PYCOLLO_AMD_KKT_CR": "0"}),
    ("hypersensitive", dict(K=300, order=6), None, {"PYCOLLO_AMD_KKT_LEAF_FWD_LDS": "0"}),
    ("hypersensitive", dict(K=300, order=6), None, {"PYCOLLO_AMD_KKT_CR_TOP": "0"}),
]
# (problem, kwargs, ranks): cut across ranks, shared nodes as chain ends
SHARDED = [("sliding_mass", dict(num_phases=3, K=8, order=4), 2), ("shuttle", dict(K=60, order=4), 3)]


def _put(label, a):
    a = np.ascontiguousarray(a)
    print(f"{label} {a.dtype.str}{list(a.shape)} {hashlib.sha256(a.tobytes()).hexdigest()}", flush=True)


class _Recorded:
    """A rank's handle that prints what it hands out."""

    def __init__(self, handle, label):
        self._h, self._label = handle, label

    def __getattr__(self, name):
        fn = getattr(self._h, name)
        if name not in ("factor_partial", "export_panels", "forward_partial", "export_rhs", "backward_partial"):
            return fn

        def call(*args):
            out = fn(*args)
            parts = out if isinstance(out, (tuple, list)) else [out]
            for i, part in enumerate(parts):
                _put(f"{self._label} {name}[{i}]", np.asarray(part))
            return out
        return call


def main():
    build_only = "--build-only" in sys.argv[1:]
    from test_kkt_cpu import kkt_case
    from pycollo_amd import codegen
    for k in KNOBS:
        os.environ.pop(k, None)
    if build_only:
        for name, kw in {(n, tuple(sorted(kw.items()))) for n, kw, *_ in CASES + SHARDED}:
            eng = kkt_case(name, dict(kw), device=None)[0]
            print(codegen.build_code_object(eng.model, eng.orders, mixed=eng.mixed), flush=True)
        return
    from pycollo_amd import kkt_sharded
    from pycollo_amd.kkt import GpuKkt
    from pycollo_amd.sharding import ShardPlan
    for name, kw, group, env in CASES:
        at = f"{name} {kw} group {group} {env}"
        eng, _, x, lam, ineq, fixed, sc, dvec = kkt_case(name, kw, device=0)
        eng.evaluate_resident(x, 1.0, lam)
        os.environ.update(env)
        k = GpuKkt(eng, ineq, fixed, sc, group)
        for key in env:
            del os.environ[key]
        rng = np.random.default_rng(11)
        rhs = rng.normal(size=k.nu)
        rhs[np.nonzero(fixed)[0]] = 0.0
        _put(f"{at} inertia", np.array(k.factor(dvec), np.int64))
        _put(f"{at} solve", k.solve(rhs))
        _put(f"{at} matvec", k.matvec(dvec, rhs))
        xs, n = k.solve_refined(rhs, dvec + np.where(dvec < 0, 1e-8, 0.0))
        _put(f"{at} solve_refined", xs)
        print(f"{at} back-substitutions {n}")
        print(f"{at} info {k.info}", flush=True)
        k.close()
        eng.close()
    import torch
    from test_kkt_sharded_cpu import rank_values
    for name, kw, world in SHARDED:
        at = f"{name} {kw} ranks {world}"
        eng, _, x, lam, ineq, fixed, sc, dvec = kkt_case(name, kw, device=0)
        _, G, H = eng.evaluate_all(x, 1.0, lam)
        eng.evaluate_resident(x, 1.0, lam)
        sp = ShardPlan(eng, world)
        plan = kkt_sharded.ShardedKktPlan(eng, ineq, fixed, sc, sp, ends="chain", whole_entries=True)
        dev = torch.device("cuda", 0)
        vals = [[torch.from_numpy(a).to(dev) for a in rank_values(plan, sp, r, G, H)] for r in range(world)]
        sk = kkt_sharded.ShardedKkt(eng, plan, range(world), d_jac=[g.data_ptr() for g, _ in vals], d_hess=[h.data_ptr() for _, h in vals])
        for r in list(sk.handles):
            print(f"{at} rank {r} info {sk.handles[r].info}")
            sk.handles[r] = _Recorded(sk.handles[r], f"{at} rank {r}")
        rhs = np.random.default_rng(12).normal(size=plan.nu)
        rhs[np.nonzero(fixed)[0]] = 0.0
        _put(f"{at} inertia", np.array(sk.factor(dvec), np.int64))
        _put(f"{at} solve", sk.solve(rhs))
        sk.close()
        eng.close()


if __name__ == "__main__":
    main()
