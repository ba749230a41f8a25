"""What pc_create decides (csrc/pc_eval_shape.hpp) over a wide grid of descriptors, as text: run it from two trees that
should decide the same and compare the outputs byte for byte.

Without a device (the default) every case is a structure-only or plan-only handle: ``info`` and a SHA-256 of every
phase's tile table and tile orders.  The two-wave build is reached by setting the descriptor's ``two_wave_occupancy``,
which a device handle reads from its code object.  With ``--device`` the same cases at their smallest sizes run on real
handles, one short process each: ``info`` after one evaluation (n_launches, waves_per_tile, last_launch) and a SHA-256
each of J, grad J, c, G and H at a seeded point.

    python tools/eval_shape_digest.py > digest.txt
    python tools/eval_shape_digest.py --device > digest_device.txt     # needs a GPU
    python tools/eval_shape_digest.py --device-case N                  # (what --device starts)"""
import hashlib
import os
import subprocess
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
import numpy as np

KNOBS = {"PYCOLLO_AMD_TB": "128", "PYCOLLO_AMD_WPT": "2", "PYCOLLO_AMD_TILE_NODES": "40", "PYCOLLO_AMD_TWO_WAVE": "0",
         "PYCOLLO_AMD_TWO_WAVE_MAX_TILES": "500", "PYCOLLO_AMD_TWO_WAVE_TILES": "0", "PYCOLLO_AMD_TWO_WAVE_MAX_WAVES": "1500",
         "PYCOLLO_AMD_MIX_MIN_RUN_ROWS": "40", "PYCOLLO_AMD_MIX_CAP_ROWS": "20", "PYCOLLO_AMD_RESIDENT": "0",
         "PYCOLLO_AMD_TAIL_BLOCKS": "3", "PYCOLLO_AMD_MERGE": "0"}
OCC = [None]   # two_wave_occupancy of the descriptors made from here on (None: what the engine finds)


def _sha(a):
    a = np.ascontiguousarray(a)
    return f"{a.dtype.str}{list(a.shape)} {hashlib.sha256(a.tobytes()).hexdigest()[:16]}"


def _patch():
    from pycollo_amd.engine import NlpEngine
    make = NlpEngine._make_desc

    def make_desc(self, code_object, tpb):
        desc = make(self, code_object, tpb)
        if OCC[0] is not None:
            desc.two_wave_occupancy = OCC[0]
        return desc
    NlpEngine._make_desc = make_desc


def _report(at, eng):
    print(f"{at} info {eng.info}")
    for ip in range(len(eng.model.phases)):
        tiles = eng.phase_tiles(ip)
        print(f"{at} phase {ip} tiles " + " ".join(_sha(a) for a in (tiles if isinstance(tiles, tuple) else (tiles,)))
              + " orders " + _sha(eng.phase_tile_orders(ip)), flush=True)


def _case(at, make, occ=None, env=None):
    OCC[0] = occ
    os.environ.update(env or {})
    at = f"{at} occ {occ} {env or {}}"
    try:
        obj = make()
        _report(at, getattr(obj, "engine", obj))
        obj.close()
    except Exception as e:   # a refusal is a decision too
        print(f"{at} refused: {e}", flush=True)
    for k in env or {}:
        del os.environ[k]
    OCC[0] = None


def structure_only():
    from pycollo_amd import problems
    from pycollo_amd.engine import NlpEngine
    from pycollo_amd.sharding import LocalShard
    R = problems.REGISTRY
    for name in R:
        if name != "function_family":
            _case(f"{name} default", lambda: NlpEngine(R[name](), device=None))
    # tile counts on either side of 400, 512, 896, 1024 and 2048: sections of order 4, 21 to a 64-node tile
    for name in ("hypersensitive", "sliding_mass", "shuttle"):
        for T in (400, 401, 512, 513, 896, 897, 1024, 1025, 2048, 2049):
            _case(f"{name} K={21 * T} order 4", lambda: NlpEngine(R[name](K=21 * T, order=4), device=None), occ=2)
    for name, K, orders in (("shuttle", 3000, range(3, 9)), ("delta_iii", 700, range(3, 9)), ("delta_iii", 3000, range(3, 9)),
                            ("delta_iii", 1300, (5,)), ("delta_iii", 6000, (5,)), ("two_phase_transfer", 3000, range(3, 9))):
        for order in orders:
            for occ in (0, 2):
                _case(f"{name} K={K} order {order}", lambda: NlpEngine(R[name](K=K, order=order), device=None), occ=occ)
    for name in ("hypersensitive", "shuttle", "delta_iii"):
        for tpb in (0, 64, 128, 256):
            _case(f"{name} K=3000 order 5 tpb {tpb}", lambda: NlpEngine(R[name](K=3000, order=5), device=None, threads_per_block=tpb), occ=2)
    for K in (8333, 8334, 21845, 21846, 87381, 87382):   # 24 999 / 25 000, 65 535 / 65 536, 262 143 / 262 144 nodes
        _case(f"hypersensitive K={K} order 4", lambda: NlpEngine(R["hypersensitive"](K=K, order=4), device=None))
    for name, nodes, seeds in (("hypersensitive", 30000, (3,)), ("delta_iii", 12500, (7, 8, 9, 10)), ("shuttle", 20000, (5,)),
                               ("two_phase_transfer", 12000, (1, 2))):
        for occ in (0, 2):
            _case(f"{name} refined {nodes}", lambda: NlpEngine(problems.with_refined_mesh(R[name](), nodes, seeds=seeds), device=None, mixed="auto"), occ=occ)
    for name, kw, world in (("two_phase_transfer", dict(K=40, order=4), 3), ("delta_iii", dict(K=3000, order=5), 4), ("hypersensitive", dict(K=2000, order=6), 2)):
        for rank in range(world):
            for occ in (0, 2):
                _case(f"{name} {kw} rank {rank} of {world}", lambda: LocalShard(R[name](**kw), rank, world, device=None), occ=occ)
    for name, kw in (("delta_iii", dict(K=3000, order=5)), ("hypersensitive", dict(K=2000, order=6))):
        _case(f"{name} {kw} plan_only", lambda: NlpEngine(R[name](**kw), device=None, plan_only=True), occ=2)
    _case("delta_iii refined 12500 plan_only", lambda: NlpEngine(problems.with_refined_mesh(R["delta_iii"](), 12500, seeds=(7, 8, 9, 10)),
                                                                  device=None, mixed="auto", plan_only=True), occ=2)
    for key, v in KNOBS.items():
        _case("delta_iii K=3000 order 5", lambda: NlpEngine(R["delta_iii"](K=3000, order=5), device=None), occ=2, env={key: v})
        _case("delta_iii refined 12500", lambda: NlpEngine(problems.with_refined_mesh(R["delta_iii"](), 12500, seeds=(7, 8, 9, 10)), device=None, mixed="auto"), occ=2, env={key: v})
        _case("hypersensitive K=2000 order 6", lambda: NlpEngine(R["hypersensitive"](K=2000, order=6), device=None), env={key: v})


# (problem, kwargs, refined nodes or 0, environment): orders and models the build step compiles code objects for
DEVICE_CASES = [("hypersensitive", dict(K=40, order=5), 0, {}), ("hypersensitive", dict(K=2000, order=6), 0, {}),
                ("cart_pole", dict(K=50, order=4), 0, {}), ("shuttle", dict(K=300, order=5), 0, {}),
                ("two_phase_transfer", dict(K=40, order=4), 0, {}), ("time_coupled_transfer", dict(K=40, order=4), 0, {}),
                ("delta_iii", dict(K=40, order=5), 0, {}), ("delta_iii", dict(K=3000, order=5), 0, {}),
                ("sliding_mass", dict(num_phases=3, K=8, order=4), 0, {}),
                ("hypersensitive", {}, 30000, {}), ("delta_iii", {}, 12500, {})]
DEVICE_CASES += [("delta_iii", dict(K=3000, order=5), 0, {k: v}) for k, v in KNOBS.items()]
DEVICE_CASES += [("hypersensitive", dict(K=2000, order=6), 0, {k: KNOBS[k]}) for k in ("PYCOLLO_AMD_TB", "PYCOLLO_AMD_WPT", "PYCOLLO_AMD_RESIDENT", "PYCOLLO_AMD_TAIL_BLOCKS")]
DEVICE_CASES += [("delta_iii", {}, 12500, {k: KNOBS[k]}) for k in ("PYCOLLO_AMD_MIX_CAP_ROWS", "PYCOLLO_AMD_TWO_WAVE_MAX_WAVES")]
REFINED_SEEDS = {"hypersensitive": (3,), "delta_iii": (7, 8, 9, 10)}


def device_case(i):
    from pycollo_amd import problems
    from pycollo_amd.engine import NlpEngine
    name, kw, refined, env = DEVICE_CASES[i]
    os.environ.update(env)
    prob = problems.REGISTRY[name](**kw)
    if refined:
        prob = problems.with_refined_mesh(prob, refined, seeds=REFINED_SEEDS[name])
    at = f"{name} {kw} refined {refined} {env}"
    eng = NlpEngine(prob, device=0)
    rng = np.random.default_rng(5)
    x = rng.uniform(0.05, 0.3, eng.num_x)
    lam = rng.normal(size=eng.num_c)
    c, G, H = eng.evaluate_all(x, 1.0, lam)
    print(f"{at} info {eng.info}")
    for label, a in (("J", np.array(eng.evaluate_J(x))), ("grad", eng.evaluate_g(x)), ("c", c), ("G", G), ("H", H)):
        print(f"{at} {label} {_sha(np.asarray(a))}")
    sys.stdout.flush()
    eng.close()


def main():
    args = sys.argv[1:]
    for k in KNOBS:
        os.environ.pop(k, None)
    if args[:1] == ["--device-case"]:
        return device_case(int(args[1]))
    if args[:1] == ["--device"]:
        for i in range(len(DEVICE_CASES)):   # a case that fails or runs out of time ends the run: nothing more is started on the device
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--device-case", str(i)], capture_output=True, text=True, timeout=120)
            sys.stdout.write(res.stdout)
            sys.stdout.flush()
            if res.returncode != 0:
                sys.stdout.write(f"case {i} ended with status {res.returncode}: {res.stderr[-2000:]}\n")
                return 1
        return 0
    _patch()
    structure_only()
    return 0


if __name__ == "__main__":
    sys.exit(main())
