"""Wall time of the derivative check (NlpEngine.check_derivatives, pc_check_derivatives_device) against one fused
evaluation of the same NLP, at BASELINE.json configs 2-5 and on the refined Delta III mesh; under
rocprofv3 --kernel-trace --stats it gives the per-kernel table of the check (profiles/r05_deriv_check_*).
Both times are warm and taken between HIP events on the handle's stream.  The dense forward-difference count (n + 1,
IPOPT's derivative_test) is computed from the size of the NLP, not measured."""
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
import numpy as np
import torch

from pycollo_amd import problems
from pycollo_amd.engine import NlpEngine
from pycollo_amd.iteration import MeshIteration

CONFIGS = [
    ("config 2: hypersensitive 2000 x 6", lambda: problems.hypersensitive(K=2000, order=6), (-0.45, 0.45)),
    ("config 3: cart-pole 5000 x 4", lambda: problems.cart_pole(K=5000, order=4), (-0.45, 0.45)),
    ("config 4: shuttle 20000 x 4", lambda: problems.shuttle(K=20000, order=4), (-0.45, 0.45)),
    # (Delta III near its mesh iteration's scaled guess, velocities moved off v_rel = 0: at a random x~ its c~ reaches 1e8 and
    # differences lose every digit.  Its G~ does not pass there)
    ("config 5: Delta III 4 x 3125 x 5", lambda: problems.delta_iii(K=3125, order=5), None),
    ("refined Delta III (4 x 12500 nodes)", lambda: problems.with_refined_mesh(problems.delta_iii(), 12500, seeds=(7, 8, 9, 10)),
     None),
]


def _events_ms(stream, fn, reps):
    s = torch.cuda.ExternalStream(stream)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(s)
    for _ in range(reps):
        fn()
    b.record(s)
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    only = sys.argv[1:]
    print(f"{'config':40s} {'n':>8s} {'colours':>7s} {'evals':>5s} {'check ms':>9s} {'fused ms':>9s} {'ratio':>6s} "
          f"{'n+1 (computed)':>14s}  max err G / H / grad J  ok", flush=True)
    for label, make, rng_range in CONFIGS:
        if only and not any(o in label for o in only):
            continue
        rng = np.random.default_rng(0)
        if rng_range is None:
            it = MeshIteration(make())
            eng = it.engine
            x0 = it.guess_x_tilde + rng.uniform(-0.02, 0.02, eng.num_x)
            for pl in it.layout.phases:   # velocities off v_rel = 0, where the drag's |v_rel| has no derivative
                x0[pl.x_off + 3 * pl.N:pl.x_off + 6 * pl.N] += 0.1
        else:
            eng = NlpEngine(make(), device=0)
            x0 = rng.uniform(*rng_range, eng.num_x)
        x = torch.tensor(x0, dtype=torch.float64, device="cuda:0")
        lam = torch.tensor(rng.uniform(-1, 1, eng.num_c), dtype=torch.float64, device="cuda:0")
        c = torch.empty(eng.num_c, dtype=torch.float64, device="cuda:0")
        G = torch.empty(eng.nnz_jac, dtype=torch.float64, device="cuda:0")
        H = torch.empty(eng.nnz_hess, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        ev = eng.bind_device(x, lam, c, G, H, stream=eng.stream)
        for _ in range(5):
            ev()
        fused = _events_ms(eng.stream, ev, 50)
        out = {}

        delta = 1e-5 if rng_range is not None else 1e-7   # (Delta III: a scaled step of 1e-5 is about a kilometre of altitude)

        def check():
            out["r"] = eng.check_derivatives(x, 1.0, lam, delta=delta)

        check()   # (plan, scratch and the first launches)
        t = min(_events_ms(eng.stream, check, 1) for _ in range(3))
        r = out["r"]
        ratio = t / (r.n_evaluations * fused)
        print(f"{label:40s} {eng.num_x:8d} {r.n_colours:7d} {r.n_evaluations:5d} {t:9.3f} {fused:9.4f} {ratio:6.2f} "
              f"{eng.num_x + 1:14d}  {r.max_err_jac:.1e} / {r.max_err_hess:.1e} / {r.max_err_grad:.1e}  {r.ok}", flush=True)
        eng.close()


if __name__ == "__main__":
    main()
