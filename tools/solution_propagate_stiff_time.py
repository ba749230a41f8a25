"""Times of the implicit propagation (``Solution.propagate(method="sdirk4")`` / ``pc_solution_propagate_stiff_device``;
DESIGN 8h) next to the explicit pair's under the same ``max_steps``, at BASELINE.json config 2 (hypersensitive
2000 x 6, 10 001 nodes) with the final time left at 10 000: restart = "nodes" and "sections", adaptive at rtol 1e-6,
between HIP events on the handle's stream after a warm-up (a call stages its segment list first, so the figure is the
call, not the kernel alone; the least of three windows).  Two points: ``mild``, the smooth point of
tools/solution_propagate_time.py (|y|, |u| <= 0.15 in unscaled variables, df/dy = -3 y^2 >= -0.07), and ``tests``, the
smooth point of the tests (drawn in scaled variables: |y| reaches 15 and df/dy -675).  Per method: ms per call, the
accepted, rejected and Newton totals, and how many segments complete.  One JSON line.

    python tools/solution_propagate_stiff_time.py  > profiles/propagate_stiff_time.txt"""
import json
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
import numpy as np
import torch

from pycollo_amd import problems
from pycollo_amd.engine import NlpEngine
from pycollo_amd.solution import Solution, propagation_segments

RTOL, MAX_STEPS, NEWTON_MAX = 1e-6, 4096, 8


def _events_ms(stream, fn, reps):
    s = torch.cuda.ExternalStream(stream)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(s)
    for _ in range(reps):
        fn()
    b.record(s)
    b.synchronize()
    return a.elapsed_time(b) / reps


def _point(eng, which):
    mesh, pl = eng.meshes[0], eng.layout.phases[0]
    V, r = eng.layout.expand_x(eng.V_ocp), eng.layout.expand_x(eng.r_ocp)
    x = np.zeros(eng.num_x)
    rng = np.random.default_rng(0 if which == "mild" else 5)
    for b in range(pl.n_z):
        sl = slice(pl.x_off + b * pl.N, pl.x_off + (b + 1) * pl.N)
        if which == "mild":
            x[sl] = (np.polynomial.polynomial.polyval(mesh.tau, rng.uniform(-0.0375, 0.0375, 4)) - r[sl]) / V[sl]
        else:
            x[sl] = np.polynomial.polynomial.polyval(mesh.tau, rng.uniform(-0.15, 0.15, 4))
    x[pl.q_off:pl.q_off + pl.n_q + pl.n_t] = 0.2
    return x


def main():
    eng = NlpEngine(problems.hypersensitive(K=2000, order=6), device=0)
    mesh, pl = eng.meshes[0], eng.layout.phases[0]
    N = pl.N
    y = torch.empty((pl.n_y, N), dtype=torch.float64, device="cuda:0")
    acc, rej, nrej, nit = (torch.empty((N,), dtype=torch.int32, device="cuda:0") for _ in range(4))
    rec = {"config": "config 2: hypersensitive 2000 x 6, final time 10000", "nodes": int(N), "sections": int(pl.K), "rtol": RTOL,
           "max_steps": MAX_STEPS, "newton_max": NEWTON_MAX}
    for which in ("mild", "tests"):
        sol = Solution(eng, _point(eng, which))
        lib, h = sol._lib, sol._h
        atol = np.ascontiguousarray(RTOL * sol.state_scale(0))
        rec[f"{which}_max_abs_y"] = float(np.max(np.abs(sol.state[0])))
        for restart in ("nodes", "sections"):
            seg = propagation_segments(restart, mesh.s, N)
            st = torch.empty((len(seg) - 1,), dtype=torch.int32, device="cuda:0")
            for method in ("sdirk4", "dopri5"):
                def call(seg=seg, st=st, method=method):
                    if method == "sdirk4":
                        ok = lib.pc_solution_propagate_stiff_device(h, 0, len(seg) - 1, seg.ctypes.data, 0, RTOL, atol.ctypes.data,
                                                                    MAX_STEPS, NEWTON_MAX, y.data_ptr(), acc.data_ptr(), rej.data_ptr(),
                                                                    st.data_ptr(), nrej.data_ptr(), nit.data_ptr())
                    else:
                        ok = lib.pc_solution_propagate_device(h, 0, len(seg) - 1, seg.ctypes.data, 0, RTOL, atol.ctypes.data, MAX_STEPS,
                                                              y.data_ptr(), acc.data_ptr(), rej.data_ptr(), st.data_ptr())
                    if not ok:
                        raise RuntimeError(lib.pc_last_error().decode())
                for _ in range(3):
                    call()
                key = f"{which}_{restart}_{method}"
                rec[key + "_call_ms"] = min(_events_ms(eng.stream, call, 10) for _ in range(3))
                torch.cuda.synchronize()
                rec[key + "_segments"] = int(len(seg) - 1)
                rec[key + "_complete"] = int((st == -1).sum().item())
                rec[key + "_accepted"] = int(acc.sum().item())
                rec[key + "_rejected"] = int(rej.sum().item())
                if method == "sdirk4":
                    rec[key + "_newton_rejected"] = int(nrej.sum().item())
                    rec[key + "_newton_iterations"] = int(nit.sum().item())
        sol.close()
    eng.close()
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
