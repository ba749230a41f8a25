"""Times of the forward propagation (``Solution.propagate`` / ``pc_solution_propagate_device``) at
BASELINE.json config 2 (hypersensitive 2000 x 6, 10 001 nodes): restart = "nodes", "sections" and "phase", each fixed
with 4 substeps and adaptive at rtol 1e-9, between HIP events on the handle's stream after a warm-up (a call stages its
segment list first, so the figure is the call, not the kernel alone); next to ``scipy.integrate.solve_ivp(method=
"RK45")`` restarted per node interval on the host under the same control interpolant (a host clock).  The point is
smooth with |y|, |u| <= 0.15 in unscaled variables, where the dynamics are as mild as along the problem's solution
(df/dy = -3 y^2).  One JSON line.

    python tools/solution_propagate_time.py  > profiles/propagate_time.txt"""
import json
import os
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
import numpy as np
import torch

from pycollo_amd import problems
from pycollo_amd.engine import NlpEngine
from pycollo_amd.solution import Solution, propagation_segments


def _events_ms(stream, fn, reps):
    s = torch.cuda.ExternalStream(stream)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(s)
    for _ in range(reps):
        fn()
    b.record(s)
    b.synchronize()
    return a.elapsed_time(b) / reps


def _host_rk45(sol, mesh, rtol, atol):
    """solve_ivp(RK45) over every node interval from the node's own state, u(c) by numpy's Legendre evaluation"""
    from numpy.polynomial.legendre import legval
    from scipy.integrate import solve_ivp
    uc = sol.coefficients(0)[1][0]
    stretch = 0.5 * (sol.final_time[0] - sol.initial_time[0])
    y, tau, nfev = sol.state[0][0], mesh.tau, 0
    out = np.empty(mesh.N)
    out[0] = y[0]
    for k in range(mesh.K):
        s, n = int(mesh.s[k]), int(mesh.n[k])
        ta = tau[s]
        w = tau[int(mesh.s[k + 1])] - ta
        cf, g = uc[s + k:s + k + n], stretch * 0.5 * w
        for j in range(s, int(mesh.s[k + 1])):
            ca, cb = 2.0 * (tau[j] - ta) / w - 1.0, 2.0 * (tau[j + 1] - ta) / w - 1.0
            r = solve_ivp(lambda c, v: g * (-v**3 + legval(c, cf)), (ca, cb), [y[j]], method="RK45", rtol=rtol, atol=atol)
            out[j + 1] = r.y[0, -1]
            nfev += r.nfev
    return out, nfev


def main():
    eng = NlpEngine(problems.hypersensitive(K=2000, order=6), device=0)
    mesh, pl = eng.meshes[0], eng.layout.phases[0]
    rng = np.random.default_rng(0)
    V, r = eng.layout.expand_x(eng.V_ocp), eng.layout.expand_x(eng.r_ocp)
    x = np.zeros(eng.num_x)
    for b in range(pl.n_z):
        sl = slice(pl.x_off + b * pl.N, pl.x_off + (b + 1) * pl.N)
        x[sl] = (np.polynomial.polynomial.polyval(mesh.tau, rng.uniform(-0.0375, 0.0375, 4)) - r[sl]) / V[sl]
    sol = Solution(eng, x)
    lib, h = sol._lib, sol._h
    N = pl.N
    y = torch.empty((pl.n_y, N), dtype=torch.float64, device="cuda:0")
    acc, rej = (torch.empty((N,), dtype=torch.int32, device="cuda:0") for _ in range(2))
    rtol = 1e-9
    atol = np.ascontiguousarray(rtol * sol.state_scale(0))
    rec = {"config": "config 2: hypersensitive 2000 x 6", "nodes": int(N), "sections": int(pl.K), "rtol": rtol}
    for restart in ("nodes", "sections", "phase"):
        seg = propagation_segments(restart, mesh.s, N)
        st = torch.empty((len(seg) - 1,), dtype=torch.int32, device="cuda:0")
        for label, m in (("fixed_m4", 4), ("adaptive", 0)):
            def call(seg=seg, st=st, m=m):
                if not lib.pc_solution_propagate_device(h, 0, len(seg) - 1, seg.ctypes.data, m, rtol, atol.ctypes.data, 4096,
                                                        y.data_ptr(), acc.data_ptr(), rej.data_ptr(), st.data_ptr()):
                    raise RuntimeError(lib.pc_last_error().decode())
            for _ in range(3):
                call()
            reps = 20 if restart != "phase" else 3
            key = f"{restart}_{label}"
            rec[key + "_call_ms"] = min(_events_ms(eng.stream, call, reps) for _ in range(3))
            torch.cuda.synchronize()
            rec[key + "_segments"] = int(len(seg) - 1)
            rec[key + "_steps"] = int(acc.sum().item()) + int(rej.sum().item())
            rec[key + "_complete"] = bool((st == -1).all().item())
            if restart == "nodes" and m == 0:
                gpu_nodes = y.cpu().numpy()[0].copy()
    t = time.perf_counter()
    host, nfev = _host_rk45(sol, mesh, rtol, float(atol[0]))
    rec["host_scipy_rk45_per_interval_ms"] = 1e3 * (time.perf_counter() - t)
    rec["host_scipy_rk45_f_evaluations"] = int(nfev)
    rec["nodes_adaptive_max_abs_difference_from_scipy"] = float(np.max(np.abs(host - gpu_nodes)))
    sol.close()
    eng.close()
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
