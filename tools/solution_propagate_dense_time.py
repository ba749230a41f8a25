"""Times of the propagation with integrals and dense output (``Solution.propagate_dense`` /
``pc_solution_propagate_dense_device``) at BASELINE.json config 2 (hypersensitive 2000 x 6, 10 001 nodes):
restart = "nodes", "sections" and "phase", adaptive at rtol 1e-9 without ``integral_atol``, with Q = 0 and Q = 10 N
queries (equispaced in tau), between HIP events on the handle's stream after a warm-up, the least of three windows (a
call sorts and stages its queries first, so the figure is the call, not the kernel alone).  Next to every figure:
``pc_solution_propagate_device`` for the same arguments in the same run -- the kernel this one shares its steps with,
which this change leaves as it was.  The point is tools/solution_propagate_time.py's.  One JSON line.

    python tools/solution_propagate_dense_time.py  > profiles/propagate_dense_time.txt"""
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
    N, dev = pl.N, "cuda:0"
    new = lambda sh, dt=torch.float64: torch.empty(sh, dtype=dt, device=dev)   # noqa: E731
    y, qa = new((pl.n_y, N)), new((pl.n_q, N))
    acc, rej = new((N,), torch.int32), new((N,), torch.int32)
    rtol = 1e-9
    atol = np.ascontiguousarray(rtol * sol.state_scale(0))
    rec = {"config": "config 2: hypersensitive 2000 x 6", "nodes": int(N), "sections": int(pl.K), "rtol": rtol, "mode": "adaptive"}
    for restart in ("nodes", "sections", "phase"):
        seg = propagation_segments(restart, mesh.s, N)
        st = new((len(seg) - 1,), torch.int32)
        reps = 20 if restart != "phase" else 3

        def plain(seg=seg, st=st):
            if not lib.pc_solution_propagate_device(h, 0, len(seg) - 1, seg.ctypes.data, 0, rtol, atol.ctypes.data, 4096,
                                                    y.data_ptr(), acc.data_ptr(), rej.data_ptr(), st.data_ptr()):
                raise RuntimeError(lib.pc_last_error().decode())
        for _ in range(3):
            plain()
        rec[f"{restart}_propagate_call_ms"] = min(_events_ms(eng.stream, plain, reps) for _ in range(3))
        torch.cuda.synchronize()
        rec[f"{restart}_steps"] = int(acc.sum().item()) + int(rej.sum().item())
        for Q in (0, 10 * N):
            tq = np.ascontiguousarray(np.linspace(-1.0, 1.0, Q)) if Q else np.zeros(0)
            yd, qd = new((pl.n_y, Q)), new((pl.n_q, Q))

            def dense(seg=seg, st=st, tq=tq, yd=yd, qd=qd, Q=Q):
                if not lib.pc_solution_propagate_dense_device(h, 0, len(seg) - 1, seg.ctypes.data, 0, rtol, atol.ctypes.data, None,
                                                              4096, Q, tq.ctypes.data if Q else None, y.data_ptr(), acc.data_ptr(),
                                                              rej.data_ptr(), st.data_ptr(), qa.data_ptr(),
                                                              yd.data_ptr() if Q else None, qd.data_ptr() if Q else None):
                    raise RuntimeError(lib.pc_last_error().decode())
            for _ in range(3):
                dense()
            key = f"{restart}_dense_Q{'0' if Q == 0 else '10N'}"
            rec[key + "_call_ms"] = min(_events_ms(eng.stream, dense, reps) for _ in range(3))
            torch.cuda.synchronize()
            rec[key + "_steps"] = int(acc.sum().item()) + int(rej.sum().item())
            rec[key + "_complete"] = bool((st == -1).all().item())
            if Q:
                rec[key + "_all_finite"] = bool(torch.isfinite(yd).all().item() and torch.isfinite(qd).all().item())
    sol.close()
    eng.close()
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
