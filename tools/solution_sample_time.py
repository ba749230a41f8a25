"""Times of the dense output (pycollo_amd/solution.py) at BASELINE.json configs 2 and 3: creating a Solution from a
device x (uploads, the fit kernel, the synchronise: a host clock around a call that ends in one), sampling 10^6 queries
(sorted and shuffled, with and without f) between HIP events on the handle's stream after a warm-up, next to the
reference's method restated on the host (the per-section NumPy ``fit`` loop of solution_abc.py:60-102) and to
``Mi355x._dy`` for the node derivatives (host clocks).  The bytes of a sampling call are what it must move: the
queries, the outputs, and the coefficient and start-value arrays once.  One JSON line per config.

    python tools/solution_sample_time.py [config-substring ...]  > profiles/r08_solution_sample_time.txt"""
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
from pycollo_amd.pycollo_backend import Mi355x
from pycollo_amd.solution import Solution

CONFIGS = [
    ("config 2: hypersensitive 2000 x 6", lambda: problems.hypersensitive(K=2000, order=6)),
    ("config 3: cart-pole 5000 x 4", lambda: problems.cart_pole(K=5000, order=4)),
]
Q = 1_000_000


def _events_ms(stream, fn, reps):
    s = torch.cuda.ExternalStream(stream)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(s)
    for _ in range(reps):
        fn()
    b.record(s)
    b.synchronize()
    return a.elapsed_time(b) / reps


def _reference_fit_loop(tau, s, n, y, dy, u, stretch):
    """solution_abc.py:60-102 on the host: K (2 n_y + n_u) NumPy fits"""
    for k in range(len(n)):
        i0, i1 = int(s[k]), int(s[k + 1])
        t_k = tau[i0:i1 + 1]
        for a in range(y.shape[0]):
            np.polynomial.Legendre.fit(t_k, dy[a, i0:i1 + 1], deg=n[k] - 1, window=[0, 1])
            np.polynomial.Legendre.fit(t_k, dy[a, i0:i1 + 1] * stretch, deg=n[k] - 1, window=[0, 1]).integ(k=y[a, i0])
        for b in range(u.shape[0]):
            np.polynomial.Polynomial.fit(t_k, u[b, i0:i1 + 1], deg=n[k] - 1, window=[0, 1])


def main():
    only = sys.argv[1:]
    for label, make in CONFIGS:
        if only and not any(o in label for o in only):
            continue
        eng = NlpEngine(make(), device=0)
        mesh, pl = eng.meshes[0], eng.layout.phases[0]
        rng = np.random.default_rng(0)
        x = np.zeros(eng.num_x)
        for b in range(pl.n_z):
            x[pl.x_off + b * pl.N:pl.x_off + (b + 1) * pl.N] = np.polynomial.polynomial.polyval(mesh.tau, rng.uniform(-0.15, 0.15, 4))
        x[pl.q_off:pl.q_off + pl.n_q + pl.n_t] = rng.uniform(0.1, 0.3, pl.n_q + pl.n_t)
        d_x = torch.tensor(x, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        Solution(eng, d_x).close()   # (code object functions resolved, tables cached)
        create = []
        for _ in range(5):
            t = time.perf_counter()
            sol = Solution(eng, d_x)
            create.append(1e3 * (time.perf_counter() - t))
            sol.close()
        sol = Solution(eng, d_x)
        lib, h = sol._lib, sol._h
        tau_sorted = torch.linspace(-1.0, 1.0, Q, dtype=torch.float64, device="cuda:0")
        tau_shuffled = tau_sorted[torch.randperm(Q, device="cuda:0", generator=torch.Generator("cuda:0").manual_seed(0))].contiguous()
        out = [torch.empty((max(r, 1), Q), dtype=torch.float64, device="cuda:0") for r in (pl.n_y, pl.n_y, pl.n_u, pl.n_y)]
        torch.cuda.synchronize()
        rec = {"config": label, "nodes": int(pl.N), "sections": int(pl.K), "n_y": pl.n_y, "n_u": pl.n_u, "queries": Q,
               "create_from_device_x_ms_min_of_5": min(create), "create_from_device_x_ms_all": create}
        fixed = 8 * ((pl.N + pl.K - 1) * (pl.n_y + pl.n_u) + pl.N * pl.n_y)
        for order, tq in (("sorted", tau_sorted), ("shuffled", tau_shuffled)):
            for with_f in (False, True):
                def call(tq=tq, with_f=with_f):
                    if not lib.pc_solution_sample_device(h, 0, tq.data_ptr(), Q, 1, out[0].data_ptr(), out[1].data_ptr(),
                                                         out[2].data_ptr() if pl.n_u else None, out[3].data_ptr() if with_f else None):
                        raise RuntimeError(lib.pc_last_error().decode())
                for _ in range(5):
                    call()
                ms = min(_events_ms(eng.stream, call, 50) for _ in range(3))
                nbytes = 8 * Q * (1 + 2 * pl.n_y + pl.n_u + (pl.n_y if with_f else 0)) + fixed
                key = f"sample_{order}{'_with_f' if with_f else ''}"
                rec[key + "_ms"] = ms
                rec[key + "_bytes"] = nbytes
                rec[key + "_GB_per_s"] = nbytes / (ms * 1e-3) / 1e9
        # the host methods it replaces
        stretch = 0.5 * (sol.final_time[0] - sol.initial_time[0])
        t = time.perf_counter()
        _reference_fit_loop(mesh.tau, mesh.s, mesh.n, sol.state[0], sol.state_derivative[0],
                            sol.control[0] if pl.n_u else np.empty((0, pl.N)), stretch)
        rec["host_numpy_fit_loop_ms"] = 1e3 * (time.perf_counter() - t)
        b = Mi355x(device=0)
        b.engine = eng
        b._dy(x)        # (lambdify once)
        t = time.perf_counter()
        b._dy(x)
        rec["host_dy_callable_ms"] = 1e3 * (time.perf_counter() - t)
        b.engine = None
        sol.close()
        eng.close()
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
