"""Time of the ph mesh-error estimate (``pc_mesh_error``: uploads, the kernel, the synchronise, the copies back) at
BASELINE.json config 2 (hypersensitive 2000 x 6): a host clock around the call, which ends in a synchronise; after ten
warm-up calls the median and minimum of 200.  One JSON line.

    python tools/mesh_error_time.py"""
import json
import os
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _R)
import numpy as np

from pycollo_amd import problems
from pycollo_amd.engine import NlpEngine
from pycollo_amd.refinement import ph_tables

eng = NlpEngine(problems.hypersensitive(K=2000, order=6), device=0)
mesh, pl = eng.meshes[0], eng.layout.phases[0]
rng = np.random.default_rng(0)
x = np.zeros(eng.num_x)
for b in range(pl.n_z):
    x[pl.x_off + b * pl.N:pl.x_off + (b + 1) * pl.N] = np.polynomial.polynomial.polyval(mesh.tau, rng.uniform(-0.15, 0.15, 4))
orders = sorted({int(n) for n in np.unique(mesh.n)})
tabs = [ph_tables(eng.quad, n) for n in orders]
B, E, A = (np.concatenate([t[i].ravel() for t in tabs]) for i in range(3))
for _ in range(10):
    eng.mesh_error(0, x, orders, B, E, A)
ms = []
for _ in range(200):
    t = time.perf_counter()
    eng.mesh_error(0, x, orders, B, E, A)
    ms.append(1e3 * (time.perf_counter() - t))
print(json.dumps({"config": "config 2: hypersensitive 2000 x 6", "mesh_error_call_ms_median_of_200": float(np.median(ms)),
                  "mesh_error_call_ms_min": float(np.min(ms))}), flush=True)
eng.close()
