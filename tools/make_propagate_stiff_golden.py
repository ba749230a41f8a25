"""Generator of tests/golden/propagate_stiff_headline.npz: the 60-digit truth of the implicit propagation's headline case
(DESIGN 8h), hypersensitive (K = 5, order 4) at its own final time of 10 000 and the tests' smooth point, restarted at
every node and at every section start.

The truth is the method's own fixed mode in mpmath (tests/propagate_stiff_ref.py ``ExactFixed``: every stage equation
solved to 1e-40), with m doubled from 64 until no arrival moves by 1e-3 (atol + rtol |y|) at rtol 1e-6, atol = rtol V.
The m it took is stored.  The phase is stiff (h |df/dy| ~ 4e5 over a node interval), the method's order drops towards 1
there and m = 512 is what it took: minutes of mpmath, which is why the arrivals are a fixture and
tests/test_propagate_stiff_ref_cpu.py recomputes one segment only.  CPU only.

    python tools/make_propagate_stiff_golden.py
"""
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "tests")]
import numpy as np

import propagate_ref as pr
import propagate_stiff_ref as ps
from conftest import golden_tables
from oracle.ref_numpy import OracleNlp
from pycollo_amd import problems

RTOL = 1e-6
OUT = os.path.join(_R, "tests", "golden", "propagate_stiff_headline.npz")


def main():
    prob = problems.hypersensitive(K=5, order=4)
    ora = OracleNlp(prob, golden_tables("lobatto"))
    d = pr.PhaseData.from_oracle(ora, 0, pr.smooth_x_oracle(ora), "lobatto")
    atol = RTOL * np.asarray(ora.V_ocp[ora.P[0].ox:ora.P[0].ox + d.n_y], dtype=np.float64)
    ex = ps.ExactFixed(d)
    rec = dict(rtol=RTOL, atol=atol, node_y=d.node_y, coef_u=d.coef_u, tau=d.tau)
    for restart in ("nodes", "sections"):
        seg = pr.segments(restart, d.s, d.N)
        m, prev = 64, ex.arrivals(seg, 64)[0]
        while True:
            m *= 2
            y = ex.arrivals(seg, m)[0]
            moved = float(np.max(np.abs(y - prev) / (atol[:, None] + RTOL * np.abs(y))))
            print(f"{restart}: m = {m} moves the arrivals by {moved:.3e} (atol + rtol |y|)", flush=True)
            prev = y
            if moved <= 1e-3:
                break
        rec[f"y_{restart}"], rec[f"m_{restart}"], rec[f"moved_{restart}"] = y, m, moved
    np.savez(OUT, **rec)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
