"""The host index arithmetic of the costate kernel (pycollo_amd/csrc/pc_costate_plan.hpp) under AddressSanitizer + UBSan
(CPU only).

``tests/c/costate_plan_sanitize.cpp`` is a stand-alone program: it compiles the header with ``g++
-fsanitize=address,undefined -fno-sanitize-recover=all``, builds the plan of every mesh it is fed (the meshes of
test_solution_plan_sanitize.py, a one-section mesh and an all-order-2 mesh), walks every multiplier row, A entry,
staged row and coefficient slot a lane of ``pc_sol_costate`` would touch with bounds-checked accesses, and prints the
offsets; here they are compared with a NumPy restatement."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_solution_plan_sanitize import _cases as _solution_cases

SRC = os.path.join(ROOT, "tests", "c", "costate_plan_sanitize.cpp")
EXE = os.path.join(ROOT, "tests", "_build", "costate_plan_sanitize")


@pytest.fixture(scope="module")
def harness():
    deps = [SRC] + [os.path.join(ROOT, "pycollo_amd", "csrc", f) for f in ("pc_costate_plan.hpp", "pc_solution_plan.hpp", "pc_args.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        os.makedirs(os.path.dirname(EXE), exist_ok=True)
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
               "-fno-omit-frame-pointer", "-o", EXE + f".tmp{os.getpid()}", SRC]
        res = subprocess.run(cmd, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-3000:]
        os.replace(EXE + f".tmp{os.getpid()}", EXE)
    return EXE


def _lds(orders, TB, NY):
    """the costate kernel's LDS: C_u and A tables, per state TB + 40 staged multiplier rows and TB costates, TB tags"""
    return 8 * (sum(n * n for n in orders) + sum((n - 1) * n for n in orders) + max(NY, 1) * (2 * TB + 40)) + 4 * TB


def _cases():
    """(n_k, TB, NY, NU, NQ, NP, c_off, lds_limit, orders, accepted).  The fit kernel's LDS limit is not applied (0 is
    passed to its plan): the limit here is the costate kernel's own, which accepts and refuses the same meshes of that
    list (every table with 4 + 2 variables: 62 920 B; with 8 + 4: 80 584 B)."""
    out = []
    for i, (n_k, TB, NY, NU, lim, orders, ok) in enumerate(_solution_cases()):
        out.append((n_k, TB, NY, NU, i % 3, i % 2, 7 * i, lim, orders, ok))
    out += [
        (np.array([4]), 256, 1, 1, 1, 0, 0, 65536, [4], True),               # one section: no neighbour on either side
        (np.array([2]), 256, 2, 1, 0, 0, 5, 65536, [2], True),               # ... of two nodes: one defect row
        (np.full(7, 2), 256, 1, 1, 1, 0, 0, 65536, [2], True),               # all order 2: every interior node is shared
        (np.full(300, 2), 256, 3, 1, 2, 1, 11, 65536, [2], True),            # ... over three workgroups
        (np.array([20, 20] + [2] * 108 + [20, 20]), 256, 1, 1, 0, 0, 0, 65536, [2, 20], True),   # widest neighbours next to full tiles
        (rng_mesh(9, 50), 256, 4, 2, 1, 0, 0, 65536, list(range(2, 21)), True),       # every table: 62 920 B
        (rng_mesh(9, 50), 256, 5, 2, 1, 0, 0, 65536, list(range(2, 21)), False),      # ... 67 336 B with a fifth state
        (np.full(5, 4), 256, 2, 1, 1, 0, -1, 65536, [4], False),             # negative row offset
    ]
    return out


def rng_mesh(seed, K):
    return np.random.default_rng(seed).integers(2, 21, K)


def _restate(n_k, TB, NY, NQ, NP, c_off, orders):
    n_k = np.asarray(n_k, dtype=np.int64)
    K = len(n_k)
    sec_s = np.concatenate(([0], np.cumsum(n_k - 1)))
    N = int(sec_s[-1]) + 1
    tile_k0, lanes = [0], 0
    for k in range(K):
        if lanes + n_k[k] > TB:
            tile_k0.append(k)
            lanes = 0
        lanes += int(n_k[k])
    tile_k0.append(K)
    offA = np.full(21, -1)
    o = 0
    for n in orders:
        offA[n] = o
        o += (n - 1) * n
    row_lo = [int(sec_s[max(k0 - 1, 0)]) for k0 in tile_k0[:-1]]
    row_hi = [int(sec_s[min(k1 + 1, K)]) for k1 in tile_k0[1:]]
    return dict(N=N, NC=N + K - 1, n_tiles=len(tile_k0) - 1, a_total=o, lds=_lds(orders, TB, NY),
                lam_int_off=c_off + NY * (N - 1) + NP * N, offA=offA, lam_off=c_off + (N - 1) * np.arange(NY),
                row_lo=np.array(row_lo), row_hi=np.array(row_hi))


def test_costate_plan_under_asan_ubsan(harness, tmp_path):
    cases = _cases()
    fin, fout = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    with open(fin, "w") as f:
        f.write(f"{len(cases)}\n")
        for n_k, TB, NY, NU, NQ, NP, c_off, lim, orders, _ in cases:
            f.write(f"{len(n_k)} {TB} {NY} {NU} {NQ} {NP} {c_off} {lim} {len(orders)}\n")
            f.write(" ".join(str(int(v)) for v in orders) + "\n")
            f.write(" ".join(str(int(v)) for v in n_k) + "\n")
    res = subprocess.run([harness, fin, fout], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-3000:]
    lines = open(fout).read().splitlines()
    assert lines[-1] == "ok" and lines[-2] == "refused 6"
    it = iter(lines[:-2])
    n_ok = 0
    for c, (n_k, TB, NY, NU, NQ, NP, c_off, lim, orders, accepted) in enumerate(cases):
        head = next(it).split()
        assert head[:2] == ["case", str(c)]
        assert (head[2] == "ok") == accepted, (c, head)
        if not accepted:
            continue
        n_ok += 1
        ref = _restate(n_k, TB, NY, NQ, NP, c_off, orders)
        assert [int(v) for v in head[3:]] == [ref["N"], ref["NC"], ref["n_tiles"], ref["a_total"], ref["lds"], ref["lam_int_off"]]
        for name in ("offA", "lam_off", "row_lo", "row_hi"):
            p = next(it).split()
            assert p[0] == name and int(p[1]) == len(ref[name])
            np.testing.assert_array_equal(np.array([int(v) for v in p[2:]]), ref[name], err_msg=f"case {c}: {name}")
        assert np.all(ref["row_hi"] - ref["row_lo"] <= TB + 40)
    assert n_ok >= 14
