"""The host index arithmetic of the multiplier kernels (pycollo_amd/csrc/pc_optimality_plan.hpp) under AddressSanitizer +
UBSan (CPU only).

``tests/c/optimality_plan_sanitize.cpp`` is a stand-alone program: it compiles the header with ``g++
-fsanitize=address,undefined -fno-sanitize-recover=all``, builds the plan of every mesh it is fed, walks every multiplier
row, x column, weight-row entry, table entry, staged slot and coefficient slot a lane of ``pc_sol_multipliers`` would
touch with bounds-checked accesses, checks that every output slot (mu, zeta, H_z at the nodes, the endpoint
multipliers, both coefficient arrays) is written exactly once, and prints the offsets; here they are compared with a
NumPy restatement.  Meshes: those of test_solution_plan_sanitize.py, and n_p = 0, n_u = 0, a one-section mesh, an
all-order-2 mesh, orders 2 and 20 adjacent and a refused LDS size.  Nothing is loaded into Python under a sanitizer."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_solution_plan_sanitize import _cases as _solution_cases

SRC = os.path.join(ROOT, "tests", "c", "optimality_plan_sanitize.cpp")
EXE = os.path.join(ROOT, "tests", "_build", "optimality_plan_sanitize")
HEADERS = ("pc_optimality_plan.hpp", "pc_costate_plan.hpp", "pc_solution_plan.hpp", "pc_args.h")


@pytest.fixture(scope="module")
def harness():
    deps = [SRC] + [os.path.join(ROOT, "pycollo_amd", "csrc", f) for f in HEADERS]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        os.makedirs(os.path.dirname(EXE), exist_ok=True)
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
               "-fno-omit-frame-pointer", "-o", EXE + f".tmp{os.getpid()}", SRC]
        res = subprocess.run(cmd, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-3000:]
        os.replace(EXE + f".tmp{os.getpid()}", EXE)
    return EXE


def _lds(orders, TB, NP, NZ):
    """the multiplier kernel's LDS: the C_u and ydot tables, the weight rows, one staged value per lane and multiplier
    function, TB tags"""
    return 8 * (2 * sum(n * n for n in orders) + sum(orders) + max(NP + NZ, 1) * TB) + 4 * TB


def _valid(n_k, TB, orders):
    """what the fit plan and the table offsets accept"""
    return (len(n_k) >= 1 and 20 <= TB <= 1024 and len(set(orders)) == len(orders) and all(2 <= n <= 20 for n in orders)
            and all(2 <= n <= 20 and n in orders for n in n_k))


def rng_mesh(seed, K):
    return np.random.default_rng(seed).integers(2, 21, K)


def _cases():
    """(n_k, TB, NY, NU, NQ, NP, c_off, x_off, lds_limit, orders).  The fit kernel's LDS limit is not applied (0 is passed
    to its plan): the limit here is the multiplier kernel's own."""
    out = []
    for i, (n_k, TB, NY, NU, lim, orders, _) in enumerate(_solution_cases()):
        out.append((n_k, TB, NY, NU, i % 3, i % 2, 7 * i, 3 * i, lim, orders))
    every = list(range(2, 21))
    out += [
        (np.full(5, 4), 256, 2, 1, 1, 0, 0, 0, 65536, [4]),                  # n_p = 0
        (np.full(5, 4), 256, 2, 0, 1, 2, 3, 9, 65536, [4]),                  # n_u = 0
        (np.full(5, 4), 256, 0, 0, 0, 0, 0, 0, 65536, [4]),                  # nothing to stage: one slot per lane is kept
        (np.array([4]), 256, 1, 1, 1, 1, 0, 0, 65536, [4]),                  # one section: it is the last, formed with the ydot table
        (np.array([2]), 256, 2, 1, 0, 0, 5, 2, 65536, [2]),                  # ... of two nodes: both are end nodes
        (np.full(7, 2), 256, 1, 1, 1, 1, 0, 0, 65536, [2]),                  # all order 2: every interior node is shared
        (np.full(300, 2), 256, 3, 1, 2, 1, 11, 4, 65536, [2]),               # ... over three workgroups
        (np.array([2, 20, 2, 20, 20, 2]), 256, 2, 1, 1, 1, 0, 0, 65536, [2, 20]),   # orders 2 and 20 adjacent
        (np.array([20, 20] + [2] * 108 + [20, 20]), 256, 1, 1, 0, 1, 0, 0, 65536, [2, 20]),
        (rng_mesh(9, 50), 256, 4, 2, 1, 1, 0, 0, 65536, every),              # every table, 7 functions: 62 936 B
        (rng_mesh(9, 50), 256, 4, 2, 1, 3, 0, 0, 65536, every),              # ... 9 functions: 67 032 B, refused
        (np.full(5, 4), 256, 0, 1, 1, 1, -1, 0, 65536, [4]),                 # negative row offset (no defect rows before the path rows)
        (np.full(5, 4), 256, 2, 1, 1, 1, 0, -2, 65536, [4]),                 # negative column offset
    ]
    return out


def _accepted(n_k, TB, NY, NU, NP, c_off, x_off, lim, orders):
    if not _valid(n_k, TB, orders) or c_off + NY * (int(np.sum(np.asarray(n_k) - 1))) < 0 or x_off < 0:
        return False
    return lim <= 0 or _lds(orders, TB, NP, NY + NU) <= lim


def _restate(n_k, TB, NY, NU, NP, c_off, x_off, orders):
    n_k = np.asarray(n_k, dtype=np.int64)
    K = len(n_k)
    N = int(np.sum(n_k - 1)) + 1
    n_tiles, lanes = 1, 0
    for k in range(K):
        if lanes + n_k[k] > TB:
            n_tiles += 1
            lanes = 0
        lanes += int(n_k[k])
    offW = np.full(21, -1)
    o = 0
    for n in orders:
        offW[n] = o
        o += n
    return dict(N=N, NC=N + K - 1, n_tiles=n_tiles, w_total=o, lds=_lds(orders, TB, NP, NY + NU), offW=offW,
                path_off=c_off + NY * (N - 1) + N * np.arange(NP), x_col=x_off + N * np.arange(NY + NU))


def test_optimality_plan_under_asan_ubsan(harness, tmp_path):
    cases = _cases()
    fin, fout = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    with open(fin, "w") as f:
        f.write(f"{len(cases)}\n")
        for n_k, TB, NY, NU, NQ, NP, c_off, x_off, lim, orders in cases:
            f.write(f"{len(n_k)} {TB} {NY} {NU} {NQ} {NP} {c_off} {x_off} {lim} {len(orders)}\n")
            f.write(" ".join(str(int(v)) for v in orders) + "\n")
            f.write(" ".join(str(int(v)) for v in n_k) + "\n")
    res = subprocess.run([harness, fin, fout], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-3000:]
    lines = open(fout).read().splitlines()
    assert lines[-1] == "ok" and lines[-2] == "refused 10"
    it = iter(lines[:-2])
    n_ok = n_refused = 0
    for c, (n_k, TB, NY, NU, NQ, NP, c_off, x_off, lim, orders) in enumerate(cases):
        head = next(it).split()
        assert head[:2] == ["case", str(c)]
        accepted = _accepted(n_k, TB, NY, NU, NP, c_off, x_off, lim, orders)
        assert (head[2] == "ok") == accepted, (c, head)
        if not accepted:
            n_refused += 1
            continue
        n_ok += 1
        ref = _restate(n_k, TB, NY, NU, NP, c_off, x_off, orders)
        assert [int(v) for v in head[3:]] == [ref["N"], ref["NC"], ref["n_tiles"], ref["w_total"], ref["lds"]], (c, head)
        for name in ("offW", "path_off", "x_col"):
            p = next(it).split()
            assert p[0] == name and int(p[1]) == len(ref[name])
            np.testing.assert_array_equal(np.array([int(v) for v in p[2:]], dtype=np.int64), ref[name], err_msg=f"case {c}: {name}")
    assert n_ok >= 20 and n_refused >= 10
    # the refused LDS size is refused for its size alone: the same mesh with two functions fewer is accepted
    assert _lds(list(range(2, 21)), 256, 1, 6) == 62936 <= 65536 < 67032 == _lds(list(range(2, 21)), 256, 3, 6)
