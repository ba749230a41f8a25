"""The host index arithmetic of the dense output and of the mesh-error estimate (pycollo_amd/csrc/pc_solution_plan.hpp)
under AddressSanitizer + UBSan (CPU only).

``tests/c/solution_plan_sanitize.cpp`` compiles the header with ``g++ -fsanitize=address,undefined
-fno-sanitize-recover=all``, builds the fit plan and the mesh-error plan of every mesh it is fed, walks every lane,
node, coefficient slot and table row the kernels would touch with bounds-checked accesses, and prints the plans; here
they are compared with a NumPy restatement."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "c", "solution_plan_sanitize.cpp")
EXE = os.path.join(ROOT, "tests", "_build", "solution_plan_sanitize")


@pytest.fixture(scope="module")
def harness():
    deps = [SRC] + [os.path.join(ROOT, "pycollo_amd", "csrc", f) for f in ("pc_solution_plan.hpp", "pc_args.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        os.makedirs(os.path.dirname(EXE), exist_ok=True)
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
               "-fno-omit-frame-pointer", "-o", EXE + f".tmp{os.getpid()}", SRC]
        res = subprocess.run(cmd, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-3000:]
        os.replace(EXE + f".tmp{os.getpid()}", EXE)
    return EXE


def _cases():
    rng = np.random.default_rng(11)
    every = list(range(2, 21))
    out = [
        # (n_k, TB, NY, NU, lds_limit, orders, accepted)
        (np.full(5, 4), 256, 2, 1, 65536, [4], True),                       # below one wave
        (rng.integers(3, 9, 23), 256, 4, 1, 65536, list(range(3, 9)), True),   # ragged
        (rng.integers(3, 9, 60), 256, 4, 1, 65536, list(range(3, 9)), True),   # more than one workgroup
        (np.array([2, 20, 2, 20, 20]), 256, 1, 1, 65536, [2, 20], True),      # order extremes
        (np.full(64, 4), 256, 1, 0, 65536, [4], True),                        # a tile filled to the last lane
        (np.full(13, 20), 256, 1, 1, 65536, [20], True),                      # 12 sections fill 240 lanes, the 13th starts a tile
        (rng.integers(2, 21, 400), 64, 3, 2, 0, every, True),                 # small workgroup, every order, no LDS limit
        (np.array([20]), 20, 1, 1, 65536, [20], True),                        # one section = one tile exactly
        (rng.integers(2, 21, 50), 256, 4, 2, 65536, every, True),             # every table at once: 45 904 + 12 288 + 1 024 B
        (rng.integers(2, 21, 50), 256, 8, 4, 65536, every, False),            # ... which no longer fits with 12 variables
        (np.array([4, 5, 4]), 256, 1, 1, 65536, [4], False),                  # an order without a table
        (np.array([4, 1, 4]), 256, 1, 1, 65536, [4], False),                  # order below 2
        (np.array([4, 21]), 256, 1, 1, 65536, [4], False),                    # order above 20
        (np.array([4, 4]), 256, 1, 1, 65536, [4, 4], False),                  # an order listed twice
        (np.array([4, 4]), 256, 1, 1, 65536, [4, 21], False),                 # a table for an impossible order
        (np.array([4, 4]), 16, 1, 1, 65536, [4], False),                      # workgroup smaller than a section can be
        (np.array([], dtype=int), 256, 1, 1, 65536, [4], False),              # no section
        # the mesh-error kernel gives a section n_k + 1 lanes and has tables for orders 2 .. 19
        (np.array([19]), 256, 1, 1, 65536, [19], True),                       # a single section of its highest order
        (np.array([2]), 256, 1, 0, 65536, [2], True),                         # ... and of its lowest
        (np.full(64, 3), 256, 2, 1, 65536, [3], True),                        # 64 x 4 ph nodes fill 256 lanes to the last
        (np.full(65, 3), 256, 2, 1, 65536, [3], True),                        # ... and one section more starts a tile
        (rng.integers(2, 20, 400), 64, 3, 2, 0, list(range(2, 20)), True),    # small workgroup, every order it has, no LDS limit
        (rng.integers(2, 20, 50), 256, 1, 1, 65536, list(range(2, 20)), True),   # every table: fits the fit kernel, not this one
    ]
    return out


def _restate(n_k, TB, NY, NU, orders):
    n_k = np.asarray(n_k, dtype=np.int64)
    K = len(n_k)
    sec_s = np.concatenate(([0], np.cumsum(n_k - 1)))
    tile_k0, lane0, lanes = [0], [], 0
    for k in range(K):
        if lanes + n_k[k] > TB:
            tile_k0.append(k)
            lanes = 0
        lane0.append(lanes)
        lanes += int(n_k[k])
    tile_k0.append(K)
    offC = np.full(21, -1)
    o = 0
    for n in orders:
        offC[n] = o
        o += n * n
    N = int(sec_s[-1]) + 1
    lds = 8 * (2 * o + TB * (max(NY, 1) + max(NU, 1))) + 4 * TB
    return dict(N=N, NC=N + K - 1, n_tiles=len(tile_k0) - 1, tab_total=o, lds=lds, tile_k0=np.array(tile_k0),
                lane0=np.array(lane0), sec_s=sec_s, coef_off=sec_s + np.arange(K + 1), offC=offC)


def _restate_mesh_error(n_k, TB, NY, NU, lim, orders):
    """The refusal's text where pc_mesh_error refuses: no section, a listed order outside [2, 19], an order in use
    without a table, LDS"""
    n_k = np.asarray(n_k, dtype=np.int64)
    if len(n_k) == 0:
        return "mesh-error kernel: a phase needs at least one section"
    if any(not 2 <= n <= 19 for n in orders):
        return "mesh-error tables: order outside [2, 19]"
    if any(int(n) not in orders for n in n_k):
        return "mesh-error tables: an order in use has no table"
    offBE, offA = np.full(21, -1), np.full(21, -1)
    oBE = oA = 0
    for n in orders:
        offBE[n], offA[n] = oBE, oA
        oBE += (n - 1) * n
        oA += n * (n + 1)
    tile_k0, lane0, lanes = [0], [], 0
    for k in range(len(n_k)):
        if lanes + n_k[k] + 1 > TB:
            tile_k0.append(k)
            lanes = 0
        lane0.append(lanes)
        lanes += int(n_k[k]) + 1
    tile_k0.append(len(n_k))
    lds = 8 * (2 * oBE + oA + TB * (5 * NY + max(NU, 1) + 1)) + 4 * TB
    if lim > 0 and lds > lim:
        return "mesh-error kernel: tables do not fit in LDS"
    return dict(head=[len(tile_k0) - 1, oBE, oA, lds], tile_k0=np.array(tile_k0), lane0=np.array(lane0, dtype=np.int64),
                offBE=offBE, offA=offA)


def _check_mesh_error(it, c, case):
    n_k, TB, NY, NU, lim, orders, _ = case
    ref = _restate_mesh_error(n_k, TB, NY, NU, lim, orders)
    head = next(it).split()
    assert head[:2] == ["mesh_error", str(c)]
    if isinstance(ref, str):
        assert " ".join(head[2:]) == "refused " + ref, (c, head)
        return 0
    assert head[2] == "ok", (c, head)
    assert [int(v) for v in head[3:]] == ref["head"], (c, head)
    for name in ("tile_k0", "lane0", "offBE", "offA"):
        p = next(it).split()
        assert p[0] == name and int(p[1]) == len(ref[name])
        np.testing.assert_array_equal(np.array([int(v) for v in p[2:]]), ref[name], err_msg=f"mesh error, case {c}: {name}")
    return 1


def test_solution_plan_under_asan_ubsan(harness, tmp_path):
    cases = _cases()
    fin, fout = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    with open(fin, "w") as f:
        f.write(f"{len(cases)}\n")
        for n_k, TB, NY, NU, lim, orders, _ in cases:
            f.write(f"{len(n_k)} {TB} {NY} {NU} {lim} {len(orders)}\n")
            f.write(" ".join(str(int(v)) for v in orders) + "\n")
            f.write(" ".join(str(int(v)) for v in n_k) + "\n")
    res = subprocess.run([harness, fin, fout], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-3000:]
    lines = open(fout).read().splitlines()
    assert lines[-1] == "ok" and lines[-2] == "refused 6"
    it = iter(lines[:-2])
    mesh_error_plans = 0
    for c, (n_k, TB, NY, NU, lim, orders, accepted) in enumerate(cases):
        head = next(it).split()
        assert head[:2] == ["case", str(c)]
        assert (head[2] == "ok") == accepted, (c, head)
        if not accepted:
            mesh_error_plans += _check_mesh_error(it, c, cases[c])
            continue
        ref = _restate(n_k, TB, NY, NU, orders)
        assert [int(v) for v in head[3:]] == [ref["N"], ref["NC"], ref["n_tiles"], ref["tab_total"], ref["lds"]]
        for name in ("tile_k0", "lane0", "sec_s", "coef_off", "offC"):
            p = next(it).split()
            assert p[0] == name and int(p[1]) == len(ref[name])
            np.testing.assert_array_equal(np.array([int(v) for v in p[2:]]), ref[name], err_msg=f"case {c}: {name}")
        mesh_error_plans += _check_mesh_error(it, c, cases[c])
    assert next(it, None) is None
    # a single section, a workgroup filled to its last lane, multi-tile ragged meshes and the refusals all occur
    assert mesh_error_plans >= 9 and mesh_error_plans < len(cases)
