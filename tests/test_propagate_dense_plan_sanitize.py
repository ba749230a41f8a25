"""The host index arithmetic of the propagation with integrals and dense output (pycollo_amd/csrc/pc_propagate_plan.hpp:
``check_integral_atol``, ``build_dense_query_plan``) under AddressSanitizer + UBSan (CPU only).

``tests/c/propagate_dense_plan_sanitize.cpp`` compiles the header with ``g++ -fsanitize=address,undefined
-fno-sanitize-recover=all``, builds the plan of every mesh, segment list and query list it is fed, walks every slot a
lane of ``pc_sol_propagate_dense`` would read or write with bounds-checked accesses -- every dense column and every
arrive column written exactly once -- and prints the plan; here ``q_order`` and ``node_q0`` are compared with the NumPy
restatement ``propagate_dense_ref.query_plan``.  The meshes are those of tests/test_propagate_plan_sanitize.py (every
interior section boundary is a node two sections share); the queries: none, one, every node, repeated, unsorted, the two
ends; then every refusal."""
import os
import subprocess

import numpy as np
import pytest

import propagate_dense_ref as pd
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "c", "propagate_dense_plan_sanitize.cpp")
EXE = os.path.join(ROOT, "tests", "_build", "propagate_dense_plan_sanitize")


@pytest.fixture(scope="module")
def harness():
    deps = [SRC] + [os.path.join(ROOT, "pycollo_amd", "csrc", f)
                    for f in ("pc_propagate_plan.hpp", "pc_solution_plan.hpp", "pc_args.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        os.makedirs(os.path.dirname(EXE), exist_ok=True)
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
               "-fno-omit-frame-pointer", "-o", EXE + f".tmp{os.getpid()}", SRC]
        res = subprocess.run(cmd, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-3000:]
        os.replace(EXE + f".tmp{os.getpid()}", EXE)
    return EXE


def _segments(kind, sec_s, N):
    if kind == "nodes":
        return np.arange(N)
    if kind == "sections":
        return sec_s
    if kind == "phase":
        return np.array([0, N - 1])
    return np.array(sorted({0, 1, N - 1} | {int(v) for v in np.arange(3, N - 1, 2.5)}))     # irregular


def plan_cases():
    rng = np.random.default_rng(12)
    patterns = [np.full(5, 4), rng.integers(3, 9, 23), rng.integers(3, 9, 60), np.array([2, 20, 2, 20, 20]), np.array([20]),
                np.array([2])]
    out = []
    for n_k in patterns:
        sec_s = np.concatenate(([0], np.cumsum(n_k - 1)))
        N = int(sec_s[-1]) + 1
        tau = np.cumsum(np.concatenate(([0.0], rng.uniform(0.2, 1.0, N - 1))))
        tau = 2.0 * tau / tau[-1] - 1.0
        tau[0], tau[-1] = -1.0, 1.0
        inner = rng.uniform(-1.0, 1.0, 3 * N)
        queries = {
            "none": np.zeros(0),
            "one": inner[:1],
            "one_at_the_start": tau[:1],
            "nodes": tau.copy(),
            "nodes_reversed_twice": np.concatenate([tau[::-1], tau[::-1]]),
            "unsorted_repeated": rng.permutation(np.concatenate([inner, inner[:7], tau, np.nextafter(tau[1:], -2.0),
                                                                 np.nextafter(tau[:-1], 2.0)])),
            "ends": np.array([1.0, -1.0, 1.0, -1.0]),
        }
        for i, (name, tq) in enumerate(queries.items()):
            kind = ("nodes", "sections", "phase", "irregular")[i % 4]
            out.append(dict(n_k=n_k, tau=tau, seg=_segments(kind, sec_s, N), tq=tq, NQ=i % 3, iatol=[1e-9] * (i % 3) if i % 2 else None,
                            accepted=True, what=name))
    n_k = np.full(5, 4)
    tau = np.linspace(-1.0, 1.0, 16)
    base = dict(n_k=n_k, tau=tau, seg=np.array([0, 3, 4, 15]), tq=np.array([0.3, -0.2]), NQ=2, iatol=[1e-9, 2e-9], accepted=False)
    for bad in (dict(tq=np.array([0.3, np.nan])), dict(tq=np.array([np.inf])), dict(tq=np.array([-np.inf, 0.0])),
                dict(tq=np.array([np.nextafter(1.0, 2.0)])), dict(tq=np.array([0.0, np.nextafter(-1.0, -2.0)])), dict(tq=np.array([7.0])),
                dict(iatol=[1e-9, 0.0]), dict(iatol=[-1e-9, 1e-9]), dict(iatol=[np.nan, 1e-9]), dict(iatol=[1e-9, np.inf]),
                dict(seg=np.array([0, 4, 4, 15]))):
        out.append(dict(base, what="refusal", **bad))
    return out


def run_plan_cases(exe, cases, tmp_path):
    """[(q_order, node_q0) or None (refused)] of the C++ plan, one per case"""
    fin, fout = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    row = lambda v: " ".join(repr(float(x)) for x in v) + "\n"   # noqa: E731
    with open(fin, "w") as f:
        f.write(f"{len(cases)}\n")
        for cs in cases:
            orders = sorted({int(n) for n in cs["n_k"]})
            f.write(f"{len(cs['n_k'])} {len(orders)} {len(cs['seg']) - 1} {cs['NQ']} {int(cs['iatol'] is not None)} {len(cs['tq'])}\n")
            f.write(" ".join(str(v) for v in orders) + "\n")
            f.write(" ".join(str(int(v)) for v in cs["n_k"]) + "\n")
            f.write(" ".join(str(int(v)) for v in cs["seg"]) + "\n")
            f.write(row(cs["tau"]) + row(cs["iatol"] or []) + row(cs["tq"]))
    res = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-3000:]
    lines = open(fout).read().splitlines()
    assert lines[-1] == "ok"
    it, out = iter(lines[:-2]), []
    for c, cs in enumerate(cases):
        head = next(it).split()
        assert head[:2] == ["case", str(c)]
        if head[2] != "ok":
            out.append(None)
            continue
        assert [int(v) for v in head[3:]] == [len(cs["tau"]), len(cs["tq"])]
        got = []
        for name in ("q_order", "node_q0"):
            p = next(it).split()
            assert p[0] == name
            got.append(np.array([int(v) for v in p[2:]], dtype=np.int64))
            assert int(p[1]) == len(got[-1])
        out.append(tuple(got))
    assert lines[-2] == f"refused {sum(g is None for g in out)}"
    return out


def test_dense_query_plan_under_asan_ubsan(harness, tmp_path):
    cases = plan_cases()
    got = run_plan_cases(harness, cases, tmp_path)
    assert sum(g is None for g in got) == 11
    for c, (cs, g) in enumerate(zip(cases, got)):
        assert (g is not None) == cs["accepted"], (c, cs["what"])
        if g is None:
            continue
        order, q0 = pd.query_plan(cs["tau"], cs["tq"])
        np.testing.assert_array_equal(g[0], order, err_msg=f"case {c} ({cs['what']}): q_order")
        np.testing.assert_array_equal(g[1], q0, err_msg=f"case {c} ({cs['what']}): node_q0")
        assert len(g[1]) == len(cs["tau"]) + 1 and g[1][0] == 0 and g[1][-1] == len(cs["tq"])
