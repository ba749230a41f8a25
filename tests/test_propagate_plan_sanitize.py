"""The host index arithmetic of the propagation (pycollo_amd/csrc/pc_propagate_plan.hpp) under AddressSanitizer + UBSan
(CPU only).

``tests/c/propagate_plan_sanitize.cpp`` compiles the header with ``g++ -fsanitize=address,undefined
-fno-sanitize-recover=all``, builds the plan of every mesh and segment list it is fed, walks every node, section and
coefficient slot a lane would touch with bounds-checked accesses, and prints the plan; here it is compared with a NumPy
restatement.  The section patterns are those of tests/test_solution_plan_sanitize.py; the segment lists are "every
node", "section starts", "one segment" and an irregular one; then every refusal."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "c", "propagate_plan_sanitize.cpp")
EXE = os.path.join(ROOT, "tests", "_build", "propagate_plan_sanitize")
TB = 64
MAX_STEPS = 1 << 20


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


def _cases():
    rng = np.random.default_rng(11)
    patterns = [
        np.full(5, 4),                         # below one wave
        rng.integers(3, 9, 23),                # ragged
        rng.integers(3, 9, 60),                # several workgroups
        np.array([2, 20, 2, 20, 20]),          # order extremes
        np.full(64, 4),                        # sections: a 64-lane workgroup filled to the last lane; nodes: three of them
        np.array([20]),                        # one section
    ]
    good = dict(substeps=0, rtol=1e-9, max_steps=4096, atol=[1e-9, 2e-9])
    out = []
    for n_k in patterns:
        sec_s = np.concatenate(([0], np.cumsum(n_k - 1)))
        for kind in ("nodes", "sections", "phase", "irregular"):
            out.append(dict(good, n_k=n_k, seg=_segments(kind, sec_s, int(sec_s[-1]) + 1), accepted=True))
    n_k = np.full(5, 4)                        # 16 nodes
    ok_seg = np.array([0, 3, 4, 15])
    out.append(dict(good, n_k=n_k, seg=ok_seg, substeps=3, rtol=float("nan"), accepted=True))   # fixed: rtol is not read
    out.append(dict(good, n_k=n_k, seg=ok_seg, substeps=MAX_STEPS, max_steps=MAX_STEPS, accepted=True))
    out.append(dict(good, n_k=n_k, seg=ok_seg, max_steps=1, atol=[], accepted=True))            # a phase without states
    for bad in (dict(seg=np.array([0, 4, 4, 15])), dict(seg=np.array([0, 5, 4, 15])),           # not strictly ascending
                dict(seg=np.array([1, 4, 15])), dict(seg=np.array([0, 4, 14])), dict(seg=np.array([0, 4, 16])),
                dict(seg=np.array([], dtype=int)),                                              # no segment
                dict(seg=np.arange(16), n_k=np.full(4, 4)),                                     # more segments than intervals
                dict(substeps=-1), dict(substeps=MAX_STEPS + 1),
                dict(rtol=0.0), dict(rtol=-1e-9), dict(rtol=float("nan")), dict(rtol=float("inf")),
                dict(atol=[1e-9, 0.0]), dict(atol=[-1e-9, 1e-9]), dict(atol=[float("nan"), 1e-9]),
                dict(atol=[1e-9, float("inf")]), dict(substeps=2, atol=[0.0, 1e-9]),            # atol is always checked
                dict(max_steps=0), dict(max_steps=MAX_STEPS + 1)):
        out.append(dict(dict(good, n_k=n_k, seg=ok_seg, accepted=False), **bad))
    return out


def _restate(n_k, seg):
    sec_s = np.concatenate(([0], np.cumsum(np.asarray(n_k) - 1)))
    n_seg = len(seg) - 1
    seg_sec = np.searchsorted(sec_s, seg[:-1], side="right") - 1          # the last start <= the node
    return dict(N=int(sec_s[-1]) + 1, n_seg=n_seg, blocks=-(-n_seg // TB), seg_node=np.asarray(seg), seg_sec=seg_sec)


def test_propagate_plan_under_asan_ubsan(harness, tmp_path):
    cases = _cases()
    fin, fout = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    with open(fin, "w") as f:
        f.write(f"{len(cases)}\n")
        for cs in cases:
            orders = sorted({int(n) for n in cs["n_k"]})
            n_seg = max(len(cs["seg"]) - 1, 0)
            f.write(f"{len(cs['n_k'])} {len(orders)} {n_seg} {cs['substeps']} {cs['rtol']!r} {cs['max_steps']} {len(cs['atol'])}\n")
            f.write(" ".join(str(v) for v in orders) + "\n")
            f.write(" ".join(str(int(v)) for v in cs["n_k"]) + "\n")
            f.write(" ".join(str(int(v)) for v in (cs["seg"] if n_seg else [])) + "\n")
            f.write(" ".join(repr(float(v)) for v in cs["atol"]) + "\n")
    res = subprocess.run([harness, fin, fout], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-3000:]
    lines = open(fout).read().splitlines()
    n_refused = sum(not cs["accepted"] for cs in cases)
    assert n_refused == 20 and lines[-1] == "ok" and lines[-2] == f"refused {n_refused}"
    it = iter(lines[:-2])
    for c, cs in enumerate(cases):
        head = next(it).split()
        assert head[:2] == ["case", str(c)]
        assert (head[2] == "ok") == cs["accepted"], (c, head)
        if not cs["accepted"]:
            continue
        ref = _restate(cs["n_k"], cs["seg"])
        assert [int(v) for v in head[3:]] == [ref["N"], ref["n_seg"], ref["blocks"], TB]
        for name in ("seg_node", "seg_sec"):
            p = next(it).split()
            assert p[0] == name and int(p[1]) == len(ref[name])
            np.testing.assert_array_equal(np.array([int(v) for v in p[2:]]), ref[name], err_msg=f"case {c}: {name}")
