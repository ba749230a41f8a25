"""The colouring plan of the derivative check (pycollo_amd/csrc/pc_deriv.hpp) under AddressSanitizer + UBSan (CPU only).

``tests/c/deriv_plan_sanitize.cpp`` compiles pc_deriv.hpp with the pattern builder it reads (pc_desc.hpp, pc_pattern.hpp)
using ``g++ -fsanitize=address,undefined -fno-sanitize-recover=all``, is fed the descriptor the engine hands the library
(the text format of tests/c/pattern_sanitize.cpp) and must exit cleanly and print the plan arrays the library returns
(``pc_deriv_plan``)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from pycollo_amd import problems
from pycollo_amd.engine import NlpEngine
from test_sanitized_host import _serialise

SRC = os.path.join(ROOT, "tests", "c", "deriv_plan_sanitize.cpp")
EXE = os.path.join(ROOT, "tests", "_build", "deriv_plan_sanitize")


@pytest.fixture(scope="module")
def harness():
    deps = [SRC] + [os.path.join(ROOT, "pycollo_amd", "csrc", f) for f in ("pc_deriv.hpp", "pc_desc.hpp", "pc_eval_shape.hpp", "pc_pattern.hpp", "pc_args.h")]
    deps.append(os.path.join(ROOT, "tests", "c", "desc_reader.hpp"))
    deps.append(os.path.join(ROOT, "include", "pycollo_amd.h"))
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        os.makedirs(os.path.dirname(EXE), exist_ok=True)
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
               "-fno-omit-frame-pointer", "-o", EXE + f".tmp{os.getpid()}", SRC]
        res = subprocess.run(cmd, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-3000:]
        os.replace(EXE + f".tmp{os.getpid()}", EXE)
    return EXE


def _parse(path):
    out = {}
    with open(path) as f:
        for line in f:
            p = line.split()
            if p[0] in ("sizes", "ok"):
                out[p[0]] = tuple(int(v) for v in p[1:])
            else:
                vals = np.array([int(v) for v in p[2:]], dtype=np.int64)
                assert len(vals) == int(p[1])
                out[p[0]] = vals
    return out


@pytest.mark.parametrize("name,kw,refined", [
    ("brachistochrone", {}, False), ("hypersensitive", {"K": 40, "order": 6}, False), ("two_phase_transfer", {}, False),
    ("time_coupled_transfer", {}, False), ("delta_iii", {}, False), ("sliding_mass", {"num_phases": 3}, False),
    ("hypersensitive", {}, True)])
def test_deriv_plan_under_asan_ubsan(harness, tmp_path, name, kw, refined):
    prob = problems.REGISTRY[name](**kw)
    if refined:
        prob = problems.with_refined_mesh(prob, 2000, seeds=(3,))
    eng = NlpEngine(prob, device=None)
    desc = eng._make_desc(None, 0)
    fin, fout = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    _serialise(eng, desc, fin)
    res = subprocess.run([harness, fin, fout], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-3000:]
    got = _parse(fout)
    assert "ok" in got
    plan = eng.derivative_plan()
    assert got["sizes"][0] == plan.n_colours and got["sizes"][2] == 0
    np.testing.assert_array_equal(got["colour"], plan.colour)
    np.testing.assert_array_equal(got["g_flag"], plan.jac_located.astype(np.int64))
    np.testing.assert_array_equal(got["h_flag"], plan.hess_flag.astype(np.int64))
    np.testing.assert_array_equal(got["j_flag"], plan.jgrad_located.astype(np.int64))
