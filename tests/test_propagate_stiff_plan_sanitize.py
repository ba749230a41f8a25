"""The host side of the implicit propagation (pycollo_amd/csrc/pc_propagate_plan.hpp: ``check_propagate_stiff_options``
and the lane's LDS indexing of ``pc_sol_propagate_stiff``) under AddressSanitizer + UBSan (CPU only).

``tests/c/propagate_stiff_plan_sanitize.cpp`` compiles the header with ``g++ -fsanitize=address,undefined
-fno-sanitize-recover=all`` and runs as a program: nothing is loaded into Python.  Every refusal of the option check, in
both modes; then, for NY = 1 .. PC_SOL_STIFF_MAX_NY, the addresses ``e * 64 + lane`` of the factors and of the row swaps
of all 64 lanes, walked as the kernel's LU walks them with bounds-checked accesses: no two lanes share one, none lies
beyond the array, and the arrays fit 64 KiB."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "c", "propagate_stiff_plan_sanitize.cpp")
EXE = os.path.join(ROOT, "tests", "_build", "propagate_stiff_plan_sanitize")
MAX_STEPS = 1 << 20
MAX_NY, MAX_NEWTON, TB = 11, 32, 64


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


GOOD = dict(substeps=0, rtol=1e-6, max_steps=4096, newton_max=8, atol=[1e-6, 2e-6], with_atol=1)
# (changes to GOOD, a word of the refusal or None when the options are accepted)
OPTIONS = [
    ({}, None), (dict(substeps=3), None), (dict(newton_max=1), None), (dict(newton_max=MAX_NEWTON), None),
    (dict(substeps=MAX_STEPS, max_steps=MAX_STEPS), None), (dict(atol=[1e-9] * MAX_NY), None), (dict(atol=[]), None),
    (dict(newton_max=0), "newton_max"), (dict(newton_max=MAX_NEWTON + 1), "newton_max"), (dict(newton_max=-3), "newton_max"),
    (dict(substeps=3, newton_max=0), "newton_max"),
    (dict(rtol=0.0), "rtol"), (dict(rtol=-1e-6), "rtol"), (dict(rtol="nan"), "rtol"), (dict(rtol="inf"), "rtol"),
    (dict(substeps=3, rtol=0.0), "rtol"), (dict(substeps=3, rtol="nan"), "rtol"), (dict(substeps=3, rtol="inf"), "rtol"),
    (dict(substeps=-1), "substeps"), (dict(substeps=MAX_STEPS + 1), "substeps"),
    (dict(max_steps=0), "max_steps"), (dict(max_steps=MAX_STEPS + 1), "max_steps"), (dict(substeps=3, max_steps=0), "max_steps"),
    (dict(atol=[1e-6, 0.0]), "atol"), (dict(atol=[-1e-6, 1e-6]), "atol"), (dict(atol=["nan", 1e-6]), "atol"),
    (dict(atol=[1e-6, "inf"]), "atol"), (dict(substeps=3, atol=[0.0, 1e-6]), "atol"), (dict(with_atol=0), "atol"),
    (dict(atol=[1e-9] * (MAX_NY + 1)), f"at most {MAX_NY} states"), (dict(substeps=3, atol=[1e-9] * 40), f"at most {MAX_NY} states"),
]


def test_option_check_and_lds_indexing_under_the_sanitizers(harness, tmp_path):
    lines = [str(len(OPTIONS))]
    for change, _ in OPTIONS:
        o = {**GOOD, **change}
        lines.append(" ".join(str(v) for v in [o["substeps"], o["rtol"], o["max_steps"], o["newton_max"], len(o["atol"]), *o["atol"],
                                                o["with_atol"]]))
    fin, fout = tmp_path / "in.txt", tmp_path / "out.txt"
    fin.write_text("\n".join(lines) + "\n")
    res = subprocess.run([harness, str(fin), str(fout)], capture_output=True, text=True)
    assert res.returncode == 0, (res.stderr[-3000:], fout.read_text()[-500:] if fout.exists() else "")
    assert "ERROR" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-3000:]
    out = fout.read_text().splitlines()
    for i, (change, word) in enumerate(OPTIONS):
        head = f"case {i} "
        assert out[i].startswith(head)
        if word is None:
            assert out[i] == head + "ok", (change, out[i])
        else:
            assert out[i].startswith(head + "refused propagate:") and word in out[i], (change, out[i])
    assert out[len(OPTIONS)] == f"max_ny {MAX_NY} max_newton {MAX_NEWTON} tb {TB}"
    lds = out[len(OPTIONS) + 1:]
    assert len(lds) == MAX_NY
    for ny, line in enumerate(lds, start=1):
        n_lu, n_piv = ny * ny * TB, ny * TB
        assert line == f"lds {ny} {n_lu} {n_piv} {8 * n_lu + 4 * n_piv} {n_lu + n_piv}", line
        assert 8 * n_lu + 4 * n_piv <= 65536
    assert 8 * (MAX_NY + 1) ** 2 * TB + 4 * (MAX_NY + 1) * TB > 65536


def test_python_layer_makes_the_same_refusals():
    import numpy as np
    from pycollo_amd.solution import (PROPAGATE_STIFF_MAX_NEWTON, PROPAGATE_STIFF_MAX_NY, check_propagate_method,
                                      check_propagate_tolerances)
    assert (PROPAGATE_STIFF_MAX_NY, PROPAGATE_STIFF_MAX_NEWTON) == (MAX_NY, MAX_NEWTON)
    check_propagate_method("dopri5", 0, 0.0, 40)                         # the explicit pair reads none of them
    check_propagate_method("sdirk4", 8, 1e-6, MAX_NY)
    for args in (("radau", 8, 1e-6, 2), (None, 8, 1e-6, 2), ("sdirk4", 0, 1e-6, 2), ("sdirk4", 33, 1e-6, 2), ("sdirk4", 2.5, 1e-6, 2),
                 ("sdirk4", 8, 0.0, 2), ("sdirk4", 8, float("nan"), 2), ("sdirk4", 8, float("inf"), 2), ("sdirk4", 8, 1e-6, MAX_NY + 1)):
        with pytest.raises(ValueError):
            check_propagate_method(*args)
    check_propagate_tolerances(3, 0.0, np.array([1e-6]), 4096)           # (fixed mode of the explicit pair: rtol is not read)
