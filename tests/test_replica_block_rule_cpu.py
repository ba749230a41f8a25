"""The host side of the per-replica kernels' compile-time block shape (csrc/pc_eval_launch.hpp; host work, no GPU).

The bodies of a _w<W> kernel take the block's thread count (64 W), the tile width (64) and the wave index as constants
(pc_kernels.hpp), so the plan must never launch one with another block: pcl::plan refuses, by check_replica_block, a
per-replica kernel whose block is not 64 W threads or whose argument block names another W.  tests/c/replica_block_rule.cpp
plans hand-made shapes under AddressSanitizer + UBSan and prints one line per case; the expectations below restate the
rule.  That the shapes pc_eval_shape.hpp builds keep the rule (more than one wave per tile only with 64-thread tiles) is
tests/test_eval_shape_cpu.py's subject."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "c", "replica_block_rule.cpp")
EXE = os.path.join(ROOT, "tests", "_build", "replica_block_rule")
REFUSAL = "a per-replica kernel (_w<W>) takes a block of exactly 64 W threads"


@pytest.fixture(scope="module")
def lines():
    deps = [SRC, os.path.join(ROOT, "include", "pycollo_amd.h")]
    deps += [os.path.join(ROOT, "pycollo_amd", "csrc", f) for f in ("pc_eval_launch.hpp", "pc_eval_shape.hpp", "pc_desc.hpp", "pc_pattern.hpp", "pc_args.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        os.makedirs(os.path.dirname(EXE), exist_ok=True)
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
               "-fno-omit-frame-pointer", "-o", EXE + f".tmp{os.getpid()}", SRC]
        res = subprocess.run(cmd, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-3000:]
        os.replace(EXE + f".tmp{os.getpid()}", EXE)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([EXE], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0, res.stderr[-4000:]
    assert "Sanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-4000:]
    out = {}
    for ln in res.stdout.splitlines():
        name, rest = ln.split(" ", 1)
        out[name] = rest
    return out


def kernels(lines):
    return dict(zip(("res", "res_w", "all_res", "all_res_w"), lines["kernels"].split()))


@pytest.mark.parametrize("case,kernel,block", [("single_w4", "res_w", 256), ("single_w2", "res_w", 128), ("merged_w2", "all_res_w", 128)])
def test_per_replica_kernel_planned_with_its_block(lines, case, kernel, block):
    assert lines[case] == f"ok {kernels(lines)[kernel]} {block}"


@pytest.mark.parametrize("case,wpt,block", [("single_w2_tb128", 2, 256), ("single_w4_args_w2", 2, 256), ("merged_w2_tb256", 2, 512)])
def test_per_replica_kernel_refused_with_another_block(lines, case, wpt, block):
    assert lines[case] == f"refused {REFUSAL} (waves per tile {wpt}, block threads {block})"


@pytest.mark.parametrize("case,kernel,block", [("single_w2_tb128_plain", "res", 256), ("merged_w2_tb256_plain", "all_res", 512)])
def test_run_time_body_takes_any_block(lines, case, kernel, block):
    """Without a per-replica kernel in the code object the launch falls to the body that reads the block's shape at run time."""
    assert lines[case] == f"ok {kernels(lines)[kernel]} {block}"


@pytest.mark.parametrize("wpt,block,ok", [(2, 128, True), (4, 256, True), (1, 64, True), (4, 128, False), (2, 256, False),
                                          (2, 64, False), (0, 0, False)])
def test_rule(lines, wpt, block, ok):
    got = lines[f"rule_{wpt}_{block}"]
    assert got == "ok" if ok else got == f"refused {REFUSAL} (waves per tile {wpt}, block threads {block})"
