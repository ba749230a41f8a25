"""The cache behind IPOPT's new_x flag (csrc/pc_callback_cache.hpp; host work, no GPU).

tests/c/callback_cache_sanitize.cpp drives the header under AddressSanitizer + UBSan against a simulated device whose
buffers are tagged with point, epoch and completeness.  It checks, for every sequence of calls up to LENGTH from every
starting setting, that a callback never hands back data that is incomplete, of another point or of an older scaling /
tile range, and prints what every call of the short sequences and of the call sequences of tests/test_gpu_hostpath.py
did.  ``Rules`` below restates the cache's rules from their description, not from the C++, and must
arrive at the same lines.

Tokens: f / gf / g / jac / h + new_x (pc_eval_f, grad_f, g, jac_g, h), all (pc_eval_all), dev (a device-pointer launch),
ipm (an interior-point launch), mesh (pc_mesh_error at another point), norms (pc_row_norms_jac), res (pc_eval_resident),
scal, range, mode<m>, pf<0|1>."""
import itertools
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "c", "callback_cache_sanitize.cpp")
EXE = os.path.join(ROOT, "tests", "_build", "callback_cache_sanitize")
HEADER = os.path.join(ROOT, "pycollo_amd", "csrc", "pc_callback_cache.hpp")
TOKENS = ["f0", "f1", "gf0", "gf1", "g0", "g1", "jac0", "jac1", "h0", "h1", "all", "dev", "ipm", "mesh", "norms", "res",
          "scal", "range", "mode0", "mode1", "mode2", "mode3", "pf0", "pf1"]
N_CALLBACKS = 10
LENGTH = 4
NO_WAIT, EV_SMALL, EV_G = 0, 1, 2

# the call sequences of tests/test_gpu_hostpath.py (mode, prefetch, calls), test by test
_MODES = " ".join(f"mode{m} all all f1 gf0 g0 jac0 h0" for m in range(4))
_MESH = " ".join(f"pf{p} g1 jac0 h0 mesh g0 jac0 h0 all mesh all" for p in (1, 0))
SCRIPTS = [
    "0 1 g1 f1 g0 jac0 gf0 gf1 jac0 g0 h1 g0 f0 scal g0",                  # test_new_x_protocol
    "0 1 " + " ".join(["f1 gf0 g0 jac0 h0"] * 3),                          # test_cyipopt_object_recovers_new_x
    f"0 1 all f1 gf1 {_MODES} mode0 norms",                                # test_host_modes_and_inplace_views_...
    "0 1 mode0 pf1 jac1 pf0 g1 h0 jac0",                                   # test_prefetch_off_...[hessian]
    "0 1 mode0 pf1 jac1 pf0 g1 norms jac0 g1 jac0",                        # ...[row_norms]
    f"0 1 mode0 {_MESH}",                                                  # ...[mesh_error]
    "0 1 f1 all g1 jac0 gf0 g1 g1 jac0",                                   # test_cyipopt_object_survives_direct_engine_calls
    "0 1 f1 dev f1 g0 gf0 f1 dev f0",                                      # test_cyipopt_object_survives_device_api_calls
    "0 1 dev mesh dev dev mesh dev g1 jac0",                               # test_device_api_is_unaffected_by_a_mesh_error_...
]


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in (SRC, HEADER)):
        os.makedirs(os.path.dirname(EXE), exist_ok=True)
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
               "-fno-omit-frame-pointer", "-o", EXE + f".tmp{os.getpid()}", SRC]
        res = subprocess.run(cmd, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-3000:]
        os.replace(EXE + f".tmp{os.getpid()}", EXE)
    tmp = tmp_path_factory.mktemp("callback_cache")
    fscripts, fout = str(tmp / "scripts.txt"), str(tmp / "out.txt")
    open(fscripts, "w").write("\n".join(SCRIPTS) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([EXE, str(LENGTH), fscripts, fout], capture_output=True, text=True, env=env, timeout=300)
    assert res.returncode == 0, res.stderr[-4000:]
    assert "Sanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-4000:]
    lines = open(fout).read().splitlines()
    assert lines[-1] == "ok"
    return lines[:-1]


def test_no_sequence_hands_back_stale_or_incomplete_data(output):
    """Every sequence of 1 .. LENGTH calls from the 8 starting settings was run (none skipped), and every callback in
    last place was checked: the program exits non-zero at the first that fails."""
    n = len(TOKENS)
    assert output[0] == f"sequences {8 * sum(n ** k for k in range(1, LENGTH + 1))}"
    assert output[1] == f"callbacks {8 * sum(n ** (k - 1) * N_CALLBACKS for k in range(1, LENGTH + 1))}"


class Rules:
    """The rules of DESIGN section 4.3, one method per event."""

    def __init__(self, mode, prefetch):
        self.x_staged = self.filled = self.small_down = self.G_down = self.G_queued = False
        self.prefetch, self.mode, self.gen = bool(prefetch), mode, 0
        self.input_overwritten()   # the mode is set through pc_set_host_mode's rule

    def stage(self, new_x):
        if new_x or not self.x_staged:
            self.x_staged, self.filled = True, False
            self.gen += 1
            return 1
        return 0

    def callback(self, new_x, want):
        stage, launch, q_small, q_G, wait = self.stage(new_x), 0, 0, 0, NO_WAIT
        if not self.filled:
            launch = q_small = 1
            self.G_queued = self.prefetch or bool(self.mode & 2)
            q_G = int(self.G_queued)
            self.filled, self.small_down, self.G_down = True, False, False
            self.gen += 1
        if want == "small" and not self.small_down:
            wait, self.small_down = EV_SMALL, True
        if want == "G" and not self.G_down:
            if not self.G_queued:
                q_G, self.G_queued = 1, True
            wait, self.small_down, self.G_down = EV_G, True, True
        return stage, launch, q_small, q_G, wait

    def drained(self):
        self.small_down = self.filled
        self.G_down = self.filled and self.G_queued

    def result_overwritten(self):
        self.filled = self.small_down = self.G_down = False
        self.gen += 1

    def input_overwritten(self):
        self.x_staged = self.filled = False
        self.gen += 1

    def call(self, tok):
        record = (0, 0, 0, 0, NO_WAIT)
        if tok[:-1] in ("f", "gf", "g"):
            record = self.callback(int(tok[-1]), "small")
        elif tok[:-1] == "jac":
            record = self.callback(int(tok[-1]), "G")
        elif tok[:-1] == "h":
            record = (self.stage(int(tok[-1])), 0, 0, 0, NO_WAIT)
            self.drained()
        elif tok == "all":   # everything came down, G~ included: the one quirk of the old flags that was fixed
            self.x_staged = self.filled = self.small_down = self.G_down = self.G_queued = True
            self.gen += 1
        elif tok in ("dev", "ipm"):
            self.result_overwritten()
        elif tok in ("mesh", "res", "scal"):
            self.input_overwritten()
        elif tok == "range":
            self.filled = False
            self.gen += 1
        elif tok == "norms":
            mode, self.mode = self.mode, 0
            self.input_overwritten()
            record = self.callback(1, "nothing")
            self.mode = mode
            self.x_staged = self.filled = mode == 0
            self.drained()
            self.gen += 1
        elif tok.startswith("mode"):
            self.mode = int(tok[-1])
            self.input_overwritten()
        else:
            self.prefetch = tok == "pf1"
        state = (self.x_staged, self.filled, self.small_down, self.G_down, self.G_queued, self.prefetch)
        return "%s %d %d %d %d %d | " % ((tok,) + record) + " ".join(str(int(v)) for v in state) + f" {self.mode} {self.gen}"


def expect(mode, prefetch, toks):
    r = Rules(mode, prefetch)
    return [f"start {mode} {prefetch}"] + [r.call(t) for t in toks]


def test_every_call_does_what_the_rules_say(output):
    want = []
    for mode, prefetch in itertools.product(range(4), range(2)):
        for a in TOKENS:
            want += expect(mode, prefetch, [a])
            for b in TOKENS:
                want += expect(mode, prefetch, [a, b])
    for s in SCRIPTS:
        w = s.split()
        want += expect(int(w[0]), int(w[1]), w[2:])
    got = output[2:]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i}: program {g!r}, rules {w!r}"
