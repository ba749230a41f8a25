"""The step controller of the propagation kernels (pycollo_amd/csrc/pc_step_control.hpp: ``StepControl``) under
AddressSanitizer + UBSan (CPU only), against a restatement of DESIGN 8e / 8h.

``tests/c/step_control_sanitize.cpp`` compiles the header with ``g++ -fsanitize=address,undefined
-fno-sanitize-recover=all`` and runs as a program: nothing is loaded into Python.  It drives the controller through
scripted outcomes (newton_ok, bad, err) of the attempts of one interval (ca, cb) and prints every attempt's c, h and end
as hex floats, the decision, and the final counts and status.  ``restate`` below is written from the text of the
design, not from the header; both sides call the same libm ``pow``, so every figure is held to exact equality.  Every
script runs with the exponent -1/5 and with -1/4, with and without Newton failures being read."""
import math
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "c", "step_control_sanitize.cpp")
EXE = os.path.join(ROOT, "tests", "_build", "step_control_sanitize")


@pytest.fixture(scope="module")
def harness():
    deps = [SRC, os.path.join(ROOT, "pycollo_amd", "csrc", "pc_step_control.hpp")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        os.makedirs(os.path.dirname(EXE), exist_ok=True)
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
               "-fno-omit-frame-pointer", "-o", EXE + f".tmp{os.getpid()}", SRC]
        res = subprocess.run(cmd, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-3000:]
        os.replace(EXE + f".tmp{os.getpid()}", EXE)
    return EXE


def restate(exponent, newton, m, ca, cb, max_steps, script):
    """DESIGN 8e (8h with ``newton``): the attempts of one interval as (c, h, end, last, accepted) and the final
    (c, accepted, rejected, newton_rejected, failed).  Attempt k gets script[min(k, len - 1)]."""
    attempts, n_acc, n_rej, n_newt = [], 0, 0, 0
    outcome = lambda: script[min(len(attempts), len(script) - 1)]   # noqa: E731
    if m > 0:   # fixed: step q starts at ca + q h0 (computed, not accumulated), the last one ends at cb
        h0 = (cb - ca) / float(m)
        c = ca
        for q in range(m):
            c = ca + float(q) * h0
            last = q == m - 1
            h, end = (cb - c, cb) if last else (h0, c + h0)
            newton_ok = outcome()[0]
            if newton and not newton_ok:   # ends the interval as failed: its one rejected step
                attempts.append((c, h, end, last, False))
                return attempts, (c, n_acc, 1, 1, True)
            attempts.append((c, h, end, last, True))
            n_acc += 1
        # (c: where the last step started; the kernels do not read it behind a fixed interval)
        return attempts, (c, n_acc, 0, 0, False)
    c, h, last, after_reject = ca, cb - ca, True, False
    while n_acc + n_rej < max_steps:
        newton_ok, bad, err = outcome()
        ok = newton_ok or not newton
        end = cb if last else c + h
        if not ok:
            factor = 0.25
        elif bad:
            factor = 0.2
        elif err == 0.0:
            factor = 5.0
        else:
            factor = min(5.0, max(0.2, 0.9 * math.pow(err, exponent)))
        if ok and not bad and err <= 1.0:
            attempts.append((c, h, end, last, True))
            n_acc += 1
            c = end
            if after_reject:
                factor = min(factor, 1.0)
            after_reject = False
            rest = cb - c
            if last or not rest > 0.0:
                return attempts, (c, n_acc, n_rej, n_newt, False)
            h = h * factor
            last = h >= rest
            if last:
                h = rest
        else:
            attempts.append((c, h, end, last, False))
            n_rej += 1
            n_newt += 0 if ok else 1
            h = h * factor
            last = False
            after_reject = True
    return attempts, (c, n_acc, n_rej, n_newt, True)


CA, CB = -0.3, 0.7 / 3.0            # a width that is no binary fraction
OK, BAD, NEWTON = (1, 0), (1, 1), (0, 0)
HUGE, TINY = 1e300, 1e-300


def _round_to_cb(exponent):
    """An interval and a script whose last step does not take the rest (h < rest, so ``last`` is not set) and
    still lands on cb: c + h rounds to cb, the rest is not positive, the interval is done.  The err that does it is
    searched in the restatement; next to a large cb one ulp of cb is thousands of ulps of h."""
    ca, cb = 1000.0, 1000.7
    head = [(1, 0, HUGE), (1, 0, 1.0), (1, 0, 1.0), (1, 0, 1.0)]     # h = 0.2 w, then three steps, each 0.9 of the one before
    att, _ = restate(exponent, False, 0, ca, cb, 50, head + [(1, 0, 1.0)])
    c4, h4 = att[4][0], att[4][1]                                   # the fourth step
    want = (cb - (c4 + h4)) / h4                                    # the factor that would make the next h the rest
    err = (want / 0.9) ** (1.0 / exponent) * (1.0 - 1e-11)
    for _ in range(20000):
        script = head + [(1, 0, err), (1, 0, 0.5)]
        att, end = restate(exponent, False, 0, ca, cb, 50, script)
        if len(att) == 6 and att[5][3] is False and att[5][4] and end[0] == cb and not end[4]:
            return ca, cb, script
        err *= 1.0 + 2e-15
    raise AssertionError("no err found that lands on cb without taking the rest")


def _scripts():
    s = [
        ("accepted at once", 0, CA, CB, 10, [(*OK, 0.5)]),
        ("one rejection, the factor behind it capped at 1", 0, CA, CB, 50, [(*OK, 1e3), (*OK, 1e-3)]),
        ("err = 0 gives 5", 0, CA, CB, 50, [(*OK, HUGE)] * 3 + [(*OK, 0.5), (*OK, 0.0), (*OK, 0.9)]),
        ("bad gives 0.2 and a rejection", 0, CA, CB, 50, [(*BAD, float("nan")), (*BAD, 0.5), (*OK, 0.5)]),
        ("both clamps", 0, CA, CB, 50, [(*OK, HUGE), (*OK, HUGE), (*OK, 0.9), (*OK, TINY), (*OK, 0.9)]),
        ("err infinite and not flagged", 0, CA, CB, 50, [(*OK, float("inf")), (*OK, 0.5)]),
        ("a growth that overshoots the rest", 0, CA, CB, 50, [(*OK, 50.0), (*OK, 1e-9), (*OK, 1e-9)]),
        ("Newton failures, adaptive", 0, CA, CB, 50, [(*NEWTON, 0.5), (*NEWTON, 0.0), (*OK, 2.0), (*OK, 0.5)]),
        ("Newton failures only", 0, CA, CB, 3, [(*NEWTON, 0.5)]),
        ("fixed, a Newton failure at the first step", 5, CA, CB, 1, [(*NEWTON, 0.5)]),
        ("fixed, a Newton failure at a later step", 5, CA, CB, 1, [(*OK, 0.5), (*OK, 7.0), (*NEWTON, 0.5)]),
    ]
    s += [(f"max_steps = {k} used up", 0, CA, CB, k, [(*OK, 30.0)]) for k in (1, 2, 3)]
    s += [(f"max_steps = {k}, the last attempt accepted short of cb", 0, CA, CB, k, [(*OK, 30.0), (*OK, 0.9)]) for k in (2, 3)]
    s += [(f"fixed, m = {m}", m, CA, CB, 1, [(*BAD, HUGE)]) for m in (1, 2, 5)]      # (bad and err are not read)
    for e in (-0.2, -0.25):
        ca, cb, script = _round_to_cb(e)
        s.append((f"c + h rounds to cb, exponent {e}", 0, ca, cb, 50, script))
    return s


KINDS = [(5, -0.2, 0), (5, -0.2, 1), (4, -0.25, 1), (4, -0.25, 0)]   # (the program's name of the exponent, it, newton)


def _hex(x):
    return "nan" if x != x else float(x).hex()


def test_controller_equals_the_restatement_under_the_sanitizers(harness, tmp_path):
    scripts = _scripts()
    cases = [(kind, sc) for sc in scripts for kind in KINDS]
    lines = [str(len(cases))]
    for (tag, _, newton), (_, m, ca, cb, max_steps, script) in cases:
        lines.append(f"{tag} {newton} {m} {ca.hex()} {cb.hex()} {max_steps} {len(script)}")
        lines += [f"{o[0]} {o[1]} {'nan' if o[2] != o[2] else ('inf' if o[2] == math.inf else float(o[2]).hex())}" for o in script]
    fin, fout = tmp_path / "in.txt", tmp_path / "out.txt"
    fin.write_text("\n".join(lines) + "\n")
    res = subprocess.run([harness, str(fin), str(fout)], capture_output=True, text=True)
    assert res.returncode == 0, (res.stderr[-3000:], fout.read_text()[-500:] if fout.exists() else "")
    assert "ERROR" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-3000:]
    out = iter(fout.read_text().splitlines())
    for ic, ((_, exponent, newton), (name, m, ca, cb, max_steps, script)) in enumerate(cases):
        what = (name, exponent, newton)
        attempts, (c_end, n_acc, n_rej, n_newt, failed) = restate(exponent, bool(newton), m, ca, cb, max_steps, script)
        assert next(out) == f"case {ic}", what
        calls = 0
        for c, h, end, last, accepted in attempts:
            calls += accepted
            tok = next(out).split()
            assert tok[0] == "attempt", (what, tok)
            got = [_hex(float.fromhex(t)) for t in tok[1:4]] + [int(t) for t in tok[4:]]
            assert got == [_hex(c), _hex(h), _hex(end), int(last), int(accepted), calls], (what, tok)
        tok = next(out).split()
        assert tok[0] == "end", (what, tok)
        assert [int(t) for t in tok[2:]] == [n_acc, n_rej, n_newt, int(failed)], (what, tok)
        if m == 0 or failed:      # (behind a complete fixed interval c is where the last step started: not read)
            assert _hex(float.fromhex(tok[1])) == _hex(c_end), (what, tok)
    assert next(out, None) is None


def test_the_scripts_reach_what_they_are_for():
    """The restatement's own figures on the scripts: each case of the list in the module's purpose is really hit."""
    by_name = {sc[0]: sc for sc in _scripts()}

    def run(name, exponent=-0.2, newton=True):
        _, m, ca, cb, max_steps, script = by_name[name]
        return restate(exponent, newton, m, ca, cb, max_steps, script)

    w = CB - CA
    att, end = run("accepted at once")
    assert att == [(CA, w, CB, True, True)] and end == (CB, 1, 0, 0, False)
    att, end = run("one rejection, the factor behind it capped at 1")
    assert [a[4] for a in att[:2]] == [False, True] and att[2][1] == att[1][1] and end[0] == CB and not end[4]
    att, _ = run("err = 0 gives 5")
    assert att[5][1] == att[4][1] * 5.0 and not att[5][3]
    att, _ = run("bad gives 0.2 and a rejection")
    assert [a[4] for a in att[:2]] == [False, False] and att[1][1] == w * 0.2 and att[2][1] == w * 0.2 * 0.2
    att, _ = run("both clamps")
    assert att[1][1] == w * 0.2 and att[4][1] == att[3][1] * 5.0
    att, end = run("a growth that overshoots the rest")
    assert att[-1][3] and att[-1][1] == CB - att[-1][0] and att[-1][1] < att[-2][1] * 5.0 and end[0] == CB
    for e in (-0.2, -0.25):
        att, end = run(f"c + h rounds to cb, exponent {e}", e)
        assert not att[-1][3] and att[-1][1] < 1000.7 - att[-1][0] and end == (1000.7, 5, 1, 0, False)
    for k in (1, 2, 3):
        assert run(f"max_steps = {k} used up")[1][1:] == (0, k, 0, True)
    for k in (2, 3):
        assert run(f"max_steps = {k}, the last attempt accepted short of cb")[1][1:] == (k - 1, 1, 0, True)
    att, end = run("Newton failures, adaptive")
    assert att[1][1] == w * 0.25 and att[2][1] == w * 0.25 * 0.25 and end[2:4] == (3, 2)
    assert run("Newton failures, adaptive", newton=False)[1][3] == 0
    assert run("Newton failures only")[1][1:] == (0, 3, 3, True)
    assert run("fixed, a Newton failure at the first step")[1][1:] == (0, 1, 1, True)
    assert run("fixed, a Newton failure at a later step")[1][1:] == (2, 1, 1, True)
    assert run("fixed, a Newton failure at a later step", newton=False)[1][1:] == (5, 0, 0, False)
    for m in (1, 2, 5):
        att, end = run(f"fixed, m = {m}")
        h0 = w / float(m)
        assert [a[0] for a in att] == [CA + float(q) * h0 for q in range(m)]
        assert att[-1][1] == CB - att[-1][0] and att[-1][2] == CB and all(a[1] == h0 and a[2] == a[0] + h0 for a in att[:-1])
        assert end[1:] == (m, 0, 0, False)
