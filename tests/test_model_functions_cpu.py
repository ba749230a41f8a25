"""The generated model math, function family by function family, without a GPU.

* the high-precision reference itself: OracleNlp(fn_modules="mpmath") against the fp64 numpy oracle every other parity
  test trusts, on registered problems;
* the text the product's printer emits for each family's node functions, first and second partials and endpoint block,
  compiled on the host with the shared pc_powi prelude and compared, output by output, with the mpmath value of the
  model's own expression -- |got - ref| <= 1e-10 |ref| + 64 eps mag, mag from the oracle's _mag_expr;
* the structural patterns of the engine's host pattern builder against the oracle's;
* what compile_model refuses.
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import sympy as sym

from conftest import entry_err, golden_tables, vec_err
from model_function_cases import EDGE_NODES, FAMILIES, family_problem, kink_arguments
from oracle.ref_numpy import OracleNlp, _lam, _mag_expr
from pycollo_amd import codegen, problems
from pycollo_amd.model import compile_model
from pycollo_amd.problem import ProblemSpec

EPS = np.finfo(float).eps
N_RANDOM = 200


# ---------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", [("brachistochrone", {}), ("cart_pole", dict(K=5)), ("tumour_anti_angiogenesis", dict(K=5))])
def test_mpmath_oracle_agrees_with_numpy_oracle(name, kw):
    tab = golden_tables("lobatto")
    prob = problems.REGISTRY[name](**kw)
    a = OracleNlp(prob, tab)
    b = OracleNlp(prob, tab, fn_modules="mpmath")
    rng = np.random.default_rng(17)
    x = rng.uniform(-0.45, 0.45, a.num_x)
    lam = rng.normal(size=a.num_c)
    assert entry_err(a.c(x), b.c(x), b.c_mag(x)) <= 1.0
    assert entry_err(a.G(x), b.G(x), b.G_mag(x)) <= 1.0
    assert entry_err(a.H(x, 0.6, lam), b.H(x, 0.6, lam), b.H_mag(x, 0.6, lam)) <= 1.0
    assert vec_err(a.grad_J(x), b.grad_J(x)) <= 1.0
    assert abs(a.J(x) - b.J(x)) <= 1e-10 * max(1.0, abs(b.J(x)))
    for sa, sb in ((a.G_structure(), b.G_structure()), (a.H_structure(), b.H_structure())):
        np.testing.assert_array_equal(sa[0], sb[0])
        np.testing.assert_array_equal(sa[1], sb[1])


# ---------------------------------------------------------------------------------------------------
# the printed text, compiled on the host
# ---------------------------------------------------------------------------------------------------
def _host_source(model):
    """The C the printer emits for phase 0's node functions and partials and for the endpoint block -- through
    codegen._emit_block, inputs and outputs named as generate_source names them -- as two host functions."""
    pm, pt = model.phases[0], model.point
    v_in = {s: sym.Symbol(f"v[{i}]") for i, s in enumerate(pm.z + pm.s)}
    m_in = {s: sym.Symbol(f"mult[{i}]") for i, s in enumerate(pm.mf + pm.mp + pm.mg)}
    outs = [(f"F[{i}]", e) for i, e in enumerate(pm.f + pm.p + pm.g)]
    outs += [(f"Jv[{i}]", e) for i, (_, _, e) in enumerate(pm.jac)]
    outs += [(f"Hv[{i}]", e) for i, (_, _, e) in enumerate(pm.hess)]
    phase = [f"    constexpr double {k} = {float(val)!r};" for k, val in pm.consts] + codegen._emit_block({**v_in, **m_in}, outs, "w")
    p_in = {pv.symbol: sym.Symbol(f"xb[{i}]") for i, pv in enumerate(pt.vars)}
    p_in[pt.sigma] = sym.Symbol("sw")
    p_in.update({s: sym.Symbol(f"lb[{i}]") for i, s in enumerate(pt.lam)})
    pouts = [("Jval", pt.J)] + [(f"gJ[{i}]", e) for i, (_, e) in enumerate(pt.J_grad)] + [(f"b[{i}]", e) for i, e in enumerate(pt.b)]
    pouts += [(f"jb[{i}]", e) for i, (_, _, e) in enumerate(pt.b_jac)] + [(f"hb[{i}]", e) for i, (_, _, e) in enumerate(pt.hess)]
    point = [f"    constexpr double {k} = {float(val)!r};" for k, val in pt.consts] + codegen._emit_block(p_in, pouts, "w")
    lines = ["#include <cmath>", "#define __device__", "#define __forceinline__ inline", codegen.POWI_PRELUDE,
             'extern "C" void phase_eval(const double* v, const double* mult, double* F, double* Jv, double* Hv) {',
             "    (void)v; (void)mult; (void)F; (void)Jv; (void)Hv;"] + phase + ["}",
             'extern "C" void point_eval(const double* xb, double sw, const double* lb, double* Jout, double* gJ, double* b, '
             "double* jb, double* hb) {",
             "    (void)xb; (void)sw; (void)lb; (void)gJ; (void)b; (void)jb; (void)hb; double Jval = 0.0;"] + point + ["    *Jout = Jval;", "}", ""]
    return "\n".join(lines), "\n".join(phase + point)


def _compile_host(src, workdir, name):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed to compile the printed model text"
    path = os.path.join(workdir, name + ".cpp")
    with open(path, "w") as f:
        f.write(src)
    lib = os.path.join(workdir, name + ".so")
    # -ffp-contract=off as for the code objects: no fused multiply-add
    res = subprocess.run([cxx, "-O1", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", lib, path, "-lm"],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return ctypes.CDLL(lib)


def _dptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _worst(got, ref, mag):
    """max over entries of |got - ref| / (1e-10 |ref| + 64 eps mag); inf when a reference or magnitude is not finite."""
    got, ref, mag = (np.asarray(a, float) for a in (got, ref, mag))
    if not (np.all(np.isfinite(ref)) and np.all(np.isfinite(mag))):
        return float("inf")
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.abs(got - ref) / (1e-10 * np.abs(ref) + 64 * EPS * np.abs(mag) + 1e-290)
    return float(np.max(np.where(np.isnan(ratio), np.inf, ratio))) if ratio.size else 0.0


def _phase_points(family, model, rng):
    pm = model.phases[0]
    box = np.array(list(pm.x_bounds[:pm.n_z]) + list(model.s_bounds), dtype=float)
    assert pm.n_s == len(model.s_bounds)        # (the families use no q / t inside their node functions)
    pts = rng.uniform(box[:, 0], box[:, 1], (N_RANDOM, box.shape[0]))
    mid_s = 0.5 * (box[pm.n_z:, 0] + box[pm.n_z:, 1])
    edges = np.array([list(e) + list(mid_s) for e in EDGE_NODES[family]])
    return np.vstack([pts, edges])


def _point_points(family, model, rng):
    pm, pt = model.phases[0], model.point
    box = []
    for pv in pt.vars:
        box.append(pm.x_bounds[pv.idx] if pv.kind in ("y0", "yF") else
                   pm.x_bounds[pm.n_z + pv.idx] if pv.kind == "q" else model.s_bounds[pv.idx])
    box = np.array(box, dtype=float)
    pts = rng.uniform(box[:, 0], box[:, 1], (N_RANDOM, box.shape[0]))
    # the edge nodes, two at a time, as the values at t0 and at tF
    mid = 0.5 * (box[:, 0] + box[:, 1])
    edges = []
    for e0 in EDGE_NODES[family]:
        for eF in EDGE_NODES[family]:
            if family == "trig" and e0[2] == 0.0 and eF[2] == 0.0:
                continue        # atan2(wF, w0) at the origin: the reference itself is not finite there
            row = mid.copy()
            for i, pv in enumerate(pt.vars):
                if pv.kind == "y0":
                    row[i] = e0[pv.idx]
                elif pv.kind == "yF":
                    row[i] = eF[pv.idx]
            edges.append(row)
    return np.vstack([pts, np.array(edges)])


@pytest.mark.parametrize("family", FAMILIES)
def test_printed_text_on_the_host(family, tmp_path):
    model = compile_model(family_problem(family))
    pm, pt = model.phases[0], model.point
    src, body = _host_source(model)
    if family == "powers":
        # which branch of the power printer each exponent takes is part of what is tested: products up to the 4th power
        # (and k <= 4 under a half-integer), pc_powi from 5 up, libm's pow past |p| = 15/2 and for everything else
        x = sym.Symbol("x", real=True)
        assert codegen._c(x**4) == "(x*x*x*x)" and codegen._c(x**5) == "pc_powi<5>(x)"
        assert codegen._c(x**sym.Rational(9, 2)) == "((x*x*x*x)*sqrt(x))"
        assert codegen._c(x**sym.Rational(11, 2)) == "((pc_powi<5>(x))*sqrt(x))"
        assert codegen._c(x**sym.Rational(-15, 2)) == "(1.0/((pc_powi<7>(x))*sqrt(x)))"
        assert codegen._c(x**sym.Rational(17, 2)) == "pow(x, (17.0/2.0))"
        found = {int(n) for n in re.findall(r"pc_powi<(\d+)>", body)}
        assert found and min(found) == 5 and {5, 6, 7, 8} <= found
        assert "pow(" in body and "sqrt(" in body
    if family == "trig":
        # the reciprocal overrides are what printed sec / csc / cot here (SymPy's own rewrite spells them 1.0/(cos(x)))
        assert "(1.0/cos(" in body and "(1.0/sin(" in body and "(1.0/tan(" in body
        assert "atan2(" in body and "M_PI" in body and "M_E" in body and "M_LN10" in body
    lib = _compile_host(src, str(tmp_path), family)
    rng = np.random.default_rng(2024)

    # ---- node functions and partials
    exprs = list(pm.f + pm.p + pm.g) + [e for _, _, e in pm.jac] + [e for _, _, e in pm.hess]
    nF, nJ, nH = pm.n_fn, len(pm.jac), len(pm.hess)
    mult = pm.mf + pm.mp + pm.mg
    args = pm.z + pm.s + mult
    consts = dict(pm.consts)
    ref_fn = [_lam(args, e, consts, "mpmath") for e in exprs]
    mag_fn = [_lam(args, _mag_expr(e), consts, "mpmath") for e in exprs]
    pts = _phase_points(family, model, rng)
    worst = 0.0
    for row in pts:
        v = np.ascontiguousarray(row)
        m = rng.normal(size=len(mult))
        F, Jv, Hv = np.full(nF, np.nan), np.full(max(nJ, 1), np.nan), np.full(max(nH, 1), np.nan)
        lib.phase_eval(_dptr(v), _dptr(m), _dptr(F), _dptr(Jv), _dptr(Hv))
        got = np.concatenate([F, Jv[:nJ], Hv[:nH]])
        a = list(v) + list(m)
        ref = np.array([f(*a) for f in ref_fn])
        mag = np.array([f(*a) for f in mag_fn])
        w = _worst(got, ref, mag)
        assert w <= 1.0, f"{family}: node output {int(np.argmax(np.abs(got - ref)))} at v = {row.tolist()}: {w:.3g} x its bound"
        worst = max(worst, w)

    # ---- endpoint block
    pexprs = [pt.J] + [e for _, e in pt.J_grad] + list(pt.b) + [e for _, _, e in pt.b_jac] + [e for _, _, e in pt.hess]
    pargs = [pv.symbol for pv in pt.vars] + [pt.sigma] + list(pt.lam)
    pconsts = dict(pt.consts)
    pref = [_lam(pargs, e, pconsts, "mpmath") for e in pexprs]
    pmag = [_lam(pargs, _mag_expr(e), pconsts, "mpmath") for e in pexprs]
    lib.point_eval.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_double] + [ctypes.POINTER(ctypes.c_double)] * 6
    for row in _point_points(family, model, rng):
        xb = np.ascontiguousarray(row)
        sw, lb = float(rng.normal()), rng.normal(size=max(len(pt.lam), 1))
        Jo = np.full(1, np.nan)
        gJ, b, jb, hb = (np.full(max(n, 1), np.nan) for n in (len(pt.J_grad), len(pt.b), len(pt.b_jac), len(pt.hess)))
        lib.point_eval(_dptr(xb), sw, _dptr(lb), _dptr(Jo), _dptr(gJ), _dptr(b), _dptr(jb), _dptr(hb))
        got = np.concatenate([Jo, gJ[:len(pt.J_grad)], b[:len(pt.b)], jb[:len(pt.b_jac)], hb[:len(pt.hess)]])
        a = list(xb) + [sw] + list(lb[:len(pt.lam)])
        ref = np.array([f(*a) for f in pref])
        mag = np.array([f(*a) for f in pmag])
        w = _worst(got, ref, mag)
        assert w <= 1.0, f"{family}: endpoint output {int(np.argmax(np.abs(got - ref)))} at xb = {row.tolist()}: {w:.3g} x its bound"
        worst = max(worst, w)
    print(f"{family}: worst ratio to the bound {worst:.3g}")


def test_families_use_what_they_claim():
    """Every function the issue lists for a family is in its model (node functions and endpoint functions both use
    the family), so the tests above and on the GPU run it."""
    want = {
        "trig": {"tan", "sec", "csc", "cot", "asin", "acos", "atan", "sinh", "cosh", "tanh", "asinh", "acosh", "atanh", "atan2", "log"},
        "special": {"erf", "erfc", "exp", "log"},
        "kinks": {"Abs", "sign", "Max", "Min", "Piecewise", "Heaviside"},
    }
    for family, names in want.items():
        prob = family_problem(family)
        ph = prob.phases[0]
        node = list(ph.state_equations) + list(ph.path_constraints) + list(ph.integrand_functions)
        point = [prob.objective_function] + list(prob.endpoint_constraints)
        for group in (node, point):
            have = set()
            for e in group:
                have |= {type(a).__name__ for a in sym.sympify(e).atoms(sym.Function, sym.Max, sym.Min)}
            if group is node:
                assert names <= have, (family, names - have)
            else:
                assert have & names, family
    trig = family_problem("trig").phases[0]
    assert any(sym.sympify(e).has(sym.pi) for e in trig.integrand_functions) and any(sym.sympify(e).has(sym.E) for e in trig.integrand_functions)
    kinks = family_problem("kinks").phases[0]
    assert any(len(a.args) == 3 for e in kinks.state_equations for a in sym.sympify(e).atoms(sym.Min))
    assert len(kink_arguments(list(kinks.state_equations) + list(kinks.path_constraints) + list(kinks.integrand_functions))) >= 10


# ---------------------------------------------------------------------------------------------------
# patterns
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_patterns_equal_the_oracles(family, built):
    from pycollo_amd.engine import NlpEngine
    prob = family_problem(family)
    eng = NlpEngine(prob, device=None)
    ora = OracleNlp(prob, golden_tables("lobatto"), fn_modules="mpmath")
    for got, ref in ((eng.evaluate_G_structure(), ora.G_structure()), (eng.evaluate_H_structure(), ora.H_structure())):
        np.testing.assert_array_equal(got[0], ref[0])
        np.testing.assert_array_equal(got[1], ref[1])
    eng.close()
    if family == "kinks":
        # second partials that are a delta function only are in neither pattern: d2|y - 1/4| u / dy2 (the (y, y) entry
        # of state equation 0 comes from sign(v) y^2 alone), d2 Abs(u2) / du2^2 (nothing else is curved in u2 there)
        model = compile_model(prob)
        pm = model.phases[0]
        for _, _, e in pm.jac + pm.hess:
            assert not e.has(sym.DiracDelta) and not e.has(sym.Derivative)
        P = ora.P[0]
        y, v, u, u2 = P.z
        path_row = P.n_y
        assert (path_row, P.v.index(u2)) in P.dF and (path_row, P.v.index(u2), P.v.index(u2)) not in P.d2F
        iu2 = P.v.index(u2)
        others = [k for k in P.d2F if k[1] == iu2 and k[2] == iu2]
        assert {r for r, _, _ in others} <= {1}       # only the Piecewise branch -u2^2 of state equation 1 is curved in u2


# ---------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------
def _tiny(where, fn):
    y, u = sym.symbols("y u", real=True)
    prob = ProblemSpec("refused")
    ph = prob.new_phase("A")
    ph.state_variables = [y]
    ph.control_variables = [u]
    ph.state_equations = [fn(y) * u if where == "state equation" else y * u]
    ph.path_constraints = [fn(y) + u] if where == "path constraint" else []
    ph.integrand_functions = [fn(u) * y if where == "integrand" else y**2]
    yF = ph.final_state_variables[0]
    prob.objective_function = ph.integral_variables[0] + (fn(yF) if where == "objective" else 0)
    if where == "endpoint constraint":
        prob.endpoint_constraints = [fn(yF) + ph.initial_state_variables[0]]
        prob.bounds.endpoint_constraints = [[-1, 1]]
    ph.bounds.initial_time = 0
    ph.bounds.final_time = 1
    ph.bounds.state_variables = [[0.5, 2]]
    ph.bounds.control_variables = [[0.5, 2]]
    ph.bounds.integral_variables = [[0, 10]]
    if where == "path constraint":
        ph.bounds.path_constraints = [[-10, 10]]
    return prob


REFUSED = {"floor": sym.floor, "Mod": lambda a: sym.Mod(a, 2), "gamma": sym.gamma, "f": sym.Function("f")}
PLACES = {"state equation": "state equation 0", "path constraint": "path constraint 0", "integrand": "integrand 0",
          "objective": "objective function", "endpoint constraint": "endpoint constraint 0"}


@pytest.mark.parametrize("where", list(PLACES))
@pytest.mark.parametrize("name", list(REFUSED))
def test_compile_model_refuses_what_cannot_be_printed(name, where, monkeypatch):
    def no_hipcc(*a, **k):
        raise AssertionError("the refusal must come before any compiler call")
    monkeypatch.setattr(subprocess, "Popen", no_hipcc)
    monkeypatch.setattr(subprocess, "run", no_hipcc)
    with pytest.raises(ValueError) as err:
        compile_model(_tiny(where, REFUSED[name]))
    msg = str(err.value)
    assert re.search(rf"\b(poly)?{name}\b", msg), msg     # (gamma itself prints; its derivative, polygamma, does not)
    assert name in msg and PLACES[where] in msg, msg


def test_supported_kinks_compile():
    """What the refusals must not catch: the kink family goes through compile_model and generate_source."""
    src = codegen.generate_source(compile_model(family_problem("kinks")))
    assert "fabs(" in src and "fmax(" in src and "fmin(" in src and "DiracDelta" not in src
