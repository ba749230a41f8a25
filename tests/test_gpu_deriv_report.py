"""GPU tests of what the derivative check reports (pc_check_derivatives_device, NlpEngine.check_derivatives; run with
-m gpu), next to tests/test_gpu_deriv_check.py: many failures at once, in several reduction blocks, at the block and kind
boundaries, beyond the cap of the list, with ties and non-finite values; grad L rows cut into chunks (long columns of
G~); tol's strictness, max_report, delta; every single entry of a small NLP corrupted in turn.

The reference side is tests/deriv_restate.py (pinned without a GPU by tests/test_deriv_report_cpu.py) on the SAME
engine's evaluators (evaluate_c / _J / _G_nonzeros / _g): the perturbed points and c~, G~, grad J~ at them are then the
same bits on both sides, which isolates the check's own kernels and gives the bounds used here:
  FD of a located G~ entry, of a grad J~ non-zero   2 ulps (one division each side)
  (c+ - c-) / 2 of a sum                            bit-equal
  FD of an H~ entry read from grad L row q          n_q eps sum|t_e| / |step2| + 4 eps |ref|: the terms t_e = (G+_e -
                                                    G-_e) lambda_r are the same bits, only the summation order differs
  sum an_j h_j of a sum of n terms                  (n + 1) eps sum|an_j h_j|
  err of a reported entry                           bit-equal to NumPy's |an - fd| / max(1, |an|) on the reported values
Every scenario corrupts entries by 1e-3 max(1, |v|) at x~ ~ U(-0.45, 0.45) (seed 11), lambda ~ U(-1, 1), sigma = 0.7 and
first asserts, on the restatement alone, that every uncorrupted err is <= tol / 10 and every corrupted one >= 5 tol: the
failing set does not hang on a rounding.  Only builds build() makes are loaded."""
import numpy as np
import pytest

from deriv_restate import errors, expected_report, restate, sum_keys
from pycollo_amd import problems
from pycollo_amd.engine import NlpEngine
from test_gpu_deriv_check import _categories, _point, _radau_brachistochrone
from test_gpu_mixed import mixed_problem

pytestmark = pytest.mark.gpu

SIGMA, TOL, EPS = 0.7, 1e-4, float(np.finfo(float).eps)
DERIV_CHUNK = 1024   # pc_deriv_check.hpp: a column of G~ with more entries is summed in chunks

ENGINES = {
    "two_phase_K40": (lambda: problems.two_phase_transfer(K=40, order=4), {}),
    "two_phase_default": (problems.two_phase_transfer, {}),
    "brachistochrone_K113": (lambda: problems.brachistochrone(K=113, order=4), {}),
    "brachistochrone_K114": (lambda: problems.brachistochrone(K=114, order=4), {}),
    "brachistochrone_K230": (lambda: problems.brachistochrone(K=230, order=4), {}),
    "time_coupled_K150": (lambda: problems.time_coupled_transfer(K=150, order=4), {}),
    "time_coupled_mixed": (lambda: mixed_problem("time_coupled_transfer"), {"mixed": ((4, 6), (4, 6))}),
    "brachistochrone_radau": (_radau_brachistochrone, {}),
}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    """Bit-equal doubles (any NaN equals any NaN: a payload is not part of the contract)."""
    a, b = np.float64(a), np.float64(b)
    return bool((np.isnan(a) and np.isnan(b)) or _bits([a])[0] == _bits([b])[0])


class _Case:
    """An engine at the clean point, its structures and plan, its own analytic values, and per delta the restatement on
    its evaluators and a clean check with return_fd -- each computed once and left unchanged."""

    def __init__(self, eng):
        self.eng = eng
        self.x, self.lam = _point(eng, (-0.45, 0.45), seed=11)
        self.plan = eng.derivative_plan()
        self.g_struct = tuple(a.astype(np.int64) for a in eng.evaluate_G_structure())
        self.h_struct = tuple(a.astype(np.int64) for a in eng.evaluate_H_structure())
        self.jcols = np.asarray(eng.jgrad_columns(), np.int64)
        self.struct = (self.g_struct, self.h_struct, self.jcols)
        self.G = eng.evaluate_G_nonzeros(self.x)
        self.H = eng.evaluate_H_nonzeros(self.x, SIGMA, self.lam)
        self.J = eng.evaluate_g(self.x)[self.jcols]
        self.keys = sum_keys(self.g_struct, self.plan)
        self.nG, self.nS, self.nH, self.nJ = self.G.size, len(self.keys), self.H.size, self.J.size
        self.T = self.nG + self.nS + self.nH + self.nJ
        self.fns = (eng.evaluate_c, eng.evaluate_J, eng.evaluate_G_nonzeros, eng.evaluate_g)
        self._ref, self._clean = {}, {}

    def ref(self, delta=1e-5):
        """(fdG, fdH, fdJ, sums, rounding) of the restatement on the engine's own evaluators."""
        if delta not in self._ref:
            rounding = {}
            out = restate(self.fns, self.plan, self.g_struct, self.h_struct, self.jcols, self.x, SIGMA, self.lam, delta,
                          rounding=rounding)
            self._ref[delta] = out + (rounding,)
        return self._ref[delta]

    def check(self, G=None, H=None, J=None, **kw):
        return self.eng.check_derivatives(self.x, SIGMA, self.lam, jac_values=self.G if G is None else G,
                                          hess_values=self.H if H is None else H, jgrad_values=self.J if J is None else J, **kw)

    def clean(self, delta=1e-5):
        if delta not in self._clean:
            self._clean[delta] = self.check(delta=delta, return_fd=True)
        return self._clean[delta]

    def blocks(self):
        """(chunk, blocks) of the reduction over the concatenated error array: for PLACING failures only."""
        nb = min(256, max(1, -(-self.T // 4096)))
        return max(1, -(-self.T // nb)), nb

    def pos(self, kind, i):
        return {"jac": 0, "jac_sum": self.nG, "hess": self.nG + self.nS, "grad": self.nG + self.nS + self.nH}[kind] + i

    def sum_of(self, e):
        """Number of the sum the G~ entry e is a term of."""
        return self.keys.index((int(self.g_struct[0][e]), int(self.plan.colour[self.g_struct[1][e]])))

    def largest_term(self, s):
        ents = np.array(self.ref()[3][self.keys[s]][0])
        return int(ents[np.argmax(np.abs(self.G[ents]))])

    def col_sizes(self):
        return np.bincount(self.g_struct[1], minlength=self.eng.num_x)

    def grad_l_row(self):
        """Per H~ entry, the row of grad L (= column of G~) its difference is read from."""
        hr, hc = self.h_struct
        return np.where((self.plan.hess_flag & 1).astype(bool), hr, hc)


_CASES = {}


def _case(key):
    if key not in _CASES:
        make, kw = ENGINES[key]
        _CASES[key] = _Case(NlpEngine(make(), device=0, **kw))
    return _CASES[key]


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    for case in _CASES.values():
        case.eng.close()
    _CASES.clear()


def _bump(v, idx):
    v = v.copy()
    for i in idx:
        v[i] += 1e-3 * max(1.0, abs(v[i]))
    return v


def _scenario(case, g=(), h=(), j=()):
    return _bump(case.G, g), _bump(case.H, h), _bump(case.J, j)


def _corrupted(case, G2, H2, J2):
    """Mask over the concatenated positions of what the scenario changed (a changed sum term marks its sum)."""
    m = np.zeros(case.T, bool)
    for e in np.flatnonzero(_bits(G2) != _bits(case.G)):
        m[e if case.plan.jac_located[e] else case.pos("jac_sum", case.sum_of(e))] = True
    m[case.pos("hess", 0) + np.flatnonzero(_bits(H2) != _bits(case.H))] = True
    m[case.pos("grad", 0) + np.flatnonzero(_bits(J2) != _bits(case.J))] = True
    return m


def _precondition(case, G2, H2, J2, delta=1e-5):
    """On the restatement alone: every uncorrupted err <= tol / 10, every corrupted err >= 5 tol."""
    fdG, fdH, fdJ, sums, _ = case.ref(delta)
    err = errors(G2, H2, J2, fdG, fdH, fdJ, sums, case.g_struct, case.plan)
    m = _corrupted(case, G2, H2, J2)
    hi = float(np.max(err[~m])) if (~m).any() else 0.0
    lo = float(np.min(err[m])) if m.any() else np.inf
    print(f"precondition (delta {delta:g}): largest uncorrupted err {hi:.3e}, smallest corrupted err {lo:.3e}, {int(m.sum())} corrupted")
    assert hi <= TOL / 10 and lo >= 5 * TOL, (hi, lo)
    return m


def _ident(f):
    return (f.kind, f.row, f.col) if f.kind == "jac_sum" else (f.kind, f.index, f.row, f.col)


def _exp_ident(e):
    return (e[0], e[2], e[3]) if e[0] == "jac_sum" else e


def _assert_entry(case, f, G2, H2, J2, err, delta):
    """A reported entry carries the analytic value passed in, the clean run's FD value and NumPy's err of the two."""
    clean = case.clean(delta)
    if f.kind == "jac_sum":
        ents, half, hs = case.ref(delta)[3][(f.row, f.col)]
        an, hs = G2[np.array(ents)], np.array(hs)
        assert not f.located and _same(f.fd, half), (f, half)
        if not np.all(np.isfinite(an)):
            assert f.err == np.inf, f
            return
        ref = np.sum(an * hs)
        assert abs(f.analytic - ref) <= (len(ents) + 1) * EPS * np.sum(np.abs(an * hs)), (f, ref)
        e = np.abs(np.float64(f.analytic) - np.float64(f.fd)) / max(np.max(np.abs(an) * hs), np.max(hs))
        assert _same(f.err, e), (f, e)
        return
    vals, fd = {"jac": (G2, clean.jac_fd), "hess": (H2, clean.hess_fd), "grad": (J2, clean.jgrad_fd)}[f.kind]
    assert f.located and _same(f.analytic, vals[f.index]) and _same(f.fd, fd[f.index]), (f, vals[f.index], fd[f.index])
    assert _same(f.err, err[case.pos(f.kind, f.index)]), (f, err[case.pos(f.kind, f.index)])


def _verify(case, chk, G2, H2, J2, tol=TOL, max_report=20, delta=1e-5):
    """The whole DerivativeCheck against expected_report on NumPy's errors of the passed values and the clean run's FD
    values (sums: the restatement's).  The expected report knows nothing of blocks, waves or steps."""
    clean = case.clean(delta)
    err = errors(G2, H2, J2, clean.jac_fd, clean.hess_fd, clean.jgrad_fd, case.ref(delta)[3], case.g_struct, case.plan)
    exp = expected_report(err, tol, max_report, case.struct, case.plan)
    assert (chk.n_fail_jac, chk.n_fail_hess, chk.n_fail_grad) == tuple(exp["n_fail"][k] for k in ("jac", "hess", "grad"))
    assert chk.ok == (sum(exp["n_fail"].values()) == 0) and chk.tol == tol
    for kind, w, mx in (("jac", chk.worst_jac, chk.max_err_jac), ("hess", chk.worst_hess, chk.max_err_hess),
                        ("grad", chk.worst_grad, chk.max_err_grad)):
        if exp["worst"][kind] is None:
            assert w is None and mx == 0.0
            continue
        assert _ident(w) == _exp_ident(exp["worst"][kind]), (kind, w, exp["worst"][kind])
        assert _same(mx, max(w.err, 0.0)), (kind, mx, w)
        if w.kind != "jac_sum":   # (a sum's err follows the device's own sum an_j h_j: held to its bound by _assert_entry)
            assert _same(mx, exp["max_err"][kind]), (kind, mx, exp["max_err"][kind])
        _assert_entry(case, w, G2, H2, J2, err, delta)
    assert [_ident(f) for f in chk.failures] == [_exp_ident(e) for e in exp["failures"]]
    for f in chk.failures:
        _assert_entry(case, f, G2, H2, J2, err, delta)
    nums = [f.index for f in chk.failures if f.kind == "jac_sum"]
    assert all(a < b for a, b in zip(nums, nums[1:])) and all(0 <= s < case.nS for s in nums), nums
    return exp


def _run(case, G2, H2, J2, tol=TOL, max_report=20, delta=1e-5):
    _precondition(case, G2, H2, J2, delta)
    chk = case.check(G2, H2, J2, tol=tol, max_report=max_report, delta=delta)
    return chk, _verify(case, chk, G2, H2, J2, tol, max_report, delta)


def _assert_fd(case, chk, delta, long_rows=None):
    """jac_fd / hess_fd / jgrad_fd of a return_fd run against the restatement on the engine's evaluators."""
    fdG, fdH, fdJ, _, rnd = case.ref(delta)
    loc = case.plan.jac_located
    assert np.all(np.isnan(chk.jac_fd[~loc]))
    for name, got, ref in (("G~", chk.jac_fd[loc], fdG[loc]), ("grad J~", chk.jgrad_fd, fdJ)):
        ulps = np.max(np.abs(got - ref) / np.spacing(np.abs(ref))) if got.size else 0.0
        print(f"FD of {name}: at most {ulps:.2f} ulps from the restatement ({got.size} entries)")
        assert ulps <= 2.0, (name, ulps)
    bound = rnd["n"] * EPS * rnd["mag"] + 4 * EPS * np.abs(fdH)
    ratio = np.abs(chk.hess_fd - fdH) / np.maximum(bound, 1e-300)
    n_long = 0 if long_rows is None else int(long_rows.sum())
    worst_long = float(np.max(ratio[long_rows])) if n_long else 0.0
    most = int(rnd["n"][long_rows].max()) if n_long else 0
    msg = (f"FD of H~: at most {np.max(ratio):.3f} of the summation bound; {n_long} entries read from the long grad L rows "
           f"(up to {most} terms, chunks of {DERIV_CHUNK}), at most {worst_long:.3f} of their bound")
    print(msg)
    assert np.all(np.isfinite(chk.hess_fd)) and np.max(ratio) <= 1.0, msg
    return n_long


# ---- A. the report machinery: two_phase_transfer(K=40, order=4), three reduction blocks -------------------------------

def test_case_a_is_what_the_scenarios_assume(built):
    case = _case("two_phase_K40")
    chunk, nb = case.blocks()
    print(f"nG {case.nG} nS {case.nS} nH {case.nH} nJ {case.nJ} T {case.T}: {nb} blocks of {chunk}")
    assert (case.nG, case.nS, case.nH, case.nJ, case.T, nb, chunk) == (8560, 25, 3120, 6, 11711, 3, 3904)
    chk = case.clean()
    assert chk.ok and chk.failures == []
    _verify(case, chk, case.G, case.H, case.J)
    _precondition(case, case.G, case.H, case.J)
    _assert_fd(case, chk, 1e-5)
    # the engine's own analytic values (no override) pass as well, against the same FD values
    own = case.eng.check_derivatives(case.x, SIGMA, case.lam, return_fd=True)
    assert own.ok and max(own.max_err_jac, own.max_err_hess, own.max_err_grad) <= TOL / 10
    assert own.jac_fd.tobytes() == chk.jac_fd.tobytes() and own.hess_fd.tobytes() == chk.hess_fd.tobytes()


def _boundary_entries(case, variant):
    chunk, nb = case.blocks()
    assert nb == 3 and 2 * chunk < case.nG
    last_located = int(np.flatnonzero(case.plan.jac_located)[-1])
    g = {"every_block": [0, chunk - 1, chunk, 2 * chunk - 1, 2 * chunk, last_located, case.largest_term(0),
                         case.largest_term(case.nS - 1)],
         "middle_block_empty": [0, chunk - 1, 2 * chunk, last_located, case.largest_term(0), case.largest_term(case.nS - 1)],
         "middle_block_only": [chunk, chunk + 1000, 2 * chunk - 1]}[variant]
    if variant == "middle_block_only":
        return g, [], [], {1}
    return g, [0, case.nH - 1], [case.nJ - 1], {0, 1, 2} if variant == "every_block" else {0, 2}


@pytest.mark.parametrize("variant", ["every_block", "middle_block_empty", "middle_block_only"])
def test_failures_at_block_and_kind_boundaries(built, variant):
    """Positions 0, chunk - 1, chunk, 2 chunk - 1, 2 chunk and T - 1, the last located G~ entry, the first and the last
    sum, H~ entries 0 and nH - 1; then the same without a failure in the middle block; then the middle block alone."""
    case = _case("two_phase_K40")
    chunk, _ = case.blocks()
    g, h, j, blocks = _boundary_entries(case, variant)
    G2, H2, J2 = _scenario(case, g, h, j)
    m = _precondition(case, G2, H2, J2)
    assert set((np.flatnonzero(m) // chunk).tolist()) == blocks
    if variant != "middle_block_only":
        assert m[[0, chunk - 1, 2 * chunk, case.nG, case.nG + case.nS - 1, case.pos("hess", 0), case.pos("hess", case.nH - 1),
                  case.T - 1]].all() and m[chunk] == (variant == "every_block")
    chk = case.check(G2, H2, J2, max_report=64)
    exp = _verify(case, chk, G2, H2, J2, max_report=64)
    assert len(chk.failures) == int(m.sum()) == len(exp["failures"])


def _run_of_70(case):
    """70 consecutive located G~ entries of the middle block over a 64-lane boundary and a 256-entry step of its scan."""
    chunk, _ = case.blocks()
    loc = case.plan.jac_located
    for step in range(chunk + 256, 2 * chunk - 64, 256):   # (steps and lanes count from the block's first position)
        s = step - 66
        if loc[s:s + 70].all():
            assert s < step - 64 < step < s + 70
            return s
    raise AssertionError("no run of 70 located entries over a step of the middle block")


@pytest.mark.parametrize("max_report", [0, 1, 5, 63, 64, 1000])
def test_seventy_failures_and_the_cap(built, max_report):
    case = _case("two_phase_K40")
    s = _run_of_70(case)
    G2, H2, J2 = _scenario(case, range(s, s + 70), [5, 6])
    chk, exp = _run(case, G2, H2, J2, max_report=max_report)
    assert (chk.n_fail_jac, chk.n_fail_hess, chk.n_fail_grad, chk.n_fail) == (70, 2, 0, 72) and not chk.ok
    assert len(chk.failures) == min(max_report, 64)
    assert [f.index for f in chk.failures] == (list(range(s, s + 70)) + [5, 6])[:min(max_report, 64)]


def test_failures_straddling_two_blocks(built):
    """30 failures at the end of one block, 50 at the start of the next: the cap of the list falls inside the second."""
    case = _case("two_phase_K40")
    chunk, _ = case.blocks()
    b = next(b for b in (chunk, 2 * chunk) if case.plan.jac_located[b - 30:b + 50].all())
    G2, H2, J2 = _scenario(case, range(b - 30, b + 50))
    for max_report in (64, 40, 30, 31):
        chk, _ = _run(case, G2, H2, J2, max_report=max_report)
        assert chk.n_fail_jac == 80 and [f.index for f in chk.failures] == list(range(b - 30, b - 30 + max_report))
    # below the cap: the second block ranks the failures of two of its waves behind the 30 of the first block
    idx = list(range(b - 30, b + 10)) + list(range(b + 64, b + 74))
    assert case.plan.jac_located[idx].all()
    chk, _ = _run(case, *_scenario(case, idx), max_report=64)
    assert [f.index for f in chk.failures] == idx


def test_non_finite_values(built):
    case = _case("two_phase_K40")
    loc = np.flatnonzero(case.plan.jac_located)
    a, b = int(loc[loc.size // 3]), int(loc[2 * loc.size // 3])
    t = case.largest_term(case.nS // 2)
    G2, H2, J2 = case.G.copy(), case.H.copy(), case.J.copy()
    G2[a], G2[b], G2[t] = np.inf, np.nan, np.nan
    H2[case.nH // 2] = -np.inf
    J2[2] = np.nan
    # (the precondition holds with err = +inf for the five corrupted positions)
    chk, exp = _run(case, G2, H2, J2)
    assert (chk.n_fail_jac, chk.n_fail_hess, chk.n_fail_grad) == (3, 1, 1)
    assert chk.max_err_jac == chk.max_err_hess == chk.max_err_grad == np.inf
    assert _ident(chk.worst_jac) == ("jac", a, case.g_struct[0][a], case.g_struct[1][a]) and a < b
    assert np.isposinf(chk.worst_jac.analytic) and [f.err for f in chk.failures] == [np.inf] * 5
    assert [f.kind for f in chk.failures] == ["jac", "jac", "jac_sum", "hess", "grad"]
    assert np.isnan(chk.failures[1].analytic) and chk.failures[3].analytic == -np.inf and np.isnan(chk.failures[4].analytic)
    assert (chk.failures[2].row, chk.failures[2].col) == case.keys[case.nS // 2]
    # the NaN in the highest block only: the lower, finite failure is not the worst
    G3 = _bump(case.G, [a])
    G3[b] = np.nan
    chk, _ = _run(case, G3, case.H, case.J)
    assert chk.worst_jac.index == b and chk.max_err_jac == np.inf and chk.n_fail_jac == 2


def _tied(an, fd, want, start=0):
    """`want` entries i >= start with |an| < 0.5 whose value fd[i] + 2^-9 gives err = 2^-9 exactly, in index order."""
    E = 2.0 ** -9
    v = fd + E
    ok = (np.abs(an) < 0.5) & (np.abs(v) < 1.0) & (np.abs(v - fd) == E)
    idx = np.flatnonzero(ok)
    idx = idx[idx >= start]
    assert idx.size >= want
    return idx, v


def test_ties_report_the_lowest_index(built):
    """Bit-equal finite errors (2^-9): G~ entries of the first and the last block tie across blocks, two H~ entries
    within one block; a smaller failure stands before each of them."""
    case = _case("two_phase_K40")
    chunk, _ = case.blocks()
    clean = case.clean()
    loc = case.plan.jac_located
    gi, gv = _tied(np.where(loc, case.G, 1.0), np.where(loc, clean.jac_fd, 0.0), 3, start=10)
    g_lo, g_mid, g_hi = int(gi[0]), int(gi[gi.size // 2]), int(gi[-1])
    assert g_lo < chunk <= g_mid < 2 * chunk <= g_hi
    hi_, hv = _tied(case.H, clean.hess_fd, 2, start=10)
    h_lo, h_hi = int(hi_[0]), int(hi_[1])
    G2, H2, J2 = _scenario(case, [3], [4])   # (smaller failures, err about 1e-3, at lower indices)
    for i in (g_lo, g_mid, g_hi):
        G2[i] = gv[i]
    for i in (h_lo, h_hi):
        H2[i] = hv[i]
    chk, exp = _run(case, G2, H2, J2)
    assert chk.max_err_jac == chk.max_err_hess == 2.0 ** -9
    assert chk.worst_jac.index == g_lo and chk.worst_hess.index == h_lo
    assert [f.err for f in chk.failures if f.index in (g_lo, g_mid, g_hi, h_lo, h_hi)] == [2.0 ** -9] * 5
    # the tie the other way round in block order: only the later blocks hold the maximum
    G3 = G2.copy()
    G3[g_lo] = case.G[g_lo]
    chk, _ = _run(case, G3, H2, J2)
    assert chk.worst_jac.index == g_mid


def test_tol_is_strict(built):
    case = _case("two_phase_K40")
    s = _run_of_70(case)
    G2, H2, J2 = _scenario(case, range(s, s + 70), [5, 6])
    base = case.check(G2, H2, J2, max_report=64)
    errs = sorted(f.err for f in base.failures)
    e = errs[len(errs) // 2]
    larger = sum(1 for f in base.failures if f.err > e)
    at = case.check(G2, H2, J2, tol=e, max_report=64)
    _verify(case, at, G2, H2, J2, tol=e, max_report=64)
    assert all(f.err > e for f in at.failures) and e not in [f.err for f in at.failures]
    below = case.check(G2, H2, J2, tol=float(np.nextafter(e, 0.0)), max_report=64)
    _verify(case, below, G2, H2, J2, tol=float(np.nextafter(e, 0.0)), max_report=64)
    n_equal = sum(1 for f in base.failures if f.err == e)
    assert below.n_fail == at.n_fail + n_equal and n_equal >= 1 and at.n_fail >= larger > 0
    assert e in [f.err for f in below.failures]


def test_reports_of_many_failures_are_reproducible(built):
    case = _case("two_phase_K40")
    s = _run_of_70(case)
    G2, H2, J2 = _scenario(case, range(s, s + 70), [5, 6])
    a = case.check(G2, H2, J2, max_report=64)
    b = case.check(G2, H2, J2, max_report=64)
    assert a == b and len(a.failures) == 64
    for f, g in zip(a.failures, b.failures):
        assert all(_bits([getattr(f, k)])[0] == _bits([getattr(g, k)])[0] for k in ("analytic", "fd", "err"))


def test_one_nan_in_lagrange(built):
    """A NaN multiplier of one defect row: exactly the H~ entries whose grad L row has a G~ entry in that row get
    err = inf, on the device as in the restatement; G~ and grad J~ are judged as before."""
    case = _case("two_phase_K40")
    gr, gc = case.g_struct
    pl = case.eng.layout.phases[1]
    r = pl.c_off + 7
    assert pl.c_off <= r < pl.c_path_off
    lam = case.lam.copy()
    lam[r] = np.nan
    hit = np.isin(case.grad_l_row(), gc[gr == r])
    assert 0 < hit.sum() < case.nH
    fdG, fdH, fdJ, sums = restate(case.fns, case.plan, case.g_struct, case.h_struct, case.jcols, case.x, SIGMA, lam)
    np.testing.assert_array_equal(np.isnan(fdH), hit)
    err = errors(case.G, case.H, case.J, fdG, fdH, fdJ, sums, case.g_struct, case.plan)
    exp = expected_report(err, TOL, 20, case.struct, case.plan)
    assert exp["n_fail"] == dict(jac=0, hess=int(hit.sum()), grad=0)
    chk = case.eng.check_derivatives(case.x, SIGMA, lam, jac_values=case.G, hess_values=case.H, jgrad_values=case.J,
                                     return_fd=True)
    clean = case.clean()
    np.testing.assert_array_equal(np.isnan(chk.hess_fd), hit)
    assert chk.hess_fd[~hit].tobytes() == clean.hess_fd[~hit].tobytes()
    assert chk.jac_fd.tobytes() == clean.jac_fd.tobytes() and chk.jgrad_fd.tobytes() == clean.jgrad_fd.tobytes()
    assert (chk.n_fail_jac, chk.n_fail_hess, chk.n_fail_grad) == (0, int(hit.sum()), 0)
    assert chk.max_err_hess == np.inf and (chk.max_err_jac, chk.max_err_grad) == (clean.max_err_jac, clean.max_err_grad)
    assert [_ident(f) for f in chk.failures] == [_exp_ident(e) for e in exp["failures"]]
    assert _ident(chk.worst_hess) == _exp_ident(exp["worst"]["hess"]) and all(f.err == np.inf for f in chk.failures)


# ---- B. long columns: grad L rows summed in chunks ------------------------------------------------------------------

# (engine, delta, sizes of the columns of G~ longer than DERIV_CHUNK -- or of the longest -- , chunks of the longest, its last chunk)
LONG = {
    "brachistochrone_K113": ("brachistochrone_K113", 1e-5, 1017, 1, 1017),
    "brachistochrone_K114": ("brachistochrone_K114", 1e-5, 1026, 2, 2),
    "brachistochrone_K230": ("brachistochrone_K230", 1e-5, 2070, 3, 22),
    "brachistochrone_K230_delta_1e-4": ("brachistochrone_K230", 1e-4, 2070, 3, 22),
    "time_coupled_K150": ("time_coupled_K150", 1e-5, 2113, 3, 65),
}


@pytest.mark.parametrize("name", list(LONG))
def test_long_columns(built, name):
    """One chunk just under DERIV_CHUNK, a second chunk of 2 entries, three chunks with a last one shorter than a wave,
    five long columns in two phases (some with a grad J~ term): the check is clean, every FD value is the
    restatement's within the bounds, and the largest H~ entry read from the longest rows is found when corrupted."""
    key, delta, longest, n_chunks, last_chunk = LONG[name]
    case = _case(key)
    sizes = case.col_sizes()
    assert sizes.max() == longest and -(-longest // DERIV_CHUNK) == n_chunks and longest - (n_chunks - 1) * DERIV_CHUNK == last_chunk
    long_cols = np.flatnonzero(sizes > DERIV_CHUNK) if n_chunks > 1 else np.flatnonzero(sizes == longest)
    if key == "time_coupled_K150":
        assert long_cols.size == 5 and sizes[long_cols].min() == 1211
        assert 0 < np.isin(case.jcols, long_cols).sum() < long_cols.size
    long_rows = np.isin(case.grad_l_row(), long_cols)
    own = case.eng.check_derivatives(case.x, SIGMA, case.lam, delta=delta)
    assert own.ok, (own.max_err_jac, own.max_err_hess, own.max_err_grad, own.failures[:3])
    chk = case.clean(delta)
    assert chk.ok
    n_long = _assert_fd(case, chk, delta, long_rows)
    assert n_long > 0, "no H~ entry is read from a long row"
    print(f"{name}: columns {sizes[long_cols].tolist()}, {n_long} H~ entries read from them")
    if key.startswith("brachistochrone"):
        assert n_long == 4
    else:
        assert n_long == 45
    e = int(np.flatnonzero(long_rows)[np.argmax(np.abs(case.H[long_rows]))])
    G2, H2, J2 = _scenario(case, h=[e])
    chk, _ = _run(case, G2, H2, J2, delta=delta)
    assert chk.n_fail == 1 and _ident(chk.failures[0]) == ("hess", e, case.h_struct[0][e], case.h_struct[1][e])


# ---- C. completeness on the device ----------------------------------------------------------------------------------

def test_every_single_entry_is_reported_as_itself(built):
    """Every entry of G~, H~ and grad J~ of two_phase_transfer() at its default mesh (T = 935; 917 entries, all of them:
    no thinning) corrupted in turn, the values resident on the device: a located entry is the one failure, with its
    kind, index, row and col; a sum term fails its (row, colour) sum and nothing else."""
    import torch
    case = _case("two_phase_default")
    assert case.T == 935 and case.nG + case.nH + case.nJ == 917
    fdG, fdH, fdJ, sums, _ = case.ref()
    loc = case.plan.jac_located
    gr, gc = case.g_struct
    hr, hc = case.h_struct
    # the precondition, for all 917 scenarios
    clean = errors(case.G, case.H, case.J, fdG, fdH, fdJ, sums, case.g_struct, case.plan)
    assert np.max(clean) <= TOL / 10

    def bumped(v):
        return v + 1e-3 * np.maximum(1.0, np.abs(v))

    with np.errstate(invalid="ignore"):
        hit = np.concatenate([(np.abs(bumped(v) - fd) / np.maximum(1.0, np.abs(bumped(v))))[m] for v, fd, m in
                              ((case.G, fdG, loc), (case.H, fdH, slice(None)), (case.J, fdJ, slice(None)))])
    lo = float(np.min(hit))
    for e in np.flatnonzero(~loc):
        err = errors(_bump(case.G, [e]), case.H, case.J, fdG, fdH, fdJ, sums, case.g_struct, case.plan)
        s = case.pos("jac_sum", case.sum_of(e))
        lo = min(lo, float(err[s]))
        err[s] = 0.0
        assert np.max(err) <= TOL / 10
    print(f"precondition: largest clean err {np.max(clean):.3e}, smallest corrupted err over 917 scenarios {lo:.3e}")
    assert lo >= 5 * TOL
    dev = torch.device("cuda", 0)
    dx, dl = (torch.as_tensor(a, dtype=torch.float64, device=dev) for a in (case.x, case.lam))
    host = {"jac": case.G, "hess": case.H, "grad": case.J}
    vals = {k: torch.as_tensor(v, dtype=torch.float64, device=dev).clone() for k, v in host.items()}
    wrong = []
    for kind, rows, cols in (("jac", gr, gc), ("hess", hr, hc), ("grad", np.full(case.nJ, -1), case.jcols)):
        for e in range(host[kind].size):
            v = float(host[kind][e])
            vals[kind][e] = v + 1e-3 * max(1.0, abs(v))
            chk = case.eng.check_derivatives(dx, SIGMA, dl, jac_values=vals["jac"], hess_values=vals["hess"],
                                             jgrad_values=vals["grad"], max_report=3)
            vals[kind][e] = v
            if kind == "jac" and not loc[e]:
                want = ("jac_sum", int(gr[e]), int(case.plan.colour[gc[e]]))
            else:
                want = (kind, e, int(rows[e]), int(cols[e]))
            if chk.ok or chk.n_fail != 1 or len(chk.failures) != 1 or _ident(chk.failures[0]) != want:
                wrong.append((want, chk.n_fail, [_ident(f) for f in chk.failures]))
    assert wrong == [], (len(wrong), wrong[:5])
    assert case.eng.check_derivatives(dx, SIGMA, dl, jac_values=vals["jac"], hess_values=vals["hess"],
                                      jgrad_values=vals["grad"]).ok


# ---- D. one entry per category beyond the default mesh --------------------------------------------------------------

@pytest.mark.parametrize("key", ["time_coupled_K150", "time_coupled_mixed"])
def test_categories_on_multi_block_meshes_with_long_columns(built, key):
    case = _case(key)
    assert case.blocks()[1] > 1 and case.nS > 0 and case.col_sizes().max() > DERIV_CHUNK
    cats, gr, gc, hr, hc = _categories(case.eng, case.plan, case.G, case.H)
    cats = cats + [("grad J~ non-zero", "grad", int(np.argmax(np.abs(case.J)))),
                   ("sum term", "jac", int(np.flatnonzero(~case.plan.jac_located)[np.argmax(np.abs(case.G[~case.plan.jac_located]))]))]
    for cat, kind, e in cats:
        G2, H2, J2 = _scenario(case, **{{"jac": "g", "hess": "h", "grad": "j"}[kind]: [e]})
        chk, _ = _run(case, G2, H2, J2)
        assert not chk.ok and chk.n_fail == 1 and len(chk.failures) == 1, (cat, chk.n_fail, chk.failures)
        f = chk.failures[0]
        if cat == "sum term":
            assert _ident(f) == ("jac_sum", gr[e], case.plan.colour[gc[e]]), (cat, f)
        elif kind == "grad":
            assert _ident(f) == ("grad", e, -1, case.jcols[e]), (cat, f)
        else:
            rows, cols = (gr, gc) if kind == "jac" else (hr, hc)
            assert _ident(f) == (kind, e, rows[e], cols[e]), (cat, f)


def test_radau_brachistochrone_entries(built):
    """The Radau brachistochrone has defect rows only (no path, integral or endpoint row, no parameter column, no sum), so
    the categories above do not all exist; its largest G~ entry of a node column and of the t_F column, its largest H~
    entry on the diagonal, off it and in the t_F row, and every grad J~ non-zero are corrupted in turn."""
    case = _case("brachistochrone_radau")
    gr, gc = case.g_struct
    hr, hc = case.h_struct
    lay = case.eng.layout
    pl = lay.phases[0]
    loc = case.plan.jac_located

    def pick(mask, vals):
        idx = np.flatnonzero(mask)
        assert idx.size
        return int(idx[np.argmax(np.abs(vals[idx]))])

    t_cols = (gc >= pl.t_off) & (gc < pl.t_off + pl.n_t)
    assert lay.c_end_off == case.eng.num_c == pl.c_path_off and loc.all() and case.nS == 0   # defect rows only, no sum
    todo = [("g", pick(~t_cols, case.G)), ("g", pick(t_cols, case.G)), ("h", pick(hr == hc, case.H)),
            ("h", pick(hr != hc, case.H)), ("h", pick((hr >= pl.t_off) | (hc >= pl.t_off), case.H))]
    todo += [("j", i) for i in range(case.nJ)]
    for which, e in todo:
        G2, H2, J2 = _scenario(case, **{which: [e]})
        chk, _ = _run(case, G2, H2, J2)
        assert chk.n_fail == 1 and chk.failures[0].index == e and chk.failures[0].kind == {"g": "jac", "h": "hess", "j": "grad"}[which]
