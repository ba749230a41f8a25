"""The solution of one NLP as the user sees it: node values, and dense output sampled on the device.

Restates ``CasadiSolution`` (pycollo/solution/casadi_solution.py:15-86) and the interpolants of ``SolutionABC``
(pycollo/solution/solution_abc.py:60-142).  The attribute names and the per-phase tuples are the reference's
(``objective``, ``initial_time``, ``final_time``, ``state``, ``state_derivative``, ``control``, ``integral``, ``time``,
``parameter``); ``node_time`` is the reference's ``_time_`` and ``tau`` its ``tau``.  The reference fits
``K (n_y + n_u)`` NumPy polynomials in a Python loop and leaves evaluating them to the caller; here one kernel per phase
forms every section's Legendre coefficients (``pc_sol_fit_p<i>``) and a second evaluates them at any number of times in
any order (``pc_sol_sample_p<i>``).

What the interpolant is, per section k with n nodes, section variable c in [-1, 1], stretch = (tF - t0) / 2:

* Lobatto: ``ydot`` is the degree n-1 interpolant of f(y, u, q, t, s) at the section's nodes; Radau
  (solution_abc.py:104-142): degree n-2 through the first n-1 nodes.  ``u`` is the degree n-1 interpolant of the node
  controls through all n nodes (the reference fits it in a monomial basis, solution_abc.py:98-100; here it is held in
  the Legendre basis like ``ydot``).
* ``y(tau) = y(tau_k) + stretch * int_{tau_k}^{tau} ydot``, with ``y(tau_k)`` the NLP's own value at the section's first
  node.  **At a node, y is this integrated form**: it differs from the node's NLP value (``state``) by the residual
  of that defect row, which is zero only to the NLP tolerance.
* a query at an interior section boundary belongs to the section on its right; the end of the phase to the last one.

It reports the NLP's variables: variables eliminated as constants are not re-inserted (the scope of
``MeshIteration.solution()``).

Costates and the Hamiltonian (``multipliers=``; no reference counterpart).  Per phase: N is the number of
nodes; section k has n_k nodes and its first node is s_k; h_k = tau[s_{k+1}] - tau[s_k]; A^(n) is the (n-1) x n
integration table.  Defect row r of state a in section k is global row s_k + r of that state's N - 1 rows; its value
is c~ = W_a (y_{s_k} - y_{s_k+r+1} + stretch h_k sum_j A^(n_k)[r][j] f_a(node s_k + j)).  w is the objective scaling,
W the per-OCP-row constraint scaling the handle holds.  Then:

* Lam = W lam~ / w for the defect rows (Lam_a) and for the integral rows (Lam_q): the multipliers of the unscaled rows
  for the unscaled objective.
* omega_j = sum over the one or two sections containing node j of h_k A^(n_k)[n_k - 2][pos_k(j)].  (The last row of A
  sums to 1 under both methods and is the Lobatto weights; the Radau weight table sums to 2.)
* p_a(j) = ( sum_{k contains j} h_k sum_{r=0}^{n_k-2} Lam_a[s_k + r] A^(n_k)[r][pos_k(j)] ) / omega_j where
  omega_j != 0.  A node with omega_j = 0 is the Radau phase-final node only (the table entry is an exact zero: the
  node is not collocated); there p_a(N - 1) = Lam_a[N - 2], the multiplier of the phase's last defect row.
* nu_m = -Lam_q[m]: the weight of integrand m in the Hamiltonian (1 when J = q).
* H(j) = sum_a p_a(j) f_a(j) + sum_m nu_m g_m(j), f and g the dynamics and integrands at the node's (y, u, q, t, s).
  No path-constraint term: by complementarity it is zero at a solution.  At the Radau phase-final node, whose control
  the NLP does not determine, H is NaN.
* Summation order: lower section first, rows ascending, then the upper section, one division at the end.  A shared
  node is computed by both of its sections in exactly this order (bit-equal); the section the node opens writes it.
* Between the nodes p_a on section k is the degree n_k - 1 interpolant through the section's n_k node values, held as
  Legendre coefficients formed with the ``C_u`` table like u; H(t) is formed from the interpolated p(t) and the model
  at the interpolated (y(t), u(t)), the route by which ``sample(..., residual=True)`` forms f.

Path and bound multipliers, the gradients of the augmented Hamiltonian (``bound_multipliers=``; no reference counterpart;
DESIGN 8f).  With stretch, omega_j, w, W and Lam as above, V the variable scaling and z~ = zu - zl the signed bound
multipliers of the scaled NLP's ``num_x`` variables:

* mu_i(j) = W_p,i lam~[c_path_off + i N + j] / (w stretch omega_j): the multiplier function of path row i.
* zeta_v(j) = z~[x_off + v N + j] / (w V_v stretch omega_j), v over the n_y states and then the n_u controls.  A state's
  bound at nodes 0 and N - 1 is the endpoint bound: zeta_y is 0 there and z~ / (w V_a) is ``endpoint_bound_multiplier``
  [n_y][2].
* H_z(j) = sum_a p_a df_a/dz + sum_i mu_i dp_i/dz + sum_m rho nu_m dg_m/dz for a node variable z, from the generated
  first partials in table order.  rho is the weight the NLP's integral rows give a node over omega_j: 1 under Lobatto, 2
  under Radau, whose rule weights sum to 2 where the last row of A sums to 1 (``hamiltonian`` keeps nu_m alone).  At the
  Radau phase-final node mu, zeta_u and H_z are NaN.
* ``control_stationarity`` = H_u + zeta_u and ``costate_defect`` = D_a / (stretch omega) + H_y + zeta_y with
  D_a(j) = sum_{r < n_k - 1} Lam_a[s_k + r] if j opens section k, minus Lam_a[j - 1] if j >= 1: the dual residual of the
  scaled NLP over w V stretch omega, column by column.
* Between the nodes mu and zeta are held like u and p (the phase's last section: formed with the ydot table, which
  under Radau leaves the final node out); dp/dt = 2 / (h_k stretch) d/dc of the costate's Legendre series; H_y(t), H_u(t)
  are formed at the interpolated (y(t), u(t)) with p(t), mu(t) and rho nu.  ``costate_residual`` = dp + H_y + zeta_y.
* All of it is formed on first use (``pc_sol_multipliers_p<i>``, one launch per phase).

Propagation (:meth:`Solution.propagate`; no reference counterpart): the dynamics integrated forward under the
solution's control interpolant by the Dormand-Prince 5(4) pair, restarted from the NLP's own state at chosen nodes
(``pc_sol_propagate_p<i>``, one lane per restart).  ``defect = y_arrive - state`` is what the collocation residual
accumulates to over a node interval, a section or the whole phase.  :meth:`Solution.propagate_dense` (DESIGN 8g;
``pc_sol_propagate_dense_p<i>``) takes the same steps, carries the phase's integrals beside the state
(``integral_defect`` = what they come to, less the NLP's integral variables) and samples the propagated path between the
nodes by the pair's continuous extension.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools

import numpy as np

from .quadrature import LOBATTO, RADAU, QuadratureTables

PC_SOLUTION_TAU = 1
PC_SOLUTION_EXTRAPOLATE = 2
_MP_DIGITS = 60


def section_points(quad: QuadratureTables, n: int) -> np.ndarray:
    """The n node abscissae of a section of order n on [-1, 1].  Lobatto: the rule's points.  Radau: its n-1 points
    and the section's end, +1 (the rule's trailing placeholder, pycollo/quadrature.py:117-134, is not a node:
    pycollo/mesh.py:255-265 drops it and the next section's first node closes the section)."""
    x = np.array(quad.points(int(n)), dtype=np.float64)
    if quad.method == RADAU:
        x[-1] = 1.0
    return x


def _mp_legvander(points, deg):
    """V[i][k] = P_k(x_i), k = 0 .. deg, in mpmath arithmetic (the doubles x_i are taken as exact)."""
    import mpmath as mp
    V = mp.matrix(len(points), deg + 1)
    for i, xi in enumerate(points):
        x = mp.mpf(float(xi))
        p0, p1 = mp.mpf(1), x
        for k in range(deg + 1):
            V[i, k] = p0
            p0, p1 = p1, ((2 * k + 3) * x * p1 - (k + 1) * p0) / (k + 2)
    return V


def exact_tables(method: str, n: int):
    """(C_dy, C_u) as mpmath matrices, n x n: node values of a section -> Legendre coefficients of the interpolant.
    C_u = inverse of the Legendre Vandermonde at the n nodes; C_dy the same for Lobatto, and for Radau the inverse at
    the first n-1 nodes, bordered by a zero row and column (degree n-2, last node unused)."""
    import mpmath as mp
    quad = QuadratureTables(method)
    x = section_points(quad, n)
    with mp.workdps(_MP_DIGITS):
        Cu = mp.inverse(_mp_legvander(x, n - 1))
        if method == LOBATTO:
            Cd = Cu.copy()
        else:
            Cd = mp.zeros(n, n)
            inner = mp.inverse(_mp_legvander(x[:-1], n - 2))
            for i in range(n - 1):
                for j in range(n - 1):
                    Cd[i, j] = inner[i, j]
    return Cd, Cu


@functools.lru_cache(maxsize=None)
def solution_tables(method: str, n: int):
    """(C_dy, C_u) of order n as float64 arrays [n][n]: the exact tables, rounded once.  (A float64
    ``inv(legvander)`` costs up to several hundred eps sum |l_i(t)||f_i| in the sampled values at orders 8-19; the
    rounded exact tables keep it near one.)  Cached per (method, order)."""
    Cd, Cu = exact_tables(method, int(n))
    to = lambda M: np.array([[float(M[i, j]) for j in range(M.cols)] for i in range(M.rows)], dtype=np.float64)   # noqa: E731
    a, b = to(Cd), to(Cu)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


PROPAGATE_MAX_STEPS = 1 << 20           # csrc/pc_args.h PC_SOL_PROP_MAX_STEPS
PROPAGATE_METHODS = ("dopri5", "sdirk4")
PROPAGATE_STIFF_MAX_NY = 11             # csrc/pc_args.h PC_SOL_STIFF_MAX_NY
PROPAGATE_STIFF_MAX_NEWTON = 32         # csrc/pc_args.h PC_SOL_STIFF_MAX_NEWTON


@dataclasses.dataclass
class Propagation:
    """What :meth:`Solution.propagate` returns (NumPy arrays, or torch tensors on the device of the call's inputs).
    ``y`` [n_y][N]: column j >= 1 is the state arriving at node j from the segment that contains the interval
    (j - 1, j), column 0 is y(0).  ``defect`` = ``y`` - the NLP's node states; ``relative_defect`` = ``defect`` over
    the state's scale V_a of the engine's scaling; ``terminal_defect`` [n_y]: the last column of ``defect``.
    ``accepted`` / ``rejected`` [N]: the steps of the interval that ends at the node.  ``segments`` [n_seg + 1]: the
    node every segment starts at, and N - 1.  ``status`` [n_seg]: -1, or the first node of the interval that used up
    ``max_steps`` (arrivals from there to the segment's end are NaN); ``ok`` = ``status == -1``.
    ``newton_rejected`` / ``newton_iterations`` [N] (``method="sdirk4"``; ``None`` otherwise): the rejected steps of the
    interval whose cause was a Newton failure (they count in ``rejected`` too), and all its Newton iterations."""
    y: object
    defect: object
    relative_defect: object
    accepted: object
    rejected: object
    segments: np.ndarray
    status: object
    ok: object
    terminal_defect: object
    newton_rejected: object = None
    newton_iterations: object = None


@dataclasses.dataclass
class DensePropagation:
    """What :meth:`Solution.propagate_dense` returns (NumPy arrays, or torch tensors on the device of the call's inputs).
    ``y``, ``defect``, ``relative_defect``, ``terminal_defect``, ``accepted``, ``rejected``, ``segments``, ``status``,
    ``ok``: as in :class:`Propagation`.  ``q`` [n_q][N]: column j >= 1 is the integral of the integrands from the first
    node of the segment that contains the interval (j - 1, j) to node j, column 0 is 0.  ``integral`` [n_q]: the sum of
    ``q`` over the segments' last nodes, the whole phase's integrals; ``integral_defect`` = ``integral`` - the NLP's
    (unscaled) integral variables.  ``tau`` [Q]: the queries as abscissae; ``y_dense`` [n_y][Q], ``q_dense`` [n_q][Q]
    (the integral from the first node of the query's segment) and ``u_dense`` [n_u][Q] (the control interpolant,
    :meth:`Solution.sample`'s) in the caller's query order."""
    y: object
    defect: object
    relative_defect: object
    accepted: object
    rejected: object
    segments: np.ndarray
    status: object
    ok: object
    terminal_defect: object
    q: object
    integral: object
    integral_defect: object
    tau: np.ndarray
    y_dense: object
    q_dense: object
    u_dense: object


def dense_query_tau(t, tau, t0: float, tF: float) -> np.ndarray:
    """The queries of ``Solution.propagate_dense`` as abscissae: ``tau`` itself, or ``t`` mapped as the sampling kernel
    maps it (a time within 8 eps in tau of the phase's ends is the end).  ``ValueError`` for a NaN and for a query
    outside the phase; both ``None``: no queries."""
    if t is None and tau is None:
        return np.zeros(0)
    q, is_tau = normalise_query(t, tau)
    if _is_torch(q):
        q = q.detach().cpu().numpy()
    q = np.ascontiguousarray(q, dtype=np.float64)
    if np.isnan(q).any():
        raise ValueError("a query is NaN")
    if not is_tau:
        q = (q - 0.5 * (t0 + tF)) / (0.5 * (tF - t0))
        near = np.abs(q) <= 1.0 + END_SLACK
        q = np.where(near, np.clip(q, -1.0, 1.0), q)
    if q.size and not (q.min() >= -1.0 and q.max() <= 1.0):
        raise ValueError(f"queries reach tau = [{float(q.min())!r}, {float(q.max())!r}], outside the phase's [-1, 1]: a "
                         f"propagated path is not extrapolated")
    return np.ascontiguousarray(q)


def _sum_ascending(cols: np.ndarray) -> np.ndarray:
    """sum over the columns, first to last, one addition per column (``np.sum`` adds pairwise)"""
    cols = np.asarray(cols, dtype=np.float64)
    return np.cumsum(cols, axis=1)[:, -1] if cols.shape[1] else np.zeros(cols.shape[0])


def check_integral_atol(integral_atol, n_q: int):
    """``None``, or ``n_q`` finite positive numbers as a contiguous float64 array (csrc/pc_propagate_plan.hpp makes the
    same refusal)."""
    if integral_atol is None:
        return None
    if _is_torch(integral_atol):
        integral_atol = integral_atol.detach().cpu().numpy()
    try:
        ia = np.ascontiguousarray(np.broadcast_to(np.asarray(integral_atol, dtype=np.float64), (n_q,)))
    except ValueError:
        raise ValueError(f"integral_atol must be a number or {n_q} numbers") from None
    if not (np.all(np.isfinite(ia)) and np.all(ia > 0)):
        raise ValueError("every integral_atol must be finite and positive")
    return ia


def propagation_segments(restart, s, N: int) -> np.ndarray:
    """The segment list [n_seg + 1] of ``Solution.propagate``'s ``restart``: "nodes" (every node), "sections" (the
    section starts ``s`` [K + 1]), "phase" (one segment), or an array of node indices, which must be strictly
    ascending from 0 to N - 1."""
    if isinstance(restart, str):
        if restart == "nodes":
            return np.arange(N, dtype=np.int32)
        if restart == "sections":
            return np.ascontiguousarray(s, dtype=np.int32)
        if restart == "phase":
            return np.array([0, N - 1], dtype=np.int32)
        raise ValueError(f'restart must be "nodes", "sections", "phase" or an array of node indices, not {restart!r}')
    if _is_torch(restart):
        restart = restart.detach().cpu().numpy()
    seg = np.asarray(restart)
    if seg.ndim != 1 or seg.size < 2 or not np.issubdtype(seg.dtype, np.integer):
        raise ValueError("a segment list is a one-dimensional integer array of at least two node indices")
    if seg[0] != 0 or seg[-1] != N - 1 or np.any(np.diff(seg.astype(np.int64)) <= 0):
        raise ValueError(f"a segment list must be strictly ascending from node 0 to node {N - 1}")
    return np.ascontiguousarray(seg, dtype=np.int32)


def check_propagate_tolerances(substeps, rtol, atol, max_steps):
    """The refusals of ``Solution.propagate`` (csrc/pc_propagate_plan.hpp makes the same ones)."""
    if substeps is not None and (int(substeps) != substeps or not 1 <= substeps <= PROPAGATE_MAX_STEPS):
        raise ValueError("substeps must be None (adaptive) or an integer in [1, 2^20]")
    if substeps is None and not (np.isfinite(rtol) and rtol > 0):
        raise ValueError("rtol must be finite and positive")
    if not (np.all(np.isfinite(atol)) and np.all(atol > 0)):
        raise ValueError("every atol must be finite and positive")
    if int(max_steps) != max_steps or not 1 <= max_steps <= PROPAGATE_MAX_STEPS:
        raise ValueError("max_steps must be an integer in [1, 2^20]")


def check_propagate_method(method, newton_max, rtol, n_y: int):
    """The further refusals of ``Solution.propagate(method=...)`` (csrc/pc_propagate_plan.hpp makes the same ones for
    the implicit method)."""
    if method not in PROPAGATE_METHODS:
        raise ValueError(f"method must be one of {PROPAGATE_METHODS}, not {method!r}")
    if method == "dopri5":
        return
    if int(newton_max) != newton_max or not 1 <= newton_max <= PROPAGATE_STIFF_MAX_NEWTON:
        raise ValueError(f"newton_max must be an integer in [1, {PROPAGATE_STIFF_MAX_NEWTON}]")
    if not (np.isfinite(rtol) and rtol > 0):
        raise ValueError('rtol must be finite and positive (method="sdirk4" reads it in both modes)')
    if n_y > PROPAGATE_STIFF_MAX_NY:
        raise ValueError(f'method="sdirk4" takes phases of at most {PROPAGATE_STIFF_MAX_NY} states, this one has {n_y}')


def _is_torch(t) -> bool:
    return hasattr(t, "data_ptr") and hasattr(t, "device")


def signed_bound_multipliers(bound_multipliers, num_x: int, has_multipliers: bool):
    """``Solution``'s ``bound_multipliers`` as one signed vector zu - zl of ``num_x`` float64 entries (a NumPy array, or
    a CUDA tensor when one was given), or ``None``.  Accepted: a pair ``(zl, zu)`` or one signed vector, host arrays or
    device tensors, contiguous float64 of ``num_x`` entries.  ``ValueError`` otherwise, and when bound multipliers
    come without constraint multipliers.  Touches no device."""
    if bound_multipliers is None:
        return None
    if not has_multipliers:
        raise ValueError("bound_multipliers need multipliers: the costates they are read with come from them")

    def one(v):
        if _is_torch(v):
            import torch
            if v.dtype != torch.float64 or v.dim() != 1 or v.numel() != num_x or not v.is_contiguous():
                raise ValueError(f"bound_multipliers must be contiguous float64 vectors of {num_x} entries")
            return v
        v = np.asarray(v)
        if v.dtype != np.float64 or v.shape != (num_x,) or not v.flags.c_contiguous:
            raise ValueError(f"bound_multipliers must be contiguous float64 vectors of {num_x} entries")
        return v

    if isinstance(bound_multipliers, (tuple, list)):
        if len(bound_multipliers) != 2:
            raise ValueError("bound_multipliers must be a pair (zl, zu) or one signed vector")
        zl, zu = (one(v) for v in bound_multipliers)
        if _is_torch(zl) != _is_torch(zu):
            raise ValueError("bound_multipliers: zl and zu must both be host arrays or both device tensors")
        return zu - zl
    return one(bound_multipliers)


@dataclasses.dataclass
class OptimalitySample:
    """What :meth:`Solution.sample_optimality` returns (NumPy arrays, or torch tensors where the queries live):
    ``H_y`` [n_y][Q], ``H_u`` [n_u][Q], ``dp`` = dp/dt [n_y][Q], ``mu`` [n_p][Q], ``zeta`` [n_y + n_u][Q] (``None``
    without bound multipliers), ``costate_residual`` = dp + H_y (+ zeta_y), ``control_stationarity`` = H_u (+ zeta_u)."""
    H_y: object
    H_u: object
    dp: object
    mu: object
    zeta: object
    costate_residual: object
    control_stationarity: object


@dataclasses.dataclass
class OptimalityReport:
    """What :meth:`Solution.optimality_report` returns.  Per section [K]: ``control_stationarity`` / ``costate_residual``
    (the maxima of their absolute values over the section's samples, 0 where the phase has no control / state) and
    ``control_stationarity_time`` / ``costate_residual_time`` (where).  ``max_*``: the phase maxima; ``interior_max_*``:
    with the first and last section left out (NaN when the phase has no other).  ``has_bound_multipliers``: whether zeta
    is part of the two residuals."""
    control_stationarity: np.ndarray
    control_stationarity_time: np.ndarray
    costate_residual: np.ndarray
    costate_residual_time: np.ndarray
    max_control_stationarity: float
    max_costate_residual: float
    interior_max_control_stationarity: float
    interior_max_costate_residual: float
    has_bound_multipliers: bool


END_SLACK = 8 * np.finfo(float).eps     # csrc/pc_args.h PC_SOL_END_SLACK


def check_queries(tau_min: float, tau_max: float, has_nan: bool, extrapolate: bool, slack: float = 0.0):
    """The range check of :meth:`Solution.sample` on the queries' extremes in tau: inside [-1, 1] (by ``slack``:
    a *time* within a few ulp of the phase's end is the end) unless ``extrapolate``."""
    if has_nan:
        raise ValueError("a query is NaN")
    if extrapolate:
        return
    if not (tau_min >= -1.0 - slack and tau_max <= 1.0 + slack):
        raise ValueError(f"queries reach tau = [{tau_min!r}, {tau_max!r}], outside the phase's [-1, 1]; pass "
                         f"extrapolate=True to extend the end sections' polynomials")


def _tau_extremes(q_min: float, q_max: float, is_tau: bool, t0: float, tF: float):
    if is_tau:
        return q_min, q_max, 0.0
    stretch, shift = 0.5 * (tF - t0), 0.5 * (t0 + tF)
    a, b = (q_min - shift) / stretch, (q_max - shift) / stretch
    return min(a, b), max(a, b), END_SLACK


def normalise_query(t, tau):
    """(array, is_tau) of ``sample``'s two ways to say where: exactly one of ``t`` / ``tau``, one-dimensional."""
    if (t is None) == (tau is None):
        raise ValueError("give either t or tau, not both and not neither")
    q = t if tau is None else tau
    if not _is_torch(q):
        q = np.asarray(q, dtype=np.float64)
    if q.ndim != 1:
        raise ValueError("queries must be one-dimensional")
    return q, tau is not None


class Solution:
    """``Solution(engine, x_tilde, objective=None, multipliers=None, bound_multipliers=None)``: the NLP point ``x_tilde`` (scaled; a NumPy array
    or a torch device tensor, e.g. the resident solver's iterate) of ``engine`` as node values and dense output.
    ``multipliers``: the scaled multipliers of the ``engine.num_c`` constraint rows at that point (NumPy array or torch
    device tensor, contiguous float64), belonging to the scaling the engine holds now; with them ``costate``
    ([n_y][N] per phase), ``hamiltonian`` ([N] per phase) and ``integrand_multiplier`` ([n_q] per phase) are filled and
    :meth:`sample_costate` works; without them the three are ``None``.  ``bound_multipliers``: the multipliers of the ``engine.num_x`` variable bounds,
    a pair ``(zl, zu)`` or one signed vector ``zu - zl`` (needs ``multipliers``); the path and bound multipliers, the
    gradients of the augmented Hamiltonian and the two Pontryagin residuals (``path_multiplier``, ``bound_multiplier``,
    ``endpoint_bound_multiplier``, ``hamiltonian_gradient``, ``control_stationarity``, ``costate_defect``,
    :meth:`sample_optimality`, :meth:`optimality_report`) are formed on first use.  Holds device memory: ``close()`` it (or let it
    go) before the engine is closed."""

    def __init__(self, engine, x_tilde, objective=None, multipliers=None, bound_multipliers=None):
        self._h = None
        self._optimality = None
        self._z = signed_bound_multipliers(bound_multipliers, engine.num_x, multipliers is not None)
        self.engine = engine
        self._lib = engine._lib
        self._h = C.c_void_p()
        self._declare(self._lib)
        lay, model = engine.layout, engine.model
        method = engine.quad.method
        orders = sorted({int(n) for mesh in engine.meshes for n in np.unique(mesh.n)})
        tabs = [solution_tables(method, n) for n in orders]
        tabD = np.ascontiguousarray(np.concatenate([t[0].ravel() for t in tabs]))
        tabU = np.ascontiguousarray(np.concatenate([t[1].ravel() for t in tabs]))
        od = np.ascontiguousarray(orders, dtype=np.int32)
        tau = np.ascontiguousarray(np.concatenate([np.asarray(m.tau, dtype=np.float64) for m in engine.meshes]))
        if _is_torch(x_tilde):
            import torch
            if x_tilde.dtype != torch.float64 or x_tilde.numel() != engine.num_x or not x_tilde.is_contiguous():
                raise ValueError(f"x_tilde must be a contiguous float64 tensor of {engine.num_x} entries")
            torch.cuda.current_stream(x_tilde.device).synchronize()
            ok = self._lib.pc_solution_create_device(engine._h, x_tilde.data_ptr(), len(od), od.ctypes.data, tabD.ctypes.data,
                                                     tabU.ctypes.data, tau.ctypes.data, C.byref(self._h))
            x_host = x_tilde.detach().cpu().numpy()
        else:
            x_host = np.ascontiguousarray(x_tilde, dtype=np.float64).reshape(-1)
            if x_host.shape[0] != engine.num_x:
                raise ValueError(f"x_tilde must have {engine.num_x} entries")
            ok = self._lib.pc_solution_create(engine._h, x_host.ctypes.data, len(od), od.ctypes.data, tabD.ctypes.data,
                                              tabU.ctypes.data, tau.ctypes.data, C.byref(self._h))
        if not ok:
            raise RuntimeError("pc_solution_create failed: " + self._lib.pc_last_error().decode())
        # node values from the device; q, t, s unscaled here (a handful of numbers)
        x = lay.expand_x(engine.V_ocp) * x_host + lay.expand_x(engine.r_ocp)
        self.objective = None if objective is None else float(objective)
        node_time, state, dstate, control, integral, time, t0s, tFs = [], [], [], [], [], [], [], []
        for ip, (pm, pl, mesh) in enumerate(zip(model.phases, lay.phases, engine.meshes)):
            N = pl.N
            tt = np.empty(N)
            y, dy, u = np.empty((pm.n_y, N)), np.empty((pm.n_y, N)), np.empty((pm.n_u, N))
            self._check(self._lib.pc_solution_nodes(self._h, ip, tt.ctypes.data, y.ctypes.data if y.size else None,
                                                    dy.ctypes.data if dy.size else None, u.ctypes.data if u.size else None))
            node_time.append(tt)
            # (casadi_solution.py:45-59: an empty 1-D array where a phase has no such variable)
            state.append(y if pm.n_y else np.array([], dtype=float))
            dstate.append(dy if pm.n_y else np.array([], dtype=float))
            control.append(u if pm.n_u else np.array([], dtype=float))
            integral.append(x[pl.q_off:pl.q_off + pm.n_q].copy())
            tv = x[pl.t_off:pl.t_off + pl.n_t].copy()
            time.append(tv)
            j = 0
            t0 = float(pm.t_fixed[0])
            tF = float(pm.t_fixed[1])
            if pm.t_free[0]:
                t0 = float(tv[j])
                j += 1
            if pm.t_free[1]:
                tF = float(tv[j])
            t0s.append(t0)
            tFs.append(tF)
        self.tau = tuple(np.asarray(m.tau, dtype=float) for m in engine.meshes)
        self.node_time = tuple(node_time)           # the reference's _time_
        self.state = tuple(state)
        self.state_derivative = tuple(dstate)
        self.control = tuple(control)
        self.integral = tuple(integral)
        self.time = tuple(time)                     # the time *variables* of every phase (casadi_solution.py:38)
        self.initial_time = tuple(t0s)
        self.final_time = tuple(tFs)
        self.parameter = x[lay.s_off:lay.s_off + lay.n_s].copy()
        self.costate = self.hamiltonian = self.integrand_multiplier = None
        if multipliers is not None:
            try:
                self._set_multipliers(multipliers, orders)
            except Exception:
                self.close()
                raise

    # ---- plumbing ----------------------------------------------------------------------------------
    @staticmethod
    def _declare(lib):
        if getattr(lib, "_pc_solution_declared", False):
            return
        vp = C.c_void_p
        i32p = C.POINTER(C.c_int32)
        lib.pc_solution_create.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, C.POINTER(vp)]
        lib.pc_solution_create_device.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, C.POINTER(vp)]
        lib.pc_solution_destroy.argtypes = [vp]
        lib.pc_solution_destroy.restype = None
        lib.pc_solution_sizes.argtypes = [vp, C.c_int, i32p, i32p, i32p, i32p, i32p]
        lib.pc_solution_nodes.argtypes = [vp, C.c_int, vp, vp, vp, vp]
        lib.pc_solution_coefficients.argtypes = [vp, C.c_int, vp, vp]
        lib.pc_solution_sample.argtypes = [vp, C.c_int, vp, C.c_int64, C.c_int, vp, vp, vp, vp]
        lib.pc_solution_sample_device.argtypes = [vp, C.c_int, vp, C.c_int64, C.c_int, vp, vp, vp, vp]
        lib.pc_solution_set_multipliers.argtypes = [vp, vp, C.c_int64, C.c_int, vp, vp]
        lib.pc_solution_set_multipliers_device.argtypes = [vp, vp, C.c_int64, C.c_int, vp, vp]
        lib.pc_solution_costate_nodes.argtypes = [vp, C.c_int, vp, vp, vp]
        lib.pc_solution_costate_coefficients.argtypes = [vp, C.c_int, vp]
        lib.pc_solution_sample_costate.argtypes = [vp, C.c_int, vp, C.c_int64, C.c_int, vp, vp]
        lib.pc_solution_sample_costate_device.argtypes = [vp, C.c_int, vp, C.c_int64, C.c_int, vp, vp]
        prop = [vp, C.c_int, C.c_int64, vp, C.c_int64, C.c_double, vp, C.c_int64, vp, vp, vp, vp]
        lib.pc_solution_propagate.argtypes = prop
        lib.pc_solution_propagate_device.argtypes = prop
        stiff = prop[:8] + [C.c_int64] + [vp] * 6
        lib.pc_solution_propagate_stiff.argtypes = stiff
        lib.pc_solution_propagate_stiff_device.argtypes = stiff
        dense = [vp, C.c_int, C.c_int64, vp, C.c_int64, C.c_double, vp, vp, C.c_int64, C.c_int64, vp] + [vp] * 7
        lib.pc_solution_propagate_dense.argtypes = dense
        lib.pc_solution_propagate_dense_device.argtypes = dense
        lib.pc_solution_set_bound_multipliers.argtypes = [vp, vp, C.c_int64]
        lib.pc_solution_set_bound_multipliers_device.argtypes = [vp, vp, C.c_int64]
        lib.pc_solution_multiplier_nodes.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
        lib.pc_solution_multiplier_coefficients.argtypes = [vp, C.c_int, vp, vp]
        lib.pc_solution_defect_multipliers.argtypes = [vp, C.c_int, vp]
        lib.pc_solution_sample_optimality.argtypes = [vp, C.c_int, vp, C.c_int64, C.c_int, vp, vp, vp, vp, vp]
        lib.pc_solution_sample_optimality_device.argtypes = [vp, C.c_int, vp, C.c_int64, C.c_int, vp, vp, vp, vp, vp]
        lib._pc_solution_declared = True

    def _set_multipliers(self, lam, orders):
        """``pc_solution_set_multipliers``: the costate kernel on the multipliers, then the node values."""
        engine = self.engine
        od = np.ascontiguousarray(orders, dtype=np.int32)
        tabA = np.ascontiguousarray(np.concatenate([np.asarray(engine.quad.A(n), dtype=np.float64).ravel() for n in orders]))
        if _is_torch(lam):
            import torch
            if lam.dtype != torch.float64 or lam.dim() != 1 or lam.numel() != engine.num_c or not lam.is_contiguous() \
                    or not lam.is_cuda:
                raise ValueError(f"multipliers must be a contiguous float64 device tensor of {engine.num_c} entries")
            torch.cuda.current_stream(lam.device).synchronize()
            ok = self._lib.pc_solution_set_multipliers_device(self._h, lam.data_ptr(), lam.numel(), len(od), od.ctypes.data,
                                                              tabA.ctypes.data)
        else:
            lam = np.asarray(lam)
            if lam.dtype != np.float64 or lam.shape != (engine.num_c,) or not lam.flags.c_contiguous:
                raise ValueError(f"multipliers must be a contiguous float64 array of {engine.num_c} entries")
            ok = self._lib.pc_solution_set_multipliers(self._h, lam.ctypes.data, lam.shape[0], len(od), od.ctypes.data,
                                                       tabA.ctypes.data)
        self._check(ok)
        costate, hamiltonian, nu = [], [], []
        for ip, (pm, pl) in enumerate(zip(engine.model.phases, engine.layout.phases)):
            p, H, v = np.empty((pm.n_y, pl.N)), np.empty(pl.N), np.empty(pm.n_q)
            self._check(self._lib.pc_solution_costate_nodes(self._h, ip, p.ctypes.data if p.size else None, H.ctypes.data,
                                                            v.ctypes.data if v.size else None))
            costate.append(p)
            hamiltonian.append(H)
            nu.append(v)
        self.costate = tuple(costate)
        self.hamiltonian = tuple(hamiltonian)
        self.integrand_multiplier = tuple(nu)

    def _check(self, ok):
        if not ok:
            raise RuntimeError(self._lib.pc_last_error().decode())

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            if getattr(self.engine, "_h", None):          # (a closed engine has released the stream and the module)
                self._lib.pc_solution_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _phase(self, phase: int, need_handle: bool = True) -> int:
        phase = int(phase)
        if not 0 <= phase < len(self.state):
            raise ValueError(f"phase {phase} out of range (the solution has {len(self.state)})")
        if need_handle and not self._h:
            raise ValueError("the solution is closed")
        return phase

    # ---- polynomials -------------------------------------------------------------------------------
    def coefficients(self, phase: int):
        """(dy_coef [n_y][N + K - 1], u_coef [n_u][N + K - 1]): section k's n_k Legendre coefficients in the section
        variable start at column ``mesh.s[k] + k`` (``pc_solution_coefficients``)."""
        phase = self._phase(phase)
        pl = self.engine.layout.phases[phase]
        NC = pl.N + pl.K - 1
        dc, uc = np.empty((pl.n_y, NC)), np.empty((pl.n_u, NC))
        self._check(self._lib.pc_solution_coefficients(self._h, phase, dc.ctypes.data if dc.size else None,
                                                       uc.ctypes.data if uc.size else None))
        return dc, uc

    def polys(self, phase: int):
        """``phase_polys[phase]`` of the reference (solution_abc.py:60-142) as ``(y, dy, u)`` object arrays
        [var][K] of ``numpy.polynomial.Legendre`` over ``domain = [tau_k, tau_k+1]``, built from the exported
        coefficients; ``y[var, k](tau)`` is the integrated form."""
        from numpy.polynomial import Legendre
        phase = self._phase(phase)
        mesh, pl = self.engine.meshes[phase], self.engine.layout.phases[phase]
        dc, uc = self.coefficients(phase)
        stretch = 0.5 * (self.final_time[phase] - self.initial_time[phase])
        y_p = np.empty((pl.n_y, pl.K), dtype=object)
        dy_p = np.empty((pl.n_y, pl.K), dtype=object)
        u_p = np.empty((pl.n_u, pl.K), dtype=object)
        for k in range(pl.K):
            s, n = int(mesh.s[k]), int(mesh.n[k])
            dom = [float(mesh.tau[s]), float(mesh.tau[int(mesh.s[k + 1])])]
            sl = slice(s + k, s + k + n)
            for a in range(pl.n_y):
                dy_p[a, k] = Legendre(dc[a, sl], domain=dom)
                # integ() integrates in tau (it scales by the domain's half width itself); lbnd: zero at tau_k
                y_p[a, k] = Legendre(dc[a, sl] * stretch, domain=dom).integ(lbnd=dom[0], k=[float(self.state[phase][a][s])])
            for b in range(pl.n_u):
                u_p[b, k] = Legendre(uc[b, sl], domain=dom)
        return y_p, dy_p, u_p

    def quadrature_weights(self, phase: int) -> np.ndarray:
        """omega [N] of the costate definition: the node weights of the phase's quadrature in tau, from the last rows
        of the sections' integration tables (they sum to 2, the length of [-1, 1]; the Radau phase-final node has
        none).  ``sum(omega * hamiltonian) / sum(omega)`` over the weighted nodes is the mean the NLP's stationarity
        in the final time speaks about."""
        phase = self._phase(phase, need_handle=False)
        mesh, quad = self.engine.meshes[phase], self.engine.quad
        w = np.zeros(mesh.N)
        for k in range(mesh.K):
            s, n = int(mesh.s[k]), int(mesh.n[k])
            w[s:s + n] += (mesh.tau[int(mesh.s[k + 1])] - mesh.tau[s]) * quad.A(n)[n - 2]
        return w

    def costate_coefficients(self, phase: int):
        """p_coef [n_y][N + K - 1], laid out like the controls' coefficients (``pc_solution_costate_coefficients``)."""
        phase = self._phase(phase)
        if self.costate is None:
            raise ValueError("the solution was made without multipliers: it has no costates")
        pl = self.engine.layout.phases[phase]
        pc = np.empty((pl.n_y, pl.N + pl.K - 1))
        self._check(self._lib.pc_solution_costate_coefficients(self._h, phase, pc.ctypes.data if pc.size else None))
        return pc

    # ---- dense output ------------------------------------------------------------------------------
    def _queries(self, phase, t, tau, extrapolate, *, check_range=True, host_only=False):
        """``(phase, q, flags)`` of a sampling call: the queries as a contiguous float64 NumPy array or (unless
        ``host_only``) CUDA tensor.  Raises, in this order: bad ``t`` / ``tau``, phase out of range, with ``check_range``
        a NaN or a query outside the phase, the solution is closed."""
        q, is_tau = normalise_query(t, tau)
        phase = self._phase(phase, need_handle=False)
        flags = (PC_SOLUTION_TAU if is_tau else 0) | (PC_SOLUTION_EXTRAPOLATE if extrapolate else 0)
        if _is_torch(q) and not host_only:
            import torch
            if q.dtype != torch.float64 or not q.is_cuda:
                raise ValueError("a tensor of queries must be float64 on the GPU")
            q, isnan = q.contiguous(), torch.isnan
        else:
            q, isnan = np.ascontiguousarray(np.asarray(q, dtype=np.float64)), np.isnan
        if check_range and q.shape[0]:
            has_nan = bool(isnan(q).any())
            lo, hi = (0.0, 0.0) if has_nan else (float(q.min()), float(q.max()))
            lo, hi, slack = _tau_extremes(lo, hi, is_tau, self.initial_time[phase], self.final_time[phase])
            check_queries(lo, hi, has_nan, extrapolate, slack)
        self._phase(phase)     # (the device is needed from here on)
        return phase, q, flags

    def _sample_into(self, host_call, device_call, phase, q, flags, shapes):
        """One output array per entry of ``shapes`` (None: not wanted), where the queries live, filled by the exported
        call: NumPy queries -> ``host_call``, a device tensor -> ``device_call`` on the handle's stream."""
        Q = int(q.shape[0])
        if _is_torch(q):
            import torch
            outs = [None if sh is None else torch.empty(sh, dtype=torch.float64, device=q.device) for sh in shapes]
            ptr = lambda a: a.data_ptr() if (a is not None and a.numel()) else None   # noqa: E731
            torch.cuda.current_stream(q.device).synchronize()     # the handle's stream is not torch's
            self._check(device_call(self._h, phase, ptr(q), Q, flags, *(ptr(a) for a in outs)))
            self._check(self._lib.pc_synchronize(self.engine._h))
        else:
            outs = [None if sh is None else np.empty(sh) for sh in shapes]
            ptr = lambda a: a.ctypes.data if (a is not None and a.size) else None   # noqa: E731
            self._check(host_call(self._h, phase, ptr(q), Q, flags, *(ptr(a) for a in outs)))
        return outs

    def _sample(self, phase, q, flags, with_f):
        pl, Q = self.engine.layout.phases[phase], int(q.shape[0])
        return self._sample_into(self._lib.pc_solution_sample, self._lib.pc_solution_sample_device, phase, q, flags,
                                 [(pl.n_y, Q), (pl.n_y, Q), (pl.n_u, Q), (pl.n_y, Q) if with_f else None])

    def sample(self, phase: int, t=None, *, tau=None, residual: bool = False, extrapolate: bool = False):
        """``(y [n_y][Q], ydot [n_y][Q], u [n_u][Q])`` at the Q times ``t`` (or abscissae ``tau`` in [-1, 1]) of one
        phase, in the order given (any order, duplicates allowed); with ``residual=True`` a fourth array
        ``ydot - f(y(t), u(t), q, t, s)`` [n_y][Q], the collocation residual between the nodes.  NumPy in, NumPy out;
        torch device tensor in, torch tensors on that device out.  Queries outside the phase raise ``ValueError``
        unless ``extrapolate=True`` (then the end sections' polynomials are extended); a time within 8 eps (in tau) of
        the phase's end, such as ``node_time``'s own last entry, is the end."""
        y, dy, u, f = self._sample(*self._queries(phase, t, tau, extrapolate), residual)
        if residual:
            return y, dy, u, dy - f
        return y, dy, u

    def sample_f(self, phase: int, t=None, *, tau=None, extrapolate: bool = False):
        """``pc_solution_sample`` as it is (NumPy queries): ``(y, ydot, u, f)`` with f(y(t), u(t), q, t, s) itself as
        the fourth array, and no range check -- a query outside the phase gives NaN in every output unless
        ``extrapolate=True``."""
        return tuple(self._sample(*self._queries(phase, t, tau, extrapolate, check_range=False, host_only=True), True))

    def sample_costate(self, phase: int, t=None, *, tau=None, extrapolate: bool = False):
        """``(p [n_y][Q], H [Q])`` at the Q times ``t`` (or abscissae ``tau``) of one phase: the costates' section
        interpolants and the Hamiltonian formed from them and the model at the interpolated (y(t), u(t)).  Queries, range
        checks and array types as in :meth:`sample`.  ``ValueError`` if the solution was made without multipliers."""
        if self.costate is None:
            raise ValueError("the solution was made without multipliers: it has no costates")
        return self.sample_costate_unchecked(*self._queries(phase, t, tau, extrapolate))

    def sample_costate_unchecked(self, phase, q, flags):
        """``pc_solution_sample_costate`` as it is: no range check, NaN for a query outside the phase."""
        pl, Q = self.engine.layout.phases[phase], int(q.shape[0])
        p, H = self._sample_into(self._lib.pc_solution_sample_costate, self._lib.pc_solution_sample_costate_device, phase, q,
                                 flags, [(pl.n_y, Q), (Q,)])
        return p, H

    # ---- path and bound multipliers, the gradients of the augmented Hamiltonian --------------------
    def _form_optimality(self):
        """``pc_solution_set_bound_multipliers`` (one launch per phase) and the node values; once."""
        if self._optimality is not None:
            return self._optimality
        if self.costate is None:
            raise ValueError("the solution was made without multipliers: it has no path or bound multipliers")
        if not self._h:
            raise ValueError("the solution is closed")
        z, eng = self._z, self.engine
        if z is None:
            ok = self._lib.pc_solution_set_bound_multipliers(self._h, None, 0)
        elif _is_torch(z):
            import torch
            if not z.is_cuda:
                raise ValueError("a tensor of bound multipliers must be on the GPU")
            torch.cuda.current_stream(z.device).synchronize()
            ok = self._lib.pc_solution_set_bound_multipliers_device(self._h, z.data_ptr(), z.numel())
        else:
            ok = self._lib.pc_solution_set_bound_multipliers(self._h, z.ctypes.data, z.shape[0])
        self._check(ok)
        ptr = lambda a: a.ctypes.data if (a is not None and a.size) else None   # noqa: E731
        mu, zeta, end_z, H_y, H_u, defect = [], [], [], [], [], []
        for ip, (pm, pl, mesh) in enumerate(zip(eng.model.phases, eng.layout.phases, eng.meshes)):
            N, n_y, n_u = pl.N, pm.n_y, pm.n_u
            m, hy, hu = np.empty((pm.n_p, N)), np.empty((n_y, N)), np.empty((n_u, N))
            zt = np.empty((n_y + n_u, N)) if z is not None else None
            ez = np.empty((n_y, 2)) if z is not None else None
            self._check(self._lib.pc_solution_multiplier_nodes(self._h, ip, ptr(m), ptr(zt), ptr(ez), ptr(hy), ptr(hu)))
            # the discrete defect term D_a(j) over stretch omega_j, at the interior weighted nodes
            Lam = np.empty((n_y, N - 1))     # W lam~ / w from the solution's own device copy, as the multipliers were set
            self._check(self._lib.pc_solution_defect_multipliers(self._h, ip, ptr(Lam)))
            D = np.zeros((n_y, N))
            D[:, 1:] -= Lam
            for k in range(mesh.K):
                s, n = int(mesh.s[k]), int(mesh.n[k])
                D[:, s] += np.sum(Lam[:, s:s + n - 1], axis=1)
            omega = self.quadrature_weights(ip)
            stretch = 0.5 * (self.final_time[ip] - self.initial_time[ip])
            cd = np.full((n_y, N), np.nan)
            use = omega != 0
            use[0] = use[-1] = False
            cd[:, use] = D[:, use] / (stretch * omega[use]) + hy[:, use] + (zt[:n_y, use] if zt is not None else 0.0)
            mu.append(m)
            zeta.append(zt)
            end_z.append(ez)
            H_y.append(hy)
            H_u.append(hu)
            defect.append(cd)
        self._optimality = dict(mu=tuple(mu), zeta=None if z is None else tuple(zeta),
                                end_z=None if z is None else tuple(end_z), H_y=tuple(H_y), H_u=tuple(H_u),
                                defect=tuple(defect))
        return self._optimality

    def _optimality_or_none(self, key):
        if self.costate is None:
            return None
        return self._form_optimality()[key]

    @property
    def path_multiplier(self):
        """mu [n_p][N] per phase; ``None`` without multipliers.  Formed on first use, like the five below."""
        return self._optimality_or_none("mu")

    @property
    def bound_multiplier(self):
        """zeta [n_y + n_u][N] per phase (states first); ``None`` without bound multipliers."""
        return self._optimality_or_none("zeta")

    @property
    def endpoint_bound_multiplier(self):
        """z~ / (w V_a) [n_y][2] per phase at nodes 0 and N - 1: the endpoint bounds' multipliers (transversality);
        ``None`` without bound multipliers."""
        return self._optimality_or_none("end_z")

    @property
    def hamiltonian_gradient(self):
        """``(H_y, H_u)``: per phase [n_y][N] and [n_u][N], at the nodes' NLP values; ``None`` without multipliers."""
        if self.costate is None:
            return None
        o = self._form_optimality()
        return o["H_y"], o["H_u"]

    @property
    def control_stationarity(self):
        """H_u + zeta_u [n_u][N] per phase (H_u alone without bound multipliers); ``None`` without multipliers."""
        if self.costate is None:
            return None
        o = self._form_optimality()
        if o["zeta"] is None:
            return o["H_u"]
        return tuple(hu + zt[zt.shape[0] - hu.shape[0]:] for hu, zt in zip(o["H_u"], o["zeta"]))

    @property
    def costate_defect(self):
        """D_a / (stretch omega) + H_y + zeta_y [n_y][N] per phase: the costate equation as the NLP discretises it; NaN
        at nodes 0, N - 1 and a node without quadrature weight.  ``None`` without multipliers."""
        return self._optimality_or_none("defect")

    def multiplier_coefficients(self, phase: int):
        """(mu_coef [n_p][N + K - 1], zeta_coef [n_y + n_u][N + K - 1] or ``None``), laid out like the controls'."""
        phase = self._phase(phase)
        self._form_optimality()
        pl, pm = self.engine.layout.phases[phase], self.engine.model.phases[phase]
        NC = pl.N + pl.K - 1
        mc = np.empty((pm.n_p, NC))
        zc = np.empty((pl.n_y + pl.n_u, NC)) if self._z is not None else None
        self._check(self._lib.pc_solution_multiplier_coefficients(self._h, phase, mc.ctypes.data if mc.size else None,
                                                                  zc.ctypes.data if zc is not None and zc.size else None))
        return mc, zc

    def sample_optimality(self, phase: int, t=None, *, tau=None, extrapolate: bool = False):
        """An :class:`OptimalitySample` at the Q times ``t`` (or abscissae ``tau``) of one phase.  Queries, range checks
        and array types as in :meth:`sample`.  ``ValueError`` if the solution was made without multipliers."""
        phase = self._phase(phase, need_handle=False)
        if self.costate is None:
            raise ValueError("the solution was made without multipliers: it has no path or bound multipliers")
        return self.sample_optimality_unchecked(*self._queries(phase, t, tau, extrapolate))

    def sample_optimality_unchecked(self, phase, q, flags):
        """``pc_solution_sample_optimality`` as it is: no range check, NaN for a query outside the phase."""
        self._form_optimality()
        pl, pm, Q = self.engine.layout.phases[phase], self.engine.model.phases[phase], int(q.shape[0])
        n_y, n_u = pl.n_y, pl.n_u
        H_y, H_u, dp, mu, zeta = self._sample_into(
            self._lib.pc_solution_sample_optimality, self._lib.pc_solution_sample_optimality_device, phase, q, flags,
            [(n_y, Q), (n_u, Q), (n_y, Q), (pm.n_p, Q), (n_y + n_u, Q) if self._z is not None else None])
        res, stat = dp + H_y, H_u
        if zeta is not None:
            res, stat = res + zeta[:n_y], H_u + zeta[n_y:]
        return OptimalitySample(H_y=H_y, H_u=H_u, dp=dp, mu=mu, zeta=zeta, costate_residual=res, control_stationarity=stat)

    def optimality_report(self, phase: int, samples_per_section: int = 33):
        """An :class:`OptimalityReport` of one phase: ``samples_per_section`` equispaced points c in [-1, 1] of every
        section (its two ends included; at least 2), sampled and reduced on the device."""
        import torch
        phase = self._phase(phase, need_handle=False)
        if self.costate is None:
            raise ValueError("the solution was made without multipliers: it has no path or bound multipliers")
        m = int(samples_per_section)
        if m < 2:
            raise ValueError("samples_per_section must be at least 2")
        self._phase(phase)
        mesh, eng = self.engine.meshes[phase], self.engine
        dev = torch.device("cuda", max(int(eng.device), 0))
        edges = torch.as_tensor(np.asarray(mesh.tau, dtype=np.float64)[np.asarray(mesh.s)], device=dev)
        c = torch.linspace(-1.0, 1.0, m, dtype=torch.float64, device=dev)
        tau_q = edges[:-1, None] + 0.5 * (c[None, :] + 1.0) * (edges[1:, None] - edges[:-1, None])
        tau_q[:, 0] = edges[:-1]
        # an interior boundary belongs to the section on its right: a section's last sample is the double below it
        tau_q[:, -1] = torch.nextafter(edges[1:], torch.full_like(edges[1:], -2.0))
        tau_q[-1, -1] = edges[-1]
        tau_q = tau_q.reshape(-1).contiguous()
        smp = self.sample_optimality(phase, tau=tau_q)
        t0, tF = self.initial_time[phase], self.final_time[phase]
        time = (tau_q * (0.5 * (tF - t0)) + 0.5 * (t0 + tF)).reshape(mesh.K, m)

        def reduce(a):
            if a.shape[0] == 0:
                return np.zeros(mesh.K), np.full(mesh.K, np.nan)
            v = a.abs().amax(dim=0).reshape(mesh.K, m)
            v = torch.where(torch.isnan(v), torch.full_like(v, float("inf")), v)     # a NaN sample shows as inf
            val, idx = v.max(dim=1)
            return val.cpu().numpy(), time.gather(1, idx[:, None])[:, 0].cpu().numpy()

        cs, cs_t = reduce(smp.control_stationarity)
        cr, cr_t = reduce(smp.costate_residual)
        inner = lambda v: float(np.max(v[1:-1])) if mesh.K > 2 else float("nan")   # noqa: E731
        return OptimalityReport(control_stationarity=cs, control_stationarity_time=cs_t, costate_residual=cr,
                                costate_residual_time=cr_t, max_control_stationarity=float(np.max(cs)),
                                max_costate_residual=float(np.max(cr)), interior_max_control_stationarity=inner(cs),
                                interior_max_costate_residual=inner(cr), has_bound_multipliers=self._z is not None)

    # ---- propagation -------------------------------------------------------------------------------
    def state_scale(self, phase: int) -> np.ndarray:
        """V_a [n_y]: the scale of every state of the phase in the engine's variable scaling (y = V y~ + r)."""
        phase = self._phase(phase, need_handle=False)
        pl = self.engine.layout.phases[phase]
        V = self.engine.layout.expand_x(self.engine.V_ocp)
        return np.array([V[pl.x_off + a * pl.N] for a in range(pl.n_y)], dtype=np.float64)

    def _propagate_prelude(self, phase, restart, rtol, atol, substeps, max_steps, maybe_device):
        """What :meth:`propagate` and :meth:`propagate_dense` do first: the segment list, ``atol`` (its default, its
        broadcast, its checks with the other tolerances) and where the outputs go -- the device of the first torch
        device tensor among ``maybe_device``, else ``None`` for NumPy.  Returns seg, at, V, device, n_seg, m."""
        pl, mesh = self.engine.layout.phases[phase], self.engine.meshes[phase]
        device = next((a.device for a in maybe_device if _is_torch(a) and a.is_cuda), None)
        seg = propagation_segments(restart, mesh.s, pl.N)
        V = self.state_scale(phase)
        if atol is None:
            at = float(rtol) * V
        else:
            if _is_torch(atol):
                atol = atol.detach().cpu().numpy()
            at = np.ascontiguousarray(np.broadcast_to(np.asarray(atol, dtype=np.float64), (pl.n_y,)))
        check_propagate_tolerances(substeps, rtol, at, max_steps)
        return seg, np.ascontiguousarray(at, dtype=np.float64), V, device, len(seg) - 1, 0 if substeps is None else int(substeps)

    def _propagation_fields(self, phase, y, status, V, device):
        """What :class:`Propagation` and :class:`DensePropagation` derive from the arrivals ``y`` and ``status``, as
        NumPy arrays or as torch tensors on ``device``: defect, relative_defect, ok, terminal_defect."""
        node_y = np.asarray(self.state[phase], dtype=np.float64).reshape(y.shape)
        scale = V[:, None]
        if device is not None:
            import torch
            node_y, scale = torch.as_tensor(node_y, device=device), torch.as_tensor(V, device=device)[:, None]
        defect = y - node_y
        return dict(defect=defect, relative_defect=defect / scale, ok=status == -1, terminal_defect=defect[:, -1])

    def propagate(self, phase: int, *, restart="nodes", rtol: float = 1e-9, atol=None, substeps=None, max_steps: int = 4096,
                  method: str = "dopri5", newton_max: int = 8):
        """Integrate the dynamics forward under the solution's controls (``pc_sol_propagate_p<i>``) and
        return a :class:`Propagation`.

        ``restart``: where the integration restarts from the NLP's own state -- "nodes" (every node: N - 1
        independent one-interval problems, the multiple-shooting defect per interval), "sections" (every section
        start), "phase" (one open-loop pass) or an array of node indices, strictly ascending from 0 to N - 1 (a host
        array or a device tensor).  Inside section k the independent variable is the section variable c and
        dy/dc = stretch (w_k / 2) f(y, u(c), q, t0, tF, s); no step straddles a node.  **u(c) is the interpolant**
        :meth:`sample` **returns**: the degree n_k - 1 polynomial through all n_k node controls of the section.  Under
        Radau that includes the section's end node, and in the last section the phase-final control, whatever the
        NLP left there (no collocation row reads it).

        ``substeps=m``: m equal Dormand-Prince steps per node interval, no error control (deterministic).
        ``substeps=None``: adaptive, every interval starting with one step over the whole interval; err = max_a |e_a| /
        (atol_a + rtol max(|y_a|, |y_a,new|)) <= 1 accepts; ``atol=None`` means rtol V_a per state (``state_scale``).
        ``max_steps`` (accepted + rejected per interval, 1 .. 2^20) bounds the work: a segment whose interval uses it up
        stops there (``ok`` False, NaN from that interval to the segment's end); the other segments are unaffected.

        ``method="sdirk4"`` (``pc_sol_propagate_stiff_p<i>``) is for stiff phases, where stability and not
        accuracy sets the explicit pair's step: the five-stage L-stable SDIRK method of order 4 (Hairer & Wanner), one
        Jacobian and one LU factorisation per attempt, a Newton iteration per stage of at most ``newton_max`` (1 .. 32)
        iterations, stopped by ``rtol`` and ``atol`` -- so ``rtol`` is read and checked in both modes.  A Newton failure
        rejects the step (adaptive) or ends the segment there (fixed); ``newton_rejected`` and ``newton_iterations``
        of the result count them.  Phases of up to 11 states.  ``"dopri5"`` is the default and ignores ``newton_max``.

        NumPy out, unless ``restart`` or ``atol`` is a torch device tensor: then torch tensors on that device.  Bad
        arguments raise ``ValueError`` before anything is launched."""
        phase = self._phase(phase, need_handle=False)
        pl = self.engine.layout.phases[phase]
        N, n_y = pl.N, pl.n_y
        seg, at, V, device, n_seg, m = self._propagate_prelude(phase, restart, rtol, atol, substeps, max_steps, (restart, atol))
        check_propagate_method(method, newton_max, rtol, n_y)
        stiff = method == "sdirk4"
        self._phase(phase)     # (the device is needed from here on)
        head = (self._h, phase, n_seg, seg.ctypes.data, m, float(rtol), at.ctypes.data if n_y else None, int(max_steps))
        if stiff:
            head += (int(newton_max),)
        nrej = nit = None
        if device is not None:
            import torch
            y = torch.empty((n_y, N), dtype=torch.float64, device=device)
            acc, rej = (torch.empty((N,), dtype=torch.int32, device=device) for _ in range(2))
            status = torch.empty((n_seg,), dtype=torch.int32, device=device)
            torch.cuda.current_stream(device).synchronize()     # the handle's stream is not torch's
            if stiff:
                nrej, nit = (torch.empty((N,), dtype=torch.int32, device=device) for _ in range(2))
                self._check(self._lib.pc_solution_propagate_stiff_device(*head, y.data_ptr() if n_y else None, acc.data_ptr(),
                                                                         rej.data_ptr(), status.data_ptr(), nrej.data_ptr(),
                                                                         nit.data_ptr()))
            else:
                self._check(self._lib.pc_solution_propagate_device(*head, y.data_ptr() if n_y else None, acc.data_ptr(),
                                                                   rej.data_ptr(), status.data_ptr()))
            self._check(self._lib.pc_synchronize(self.engine._h))
        else:
            y = np.empty((n_y, N))
            acc, rej, status = np.empty(N, dtype=np.int32), np.empty(N, dtype=np.int32), np.empty(n_seg, dtype=np.int32)
            if stiff:
                nrej, nit = np.empty(N, dtype=np.int32), np.empty(N, dtype=np.int32)
                self._check(self._lib.pc_solution_propagate_stiff(*head, y.ctypes.data if n_y else None, acc.ctypes.data,
                                                                  rej.ctypes.data, status.ctypes.data, nrej.ctypes.data,
                                                                  nit.ctypes.data))
            else:
                self._check(self._lib.pc_solution_propagate(*head, y.ctypes.data if n_y else None, acc.ctypes.data,
                                                            rej.ctypes.data, status.ctypes.data))
        return Propagation(y=y, accepted=acc, rejected=rej, segments=seg, status=status, newton_rejected=nrej,
                           newton_iterations=nit, **self._propagation_fields(phase, y, status, V, device))

    def propagate_dense(self, phase: int, t=None, *, tau=None, restart="nodes", rtol: float = 1e-9, atol=None,
                        integral_atol=None, substeps=None, max_steps: int = 4096):
        """:meth:`propagate` with the phase's integrals carried along and the propagated path sampled between the nodes
        (``pc_sol_propagate_dense_p<i>``); returns a :class:`DensePropagation`.

        ``restart``, ``rtol``, ``atol``, ``substeps``, ``max_steps``: as in :meth:`propagate`, and the steps are the
        same.  The integrals I_m follow dI_m/dc = stretch (w_k / 2) g_m from 0 at every segment's first node.
        ``integral_atol=None``: they take no part in the step control, and ``y``, ``accepted``, ``rejected`` and
        ``status`` equal :meth:`propagate`'s to the bit.  ``integral_atol`` (a number or n_q numbers, finite and
        positive): integral m adds |e_m| / (integral_atol_m + rtol max(|I_m|, |I_m,new|)) to the adaptive error norm.

        ``t`` (times) or ``tau`` (abscissae in [-1, 1]), any order, duplicates allowed, or neither (the integrals
        only): where the path is wanted.  A query belongs to the node interval (tau_j, tau_j+1] that holds it and is
        answered by the first accepted step that reaches it, through the pair's continuous extension (fourth order);
        at a node it is the arriving value itself.  Queries behind an interval that used up ``max_steps`` are NaN.
        A NaN query or one outside the phase raises ``ValueError``: there is no extrapolation of a propagated path.

        NumPy out, unless ``t`` / ``tau``, ``restart``, ``atol`` or ``integral_atol`` is a torch device tensor: then
        torch tensors on that device.  Bad arguments raise ``ValueError`` before anything is launched."""
        phase = self._phase(phase, need_handle=False)
        pl = self.engine.layout.phases[phase]
        N, n_y, n_q = pl.N, pl.n_y, pl.n_q
        seg, at, V, device, n_seg, m = self._propagate_prelude(phase, restart, rtol, atol, substeps, max_steps,
                                                               (t, tau, restart, atol, integral_atol))
        ia = check_integral_atol(integral_atol, n_q)
        tq = dense_query_tau(t, tau, self.initial_time[phase], self.final_time[phase])
        self._phase(phase)     # (the device is needed from here on)
        Q = int(tq.shape[0])
        head = (self._h, phase, n_seg, seg.ctypes.data, m, float(rtol), at.ctypes.data if n_y else None,
                ia.ctypes.data if (ia is not None and n_q) else None, int(max_steps), Q, tq.ctypes.data if Q else None)
        q_nlp = np.asarray(self.integral[phase], dtype=np.float64).reshape(n_q)
        ends = seg[1:].astype(np.int64)
        if device is not None:
            import torch
            new = lambda sh, dt=torch.float64: torch.empty(sh, dtype=dt, device=device)   # noqa: E731
            y, qa, yd, qd = new((n_y, N)), new((n_q, N)), new((n_y, Q)), new((n_q, Q))
            acc, rej, status = new((N,), torch.int32), new((N,), torch.int32), new((n_seg,), torch.int32)
            ptr = lambda a: a.data_ptr() if a.numel() else None   # noqa: E731
            torch.cuda.current_stream(device).synchronize()     # the handle's stream is not torch's
            self._check(self._lib.pc_solution_propagate_dense_device(*head, ptr(y), ptr(acc), ptr(rej), ptr(status), ptr(qa),
                                                                     ptr(yd), ptr(qd)))
            self._check(self._lib.pc_synchronize(self.engine._h))
            integral = torch.as_tensor(_sum_ascending(qa[:, torch.as_tensor(ends, device=device)].cpu().numpy()), device=device)
            q_nlp = torch.as_tensor(q_nlp, device=device)
            tq_where = torch.as_tensor(tq, device=device)
        else:
            y, qa, yd, qd = np.empty((n_y, N)), np.empty((n_q, N)), np.empty((n_y, Q)), np.empty((n_q, Q))
            acc, rej, status = np.empty(N, dtype=np.int32), np.empty(N, dtype=np.int32), np.empty(n_seg, dtype=np.int32)
            ptr = lambda a: a.ctypes.data if a.size else None   # noqa: E731
            self._check(self._lib.pc_solution_propagate_dense(*head, ptr(y), ptr(acc), ptr(rej), ptr(status), ptr(qa), ptr(yd),
                                                              ptr(qd)))
            integral = _sum_ascending(qa[:, ends])
            tq_where = tq
        if Q:
            u_dense = self.sample(phase, tau=tq_where)[2]
        else:
            u_dense = yd.new_empty((pl.n_u, 0)) if device is not None else np.empty((pl.n_u, 0))
        return DensePropagation(y=y, accepted=acc, rejected=rej, segments=seg, status=status, q=qa, integral=integral,
                                integral_defect=integral - q_nlp, tau=tq, y_dense=yd, q_dense=qd, u_dense=u_dense,
                                **self._propagation_fields(phase, y, status, V, device))
