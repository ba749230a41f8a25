"""Symbolic side of the GPU KKT solve.

What it replaces: the sparse symmetric-indefinite factorisation inside IPOPT -- MUMPS by default -- that the reference
selects by name only (``linear_solver``, pycollo/backend.py:1703-1711, pycollo/settings.py:49-59).  One interior-point
iteration solves

    [ W + Sigma + dw I    J^T   ] [dv  ]   [r1]
    [ J                 -dc I   ] [dlam] = [r2]

with W = the Lagrangian Hessian H~, J = the constraint Jacobian G~ (plus -1 columns of the slacks of inequality rows).
The matrix is *quasi-definite* whenever the (1,1) block is positive definite, so L D L^T exists for every symmetric
ordering with 1 x 1 pivots, and the signs of D are the inertia IPOPT's regularisation is driven by.  That freedom is
spent on the collocation structure (no fill-reducing heuristic, no pivot search):

  leaf (p, k)     the nodes strictly inside a run of g consecutive mesh sections of phase p: their z, path slacks and
                  path multipliers, and the defect multipliers of the rows that end on those nodes.  Leaves touch each
                  other only through separators, so all leaves are eliminated at once (one workgroup each, dense).
  chain node      the section boundary node between two leaves (its z, path slacks / multipliers) and the defect
  (p, k)          multipliers of the rows that end on it.  After the leaves are gone these nodes form a
                  block-tridiagonal chain per phase, eliminated by cyclic reduction (log2 of its length levels, tables
                  in csrc/pc_kkt_cr.hpp; node by node in one workgroup per phase where a block is too large for the
                  level kernels) -- the only sequential part, which is why g > 1: g sections per leaf divide its length.
  border          everything global: integrals q, free times, static parameters, integral and endpoint multipliers,
                  endpoint slacks, and any endpoint variable an endpoint Hessian term couples across nodes.  Dense,
                  factorised last.

Every defect multiplier sits with the node its row ends on, i.e. next to the -W V entry that pairs it with that node's
state, so no block's multiplier part rests on the -dc I regularisation alone.

The table build is three stages, each a function of a record: ``classify`` (an NLP's unknowns -> ``NlpClassification``,
whose ``system`` is a ``Classified``: class, block and ordering keys per unknown -- the form a rank's part and the reduced
system of kkt_sharded.py have too), ``layout`` (``Classified`` -> ``Layout``: block order and value-buffer offsets, pure
arithmetic), and the entry tables under the position rule ``dest_numpy`` / ``dest_library``: ``entries_from_list`` for any
system with an explicit entry list, ``entries_of_nlp`` for a whole NLP in one pass of host C++.  ``make_tables`` puts a
layout and entry tables together; ``build_tables`` is the three in a row.

This module only builds index tables (NumPy); the numeric work is in ``csrc/pc_kkt.hip`` (``pc_kkt_*`` in
include/pycollo_amd.h).  ``oracle/ref_kkt.py`` holds a NumPy execution of the same tables for the tests.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

LEAF, CHAIN, BORDER = 0, 1, 2
SRC_G, SRC_H, SRC_ONE = 0, 1, 2


@dataclass
class KktTables:
    """Everything ``pc_kkt_create`` needs, as flat arrays (see ``pc_kkt_desc`` in include/pycollo_amd.h)."""
    nu: int                      # unknowns: nv primal (x, slacks) then m multipliers, natural order
    nv: int
    n_leaf: int
    n_chain: int
    n_phase: int
    nb: int                      # border size
    n_primal: int                # expected positive pivots (unit pivots of fixed unknowns included)
    n_dual: int                  # expected negative pivots
    # unknown -> block
    perm: np.ndarray             # [nu] natural index of every unknown in block order: leaves, chain nodes, border
    leaf_ptr: np.ndarray         # [n_leaf + 1] into perm
    chain_ptr: np.ndarray        # [n_chain + 1] into perm (offset by leaf_ptr[-1])
    chain_phase_ptr: np.ndarray  # [n_phase + 1] chain nodes of every phase (consecutive)
    leaf_left: np.ndarray        # [n_leaf] chain node on the left of a leaf; the right one is left + 1
    # value buffer layout (doubles)
    leafA_off: np.ndarray        # [n_leaf] A | C of a leaf, row stride m + w
    leafS_off: np.ndarray        # [n_leaf] Schur block of a leaf, w x w
    chainD_off: np.ndarray       # [n_chain] D | E | F of a chain node, row stride nzb + nzb_next + nb
    chainS_off: np.ndarray       # [n_chain] Schur block of a chain node, (nzb_next + nb)^2
    border_off: int
    total_vals: int
    # scatter recipe: destination runs
    dst: np.ndarray              # [n_dst] int64 position in the value buffer
    run_ptr: np.ndarray          # [n_dst + 1]
    src_kind: np.ndarray         # [n_src] int32 SRC_*
    src_idx: np.ndarray          # [n_src] int32 index into G~ / H~ values
    src_coef: np.ndarray         # [n_src] double
    diag_pos: np.ndarray         # [nu] position of every unknown's diagonal entry (natural order)
    fixed: np.ndarray            # [nu] uint8
    # full symmetric matrix as CSR over natural unknowns, for products K x (refinement, J^T lambda)
    mv_ptr: np.ndarray
    mv_col: np.ndarray
    mv_kind: np.ndarray
    mv_idx: np.ndarray
    mv_coef: np.ndarray
    chain_export: np.ndarray | None = None   # [n_chain] uint8: chain nodes that are not eliminated (kkt_sharded.py), or None


# The field specification of the tables, in the order of ``pc_kkt_desc``: what ``_Desc``, the marshalling of ``GpuKkt`` and
# the dtype normalisation of ``make_tables`` are made from.  (``chain_export`` is the one optional array: last in the
# structure, NULL unless a node is exported.)
SCALAR_FIELDS = ("nu", "nv", "n_leaf", "n_chain", "n_phase", "nb", "total_vals", "border_off")
COUNT_FIELDS = (("n_dst", "dst"), ("n_src", "src_kind"), ("n_mv", "mv_col"))        # (field of the structure, array it counts)
ARRAY_FIELDS = (("perm", np.int64), ("leaf_ptr", np.int64), ("chain_ptr", np.int64), ("chain_phase_ptr", np.int64),
                ("leaf_left", np.int64), ("leafA_off", np.int64), ("leafS_off", np.int64), ("chainD_off", np.int64),
                ("chainS_off", np.int64), ("dst", np.int64), ("run_ptr", np.int64), ("src_kind", np.int32),
                ("src_idx", np.int32), ("src_coef", np.float64), ("diag_pos", np.int64), ("fixed", np.uint8),
                ("mv_ptr", np.int64), ("mv_col", np.int32), ("mv_kind", np.int32), ("mv_idx", np.int32), ("mv_coef", np.float64))
_CTYPE = {np.dtype(np.int8): C.c_int8, np.dtype(np.int64): C.c_int64, np.dtype(np.int32): C.c_int32,
          np.dtype(np.float64): C.c_double, np.dtype(np.uint8): C.c_uint8}


def _pointer(arr):
    return arr.ctypes.data_as(C.POINTER(_CTYPE[arr.dtype]))


class NodeMap(NamedTuple):
    """One phase's nodes (``_node_maps``).  Chain nodes are counted from the phase's first."""
    s: np.ndarray             # leaf boundaries: every ``group``-th section boundary, restarting at every cut
    N: int                    # nodes of the phase
    is_boundary: np.ndarray   # [N] the node is a leaf boundary
    section: np.ndarray       # [N] the boundary at or before a node, i.e. the leaf of an interior node
    is_cut: np.ndarray        # [len(s)] the boundary is a cut
    chain_id: np.ndarray      # [len(s)] chain node of a boundary (the left copy of a cut)
    leaf_left: np.ndarray     # [len(s) - 1] chain node on the left of a leaf
    n_chain: int
    seg_ptr: np.ndarray       # first chain node of every segment and one past the last


@dataclass
class Classified:
    """A classified system: all the layout and entry stages need to know about a set of ``nu`` unknowns -- a whole NLP's,
    one rank's part of it, or the reduced border system (kkt_sharded.py)."""
    nu: int
    nv: int                      # goes into ``pc_kkt_desc`` as it is (0 for a rank's part and for the reduced system)
    cls: np.ndarray              # [nu] int8 LEAF / CHAIN / BORDER
    blk: np.ndarray              # [nu] leaf or chain node of the unknown (0 in the border)
    key_node: np.ndarray         # [nu] ordering inside a block: primal before dual, then node, kind, natural index
    key_kind: np.ndarray
    dual: np.ndarray             # [nu] bool
    fixed: np.ndarray            # [nu] bool
    n_leaf: int
    n_chain: int
    chain_phase_ptr: np.ndarray  # as in KktTables
    leaf_left: np.ndarray
    n_primal: int
    n_dual: int
    chain_export: np.ndarray | None = None


def border_system(nu, n_primal, n_dual) -> Classified:
    """``nu`` unknowns that are all border: one dense block."""
    z = np.zeros(nu, np.int64)
    return Classified(nu=nu, nv=0, cls=np.full(nu, BORDER, np.int8), blk=z, key_node=z, key_kind=z, dual=np.zeros(nu, bool),
                      fixed=np.zeros(nu, bool), n_leaf=0, n_chain=0, chain_phase_ptr=np.zeros(1, np.int64),
                      leaf_left=np.zeros(0, np.int64), n_primal=n_primal, n_dual=n_dual)


@dataclass
class NlpClassification:
    """``classify``: the classified system of a whole NLP and what only a whole NLP has."""
    system: Classified
    n: int                       # NLP variables, constraint rows, slacks (system.nv = n + ns, system.nu = n + ns + m)
    m: int
    ns: int
    ineq_rows: np.ndarray        # [ns] int64
    hr: np.ndarray               # structure of H~ (lower triangle) and of G~
    hc: np.ndarray
    jr: np.ndarray
    jc: np.ndarray
    maps: list                   # NodeMap per phase
    chain_base: np.ndarray       # [phases + 1] first chain node of a phase
    leaf_phase_ptr: np.ndarray   # [phases + 1] first leaf of a phase
    u_phase: np.ndarray          # [nu] the phase and node an unknown sits on (-1: none)
    u_node: np.ndarray
    group: list


def _node_maps(engine, group, cuts=None) -> list[NodeMap]:
    """Per phase: leaf boundaries (every ``group``-th section boundary, restarting at every cut), node -> (is boundary,
    leaf index), and the chain numbering.  ``cuts[ip]``: interior section-boundary nodes at which the phase's chain is cut
    (the sharded factorisation, kkt_sharded.py): a cut node's unknowns go to the border, and the node stands in the
    chain twice with no unknowns -- as the last node of the segment on its left and the first of the one on its right --
    so every segment is a chain of its own, exactly like a phase."""
    out = []
    for ip, (mesh, g) in enumerate(zip(engine.meshes, group)):
        s_all = np.asarray(mesh.s, dtype=np.int64)
        cut = np.zeros(0, np.int64) if cuts is None else np.unique(np.asarray(cuts[ip], dtype=np.int64))
        kc = np.searchsorted(s_all, cut)
        if len(cut) and (np.any(kc >= len(s_all)) or np.any(s_all[np.minimum(kc, len(s_all) - 1)] != cut)
                         or cut[0] <= 0 or cut[-1] >= s_all[-1]):
            raise ValueError(f"phase {ip}: a cut must be an interior section boundary")
        edges = np.concatenate([[0], kc, [len(s_all) - 1]]).astype(np.int64)
        s = np.unique(np.concatenate([s_all[a:b:g] for a, b in zip(edges[:-1], edges[1:])] + [s_all[-1:]]))
        N = int(s[-1]) + 1
        is_b = np.zeros(N, bool)
        is_b[s] = True
        sec = np.searchsorted(s, np.arange(N), side="right") - 1      # section whose start <= node
        is_cut = np.isin(s, cut)
        upto = np.cumsum(is_cut)
        before = upto - is_cut
        chain_id = np.arange(len(s), dtype=np.int64) + before
        leaf_left = (np.arange(len(s) - 1, dtype=np.int64) + upto[:-1]).astype(np.int64)
        n_chain = len(s) + int(is_cut.sum())
        seg_ptr = np.concatenate([[0], chain_id[is_cut] + 1, [n_chain]]).astype(np.int64)
        out.append(NodeMap(s, N, is_b, sec, is_cut, chain_id, leaf_left, n_chain, seg_ptr))
    return out


LEAF_TARGET = 72   # unknowns a leaf should hold: its dense [A | C] then fits the workgroup's 64 KB of LDS


def default_group(engine, ineq_rows) -> list[int]:
    """Sections per leaf, per phase.  The chain of separators is eliminated node after node by one workgroup per
    phase, ~10 us a node; a leaf costs its size cubed.  Merging g sections into a leaf divides the chain by g: g is the
    largest that keeps a typical leaf near LEAF_TARGET unknowns."""
    ineq = set(int(r) for r in np.asarray(ineq_rows).reshape(-1))
    out = []
    for pl, pm, mesh in zip(engine.layout.phases, engine.model.phases, engine.meshes):
        n_mean = float(np.mean(mesh.n))
        slack = sum(1 for mm in range(pm.n_p) if (pl.c_path_off + mm * pl.N) in ineq)
        per_node = pm.n_z + pm.n_p + slack + pm.n_y
        per_section = per_node * (n_mean - 1)
        out.append(int(max(1, min(64, LEAF_TARGET // max(1.0, per_section)))))
    return out


# ---- stage 1: classification of a whole NLP's unknowns ------------------------------------------------------------------
def classify(engine, ineq_rows, fixed_v, group=None, cuts=None) -> NlpClassification:
    """Leaf, chain node or border for every unknown of the NLP's KKT system (arguments as ``build_tables``)."""
    lay, model = engine.layout, engine.model
    if group is None:
        group = default_group(engine, ineq_rows)
    elif np.isscalar(group):
        group = [int(group)] * len(lay.phases)
    n, m = engine.num_x, engine.num_c
    ineq_rows = np.asarray(ineq_rows, dtype=np.int64)
    ns = len(ineq_rows)
    nv, nu = n + ns, n + ns + m
    fixed = np.zeros(nu, bool)
    fixed[:nv] = np.asarray(fixed_v, bool)
    maps = _node_maps(engine, group, cuts)
    chain_base = np.concatenate([[0], np.cumsum([mp.n_chain for mp in maps])]).astype(np.int64)
    leaf_phase_ptr = np.concatenate([[0], np.cumsum([len(mp.s) - 1 for mp in maps])]).astype(np.int64)
    n_chain, n_leaf = int(chain_base[-1]), int(leaf_phase_ptr[-1])
    # the chain's independent pieces: a phase, or with cuts a segment of one (what the tables call a phase of the chain)
    chain_phase_ptr = np.concatenate([chain_base[ip] + mp.seg_ptr[:-1] for ip, mp in enumerate(maps)] + [chain_base[-1:]]).astype(np.int64)

    cls = np.full(nu, BORDER, np.int8)
    blk = np.zeros(nu, np.int64)
    key_node = np.zeros(nu, np.int64)
    key_kind = np.zeros(nu, np.int64)
    dual = np.zeros(nu, bool)
    dual[nv:] = True
    u_phase = np.full(nu, -1, np.int64)
    u_node = np.full(nu, -1, np.int64)

    def place_nodes(u, ip, nodes):
        u_phase[u], u_node[u] = ip, nodes
        mp = maps[ip]
        b = mp.is_boundary[nodes]
        k = mp.section[nodes]
        cls[u] = np.where(b, np.where(mp.is_cut[k], BORDER, CHAIN), LEAF)
        blk[u] = np.where(b, chain_base[ip] + mp.chain_id[k], leaf_phase_ptr[ip] + k)
        key_node[u] = nodes

    row_slack = np.full(m, -1, np.int64)
    row_slack[ineq_rows] = np.arange(ns)
    for ip, (pl, pm) in enumerate(zip(lay.phases, model.phases)):
        N = maps[ip].N
        nz = pm.n_z
        u = pl.x_off + np.arange(nz * N, dtype=np.int64)
        place_nodes(u, ip, (u - pl.x_off) % N)
        key_kind[u] = 0
        # defect rows: the row of node i >= 1 goes with node i
        for a in range(pm.n_y):
            rows = pl.c_off + a * (N - 1) + np.arange(N - 1, dtype=np.int64)
            place_nodes(nv + rows, ip, np.arange(1, N, dtype=np.int64))
            key_kind[nv + rows] = 1
        for mm in range(pm.n_p):
            rows = pl.c_path_off + mm * N + np.arange(N, dtype=np.int64)
            place_nodes(nv + rows, ip, np.arange(N, dtype=np.int64))
            key_kind[nv + rows] = 0
            sl = row_slack[rows]
            has = sl >= 0
            if has.any():
                place_nodes(n + sl[has], ip, np.arange(N, dtype=np.int64)[has])
                key_kind[n + sl[has]] = 1
    # endpoint Hessian terms that couple two different nodes: both variables move to the border
    hr, hc = (np.asarray(a, np.int64) for a in engine.evaluate_H_structure())
    both_node = (cls[hr] != BORDER) & (cls[hc] != BORDER)
    cross = both_node & ((cls[hr] != cls[hc]) | (blk[hr] != blk[hc]))
    promoted = np.unique(np.concatenate([hr[cross], hc[cross]]))
    cls[promoted] = BORDER
    blk[cls == BORDER] = 0
    key_node[cls == BORDER] = 0
    leaf_left = np.concatenate([chain_base[ip] + mp.leaf_left for ip, mp in enumerate(maps)]).astype(np.int64) \
        if n_leaf else np.zeros(0, np.int64)
    jr, jc = (np.asarray(a, np.int64) for a in engine.evaluate_G_structure())
    system = Classified(nu=nu, nv=nv, cls=cls, blk=blk, key_node=key_node, key_kind=key_kind, dual=dual, fixed=fixed,
                        n_leaf=n_leaf, n_chain=n_chain, chain_phase_ptr=chain_phase_ptr, leaf_left=leaf_left,
                        n_primal=nv, n_dual=m)
    return NlpClassification(system=system, n=n, m=m, ns=ns, ineq_rows=ineq_rows, hr=hr, hc=hc, jr=jr, jc=jc, maps=maps,
                             chain_base=chain_base, leaf_phase_ptr=leaf_phase_ptr, u_phase=u_phase, u_node=u_node,
                             group=list(group))


# ---- stage 2: block order and value-buffer layout (arithmetic on the classification, no library call) -------------------
# ``layout``: block order (perm, leaf_ptr, chain_ptr, nb) and value-buffer offsets as in KktTables, and per unknown its index
# inside its block (local); per leaf its unknowns m_l and the width w_l of its C (both chain nodes and the border); per
# chain node its unknowns nzb, those of the next node of its phase nzb_next (0: last_of_phase), and wc = nzb_next + nb
Layout = namedtuple("Layout", "sys perm leaf_ptr chain_ptr local m_l w_l nzb nzb_next wc last_of_phase "
                              "leafA_off leafS_off chainD_off chainS_off nb border_off total_vals")


def _starts(base, sizes):
    """``base`` + the exclusive prefix sums of ``sizes``, and ``base`` + their sum."""
    c = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return base + c[:-1], base + int(c[-1])


def layout(S: Classified) -> Layout:
    """Block order and value-buffer layout of a classified system: arithmetic on the classification alone."""
    cls, blk, n_leaf = S.cls, S.blk, S.n_leaf
    perm = np.lexsort((S.key_kind, S.key_node, S.dual, blk, cls)).astype(np.int64)    # (stable: then by natural index)
    is_leaf, is_chain, is_border = cls == LEAF, cls == CHAIN, cls == BORDER
    counts_leaf = np.bincount(blk[is_leaf], minlength=n_leaf) if n_leaf else np.zeros(0, np.int64)
    counts_chain = np.bincount(blk[is_chain], minlength=S.n_chain)
    leaf_ptr = np.concatenate([[0], np.cumsum(counts_leaf)]).astype(np.int64)
    chain_ptr = np.concatenate([[0], np.cumsum(counts_chain)]).astype(np.int64)
    nb = int(np.sum(is_border))
    local = np.empty(S.nu, np.int64)
    pos = np.empty(S.nu, np.int64)
    pos[perm] = np.arange(S.nu)
    base_chain = int(leaf_ptr[-1])
    base_border = base_chain + int(chain_ptr[-1])
    local[is_leaf] = pos[is_leaf] - leaf_ptr[blk[is_leaf]]
    local[is_chain] = pos[is_chain] - base_chain - chain_ptr[blk[is_chain]]
    local[is_border] = pos[is_border] - base_border

    nzb = counts_chain.astype(np.int64)
    last_of_phase = np.zeros(S.n_chain, bool)
    last_of_phase[S.chain_phase_ptr[1:] - 1] = True
    nzb_next = np.where(last_of_phase, 0, np.concatenate([nzb[1:], [0]]))
    m_l = counts_leaf.astype(np.int64)
    w_l = (nzb[S.leaf_left] + nzb[S.leaf_left + 1] + nb) if n_leaf else np.zeros(0, np.int64)
    wc = nzb_next + nb
    # value buffer: A | C of every leaf, their Schur blocks, D | E | F of every chain node, their Schur blocks, the border
    leafA_off, o = _starts(0, m_l * (m_l + w_l))
    leafS_off, o = _starts(o, w_l * w_l)
    chainD_off, o = _starts(o, nzb * (nzb + wc))
    chainS_off, o = _starts(o, wc * wc)
    return Layout(sys=S, perm=perm, leaf_ptr=leaf_ptr, chain_ptr=chain_ptr, local=local, m_l=m_l, w_l=w_l, nzb=nzb,
                  nzb_next=nzb_next, wc=wc, last_of_phase=last_of_phase, leafA_off=leafA_off, leafS_off=leafS_off,
                  chainD_off=chainD_off, chainS_off=chainS_off, nb=nb, border_off=o, total_vals=o + nb * nb)


# ---- the position rule: where K[u, v] (u, v natural) lies in the value buffer ---------------------------------------------
def dest_numpy(L: Layout, u, v):
    """Position in the value buffer of K[u, v], vectorised; -1 where the pair has no place.  (The statement of the rule;
    ``positions="numpy"`` selects it, the CPU tests hold the library against it.)"""
    cls, blk, local, leaf_left = L.sys.cls, L.sys.blk, L.local, L.sys.leaf_left
    leafA_off, m_l, w_l, chainD_off, nzb, nzb_next, wc = L.leafA_off, L.m_l, L.w_l, L.chainD_off, L.nzb, L.nzb_next, L.wc
    cu, cv = cls[u], cls[v]
    # order the pair so that `a` is the one eliminated first: leaf < chain < border; inside a class lower block first
    swap = (cu > cv) | ((cu == cv) & (blk[u] > blk[v])) | ((cu == cv) & (blk[u] == blk[v]) & (local[u] < local[v]))
    a, b = np.where(swap, v, u), np.where(swap, u, v)
    ca, cb, ba, bb, la, lb = cls[a], cls[b], blk[a], blk[b], local[a], local[b]
    out = np.full(len(u), -1, np.int64)
    # leaf x leaf (same leaf): lower triangle of A (a has the larger local index after the swap rule above)
    k = (ca == LEAF) & (cb == LEAF) & (ba == bb)
    out[k] = leafA_off[ba[k]] + la[k] * (m_l[ba[k]] + w_l[ba[k]]) + lb[k]
    # leaf x chain
    k = (ca == LEAF) & (cb == CHAIN)
    left = leaf_left[ba[k]]
    col = np.where(bb[k] == left, lb[k], np.where(bb[k] == left + 1, nzb[left] + lb[k], -1))
    ok = col >= 0
    tmp = np.full(int(k.sum()), -1, np.int64)
    tmp[ok] = leafA_off[ba[k]][ok] + la[k][ok] * (m_l[ba[k]] + w_l[ba[k]])[ok] + m_l[ba[k]][ok] + col[ok]
    out[k] = tmp
    # leaf x border
    k = (ca == LEAF) & (cb == BORDER)
    left = leaf_left[ba[k]]
    out[k] = leafA_off[ba[k]] + la[k] * (m_l[ba[k]] + w_l[ba[k]]) + m_l[ba[k]] + nzb[left] + nzb[left + 1] + lb[k]
    # chain x chain
    k = (ca == CHAIN) & (cb == CHAIN) & (ba == bb)
    out[k] = chainD_off[ba[k]] + la[k] * (nzb[ba[k]] + wc[ba[k]]) + lb[k]
    k = (ca == CHAIN) & (cb == CHAIN) & (bb == ba + 1) & ~L.last_of_phase[ba]
    out[k] = chainD_off[ba[k]] + la[k] * (nzb[ba[k]] + wc[ba[k]]) + nzb[ba[k]] + lb[k]
    # chain x border
    k = (ca == CHAIN) & (cb == BORDER)
    out[k] = chainD_off[ba[k]] + la[k] * (nzb[ba[k]] + wc[ba[k]]) + nzb[ba[k]] + nzb_next[ba[k]] + lb[k]
    # border x border, lower
    k = (ca == BORDER) & (cb == BORDER)
    out[k] = L.border_off + la[k] * L.nb + lb[k]
    return out


PLAN_FIELDS = (("cls", np.int8), ("blk", np.int64), ("local", np.int64), ("leafA_off", np.int64), ("m_l", np.int64),
               ("w_l", np.int64), ("leaf_left", np.int64), ("chainD_off", np.int64), ("nzb", np.int64), ("nzb_next", np.int64),
               ("wc", np.int64), ("last_of_phase", np.uint8))      # the arrays of ``pc_kkt_plan``, in its order


class _Plan(C.Structure):
    _fields_ = ([(k, C.c_int64) for k in ("nu", "nb", "border_off")]
                + [(k, C.POINTER(_CTYPE[np.dtype(t)])) for k, t in PLAN_FIELDS])


def _library_plan(L: Layout):
    """The layout as the C structure ``pc_kkt_plan``: (library, structure, the arrays it points into)."""
    from .engine import load_library
    lib = load_library()
    lib.pc_kkt_plan_positions.argtypes = [C.POINTER(_Plan), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pc_kkt_plan_entries.argtypes = [C.POINTER(_Plan), C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p] + [C.c_void_p] * 11
    lib.pc_kkt_last_error.restype = C.c_char_p
    P = _Plan()
    P.nu, P.nb, P.border_off = int(L.sys.nu), int(L.nb), int(L.border_off)
    keep = []
    for name, typ in PLAN_FIELDS:
        a = np.ascontiguousarray(getattr(L.sys if name in ("cls", "blk", "leaf_left") else L, name), dtype=typ)
        keep.append(a if a.size else np.zeros(1, typ))
        setattr(P, name, _pointer(keep[-1]))
    return lib, P, keep


def dest_library(L: Layout, u, v, plan=None):
    """The same rule as ``dest_numpy`` in one pass of host C++ (``pc_kkt_plan_positions``): the vectorised form
    allocates ~100 temporaries of the entry count each, and their first-touch page faults were most of a table
    build inside a solve (95 of 110 ms at config 2).  ``plan``: a ``_library_plan(L)`` the caller already has."""
    lib, P, _keepalive = plan or _library_plan(L)
    u = np.ascontiguousarray(u, dtype=np.int64)
    v = np.ascontiguousarray(v, dtype=np.int64)
    out = np.empty(len(u), np.int64)
    if not lib.pc_kkt_plan_positions(C.byref(P), len(u), u.ctypes.data, v.ctypes.data, out.ctypes.data):
        raise RuntimeError(lib.pc_kkt_last_error().decode())
    return out


# ---- stage 3: the entry tables ----------------------------------------------------------------------------------------
# the scatter recipe, the diagonal's positions and the symmetric CSR matrix: the fields of KktTables of these names
EntryTables = namedtuple("EntryTables", "dst run_ptr src_kind src_idx src_coef diag_pos mv_ptr mv_col mv_kind mv_idx mv_coef")
NO_ENTRIES = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0))


def natural_entries(nlp: NlpClassification, row_scale):
    """Lower-triangle entries of K over natural unknowns as (row, column, source kind, source index, coefficient):
    H~, the row-scaled G~, the -1 of every slack -- without those of a fixed unknown."""
    nv, ns, hr, jr, fixed = nlp.system.nv, nlp.ns, nlp.hr, nlp.jr, nlp.system.fixed
    eu = np.concatenate([hr, nv + jr, nv + nlp.ineq_rows])
    ev = np.concatenate([nlp.hc, nlp.jc, nlp.n + np.arange(ns, dtype=np.int64)])
    ekind = np.concatenate([np.full(len(hr), SRC_H), np.full(len(jr), SRC_G), np.full(ns, SRC_ONE)]).astype(np.int32)
    eidx = np.concatenate([np.arange(len(hr)), np.arange(len(jr)), np.zeros(ns, np.int64)]).astype(np.int64)
    ecoef = np.concatenate([np.ones(len(hr)), np.asarray(row_scale, float)[jr], -np.ones(ns)])
    keep = ~(fixed[eu] | fixed[ev])
    return eu[keep], ev[keep], ekind[keep], eidx[keep], ecoef[keep]


def entries_from_list(L: Layout, entries, positions: str) -> EntryTables:
    """The entry tables of any classified system from its lower-triangle entries (``natural_entries`` form), in NumPy:
    the statement of the rule.  ``positions``: "numpy", or "positions" to take the position rule alone from the library."""
    if positions not in ("positions", "numpy"):
        raise ValueError("explicit entries need positions='positions' or 'numpy'")
    dest = {"positions": dest_library, "numpy": dest_numpy}[positions]
    nu = L.sys.nu
    eu, ev, ekind, eidx, ecoef = entries
    d = dest(L, eu, ev)
    if np.any(d < 0):
        bad = np.nonzero(d < 0)[0][0]
        raise RuntimeError(f"KKT entry ({eu[bad]}, {ev[bad]}) couples two blocks the elimination order keeps apart")
    so = np.argsort(d, kind="stable")
    d_sorted = d[so]
    first = np.concatenate([[True], d_sorted[1:] != d_sorted[:-1]]) if len(d) else np.zeros(0, bool)
    run_ptr = np.concatenate([np.nonzero(first)[0], [len(d_sorted)]]).astype(np.int64)
    diag_pos = dest(L, np.arange(nu, dtype=np.int64), np.arange(nu, dtype=np.int64))
    # full symmetric CSR over natural unknowns (products)
    off = eu != ev
    ru = np.concatenate([eu, ev[off]])
    rv = np.concatenate([ev, eu[off]])
    rk = np.concatenate([ekind, ekind[off]])
    ri = np.concatenate([eidx, eidx[off]])
    rc = np.concatenate([ecoef, ecoef[off]])
    # row-major order of the entries, columns ascending inside a row: one sort of the combined key (no pair occurs
    # twice -- checked -- so the order is unique; np.lexsort over the two keys took 60-90 of the 150 ms of a 15 k-node
    # build, a merge sort of the one int64 key -- the entries arrive as a few long sorted runs -- 17)
    key = ru * np.int64(nu) + rv
    o2 = np.argsort(key, kind="stable")
    ks = key[o2]
    if len(ks) > 1 and np.any(ks[1:] == ks[:-1]):
        raise RuntimeError("a KKT entry occurs twice in the symmetric expansion")
    mv_ptr = np.concatenate([[0], np.cumsum(np.bincount(ru, minlength=nu))]).astype(np.int64)
    return EntryTables(d_sorted[first], run_ptr, ekind[so], eidx[so], ecoef[so], diag_pos, mv_ptr, rv[o2], rk[o2], ri[o2], rc[o2])


def entries_of_nlp(L: Layout, nlp: NlpClassification, row_scale) -> EntryTables:
    """The entry tables of a whole NLP in one pass of host C++ (``pc_kkt_plan_entries``): ``entries_from_list`` builds them
    from a dozen entry-sized temporaries, sorts twice and gathers nine times -- 150 ms for 15 k nodes, and several times
    that whenever the allocator has to fault the temporaries in afresh, which inside a solve is every time."""
    lib, P, _keepalive = plan = _library_plan(L)
    nu = L.sys.nu
    hr, hc, jr, jc, iq = (np.ascontiguousarray(a, dtype=np.int64) for a in (nlp.hr, nlp.hc, nlp.jr, nlp.jc, nlp.ineq_rows))
    rs = np.ascontiguousarray(row_scale, dtype=np.float64)
    fx = np.ascontiguousarray(L.sys.fixed, dtype=np.uint8)
    counts = np.zeros(3, np.int64)
    # one call with outputs sized for the most there can be (np.empty touches no page), trimmed afterwards
    cap = len(hr) + len(jr) + nlp.ns
    dst, run_ptr = np.empty(cap, np.int64), np.empty(cap + 1, np.int64)
    src_kind, src_idx, src_coef = np.empty(cap, np.int32), np.empty(cap, np.int32), np.empty(cap, np.float64)
    mv_ptr, mv_col = np.empty(nu + 1, np.int64), np.empty(2 * cap, np.int32)
    mv_kind, mv_idx, mv_coef = np.empty(2 * cap, np.int32), np.empty(2 * cap, np.int32), np.empty(2 * cap, np.float64)
    outs = (dst, run_ptr, src_kind, src_idx, src_coef, mv_ptr, mv_col, mv_kind, mv_idx, mv_coef)
    if not lib.pc_kkt_plan_entries(C.byref(P), int(nlp.n), int(L.sys.nv), len(hr), hr.ctypes.data, hc.ctypes.data, len(jr), jr.ctypes.data,
                                   jc.ctypes.data, rs.ctypes.data, int(nlp.ns), iq.ctypes.data, fx.ctypes.data, counts.ctypes.data,
                                   *[o.ctypes.data for o in outs]):
        raise RuntimeError(lib.pc_kkt_last_error().decode())
    n_src, n_dst, n_mv = (int(c) for c in counts)
    ar = np.arange(nu, dtype=np.int64)
    return EntryTables(dst[:n_dst], run_ptr[:n_dst + 1], src_kind[:n_src], src_idx[:n_src], src_coef[:n_src],
                       dest_library(L, ar, ar, plan), mv_ptr, mv_col[:n_mv], mv_kind[:n_mv], mv_idx[:n_mv], mv_coef[:n_mv])


# ---- the tables ---------------------------------------------------------------------------------------------------------
def make_tables(L: Layout, E: EntryTables) -> KktTables:
    """The one place a ``KktTables`` is made: every array in the type ``ARRAY_FIELDS`` states."""
    S = L.sys
    src = {**vars(S), **L._asdict(), **E._asdict()}
    return KktTables(nu=S.nu, nv=S.nv, n_leaf=S.n_leaf, n_chain=S.n_chain, n_phase=len(S.chain_phase_ptr) - 1, nb=L.nb,
                     n_primal=S.n_primal, n_dual=S.n_dual, border_off=int(L.border_off), total_vals=int(L.total_vals),
                     chain_export=S.chain_export, **{k: np.asarray(src[k], dtype=t) for k, t in ARRAY_FIELDS})


def system_tables(S: Classified, entries, positions: str) -> KktTables:
    """Layout and entry tables of a classified system with an explicit entry list (``entries_from_list``)."""
    L = layout(S)
    return make_tables(L, entries_from_list(L, entries, positions))


def build_tables(engine, ineq_rows, fixed_v, row_scale, group=None, positions: str = "library", cuts=None) -> KktTables:
    """``ineq_rows``: constraint rows with a slack (in order); ``fixed_v`` [n + ns]: primal unknowns held fixed;
    ``row_scale`` [m]: the solver's constraint-row scaling (multiplies G~ row-wise); ``group``: mesh sections per leaf
    (int or one per phase; default ``default_group``); ``cuts``: per phase the nodes at which the chain is cut
    (``_node_maps``; ``n_phase`` of the result then counts chain segments).  ``positions``: "library" (the entry tables
    in one pass of host C++), or "positions" / "numpy" (``entries_from_list``)."""
    nlp = classify(engine, ineq_rows, fixed_v, group, cuts)
    if positions != "library":
        return system_tables(nlp.system, natural_entries(nlp, row_scale), positions)
    L = layout(nlp.system)
    return make_tables(L, entries_of_nlp(L, nlp, row_scale))


def export_shapes(T: KktTables):
    """(chain node, its unknowns, unknowns of the exported last node of its segment it is coupled to) for every exported
    chain node, ascending: the layout of ``pc_kkt_export_panels``."""
    if T.chain_export is None:
        return []
    nzb = np.diff(T.chain_ptr)
    out = []
    for c in np.nonzero(T.chain_export)[0]:
        seg = int(np.searchsorted(T.chain_phase_ptr, c, side="right") - 1)
        last = int(T.chain_phase_ptr[seg + 1] - 1)
        nr = int(nzb[last]) if (c == T.chain_phase_ptr[seg] and last != c and T.chain_export[last]) else 0
        out.append((int(c), int(nzb[c]), nr))
    return out


class _Desc(C.Structure):
    _fields_ = ([(k, C.c_int64) for k in SCALAR_FIELDS + tuple(k for k, _ in COUNT_FIELDS)]
                + [(k, C.POINTER(_CTYPE[np.dtype(t)])) for k, t in ARRAY_FIELDS] + [("chain_export", C.POINTER(C.c_uint8))])


class _KktInfo(C.Structure):
    _fields_ = [("n_leaf", C.c_int64), ("n_chain", C.c_int64), ("nb", C.c_int64), ("n_mv_long", C.c_int64),
                ("chain_cr", C.c_int32), ("cr_levels", C.c_int32), ("cr_top_levels", C.c_int32), ("cr_top_waves", C.c_int32),
                ("border_blocks", C.c_int32), ("leaf_forward_stage", C.c_int32), ("leaf_waves", C.c_int32),
                ("reserved", C.c_int32)]


def _descriptor(T: KktTables):
    """``pc_kkt_desc`` of the tables, and the arrays it points into (to be kept alive as long as it is used)."""
    d = _Desc()
    keep = []
    for k in SCALAR_FIELDS:
        setattr(d, k, int(getattr(T, k)))
    for k, counted in COUNT_FIELDS:
        setattr(d, k, len(getattr(T, counted)))
    for k, typ in ARRAY_FIELDS:
        arr = np.ascontiguousarray(getattr(T, k), dtype=typ)
        keep.append(arr if arr.size else np.zeros(1, dtype=typ))
        setattr(d, k, _pointer(keep[-1]))
    if T.chain_export is not None and np.any(T.chain_export):
        keep.append(np.ascontiguousarray(T.chain_export, dtype=np.uint8))
        d.chain_export = _pointer(keep[-1])
    return d, keep


def _info_dict(info) -> dict:
    return {k: int(getattr(info, k)) for k, _ in _KktInfo._fields_ if k != "reserved"}


def shape_info(tables: KktTables) -> dict:
    """What ``GpuKkt.info`` of a fresh handle on ``tables`` would say, decided on the host alone (``pc_kkt_shape_info``:
    no GPU is touched) under the current ``PYCOLLO_AMD_KKT_*`` environment; ``leaf_forward_stage`` is what the first
    solve will pick.  Raises what ``pc_kkt_create`` would refuse."""
    from .engine import load_library
    lib = load_library()
    lib.pc_kkt_last_error.restype = C.c_char_p
    lib.pc_kkt_shape_info.argtypes = [C.POINTER(_Desc), C.POINTER(_KktInfo)]
    d, keep = _descriptor(tables)
    info = _KktInfo()
    if not lib.pc_kkt_shape_info(C.byref(d), C.byref(info)):
        raise RuntimeError("pc_kkt_shape_info failed: " + lib.pc_kkt_last_error().decode())
    del keep
    return _info_dict(info)


class GpuKkt:
    """The factorisation object: ``pc_kkt_*`` bound to one engine's device-resident G~ / H~."""

    def __init__(self, engine, ineq_rows, fixed_v, row_scale, group=None, tables=None, d_jac=None, d_hess=None):
        """``tables``: ready-made tables instead of the whole NLP's (a rank's part of a sharded factorisation,
        kkt_sharded.py); ``d_jac`` / ``d_hess``: device addresses of the G~ / H~ values to read instead of the engine's."""
        from .engine import load_library
        if engine.device < 0:
            raise RuntimeError("the KKT solver needs a GPU engine; pycollo_amd has no CPU fallback")
        self.engine = engine
        import time
        t0 = time.perf_counter()
        self.tables = T = tables if tables is not None else build_tables(engine, ineq_rows, fixed_v, row_scale, group)
        self.seconds_tables = time.perf_counter() - t0          # host: the elimination plan as index tables
        self._lib = lib = load_library()
        vp = C.c_void_p
        lib.pc_kkt_last_error.restype = C.c_char_p
        lib.pc_kkt_create.argtypes = [C.POINTER(_Desc), vp, vp, C.c_int, C.POINTER(vp)]
        lib.pc_kkt_destroy.argtypes = [vp]
        lib.pc_kkt_destroy.restype = None
        lib.pc_kkt_get_info.argtypes = [vp, C.POINTER(_KktInfo)]
        lib.pc_kkt_factor.argtypes = [vp, C.c_int, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        lib.pc_kkt_solve.argtypes = [vp, vp, vp]
        lib.pc_kkt_matvec.argtypes = [vp, C.c_int, vp, vp, vp]
        lib.pc_kkt_solve_refined.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, C.POINTER(C.c_int32)]
        lib.pc_device_results.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        lib.pc_kkt_factor_partial.argtypes = [vp, C.c_int, vp, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        lib.pc_kkt_border_load_factor.argtypes = [vp, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        lib.pc_kkt_forward_partial.argtypes = [vp, vp, vp]
        lib.pc_kkt_backward_partial.argtypes = [vp, vp, vp]
        lib.pc_kkt_export_panels.argtypes = [vp, vp]
        lib.pc_kkt_export_rhs.argtypes = [vp, vp]
        lib.pc_kkt_import_solution.argtypes = [vp, vp]
        d, self._keep = _descriptor(T)
        self._export_shapes = export_shapes(T)
        dg, dj, dh = vp(), vp(), vp()
        if not lib.pc_device_results(engine._h, C.byref(dg), C.byref(dj), C.byref(dh)):
            raise RuntimeError(lib.pc_last_error().decode())
        if d_jac is not None:
            dj = vp(int(d_jac))
        if d_hess is not None:
            dh = vp(int(d_hess))
        self._h = vp()
        if not lib.pc_kkt_create(C.byref(d), dj, dh, int(engine.device), C.byref(self._h)):
            raise RuntimeError("pc_kkt_create failed: " + lib.pc_kkt_last_error().decode())
        self.nu = T.nu
        self.seconds_create = time.perf_counter() - t0 - self.seconds_tables   # descriptor + device allocation / upload

    def _check(self, ok):
        if not ok:
            raise RuntimeError(self._lib.pc_kkt_last_error().decode())

    @property
    def info(self) -> dict:
        """Which builds of the solver the handle runs (``pc_kkt_info``): block counts, the chain's cyclic reduction and
        the levels its substitutions run in one launch, the grid that sums the border terms, the staging of the last
        leaf forward elimination (-1 before the first solve), the waves per leaf of the factorisation."""
        info = _KktInfo()
        self._check(self._lib.pc_kkt_get_info(self._h, C.byref(info)))
        return _info_dict(info)

    def factor(self, dvec, use_hess=True):
        """Assemble from the engine's current device G~ / H~ and factorise; returns (n_pos, n_neg) pivots."""
        dvec = np.ascontiguousarray(dvec, dtype=np.float64)
        p, q = C.c_int32(), C.c_int32()
        self._check(self._lib.pc_kkt_factor(self._h, int(bool(use_hess)), dvec.ctypes.data, C.byref(p), C.byref(q)))
        return p.value, q.value

    def solve(self, rhs):
        rhs = np.ascontiguousarray(rhs, dtype=np.float64)
        x = np.empty(self.nu)
        self._check(self._lib.pc_kkt_solve(self._h, rhs.ctypes.data, x.ctypes.data))
        return x

    def matvec(self, dvec, x, use_hess=True):
        dvec = np.ascontiguousarray(dvec, dtype=np.float64)
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty(self.nu)
        self._check(self._lib.pc_kkt_matvec(self._h, int(bool(use_hess)), dvec.ctypes.data, x.ctypes.data, y.ctypes.data))
        return y

    def solve_refined(self, rhs, dvec_true, use_hess=True, max_steps=3):
        """``K^-1 rhs`` with the current factors, iteratively refined on the device against the system with
        ``dvec_true`` on its diagonal (``pc_kkt_solve_refined``); returns (x, back-substitutions performed)."""
        rhs = np.ascontiguousarray(rhs, dtype=np.float64)
        dvec_true = np.ascontiguousarray(dvec_true, dtype=np.float64)
        x = np.empty(self.nu)
        n = C.c_int32()
        self._check(self._lib.pc_kkt_solve_refined(self._h, int(bool(use_hess)), dvec_true.ctypes.data, rhs.ctypes.data,
                                                   int(max_steps), x.ctypes.data, C.byref(n)))
        return x, n.value

    # ---- a rank's part of a factorisation cut across ranks (kkt_sharded.py) ------------------------------------------
    def factor_partial(self, dvec, use_hess=True):
        """Assemble, eliminate the leaves and the chain, and return the border block with every Schur complement added
        but *not* factorised ([nb, nb], lower triangle valid), plus the (positive, negative) pivots so far."""
        dvec = np.ascontiguousarray(dvec, dtype=np.float64)
        nb = self.tables.nb
        B = np.zeros((nb, nb))
        p, q = C.c_int32(), C.c_int32()
        self._check(self._lib.pc_kkt_factor_partial(self._h, int(bool(use_hess)), dvec.ctypes.data, B.ctypes.data,
                                                    C.byref(p), C.byref(q)))
        return B, p.value, q.value

    def border_load_factor(self, B):
        """Take the border block as given (lower triangle read) and factorise it; returns its pivot counts."""
        B = np.ascontiguousarray(B, dtype=np.float64)
        if B.shape != (self.tables.nb, self.tables.nb):
            raise ValueError("border block of the wrong shape")
        p, q = C.c_int32(), C.c_int32()
        self._check(self._lib.pc_kkt_border_load_factor(self._h, B.ctypes.data, C.byref(p), C.byref(q)))
        return p.value, q.value

    def forward_partial(self, rhs):
        """Forward elimination through leaves and chain; returns the border's right-hand side minus what they owe it."""
        rhs = np.ascontiguousarray(rhs, dtype=np.float64)
        rb = np.empty(self.tables.nb)
        self._check(self._lib.pc_kkt_forward_partial(self._h, rhs.ctypes.data, rb.ctypes.data))
        return rb

    def backward_partial(self, xb):
        """Back-substitution from the given border solution (block order); returns the whole local solution."""
        xb = np.ascontiguousarray(xb, dtype=np.float64)
        if xb.shape != (self.tables.nb,):
            raise ValueError("border solution of the wrong length")
        x = np.empty(self.nu)
        self._check(self._lib.pc_kkt_backward_partial(self._h, xb.ctypes.data, x.ctypes.data))
        return x

    def export_panels(self):
        """After ``factor_partial``: the assembled panels [D | K(node, exported last node) | F] of the exported chain nodes,
        in ascending node order (``export_shapes``)."""
        out = np.zeros(sum(nz * (nz + nr + self.tables.nb) for _, nz, nr in self._export_shapes) or 1)
        self._check(self._lib.pc_kkt_export_panels(self._h, out.ctypes.data))
        panels, o = [], 0
        for _, nz, nr in self._export_shapes:
            n = nz * (nz + nr + self.tables.nb)
            panels.append(out[o:o + n].reshape(nz, nz + nr + self.tables.nb))
            o += n
        return panels

    def export_rhs(self):
        """After ``forward_partial``: the exported nodes' right-hand sides minus what the eliminated blocks owe them."""
        out = np.zeros(sum(nz for _, nz, _ in self._export_shapes) or 1)
        self._check(self._lib.pc_kkt_export_rhs(self._h, out.ctypes.data))
        return out[:sum(nz for _, nz, _ in self._export_shapes)]

    def import_solution(self, x):
        """Before ``backward_partial``: the exported nodes' solution (concatenated in node order)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape != (sum(nz for _, nz, _ in self._export_shapes),):
            raise ValueError("exported solution of the wrong length")
        if x.size:
            self._check(self._lib.pc_kkt_import_solution(self._h, x.ctypes.data))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pc_kkt_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
