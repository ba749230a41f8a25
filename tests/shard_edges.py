"""Partitions of the sharded evaluation (pycollo_amd/sharding.py) at which a rank's share degenerates: tiny meshes cut
with PYCOLLO_AMD_TILE_NODES=6 -- one order-4 or order-5 section fills a tile, three order-2 sections do -- over enough
ranks that ranks idle, own tiles in some phases only, or own exactly one tile.  A solved mesh of a few hundred nodes over
several phases is sharded like this.  Shared by tests/test_local_shard_cpu.py (host side) and
tests/test_gpu_shard_edges.py (the kernels); ``check_situation`` asserts from the computed tile ranges that a case still
exhibits what it is listed for, so that a change to ``tile_cuts`` or to the tile cutter cannot empty it of its point."""
import numpy as np

from pycollo_amd import problems

TILE_NODES = 6
# the environment knobs that change how pc_create cuts and launches tiles: cleared, then PYCOLLO_AMD_TILE_NODES set
KNOBS = ("PYCOLLO_AMD_WPT", "PYCOLLO_AMD_RESIDENT", "PYCOLLO_AMD_TAIL_BLOCKS", "PYCOLLO_AMD_MERGE", "PYCOLLO_AMD_TILE_NODES",
         "PYCOLLO_AMD_TB", "PYCOLLO_AMD_TWO_WAVE")

MIXED_ORDERS = (4, 4, 6, 6, 2, 5, 4)

# id -> (problem, sections per phase, section order (or the order list), world, quadrature method, mixed spec,
#        expected tiles per phase)
CASES = {
    "two_phase_w3": ("two_phase_transfer", (5, 2), 4, 3, "lobatto", None, [5, 2]),
    "two_phase_w8": ("two_phase_transfer", (5, 2), 4, 8, "lobatto", None, [5, 2]),
    "time_coupled_w4": ("time_coupled_transfer", (1, 6), 4, 4, "lobatto", None, [1, 6]),
    "delta_iii_w3": ("delta_iii", (3, 1, 2, 1), 5, 3, "lobatto", None, [3, 1, 2, 1]),
    "hyper_order2_w4": ("hypersensitive", (6,), 2, 4, "lobatto", None, [2]),
    "hyper_radau_w3": ("hypersensitive", (7,), 5, 3, "radau", None, [7]),
    "hyper_mixed_w4": ("hypersensitive", (7,), MIXED_ORDERS, 4, "lobatto", ((4, 6),), [6]),
}
IDS = list(CASES)


def set_environment(monkeypatch):
    """Before any handle is made: the plan-only handle of ``global_tile_plan``, the whole-NLP handle and the rank-local
    handles read the same environment, so all of them cut the same tiles."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("PYCOLLO_AMD_TILE_NODES", str(TILE_NODES))


def make_problem(case):
    name, Ks, order, _, method, _, _ = CASES[case]
    prob = problems.REGISTRY[name](K=max(Ks), order=order if np.ndim(order) == 0 else 4)
    for ph, K in zip(prob.phases, Ks):
        ph.mesh.number_mesh_sections = K
        ph.mesh.mesh_section_sizes = np.full(K, 1.0 / K)
        ph.mesh.number_mesh_section_nodes = np.full(K, order) if np.ndim(order) == 0 else np.asarray(order)
    prob.quadrature_method = method
    return prob


def world_of(case):
    return CASES[case][3]


def mixed_of(case):
    return CASES[case][5]


def x_range(case):
    return (0.05, 0.3) if CASES[case][0] == "delta_iii" else (-0.45, 0.45)   # Delta III: keep |r| away from 0 for mu / r^3


def _shape(plan, meshes, r, ip):
    """(tiles, halo section before, halo section after, owns the phase-final node) of rank r's range in phase ip; the
    halo entries are the sections' orders, or None without a halo (sharding.LocalShard cuts the same way)."""
    tb, te = plan.tile_ranges[r][ip]
    k0 = plan.tiles[ip][0]
    mesh = meshes[ip]
    if te <= tb:
        return 0, None, None, False
    ka, kb = int(k0[tb]), int(k0[te])
    return te - tb, (int(mesh.n[ka - 1]) if ka > 0 else None), (int(mesh.n[kb]) if kb < mesh.K else None), kb == mesh.K


def check_situation(case, plan, meshes, model):
    """``plan``: the ShardPlan of the case's world; asserts the situation the case is listed for."""
    world, n_ph = plan.world, len(plan.tiles)
    assert world == world_of(case)
    tiles = [len(k0) - 1 for k0, _ in plan.tiles]
    assert tiles == CASES[case][6], tiles
    shape = [[_shape(plan, meshes, r, ip) for ip in range(n_ph)] for r in range(world)]
    owned = [[ip for ip in range(n_ph) if shape[r][ip][0]] for r in range(world)]     # phases with tiles, per rank
    idle = [r for r in range(world) if not owned[r]]
    assert [r for r in range(world) if plan.lengths[r] == 0] == idle
    for ip in range(n_ph):                                                            # the ranges tile every phase
        rs = [plan.tile_ranges[r][ip] for r in range(world)]
        assert rs[0][0] == 0 and rs[-1][1] == tiles[ip] and all(a[1] == b[0] for a, b in zip(rs, rs[1:]))
    if case == "two_phase_w3":
        assert idle == [] and n_ph == 2                      # every rank busy,
        assert owned[2] == [0]                               # rank 2 with an empty LAST phase
        assert owned[0] == [0, 1] and owned[1] == [0, 1]
    elif case == "two_phase_w8":
        assert idle == [2, 5, 7]
        assert shape[0][0] == (1, None, 4, False)                         # one first tile: no leading halo
        assert owned[1] == [0] and shape[1][0] == (1, 4, 4, False)        # one interior tile, both halos; empty last phase
        assert owned[6] == [0] and shape[6][0] == (1, 4, None, True)      # one last tile: the phase-final node, no trailing halo
    elif case == "time_coupled_w4":
        assert meshes[0].K == 1 and tiles[0] == 1            # a one-section phase
        assert owned[0] == [0, 1]
        assert owned[1] == [1] and owned[2] == [1] and owned[3] == [1]    # an empty FIRST phase of the merged launch
        pm = model.phases
        assert all(p.n_q > 0 and p.n_t > 0 for p in pm)      # q and the times are variables of both phases
    elif case == "delta_iii_w3":
        assert n_ph == 4
        assert owned[1] == [0, 2]                            # phases 1 (middle) and 3 (end) empty
        assert owned[2] == [0]
        assert owned[0] == [0, 1, 2, 3]
    elif case == "hyper_order2_w4":
        assert n_ph == 1 and idle == [1, 2]                  # a single phase: BULK, not BULK_ALL
        assert shape[0][0] == (1, None, 2, False) and shape[3][0] == (1, 2, None, True)   # halo sections of 2 nodes
    elif case == "hyper_radau_w3":
        assert model.quadrature_method == "radau" and idle == []
        assert all(shape[r][0][0] >= 2 for r in range(world))
        assert shape[1][0][1:] == (5, 5, False)
    elif case == "hyper_mixed_w4":
        spec = mixed_of(case)[0]
        befores = [shape[r][0][1] for r in range(world) if shape[r][0][1] is not None]
        afters = [shape[r][0][2] for r in range(world) if shape[r][0][2] is not None]
        halos = befores + afters
        assert 6 in halos and 6 in spec                      # a halo section whose order is in the spec, before a cut
        assert 6 in befores
        assert set(halos) - set(spec) == {2, 5}              # ... and halo sections whose order is not
        assert any(shape[r][0][0] == 1 for r in range(world))                            # ranks of one tile
    else:
        raise AssertionError(case)
