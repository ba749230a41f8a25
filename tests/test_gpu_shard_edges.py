"""The sharded evaluation where a rank's share degenerates (run with -m gpu on an MI355X): the partitions of
tests/shard_edges.py -- idle ranks, ranks that own tiles in some phases only (an empty first, middle or last range of the
merged launch), ranks of exactly one tile (a phase's first, an interior one, its last), halo sections of 2 nodes, Radau
tables and a mixed build on rank-local handles.  A solved mesh of a few hundred nodes over several phases is sharded
like this; the other sharding tests give every rank several tiles in every phase.

Per case, on one whole-NLP handle: (a) the unsharded evaluation is held to the oracle at this mesh -- the bitwise
comparisons are worth what that reference is worth; (b) ranks emulated on the whole-NLP handle (``set_tile_range`` +
``launch_bulk_only``) write their own share and nothing else, and reassemble to the unsharded bits; (c) rank-local handles
(``LocalShard``) do the same from their own part of the mesh.  ``pc_copy_runs`` is tested on its own at the end."""
import types

import numpy as np
import pytest

import shard_edges
from conftest import entry_err, golden_tables, vec_err
from oracle.ref_numpy import OracleNlp

pytestmark = pytest.mark.gpu
TOL = 1e-10
SIGMA, W_J = 0.9, 1.3


@pytest.fixture(scope="module", params=shard_edges.IDS)
def edge(request, built):
    """One case: the whole-NLP handle (alive for the three checks), the inputs of tests/test_gpu_local_shard.py, the
    unsharded outputs and the plan, held to the situation the case is listed for."""
    from pycollo_amd.engine import NlpEngine
    from pycollo_amd.sharding import ShardPlan
    case = request.param
    mp = pytest.MonkeyPatch()
    shard_edges.set_environment(mp)       # stays set for the three checks: the rank-local handles read it too
    eng = None
    try:
        prob = shard_edges.make_problem(case)
        mixed = shard_edges.mixed_of(case)
        eng = NlpEngine(prob, device=0, **({"mixed": mixed} if mixed else {}))
        rng = np.random.default_rng(4)
        lo, hi = shard_edges.x_range(case)
        x = rng.uniform(lo, hi, eng.num_x)
        lam = rng.normal(size=eng.num_c)
        W = rng.uniform(0.5, 2.0, eng.layout.num_ocp_c)
        eng.set_scaling(eng.V_ocp, eng.r_ocp, W, W_J)
        c, G, H = (a.copy() for a in eng.evaluate_all(x, SIGMA, lam))
        plan = ShardPlan(eng, shard_edges.world_of(case))
        shard_edges.check_situation(case, plan, eng.meshes, eng.model)
        yield types.SimpleNamespace(case=case, prob=prob, eng=eng, x=x, lam=lam, W=W, c=c, G=G, H=H, plan=plan,
                                    world=plan.world)
    finally:
        if eng is not None:
            eng.close()
        mp.undo()


def test_unsharded_evaluation_matches_the_oracle(edge):
    """(a) What test_gpu_parity._check_all asks, at the point whose bits (b) and (c) compare: c~, G~, H~ entry by entry
    (conftest.entry_err <= 1), the separate callbacks, J, grad J (vec_err <= 1) and the index arrays equal."""
    eng, x, lam = edge.eng, edge.x, edge.lam
    ora = OracleNlp(edge.prob, golden_tables(edge.prob.quadrature_method), V_ocp=eng.V_ocp, r_ocp=eng.r_ocp, W_ocp=edge.W, w_J=W_J)
    cr, Gr, Hr = ora.c(x), ora.G(x), ora.H(x, SIGMA, lam)
    cm, Gm, Hm = ora.c_mag(x), ora.G_mag(x), ora.H_mag(x, SIGMA, lam)
    errs = (entry_err(edge.c, cr, cm), entry_err(edge.G, Gr, Gm), entry_err(edge.H, Hr, Hm))
    print(f"\n   {edge.case}: c {errs[0]:.2e} G {errs[1]:.2e} H {errs[2]:.2e} of the bound")
    assert errs[0] <= 1.0 and errs[1] <= 1.0 and errs[2] <= 1.0
    assert entry_err(eng.evaluate_c(x), cr, cm) <= 1.0
    assert entry_err(eng.evaluate_G_nonzeros(x, new_x=False), Gr, Gm) <= 1.0
    assert entry_err(eng.evaluate_H_nonzeros(x, SIGMA, lam), Hr, Hm) <= 1.0
    assert abs(eng.evaluate_J(x) - ora.J(x)) <= TOL * max(1.0, abs(ora.J(x)))
    assert vec_err(eng.evaluate_g(x), ora.grad_J(x)) <= 1.0
    for got, ref in ((eng.evaluate_G_structure(), ora.G_structure()), (eng.evaluate_H_structure(), ora.H_structure())):
        np.testing.assert_array_equal(got[0], ref[0])
        np.testing.assert_array_equal(got[1], ref[1])
    # the callbacks left the fused evaluation's bits as they were
    for got, ref in zip(eng.evaluate_all(x, SIGMA, lam), (edge.c, edge.G, edge.H)):
        assert np.array_equal(got, ref)


def _assert_bits(out, edge):
    plan = edge.plan
    oG, oH = plan.num_c, plan.num_c + plan.nnz_G
    assert np.array_equal(out[:oG], edge.c)
    assert np.array_equal(out[oG:oH], edge.G)
    assert np.array_equal(out[oH:oH + plan.nnz_H], edge.H)


def test_emulated_ranks_write_their_share_only_and_reassemble_bitwise(edge):
    """(b) Every rank's tiles run over its tile range into a NaN-filled buffer of its own.  Ownership: whatever lies
    outside the rank's own share -- the other ranks' shares and what the tail writes -- is still NaN, so a tile range
    that is off by one cannot hide behind the merge; an idle rank writes nothing at all (its call plans no launch: a
    launch of no workgroups would be refused by the runtime and raise here).  Merged by the plan's index and finished by
    the tail, the result is the unsharded evaluation bit for bit."""
    import torch
    eng, plan, world = edge.eng, edge.plan, edge.world
    dev = torch.device("cuda", 0)
    dx, dl = torch.from_numpy(edge.x).to(dev), torch.from_numpy(edge.lam).to(dev)
    oG, oH = plan.num_c, plan.num_c + plan.nnz_G
    s = torch.cuda.Stream(device=dev)
    merged = torch.full((plan.total,), float("nan"), dtype=torch.float64, device=dev)
    n_launches = eng.info["n_launches"]
    try:
        with torch.cuda.stream(s):
            for r in range(world):
                buf = torch.full((plan.total,), float("nan"), dtype=torch.float64, device=dev)
                for ip, ((k0, nred), off) in enumerate(zip(plan.tiles, plan.part_off)):
                    if nred:
                        eng.set_partials_buffer(ip, buf[off:off + (len(k0) - 1) * nred])
                    eng.set_tile_range(ip, *plan.tile_ranges[r][ip])
                eng.launch_bulk_only(dx, dl, buf[:oG], buf[oG:oH], buf[oH:oH + plan.nnz_H], s.cuda_stream)
                s.synchronize()
                assert eng.info["n_launches"] == n_launches
                got = buf.cpu().numpy()
                mine = np.zeros(plan.total, dtype=bool)
                mine[plan.index[r]] = True
                written = ~np.isnan(got)
                others = np.zeros(plan.total, dtype=bool)
                for q in range(world):
                    if q != r:
                        others[plan.index[q]] = True
                print(f"   {edge.case} rank {r}: ranges {plan.tile_ranges[r]}, share {plan.lengths[r]}, written {int(written.sum())}, "
                      f"in other ranks' shares {int((written & others).sum())}, outside every share {int((written & ~mine & ~others).sum())}")
                assert not (written & others).any(), f"rank {r} wrote into another rank's share at {np.nonzero(written & others)[0][:8]}"
                assert not (written & ~mine).any(), f"rank {r} wrote outside its share at {np.nonzero(written & ~mine)[0][:8]}"
                if plan.lengths[r] == 0:
                    assert not written.any()
                idx = torch.from_numpy(plan.index[r]).to(dev)
                merged[idx] = buf[idx]
                s.synchronize()
            for ip, ((k0, nred), off) in enumerate(zip(plan.tiles, plan.part_off)):
                if nred:
                    eng.set_partials_buffer(ip, merged[off:off + (len(k0) - 1) * nred])
                eng.set_tile_range(ip, 0, len(k0) - 1)
            eng.launch_tail_only(dx, SIGMA, dl, merged[:oG], merged[oG:oH], merged[oH:oH + plan.nnz_H], s.cuda_stream)
            s.synchronize()
        _assert_bits(merged.cpu().numpy(), edge)
    finally:
        torch.cuda.synchronize()
        for ip, (k0, _) in enumerate(plan.tiles):
            eng.set_partials_buffer(ip, 0)
            eng.set_tile_range(ip, 0, len(k0) - 1)
    # the handle is whole again
    for got, ref in zip(eng.evaluate_all(edge.x, SIGMA, edge.lam), (edge.c, edge.G, edge.H)):
        assert np.array_equal(got, ref)


def test_rank_local_handles_reassemble_bitwise(edge):
    """(c) Every rank evaluates its part of the mesh on a handle of its own (a phase in which it owns nothing is a
    one-section phase whose tile is computed and thrown away; an idle rank owns nothing anywhere), packs its segments, the
    root scatters them by the plan's index and runs the tail of the whole NLP: the unsharded bits."""
    import torch
    from pycollo_amd.sharding import LocalShard, global_tile_plan
    eng, plan, world = edge.eng, edge.plan, edge.world
    dev = torch.device("cuda", 0)
    dx, dl = torch.from_numpy(edge.x).to(dev), torch.from_numpy(edge.lam).to(dev)
    oG, oH = plan.num_c, plan.num_c + plan.nnz_G
    merged = torch.full((plan.total,), float("nan"), dtype=torch.float64, device=dev)
    s = torch.cuda.Stream(device=dev)
    tile_plan = global_tile_plan(eng.model, eng.meshes, device=0, mixed=eng.mixed, orders=eng.orders)
    for ip in range(len(eng.model.phases)):          # the plan-only handle cut what the device handle cut
        np.testing.assert_array_equal(tile_plan["tiles"][ip][0], eng.phase_tiles(ip)[0])
    try:
        with torch.cuda.stream(s):
            for r in range(world):
                ls = LocalShard(eng.model, r, world, device=0, meshes=eng.meshes, plan=tile_plan)
                try:
                    ls.set_scaling(eng.V_ocp, eng.r_ocp, edge.W, W_J)
                    assert ls.ranges == [tuple(t) for t in plan.tile_ranges[r]]
                    packed = ls.evaluate_packed(dx, dl, s.cuda_stream)
                    s.synchronize()
                    assert packed.numel() == plan.lengths[r]
                    merged[torch.from_numpy(plan.index[r]).to(dev)] = packed
                    s.synchronize()
                finally:
                    ls.close()
            for ip, ((k0, nred), off) in enumerate(zip(plan.tiles, plan.part_off)):
                if nred:
                    eng.set_partials_buffer(ip, merged[off:off + (len(k0) - 1) * nred])
            eng.launch_tail_only(dx, SIGMA, dl, merged[:oG], merged[oG:oH], merged[oH:oH + plan.nnz_H], s.cuda_stream)
            s.synchronize()
        _assert_bits(merged.cpu().numpy(), edge)
    finally:
        torch.cuda.synchronize()
        for ip in range(len(plan.tiles)):
            eng.set_partials_buffer(ip, 0)


def test_copy_runs_moves_exactly_the_runs_bit_for_bit(built):
    """``pc_copy_runs`` (the pack and unpack of every exchange) against dst[d0:d0+n] = src[s0:s0+n] in NumPy, compared as
    bit patterns: run lengths on both sides of the chunk a workgroup copies, payloads with NaNs (two payloads), -0.0 and
    denormals, odd offsets; whatever lies between the runs keeps its NaN fill.  A table of no runs is a call that
    succeeds and writes nothing."""
    import torch
    from pycollo_amd.engine import load_library
    from pycollo_amd.sharding import _chunk_table
    lib = load_library()
    chunk = int(lib.pc_run_chunk())
    lengths = [1, chunk - 1, chunk, chunk + 1, 2 * chunk + 1]
    rng = np.random.default_rng(21)
    n_src = sum(lengths) + 3 * len(lengths) + 5
    src = rng.normal(size=n_src)
    special = np.array([np.nan, -0.0, 5e-324, -2.5e-310, 0.0, np.inf, -np.inf])
    src[rng.choice(n_src, size=n_src // 3, replace=False)] = rng.choice(special, size=n_src // 3)
    src_bits = src.view(np.uint64)
    src_bits[7] = 0xFFF8000000000123          # a NaN with a sign and a payload: copied, not recomputed
    runs, so, do = [], 1, 3                   # (src offset, dst offset, length): out of order in dst, gaps on both sides
    for n in lengths:
        if n >= 3:                            # every longer run starts with a NaN, -0.0 and the smallest denormal
            src[so:so + 3] = [np.nan, -0.0, 5e-324]
            src[so + n - 1] = -5e-324         # and its last element (the chunk's tail) is a denormal too
        runs.append((so, do, n))
        so += n + 2
        do += n + 5
    src[runs[0][0]] = -0.0                    # the run of one element carries the sign of zero
    n_dst = do + 4
    runs = [runs[i] for i in (3, 0, 4, 2, 1)]
    tab = _chunk_table(runs, chunk)
    assert tab[:, 2].max() == chunk and tab[:, 2].min() == 1 and tab.shape[0] == 1 + 1 + 1 + 2 + 3
    fill = np.full(n_dst, np.nan)
    want = fill.copy()
    for s0, d0, n in runs:
        want[d0:d0 + n] = src[s0:s0 + n]
    for needle in (np.float64(-0.0).view(np.uint64), np.float64(5e-324).view(np.uint64), np.uint64(0xFFF8000000000123)):
        assert (want.view(np.uint64) == needle).any()
    dev = torch.device("cuda", 0)
    d_src, d_dst, d_tab = torch.from_numpy(src).to(dev), torch.from_numpy(fill).to(dev), torch.from_numpy(tab).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.pc_copy_runs(d_src.data_ptr(), d_dst.data_ptr(), d_tab.data_ptr(), tab.shape[0], st), lib.pc_last_error().decode()
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    covered = np.zeros(n_dst, dtype=bool)
    for _, d0, n in runs:
        covered[d0:d0 + n] = True
    assert np.array_equal(got.view(np.uint64)[~covered], fill.view(np.uint64)[~covered]) and (~covered).sum() >= 5 * len(runs)
    assert np.array_equal(d_src.cpu().numpy().view(np.uint64), src.view(np.uint64))     # the source is read only
    # no runs: the call succeeds (an idle rank's pack, a single rank's unpack) and writes nothing
    empty = torch.from_numpy(_chunk_table([], chunk)).to(dev)
    assert empty.shape == (0, 3)
    assert lib.pc_copy_runs(d_src.data_ptr(), d_dst.data_ptr(), empty.data_ptr(), 0, st), lib.pc_last_error().decode()
    torch.cuda.synchronize()
    assert np.array_equal(d_dst.cpu().numpy().view(np.uint64), want.view(np.uint64))
