"""The builds of the evaluation that a tile count, a block size or an environment knob selects, at the smallest meshes
that select them (run with -m gpu on an MI355X).

Uniform meshes of order 3 with PYCOLLO_AMD_TILE_NODES=3 put one section into every tile, so a phase of K sections has
exactly K tiles.  The tile counts sit on both sides of every boundary at which one of the tail's summation loops
takes another pass: SL * {64, 128, 256} tiles per pass of the resident walk (pc_kernels.hpp, tail_phase_issue<RES>;
SL = 4 / 2 / 1 by the number of partial sums per tile, NRED), 256 tiles per stride of the plain separate tail, 2048 / 1024
per iteration of pc_tail_big (picked above 1024 tiles), with nt % 8 in {0, 1, 5, 7} for the XCD-major tile order.  Every
build must return the same bits and one of them is held to the oracle as in test_gpu_parity.py;
``NlpEngine.info`` says which build an evaluation launched.
"""
import numpy as np
import pytest

from conftest import entry_err, golden_tables, vec_err
from oracle.ref_numpy import OracleNlp
from pycollo_amd import problems

pytestmark = pytest.mark.gpu
TOL = 1e-10

NT = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 2055, 4101]
# hypersensitive: one sum per tile (SL = 4, U = 8); time_coupled_transfer: two phases, q / t / parameter sums, 13 and 18
# sums per tile (SL = 1, U = 4), the merged launch; two_phase_transfer: 3 and 4 sums per tile (SL = 2)
MODELS = ["hypersensitive", "time_coupled_transfer"]
# (label, environment, threads_per_block, threads of the workgroup that runs the tail)
BUILDS = [("wpt1", {"PYCOLLO_AMD_WPT": "1"}, 64, 64), ("wpt2", {"PYCOLLO_AMD_WPT": "2"}, 64, 128),
          ("wpt4", {"PYCOLLO_AMD_WPT": "4"}, 64, 256), ("tb128", {}, 128, 128), ("tb256", {}, 256, 256),
          ("two_launch", {"PYCOLLO_AMD_RESIDENT": "0"}, 64, 256)]
KNOBS = ("PYCOLLO_AMD_WPT", "PYCOLLO_AMD_RESIDENT", "PYCOLLO_AMD_TAIL_BLOCKS", "PYCOLLO_AMD_MERGE", "PYCOLLO_AMD_TILE_NODES")


@pytest.fixture(scope="module")
def tab():
    return golden_tables("lobatto")


def _uniform(name, K, order=3):
    prob = problems.REGISTRY[name](K=K, order=order)
    for ph in prob.phases:
        ph.mesh.number_mesh_sections = K
        ph.mesh.number_mesh_section_nodes = order
    return prob


def _ragged(name, K, seed):
    """Orders 2..4 at random, section by section: the any-order kernel, tiles of one to three sections."""
    prob = problems.REGISTRY[name](K=K, order=3)
    rng = np.random.default_rng(seed)
    for ph in prob.phases:
        ph.mesh.number_mesh_sections = K
        ph.mesh.mesh_section_sizes = rng.uniform(0.5, 1.5, K)
        ph.mesh.number_mesh_section_nodes = rng.integers(2, 5, K)
    return prob


def _engine(monkeypatch, prob, env, tpb, tile_nodes=3):
    from pycollo_amd.engine import NlpEngine
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if tile_nodes:
        monkeypatch.setenv("PYCOLLO_AMD_TILE_NODES", str(tile_nodes))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return NlpEngine(prob, device=0, threads_per_block=tpb)


def _outputs(eng, x, lam, sigma):
    """c~, G~, H~, J, grad J at one point, and the builds the fused evaluation launched."""
    c, G, H = (a.copy() for a in eng.evaluate_all(x, sigma, lam))
    info = eng.info
    J = np.array([eng.evaluate_J(x)])
    g = eng.evaluate_g(x, new_x=False)
    return (c, G, H, J, g), info


def _phase_tiles(eng):
    return [len(eng.phase_tiles(ip)[0]) - 1 for ip in range(len(eng.model.phases))]


def _points(eng, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.45, 0.45, eng.num_x), rng.normal(size=eng.num_c), rng.uniform(-0.45, 0.45, eng.num_x)


def _check_oracle(prob, tab, eng, x, lam, sigma, out):
    ora = OracleNlp(prob, tab, V_ocp=eng.V_ocp, r_ocp=eng.r_ocp, W_ocp=eng.W_ocp, w_J=1.0)
    c, G, H, J, g = out
    errs = (entry_err(c, ora.c(x), ora.c_mag(x)), entry_err(G, ora.G(x), ora.G_mag(x)),
            entry_err(H, ora.H(x, sigma, lam), ora.H_mag(x, sigma, lam)))
    Jr = ora.J(x)
    print(f"   oracle: c {errs[0]:.3f} G {errs[1]:.3f} H {errs[2]:.3f} of the bound; |J - Jref| {abs(J[0] - Jr):.3e}; "
          f"grad J {vec_err(g, ora.grad_J(x)):.3f}")
    assert errs[0] <= 1.0 and errs[1] <= 1.0 and errs[2] <= 1.0
    assert abs(J[0] - Jr) <= TOL * max(1.0, abs(Jr))
    assert vec_err(g, ora.grad_J(x)) <= 1.0


def _all_builds_agree(monkeypatch, tab, prob, tile_nodes, min_tiles=None, exact_tiles=None):
    """The six builds at one (x, lambda, sigma): equal bits, the launched build as ``info`` reports it, one of them held
    to the oracle, and a second point on the resident and the two-launch build (the granule tag advances)."""
    sigma = 0.6
    res, second = {}, {}
    for label, env, tpb, tail_threads in BUILDS:
        eng = _engine(monkeypatch, prob, env, tpb, tile_nodes)
        tiles = _phase_tiles(eng)
        if label == "wpt1":
            x, lam, x2 = _points(eng, 23)
            print(f"\n   tiles per phase {tiles}, partial sums per tile {[eng.phase_tiles(ip)[1] for ip in range(len(tiles))]}")
        assert eng.info["n_tiles_total"] == sum(tiles)
        if exact_tiles is not None:
            assert tiles == [exact_tiles] * len(tiles)
        if min_tiles is not None:
            assert min(tiles) > min_tiles
        res[label], info = _outputs(eng, x, lam, sigma)
        if label == "two_launch":
            assert not info["resident"] and info["n_launches"] == 2
            assert info["tail_big"] == (max(tiles) > 1024)
            assert info["merged"] == (len(tiles) > 1)
            assert info["tail_blocks"] == 0
        else:
            assert info["resident"] and info["n_launches"] == 1 and not info["tail_big"]
            assert info["merged"] == (len(tiles) > 1)
            assert info["tail_blocks"] >= 1
        assert info["tail_block_threads"] == tail_threads
        if label in ("wpt1", "two_launch"):
            second[label], _ = _outputs(eng, x2, lam, 0.3)
            if label == "two_launch":
                _check_oracle(prob, tab, eng, x, lam, sigma, res[label])
        eng.close()
    for label in res:
        for a, b in zip(res[label], res["two_launch"]):
            np.testing.assert_array_equal(a, b, err_msg=label)
    for a, b in zip(second["wpt1"], second["two_launch"]):
        np.testing.assert_array_equal(a, b)
    assert not np.array_equal(second["wpt1"][0], res["wpt1"][0])


@pytest.mark.parametrize("nt", NT)
@pytest.mark.parametrize("name", MODELS)
def test_builds_write_the_same_bits_at_every_pass_boundary(built, tab, monkeypatch, name, nt):
    _all_builds_agree(monkeypatch, tab, _uniform(name, nt), 3, exact_tiles=nt)


@pytest.mark.parametrize("nt", [127, 129, 257, 511, 513, 1025, 2055])
def test_builds_agree_with_two_tiles_per_lane_and_pass(built, tab, monkeypatch, nt):
    """3 and 4 sums per tile: the resident walk takes two tiles per lane and pass (boundaries at 128, 256, 512)."""
    prob = _uniform("two_phase_transfer", nt)
    _all_builds_agree(monkeypatch, tab, prob, 3, exact_tiles=nt)


# sections per phase that give a little more than 256 / 2048 tiles of at most four nodes
@pytest.mark.parametrize("name,K,min_tiles", [("hypersensitive", 335, 256), ("time_coupled_transfer", 335, 256),
                                               ("hypersensitive", 2660, 1024), ("time_coupled_transfer", 2660, 1024)])
def test_builds_agree_on_a_ragged_mesh(built, tab, monkeypatch, name, K, min_tiles):
    """Orders 2..4 at random (the any-order kernel, tiles that differ in size): more than one pass of every walk, and
    pc_tail_big, on tile tables that are read rather than computed."""
    _all_builds_agree(monkeypatch, tab, _ragged(name, K, seed=K), 4, min_tiles=min_tiles)


@pytest.mark.parametrize("nt", [2055, 4101])
@pytest.mark.parametrize("name", MODELS)
def test_sharded_ranks_reassemble_bitwise_with_the_big_tail(built, monkeypatch, name, nt):
    """Three emulated ranks (bulk kernels over a tile range each, segments merged, tail on the merged buffer: as
    test_gpu_parity.test_sharded_ranks_reassemble_bitwise) at tile counts that pick pc_tail_big."""
    import torch
    from pycollo_amd.sharding import ShardPlan
    world = 3
    eng = _engine(monkeypatch, _uniform(name, nt), {}, 0)
    assert _phase_tiles(eng) == [nt] * len(eng.model.phases)
    x, lam, _ = _points(eng, 4)
    c, G, H = (a.copy() for a in eng.evaluate_all(x, 0.9, lam))
    assert eng.info["resident"]
    plan = ShardPlan(eng, world)
    dev = torch.device("cuda", 0)
    dx, dl = torch.from_numpy(x).to(dev), torch.from_numpy(lam).to(dev)
    oG, oH = plan.num_c, plan.num_c + plan.nnz_G
    s = torch.cuda.Stream(device=dev)
    merged = torch.full((plan.total,), float("nan"), dtype=torch.float64, device=dev)
    with torch.cuda.stream(s):
        for r in range(world):
            buf = torch.full((plan.total,), float("nan"), dtype=torch.float64, device=dev)
            for ip, ((k0, nred), off) in enumerate(zip(plan.tiles, plan.part_off)):
                if nred:
                    eng.set_partials_buffer(ip, buf[off:off + (len(k0) - 1) * nred])
                eng.set_tile_range(ip, *plan.tile_ranges[r][ip])
            eng.launch_bulk_only(dx, dl, buf[:oG], buf[oG:oH], buf[oH:oH + plan.nnz_H], s.cuda_stream)
            assert not eng.info["resident"] and not eng.info["tail_big"]
            idx = torch.from_numpy(plan.index[r]).to(dev)
            merged[idx] = buf[idx]
            s.synchronize()
        for ip, ((k0, nred), off) in enumerate(zip(plan.tiles, plan.part_off)):
            if nred:
                eng.set_partials_buffer(ip, merged[off:off + (len(k0) - 1) * nred])
            eng.set_tile_range(ip, 0, len(k0) - 1)
        eng.launch_tail_only(dx, 0.9, dl, merged[:oG], merged[oG:oH], merged[oH:oH + plan.nnz_H], s.cuda_stream)
        s.synchronize()
    assert eng.info["tail_big"] and eng.info["tail_block_threads"] == 256
    out = merged.cpu().numpy()
    assert np.array_equal(out[:oG], c)
    assert np.array_equal(out[oG:oH], G)
    assert np.array_equal(out[oH:oH + plan.nnz_H], H)
    for ip in range(len(plan.tiles)):
        eng.set_partials_buffer(ip, 0)
    eng.close()


# the models whose endpoint block is worth a tail workgroup per part (pc_engine.hip, heavy_point)
HEAVY_POINT = [("two_phase_transfer", {}), ("time_coupled_transfer", {}), ("space_station", dict(K=12, order=4)),
               ("delta_iii", dict(K=9, order=4))]


@pytest.mark.parametrize("name,kw", HEAVY_POINT)
def test_tail_blocks_hand_over_the_same_bits(built, monkeypatch, name, kw):
    """One to four workgroups share the resident tail (the helpers hand their endpoint Hessian terms over as granules,
    hb_gran): every split, at every block size, writes the bits of the two-launch build."""
    prob = problems.REGISTRY[name](**kw)
    lo, hi = (0.05, 0.3) if name == "delta_iii" else (-0.45, 0.45)
    sigma = 0.6
    x = lam = None
    # (environment, tail workgroups expected -- 0: the separate tail --, threads of the workgroup that runs the tail)
    for tpb, counts in ((64, (1, 2, 3, 4)), (128, (1, 2, 3, 4)), (256, (1,))):
        wpt = {"PYCOLLO_AMD_WPT": "1"} if tpb == 64 else {}      # (64-node tiles would otherwise be shared by 2 or 4 waves)
        sweep = [({"PYCOLLO_AMD_RESIDENT": "0", **wpt}, 0, 256)]
        sweep += [({"PYCOLLO_AMD_TAIL_BLOCKS": str(n), **wpt}, n, tpb) for n in counts]
        ref = None
        for env, ntb, threads in sweep:
            eng = _engine(monkeypatch, prob, env, tpb, tile_nodes=0)
            if x is None:
                rng = np.random.default_rng(29)
                x, lam = rng.uniform(lo, hi, eng.num_x), rng.normal(size=eng.num_c)
            got = []
            for rep in range(2):   # twice: the hand-over granules carry the launch's tag
                out, info = _outputs(eng, x if rep == 0 else 0.9 * x, lam, sigma)
                assert info["tail_blocks"] == ntb and info["tail_block_threads"] == threads
                assert info["resident"] == (ntb > 0)
                got += list(out)
            eng.close()
            if ref is None:
                ref = got        # the two-launch build with the same tiles
            for a, b in zip(got, ref):
                np.testing.assert_array_equal(a, b, err_msg=f"{env} threads_per_block {tpb}")


@pytest.mark.parametrize("name,kw", [("two_phase_transfer", {}), ("time_coupled_transfer", {}), ("delta_iii", dict(K=9, order=4)),
                                     ("sliding_mass", dict(num_phases=3, K=7, order=4))])
def test_per_phase_launches_match_the_merged_launch(built, tab, monkeypatch, name, kw):
    """PYCOLLO_AMD_MERGE=0 (what a code object without pc_bulk_all gets): a launch per phase and the tail, against the
    merged two-launch build, and held to the oracle."""
    prob = problems.REGISTRY[name](**kw)
    lo, hi = (0.05, 0.3) if name == "delta_iii" else (-0.45, 0.45)
    outs = {}
    for merge in ("1", "0"):
        eng = _engine(monkeypatch, prob, {"PYCOLLO_AMD_RESIDENT": "0", "PYCOLLO_AMD_MERGE": merge}, 64, tile_nodes=0)
        if merge == "1":
            rng = np.random.default_rng(31)
            x, lam = rng.uniform(lo, hi, eng.num_x), rng.normal(size=eng.num_c)
        outs[merge], info = _outputs(eng, x, lam, 0.6)
        assert not info["resident"] and info["tail_block_threads"] == 256
        if merge == "1":
            assert info["merged"] and info["n_launches"] == 2
        else:
            assert not info["merged"] and info["n_launches"] == len(prob.phases) + 1
            if name != "delta_iii":   # (its oracle takes a quarter of a minute to build; test_gpu_parity.py holds the merged build to it)
                _check_oracle(prob, tab, eng, x, lam, 0.6, outs[merge])
        eng.close()
    for a, b in zip(outs["0"], outs["1"]):
        np.testing.assert_array_equal(a, b)
