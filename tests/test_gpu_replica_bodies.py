"""The per-replica tile bodies (pc::bulk with the waves-per-tile count and the wave index compiled in: pc_bulk_p0_r_w<W>)
at the smallest meshes where they can go wrong.  In those bodies the block's thread count, the lane's thread index and
the tile width are constants and the staging guards a replica can never satisfy are gone (pc_kernels.hpp) -- all of
which depends on which lanes of which wave see which table entry, i.e. on the tile's geometry:

* K = 1: one tile that is both the first and the last, holding one section (no previous section, tables shorter than
  any guard);
* K = spt: exactly one full tile;
* K = spt + 1: two edge tiles, the last with a single section (and a previous section to stage);
* K = 3 spt - 1: an interior tile and a short last tile;
* cart-pole (four states: the rows of the second and later multipliers, staging per state), K = 2 spt + 1.

spt = sections per 64-node tile = 63 // (order - 1), checked against the tile cuts the engine reports.  c~, G~ and H~ are
compared with the oracle entry by entry as tests/test_gpu_parity.py does (conftest.entry_err, no entry skipped) for 1, 2
and 4 waves per tile (PYCOLLO_AMD_WPT), and the three launches must agree bit for bit: one wave per tile runs the body
with the run-time block shape, two and four the per-replica bodies.  Only (model, order) pairs the entry script
prebuilds, so nothing is compiled here."""
import numpy as np
import pytest

from conftest import entry_err, golden_tables
from oracle.ref_numpy import OracleNlp
from pycollo_amd import codegen, problems

pytestmark = pytest.mark.gpu

HYPER_ORDER, CART_ORDER = 6, 4


def spt_of(order):
    return 63 // (order - 1)


CASES = [("hypersensitive", HYPER_ORDER, 1), ("hypersensitive", HYPER_ORDER, spt_of(HYPER_ORDER)),
         ("hypersensitive", HYPER_ORDER, spt_of(HYPER_ORDER) + 1), ("hypersensitive", HYPER_ORDER, 3 * spt_of(HYPER_ORDER) - 1),
         ("cart_pole", CART_ORDER, 2 * spt_of(CART_ORDER) + 1)]


@pytest.fixture(scope="module")
def tab():
    return golden_tables("lobatto")


@pytest.mark.parametrize("name,order,K", CASES)
def test_replica_bodies_match_oracle_and_each_other(built, tab, monkeypatch, name, order, K):
    from pycollo_amd.engine import NlpEngine
    prob = problems.REGISTRY[name](K=K, order=order)
    spt = spt_of(order)
    outs, ref = {}, None
    for wpt in (1, 2, 4):
        monkeypatch.setenv("PYCOLLO_AMD_WPT", str(wpt))
        eng = NlpEngine(prob, device=0, threads_per_block=64)
        try:
            assert eng.info["waves_per_tile"] == wpt
            if wpt > 1:   # the handle falls back to the run-time body without a word when the object lacks the kernel
                assert f"pc_bulk_p0_r_w{wpt}" in codegen.code_object_resources(eng.code_object), "no per-replica kernel in the code object"
            k0, _ = eng.phase_tiles(0)
            np.testing.assert_array_equal(k0, np.minimum(np.arange(-(-K // spt) + 1) * spt, K))   # the tiles the case is about
            if ref is None:
                ora = OracleNlp(prob, tab, V_ocp=eng.V_ocp, r_ocp=eng.r_ocp, W_ocp=eng.W_ocp, w_J=1.0)
                rng = np.random.default_rng(1000 * order + K)
                x, lam, sigma = rng.uniform(-0.45, 0.45, eng.num_x), rng.normal(size=eng.num_c), 0.6
                ref = ((ora.c(x), ora.c_mag(x)), (ora.G(x), ora.G_mag(x)), (ora.H(x, sigma, lam), ora.H_mag(x, sigma, lam)))
                for r, m in ref:
                    assert np.all(np.isfinite(r)) and np.all(np.isfinite(m))
            outs[wpt] = [np.ascontiguousarray(a, dtype=np.float64) for a in eng.evaluate_all(x, sigma, lam)]
        finally:
            eng.close()
        for what, got, (r, m) in zip("cGH", outs[wpt], ref):
            err = entry_err(got, r, m)
            print(f"{name} n={order} K={K} W={wpt} {what}: {err:.3e} of the bound")
            assert err <= 1.0, f"{what}~ differs from the oracle with {wpt} waves per tile"
    for wpt in (2, 4):
        for what, a, b in zip("cGH", outs[1], outs[wpt]):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), f"{what}~: {wpt} waves per tile differ from one in some bit"
