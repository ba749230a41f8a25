"""Host side of tests/test_gpu_tail_variants.py, without a GPU: the meshes that test relies on give exactly one tile
per section, and pc_info kept its layout when its last field became ``last_launch``."""
import ctypes as C

import pytest

from pycollo_amd import problems

NT = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 2055, 4101]


def _uniform(name, K, order=3):
    prob = problems.REGISTRY[name](K=K, order=order)
    for ph in prob.phases:
        ph.mesh.number_mesh_sections = K
        ph.mesh.number_mesh_section_nodes = order
    return prob


@pytest.mark.parametrize("name", ["hypersensitive", "time_coupled_transfer"])
def test_one_tile_per_section_with_three_node_tiles(built, monkeypatch, name):
    from pycollo_amd.engine import NlpEngine
    monkeypatch.setenv("PYCOLLO_AMD_TILE_NODES", "3")
    for nt in NT:
        prob = _uniform(name, nt)
        eng = NlpEngine(prob, device=None)
        assert eng.info["n_tiles_total"] == nt * len(prob.phases)
        for ip in range(len(prob.phases)):
            k0, _ = eng.phase_tiles(ip)
            assert list(k0) == list(range(nt + 1))
        # nothing was launched: every field of last_launch reads zero
        info = eng.info
        assert info["last_launch"] == 0 and not info["resident"] and not info["tail_big"] and not info["merged"]
        assert info["tail_blocks"] == 0 and info["tail_block_threads"] == 0
        eng.close()
        assert eng.info["n_tiles_total"] == nt * len(prob.phases)   # (a closed engine reports what its handle said last)


def test_info_struct_layout_is_unchanged():
    """include/pycollo_amd.h, pc_info: two int32, three int64, six int32 -- 56 bytes, ``last_launch`` where
    ``reserved`` was."""
    from pycollo_amd.engine import _Info
    assert C.sizeof(_Info) == 56
    assert _Info.last_launch.offset == 52 and _Info.last_launch.size == 4
    assert _Info.waves_per_tile.offset == 48
    assert [k for k, _ in _Info._fields_][-1] == "last_launch"


def test_kkt_info_struct_layout():
    """include/pycollo_amd.h, pc_kkt_info: four int64, eight int32."""
    from pycollo_amd.kkt import _KktInfo
    assert C.sizeof(_KktInfo) == 64
    assert _KktInfo.chain_cr.offset == 32 and _KktInfo.leaf_waves.offset == 56
