"""The launch shape of the KKT solver (csrc/pc_kkt_shape.hpp; host integer work, no GPU).

1. tests/c/kkt_shape_sanitize.cpp builds the shape of synthetic descriptors under AddressSanitizer + UBSan, walks every offset
   table against the buffer it indexes and prints the shape; ``rules`` below restates the rules in NumPy -- from their
   description (the comments of the kernels), not from the C++ -- and must print the same.  The cases
   are the smallest descriptors on either side of every rule.
2. ``kkt.shape_info`` (``pc_kkt_shape_info``) on the real tables of the meshes tests/test_gpu_kkt_variants.py builds on a
   device: the same ``info`` facts, without one.

Two cases the rules allow cannot be built: cyclic reduction switched off by a pull list of more than 64 entries (a node is
named by at most two eliminated nodes per level: 33 levels, a segment of 2^32 nodes) and the 17-level cap of kkt_cr_top (the
trailing levels of at most 16 nodes are at most seven: 1, 1, 1, 2, 4, 8, 16).  Both stay in ``rules``."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

MV_LONG, MV_CHUNK, CR_MAX_PULL = 256, 1024, 64
LDS_BLOCK_MAX, LDS_VECTORS_MAX, LDS_WORKGROUP = 64000, 60000, 65536


def case(name, segs=(), nz=2, m=3, nb=2, chain=None, leaf=None, left=None, rows=(7, 14, 9), entries=(), export=None,
         leaf_fwd=-1, leaf_waves=4, cr=1, cr_top_cap=-1):
    """A synthetic descriptor: chain segments of ``segs`` nodes with ``nz`` unknowns each (or ``chain`` sizes), one leaf of
    ``m`` unknowns (or ``leaf`` sizes) right of every chain node that is not the last of its segment."""
    seg = np.concatenate([[0], np.cumsum(segs)]).astype(int)
    chain = np.full(seg[-1], nz) if chain is None else np.asarray(chain)
    last = np.zeros(len(chain), bool)
    last[seg[1:][np.diff(seg) > 0] - 1] = True
    if left is None:
        left = np.nonzero(~last)[0]
    leaf = np.full(len(left), m) if leaf is None else np.asarray(leaf)
    return dict(name=name, nb=nb, chain=chain, seg=seg, leaf=leaf, left=np.asarray(left), rows=np.asarray(rows), entries=list(entries),
                export=None if export is None else np.asarray(export), knobs=(leaf_fwd, leaf_waves, cr, cr_top_cap))


def text(c):
    def runs(v):     # "3x5" for 3 3 3 3 3
        out, v = [], [int(x) for x in v]
        i = 0
        while i < len(v):
            j = i
            while j < len(v) and v[j] == v[i]:
                j += 1
            out.append(f"{v[i]}x{j - i}" if j - i > 1 else str(v[i]))
            i = j
        return " ".join(out)
    lines = [f"case {c['name']}", f"nb {c['nb']}", "chain " + runs(c["chain"]), "seg " + " ".join(str(int(x)) for x in c["seg"]),
             "leaf " + runs(c["leaf"]), "left " + " ".join(str(int(x)) for x in c["left"]), "rows " + runs(c["rows"])]
    lines += [f"entry {e} {i} {k}" for e, i, k in c["entries"]]
    if c["export"] is not None:
        lines.append("export " + runs(c["export"]))
    lines += ["knobs " + " ".join(str(x) for x in c["knobs"]), "end"]
    return "\n".join(lines) + "\n"


def cr_rules(chain, seg, nb, export):
    """Odd-even elimination of every segment: level, separators, LDS bytes of the largest node, longest pull list, buffer."""
    nc = len(chain)
    lvl, ca, cb = np.ones(nc, int), -np.ones(nc, int), -np.ones(nc, int)
    lmax = 1
    for s0, s1 in zip(seg[:-1], seg[1:]):
        n = s1 - s0
        if n <= 0:
            continue
        assert not export[s0 + 1:s1 - 1].any()
        exp_last = n >= 2 and export[s1 - 1]                 # stays: the right separator of whoever would look beyond it
        anchor, n1 = (s1 - 1, n - 1) if exp_last else (-1, n)
        levels = int(n1 - 1).bit_length()
        lvl[s0], cb[s0] = levels + 1, anchor                   # position 0 goes last
        for p in range(1, n1):
            h = p & -p                                         # eliminated at level log2(h) + 1 against p - h and p + h
            lvl[s0 + p], ca[s0 + p] = h.bit_length(), s0 + p - h
            cb[s0 + p] = s0 + p + h if p + h <= n1 - 1 else anchor
        if exp_last:
            lvl[anchor] = levels + 2
        lmax = max(lmax, levels + (2 if exp_last else 1))
    pulls = np.zeros(nc, int)
    for c in range(nc):
        if not export[c]:
            for sep in (ca[c], cb[c]):
                if sep >= 0:
                    pulls[sep] += 1
    w = np.where(ca >= 0, chain[ca], 0) + np.where(cb >= 0, chain[cb], 0) + nb if nc else np.zeros(0, int)
    lds = 8 * (2 * chain + w + chain * (chain + w) + w * w + 2)
    ldsmax = 0 if nc == 0 else (1 << 30 if (chain > 64).any() or (w > 64).any() else int(lds.max()))
    return lvl, lmax, ldsmax, int(pulls.max()) if nc else 0, int((chain * (chain + w) + w * w + w).sum())


def rules(c):
    nb, chain, seg, leaf, left, rows = c["nb"], c["chain"], c["seg"], c["leaf"], c["left"], c["rows"]
    leaf_fwd, leaf_waves, cr_knob, cr_top_cap = c["knobs"]
    nc, nl, nu = len(chain), len(leaf), len(rows)
    out = {}
    # the product
    n_mv = int(rows.sum())
    idx, kind = np.arange(n_mv) % 1000, np.arange(n_mv) % 3
    for e, i, k in c["entries"]:
        idx[e], kind[e] = i, k
    if ((idx < 0) | (idx >= 2 ** 30) | (kind < 0) | (kind > 2)).any():
        return "matvec table entry out of range"
    h = 1469598103934665603
    for wd in (kind.astype(object) << 30) | idx.astype(object):
        h = ((h ^ int(wd)) * 1099511628211) % 2 ** 64
    out["mv_src_hash"] = [h]
    ptr = np.concatenate([[0], np.cumsum(rows)])
    longs = [r for r in range(nu) if rows[r] > MV_LONG]
    e0 = [e for r in longs for e in range(ptr[r], ptr[r + 1], MV_CHUNK)]
    e1 = [min(e + MV_CHUNK, ptr[r + 1]) for r in longs for e in range(ptr[r], ptr[r + 1], MV_CHUNK)]
    out.update(mv_long=longs, mv_long_c0=np.concatenate([[0], np.cumsum([-(-rows[r] // MV_CHUNK) for r in longs])]),
               mv_chunk_e0=e0, mv_chunk_e1=e1, n_mv_long=[len(longs)], n_mv_chunks=[len(e0)], n_mv_long_part=[max(1, len(e0))])
    # leaves and chain nodes: widths of their coupling, offsets of their gathered vectors
    last = np.zeros(nc, bool)
    last[seg[1:][np.diff(seg) > 0] - 1] = True
    w_leaf = chain[left] + chain[left + 1] + nb if nl else np.zeros(0, int)
    leaf_of_left = -np.ones(nc, int)
    leaf_of_left[left] = np.arange(nl)
    if (~last & (leaf_of_left < 0)).any():
        return "chain node without a leaf on its right"
    nx = np.where(last, 0, np.append(chain[1:], 0)) if nc else np.zeros(0, int)
    out.update(chain_last=last.astype(int), leaf_of_left=leaf_of_left, leafG_off=np.cumsum(w_leaf) - w_leaf,
               chainG_off=np.cumsum(nx + nb) - (nx + nb), n_leafG=[max(1, int(w_leaf.sum()))], n_chainG=[max(1, int((nx + nb).sum()))])
    mmax, wmax = max([1] + list(leaf)), max([1] + list(w_leaf))
    nzmax, wcmax = max([1] + list(chain)), max([1] + list(nx + nb))
    lds_leaf = 8 * (2 * mmax + wmax + 2)
    staged = [b for b in 8 * (leaf * (leaf + w_leaf) + 2 * leaf + w_leaf + 2) if b <= LDS_BLOCK_MAX]
    lds_chain = 8 * (2 * nzmax + wcmax + 2)
    full = 8 * (2 * nzmax + wcmax + 2 * wcmax * wcmax + nzmax * (nzmax + wcmax) + 2)
    out.update(lds_leaf=[lds_leaf], lds_leaf_full=[max(staged + [lds_leaf])], lds_chain=[lds_chain], chain_lds=[int(full <= LDS_BLOCK_MAX)],
               lds_chain_factor=[full if full <= LDS_BLOCK_MAX else lds_chain], nzmax=[nzmax], wcmax=[wcmax])
    # the chain by cyclic reduction
    export = np.zeros(nc, bool) if c["export"] is None else c["export"].astype(bool)
    lvl, lmax, ldsmax, max_pull, buf_len = cr_rules(chain, seg, nb, export)
    chain_cr = ldsmax <= LDS_BLOCK_MAX and max_pull <= CR_MAX_PULL and bool(cr_knob)
    if export.any() and not chain_cr:
        return "exported chain nodes need the cyclic-reduction kernels (blocks too large for their LDS)"
    out.update(chain_cr=[int(chain_cr)], any_export=[int(export.any())])
    levels_reported = top_n = top_waves = 0
    if chain_cr:
        nodes = [x for l in range(1, lmax + 1) for x in np.nonzero(lvl == l)[0]]
        lvl_ptr = np.concatenate([[0], np.cumsum([(lvl == l).sum() for l in range(1, lmax + 1)])])
        L = len(lvl_ptr)
        wave_bytes = (ldsmax + 24 * CR_MAX_PULL + 15) // 16 * 16
        nw = min(16, LDS_WORKGROUP // wave_bytes)
        if cr_top_cap >= 0:
            nw = min(nw, cr_top_cap)
        first = L                                              # trailing levels of at most nw nodes, 17 at the most; not one alone
        if nw >= 2:
            while first > 1 and lvl_ptr[first - 1] - lvl_ptr[first - 2] <= nw and L - (first - 1) <= 17:
                first -= 1
            if L - first < 2:
                first = L
        out.update(cr_lvl_ptr=lvl_ptr, cr_nodes=nodes, export_nodes=np.nonzero(export)[0], cr_top_from=[first], cr_top_waves=[nw],
                   cr_top_lds=[nw * wave_bytes], cr_top_n=[L - first], cr_top_wave_bytes=[wave_bytes],
                   cr_top_ptr=lvl_ptr[first - 1:] if L - first else [], lds_cr=[ldsmax], n_crbuf=[max(1, buf_len)])
        levels_reported, top_n, top_waves = L - 1, L - first, nw
    # the border
    terms = nl + nc
    grid = nb > 0 and (nb * nb * terms > 2 ** 18 or terms >= 2048)
    blocks = min(256, terms) if grid else 0
    lds_border = 8 * (2 * nb + 2 + 256)
    out.update(lds_border=[lds_border], border_blocks=[blocks], n_border_part=[blocks * nb * nb])
    if max(lds_leaf, lds_chain, lds_border) > LDS_VECTORS_MAX:
        return "KKT block too large for the solver's LDS staging"
    out.update(n_vals=[int(leaf.sum()) * 3 + 7], n_vec=[nu], n_counts=[2 * (terms + 1)],
               leaf_forward_stage=[leaf_fwd if leaf_fwd >= 0 else (2 if nl <= 4096 else 0)])
    out["info"] = [nl, nc, nb, len(longs), int(chain_cr), levels_reported, top_n, top_waves, blocks, -1, leaf_waves]
    return {k: [int(x) for x in v] for k, v in out.items()}


CASES = [
    # border grid by term count (2 n_chain - segments terms), by width, and no border at all
    case("terms_2047", segs=[1024]), case("terms_2048", segs=[1000, 25]),
    case("wide_655", segs=[328], nb=20), case("wide_656", segs=[300, 29], nb=20),
    case("no_border_5000", segs=[2500, 1], nb=0),
    # long rows of the product
    case("rows_256_257", segs=[3], rows=[256, 257, 3]), case("rows_chunks", segs=[3], rows=[5, 1024, 1025, 8, 2049, 256]),
    case("rows_none", segs=[3], rows=[1, 256, 12]),
    # leaf staging: 8 (m (m + w) + 2 m + w + 2) bytes against 64000, w = 8 + 8 + 2
    case("leaf_62728", segs=[2], nz=8, m=79), case("leaf_64160", segs=[2], nz=8, m=80),
    case("leaf_mixed", segs=[4], nz=8, leaf=[79, 80, 5]),
    # the chain's panel in LDS: 43 unknowns per node 63 736 bytes, 44 66 624 (both too wide for the cyclic reduction)
    case("chain_lds_on", segs=[3], nz=43), case("chain_lds_off", segs=[3], nz=44),
    # cyclic reduction on / off; level lists
    case("cr_on", segs=[8]), case("cr_off_knob", segs=[8], cr=0), case("cr_off_65", segs=[4], chain=[2, 65, 2, 2]),
    case("cr_off_wide", segs=[3], chain=[31, 32, 32]), case("cr_on_64", segs=[3], chain=[31, 31, 31]),
    case("cr_seg_1", segs=[1]), case("cr_seg_2", segs=[2]), case("cr_seg_3", segs=[3]), case("cr_seg_8", segs=[8]), case("cr_seg_9", segs=[9]),
    case("cr_two_phases", segs=[9, 3]),
    case("cr_export", segs=[9, 5, 2], export=[1] + [0] * 7 + [1] + [0] * 4 + [1] + [1, 1]),
    # kkt_cr_top: the cap, one and two trailing levels
    case("top_cap_none", segs=[1024]), case("top_cap_0", segs=[1024], cr_top_cap=0), case("top_cap_1", segs=[1024], cr_top_cap=1),
    case("top_cap_2", segs=[1024], cr_top_cap=2),
    case("top_one_level", segs=[3] + [2] * 20), case("top_two_levels", segs=[5] + [2] * 20),
    case("top_big_nodes", segs=[64], nz=30, nb=1),       # 16 x the wave's bytes no longer fit the workgroup's LDS
    # leaf-forward staging by the leaf count and by the knob
    case("leaves_4096", segs=[4097]), case("leaves_4097", segs=[4098]),
    case("leaf_fwd_0", segs=[5], leaf_fwd=0), case("leaf_fwd_1", segs=[5], leaf_fwd=1), case("leaf_fwd_2", segs=[4098], leaf_fwd=2),
    case("leaf_waves_7", segs=[5], leaf_waves=7),
    # empty parts
    case("no_leaves", segs=[1, 1, 1]), case("no_chain", segs=[]),
    # refusals
    case("refuse_block", segs=[2], nz=8, m=3741),          # 2 m + w + 2 = 7502 doubles
    case("accept_block", segs=[2], nz=8, m=3740),          # 7500
    case("refuse_no_leaf", segs=[3], left=[1]),
    case("refuse_mv_idx", segs=[3], entries=[(4, 2 ** 30, 1)]), case("refuse_mv_kind", segs=[3], entries=[(4, 5, 3)]),
    case("accept_mv_idx", segs=[3], entries=[(4, 2 ** 30 - 1, 2)]),
    case("refuse_export_wide", segs=[3], chain=[31, 32, 32], export=[1, 0, 0]), case("refuse_export_knob", segs=[3], export=[0, 0, 1], cr=0),
]


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    """The sanitizer build's output for every case, by name."""
    exe = os.path.join(ROOT, "tests", "_build", "kkt_shape_sanitize")
    src = os.path.join(ROOT, "tests", "c", "kkt_shape_sanitize.cpp")
    hdrs = [os.path.join(ROOT, "pycollo_amd", "csrc", h) for h in ("pc_kkt_shape.hpp", "pc_kkt_cr.hpp")] + [os.path.join(ROOT, "include", "pycollo_amd.h")]
    if not os.path.exists(exe) or max(os.path.getmtime(f) for f in [src] + hdrs) > os.path.getmtime(exe):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        res = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                              "-fno-omit-frame-pointer", "-o", exe + f".tmp{os.getpid()}", src], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-3000:]
        os.replace(exe + f".tmp{os.getpid()}", exe)
    path = tmp_path_factory.mktemp("kkt_shape") / "cases.txt"
    path.write_text("".join(text(c) for c in CASES))
    res = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-3000:]
    assert res.returncode == 0 and not res.stderr.strip(), res.stderr[-3000:]
    out, name = {}, None
    for ln in res.stdout.splitlines():
        key, _, rest = ln.partition(" ")
        if key == "case":
            name = rest
            out[name] = {}
        elif key == "error":
            out[name] = rest
        elif key != "end":
            out[name][key] = [int(v) for v in rest.split()]
    return out


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_the_shape_follows_the_stated_rules(printed, c):
    want, got = rules(c), printed[c["name"]]
    if isinstance(want, str) or isinstance(got, str):
        assert got == want
        assert c["name"].startswith("refuse_")
        return
    assert not c["name"].startswith("refuse_")
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], k


def test_the_cases_stand_where_they_claim(printed):
    """The thresholds the case names speak of, read off the printed shapes."""
    p = printed
    assert (p["terms_2047"]["border_blocks"], p["terms_2048"]["border_blocks"]) == ([0], [256])
    assert p["terms_2047"]["n_counts"] == [2 * 2048] and p["terms_2048"]["n_counts"] == [2 * 2049]
    assert (p["wide_655"]["border_blocks"], p["wide_656"]["border_blocks"]) == ([0], [256])
    assert p["wide_656"]["n_border_part"] == [256 * 400]
    assert p["no_border_5000"]["border_blocks"] == [0] and p["no_border_5000"]["n_counts"] == [2 * 5001]
    assert p["rows_256_257"]["mv_long"] == [1] and p["rows_256_257"]["n_mv_chunks"] == [1]
    assert p["rows_chunks"]["mv_long"] == [1, 2, 4] and p["rows_chunks"]["mv_long_c0"] == [0, 1, 3, 6]
    assert p["rows_none"]["n_mv_long"] == [0] and p["rows_none"]["n_mv_long_part"] == [1]
    assert p["leaf_62728"]["lds_leaf_full"] == [62728]
    assert p["leaf_64160"]["lds_leaf_full"] == p["leaf_64160"]["lds_leaf"] == [8 * (160 + 18 + 2)]
    assert p["leaf_mixed"]["lds_leaf_full"] == [62728]
    assert (p["chain_lds_on"]["chain_lds"], p["chain_lds_on"]["lds_chain_factor"]) == ([1], [63736])
    assert p["chain_lds_off"]["chain_lds"] == [0] and p["chain_lds_off"]["lds_chain_factor"] == p["chain_lds_off"]["lds_chain"]
    assert [p[k]["chain_cr"] for k in ("cr_on", "cr_off_knob", "cr_off_65", "cr_off_wide", "cr_on_64")] == [[1], [0], [0], [0], [1]]
    assert [len(p[f"cr_seg_{n}"]["cr_lvl_ptr"]) - 1 for n in (1, 2, 3, 8, 9)] == [1, 2, 3, 4, 5]
    assert p["cr_seg_9"]["cr_nodes"] == [1, 3, 5, 7, 2, 6, 4, 8, 0]
    assert p["cr_export"]["export_nodes"] == [0, 8, 13, 14, 15]
    assert [p[f"top_cap_{k}"]["cr_top_n"] for k in ("none", 0, 1, 2)] == [[6], [0], [0], [3]]
    assert p["top_cap_2"]["cr_top_waves"] == [2]
    assert p["top_one_level"]["cr_top_n"] == [0] and p["top_two_levels"]["cr_top_n"] == [2]
    assert p["top_big_nodes"]["cr_top_waves"][0] < 16
    assert (p["leaves_4096"]["leaf_forward_stage"], p["leaves_4097"]["leaf_forward_stage"]) == ([2], [0])
    assert [p[f"leaf_fwd_{k}"]["leaf_forward_stage"] for k in (0, 1, 2)] == [[0], [1], [2]]
    assert p["leaf_waves_7"]["info"][-1] == 7
    assert p["no_leaves"]["info"][:2] == [0, 3] and p["no_chain"]["info"][:2] == [0, 0]
    assert p["refuse_block"] == "KKT block too large for the solver's LDS staging" and isinstance(p["accept_block"], dict)
    assert p["refuse_no_leaf"] == "chain node without a leaf on its right"
    assert p["refuse_mv_idx"] == p["refuse_mv_kind"] == "matvec table entry out of range" and isinstance(p["accept_mv_idx"], dict)
    assert p["refuse_export_wide"] == p["refuse_export_knob"] == "exported chain nodes need the cyclic-reduction kernels (blocks too large for their LDS)"


# ---- the real tables through pc_kkt_shape_info: what tests/test_gpu_kkt_variants.py asserts of GpuKkt.info on a device ----
KNOBS = ("PYCOLLO_AMD_KKT_LEAF_FWD_LDS", "PYCOLLO_AMD_KKT_LEAF_WAVES", "PYCOLLO_AMD_KKT_CR_TOP", "PYCOLLO_AMD_KKT_CR")


def _tables(name, kw, group):
    from pycollo_amd import kkt
    from test_kkt_cpu import kkt_case
    eng, _, _, _, ineq, fixed, sc, _ = kkt_case(name, kw, device=None)
    return kkt.build_tables(eng, ineq, fixed, sc, group)


def _info(monkeypatch, tables, env=None):
    from pycollo_amd import kkt
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    return kkt.shape_info(tables)


def test_border_grid_from_2048_terms(built, monkeypatch):
    info1 = _info(monkeypatch, _tables("hypersensitive", dict(K=1100, order=3), 1))
    assert info1["n_leaf"] + info1["n_chain"] >= 2048 and info1["border_blocks"] > 0
    assert info1["nb"] ** 2 * (info1["n_leaf"] + info1["n_chain"]) <= 2 ** 18
    info0 = _info(monkeypatch, _tables("hypersensitive", dict(K=1100, order=3), None))
    assert info0["n_leaf"] + info0["n_chain"] < 2048 and info0["border_blocks"] == 0


@pytest.mark.parametrize("K,grid", [(163, True), (162, False)])
def test_border_grid_on_a_wide_border(built, monkeypatch, K, grid):
    info = _info(monkeypatch, _tables("time_coupled_transfer", dict(K=K, order=3), 1))
    terms = info["n_leaf"] + info["n_chain"]
    assert terms < 2048
    assert (info["nb"] ** 2 * terms > 2 ** 18) == grid
    assert (info["border_blocks"] > 0) == grid


def test_leaf_forward_from_device_memory_above_4096_leaves(built, monkeypatch):
    info = _info(monkeypatch, _tables("hypersensitive", dict(K=4200, order=3), 1))
    assert info["n_leaf"] > 4096 and info["leaf_forward_stage"] == 0
    assert info["border_blocks"] > 0


@pytest.mark.parametrize("name,kw", [("hypersensitive", dict(K=300, order=6)), ("two_phase_transfer", {}), ("shuttle", dict(K=60, order=4))])
def test_knob_sweeps(built, monkeypatch, name, kw):
    T = _tables(name, kw, None)
    base = _info(monkeypatch, T)
    assert base["leaf_forward_stage"] == 2 and base["leaf_waves"] == 4 and base["chain_cr"] == 1
    assert base["cr_levels"] >= 1
    if kw.get("K") == 300:
        assert base["cr_top_levels"] > 0
    for stage in (0, 1, 2):
        assert _info(monkeypatch, T, {"PYCOLLO_AMD_KKT_LEAF_FWD_LDS": str(stage)})["leaf_forward_stage"] == stage
    for waves in (1, 2, 4):
        assert _info(monkeypatch, T, {"PYCOLLO_AMD_KKT_LEAF_WAVES": str(waves)})["leaf_waves"] == waves
    assert _info(monkeypatch, T, {"PYCOLLO_AMD_KKT_CR_TOP": "0"})["cr_top_levels"] == 0
    info = _info(monkeypatch, T, {"PYCOLLO_AMD_KKT_CR_TOP": "2"})
    assert info["cr_top_waves"] == 2 and info["cr_top_levels"] <= base["cr_top_levels"]
    off = _info(monkeypatch, T, {"PYCOLLO_AMD_KKT_CR": "0"})
    assert off["chain_cr"] == 0 and off["cr_levels"] == 0 and off["cr_top_levels"] == 0
