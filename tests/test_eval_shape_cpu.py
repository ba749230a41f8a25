"""The launch shape of the evaluation (csrc/pc_eval_shape.hpp; host integer work, no GPU).

tests/c/eval_shape_sanitize.cpp builds the shape of real descriptors (the engine's, with the knobs and a few fields set by
the case) under AddressSanitizer + UBSan, walks every table against what it indexes and prints the shape.  ``rules`` below
restates the decisions from their description (the header's comments, DESIGN sections 3, 3.1, 3.2 and 4.1), not from the
C++, and must arrive at the same numbers.  The LDS byte counts a rule compares are taken from the program's own output
(tests/test_sanitized_host.py checks those); this file checks the choices.  The cases are the smallest descriptors on
either side of every rule: tile counts come from sections of order 3 with a tile capacity of 3 nodes (one section per
tile) where the rule allows the tile-nodes knob, the two-wave rules -- which that knob switches off -- have meshes of
their own.

For a mixed mesh whose tiles the library cuts, the tile count of every candidate capacity comes from the tile cutter
(tests/test_mixed_tiles_cpu.py), which ``rules`` does not restate: it takes the program's capacity and count and checks
that the rule allows them (the search's first candidate, the quarter CU, the wave slots); where the search must stop at
its first candidate the cases assert the capacity itself.  A caller's tile table leaves nothing to the cutter and is
restated in full.  The floor of 24 nodes cannot bind on a uniform mesh (more than 400 64-node tiles in at most 1024 tiles
are 25 rows or more to a tile), so it is tested on the mixed path."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from pycollo_amd import problems
from test_sanitized_host import _serialise

SRC = os.path.join(ROOT, "tests", "c", "eval_shape_sanitize.cpp")
EXE = os.path.join(ROOT, "tests", "_build", "eval_shape_sanitize")
QUARTER_CU = 30 * 1280
REFUSALS = {
    "order": "quadrature order outside [2, 20]",
    "tb": "threads_per_block must be 64, 128 or 256",
    "lds": "tile needs more dynamic LDS than a workgroup may request; use a smaller threads_per_block",
    "edge": "the phase descriptor's edge-record counts do not match the Hessian pattern (codegen.edge_flags and pc_pattern.hpp disagree)",
    "quad": "no quadrature table for a section order in use",
    "point": "too many endpoint variables / endpoint constraints for the tail kernel's argument block",
    "owned": "too many Hessian entries owned by the tail kernel (static parameters / endpoint terms)",
    "goff": "too many variables/constraints per phase for the kernel argument block",
    "uniform": "internal error: uniform tiling mismatch",
}
# places in the descriptor text (tests/c/desc_reader.hpp): the header, then the first phase's
TOKEN = dict(n_point=2, n_b=3, n_pthess=6, n_y=9, n_u=10, n_q=11, n_p=12)


@pytest.fixture(scope="module")
def harness():
    deps = [SRC, os.path.join(ROOT, "tests", "c", "desc_reader.hpp"), os.path.join(ROOT, "include", "pycollo_amd.h")]
    deps += [os.path.join(ROOT, "pycollo_amd", "csrc", f) for f in ("pc_eval_shape.hpp", "pc_desc.hpp", "pc_pattern.hpp", "pc_args.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        os.makedirs(os.path.dirname(EXE), exist_ok=True)
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
               "-fno-omit-frame-pointer", "-o", EXE + f".tmp{os.getpid()}", SRC]
        res = subprocess.run(cmd, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-3000:]
        os.replace(EXE + f".tmp{os.getpid()}", EXE)
    return EXE


_ENGINES = {}


def engine(name, kw=(), nodes=None, mixed=None, shard=None):
    """A structure-only engine, kept for the module: ``nodes``: a mesh of exactly so many nodes (sections of order 4 and
    one shorter section for the remainder); ``shard``: (rank, world) of a rank-local handle."""
    key = (name, kw, nodes, mixed, shard)
    if key not in _ENGINES:
        from pycollo_amd.engine import NlpEngine
        from pycollo_amd.sharding import LocalShard
        prob = problems.REGISTRY[name](**dict(kw))
        if nodes:
            n = np.full((nodes - 1) // 3, 4)
            if (nodes - 1) % 3:
                n = np.append(n, (nodes - 1) % 3 + 1)
            for ph in prob.phases:
                ph.mesh.number_mesh_sections, ph.mesh.mesh_section_sizes, ph.mesh.number_mesh_section_nodes = n.size, np.ones(n.size), n
        if mixed:   # runs of orders 4 and 6 with a stretch of several orders between them: 27 000 rows or so
            n = np.concatenate([np.full(2000, 4), np.full(1500, 6), np.random.default_rng(3).integers(4, 9, 300), np.full(2000, 4), np.full(1200, 6)])
            for ph in prob.phases:
                ph.mesh.number_mesh_sections, ph.mesh.mesh_section_sizes, ph.mesh.number_mesh_section_nodes = n.size, np.ones(n.size), n
        if shard:
            _ENGINES[key] = LocalShard(prob, shard[0], shard[1], device=None).engine
        else:
            _ENGINES[key] = NlpEngine(prob, device=None, **(dict(mixed=tuple(mixed for _ in prob.phases)) if mixed else {}))
    return _ENGINES[key]


def run(harness, tmp_path, eng, tpb=0, occ=0, plan_only=0, knobs=None, eval_ops=None, n_edge_rec=None, orders=None, plant=None,
        pthess=None):
    """The harness's output for the engine's descriptor with the case's fields, and the facts the rules need.  ``plant``:
    counts (TOKEN) set in the text alone; ``pthess``: (row, col) pairs in place of the endpoint Hessian list."""
    desc = eng._make_desc(None, tpb)
    desc.two_wave_occupancy, desc.plan_only = occ, plan_only
    fin, fout = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    ph = [desc.phases[i] for i in range(desc.n_phases)]
    ops = list(eval_ops) if isinstance(eval_ops, (list, tuple)) else [eval_ops if eval_ops is not None else s.eval_ops for s in ph]
    _serialise(eng, desc, fin, knobs=knobs, eval_ops=ops, n_edge_rec=n_edge_rec)
    if orders is not None:   # the list of quadrature orders alone, in the text: the tables keep their sizes
        tok = open(fin).read().split()
        at = len(tok) - (17 + 3 * desc.n_phases + sum(desc.orders[i] for i in range(desc.n_orders)) + desc.n_orders)
        tok[at:at + len(orders)] = [str(n) for n in orders]
        open(fin, "w").write(" ".join(tok) + "\n")
    if plant or pthess is not None:
        tok = open(fin).read().split()
        for key, v in (plant or {}).items():
            tok[TOKEN[key]] = str(v)
        if pthess is not None:
            end = len(tok) - (17 + 3 * desc.n_phases + sum(desc.orders[i] for i in range(desc.n_orders)) + desc.n_orders + 4)
            tok[end - 2 * desc.n_pthess:end] = [str(r) for r, _ in pthess] + [str(c) for _, c in pthess]
            tok[TOKEN["n_pthess"]] = str(len(pthess))
        open(fin, "w").write(" ".join(tok) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([harness, fin, fout], capture_output=True, text=True, env=env, timeout=300)
    assert res.returncode == 0, res.stderr[-4000:]
    assert "Sanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-4000:]
    got = {"phase": [], "lds": [], "caps": []}
    for line in open(fout):
        p = line.split()
        if p[0] == "refused":
            got["refused"] = line[len("refused "):].strip()
        elif p[0] == "rec":
            got["rec"] = p[1:]
        elif p[0] in got and isinstance(got[p[0]], list):
            got[p[0]].append([int(v) for v in p[1:]])
        else:
            got[p[0]] = [int(v) for v in p[1:]]
    facts = dict(tpb=tpb, occ=occ, plan_only=plan_only, knobs=dict(knobs or {}), eval_ops=ops,
                 n_y=[s.n_y for s in ph], n_k=[np.array([s.n_k[k] for k in range(s.K)]) for s in ph],
                 mixed=[s.n_spec > 0 for s in ph], fixed=[s.n_fixed_tiles for s in ph])
    return got, facts


def rules(f, got):
    """What the header's comments say the shape must be, given the facts of the descriptor and the byte counts (and, for a
    mixed mesh, the tile counts) the program printed.  Returns the shape in the program's terms."""
    kn = f["knobs"]
    lds_limit = kn.get("lds_limit", 64 * 1024)
    rows = [int((n - 1).sum()) for n in f["n_k"]]
    nodes = max(r + 1 for r in rows)
    max_nk = max(2, max(int(n.max()) for n in f["n_k"]))
    heavy = [ops > 4000 for ops in f["eval_ops"]]
    mixed = any(f["mixed"])
    # threads per block: the knob, else the descriptor, else by the longest phase -- a one-state light model goes wide early
    tb = kn.get("tb", f["tpb"])
    auto = tb == 0
    if auto:
        tb = 256 if nodes >= 262144 else 128 if nodes >= 65536 else 64
        if all(ny == 1 and not h for ny, h in zip(f["n_y"], heavy)) and nodes >= 25000:
            tb = 256
    if tb not in (64, 128, 256):
        return {"refused": REFUSALS["tb"]}
    while auto and tb > 64 and got["need1"][{64: 0, 128: 1, 256: 2}[tb]] > lds_limit:
        tb //= 2
    # two waves per 64-node tile, four workgroups per CU
    tiles64 = sum((r + 63) // 63 for r in rows)
    two_wave = (f["occ"] >= 2 and tb == 64 and "wpt" not in kn and "tile_nodes" not in kn and kn.get("two_wave", 1) != 0
                and min(f["n_y"]) >= 2 and 400 < tiles64 <= kn.get("two_wave_max_tiles", 1 << 30))
    tc = tb
    out = {}
    if two_wave:
        need2 = dict(zip(range(2, 65), got["need2u" if mixed else "need2"]))
        cap = 64
        while cap > max(max_nk, 32) and need2[cap] > QUARTER_CU:
            cap -= 1
        want = kn.get("two_wave_tiles", 896)
        first = cap if want <= 0 else max(max_nk, 24, min(cap, -(-sum(rows) // want) + 1))
        first = min(first, cap)
        if not mixed:
            def tiles_at(t):   # whole sections of the largest order per tile
                return sum(-(-r // max(1, (t - 1) // (int(n.max()) - 1) * (int(n.max()) - 1))) for r, n in zip(rows, f["n_k"]))
            fit = [t for t in range(first, cap + 1) if 2 * tiles_at(t) <= 2048] if need2[cap] <= QUARTER_CU else []
            two_wave, tc = (True, fit[0]) if fit else (False, tb)
        elif any(f["fixed"]):   # the caller's tiles: kept when they fit a quarter CU with two regions and the wave slots
            fits = all(l[1] <= QUARTER_CU for l, m in zip(got["lds"], f["mixed"]) if m) and need2[64] <= QUARTER_CU
            two_wave = fits and 2 * sum(f["fixed"]) <= kn.get("two_wave_max_waves", 2048)
            tc = 64
        else:   # the cutter's tile count decides: the program's choice must be one the rule allows
            n_tiles = sum(p[0] for p in got["phase"])
            two_wave = bool(got["shape"][2])
            if two_wave:
                assert 2 * n_tiles <= kn.get("two_wave_max_waves", 2048)
                assert first <= got["shape"][1] <= cap and need2[got["shape"][1]] <= QUARTER_CU
                assert all(l[1] <= QUARTER_CU for l in got["lds"])
            tc = got["shape"][1] if two_wave else tb
    if "tile_nodes" in kn and max_nk <= kn["tile_nodes"] <= tb:
        tc = kn["tile_nodes"]
    out["shape"] = [tb, tc, int(two_wave), int(mixed)]
    if f["plan_only"]:
        return out

    def wpt_rule(n_y, is_heavy, tiles, lds, per_phase):
        if tb != 64:
            return 1
        w = 1
        if n_y >= 2 and tiles <= (512 if is_heavy else 1024):
            w = 2
        if n_y >= 3 and tiles <= 400:
            w = 4
        if per_phase and n_y == 1 and not is_heavy and kn.get("resident", 1):   # the tail beside the tiles waits for the last store
            w = 4 if tiles <= 400 else 2 if tiles <= 1024 else 1
        if kn.get("wpt") in (1, 2, 4):
            w = kn["wpt"]
        if two_wave:
            w = 2
        while w > 1 and lds[w] > lds_limit:
            w //= 2
        return w
    out["phase"], lds_all = [], {1: 0, 2: 0, 4: 0}
    for ip, n in enumerate(f["n_k"]):
        lds = dict(zip((1, 2, 4), got["lds"][ip]))
        uniform = bool((n == n[0]).all()) and not f["fixed"][ip]
        spt = (tc - 1) // (int(n[0]) - 1) if uniform else 0
        n_tiles = -(-len(n) // spt) if uniform and not f["mixed"][ip] else got["phase"][ip][0]
        w = wpt_rule(f["n_y"][ip], heavy[ip], n_tiles, lds, True)
        if lds[w] > lds_limit:
            return {"refused": REFUSALS["lds"]}
        out["phase"].append(dict(n_tiles=n_tiles, uni_n=int(n[0]) if uniform else 0, spt=spt, wpt=w, lds_bytes=lds[w]))
        lds_all = {k: max(v, lds[k]) for k, v in lds_all.items()}
    total = sum(p["n_tiles"] for p in out["phase"])
    w_all = wpt_rule(min(f["n_y"]), any(heavy), total, lds_all, False) if len(rows) > 1 else 1
    out["merged"] = [w_all, lds_all[w_all] if len(rows) > 1 else 0]
    # the tail: its carve, and a workgroup per part of a large endpoint block when the tiles' workgroups are narrow
    owned, point, n_b, pthess = got["carve"]
    heavy_point = point + n_b + pthess > 16
    knob = min(4, max(0, kn.get("tail_blocks", 0)))
    blocks = [knob if knob > 0 else (4 if heavy_point and tb * w < 256 else 1) for w in (out["phase"][0]["wpt"], w_all)]
    nred = got["tail"][1]
    out["tail"] = [max(p["lds_bytes"] for p in out["phase"]), nred, 8 * (owned + 17 * nred + point + n_b + 2 * pthess + 2), int(heavy_point)] + blocks
    out["tail"].append(int(any(p["n_tiles"] > 4 * 256 for p in out["phase"])))   # a separate tail launch: more than four strides of 256 lanes
    num_x, num_c, n_jgrad, nG, nH = got["sizes"]
    up = lambda v: -(-v // 32) * 32   # noqa: E731  (256-byte boundaries)
    o_lam, o_c = up(num_x), up(1 + n_jgrad)
    o_G = o_c + up(num_c)
    out["blocks"] = [o_lam, o_lam + up(num_c), 0, 1, o_c, o_G, o_G + up(nG), o_G + up(nG) + up(nH)]
    return out


def check(got, f):
    want = rules(f, got)
    if "refused" in want or "refused" in got:
        assert got.get("refused") == want.get("refused"), (got.get("refused"), want)
        return want
    assert got["shape"] == want["shape"], (got["shape"], want["shape"])
    if f["plan_only"]:
        return want
    for ip, p in enumerate(want["phase"]):
        g = got["phase"][ip]
        assert dict(n_tiles=g[0], uni_n=g[1], spt=g[2], wpt=g[8], lds_bytes=g[9]) == p, (ip, g, p)
    for key in ("merged", "tail", "blocks"):
        assert got[key] == want[key], (key, got[key], want[key])
    return want


def tiles_case(name, kw, tiles):
    """``tiles`` tiles per phase: as many sections of order 3, one to a tile of 3 nodes."""
    return engine(name, tuple(sorted(dict(kw, K=tiles, order=3).items()))), {"tile_nodes": 3}


# n_y = 1, 2, 3
MODELS = [("hypersensitive", {}), ("sliding_mass", {"num_phases": 1}), ("brachistochrone", {})]


@pytest.mark.parametrize("tiles", [400, 401, 512, 513, 1024, 1025])
@pytest.mark.parametrize("name,kw", MODELS)
def test_waves_per_tile_by_tile_count(built, harness, tmp_path, name, kw, tiles):
    eng, knobs = tiles_case(name, kw, tiles)
    seen = set()
    for ops in (4000, 4001):
        for resident in (1, 0):
            got, f = run(harness, tmp_path, eng, knobs=dict(knobs, resident=resident), eval_ops=ops)
            seen.add(check(got, f)["phase"][0]["wpt"])
    assert got["phase"][0][0] == tiles
    assert seen <= {1, 2, 4}


@pytest.mark.parametrize("wpt,expect", [(1, 1), (2, 2), (4, 4), (3, None)])
def test_waves_per_tile_knob(built, harness, tmp_path, wpt, expect):
    eng, knobs = tiles_case("brachistochrone", {}, 450)
    got, f = run(harness, tmp_path, eng, knobs=dict(knobs, wpt=wpt))
    want = check(got, f)
    assert want["phase"][0]["wpt"] == (expect if expect else 2)   # 3 is ignored: 450 tiles of a light three-state model run two waves


def test_waves_per_tile_halve_until_the_lds_fits(built, harness, tmp_path):
    eng, knobs = engine("brachistochrone", (("K", 100), ("order", 4))), {}   # five tiles of 64 nodes: the staging counts
    got, f = run(harness, tmp_path, eng, knobs=knobs)
    l1, l2, l4 = got["lds"][0]
    assert l1 < l2 < l4
    for limit, w in ((l4, 4), (l4 - 1, 2), (l2 - 1, 1)):
        got, f = run(harness, tmp_path, eng, knobs=dict(knobs, lds_limit=limit))
        assert check(got, f)["phase"][0]["wpt"] == w
    got, f = run(harness, tmp_path, eng, knobs=dict(knobs, lds_limit=l1 - 1))
    assert got["refused"] == REFUSALS["lds"]


@pytest.mark.parametrize("tiles", [200, 201, 256, 257, 512, 513])   # per phase: 400 / 401 ... in the merged launch
def test_merged_launch_waves_per_tile(built, harness, tmp_path, tiles):
    """Two phases in one launch: the rule on the total tile count, the smaller n_y and "any phase heavy" -- and no
    one-state rule."""
    eng, knobs = tiles_case("sliding_mass", {"num_phases": 2}, tiles)
    for ops in (None, [10, 4001]):
        got, f = run(harness, tmp_path, eng, knobs=knobs, eval_ops=ops)
        assert check(got, f)["merged"][0] == (2 if 2 * tiles <= (512 if ops else 1024) else 1)
    for wpt in (1, 2, 4, 3):
        got, f = run(harness, tmp_path, eng, knobs=dict(knobs, wpt=wpt))
        check(got, f)
    eng3, knobs = tiles_case("two_phase_transfer", {}, tiles)   # n_y = 2 in both phases
    got, f = run(harness, tmp_path, eng3, knobs=knobs)
    check(got, f)


def uneven_phases(K):
    """sliding_mass in two phases whose first carries a third state (the distance again): n_y = 3 and 2."""
    prob = problems.sliding_mass(num_phases=2, K=K, order=3)
    ph = prob.phases[0]
    x, v = ph.state_variables[0], ph.state_variables[1]
    import sympy as sym
    w = sym.Symbol("w")
    ph.state_variables = [x, v, w]
    ph.state_equations = list(ph.state_equations) + [v]
    ph.bounds.state_variables = [[0.0, 0.5], [0, 10.0], [0.0, 1.0]]
    ph.bounds.initial_state_constraints = {x: 0.0, v: 0, w: 0.0}
    ph.bounds.final_state_constraints = {x: 0.5, v: [0, 10.0], w: [0.0, 1.0]}
    ph.guess.state_variables = np.array([[0.0, 0.5], [0.0, 0.0], [0.0, 0.5]])
    return prob


@pytest.mark.parametrize("tiles", [200, 201])
def test_merged_launch_takes_the_smallest_state_count(built, harness, tmp_path, tiles):
    """Phases of three and two states: four waves per tile need three states in every phase, so the merged launch of
    400 tiles runs two where the first phase alone runs four; and its waves are halved until the LDS fits."""
    from pycollo_amd.engine import NlpEngine
    key = ("uneven", tiles)
    if key not in _ENGINES:
        _ENGINES[key] = NlpEngine(uneven_phases(tiles), device=None)
    got, f = run(harness, tmp_path, _ENGINES[key], knobs={"tile_nodes": 3})
    assert f["n_y"] == [3, 2]
    want = check(got, f)
    assert want["merged"][0] == 2 and [p["wpt"] for p in want["phase"]] == [4, 2]
    eng = engine("sliding_mass", (("K", 40), ("num_phases", 2), ("order", 4)))   # two tiles of 64 nodes a phase: the staging counts
    got, f = run(harness, tmp_path, eng)
    l1, l2 = max(l[0] for l in got["lds"]), max(l[1] for l in got["lds"])
    assert l1 < l2 and check(got, f)["merged"] == [2, l2]
    got, f = run(harness, tmp_path, eng, knobs={"lds_limit": l2 - 1})
    assert check(got, f)["merged"] == [1, l1]


@pytest.mark.parametrize("nodes", [65535, 65536, 262143, 262144])
def test_auto_threads_per_block_by_nodes(built, harness, tmp_path, nodes):
    eng = engine("hypersensitive", nodes=nodes)
    got, f = run(harness, tmp_path, eng, eval_ops=4001)   # (not the one-state rule)
    assert check(got, f)["shape"][0] == (256 if nodes >= 262144 else 128 if nodes >= 65536 else 64)


@pytest.mark.parametrize("nodes", [24999, 25000])
def test_auto_threads_per_block_one_state(built, harness, tmp_path, nodes):
    eng = engine("hypersensitive", nodes=nodes)
    for ops in (4000, 4001):
        got, f = run(harness, tmp_path, eng, eval_ops=ops)
        assert check(got, f)["shape"][0] == (256 if nodes >= 25000 and ops <= 4000 else 64)
    got, f = run(harness, tmp_path, eng)
    n256, n128 = got["need1"][2], got["need1"][1]
    for limit, tb in ((n256, 256), (n256 - 1, 128), (n128 - 1, 64)):   # halved until the staging fits
        got, f = run(harness, tmp_path, eng, knobs=dict(lds_limit=limit))
        assert check(got, f)["shape"][0] == (tb if nodes >= 25000 else 64)


@pytest.mark.parametrize("tpb,knob,ok", [(64, None, True), (128, None, True), (256, None, True), (96, None, False), (0, 128, True), (64, 32, False)])
def test_threads_per_block_given(built, harness, tmp_path, tpb, knob, ok):
    got, f = run(harness, tmp_path, engine("cart_pole", (("K", 50), ("order", 4))), tpb=tpb, knobs={} if knob is None else {"tb": knob})
    want = check(got, f)
    assert ("refused" in want) == (not ok)
    if ok:
        assert want["shape"][0] == (knob or tpb)


# the rule counts 63 rows to a tile on the node count: 400 from 25 197 rows, 401 from 25 200
@pytest.mark.parametrize("K", [8399, 8400])
def test_two_wave_build(built, harness, tmp_path, K):
    eng = engine("sliding_mass", (("K", K), ("num_phases", 1), ("order", 4)))
    on = (3 * K + 1 + 62) // 63 > 400
    for occ in (1, 2):
        got, f = run(harness, tmp_path, eng, occ=occ)
        assert check(got, f)["shape"][2] == int(on and occ == 2)
    for knobs in ({"wpt": 2}, {"tile_nodes": 64}, {"two_wave": 0}, {"two_wave_max_tiles": 400}, {"two_wave_max_tiles": 401}):
        got, f = run(harness, tmp_path, eng, occ=2, knobs=knobs)
        assert check(got, f)["shape"][2] == int(on and knobs == {"two_wave_max_tiles": 401})
    got, f = run(harness, tmp_path, engine("hypersensitive", (("K", K), ("order", 4))), occ=2)   # one state
    assert check(got, f)["shape"][2] == 0


def test_two_wave_tile_capacity(built, harness, tmp_path):
    """The capacity that cuts the mesh into about 896 tiles, never under max(largest section, 24) nodes, at most what a
    quarter CU holds; every wave resident (2048) or one wave per tile and tiles of the block's size."""
    eng = engine("sliding_mass", (("K", 12000), ("num_phases", 1), ("order", 4)))   # 36 000 rows: 41 to a tile for 896 tiles, 42 nodes
    got, f = run(harness, tmp_path, eng, occ=2)
    assert check(got, f)["shape"][1:3] == [42, 1]
    got, f = run(harness, tmp_path, eng, occ=2, knobs={"two_wave_tiles": 0})
    assert check(got, f)["shape"][1:3] == [64, 1]
    big = engine("sliding_mass", (("K", 22000), ("num_phases", 1), ("order", 4)))   # 66 000 rows: 1048 tiles at 64 nodes
    got, f = run(harness, tmp_path, big, tpb=64, occ=2)
    assert check(got, f)["shape"] == [64, 64, 0, 0]
    edge = engine("sliding_mass", (("K", 21 * 1024), ("num_phases", 1), ("order", 4)))   # exactly 1024 tiles of 64 nodes
    got, f = run(harness, tmp_path, edge, occ=2)
    assert check(got, f)["shape"] == [64, 64, 1, 0]


def test_mixed_mesh(built, harness, tmp_path):
    eng = engine("sliding_mass", (("num_phases", 1),), mixed=(4, 6))
    got, f = run(harness, tmp_path, eng)
    assert check(got, f)["shape"][3] == 1 and got["caps"][0][0] <= 32
    for occ in (0, 2):
        for knobs in ({}, {"mix_cap_rows": 20}, {"mix_cap_rows": 4}, {"mix_min_run_rows": 40}, {"two_wave_max_waves": 100}):
            got, f = run(harness, tmp_path, eng, occ=occ, knobs=knobs)
            want = check(got, f)
            assert got["caps"][0][0] <= max(8, knobs.get("mix_cap_rows", 32))
            assert got["caps"][0][1] == knobs.get("mix_min_run_rows", 24)
            if knobs == {"two_wave_max_waves": 100} or occ == 0:
                assert want["shape"][1:3] == [64, 0]       # dropped: one wave per tile, tiles of the block's size
    got, f = run(harness, tmp_path, eng, occ=2)
    assert got["shape"][2] == 1                             # kept
    # a target of 5000 tiles asks for 7 nodes a tile: never under max(largest section, 24); with wave slots to spare the
    # search stops at its first candidate
    got, f = run(harness, tmp_path, eng, occ=2, knobs={"two_wave_tiles": 5000, "two_wave_max_waves": 1 << 20})
    assert check(got, f)["shape"][1:3] == [24, 1]
    got, f = run(harness, tmp_path, eng, occ=2, knobs={"two_wave_tiles": 896, "two_wave_max_waves": 1 << 20})
    assert check(got, f)["shape"][1:3] == [-(-sum(int((n - 1).sum()) for n in f["n_k"]) // 896) + 1, 1]


def test_two_wave_dropped_over_a_quarter_cu(built, harness, tmp_path):
    """One 16-node section among sections of order 4 in a kernel for any order: the staging is sized by the longest row,
    two regions of 31 rows pass a quarter CU while one region of 63 rows fits a workgroup -- one wave per tile, tiles of
    the block's size; the same mesh without that section keeps the build."""
    from pycollo_amd.engine import NlpEngine
    for name in ("shuttle", "free_flying_robot"):
        for long_section in (True, False):
            key = ("quarter", name, long_section)
            if key not in _ENGINES:
                prob = problems.REGISTRY[name]()
                n = np.append(np.full(8400, 4), 16) if long_section else np.full(8400, 4)
                for ph in prob.phases:
                    ph.mesh.number_mesh_sections, ph.mesh.mesh_section_sizes, ph.mesh.number_mesh_section_nodes = n.size, np.ones(n.size), n
                _ENGINES[key] = NlpEngine(prob, device=None)
            got, f = run(harness, tmp_path, _ENGINES[key], tpb=64, occ=2)
            want = check(got, f)
            over = got["need2"][32 - 2] > QUARTER_CU
            assert over == long_section
            if over:
                assert want["shape"] == [64, 64, 0, 0] and want["phase"][0]["wpt"] == 1 and got["lds"][0][0] <= 64 * 1024
            else:
                assert want["shape"][2] == 1


def test_rank_local_handle(built, harness, tmp_path):
    """A caller's tile table: two waves per tile when its tiles fit a quarter CU and the wave slots, else one."""
    eng = engine("sliding_mass", (("K", 18900), ("num_phases", 1), ("order", 4)), shard=(1, 2))   # half of 900 tiles and a halo
    got, f = run(harness, tmp_path, eng, tpb=64, occ=2)
    assert check(got, f)["shape"][2] == 1
    got, f = run(harness, tmp_path, eng, tpb=64, occ=2, knobs={"two_wave_max_waves": 2 * sum(p[0] for p in got["phase"]) - 1})
    assert check(got, f)["shape"][1:3] == [64, 0]


@pytest.mark.parametrize("name,kw,heavy", [("hypersensitive", {}, False), ("time_coupled_transfer", {}, True), ("delta_iii", {}, True)])
def test_tail(built, harness, tmp_path, name, kw, heavy):
    eng = engine(name, tuple(sorted(kw.items())))
    for tpb in (64, 128, 256):
        for blocks in (0, 3, 9):
            got, f = run(harness, tmp_path, eng, tpb=tpb, knobs={"tail_blocks": blocks, "wpt": 1})
            want = check(got, f)
            assert want["tail"][3] == int(heavy)
            assert want["tail"][4] == (min(blocks, 4) if blocks else 4 if heavy and tpb < 256 else 1)


def test_heavy_point_boundary(built, harness, tmp_path):
    """16 / 17 endpoint variables, constraints and Hessian entries: the count of endpoint constraints set in the text."""
    eng = engine("hypersensitive")
    got, f = run(harness, tmp_path, eng)
    _, point, n_b, pthess = got["carve"]
    assert point + n_b + pthess < 16
    seen = {}
    for total in (16, 17):
        got, f = run(harness, tmp_path, eng, plant={"n_b": total - point - pthess}, knobs={"wpt": 1})
        assert sum(got["carve"][1:]) == total
        seen[total] = check(got, f)["tail"][3:5]
    assert seen == {16: [0, 1], 17: [1, 4]}   # ... and with it a tail workgroup per part beside tiles of one wave
    for name in ("brachistochrone", "cart_pole", "sliding_mass", "two_phase_transfer", "shuttle", "free_flying_robot"):
        got, f = run(harness, tmp_path, engine(name))
        check(got, f)


@pytest.mark.parametrize("name,kw", [("time_coupled_transfer", {}), ("delta_iii", {"K": 7, "order": 5}), ("two_phase_transfer", {})])
def test_edge_records(built, harness, tmp_path, name, kw):
    """Endpoint terms on edge-node Hessian entries: the records the shape finds are the counts the code generator ranks its
    flags by; a count that is off by one is refused."""
    eng = engine(name, tuple(sorted(kw.items())))
    got, f = run(harness, tmp_path, eng)
    check(got, f)
    desc = eng._make_desc(None, 0)
    counts = [[desc.phases[i].n_edge_rec[0], desc.phases[i].n_edge_rec[1]] for i in range(desc.n_phases)]
    assert int(got["rec"][0]) == sum(map(sum, counts)) > 0
    first = [p[10] for p in got["phase"]]
    assert first == [int(v) for v in np.concatenate([[0], np.cumsum([sum(c) for c in counts])[:-1]])]
    ip = max(range(len(counts)), key=lambda i: sum(counts[i]))
    counts[ip][1] += 1
    got, f = run(harness, tmp_path, eng, n_edge_rec=counts)
    assert got["refused"] == REFUSALS["edge"]


def test_refusals(built, harness, tmp_path):
    eng = engine("cart_pole", (("K", 50), ("order", 4)))
    got, _ = run(harness, tmp_path, eng, orders=[21])
    assert got["refused"] == REFUSALS["order"]
    got, _ = run(harness, tmp_path, eng, orders=[5])
    assert got["refused"] == REFUSALS["quad"]
    got, _ = run(harness, tmp_path, eng, tpb=100)
    assert got["refused"] == REFUSALS["tb"]
    got, _ = run(harness, tmp_path, eng, tpb=256, knobs={"lds_limit": 4096})
    assert got["refused"] == REFUSALS["lds"]
    got, _ = run(harness, tmp_path, eng, plant={"n_b": 33})    # PC_MAX_ENDPOINT_ROWS = 32
    assert got["refused"] == REFUSALS["point"]
    got, _ = run(harness, tmp_path, eng, plant={"n_b": 32})
    assert "refused" not in got
    ph = eng._make_desc(None, 0).phases[0]
    got, _ = run(harness, tmp_path, eng, plant={"n_p": 33 - ph.n_y - ph.n_q})    # 33 functions a phase, PC_MAX_GOFF = 32
    assert got["refused"] == REFUSALS["goff"]
    got, _ = run(harness, tmp_path, eng, plant={"n_p": 32 - ph.n_y - ph.n_q})
    assert "refused" not in got
    # every pair of Delta III's endpoint variables as an endpoint Hessian entry: more than PC_TAIL_OWNED_MAX = 1024 of them
    # are the tail's alone
    big = engine("delta_iii", (("K", 7), ("order", 5)))
    n_point = big._make_desc(None, 0).n_point
    pairs = [(r, c) for r in range(n_point) for c in range(r + 1)]
    assert len(pairs) > 1024 + 4 * 2 * 7 * 8
    got, _ = run(harness, tmp_path, big, pthess=pairs)
    assert got["refused"] == REFUSALS["owned"]


def test_uniform_tiling_mismatch(built, harness, tmp_path):
    """A uniform mesh computes its tiles from the tile index; the mixed build's cutter must have cut the same tiles: 20
    sections of order 4 are one tile either way.  With the run kept out of tiles of its own (the min-run-rows knob) the
    cutter's 32-row tiles are not those."""
    from pycollo_amd.engine import NlpEngine
    if "uniform mixed" not in _ENGINES:
        _ENGINES["uniform mixed"] = NlpEngine(problems.sliding_mass(num_phases=1, K=20, order=4), device=None, mixed=((4,),))
    got, f = run(harness, tmp_path, _ENGINES["uniform mixed"])
    assert check(got, f)["phase"][0]["spt"] == 21
    got, f = run(harness, tmp_path, _ENGINES["uniform mixed"], knobs={"mix_min_run_rows": 1000})
    assert got["refused"] == REFUSALS["uniform"]


def test_plan_only_stops_at_the_tiles(built, harness, tmp_path):
    eng = engine("delta_iii", (("K", 3000), ("order", 5)))
    got, f = run(harness, tmp_path, eng, occ=2, plan_only=1)
    check(got, f)
    full, f = run(harness, tmp_path, eng, occ=2)
    check(full, f)
    assert got["shape"] == full["shape"] and [p[0] for p in got["phase"]] == [p[0] for p in full["phase"]]
    assert "tail" not in got and "ok" in got
