"""What the evaluation's kernels are handed and how they are launched (csrc/pc_eval_launch.hpp; host work, no GPU).

tests/c/eval_launch_sanitize.cpp builds the argument blocks of real descriptors with made-up device addresses under
AddressSanitizer + UBSan and plans the calls a case lists.  ``expect`` below restates the rules from their description
(DESIGN sections 4 and 4.1, the header's comments, pc_args.h and include/pycollo_amd.h), not from the C++, and must arrive
at the same lines.  The launch shape itself (waves per tile, LDS, tail blocks) is pc_eval_shape.hpp's and is taken from
the program's first lines (tests/test_eval_shape_cpu.py checks those); this file checks what is made of it.  The cases
are the smallest descriptors that reach each rule: sections of order 3 with the tile-nodes knob at 3 give one section per
tile.

The made-up addresses: buffer r starts at r << 32 and prints as "r+bytes" -- Addr's members 1 .. 15 in order, a phase's 13
buffers from 32 + 16 p (sec_h 3, scal 9, partials 11), a caller's partials buffer 0x700 + p, the call's x, lam, c, G, H,
fobj, grad_nz 0x100 .. 0x106."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from pycollo_amd import problems
from test_eval_shape_cpu import engine, tiles_case
from test_sanitized_host import _serialise

SRC = os.path.join(ROOT, "tests", "c", "eval_launch_sanitize.cpp")
EXE = os.path.join(ROOT, "tests", "_build", "eval_launch_sanitize")
HEADER = os.path.join(ROOT, "include", "pycollo_amd.h")
KERNELS = ("res", "res_w", "all", "all_res", "all_res_w", "tail_big")
C, G, H = 1, 2, 4
TAIL_THREADS = 256
MAX_PHASES = 8
X, LAM, NULL = "256+0", "257+0", "0+0"
OUTPUTS = ["258+0", "259+0", "260+0", "261+0", "262+0"]   # c G H fobj grad_nz
SCAL_REFUSAL = "too many scaling constants for the kernel argument block"


def header_constants():
    """PC_LAUNCH_* as include/pycollo_amd.h defines them."""
    text = open(HEADER).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define PC_LAUNCH_(\w+) (\d+)", text)}


L = header_constants()


@pytest.fixture(scope="module")
def harness():
    deps = [SRC, os.path.join(ROOT, "tests", "c", "desc_reader.hpp"), HEADER]
    deps += [os.path.join(ROOT, "pycollo_amd", "csrc", f) for f in ("pc_eval_launch.hpp", "pc_eval_shape.hpp", "pc_desc.hpp", "pc_pattern.hpp", "pc_args.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        os.makedirs(os.path.dirname(EXE), exist_ok=True)
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
               "-fno-omit-frame-pointer", "-o", EXE + f".tmp{os.getpid()}", SRC]
        res = subprocess.run(cmd, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-3000:]
        os.replace(EXE + f".tmp{os.getpid()}", EXE)
    return EXE


def run(harness, tmp_path, eng, steps, knobs=None, compiled=False):
    """The program's lines for the engine's descriptor and the steps, and the facts the rules need.  ``compiled``: the
    descriptor names the kernels compiled for the mesh's one order, as a device handle's does."""
    desc = eng._make_desc(None, 0)
    for ip in range(desc.n_phases if compiled else 0):
        desc.phases[ip].compiled_order = eng.orders[ip]
    fin, fsteps, fout = str(tmp_path / "in.txt"), str(tmp_path / "steps.txt"), str(tmp_path / "out.txt")
    _serialise(eng, desc, fin, knobs=knobs)
    open(fsteps, "w").write("\n".join(steps) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([harness, fin, fsteps, fout], capture_output=True, text=True, env=env, timeout=300)
    assert res.returncode == 0, res.stderr[-4000:]
    assert "Sanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-4000:]
    lines = [ln.split() for ln in open(fout)]
    assert lines[-1] == ["ok"]
    shape = [int(v) for v in lines[0][1:]]
    sizes = [int(v) for v in lines[1][1:]]
    nph = desc.n_phases
    orders = [desc.orders[i] for i in range(desc.n_orders)]
    f = dict(zip(("TB", "wpt_all", "lds_all", "tail_blocks", "tail_blocks_all", "tail_lds", "tail_big", "mixed", "resident", "qa_n"), shape))
    f["size"] = dict(zip(("lead", "phase", "bulk", "tail", "bulk_tail", "multi", "multi_tail", "tail_lead", "tail_launch"), sizes))
    # the tables of the orders in use, packed in the descriptor's order: A (n - 1) x n, weights n
    f["qa_off"] = {n: sum((m - 1) * m for m in orders[:i]) for i, n in enumerate(orders)}
    f["qw_off"] = {n: sum(orders[:i]) for i, n in enumerate(orders)}
    assert f["qa_n"] == sum((m - 1) * m for m in orders)
    f["ph"] = []
    for ip in range(nph):
        v = [int(t) for t in lines[2 + ip][1:]]
        s = desc.phases[ip]
        n_k = [s.n_k[k] for k in range(s.K)]
        p = dict(zip(("n_tiles", "wpt", "lds", "lds_out", "lds_out4", "uni_n", "spt", "x_off", "c_off"), v), K=s.K, N=sum(n_k) - s.K + 1)
        assert p["uni_n"] == (n_k[0] if len(set(n_k)) == 1 and not s.n_fixed_tiles else 0)
        f["ph"].append(p)
    return lines[2 + nph:-1], f


def struct_sizes_hold(f):
    """The composite layouts: the lead's 14 dwords in front of the phase block, the tail's block right behind either bulk
    block (PcMultiArgs is 6 pointers, 2 + 9 + 2 ints and a pointer: 112 bytes), the tail's 12 dwords in front of its own."""
    s = f["size"]
    assert s["lead"] == 56 and s["tail_lead"] == 48 and s["multi"] == 112
    assert s["bulk"] == 56 + s["phase"] and s["bulk_tail"] == s["bulk"] + s["tail"]
    assert s["multi_tail"] == 112 + s["tail"] and s["tail_launch"] == 48 + s["tail"]


class State:
    """What the steps set: the kernels the code object has, ranges, partials buffers, the epoch."""

    def __init__(self, f, have=None, epoch=0):
        self.f, self.have, self.epoch = f, dict(dict.fromkeys(KERNELS, 0), **(have or {})), epoch
        self.rg = [[0, p["n_tiles"], False] for p in f["ph"]]

    def first_record(self, ip):   # records of the launched ranges, phase after phase
        return sum(max(0, e - b) for b, e, _ in self.rg[:ip])


def expect(st, bulk=1, tail=1, flags=C | G | H, lam=1, sigma=1.0):
    """The lines of one call, by the rules."""
    f, have, ph, rg = st.f, st.have, st.f["ph"], st.rg
    n, TB = len(ph), f["TB"]
    lam_s = LAM if lam else NULL
    whole = all(b == 0 and e == p["n_tiles"] and not ext for (b, e, ext), p in zip(rg, ph))
    # one launch: both parts asked for, the knob, the kernel, every phase whole and no caller's partials buffer
    res = bool(bulk and tail and f["resident"] and have["all_res" if n > 1 else "res"] and whole)
    if res:   # the epoch advances on a resident launch only, and is never 0
        st.epoch = (st.epoch + 1) % 2 ** 32 or 1
    out, last = [], 0

    def part(ip):
        return f"{0x700 + ip}+0" if rg[ip][2] else f"{32 + 16 * ip + 11}+0"

    def args(tag, ip, w, epoch, flg, x, lm):
        p = ph[ip]
        rec = st.first_record(ip) if f["mixed"] else -1
        return [tag, ip, rg[ip][0], max(0, rg[ip][1] - rg[ip][0]), w, TB * w, p["lds_out4"] if w == 4 else p["lds_out"], part(ip), rec, epoch,
                flg, p["uni_n"], p["spt"], p["n_tiles"], "1+0", f"1+{8 * f['qa_n']}", x, lm]

    def lead(ip, ntb):
        p, un = ph[ip], ph[ip]["uni_n"]
        return ["lead", p["x_off"], p["c_off"] if lam else -1, "1+0", f"{32 + 16 * ip + 3}+0", p["N"], p["K"], rg[ip][0], max(0, rg[ip][1] - rg[ip][0]),
                flags, p["wpt"], TB * p["wpt"], p["spt"], ntb, f["qa_off"][un] if un else 0, f["qa_n"] + f["qw_off"][un] if un else 0]

    def tail_line(ntb, threads):
        t = ["tail", ntb, threads, st.epoch, flags, f"{sigma:g}", "0.25", X, lam_s] + OUTPUTS
        for ip, p in enumerate(ph):
            t += [part(ip), p["n_tiles"]]
        return t

    if bulk and n > 1 and have["all"]:   # several phases, one launch
        last |= L["MERGED"]
        w, ntb = f["wpt_all"], f["tail_blocks_all"]
        fb = list(np.cumsum([0] + [max(0, e - b) for b, e, _ in rg]))
        fb += [fb[-1]] * (MAX_PHASES + 1 - len(fb))
        multi = ["multi", n, flags, st.epoch, ntb, "15+0" if f["mixed"] else NULL, "14+0", X, lam_s] + fb
        merged = [args("merged", ip, w, 0, 0, NULL, NULL) for ip in range(n)]
        if res:
            name = f"pc_bulk_all_r_w{w}" if have["all_res_w"] else "pc_bulk_all_r"
            out.append(["launch", name, 0, fb[-1] + ntb, TB * w, max(f["lds_all"], f["tail_lds"]), f["size"]["multi_tail"], 1])
            out += [multi] + merged + [tail_line(ntb, TB * w)]
            last |= L["RESIDENT"] | ntb << L["TAIL_BLOCKS_SHIFT"] | (TB * w // 64) << L["TAIL_WAVES_SHIFT"]
            return [["call", 1, last, st.epoch]] + out
        if fb[-1] > 0:
            out.append(["launch", "pc_bulk_all", 0, fb[-1], TB * w, f["lds_all"], f["size"]["multi"], 1])
            out += [multi] + merged
    elif res:   # a single phase with the tail as its leading workgroups
        w, ntb = ph[0]["wpt"], f["tail_blocks"]
        name = f"pc_bulk_p0_r_w{w}" if have["res_w"] else "pc_bulk_p0_r"
        out.append(["launch", name, 0, ph[0]["n_tiles"] + ntb, TB * w, max(ph[0]["lds"], f["tail_lds"]), f["size"]["bulk_tail"], 1])
        out += [lead(0, ntb), args("args", 0, w, st.epoch, flags, X, lam_s), tail_line(ntb, TB * w)]
        last = L["RESIDENT"] | ntb << L["TAIL_BLOCKS_SHIFT"] | (TB * w // 64) << L["TAIL_WAVES_SHIFT"]
        return [["call", 1, last, st.epoch]] + out
    elif bulk:   # a launch per phase; a phase with an empty range has none
        for ip, p in enumerate(ph):
            if rg[ip][1] <= rg[ip][0]:
                continue
            out.append(["launch", f"pc_bulk_p{ip}", ip, rg[ip][1] - rg[ip][0], TB * p["wpt"], p["lds"], f["size"]["bulk"], 1])
            out += [lead(ip, 0), args("args", ip, p["wpt"], st.epoch, flags, X, lam_s)]
    if tail:
        big = bool(have["tail_big"] and f["tail_big"])
        out.append(["launch", "pc_tail_big" if big else "pc_tail", 0, 1, TAIL_THREADS, f["tail_lds"], f["size"]["tail_launch"], 1])
        out.append(["taillead", X, part(0), "41+0", ph[0]["x_off"], ph[0]["n_tiles"], ph[0]["N"], flags, TAIL_THREADS])
        out.append(tail_line(1, TAIL_THREADS))
        last |= (L["TAIL_BIG"] if big else 0) | (TAIL_THREADS // 64) << L["TAIL_WAVES_SHIFT"]
    return [["call", sum(1 for ln in out if ln[0] == "launch"), last, st.epoch]] + out


def have_step(have):
    return "have " + " ".join(str(int(dict(dict.fromkeys(KERNELS, 0), **have)[k])) for k in KERNELS)


def call_step(bulk=1, tail=1, flags=C | G | H, lam=1, sigma=1.0):
    return f"call {bulk} {tail} {flags} {lam} {sigma:g}"


def split_calls(lines):
    """The program's lines, cut at every "call"."""
    calls, other = [], []
    for ln in lines:
        if ln[0] == "call":
            calls.append([ln])
        elif ln[0] in ("launch", "lead", "args", "multi", "merged", "tail", "taillead") and calls:
            calls[-1].append(ln)
        else:
            other.append(ln)
    return calls, other


def same(got, want):
    want = [[str(t) for t in ln] for ln in want]
    assert len(got) == len(want), (got, want)
    for g, w in zip(got, want):
        assert g == w, (g, w)


def decoded(last):
    from pycollo_amd.engine import decode_last_launch
    return decode_last_launch(last)


CALLS = [dict(), dict(flags=C | G, lam=0), dict(flags=H, sigma=2.5), dict(tail=0), dict(bulk=0), dict(tail=0, flags=G, lam=0)]


def check_calls(harness, tmp_path, eng, knobs, have, setup=(), calls=CALLS, epoch=0, ranges=None, compiled=False):
    """Build the blocks once, plan `calls` one after the other, compare every line; returns the facts and the decoded
    last_launch of every call."""
    steps = [have_step(have)] + list(setup) + ([f"epoch {epoch}"] if epoch else []) + ["build"] + [call_step(**c) for c in calls]
    lines, f = run(harness, tmp_path, eng, steps, knobs=knobs, compiled=compiled)
    struct_sizes_hold(f)
    got, other = split_calls(lines)
    assert ["built"] in other, other
    st = State(f, have, epoch)
    for ip, (b, e, ext) in (ranges or {}).items():
        st.rg[ip] = [b, e, ext]
    out = []
    for c, g in zip(calls, got):
        want = expect(st, **c)
        same(g, want)
        out.append(decoded(int(g[0][2])))
        # engine.py decodes what the header's constants encode
        ll = int(g[0][2])
        assert out[-1] == dict(resident=bool(ll & L["RESIDENT"]), tail_big=bool(ll & L["TAIL_BIG"]), merged=bool(ll & L["MERGED"]),
                               tail_blocks=(ll >> L["TAIL_BLOCKS_SHIFT"]) & L["TAIL_BLOCKS_MASK"],
                               tail_block_threads=64 * ((ll >> L["TAIL_WAVES_SHIFT"]) & L["TAIL_WAVES_MASK"]))
    assert len(got) == len(calls)
    return f, out, other


def test_last_launch_constants_mirror_the_header():
    from pycollo_amd.engine import PC_LAUNCH
    assert PC_LAUNCH == L and len(L) == 7
    assert L["RESIDENT"] == 1 and L["TAIL_BIG"] == 2 and L["MERGED"] == 4   # bits 0, 1, 2 (pc_info's comment)
    assert (L["TAIL_BLOCKS_SHIFT"], L["TAIL_BLOCKS_MASK"], L["TAIL_WAVES_SHIFT"], L["TAIL_WAVES_MASK"]) == (4, 7, 8, 15)


def test_single_phase_four_tiles(built, harness, tmp_path):
    eng, knobs = tiles_case("hypersensitive", {}, 4)
    f, info, other = check_calls(harness, tmp_path, eng, knobs, dict(res=1, res_w=1, tail_big=1))
    assert ["launches", "1"] in other
    assert [i["resident"] for i in info] == [True, True, True, False, False, False]
    assert f["ph"][0]["n_tiles"] == 4 and f["ph"][0]["wpt"] == 4 and info[0]["tail_block_threads"] == 256
    # the resident knob off: the tiles, then pc_tail; a code object without the kernel does the same
    for kn, have in ((dict(knobs, resident=0), dict(res=1, res_w=1)), (knobs, dict())):
        f, info, other = check_calls(harness, tmp_path, eng, kn, have)
        assert ["launches", "2"] in other and not any(i["resident"] or i["tail_big"] or i["merged"] for i in info)
        assert [i["tail_block_threads"] for i in info] == [256, 256, 256, 0, 256, 0] and all(i["tail_blocks"] == 0 for i in info)


@pytest.mark.parametrize("tiles", [1024, 1025])
def test_tail_big_by_tile_count(built, harness, tmp_path, tiles):
    eng, knobs = tiles_case("hypersensitive", {}, tiles)
    f, info, _ = check_calls(harness, tmp_path, eng, dict(knobs, resident=0), dict(res=1, tail_big=1), calls=[dict(), dict(bulk=0)])
    assert [i["tail_big"] for i in info] == [tiles == 1025] * 2 and f["tail_big"] == (tiles == 1025)
    f, info, _ = check_calls(harness, tmp_path, eng, dict(knobs, resident=0), dict(res=1), calls=[dict()])   # no such kernel: pc_tail
    assert not info[0]["tail_big"]
    f, info, _ = check_calls(harness, tmp_path, eng, knobs, dict(res=1, tail_big=1), calls=[dict()])   # resident: no separate tail
    assert info[0]["resident"] and not info[0]["tail_big"]


@pytest.mark.parametrize("wpt", [2, 4])
def test_waves_per_tile(built, harness, tmp_path, wpt):
    # five tiles of 64 nodes; the kernel compiled for order 8 stages a state's block in row groups, but in one piece with
    # four waves: the two staging sizes differ (the LDS limit raised so that four waves stand)
    for name, kw, compiled in (("brachistochrone", (("K", 100), ("order", 4)), False), ("shuttle", (("K", 100), ("order", 8)), True)):
        eng = engine(name, kw)
        for have in (dict(res=1, res_w=1), dict(res=1), dict()):
            f, info, _ = check_calls(harness, tmp_path, eng, dict(wpt=wpt, lds_limit=160 * 1024), have, compiled=compiled)
            assert f["ph"][0]["wpt"] == wpt and info[0]["tail_block_threads"] == (64 * wpt if have else 256)
    assert f["ph"][0]["lds_out4"] > f["ph"][0]["lds_out"]
    eng, knobs = tiles_case("sliding_mass", {"num_phases": 2}, 5)
    for have in (dict(all=1, all_res=1, all_res_w=1), dict(all=1, all_res=1), dict(all=1), dict()):
        f, info, _ = check_calls(harness, tmp_path, eng, dict(knobs, wpt=wpt), have)
        assert f["wpt_all"] == wpt and info[0]["merged"] == bool(have) and info[0]["resident"] == ("all_res" in have)


def test_tail_blocks_knob(built, harness, tmp_path):
    eng, knobs = tiles_case("hypersensitive", {}, 4)
    f, info, _ = check_calls(harness, tmp_path, eng, dict(knobs, tail_blocks=3), dict(res=1, res_w=1))
    assert f["tail_blocks"] == 3 and info[0]["tail_blocks"] == 3 and info[3]["tail_blocks"] == 0
    eng, knobs = tiles_case("sliding_mass", {"num_phases": 2}, 4)
    f, info, _ = check_calls(harness, tmp_path, eng, dict(knobs, tail_blocks=3), dict(all=1, all_res=1))
    assert f["tail_blocks_all"] == 3 and info[0]["tail_blocks"] == 3 and info[0]["merged"]


def three_phases(tiles=(5, 1, 3)):
    key = ("three phases", tiles)
    from test_eval_shape_cpu import _ENGINES
    if key not in _ENGINES:
        from pycollo_amd.engine import NlpEngine
        prob = problems.sliding_mass(num_phases=3, K=max(tiles), order=3)
        for ph, t in zip(prob.phases, tiles):
            ph.mesh.number_mesh_sections, ph.mesh.mesh_section_sizes, ph.mesh.number_mesh_section_nodes = t, np.ones(t), np.full(t, 3)
        _ENGINES[key] = NlpEngine(prob, device=None)
    return _ENGINES[key], {"tile_nodes": 3}


def test_three_phases(built, harness, tmp_path):
    eng, knobs = three_phases()
    f, info, other = check_calls(harness, tmp_path, eng, knobs, dict(all=1, all_res=1, all_res_w=1, tail_big=1))
    assert [p["n_tiles"] for p in f["ph"]] == [5, 1, 3] and ["launches", "1"] in other
    assert [(i["resident"], i["merged"]) for i in info] == [(True, True)] * 3 + [(False, True), (False, False), (False, True)]
    # the merged launch and pc_tail: the resident knob off, or no resident kernel
    for kn, have in ((dict(knobs, resident=0), dict(all=1, all_res=1)), (knobs, dict(all=1))):
        f, info, other = check_calls(harness, tmp_path, eng, kn, have)
        assert ["launches", "2"] in other and [(i["resident"], i["merged"]) for i in info][0] == (False, True)
    # the merge knob off (pc_create then looks no merged kernel up): a launch per phase and the tail
    f, info, other = check_calls(harness, tmp_path, eng, dict(knobs, merge=0), dict())
    assert ["launches", "4"] in other and not info[0]["merged"]


def test_tile_range_and_partials_buffer(built, harness, tmp_path):
    eng, knobs = tiles_case("hypersensitive", {}, 4)
    have = dict(res=1, res_w=1)
    f, info, _ = check_calls(harness, tmp_path, eng, knobs, have, setup=["range 0 1 3"], ranges={0: (1, 3, False)})
    assert not any(i["resident"] for i in info)
    f, info, _ = check_calls(harness, tmp_path, eng, knobs, have, setup=["partials 0 1"], ranges={0: (0, 4, True)})
    assert not any(i["resident"] for i in info)
    f, info, _ = check_calls(harness, tmp_path, eng, knobs, have, setup=["range 0 1 3", "range 0 0 4"])   # whole again: resident again
    assert info[0]["resident"]
    # three phases, the middle one's range empty: the others keep their blocks; a rank's range on the last
    eng, knobs = three_phases()
    for have in (dict(all=1, all_res=1), dict()):
        check_calls(harness, tmp_path, eng, knobs, have, setup=["range 1 0 0"], ranges={1: (0, 0, False)})
        check_calls(harness, tmp_path, eng, knobs, have, setup=["range 1 1 1", "range 2 1 3", "partials 2 1"], ranges={1: (1, 1, False), 2: (1, 3, True)})
        f, info, _ = check_calls(harness, tmp_path, eng, knobs, have, setup=[f"range {ip} 0 0" for ip in range(3)], ranges={ip: (0, 0, False) for ip in range(3)})
        assert info[0]["merged"] == bool(have)   # nothing to launch but the tail; the merged path was still the one taken


def mixed_engine(name, kw=()):
    key = ("mixed launch", name, kw)
    from test_eval_shape_cpu import _ENGINES
    if key not in _ENGINES:
        from pycollo_amd.engine import NlpEngine
        prob = problems.REGISTRY[name](**dict(kw))
        n = np.concatenate([np.full(40, 4), np.random.default_rng(3).integers(4, 9, 12), np.full(30, 6)])   # runs of orders 4 and 6, a stretch between
        for ph in prob.phases:
            ph.mesh.number_mesh_sections, ph.mesh.mesh_section_sizes, ph.mesh.number_mesh_section_nodes = n.size, np.ones(n.size), n
        _ENGINES[key] = NlpEngine(prob, device=None, mixed=tuple((4, 6) for _ in prob.phases))
    return _ENGINES[key]


@pytest.mark.parametrize("name,kw", [("sliding_mass", (("num_phases", 1),)), ("sliding_mass", (("num_phases", 2),))])
def test_mixed_records(built, harness, tmp_path, name, kw):
    eng = mixed_engine(name, kw)
    nph = dict(kw)["num_phases"]
    have = dict(res=1, res_w=1) if nph == 1 else dict(all=1, all_res=1)
    f, info, other = check_calls(harness, tmp_path, eng, {}, have)
    nt = [p["n_tiles"] for p in f["ph"]]
    assert f["mixed"] and min(nt) > 4 and all(p["uni_n"] == 0 for p in f["ph"]) and info[0]["resident"]

    def records(other):
        head = [ln for ln in other if ln[0] == "records"][0]
        return [int(v) for v in head[1:]], [[int(v) for v in ln[1:]] for ln in other if ln[0] == "rec"]
    (count, *first), recs = records(other)
    assert count == sum(nt) and first == [sum(nt[:ip]) for ip in range(nph)]
    assert [r[:2] for r in recs] == [[ip, t] for ip in range(nph) for t in range(nt[ip])]
    orders = {(r[0], r[1]): r[2] for r in recs}
    assert {0, 4, 6} <= set(orders.values())   # order-pure tiles of both runs and any-order tiles between
    # a rank's ranges: the records of the launched tiles alone, in launch order
    rg = {ip: (2 + ip, nt[ip] - 1, False) for ip in range(nph)}
    f, info, other = check_calls(harness, tmp_path, eng, {}, have, setup=[f"range {ip} {b} {e}" for ip, (b, e, _) in rg.items()], ranges=rg)
    (count, *first), recs = records(other)
    assert [r[:2] for r in recs] == [[ip, t] for ip in range(nph) for t in range(rg[ip][0], rg[ip][1])] and count == len(recs)
    assert first == [0, nt[0] - 3][:nph] and all(r[2] == orders[(r[0], r[1])] for r in recs)
    # nothing launched: one empty record, so that the buffer is never empty
    f, info, other = check_calls(harness, tmp_path, eng, {}, have, setup=[f"range {ip} 0 0" for ip in range(nph)], ranges={ip: (0, 0, False) for ip in range(nph)})
    assert records(other) == ([1] + [0] * nph, [[0, 0, 0]])


def test_epoch(built, harness, tmp_path):
    eng, knobs = tiles_case("hypersensitive", {}, 4)
    calls = [dict(), dict(tail=0), dict(bulk=0), dict()]
    lines, f = run(harness, tmp_path, eng, [have_step(dict(res=1)), "epoch 4294967295", "build"] + [call_step(**c) for c in calls] +
                   ["range 0 0 2", "build", call_step(), "range 0 0 4", "build", call_step()], knobs=knobs)
    got, _ = split_calls(lines)
    assert [int(g[0][3]) for g in got] == [1, 1, 1, 2, 2, 3]   # wraps past 0; two-launch calls and a rebuild leave it alone
    st = State(f, dict(res=1), 2 ** 32 - 1)
    for c, g in zip(calls, got):
        same(g, expect(st, **c))
    check_calls(harness, tmp_path, eng, knobs, dict(res=1), epoch=41)
    eng, knobs = three_phases()
    check_calls(harness, tmp_path, eng, knobs, dict(all=1, all_res=1), epoch=2 ** 32 - 1)


# the largest value every field can take: flags C | G | H; four waves per tile; 256 threads; a 256-node tile of 2-node
# sections; four tail blocks; the tables of every order 2 .. 20 (A: sum (n - 1) n = 2660 doubles, weights: sum n = 209)
LARGEST = dict(flags=7, wpt=4, threads=256, spt=255, ntb=4, qa=2660, qw=2660 + 209)


def test_lead_words(built, harness, tmp_path):
    eng, knobs = tiles_case("hypersensitive", {}, 4)
    cases = [LARGEST, dict(flags=1, wpt=1, threads=64, spt=0, ntb=0, qa=0, qw=0), dict(flags=2, wpt=2, threads=128, spt=21, ntb=1, qa=12, qw=40)]
    beyond = [dict(LARGEST, wpt=8), dict(LARGEST, wpt=3), dict(LARGEST, threads=320), dict(LARGEST, threads=96), dict(LARGEST, spt=256),
              dict(LARGEST, ntb=5), dict(LARGEST, qa=2661), dict(LARGEST, qw=2660 + 210), dict(LARGEST, spt=-1), dict(LARGEST, ntb=-1)]
    steps = ["words {flags} {wpt} {threads} {spt} {ntb} {qa} {qw}".format(**c) for c in cases + beyond]
    # the check where the blocks are rebuilt, on a real block: wpt, block threads, sections per tile, tail blocks
    steps += [have_step(dict(res=1)), "build", "check 4 256 255 4", "check 8 256 255 4", "check 4 320 255 4", "check 4 256 256 4", "check 4 256 255 5"]
    lines, f = run(harness, tmp_path, eng, steps, knobs=knobs)
    words = [ln for ln in lines if ln[0] == "words"]
    for c, ln in zip(cases, words):
        assert [int(v) for v in ln[1:]] == [1, c["flags"], c["wpt"], c["threads"], c["spt"], c["ntb"], c["qa"], c["qw"]]
    assert [ln[1:] for ln in words[len(cases):]] == [["0"]] * len(beyond)
    assert [ln[1] for ln in lines if ln[0] == "check"] == ["ok", "refused", "refused", "refused", "refused"]
    # ... and fits its bits: 8 of flags, 4 of waves, 4 of threads / 64, 12 of sections, 3 of tail blocks below the sign;
    # 16 of the A-table offset, 15 of the weight-table offset below the sign
    assert LARGEST["flags"] < 2 ** 8 and LARGEST["wpt"] < 2 ** 4 and LARGEST["threads"] // 64 < 2 ** 4 and LARGEST["spt"] < 2 ** 12
    assert LARGEST["ntb"] < 2 ** 3 and LARGEST["qa"] < 2 ** 16 and LARGEST["qw"] < 2 ** 15


def test_scaling_refusal_moves_with_the_blocks(built, harness, tmp_path):
    eng, knobs = tiles_case("hypersensitive", {}, 4)
    lines, _ = run(harness, tmp_path, eng, [have_step(dict(res=1)), "view 0", "scal 96", "build", "view 0", "scal 97", "build", "view 0"], knobs=knobs)
    kinds = [ln[0] for ln in lines if ln[0] in ("view", "built", "refused")]
    assert kinds == ["view", "built", "view", "refused", "refused"]
    assert [" ".join(ln[1:]) for ln in lines if ln[0] == "refused"] == [SCAL_REFUSAL] * 2
    view = [ln for ln in lines if ln[0] == "view"][0]
    assert view[1:3] == [X, "34+0"]   # the point and the phase's sec_s


def kernel_names(source):
    return set(re.findall(r'extern "C" __global__ void (?:__launch_bounds__\(\w+\) )?(?:__attribute__\(\(\w+\([\d,]+\)\)\) )*(\w+)\(', source))


@pytest.mark.parametrize("name,kw,mixed", [("hypersensitive", {}, False), ("hypersensitive", {}, True), ("two_phase_transfer", {}, False),
                                            ("two_phase_transfer", {}, True), ("delta_iii", {}, False)])
def test_names_are_kernels_of_the_generated_source(built, harness, tmp_path, monkeypatch, name, kw, mixed):
    from pycollo_amd import codegen
    eng = engine(name, tuple(sorted(kw.items())))
    model = eng.model
    nph = len(model.phases)
    source = codegen.generate_source(model, mixed=tuple((4, 6) for _ in range(nph)) if mixed else None)
    kernels = kernel_names(source)
    assert "pc_tail" in kernels and "pc_mesh_err_p0" in kernels   # (the pattern finds them)
    lines, _ = run(harness, tmp_path, eng, ["names"])
    names = {ln[1] for ln in lines if ln[0] == "name"}
    names_w = {ln[1] for ln in lines if ln[0] == "name_w"}   # asked for only with that many waves per tile; absent: the plain kernel
    assert names and names <= kernels, names - kernels
    launchable = {k for k in kernels if k.startswith(("pc_bulk", "pc_tail"))}
    assert launchable <= names | names_w, launchable - names - names_w   # ... and the source has no launch kernel the header cannot name
    ws = codegen._static_w_list(model.phases[0], single_phase=True) if nph == 1 else sorted(set.intersection(*[set(codegen._static_w_list(pm)) for pm in model.phases]))
    for w in ws:
        assert (f"pc_bulk_p0_r_w{w}" if nph == 1 else f"pc_bulk_all_r_w{w}") in kernels & (names | names_w)
    # the kernel whose registers decide the two-wave build (codegen.two_wave_occupancy)
    seen = []

    class Recorder(dict):
        def get(self, key, default=None):
            seen.append(key)
            return default
    monkeypatch.setattr(codegen, "code_object_resources", lambda path: Recorder())
    assert codegen.two_wave_occupancy(model, "none.hsaco") == 0
    if any(codegen.is_heavy(pm) for pm in model.phases):
        assert seen and set(seen) <= (names | names_w) & kernels
    else:
        assert not seen
