"""Static instruction counts of a kernel's per-replica tile bodies, from a code object and without a GPU.

    python tools/replica_body_stats.py pycollo_amd/_cache/model_<digest>_<stamp>_n6.hsaco pc_bulk_p0_r_w4
    python tools/replica_body_stats.py OBJ KERNEL --count s_xor --count s_cbranch_execz

The code object (an offload bundle as hipcc --genco writes it, or the bare ELF) is unbundled with
clang-offload-bundler and disassembled with llvm-objdump.  A _w<W> kernel dispatches on the wave index with a chain
of scalar compare-and-branch at its entry, so the kernel's text is cut at that chain's targets (and again where a
piece starts with such a chain of its own): piece 0 is the entry, the others are the replica bodies in address
order -- the highest replica first, as the compiler lays them out -- and the last one also holds whatever code the
compiler shares between bodies or places behind them (the resident tail).  A body is nearly all straight-line code
for an interior tile, so the static counts are close to the executed ones.

Mnemonics are classified by prefix only: s_load, s_waitcnt, s_cbranch / s_branch, other s_, v_, ds_, global_ / buffer_,
anything else.  --count PREFIX adds a column with the mnemonics that start with PREFIX (any prefix the caller likes).
The only mnemonics the tool itself names are the two it finds the branch chain by: the broadcast of a lane's value to a
scalar and the conditional branch on the scalar condition code.  A reporting tool, not a test."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

CLASSES = (("s_load", ("s_load",)), ("s_waitcnt", ("s_waitcnt",)), ("branch", ("s_cbranch", "s_branch")), ("other s_", ("s_",)),
           ("v_", ("v_",)), ("ds_", ("ds_",)), ("vmem", ("global_", "buffer_")))


def llvm_tool(name):
    for cand in (shutil.which(name), f"/opt/rocm/llvm/bin/{name}", f"/opt/rocm/lib/llvm/bin/{name}"):
        if cand and os.path.exists(cand):
            return cand
    raise SystemExit(f"{name} not found (ROCm's llvm/bin)")


def bare_elf(path, arch, tmp):
    """The device ELF of ``path``: the file itself, or the bundle's entry for ``arch``."""
    with open(path, "rb") as f:
        if f.read(24) != b"__CLANG_OFFLOAD_BUNDLE__":
            return path
    out = os.path.join(tmp, "device.elf")
    subprocess.run([llvm_tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--input={path}", f"--output={out}",
                    f"--targets=hipv4-amdgcn-amd-amdhsa--{arch}"], check=True)
    return out


def kernel_text(elf, kernel, arch):
    """[(address, mnemonic, branch target or None)] of the kernel's instructions."""
    dis = subprocess.run([llvm_tool("llvm-objdump"), "-d", f"--mcpu={arch}", f"--disassemble-symbols={kernel}", elf],
                         check=True, capture_output=True, text=True).stdout
    ins = []
    for line in dis.splitlines():
        m = re.match(r"\s+(\w+)\b.*//\s*([0-9A-Fa-f]+):", line)
        if m:
            t = re.search(r"<[\w.$]+\+0x([0-9A-Fa-f]+)>\s*$", line)
            ins.append((int(m.group(2), 16), m.group(1), int(t.group(1), 16) if t else None))
    if not ins:
        raise SystemExit(f"no kernel {kernel} in {elf}")
    return [(a, m, None if t is None else ins[0][0] + t) for a, m, t in ins]


def classify(mnemonic):
    for name, prefixes in CLASSES:
        if mnemonic.startswith(prefixes):
            return name
    return "other"


def chain_cuts(ins, lo, hi, first_only=False):
    """Cut addresses of a chain of compare-and-branch on a scalar inside ins[lo:hi]: the forward targets of its
    branches and the instruction behind its last one.  The entry's chain is looked for behind the first broadcast of a
    lane's value (the wave index); a body that still holds two replicas starts with such a chain itself."""
    i = lo
    if not first_only:
        while i < hi and not ins[i][1].startswith("v_readfirstlane"):
            i += 1
    cuts, last, end = [], None, min(hi, i + 10)
    while i < end:
        a, m, tgt = ins[i]
        if m.startswith("s_cbranch_scc") and tgt is not None and a < tgt <= ins[hi - 1][0]:
            cuts.append(tgt)
            last, end = i, min(hi, i + 5)   # (compares, moves of the condition, the next branch)
        i += 1
    if last is None:
        return []
    return sorted(set(cuts + [ins[last + 1][0]]))


def pieces(ins):
    """The kernel's text cut at the wave-index branch chain, and again where a piece starts with a chain of its own."""
    index = {a: i for i, (a, _, _) in enumerate(ins)}
    bounds = [0] + [index[c] for c in chain_cuts(ins, 0, len(ins)) if c in index] + [len(ins)]
    k = 1
    while k < len(bounds) - 1:   # (bounds[0] .. bounds[1] is the entry)
        more = [index[c] for c in chain_cuts(ins, bounds[k], bounds[k + 1], first_only=True) if c in index]
        more = [b for b in more if b - bounds[k] > 8 and b not in bounds]   # the cut behind the chain is the piece's own start
        bounds = sorted(set(bounds + more))
        k += 1
    bounds = [b for j, b in enumerate(bounds) if j == 0 or b - bounds[j - 1] >= 8 or b == len(ins)]   # (a lone `return`)
    return [ins[a:b] for a, b in zip(bounds[:-1], bounds[1:]) if b > a]


def table(ins, extra):
    cols = [c for c, _ in CLASSES] + ["other"] + list(extra)
    head = f"{'piece':>5s} {'first':>8s} {'instrs':>7s} " + " ".join(f"{c:>9s}" for c in cols)
    rows = [head]
    for i, p in enumerate(pieces(ins)):
        n = dict.fromkeys(cols, 0)
        for _, m, _ in p:
            n[classify(m)] += 1
            for e in extra:
                n[e] += m.startswith(e)
        rows.append(f"{i:5d} {p[0][0]:8x} {len(p):7d} " + " ".join(f"{n[c]:9d}" for c in cols))
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("code_object")
    ap.add_argument("kernel")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--count", action="append", default=[], metavar="PREFIX", help="also count mnemonics that start with PREFIX")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        ins = kernel_text(bare_elf(args.code_object, args.arch, tmp), args.kernel, args.arch)
    print(f"{args.kernel} of {os.path.basename(args.code_object)}: {len(ins)} instructions")
    print(table(ins, args.count))


if __name__ == "__main__":
    sys.exit(main())
