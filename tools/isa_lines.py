"""Static instruction classes of one kernel per source line (no GPU needed).

Compiles a HIP source for the device with -gline-tables-only -S (or reads an assembly file made that way), takes one
kernel by its symbol and one source line of its inline chain, and counts the kernel's instructions per source line of
the frame that line calls into. The assembly names every instruction's location as
    file:line:col @[ caller:line:col @[ ... ] ]
so with --at L an instruction counts if some frame of its chain is line L of the source, and it is attributed to the
line of the frame just inside that one (to L itself when L is the innermost frame): --at the line of k_count's
`rounds(std::true_type{}, std::true_type{})` call gives the dynamic cold round loop line by line, with everything its
lines inline (examine, adds, queue) summed into them. Without --at every instruction goes to its innermost line, or
with --outer to the outermost frame of its chain that lies in the source: the kernel body's own lines, each with all
it inlines (lambdas, helpers) summed into it, which is the account of the per-bucket code around the round loop.

Classes come from the mnemonic's leading prefix alone: v_ (valu), s_ (salu; of these s_cbranch / s_branch, s_nop and
s_waitcnt are shown apart as branch, nop, wait), ds_ (lds), global_ (vmem), anything else (other). The counts are
static: a line's instructions once each, whatever path or trip count they have at run time.

  python tools/isa_lines.py --kernel k_countILi1ELb1ELb1ELb0E --at 2880 [-DMHMKC_VERDICT=0 ...]
  python tools/isa_lines.py --asm kcount.s --kernel k_countILi1ELb1ELb1ELb0E --at 2880 --lines 2560-2760
  python tools/isa_lines.py --kernel k_countILi1ELb1ELb1ELb0E --outer      (the kernel body line by line)
  python tools/isa_lines.py --regs k_count      (NumVgprs / ScratchSize / Occupancy of every kernel whose symbol matches)
"""
from __future__ import annotations

import argparse
import re
import subprocess
import sys
import tempfile
from collections import defaultdict
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

CLASSES = ("valu", "salu", "branch", "nop", "wait", "lds", "vmem", "other")
LOC = re.compile(r"^\s*\.loc\s+\d+\s+(\d+)\s+\d+[^;]*(?:;\s*(.*))?$")
FRAME = re.compile(r"([^\s@\[\]]+):(\d+):\d+")
LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
INSN = re.compile(r"^\s+([a-z][a-z0-9_]*)\b")


def classify(mn: str) -> str:
    if mn.startswith("v_"):
        return "valu"
    if mn.startswith("s_"):
        if mn.startswith("s_cbranch") or mn.startswith("s_branch"):
            return "branch"
        if mn.startswith("s_nop"):
            return "nop"
        if mn.startswith("s_waitcnt"):
            return "wait"
        return "salu"
    if mn.startswith("ds_"):
        return "lds"
    if mn.startswith("global_"):
        return "vmem"
    return "other"


def compile_asm(src: Path, defines, out: Path) -> None:
    from mhm2_proxy_amd.build import ARCH, hipcc

    cmd = [hipcc(), f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-gline-tables-only",
           "-S", *defines, str(src), "-o", str(out)]
    print("+", " ".join(cmd), file=sys.stderr, flush=True)
    subprocess.run(cmd, check=True, cwd=ROOT)


def kernels(lines):
    """(symbol, first line, last line) of every function of the assembly: from its label to its .Lfunc_end."""
    out, cur = [], None
    for i, ln in enumerate(lines):
        mt = LABEL.match(ln)
        if mt and not mt.group(1).startswith(".") and cur is None:
            cur = (mt.group(1), i)
        elif cur and ln.startswith(".Lfunc_end"):
            out.append((cur[0], cur[1], i))
            cur = None
    return out


def chain_of(loc_match, src_name: str):
    """The frames of a .loc as (is the source file, line), innermost first."""
    line, comment = int(loc_match.group(1)), loc_match.group(2)
    if not comment:
        return [(True, line)]
    return [(f.endswith(src_name), int(l)) for f, l in FRAME.findall(comment)] or [(True, line)]


def count(lines, src_name: str, at: int | None, outer: bool = False):
    per = defaultdict(lambda: dict.fromkeys(CLASSES, 0))
    chain = []
    for ln in lines:
        mt = LOC.match(ln)
        if mt:
            chain = chain_of(mt, src_name)
            continue
        mi = INSN.match(ln)
        if not mi or ln.lstrip().startswith((".", ";")):
            continue
        if at is None:
            own = [l for s, l in chain if s]
            key = (own[-1] if outer else own[0]) if own else 0
        else:
            idx = [i for i, (s, l) in enumerate(chain) if s and l == at]
            if not idx:
                continue
            # the nearest frame inside it that lies in the source file (a frame of a header goes to its caller's line)
            key = next((l for s, l in reversed(chain[:idx[0]]) if s), at)
        per[key][classify(mi.group(1))] += 1
    return per


def regs(lines, pattern: str):
    rows, name = [], None
    for ln in lines:
        mt = LABEL.match(ln)
        if mt and not mt.group(1).startswith("."):
            name = mt.group(1)
        mr = re.match(r"^; (NumVgprs|ScratchSize|Occupancy): (\d+)", ln)
        if mr and name and pattern in name:
            if not rows or rows[-1][0] != name:
                rows.append((name, {}))
            rows[-1][1][mr.group(1)] = int(mr.group(2))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--src", default="mhm2_proxy_amd/csrc/kcount_kernels.hip")
    ap.add_argument("--asm", help="an assembly file made with -gline-tables-only -S (default: compile --src)")
    ap.add_argument("--kernel", help="the kernel's symbol, or a part of it that only one function has")
    ap.add_argument("--at", type=int, help="a source line of the kernel's inline chain")
    ap.add_argument("--outer", action="store_true", help="without --at: attribute to the outermost frame in the source")
    ap.add_argument("--lines", help="LO-HI: print these source lines only (the totals too)")
    ap.add_argument("--per", type=float, default=1.0, help="also print the totals divided by this (records per pass)")
    ap.add_argument("--regs", metavar="PATTERN", help="print NumVgprs / ScratchSize / Occupancy of matching kernels")
    args, defines = ap.parse_known_args()
    if any(not d.startswith("-D") for d in defines):
        ap.error(f"unknown arguments {defines}")
    src = ROOT / args.src
    with tempfile.TemporaryDirectory() as td:
        asm = Path(args.asm) if args.asm else Path(td) / "out.s"
        if not args.asm:
            compile_asm(src, defines, asm)
        text = asm.read_text(errors="replace").splitlines()
    if args.regs:
        for name, r in regs(text, args.regs):
            print(f"{name} vgpr={r.get('NumVgprs')} scratch={r.get('ScratchSize')} occ={r.get('Occupancy')}")
    if not args.kernel:
        return
    hits = [k for k in kernels(text) if args.kernel in k[0]]
    if len(hits) != 1:
        raise SystemExit(f"--kernel {args.kernel!r} matches {[h[0] for h in hits]}")
    name, a, b = hits[0]
    per = count(text[a:b], src.name, args.at, args.outer)
    lo, hi = (int(x) for x in args.lines.split("-")) if args.lines else (0, 1 << 30)
    print(f"# {name}" + (f", frames inside line {args.at}" if args.at else ""))
    print("line   " + " ".join(f"{c:>6}" for c in CLASSES))
    tot = dict.fromkeys(CLASSES, 0)
    for line in sorted(per):
        if lo <= line <= hi:
            print(f"{line:<6} " + " ".join(f"{per[line][c]:>6}" for c in CLASSES))
            for c in CLASSES:
                tot[c] += per[line][c]
    print("total  " + " ".join(f"{tot[c]:>6}" for c in CLASSES))
    if args.per != 1.0:
        print(f"/{args.per:<5g} " + " ".join(f"{tot[c] / args.per:>6.1f}" for c in CLASSES))


if __name__ == "__main__":
    main()
