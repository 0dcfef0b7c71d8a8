#!/usr/bin/env python3
"""Static report of the LDS waits in the compiled solve kernels (CPU only, no GPU).

Compiles srb-cbf-nmpc_amd/csrc/srb_kernels.hip for a list of instances with the product flags to
gfx950 assembly (device only, as `make dev` does with SRB_DEV_INSTANCES) and prints, per kernel and per
loop nest of the kernel:

  waits     s_waitcnt instructions that name the LDS counter (lgkmcnt)
  exposed   those that come within three instructions of an LDS read (ds_read*): nothing to hide the
            round trip behind
  stall     cycles a straight-line model spends in those waits
  issue     cycles the same model spends issuing

The model walks the instructions in program order, once each (no trip counts, no branches): every
instruction issues in 4 cycles (an fp64 MFMA in 32, s_nop n in n + 1), an LDS or scalar-memory operation
returns LATENCY cycles after it issued, in order, and `s_waitcnt lgkmcnt(k)` stalls until all but the k
latest have returned.  It looks only at LDS reads, waits and issue order: a guide to where round trips are
exposed, not a cycle count of the kernel.

A loop nest is a loop that has child loops (the compiler's "Loop Header" comments); its region runs from
its header to the next loop header of the same or a smaller depth.  In the solve kernel the depth-2 nest
inside the first depth-1 nest is the interior-point iteration loop and the last depth-1 nest the fused polish.

  --lines   adds -gline-tables-only and splits the same figures by source line (of the innermost inlined
            function) over the whole kernel, worst first

usage: tools/lds_wait_report.py [--lines] [--latency 64] [--asm FILE] ['X(12,4,1,10,2,11)' ...]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "srb-cbf-nmpc_amd")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "-std=c++17", "-fPIC"]

LGKM = re.compile(r"lgkmcnt\((\d+)\)")
LOOP = re.compile(r"^\.LBB(\d+_\d+):\s*;.*?(=>)?\s*This (Inner )?Loop Header: Depth=(\d+)")
LOOP2 = re.compile(r"^\s*;\s*=>\s*This (Inner )?Loop Header: Depth=(\d+)")
LABEL = re.compile(r"^\.LBB(\d+_\d+):")


def compile_asm(instances, lines, out):
    cmd = [HIPCC] + FLAGS + ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(SRC, "csrc"),
                             "-DSRB_DEV_INSTANCES(X)=" + " ".join(instances), "--cuda-device-only", "-S",
                             os.path.join(SRC, "csrc", "srb_kernels.hip"), "-o", out]
    if lines:
        cmd.insert(1, "-gline-tables-only")
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)


class Acc:
    __slots__ = ("waits", "exposed", "stall", "issue")

    def __init__(self):
        self.waits = self.exposed = self.stall = self.issue = 0


def issue_cycles(op, args):
    if op.startswith("v_mfma_f64"):
        return 32
    if op == "s_nop":
        try:
            return int(args.strip(), 0) + 1
        except ValueError:
            return 1
    return 4


def kernels(text):
    """(name, [lines]) of every solve / polish kernel in the assembly"""
    out, name, body = [], None, []
    for ln in text.splitlines():
        m = re.match(r"^(srb_(?:nmpc|polish)_kernel_\w+):", ln)
        if m:
            name, body = m.group(1), []
            continue
        if name:
            if ln.startswith(".Lfunc_end"):
                out.append((name, body))
                name = None
            else:
                body.append(ln)
    return out


def analyse(body, latency):
    """walk one kernel: totals, per loop nest, per source line"""
    total = Acc()
    nests = []                       # [label, depth, Acc], in program order
    open_nests = []                  # indices into nests whose region is open
    by_line = defaultdict(Acc)
    files = {}
    cur_line = "?"
    now = 0
    pending = []                     # return times of outstanding lgkm operations, issue order
    recent = []                      # the last three instructions: is it an LDS read
    header = None
    i = 0
    while i < len(body):
        ln = body[i]
        i += 1
        s = ln.strip()
        if not s:
            continue
        m = LABEL.match(ln)
        if m:
            header = m.group(1)
            depth, inner = None, True
            mm = LOOP.match(ln)
            if mm:
                depth, inner = int(mm.group(4)), bool(mm.group(3))
            else:                    # the "This Loop Header" comment may sit on a following comment line
                j = i
                while j < len(body) and body[j].lstrip().startswith(";"):
                    m2 = LOOP2.match(body[j])
                    if m2:
                        depth, inner = int(m2.group(2)), bool(m2.group(1))
                        break
                    j += 1
            if depth is not None:
                open_nests = [k for k in open_nests if nests[k][1] < depth]
                if not inner:
                    nests.append(["BB" + header, depth, Acc()])
                    open_nests.append(len(nests) - 1)
            continue
        if s.startswith(".file"):
            p = s.split(None, 2)                      # .file N "dir" "name" [md5 ..]
            names = re.findall(r'"([^"]*)"', s)
            if len(p) == 3 and p[1].isdigit() and names:
                files[p[1]] = os.path.basename(names[-1])
            continue
        if s.startswith(".loc"):
            p = s.split()
            cur_line = "%s:%s" % (files.get(p[1], p[1]), p[2])
            continue
        if s[0] in ".;" or s.endswith(":"):
            continue
        code = s.split(";", 1)[0].strip()
        if not code:
            continue
        op, _, args = code.partition(" ")
        accs = [total, by_line[cur_line]] + [nests[k][2] for k in open_nests]
        c = issue_cycles(op, args)
        now += c
        for a in accs:
            a.issue += c
        is_read = op.startswith("ds_read") or op.startswith("ds_load")
        if op.startswith("ds_") or op.startswith("s_load") or op.startswith("s_buffer_load"):
            pending.append(now + latency)
        if op == "s_waitcnt":
            m = LGKM.search(args)
            if m:
                keep = int(m.group(1))
                done = pending[:len(pending) - keep] if keep else pending
                st = max(0, max(done) - now) if done else 0
                pending = pending[len(pending) - keep:] if keep else []
                now += st
                exp = any(recent[-3:])
                for a in accs:
                    a.waits += 1
                    a.exposed += exp
                    a.stall += st
        recent.append(is_read)
        if len(recent) > 3:
            recent.pop(0)
    return total, nests, by_line


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("instances", nargs="*", default=["X(12,4,1,10,2,11)"])
    ap.add_argument("--lines", action="store_true")
    ap.add_argument("--latency", type=int, default=64)
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("--top", type=int, default=25, help="source lines shown with --lines")
    a = ap.parse_args()
    if a.asm:
        text = open(a.asm).read()
    else:
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "k.s")
            compile_asm(a.instances, a.lines, out)
            text = open(out).read()
    fmt = "%-44s %6s %8s %8s %8s"
    for name, body in kernels(text):
        total, nests, by_line = analyse(body, a.latency)
        print(name)
        print(fmt % ("  region", "waits", "exposed", "stall", "issue"))
        print(fmt % ("  whole kernel", total.waits, total.exposed, total.stall, total.issue))
        for label, depth, acc in nests:
            print(fmt % ("  " + "  " * depth + "nest %s (depth %d)" % (label, depth), acc.waits, acc.exposed, acc.stall, acc.issue))
        if a.lines:
            rows = sorted(by_line.items(), key=lambda kv: -kv[1].stall)[:a.top]
            for line, acc in rows:
                if acc.waits:
                    print(fmt % ("    " + line, acc.waits, acc.exposed, acc.stall, acc.issue))
        print()
    return 0


if __name__ == "__main__":
    sys.exit(main())
