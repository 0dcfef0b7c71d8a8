"""Per-kernel machine-code diff of two builds of the library: the acceptance check of a refactor that is to
change no generated code.

    python tools/isa_diff.py A.so B.so          exit status 0 only if nothing differs

For every gfx950 code object the two libraries carry (tools/codeobj.py): the disassembly of each function, with
the branch labels renumbered per function in order of first appearance (llvm-objdump --symbolize-operands numbers
them per code object, so a kernel that moves to another translation unit differs in label numbers only), and the
kernel descriptor fields of `llvm-readelf --notes`.  Reported: names present in one library only, bodies that
differ (with the first differing line), descriptor fields that differ.

Two things that depend on where the linker put a function, not on its code, are normalised: trailing s_nop padding
is dropped (the assembler pads the end of a code object, so the function that happens to be last carries it), and
the literal of a pc-relative address (s_getpc_b64; s_add_u32 lo, lo, <literal>; s_addc_u32 hi, hi, <0 or -1>) is
replaced by the symbol it resolves to, `<name+offset>`.  Only the compiler's usual form is recognised, the three
instructions adjacent and on one register pair; anything else keeps its raw literal, which can report a difference
that is only one of layout but never hides one.  A function name that several code objects carry (a helper that
was not inlined) is kept once per code object, as `name#2`, `name#3`, .. in code-object order, so no copy goes
uncompared.  The bodies are split at the symbol labels
(isa_exec_hazard.normalize's form); isa_exec_hazard.kernels itself ends a body at its first s_endpgm, which would
hide a change behind an early exit.
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import codeobj  # noqa: E402
import isa_exec_hazard as hz  # noqa: E402

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".sgpr_spill_count", ".vgpr_spill_count",
          ".group_segment_fixed_size", ".private_segment_fixed_size", ".kernarg_segment_size",
          ".max_flat_workgroup_size")
LABEL = re.compile(r"\.LBBL\d+\b")


ADDR = re.compile(r"//\s*([0-9A-Fa-f]+):")
GETPC = re.compile(r"^s_getpc_b64 s\[(\d+):")
PCADD = re.compile(r"^(s_add_u32 s(\d+), s(\d+), )(0x[0-9a-fA-F]+|-?\d+)$")


def pcrel(body, ln, addr, symbols):
    """`ln` with the literal of a pc-relative address (see the module docstring) replaced by symbol+offset."""
    m = PCADD.match(ln)
    g = GETPC.match(body[-1]) if m and body else None
    if g and addr is not None and m.group(2) == m.group(3) == g.group(1):
        lit = int(m.group(4), 0) & 0xffffffff
        target = addr + lit - (1 << 32 if lit >> 31 else 0)
        for a, size, name in symbols:
            if a <= target < a + max(size, 1):
                return f"{m.group(1)}<{name}+{target - a}>"
    g = GETPC.match(body[-2]) if len(body) > 1 else None     # the high half, behind a low half rewritten just above
    if g and body[-1].startswith(f"s_add_u32 s{g.group(1)}, ") and body[-1].endswith(">"):
        hi = int(g.group(1)) + 1
        if re.match(rf"^s_addc_u32 s{hi}, s{hi}, (0|-1)$", ln):
            return ln.rsplit(",", 1)[0] + ", <hi>"
    return ln


def bodies(lines, symbols=()):
    """{function name: body lines} of one disassembly text, labels renumbered per function; symbols:
    (address, size, name) of the code object's data and function symbols, for the pc-relative addresses."""
    out, name, body = {}, None, []
    for ln in lines:
        a = ADDR.search(ln)
        ln = hz.normalize(ln.rstrip("\n"))
        m = re.match(r"^([A-Za-z_][\w.]*):\s*$", ln)
        if m and not m.group(1).startswith(".L"):
            if name is not None:
                out[name] = renumber(body)
            name, body = m.group(1), []
        elif name is not None and ln.strip():
            body.append(pcrel(body, ln.strip(), int(a.group(1), 16) if a else None, symbols))
    if name is not None:
        out[name] = renumber(body)
    return out


def renumber(body):
    while body and body[-1].startswith("s_nop"):       # the code object's end padding, behind whichever function is last
        body = body[:-1]
    ids = {}
    return [LABEL.sub(lambda m: ids.setdefault(m.group(0), f".L{len(ids)}"), ln) for ln in body]


def descriptors(notes):
    """{kernel name: {field: value}} from the amdhsa.kernels metadata of `llvm-readelf --notes` output."""
    out, cur = {}, None
    for ln in notes.splitlines():
        m = re.match(r"^(  - | {4})(\.\w+):\s*(.*?)\s*$", ln)      # kernel-level keys only (argument keys sit deeper)
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
        if cur is None:
            continue
        if m.group(2) == ".name":
            out[m.group(3).strip("'\"")] = cur
        elif m.group(2) in FIELDS:
            cur[m.group(2)] = m.group(3)
    return out


def diff(bod_a, des_a, bod_b, des_b):
    """Report lines for two (bodies, descriptors) tables; empty when nothing differs."""
    rep = []
    for n in sorted(set(bod_a) ^ set(bod_b)):
        rep.append(f"{n}: only in {'A' if n in bod_a else 'B'}")
    for n in sorted(set(bod_a) & set(bod_b)):
        a, b = bod_a[n], bod_b[n]
        if a != b:
            k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            rep.append(f"{n}: body differs at line {k} ({len(a)} / {len(b)} lines): "
                       f"{a[k] if k < len(a) else '<end>'!r} | {b[k] if k < len(b) else '<end>'!r}")
    for n in sorted(set(des_a) ^ set(des_b)):
        rep.append(f"{n}: descriptor only in {'A' if n in des_a else 'B'}")
    for n in sorted(set(des_a) & set(des_b)):
        for f in FIELDS:
            if des_a[n].get(f) != des_b[n].get(f):
                rep.append(f"{n}: {f} {des_a[n].get(f)} | {des_b[n].get(f)}")
    return rep


def merge(table, new):
    """Add one code object's entries; a name already there gets the next free `name#k`."""
    for name, v in new.items():
        k, key = 1, name
        while key in table:
            k += 1
            key = f"{name}#{k}"
        table[key] = v


def load(lib, tmp):
    """(bodies, descriptors) over every gfx950 code object of a library."""
    bod, des = {}, {}
    for s in codeobj.disassemble(lib, tmp):
        table = subprocess.run([codeobj.OBJDUMP, "-t", s[:-2] + ".o"], capture_output=True, text=True, check=True).stdout
        syms = [(int(m.group(1), 16), int(m.group(2), 16), m.group(3)) for m in
                re.finditer(r"^([0-9a-f]{16}) \S+\s+[OF] \S+\s+([0-9a-f]{16}) (?:\.\w+ )?(\S+)$", table, re.M)]
        with open(s) as f:
            merge(bod, bodies(f, syms))
        notes = subprocess.run([READELF, "--notes", s[:-2] + ".o"], capture_output=True, text=True, check=True).stdout
        merge(des, descriptors(notes))
    return bod, des


def main():
    a, b = sys.argv[1:3]
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        (ba, da), (bb, db) = load(a, ta), load(b, tb)
    rep = diff(ba, da, bb, db)
    for r in rep:
        print(r)
    print(f"{len(da)} / {len(db)} kernels, {len(ba)} / {len(bb)} functions, {len(rep)} differences")
    return 1 if rep else 0


if __name__ == "__main__":
    sys.exit(main())
