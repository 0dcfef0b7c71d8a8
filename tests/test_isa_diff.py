"""tools/isa_diff.py on two tiny synthetic disassembly / metadata texts (no built library needed): label numbers
alone do not count as a difference; one changed instruction or one changed descriptor field is reported."""
import os
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_diff  # noqa: E402

ASM = """
lib.o:	file format elf64-amdgpu

Disassembly of section .text:

<kern_a>:
	s_load_dwordx2 s[0:1], s[4:5], 0x0                         // 000000001000: C0060002 00000000
	s_cbranch_scc1 L{l0}                                          // 000000001008: BF850002
	s_endpgm                                                   // 00000000100C: BF810000
<L{l0}>:
	v_mov_b32_e32 v0, {imm}                                       // 000000001010: 7E000280
	s_cbranch_execz L{l1}                                         // 000000001014: BF880001
	v_add_f64 v[2:3], v[2:3], v[2:3]                           // 000000001018: D2800002 00020502
<L{l1}>:
	s_endpgm                                                   // 000000001020: BF810000

<kern_b>:
	s_branch L{l2}                                                // 000000001100: BF820000
<L{l2}>:
	s_endpgm                                                   // 000000001104: BF810000
{pad}"""

NOTES = """
Displaying notes found in: .note
  Owner                Data size 	Description
  AMDGPU               0x00000400	NT_AMDGPU_METADATA (AMDGPU Metadata)
    AMDGPU Metadata:
---
amdhsa.kernels:
  - .agpr_count:     0
    .args:
      - .address_space:  global
        .name:           x
        .offset:         0
        .size:           8
        .value_kind:     global_buffer
    .group_segment_fixed_size: 0
    .kernarg_segment_size: 8
    .max_flat_workgroup_size: 64
    .name:           kern_a
    .private_segment_fixed_size: {scratch}
    .sgpr_count:     12
    .sgpr_spill_count: 0
    .symbol:         kern_a.kd
    .vgpr_count:     {vgpr}
    .vgpr_spill_count: 0
    .wavefront_size: 64
  - .agpr_count:     0
    .args:           []
    .group_segment_fixed_size: 128
    .kernarg_segment_size: 0
    .max_flat_workgroup_size: 256
    .name:           kern_b
    .private_segment_fixed_size: 0
    .sgpr_count:     6
    .sgpr_spill_count: 0
    .symbol:         kern_b.kd
    .vgpr_count:     1
    .vgpr_spill_count: 0
    .wavefront_size: 64
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
"""


def tables(l0=0, l1=1, l2=2, imm="0", vgpr=4, scratch=0, pad=0):
    return (isa_diff.bodies(ASM.format(l0=l0, l1=l1, l2=l2, imm=imm, pad="\ts_nop 0\n" * pad).splitlines()),
            isa_diff.descriptors(NOTES.format(vgpr=vgpr, scratch=scratch)))


def test_tables_hold_whole_bodies_and_kernel_level_fields():
    bod, des = tables()
    assert sorted(bod) == ["kern_a", "kern_b"] and sorted(des) == ["kern_a", "kern_b"]
    assert len(bod["kern_a"]) == 9 and bod["kern_a"][-1] == "s_endpgm"          # past the early s_endpgm
    assert des["kern_a"] == {".agpr_count": "0", ".group_segment_fixed_size": "0", ".kernarg_segment_size": "8",
                             ".max_flat_workgroup_size": "64", ".private_segment_fixed_size": "0", ".sgpr_count": "12",
                             ".sgpr_spill_count": "0", ".vgpr_count": "4", ".vgpr_spill_count": "0"}
    assert des["kern_b"][".group_segment_fixed_size"] == "128"


def test_shifted_label_numbers_compare_equal():
    assert isa_diff.diff(*tables(), *tables(l0=17, l1=40, l2=3)) == []


def test_end_padding_of_the_code_object_is_not_part_of_the_last_function():
    assert isa_diff.diff(*tables(), *tables(pad=5)) == []


PCREL = """
<kern_c>:
	s_getpc_b64 s[6:7]                                         // 0000002864BC: BE861C00
	s_add_u32 s6, s6, {lit}                               // {at}: 8006FF06 FFD9F680
	s_addc_u32 s7, s7, -1                                      // 0000002864C8: 8207FF07 FFFFFFFF
	s_endpgm                                                   // 0000002864D0: BF810000
"""


def test_pc_relative_address_compares_by_the_symbol_it_reaches():
    """The same table at another distance from the code is no difference; another symbol is."""
    a = isa_diff.bodies(PCREL.format(lit="0xffd9f680", at="0000002864C0").splitlines(), [(0x25b40, 64, "table"), (0x25b80, 16, "legs")])
    b = isa_diff.bodies(PCREL.format(lit="0xffd9f640", at="000000286540").splitlines(), [(0x25b80, 64, "table"), (0x25b40, 16, "legs")])
    assert a["kern_c"][1:3] == ["s_add_u32 s6, s6, <table+0>", "s_addc_u32 s7, s7, <hi>"] and a == b
    c = isa_diff.bodies(PCREL.format(lit="0xffd9f6c0", at="0000002864C0").splitlines(), [(0x25b40, 64, "table"), (0x25b80, 16, "legs")])
    assert c["kern_c"][1] == "s_add_u32 s6, s6, <legs+0>" and isa_diff.diff(a, {}, c, {}) != []
    # not the recognised form (another register pair in the high half): the raw text stays and is compared
    d = isa_diff.bodies(PCREL.replace("s_addc_u32 s7, s7", "s_addc_u32 s9, s9").format(lit="0xffd9f680", at="0000002864C0").splitlines(),
                        [(0x25b40, 64, "table")])
    assert d["kern_c"][2] == "s_addc_u32 s9, s9, -1"


def test_same_name_in_several_code_objects_is_kept_per_code_object():
    t = {}
    isa_diff.merge(t, {"helper": ["s_endpgm"], "k": ["s_nop 1"]})
    isa_diff.merge(t, {"helper": ["s_nop 2", "s_endpgm"]})
    assert t == {"helper": ["s_endpgm"], "k": ["s_nop 1"], "helper#2": ["s_nop 2", "s_endpgm"]}
    u = dict(t, helper=["s_nop 3"])
    assert len(isa_diff.diff(t, {}, u, {})) == 1


def test_changed_instruction_is_reported_with_its_line():
    rep = isa_diff.diff(*tables(), *tables(imm="1"))
    assert len(rep) == 1 and rep[0].startswith("kern_a: body differs at line 4 ") and "v_mov_b32_e32 v0, 1" in rep[0], rep
    # a branch retargeted to another block is a changed instruction too, whatever the numbers
    assert len(isa_diff.diff(*tables(), *tables(l0=1, l1=0, l2=2))) == 0
    swapped = ASM.replace("s_cbranch_execz L{l1}", "s_cbranch_execz L{l0}")
    bod = isa_diff.bodies(swapped.format(l0=0, l1=1, l2=2, imm="0", pad="").splitlines())
    rep = isa_diff.diff(bod, tables()[1], *tables())
    assert len(rep) == 1 and "kern_a: body differs at line 5 " in rep[0], rep


def test_changed_descriptor_field_and_missing_kernel_are_reported():
    assert isa_diff.diff(*tables(), *tables(vgpr=5)) == ["kern_a: .vgpr_count 4 | 5"]
    assert isa_diff.diff(*tables(), *tables(scratch=16)) == ["kern_a: .private_segment_fixed_size 0 | 16"]
    bod, des = tables()
    del bod["kern_b"], des["kern_b"]
    assert isa_diff.diff(*tables(), bod, des) == ["kern_b: only in A", "kern_b: descriptor only in A"]
