"""tools/kernel_diff.py gates kernel refactors on compiler output; a parser of it that silently matches nothing would
let every change through.  Short canned tool output, written for this test."""
from tools import kernel_diff as kd

DIS = """
a.co:\tfile format elf64-amdgpu

Disassembly of section .text:

0000000000001000 <_Z5alphaPf>:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0                         // 000000001000: C0060002 00000000
\tv_mfma_f32_16x16x32_bf16 a[0:3], v[0:3], v[4:7], a[0:3]    // 000000001008: D3B58000 04020900
\tglobal_store_dword v1, v0, s[0:1]                          // 000000001010: DC708000 00000001
\ts_endpgm                                                   // 000000001018: BF810000

0000000000001100 <_Z4betaPf>:
\tds_read_b128 v[0:3], v4                                    // 000000001100: D9FE0000 00000004
\ts_barrier                                                  // 000000001108: BF8A0000
\ts_endpgm                                                   // 00000000110C: BF810000
"""

NOTES = """
Displaying notes found in: .note
  Owner                Data size \tDescription
  AMDGPU               0x00000400\tNT_AMDGPU_METADATA (AMDGPU Metadata)
    AMDGPU Metadata:
        ---
amdhsa.kernels:
  - .agpr_count:     4
    .args:
      - .address_space:  global
        .offset:         0
        .size:           8
        .value_kind:     global_buffer
    .group_segment_fixed_size: 1088
    .name:           _Z5alphaPf
    .private_segment_fixed_size: 0
    .sgpr_count:     25
    .sgpr_spill_count: 0
    .symbol:         _Z5alphaPf.kd
    .vgpr_count:     32
    .vgpr_spill_count: 0
  - .agpr_count:     0
    .args:
      - .offset:         0
        .size:           8
        .value_kind:     global_buffer
    .group_segment_fixed_size: 0
    .name:           _Z4betaPf
    .private_segment_fixed_size: 16
    .sgpr_count:     10
    .sgpr_spill_count: 0
    .symbol:         _Z4betaPf.kd
    .vgpr_count:     8
    .vgpr_spill_count: 2
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
amdhsa.version:
  - 1
  - 2
...
"""

REMARKS = """
a.hip:3:1: remark: Function Name: _Z5alphaPf [-Rpass-analysis=kernel-resource-usage]
a.hip:3:1: remark:     VGPRs: 32 [-Rpass-analysis=kernel-resource-usage]
a.hip:3:1: remark:     Occupancy [waves/SIMD]: 8 [-Rpass-analysis=kernel-resource-usage]
a.hip:9:1: remark: Function Name: _Z4betaPf [-Rpass-analysis=kernel-resource-usage]
a.hip:9:1: remark:     Occupancy [waves/SIMD]: 5 [-Rpass-analysis=kernel-resource-usage]
"""


def test_disassembly_parser_splits_symbols_and_drops_only_the_address():
    s = kd.parse_disassembly(DIS)
    assert list(s) == ["_Z5alphaPf", "_Z4betaPf"]
    assert [len(v) for v in s.values()] == [4, 3]
    assert s["_Z5alphaPf"][1] == "v_mfma_f32_16x16x32_bf16 a[0:3], v[0:3], v[4:7], a[0:3] // D3B58000 04020900"
    moved = kd.parse_disassembly(DIS.replace("000000001", "000000007"))       # the same code at other addresses
    assert moved == s
    assert kd.parse_disassembly(DIS.replace("D3B58000", "D3B58001")) != s    # an encoding bit is not an address
    assert kd.opcode_counts(s["_Z5alphaPf"]) == {"v_mfma_f32_16x16x32_bf16": 1, "global_store_dword": 1}
    assert kd.opcode_counts(s["_Z4betaPf"]) == {"ds_read_b128": 1, "s_barrier": 1}


def test_notes_parser_reads_every_kernel_and_not_its_arguments():
    n = kd.parse_notes(NOTES)
    assert set(n) == {"_Z5alphaPf", "_Z4betaPf"}
    a, b = n["_Z5alphaPf"], n["_Z4betaPf"]
    assert (a["agpr_count"], a["vgpr_count"], a["group_segment_fixed_size"], a["sgpr_count"]) == (4, 32, 1088, 25)
    assert (b["private_segment_fixed_size"], b["vgpr_spill_count"], b["vgpr_count"]) == (16, 2, 8)
    assert "offset" not in a and "size" not in b                  # keys of the nested .args entries
    assert all(k in a and k in b for k in kd.RESOURCE_KEYS)
    assert kd.parse_occupancy(REMARKS) == {"_Z5alphaPf": 8, "_Z4betaPf": 5}


def test_verdicts():
    s, n, o = kd.parse_disassembly(DIS), kd.parse_notes(NOTES), kd.parse_occupancy(REMARKS)
    k = "_Z5alphaPf"
    base = (s[k], n[k], o[k])
    assert kd.verdict(base, base) == "identical"
    renamed = [ln.replace("v1, v0", "v0, v1").replace("DC708000", "DC708001") for ln in s[k]]
    assert kd.verdict(base, (renamed, n[k], o[k])) == "equivalent"
    assert kd.verdict(base, (renamed, dict(n[k], vgpr_count=33), o[k])) == "changed"
    assert kd.verdict(base, (renamed, n[k], 7)) == "changed"
    assert kd.verdict(base, (renamed + [renamed[2]], n[k], o[k])) == "changed"          # one global store more
    assert kd.verdict(base, (renamed + ["v_mov_b32_e32 v2, 0 // 7E040280"], n[k], o[k])) == "equivalent"


def test_rename_pairs_a_renamed_kernel_and_leaves_the_rest_alone():
    parent = {"_Z3genILi4EEvPf": 1, "_Z3genILi8EEvPf": 2, "_Z3oldILi1EEvPf": 3, "_Z4keepPf": 4, "_Z4gonePf": 5}
    cand = {"_Z3genILi1ELi4EEvPf": 1, "_Z3genILi1ELi8EEvPf": 2, "_Z4keepPf": 4, "_Z3newPf": 6}
    pairs, only_p, only_c = kd.pair_symbols(parent, cand)
    assert pairs == [("_Z4keepPf", "_Z4keepPf")] and len(only_p) == 4 and len(only_c) == 3
    # a substring of the mangled name, every occurrence in every parent symbol; renames apply in the order given
    pairs, only_p, only_c = kd.pair_symbols(parent, cand, [("genILi", "genILi1ELi"), ("3oldILi1E", "3genILi1ELi4E")])
    assert pairs == [("_Z3genILi4EEvPf", "_Z3genILi1ELi4EEvPf"), ("_Z3genILi8EEvPf", "_Z3genILi1ELi8EEvPf"),
                     ("_Z3oldILi1EEvPf", "_Z3genILi1ELi4EEvPf"), ("_Z4keepPf", "_Z4keepPf")]   # two parents, one candidate
    assert only_p == ["_Z4gonePf"] and only_c == ["_Z3newPf"]
    # a rename that produces no candidate symbol leaves the parent symbol unpaired under its own name
    # the renamed kernel's own name after a branch, and the padding behind it, are no difference
    old = DIS.replace("\ts_barrier ", "\ts_cbranch_scc0 2                 // 000000001104: BF840002 <_Z4betaPf+0x10>\n\ts_barrier ")
    new = old.replace("_Z4betaPf", "_Z4betaILi1EEPf").replace("00000000110C: BF810000", "00000000110C: BF810000\n\t...")
    so, sn = kd.parse_disassembly(old), kd.parse_disassembly(new)
    assert so["_Z4betaPf"] == sn["_Z4betaILi1EEPf"] and len(so["_Z4betaPf"]) == 4
    assert so["_Z4betaPf"][1] == "s_cbranch_scc0 2 // BF840002"
    assert kd.pair_symbols({"_Z1aPf": 1}, {"_Z1bPf": 1}, [("1a", "1c")]) == ([], ["_Z1aPf"], ["_Z1bPf"])
