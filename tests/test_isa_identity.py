"""tools/isa_identity.py's normaliser on hand-written kernels (no compiler runs): what a renaming of a kernel changes -- label
numbers, comments, its own symbol -- compares equal; an operand or a register figure of the kernel descriptor does not."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import isa_identity  # noqa: E402

KERNEL = """%(sym)s: ; @%(sym)s
; %%bb.0:
\ts_load_dword s3, s[0:1], 0x110
\ts_cbranch_scc1 .LBB%(fn)d_2
; %%bb.1:                                ; %(note)s
\tv_add_f64 v[0:1], v[2:3], %(operand)s
.LBB%(fn)d_2:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel %(sym)s
\t\t.amdhsa_group_segment_fixed_size 13536
\t\t.amdhsa_next_free_vgpr %(vgpr)d
\t.end_amdhsa_kernel
"""
META = """\t.amdgpu_metadata
---
amdhsa.kernels:
  - .agpr_count:     0
    .group_segment_fixed_size: 13536
    .name:           %(sym)s
    .private_segment_fixed_size: 0
    .sgpr_spill_count: 0
    .vgpr_count:     %(vgpr)d
    .vgpr_spill_count: 0
...
\t.end_amdgpu_metadata
"""
OLD = dict(sym="_ZN3ccv1kILb1ELb1EEEvv", fn=3, note="in Loop: Header=BB3_1", operand="v[4:5]", vgpr=128)
RENAMED = dict(OLD, sym="_ZN3ccv1kILNS_9BatchFormE2EEEvv", fn=0, note="=>This Inner Loop Header")


def fingerprint(fields):
    (name, fp), = isa_identity.fingerprints((KERNEL + META) % fields)
    assert name == fields["sym"]
    return fp


def test_a_renamed_kernel_compares_equal():
    assert fingerprint(OLD) == fingerprint(RENAMED)
    assert isa_identity.unpaired([("a", fingerprint(OLD))], [("b", fingerprint(RENAMED))]) == ([], [])
    text = fingerprint(OLD)[0]
    assert "v_add_f64 v[0:1], v[2:3], v[4:5]" in text and ".amdhsa_next_free_vgpr 128" in text and ".p2align" not in text


def test_a_changed_operand_compares_unequal():
    changed = fingerprint(dict(RENAMED, operand="v[6:7]"))
    assert fingerprint(OLD) != changed
    assert isa_identity.unpaired([("a", fingerprint(OLD))], [("b", changed)]) == (["a"], ["b"])


def test_a_changed_next_free_vgpr_compares_unequal():
    assert fingerprint(OLD)[0] != fingerprint(dict(RENAMED, vgpr=132))[0]
    assert fingerprint(OLD) != fingerprint(dict(RENAMED, vgpr=132))
