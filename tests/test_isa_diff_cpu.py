"""tools/isa_diff.py on synthetic assembly: a renamed, moved kernel is
identical; other registers are renamed-registers; other instructions differ."""
import io
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import isa_diff  # noqa: E402

KERNEL = """\t.globl\t{name}
{name}: ; @{name}
; %bb.0:
\ts_load_dword s0, s[4:5], 0x0
\tv_add_u32_e32 {reg}, s0, v0 ; a comment
\ts_cbranch_scc1 .LBB{f}_2
.LBB{f}_2:
\t{last} {reg}, {name}@rel32@lo
\ts_endpgm
.Lfunc_end{f}:
\t.amdhsa_kernel {name}
\t\t.amdhsa_next_free_vgpr {vgprs}
\t.end_amdhsa_kernel
"""


def _verdicts(new, names=None):
    old = KERNEL.format(name="_Z1aILb1EEvv", f=0, reg="v1", last="v_mov_b32_e32", vgprs=2)
    return isa_diff.compare(old, new, names or {}, out=io.StringIO())


def test_isa_diff_verdicts():
    other = KERNEL.format(name="_Z5other", f=0, reg="v1", last="v_mov_b32_e32", vgprs=2)
    moved = other + KERNEL.format(name="_Z1aI1CEvv", f=7, reg="v1", last="v_mov_b32_e32", vgprs=2)
    assert _verdicts(moved, {"_Z1aILb1EEvv": "_Z1aI1CEvv"}) == ["identical", "unmatched (new)"]
    assert _verdicts(moved) == ["unmatched (old)", "unmatched (new)", "unmatched (new)"]
    fmt = dict(name="_Z1aILb1EEvv", f=3)
    assert _verdicts(KERNEL.format(reg="v2", last="v_mov_b32_e32", vgprs=2, **fmt)) == ["renamed-registers"]
    assert _verdicts(KERNEL.format(reg="v2", last="v_mov_b32_e32", vgprs=3, **fmt)) == ["different"]
    assert _verdicts(KERNEL.format(reg="v1", last="v_not_b32_e32", vgprs=2, **fmt)) == ["different"]
