"""CPU: tools/isa_diff.py on two made-up listings -- comments and label numbers
do not count, an operand does."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "k-hip-amdgcn-amd-amdhsa-gfx950.s"
LISTING = """\t.type\t_Z1kPm,@function
_Z1kPm:                                 ; @_Z1kPm
; %bb.0:
\ts_cbranch_scc1 .LBB{f}_{l}
\tv_add_u32_e32 v0, {op}, v0 ; {note}
.LBB{f}_{l}:
\ts_endpgm
\t.amdhsa_kernel _Z1kPm
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_private_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr 4
\t\t.amdhsa_next_free_sgpr 8
\t.end_amdhsa_kernel
.Lfunc_end{f}:
; Occupancy: 8
"""


def run(tmp_path, **new):
    for d, kw in (("old", dict(f=0, l=2, op="v1", note="first")), ("new", new)):
        os.makedirs(tmp_path / d)
        (tmp_path / d / NAME).write_text(LISTING.format(**kw))
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_diff.py"), str(tmp_path / "old"),
                           str(tmp_path / "new")], capture_output=True, text=True)


def test_comments_and_labels_do_not_count(tmp_path):
    p = run(tmp_path, f=3, l=7, op="v1", note="second  ")
    assert p.returncode == 0, p.stdout + p.stderr
    assert "k _Z1kPm same | 4 8 0 0 8" in p.stdout


def test_an_operand_counts(tmp_path):
    p = run(tmp_path, f=0, l=2, op="v2", note="first")
    assert p.returncode != 0
    assert "k _Z1kPm DIFF (2 lines)" in p.stdout
