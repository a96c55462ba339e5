"""CPU: the window / halo instantiations of csrc/attention_hd.hip (WX = true: forward, dQ, dK / dV, and the bias-gradient kernel; bf16 and
fp32 at the padded widths 32 | 64 | 96 | 128) assemble for gfx950 without scratch -- tools/probe/scan_attn_hdw_isa.py reads the private
segment size and the register count of every kernel descriptor (nothing else)."""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_instantiations_have_no_scratch():
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "probe", "scan_attn_hdw_isa.py")], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 violations in 32 of 32" in r.stdout, r.stdout
