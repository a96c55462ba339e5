"""Compile-time budget of the window / halo instantiations of the any-head-width attention kernels (csrc/attention_hd.hip, WX = true,
behind vtx_attn_hdw_*) on the gfx950 assembly hipcc generates (no GPU needed): forward, dQ, dK / dV and the bias-gradient kernel, for
bf16 and fp32 at the padded widths 32 | 64 | 96 | 128 -- 32 kernels.

  1. no scratch: `.amdhsa_private_segment_fixed_size 0`;
  2. the register count and the static LDS are printed per instantiation (DESIGN.md section 7f quotes these numbers); no bound is
     asserted on them.

It looks at the kernel descriptors only (scratch size, register count, LDS size), not at instructions.

    python tools/probe/scan_attn_hdw_isa.py        exit status 1 on a violation
"""
import atexit, os, re, shutil, subprocess, sys, tempfile

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SRC = os.path.join(REPO, "vision-transformers-pytorch_amd", "csrc", "attention_hd.hip")
sys.path.insert(0, os.path.join(REPO, "vision-transformers-pytorch_amd"))
from vtx.build import FLAGS, HIPCC   # the flags of the shipped library: a scan validates THAT binary
TMP = tempfile.mkdtemp(prefix="vtx_scan_")
atexit.register(shutil.rmtree, TMP, True)

TYPES = (("bf16", "DF16b"), ("fp32", "f"))
PADS = (32, 64, 96, 128)
# (label, mangled kernel name, template tail after <T, DP>)
KERNELS = (("fwd", "hdattn_fwd_kernel", "Lb1E"), ("dq", "hdattn_bwd_dq_kernel", "Lb1E"), ("dkv", "hdattn_bwd_dkv_kernel", "Lb1E"),
           ("dbias", "hdattn_bwd_dbias_kernel", ""))


def descriptors():
    out = os.path.join(TMP, "scan_attn_hd.s")
    r = subprocess.run([HIPCC] + FLAGS + ["-S", "--cuda-device-only", "-o", out, SRC], capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError("COMPILE FAILED: " + r.stderr[-800:])
    meta = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", open(out).read(), re.S):
        g = lambda k: int(re.search(k + r"\s+(\d+)", m.group(2)).group(1))
        meta[m.group(1)] = dict(vgpr=g(r"\.amdhsa_next_free_vgpr"), scratch=g(r"\.amdhsa_private_segment_fixed_size"),
                                lds=g(r"\.amdhsa_group_segment_fixed_size"))
    return meta


def instances(meta):
    """-> {(kernel label, type label, DP): descriptor} of the WX instantiations that were found"""
    found = {}
    for label, name, tail in KERNELS:
        for tl, tm in TYPES:
            for dp in PADS:
                pat = f"{name}I{tm}Li{dp}E{tail}E"
                names = [k for k in meta if pat in k]
                if len(names) == 1:
                    found[(label, tl, dp)] = meta[names[0]]
    return found


def main():
    try:
        found = instances(descriptors())
    except RuntimeError as e:
        print(e)
        return 1
    bad = 0
    for label, _, _ in KERNELS:
        for tl, _ in TYPES:
            for dp in PADS:
                d = found.get((label, tl, dp))
                if d is None:
                    print(f"{label} {tl} DP{dp}: instantiation not found -- the scanner no longer recognises the kernel"); bad += 1
                    continue
                if d["scratch"]:
                    print(f"{label} {tl} DP{dp}: {d['scratch']} bytes of scratch per lane"); bad += 1
                print(f"  {label:5s} {tl} DP{dp:<3d}: {d['vgpr']:3d} registers, scratch {d['scratch']}, static LDS {d['lds']} bytes")
    print(f"{bad} violations in {len(found)} of {len(KERNELS) * len(TYPES) * len(PADS)} window / halo attention instantiations")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
