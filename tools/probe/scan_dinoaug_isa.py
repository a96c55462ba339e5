"""Compile-time invariants of the DINOAugment kernels (csrc/dinoaug.hip) on the gfx950 assembly hipcc generates (no GPU
needed), for all four instantiations (4-byte / 1-byte groups x blur planes in LDS / in the caller's scratch):

  1. no scratch (`.amdhsa_private_segment_fixed_size 0`, no scratch_* / buffer_* private-segment instruction);
  2. no flat_* instruction: the blur's plane pointers resolve to LDS (ds_*) or global memory at compile time;
  3. the register allocation admits the 16 waves of a 1024-thread workgroup (<= 128);
  4. the LDS instantiations read their planes with ds_read and the static LDS is the 8-byte reduction cell only, so the two
     planes (dynamic, up to 144 KB) fit the CU's 160 KB.

    python tools/probe/scan_dinoaug_isa.py        exit status 1 on a violation
"""
import atexit, os, re, shutil, subprocess, sys, tempfile

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SRC = os.path.join(REPO, "vision-transformers-pytorch_amd", "csrc", "dinoaug.hip")
sys.path.insert(0, os.path.join(REPO, "vision-transformers-pytorch_amd"))
from vtx.build import FLAGS, HIPCC   # the flags of the shipped library: a scan validates THAT binary
TMP = tempfile.mkdtemp(prefix="vtx_scan_")
atexit.register(shutil.rmtree, TMP, True)

INSTANCES = [(v, lds) for v in (4, 1) for lds in (1, 0)]


def main():
    out = os.path.join(TMP, "scan_dinoaug.s")
    r = subprocess.run([HIPCC] + FLAGS + ["-S", "--cuda-device-only", "-o", out, SRC], capture_output=True, text=True)
    if r.returncode:
        print("COMPILE FAILED:", r.stderr[-500:])
        return 1
    txt = open(out).read()
    meta = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        g = lambda k: int(re.search(k + r"\s+(\d+)", m.group(2)).group(1))
        meta[m.group(1)] = (g(r"\.amdhsa_next_free_vgpr"), g(r"\.amdhsa_private_segment_fixed_size"), g(r"\.amdhsa_group_segment_fixed_size"))
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\S*dinoaug_kernel\w+):[^\n]*\n(.*?)s_endpgm", txt, re.S | re.M)}
    bad = n = 0
    for v, lds in INSTANCES:
        pat = f"dinoaug_kernelILi{v}ELb{lds}EE"
        names = [k for k in meta if pat in k]
        if len(names) != 1 or names[0] not in bodies:
            print(f"{pat}: instantiation not found -- the scanner no longer recognises the kernel"); bad += 1
            continue
        n += 1
        vgpr, scratch, static_lds = meta[names[0]]
        alloc = (vgpr + 7) // 8 * 8
        if scratch:
            print(f"{pat}: {scratch} bytes of scratch per lane"); bad += 1
        if alloc > 128:
            print(f"{pat}: {alloc} registers allocated, 128 admit the workgroup's 16 waves"); bad += 1
        if static_lds > 16:
            print(f"{pat}: {static_lds} bytes of static LDS next to the 144 KB of planes"); bad += 1
        nds = 0
        for l in bodies[names[0]].split("\n"):
            code = l.strip().split(";")[0]
            if re.match(r"(scratch_|buffer_(load|store))", code):
                print(f"{pat}: spill / private-segment access: {code}"); bad += 1
            if code.startswith("flat_"):
                print(f"{pat}: flat access: {code}"); bad += 1
            nds += code.startswith("ds_read") or code.startswith("ds_load")
        if lds and nds == 0:
            print(f"{pat}: no LDS read in the body -- the planes are not where the scanner expects them"); bad += 1
        print(f"  {pat}: {vgpr} registers ({alloc} allocated), scratch {scratch}, static LDS {static_lds} bytes, {nds} LDS reads")
    print(f"{bad} violations in {n} DINOAugment instantiations")
    return 1 if (bad or n != len(INSTANCES)) else 0


if __name__ == "__main__":
    sys.exit(main())
