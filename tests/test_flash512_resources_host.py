"""Register budget of flash_attn512_kernel (attention.hip), read from the compiler's own output: no GPU needed.

The kernel keeps O^T in all 256 accumulator registers, allocated by hand (named literally in asm statements), and runs one wave per SIMD; every
other value has to fit the 256 arch registers.  Two things follow, and both are checked here, for both element types:

  * it must not spill: `vgpr_spill_count 0`, `private_segment_fixed_size 0` (before the P.V phase was pipelined the kernel spilled 184 registers,
    660 bytes of scratch per lane, and the scheduler sank every V^T fragment read to its use);
  * the compiler must never touch an accumulator register itself (a spill into the accumulator half, a v_accvgpr copy): outside the kernel's asm
    statements no instruction of the kernel names one, and the descriptor allocates all 256.

attention.hip is compiled device-only to assembly with build.py's flags, once per element type, into a temporary directory; only the
flash_attn512_kernel symbol is read.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "genpercept_amd", "csrc", "attention.hip")
KERNEL = "_Z20flash_attn512_kernel"


def _hipcc():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def kernel_asm(request, tmp_path_factory):
    """(text of the kernel's code, its .amdhsa descriptor block, its metadata entry) for one element type"""
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc is not on this machine: the register budget of flash_attn512_kernel cannot be read")
    from genpercept_amd.build import FLAGS
    out = tmp_path_factory.mktemp("flash512_" + request.param) / "attention.s"
    defs = ["-DGP_F16=1"] if request.param == "fp16" else []
    r = subprocess.run([hipcc, *FLAGS, *defs, "--cuda-device-only", "-S", SRC, "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = out.read_text().splitlines()
    start = next(i for i, ln in enumerate(lines) if re.match(KERNEL + r"\w*:", ln))
    desc0 = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".amdhsa_kernel " + KERNEL))
    desc1 = next(i for i in range(desc0, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
    # the metadata holds one entry per kernel, `.key: value` lines, each entry opening with `- .agpr_count:`
    name = next(i for i, ln in enumerate(lines) if re.match(r"\s*\.name:\s+" + KERNEL, ln))
    m0 = max(i for i in range(name) if lines[i].lstrip().startswith("- .agpr_count:"))
    m1 = next((i for i in range(name, len(lines)) if lines[i].lstrip().startswith("- .agpr_count:")), len(lines))
    meta = dict(m.groups() for m in (re.match(r"  [ -] \.(\w+):\s+(\S+)\s*$", ln) for ln in lines[m0:m1]) if m)
    return lines[start:desc0], lines[desc0:desc1], meta


def test_flash512_does_not_spill(kernel_asm):
    code, desc, meta = kernel_asm
    assert int(meta["vgpr_spill_count"]) == 0, meta
    assert int(meta["private_segment_fixed_size"]) == 0, meta
    d = dict(ln.split()[:2] for ln in desc if ln.strip().startswith(".amdhsa_") and len(ln.split()) >= 2)
    assert int(d[".amdhsa_private_segment_fixed_size"]) == 0
    assert not [ln for ln in code if re.match(r"\s*scratch_", ln)], "scratch access in flash_attn512_kernel"


def test_flash512_accumulators_are_the_kernels_own(kernel_asm):
    code, desc, meta = kernel_asm
    assert int(meta["agpr_count"]) == 256, meta
    inside, foreign, own_mfma = False, [], 0
    for ln in code:
        s = ln.strip()
        if s.startswith(";;#ASMSTART"):
            inside = True
        elif s.startswith(";;#ASMEND"):
            inside = False
        elif s and not s.startswith(";") and not s.startswith("."):
            touches = re.search(r"(^v_accvgpr)|([\s,]a\[?\d)", s) is not None
            if inside:
                own_mfma += s.startswith("v_mfma") and " a[" in s
            elif touches:
                foreign.append(s)
    assert not foreign, f"compiler-generated accumulator accesses: {foreign[:5]}"
    assert own_mfma >= 32, own_mfma   # (the P.V phase: 32 per copy of the tile body)
