"""Register / LDS budget of the kernel the headline number runs, from the compiler's own report: the metadata of the code object `build()` left in csrc/ when it is
current, else `-Rpass-analysis=kernel-resource-usage` of a device compilation of csrc/lg_step.hip (four minutes); no GPU needed.  Round 2's build of `physics_kernel<0, false>` spilled 1 157 SGPRs and 79 VGPRs,
nearly all of it in the single-wave fallback paths inlined next to the hot code; they are a separate template instance now
(`physics_kernel<0, TMESH, HELPERS>`), and this test keeps it that way."""
import os
import re
import subprocess

import pytest

from tests.abi_checks import CSRC, HIPCC, LLVM, ROOT, object_metadata


def _from_built_object(obj):
    """Kernel resources from the code object inside an object file `build()` left in csrc/ -- when it is at least as new as every source it was compiled from.
    The same numbers the compiler reports (the metadata notes of the code object), without the four minutes of compiling the file again.  None: no such object."""
    if not (os.path.exists(obj) and os.path.exists(os.path.join(LLVM, "clang-offload-bundler"))):
        return None
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h") or f == "lg_step.hip"] + [os.path.join(ROOT, "include", "lgstep.h")]      # (what lg_step.hip includes)
    if os.path.getmtime(obj) < max(os.path.getmtime(f) for f in srcs):
        return None
    try:
        blocks = object_metadata(obj)
    except (subprocess.CalledProcessError, OSError):
        return None
    out = {}
    for name, r in blocks.items():
        if "vgpr_count" in r:
            out[name] = {"VGPRs": r["vgpr_count"] - r.get("agpr_count", 0), "AGPRs": r.get("agpr_count", 0), "VGPRs Spill": r.get("vgpr_spill_count", 0),
                         "SGPRs Spill": r.get("sgpr_spill_count", 0), "ScratchSize": r.get("private_segment_fixed_size", 0), "LDS Size": r.get("group_segment_fixed_size", 0),
                         "Occupancy": 1 if r["vgpr_count"] > 256 else 2}
    return out or None


def _resources(tmp_path, legs):
    built = _from_built_object(os.path.join(CSRC, f"lg_step{legs}.o"))
    if built is not None:
        return built
    src = os.path.join(CSRC, "lg_step.hip")
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "-fno-slp-vectorize", "--cuda-device-only", f"-DLG_LEGS={legs}",
           "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / f"lg_step{legs}.o")]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    blocks, name = {}, None
    for line in out.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1); blocks[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/(?:lane|block)\])?(?: \[waves/SIMD\])?: (\d+)", line)
        if m and name:
            blocks[name][m.group(1).strip()] = int(m.group(2))
    return blocks


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_headline_kernel_register_and_lds_budget(tmp_path):
    blocks = _resources(tmp_path, 4)
    # physics_kernel<0, false, true>: heightfield / plane terrain, helper waves present = every policy step of the headline config
    # (lg_step.hip is compiled once per leg count, lg_instance.h; without -DLG_LEGS this is the four-legged instance, namespace lg4)
    key = [k for k in blocks if k.startswith("_ZN3lg414physics_kernelILi0ELb0ELb1ELi0E")]
    assert len(key) == 1, sorted(blocks)
    r = blocks[key[0]]
    print(r)
    assert r["VGPRs Spill"] == 0, r
    # round 2: 1 157.  What is left (~160) is written once per launch in the wave prologues (terrain view, solver parameters, actuator scales:
    # scalars the helper waves use in every substep next to the SGPR-resident LSTM weights) and read back where used; none of it is inside the
    # Gauss-Seidel passes.  The tail reads the context through `late_ctx`, so its ~40 row pointers are no longer among them.
    assert r["SGPRs Spill"] <= 200, r
    assert r["ScratchSize"] <= 64, r
    assert r["VGPRs"] + r["AGPRs"] <= 512 and r["Occupancy"] == 1, r     # one wave per SIMD by design (s5): the budget of a lone wave
    assert r["LDS Size"] <= 160 * 1024, r
    # the triangle-mesh instance: also without the fallback
    key = [k for k in blocks if k.startswith("_ZN3lg414physics_kernelILi0ELb1ELb1ELi0E")]
    assert len(key) == 1 and blocks[key[0]]["SGPRs Spill"] <= 400 and blocks[key[0]]["LDS Size"] <= 160 * 1024, blocks[key[0]]
    # ... and without vector spills: the lattice contact queries (closest_point_lattice_pair) with sixteen cell records in registers spilled 57 VGPRs and
    # 240 B of scratch per lane into every phase of this instance (round 5); eight records fit
    assert blocks[key[0]]["VGPRs Spill"] == 0 and blocks[key[0]]["ScratchSize"] <= 64, blocks[key[0]]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_six_legged_instance_fits_a_compute_unit(tmp_path):
    """The hexapod instance (-DLG_LEGS=6: eight lanes per env) of the same source: no vector spills, one workgroup's LDS."""
    blocks = _resources(tmp_path, 6)
    key = [k for k in blocks if k.startswith("_ZN3lg614physics_kernelILi0ELb0ELb1ELi0E")]
    assert len(key) == 1, sorted(blocks)
    r = blocks[key[0]]
    print(r)
    assert r["VGPRs Spill"] == 0 and r["ScratchSize"] <= 64 and r["LDS Size"] <= 160 * 1024, r
