"""CPU side of the wide input row (include/lgpolicy_wide.h: `lg_mlp_create_wide`, `LG_MLP_MAX_INPUT`): the header, `abi.py` and the built library agree, the
refusals name the entry point and the width that is wrong, `lg_mlp_create` keeps its own limit and message, and the wide instances of the forward,
act and training-forward kernels report no scratch, no spills and no more LDS than the narrow instances.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from extended_legged_gym_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "extended_legged_gym_amd", "csrc")
LIB = os.path.join(CSRC, "liblgstep.so")
HIPCC = "/opt/rocm/bin/hipcc"
LLVM = "/opt/rocm/lib/llvm/bin"


def _lib():
    return abi.declare_policy_wide(abi.declare_policy(C.CDLL(LIB)))


def test_header_abi_and_library_agree():
    hdr = open(os.path.join(ROOT, "include", "lgpolicy_wide.h")).read()
    narrow_hdr = open(os.path.join(ROOT, "include", "lgpolicy.h")).read()
    assert sorted(set(re.findall(r"\b(lg_[a-z_]+)\s*\(", hdr)) - set(abi.POLICY_SYMBOLS)) == sorted(abi.POLICY_WIDE_SYMBOLS) == ["lg_mlp_create_wide"]
    assert int(re.search(r"#define\s+LG_MLP_MAX_INPUT\s+(\d+)", hdr).group(1)) == abi.MLP_MAX_INPUT == 2048
    assert abi.MLP_MAX_WIDTH == 512 and abi.MLP_MAX_INPUT % abi.MLP_MAX_WIDTH == 0
    proto = re.search(r"lg_mlp\*\s+lg_mlp_create_wide\(([^)]*)\)", hdr).group(1)
    narrow = re.search(r"lg_mlp\*\s+lg_mlp_create\(([^)]*)\)", narrow_hdr).group(1)
    assert re.sub(r"\s+", " ", proto) == re.sub(r"\s+", " ", narrow)          # the arguments of lg_mlp_create
    lib = _lib()
    assert hasattr(lib, "lg_mlp_create_wide") and lib.lg_mlp_create_wide.argtypes == lib.lg_mlp_create.argtypes
    assert lib.lg_mlp_create_wide.restype is C.c_void_p


def _create(lib, name, dims):
    fp = C.POINTER(C.c_float)
    L = len(dims) - 1
    w = np.zeros(max(1, max(dims)) ** 2, np.float32)
    ptrs = (fp * L)(*[w.ctypes.data_as(fp)] * L)
    handle = getattr(lib, name)(L, (C.c_int32 * (L + 1))(*dims), ptrs, ptrs, abi.ACTIVATIONS["elu"], 0)
    return handle, (lib.lg_mlp_last_error(None) or b"").decode()


@pytest.mark.parametrize("dims,words", [([2049, 16], ("input", "2049", "2048")), ([600, 513, 4], ("hidden", "513", "512")), ([600, 64, 513], ("output", "513", "512")),
                                        ([600, 0, 4], ("hidden", "width 0")), ([0, 4], ("input", "width 0")), ([600, 64, 0], ("output", "width 0"))])
def test_refusals_name_the_entry_point_and_the_width(dims, words):
    handle, msg = _create(_lib(), "lg_mlp_create_wide", dims)
    assert not handle and msg.startswith("lg_mlp_create_wide: "), msg
    for word in words:
        assert word in msg, (dims, msg)


def test_the_narrow_entry_point_keeps_its_limit_and_message():
    lib = _lib()
    for dims in ([513, 16], [578, 512, 18], [2048, 1]):
        handle, msg = _create(lib, "lg_mlp_create", dims)
        assert not handle and msg == "lg_mlp_create: layer width out of range (1..512)", (dims, msg)


def _metadata(tmp_path, source):
    """Metadata notes of the gfx950 code object of a csrc file, compiled with the Makefile's flags (the route of tests/test_policy_recurrent_abi.py)."""
    obj, fat, co = (str(tmp_path / (source + n)) for n in (".o", ".fat", ".co"))
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-fno-slp-vectorize", "-c", "-o", obj,
                    os.path.join(CSRC, source)], check=True, capture_output=True)
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}",
                    "--unbundle"], check=True, capture_output=True)
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    blocks, cur = {}, None
    for line in notes.splitlines():
        line = line.strip()
        if line.startswith("- .agpr_count:") or line.startswith("- .args:"):
            cur = {}
        m = re.match(r"-?\s*\.(\w+):\s+(\S+)$", line)
        if m and cur is not None:
            if m.group(1) == "name":
                blocks[m.group(2)] = cur
            elif m.group(2).isdigit():
                cur[m.group(1)] = int(m.group(2))
    return blocks


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("source,kernels", [("lg_policy.hip", (("mlp_forward_kernel", "mlp_wide_forward_kernel"), ("policy_act_kernel", "policy_wide_act_kernel"),
                                                              ("distill_act_kernel", "distill_wide_act_kernel"))),
                                            ("lg_train.hip", (("ppo_forward_kernel", "ppo_wide_forward_kernel"),))])
def test_wide_instances_use_no_scratch_no_spills_and_no_more_lds(tmp_path, source, kernels):
    blocks = _metadata(tmp_path, source)
    for kernel, wide_kernel in kernels:          # (the wide names do not contain the narrow ones: the existing metadata tests find a kernel by substring)
        narrow = [v for k, v in blocks.items() if kernel in k]
        wide = [v for k, v in blocks.items() if wide_kernel in k]
        assert len(narrow) == 1 and len(wide) == 1, (kernel, sorted(blocks))
        print(kernel, "narrow", narrow[0], "wide", wide[0])
        for r in (narrow[0], wide[0]):
            assert r["private_segment_fixed_size"] == 0 and r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0, (kernel, r)
        assert wide[0]["group_segment_fixed_size"] <= narrow[0]["group_segment_fixed_size"], (kernel, wide[0], narrow[0])
        assert wide[0]["vgpr_count"] <= 256, (kernel, wide[0])          # two waves per SIMD
