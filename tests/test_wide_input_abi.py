"""CPU side of the wide input row (include/lgpolicy_wide.h: `lg_mlp_create_wide`, `LG_MLP_MAX_INPUT`): the header, `abi.py` and the built library agree, the
refusals name the entry point and the width that is wrong, `lg_mlp_create` keeps its own limit and message, and the wide instances of the forward,
act and training-forward kernels report no scratch, no spills and no more LDS than the narrow instances.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from extended_legged_gym_amd import abi
from tests.abi_checks import HIPCC, header_source, kernel, kernel_metadata, last_error, library

WIDE = ["lg_mlp_create_wide"]          # what include/lgpolicy_wide.h itself declares (the memory's two: tests/test_wide_recurrent_abi.py)


def _lib():
    return library("policy", "policy_wide")


def test_header_abi_and_library_agree():
    hdr, narrow_hdr = header_source("lgpolicy_wide.h"), header_source("lgpolicy.h")
    assert sorted(set(re.findall(r"\b(lg_[a-z0-9_]+)\s*\(", hdr)) - set(abi.POLICY_SYMBOLS)) == WIDE and set(WIDE) < set(abi.symbols("policy_wide"))
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
    return handle, last_error(lib)


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


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("source,kernels", [("lg_policy.hip", (("mlp_forward_kernel", "mlp_wide_forward_kernel"), ("policy_act_kernel", "policy_wide_act_kernel"),
                                                              ("distill_act_kernel", "distill_wide_act_kernel"))),
                                            ("lg_train.hip", (("ppo_forward_kernel", "ppo_wide_forward_kernel"),))])
def test_wide_instances_use_no_scratch_no_spills_and_no_more_lds(source, kernels):
    blocks = kernel_metadata(source)
    for name, wide_name in kernels:          # (the wide names do not contain the narrow ones: the existing metadata tests find a kernel by substring)
        narrow, wide = kernel(blocks, name), kernel(blocks, wide_name)
        print(name, "narrow", narrow, "wide", wide)
        for r in (narrow, wide):
            assert r["private_segment_fixed_size"] == 0 and r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0, (name, r)
        assert wide["group_segment_fixed_size"] <= narrow["group_segment_fixed_size"], (name, wide, narrow)
        assert wide["vgpr_count"] <= 256, (name, wide)          # two waves per SIMD
