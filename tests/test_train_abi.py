"""CPU side of the native PPO update (include/lgtrain.h); names, exports, declarations and struct layouts: tests/test_abi_units.py.  Here: the
header keeps `lg_ppo_*` out of lgpolicy.h and its two enums agree with abi.py; one refused call per entry point leaves a message that starts
with that entry point's name; the kernels' code-object metadata (cross-compiled for gfx950) shows no spills, no scratch, and LDS within bounds:
the two 32-row tile kernels (512 lanes, a workgroup that owns its compute unit, 160 KB in tests/test_estimator_abi.py's words) are held to the
128 KB `mlp_forward_kernel` already lives in; every other kernel to the 80 KB that file allows a workgroup that shares its compute unit.  No
GPU needed."""
import ctypes as C
import os
import re

import pytest

from extended_legged_gym_amd import abi
from tests.abi_checks import HIPCC, check_no_spill_no_scratch, check_refusals, header_source, kernel_metadata, library

LDS_OWNER, LDS_SHARED = 128 * 1024, 80 * 1024          # the two tile kernels; everything else


def test_header_exports_and_declarations_agree():
    assert not re.search(r"lg_ppo_[a-z_]+\(", header_source("lgpolicy.h"))
    from extended_legged_gym_amd import rl
    assert hasattr(rl, "NativePPO")


def test_struct_layouts_match_the_c_compiler():
    """(The layouts: tests/test_abi_units.py.)  The two enums whose values lg_ppo_create and lg_ppo_hyper.schedule take."""
    header = header_source("lgtrain.h")
    assert re.search(r"LG_STD_SCALAR = 0, LG_STD_LOG = 1", header) and abi.NOISE_STD_TYPES == {"scalar": 0, "log": 1}
    assert re.search(r"LG_SCHEDULE_FIXED = 0, LG_SCHEDULE_ADAPTIVE = 1", header) and abi.LR_SCHEDULES == {"fixed": 0, "adaptive": 1}


def test_one_refusal_per_entry_point_names_it():
    lib = library("policy", "train")
    p = 0x1000          # never read: the NULL handle is refused first
    rows, hyper = abi.lg_ppo_rows(*[p] * 9), abi.lg_ppo_hyper(0.2, 1.0, 0.0, 1, 1.0, 0, 0.01)
    calls = {
        "lg_ppo_create": lambda: lib.lg_ppo_create(None, None, None, None, None, None, p, 0, 1e-3, 64, p),
        "lg_ppo_minibatch": lambda: lib.lg_ppo_minibatch(None, C.byref(rows), p, 8, C.byref(hyper), None),
        "lg_ppo_update": lambda: lib.lg_ppo_update(None, C.byref(rows), 8, p, 1, 1, C.byref(hyper), None, None),
        "lg_ppo_parameter_count": lambda: lib.lg_ppo_parameter_count(None),
        "lg_ppo_gradients": lambda: lib.lg_ppo_gradients(None, p, p, p, None),
        "lg_ppo_forward_outputs": lambda: lib.lg_ppo_forward_outputs(None, p, p, None),
        "lg_ppo_get_parameters": lambda: lib.lg_ppo_get_parameters(None, p, None),
        "lg_ppo_get_state": lambda: lib.lg_ppo_get_state(None, p, p, p, None, None, None),
        "lg_ppo_set_state": lambda: lib.lg_ppo_set_state(None, p, p, p, 0, 1e-3, None),
        "lg_ppo_set_learning_rate": lambda: lib.lg_ppo_set_learning_rate(None, 1e-3, None),
    }
    # the two that cannot fail: destroy (NULL is a no-op) and the slab size
    check_refusals("train", lib, calls, quiet={"lg_ppo_destroy", "lg_ppo_wgrad_slab_rows"}, returns_handle={"lg_ppo_create"})
    lib.lg_ppo_destroy(None)
    slab = lib.lg_ppo_wgrad_slab_rows()
    assert slab > 0 and slab % 4 == 0          # whole k-steps of the 16x16x4 MFMA


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_train_kernels_do_not_spill_and_fit_the_lds():
    kernels = ("ppo_forward_kernel", "ppo_loss_kernel", "ppo_loss_finish_kernel", "ppo_backward_kernel", "ppo_wgrad_kernel", "ppo_grad_reduce_kernel",
               "ppo_norm_finish_kernel", "ppo_adam_kernel", "ppo_stats_kernel")
    check_no_spill_no_scratch(kernel_metadata("lg_train.hip"), kernels,
                              lambda part: LDS_OWNER if part in ("ppo_forward_kernel", "ppo_backward_kernel") else LDS_SHARED)
