"""CPU side of the native terrain-estimator update (include/lgestimator_train.h); names, exports, declarations and struct layouts:
tests/test_abi_units.py.  Here: the prefix, which the other trainers' headers leave alone, and the loss enum; one refused call per entry point
leaves a message that starts with that entry point's name; the Python layer's refusals (loss type with the reference's text, multi_gpu_cfg, a
bf16 encoder) need no GPU; the kernels' code-object metadata (cross-compiled for gfx950) shows no spills, no scratch, and LDS within the 80 KB
tests/test_train_abi.py allows a workgroup that shares its compute unit (none of them is a 512-lane tile kernel).  No GPU needed."""
import ctypes as C
import os
import re

import pytest

from extended_legged_gym_amd import abi
from tests.abi_checks import HIPCC, check_no_spill_no_scratch, check_refusals, header_source, kernel_metadata, library

LDS_SHARED = 80 * 1024
KERNELS = ("est_dgrad_kernel", "est_pool_backward_kernel", "est_act_delta_kernel", "est_conv_wgrad_kernel", "est_conv_retile_kernel")


def test_header_exports_and_declarations_agree():
    assert all(n.startswith("lg_estimator_train_") for n in abi.symbols("estimator_train"))
    for other in ("lgpolicy.h", "lgtrain.h", "lgdistill.h", "lgtrain_recurrent.h"):
        assert not re.search(r"lg_estimator_train_[a-z_]+\(", header_source(other)), other
    from extended_legged_gym_amd import rl
    assert hasattr(rl, "NativeEstimatorDistillation")
    assert library("estimator_train").lg_estimator_train_wgrad_slab_rows() > 0


def test_struct_layouts_match_the_c_compiler():
    """(The layouts: tests/test_abi_units.py.)  The enum whose values lg_estimator_train_hyper.loss_type takes."""
    assert re.search(r"LG_EST_LOSS_MSE = 0, LG_EST_LOSS_HUBER = 1, LG_EST_LOSS_L1 = 2", header_source("lgestimator_train.h"))
    assert abi.ESTIMATOR_LOSSES == {"mse": 0, "huber": 1, "l1": 2}


def test_one_refusal_per_entry_point_names_it():
    lib = library("policy", "estimator_train")
    p = 0x1000          # never read: the NULL handle is refused first
    hyper = abi.lg_estimator_train_hyper(0, 1.0, 0)
    calls = {
        "lg_estimator_train_create": lambda: lib.lg_estimator_train_create(None, None, None, None, None, 1e-3, 64),
        "lg_estimator_train_group": lambda: lib.lg_estimator_train_group(None, p, p, p, None, 4, 8, 0, 3, 1, C.byref(hyper), None),
        "lg_estimator_train_update": lambda: lib.lg_estimator_train_update(None, p, p, p, None, 4, 8, 1, 3, C.byref(hyper), None, None),
        "lg_estimator_train_parameter_count": lambda: lib.lg_estimator_train_parameter_count(None),
        "lg_estimator_train_workspace_bytes": lambda: lib.lg_estimator_train_workspace_bytes(None),
        "lg_estimator_train_gradients": lambda: lib.lg_estimator_train_gradients(None, p, p, p, 3, None),
        "lg_estimator_train_forward_outputs": lambda: lib.lg_estimator_train_forward_outputs(None, p, None),
        "lg_estimator_train_step_losses": lambda: lib.lg_estimator_train_step_losses(None, p, 4, None),
        "lg_estimator_train_get_carry": lambda: lib.lg_estimator_train_get_carry(None, p, p, 4, 0, None),
        "lg_estimator_train_set_carry": lambda: lib.lg_estimator_train_set_carry(None, p, p, 4, None),
        "lg_estimator_train_reset_carry": lambda: lib.lg_estimator_train_reset_carry(None, None),
        "lg_estimator_train_get_parameters": lambda: lib.lg_estimator_train_get_parameters(None, p, None),
        "lg_estimator_train_get_state": lambda: lib.lg_estimator_train_get_state(None, p, p, p, None, None, None),
        "lg_estimator_train_set_state": lambda: lib.lg_estimator_train_set_state(None, p, p, p, 0, 1e-3, None),
        "lg_estimator_train_set_learning_rate": lambda: lib.lg_estimator_train_set_learning_rate(None, 1e-3, None),
    }
    # destroy cannot fail (NULL is a no-op) and the slab size takes no argument
    check_refusals("estimator_train", lib, calls, quiet={"lg_estimator_train_destroy", "lg_estimator_train_wgrad_slab_rows"},
                   returns_handle={"lg_estimator_train_create"})
    lib.lg_estimator_train_destroy(None)


def test_python_refusals_that_need_no_gpu():
    from extended_legged_gym_amd.rl import NativeEstimatorDistillation
    with pytest.raises(ValueError, match=r"Unknown loss type: smooth\. Supported types are: mse, huber, l1"):
        NativeEstimatorDistillation(None, {}, loss_type="smooth")
    with pytest.raises(NotImplementedError, match="multi_gpu_cfg"):
        NativeEstimatorDistillation(object(), {}, multi_gpu_cfg={"global_rank": 0, "world_size": 2})

    class Bf16:
        precision = "bf16"
    with pytest.raises(NotImplementedError, match="bf16"):
        NativeEstimatorDistillation(Bf16(), {})
    with pytest.raises(TypeError, match="NativeTerrainEstimator"):
        NativeEstimatorDistillation(object(), {})


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_estimator_train_kernels_do_not_spill_and_fit_the_lds():
    blocks = kernel_metadata("lg_estimator_train.hip")
    assert len(blocks) == len(KERNELS), sorted(blocks)          # every kernel of the translation unit is held to the bounds
    check_no_spill_no_scratch(blocks, KERNELS, LDS_SHARED)
