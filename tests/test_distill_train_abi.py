"""CPU side of the native distillation update (include/lgdistill.h); names, exports, declarations and struct layouts: tests/test_abi_units.py.
Here: the prefix, which lgpolicy.h and lgtrain.h leave alone, and the loss enum; one refused call per entry point leaves a message that starts
with that entry point's name; the Python layer's bad-loss-type refusal carries the reference's text; the kernels' code-object metadata
(cross-compiled for gfx950) shows no spills, no scratch, and LDS within the 80 KB tests/test_train_abi.py allows a workgroup that shares its
compute unit (none of them is a 512-lane tile kernel).  No GPU needed."""
import ctypes as C
import os
import re

import pytest

from extended_legged_gym_amd import abi
from tests.abi_checks import HIPCC, check_no_spill_no_scratch, check_refusals, header_source, kernel_metadata, library

LDS_SHARED = 80 * 1024
KERNELS = ("seq_rows_kernel", "seq_loss_kernel", "seq_loss_finish_kernel", "seq_stats_kernel", "seq_mask_rows_kernel")


def test_header_exports_and_declarations_agree():
    assert all(n.startswith("lg_distill_train_") for n in abi.symbols("distill_train"))
    for other in ("lgpolicy.h", "lgtrain.h"):
        assert not re.search(r"lg_distill_train_[a-z_]+\(", header_source(other)), other
    from extended_legged_gym_amd import rl
    assert hasattr(rl, "NativeDistillation")


def test_struct_layouts_match_the_c_compiler():
    """(The layouts: tests/test_abi_units.py.)  The enum whose values lg_distill_train_hyper.loss_type takes."""
    assert re.search(r"LG_LOSS_MSE = 0, LG_LOSS_HUBER = 1", header_source("lgdistill.h")) and abi.DISTILL_LOSSES == {"mse": 0, "huber": 1}


def test_one_refusal_per_entry_point_names_it():
    lib = library("policy", "distill_train")
    p = 0x1000          # never read: the NULL handle is refused first
    hyper = abi.lg_distill_train_hyper(0, 1.0)
    calls = {
        "lg_distill_train_create": lambda: lib.lg_distill_train_create(None, None, None, 1e-3, 64),
        "lg_distill_train_group": lambda: lib.lg_distill_train_group(None, p, p, 4, 8, 0, 3, C.byref(hyper), None),
        "lg_distill_train_update": lambda: lib.lg_distill_train_update(None, p, p, 4, 8, 1, 3, C.byref(hyper), None, None),
        "lg_distill_train_parameter_count": lambda: lib.lg_distill_train_parameter_count(None),
        "lg_distill_train_gradients": lambda: lib.lg_distill_train_gradients(None, p, p, p, 3, None),
        "lg_distill_train_forward_outputs": lambda: lib.lg_distill_train_forward_outputs(None, p, None),
        "lg_distill_train_step_losses": lambda: lib.lg_distill_train_step_losses(None, p, 4, None),
        "lg_distill_train_get_parameters": lambda: lib.lg_distill_train_get_parameters(None, p, None),
        "lg_distill_train_get_state": lambda: lib.lg_distill_train_get_state(None, p, p, p, None, None, None),
        "lg_distill_train_set_state": lambda: lib.lg_distill_train_set_state(None, p, p, p, 0, 1e-3, None),
        "lg_distill_train_set_learning_rate": lambda: lib.lg_distill_train_set_learning_rate(None, 1e-3, None),
    }
    # destroy cannot fail: NULL is a no-op
    check_refusals("distill_train", lib, calls, quiet={"lg_distill_train_destroy"}, returns_handle={"lg_distill_train_create"})
    lib.lg_distill_train_destroy(None)


def test_python_refusals_that_need_no_gpu():
    from extended_legged_gym_amd.rl import NativeDistillation
    with pytest.raises(ValueError, match=r"Unknown loss type: l1\. Supported types are: mse, huber"):
        NativeDistillation(None, {}, loss_type="l1")

    class Recurrent:
        is_recurrent = True
    with pytest.raises(NotImplementedError, match="NativeStudentTeacherRecurrent"):
        NativeDistillation(Recurrent(), {})
    with pytest.raises(NotImplementedError, match="multi_gpu_cfg"):
        NativeDistillation(object(), {}, multi_gpu_cfg={"global_rank": 0, "world_size": 2})


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_distill_kernels_do_not_spill_and_fit_the_lds():
    """csrc/lg_train_sequence.hip, where the kernels of the feed-forward trainer (which has none of its own) and the shared ones of the recurrent
    student's and the estimator's live."""
    blocks = kernel_metadata("lg_train_sequence.hip")
    assert len(blocks) == len(KERNELS), sorted(blocks)          # every kernel of the translation unit is held to the bounds
    check_no_spill_no_scratch(blocks, KERNELS, LDS_SHARED)
