"""CPU side of the recurrent student's native distillation update (include/lgdistill_recurrent.h); names, exports, declarations and struct
layouts: tests/test_abi_units.py.  Here: the prefix, which the other trainers' headers leave alone, and the stats fields; one refused call per
entry point leaves a message that starts with that entry point's name; the Python layer's refusals (loss type with the reference's text,
multi_gpu_cfg, a policy that is not a `NativeStudentTeacherRecurrent`) need no GPU, and `NativeDistillation` keeps refusing a recurrent policy;
the kernels' code-object metadata (cross-compiled for gfx950) shows no spills, no scratch, and LDS within the 80 KB tests/test_train_abi.py
allows a workgroup that shares its compute unit (none of them is a 512-lane tile kernel).  No GPU needed."""
import ctypes as C
import os
import re

import pytest

from extended_legged_gym_amd import abi
from tests.abi_checks import HIPCC, check_no_spill_no_scratch, check_refusals, header_source, kernel_metadata, library

LDS_SHARED = 80 * 1024
KERNELS = ("rdistill_norm_kernel", "rdistill_adam_kernel")


def test_header_exports_and_declarations_agree():
    assert all(n.startswith("lg_distill_rtrain_") for n in abi.symbols("distill_rtrain"))
    for other in ("lgpolicy.h", "lgtrain.h", "lgdistill.h", "lgtrain_recurrent.h", "lgestimator_train.h"):
        assert not re.search(r"lg_distill_rtrain_[a-z_]+\(", header_source(other)), other
    assert "lgdistill_recurrent.h" in header_source("lgdistill.h")
    from extended_legged_gym_amd import rl
    assert hasattr(rl, "NativeRecurrentDistillation")


def test_struct_layouts_match_the_c_compiler():
    """(The layouts: tests/test_abi_units.py.)  The stats the Python layer reads by position."""
    assert [f for f, _ in abi.lg_distill_rtrain_stats._fields_] == ["behavior", "optimizer_steps", "grad_norm", "memory_grad_norm"]


def test_one_refusal_per_entry_point_names_it():
    lib = library("policy", "distill_rtrain")
    p = 0x1000          # never read: the NULL handle is refused first
    hyper = abi.lg_distill_train_hyper(0, 1.0)
    calls = {
        "lg_distill_rtrain_create": lambda: lib.lg_distill_rtrain_create(None, None, None, 1e-3, 64),
        "lg_distill_rtrain_group": lambda: lib.lg_distill_rtrain_group(None, p, p, p, 4, 8, 0, 3, 1, C.byref(hyper), None),
        "lg_distill_rtrain_update": lambda: lib.lg_distill_rtrain_update(None, p, p, p, 4, 8, 1, 3, C.byref(hyper), None, None),
        "lg_distill_rtrain_parameter_count": lambda: lib.lg_distill_rtrain_parameter_count(None),
        "lg_distill_rtrain_student_parameter_count": lambda: lib.lg_distill_rtrain_student_parameter_count(None),
        "lg_distill_rtrain_workspace_bytes": lambda: lib.lg_distill_rtrain_workspace_bytes(None),
        "lg_distill_rtrain_gradients": lambda: lib.lg_distill_rtrain_gradients(None, p, p, p, 3, None),
        "lg_distill_rtrain_forward_outputs": lambda: lib.lg_distill_rtrain_forward_outputs(None, p, None),
        "lg_distill_rtrain_step_losses": lambda: lib.lg_distill_rtrain_step_losses(None, p, 4, None),
        "lg_distill_rtrain_get_carry": lambda: lib.lg_distill_rtrain_get_carry(None, p, p, 4, 0, None),
        "lg_distill_rtrain_set_carry": lambda: lib.lg_distill_rtrain_set_carry(None, p, p, 4, None),
        "lg_distill_rtrain_reset_carry": lambda: lib.lg_distill_rtrain_reset_carry(None, None),
        "lg_distill_rtrain_get_parameters": lambda: lib.lg_distill_rtrain_get_parameters(None, p, None),
        "lg_distill_rtrain_get_state": lambda: lib.lg_distill_rtrain_get_state(None, p, p, p, None, None, None),
        "lg_distill_rtrain_set_state": lambda: lib.lg_distill_rtrain_set_state(None, p, p, p, 0, 1e-3, None),
        "lg_distill_rtrain_set_learning_rate": lambda: lib.lg_distill_rtrain_set_learning_rate(None, 1e-3, None),
    }
    # destroy cannot fail (NULL is a no-op)
    check_refusals("distill_rtrain", lib, calls, quiet={"lg_distill_rtrain_destroy"}, returns_handle={"lg_distill_rtrain_create"})
    lib.lg_distill_rtrain_destroy(None)


def test_python_refusals_that_need_no_gpu():
    from extended_legged_gym_amd.rl import NativeDistillation, NativeRecurrentDistillation
    with pytest.raises(ValueError, match=r"Unknown loss type: l1\. Supported types are: mse, huber"):
        NativeRecurrentDistillation(None, {}, loss_type="l1")
    with pytest.raises(NotImplementedError, match="multi_gpu_cfg"):
        NativeRecurrentDistillation(object(), {}, multi_gpu_cfg={"global_rank": 0, "world_size": 2})
    with pytest.raises(TypeError, match="NativeStudentTeacherRecurrent"):
        NativeRecurrentDistillation(object(), {})

    class Recurrent:
        is_recurrent = True
    with pytest.raises(NotImplementedError, match="recurrent student"):          # the feed-forward trainer keeps refusing, as NativePPO does
        NativeDistillation(Recurrent(), {})


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_recurrent_distillation_kernels_do_not_spill_and_fit_the_lds():
    blocks = kernel_metadata("lg_distill_train_recurrent.hip")
    assert len(blocks) == len(KERNELS), sorted(blocks)          # every kernel of the translation unit is held to the bounds
    check_no_spill_no_scratch(blocks, KERNELS, LDS_SHARED)
