"""CPU side of the bf16-encoder trainer of the terrain estimator (include/lgestimator_train_bf16.h): the unit of `abi.UNITS` against its header, the
built library and a C compiler (tests/abi_checks.py); one refused call per entry point leaves a message that starts with that entry point's name; the
Python layer's refusals need no GPU; the kernels' code-object metadata (cross-compiled for gfx950) shows no spills, no scratch and LDS within the 80 KB
the other estimator kernels are held to.  No GPU needed."""
import os
import re

import pytest

from extended_legged_gym_amd import abi
from tests.abi_checks import HIPCC, check_no_spill_no_scratch, check_refusals, check_struct_layouts, check_unit_agreement, header_source, kernel_metadata, library

UNIT = "estimator_train_bf16"
LDS_SHARED = 80 * 1024
# every kernel of the translation unit, by a part of its (mangled) name that no other one contains; the weight gradient is three instances
KERNELS = ("est16_dgrad_kernel", "est16_pool_backward_kernel", "est16_expand_kernel", "est16_round_kernel", "est16_retile_kernel",
           "est16_wgrad_kernelILi2ELb1E", "est16_wgrad_kernelILi4ELb0E", "est16_wgrad_kernelILi8ELb0E")


def test_unit_agrees_with_its_header_and_the_library(tmp_path):
    check_unit_agreement(UNIT)
    check_struct_layouts(UNIT, tmp_path)
    assert all(n.startswith("lg_estimator_bf16train_") for n in abi.symbols(UNIT))
    for other in ("lgpolicy.h", "lgtrain.h", "lgestimator_train.h"):
        assert not re.search(r"lg_estimator_bf16train_[a-z_]+\(", header_source(other)), other
    slab = library(UNIT).lg_estimator_bf16train_wgrad_slab_rows()
    assert slab > 0 and slab % 32 == 0          # a slab is whole k-steps of 32 rows
    stages = dict(re.findall(r"LG_EST16_([A-Z0-9_]+) = (\d+)", header_source("lgestimator_train_bf16.h")))
    assert {k.lower(): int(v) for k, v in stages.items()} == abi.ESTIMATOR_BF16_STAGES


def test_one_refusal_per_entry_point_names_it():
    lib = library("policy", "estimator_train", UNIT)
    p = 0x1000          # never read: the NULL handle is refused first
    calls = {
        "lg_estimator_bf16train_create": lambda: lib.lg_estimator_bf16train_create(None, None, None, None, None, 1e-3, 64),
        "lg_estimator_bf16train_saved_stage": lambda: lib.lg_estimator_bf16train_saved_stage(None, 1, p, 4, None),
        "lg_estimator_bf16train_backward_stage": lambda: lib.lg_estimator_bf16train_backward_stage(None, 0, p, 4, p, p, None),
    }
    check_refusals(UNIT, lib, calls, quiet={"lg_estimator_bf16train_wgrad_slab_rows"}, returns_handle={"lg_estimator_bf16train_create"})


def test_python_refusals_that_need_no_gpu():
    from extended_legged_gym_amd.rl import NativeEstimatorDistillation

    class Fp32:
        precision = "fp32"

    class Bf16:
        precision = "bf16"
    with pytest.raises(ValueError, match=r"encoder_precision=\"bf16\""):
        NativeEstimatorDistillation(Fp32(), {}, encoder_training="bf16")
    with pytest.raises(ValueError, match=r"Unknown encoder_training: fp16"):
        NativeEstimatorDistillation(Bf16(), {}, encoder_training="fp16")
    with pytest.raises(NotImplementedError, match=r"encoder_training=\"bf16\""):          # the default still refuses a bf16 estimator, and names the option
        NativeEstimatorDistillation(Bf16(), {})
    with pytest.raises(TypeError, match="NativeTerrainEstimator"):
        NativeEstimatorDistillation(Bf16(), {}, encoder_training="bf16")
    # the runner's pair: bf16 training plays the estimator it trains
    from extended_legged_gym_amd.rl.estimator_runner import parse_encoder_training
    assert parse_encoder_training({}, "bf16") == "fp32" and parse_encoder_training({"encoder_training": "bf16"}, "bf16") == "bf16"
    with pytest.raises(ValueError, match=r"runner\.encoder_precision is \"fp32\""):
        parse_encoder_training({"encoder_training": "bf16"}, "fp32")
    with pytest.raises(ValueError, match="Unknown algorithm.encoder_training: half"):
        parse_encoder_training({"encoder_training": "half"}, "bf16")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_bf16_trainer_kernels_do_not_spill_and_fit_the_lds():
    blocks = kernel_metadata("lg_estimator_train_bf16.hip")
    assert len(blocks) == len(KERNELS), sorted(blocks)          # every kernel of the translation unit is held to the bounds
    check_no_spill_no_scratch(blocks, KERNELS, LDS_SHARED)
