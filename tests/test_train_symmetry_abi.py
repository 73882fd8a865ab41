"""CPU side of the symmetric PPO trainer (include/lgtrain_symmetry.h); names, exports, declarations and struct layouts: tests/test_abi_units.py.
Here: the prefix and the block limit; the stats struct extends lg_ppo_stats; one refused call per entry point leaves a message that starts with
that entry point's name; the unit's kernels (cross-compiled for gfx950) show no spills, no scratch, and LDS within the two bounds of
tests/test_train_abi.py: the 32-row forward tile (a workgroup that owns its compute unit) within 128 KB, every other kernel within 80 KB.  No GPU
needed."""
import ctypes as C
import os
import re

import pytest

from extended_legged_gym_amd import abi
from tests.abi_checks import HIPCC, check_no_spill_no_scratch, check_refusals, header_source, kernel_metadata, library

LDS_OWNER, LDS_SHARED = 128 * 1024, 80 * 1024


def test_header_exports_and_declarations_agree():
    assert all(n.startswith("lg_ppo_sym_") for n in abi.symbols("train_symmetry"))
    assert int(re.search(r"#define\s+LG_PPO_SYM_MAX_BLOCKS\s+(\d+)", header_source("lgtrain_symmetry.h")).group(1)) == abi.SYMMETRY_MAX_BLOCKS == 4
    from extended_legged_gym_amd import rl
    assert hasattr(rl, "NativeSymmetricPPO") and hasattr(rl, "signed_permutation_tables")


def test_struct_layouts_match_the_c_compiler():
    """(The layouts: tests/test_abi_units.py.)  lg_ppo_stats plus one double: an lg_ppo_stats reader sees its five fields where it expects them."""
    assert [f for f, _ in abi.lg_ppo_sym_stats._fields_][:5] == [f for f, _ in abi.lg_ppo_stats._fields_]
    assert C.sizeof(abi.lg_ppo_sym_stats) == C.sizeof(abi.lg_ppo_stats) + 8


def test_one_refusal_per_entry_point_names_it():
    lib = library("policy", "train_symmetry")
    p = 0x1000          # never read: the NULL handle is refused first
    rows, hyper = abi.lg_ppo_rows(*[p] * 9), abi.lg_ppo_hyper(0.2, 1.0, 0.0, 1, 1.0, 0, 0.01)
    calls = {
        "lg_ppo_sym_create": lambda: lib.lg_ppo_sym_create(None, None, None, None, None, None, p, 0, 1e-3, 64, p, None, None),
        "lg_ppo_sym_minibatch": lambda: lib.lg_ppo_sym_minibatch(None, C.byref(rows), p, 8, C.byref(hyper), None),
        "lg_ppo_sym_update": lambda: lib.lg_ppo_sym_update(None, C.byref(rows), 8, p, 1, 1, C.byref(hyper), None, None),
        "lg_ppo_sym_parameter_count": lambda: lib.lg_ppo_sym_parameter_count(None),
        "lg_ppo_sym_gradients": lambda: lib.lg_ppo_sym_gradients(None, p, p, p, p, None),
        "lg_ppo_sym_forward_outputs": lambda: lib.lg_ppo_sym_forward_outputs(None, p, p, None),
        "lg_ppo_sym_get_parameters": lambda: lib.lg_ppo_sym_get_parameters(None, p, None),
        "lg_ppo_sym_get_state": lambda: lib.lg_ppo_sym_get_state(None, p, p, p, None, None, None),
        "lg_ppo_sym_set_state": lambda: lib.lg_ppo_sym_set_state(None, p, p, p, 0, 1e-3, None),
        "lg_ppo_sym_set_learning_rate": lambda: lib.lg_ppo_sym_set_learning_rate(None, 1e-3, None),
    }
    check_refusals("train_symmetry", lib, calls, quiet={"lg_ppo_sym_destroy"}, returns_handle={"lg_ppo_sym_create"})          # destroy cannot fail: NULL is a no-op
    lib.lg_ppo_sym_destroy(None)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_symmetry_kernels_do_not_spill_and_fit_the_lds():
    blocks = kernel_metadata("lg_train_symmetry.hip")
    kernels = ("sym_fwd_kernel", "sym_loss_kernel", "sym_loss_finish_kernel", "sym_wgrad_kernel", "sym_stats_kernel")
    existing = ("ppo_forward_kernel", "ppo_loss_kernel", "ppo_loss_finish_kernel", "ppo_backward_kernel", "ppo_wgrad_kernel", "ppo_grad_reduce_kernel",
                "ppo_norm_finish_kernel", "ppo_adam_kernel", "ppo_stats_kernel")
    assert len(blocks) == len(kernels), sorted(blocks)
    for name in blocks:          # tests/test_train_abi.py finds lg_train.hip's kernels by substring: no new kernel may carry one of their names
        assert not any(e in name for e in existing), name
    check_no_spill_no_scratch(blocks, kernels, lambda part: LDS_OWNER if part == "sym_fwd_kernel" else LDS_SHARED)
