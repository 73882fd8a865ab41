"""CPU side of the runner's collection with privileged critic observations (include/lgrunner_privileged.h); names, exports, declarations and
the struct layout: tests/test_abi_units.py.  Here: the Python surface and the struct's field order; one refused call per entry point leaves a
message that starts with that entry point's name; the unit's kernels (cross-compiled for gfx950) show no spills, no scratch, and LDS within the
80 KB the other policy-side units hold.  No GPU needed."""
import ctypes as C
import os

import pytest

from extended_legged_gym_amd import abi
from tests.abi_checks import HIPCC, check_no_spill_no_scratch, check_refusals, kernel_metadata, last_error, library

LDS_SHARED = 80 * 1024


def test_header_exports_and_declarations_agree():
    from extended_legged_gym_amd import rl
    from extended_legged_gym_amd.rl import runner
    assert hasattr(rl.NativeEmpiricalNormalization, "step_pair") and hasattr(runner, "collects_privileged_natively")


def test_struct_layout_matches_the_c_compiler():
    """(The layout: tests/test_abi_units.py.)  The order the collector fills the struct in."""
    assert [f for f, _ in abi.lg_runner_privileged._fields_] == ["history", "critic_normalizer", "privileged_observations", "last_observations"]


def test_one_refusal_per_entry_point_names_it():
    lib = library("policy", "runner", "runner_privileged")
    p = 0x1000          # never read: the NULL handle / the NULL struct is refused first
    rows = abi.lg_rollout(*[p] * 11)
    calls = {
        "lg_obsnorm_step_pair": lambda: lib.lg_obsnorm_step_pair(None, p, 8, p, None, p, 8, p, 4, 1, None),
        "lg_runner_collect_privileged": lambda: lib.lg_runner_collect_privileged(p, None, p, None, p, p, 0, 1, 4, 0.99, 0.95, 1, C.byref(rows), None, None, None, None,
                                                                                None, None, None, None),
    }
    check_refusals("runner_privileged", lib, calls)
    assert "privileged" in last_error(lib)          # (the NULL struct, refused before anything is read or launched)
    priv = abi.lg_runner_privileged()          # a struct without rows
    assert lib.lg_runner_collect_privileged(p, None, p, None, p, p, 0, 1, 4, 0.99, 0.95, 1, C.byref(rows), None, None, None, None, None, None, C.byref(priv),
                                            None) == abi.LG_ERR_INVALID
    assert last_error(lib).startswith("lg_runner_collect_privileged: ") and "privileged_observations" in last_error(lib)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_pair_kernels_do_not_spill_and_fit_the_lds():
    """csrc/lg_runner_privileged.hip: the three kernels over two handles, and nothing else."""
    blocks = kernel_metadata("lg_runner_privileged.hip")
    kernels = ("obsnorm_partial_pair_kernel", "obsnorm_update_pair_kernel", "obsnorm_apply_pair_kernel")
    assert len(blocks) == len(kernels), sorted(blocks)
    check_no_spill_no_scratch(blocks, kernels, LDS_SHARED)
