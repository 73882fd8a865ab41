"""CPU side of the runner's device pieces (include/lgrunner.h); names, exports, declarations and struct layouts: tests/test_abi_units.py.  Here:
the two prefixes and the Python surface; one refused call per entry point leaves a message that starts with that entry point's name; the unit's
kernels (cross-compiled for gfx950) show no spills, no scratch, and LDS within the 80 KB the other policy-side units hold.  No GPU needed."""
import ctypes as C
import os

import pytest

from extended_legged_gym_amd import abi
from tests.abi_checks import HIPCC, check_no_spill_no_scratch, check_refusals, kernel_metadata, library

LDS_SHARED = 80 * 1024


def test_header_exports_and_declarations_agree():
    assert all(n.startswith(("lg_runner_", "lg_obsnorm_")) for n in abi.symbols("runner"))
    from extended_legged_gym_amd import rl
    assert all(hasattr(rl, n) for n in ("NativeEmpiricalNormalization", "NativeOnPolicyRunner", "collect_rollout_tracked", "EpisodeTracker"))


def test_one_refusal_per_entry_point_names_it():
    lib = library("policy", "runner")
    p = 0x1000          # never read: the NULL handle / the bad argument is refused first
    rows = abi.lg_rollout(*[p] * 11)
    calls = {
        "lg_obsnorm_create": lambda: lib.lg_obsnorm_create(0, 1e-2, -1, 0),
        "lg_obsnorm_get_state": lambda: lib.lg_obsnorm_get_state(None, p, p, p, None, None),
        "lg_obsnorm_set_state": lambda: lib.lg_obsnorm_set_state(None, p, p, p, 0, None),
        "lg_obsnorm_step": lambda: lib.lg_obsnorm_step(None, p, 4, 8, 1, p, None),
        "lg_obsnorm_inverse": lambda: lib.lg_obsnorm_inverse(None, p, 4, 8, p, None),
        "lg_obsnorm_carried": lambda: lib.lg_obsnorm_carried(None, p, 4, None),
        "lg_obsnorm_forget_carried": lambda: lib.lg_obsnorm_forget_carried(None),
        "lg_runner_collect": lambda: lib.lg_runner_collect(None, None, None, None, None, p, 0, 1, 4, 0.99, 0.95, 1, C.byref(rows), None, None, None, None, None,
                                                          None, None),
        "lg_runner_episode_track": lambda: lib.lg_runner_episode_track(None, p, 4, 8, p, p, p, p, None),
    }
    check_refusals("runner", lib, calls, quiet={"lg_obsnorm_destroy"}, returns_handle={"lg_obsnorm_create"})          # destroy cannot fail: NULL is a no-op
    lib.lg_obsnorm_destroy(None)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_runner_kernels_do_not_spill_and_fit_the_lds():
    blocks = kernel_metadata("lg_runner.hip")
    kernels = ("obsnorm_partial_kernel", "obsnorm_update_kernel", "obsnorm_apply_kernel", "runner_episode_kernel")
    assert len(blocks) == len(kernels), sorted(blocks)
    check_no_spill_no_scratch(blocks, kernels, LDS_SHARED)
