"""CPU side of the native recurrent PPO update (include/lgtrain_recurrent.h); names, exports, declarations and the struct layout:
tests/test_abi_units.py.  Here: the header keeps its prefix to itself; one refused call per entry point leaves a message that starts with that
entry point's name; the kernels of csrc/lg_train_recurrent.hip, cross-compiled for gfx950, use no scratch and fit the LDS: the three 32-row tile
kernels (512 lanes, a workgroup that owns its compute unit) are held to the 128 KB the inference memory kernel already lives in, the two
element-wise kernels to the 80 KB of a workgroup that shares its compute unit.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

from extended_legged_gym_amd import abi
from tests.abi_checks import HIPCC, check_no_spill_no_scratch, check_refusals, header_source, kernel_metadata, library

LDS_OWNER, LDS_SHARED = 128 * 1024, 80 * 1024
TILE_KERNELS = ("rnn_train_forward_kernel", "rnn_backward_kernel", "rows_matmul_kernel")


def test_header_exports_and_declarations_agree():
    for other in ("lgpolicy.h", "lgtrain.h"):
        assert not re.search(r"lg_ppo_recurrent_[a-z_]+\(", header_source(other))
    from extended_legged_gym_amd import rl
    assert hasattr(rl, "NativeRecurrentPPO") and issubclass(rl.NativeRecurrentPPO, rl.NativePPO)


def test_one_refusal_per_entry_point_names_it():
    lib = library("policy", "train_recurrent")
    p = 0x1000          # never read: the NULL handle is refused first
    rows, hyper = abi.lg_ppo_rows(*[p] * 9), abi.lg_ppo_hyper(0.2, 1.0, 0.0, 1, 1.0, 0, 0.01)
    hid, params = abi.lg_rollout_hidden(p, p, p, p), abi.lg_ppo_recurrent_params()
    calls = {
        "lg_ppo_recurrent_create": lambda: lib.lg_ppo_recurrent_create(None, None, None, None, C.byref(params), 0, 1e-3, 64, p),
        "lg_ppo_recurrent_minibatch": lambda: lib.lg_ppo_recurrent_minibatch(None, C.byref(rows), C.byref(hid), p, 4, 8, 0, 8, C.byref(hyper), None),
        "lg_ppo_recurrent_update": lambda: lib.lg_ppo_recurrent_update(None, C.byref(rows), C.byref(hid), p, 4, 8, 1, 1, C.byref(hyper), None, None),
        "lg_ppo_recurrent_parameter_count": lambda: lib.lg_ppo_recurrent_parameter_count(None),
        "lg_ppo_recurrent_workspace_bytes": lambda: lib.lg_ppo_recurrent_workspace_bytes(None),
        "lg_ppo_recurrent_gradients": lambda: lib.lg_ppo_recurrent_gradients(None, p, p, p, None),
        "lg_ppo_recurrent_forward_outputs": lambda: lib.lg_ppo_recurrent_forward_outputs(None, p, p, None),
        "lg_ppo_recurrent_get_parameters": lambda: lib.lg_ppo_recurrent_get_parameters(None, p, None),
        "lg_ppo_recurrent_get_state": lambda: lib.lg_ppo_recurrent_get_state(None, p, p, p, None, None, None),
        "lg_ppo_recurrent_set_state": lambda: lib.lg_ppo_recurrent_set_state(None, p, p, p, 0, 1e-3, None),
        "lg_ppo_recurrent_set_learning_rate": lambda: lib.lg_ppo_recurrent_set_learning_rate(None, 1e-3, None),
        "lg_ppo_recurrent_get_images": lambda: lib.lg_ppo_recurrent_get_images(None, 0, 0, p, p, None),
    }
    # destroy cannot fail: NULL is a no-op
    check_refusals("train_recurrent", lib, calls, quiet={"lg_ppo_recurrent_destroy"}, returns_handle={"lg_ppo_recurrent_create"})
    lib.lg_ppo_recurrent_destroy(None)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_recurrent_train_kernels_do_not_spill_and_fit_the_lds():
    check_no_spill_no_scratch(kernel_metadata("lg_train_recurrent.hip"), TILE_KERNELS + ("rnn_retile_kernel", "rec_index_kernel"),
                              lambda part: LDS_OWNER if part in TILE_KERNELS else LDS_SHARED)
