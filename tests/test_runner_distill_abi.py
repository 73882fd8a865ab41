"""CPU side of the runner's distillation collection (include/lgrunner_distill.h); names, exports, declarations and the struct layout:
tests/test_abi_units.py.  Here: the two calls take the plain collectors' arguments plus the hooks, the unit is in the Makefile and on the
Python surface; the struct's field order; one refused call per entry point leaves a message that starts with that entry point's name.  The unit
holds no kernel (it strings existing launches together), which is checked too, so there is no register or LDS budget to hold.  No GPU needed."""
import ctypes as C
import os
import re

from extended_legged_gym_amd import abi
from tests.abi_checks import CSRC, last_error, library


def test_header_exports_and_declarations_agree():
    lib = library("policy", "runner_distill")
    # the recurrent call takes the plain collector's arguments, then the hooks, then the stream
    plain_args = lib.lg_collect_distillation_recurrent.argtypes
    assert lib.lg_runner_collect_distillation_recurrent.argtypes == plain_args[:-1] + [C.POINTER(abi.lg_runner_distill), C.c_void_p]
    assert lib.lg_runner_collect_distillation.argtypes[:-2] == lib.lg_collect_distillation.argtypes[:-1]
    from extended_legged_gym_amd import rl
    assert hasattr(rl, "collect_distillation_tracked") and hasattr(rl, "NativeDistillationRunner")
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^OTHER :=.*\blg_runner_distill\.hip\b", makefile, flags=re.M) and "lgrunner_distill.h" in makefile


def test_struct_layout_matches_the_c_compiler():
    """(The layout: tests/test_abi_units.py.)  The order the collector fills the struct in."""
    assert [f for f, _ in abi.lg_runner_distill._fields_] == ["student_normalizer", "teacher_normalizer", "training", "episode"]


def test_one_refusal_per_entry_point_names_it():
    lib = library("policy", "runner", "runner_distill")
    p = 0x1000          # never read: a NULL argument or a NULL episode row is refused first
    rows = abi.lg_distill_rollout(*[p] * 7)
    calls = {
        "lg_runner_collect_distillation": lambda hooks: lib.lg_runner_collect_distillation(None, None, None, p, 0, 1, 4, None, C.byref(rows), hooks, None),
        "lg_runner_collect_distillation_recurrent": lambda hooks: lib.lg_runner_collect_distillation_recurrent(None, None, None, None, None, p, 0, 1, 4, None,
                                                                                                               C.byref(rows), *[None] * 8, hooks, None),
    }
    episode = abi.lg_runner_episode(raw_rewards=p, extras=p, cur_reward_sum=p, cur_episode_length=p, ep_return=None, ep_length=p)
    bad = abi.lg_runner_distill(episode=C.pointer(episode))
    # everything lg_collect_distillation refuses: NULL arguments; all-NULL hooks: the same refusal; an episode with a NULL row, before anything else is looked at
    assert set(calls) == set(abi.symbols("runner_distill"))          # (three refusals each: check_refusals' loop, with the word each message carries)
    for name, call in calls.items():
        for hooks, word in ((None, "null argument"), (C.byref(abi.lg_runner_distill()), "null argument"), (C.byref(bad), "null episode row")):
            assert call(hooks) == abi.LG_ERR_INVALID, (name, word)
            assert last_error(lib).startswith(name + ": ") and word in last_error(lib), (name, last_error(lib))


def test_the_unit_adds_no_kernel():
    """include/lgrunner_distill.h promises the bits of the kernels it strings together; that holds because the unit launches nothing of its own."""
    text = open(os.path.join(CSRC, "lg_runner_distill.hip")).read()
    assert "__global__" not in text and "hipLaunchKernelGGL" not in text and "<<<" not in text
