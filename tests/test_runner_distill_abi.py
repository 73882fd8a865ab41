"""CPU side of the runner's distillation collection (include/lgrunner_distill.h), the pattern of tests/test_runner_privileged_abi.py: the header's
names, the library's exports and the ctypes mirror agree; the symbol list is disjoint from every other and declared by no other declare function;
the new struct's layout matches a C compiler's; one refused call per entry point leaves a message that starts with that entry point's name.  The
unit holds no kernel (it strings existing launches together), which is checked too, so there is no register or LDS budget to hold.  No GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

from extended_legged_gym_amd import abi
from tests.test_policy_recurrent_abi import LLVM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "extended_legged_gym_amd", "csrc")
LIB = os.path.join(CSRC, "liblgstep.so")
HEADER = os.path.join(ROOT, "include", "lgrunner_distill.h")


def _msg(lib):
    return (lib.lg_mlp_last_error(None) or b"").decode()


def test_header_exports_and_declarations_agree():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)          # (the comments speak of other headers' calls)
    names = sorted(set(re.findall(r"\b(lg_(?:runner|obsnorm)_[a-z_]+)\(", text)))
    assert names == sorted(abi.RUNNER_DISTILL_SYMBOLS), (names, abi.RUNNER_DISTILL_SYMBOLS)
    for other in (abi.RUNNER_SYMBOLS, abi.RUNNER_PRIVILEGED_SYMBOLS, abi.TRAIN_SYMBOLS, abi.POLICY_SYMBOLS, abi.TRAIN_RECURRENT_SYMBOLS, abi.DISTILL_TRAIN_SYMBOLS,
                  abi.DISTILL_RTRAIN_SYMBOLS, abi.ESTIMATOR_TRAIN_SYMBOLS, abi.SYMMETRY_TRAIN_SYMBOLS, abi.PRODUCT_SYMBOLS, abi.ESTIMATOR_SYMBOLS,
                  abi.ESTIMATOR_BF16_SYMBOLS):
        assert not set(names) & set(other)
    plain = abi.declare_runner_privileged(abi.declare_runner(abi.declare_distill_rtrain(abi.declare_distill_train(abi.declare_train(abi.declare_policy(C.CDLL(LIB)))))))
    for sym in names:
        assert hasattr(plain, sym), sym
        assert getattr(plain, sym).argtypes is None, f"another declare function declares {sym}"
    lib = abi.declare_runner_distill(C.CDLL(LIB))
    for sym in names:
        assert getattr(lib, sym).argtypes is not None, sym
    # the recurrent call takes the plain collector's arguments, then the hooks, then the stream
    plain_args = abi.declare_policy(C.CDLL(LIB)).lg_collect_distillation_recurrent.argtypes
    assert lib.lg_runner_collect_distillation_recurrent.argtypes == plain_args[:-1] + [C.POINTER(abi.lg_runner_distill), C.c_void_p]
    assert lib.lg_runner_collect_distillation.argtypes[:-2] == abi.declare_policy(C.CDLL(LIB)).lg_collect_distillation.argtypes[:-1]
    from extended_legged_gym_amd import rl
    assert hasattr(rl, "collect_distillation_tracked") and hasattr(rl, "NativeDistillationRunner")
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^OTHER :=.*\blg_runner_distill\.hip\b", makefile, flags=re.M) and "lgrunner_distill.h" in makefile


def test_struct_layout_matches_the_c_compiler(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or os.path.join(LLVM, "clang")
    name, cls = "lg_runner_distill", abi.lg_runner_distill
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "lgrunner_distill.h"', "int main(void) {", f'  printf("{name} %zu\\n", sizeof({name}));']
    for field, _ in cls._fields_:
        lines.append(f'  printf("{name}.{field} %zu\\n", offsetof({name}, {field}));')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True, capture_output=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got[name]) == C.sizeof(cls)
    assert [f for f, _ in cls._fields_] == ["student_normalizer", "teacher_normalizer", "training", "episode"]
    for field, _ in cls._fields_:
        assert int(got[f"{name}.{field}"]) == getattr(cls, field).offset, field


def test_one_refusal_per_entry_point_names_it():
    lib = abi.declare_runner_distill(abi.declare_runner(abi.declare_policy(C.CDLL(LIB))))
    p = 0x1000          # never read: a NULL argument or a NULL episode row is refused first
    rows = abi.lg_distill_rollout(*[p] * 7)
    calls = {
        "lg_runner_collect_distillation": lambda hooks: lib.lg_runner_collect_distillation(None, None, None, p, 0, 1, 4, None, C.byref(rows), hooks, None),
        "lg_runner_collect_distillation_recurrent": lambda hooks: lib.lg_runner_collect_distillation_recurrent(None, None, None, None, None, p, 0, 1, 4, None,
                                                                                                               C.byref(rows), *[None] * 8, hooks, None),
    }
    assert set(calls) == set(abi.RUNNER_DISTILL_SYMBOLS)
    episode = abi.lg_runner_episode(raw_rewards=p, extras=p, cur_reward_sum=p, cur_episode_length=p, ep_return=None, ep_length=p)
    bad = abi.lg_runner_distill(episode=C.pointer(episode))
    for name, call in calls.items():
        assert call(None) == abi.LG_ERR_INVALID, name          # everything lg_collect_distillation refuses: NULL arguments
        assert _msg(lib).startswith(name + ": ") and "null argument" in _msg(lib), (name, _msg(lib))
        assert call(C.byref(abi.lg_runner_distill())) == abi.LG_ERR_INVALID, name          # all-NULL hooks: the same refusal
        assert _msg(lib).startswith(name + ": ") and "null argument" in _msg(lib), (name, _msg(lib))
        assert call(C.byref(bad)) == abi.LG_ERR_INVALID, name          # an episode with a NULL row, before anything else is looked at
        assert _msg(lib).startswith(name + ": ") and "null episode row" in _msg(lib), (name, _msg(lib))


def test_the_unit_adds_no_kernel():
    """include/lgrunner_distill.h promises the bits of the kernels it strings together; that holds because the unit launches nothing of its own."""
    text = open(os.path.join(CSRC, "lg_runner_distill.hip")).read()
    assert "__global__" not in text and "hipLaunchKernelGGL" not in text and "<<<" not in text
