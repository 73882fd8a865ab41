"""CPU side of the runner's device pieces (include/lgrunner.h), the pattern of tests/test_train_symmetry_abi.py: the header names, the library's
exports and the ctypes mirror agree; the symbol list is disjoint from every other; the struct layouts match a C compiler's; one refused call per
entry point leaves a message that starts with that entry point's name; the unit's kernels (cross-compiled for gfx950) show no spills, no
scratch, and LDS within the 80 KB the other policy-side units hold.  No GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from extended_legged_gym_amd import abi
from tests.test_policy_recurrent_abi import HIPCC, LLVM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "extended_legged_gym_amd", "csrc")
LIB = os.path.join(CSRC, "liblgstep.so")
HEADER = os.path.join(ROOT, "include", "lgrunner.h")
LDS_SHARED = 80 * 1024


def _msg(lib):
    return (lib.lg_mlp_last_error(None) or b"").decode()


def test_header_exports_and_declarations_agree():
    text = open(HEADER).read()
    names = sorted(set(re.findall(r"\b(lg_(?:runner|obsnorm)_[a-z_]+)\(", text)))
    assert names == sorted(abi.RUNNER_SYMBOLS), (names, abi.RUNNER_SYMBOLS)
    assert all(n.startswith(("lg_runner_", "lg_obsnorm_")) for n in names)
    for other in (abi.TRAIN_SYMBOLS, abi.POLICY_SYMBOLS, abi.TRAIN_RECURRENT_SYMBOLS, abi.DISTILL_TRAIN_SYMBOLS, abi.DISTILL_RTRAIN_SYMBOLS,
                  abi.ESTIMATOR_TRAIN_SYMBOLS, abi.SYMMETRY_TRAIN_SYMBOLS, abi.PRODUCT_SYMBOLS, abi.ESTIMATOR_SYMBOLS, abi.ESTIMATOR_BF16_SYMBOLS):
        assert not set(names) & set(other)
    plain = abi.declare_train_symmetry(abi.declare_train(abi.declare_policy(C.CDLL(LIB))))
    for sym in names:
        assert hasattr(plain, sym), sym
        assert getattr(plain, sym).argtypes is None, f"another declare function declares {sym}"
    lib = abi.declare_runner(C.CDLL(LIB))
    for sym in names:
        assert getattr(lib, sym).argtypes is not None, sym
    from extended_legged_gym_amd import rl
    assert all(hasattr(rl, n) for n in ("NativeEmpiricalNormalization", "NativeOnPolicyRunner", "collect_rollout_tracked", "EpisodeTracker"))


def test_struct_layouts_match_the_c_compiler(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or os.path.join(LLVM, "clang")
    structs = {"lg_runner_episode": abi.lg_runner_episode, "lg_runner_hooks": abi.lg_runner_hooks}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "lgrunner.h"', "int main(void) {"]
    for name, cls in structs.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        for field, _ in cls._fields_:
            lines.append(f'  printf("{name}.{field} %zu\\n", offsetof({name}, {field}));')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True, capture_output=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for name, cls in structs.items():
        assert int(got[name]) == C.sizeof(cls), name
        for field, _ in cls._fields_:
            assert int(got[f"{name}.{field}"]) == getattr(cls, field).offset, (name, field)


def test_one_refusal_per_entry_point_names_it():
    lib = abi.declare_runner(abi.declare_policy(C.CDLL(LIB)))
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
    assert set(calls) | {"lg_obsnorm_destroy"} == set(abi.RUNNER_SYMBOLS)          # destroy cannot fail: NULL is a no-op
    for name, call in calls.items():
        rc = call()
        assert (rc is None or rc == 0) if name == "lg_obsnorm_create" else rc == abi.LG_ERR_INVALID, (name, rc)
        assert _msg(lib).startswith(name + ": "), (name, _msg(lib))
    lib.lg_obsnorm_destroy(None)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_runner_kernels_do_not_spill_and_fit_the_lds(tmp_path):
    """The route of tests/test_train_abi.py on csrc/lg_runner.hip."""
    obj, fat, co = (str(tmp_path / n) for n in ("lg_runner.o", "fat.bin", "k.co"))
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-fno-slp-vectorize", "-c", "-o", obj,
                    os.path.join(CSRC, "lg_runner.hip")], check=True, capture_output=True)
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}",
                    "--unbundle"], check=True, capture_output=True)
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    blocks, cur = {}, None
    for line in notes.splitlines():
        line = line.strip()
        if line.startswith("- .agpr_count:") or line.startswith("- .args:"):
            cur = {}
        m = re.match(r"-?\s*\.(\w+):\s+(\S+)$", line)
        if m and cur is not None:
            if m.group(1) == "name":
                blocks[m.group(2)] = cur
            elif m.group(2).isdigit():
                cur[m.group(1)] = int(m.group(2))
    kernels = ("obsnorm_partial_kernel", "obsnorm_update_kernel", "obsnorm_apply_kernel", "runner_episode_kernel")
    assert len(blocks) == len(kernels), sorted(blocks)
    for part in kernels:
        hit = [v for k, v in blocks.items() if part in k]
        assert len(hit) == 1, (part, sorted(blocks))
        r = hit[0]
        print(part, r)
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0 and r["private_segment_fixed_size"] == 0, (part, r)
        assert r["group_segment_fixed_size"] <= LDS_SHARED, (part, r)
