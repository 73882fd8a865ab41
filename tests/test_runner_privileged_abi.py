"""CPU side of the runner's collection with privileged critic observations (include/lgrunner_privileged.h), the pattern of tests/test_runner_abi.py:
the header's names, the library's exports and the ctypes mirror agree; the symbol list is disjoint from every other; the new struct's layout matches
a C compiler's; one refused call per entry point leaves a message that starts with that entry point's name; the unit's kernels (cross-compiled
for gfx950) show no spills, no scratch, and LDS within the 80 KB the other policy-side units hold.  No GPU needed."""
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
HEADER = os.path.join(ROOT, "include", "lgrunner_privileged.h")
LDS_SHARED = 80 * 1024


def _msg(lib):
    return (lib.lg_mlp_last_error(None) or b"").decode()


def test_header_exports_and_declarations_agree():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)          # (the comments speak of lgrunner.h's calls)
    names = sorted(set(re.findall(r"\b(lg_(?:runner|obsnorm)_[a-z_]+)\(", text)))
    assert names == sorted(abi.RUNNER_PRIVILEGED_SYMBOLS), (names, abi.RUNNER_PRIVILEGED_SYMBOLS)
    for other in (abi.RUNNER_SYMBOLS, abi.TRAIN_SYMBOLS, abi.POLICY_SYMBOLS, abi.TRAIN_RECURRENT_SYMBOLS, abi.DISTILL_TRAIN_SYMBOLS, abi.DISTILL_RTRAIN_SYMBOLS,
                  abi.ESTIMATOR_TRAIN_SYMBOLS, abi.SYMMETRY_TRAIN_SYMBOLS, abi.PRODUCT_SYMBOLS, abi.ESTIMATOR_SYMBOLS, abi.ESTIMATOR_BF16_SYMBOLS):
        assert not set(names) & set(other)
    plain = abi.declare_runner(abi.declare_train(abi.declare_policy(C.CDLL(LIB))))
    for sym in names:
        assert hasattr(plain, sym), sym
        assert getattr(plain, sym).argtypes is None, f"another declare function declares {sym}"
    lib = abi.declare_runner_privileged(C.CDLL(LIB))
    for sym in names:
        assert getattr(lib, sym).argtypes is not None, sym
    from extended_legged_gym_amd import rl
    from extended_legged_gym_amd.rl import runner
    assert hasattr(rl.NativeEmpiricalNormalization, "step_pair") and hasattr(runner, "collects_privileged_natively")


def test_struct_layout_matches_the_c_compiler(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or os.path.join(LLVM, "clang")
    name, cls = "lg_runner_privileged", abi.lg_runner_privileged
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "lgrunner_privileged.h"', "int main(void) {", f'  printf("{name} %zu\\n", sizeof({name}));']
    for field, _ in cls._fields_:
        lines.append(f'  printf("{name}.{field} %zu\\n", offsetof({name}, {field}));')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True, capture_output=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got[name]) == C.sizeof(cls)
    assert [f for f, _ in cls._fields_] == ["history", "critic_normalizer", "privileged_observations", "last_observations"]
    for field, _ in cls._fields_:
        assert int(got[f"{name}.{field}"]) == getattr(cls, field).offset, field


def test_one_refusal_per_entry_point_names_it():
    lib = abi.declare_runner_privileged(abi.declare_runner(abi.declare_policy(C.CDLL(LIB))))
    p = 0x1000          # never read: the NULL handle / the NULL struct is refused first
    rows = abi.lg_rollout(*[p] * 11)
    calls = {
        "lg_obsnorm_step_pair": lambda: lib.lg_obsnorm_step_pair(None, p, 8, p, None, p, 8, p, 4, 1, None),
        "lg_runner_collect_privileged": lambda: lib.lg_runner_collect_privileged(p, None, p, None, p, p, 0, 1, 4, 0.99, 0.95, 1, C.byref(rows), None, None, None, None,
                                                                                None, None, None, None),
    }
    assert set(calls) == set(abi.RUNNER_PRIVILEGED_SYMBOLS)
    for name, call in calls.items():
        assert call() == abi.LG_ERR_INVALID, name
        assert _msg(lib).startswith(name + ": "), (name, _msg(lib))
    assert "privileged" in _msg(lib)          # (the NULL struct, refused before anything is read or launched)
    priv = abi.lg_runner_privileged()          # a struct without rows
    assert lib.lg_runner_collect_privileged(p, None, p, None, p, p, 0, 1, 4, 0.99, 0.95, 1, C.byref(rows), None, None, None, None, None, None, C.byref(priv),
                                            None) == abi.LG_ERR_INVALID
    assert _msg(lib).startswith("lg_runner_collect_privileged: ") and "privileged_observations" in _msg(lib)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_pair_kernels_do_not_spill_and_fit_the_lds(tmp_path):
    """The route of tests/test_runner_abi.py on csrc/lg_runner_privileged.hip: the three kernels over two handles, and nothing else."""
    obj, fat, co = (str(tmp_path / n) for n in ("lg_runner_privileged.o", "fat.bin", "k.co"))
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-fno-slp-vectorize", "-c", "-o", obj,
                    os.path.join(CSRC, "lg_runner_privileged.hip")], check=True, capture_output=True)
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
    kernels = ("obsnorm_partial_pair_kernel", "obsnorm_update_pair_kernel", "obsnorm_apply_pair_kernel")
    assert len(blocks) == len(kernels), sorted(blocks)
    for part in kernels:
        hit = [v for k, v in blocks.items() if part in k]
        assert len(hit) == 1, (part, sorted(blocks))
        r = hit[0]
        print(part, r)
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0 and r["private_segment_fixed_size"] == 0, (part, r)
        assert r["group_segment_fixed_size"] <= LDS_SHARED, (part, r)
