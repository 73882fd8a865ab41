"""CPU side of the native PPO update (include/lgtrain.h): the header names, the library's exports and the ctypes mirror agree; the struct layouts
match a C compiler's; one refused call per entry point leaves a message that starts with that entry point's name; the new kernels' code-object
metadata (cross-compiled for gfx950) shows no spills, no scratch, and LDS within bounds: the two 32-row tile kernels (512 lanes, a workgroup that owns
its compute unit, 160 KB in tests/test_estimator_abi.py's words) are held to the 128 KB `mlp_forward_kernel` already lives in; every other kernel to
the 80 KB that file allows a workgroup that shares its compute unit.  No GPU needed."""
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
HEADER = os.path.join(ROOT, "include", "lgtrain.h")
LDS_OWNER, LDS_SHARED = 128 * 1024, 80 * 1024          # the two tile kernels; everything else


def _msg(lib):
    return (lib.lg_mlp_last_error(None) or b"").decode()


def test_header_exports_and_declarations_agree():
    names = sorted(set(re.findall(r"\b(lg_[a-z_]+)\(", open(HEADER).read())))
    assert names == sorted(abi.TRAIN_SYMBOLS), (names, abi.TRAIN_SYMBOLS)
    plain = abi.declare_policy(C.CDLL(LIB))
    for sym in names:
        assert hasattr(plain, sym), sym
        assert getattr(plain, sym).argtypes is None, f"declare_policy declares {sym}"
        assert sym not in abi.POLICY_SYMBOLS
    lib = abi.declare_train(C.CDLL(LIB))
    for sym in names:
        assert getattr(lib, sym).argtypes is not None, sym
    assert not re.search(r"lg_ppo_[a-z_]+\(", open(os.path.join(ROOT, "include", "lgpolicy.h")).read())
    from extended_legged_gym_amd import rl
    assert hasattr(rl, "NativePPO")


def test_struct_layouts_match_the_c_compiler(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or os.path.join(LLVM, "clang")
    structs = {"lg_ppo_rows": abi.lg_ppo_rows, "lg_ppo_hyper": abi.lg_ppo_hyper, "lg_ppo_stats": abi.lg_ppo_stats}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "lgtrain.h"', "int main(void) {"]
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
    header = open(HEADER).read()
    assert re.search(r"LG_STD_SCALAR = 0, LG_STD_LOG = 1", header) and abi.NOISE_STD_TYPES == {"scalar": 0, "log": 1}
    assert re.search(r"LG_SCHEDULE_FIXED = 0, LG_SCHEDULE_ADAPTIVE = 1", header) and abi.LR_SCHEDULES == {"fixed": 0, "adaptive": 1}


def test_one_refusal_per_entry_point_names_it():
    lib = abi.declare_train(abi.declare_policy(C.CDLL(LIB)))
    p = 0x1000          # never read: the NULL handle is refused first
    rows, hyper = abi.lg_ppo_rows(*[p] * 9), abi.lg_ppo_hyper(0.2, 1.0, 0.0, 1, 1.0, 0, 0.01)
    calls = {
        "lg_ppo_create": lambda: lib.lg_ppo_create(None, None, None, None, None, None, p, 0, 1e-3, 64, p),
        "lg_ppo_minibatch": lambda: lib.lg_ppo_minibatch(None, C.byref(rows), p, 8, C.byref(hyper), None),
        "lg_ppo_update": lambda: lib.lg_ppo_update(None, C.byref(rows), 8, p, 1, 1, C.byref(hyper), None, None),
        "lg_ppo_parameter_count": lambda: lib.lg_ppo_parameter_count(None),
        "lg_ppo_gradients": lambda: lib.lg_ppo_gradients(None, p, p, p, None),
        "lg_ppo_forward_outputs": lambda: lib.lg_ppo_forward_outputs(None, p, p, None),
        "lg_ppo_get_parameters": lambda: lib.lg_ppo_get_parameters(None, p, None),
        "lg_ppo_get_state": lambda: lib.lg_ppo_get_state(None, p, p, p, None, None, None),
        "lg_ppo_set_state": lambda: lib.lg_ppo_set_state(None, p, p, p, 0, 1e-3, None),
        "lg_ppo_set_learning_rate": lambda: lib.lg_ppo_set_learning_rate(None, 1e-3, None),
    }
    # the two that cannot fail: destroy (NULL is a no-op) and the slab size
    assert set(calls) | {"lg_ppo_destroy", "lg_ppo_wgrad_slab_rows"} == set(abi.TRAIN_SYMBOLS)
    for name, call in calls.items():
        rc = call()
        assert (rc is None or rc == 0) if name == "lg_ppo_create" else rc == abi.LG_ERR_INVALID, (name, rc)
        assert _msg(lib).startswith(name + ": "), (name, _msg(lib))
    lib.lg_ppo_destroy(None)
    slab = lib.lg_ppo_wgrad_slab_rows()
    assert slab > 0 and slab % 4 == 0          # whole k-steps of the 16x16x4 MFMA


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_train_kernels_do_not_spill_and_fit_the_lds(tmp_path):
    """The route of tests/test_estimator_abi.py on csrc/lg_train.hip."""
    obj, fat, co = (str(tmp_path / n) for n in ("lg_train.o", "fat.bin", "k.co"))
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-fno-slp-vectorize", "-c", "-o", obj,
                    os.path.join(CSRC, "lg_train.hip")], check=True, capture_output=True)
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
    kernels = ("ppo_forward_kernel", "ppo_loss_kernel", "ppo_loss_finish_kernel", "ppo_backward_kernel", "ppo_wgrad_kernel", "ppo_grad_reduce_kernel",
               "ppo_norm_finish_kernel", "ppo_adam_kernel", "ppo_stats_kernel")
    for part in kernels:
        hit = [v for k, v in blocks.items() if part in k]
        assert len(hit) == 1, (part, sorted(blocks))
        r = hit[0]
        print(part, r)
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0 and r["private_segment_fixed_size"] == 0, (part, r)
        bound = LDS_OWNER if part in ("ppo_forward_kernel", "ppo_backward_kernel") else LDS_SHARED
        assert r["group_segment_fixed_size"] <= bound, (part, r)
