"""CPU side of the native recurrent PPO update (include/lgtrain_recurrent.h), by the route of tests/test_train_abi.py: the header names, the
library's exports and the ctypes mirror agree and are disjoint from the other lists; the struct layout matches a C compiler's; one refused call per
entry point leaves a message that starts with that entry point's name; the kernels of csrc/lg_train_recurrent.hip, cross-compiled for gfx950, use no
scratch and fit the LDS: the three 32-row tile kernels (512 lanes, a workgroup that owns its compute unit) are held to the 128 KB the inference
memory kernel already lives in, the two element-wise kernels to the 80 KB of a workgroup that shares its compute unit.  No GPU needed."""
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
HEADER = os.path.join(ROOT, "include", "lgtrain_recurrent.h")
LDS_OWNER, LDS_SHARED = 128 * 1024, 80 * 1024
TILE_KERNELS = ("rnn_train_forward_kernel", "rnn_backward_kernel", "rows_matmul_kernel")


def _msg(lib):
    return (lib.lg_mlp_last_error(None) or b"").decode()


def test_header_exports_and_declarations_agree():
    names = sorted(set(re.findall(r"\b(lg_[a-z_]+)\(", open(HEADER).read())))
    assert names == sorted(abi.TRAIN_RECURRENT_SYMBOLS), (names, abi.TRAIN_RECURRENT_SYMBOLS)
    others = set(abi.POLICY_SYMBOLS) | set(abi.TRAIN_SYMBOLS) | set(abi.DISTILL_TRAIN_SYMBOLS) | set(abi.PRODUCT_SYMBOLS)
    assert not others & set(names)
    plain = abi.declare_distill_train(abi.declare_train(abi.declare_policy(C.CDLL(LIB))))
    for sym in names:
        assert hasattr(plain, sym), sym
        assert getattr(plain, sym).argtypes is None, f"another declare_* declares {sym}"
    lib = abi.declare_train_recurrent(C.CDLL(LIB))
    for sym in names:
        assert getattr(lib, sym).argtypes is not None, sym
    for other in ("lgpolicy.h", "lgtrain.h"):
        assert not re.search(r"lg_ppo_recurrent_[a-z_]+\(", open(os.path.join(ROOT, "include", other)).read())
    from extended_legged_gym_amd import rl
    assert hasattr(rl, "NativeRecurrentPPO") and issubclass(rl.NativeRecurrentPPO, rl.NativePPO)


def test_struct_layout_matches_the_c_compiler(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or os.path.join(LLVM, "clang")
    name, cls = "lg_ppo_recurrent_params", abi.lg_ppo_recurrent_params
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "lgtrain_recurrent.h"', "int main(void) {", f'  printf("{name} %zu\\n", sizeof({name}));']
    for field, _ in cls._fields_:
        lines.append(f'  printf("{name}.{field} %zu\\n", offsetof({name}, {field}));')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True, capture_output=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got[name]) == C.sizeof(cls)
    for field, _ in cls._fields_:
        assert int(got[f"{name}.{field}"]) == getattr(cls, field).offset, field


def test_one_refusal_per_entry_point_names_it():
    lib = abi.declare_train_recurrent(abi.declare_policy(C.CDLL(LIB)))
    p = 0x1000          # never read: the NULL handle is refused first
    rows, hyper = abi.lg_ppo_rows(*[p] * 9), abi.lg_ppo_hyper(0.2, 1.0, 0.0, 1, 1.0, 0, 0.01)
    hid, params = abi.lg_rollout_hidden(p, p, p, p), abi.lg_ppo_recurrent_params()
    pre = "lg_ppo_recurrent_"
    calls = {
        "create": lambda: lib.lg_ppo_recurrent_create(None, None, None, None, C.byref(params), 0, 1e-3, 64, p),
        "minibatch": lambda: lib.lg_ppo_recurrent_minibatch(None, C.byref(rows), C.byref(hid), p, 4, 8, 0, 8, C.byref(hyper), None),
        "update": lambda: lib.lg_ppo_recurrent_update(None, C.byref(rows), C.byref(hid), p, 4, 8, 1, 1, C.byref(hyper), None, None),
        "parameter_count": lambda: lib.lg_ppo_recurrent_parameter_count(None),
        "workspace_bytes": lambda: lib.lg_ppo_recurrent_workspace_bytes(None),
        "gradients": lambda: lib.lg_ppo_recurrent_gradients(None, p, p, p, None),
        "forward_outputs": lambda: lib.lg_ppo_recurrent_forward_outputs(None, p, p, None),
        "get_parameters": lambda: lib.lg_ppo_recurrent_get_parameters(None, p, None),
        "get_state": lambda: lib.lg_ppo_recurrent_get_state(None, p, p, p, None, None, None),
        "set_state": lambda: lib.lg_ppo_recurrent_set_state(None, p, p, p, 0, 1e-3, None),
        "set_learning_rate": lambda: lib.lg_ppo_recurrent_set_learning_rate(None, 1e-3, None),
        "get_images": lambda: lib.lg_ppo_recurrent_get_images(None, 0, 0, p, p, None),
    }
    assert {pre + k for k in calls} | {pre + "destroy"} == set(abi.TRAIN_RECURRENT_SYMBOLS)          # destroy cannot fail: NULL is a no-op
    for name, call in calls.items():
        rc = call()
        assert (rc is None or rc == 0) if name == "create" else rc == abi.LG_ERR_INVALID, (name, rc)
        assert _msg(lib).startswith(pre + name + ": "), (name, _msg(lib))
    lib.lg_ppo_recurrent_destroy(None)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_recurrent_train_kernels_do_not_spill_and_fit_the_lds(tmp_path):
    obj, fat, co = (str(tmp_path / n) for n in ("lg_train_recurrent.o", "fat.bin", "k.co"))
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-fno-slp-vectorize", "-c", "-o", obj,
                    os.path.join(CSRC, "lg_train_recurrent.hip")], check=True, capture_output=True)
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
    for part in TILE_KERNELS + ("rnn_retile_kernel", "rec_index_kernel"):
        hit = [v for k, v in blocks.items() if part in k]
        assert len(hit) == 1, (part, sorted(blocks))
        r = hit[0]
        print(part, r)
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0 and r["private_segment_fixed_size"] == 0, (part, r)
        assert r["group_segment_fixed_size"] <= (LDS_OWNER if part in TILE_KERNELS else LDS_SHARED), (part, r)
