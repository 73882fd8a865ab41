"""CPU side of the symmetric PPO trainer (include/lgtrain_symmetry.h), the pattern of tests/test_train_abi.py: the header names, the library's exports
and the ctypes mirror agree; the struct layouts match a C compiler's; one refused call per entry point leaves a message that starts with that entry
point's name; the new unit's kernels (cross-compiled for gfx950) show no spills, no scratch, and LDS within the same two bounds: the 32-row forward
tile (a workgroup that owns its compute unit) within 128 KB, every other kernel within 80 KB.  No GPU needed."""
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
HEADER = os.path.join(ROOT, "include", "lgtrain_symmetry.h")
LDS_OWNER, LDS_SHARED = 128 * 1024, 80 * 1024


def _msg(lib):
    return (lib.lg_mlp_last_error(None) or b"").decode()


def test_header_exports_and_declarations_agree():
    text = open(HEADER).read()
    names = sorted(set(re.findall(r"\b(lg_[a-z_]+)\(", text)))
    assert names == sorted(abi.SYMMETRY_TRAIN_SYMBOLS), (names, abi.SYMMETRY_TRAIN_SYMBOLS)
    assert all(n.startswith("lg_ppo_sym_") for n in names)
    for other in (abi.TRAIN_SYMBOLS, abi.POLICY_SYMBOLS, abi.TRAIN_RECURRENT_SYMBOLS, abi.DISTILL_TRAIN_SYMBOLS, abi.DISTILL_RTRAIN_SYMBOLS,
                  abi.ESTIMATOR_TRAIN_SYMBOLS, abi.PRODUCT_SYMBOLS):
        assert not set(names) & set(other)
    plain = abi.declare_train(abi.declare_policy(C.CDLL(LIB)))
    for sym in names:
        assert hasattr(plain, sym), sym
        assert getattr(plain, sym).argtypes is None, f"another declare function declares {sym}"
    lib = abi.declare_train_symmetry(C.CDLL(LIB))
    for sym in names:
        assert getattr(lib, sym).argtypes is not None, sym
    assert int(re.search(r"#define\s+LG_PPO_SYM_MAX_BLOCKS\s+(\d+)", text).group(1)) == abi.SYMMETRY_MAX_BLOCKS == 4
    from extended_legged_gym_amd import rl
    assert hasattr(rl, "NativeSymmetricPPO") and hasattr(rl, "signed_permutation_tables")


def test_struct_layouts_match_the_c_compiler(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or os.path.join(LLVM, "clang")
    structs = {"lg_ppo_sym_tables": abi.lg_ppo_sym_tables, "lg_ppo_sym_config": abi.lg_ppo_sym_config, "lg_ppo_sym_stats": abi.lg_ppo_sym_stats}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "lgtrain_symmetry.h"', "int main(void) {"]
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
    # lg_ppo_stats plus one double: an lg_ppo_stats reader sees its five fields where it expects them
    assert [f for f, _ in abi.lg_ppo_sym_stats._fields_][:5] == [f for f, _ in abi.lg_ppo_stats._fields_]
    assert C.sizeof(abi.lg_ppo_sym_stats) == C.sizeof(abi.lg_ppo_stats) + 8


def test_one_refusal_per_entry_point_names_it():
    lib = abi.declare_train_symmetry(abi.declare_policy(C.CDLL(LIB)))
    p = 0x1000          # never read: the NULL handle is refused first
    rows, hyper = abi.lg_ppo_rows(*[p] * 9), abi.lg_ppo_hyper(0.2, 1.0, 0.0, 1, 1.0, 0, 0.01)
    pre = "lg_ppo_sym_"
    calls = {
        "create": lambda: lib.lg_ppo_sym_create(None, None, None, None, None, None, p, 0, 1e-3, 64, p, None, None),
        "minibatch": lambda: lib.lg_ppo_sym_minibatch(None, C.byref(rows), p, 8, C.byref(hyper), None),
        "update": lambda: lib.lg_ppo_sym_update(None, C.byref(rows), 8, p, 1, 1, C.byref(hyper), None, None),
        "parameter_count": lambda: lib.lg_ppo_sym_parameter_count(None),
        "gradients": lambda: lib.lg_ppo_sym_gradients(None, p, p, p, p, None),
        "forward_outputs": lambda: lib.lg_ppo_sym_forward_outputs(None, p, p, None),
        "get_parameters": lambda: lib.lg_ppo_sym_get_parameters(None, p, None),
        "get_state": lambda: lib.lg_ppo_sym_get_state(None, p, p, p, None, None, None),
        "set_state": lambda: lib.lg_ppo_sym_set_state(None, p, p, p, 0, 1e-3, None),
        "set_learning_rate": lambda: lib.lg_ppo_sym_set_learning_rate(None, 1e-3, None),
    }
    assert {pre + k for k in calls} | {pre + "destroy"} == set(abi.SYMMETRY_TRAIN_SYMBOLS)          # destroy cannot fail: NULL is a no-op
    for name, call in calls.items():
        rc = call()
        assert (rc is None or rc == 0) if name == "create" else rc == abi.LG_ERR_INVALID, (name, rc)
        assert _msg(lib).startswith(pre + name + ": "), (name, _msg(lib))
    lib.lg_ppo_sym_destroy(None)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_symmetry_kernels_do_not_spill_and_fit_the_lds(tmp_path):
    """The route of tests/test_train_abi.py on csrc/lg_train_symmetry.hip."""
    obj, fat, co = (str(tmp_path / n) for n in ("lg_train_symmetry.o", "fat.bin", "k.co"))
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-fno-slp-vectorize", "-c", "-o", obj,
                    os.path.join(CSRC, "lg_train_symmetry.hip")], check=True, capture_output=True)
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
    kernels = ("sym_fwd_kernel", "sym_loss_kernel", "sym_loss_finish_kernel", "sym_wgrad_kernel", "sym_stats_kernel")
    existing = ("ppo_forward_kernel", "ppo_loss_kernel", "ppo_loss_finish_kernel", "ppo_backward_kernel", "ppo_wgrad_kernel", "ppo_grad_reduce_kernel",
                "ppo_norm_finish_kernel", "ppo_adam_kernel", "ppo_stats_kernel")
    assert len(blocks) == len(kernels), sorted(blocks)
    for name in blocks:          # tests/test_train_abi.py finds lg_train.hip's kernels by substring: no new kernel may carry one of their names
        assert not any(e in name for e in existing), name
    for part in kernels:
        hit = [v for k, v in blocks.items() if part in k]
        assert len(hit) == 1, (part, sorted(blocks))
        r = hit[0]
        print(part, r)
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0 and r["private_segment_fixed_size"] == 0, (part, r)
        assert r["group_segment_fixed_size"] <= (LDS_OWNER if part == "sym_fwd_kernel" else LDS_SHARED), (part, r)
