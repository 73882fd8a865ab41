"""CPU side of the native distillation update (include/lgdistill.h): the header names, the library's exports and the ctypes mirror agree and are
disjoint from the other headers' lists; the struct layouts match a C compiler's; one refused call per entry point leaves a message that starts with
that entry point's name; the Python layer's bad-loss-type refusal carries the reference's text; the new kernels' code-object metadata
(cross-compiled for gfx950) shows no spills, no scratch, and LDS within the 80 KB tests/test_train_abi.py allows a workgroup that shares its compute
unit (none of the new kernels is a 512-lane tile kernel).  No GPU needed."""
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
HEADER = os.path.join(ROOT, "include", "lgdistill.h")
LDS_SHARED = 80 * 1024
KERNELS = ("seq_rows_kernel", "seq_loss_kernel", "seq_loss_finish_kernel", "seq_stats_kernel", "seq_mask_rows_kernel")


def _msg(lib):
    return (lib.lg_mlp_last_error(None) or b"").decode()


def test_header_exports_and_declarations_agree():
    names = sorted(set(re.findall(r"\b(lg_[a-z_]+)\(", open(HEADER).read())))
    assert names == sorted(abi.DISTILL_TRAIN_SYMBOLS), (names, abi.DISTILL_TRAIN_SYMBOLS)
    assert not set(names) & set(abi.TRAIN_SYMBOLS) and not set(names) & set(abi.POLICY_SYMBOLS)
    assert all(n.startswith("lg_distill_train_") for n in names)
    plain = abi.declare_train(abi.declare_policy(C.CDLL(LIB)))
    for sym in names:
        assert hasattr(plain, sym), sym
        assert getattr(plain, sym).argtypes is None, f"declare_policy or declare_train declares {sym}"
    lib = abi.declare_distill_train(C.CDLL(LIB))
    for sym in names:
        assert getattr(lib, sym).argtypes is not None, sym
    for other in ("lgpolicy.h", "lgtrain.h"):
        assert not re.search(r"lg_distill_train_[a-z_]+\(", open(os.path.join(ROOT, "include", other)).read()), other
    from extended_legged_gym_amd import rl
    assert hasattr(rl, "NativeDistillation")


def test_struct_layouts_match_the_c_compiler(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or os.path.join(LLVM, "clang")
    structs = {"lg_distill_train_hyper": abi.lg_distill_train_hyper, "lg_distill_train_stats": abi.lg_distill_train_stats}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "lgdistill.h"', "int main(void) {"]
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
    assert re.search(r"LG_LOSS_MSE = 0, LG_LOSS_HUBER = 1", open(HEADER).read()) and abi.DISTILL_LOSSES == {"mse": 0, "huber": 1}


def test_one_refusal_per_entry_point_names_it():
    lib = abi.declare_distill_train(abi.declare_policy(C.CDLL(LIB)))
    p = 0x1000          # never read: the NULL handle is refused first
    hyper = abi.lg_distill_train_hyper(0, 1.0)
    calls = {
        "lg_distill_train_create": lambda: lib.lg_distill_train_create(None, None, None, 1e-3, 64),
        "lg_distill_train_group": lambda: lib.lg_distill_train_group(None, p, p, 4, 8, 0, 3, C.byref(hyper), None),
        "lg_distill_train_update": lambda: lib.lg_distill_train_update(None, p, p, 4, 8, 1, 3, C.byref(hyper), None, None),
        "lg_distill_train_parameter_count": lambda: lib.lg_distill_train_parameter_count(None),
        "lg_distill_train_gradients": lambda: lib.lg_distill_train_gradients(None, p, p, p, 3, None),
        "lg_distill_train_forward_outputs": lambda: lib.lg_distill_train_forward_outputs(None, p, None),
        "lg_distill_train_step_losses": lambda: lib.lg_distill_train_step_losses(None, p, 4, None),
        "lg_distill_train_get_parameters": lambda: lib.lg_distill_train_get_parameters(None, p, None),
        "lg_distill_train_get_state": lambda: lib.lg_distill_train_get_state(None, p, p, p, None, None, None),
        "lg_distill_train_set_state": lambda: lib.lg_distill_train_set_state(None, p, p, p, 0, 1e-3, None),
        "lg_distill_train_set_learning_rate": lambda: lib.lg_distill_train_set_learning_rate(None, 1e-3, None),
    }
    assert set(calls) | {"lg_distill_train_destroy"} == set(abi.DISTILL_TRAIN_SYMBOLS)          # destroy cannot fail: NULL is a no-op
    for name, call in calls.items():
        rc = call()
        assert (rc is None or rc == 0) if name == "lg_distill_train_create" else rc == abi.LG_ERR_INVALID, (name, rc)
        assert _msg(lib).startswith(name + ": "), (name, _msg(lib))
    lib.lg_distill_train_destroy(None)


def test_python_refusals_that_need_no_gpu():
    from extended_legged_gym_amd.rl import NativeDistillation
    with pytest.raises(ValueError, match=r"Unknown loss type: l1\. Supported types are: mse, huber"):
        NativeDistillation(None, {}, loss_type="l1")

    class Recurrent:
        is_recurrent = True
    with pytest.raises(NotImplementedError, match="NativeStudentTeacherRecurrent"):
        NativeDistillation(Recurrent(), {})
    with pytest.raises(NotImplementedError, match="multi_gpu_cfg"):
        NativeDistillation(object(), {}, multi_gpu_cfg={"global_rank": 0, "world_size": 2})


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_distill_kernels_do_not_spill_and_fit_the_lds(tmp_path):
    """The route of tests/test_train_abi.py on csrc/lg_train_sequence.hip, where the kernels of the feed-forward trainer (which has none of its own) and the
    shared ones of the recurrent student's and the estimator's live."""
    obj, fat, co = (str(tmp_path / n) for n in ("lg_train_sequence.o", "fat.bin", "k.co"))
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-fno-slp-vectorize", "-c", "-o", obj,
                    os.path.join(CSRC, "lg_train_sequence.hip")], check=True, capture_output=True)
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
    assert len(blocks) == len(KERNELS), sorted(blocks)          # every kernel of the translation unit is held to the bounds
    for part in KERNELS:
        hit = [v for k, v in blocks.items() if part in k]
        assert len(hit) == 1, (part, sorted(blocks))
        r = hit[0]
        print(part, r)
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0 and r["private_segment_fixed_size"] == 0, (part, r)
        assert r["group_segment_fixed_size"] <= LDS_SHARED, (part, r)
