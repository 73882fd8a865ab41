"""CPU side of the native terrain-estimator update (include/lgestimator_train.h): the header names, the library's exports and the ctypes mirror
agree and are disjoint from the other headers' lists; the struct layouts match a C compiler's; one refused call per entry point leaves a message that
starts with that entry point's name; the Python layer's refusals (loss type with the reference's text, multi_gpu_cfg, a bf16 encoder) need no GPU; the
new kernels' code-object metadata (cross-compiled for gfx950) shows no spills, no scratch, and LDS within the 80 KB tests/test_train_abi.py allows a
workgroup that shares its compute unit (none of the new kernels is a 512-lane tile kernel).  No GPU needed."""
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
HEADER = os.path.join(ROOT, "include", "lgestimator_train.h")
LDS_SHARED = 80 * 1024
KERNELS = ("est_dgrad_kernel", "est_pool_backward_kernel", "est_act_delta_kernel", "est_conv_wgrad_kernel", "est_conv_retile_kernel")


def _msg(lib):
    return (lib.lg_mlp_last_error(None) or b"").decode()


def test_header_exports_and_declarations_agree():
    names = sorted(set(re.findall(r"\b(lg_[a-z_]+)\(", open(HEADER).read())))
    assert names == sorted(abi.ESTIMATOR_TRAIN_SYMBOLS), (names, abi.ESTIMATOR_TRAIN_SYMBOLS)
    for other in (abi.TRAIN_SYMBOLS, abi.POLICY_SYMBOLS, abi.DISTILL_TRAIN_SYMBOLS, abi.TRAIN_RECURRENT_SYMBOLS, abi.ESTIMATOR_SYMBOLS, abi.ESTIMATOR_BF16_SYMBOLS,
                  abi.PRODUCT_SYMBOLS):
        assert not set(names) & set(other)
    assert all(n.startswith("lg_estimator_train_") for n in names)
    plain = abi.declare_distill_train(abi.declare_train(abi.declare_policy(C.CDLL(LIB))))
    for sym in names:
        assert hasattr(plain, sym), sym
        assert getattr(plain, sym).argtypes is None, f"another declare function declares {sym}"
    lib = abi.declare_estimator_train(C.CDLL(LIB))
    for sym in names:
        assert getattr(lib, sym).argtypes is not None, sym
    for other in ("lgpolicy.h", "lgtrain.h", "lgdistill.h", "lgtrain_recurrent.h"):
        assert not re.search(r"lg_estimator_train_[a-z_]+\(", open(os.path.join(ROOT, "include", other)).read()), other
    from extended_legged_gym_amd import rl
    assert hasattr(rl, "NativeEstimatorDistillation")
    assert lib.lg_estimator_train_wgrad_slab_rows() > 0


def test_struct_layouts_match_the_c_compiler(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or os.path.join(LLVM, "clang")
    structs = {"lg_estimator_train_hyper": abi.lg_estimator_train_hyper, "lg_estimator_train_stats": abi.lg_estimator_train_stats,
               "lg_estimator_train_params": abi.lg_estimator_train_params}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "lgestimator_train.h"', "int main(void) {"]
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
    assert re.search(r"LG_EST_LOSS_MSE = 0, LG_EST_LOSS_HUBER = 1, LG_EST_LOSS_L1 = 2", open(HEADER).read())
    assert abi.ESTIMATOR_LOSSES == {"mse": 0, "huber": 1, "l1": 2}


def test_one_refusal_per_entry_point_names_it():
    lib = abi.declare_estimator_train(abi.declare_policy(C.CDLL(LIB)))
    p = 0x1000          # never read: the NULL handle is refused first
    hyper = abi.lg_estimator_train_hyper(0, 1.0, 0)
    calls = {
        "lg_estimator_train_create": lambda: lib.lg_estimator_train_create(None, None, None, None, None, 1e-3, 64),
        "lg_estimator_train_group": lambda: lib.lg_estimator_train_group(None, p, p, p, None, 4, 8, 0, 3, 1, C.byref(hyper), None),
        "lg_estimator_train_update": lambda: lib.lg_estimator_train_update(None, p, p, p, None, 4, 8, 1, 3, C.byref(hyper), None, None),
        "lg_estimator_train_parameter_count": lambda: lib.lg_estimator_train_parameter_count(None),
        "lg_estimator_train_workspace_bytes": lambda: lib.lg_estimator_train_workspace_bytes(None),
        "lg_estimator_train_gradients": lambda: lib.lg_estimator_train_gradients(None, p, p, p, 3, None),
        "lg_estimator_train_forward_outputs": lambda: lib.lg_estimator_train_forward_outputs(None, p, None),
        "lg_estimator_train_step_losses": lambda: lib.lg_estimator_train_step_losses(None, p, 4, None),
        "lg_estimator_train_get_carry": lambda: lib.lg_estimator_train_get_carry(None, p, p, 4, 0, None),
        "lg_estimator_train_set_carry": lambda: lib.lg_estimator_train_set_carry(None, p, p, 4, None),
        "lg_estimator_train_reset_carry": lambda: lib.lg_estimator_train_reset_carry(None, None),
        "lg_estimator_train_get_parameters": lambda: lib.lg_estimator_train_get_parameters(None, p, None),
        "lg_estimator_train_get_state": lambda: lib.lg_estimator_train_get_state(None, p, p, p, None, None, None),
        "lg_estimator_train_set_state": lambda: lib.lg_estimator_train_set_state(None, p, p, p, 0, 1e-3, None),
        "lg_estimator_train_set_learning_rate": lambda: lib.lg_estimator_train_set_learning_rate(None, 1e-3, None),
    }
    # destroy cannot fail (NULL is a no-op) and the slab size takes no argument
    assert set(calls) | {"lg_estimator_train_destroy", "lg_estimator_train_wgrad_slab_rows"} == set(abi.ESTIMATOR_TRAIN_SYMBOLS)
    for name, call in calls.items():
        rc = call()
        assert (rc is None or rc == 0) if name == "lg_estimator_train_create" else rc == abi.LG_ERR_INVALID, (name, rc)
        assert _msg(lib).startswith(name + ": "), (name, _msg(lib))
    lib.lg_estimator_train_destroy(None)


def test_python_refusals_that_need_no_gpu():
    from extended_legged_gym_amd.rl import NativeEstimatorDistillation
    with pytest.raises(ValueError, match=r"Unknown loss type: smooth\. Supported types are: mse, huber, l1"):
        NativeEstimatorDistillation(None, {}, loss_type="smooth")
    with pytest.raises(NotImplementedError, match="multi_gpu_cfg"):
        NativeEstimatorDistillation(object(), {}, multi_gpu_cfg={"global_rank": 0, "world_size": 2})

    class Bf16:
        precision = "bf16"
    with pytest.raises(NotImplementedError, match="bf16"):
        NativeEstimatorDistillation(Bf16(), {})
    with pytest.raises(TypeError, match="NativeTerrainEstimator"):
        NativeEstimatorDistillation(object(), {})


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_estimator_train_kernels_do_not_spill_and_fit_the_lds(tmp_path):
    """The route of tests/test_train_abi.py on csrc/lg_estimator_train.hip."""
    obj, fat, co = (str(tmp_path / n) for n in ("lg_estimator_train.o", "fat.bin", "k.co"))
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-fno-slp-vectorize", "-c", "-o", obj,
                    os.path.join(CSRC, "lg_estimator_train.hip")], check=True, capture_output=True)
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
