"""What the bf16 tests of the depth encoder share (tests/test_encoder_bf16_cpu.py, tests/test_hip_encoder_bf16.py): the rounding R, the bf16-operand
reference of one stage, its bar and the acceptance interval.  Shapes, inputs, weights, `run_stage` and the bar rule come from
tests/test_encoder_reference_power.py; nothing is copied from it.

R(v): v rounded to bf16, nearest even, by torch's cast on the CPU.  For stage 7 (fp32 features) R is the identity.
Reference of stage k: `run_stage` on a float64 copy of the module whose layer WEIGHTS went through R (biases not), on the native encoder's own
    stage k - 1 output (for k = 1: the image through R).  Call it u.  Feeding every stage the kernel's own previous output keeps one rounding flip
    from spreading into the later stages; what is left is the fp32 accumulation difference.
Bar of stage k: max(FLOOR, 4 x gap_k), gap_k = torch fp32 against float64 for that same stage on those same bf16-rounded operands: the rule of
    tests/test_hip_estimator.py.
Acceptance: every entry of the native stage-k output lies in [R(u - bar_k), R(u + bar_k)]: the neighbouring bf16 value is accepted only where the
    exact value is within bar_k of a rounding boundary."""
import copy

import numpy as np
import torch

from tests.test_encoder_reference_power import FLOOR, STAGE_NAMES, run_stage


def rne_bf16_bits(x):
    """fp32 -> the 16 bits of bf16, round to nearest even, by integer arithmetic on the fp32 pattern (NaN is not handled: no caller has one)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def R(v):
    """v (CPU tensor) through bf16 and back to its own dtype."""
    return v.to(torch.bfloat16).to(v.dtype)


def bf16_operand_pair(m32):
    """(fp32, float64) copies of the module whose depth-encoder weights went through R; biases and everything behind the encoder untouched."""
    r32 = copy.deepcopy(m32)
    with torch.no_grad():
        for layer in r32.depth_encoder:
            if hasattr(layer, "weight"):
                layer.weight.copy_(R(layer.weight))
    return r32, copy.deepcopy(r32).double()


def stage_reference(r32, r64, k, x, **fault):
    """(u, gap_k, bar_k) of stage k on its input x (float32 values that are bf16-representable; (n, 1, h, w) for k = 1)."""
    with torch.no_grad():
        u = run_stage(r64, k, x.double(), **fault)
        gap = float((run_stage(r32, k, x.float()).double() - run_stage(r64, k, x.double())).abs().max())
    return u, gap, max(FLOOR, 4.0 * gap)


def interval(u, bar, k):
    lo, hi = u - bar, u + bar
    return (lo, hi) if k == 7 else (R(lo), R(hi))


def outside(got, u, bar, k):
    """Boolean mask of the entries of `got` outside the acceptance interval (non-finite entries count as outside)."""
    lo, hi = interval(u, bar, k)
    got = got.double()
    return ~((got >= lo) & (got <= hi)) | ~torch.isfinite(got)


def check_interval(tag, got, u, bar, gap, k):
    """Assert the acceptance rule; the one failure report.  got / u: (n, C, H, W) maps or (rows, width).  Returns the worst |got - u| / bar."""
    got, u = got.detach().double().cpu(), u.detach().double().cpu()
    assert got.shape == u.shape, (tag, k, tuple(got.shape), tuple(u.shape))
    bad = outside(got, u, bar, k)
    diff = (got - u).abs()
    diff[~torch.isfinite(got)] = float("inf")
    print(f"{tag} stage {k} ({STAGE_NAMES[k - 1]}): max |got - u| {float(diff.max()):.3e}  gap {gap:.3e}  bar {bar:.3e}  outside {int(bad.sum())} of {bad.numel()}")
    if bool(bad.any()):
        lo, hi = interval(u, bar, k)
        idx = np.unravel_index(int((diff * bad).argmax()), tuple(diff.shape))
        if got.dim() == 4:
            e, c, y, x = (int(v) for v in idx)
            where = f"env {e} (y, x, channel) = ({y}, {x}, {c}) of a {got.shape[2]} x {got.shape[3]} map, " + \
                    ("on its border" if y in (0, got.shape[2] - 1) or x in (0, got.shape[3] - 1) else "interior")
        else:
            where = f"env {int(idx[0])} of {got.shape[0]}, column {int(idx[1])} of {got.shape[1]}"
        raise AssertionError(f"{tag} stage {k} ({STAGE_NAMES[k - 1]}): {int(bad.sum())} entries outside; worst at {where}: got {float(got[idx])!r}, "
                             f"interval [{float(lo[idx])!r}, {float(hi[idx])!r}] (u {float(u[idx])!r}, bar {bar:.3e}, gap {gap:.3e})")
    return float(diff.max()) / bar
