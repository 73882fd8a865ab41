"""CPU side of the recurrent student's native update: tests/distill_recurrent_reference.py (the float64 restatement the GPU test is held to) against
the reference's own record, and the power of the GPU test's bar.  No GPU needed.

1. The restatement in float64 reproduces tests/golden/distillation_recurrent_update.npz (the reference's `Distillation` + `StudentTeacherRecurrent`
   on torch-CPU, two collect-and-update rounds per case): step losses, the mean, the clip's norms, `student.*` / `memory_s.*` after both updates, the
   carry and the post-update hidden states.  Measured deviation in this container: 0.0 on every tensor of both cases and both rounds (bit-equal: the
   restatement performs the reference's float64 operations in the reference's order).  100 x that figure is a bar of zero, which would pin the BLAS's
   summation order rather than the semantics; the bar is 1e-12 relative (4500 float64 ulps), a thousand times tighter than the 1e-9 it may not
   exceed.  The restatement in fp32 stays within 8 x the golden's own fp32-vs-float64 figure, per tensor.
2. Each seeded fault of the restatement pushes at least one tensor over the GPU test's bar max(8 e32, 2e-5) -- for the two clip faults, over the
   optimiser-step test's 1e-5 lr + 1 ulp -- on the cases the GPU test uses, while the unfaulted fp32 run stays within it."""
import numpy as np
import pytest
import torch

from tests import distill_recurrent_reference as ref

F64_BAR = 1e-12
SLAB = 256          # WGRAD_SLAB of csrc/lg_train_internal.h; the GPU test takes it from the library


def _ulp(t):
    t = t.double().abs()
    return torch.where(t > 0, 2.0 ** (torch.floor(torch.log2(t.clamp_min(1e-300))) - 23), torch.full_like(t, 2.0 ** -149))


def _golden_case(name):
    G, cfg = ref.GOLDEN, ref.GOLDEN_CASES[name]
    return ref.Case(name, S=G["S"], H=G["H"], layers=G["layers"], mlp=G["mlp"], A=G["A"], N=G["N"], G=G["G"], T=G["T"], rnn=cfg["rnn"], loss=G["loss"])


def _replay(name, dtype, tag):
    """The restatement on the golden's inputs: per round {key: tensor} in the golden's names."""
    G, z, case = ref.GOLDEN, ref.golden(name), _golden_case(name)
    sd0 = ref.golden_state(z)
    model = case.module(dtype, {k: v for k, v in sd0.items() if k.startswith("student.") or k.startswith("memory_s.")})
    opt, carry, rounds = torch.optim.Adam(model.parameters(), lr=G["lr"]), None, []
    for r in range(G["rounds"]):
        res = ref.run_update(case, dtype, E=G["E"], G=G["G"], max_grad_norm=ref.CLIP_SMALL, carry=carry, model=model, optimizer=opt, rows=ref.golden_rows(z, r, tag),
                             record_norms=True)
        carry = res["carry"]
        got = {"step_losses": torch.tensor(res["losses"], dtype=torch.float64), "loss": torch.tensor(res["mean"], dtype=torch.float64),
               "norms": torch.tensor(res["norms"], dtype=torch.float64)}
        got.update({f"sd.{k}": v.detach().clone() for k, v in model.state_dict().items()})
        for k, v in ref.state_parts(carry).items():
            got[f"carry.{k}"] = v
            got[f"hidden_s.{k}"] = v          # the reference replays through the policy's own memory: its live state is the carry
        rounds.append(got)
    return z, rounds


@pytest.mark.parametrize("name", sorted(ref.GOLDEN_CASES))
def test_restatement_reproduces_the_references_float64_run(name):
    z, rounds = _replay(name, torch.float64, "f64")
    worst = 0.0
    for r, got in enumerate(rounds):
        assert int(z[f"r{r}.f64.hidden_t.present"]) == 0          # the teacher's memory is forgotten on every update, teacher_recurrent or not
        assert float(np.min(z[f"r{r}.f64.norms"])) > ref.CLIP_SMALL          # the clip bit in every optimiser step of the record
        for k, v in got.items():
            e = ref.err(v, z[f"r{r}.f64.{k}"])
            worst = max(worst, e)
            assert e <= F64_BAR, (name, r, k, e)
    print(f"{name}: largest float64 deviation from the reference's record {worst:.3e}")


@pytest.mark.parametrize("name", sorted(ref.GOLDEN_CASES))
def test_restatement_in_fp32_stays_within_the_goldens_own_figure(name):
    z, rounds = _replay(name, torch.float32, "f32")
    for r, got in enumerate(rounds):
        for k, v in got.items():
            want = z[f"r{r}.f64.{k}"]
            e, e32 = ref.err(v, want), ref.err(z[f"r{r}.f32.{k}"], want)
            print(f"{name} round {r} {k}: e {e:.3e}  golden fp32-vs-float64 {e32:.3e}")
            assert e <= 8.0 * e32 + 1e-300, (name, r, k, e, e32)


# ------------------------------------------------------------------------------------------------------------ the power of the GPU test's bar
def _over(faulted, clean64, clean32):
    """The tensors of `faulted` beyond the bar, and whether the unfaulted fp32 run is within it everywhere."""
    hit, clean_ok = [], True
    for k in clean64:
        e32 = ref.err(clean32[k], clean64[k])
        clean_ok &= e32 <= ref.bar(e32)
        if ref.err(faulted[k], clean64[k]) > ref.bar(e32):
            hit.append(k)
    return hit, clean_ok


def _update_tensors(res):
    out = {"losses": torch.tensor(res["losses"], dtype=torch.float64), **{k: v.detach() for k, v in res["model"].state_dict().items()}}
    out.update({"carry." + k: v for k, v in ref.state_parts(res["carry"]).items()})
    return out


@pytest.mark.parametrize("rnn", ["lstm", "gru"])
def test_group_faults_are_seen(rnn):
    """On the carry + dones group case: a gradient crossing a done row; the upper layer's weight_hh gradient missing the group's first step.  On
    the update case's second group entered after the first group's steps: a gradient crossing the group boundary.  Every gradient tensor of the
    unfaulted runs is non-zero."""
    case = ref.group_cases(SLAB, rnn)[3]
    assert case.name.endswith(ref.CARRY_CASE)
    carry = ref.carry_of(case)
    g64 = ref.group_gradients(case, torch.float64, carry=carry)[0]
    g32 = ref.group_gradients(case, torch.float32, carry=carry)[0]
    assert all(float(g.abs().max()) > 0 for g in g64.values())
    for fault in ("cross_done", "whh_first_step"):
        hit, clean_ok = _over(ref.group_gradients(case, torch.float64, carry=carry, faults={fault: True})[0], g64, g32)
        print(rnn, fault, "over the bar:", hit)
        assert hit and clean_ok, fault
        if fault == "whh_first_step":
            assert hit == [f"memory_s.rnn.weight_hh_l{case.layers - 1}"]
    up = ref.update_case(rnn)
    kw = dict(first_step=up.G, num_steps=up.G, pre_steps=up.G)
    b64, b32 = ref.group_gradients(up, torch.float64, **kw)[0], ref.group_gradients(up, torch.float32, **kw)[0]
    assert all(float(g.abs().max()) > 0 for g in b64.values())
    hit, clean_ok = _over(ref.group_gradients(up, torch.float64, faults={"no_detach": True}, **kw)[0], b64, b32)
    print(rnn, "no_detach over the bar:", hit)
    assert hit and clean_ok


@pytest.mark.parametrize("rnn", ["lstm", "gru"])
def test_update_faults_are_seen(rnn):
    """On the update case (E = 2, T = 7, G = 3): an epoch seeded from the previous epoch's end; the zeroing of a group's last step lost at the
    optimiser step's detach -- shown on the parameters after the update."""
    case = ref.update_case(rnn)
    kw = dict(E=ref.UPDATE_E, lr=ref.UPDATE_LR, max_grad_norm=ref.CLIP_SMALL)
    r64, r32 = ref.run_update(case, torch.float64, **kw), ref.run_update(case, torch.float32, **kw)
    assert r64["steps"] == 4 and ref.CLIP_SMALL < r64["grad_norm"] < ref.CLIP_LARGE
    c64, c32 = _update_tensors(r64), _update_tensors(r32)
    for fault in ("epoch_chain", "dones_before_detach"):
        hit, clean_ok = _over(_update_tensors(ref.run_update(case, torch.float64, faults={fault: True}, **kw)), c64, c32)
        print(rnn, fault, "over the bar:", hit)
        assert clean_ok and hit, fault
        if fault == "dones_before_detach":
            assert any(k.startswith("student.") or k.startswith("memory_s.") for k in hit)


@pytest.mark.parametrize("rnn", ["lstm", "gru"])
def test_clip_faults_are_seen_by_the_optimiser_step_check(rnn):
    """The GPU test's optimiser-step check (float64 `clip_and_adam` with the MLP-only rule from loaded moments at step 7, parameters within
    1e-5 lr + 1 ulp): the clip's norm taken over all parameters, and the clip's scale applied to memory_s.*, both leave it; the same step in fp32
    stays within it.  The clip bites."""
    case = ref.group_cases(SLAB, rnn)[0]
    lr, params = 2.5e-3, case.state()
    grads, (norm, mnorm), _, _, _ = ref.group_gradients(case, torch.float64)
    assert all(float(g.abs().max()) > 0 for g in grads.values())
    assert ref.CLIP_SMALL < norm < ref.CLIP_LARGE and mnorm > 0
    state = ref.seeded_moments(params)
    want, _, used = ref.student_clip_and_adam(params, grads, state, lr, ref.CLIP_SMALL)
    assert used == pytest.approx(norm, rel=1e-12)

    def worst(got, keys):
        return max(float(((got[k].double() - want[k]).abs() / (1e-5 * lr + _ulp(want[k]))).max()) for k in keys)

    fp32 = ref.student_clip_and_adam(params, {k: v.float() for k, v in grads.items()}, state, lr, ref.CLIP_SMALL, dtype=torch.float32)[0]
    print(rnn, "fp32 step, largest |theta - theta64| / tol:", worst(fp32, params))
    assert worst(fp32, params) <= 1.0
    memory = [k for k in params if k.startswith("memory_s.")]
    for fault in ("clip_all", "clip_memory"):
        got = ref.student_clip_and_adam(params, grads, state, lr, ref.CLIP_SMALL, faults={fault: True})[0]
        print(rnn, fault, "largest |theta - theta64| / tol:", worst(got, params), "on memory_s.*:", worst(got, memory))
        assert worst(got, params) > 1.0, fault
    assert worst(ref.student_clip_and_adam(params, grads, state, lr, ref.CLIP_SMALL, faults={"clip_memory": True})[0], memory) > 1.0


def test_every_group_case_has_gradients_everywhere():
    """The cases of the GPU group test: every gradient tensor is non-zero (the carry case enters from its seeded carry)."""
    for rnn in ("lstm", "gru"):
        for case in ref.group_cases(SLAB, rnn):
            carry = ref.carry_of(case) if case.name.endswith(ref.CARRY_CASE) or case.G == 1 else None
            grads = ref.group_gradients(case, torch.float64, carry=carry)[0]
            zero = [k for k, g in grads.items() if float(g.abs().max()) == 0]
            assert not zero, (case.name, zero)
