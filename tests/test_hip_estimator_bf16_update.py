"""`NativeEstimatorDistillation(encoder_training="bf16")` (include/lgestimator_train_bf16.h) on the GPU against the rule of
tests/estimator_bf16_update_rule.py.

Group gradients: every tensor's gradient and the global norm against the float64 rule reference, within max(4 y, 2e-5): y is the error of the fp32
emulation of the same rule (map-shaped deltas through R) against that reference for the same tensor, computed here on the CPU; 4 is the project's
multiplier over a torch yardstick.  tests/test_estimator_bf16_update_rule.py shows that a trainer which differentiates the fp32 function instead lies
outside.  Step losses within the fp32 bar max(8 e32, 2e-5) of tests/test_hip_estimator_update.py, e32 the emulation's own loss error.  Predictions bit
equal to `act_inference` of the bf16 estimator.  This shows the chain is wired; tests/test_hip_estimator_bf16_stages.py holds the arithmetic of each
kernel.  Every figure is printed before it is asserted."""
import pytest
import torch

from tests import estimator_bf16_update_rule as rule
from tests import estimator_update_reference as ref
from tests import ppo_reference as pref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib():
    from extended_legged_gym_amd import abi
    from extended_legged_gym_amd.rl.estimator_distillation import _estimator_train_lib
    return abi.declare(_estimator_train_lib(), "estimator_train_bf16")


def _slab():
    return int(_lib().lg_estimator_bf16train_wgrad_slab_rows())


def _estimator(case, state, precision="bf16"):
    from extended_legged_gym_amd.rl import NativeTerrainEstimator
    return NativeTerrainEstimator(state, case.shape, case.P, activation=case.act, memory_type=case.memory, device=DEV, encoder_precision=precision)


def _build(case, state=None, precision="bf16", **kw):
    from extended_legged_gym_amd.rl import NativeEstimatorDistillation
    state = state or case.state()
    est = _estimator(case, state, precision)
    kw.setdefault("gradient_length", case.G)
    kw.setdefault("loss_type", case.loss)
    return est, NativeEstimatorDistillation(est, state, encoder_training=precision, **kw)


def _cuda(rows):
    return {k: v.to(DEV) for k, v in rows.items()}


def _dev(state):
    return tuple(s.to(DEV) for s in state) if isinstance(state, tuple) else state.to(DEV)


def _rel(got, want):
    return abs(float(got) - float(want)) / abs(float(want))


def _within(name, e, y, mult, tag):
    bar = max(mult * y, 2e-5)
    print(f"{name}: e {e:.3e}  {tag} {y:.3e}  bar {bar:.3e}")
    return e <= bar


# ------------------------------------------------------------------------------------------------------------ 1. one group against the rule
@pytest.mark.parametrize("case", ref.group_cases() + [ref.slab_case(8192)], ids=lambda c: c.name)
def test_group_gradients_against_the_rule(case):
    if case.name == "9x11_slabs":
        case = ref.slab_case(_slab())
    use_dones, carry, rows = bool(case.dones_at), ref.carry_of(case), case.rows()
    g64, n64, l64, p64, _ = rule.group_gradients(case, torch.float64, carry=carry, use_dones=use_dones)
    g32, n32, l32, _, _ = rule.group_gradients(case, torch.float32, round_deltas=True, carry=carry, use_dones=use_dones)
    assert all(float(g.abs().max()) > 0 for g in g64.values())
    est, alg = _build(case, use_dones=use_dones)
    alg.set_hidden_states(carry)
    alg.group(_cuda(rows), 0, case.G)
    grads, norm, losses = alg.gradients()
    preds = alg.forward_outputs().view(case.G, case.N, case.R)
    ok = True
    for k in g64:
        ok &= _within(f"{case.name} {k}", ref.err(grads[k], g64[k]), ref.err(g32[k], g64[k]), 4.0, "y")
    ok &= _within(f"{case.name} norm", _rel(norm, n64), _rel(n32, n64), 4.0, "y")
    for s in range(case.G):
        ok &= _within(f"{case.name} loss[{s}]", _rel(losses[s], l64[s]), _rel(l32[s], l64[s]), 8.0, "e32")
    print(f"{case.name} predictions vs the float64 rule: {ref.err(preds, p64):.3e}")
    # the same rows through the inference kernels of a second bf16 estimator with the weights the group started from
    live = _estimator(case, case.state())
    live.set_hidden_states(_dev(carry))
    crows = _cuda(rows)
    for s in range(case.G):
        out = live.act_inference(crows["depth_images"][s], crows["proprio_data"][s])
        assert torch.equal(out.cpu(), preds[s]), f"step {s}: the trainer's forward is not the bf16 estimator's act_inference bit for bit"
        if use_dones:
            live.reset(crows["dones"][s])
    for part in (alg, est, live):
        part.close()
    assert ok


# ------------------------------------------------------------------------------------------------------------ 2. the optimiser step
def _ulp(t):
    t = t.double().abs()
    return torch.where(t > 0, 2.0 ** (torch.floor(torch.log2(t.clamp_min(1e-300))) - 23), torch.full_like(t, 2.0 ** -149))


@pytest.mark.parametrize("max_grad_norm", [ref.CLIP_SMALL, ref.CLIP_LARGE, None])
def test_optimiser_step_on_the_kernels_own_gradients(max_grad_norm):
    """`clip_and_adam` in float64 on the gradients the kernels produced, from loaded non-zero moments at step 7: the fp32 masters within 1e-5 lr + 1 ulp,
    moments within 1e-6 relative (the tolerances of tests/test_hip_estimator_update.py)."""
    case = ref.Case(**ref.OPT_CASE)
    lr, params = 2.5e-3, case.state()
    est, alg = _build(case, learning_rate=lr, max_grad_norm=max_grad_norm)
    g = torch.Generator().manual_seed(8)
    state = dict(parameters=params, exp_avg={k: 0.01 * torch.randn(v.shape, generator=g) for k, v in params.items()},
                 exp_avg_sq={k: 1e-4 * torch.rand(v.shape, generator=g) for k, v in params.items()}, step=7, learning_rate=lr)
    alg.load_optimizer_state(state)
    back = alg.optimizer_state()
    assert back["step"] == 7 and back["learning_rate"] == lr
    for k in params:          # the masters are fp32: what was loaded comes back, not its bf16 rounding
        assert torch.equal(back["parameters"][k], params[k]) and torch.equal(back["exp_avg"][k], state["exp_avg"][k]), k
    alg.group(_cuda(case.rows()), 0, case.G)
    grads, norm, _ = alg.gradients()
    print("norm", norm, "max_grad_norm", max_grad_norm)
    assert ref.CLIP_SMALL < norm < ref.CLIP_LARGE
    want, wstate = pref.clip_and_adam(params, grads, dict(exp_avg=state["exp_avg"], exp_avg_sq=state["exp_avg_sq"], step=7), lr,
                                      max_grad_norm if max_grad_norm else float("inf"))
    after = alg.optimizer_state()
    assert after["step"] == 8
    worst = 0.0
    for k in params:
        tol = 1e-5 * lr + _ulp(want[k])
        worst = max(worst, float(((after["parameters"][k].double() - want[k]).abs() / tol).max()))
        for moment in ("exp_avg", "exp_avg_sq"):
            assert float((after[moment][k].double() - wstate[moment][k]).abs().max()) <= 1e-6 * float(wstate[moment][k].abs().max()) + 1e-12, (moment, k)
    print("largest |theta - theta64| / (1e-5 lr + 1 ulp):", worst)
    alg.close(); est.close()
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------------ 3. after an update
def _state_equal(a, b):
    assert a["step"] == b["step"] and a["learning_rate"] == b["learning_rate"]
    for part in ("parameters", "exp_avg", "exp_avg_sq"):
        for k in a[part]:
            assert torch.equal(a[part][k], b[part][k]), (part, k)


def _states_equal(a, b):
    for x, y in zip(ref._each(a), ref._each(b)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("memory", ["gru", "lstm"])
def test_update_is_deterministic_equals_the_loop_of_groups_and_moves_the_live_estimator(memory):
    case = ref.Case(memory=memory, **ref.UPDATE_CASE)
    E, T, G, rows = 2, case.T, case.G, _cuda(case.rows())
    kw = dict(num_learning_epochs=E, learning_rate=4e-3, max_grad_norm=0.5, loss_type="huber")
    (est1, one), (est2, two), (est3, loop) = (_build(case, **kw) for _ in range(3))
    loss1, loss2 = one.update(rows), two.update(rows)
    for first, n in ((0, G), (G, G)):
        loop.group(rows, first, n)
    loop.group(rows, 2 * G, E * T - 2 * G, train=False)
    loop.set_hidden_states(loop.get_hidden_states(running=True))
    assert loss1 == loss2 and one.optimizer_steps == 2
    assert torch.equal(one.step_losses(), two.step_losses())
    for other in (two, loop):
        _state_equal(one.optimizer_state(), other.optimizer_state())
        _states_equal(one.get_hidden_states(), other.get_hidden_states())
    sd = one.state_dict()
    assert any(not torch.equal(sd[k], v) for k, v in case.state().items())          # the update moved the masters
    # the trained object, a fresh bf16 estimator from state_dict() and the estimator of a reloaded trainer act with equal bits
    fresh = _estimator(case, sd)
    est4, again = _build(case, **kw)
    again.load_state_dict(sd)
    outs = []
    for e in (est1, fresh, est4):
        e.reset()
        outs.append([e.act_inference(rows["depth_images"][t], rows["proprio_data"][t]).cpu() for t in range(2)])
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)
    for part in (one, two, loop, again, est1, est2, est3, est4, fresh):
        part.close()


# ------------------------------------------------------------------------------------------------------------ 4. workspace; the fp32 trainer beside
def test_workspace_saves_two_bytes_per_map_element():
    case = ref.Case("28x56_ws", (28, 56), 4, 2)
    max_rows = 8
    est16, alg16 = _build(case, max_rows=max_rows)
    est32, alg32 = _build(case, precision="fp32", max_rows=max_rows)
    maps = sum(est16.encoder.stage_shape(k)[0] for k in (1, 2, 3, 4))
    w32, w16 = alg32.workspace_bytes(), alg16.workspace_bytes()
    print("workspace fp32", w32, "bf16", w16, "difference", w32 - w16, "2 x rows x map elements", 2 * max_rows * maps)
    for part in (alg16, alg32, est16, est32):
        part.close()
    assert w32 - w16 >= 2 * max_rows * maps


def test_fp32_trainer_beside_a_bf16_one_gives_the_gradients_it_gives_alone():
    case = ref.Case("9x11_beside", (9, 11), 3, 2, salt=11)
    rows = _cuda(case.rows())

    def fp32_grads():
        est, alg = _build(case, precision="fp32")
        alg.group(rows, 0, case.G)
        g = alg.gradients()
        alg.close(); est.close()
        return g

    alone = fp32_grads()
    est16, alg16 = _build(case)
    alg16.group(rows, 0, case.G)
    beside = fp32_grads()
    alg16.close(); est16.close()
    assert alone[1] == beside[1] and alone[2] == beside[2]
    for k in alone[0]:
        assert torch.equal(alone[0][k], beside[0][k]), k
