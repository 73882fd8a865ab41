"""The surface the six native trainers share, per trainer (both memory types for the three recurrent ones): checkpoints through `optimizer_state` /
`load_optimizer_state` / `load_state_dict`, the handle that regrows when an update brings more rows than it was built for, `set_learning_rate`
before and after the handle exists, and the carried memory state of the two trainers that keep one.  Everything is held to bit equality between
two trainers that ought to be in the same state: no reference and no tolerance.

Shapes: the feed-forward trainers see R = 24 x 13 = 312 rows (more than one 256-row weight-gradient slab, no multiple of 16) in 2 mini-batches (for
distillation: 2 groups of 12 steps per epoch); the trainers with a memory see T = 5 steps of N = 7 rows, two epochs, and (truncated BPTT) groups
of 3 steps: one full group, an epoch boundary inside the second, a remainder of one step; the estimator's image is the smallest the encoder takes."""
import pytest
import torch

from tests import distill_recurrent_reference as dref
from tests import distill_reference as fref
from tests import estimator_update_reference as eref
from tests import ppo_recurrent_reference as rref
from tests import ppo_reference as pref
from tests import ppo_symmetry_reference as sref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T_FF, N_FF = 24, 13
T_MEM, N_MEM, G_MEM, E_MEM = 5, 7, 3, 2
PPO_KW = dict(pref.HYPER, schedule="adaptive", desired_kl=0.004, entropy_coef=0.005, learning_rate=4e-3, num_learning_epochs=2, num_mini_batches=2)


def _cuda(rows):
    return {k: (v.to(DEV) if torch.is_tensor(v) else tuple(x.to(DEV) for x in v)) for k, v in rows.items()}


class _Setup:
    """One trainer kind: `build(max_rows)` -> (trainer, everything to close), fresh from the same seeded parameters every time; `rows`, on the
    device and never written; `update(alg, rows)`; `knob` / `small` / `full`: the public attribute whose value sets how many rows an update needs,
    a value for a first update that needs fewer rows and the value of every other update; `rows_needed(value)`."""
    carries = False

    def update(self, alg, rows=None):
        return alg.update(self.rows if rows is None else rows)


class _PPO(_Setup):
    knob, small, full = "num_mini_batches", 4, 2

    def __init__(self):
        from tests.test_hip_ppo_update import _random_sd
        self.sd, self.act = _random_sd([20, 32, 12], [24, 32, 1], 31), "elu"
        self.rows = _cuda(pref.craft_rows(self.sd, self.act, T_FF * N_FF, seed=32, kl_scale=0.02))
        self.perm = torch.randperm(T_FF * N_FF, generator=torch.Generator().manual_seed(33))

    def build(self, max_rows=None):
        from extended_legged_gym_amd.rl import NativeActorCritic, NativePPO
        policy = NativeActorCritic(self.sd, self.act, noise_std_type="scalar", device=DEV, seed=1)
        return NativePPO(policy, self.sd, max_rows=max_rows, **PPO_KW), [policy]

    def update(self, alg, rows=None):
        return alg.update(self.rows, self.perm)

    def rows_needed(self, value):
        return T_FF * N_FF // value


class _SymmetricPPO(_PPO):
    def __init__(self):
        super().__init__()
        self.sym = dict(sref.MODES["both"], data_augmentation_func=sref.synthetic_function((20, 24, 12), 2, 34), _env=None)

    def build(self, max_rows=None):
        from extended_legged_gym_amd.rl import NativeActorCritic, NativeSymmetricPPO
        policy = NativeActorCritic(self.sd, self.act, noise_std_type="scalar", device=DEV, seed=1)
        return NativeSymmetricPPO(policy, self.sd, symmetry_cfg=self.sym, max_rows=max_rows, **PPO_KW), [policy]


class _RecurrentPPO(_Setup):
    knob, small, full = "num_mini_batches", 3, 2          # env slices of 2, then of 3 envs (one env unused), over all T steps

    def __init__(self, rnn):
        self.rnn, self.act = rnn, "elu"
        self.sd = rref.random_params(rnn, 2, 40, 20, 24, [32, 16], [32, 16], 12, seed=41, std_key="std")
        ro = rref.craft_rollout(self.sd, self.act, rnn, T_MEM, N_MEM, seed=42)
        rows = {k: ro[k] for k in rref.ROW_KEYS}
        rows["dones"] = ro["dones"].unsqueeze(-1)
        for tag in ("a", "c"):
            rows["hidden_states_" + tag] = (ro["h_" + tag], ro["c_" + tag]) if ro["c_" + tag] is not None else ro["h_" + tag]
        self.rows = _cuda(rows)

    def build(self, max_rows=None):
        from extended_legged_gym_amd.rl import NativeActorCriticRecurrent, NativeRecurrentPPO
        policy = NativeActorCriticRecurrent(self.sd, self.act, self.rnn, noise_std_type="scalar", device=DEV, seed=1)
        return NativeRecurrentPPO(policy, self.sd, max_rows=max_rows, **PPO_KW), [policy]

    def rows_needed(self, value):
        return T_MEM * (N_MEM // value)


class _Distillation(_Setup):
    knob, small, full = "gradient_length", 6, 12

    def __init__(self):
        self.sd, self.act = fref.random_student([20, 32, 12], 51), "elu"
        self.rows = _cuda(fref.craft_rows(self.sd, self.act, T_FF, N_FF, seed=52))

    def build(self, max_rows=None):
        from extended_legged_gym_amd.rl import NativeDistillation, NativeStudentTeacher
        policy = NativeStudentTeacher(self.sd, self.act, device=DEV, seed=1)
        return NativeDistillation(policy, self.sd, num_learning_epochs=2, gradient_length=self.full, learning_rate=2e-3, max_grad_norm=1.0, loss_type="huber",
                                  max_rows=max_rows), [policy]

    def rows_needed(self, value):
        return value * N_FF


class _RecurrentDistillation(_Setup):
    knob, small, full, carries = "gradient_length", 2, G_MEM, True
    refusal = "lg_distill_rtrain_update: N is not the carry's number of rows"

    def __init__(self, rnn):
        from tests.test_hip_distill_recurrent_update import _full_state
        self.case = dref.Case("surface_" + rnn, N=N_MEM, G=G_MEM, T=T_MEM, rnn=rnn, salt=60, dones_at={1: None, 3: None})
        self.sd = _full_state(self.case)
        self.rows = _cuda(self.case.rows())

    def build(self, max_rows=None):
        from extended_legged_gym_amd.rl import NativeRecurrentDistillation
        from tests.test_hip_distill_recurrent_update import _policy
        policy = _policy(self.case, self.sd)
        return NativeRecurrentDistillation(policy, self.sd, num_learning_epochs=E_MEM, gradient_length=self.full, learning_rate=2e-3, max_grad_norm=1.0,
                                           loss_type="huber", max_rows=max_rows), [policy]

    def rows_needed(self, value):
        return value * N_MEM


class _Estimator(_Setup):
    knob, small, full, carries = "gradient_length", 2, G_MEM, True
    refusal = "lg_estimator_train_update: N is not the carry's number of rows"

    def __init__(self, memory):
        from extended_legged_gym_amd import abi
        side = abi.ENCODER_MIN_SIDE
        self.case = eref.Case("surface_" + memory, (side, side), N=N_MEM, G=G_MEM, T=T_MEM, memory=memory, layers=2, salt=70, dones_at=(1, 3))
        self.sd = self.case.state()
        self.rows = _cuda(self.case.rows())

    def build(self, max_rows=None):
        from extended_legged_gym_amd.rl import NativeEstimatorDistillation
        from tests.test_hip_estimator_update import _estimator
        est = _estimator(self.case, self.sd)
        return NativeEstimatorDistillation(est, self.sd, num_learning_epochs=E_MEM, gradient_length=self.full, learning_rate=2e-3, max_grad_norm=1.0,
                                           loss_type="huber", use_dones=True, max_rows=max_rows), [est]

    def rows_needed(self, value):
        return value * N_MEM


KINDS = {"ppo": _PPO, "ppo_symmetry": _SymmetricPPO, "ppo_recurrent-lstm": lambda: _RecurrentPPO("lstm"), "ppo_recurrent-gru": lambda: _RecurrentPPO("gru"),
         "distillation": _Distillation, "distillation_recurrent-lstm": lambda: _RecurrentDistillation("lstm"),
         "distillation_recurrent-gru": lambda: _RecurrentDistillation("gru"), "estimator-lstm": lambda: _Estimator("lstm"),
         "estimator-gru": lambda: _Estimator("gru")}
_SETUPS = {}


def _setup(name):
    """The kind's parameters and rows, built once and left unchanged; the trainers a test built are closed behind it."""
    if name not in _SETUPS:
        _SETUPS[name] = KINDS[name]()
    kind, built = _SETUPS[name], []

    def build(max_rows=None):
        alg, owned = kind.build(max_rows)
        built.extend([alg] + owned)
        return alg
    kind.fresh = build
    yield kind
    for obj in built:
        getattr(obj, "close", lambda: None)()          # a policy made of several handles frees them when it goes


@pytest.fixture(params=sorted(KINDS))
def setup(request):
    yield from _setup(request.param)


@pytest.fixture(params=sorted(k for k in KINDS if k.startswith(("distillation_recurrent", "estimator"))))
def carrying(request):
    yield from _setup(request.param)


def _parts(hidden):
    return [] if hidden is None else list(hidden) if isinstance(hidden, (tuple, list)) else [hidden]


def _assert_same(kind, a, b, running=False):
    """Parameters (through `state_dict` and through the masters), both moments, the step count, the learning rate and the carried state."""
    sa, sb = a.optimizer_state(), b.optimizer_state()
    assert sa["step"] == sb["step"] and sa["step"] > 0
    assert sa["learning_rate"] == sb["learning_rate"] == a.learning_rate == b.learning_rate
    for part in ("parameters", "exp_avg", "exp_avg_sq"):
        assert sa[part].keys() == sb[part].keys()
        for k in sa[part]:
            assert torch.equal(sa[part][k], sb[part][k]), (part, k)
    da, db = a.state_dict(), b.state_dict()
    assert da.keys() == db.keys()
    for k in da:
        assert torch.equal(da[k].cpu(), db[k].cpu()), k
    for k, v in sa["parameters"].items():
        assert torch.equal(da[k].cpu(), v), k
    if kind.carries:
        ha, hb = _parts(a.get_hidden_states(running)), _parts(b.get_hidden_states(running))
        assert len(ha) == len(hb) > 0
        for x, y in zip(ha, hb):
            assert x.shape[1] == N_MEM and torch.equal(x.cpu(), y.cpu())


def test_a_checkpoint_into_a_fresh_trainer_continues_bit_for_bit(setup):
    a = setup.fresh()
    setup.update(a)
    setup.update(a)
    b = setup.fresh()
    b.load_optimizer_state(a.optimizer_state())
    if setup.carries:
        b.set_hidden_states(a.get_hidden_states())
    _assert_same(setup, a, b)
    assert setup.update(a) == setup.update(b)
    _assert_same(setup, a, b)


def test_a_handle_regrown_by_update_equals_one_built_large_enough(setup):
    small, large = setup.fresh(setup.rows_needed(setup.small)), setup.fresh(setup.rows_needed(setup.full))
    assert setup.rows_needed(setup.small) < setup.rows_needed(setup.full)
    for alg in (small, large):
        setattr(alg, setup.knob, setup.small)
        setup.update(alg)
    assert small.max_rows == setup.rows_needed(setup.small) and large.max_rows == setup.rows_needed(setup.full)
    for alg in (small, large):
        setattr(alg, setup.knob, setup.full)
        setup.update(alg)
        setup.update(alg)
    assert small.max_rows == setup.rows_needed(setup.full)
    _assert_same(setup, small, large)


def test_load_state_dict_leaves_moments_step_and_learning_rate(setup):
    alg = setup.fresh()
    setup.update(alg)
    before = alg.optimizer_state()
    new = {k: (0.5 * v).contiguous() for k, v in before["parameters"].items()}
    alg.load_state_dict(new)
    after = alg.optimizer_state()
    assert after["step"] == before["step"] > 0 and after["learning_rate"] == before["learning_rate"] == alg.learning_rate
    for part in ("exp_avg", "exp_avg_sq"):
        for k in before[part]:
            assert torch.equal(after[part][k], before[part][k]), (part, k)
        assert max(float(v.abs().max()) for v in before[part].values()) > 0
    sd = alg.state_dict()
    for k, v in new.items():
        assert torch.equal(after["parameters"][k], v) and torch.equal(sd[k].cpu(), v), k


def test_set_learning_rate_before_and_after_the_handle_exists(setup):
    early, late = setup.fresh(), setup.fresh(setup.rows_needed(setup.full))
    assert early.handle is None and late.handle is not None
    for alg in (early, late):
        alg.set_learning_rate(7.5e-4)
        assert alg.learning_rate == 7.5e-4
    assert early.handle is None
    assert setup.update(early) == setup.update(late)
    _assert_same(setup, early, late)
    assert early.optimizer_state()["learning_rate"] != 2e-3 and early.optimizer_state()["learning_rate"] != 4e-3


def test_running_state_of_a_loop_of_groups_continues_and_the_carry_rules(carrying):
    setup = carrying
    a = setup.fresh()
    a.group(setup.rows, 0, 2)
    a.group(setup.rows, 2, 2)
    b = setup.fresh()
    b.load_optimizer_state(a.optimizer_state())
    b.set_hidden_states(a.get_hidden_states(running=True))
    _assert_same(setup, a, b, running=True)
    for alg in (a, b):          # time index 4 of 5: the step enters with the running state
        alg.group(setup.rows, 4, 1)
    _assert_same(setup, a, b, running=True)
    fewer = {k: v[:, :2].contiguous() for k, v in setup.rows.items()}
    with pytest.raises(Exception, match=setup.refusal):
        b.update(fewer)
    b.set_hidden_states(None)
    assert b.get_hidden_states() is None
    b.update(fewer)
    assert all(p.shape[1] == 2 for p in _parts(b.get_hidden_states()))
