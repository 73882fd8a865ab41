"""The one error channel of include/lgpolicy.h: every entry point that returns a status or a handle leaves, when it refuses a call, a message in
`lg_mlp_last_error` that begins with the name of the entry point the caller called -- the same message whether the query gets a handle or NULL.

CPU half (ctypes, no device): one refused call per entry point, enumerated from what `abi.declare_policy` declares (`abi.prototypes`) so that a new
entry point cannot be left out.  GPU half: the refusals that need live handles (widths that do not chain, an LSTM without its cell state, more than 32 actions),
through the acts and through the collectors, each followed by a valid call on the same handles."""
import ctypes as C
import types

import numpy as np
import pytest

from extended_legged_gym_amd import abi
from tests.abi_checks import library

P = 0x1000                # a non-NULL pointer that is never dereferenced: every call below is refused before anything is read

# The exclusions, by name: functions that return nothing, the pure size queries of the host re-tilings (a negative count is their whole error
# report), and the query itself.
VOID = {"lg_mlp_destroy", "lg_rnn_destroy", "lg_conv_encoder_destroy"}
TILE_WEIGHTS = {"lg_rnn_tile_weights", "lg_conv_tile_weights", "lg_conv_tile_weights_bf16"}
QUERY = {"lg_mlp_last_error"}

# entry point -> one call that is refused before any device is touched
REFUSED = {
    "lg_mlp_create": lambda lib: lib.lg_mlp_create(0, None, None, None, 0, 0),
    "lg_mlp_forward": lambda lib: lib.lg_mlp_forward(None, P, 4, P, None),
    "lg_mlp_set_output_activation": lambda lib: lib.lg_mlp_set_output_activation(None, 1),
    "lg_policy_act": lambda lib: lib.lg_policy_act(None, None, P, P, 4, P, 0, 0, 0, P, P, P, P, None),
    "lg_compute_returns": lambda lib: lib.lg_compute_returns(None, P, P, P, 2, 4, 0.99, 0.95, 1, P, P, None),
    "lg_collect_rollout": lambda lib: lib.lg_collect_rollout(None, None, None, P, 0, 0, 2, 0.99, 0.95, 1, C.byref(abi.lg_rollout()), None),
    "lg_plan_from_nodes": lambda lib: lib.lg_plan_from_nodes(None, P, 4, 3, 5, 12, P, None),
    "lg_mppi_update": lambda lib: lib.lg_mppi_update(P, P, 2, 4, 5, 3, 12, 0.0, P, P, None),          # temperature 0
    "lg_mppi_sample_plans": lambda lib: lib.lg_mppi_sample_plans(None, P, 1.0, P, 2, 4, 3, 5, 12, 0, 0, P, P, None),
    "lg_planner_diffuse": lambda lib: lib.lg_planner_diffuse(None, P, P, P, 2, 4, 3, 5, 12, 1, 0.5, 0.05, 0, 0, P, 4, 0.0, P, P, P, P, None),
    "lg_rnn_create": lambda lib: lib.lg_rnn_create(7, 1, 5, 17, None, None, None, None, 0),
    "lg_rnn_step": lambda lib: lib.lg_rnn_step(None, P, 4, P, None, None, None, None),
    "lg_rnn_reset_rows": lambda lib: lib.lg_rnn_reset_rows(None, P, None, P, 4, None),
    "lg_policy_act_recurrent": lambda lib: lib.lg_policy_act_recurrent(None, None, None, None, P, P, 4, P, 0, 0, 0, P, P, P, P, None, P, P, P, P, None),
    "lg_collect_rollout_recurrent": lambda lib: lib.lg_collect_rollout_recurrent(None, None, None, None, None, P, 0, 0, 2, 0.99, 0.95, 1, C.byref(abi.lg_rollout()),
                                                                                 C.byref(abi.lg_rollout_hidden()), P, P, P, P, None),
    "lg_obs_history_step": lambda lib: lib.lg_obs_history_step(P, 8, 0, 48, P, 235, None, None, None, 0, 0, 1.0, None, None),
    "lg_distill_act": lambda lib: lib.lg_distill_act(None, None, P, P, 4, P, 0, 0, 0, P, P, P, None),
    "lg_distill_act_recurrent": lambda lib: lib.lg_distill_act_recurrent(None, None, None, None, P, P, 4, P, 0, 0, 0, P, P, P, P, None, P, P, P, None),
    "lg_collect_distillation": lambda lib: lib.lg_collect_distillation(None, None, None, P, 0, 0, 2, None, C.byref(abi.lg_distill_rollout()), None),
    "lg_collect_distillation_recurrent": lambda lib: lib.lg_collect_distillation_recurrent(None, None, None, None, None, P, 0, 0, 2, None,
                                                                                           C.byref(abi.lg_distill_rollout()), *([None] * 9)),
    "lg_conv_encoder_create": lambda lib: lib.lg_conv_encoder_create(129, 56, 64, 0, None, None, 0),
    "lg_conv_encoder_create_precision": lambda lib: lib.lg_conv_encoder_create_precision(28, 56, 64, 0, None, None, 0, 2),
    "lg_conv_encoder_precision": lambda lib: lib.lg_conv_encoder_precision(None),
    "lg_conv_encoder_forward": lambda lib: lib.lg_conv_encoder_forward(None, P, 1568, 4, P, None),
    "lg_conv_encoder_stage_shape": lambda lib: lib.lg_conv_encoder_stage_shape(None, 1, None, None, None),
    "lg_conv_encoder_forward_stages": lambda lib: lib.lg_conv_encoder_forward_stages(None, P, 1568, 4, 1, P, None),
    "lg_estimator_step": lambda lib: lib.lg_estimator_step(None, None, None, None, P, 1568, P, 4, P, None, None, P, None),
}


def _declared():
    """name -> restype of everything `abi.declare_policy` declares."""
    return {k: v.restype for k, v in abi.prototypes("policy").items()}


def _message(lib, handle=None):
    return (lib.lg_mlp_last_error(handle) or b"").decode()


def test_the_enumeration_leaves_out_nothing():
    decl = _declared()
    assert set(abi.POLICY_SYMBOLS) <= set(decl)
    assert {k for k, r in decl.items() if r is None} == VOID
    assert {k for k in decl if "tile_weights" in k} == TILE_WEIGHTS
    assert {k for k, r in decl.items() if r is C.c_char_p} == QUERY
    assert set(REFUSED) == set(decl) - VOID - TILE_WEIGHTS - QUERY
    for k in REFUSED:
        assert decl[k] in (C.c_int, C.c_int32, C.c_int64, C.c_void_p), (k, decl[k])


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_a_refused_call_names_its_entry_point(name):
    lib = library("policy")
    REFUSED["lg_obs_history_step" if name != "lg_obs_history_step" else "lg_mlp_forward"](lib)          # some other entry point's message is in the channel
    rc = REFUSED[name](lib)
    if _declared()[name] is C.c_void_p:
        assert not rc, name
    else:
        assert rc in (abi.LG_ERR_INVALID, abi.LG_ERR_UNSUPPORTED), (name, rc)
    msg = _message(lib)
    assert msg.startswith(name + ": ") and len(msg) > len(name) + 2, (name, msg)


# ------------------------------------------------------------------------------------------------------------------------------------ GPU half
SENTINEL = 7.0


def _nets():
    """5 -> 17 -> 3 / 1 (17: no multiple of 16) for the feed-forward acts; 17 -> 17 -> 3 / 1 behind an LSTM of input 5, hidden 17, one layer."""
    from extended_legged_gym_amd.rl import NativeMemory, NativeMLP
    rng = np.random.default_rng(0)

    def mlp(i, o):
        return NativeMLP([(rng.normal(size=(17, i)).astype(np.float32) * 0.3, np.zeros(17, np.float32)),
                          (rng.normal(size=(o, 17)).astype(np.float32) * 0.3, np.zeros(o, np.float32))])

    def lstm():
        return NativeMemory([[rng.normal(size=s).astype(np.float32) * 0.3 for s in ((68, 5), (68, 17), (68,), (68,))]], "lstm")
    return types.SimpleNamespace(actor=mlp(5, 3), critic=mlp(5, 1), head_a=mlp(17, 3), head_c=mlp(17, 1), mem_a=lstm(), mem_c=lstm())


def _refused(lib, rc, status, name, word, handle):
    assert rc == status, (name, rc)
    msg = _message(lib, handle)
    assert msg == _message(lib) and msg.startswith(name + ": ") and word in msg, (name, msg)


@pytest.mark.gpu
def test_acts_refuse_with_one_message_and_stay_usable():
    import torch
    N, n = _nets(), 33                                         # one row past a 32-row tile
    lib = N.actor.lib
    p = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
    full = lambda *s: torch.full(s, SENTINEL, device="cuda")          # noqa: E731
    obs, std = torch.randn(n, 5, device="cuda"), torch.full((3,), 0.5, device="cuda")
    h = [torch.zeros(1, n, 17, device="cuda") for _ in range(4)]          # h_a, c_a, h_c, c_c
    act, mean, logp, val = full(n, 3), full(n, 3), full(n), full(n, 1)

    def recurrent(actor, c_a):
        return lib.lg_policy_act_recurrent(N.mem_a.handle, actor.handle, N.mem_c.handle, N.head_c.handle, p(obs), p(obs), n, p(std), 1, 1, 0, p(h[0]), c_a, p(h[2]),
                                           p(h[3]), None, p(act), p(mean), p(logp), p(val), None)
    _refused(lib, recurrent(N.actor, p(h[1])), abi.LG_ERR_INVALID, "lg_policy_act_recurrent", "hidden width", N.actor.handle)
    _refused(lib, recurrent(N.head_a, None), abi.LG_ERR_INVALID, "lg_policy_act_recurrent", "cell state", N.head_a.handle)
    wide = type(N.actor)([(np.zeros((33, 5), np.float32), np.zeros(33, np.float32))])          # 33 actions
    big = full(n, 33)
    rc = lib.lg_policy_act(wide.handle, N.critic.handle, p(obs), p(obs), n, p(std), 1, 1, 0, p(big), p(big), p(logp), p(val), None)
    _refused(lib, rc, abi.LG_ERR_UNSUPPORTED, "lg_policy_act", "32 actions", wide.handle)
    torch.cuda.synchronize()
    for t in (act, mean, logp, val, big):
        assert float(t.min()) == float(t.max()) == SENTINEL, "a refused call must not launch"
    assert not any(bool(x.any()) for x in h)
    # the same handles, valid calls
    assert recurrent(N.head_a, p(h[1])) == abi.LG_OK
    assert lib.lg_policy_act(N.actor.handle, N.critic.handle, p(obs), p(obs), n, p(std), 1, 2, 0, p(act), p(mean), p(logp), p(val), None) == abi.LG_OK
    assert lib.lg_mlp_forward(wide.handle, p(obs), n, p(big), None) == abi.LG_OK
    torch.cuda.synchronize()
    for t in (act, mean, logp, val, big, h[0], h[2]):
        assert bool(torch.isfinite(t).all()) and not bool((t == SENTINEL).any())
    assert bool(h[0].any()) and bool(h[1].any())


@pytest.mark.gpu
def test_collectors_refuse_with_one_message_and_stay_usable():
    import torch
    from tests.test_env_api import make
    N, T = _nets(), 2
    lib = N.actor.lib
    env = make("anymal_c_flat", 5, seed=5)
    env.reset()
    n, O = env.core.t["obs_buf"].shape
    p = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
    full = lambda *s: torch.full(s, SENTINEL, device="cuda")          # noqa: E731
    std = torch.full((3,), 0.5, device="cuda")
    out = dict(observations=full(T, n, O), actions=full(T, n, 3), rewards=full(T, n), dones=full(T, n), values=full(T, n), actions_log_prob=full(T, n),
               mu=full(T, n, 3), sigma=full(T, n, 3), last_values=full(n), returns=full(T, n), advantages=full(T, n))
    rows = abi.lg_rollout(**{k: v.data_ptr() for k, v in out.items()})
    hid = {k: full(T, 1, n, 17) for k in ("h_a", "c_a", "h_c", "c_c")}
    hidden = abi.lg_rollout_hidden(**{k: v.data_ptr() for k, v in hid.items()})
    h = [torch.zeros(1, n, 17, device="cuda") for _ in range(4)]
    before = env.core.t["obs_buf"].clone()
    # the 5-input networks on a 48-wide env
    rc = lib.lg_collect_rollout(env.core.ctx, N.actor.handle, N.critic.handle, p(std), 1, 1, T, 0.99, 0.95, 1, C.byref(rows), None)
    _refused(lib, rc, abi.LG_ERR_INVALID, "lg_collect_rollout", "obs width", N.actor.handle)
    # an LSTM without its cell state
    rc = lib.lg_collect_rollout_recurrent(env.core.ctx, N.mem_a.handle, N.head_a.handle, N.mem_c.handle, N.head_c.handle, p(std), 1, 1, T, 0.99, 0.95, 1,
                                          C.byref(rows), C.byref(hidden), p(h[0]), None, p(h[2]), p(h[3]), None)
    _refused(lib, rc, abi.LG_ERR_INVALID, "lg_collect_rollout_recurrent", "cell state", N.head_a.handle)
    torch.cuda.synchronize()
    for t in list(out.values()) + list(hid.values()):
        assert float(t.min()) == float(t.max()) == SENTINEL, "a refused call must not launch"
    assert torch.equal(env.core.t["obs_buf"], before) and not any(bool(x.any()) for x in h)
    # the same handles, valid calls: the acts on n rows of the widths the networks take
    obs = torch.randn(n, 5, device="cuda")
    act, mean, logp, val = full(n, 3), full(n, 3), full(n), full(n, 1)
    assert lib.lg_policy_act(N.actor.handle, N.critic.handle, p(obs), p(obs), n, p(std), 1, 1, 0, p(act), p(mean), p(logp), p(val), None) == abi.LG_OK
    torch.cuda.synchronize()
    first = act.clone()
    assert lib.lg_policy_act_recurrent(N.mem_a.handle, N.head_a.handle, N.mem_c.handle, N.head_c.handle, p(obs), p(obs), n, p(std), 1, 1, 0, p(h[0]), p(h[1]), p(h[2]),
                                       p(h[3]), None, p(act), p(mean), p(logp), p(val), None) == abi.LG_OK
    torch.cuda.synchronize()
    for t in (first, act, mean, logp, val):
        assert bool(torch.isfinite(t).all()) and not bool((t == SENTINEL).any())
    assert all(bool(x.any()) for x in h)
    # networks that fit the env (48 -> 17 -> 12 / 1): a collection refused for a missing output row, then the same call with the row collects
    from extended_legged_gym_amd.rl import NativeMLP
    rng = np.random.default_rng(1)
    fit = [NativeMLP([(rng.normal(size=(17, O)).astype(np.float32) * 0.1, np.zeros(17, np.float32)),
                      (rng.normal(size=(o, 17)).astype(np.float32) * 0.1, np.zeros(o, np.float32))]) for o in (12, 1)]
    std12 = torch.full((12,), 0.5, device="cuda")
    out.update(actions=full(T, n, 12), mu=full(T, n, 12), sigma=full(T, n, 12))
    ptrs = {k: v.data_ptr() for k, v in out.items()}
    collect = lambda r: lib.lg_collect_rollout(env.core.ctx, fit[0].handle, fit[1].handle, p(std12), 1, 1, T, 0.99, 0.95, 1, C.byref(r), None)          # noqa: E731
    _refused(lib, collect(abi.lg_rollout(**dict(ptrs, observations=None))), abi.LG_ERR_INVALID, "lg_collect_rollout", "null output row", fit[0].handle)
    torch.cuda.synchronize()
    assert torch.equal(env.core.t["obs_buf"], before) and all(float(t.min()) == float(t.max()) == SENTINEL for t in out.values())
    assert collect(abi.lg_rollout(**ptrs)) == abi.LG_OK
    torch.cuda.synchronize()
    assert torch.equal(out["observations"][0], before)
    for t in out.values():
        assert bool(torch.isfinite(t).all()) and not bool((t == SENTINEL).any())
