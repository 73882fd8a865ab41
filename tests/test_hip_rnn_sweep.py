"""GPU: `lg_rnn_step`, `lg_rnn_reset_rows` and `lg_policy_act_recurrent` (include/lgpolicy.h; csrc/lg_rnn_tile.h: `rnn_tile`, `rnn_blocks`; csrc/lg_policy.hip:
`rnn_layer_kernel`, `rnn_step_heads`) over input widths, hidden widths, depths, row counts and both memory types, against float64 (`rnn_sweep.step`), and
the training forward of `NativeRecurrentPPO` (`rnn_tile` with SAVE) against the act, bit for bit.  Shapes, weights, inputs, the reference and the bar come
from tests/rnn_sweep.py; tests/test_rnn_sweep_power.py (no GPU) shows on those same inputs that a column not read, a missing bias, exchanged gates or rows, a
misplaced b_hn, a reset that misses c or the GRU's carry, a stale layer below or a transposed 16-block moves some state by at least ten bars.

Tolerance: the project's rule for this path, max(2e-5, 4 x yardstick), yardstick = the restatement in fp32 against float64 -- the 2e-5 floor binds on every
shape here (asserted by `rnn_sweep.case`) -- on every layer's h' and c' after every step.  Every figure is printed before it is asserted; a failure names
row, tile, accumulator half, unit, 16-chunk, wave and layer.

The test allocates every buffer itself and calls through the ctypes face.  The state (L, n, H), and `out`, are followed by 32 sentinel rows (behind the last
layer's slab) that must come back untouched; x is followed by 32 rows of NaN that must not reach any output.  Every call stays inside the documented limits
(widths 1..512, at most 4 layers).

With LG_DUMP_PARITY=1 the figures go to `rnn_sweep.json` in the directory LG_DUMP_DIR names (default: the system's temporary directory), together with the
worst e / e32 of gradient cases R6 - R12 of tests/test_hip_ppo_recurrent_update.py when those ran in the same session; the reviewed copy is
`profiles/rnn_sweep.json`."""
import json
import os

import numpy as np
import pytest
import torch

from tests import rnn_sweep as rs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -777.0
GUARD = 32                     # rows behind the last: one tile
FIGURES = {"sweep": [], "pairs": []}
IDS = [rs.case_id(r, s) for r, s in rs.CASES]


@pytest.fixture(scope="module", autouse=True)
def _dump_figures():
    yield
    if os.environ.get("LG_DUMP_PARITY") != "1":       # (the reviewed copy lives in profiles/; a partial run must not overwrite anything)
        return
    import tempfile
    from tests import test_hip_ppo_recurrent_update as grads
    root = os.environ.get("LG_DUMP_DIR") or tempfile.gettempdir()
    os.makedirs(root, exist_ok=True)
    worst = {}
    for c in FIGURES["sweep"]:
        key = f"{c['type']}-" + "-".join(str(d) for d in c["shape"])
        worst[key] = max(worst.get(key, 0.0), c["ratio"])
    with open(os.path.join(root, "rnn_sweep.json"), "w") as f:
        json.dump(dict(note="figures printed by tests/test_hip_rnn_sweep.py: the device against float64; ratio = error / bar, bar = max(2e-5, 4 x yardstick), "
                            "yardstick = the numpy restatement in fp32 against float64; gradient_cases: the worst e / e32 and the worst e / bar over the gradient "
                            "tensors of cases R6 - R12 of tests/test_hip_ppo_recurrent_update.py (bar = max(8 e32, 2e-5))", device=torch.cuda.get_device_name(0),
                       worst_ratio_per_shape=worst, worst_ratio=max(worst.values(), default=None),
                       gradient_cases={k: grads.FIGURES[k] for k in grads.SWEEP_SHAPES if k in grads.FIGURES}, **FIGURES), f, indent=1)


def memory(rnn, layers):
    from extended_legged_gym_amd.rl import NativeMemory
    return NativeMemory(layers, rnn, device=DEV)


def ptr(t):
    return t.data_ptr() if t is not None else None


def guarded(rows, width):
    return torch.full((rows + GUARD, width), SENTINEL, device=DEV)


def untouched(tag, rows, **bufs):
    for name, buf in bufs.items():
        if buf is not None:
            assert bool((buf[rows:] == SENTINEL).all()), f"{tag}: `{name}` was written behind row {rows}"


class Stepper:
    """One memory's state for n rows in guarded buffers, stepped through `lg_rnn_step`."""

    def __init__(self, mem, n):
        self.mem, self.n, self.L, self.H = mem, n, mem.num_layers, mem.hidden_size
        self.hbuf = guarded(self.L * n, self.H)
        self.cbuf = guarded(self.L * n, self.H) if mem.rnn_type == "lstm" else None
        for b in (self.hbuf, self.cbuf):
            if b is not None:
                b[:self.L * n] = 0.0

    def state(self):
        """Clones of (h, c), each (L, n, H)."""
        return tuple(b[:self.L * self.n].view(self.L, self.n, self.H).clone() if b is not None else None for b in (self.hbuf, self.cbuf))

    def step(self, x, reset=None, reset_rows=False, with_out=True, tag=""):
        """x (n, I) on the CPU.  reset (n) or None: through the step's `reset` argument, or (reset_rows) through `lg_rnn_reset_rows` before the step."""
        mem, n = self.mem, self.n
        xg = torch.cat([x, torch.full((GUARD, x.shape[1]), float("nan"))]).to(DEV).contiguous()
        rg = reset.to(DEV).contiguous() if reset is not None else None
        out = guarded(n, self.H) if with_out else None
        if rg is not None and reset_rows:
            mem._check(mem.lib.lg_rnn_reset_rows(mem.handle, ptr(self.hbuf), ptr(self.cbuf), ptr(rg), n, mem._stream()), "lg_rnn_reset_rows")
            rg = None
        mem._check(mem.lib.lg_rnn_step(mem.handle, ptr(xg), n, ptr(self.hbuf), ptr(self.cbuf), ptr(rg), ptr(out), mem._stream()), "lg_rnn_step")
        torch.cuda.synchronize()
        untouched(tag, self.L * n, h=self.hbuf, c=self.cbuf)
        untouched(tag, n, out=out)
        h, c = self.state()
        if with_out:
            assert torch.equal(out[:n], h[-1]), f"{tag}: `out` is not the top layer's h'"
        return h, c


def trace(mem, x, reset, n, reset_rows=False, with_out=True, tag=""):
    """rs.STEPS steps from a zero state on the first n rows: [(h', c') after each step]."""
    s = Stepper(mem, n)
    return [s.step(x[t, :n], reset[:n] if t == rs.RESET_STEP else None, reset_rows, with_out, f"{tag} step {t}") for t in range(x.shape[0])]


def same_bits(a, b):
    return all(torch.equal(p, q) for sa, sb in zip(a, b) for p, q in zip(sa, sb) if p is not None)


def where(l, r, u, shape):
    return (f"layer {l}, row {r} (tile {r // 32}, accumulator {(r % 32) // 16}: rows {'0-15' if r % 32 < 16 else '16-31'} of the tile), unit {u} (16-chunk {u // 16}, "
            f"wave {(u // 16) % 8}), (I, H, L) = {tuple(shape)}")


def check_states(tag, got, want, bar, shape, yardstick=None):
    """One step's (h', c') against float64: prints the figures, asserts err <= bar with the worst entry's place; returns err."""
    worst = 0.0
    for name, g, w in zip(("h", "c"), got, want):
        if g is None:
            continue
        g = g.detach().double().cpu().numpy()
        diff = np.abs(g - np.asarray(w, np.float64)[:, :g.shape[1]])
        diff[~np.isfinite(g)] = np.inf
        err = float(diff.max())
        l, r, u = (int(v) for v in np.unravel_index(int(diff.argmax()), diff.shape))
        print(f"{tag} {name}': max |err| {err:.3e}" + (f"  yardstick {yardstick:.3e}" if yardstick is not None else "") + f"  bar {bar:.3e}  ratio {err / bar:.4f}")
        assert err <= bar, f"{tag} {name}': |err| {err:.3e} > bar {bar:.3e} at {where(l, r, u, shape)}: got {g[l, r, u]!r}, float64 {w[l, r, u]!r}"
        worst = max(worst, err)
    return worst


# ------------------------------------------------------------------------------------------------ the sweep
@pytest.mark.parametrize("rnn,shape", rs.CASES, ids=IDS)
def test_states_over_shapes_rows_and_steps(rnn, shape):
    """Every layer's h' (and c') after each of three steps, for every n; the reset of step 1 through the step's argument and through `lg_rnn_reset_rows`
    gives the same bits, and so does a second identical run."""
    layers, x, reset, want, yardstick, bar = rs.case(rnn, shape)
    mem = memory(rnn, layers)
    for n in rs.ROWS:
        tag = f"{rs.case_id(rnn, shape)} n={n}"
        got = trace(mem, x, reset, n, tag=tag)
        err = max(check_states(f"{tag} step {t}", got[t], want[t], bar, shape, yardstick) for t in range(rs.STEPS))
        FIGURES["sweep"].append(dict(type=rnn, shape=list(shape), n=n, error=err, yardstick=yardstick, bar=bar, ratio=err / bar))
        assert same_bits(trace(mem, x, reset, n, reset_rows=True, tag=tag + " (lg_rnn_reset_rows)"), got), f"{tag}: the folded reset and lg_rnn_reset_rows differ in bits"
        assert same_bits(trace(mem, x, reset, n, tag=tag + " (again)"), got), f"{tag}: two identical runs differ in bits"
    mem.close()


@pytest.mark.parametrize("rnn,shape", rs.CASES, ids=IDS)
def test_a_rows_state_does_not_depend_on_n_or_on_the_other_rows(rnn, shape):
    """The first rows of the n = 70 run equal the n = 1, 31, 32, 33 runs in bits at every step and layer, and stay so when every other row changes."""
    layers, x, reset, _, _, _ = rs.case(rnn, shape)
    mem = memory(rnn, layers)
    full = trace(mem, x, reset, rs.MAX_ROWS)
    for n in rs.ROWS[:-1]:
        part = trace(mem, x, reset, n)
        cut = [tuple(a[:, :n] if a is not None else None for a in hc) for hc in full]
        assert same_bits(part, cut), f"{rs.case_id(rnn, shape)}: the first {n} rows of n = 70 are not the n = {n} run"
    other, flipped = x.clone(), reset.clone()
    other[:, 33:] = 3.0 * x[:, 33:].flip(1)
    flipped[33:] = 1.0 - reset[33:]
    moved = trace(mem, other, flipped, rs.MAX_ROWS)
    assert same_bits([tuple(a[:, :33] if a is not None else None for a in hc) for hc in moved], [tuple(a[:, :33] if a is not None else None for a in hc) for hc in full])
    assert not same_bits(moved, full)
    mem.close()


@pytest.mark.parametrize("rnn,shape", rs.CASES, ids=IDS)
def test_out_is_the_top_layers_new_h_and_changes_nothing_else(rnn, shape):
    """`Stepper.step` holds `out` to the top layer's h' after every step; with out = NULL the state takes the same bits."""
    layers, x, reset, _, _, _ = rs.case(rnn, shape)
    mem = memory(rnn, layers)
    for n in (1, 33, 70):
        assert same_bits(trace(mem, x, reset, n, with_out=False), trace(mem, x, reset, n, with_out=True)), (rnn, shape, n)
    mem.close()


@pytest.mark.parametrize("rnn", rs.TYPES)
def test_a_narrow_memory_is_not_reached_by_what_a_wide_launch_left_in_lds(rnn):
    """(1, 1, 1) reads a 32-column image; (511, 511, 1) fills all 1024 columns: equal bits before and after the wide launch on inputs of magnitude 1e3,
    on the same stream, and the reference still met."""
    layers, x, reset, want, yardstick, bar = rs.case(rnn, (1, 1, 1))
    wl, wx, wreset, _, _, _ = rs.case(rnn, (511, 511, 1))
    narrow, wide = memory(rnn, layers), memory(rnn, wl)
    for n in (1, 70):
        before = trace(narrow, x, reset, n)
        big = trace(wide, 1e3 * wx, wreset, rs.MAX_ROWS)
        assert all(bool(torch.isfinite(h).all()) for h, _ in big) and float(big[-1][0].abs().max()) > 0.5
        after = trace(narrow, x, reset, n)
        assert same_bits(before, after), (rnn, n)
        for t in range(rs.STEPS):
            check_states(f"{rs.case_id(rnn, (1, 1, 1))} n={n} step {t} after the wide launch", after[t], want[t], bar, (1, 1, 1), yardstick)
    narrow.close(); wide.close()


# ------------------------------------------------------------------------------------------------ pairs through lg_policy_act_recurrent
def flat(hs):
    return list(hs) if isinstance(hs, tuple) else [hs]


def reference_states(rnn, layers, x, dones):
    """float64 states after each step when `reset(dones[t])` follows step t."""
    L, H, n = len(layers), layers[0][1].shape[1], x.shape[1]
    h, c, out = np.zeros((L, n, H)), (np.zeros((L, n, H)) if rnn == "lstm" else None), []
    for t in range(x.shape[0]):
        h, c = rs.step(rnn, layers, x[t].numpy(), h, c, dones[t - 1].numpy() if t else None)
        out.append((h, c))
    return out


@pytest.mark.parametrize("rnn", rs.TYPES)
@pytest.mark.parametrize("pair", range(len(rs.PAIRS)), ids=["equal_depth_side_by_side", "unequal_depth_one_after_the_other"])
def test_a_pair_of_memories_steps_as_each_memory_alone(pair, rnn):
    """Both memories' states after `lg_policy_act_recurrent` equal, bit for bit, the states each memory reaches alone under `lg_rnn_step` with
    `lg_rnn_reset_rows` between the steps (and meet float64 at the bar); the action means and the values equal the heads run on those states."""
    from extended_legged_gym_amd.rl import NativeActorCriticRecurrent, NativeMLP
    ashape, cshape = rs.PAIRS[pair]
    n, sd = rs.PAIR_ROWS, rs.policy_state(rnn, ashape, cshape)
    ac = NativeActorCriticRecurrent(sd, "elu", rnn, device=DEV, seed=3)
    assert (ac.memory_a.num_layers == ac.memory_c.num_layers) == (pair == 0)
    xa, xc, dones = rs.make_rows(ashape[0], n), rs.make_rows(cshape[0], n, salt=1), rs.pair_dones(n)
    alone = [Stepper(memory(rnn, rs.memory_layers(sd, p)), n) for p in ("memory_a", "memory_c")]
    heads = [NativeMLP(rs.head_layers(sd, p), "elu", device=DEV) for p in ("actor", "critic")]
    want = [reference_states(rnn, rs.memory_layers(sd, p), x, dones) for p, x in (("memory_a", xa), ("memory_c", xc))]
    worst = 0.0
    for t in range(rs.STEPS):
        tag = f"{rnn} actor {ashape} critic {cshape} step {t}"
        _, values, _, mean, _ = ac.act_and_evaluate(xa[t].to(DEV), xc[t].to(DEV))
        torch.cuda.synchronize()
        for k, (name, x, shape, live) in enumerate((("actor memory", xa, ashape, ac.memory_a), ("critic memory", xc, cshape, ac.memory_c))):
            single = alone[k].step(x[t], dones[t - 1] if t else None, reset_rows=True, tag=f"{tag} {name} alone")
            got = flat(live.hidden_states)
            assert all(torch.equal(g, s) for g, s in zip(got, single)), f"{tag}: the {name} of the pair is not the memory stepped alone, bit for bit"
            worst = max(worst, check_states(f"{tag} {name}", single, want[k][t], rs.FLOOR, shape))
            top = single[0][-1].contiguous()
            assert torch.equal(heads[k](top), mean if k == 0 else values), f"{tag}: the {name}'s head did not read the top layer's h'"
        ac.reset(dones[t].to(DEV))
    FIGURES["pairs"].append(dict(type=rnn, actor=list(ashape), critic=list(cshape), n=n, error=worst, bar=rs.FLOOR, ratio=worst / rs.FLOOR))
    for s in alone:
        s.mem.close()
    for m in heads:
        m.close()


# ------------------------------------------------------------------------------------------------ the training forward (SAVE) against the act
@pytest.mark.parametrize("rnn", rs.TYPES)
@pytest.mark.parametrize("shape", rs.TRAIN_SHAPES, ids=["-".join(str(d) for d in s) for s in rs.TRAIN_SHAPES])
def test_the_training_forward_equals_the_act_bit_for_bit(shape, rnn):
    """A rollout of T = 3 steps on 33 envs collected with `act_and_evaluate` / `reset(dones)` from a memory that has already lived one step, episodes
    ending inside the window: `forward_outputs` of the whole-batch mini-batch equals the collected means and values in bits (what
    test_trainer_and_acts_stay_coherent_on_a_collected_rollout checks at hidden 40)."""
    from extended_legged_gym_amd.rl import NativeActorCriticRecurrent, NativeRecurrentPPO
    T, N, A = rs.TRAIN_T, rs.TRAIN_ENVS, rs.PAIR_ACTIONS
    sd = rs.policy_state(rnn, shape, shape)
    policy = NativeActorCriticRecurrent(sd, "elu", rnn, device=DEV, seed=3)
    ppo = NativeRecurrentPPO(policy, sd, num_mini_batches=1)
    obs, cobs, dones = rs.make_rows(shape[0], N).to(DEV), rs.make_rows(shape[0], N, salt=1).to(DEV), rs.pair_dones(N).to(DEV)
    assert T == rs.STEPS and float(dones[:T - 1].sum()) > 0
    policy.act_and_evaluate(rs.make_rows(shape[0], N, salt=2)[0].to(DEV), rs.make_rows(shape[0], N, salt=3)[0].to(DEV))          # one step lived
    rows = {k: [] for k in ("actions", "values", "actions_log_prob", "mu", "sigma")}
    hid = {"a": [], "c": []}
    for t in range(T):
        ha, hc = policy.get_hidden_states()
        hid["a"].append([h.clone() for h in flat(ha)]); hid["c"].append([h.clone() for h in flat(hc)])
        a, v, lp, mu, sig = policy.act_and_evaluate(obs[t], cobs[t])
        for k, val in zip(rows, (a, v, lp.view(-1, 1), mu, sig)):
            rows[k].append(val.clone())
        policy.reset(dones[t])
    out = {k: torch.stack(v) for k, v in rows.items()}
    g = torch.Generator().manual_seed(5)
    out.update(observations=obs, critic_observations=cobs, dones=dones.unsqueeze(-1), returns=out["values"] + torch.randn(T, N, 1, generator=g).to(DEV),
               advantages=torch.randn(T, N, 1, generator=g).to(DEV))
    for tag in ("a", "c"):
        stacks = tuple(torch.stack([step[j] for step in hid[tag]]) for j in range(len(hid[tag][0])))
        out["hidden_states_" + tag] = stacks if rnn == "lstm" else stacks[0]
    assert float(flat(out["hidden_states_a"])[0][0].abs().max()) > 0 and out["mu"].shape == (T, N, A)
    ppo.minibatch(out, 0, N)
    mu, val = ppo.forward_outputs(T * N)
    dm, dv = float((mu.view(T, N, A) - out["mu"].cpu()).abs().max()), float((val.view(T, N, 1) - out["values"].cpu()).abs().max())
    print(f"{rnn} {shape}: training forward against the act: means differ by {dm:.3e}, values by {dv:.3e}")
    assert torch.equal(mu.view(T, N, A), out["mu"].cpu()) and torch.equal(val.view(T, N, 1), out["values"].cpu())
    ppo.close()
