"""Float64 restatement of `EmpiricalNormalization` (rsl_rl `modules/normalizer.py:14-76`), written from its recurrences, and the golden cases of
tests/golden/empirical_normalization.npz.

The recurrences, per call on an (n, O) batch x in training mode, unless `until` is set and `count >= until`:
    count += n;  rate = n / count;  mean_x, var_x = column mean and BIASED variance of x;  delta = mean_x - mean
    mean += rate * delta;  var += rate * (var_x - var + delta * (mean_x - mean_new));  std = sqrt(var)
then, always, y = (x - mean) / (std + eps); inverse: x = y * (std + eps) + mean.  Initial state: mean 0, var 1, std 1, count 0.

The input batches are not stored in the fixture (the six shapes up to 1000 x 260, six calls each, are 8 MB of noise, past the size a committed
file may have): `case_batches` regenerates them bit for bit from integer arithmetic (a splitmix64 hash of the element index, four 16-bit fields
summed into a bell-shaped draw), and the fixture keeps each batch's float64 sum to show that it did.  tools/refgen/make_runner_golden.py feeds
the same batches to the reference module and stores its `_mean`, `_var`, `_std`, `count` after every call, and its outputs: whole for batches up
to `FULL_OUTPUT_ELEMENTS` elements, the rows `output_rows(n)` beyond."""
import json

import numpy as np

FULL_OUTPUT_ELEMENTS = 4096
SHAPES = [(1, 1), (3, 7), (64, 48), (65, 235), (257, 253), (1000, 260)]
# name, n, O, training calls, eval-mode calls after them, until, eps, special
CASES = ([dict(name=f"shape_{n}x{O}", n=n, O=O, calls=6, eval_calls=0, until=None, eps=1e-2, special=None) for n, O in SHAPES] +
         [dict(name="constant_column", n=33, O=5, calls=4, eval_calls=0, until=None, eps=1e-2, special="constant"),
          dict(name="large_mean_small_spread", n=129, O=4, calls=4, eval_calls=0, until=None, eps=1e-2, special="large_mean"),
          dict(name="until_crossed", n=40, O=9, calls=5, eval_calls=0, until=100, eps=1e-2, special=None),          # counts 40, 80, 120, then frozen
          dict(name="eval_after_training", n=50, O=11, calls=3, eval_calls=2, until=None, eps=1e-2, special=None),
          dict(name="inverse", n=50, O=11, calls=3, eval_calls=0, until=None, eps=1e-3, special="inverse")])


def _splitmix64(x):
    x = (x + np.uint64(0x9E3779B97F4A7C15)).astype(np.uint64)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def _bell(count, stream):
    """`count` float64 draws of mean 0 and variance 1 (the sum of four 16-bit uniforms, centred and scaled): exact integer arithmetic."""
    with np.errstate(over="ignore"):
        z = _splitmix64(np.arange(count, dtype=np.uint64) + (np.uint64(stream) << np.uint64(36)))
    s = sum(((z >> np.uint64(16 * k)) & np.uint64(0xFFFF)).astype(np.float64) for k in range(4))
    return (s - 131070.0) / 37837.22


def case_batches(case):
    """The float32 (n, O) batches of a case: training calls, then eval-mode calls; with `inverse`, one more batch, the argument of `inverse`."""
    i = [c["name"] for c in CASES].index(case["name"])
    n, O = case["n"], case["O"]
    scale = np.abs(_bell(O, 1000 + i)) * 1.5 + 0.1
    shift = _bell(O, 2000 + i) * 2.0
    if case["special"] == "large_mean":
        scale, shift = np.array([1.0, 1e-2, 1.0, 1e-2]), np.array([0.0, 1e3, -1e3, 1e3])
    total = case["calls"] + case["eval_calls"] + (1 if case["special"] == "inverse" else 0)
    out = []
    for call in range(total):
        x = _bell(n * O, 100 * i + call + 1).reshape(n, O) * scale + shift + 0.1 * call
        if case["special"] == "constant":
            x[:, 2] = 0.75
        out.append(x.astype(np.float32))
    return out


def output_rows(n):
    """The rows of a large batch whose outputs the fixture keeps."""
    return np.unique(np.concatenate([np.arange(min(n, 4)), np.arange(max(n - 2, 0), n), np.arange(0, n, max(n // 8, 1))]))


class Float64Normalizer:
    def __init__(self, O, eps=1e-2, until=None):
        self.mean, self.var, self.std = np.zeros(O), np.ones(O), np.ones(O)
        self.count, self.eps, self.until = 0, float(eps), until

    def update(self, x):
        if self.until is not None and self.count >= self.until:
            return
        x = np.asarray(x, np.float64)
        n = x.shape[0]
        if n == 0:
            return
        self.count += n
        rate = n / self.count
        mean_x = x.mean(axis=0)
        var_x = ((x - mean_x) ** 2).mean(axis=0)
        delta = mean_x - self.mean
        self.mean = self.mean + rate * delta
        self.var = self.var + rate * (var_x - self.var + delta * (mean_x - self.mean))
        self.std = np.sqrt(self.var)

    def __call__(self, x, training=True):
        if training:
            self.update(x)
        return (np.asarray(x, np.float64) - self.mean) / (self.std + self.eps)

    def inverse(self, y):
        return np.asarray(y, np.float64) * (self.std + self.eps) + self.mean


def run_case(case, batches=None):
    """The restatement over a case: per call dict(mean, var, std, count, y), and the inverse's result (or None)."""
    batches = case_batches(case) if batches is None else batches
    m = Float64Normalizer(case["O"], case["eps"], case["until"])
    calls = []
    for k in range(case["calls"] + case["eval_calls"]):
        y = m(batches[k], training=k < case["calls"])
        calls.append(dict(mean=m.mean.copy(), var=m.var.copy(), std=m.std.copy(), count=m.count, y=y))
    inv = m.inverse(batches[-1]) if case["special"] == "inverse" else None
    return calls, inv


def ulp32(v):
    """The spacing of float32 at |v| (float64 array)."""
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def deviation_in_ulp(got, want, magnitude=None):
    """max |got - want| in units of the float32 spacing at `magnitude` (default: |want|)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if want.size == 0:
        return 0.0
    err = np.abs(got - want)
    unit = ulp32(want if magnitude is None else np.maximum(np.abs(want), magnitude))
    return float(np.max(np.where(err == 0.0, 0.0, err / unit)))


def load_golden(path):
    z = np.load(path)
    return z, json.loads(str(z["cases"]))


def kept_rows(case):
    n = case["n"]
    return np.arange(n) if n * case["O"] <= FULL_OUTPUT_ELEMENTS else output_rows(n)


def measure(case, calls, inv, batches, fetch, rows=None):
    """The deviation of an fp32 implementation from the restatement on a case, in float32 ulp "at the value's magnitude": dict(state=, output=).
    `fetch(kind, k)`: the implementation's `_mean` / `_var` / `_std` / `y` after call k, and `inv_x` (k None); `rows`: the rows its outputs cover.
    The magnitude of `_var` and `_std` is their own; of `_mean`, max(|mean|, std): a mean near zero of a column that is not is a difference of
    values of the column's size; of an output, max(|y|, (|x| + |mean|) / (std + eps)), the size of the operands its subtraction cancels (and for the
    inverse max(|x|, |y| (std + eps), |mean|))."""
    rows = np.arange(case["n"]) if rows is None else rows
    state = output = 0.0
    for k, c in enumerate(calls):
        state = max(state, deviation_in_ulp(fetch("_mean", k).reshape(-1), c["mean"], np.maximum(np.abs(c["mean"]), c["std"])),
                    deviation_in_ulp(fetch("_var", k).reshape(-1), c["var"]), deviation_in_ulp(fetch("_std", k).reshape(-1), c["std"]))
        x = np.asarray(batches[k], np.float64)[rows]
        output = max(output, deviation_in_ulp(fetch("y", k), c["y"][rows], (np.abs(x) + np.abs(c["mean"])) / (c["std"] + case["eps"])))
    if inv is not None:
        last, y = calls[-1], np.asarray(batches[-1], np.float64)[rows]
        output = max(output, deviation_in_ulp(fetch("inv_x", None), inv[rows], np.maximum(np.abs(y) * (last["std"] + case["eps"]), np.abs(last["mean"]))))
    return dict(state=state, output=output)


def module_deviation(z, case, calls, inv, batches):
    """The reference module's own fp32 deviation from the restatement, from the fixture."""
    name = case["name"]
    return measure(case, calls, inv, batches, lambda kind, k: z[f"{name}.{kind}"] if k is None else z[f"{name}.{kind}{k}"], kept_rows(case))


FLOOR_ULP = 4.0


def bars(module):
    """The bar of a native implementation on a case: twice the module's own deviation, never below 4 ulp."""
    return {k: max(2.0 * v, FLOOR_ULP) for k, v in module.items()}
