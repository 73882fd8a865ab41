"""Does training the estimator with the bf16 encoder end where fp32 training ends?  (MEASUREMENT TOOL, not product; needs the GPU.)

`tools/train_estimator.py --update native --collect one-call` with the same iteration count, the same seeds, `--train-precision fp32` and `bf16`, one
fresh process per run, one after the other.  Each run ends with its own closing evaluation (the trained estimator played over fresh steps in the
precision it was trained in); its MSE / MAE and last training loss are recorded.  The bf16 runs are judged against the fp32 seeds' own [min, max]:
`outside_by_more_than_the_width` is true for a figure where some bf16 seed lies outside that range by more than the range's width.  Nothing here
is a pass / fail number fixed in advance.

Writes profiles/estimator_update_bf16_training.json.  usage: python tools/compare_estimator_training.py [--iters 40] [--envs 1024] [--seeds 1 2 3]"""
import argparse
import datetime
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--small-terrain", action="store_true")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "estimator_update_bf16_training.json"))
    a = ap.parse_args(argv)
    runs = {"fp32": [], "bf16": []}
    with tempfile.TemporaryDirectory() as d:
        for seed in a.seeds:
            for mode in runs:
                out = os.path.join(d, f"{mode}_{seed}.json")
                cmd = [sys.executable, os.path.join(ROOT, "tools", "train_estimator.py"), "--iters", str(a.iters), "--envs", str(a.envs), "--seed", str(seed), "--update", "native",
                       "--collect", "one-call", "--train-precision", mode, "--eval-precision", mode, "--out", out] + (["--small-terrain"] if a.small_terrain else [])
                subprocess.run(cmd, check=True, timeout=a.timeout, stdout=subprocess.DEVNULL)          # a run that fails or hangs ends the comparison
                r = json.load(open(out))
                runs[mode].append(dict(seed=seed, eval_mse=r["eval_mse"], eval_mae=r["eval_mae"], last_loss=r["loss"][-1], first_loss=r["loss"][0]))
                print(mode, json.dumps(runs[mode][-1]), flush=True)
    verdict = {}
    for key in ("eval_mse", "eval_mae"):
        lo, hi = min(r[key] for r in runs["fp32"]), max(r[key] for r in runs["fp32"])
        width = hi - lo
        worst = max(max(lo - r[key], r[key] - hi, 0.0) for r in runs["bf16"])
        verdict[key] = dict(fp32_min=lo, fp32_max=hi, fp32_width=width, bf16=[r[key] for r in runs["bf16"]], bf16_worst_distance_outside=worst,
                            outside_by_more_than_the_width=bool(worst > width))
    doc = dict(task="elspider_air_rough_raycast", envs=a.envs, steps=24, iters=a.iters, seeds=a.seeds, small_terrain=bool(a.small_terrain),
               date=datetime.date.today().isoformat(), command="tools/train_estimator.py --update native --collect one-call --train-precision <mode> --eval-precision <mode>",
               runs=runs, verdict=verdict)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(verdict, indent=1))


if __name__ == "__main__":
    main()
