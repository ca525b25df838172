#!/usr/bin/env python3
"""The headline bench in N fresh processes, one after another, alternating between environments.

    python tools/bench_series.py --runs 16 --env BH_FC_TUNE_ALLOC=0 --env "" --out profiles/series.txt

Every `--env` is one environment: space-separated NAME=VALUE pairs, "" for none.  A variable that another environment sets and
this one does not is removed from the child's environment, so "" really is the default.  Run k uses environment k mod len(envs).
Each child is `timeout -k 10 300 python bench.py --gpus 1 --steps 10 --warmup 2`; there is never more than one at a time, and
the series ends at the first child that exits non-zero (no retries: a fault is a finding, not something to run again).
Printed and appended to --out: value, ms_per_step and roofline.ms per run, the child's "[bh tune" lines (BH_DEBUG_SCRATCH=1),
and min / median / max per environment.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def parse_env(text: str) -> dict:
    pairs = {}
    for item in text.split():
        name, sep, value = item.partition("=")
        if not sep or not name:
            raise SystemExit(f"--env: {item!r} is not NAME=VALUE")
        pairs[name] = value
    return pairs


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=16, help="processes in all (default 16 = 8 pairs of two environments)")
    ap.add_argument("--env", action="append", default=None, help='one environment, e.g. "BH_FC_TUNE_ALLOC=0"; repeat; "" = none')
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_series.txt"), help="the table is appended to this file")
    ap.add_argument("--title", default="", help="a line written above the table")
    args = ap.parse_args()
    envs = [parse_env(e) for e in (args.env if args.env is not None else ["BH_FC_TUNE_ALLOC=0", ""])]
    labels = [" ".join(f"{k}={v}" for k, v in e.items()) or "(default)" for e in envs]
    named = set().union(*envs)
    width = max(len(s) for s in labels)

    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    lines = []

    def say(text: str = "") -> None:
        print(text, flush=True)
        lines.append(text)

    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(args.steps),
           "--warmup", str(args.warmup)]
    say(f"== {args.title or 'bench series'}: {args.runs} fresh processes, bench.py --gpus 1 --steps {args.steps} --warmup {args.warmup} ==")
    say(f"{'run':>3}  {'environment':<{width}}  {'value (vox/s)':>13}  {'ms_per_step':>11}  {'roofline.ms':>11}  {'wall s':>6}")
    results = [[] for _ in envs]
    status = 0
    for k in range(args.runs):
        which = k % len(envs)
        env = {n: v for n, v in os.environ.items() if n not in named}
        env.update(envs[which])
        t0 = time.monotonic()
        child = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)  # one GPU process at a time
        wall = time.monotonic() - t0
        tune = [ln for ln in child.stderr.splitlines() if ln.startswith("[bh tune")]
        if child.returncode != 0:
            say(f"{k + 1:>3}  {labels[which]:<{width}}  exit status {child.returncode} after {wall:.0f} s: the series ends here")
            for ln in child.stderr.splitlines()[-15:]:
                say("     | " + ln)
            status = 1
            break
        try:
            res = json.loads(child.stdout.strip().splitlines()[-1])
            row = (res["value"], res["ms_per_step"], res["roofline"]["ms"])
        except (IndexError, KeyError, ValueError):
            say(f"{k + 1:>3}  {labels[which]:<{width}}  no result line: the series ends here")
            status = 1
            break
        results[which].append(row)
        say(f"{k + 1:>3}  {labels[which]:<{width}}  {row[0]:>13.4e}  {row[1]:>11.2f}  {row[2]:>11.3f}  {wall:>6.0f}")
        for ln in tune:
            say("     " + ln)
    say()
    say(f"{'environment':<{width}}  runs  {'ms_per_step min / median / max':>32}  {'roofline.ms min / median / max':>32}")
    for label, rows in zip(labels, results):
        if not rows:
            continue
        cols = []
        for c in (1, 2):
            v = [r[c] for r in rows]
            cols.append(f"{min(v):.2f} / {statistics.median(v):.2f} / {max(v):.2f}")
        say(f"{label:<{width}}  {len(rows):>4}  {cols[0]:>32}  {cols[1]:>32}")
    say()
    with out.open("a") as f:
        f.write("\n".join(lines) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
