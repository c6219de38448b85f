"""Time the Tic-Tac-Toe evaluations from given positions on one MI355X, medians of 3 (after one warm-up call each),
with the 64-wide RecurrentNet (2 blocks, 2 recurrent iterations) at 100 simulations per move -- the two calls with a
search (score, openings) and, beside them, the score of the bare policy:

  score     TttTester.score_against_perfect_play(("mcts", cfg), weights): one engine of 4,520 games, reset(boards),
            search(), apply() -- engine construction and weight upload included, as a caller pays them;
  policy    the same call for ("policy",): nz_engine_policy_actions, no search;
  openings  TttTester.test_from_openings(cfg, weights_a, cfg, weights_b, plies=2): the 72 two-ply openings, both colour
            assignments, 144 matches (the tester keeps the engines of both colour assignments between calls; the
            weights are uploaded every call).

None of the three had been measured before: no threshold is set.  Prints one JSON object; --out writes it.

    python scripts/time_ttt_positions.py [--sims 100] [--reps 3] [--out profiles/ttt_positions_timing.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_ttt_positions.py measures on the GPU; there is none")
    sys.path.insert(0, ROOT)
    from nuzero_amd.search_config import legacy_ttt_search_config
    from nuzero_amd.tester import TttTester
    from nuzero_amd.weights import synthetic_recurrent_net_weights
    cfg = legacy_ttt_search_config(a.sims)
    wa, wb = (synthetic_recurrent_net_weights(s, 2, 1, 64, 2, True) for s in (0, 1))
    t = TttTester()
    calls = {"score": lambda: t.score_against_perfect_play(("mcts", cfg), wa, recurrent_iterations=2),
             "policy": lambda: t.score_against_perfect_play(("policy",), wa, recurrent_iterations=2),
             "openings": lambda: t.test_from_openings(cfg, wa, cfg, wb, plies=2, recurrent_iterations=2)}
    seen = {k: fn() for k, fn in calls.items()}                 # warm-up: code objects, buffers
    times = {k: [] for k in calls}
    for _ in range(a.reps):                                     # interleaved
        for k, fn in calls.items():
            times[k].append(timed(fn)[0])
    t.close()
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    out = {"device": torch.cuda.get_device_name(0), "commit": commit or None, "simulations": a.sims,
           "net": "RecurrentNet(64, 2), 2 iterations", "positions": seen["score"]["positions"],
           "mcts_optimal": seen["score"]["optimal"], "policy_optimal": seen["policy"]["optimal"],
           "openings_agent1_agent2_draws": list(seen["openings"])}
    for k, v in times.items():
        out[f"{k}_s"] = [round(x, 4) for x in v]
        out[f"{k}_median_s"] = round(statistics.median(v), 4)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
