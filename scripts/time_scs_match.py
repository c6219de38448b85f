"""Time an SCS evaluation round between two networks: 1024 matches on randomized_5x5 (one map per match, drawn on the
device), ConvNet(32, 8) against ConvNet(32, 8) with different weights, 200 simulations per decision.  Medians of 3:

  library      nz_scs_match_play (ScsMatch.play), the two agents' searches on two streams;
  one_stream   the same round with both searches on ONE stream (NZ_SCS_MATCH_STREAMS=1), alternating with the above;
  recipe       the reference point: the ply-by-ply recipe of INTEGRATION.md section 5 -- two ScsSelfPlay(training=False)
               engines driven from Python with torch_evaluator on the same two networks -- for --recipe-decisions
               decisions, scaled to the round by seconds per decision (the whole round that way is not worth GPU time).
               That recipe's code is the parent commit's, unchanged by the match loop.

The claim the numbers support or drop is only "two streams are not slower than one"; the margin is the spread of the
repetitions (other work shares the host).  Prints one JSON object; --out writes it.

    python scripts/time_scs_match.py [--matches 1024] [--sims 200] [--reps 3] [--out profiles/scs_match_timing.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIG = os.path.join(ROOT, "tests", "golden", "scs_configs", "randomized_5x5.yml")

from nuzero_amd.boardnet import BoardNet                                  # noqa: E402
from nuzero_amd.scs import ScsGameConfig, ScsSelfPlay, torch_evaluator    # noqa: E402
from nuzero_amd.tester import ScsMatch                                    # noqa: E402
from nuzero_amd.weights import convnet_param_shapes, synthetic_weights    # noqa: E402


def search(sims):
    return {"Simulation": {"mcts_simulations": sims, "keep_subtree": True}, "UCT": {"pb_c_base": 10000, "pb_c_init": 1.15},
            "Exploration": {"number_of_softmax_moves": 0, "epsilon_softmax_exploration": 0.04,
                            "epsilon_random_exploration": 0.001, "value_factor": 1,
                            "root_exploration_distribution": "gamma", "root_exploration_fraction": 0.2,
                            "root_dist_alpha": 0.15, "root_dist_beta": 1}}


class TorchConvNet(torch.nn.Module):
    """The reference's ConvNet(hex=False) in PyTorch on the GPU, from the same weights (oracle/net.py's forward)."""

    def __init__(self, weights, depth):
        super().__init__()
        from oracle.net import FeedForwardRef
        self.ref = FeedForwardRef(weights, "convnet", depth)
        self.ref.w = {k: v.cuda() for k, v in self.ref.w.items()}

    def forward(self, x):
        return self.ref.forward(x)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matches", type=int, default=1024)
    ap.add_argument("--sims", type=int, default=200)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--recipe-decisions", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_scs_match.py measures on the GPU; there is none")
    N = a.matches
    cfg = ScsGameConfig(CONFIG, per_game=True)
    shapes = convnet_param_shapes(cfg.channels, cfg.planes, 3, 32, a.depth)
    weights = [synthetic_weights(s, shapes, 2.0) for s in (501, 502)]
    nets = []
    for w in weights:
        n = BoardNet("convnet", cfg.channels, cfg.planes, cfg.rows, cfg.cols, width=32, num_blocks=a.depth, max_batch=N)
        n.set_weights(w, 1)
        nets.append(n)
    m = ScsMatch(cfg, search(a.sims), search(a.sims), N)

    def round_(seeds, one_stream):
        os.environ["NZ_SCS_MATCH_STREAMS"] = "1" if one_stream else "2"
        try:
            return m.play(nets[0], nets[1], seeds=seeds)
        finally:
            os.environ.pop("NZ_SCS_MATCH_STREAMS", None)

    warm = round_(range(N), False)                         # warm-up: code objects, buffers, both stream set-ups
    round_(range(N), True)
    two, one, decisions, same = [], [], [], True
    for r in range(a.reps):                                # alternating, fresh maps every repetition
        seeds = list(range((r + 1) * N, (r + 2) * N))
        t2, r2 = timed(lambda: round_(seeds, False))
        t1, r1 = timed(lambda: round_(seeds, True))
        two.append(t2); one.append(t1); decisions.append(int(r2["length_max"]))
        same &= bool(np.array_equal(r1["actions"], r2["actions"]) and np.array_equal(r1["outcomes"], r2["outcomes"]))
    persistent = [bool(x.persistent()) for x in m.agents]
    m.close()

    # the reference point: INTEGRATION.md section 5's recipe, driven from Python
    D = a.recipe_decisions
    evs = [torch_evaluator(TorchConvNet(w, a.depth), pad_to=N) for w in weights]
    e1 = ScsSelfPlay(cfg, search(a.sims), N, training=False)
    e2 = ScsSelfPlay(cfg, search(a.sims), N, training=False)

    def recipe(seeds, n_decisions):
        e1.set_games(seeds); e2.set_games(seeds)
        for _ in range(n_decisions):
            player = e1.status()[:, 0]
            # the recipe has one mover for all matches of a ply: true of a round's first decisions (placements follow
            # the schedule), which is all that is timed here
            assert (player == player[0]).all(), "the ply-by-ply recipe cannot serve matches with different movers"
            mover, other, ev_m, ev_o = (e1, e2, evs[0], evs[1]) if player[0] == 1 else (e2, e1, evs[1], evs[0])
            mover.search(ev_m); other.search(ev_o)
            mover.apply()
            other.apply(actions=mover.last_actions())
    recipe(list(range(N)), 1)                              # warm-up (MIOpen picks its algorithms)
    rec = [timed(lambda: recipe(list(range((r + 1) * N, (r + 2) * N)), D))[0] / D for r in range(a.reps)]
    e1.close(); e2.close()

    med = statistics.median
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    out = {"device": torch.cuda.get_device_name(0), "commit": commit or None, "config": "randomized_5x5.yml", "matches": N,
           "simulations": a.sims, "nets": f"ConvNet(32, {a.depth}) x 2, different weights", "persistent": persistent,
           "decisions_per_round": decisions, "library_two_streams_s": [round(x, 4) for x in two],
           "library_one_stream_s": [round(x, 4) for x in one], "two_streams_median_s": round(med(two), 4),
           "one_stream_median_s": round(med(one), 4), "same_matches_on_both": same,
           "two_streams_s_per_decision": round(med(two) / med(decisions), 5),
           "recipe_decisions_timed": D, "recipe_s_per_decision": [round(x, 4) for x in rec],
           "recipe_median_s_per_decision": round(med(rec), 4),
           "recipe_scaled_to_round_s": round(med(rec) * med(decisions), 2),
           "p1_wins_p2_wins_draws_warmup_round": [warm["p1_wins"], warm["p2_wins"], warm["draws"]]}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
