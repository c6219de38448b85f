"""Time SCS evaluation rounds against scripted agents: 1024 matches on randomized_5x5 (one map per match, drawn on the
device), ConvNet(32, 8) networks, medians of 3:

  policy_vs_random   nz_scs_agent_match_play, no search at all;
  mcts_vs_random     the same call with one MCTS side (200 simulations per decision);
  mcts_vs_mcts       nz_scs_match_play (ScsMatch) at the same settings on the same box, for comparison.

Nothing here is a threshold.  The expectation the numbers confirm or refute: a match against a scripted agent costs
about ONE engine's search per ply where an MCTS-vs-MCTS match costs two -- compared per decision, because the rounds'
lengths differ with the players.  Prints one JSON object; --out writes it.

    python scripts/time_agent_matches.py [--matches 1024] [--sims 200] [--reps 3] [--out profiles/agent_match_timing.json]
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
sys.path.insert(0, ROOT)
CONFIG = os.path.join(ROOT, "tests", "golden", "scs_configs", "randomized_5x5.yml")

from nuzero_amd.boardnet import BoardNet                                  # noqa: E402
from nuzero_amd.scs import ScsGameConfig                                  # noqa: E402
from nuzero_amd.tester import ScsAgentMatch, ScsMatch                     # noqa: E402
from nuzero_amd.weights import convnet_param_shapes, synthetic_weights    # noqa: E402
from time_scs_match import search, timed                                  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matches", type=int, default=1024)
    ap.add_argument("--sims", type=int, default=200)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_agent_matches.py measures on the GPU; there is none")
    N = a.matches
    cfg = ScsGameConfig(CONFIG, per_game=True)
    shapes = convnet_param_shapes(cfg.channels, cfg.planes, 3, 32, a.depth)
    nets = []
    for s in (501, 502):
        n = BoardNet("convnet", cfg.channels, cfg.planes, cfg.rows, cfg.cols, width=32, num_blocks=a.depth, max_batch=N)
        n.set_weights(synthetic_weights(s, shapes, 2.0), 1)
        nets.append(n)

    def measure(play, close):
        play(list(range(N)))                                 # warm-up: code objects, buffers
        secs, decisions, length_sums = [], [], []
        for r in range(a.reps):                              # fresh maps (and streams) every repetition
            seeds = list(range((r + 1) * N, (r + 2) * N))
            t, res = timed(lambda: play(seeds))
            secs.append(t); decisions.append(int(res["length_max"])); length_sums.append(int(res["length_sum"]))
        close()
        med = statistics.median
        return {"seconds": [round(x, 4) for x in secs], "median_s": round(med(secs), 4), "decisions_per_round": decisions,
                "match_decisions_per_round": length_sums, "s_per_decision": round(med(secs) / med(decisions), 5),
                "wins_p1_p2_draws_last": [res["p1_wins"], res["p2_wins"], res["draws"]]}

    out = {}
    m = ScsAgentMatch(cfg, ("policy",), ("random",), N)
    out["policy_vs_random"] = measure(lambda s: m.play(nets[0], None, seeds=s, agent_seeds=[x + 7 for x in s]), m.close)
    m = ScsAgentMatch(cfg, ("mcts", search(a.sims)), ("random",), N)
    route = {}

    def close_mcts():
        route["persistent"] = bool(m.engine.persistent())
        m.close()
    out["mcts_vs_random"] = measure(lambda s: m.play(nets[0], None, seeds=s, agent_seeds=[x + 7 for x in s]), close_mcts)
    persistent = route["persistent"]
    mm = ScsMatch(cfg, search(a.sims), search(a.sims), N)
    out["mcts_vs_mcts"] = measure(lambda s: mm.play(nets[0], nets[1], seeds=s), mm.close)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    one, two = out["mcts_vs_random"]["s_per_decision"], out["mcts_vs_mcts"]["s_per_decision"]
    out.update({"device": torch.cuda.get_device_name(0), "commit": commit or None, "config": "randomized_5x5.yml", "matches": N,
                "simulations": a.sims, "nets": f"ConvNet(32, {a.depth})", "reps": a.reps, "persistent": persistent,
                "mcts_vs_random_over_mcts_vs_mcts_per_decision": round(one / two, 3) if two else None})
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
