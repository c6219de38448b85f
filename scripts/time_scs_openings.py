"""Time the opening calls of SCS evaluation matches on mirrored_5x5 (one map), medians of 3:

  draw_and_reset_to   nz_scs_openings_draw + nz_scs_search_reset_to for 1024 matches x 6 plies;
  all_openings_3      scs_positions.all_openings to 3 plies (10 / 55 / 550 positions, nz_scs_openings_expand per level);
  match_round         one full ScsMatch.play round from those drawn openings in the same run, for scale.

Nobody has measured these before and nothing here is a threshold: the openings are meant to cost nothing next to the
round they start.  Prints one JSON object; --out writes it.

    python scripts/time_scs_openings.py [--matches 1024] [--plies 6] [--sims 200] [--reps 3] [--out profiles/scs_openings_timing.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIG = os.path.join(ROOT, "tests", "golden", "scs_configs", "mirrored_5x5.yml")

from nuzero_amd.boardnet import BoardNet                                  # noqa: E402
from nuzero_amd.scs import ScsGameConfig                                  # noqa: E402
from nuzero_amd.scs_positions import all_openings, random_openings        # noqa: E402
from nuzero_amd.tester import ScsMatch                                    # noqa: E402
from nuzero_amd.weights import convnet_param_shapes, synthetic_weights    # noqa: E402
from time_scs_match import search, timed                                  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matches", type=int, default=1024)
    ap.add_argument("--plies", type=int, default=6)
    ap.add_argument("--sims", type=int, default=200)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_scs_openings.py measures on the GPU; there is none")
    N = a.matches
    cfg = ScsGameConfig(CONFIG)
    shapes = convnet_param_shapes(cfg.channels, cfg.planes, 3, 32, a.depth)
    nets = []
    for s in (501, 502):
        n = BoardNet("convnet", cfg.channels, cfg.planes, cfg.rows, cfg.cols, width=32, num_blocks=a.depth, max_batch=N)
        n.set_weights(synthetic_weights(s, shapes, 2.0), 1)
        nets.append(n)
    m = ScsMatch(cfg, search(a.sims), search(a.sims), N)
    e = m.agents[0]

    def draw_and_reset(rep):
        start, n_plies = random_openings(e, range(rep * N, (rep + 1) * N), a.plies)
        e.reset_to(start, n_plies)
        return start, n_plies

    def median_of(fn):
        fn(0)                                                # warm-up: code objects, buffers
        secs = [timed(lambda: fn(r + 1))[0] for r in range(a.reps)]
        return {"seconds": [round(x, 5) for x in secs], "median_s": round(statistics.median(secs), 5)}

    out = {"draw_and_reset_to": median_of(draw_and_reset)}
    counts = []

    def enumerate_3(rep):
        counts[:] = [len(all_openings(e, k)) for k in (1, 2)] + [len(all_openings(e, 3))]
    out["all_openings_3"] = median_of(lambda r: all_openings(e, 3))
    enumerate_3(0)
    out["all_openings_3"]["positions_at_1_2_3_plies"] = list(counts)
    start, n_plies = draw_and_reset(0)
    res = {}

    def round_from_openings(rep):
        res.update(m.play(nets[0], nets[1], start_actions=start, n_plies=n_plies))
    out["match_round"] = median_of(round_from_openings)
    out["match_round"].update({"decisions": int(res["length_max"]), "match_decisions": int(res["length_sum"]),
                               "distinct_games": len({res["actions"][g].tobytes() for g in range(N)}),
                               "wins_p1_p2_draws": [res["p1_wins"], res["p2_wins"], res["draws"]],
                               "persistent": bool(e.persistent())})
    m.close()
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    rnd = out["match_round"]["median_s"]
    out.update({"device": torch.cuda.get_device_name(0), "commit": commit or None, "config": "mirrored_5x5.yml", "matches": N,
                "plies": a.plies, "simulations": a.sims, "nets": f"ConvNet(32, {a.depth})", "reps": a.reps,
                "draw_and_reset_to_over_match_round": round(out["draw_and_reset_to"]["median_s"] / rnd, 6) if rnd else None})
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
