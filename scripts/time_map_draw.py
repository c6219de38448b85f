"""Per-game map draw on the host (numpy, ScsGameConfig.draw_games + nz_scs_search_set_games) against the device
(nz_scs_search_draw_games): wall time of ScsSelfPlay.set_games, both ending with the games reset on the device, for
1024 and 8192 games on randomized_5x5 and randomized_10x10; and one Gamer round of 1024 games on randomized_5x5 (both
draws) against the fixed map of mirrored_5x5.  Prints one JSON object.

    python scripts/time_map_draw.py [--reps 3] [--round-games 1024]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIGS = os.path.join(ROOT, "tests", "golden", "scs_configs")

from nuzero_amd.scs import ScsGameConfig, ScsSelfPlay   # noqa: E402

SEARCH = {"Simulation": {"mcts_simulations": 16, "keep_subtree": True}, "UCT": {"pb_c_base": 10000, "pb_c_init": 1.15},
          "Exploration": {"number_of_softmax_moves": 0, "epsilon_softmax_exploration": 0.04,
                          "epsilon_random_exploration": 0.001, "value_factor": 1,
                          "root_exploration_distribution": "gamma", "root_exploration_fraction": 0.2,
                          "root_dist_alpha": 0.15, "root_dist_beta": 1}}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def set_games(name, n, reps):
    cfg = ScsGameConfig(os.path.join(CONFIGS, name), per_game=True)
    sp = ScsSelfPlay(cfg, SEARCH, n)
    sp.set_games(range(n), on_device=True)               # warm-up: code objects, buffers
    sp.set_games(range(n), on_device=False)
    host, dev = [], []
    for r in range(reps):                                 # alternating, fresh seeds every time
        seeds = list(range((r + 1) * n, (r + 2) * n))
        host.append(timed(lambda: sp.set_games(seeds, on_device=False)))
        dev.append(timed(lambda: sp.set_games(seeds, on_device=True)))
        if r == 0:
            assert np.array_equal(sp.game_maps[0], cfg.draw_games(seeds)[0])
    sp.close()
    return {"config": name, "games": n, "host_s": [round(x, 5) for x in host], "device_s": [round(x, 5) for x in dev],
            "host_median_s": round(statistics.median(host), 5), "device_median_s": round(statistics.median(dev), 5)}


def gamer_rounds(games, reps):
    from nuzero_amd.gamer import Gamer
    from nuzero_amd.network import Network_Manager
    from nuzero_amd.weights import synthetic_weights, convnet_param_shapes

    class SCS_Game:
        pass

    shapes = convnet_param_shapes(86, 21, 3, 32, 2)
    nm = Network_Manager({k: torch.from_numpy(v) for k, v in synthetic_weights(5, shapes, 2.0).items()})
    out = []
    for label, name, on_device in (("randomized_5x5 device draw", "randomized_5x5.yml", True),
                                   ("randomized_5x5 host draw", "randomized_5x5.yml", False),
                                   ("mirrored_5x5 (one map)", "mirrored_5x5.yml", None)):
        g = Gamer(None, nm, SCS_Game, [os.path.join(CONFIGS, name)], 3, SEARCH, 1, "keyless", size_estimate=4096,
                  num_games=games, concurrent_games=games, base_seed=1000, records=False)
        if on_device is not None:
            g.engine.draw_on_device = on_device
        g.play_games()                                   # warm-up round
        times = [timed(g.play_games) for _ in range(reps)]
        out.append({"round": label, "games": games, "round_s": [round(x, 4) for x in times],
                    "median_s": round(statistics.median(times), 4)})
        g.engine.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--round-games", type=int, default=1024)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "set_games": [], "gamer_round": []}
    for name in ("randomized_5x5.yml", "randomized_10x10.yml"):
        for n in (1024, 8192):
            res["set_games"].append(set_games(name, n, a.reps))
            print(json.dumps(res["set_games"][-1]), file=sys.stderr, flush=True)
    res["gamer_round"] = gamer_rounds(a.round_games, a.reps)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
