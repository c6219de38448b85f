"""The compact SCS replay buffer (ScsReplayBuffer) against the dense one (DeviceReplayBuffer), which is the yardstick:
saving a 1024-game round, gathering a batch of 2048 sampled positions, bytes per position and bytes allocated for the
same window -- on mirrored_5x5 and ten_by_ten, a round from play_round_device with ConvNet(32, 2) and 16 simulations.
Every shape is warmed up, the two classes alternate, medians of --reps repeats with a device synchronise inside the
timed region (a gather repeat is 100 batches back to back, reported per batch: sampling on the host, the upload of the
slots and the kernel); the repeats and their spread are recorded.  Writes profiles/scs_replay_timing.json.

    python scripts/time_scs_replay.py [--reps 7] [--games 1024] [--out profiles/scs_replay_timing.json]
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

from nuzero_amd.boardnet import BoardNet   # noqa: E402
from nuzero_amd.replay_device import DeviceReplayBuffer, ReplayIndex   # noqa: E402
from nuzero_amd.replay_scs import ScsReplayBuffer   # noqa: E402
from nuzero_amd.scs import ScsGameConfig, ScsSelfPlay   # noqa: E402
from nuzero_amd.weights import convnet_param_shapes, synthetic_weights   # noqa: E402

SEARCH = {"Simulation": {"mcts_simulations": 16, "keep_subtree": True}, "UCT": {"pb_c_base": 10000, "pb_c_init": 1.15},
          "Exploration": {"number_of_softmax_moves": 0, "epsilon_softmax_exploration": 0.04,
                          "epsilon_random_exploration": 0.001, "value_factor": 1,
                          "root_exploration_distribution": "gamma", "root_exploration_fraction": 0.2,
                          "root_dist_alpha": 0.15, "root_dist_beta": 1}}
BATCH = 2048
GATHERS = 100        # batches per timed repeat of the gather (one batch is tens of microseconds: too short a window)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def summary(xs):
    return {"median_s": round(statistics.median(xs), 6), "spread_s": round(max(xs) - min(xs), 6),
            "repeats_s": [round(x, 6) for x in xs]}


def case(name, games, reps):
    cfg = ScsGameConfig(os.path.join(CONFIGS, name + ".yml"))
    net = BoardNet("convnet", cfg.channels, cfg.planes, cfg.rows, cfg.cols, width=32, num_blocks=2, max_batch=games)
    net.set_weights(synthetic_weights(4, convnet_param_shapes(cfg.channels, cfg.planes, 3, 32, 2), 2.0))
    sp = ScsSelfPlay(cfg, SEARCH, games)
    ex = sp.play_round_device(net, range(1000, 1000 + games))
    lengths = ex["lengths"].cpu().numpy()
    longest = int(lengths.max())
    # one window of `games` games; the buffers are sized by the round's longest game so that the dense one fits beside it
    dense = DeviceReplayBuffer(games, BATCH, (cfg.channels, cfg.rows, cfg.cols), cfg.num_actions, max_game_length=longest)
    compact = ScsReplayBuffer(games, BATCH, cfg, longest, sp.MAX_CHILDREN)
    bufs = {"dense": dense, "compact": compact}
    save, gather = {"dense": [], "compact": []}, {"dense": [], "compact": []}
    for rep in range(reps + 1):                            # rep 0 warms up both classes
        for key, buf in bufs.items():
            buf.index = ReplayIndex(buf.window_size, buf.capacity)     # every save fills an empty window
            t = timed(lambda: buf.save_scs_games(sp, ex, 0))
            if rep:
                save[key].append(t)
    def sample_batches(buf):
        for _ in range(GATHERS):
            buf.get_sample(BATCH, True, [])

    for rep in range(reps + 1):                            # a repeat is GATHERS batches, sampled and gathered back to back
        for key, buf in bufs.items():
            np.random.seed(rep)
            t = timed(lambda: sample_batches(buf)) / GATHERS
            if rep:
                gather[key].append(t)
    np.random.seed(99); a = dense.get_sample(BATCH, True, [])
    np.random.seed(99); b = compact.get_sample(BATCH, True, [])
    same = all(torch.equal(x, y) for x, y in ((a.states, b.states), (a.policies, b.policies), (a.values, b.values),
                                              (a.game_index, b.game_index)))
    dense.check(); compact.check()
    dense_row = (cfg.channels * cfg.rows * cfg.cols + cfg.num_actions + 2) * 4
    out = {"config": name, "games": games, "positions": int(lengths.sum()), "longest_game": longest,
           "max_moves": sp.MAX_MOVES, "max_children": sp.MAX_CHILDREN, "batches_equal": bool(same),
           "save_round": {k: summary(v) for k, v in save.items()},
           "gather_%d" % BATCH: {k: summary(v) for k, v in gather.items()}, "gather_batches_per_repeat": GATHERS,
           "bytes_per_position": {"dense": dense_row, "compact": compact.bytes_per_position},
           # what each class allocates for this window at the engine's bound on a game's decisions (window x MAX_MOVES slots)
           "window_bytes_at_max_moves": {"dense": games * sp.MAX_MOVES * dense_row,
                                         "compact": games * sp.MAX_MOVES * compact.bytes_per_position}}
    dense.close(); compact.close(); sp.close(); net.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scs_replay_timing.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "simulations": 16, "network": "ConvNet(32, 2)", "cases": []}
    for name in ("mirrored_5x5", "ten_by_ten"):
        res["cases"].append(case(name, a.games, a.reps))
        print(json.dumps(res["cases"][-1]), file=sys.stderr, flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
