#!/usr/bin/env python3
"""What the board nets' plain-bf16 mode gives back, measured: float32 mode against bf16 mode on the same box, the two modes
alternating within every repetition.

  selfplay     bench_scs.py's default workload (mirrored_5x5, ConvNet(32 filters x 8 layers), 200 simulations per move,
               1024 concurrent games, the library's move loop) on the persistent route and on the wave-by-wave route:
               seconds and games/s of a whole round, median of --reps after one warm round per (mode, route);
  netbench     nz_scs_netbench: shader ticks of one per-wavefront-pair network pass, 256 workgroups x 4 game slots;
  forward      nz_boardnet_forward of 1024 positions (device events round --forward-iters calls).

The two modes play different games (the evaluations differ), so a round's seconds are compared with its own number of
expansions beside them.  Prints one JSON object; --out writes it.

    python scripts/time_bf16_mode.py [--reps 3] [--out profiles/bf16_mode_timing.json]
"""
import argparse
import ctypes
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
CONFIG = os.path.join(ROOT, "tests", "golden", "scs_configs", "mirrored_5x5.yml")

from nuzero_amd._lib import lib                                           # noqa: E402
from nuzero_amd.boardnet import BoardNet                                  # noqa: E402
from nuzero_amd.scs import ScsGameConfig, ScsSelfPlay                     # noqa: E402
from nuzero_amd.weights import convnet_param_shapes, synthetic_weights    # noqa: E402

MODES = ("float32", "bf16")


def search(sims):       # bench_scs.py's (Configs/Search/a1_search_config.yaml)
    return {"Simulation": {"mcts_simulations": sims, "keep_subtree": True}, "UCT": {"pb_c_base": 10000, "pb_c_init": 1.15},
            "Exploration": {"number_of_softmax_moves": 0, "epsilon_softmax_exploration": 0.04,
                            "epsilon_random_exploration": 0.001, "value_factor": 1,
                            "root_exploration_distribution": "gamma", "root_exploration_fraction": 0.2,
                            "root_dist_alpha": 0.15, "root_dist_beta": 1}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--sims", type=int, default=200)
    ap.add_argument("--filters", type=int, default=32)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--forward-iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: nothing here is measured without one"
    cfg = ScsGameConfig(CONFIG)
    w = synthetic_weights(0, convnet_param_shapes(cfg.channels, cfg.planes, 3, args.filters, args.layers))
    nets = {}
    for mode in MODES:
        nets[mode] = BoardNet("convnet", cfg.channels, cfg.planes, cfg.rows, cfg.cols, width=args.filters,
                              num_blocks=args.layers, kernel_size=3, max_batch=args.games, precision=mode)
        nets[mode].set_weights(w, 1)
    sp = ScsSelfPlay(cfg, search(args.sims), args.games)
    seeds = list(range(args.games))
    out = {"device": torch.cuda.get_device_name(0),
           "workload": f"SCS {cfg.rows}x{cfg.cols}, ConvNet({args.filters} x {args.layers}), {args.sims} sims/move, "
                       f"{args.games} concurrent games, library move loop", "reps": args.reps, "selfplay": {}}

    def round_of(mode, persistent):
        sp.persistent(1 if persistent else 0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = sp.play_native(nets[mode], seeds)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert sp.persistent() is persistent
        return dt, int(r["expansions"]), int(r["lengths"].sum())

    for persistent in (True, False):
        route = "persistent" if persistent else "wave_by_wave"
        rows = {m: {"seconds": [], "expansions": None, "moves": None} for m in MODES}
        for m in MODES:
            round_of(m, persistent)                       # warm: code objects, the route's buffers
        for _ in range(args.reps):
            for m in MODES:                               # alternating: both modes see the same neighbours on the box
                dt, n_exp, moves = round_of(m, persistent)
                rows[m]["seconds"].append(round(dt, 4))
                rows[m]["expansions"], rows[m]["moves"] = n_exp, moves
        for m in MODES:
            med = statistics.median(rows[m]["seconds"])
            rows[m].update(median_s=med, games_per_s=round(args.games / med, 1),
                           round_us_per_expansion=round(1e6 * med / rows[m]["expansions"], 4))
        rows["bf16_over_float32_games_per_s"] = round(rows["bf16"]["games_per_s"] / rows["float32"]["games_per_s"], 3)
        rows["bf16_over_float32_time_per_expansion"] = round(rows["bf16"]["round_us_per_expansion"] / rows["float32"]["round_us_per_expansion"], 3)
        out["selfplay"][route] = rows

    out["netbench_ticks_per_pass"] = {}
    for m in MODES:
        ticks = np.zeros(256 * 4, np.uint64)
        st = lib.nz_scs_netbench(nets[m]._h, 256, 50, ctypes.c_void_p(ticks.ctypes.data))
        assert st == 0, st
        out["netbench_ticks_per_pass"][m] = {"min": int(ticks.min()), "median": int(np.median(ticks)), "max": int(ticks.max())}
    nb = out["netbench_ticks_per_pass"]
    nb["bf16_over_float32_median"] = round(nb["bf16"]["median"] / nb["float32"]["median"], 3)

    out["forward_1024"] = {}
    x = (torch.rand((args.games, cfg.channels, cfg.rows, cfg.cols), device="cuda") < 0.15).float().contiguous()
    for m in MODES:
        for _ in range(10):
            nets[m].forward(x)
        reps = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.forward_iters):
                nets[m].forward(x)
            b.record()
            torch.cuda.synchronize()
            reps.append(round(1e3 * a.elapsed_time(b) / args.forward_iters, 2))
        out["forward_1024"][m] = {"us_per_call": reps, "median_us": statistics.median(reps)}
    fw = out["forward_1024"]
    fw["bf16_over_float32_median"] = round(fw["bf16"]["median_us"] / fw["float32"]["median_us"], 3)
    fw["note"] = "a call = layout conversion + the one-launch network + allocating the outputs"
    try:
        out["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True,
                                                stderr=subprocess.DEVNULL).strip() + " + this change"
    except Exception:
        out["commit"] = "unknown"
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
