#!/usr/bin/env python3
"""What the Tic-Tac-Toe network's plain-bf16 mode (SelfPlayEngine(precision="bf16")) gives back, measured: float32
mode against bf16 mode on the same box, the two modes alternating within every repetition, on bench.py's default
workload (RecurrentNet(2,1,64,2), 2 iterations, --games concurrent games, --sims simulations per move, rounds of
16 x --games games).

  selfplay   seconds and games/s of a whole round of the persistent kernel, median of --reps after one warm round per
             mode, with the round's expansions beside them (the modes play different games: the evaluations differ);
  phases     one stamped round per mode (the diagnostic build): a cycle's network-phase and tree-phase ticks;
  forward    nz_net_forward of --games positions (device events round --forward-iters calls).

Prints one JSON object; --out writes it.

    python scripts/time_ttt_bf16_mode.py [--reps 3] [--out profiles/ttt_bf16_mode_timing.json]
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

from nuzero_amd.engine import SelfPlayEngine                              # noqa: E402
from nuzero_amd.search_config import legacy_ttt_search_config             # noqa: E402
from nuzero_amd.weights import synthetic_recurrent_net_weights            # noqa: E402

MODES = ("float32", "bf16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096, help="concurrent games (slots)")
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--forward-iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: nothing here is measured without one"
    n_round = 16 * args.games
    cfg = legacy_ttt_search_config(args.sims)
    w = synthetic_recurrent_net_weights(0, 2, 1, 64, 2, True)
    engines = {}
    for m in MODES:
        engines[m] = SelfPlayEngine(cfg, n_round, training=True, device=0, n_slots=args.games, precision=m)
        engines[m].set_weights(w, recurrent_iterations=args.iters)
    out = {"device": torch.cuda.get_device_name(0),
           "workload": f"Tic-Tac-Toe, RecurrentNet(2,1,64,2) x {args.iters} iterations, {args.sims} sims/move, {args.games} "
                       f"concurrent games, rounds of {n_round} games (bench.py's default)", "reps": args.reps,
           "positions_per_pass": {m: engines[m].positions_per_pass for m in MODES}}

    def round_of(m, seed):
        eng = engines[m]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.play(base_seed=seed)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        c = eng.counters()
        return dt, int(c["expansions"]), int(c["simulations"])

    rows = {m: {"seconds": [], "expansions": [], "simulations": []} for m in MODES}
    for m in MODES:
        round_of(m, 0)                                    # warm: code objects, pinned buffers, the host random streams
    for rep in range(args.reps):
        for m in MODES:                                   # alternating: both modes see the same neighbours on the box
            dt, n_exp, n_sim = round_of(m, (1 + rep) * n_round)
            rows[m]["seconds"].append(round(dt, 4))
            rows[m]["expansions"].append(n_exp)
            rows[m]["simulations"].append(n_sim)
    for m in MODES:
        med = statistics.median(rows[m]["seconds"])
        i = rows[m]["seconds"].index(med)
        rows[m].update(median_s=med, games_per_s=round(n_round / med, 1),
                       round_ns_per_expansion=round(1e9 * med / rows[m]["expansions"][i], 3))
    rows["bf16_over_float32_games_per_s"] = round(rows["bf16"]["games_per_s"] / rows["float32"]["games_per_s"], 3)
    rows["bf16_over_float32_time_per_expansion"] = round(rows["bf16"]["round_ns_per_expansion"] /
                                                         rows["float32"]["round_ns_per_expansion"], 3)
    out["selfplay"] = rows

    out["phases"] = {}
    for m in MODES:
        eng = engines[m]
        eng.phase_stamps(True)
        eng.play(base_seed=7 * n_round)
        torch.cuda.synchronize()
        ph = eng.phase_stamps(False, read=True)
        out["phases"][m] = {k: round(ph[k], 1) for k in ("net_ticks_per_cycle", "tree_ticks_per_cycle", "cycles_per_workgroup",
                                                         "burst_passes_per_workgroup", "burst_sims_per_workgroup")}
    ph = out["phases"]
    ph["bf16_over_float32_net_ticks"] = round(ph["bf16"]["net_ticks_per_cycle"] / ph["float32"]["net_ticks_per_cycle"], 3)

    out["forward"] = {"positions": args.games}
    x = (torch.rand((args.games, 2, 3, 3), device="cuda") < 0.3).float().contiguous()
    for m in MODES:
        for _ in range(10):
            engines[m].net_forward(x)
        reps = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.forward_iters):
                engines[m].net_forward(x)
            b.record()
            torch.cuda.synchronize()
            reps.append(round(1e3 * a.elapsed_time(b) / args.forward_iters, 2))
        out["forward"][m] = {"us_per_call": reps, "median_us": statistics.median(reps)}
    fw = out["forward"]
    fw["bf16_over_float32_median"] = round(fw["bf16"]["median_us"] / fw["float32"]["median_us"], 3)
    fw["note"] = "a call = the network kernel + the softmax kernel + allocating the outputs"
    try:
        out["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True,
                                                stderr=subprocess.DEVNULL).strip() + " + this change"
    except Exception:
        out["commit"] = "unknown"
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    for e in engines.values():
        e.close()


if __name__ == "__main__":
    main()
