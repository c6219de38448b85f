#!/usr/bin/env python3
"""Same-box A/B of the packed network pass (NZ_NET_PACKED=0 against NZ_NET_PACKED=8) on engines of a few games per
workgroup: 256, 512, 1024, 1536 and 2048 concurrent games (1, 2, 4, 6, 8 per workgroup on 256 CUs), 100 simulations.

    python scripts/ab_packed.py [--runs 3] [--sims 100] [--slots 256,512,...] [--rounds-per-slot 4]

The two settings alternate, `--runs` engines each; per engine one warm-up round, one timed round and one round of the
stamped build (network and tree ticks per cycle).  One JSON line per run, then per size the ranges and the verdict:
the packed pass wins where its slowest run beats the 16-column pass's fastest."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from nuzero_amd.engine import SelfPlayEngine  # noqa: E402
from nuzero_amd.search_config import legacy_ttt_search_config  # noqa: E402
from nuzero_amd.weights import synthetic_recurrent_net_weights  # noqa: E402


def one_run(setting, n_slots, sims, rounds_per_slot, weights):
    os.environ["NZ_NET_PACKED"] = setting
    n_games = n_slots * rounds_per_slot
    eng = SelfPlayEngine(legacy_ttt_search_config(sims), n_games, n_slots=n_slots)
    eng.set_weights(weights)
    eng.play(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.play(n_games)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    c = eng.counters()
    eng.phase_stamps(True)
    eng.play(2 * n_games)
    torch.cuda.synchronize()
    st = eng.phase_stamps(False, read=True)
    out = {"slots": n_slots, "NZ_NET_PACKED": setting, "positions_per_pass": eng.positions_per_pass,
           "games_per_s": n_games / dt, "simulations_per_s": c["simulations"] / dt, "round_ms": dt * 1e3,
           "net_ticks_per_cycle": st["net_ticks_per_cycle"], "tree_ticks_per_cycle": st["tree_ticks_per_cycle"],
           "cycles_per_workgroup": st["cycles_per_workgroup"]}
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--slots", default="256,512,1024,1536,2048")
    ap.add_argument("--rounds-per-slot", type=int, default=4)
    args = ap.parse_args()
    weights = synthetic_recurrent_net_weights(0, 2, 1, 64, 2, True)
    for n_slots in [int(s) for s in args.slots.split(",")]:
        runs = {"0": [], "8": []}
        for _ in range(args.runs):
            for setting in ("0", "8"):
                r = one_run(setting, n_slots, args.sims, args.rounds_per_slot, weights)
                runs[setting].append(r)
                print(json.dumps(r), flush=True)
        rate = {k: sorted(r["games_per_s"] for r in v) for k, v in runs.items()}
        ticks = {k: sum(r["net_ticks_per_cycle"] for r in v) / len(v) for k, v in runs.items()}
        print(json.dumps({"slots": n_slots, "positions_per_pass": runs["8"][0]["positions_per_pass"],
                          "games_per_s_16_column": [rate["0"][0], rate["0"][-1]],
                          "games_per_s_packed": [rate["8"][0], rate["8"][-1]],
                          "net_ticks_per_cycle_16_column": ticks["0"], "net_ticks_per_cycle_packed": ticks["8"],
                          "packed_wins": rate["8"][0] > rate["0"][-1]}), flush=True)


if __name__ == "__main__":
    main()
