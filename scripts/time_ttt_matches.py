"""Time a Tic-Tac-Toe evaluation round: 4096 matches of MCTS (100 simulations per move, RecurrentNet(64, 2), 2 recurrent
iterations) against a random mover, seeds 5000...  Median of 3 interleaved runs on one box:

  library   nz_engine_match_play (TttAgentMatch.play): the whole round enqueued, one synchronisation;
  loop      the ply-by-ply Python loop of INTEGRATION.md section 5 over nz_engine_search / _apply / _last_actions, the
            random mover drawn by numpy on the host -- the only route before nz_engine_match_play.  With --loop-root PATH
            each loop run is a child process that imports nuzero_amd from that (built) checkout, e.g. the parent
            commit's; without it the loop runs in this process (those three entry points are unchanged from the parent).

Both routes must play the same games (checked in this process).  No threshold is set.  Prints one JSON object; --out
writes it.

    python scripts/time_ttt_matches.py [--matches 4096] [--sims 100] [--reps 3] [--loop-root PATH] [--out profiles/ttt_match_timing.json]
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


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def loop_round(e, seeds):
    """MCTS (engine e, player 1) against numpy random movers, ply by ply from Python; returns actions [N, 9]."""
    n = e.n_games
    rs = [np.random.RandomState(int(s)) for s in seeds]
    empty = np.ones((n, 9), bool)
    actions = np.full((n, 9), -1, np.int32)
    e.reset()
    for ply in range(9):
        alive = e.alive().cpu().numpy() != 0
        if not alive.any():
            break
        e.search()
        if ply % 2 == 0:
            e.apply()
            a = e.last_actions().cpu().numpy()
        else:
            a = np.full((n,), -1, np.int32)
            for j in np.flatnonzero(alive):
                cells = np.flatnonzero(empty[j])
                a[j] = cells[rs[j].randint(len(cells))]
            e.apply(actions=a)
        live = np.flatnonzero(alive)
        actions[live, ply] = a[live]
        empty[live, a[live]] = False
    return actions


def make_engine(cfg, n, weights):
    from nuzero_amd.engine import SelfPlayEngine
    e = SelfPlayEngine(cfg, n, training=False)
    e.set_weights(weights, recurrent_iterations=2)
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matches", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-root", default=None, help="a built checkout whose nuzero_amd the loop runs on (child processes)")
    ap.add_argument("--loop-only", action="store_true", help="(child process) warm up, time ONE loop round, print its seconds")
    ap.add_argument("--root", default=ROOT, help="(child process) the checkout to import nuzero_amd from")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_ttt_matches.py measures on the GPU; there is none")
    sys.path.insert(0, os.path.abspath(a.root))
    from nuzero_amd.search_config import legacy_ttt_search_config
    from nuzero_amd.weights import synthetic_recurrent_net_weights
    N, cfg = a.matches, legacy_ttt_search_config(a.sims)
    weights = synthetic_recurrent_net_weights(0, 2, 1, 64, 2, True)
    seeds = list(range(5000, 5000 + N))

    if a.loop_only:
        e = make_engine(cfg, N, weights)
        loop_round(e, seeds)
        t, _ = timed(lambda: loop_round(e, seeds))
        e.close()
        print(json.dumps({"loop_s": t}))
        return

    from nuzero_amd.tester import TttAgentMatch
    m = TttAgentMatch(("mcts", cfg), ("random",), N)
    e = make_engine(cfg, N, weights)
    warm = m.play(weights, None, agent_seeds=seeds, recurrent_iterations=2)          # warm-up: code objects, buffers
    same = bool(np.array_equal(loop_round(e, seeds), warm["actions"]))

    def child_loop():
        cmd = [sys.executable, os.path.abspath(__file__), "--loop-only", "--root", os.path.abspath(a.loop_root),
               "--matches", str(N), "--sims", str(a.sims)]
        out = subprocess.run(cmd, capture_output=True, text=True, check=True, timeout=600).stdout
        return json.loads(out.strip().splitlines()[-1])["loop_s"]

    lib, lib_play, loop = [], [], []
    for _ in range(a.reps):                                    # interleaved
        t, _ = timed(lambda: m.play(weights, None, agent_seeds=seeds, recurrent_iterations=2))
        lib.append(t)
        # the round alone, without handing the weights to the engine again (play() packs and uploads them every call)
        m._load = lambda *args: None
        t, _ = timed(lambda: m.play(weights, None, agent_seeds=seeds, recurrent_iterations=2))
        del m._load
        lib_play.append(t)
        loop.append(child_loop() if a.loop_root else timed(lambda: loop_round(e, seeds))[0])
    m.close()
    e.close()

    med = statistics.median
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    out = {"device": torch.cuda.get_device_name(0), "commit": commit or None, "matches": N, "simulations": a.sims,
           "pairing": "MCTS vs random", "net": "RecurrentNet(64, 2), 2 iterations",
           "library_with_weight_upload_s": [round(x, 4) for x in lib], "library_round_s": [round(x, 4) for x in lib_play],
           "loop_s": [round(x, 4) for x in loop], "loop_library": "child process on --loop-root" if a.loop_root else "this build",
           "library_with_weight_upload_median_s": round(med(lib), 4), "library_round_median_s": round(med(lib_play), 4),
           "loop_median_s": round(med(loop), 4), "same_games_on_both": same,
           "p1_wins_p2_wins_draws": [warm["p1_wins"], warm["p2_wins"], warm["draws"]]}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
