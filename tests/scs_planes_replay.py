"""scs_replay.replay_game's oracle replay of one recorded SCS game that also KEEPS every leaf's planes, for tests that
evaluate the recorded leaves again (tests/test_gpu_scs_bf16.py: every recorded leaf is nz_boardnet_forward of its
planes).  A plain module: its functions run in worker processes (CPU only: nothing here touches the GPU)."""
import os

import numpy as np


def replay_keeping_planes(args):
    """(config path, search config, seed, digests uint64 [n, 2], probs [n, A], values [n][, max_moves]) -> {"trace",
    "length", "terminal", "terminal_value", "evaluations_used", "evaluations_recorded", "planes" float32 [n, C, rows,
    cols]}: the planes in the order the device's search consumed the evaluations, each checked against the recorded
    digest.  max_moves (optional; None or 0: the whole game): the replay stops after that many decisions, as
    play_native(..., max_moves) does; terminal_value is then None unless the game ended within them."""
    path, search, seed, dig, probs, values = args[:6]
    max_moves = args[6] if len(args) > 6 else None
    from oracle import search as osearch
    from oracle.scs import ScsConfig, ScsGame
    from scs_replay import image_mix_digest
    rs = np.random.RandomState(int(seed))
    game = ScsGame(ScsConfig(path))
    planes, cursor = [], [0]

    def ev(g):
        i = cursor[0]
        if i >= len(values):
            raise AssertionError("the oracle asks for more evaluations than the device search used")
        img = g.state_image()
        if not np.array_equal(image_mix_digest(img[0]), dig[i]):
            raise AssertionError(f"leaf {i}: the oracle's leaf image is not the one the device evaluated")
        planes.append(np.asarray(img[0], np.float32).copy())
        cursor[0] = i + 1
        return probs[i], values[i]

    explorer = osearch.Explorer(search, True, rs)
    root, trace = osearch.Node(0), []
    while not game.is_terminal() and (not max_moves or len(trace) < max_moves):
        action, chosen, bias = explorer.run_mcts(game, ev, root)
        trace.append({"action": int(action), "root_visits": int(root.visit_count), "root_value_sum": float(root.value_sum),
                      "bias": float(bias), "child_actions": [c.action for c in root.children],
                      "child_visits": [c.visit_count for c in root.children],
                      "child_priors": [float(c.prior) for c in root.children],
                      "child_value_sums": [float(c.value_sum) for c in root.children]})
        game.step_index(action)
        root = chosen
    terminal = bool(game.is_terminal())
    return {"trace": trace, "length": game.length, "terminal": terminal,
            "terminal_value": game.terminal_value if terminal else None, "evaluations_used": cursor[0],
            "evaluations_recorded": len(values), "planes": np.stack(planes)}


def replay_games_keeping_planes(jobs, workers=None):
    """Several games, in worker processes (spawned: the parent holds a GPU), as scs_replay.replay_games."""
    if len(jobs) <= 1 or workers == 1:
        return [replay_keeping_planes(j) for j in jobs]
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor
    workers = workers or min(len(jobs), max(1, (os.cpu_count() or 2) - 1), 12)
    with ProcessPoolExecutor(max_workers=workers, mp_context=mp.get_context("spawn")) as ex:
        return list(ex.map(replay_keeping_planes, jobs))
