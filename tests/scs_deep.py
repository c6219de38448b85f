"""Test infrastructure: the cases on which an SCS search descends past 64 levels, and the oracle's run of each.

Both device search routes keep the first 64 levels of a descent apart from the rest (one path entry per lane, the tail
in memory), so they need games whose searches go deeper than that.  A path cannot be longer than the decisions left in
the game plus one; `two_types_6x5` plays 105-125 decisions, and an evaluation whose best legal action clearly dominates,
with a near-constant positive value (SCS never negates Q), keeps a search on the line it has visited:

  * `evaluate_image_peaked` (tests/scs_eval.py) for the host-evaluator route, on `two_types_6x5`;
  * `peaked_net_weights` for the library's routes: ConvNet 32 x 2 (a width and depth the persistent route takes) with
    the policy head's last conv times POLICY_SCALE and a relu value head whose last conv is made non-negative (the
    nets have no biases; the layer's inputs are relu outputs, so its mean is positive: values of 0.91-0.999 at the
    root positions of the games below).  Trunk and policy head are sparse (one weight in 32), which keeps float32
    arithmetic accurate enough at logits of up to 130 for a comparison of probabilities at 1e-5.  It plays
    `one_type_6x5` (103 and 113 decisions): the persistent route refuses `two_types_6x5`, whose 105 input planes on
    30 cells do not fit a wavefront's share of LDS; with stacking 2 the image has 86 planes.

Scale, value head, simulation count and seeds were chosen on the CPU with oracle/search.py;
tests/test_scs_deep_paths_host.py asserts, on the oracle alone, that every case below goes as deep as the device tests
(tests/test_gpu_scs_deep_paths.py) need."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if REPO not in sys.path:
    sys.path.insert(0, REPO)

CONFIG = os.path.join(HERE, "golden", "scs_configs", "two_types_6x5.yml")
NET_CONFIG = os.path.join(HERE, "golden", "scs_configs", "one_type_6x5.yml")
SIMS = 150
NET = ("convnet", 32, 2, "relu")          # arch, width, depth, value head activation
NET_SEED, NET_GAIN, POLICY_SCALE = 43, 2.5, 45.0
NET_KEEP = 1.0 / 32        # the share of the trunk's and the policy head's weights that is not zero

# (evaluation, training, seeds): two games each.  Without training there is no noise and no drawn move: the seeds do
# not matter and both games are the same one.
HOST_EVAL_CASES = [("peaked", True, (70, 71)), ("peaked", False, (70, 70))]
NET_CASES = [("net", True, (73, 74))]


def deep_search(sims=SIMS):
    """Configs/Search/a1_search_config.yaml of the reference with exploration switched up."""
    return {"Simulation": {"mcts_simulations": sims, "keep_subtree": True}, "UCT": {"pb_c_base": 10000, "pb_c_init": 1.15},
            "Exploration": {"number_of_softmax_moves": 2, "epsilon_softmax_exploration": 0.1,
                            "epsilon_random_exploration": 0.05, "value_factor": 1,
                            "root_exploration_distribution": "gamma", "root_exploration_fraction": 0.2,
                            "root_dist_alpha": 0.3, "root_dist_beta": 1}}


def peaked_net_weights(channels, planes):
    from nuzero_amd.weights import synthetic_weights, convnet_param_shapes
    arch, width, depth, _ = NET
    assert arch == "convnet"
    w = synthetic_weights(NET_SEED, convnet_param_shapes(channels, planes, 3, width, depth), NET_GAIN)
    # Sparse convolutions: logits of this size (up to 130) come out of float32 arithmetic with a rounding error that
    # grows with the number of terms a convolution adds up.  With one weight in 32 kept (and those scaled up to keep the
    # activations' size) the float32 oracle stays within 0.31e-5 of the float64 one on the probabilities, so a
    # comparison at 1e-5 has room (dense, at the scale of 30 it needs: 1.4e-5, more than the bound itself; an MI355X was
    # 1.1e-5 from the float32 oracle on that net).  Held by tests/test_scs_deep_paths_host.py.
    rs = np.random.RandomState(1000 + NET_SEED)
    for name in w:
        if not name.startswith("value_head"):
            kept = rs.random_sample(w[name].shape) < NET_KEEP
            w[name] = (w[name] * kept / np.sqrt(NET_KEEP)).astype(np.float32)
    w["policy_head.layers.2.weight"] = w["policy_head.layers.2.weight"] * np.float32(POLICY_SCALE)
    w["value_head.layers.6.weight"] = np.abs(w["value_head.layers.6.weight"])
    return w


def oracle_game(args):
    """(config path, search config, seed, training, evaluation, max_moves) -> the oracle's game as
    tests/scs_replay.py::replay_game reports it (per-move trace, length, outcome, path-depth measures, peak node
    count).  evaluation: "peaked" / "flat" (evaluate_image_peaked / evaluate_image on the state image) or "net" (the
    oracle network on peaked_net_weights).  Top-level so it can run in a worker process."""
    config_path, search, seed, training, evaluation, max_moves = args
    from oracle import search as osearch
    from oracle.scs import ScsConfig, ScsGame
    from scs_eval import evaluate_image, evaluate_image_peaked
    cfg = ScsConfig(config_path)
    game = ScsGame(cfg)
    A = game.get_num_actions()
    if evaluation == "net":
        from oracle.net import FeedForwardRef
        arch, _, depth, vact = NET
        ev = osearch.net_evaluator(FeedForwardRef(peaked_net_weights(cfg.channels, cfg.planes), arch, depth, vact), None)
    else:
        fn = {"peaked": evaluate_image_peaked, "flat": evaluate_image}[evaluation]
        ev = lambda gm: fn(gm.state_image()[0], A)
    explorer = osearch.Explorer(search, training, np.random.RandomState(int(seed)))
    root = osearch.Node(0)
    trace = []
    while not game.is_terminal() and (not max_moves or len(trace) < max_moves):
        action, chosen, bias = explorer.run_mcts(game, ev, root)
        trace.append({"action": int(action), "root_visits": int(root.visit_count), "root_value_sum": float(root.value_sum),
                      "bias": float(bias),
                      "child_actions": [c.action for c in root.children],
                      "child_visits": [c.visit_count for c in root.children],
                      "child_priors": [float(c.prior) for c in root.children],
                      "child_value_sums": [float(c.value_sum) for c in root.children]})
        game.step_index(action)
        root = chosen
    c = explorer.counters
    return {"trace": trace, "length": game.length, "terminal": bool(game.is_terminal()),
            "terminal_value": game.terminal_value if game.is_terminal() else None,
            "longest_path": c.longest_path, "path_lengths": dict(c.path_lengths),
            "terminal_path_lengths": dict(c.terminal_path_lengths), "peak_nodes": c.peak_nodes}


def oracle_games(jobs):
    """oracle_game for every job, distinct jobs in worker processes side by side (spawned: a parent may hold a GPU)."""
    keys = [repr(j) for j in jobs]
    todo = {k: j for k, j in zip(keys, jobs) if k not in _DONE}
    if len(todo) == 1:
        for k, j in todo.items():
            _DONE[k] = oracle_game(j)
    elif todo:
        import multiprocessing as mp
        from concurrent.futures import ProcessPoolExecutor
        workers = min(len(todo), max(1, (os.cpu_count() or 2) - 1), 12)
        with ProcessPoolExecutor(max_workers=workers, mp_context=mp.get_context("spawn")) as ex:
            for k, out in zip(todo, ex.map(oracle_game, list(todo.values()))):
                _DONE[k] = out
    return [_DONE[k] for k in keys]


_DONE = {}      # a process's finished oracle games: computed once, shared among its tests, never changed


def deep_jobs(cases):
    return [(NET_CONFIG if evaluation == "net" else CONFIG, deep_search(), seed, training, evaluation, None)
            for evaluation, training, seeds in cases for seed in seeds]


def simulations_deeper_than(out, length, terminal=False):
    hist = out["terminal_path_lengths" if terminal else "path_lengths"]
    return sum(n for plen, n in hist.items() if plen > length)


def pending_leaves(out, length):
    """Simulations of the game whose path had `length` nodes and ended in a leaf that needs an evaluation."""
    return out["path_lengths"].get(length, 0) - out["terminal_path_lengths"].get(length, 0)
