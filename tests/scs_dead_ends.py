"""Test infrastructure: searches that start next to (or on) a live SCS position without a legal action, CPU only.

Directed play reaches such dead ends (tests/scs_directed.py, DEAD_ENDS: a placement whose every arrival tile the enemy
holds).  oracle/search.py's semantics there: a dead-end leaf is evaluated, its expansion appends no child, its value is
backed up, and because the node stays unexpanded every later visit evaluates it again -- with a positive value the
search piles its visits on it.  A game that steps onto one raises in the next move's `max_action` (IndexError: the root
has no children), as the reference does; a game that steps past one carries a visited, childless, live node through the
re-rooting.

A case is a walk of DEAD_ENDS, a number of plies to stop before the walk's end (0: the search starts on the dead end
itself), a search (simulations, training, seed), a number of moves and an evaluation.  `run_case` plays it on the
oracle -- with the case's own evaluation, or replayed from evaluations a device recorded (the twin of
tests/scs_replay.py::replay_game, which cannot be used here: it lets the IndexError through) -- under a counting
Explorer that observes the oracle and never changes it (as scs_directed.Situations does for the rules).
tests/test_scs_dead_ends_host.py holds the cases to floors on those counts; tests/test_gpu_scs_dead_ends.py plays them
on the device."""
import os
import sys
from collections import Counter, namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for _p in (REPO, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import scs_directed as sd                                           # noqa: E402

PLAYS_ON, REACHES, STARTS_ON = "plays on", "reaches the dead end", "starts on it"
# ending: (PLAYS_ON, moves played) / (REACHES, searched moves before the dead-end root) / (STARTS_ON, 0)
Case = namedtuple("Case", "walk back sims training seed moves evaluation ending")

W = {w.label: w for w in sd.DEAD_ENDS}
T48, T71 = W["two_types_6x5-advance-48"], W["two_types_6x5-advance-71"]
O20, O49 = W["one_type_6x5-advance-20"], W["one_type_6x5-advance-49"]

CASES = [
    Case(T71, 1, 48, False, 0, 2, "flat", (REACHES, 1)),
    Case(O20, 1, 48, False, 0, 2, "flat", (REACHES, 1)),
    Case(O20, 3, 32, True, 5, 4, "flat", (REACHES, 3)),
    Case(T48, 3, 32, False, 0, 4, "flat", (PLAYS_ON, 4)),
    Case(T48, 2, 32, True, 7, 3, "flat", (PLAYS_ON, 3)),
    Case(O49, 2, 32, False, 0, 3, "net", (REACHES, 2)),
    Case(O49, 3, 32, True, 5, 4, "net", (PLAYS_ON, 4)),
    Case(O49, 3, 32, False, 0, 4, "net", (PLAYS_ON, 4)),
    Case(O49, 1, 32, False, 0, 2, "net", (REACHES, 1)),
    Case(O20, 2, 32, False, 0, 3, "net", (REACHES, 2)),
    Case(T71, 0, 8, False, 0, 1, "flat", (STARTS_ON, 0)),
    Case(O20, 0, 8, True, 3, 1, "net", (STARTS_ON, 0)),
]


def case_id(c):
    return f"{c.walk.label}-back{c.back}-{c.sims}sims-{'train' if c.training else 'eval'}-{c.evaluation}"


def search_config(sims):
    """Configs/Search/a1_search_config.yaml of the reference (tests/test_gpu_scs_configs.py::a1_search)."""
    return {"Simulation": {"mcts_simulations": sims, "keep_subtree": True}, "UCT": {"pb_c_base": 10000, "pb_c_init": 1.15},
            "Exploration": {"number_of_softmax_moves": 0, "epsilon_softmax_exploration": 0.04,
                            "epsilon_random_exploration": 0.001, "value_factor": 1,
                            "root_exploration_distribution": "gamma", "root_exploration_fraction": 0.2,
                            "root_dist_alpha": 0.15, "root_dist_beta": 1}}


def prefix_of(case):
    """The actions from the start to the position the case's search starts in."""
    actions = case.walk.games()[0].actions
    assert case.walk.games()[0].dead_end and 0 <= case.back <= 3 < len(actions)
    return list(actions[:len(actions) - case.back])


NET = ("convnet", 32, 2)            # _net of tests/test_gpu_scs_replay_compact.py: synthetic_weights(4, ..., 2.0)


def net_weights(cfg):
    from nuzero_amd.weights import synthetic_weights, convnet_param_shapes
    return synthetic_weights(4, convnet_param_shapes(cfg.channels, cfg.planes, 3, NET[1], NET[2]), 2.0)


def oracle_net(cfg, dtype=None):
    import torch
    from oracle.net import FeedForwardRef
    return FeedForwardRef(net_weights(cfg), NET[0], NET[2], dtype=dtype or torch.float32)


def _evaluator(case, game):
    from scipy.special import softmax
    from scs_eval import evaluate_image, evaluate_image_peaked
    A = game.get_num_actions()
    if case.evaluation == "net":
        ref = oracle_net(game.cfg)

        def ev(g):
            logits, value = ref.inference(g.state_image(), None)
            return softmax(logits.reshape(-1)), np.float32(value.reshape(-1)[0])
        return ev
    fn = {"flat": evaluate_image, "peaked": evaluate_image_peaked}[case.evaluation]
    return lambda g: fn(g.state_image()[0], A)


def _replaying(digests, probs, values, cursor):
    """replay_game's evaluator (tests/scs_replay.py): the recorded evaluation, after checking the leaf image's digest."""
    from scs_replay import image_digest, image_mix_digest

    def ev(g):
        i = cursor[0]
        if i >= len(values):
            raise AssertionError("the oracle asks for more evaluations than the device search used")
        if digests.dtype == np.uint64:
            same = np.array_equal(image_mix_digest(g.state_image()[0]), digests[i])
        else:
            same = image_digest(g.state_image()[0]) == digests[i].tobytes()
        if not same:
            raise AssertionError(f"leaf {i}: the oracle's leaf image is not the one the device evaluated")
        cursor[0] = i + 1
        return probs[i], values[i]
    return ev


def _counting_explorer(search, training, rs, log):
    """oracle/search.py's Explorer with `evaluate` observed: every evaluation of a live leaf is logged as a dict
    (index, dead_end, depth, again, n_legal, image, value, node).  Nothing the search reads is touched."""
    from oracle import search as osearch

    class Counting(osearch.Explorer):
        root_length = 0
        seen = {}                                   # id(node) -> node: every node evaluated so far (kept alive)

        def evaluate(self, node, game, evaluator):
            before = self.counters.expansions
            value = super().evaluate(node, game, evaluator)
            if self.counters.expansions != before:  # (a terminal leaf is not an evaluation)
                log.append({"index": len(log), "dead_end": not node.children, "depth": game.get_length() - self.root_length,
                            "again": id(node) in self.seen, "n_legal": len(node.children),
                            "image": game.state_image()[0].astype(np.float32), "node": node,
                            "value": value})
                self.seen[id(node)] = node
            return value
    e = Counting(search, training, rs)
    e.seen = {}
    return e


def _childless_visited(root):
    """Visited, childless, non-terminal nodes of root's subtree (the new root included)."""
    n, stack = 0, [root]
    while stack:
        node = stack.pop()
        if node.visit_count > 0 and not node.children and node.terminal_value is None:
            n += 1
        stack.extend(node.children)
    return n


def run_case(case, recorded=None):
    """The oracle's run of a case: up to case.moves searched moves from the case's position.  recorded = (digests, probs,
    values): replay from a device's evaluations instead of the case's own evaluation.  Returns replay_game's dict
    (trace, length, evaluations_used / _recorded, peak_nodes ...) and: "situations" (Counter), "depths" (set),
    "dead_end_root" (the game stopped on a root without children: the oracle raised IndexError in max_action, after
    `sims` evaluations of that root), "live_nodes" (per played move, after its search), "simulations", "expansions",
    "evaluations" (the log: dicts with index, dead_end, depth, again, image, value), "rng_state" (the stream afterwards)."""
    from oracle import search as osearch
    game = sd.new_game(case.walk.name)
    prefix = prefix_of(case)
    for a in prefix:
        game.step_index(int(a))
    rs = np.random.RandomState(int(case.seed))
    search, log, cursor = search_config(case.sims), [], [0]
    ev = _replaying(*recorded, cursor) if recorded is not None else _evaluator(case, game)
    explorer = _counting_explorer(search, case.training, rs, log)
    root = osearch.Node(0)
    sit, trace, live, dead_end_root, first_dead = Counter(), [], [], False, None
    while not game.is_terminal() and len(trace) < case.moves:
        explorer.root_length = game.get_length()
        at = len(log)
        try:
            action, chosen, bias = explorer.run_mcts(game, ev, root)
        except IndexError:
            # max_action on a root without children; every simulation of the move evaluated the root
            assert not root.children and len(log) - at == case.sims and all(e["node"] is root for e in log[at:])
            dead_end_root = True
            break
        if first_dead is None and any(e["dead_end"] for e in log):
            first_dead = len(trace)
        trace.append({"action": int(action), "root_visits": int(root.visit_count), "root_value_sum": float(root.value_sum),
                      "bias": float(bias), "child_actions": [c.action for c in root.children],
                      "child_visits": [c.visit_count for c in root.children],
                      "child_priors": [float(c.prior) for c in root.children],
                      "child_value_sums": [float(c.value_sum) for c in root.children]})
        live.append(osearch.live_nodes(root))
        game.step_index(action)
        root = chosen
        sit["childless_visited_at_reroot"] += _childless_visited(root)
    dead = [e for e in log if e["dead_end"]]
    sit["dead_end_evaluations"] = len(dead)
    sit["dead_end_nodes"] = len({id(e["node"]) for e in dead})
    sit["re_evaluations"] = sum(1 for e in log if e["again"])
    sit["dead_end_re_evaluations"] = sum(1 for e in dead if e["again"])
    sit["dead_end_root_children"] = len({id(e["node"]) for e in dead if e["depth"] == 1})
    sit["moves_after_first_dead_end"] = 0 if first_dead is None else len(trace) - first_dead
    sit["ended_on_dead_end_root"] = int(dead_end_root)
    c = explorer.counters
    return {"trace": trace, "length": game.length, "terminal": bool(game.is_terminal()),
            "terminal_value": game.terminal_value if game.is_terminal() else None,
            "evaluations_used": cursor[0] if recorded is not None else len(log),
            "evaluations_recorded": len(recorded[2]) if recorded is not None else len(log),
            "peak_nodes": c.peak_nodes, "situations": sit, "depths": {e["depth"] for e in dead},
            "dead_end_root": dead_end_root, "live_nodes": live, "simulations": c.simulations, "expansions": c.expansions,
            "evaluations": [{k: v for k, v in e.items() if k != "node"} for e in log], "rng_state": rs.get_state(),
            "first": len(prefix)}


_DONE = {}      # a process's finished oracle runs: computed once, shared among its tests, never changed


def oracle_run(case):
    if case not in _DONE:
        _DONE[case] = run_case(case)
    return _DONE[case]


def ending_of(out):
    if out["dead_end_root"]:
        return (STARTS_ON, 0) if not out["trace"] else (REACHES, len(out["trace"]))
    return (PLAYS_ON, len(out["trace"]))
