"""Test infrastructure of the Tic-Tac-Toe evaluation matches (nz_engine_match_play): the oracle replay of a match on
oracle/ttt.py with the agent restatements of tests/agents_ref.py (which fit the Tic-Tac-Toe oracle game as they are), a
seeded table evaluator both the library and the oracle read, and a numpy restatement of the random mover's rule on a 3x3
mask."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (REPO, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from agents_ref import PolicyAgentRef, RandomAgentRef, legacy_randint   # noqa: E402


def search_cfg(sims, keep=True):
    return {"Simulation": {"mcts_simulations": sims, "keep_subtree": keep}, "UCT": {"pb_c_base": 10000, "pb_c_init": 1.15},
            "Exploration": {"number_of_softmax_moves": 0, "epsilon_softmax_exploration": 0.04,
                            "epsilon_random_exploration": 0.001, "value_factor": 1,
                            "root_exploration_distribution": "gamma", "root_exploration_fraction": 0.2,
                            "root_dist_alpha": 0.15, "root_dist_beta": 1}}


def random_table(seed):
    """[3^9, 10] float32: the float32 softmax of seeded random logits, and a value in (-1, 1)."""
    rs = np.random.RandomState(seed)
    logits = rs.standard_normal((3 ** 9, 9)).astype(np.float32)
    e = np.exp(logits - logits.max(1, keepdims=True), dtype=np.float32)
    t = np.empty((3 ** 9, 10), np.float32)
    t[:, :9] = e / e.sum(1, keepdims=True, dtype=np.float32)
    t[:, 9] = rs.uniform(-1.0, 1.0, 3 ** 9).astype(np.float32)
    return t


def random_move_on_mask(rs, mask9):
    """The random mover's rule on a 3x3 mask of empty cells: k = randint(n_legal) by numpy's legacy masked rejection on
    32-bit words (n_legal == 1 draws nothing), then the k-th empty cell in ascending index."""
    cells = [c for c in range(9) if mask9[c]]
    return cells[legacy_randint(rs, len(cells))]


def make_agent(spec, table):
    """spec: ("mcts", search_cfg) | ("policy",) | ("random", seed)."""
    from oracle import search as osearch
    from oracle.agents import MctsAgentRef
    if spec[0] == "mcts":
        return MctsAgentRef(spec[1], osearch.table_evaluator(table))
    if spec[0] == "policy":
        return PolicyAgentRef(osearch.table_evaluator(table))
    return RandomAgentRef(spec[1])


def oracle_match(spec1, table1, spec2, table2):
    """One match on the oracle: actions, length, terminal value, per scripted side its own decisions by ply, and a random
    side's stream (RandomState.get_state()) after the match."""
    from oracle import ttt as ottt
    from oracle.agents import play_match
    game = ottt.TicTacToe()
    agents = [make_agent(spec1, table1), make_agent(spec2, table2)]
    actions = [int(a) for a in play_match(game, agents[0], agents[1])]
    out = {"actions": actions, "length": int(game.length), "terminal_value": int(game.terminal_value), "sides": []}
    for i, (spec, ag) in enumerate(zip((spec1, spec2), agents)):
        d = {}
        if spec[0] != "mcts":
            plies = list(range(i, len(actions), 2))                  # side 1 decides plies 0, 2, ...; side 2 plies 1, 3, ...
            assert len(plies) == len(ag.actions) == len(ag.n_legal)
            a9, n9 = [-1] * 9, [0] * 9
            for ply, a, n in zip(plies, ag.actions, ag.n_legal):
                a9[ply], n9[ply] = a, n
            d.update(agent_actions=a9, agent_n_legal=n9)
        if spec[0] == "random":
            st = ag.rs.get_state()
            d.update(keys=np.asarray(st[1], np.uint32), pos=int(st[2]))
        out["sides"].append(d)
    return out


def expected_record(games):
    """What nz_engine_match_play must return for these oracle games: actions [N, 9] (-1 past the end), lengths, outcomes
    and the 4-word tally (side-1 wins, side-2 wins, draws, unfinished)."""
    n = len(games)
    actions = np.full((n, 9), -1, np.int32)
    for i, g in enumerate(games):
        actions[i, :len(g["actions"])] = g["actions"]
    lengths = np.array([g["length"] for g in games], np.int32)
    outcomes = np.array([g["terminal_value"] for g in games], np.int32)
    tally = (int((outcomes > 0).sum()), int((outcomes < 0).sum()), int((outcomes == 0).sum()), 0)
    return actions, lengths, outcomes, tally
