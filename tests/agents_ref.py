"""Test infrastructure: CPU restatements of the two scripted evaluation agents of nz_scs_agent_match_play, usable by
`oracle.agents.play_match` (new_game / choose_action), and the oracle replay of an agent match.

The agents' rules are harness rules (the reference's Testing/Agents sources are not restated in
this repository, parity unpinned):
  * PolicyAgentRef: evaluates the current position and plays the legal action of largest softmax probability, the
    lowest flat action index winning a tie (np.argmax); no search, nothing on the opponent's turn;
  * RandomAgentRef: owns np.random.RandomState(seed); at each of its own decisions with n legal actions it draws
    k = randint(n) -- restated here word by word as numpy's legacy masked rejection on 32-bit words, n == 1 draws
    nothing -- and plays the k-th legal action in ascending flat action index.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (REPO, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def next_u32(rs):
    """One tempered 32-bit word of the MT19937 stream (what random_uint32 hands to randint's rejection loop)."""
    return int.from_bytes(rs.bytes(4), "little")


def legacy_randint(rs, n):
    """RandomState.randint(n) for 1 <= n <= 2**32, restated: mask = the smallest 2**b - 1 >= n - 1; 32-bit words are
    drawn and masked until one is <= n - 1; n == 1 returns 0 and draws nothing."""
    if n < 1:
        raise ValueError("no legal action")
    if n == 1:
        return 0
    rng = n - 1
    mask = rng
    for sh in (1, 2, 4, 8, 16):
        mask |= mask >> sh
    while True:
        v = next_u32(rs) & mask
        if v <= rng:
            return v


class RandomAgentRef:
    def __init__(self, seed):
        self.seed = int(seed)
        self.new_game()

    def new_game(self):
        self.rs = np.random.RandomState(self.seed)
        self.n_legal, self.actions = [], []

    def choose_action(self, game):
        legal = np.flatnonzero(np.asarray(game.possible_actions()).reshape(-1))
        k = legacy_randint(self.rs, len(legal))
        self.n_legal.append(len(legal))
        self.actions.append(int(legal[k]))
        return self.actions[-1]


class PolicyAgentRef:
    """evaluator(game) -> (probs [A], value)."""

    def __init__(self, evaluator, keep_images=False):
        self.evaluator, self.keep_images = evaluator, keep_images
        self.new_game()

    def new_game(self):
        self.n_legal, self.actions, self.probs, self.images = [], [], [], []

    def choose_action(self, game):
        probs, _ = self.evaluator(game)
        probs = np.asarray(probs, np.float32).reshape(-1)
        mask = np.asarray(game.possible_actions()).reshape(-1) != 0
        a = int(np.argmax(np.where(mask, probs, -np.inf)))           # first maximum: the lowest index of a tie
        assert mask[a]
        self.n_legal.append(int(mask.sum()))
        self.actions.append(a)
        self.probs.append(float(probs[a]))
        if self.keep_images:
            self.images.append(np.array(game.state_image()[0], np.float32))
        return a


def replay_agent_match(args):
    """(config path, spec 1, spec 2[, seed[, game_map]]) -> dict.  spec: ("mcts", search_cfg, records) |
    ("policy", records) | ("random", seed); records = (digests uint64 [n, 2], probs [n, A], values [n]) the DEVICE
    agent recorded -- the replay never computes an evaluation itself (match_replay.RecordedEvaluations).  Top-level:
    it can run in a worker process."""
    config_path, spec1, spec2 = args[:3]
    seed = args[3] if len(args) > 3 else None
    game_map = args[4] if len(args) > 4 else None
    from match_replay import RecordedEvaluations, oracle_game
    from oracle.agents import MctsAgentRef, play_match
    game = oracle_game(config_path, seed, game_map)
    agents, evs = [], []
    for i, spec in enumerate((spec1, spec2)):
        ev = None
        if spec[0] == "mcts":
            ev = RecordedEvaluations(*spec[2], label=f"agent {i + 1}")
            agents.append(MctsAgentRef(spec[1], ev))
        elif spec[0] == "policy":
            ev = RecordedEvaluations(*spec[1], label=f"agent {i + 1}")
            agents.append(PolicyAgentRef(ev, keep_images=True))
        else:
            agents.append(RandomAgentRef(spec[1]))
        evs.append(ev)
    movers, g2 = [], oracle_game(config_path, seed, game_map)
    actions = play_match(game, agents[0], agents[1])
    for a in actions:                                       # who decided what: side 0 moves for player index 1
        movers.append(0 if g2.get_current_player() == 1 else 1)
        g2.step_index(int(a))
    out = {"actions": [int(a) for a in actions], "movers": movers, "length": int(game.length),
           "terminal_value": int(game.terminal_value), "sides": []}
    for ag, ev in zip(agents, evs):
        d = {"lookups": ev.lookups if ev else 0, "recorded": len(ev.values) if ev else 0, "unused": ev.unused() if ev else []}
        if not isinstance(ag, MctsAgentRef):
            d.update(n_legal=ag.n_legal, agent_actions=ag.actions)
        if isinstance(ag, PolicyAgentRef):
            d.update(probs=ag.probs, images=ag.images)
        out["sides"].append(d)
    return out


def replay_agent_matches(jobs, workers=None):
    """Several matches, in worker processes when there is more than one (as match_replay.replay_matches)."""
    if len(jobs) <= 1 or workers == 1:
        return [replay_agent_match(j) for j in jobs]
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor
    workers = workers or min(len(jobs), max(1, (os.cpu_count() or 2) - 1), 12)
    with ProcessPoolExecutor(max_workers=workers, mp_context=mp.get_context("spawn")) as ex:
        return list(ex.map(replay_agent_match, jobs))
