"""Evaluation matches between two MCTS agents on SCS, played inside the library (C ABI nz_scs_match_*).

The trainer's test step -- `Tester.Test_using_agents` with two `MctsAgent`s that keep their subtrees
(Testing/Tester.py:46-121, Testing/Agents/Generic/MctsAgent.py:28-39) -- for many matches at
once: `ScsMatch` holds two `ScsSelfPlay(training=False)` engines of one game config, one per agent, each with its own
search config, network and trees.  `play(net1, net2)` runs the whole move loop on the device: per decision both
engines search the position (on two streams), a hand-over kernel tells each engine what to play, and the tally is
counted there too.  Agent 1 moves when the game's player index is 1 (oracle/agents.py play_match); wins are the
game's terminal values (+1: player 1).

Evaluation agents are deterministic (no noise, max action), so matches on ONE map are copies of one game: a win rate
means something on the reference's "Randomized" presets, `ScsGameConfig(path, per_game=True)`, one map per match
drawn on the device from `seeds`.

Out of scope: `RandomAgent`, `PolicyAgent` and SCS's scripted agents (only what oracle/agents.py restates of the
reference's agents is built; the other agents' random draw order is not pinned anywhere in this repository), and
Tic-Tac-Toe (two deterministic agents play ONE game there: the two-engine loop of INTEGRATION.md section 5 covers
it, and there is no per-match variety to batch).
"""
from ctypes import byref, c_void_p

import numpy as np

_MAP_FIELDS = ("rows", "cols", "turns", "stacking", "n_vp", "terrain", "vp", "units", "arrival", "per_game")


def _same_game(c1, c2):
    return all(np.array_equal(np.asarray(getattr(c1, k)), np.asarray(getattr(c2, k))) for k in _MAP_FIELDS)


class ScsMatch:
    """n_matches matches between agent 1 (search_cfg_1) and agent 2 (search_cfg_2).  `config`: an ScsGameConfig (or a
    path), or a pair of them, one per agent, which must describe the same game.  `agents`: the two ScsSelfPlay engines
    (persistent(), record(), cache(), status(), export() work per agent as after play_native)."""

    def __init__(self, config, search_cfg_1, search_cfg_2, n_matches, device=0, training=False):
        from .scs import ScsGameConfig
        if training:
            raise ValueError("evaluation agents do not explore: MctsAgent builds Explorer(search_config, False) "
                             "(MctsAgent.py:14-20); training engines play self-play games (ScsSelfPlay.play_native)")
        for i, sc in enumerate((search_cfg_1, search_cfg_2)):
            if not sc["Simulation"]["keep_subtree"]:
                raise ValueError(f"agent {i + 1}: keep_subtree = False is not supported (an MctsAgent that drops its "
                                 "tree never re-roots, MctsAgent.py:28-39; every shipped search config keeps it)")
        if int(n_matches) <= 0:
            raise ValueError("n_matches must be positive")
        configs = tuple(config) if isinstance(config, (tuple, list)) else (config, config)
        if len(configs) != 2:
            raise ValueError("config: one game config, or one per agent")
        configs = tuple(c if isinstance(c, ScsGameConfig) else ScsGameConfig(c) for c in configs)
        if not _same_game(*configs):
            raise ValueError(f"the two agents' game configs differ ({configs[0].rows}x{configs[0].cols} and "
                             f"{configs[1].rows}x{configs[1].cols} boards): a match is one game")
        from .scs import ScsSelfPlay              # (needs the GPU from here on)
        self.cfg, self.n_matches = configs[0], int(n_matches)
        self.agents = (ScsSelfPlay(configs[0], search_cfg_1, self.n_matches, training=False, device=device),
                       ScsSelfPlay(configs[1], search_cfg_2, self.n_matches, training=False, device=device))

    def close(self):
        for a in self.agents:
            a.close()

    def play(self, net1, net2, seeds=None, max_moves=None):
        """One round: every match from the start to the end (or for `max_moves` decisions).  net1 / net2: the agents'
        BoardNets (max_batch >= n_matches).  `seeds` (per_game configs: required, one per match): match i is played on
        the map `np.random.seed(seeds[i]); SCS_Game(config)` builds, drawn on the device in both engines (the draw is
        a pure function of the seed); `agents[0].game_maps` holds the maps for whoever replays a match.
        Returns a dict: "actions" int32 [N, T] (-1 past a match's end; T = the longest match), "lengths" [N],
        "outcomes" [N] (terminal value from player 1's view; 0 while unfinished), "p1_wins", "p2_wins", "draws",
        "unfinished" (stopped at max_moves), "length_sum", "length_max"."""
        import torch
        from . import _lib
        a1, a2 = self.agents
        if self.cfg.per_game:
            if seeds is None:
                raise ValueError("a per_game config draws one map per match: pass seeds")
            seeds = list(seeds)
            if len(seeds) != self.n_matches:
                raise ValueError(f"{len(seeds)} seeds for {self.n_matches} matches")
            a1.set_games(seeds)
            a2.set_games(seeds)
        stream = c_void_p(torch.cuda.current_stream().cuda_stream)
        a1._check(_lib.lib.nz_scs_match_play(a1._h, net1._h, a2._h, net2._h, int(max_moves or 0), stream))
        tally = _lib.ScsMatchTally()
        actions = torch.empty((self.n_matches, a1.MAX_MOVES), dtype=torch.int32, device=a1.device)
        a1._check(_lib.lib.nz_scs_match_result(a1._h, a2._h, byref(tally), c_void_p(actions.data_ptr()), stream))
        st = a1.status()
        out = {k: int(getattr(tally, k)) for k, _ in _lib.ScsMatchTally._fields_}
        out["actions"] = actions[:, :max(1, out["length_max"])].cpu().numpy()
        out["lengths"], out["outcomes"] = st[:, 6].copy(), st[:, 5].copy()
        return out


class ScsTester:
    """The shape of the reference's Tester for SCS: `test_using_agents` plays n matches between two MCTS agents and
    returns (p1_wins, p2_wins, draws), as Test_using_agents counts them over n games (Tester.py:46-121)."""

    def __init__(self, config, device=0):
        self.config, self.device = config, device
        self._match = None

    def test_using_agents(self, search_cfg_1, net1, search_cfg_2, net2, n, seeds=None, max_moves=None):
        key = (repr(search_cfg_1), repr(search_cfg_2), int(n))
        if self._match is None or self._match[0] != key:
            if self._match is not None:
                self._match[1].close()
            self._match = (key, ScsMatch(self.config, search_cfg_1, search_cfg_2, n, device=self.device))
        r = self._match[1].play(net1, net2, seeds=seeds, max_moves=max_moves)
        return r["p1_wins"], r["p2_wins"], r["draws"]

    Test_using_agents = test_using_agents
