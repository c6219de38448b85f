"""Evaluation matches between two MCTS agents on SCS, played inside the library (C ABI nz_scs_match_*).

The trainer's test step -- `Tester.Test_using_agents` with two `MctsAgent`s that keep their subtrees
(Testing/Tester.py:46-121, Testing/Agents/Generic/MctsAgent.py:28-39) -- for many matches at
once: `ScsMatch` holds two `ScsSelfPlay(training=False)` engines of one game config, one per agent, each with its own
search config, network and trees.  `play(net1, net2)` runs the whole move loop on the device: per decision both
engines search the position (on two streams), a hand-over kernel tells each engine what to play, and the tally is
counted there too.  Agent 1 moves when the game's player index is 1 (oracle/agents.py play_match); wins are the
game's terminal values (+1: player 1).

Evaluation agents are deterministic (no noise, max action), so matches on ONE map are copies of one game.  Two remedies:
the reference's "Randomized" presets, `ScsGameConfig(path, per_game=True)`, one map per match drawn on the device from
`seeds` -- which changes the game being evaluated -- or, on the map as it is, matches from opening positions:
`play(..., start_actions=..., n_plies=...)` starts match i at the position a short prefix of its own actions leads to
(nuzero_amd.scs_positions: every distinct position k plies into the game, or one opening per seed drawn by the random
agent's rule), both agents from a fresh root there, and `ScsTester.test_from_openings` plays every such opening with
both colour assignments and counts per agent (C ABI nz_scs_search_reset_to, nz_scs_match_play_from,
nz_scs_agent_match_play_from, nz_scs_openings_draw, nz_scs_openings_expand).

Cheaper opponents (C ABI nz_scs_agent_match_*): `ScsAgentMatch` plays the same rounds on ONE engine when at most one
side is an MCTS agent and the others are the bare policy `("policy",)` or a random mover `("random",)` -- the
trainer's policy-vs-random, MCTS-vs-random and MCTS-vs-policy tests.  Their rules are harness rules (DESIGN.md section
5b; the reference's Testing/Agents sources are not restated here, parity unpinned): the policy agent plays the legal
action of largest softmax probability (lowest index on a tie, no search); the random agent of match i draws
`RandomState(agent_seeds[i]).randint(n_legal)` at each of its own decisions and plays that legal action in ascending
index.  `ScsTester.test_using_agents` takes these specs in place of a search config.

Tic-Tac-Toe (C ABI nz_engine_match_play): `TttMatch` (two MCTS agents), `TttAgentMatch` (any pairing of MCTS, policy
and random sides, same specs and rules) and `TttTester`.  A game lasts at most nine plies and every match of a round is
at the same ply, so one call enqueues the whole round with no host round trip.  Two MCTS sides, or MCTS against the bare
policy, are deterministic from the empty board: N such matches are N copies of one game; only matches with a random
side differ from each other.  The remedy is to start the matches elsewhere: `play(..., start_boards=...)` starts match i
at a position of the caller's (nuzero_amd.ttt_positions; all of one round at the same ply), every MCTS side from a fresh
root there; `TttTester.test_from_openings` plays every opening of k plies with both colour assignments, and
`TttTester.score_against_perfect_play` asks one agent for its move in each of the 4,520 reachable positions of the solved
game (C ABI nz_engine_match_play_from, nz_engine_reset_to, nz_engine_policy_actions).

Out of scope: SCS's scripted agents (the reference's hand-written SCS players).
"""
from collections.abc import Mapping
from ctypes import byref, c_int32, c_int64, c_void_p

import numpy as np

_MAP_FIELDS = ("rows", "cols", "turns", "stacking", "n_vp", "terrain", "vp", "units", "arrival", "per_game")


def _same_game(c1, c2):
    return all(np.array_equal(np.asarray(getattr(c1, k)), np.asarray(getattr(c2, k))) for k in _MAP_FIELDS)


def _map_seeds(cfg, seeds, n_matches):
    """The seeds of the matches' maps: a per_game config needs one per match (returned as a list); any other config
    draws no map and `seeds` passes through."""
    if not cfg.per_game:
        return seeds
    if seeds is None:
        raise ValueError("a per_game config draws one map per match: pass seeds")
    seeds = list(seeds)
    if len(seeds) != n_matches:
        raise ValueError(f"{len(seeds)} seeds for {n_matches} matches")
    return seeds


def _round_result(engine, tally, actions):
    """The dict ScsMatch.play returns: a result call's tally and action record [N, MAX_MOVES], and the status of the
    engine that holds the games."""
    st = engine.status()
    out = {k: int(getattr(tally, k)) for k, _ in type(tally)._fields_}
    out["actions"] = actions[:, :max(1, out["length_max"])].cpu().numpy()
    out["lengths"], out["outcomes"], out["finished"] = st[:, 6].copy(), st[:, 5].copy(), st[:, 4] != 0
    return out


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

    def play(self, net1, net2, seeds=None, max_moves=None, start_actions=None, n_plies=None):
        """One round: every match from the start -- or, with `start_actions` (int32 [n_matches, max_plies], `n_plies`
        per match or None: all max_plies; nuzero_amd.scs_positions), match i from the position its opening leads to,
        both agents from a fresh root there -- to the end (or for `max_moves` decisions of the round's own; an opening's
        plies are not counted).  The records stay by the game's decision number: "actions" holds the opening's plies,
        "lengths" counts them.  net1 / net2: the agents'
        BoardNets (max_batch >= n_matches).  `seeds` (per_game configs: required, one per match): match i is played on
        the map `np.random.seed(seeds[i]); SCS_Game(config)` builds, drawn on the device in both engines (the draw is
        a pure function of the seed); `agents[0].game_maps` holds the maps for whoever replays a match.
        Returns a dict: "actions" int32 [N, T] (-1 past a match's end; T = the longest match), "lengths" [N],
        "outcomes" [N] (terminal value from player 1's view; 0 while unfinished), "finished" bool [N], "p1_wins",
        "p2_wins", "draws" (player 1 is player index 0, the side AGENT 2 moves for: scs_positions.agent_results),
        "unfinished" (stopped at max_moves), "length_sum", "length_max"."""
        import torch
        from . import _lib
        a1, a2 = self.agents
        seeds = _map_seeds(self.cfg, seeds, self.n_matches)
        if self.cfg.per_game:
            a1.set_games(seeds)
            a2.set_games(seeds)
        stream = c_void_p(torch.cuda.current_stream().cuda_stream)
        o, keep = a1._openings(start_actions, n_plies)
        if o is None:
            a1._check(_lib.lib.nz_scs_match_play(a1._h, net1._h, a2._h, net2._h, int(max_moves or 0), stream))
        else:
            a1._check(_lib.lib.nz_scs_match_play_from(a1._h, net1._h, a2._h, net2._h, byref(o), int(max_moves or 0), stream))
        tally = _lib.ScsMatchTally()
        actions = torch.empty((self.n_matches, a1.MAX_MOVES), dtype=torch.int32, device=a1.device)
        a1._check(_lib.lib.nz_scs_match_result(a1._h, a2._h, byref(tally), c_void_p(actions.data_ptr()), stream))
        return _round_result(a1, tally, actions)


def _agent_spec(spec):
    """("mcts", search_cfg) | ("policy",) | ("random",) -> (kind, search config or None); a bare search config (any
    mapping, as ScsMatch takes it) is an MCTS agent."""
    if isinstance(spec, Mapping):
        return "mcts", spec
    if isinstance(spec, str):
        spec = (spec,)
    if not isinstance(spec, (tuple, list)) or not spec or spec[0] not in ("mcts", "policy", "random"):
        raise ValueError(f"agent spec {spec!r}: (\"mcts\", search_cfg), (\"policy\",) or (\"random\",)")
    if spec[0] == "mcts":
        if len(spec) != 2 or not isinstance(spec[1], Mapping):
            raise ValueError("an MCTS agent spec is (\"mcts\", search_cfg)")
        return "mcts", spec[1]
    if len(spec) != 1:
        raise ValueError(f"agent spec {spec!r}: a {spec[0]} agent takes no arguments")
    return spec[0], None


# the search config of an engine that never searches (no MCTS side): the handle only holds the games.  Its tree arena
# grows with the simulations per move, so one simulation keeps the unused arena at its smallest.
_NO_SEARCH = {"Simulation": {"mcts_simulations": 1, "keep_subtree": True}, "UCT": {"pb_c_base": 10000, "pb_c_init": 1.15},
              "Exploration": {"number_of_softmax_moves": 0, "epsilon_softmax_exploration": 0.0,
                              "epsilon_random_exploration": 0.0, "value_factor": 1,
                              "root_exploration_distribution": "gamma", "root_exploration_fraction": 0.0,
                              "root_dist_alpha": 0.15, "root_dist_beta": 1}}


class ScsAgentMatch:
    """n_matches matches between agent1 (moves for player index 1) and agent2, at most one of them an MCTS agent:
    specs ("mcts", search_cfg), ("policy",), ("random",).  `engine`: the one ScsSelfPlay that holds the games (the MCTS
    side's search when there is one: persistent(), record(), cache(), status(), export() work as after play_native)."""

    def __init__(self, config, agent1, agent2, n_matches, device=0):
        from .scs import ScsGameConfig
        self.kinds, cfgs = zip(*(_agent_spec(a) for a in (agent1, agent2)))
        if self.kinds == ("mcts", "mcts"):
            raise ValueError("two MCTS agents need an engine each: use ScsMatch")
        for i, sc in enumerate(cfgs):
            if sc is not None and not sc["Simulation"]["keep_subtree"]:
                raise ValueError(f"agent {i + 1}: keep_subtree = False is not supported (an MctsAgent that drops its "
                                 "tree never re-roots, MctsAgent.py:28-39; every shipped search config keeps it)")
        if int(n_matches) <= 0:
            raise ValueError("n_matches must be positive")
        self.cfg = config if isinstance(config, ScsGameConfig) else ScsGameConfig(config)
        self.n_matches = int(n_matches)
        self.search_cfg = next((sc for sc in cfgs if sc is not None), None)
        from .scs import ScsSelfPlay              # (needs the GPU from here on)
        self.engine = ScsSelfPlay(self.cfg, self.search_cfg or _NO_SEARCH, self.n_matches, training=False, device=device)
        self._recorded = ([], [])

    def close(self):
        self.engine.close()

    def _check_play(self, nets, seeds, agent_seeds):
        """What play() refuses before any GPU call; returns (map seeds, per-side uint32 seed arrays or None)."""
        for i, (kind, net) in enumerate(zip(self.kinds, nets)):
            if kind != "random" and net is None:
                raise ValueError(f"agent {i + 1}: a {kind} agent needs a network")
        n_random = self.kinds.count("random")
        per_side = [None, None]
        if n_random:
            if agent_seeds is None:
                raise ValueError("a random agent draws from RandomState(agent_seeds[i]) in match i: pass agent_seeds")
            given = list(agent_seeds)
            if n_random == 2 and len(given) == 2 and all(hasattr(x, "__len__") for x in given):
                sides = [list(given[0]), list(given[1])]        # one list per random side
            else:
                sides = [given, given]
            for i, kind in enumerate(self.kinds):
                if kind != "random":
                    continue
                if len(sides[i]) != self.n_matches:
                    raise ValueError(f"agent {i + 1}: {len(sides[i])} agent_seeds for {self.n_matches} matches")
                from .scs import _seed_array
                per_side[i] = _seed_array(sides[i])
        return _map_seeds(self.cfg, seeds, self.n_matches), per_side

    def play(self, net1, net2, seeds=None, agent_seeds=None, max_moves=None, start_actions=None, n_plies=None):
        """One round, as ScsMatch.play (`start_actions` / `n_plies`: match i from its opening; a random side's stream
        starts fresh at its first own decision after it, and a scripted side's own record holds -1 / 0 at the
        opening's plies: it did not decide them).  net1 / net2: the BoardNet of a policy or MCTS side (None for a random side).
        `agent_seeds` (random sides: required, one per match; with two random sides one list for both or a pair of
        lists): match i's random agent is RandomState(agent_seeds[i]), rebuilt every round.  Returns ScsMatch.play's
        dict plus "agent_actions" / "agent_n_legal": per side int32 [N, T] by decision number (-1 / 0 where the side
        did not decide; None for the MCTS side), and "agent_probs" (the policy agent's winning probabilities)."""
        import torch
        from . import _lib
        nets = (net1, net2)
        seeds, side_seeds = self._check_play(nets, seeds, agent_seeds)
        e = self.engine
        if self.cfg.per_game:
            e.set_games(seeds)
        code = {"mcts": _lib.NZ_AGENT_MCTS, "policy": _lib.NZ_AGENT_POLICY, "random": _lib.NZ_AGENT_RANDOM}
        ag = [_lib.ScsAgent(kind=code[k], net=(n._h if k != "random" else None),
                            seeds_host=(s.ctypes.data if s is not None else None))
              for k, n, s in zip(self.kinds, nets, side_seeds)]
        stream = c_void_p(torch.cuda.current_stream().cuda_stream)
        o, keep = e._openings(start_actions, n_plies)
        if o is None:
            e._check(_lib.lib.nz_scs_agent_match_play(e._h, byref(ag[0]), byref(ag[1]), int(max_moves or 0), stream))
        else:
            e._check(_lib.lib.nz_scs_agent_match_play_from(e._h, byref(ag[0]), byref(ag[1]), byref(o), int(max_moves or 0), stream))
        tally = _lib.ScsMatchTally()
        actions = torch.empty((self.n_matches, e.MAX_MOVES), dtype=torch.int32, device=e.device)
        e._check(_lib.lib.nz_scs_agent_match_result(e._h, byref(tally), c_void_p(actions.data_ptr()), stream))
        out = _round_result(e, tally, actions)
        T = out["actions"].shape[1]
        out["agent_actions"], out["agent_n_legal"], out["agent_probs"] = [None, None], [None, None], [None, None]
        for i, kind in enumerate(self.kinds):
            if kind == "mcts":
                continue
            a = torch.empty((self.n_matches, e.MAX_MOVES), dtype=torch.int32, device=e.device)
            n = torch.empty_like(a)
            p = torch.empty((self.n_matches, e.MAX_MOVES), dtype=torch.float32, device=e.device)
            e._check(_lib.lib.nz_scs_agent_match_decisions(e._h, i, c_void_p(a.data_ptr()), c_void_p(n.data_ptr()),
                                                           c_void_p(p.data_ptr()), stream))
            out["agent_actions"][i], out["agent_n_legal"][i] = a[:, :T].cpu().numpy(), n[:, :T].cpu().numpy()
            out["agent_probs"][i] = p[:, :T].cpu().numpy()
        return out

    # ---- test hook: a policy side's evaluations in the order consumed (nz_scs_agent_record) ----
    def record(self, side, games, capacity):
        from . import _lib
        games = np.ascontiguousarray(np.asarray(list(games), dtype=np.int32))
        self._recorded[side][:] = [int(g) for g in games]
        self.engine._check(_lib.lib.nz_scs_agent_record(self.engine._h, int(side), c_void_p(games.ctypes.data), len(games),
                                                        int(capacity)))
        self._record_capacity = int(capacity)

    def records(self, side):
        """{match: (digests uint64 [n, 2], probs float32 [n, A], values float32 [n])} of the recorded matches."""
        from . import _lib
        out, A, e = {}, self.cfg.planes * self.cfg.rows * self.cfg.cols, self.engine
        for slot, g in enumerate(self._recorded[side]):
            count = c_int32(0)
            e._check(_lib.lib.nz_scs_agent_record_read(e._h, int(side), slot, byref(count), None, None, None))
            if count.value > self._record_capacity:
                raise RuntimeError(f"match {g} consumed {count.value} evaluations, capacity {self._record_capacity}")
            n = count.value
            dig, pr, va = np.empty((n, 2), np.uint64), np.empty((n, A), np.float32), np.empty((n,), np.float32)
            e._check(_lib.lib.nz_scs_agent_record_read(e._h, int(side), slot, byref(count), c_void_p(dig.ctypes.data),
                                                       c_void_p(pr.ctypes.data), c_void_p(va.ctypes.data)))
            out[g] = (dig, pr, va)
        return out


class ScsTester:
    """The shape of the reference's Tester for SCS: `test_using_agents` plays n matches between two agents and returns
    (p1_wins, p2_wins, draws), as Test_using_agents counts them over n games (Tester.py:46-121).  An agent is a search
    config (an MCTS agent, as before) or a spec ("mcts", search_cfg) / ("policy",) / ("random",); two MCTS agents play
    on ScsMatch, every other pairing on ScsAgentMatch."""

    def __init__(self, config, device=0):
        self.config, self.device = config, device
        self._match = None           # (key, ScsMatch or ScsAgentMatch) of the last call
        self._exchanged = None       # the same pairing with the agents exchanged, while test_from_openings plays both
        self.opening_rounds = None   # the play() results of the last test_from_openings (in the second, agent 1 is agent2)
        self.openings = None         # its (start_actions, n_plies)

    def close(self):
        for m in (self._match, self._exchanged):
            if m is not None:
                m[1].close()
        self._match = self._exchanged = None

    def _match_of(self, agent1, agent2, n):
        """The match of this pairing and size: the last one is kept, and beside it the one with the agents exchanged
        (as TttTester._match_of); any other pairing closes both."""
        (k1, c1), (k2, c2) = _agent_spec(agent1), _agent_spec(agent2)
        scripted = (k1, k2) != ("mcts", "mcts")
        key = (repr((k1, c1)), repr((k2, c2)), int(n)) if scripted else (repr(agent1), repr(agent2), int(n))
        other = (repr((k2, c2)), repr((k1, c1)), int(n)) if scripted else (repr(agent2), repr(agent1), int(n))
        if self._match is not None and self._match[0] == key:
            return self._match[1]
        if self._exchanged is not None and self._exchanged[0] == key:
            self._match, self._exchanged = self._exchanged, self._match
            return self._match[1]
        if self._match is not None and self._match[0] == other and key != other:
            if self._exchanged is not None:
                self._exchanged[1].close()
            self._exchanged, self._match = self._match, None
        else:
            self.close()
        m = (ScsAgentMatch(self.config, (k1, c1) if c1 else (k1,), (k2, c2) if c2 else (k2,), n, device=self.device)
             if scripted else ScsMatch(self.config, c1, c2, n, device=self.device))
        self._match = (key, m)
        return m

    def test_using_agents(self, search_cfg_1, net1, search_cfg_2, net2, n, seeds=None, max_moves=None, agent_seeds=None):
        m = self._match_of(search_cfg_1, search_cfg_2, n)
        if isinstance(m, ScsAgentMatch):
            r = m.play(net1, net2, seeds=seeds, agent_seeds=agent_seeds, max_moves=max_moves)
        else:
            r = m.play(net1, net2, seeds=seeds, max_moves=max_moves)
        return r["p1_wins"], r["p2_wins"], r["draws"]

    Test_using_agents = test_using_agents

    def test_from_openings(self, agent1, net1, agent2, net2, plies=2, openings=None, opening_seeds=None, both_colours=True,
                           max_moves=None, seeds=None, agent_seeds=None):
        """Matches that differ from each other on one map, between agents that are deterministic: every match starts at
        its own opening (nuzero_amd.scs_positions) --
          * by default every distinct position `plies` plies into the game, once each (all_openings: 55 for two plies
            of mirrored_5x5, the transposed placements counted once);
          * `openings`: the caller's, an int array [n, max_plies] or a pair (actions, n_plies);
          * `opening_seeds`: one opening per seed, drawn for `plies` plies by the random agent's rule (random_openings).
        With `both_colours` a second round plays the same openings with the agents exchanged.  Per-game configs take
        drawn openings only (`opening_seeds`, with the maps' `seeds`): a frontier belongs to one map.  `agent_seeds`
        (a random agent): one per opening, used in both rounds.  Returns the tally counted per AGENT, not per side,
        {"agent1_wins", "agent2_wins", "draws", "unfinished", "matches"} (scs_positions.agent_results: terminal value +1
        is player index 0's win, and agent 1 of a round moves for player index 1).  The rounds' play() results are kept
        in `opening_rounds` (in the second, agent 1 is `agent2`), the openings in `openings`."""
        from .scs import ScsSelfPlay
        from .scs_positions import agent_results, all_openings, random_openings
        per_game = bool(getattr(self.config, "per_game", False))       # (a path is a one-map config)
        if openings is not None and opening_seeds is not None:
            raise ValueError("openings or opening_seeds, not both")
        if per_game and opening_seeds is None:
            raise ValueError("a per_game config takes drawn openings only (opening_seeds): every match has its own map")
        n_plies = None
        if openings is not None:
            if isinstance(openings, tuple) and len(openings) == 2:
                openings, n_plies = openings
            start = np.asarray(openings)
        elif opening_seeds is not None:
            start = None                                    # drawn below, on the round's own engine
            opening_seeds = list(opening_seeds)
        else:
            e = ScsSelfPlay(self.config, _NO_SEARCH, 1, training=False, device=self.device)
            try:
                start = all_openings(e, plies)
            finally:
                e.close()
        n = len(opening_seeds) if start is None else len(start)
        if n == 0:
            raise ValueError("no opening to play")
        rounds = []
        pairs = (((agent1, net1), (agent2, net2)), ((agent2, net2), (agent1, net1)))
        for (a, na), (b, nb) in pairs[:2 if both_colours else 1]:
            m = self._match_of(a, b, n)
            if start is None:
                engine = m.engine if isinstance(m, ScsAgentMatch) else m.agents[0]
                if per_game:
                    engine.set_games(list(seeds) if seeds is not None else None)
                start, n_plies = random_openings(engine, opening_seeds, plies)
            kw = dict(seeds=seeds, max_moves=max_moves, start_actions=start, n_plies=n_plies)
            if isinstance(m, ScsAgentMatch):
                kw["agent_seeds"] = agent_seeds
            rounds.append(m.play(na, nb, **kw))
        self.opening_rounds, self.openings = tuple(rounds), (start, n_plies)
        total = {"agent1_wins": 0, "agent2_wins": 0, "draws": 0, "unfinished": 0, "matches": 0}
        for i, r in enumerate(rounds):                      # in round i == 1 agent1 sits in agent 2's seat: it moves for index 0
            for k, v in agent_results(r["outcomes"], i == 1, r["finished"]).items():
                total[k] += v
        return total


# ---- Tic-Tac-Toe -------------------------------------------------------------------------------------------------------
TTT_TABLE_ROWS = 3 ** 9


def _is_table(net):
    """A table evaluator: [3^9, 10] numbers (9 post-softmax probabilities + value), what SelfPlayEngine.set_table takes."""
    return not isinstance(net, (Mapping, tuple, list)) and hasattr(net, "shape") and len(net.shape) == 2


def _check_ttt_net(i, kind, net):
    """What a Tic-Tac-Toe side's `net` may be: None (random side), a state_dict (any mapping), a pair (state_dict,
    set_weights keyword arguments), or a table."""
    if kind == "random":
        return
    if net is None:
        raise ValueError(f"agent {i + 1}: a {kind} agent needs a network (a state_dict) or a table")
    if _is_table(net):
        if tuple(net.shape) != (TTT_TABLE_ROWS, 10):
            raise ValueError(f"agent {i + 1}: a table has shape ({TTT_TABLE_ROWS}, 10), not {tuple(net.shape)}")
        return
    if isinstance(net, (tuple, list)):
        if len(net) != 2 or not isinstance(net[0], Mapping) or not isinstance(net[1], Mapping):
            raise ValueError(f"agent {i + 1}: a network with its own arguments is (state_dict, set_weights kwargs)")
        return
    if not isinstance(net, Mapping):
        raise ValueError(f"agent {i + 1}: net must be a state_dict, (state_dict, kwargs) or a ({TTT_TABLE_ROWS}, 10) table")


def _load_ttt_net(engine, net, net_kwargs):
    if _is_table(net):
        import torch
        engine.set_table(net.cpu().numpy() if isinstance(net, torch.Tensor) else net)
    elif isinstance(net, Mapping):
        engine.set_weights(net, **net_kwargs)
    else:
        engine.set_weights(net[0], **dict(net_kwargs, **net[1]))


class TttAgentMatch:
    """n_matches Tic-Tac-Toe matches between agent1 (player 1, the first mover) and agent2: specs ("mcts", search_cfg),
    ("policy",), ("random",) as ScsAgentMatch takes them, in any pairing but two random sides.  `engines`: per side the
    SelfPlayEngine(training=False) of an MCTS or policy side, None for a random side; after play() an MCTS side's
    engine holds its search records (export()).  `share_policy_engine`: two policy sides that play with the SAME
    network use one engine instead of one each.  `precision`: the network arithmetic of the sides' engines, "float32" /
    "bf16" (SelfPlayEngine(precision=)) for both or a pair, one per side (None: the default)."""

    def __init__(self, agent1, agent2, n_matches, device=0, share_policy_engine=False, precision=None):
        self.precisions = tuple(precision) if isinstance(precision, (tuple, list)) else (precision, precision)
        if len(self.precisions) != 2 or any(p not in (None, "float32", "bf16") for p in self.precisions):
            raise ValueError(f"bad precision {precision!r}: 'float32', 'bf16' or a pair of them")
        if share_policy_engine and self.precisions[0] != self.precisions[1]:
            raise ValueError("share_policy_engine: one engine has one precision")
        self.kinds, self.search_cfgs = zip(*(_agent_spec(a) for a in (agent1, agent2)))
        if self.kinds == ("random", "random"):
            raise ValueError("two random agents: one side must be an MCTS or policy agent (its engine holds the matches)")
        for i, sc in enumerate(self.search_cfgs):
            if sc is not None and not sc["Simulation"]["keep_subtree"]:
                raise ValueError(f"agent {i + 1}: keep_subtree = False is not supported (an MctsAgent that drops its "
                                 "tree never re-roots, MctsAgent.py:28-39; every shipped search config keeps it)")
        if int(n_matches) <= 0:
            raise ValueError("n_matches must be positive")
        if share_policy_engine and self.kinds != ("policy", "policy"):
            raise ValueError("share_policy_engine: only two policy agents may share one engine (an MCTS agent owns its trees)")
        self.n_matches, self.device = int(n_matches), device
        from .engine import SelfPlayEngine            # (needs the GPU from here on)
        engines = []
        for kind, sc, prec in zip(self.kinds, self.search_cfgs, self.precisions):
            if kind == "random":
                engines.append(None)
            elif share_policy_engine and engines:
                engines.append(engines[0])            # one engine, one network
            else:
                kw = {"precision": prec} if prec is not None else {}
                engines.append(SelfPlayEngine(sc or _NO_SEARCH, self.n_matches, training=False, device=device, **kw))
        self.engines = tuple(engines)

    def close(self):
        for e in set(e for e in self.engines if e is not None):
            e.close()

    def _check_play(self, nets, agent_seeds, start_boards=None):
        """What play() refuses before any GPU call; returns the per-side uint32 seed arrays (None: not a random side)
        and the start boards as a uint32 array (None: the empty board)."""
        for i, (kind, net) in enumerate(zip(self.kinds, nets)):
            _check_ttt_net(i, kind, net)
        if start_boards is not None:
            from .ttt_positions import check_start_boards
            if len(start_boards) != self.n_matches:
                raise ValueError(f"{len(start_boards)} start_boards for {self.n_matches} matches")
            start_boards = check_start_boards(start_boards, same_ply=True)
        per_side = [None, None]
        if "random" in self.kinds:
            if agent_seeds is None:
                raise ValueError("a random agent draws from RandomState(agent_seeds[i]) in match i: pass agent_seeds")
            given = list(agent_seeds)
            i = self.kinds.index("random")
            if len(given) != self.n_matches:
                raise ValueError(f"agent {i + 1}: {len(given)} agent_seeds for {self.n_matches} matches")
            from .scs import _seed_array
            per_side[i] = _seed_array(given)
        return per_side, start_boards

    def play(self, net1, net2, agent_seeds=None, start_boards=None, **net_kwargs):
        """One round: every match from the empty board -- or, with `start_boards` (uint32 [n_matches], playable
        positions that all hold the same number of stones k: nuzero_amd.ttt_positions), match i from start_boards[i],
        every MCTS side from a fresh root there -- to its end.  The record stays by absolute ply: "actions"[i][p] is -1
        for p < k, "lengths" the stone count of the final position, side 1 moves the even plies (with odd k side 2
        moves first); an MCTS side's engine counts from the position, so its export() is the record shifted by k.
        The result then holds "start_boards" (None without them).  net1 / net2: an MCTS or policy side's network -- a
        state_dict (with `net_kwargs`, SelfPlayEngine.set_weights' keyword arguments, or as a pair (state_dict,
        kwargs) of its own) or a (3^9, 10) table (set_table) -- None for a random side; with share_policy_engine the
        same net for both.  `agent_seeds` (a random side: required, one per
        match): match i's random agent is RandomState(agent_seeds[i]), rebuilt every round.  Returns ScsMatch.play's
        keys: "p1_wins", "p2_wins", "draws", "unfinished", "actions" int32 [N, 9] (-1 past a match's end), "lengths",
        "outcomes" [N] (terminal value: +1 player 1 won), and per side "agent_actions" / "agent_n_legal" int32 [N, 9]
        by ply (-1 / 0 where the side did not decide; None for an MCTS side)."""
        import torch
        from . import _lib
        nets = (net1, net2)
        side_seeds, start = self._check_play(nets, agent_seeds, start_boards)
        if self.engines[0] is not None and self.engines[0] is self.engines[1] and net1 is not net2:
            raise ValueError("two policy agents share one engine and one network: pass the same net for both")
        loaded = set()
        for e, net in zip(self.engines, nets):
            if e is not None and id(e) not in loaded:
                _load_ttt_net(e, net, net_kwargs)
                loaded.add(id(e))
        host = next(e for e in self.engines if e is not None)
        N, dev = self.n_matches, host.device
        new = lambda: torch.empty((N, 9), dtype=torch.int32, device=dev)
        actions, lengths, outcomes = new(), torch.empty((N,), dtype=torch.int32, device=dev), torch.empty((N,), dtype=torch.int32, device=dev)
        ag_a, ag_n = [new(), new()], [new(), new()]
        tally = (c_int64 * 4)()
        res = _lib.TttMatchResult(actions=actions.data_ptr(), lengths=lengths.data_ptr(), outcomes=outcomes.data_ptr(),
                                  agent_actions=(c_void_p * 2)(*[t.data_ptr() for t in ag_a]),
                                  agent_n_legal=(c_void_p * 2)(*[t.data_ptr() for t in ag_n]), tally4_host=tally)
        code = {"mcts": _lib.NZ_AGENT_MCTS, "policy": _lib.NZ_AGENT_POLICY, "random": _lib.NZ_AGENT_RANDOM}
        h = [e._h if e is not None else None for e in self.engines]
        sp = [c_void_p(s.ctypes.data) if s is not None else None for s in side_seeds]
        with torch.cuda.device(dev):
            stream = c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.check(_lib.lib.nz_engine_match_play_from(h[0], code[self.kinds[0]], h[1], code[self.kinds[1]], sp[0], sp[1],
                                                          c_void_p(start.ctypes.data) if start is not None else None,
                                                          byref(res), stream), host._h)
        out = {"p1_wins": int(tally[0]), "p2_wins": int(tally[1]), "draws": int(tally[2]), "unfinished": int(tally[3]),
               "actions": actions.cpu().numpy(), "lengths": lengths.cpu().numpy(), "outcomes": outcomes.cpu().numpy(),
               "agent_actions": [None, None], "agent_n_legal": [None, None], "start_boards": start}
        for i, kind in enumerate(self.kinds):
            if kind != "mcts":
                out["agent_actions"][i], out["agent_n_legal"][i] = ag_a[i].cpu().numpy(), ag_n[i].cpu().numpy()
        return out

    def random_streams(self, side):
        """Test hook: the MT19937 states (key uint32 [N, 624], pos int32 [N]) the last round left random side `side` in."""
        from . import _lib
        host = next(e for e in self.engines if e is not None)
        keys, pos = np.empty((self.n_matches, 624), np.uint32), np.empty((self.n_matches,), np.int32)
        _lib.check(_lib.lib.nz_engine_match_streams(host._h, int(side), c_void_p(keys.ctypes.data), c_void_p(pos.ctypes.data)),
                   host._h)
        return keys, pos


class TttMatch(TttAgentMatch):
    """n_matches matches between two MCTS agents on Tic-Tac-Toe (search_cfg_1 plays player 1), one engine each.  Both are
    deterministic, so from the empty board the matches of a round are copies of one game: pass `start_boards` (one
    position per match, e.g. ttt_positions.openings(2)) for matches that differ."""

    def __init__(self, search_cfg_1, search_cfg_2, n_matches, device=0, precision=None):
        for i, sc in enumerate((search_cfg_1, search_cfg_2)):
            if not isinstance(sc, Mapping):
                raise ValueError(f"agent {i + 1}: TttMatch takes two search configs (scripted sides: TttAgentMatch)")
        super().__init__(("mcts", search_cfg_1), ("mcts", search_cfg_2), n_matches, device=device, precision=precision)

    def play(self, weights1, weights2, start_boards=None, **net_kwargs):
        return super().play(weights1, weights2, start_boards=start_boards, **net_kwargs)


class TttTester:
    """The shape of the reference's Tester on Tic-Tac-Toe, as ScsTester: `test_using_agents` plays n matches between
    two agents -- a search config (an MCTS agent) or a spec ("mcts", search_cfg) / ("policy",) / ("random",) -- and
    returns (p1_wins, p2_wins, draws), as Test_using_agents counts them over n games (Tester.py:46-121)."""

    def __init__(self, device=0):
        self.device = device
        self._match = None           # (key, TttAgentMatch) of the last call
        self._exchanged = None       # the same pairing with the sides exchanged, while test_from_openings plays both
        self.opening_rounds = None   # the two play() results of the last test_from_openings

    def close(self):
        for m in (self._match, self._exchanged):
            if m is not None:
                m[1].close()
        self._match = self._exchanged = None

    def _match_of(self, agent1, agent2, n):
        """The match of this pairing and size.  The last one is kept, and beside it the one with the sides exchanged,
        so repeated test_from_openings calls between two different agents build their engines once; any other
        pairing closes both."""
        (k1, c1), (k2, c2) = _agent_spec(agent1), _agent_spec(agent2)
        key = (repr((k1, c1)), repr((k2, c2)), int(n))
        if self._match is not None and self._match[0] == key:
            return self._match[1]
        if self._exchanged is not None and self._exchanged[0] == key:
            self._match, self._exchanged = self._exchanged, self._match
            return self._match[1]
        if self._match is not None and self._match[0] == (key[1], key[0], key[2]):
            if self._exchanged is not None:
                self._exchanged[1].close()
            self._exchanged, self._match = self._match, None
        else:
            self.close()
        self._match = (key, TttAgentMatch((k1, c1) if c1 else (k1,), (k2, c2) if c2 else (k2,), n, device=self.device))
        return self._match[1]

    def test_using_agents(self, agent1, net1, agent2, net2, n, agent_seeds=None, **net_kwargs):
        r = self._match_of(agent1, agent2, n).play(net1, net2, agent_seeds=agent_seeds, **net_kwargs)
        return r["p1_wins"], r["p2_wins"], r["draws"]

    Test_using_agents = test_using_agents

    def test_from_openings(self, agent1, net1, agent2, net2, plies=2, agent_seeds=None, **net_kwargs):
        """Every opening of `plies` plies (ttt_positions.openings: 72 for two plies) played twice, the second time with
        the agents exchanging sides: matches that differ from each other even between two deterministic agents.
        Returns (agent1_wins, agent2_wins, draws) over both rounds, counted per agent, not per side.  `agent_seeds` (a
        random agent): one per opening, used in both rounds.  The two rounds' play() results are kept in
        `opening_rounds` (in the second, side 1 is agent2)."""
        from .ttt_positions import openings
        boards = openings(plies)
        rounds = []
        for (a, na), (b, nb) in (((agent1, net1), (agent2, net2)), ((agent2, net2), (agent1, net1))):
            rounds.append(self._match_of(a, b, len(boards)).play(na, nb, agent_seeds=agent_seeds, start_boards=boards,
                                                                 **net_kwargs))
        self.opening_rounds = tuple(rounds)
        r1, r2 = rounds
        return r1["p1_wins"] + r2["p2_wins"], r1["p2_wins"] + r2["p1_wins"], r1["draws"] + r2["draws"]

    def score_against_perfect_play(self, agent, net, **net_kwargs):
        """An absolute strength measure that needs no opponent: the agent's move in every one of the 4,520 reachable
        non-terminal positions (each searched from a fresh root), scored against perfect play of the solved game.
        `agent`: a search config / ("mcts", cfg), or ("policy",).  Returns a dict: "positions" (4520), "optimal" (the
        decisions inside the perfect-play mask), "by_ply" int [9, 2] (positions, optimal, by stone count), "boards"
        uint32 [4520] (ttt_positions.reachable_nonterminal), "actions" int32 [4520], "is_optimal" bool [4520]."""
        from .ttt_positions import perfect_play, reachable_nonterminal, ttt_code
        kind, cfg = _agent_spec(agent)
        if kind == "random":
            raise ValueError("a random agent has no move to score: its choice is its seed's (score an MCTS or policy agent)")
        if cfg is not None and not cfg["Simulation"]["keep_subtree"]:
            raise ValueError("keep_subtree = False is not supported (every shipped search config keeps it)")
        _check_ttt_net(0, kind, net)
        boards = reachable_nonterminal()
        from .engine import SelfPlayEngine            # (needs the GPU from here on)
        e = SelfPlayEngine(cfg or _NO_SEARCH, len(boards), training=False, device=self.device)
        try:
            _load_ttt_net(e, net, net_kwargs)
            if kind == "mcts":
                e.reset(boards)
                e.search()
                e.apply()
                actions = e.last_actions().cpu().numpy()
            else:
                actions = e.policy_actions(boards).cpu().numpy()
        finally:
            e.close()
        masks = perfect_play()[1][[ttt_code(b) for b in boards]]
        ok = ((masks >> np.clip(actions, 0, 8)) & 1).astype(bool) & (actions >= 0)
        stones = np.array([bin(int(b)).count("1") for b in boards])
        by_ply = np.stack([np.bincount(stones, minlength=9), np.bincount(stones[ok], minlength=9)], 1)
        return {"positions": len(boards), "optimal": int(ok.sum()), "by_ply": by_ply, "boards": boards,
                "actions": actions, "is_optimal": ok}
