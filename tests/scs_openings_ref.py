"""Test infrastructure: the CPU reference of SCS opening positions (nuzero_amd.scs_positions, nz_scs_search_reset_to,
nz_scs_openings_draw / _expand), built on oracle/scs.py and oracle/agents.py play_match alone.

  * `apply_prefix`      steps an oracle game through a prefix; a bad prefix raises BadPrefix(ply, reason);
  * `draw_prefix`       the random agent's rule on numpy's own RandomState(seed).randint (n_legal == 1: no draw);
  * `enumerate_openings` breadth first, ascending action order, positions deduplicated on state_image().tobytes() with
                        the first sequence in lexicographic order kept;
  * `replay_match_from` / `replay_agent_match_from`  match_replay.replay_match / agents_ref.replay_agent_match started
                        at the prefix's position: play_match takes the stepped game, the agents start from fresh roots.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (REPO, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from match_replay import RecordedEvaluations, oracle_game          # noqa: E402

ILLEGAL, GAME_OVER = "illegal action", "game over before the prefix ended"


class BadPrefix(ValueError):
    def __init__(self, ply, reason):
        super().__init__(f"ply {ply}: {reason}")
        self.ply, self.reason = ply, reason


def legal_actions(game):
    return np.flatnonzero(np.asarray(game.possible_actions()).reshape(-1))


def apply_prefix(game, actions):
    for ply, a in enumerate(actions):
        if game.is_terminal():
            raise BadPrefix(ply, GAME_OVER)
        if int(a) not in set(legal_actions(game).tolist()):
            raise BadPrefix(ply, ILLEGAL)
        game.step_index(int(a))
    return game


def status_row(game):
    """What ScsSelfPlay.status() reports: player, sub_phase, stage, turn, terminal, terminal_value, length."""
    return [int(game.player), int(game.sub_phase), int(game.stage), int(game.turn), int(game.is_terminal()),
            int(game.terminal_value), int(game.length)]


def draw_prefix(config_path, opening_seed, plies, map_seed=None, n_legal_out=None):
    """(actions of the drawn prefix, at most `plies`; it ends with the game).  n_legal_out: a list that receives the
    number of legal actions at each ply."""
    game, rs, out = oracle_game(config_path, map_seed), np.random.RandomState(int(opening_seed)), []
    for _ in range(plies):
        if game.is_terminal():
            break
        legal = legal_actions(game)
        k = int(rs.randint(len(legal))) if len(legal) > 1 else 0          # randint(1) draws nothing
        if n_legal_out is not None:
            n_legal_out.append(len(legal))
        out.append(int(legal[k]))
        game.step_index(out[-1])
    return out


def random_game(config_path, seed, map_seed=None):
    """A whole uniformly random game: draw_prefix without a ply limit."""
    return draw_prefix(config_path, seed, 1 << 30, map_seed)


def enumerate_levels(config_path, plies, distinct=True):
    """Breadth first: per level 1 .. plies the pair (action sequences that continue the level before, the openings kept
    as a list of tuples in lexicographic order).  `distinct`: positions are deduplicated on state_image().tobytes(), the
    first sequence in that order kept, level by level; the raw count of a level is then the number of continuations of the
    level before's kept openings."""
    frontier, levels = [((), oracle_game(config_path))], []
    for _ in range(plies):
        nxt, seen, n_raw = [], set(), 0
        for seq, g in frontier:
            if g.is_terminal():
                continue
            for a in legal_actions(g):
                c = g.shallow_clone()
                c.step_index(int(a))
                n_raw += 1
                if distinct:
                    key = c.state_image().tobytes()
                    if key in seen:
                        continue
                    seen.add(key)
                nxt.append((seq + (int(a),), c))
        frontier = nxt
        levels.append((n_raw, [seq for seq, _ in frontier]))
    return levels


def enumerate_openings(config_path, plies, distinct=True):
    """All openings of `plies` plies in lexicographic order (a list of tuples)."""
    return enumerate_levels(config_path, plies, distinct)[-1][1] if plies else [()]


def count_sequences(config_path, plies):
    """The number of legal action sequences of `plies` plies (no images needed: the last level is only counted)."""
    frontier = [oracle_game(config_path)]
    for _ in range(plies - 1):
        nxt = []
        for g in frontier:
            if g.is_terminal():
                continue
            for a in legal_actions(g):
                c = g.shallow_clone()
                c.step_index(int(a))
                nxt.append(c)
        frontier = nxt
    return sum(len(legal_actions(g)) for g in frontier if not g.is_terminal())


def replay_match_from(args):
    """(config path, prefix, search config 1, search config 2, records 1, records 2[, seed[, game_map]]) -> dict, as
    match_replay.replay_match; "actions" holds the prefix, then the match's own decisions.  Top-level: it can run in a
    worker process."""
    config_path, prefix, search1, search2, rec1, rec2 = args[:6]
    seed = args[6] if len(args) > 6 else None
    game_map = args[7] if len(args) > 7 else None
    from oracle.agents import MctsAgentRef, play_match
    game = apply_prefix(oracle_game(config_path, seed, game_map), prefix)
    ev1, ev2 = RecordedEvaluations(*rec1, label="agent 1"), RecordedEvaluations(*rec2, label="agent 2")
    actions = play_match(game, MctsAgentRef(search1, ev1), MctsAgentRef(search2, ev2))
    return {"actions": [int(a) for a in prefix] + [int(a) for a in actions], "length": int(game.length),
            "terminal_value": int(game.terminal_value), "lookups": (ev1.lookups, ev2.lookups),
            "recorded": (len(rec1[2]), len(rec2[2])), "unused": (ev1.unused(), ev2.unused())}


def replay_agent_match_from(args):
    """(config path, prefix, spec 1, spec 2[, seed[, game_map]]) -> dict, as agents_ref.replay_agent_match (specs as
    there); "movers" and the sides' lists cover the match's own decisions, "actions" the prefix too."""
    config_path, prefix, spec1, spec2 = args[:4]
    seed = args[4] if len(args) > 4 else None
    game_map = args[5] if len(args) > 5 else None
    from agents_ref import PolicyAgentRef, RandomAgentRef
    from oracle.agents import MctsAgentRef, play_match
    game = apply_prefix(oracle_game(config_path, seed, game_map), prefix)
    agents, evs = [], []
    for i, spec in enumerate((spec1, spec2)):
        ev = None
        if spec[0] == "mcts":
            ev = RecordedEvaluations(*spec[2], label=f"agent {i + 1}")
            agents.append(MctsAgentRef(spec[1], ev))
        elif spec[0] == "policy":
            ev = RecordedEvaluations(*spec[1], label=f"agent {i + 1}")
            agents.append(PolicyAgentRef(ev))
        else:
            agents.append(RandomAgentRef(spec[1]))
        evs.append(ev)
    g2 = apply_prefix(oracle_game(config_path, seed, game_map), prefix)
    actions, movers = play_match(game, agents[0], agents[1]), []
    for a in actions:                                       # who decided what: side 0 moves for player index 1
        movers.append(0 if g2.get_current_player() == 1 else 1)
        g2.step_index(int(a))
    out = {"actions": [int(a) for a in prefix] + [int(a) for a in actions], "movers": movers, "length": int(game.length),
           "terminal_value": int(game.terminal_value), "sides": []}
    for ag, ev in zip(agents, evs):
        d = {"lookups": ev.lookups if ev else 0, "recorded": len(ev.values) if ev else 0, "unused": ev.unused() if ev else []}
        if not isinstance(ag, MctsAgentRef):
            d.update(n_legal=ag.n_legal, agent_actions=ag.actions)
        out["sides"].append(d)
    return out


def run_jobs(fn, jobs, workers=None):
    """Several replays, in spawned worker processes when there is more than one (as match_replay.replay_matches)."""
    if len(jobs) <= 1 or workers == 1:
        return [fn(j) for j in jobs]
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor
    workers = workers or min(len(jobs), max(1, (os.cpu_count() or 2) - 1), 12)
    with ProcessPoolExecutor(max_workers=workers, mp_context=mp.get_context("spawn")) as ex:
        return list(ex.map(fn, jobs))
