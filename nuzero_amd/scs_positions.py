"""SCS opening positions for evaluation matches: the twin of `ttt_positions`.

Evaluation agents are deterministic, so on one map the matches of a round are copies of one game.  The remedy that
leaves the game alone is to start match i at the position a short prefix of its own actions leads to
(`ScsMatch.play(..., start_actions=...)`, `ScsSelfPlay.reset_to`; C ABI nz_scs_search_reset_to).  An opening is a
sequence of flat action indices from the start of the game; a round's openings are an int32 array [n, max_plies] with
match i's prefix in its first n_plies[i] entries.

  * `check_openings`   what the library refuses before any launch, as a pure function (no GPU);
  * `random_openings`  one opening per seed, drawn on the device by the random agent's rule (nz_scs_openings_draw);
  * `all_openings`     every opening of k plies, level by level on the device (nz_scs_openings_expand), positions that
                       several sequences reach (transposed placements) kept once;
  * `agent_results`    the per-agent tally of a round, whichever side each agent played.

Who won: a game's terminal value +1 is a win of player index 0 (oracle/scs.py _check_termination) and agent 1 of a
match moves for player index 1, so the tally's `p1_wins` ("player 1", index 0) counts the games won by the side AGENT 2
moves for; `agent_results` counts per agent from the terminal value and from which agent moved for index 0.
"""
from ctypes import c_void_p

import numpy as np


def check_openings(actions, n_plies, num_actions, limit):
    """The host-side refusals of nz_scs_search_reset_to: `actions` must be a 2-D integer array [n, max_plies] with
    max_plies <= limit (the decisions a game's records hold, ScsSelfPlay.MAX_MOVES), `n_plies` (None: every match has
    max_plies) one length in 0 .. max_plies per match, and every action inside a match's plies in 0 .. num_actions - 1.
    Raises ValueError naming match and ply; returns (actions int32 [n, max_plies] C-contiguous, n_plies int32 [n])."""
    a = np.asarray(actions)
    if a.ndim != 2:
        raise ValueError(f"openings: a 2-D array [matches, plies], not {a.ndim}-D")
    if a.size and a.dtype.kind not in "iu":
        raise ValueError(f"openings: action indices are integers, not {a.dtype}")
    n, P = a.shape
    if P > int(limit):
        raise ValueError(f"openings of {P} plies: at most {int(limit)} (the decisions a game's records hold)")
    if n_plies is None:
        k = np.full((n,), P, np.int64)
    else:
        k = np.asarray(n_plies)
        if k.shape != (n,) or (k.size and k.dtype.kind not in "iu"):
            raise ValueError(f"n_plies: one integer per match ({n}), not {k.dtype} {k.shape}")
        k = k.astype(np.int64)
    for g in range(n):
        if not 0 <= k[g] <= P:
            raise ValueError(f"match {g}: an opening of {int(k[g])} plies, the openings hold 0 .. {P} "
                             f"(ply {int(k[g]) if k[g] < 0 else P} is not there)")
        row = a[g, :k[g]].astype(np.int64)
        bad = np.flatnonzero((row < 0) | (row >= int(num_actions)))
        if bad.size:
            ply = int(bad[0])
            raise ValueError(f"match {g}, ply {ply}: action {int(row[ply])} outside 0 .. {int(num_actions) - 1}")
    out = np.zeros((n, P), np.int32)                  # entries past a match's plies are not read: zero them
    for g in range(n):
        out[g, :k[g]] = a[g, :k[g]]
    return np.ascontiguousarray(out), np.ascontiguousarray(k.astype(np.int32))


def random_openings(engine, seeds, plies):
    """One opening per match of `engine` (an ScsSelfPlay): match i owns RandomState(seeds[i]) and plays the random
    agent's rule from the start -- k = randint(n_legal), the k-th legal action in ascending flat index -- for `plies`
    plies or to the game's end, on its own map where the config is per game (set the games first).  Returns (actions
    int32 [n_games, plies], -1 past a prefix's end; n_plies int32 [n_games])."""
    from .scs import _seed_array
    s = _seed_array(list(seeds))
    if s.shape != (engine.n_games,):
        raise ValueError(f"{s.shape[0]} opening seeds for {engine.n_games} matches")
    plies = int(plies)
    if not 1 <= plies <= engine.MAX_MOVES:
        raise ValueError(f"openings of {plies} plies: 1 .. {engine.MAX_MOVES}")
    from ._lib import lib
    actions = np.empty((engine.n_games, plies), np.int32)
    n_plies = np.empty((engine.n_games,), np.int32)
    engine._check(lib.nz_scs_openings_draw(engine._h, c_void_p(s.ctypes.data), plies, c_void_p(actions.ctypes.data),
                                           c_void_p(n_plies.ctypes.data), engine._stream()))
    return actions, n_plies


def expand_openings(engine, frontier):
    """One level: `frontier` int32 [n, depth] -> (counts int32 [n], children int32 [sum, depth + 1] in ascending action
    order per prefix, keys uint64 [sum, 2], the 128-bit digest of each child position's planes)."""
    from ._lib import lib
    f = np.ascontiguousarray(np.asarray(frontier, np.int32))
    n, depth = f.shape
    counts = np.zeros((n,), np.int32)
    fp = c_void_p(f.ctypes.data) if depth else None
    engine._check(lib.nz_scs_openings_expand(engine._h, fp, n, depth, c_void_p(counts.ctypes.data), None, None,
                                             engine._stream()))
    total = int(counts.sum())
    children, keys = np.empty((total, depth + 1), np.int32), np.empty((total, 2), np.uint64)
    if total:
        engine._check(lib.nz_scs_openings_expand(engine._h, fp, n, depth, c_void_p(counts.ctypes.data),
                                                 c_void_p(children.ctypes.data), c_void_p(keys.ctypes.data), engine._stream()))
    return counts, children, keys


def all_openings(engine, plies, distinct=True, limit=4096):
    """Every opening of `plies` plies on `engine`'s map, breadth first through nz_scs_openings_expand: int32 [n, plies]
    in lexicographic order of the sequences.  `distinct`: of the sequences that reach one position (its key: the
    digest of the position's planes) the first in that order is kept, at every level -- positions, not move orders, so a
    transposition does not weigh a tally double.  A sequence that ends the game has no continuation and is not an
    opening of more plies.  Raises ValueError naming the count when a level holds more than `limit` openings;
    per-game configs are refused by the library (one frontier belongs to one map)."""
    plies = int(plies)
    if plies < 0:
        raise ValueError("plies must not be negative")
    frontier = np.zeros((1, 0), np.int32)
    for depth in range(plies):
        counts, children, keys = expand_openings(engine, frontier)
        if distinct and len(children):
            # children are in lexicographic order (sorted prefixes, ascending actions): np.unique's first occurrence
            _, first = np.unique(keys, axis=0, return_index=True)
            children = children[np.sort(first)]
        if len(children) > int(limit):
            raise ValueError(f"{len(children)} openings of {depth + 1} plies: more than limit = {int(limit)}")
        frontier = np.ascontiguousarray(children)
        if not len(frontier):
            return np.zeros((0, plies), np.int32)
    return frontier


def agent_results(outcomes, agent1_is_x, finished=None):
    """The per-agent tally of a round.  `outcomes`: terminal values [n] (+1: player index 0 won, -1: player index 1
    won, 0: a draw); `agent1_is_x` (a bool, or one per match): whether agent 1 moved for player index 0, the first
    mover -- False in a plain round (agent 1 moves for player index 1), True in the round played with the agents
    exchanged; `finished` (None: all): bool [n], a match stopped at max_moves counts as unfinished, not as a draw.
    Returns {"agent1_wins", "agent2_wins", "draws", "unfinished", "matches"}."""
    o = np.asarray(outcomes).astype(np.int64).reshape(-1)
    x = np.broadcast_to(np.asarray(agent1_is_x, bool), o.shape)
    done = np.ones(o.shape, bool) if finished is None else np.broadcast_to(np.asarray(finished, bool), o.shape)
    if ((o < -1) | (o > 1)).any():
        raise ValueError("outcomes are terminal values: -1, 0 or +1")
    mine = np.where(x, o, -o)                         # the terminal value from agent 1's view
    return {"agent1_wins": int((done & (mine == 1)).sum()), "agent2_wins": int((done & (mine == -1)).sum()),
            "draws": int((done & (mine == 0)).sum()), "unfinished": int((~done).sum()), "matches": int(o.size)}
