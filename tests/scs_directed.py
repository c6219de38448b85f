"""Test infrastructure: directed play on the SCS oracle (oracle/scs.py), CPU only.

Uniform random play from the start almost never reaches the situations in which the device's rule forms can differ
from the oracle: combats with several attackers from several tiles against full stacks, "strongest unit" comparisons
that the second or third key decides, decisive endings, endings in which comparing captured counts and comparing
captured fractions disagree, positions with more than 64 legal actions, the 32nd unit, live positions without a legal
action.  This module plays the oracle with three weighted policies that lean into them, counts what each walk reached
(`Situations`; observing the oracle, never changing it) and pins a set of walks (`PINNED`) by configuration, policy,
seed and number of games.  tests/test_scs_directed_host.py holds the pinned walks to floors on those counts, so the
device tests that play them (tests/test_gpu_scs_directed.py) cannot pass on walks that went quiet.

A policy is a seeded weighted choice among the oracle's legal actions; the weights are plain functions of the oracle's
state and the action's plane and tile.  Game g of a walk owns np.random.RandomState([seed, g]).
"""
import functools
import os
from collections import Counter

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CONFIGS = os.path.join(HERE, "golden", "scs_configs")


def config_path(name):
    return os.path.join(CONFIGS, name + ".yml")


def unravel(cfg, action):
    plane, rem = divmod(int(action), cfg.rows * cfg.cols)
    r, k = divmod(rem, cfg.cols)
    return plane, r, k


def legal_actions(game):
    """The oracle's legal set as flat indices in ascending order."""
    return np.flatnonzero(game.possible_actions().reshape(-1)).astype(np.int32)


# ---- policies ---------------------------------------------------------------------------------------------------------
def _weight(game, action, mode):
    """advance: forward placements and moves 6 : 1.5 : 0.3 for a column gained / kept / lost, targets by 8 x stack
    height, adding an attacker 12, confirming 1, ending movement 0.3, ending fighting 0.1.  stack: placements and moves
    times 1 + 3 x the destination's height.  lone: confirming 12, so most combats have one attacker."""
    c = game.cfg
    plane, r, k = unravel(c, action)
    forward = 1 if game.player == 0 else -1
    if plane < c.placement_limit:
        cols = [kk for (_, kk) in game.reinf[game.player][game.turn][0].arrival]
        front = max(cols) if forward == 1 else min(cols)
        w = 6.0 if k == front else 1.5
        return w * (1 + 3 * len(game.stacks[r][k])) if mode == "stack" else w
    if plane < c.movement_limit:
        direction = (plane - c.placement_limit) // c.stacking
        dr, dk = game.neighbours((r, k))[direction]
        gain = (dk - k) * forward
        w = 6.0 if gain > 0 else 1.5 if gain == 0 else 0.3
        return w * (1 + 3 * len(game.stacks[dr][dk])) if mode == "stack" else w
    if plane < c.target_limit:
        return 8.0 * len(game.stacks[r][k])
    if plane < c.attackers_limit:
        return 12.0
    if plane < c.confirm_limit:
        return 12.0 if mode == "lone" else 1.0
    if plane < c.no_move_limit:
        return 0.3
    return 0.1


def choose(game, legal, mode, rs):
    w = np.array([_weight(game, a, mode) for a in legal], np.float64)
    x = rs.random_sample() * w.sum()
    return int(legal[min(int(np.searchsorted(np.cumsum(w), x, side="right")), len(legal) - 1)])


# ---- the situation counter --------------------------------------------------------------------------------------------
def deciding_key(units, keys):
    """Which key of ScsGame._strongest's tuple comparison singles the strongest unit out of two or more: 'first',
    'second', 'third', or 'tie' (several units equal in all three: the first in list order wins).  None for one unit."""
    if len(units) < 2:
        return None
    left = list(units)
    for name, key in zip(("first", "second", "third"), keys):
        top = max(getattr(u, key) for u in left)
        left = [u for u in left if getattr(u, key) == top]
        if len(left) == 1:
            return name
    return "tie"


def _bucket(n, last):
    return str(n) if n < last else f"{last}+"


MAXIMA = ("largest_legal_set", "most_attackers")


class Situations(Counter):
    """Counts of what a walk reached (and two maxima, MAXIMA).  `before_step` looks at the position and the action
    about to be played, `after_walk` at the position a game stopped in; `merge` adds another walk's counts."""

    def merge(self, other):
        top = {k: max(self[k], other[k]) for k in MAXIMA}
        self.update(other)
        for k, v in top.items():
            self[k] = v
        return self

    def before_step(self, game, legal, action):
        c, p = game.cfg, game.player
        self["largest_legal_set"] = max(self["largest_legal_set"], len(legal))
        plane, r, k = unravel(c, action)
        if game.sub_phase == 0:                                # a placement the full stack refuses (friendly or empty tile)
            for (ar, ak) in game.reinf[p][game.turn][0].arrival:
                if len(game.stacks[ar][ak]) == c.stacking and game.owner[ar][ak] != (p ^ 1):
                    self["placement_refused_by_full_stack"] += 1
                    break
        elif game.sub_phase == 1:                              # a move only the full stack refuses
            if any(n is not None and u.mov_points - c.terrain[n[0]][n[1]][2] >= 0
                   and len(game.stacks[n[0]][n[1]]) == c.stacking and game.owner[n[0]][n[1]] != (p ^ 1)
                   for u in game.available[p] for n in game.neighbours(u.position)):
                self["move_refused_by_full_stack"] += 1
        if plane < c.placement_limit:
            if game.reinf[p][game.turn][0] is game.unit_order[-1] and len(game.unit_order) == 32:
                self["unit_31_placed"] += 1
        elif plane < c.movement_limit:
            s = (plane - c.placement_limit) % c.stacking
            if s < len(game.stacks[r][k]) - 1:
                self["move_from_below_top"] += 1
        elif c.attackers_limit <= plane < c.confirm_limit:
            self._combat(game)

    def _combat(self, game):
        c = game.cfg
        tr, tk = game.target
        defenders, attackers = game.stacks[tr][tk], game.attackers
        self["attackers_" + _bucket(len(attackers), 4)] += 1
        self["most_attackers"] = max(self["most_attackers"], len(attackers))
        self["defending_stack_" + str(len(defenders))] += 1
        self["attacker_tiles_" + _bucket(len({u.position for u in attackers}), 3)] += 1
        total_defense = sum(u.defense for u in defenders) * c.terrain[tr][tk][1]
        total_attack = 0
        for u in attackers:
            total_attack += u.attack * c.terrain[u.position[0]][u.position[1]][0]
        self["result_" + ("attacker_wins" if total_attack > total_defense else
                          "defender_wins" if total_attack < total_defense else "tie")] += 1
        # what the float32 transit of the modifiers (the device's game descriptions carry float32) would make of it
        d32 = sum(u.defense for u in defenders) * float(np.float32(c.terrain[tr][tk][1]))
        a32 = 0
        for u in attackers:
            a32 += u.attack * float(np.float32(c.terrain[u.position[0]][u.position[1]][0]))
        if ((a32 > d32) - (a32 < d32)) != ((total_attack > total_defense) - (total_attack < total_defense)):
            self["result_differs_with_float32_modifiers"] += 1
        losers = []
        if total_attack <= total_defense:
            losers.append((attackers, ("attack", "defense", "mov_allowance")))
        if total_attack >= total_defense:
            losers.append((defenders, ("defense", "attack", "mov_allowance")))
        for units, keys in losers:
            how = deciding_key(units, keys)
            if how is not None:
                self["strongest_by_" + how] += 1
            lost = game._strongest(units, keys)
            stack = game.stacks[lost.position[0]][lost.position[1]]
            if stack.index(lost) < len(stack) - 1:
                self["destroyed_below_top"] += 1

    def after_walk(self, game, legal):
        if game.terminal:
            self["outcome_%+d" % game.terminal_value if game.terminal_value else "outcome_0"] += 1
            vp = game.cfg.vp
            p2_cap = sum(1 for (r, k) in vp[0] if game.owner[r][k] == 1)
            p1_cap = sum(1 for (r, k) in vp[1] if game.owner[r][k] == 0)
            if ((p1_cap > p2_cap) - (p1_cap < p2_cap)) != game.terminal_value:
                self["counts_and_fractions_disagree"] += 1
        elif len(legal) == 0:
            self["dead_end"] += 1


# every count the floors of tests/test_scs_directed_host.py ask for
SITUATIONS = (["attackers_1", "attackers_2", "attackers_3", "attackers_4+", "defending_stack_1", "defending_stack_2",
               "defending_stack_3", "attacker_tiles_1", "attacker_tiles_2", "attacker_tiles_3+", "result_attacker_wins",
               "result_defender_wins", "result_tie", "strongest_by_first", "strongest_by_second", "strongest_by_third",
               "strongest_by_tie", "destroyed_below_top", "move_from_below_top", "move_refused_by_full_stack",
               "placement_refused_by_full_stack", "outcome_+1", "outcome_0", "outcome_-1", "counts_and_fractions_disagree",
               "unit_31_placed", "dead_end"])


# ---- walks ------------------------------------------------------------------------------------------------------------
class Game:
    """One played game: `actions` [n], `legal[m]` the legal set before ply m (ascending), `final_legal` the legal set
    of the position the walk stopped in, `terminal` / `outcome` of that position, `dead_end` (live, nothing legal)."""
    __slots__ = ("actions", "legal", "final_legal", "terminal", "outcome", "dead_end", "map_seed", "situations")


def new_game(name, map_seed=None):
    from oracle.scs import ScsConfig, ScsGame
    g = ScsGame(ScsConfig(config_path(name), map_seed=map_seed))
    g.unit_order = [u for p in range(2) for turn in g.reinf[p] for u in turn]       # the device's unit indices
    return g


def play_game(name, mode, rs, cap=None, map_seed=None):
    game, out, sit = new_game(name, map_seed), Game(), Situations()
    out.actions, out.legal, out.map_seed = [], [], map_seed
    while True:
        legal = legal_actions(game)
        if game.terminal or len(legal) == 0 or (cap is not None and len(out.actions) >= cap):
            break
        a = choose(game, legal, mode, rs)
        sit.before_step(game, legal, a)
        out.actions.append(a)
        out.legal.append(legal)
        game.step_index(a)
    sit.after_walk(game, legal)
    out.final_legal, out.terminal = legal, bool(game.terminal)
    out.outcome = int(game.terminal_value) if game.terminal else None
    out.dead_end = (not game.terminal) and len(legal) == 0
    out.situations = sit
    return out


class Walk:
    def __init__(self, name, mode, seed, n_games, cap=None, map_seeds=None):
        self.name, self.mode, self.seed, self.n_games, self.cap, self.map_seeds = name, mode, seed, n_games, cap, map_seeds

    @property
    def label(self):
        return f"{self.name}-{self.mode}-{self.seed}"

    def games(self):
        return _play(self.name, self.mode, self.seed, self.n_games, self.cap, self.map_seeds)

    def situations(self):
        total = Situations()
        for g in self.games():
            total.merge(g.situations)
        return total


@functools.lru_cache(maxsize=None)
def _play(name, mode, seed, n_games, cap, map_seeds):
    return tuple(play_game(name, mode, np.random.RandomState([seed, g]), cap, None if map_seeds is None else map_seeds[g])
                 for g in range(n_games))


DIRECTED = [Walk("directed_6x5", "advance", 11, 4), Walk("directed_6x5", "stack", 12, 4), Walk("directed_6x5", "lone", 13, 4)]
EDGE = [Walk("many_units_10x10", "advance", 21, 2, cap=60), Walk("many_units_5x6", "advance", 22, 2, cap=60),
        Walk("reference_test_config", "stack", 23, 2)]
# Live positions without a legal action: a placement whose every arrival tile the enemy holds.  About one advance game
# in 25 on these two fixtures stops there; the seeds were found by playing seeds 0 .. 149 on the oracle.
DEAD_ENDS = [Walk("two_types_6x5", "advance", 48, 1), Walk("two_types_6x5", "advance", 71, 1),
             Walk("one_type_6x5", "advance", 20, 1), Walk("one_type_6x5", "advance", 49, 1)]
PINNED = DIRECTED + EDGE + DEAD_ENDS
# The per-game path (tests/test_gpu_scs_directed.py): every game on the map its own seed draws.
PER_GAME = Walk("randomized_5x5", "advance", 31, 2, map_seeds=(7801, 7802))


def pinned_situations():
    total = Situations()
    for w in PINNED:
        total.merge(w.situations())
    return total


def uniform_lockstep_situations(name, n_games, seed=7, map_seed=None):
    """What the uniform random walk of tests/test_gpu_scs.py::test_scs_device_rules_equal_oracle reaches: the same
    games, the same RandomState(seed) shared by the games of a batch in lock-step."""
    games = [new_game(name, map_seed) for _ in range(n_games)]
    rs, sit = np.random.RandomState(seed), Situations()
    live = True
    while live:
        live = False
        for g in games:
            if g.terminal:
                continue
            legal = legal_actions(g)
            a = int(rs.choice(legal))
            sit.before_step(g, legal, a)
            g.step_index(a)
            live = True
    for g in games:
        sit.after_walk(g, legal_actions(g))
    return sit
