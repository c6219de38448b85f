"""SCS opening positions, the parts that need no GPU: the CPU reference (tests/scs_openings_ref.py) reproduces the
fixtures' counts, nuzero_amd.scs_positions.check_openings refuses what nz_scs_search_reset_to refuses before a launch,
and agent_results maps terminal values to agents the way the oracle's match loop seats them."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
CONFIGS = os.path.join(HERE, "golden", "scs_configs")
MIRRORED = os.path.join(CONFIGS, "mirrored_5x5.yml")
TEN = os.path.join(CONFIGS, "ten_by_ten.yml")
TWO_TYPES = os.path.join(CONFIGS, "two_types_6x5.yml")

from scs_openings_ref import (BadPrefix, GAME_OVER, ILLEGAL, apply_prefix, count_sequences, draw_prefix,      # noqa: E402
                              enumerate_levels, enumerate_openings, legal_actions, oracle_game, random_game)


def test_the_binding_declares_the_opening_calls():
    from nuzero_amd import _lib
    for name in ("nz_scs_search_reset_to", "nz_scs_match_play_from", "nz_scs_agent_match_play_from", "nz_scs_openings_draw",
                 "nz_scs_openings_expand"):
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES, name


# action sequences and distinct positions at 1, 2 and 3 plies, measured with oracle/scs.py
COUNTS = {MIRRORED: ((10, 100, 1000), (10, 55, 550)), TEN: ((40, 1600, 63960), (40, 820, 32760)),
          TWO_TYPES: ((3, 6, 18), (3, 6, 18))}


@pytest.mark.parametrize("path", [MIRRORED, TWO_TYPES, TEN], ids=["mirrored_5x5", "two_types_6x5", "ten_by_ten"])
def test_reference_reproduces_the_fixture_counts(path):
    sequences, positions = COUNTS[path]
    levels = enumerate_levels(path, 3)                                     # one breadth-first pass for all three depths
    for plies in (1, 2, 3):
        assert count_sequences(path, plies) == sequences[plies - 1], plies
        got = levels[plies - 1][1]
        assert len(got) == positions[plies - 1], plies
        assert got == sorted(got) and len(set(got)) == len(got)            # lexicographic, each once
    if path != TEN:                                                        # (the undeduplicated list is short here)
        raw = enumerate_openings(path, 3, distinct=False)
        assert len(raw) == sequences[2] and raw == sorted(raw)


def test_mirrored_transposed_placements_keep_the_first_sequence():
    two = enumerate_openings(MIRRORED, 2)
    first = [a for (a,) in enumerate_openings(MIRRORED, 1)]
    # both soldiers are one type: (a, b) and (b, a) are one position, the kept representative has a <= b
    assert two == [(a, b) for a in first for b in first if a <= b]
    # the first four plies are placements by player indices 0, 0, 1, 1
    g, movers = oracle_game(MIRRORED), []
    for _ in range(4):
        movers.append(int(g.get_current_player()))
        assert g.sub_phase == 0
        g.step_index(int(legal_actions(g)[0]))
    assert movers == [0, 0, 1, 1]


def test_reference_prefix_application_and_draw():
    g = apply_prefix(oracle_game(MIRRORED), [])
    assert g.length == 0
    first = legal_actions(g)
    illegal = next(a for a in range(g.get_num_actions()) if a not in set(first.tolist()))
    with pytest.raises(BadPrefix) as e:
        apply_prefix(oracle_game(MIRRORED), [int(first[0]), illegal])
    assert e.value.ply == 1 and e.value.reason == ILLEGAL
    whole = random_game(MIRRORED, 5)
    assert 25 <= len(whole) <= 70
    assert apply_prefix(oracle_game(MIRRORED), whole).is_terminal()
    with pytest.raises(BadPrefix) as e:
        apply_prefix(oracle_game(MIRRORED), whole + [0])
    assert e.value.ply == len(whole) and e.value.reason == GAME_OVER
    # a drawn prefix is the start of the same seed's random game, and another seed draws another one
    assert draw_prefix(MIRRORED, 5, 6) == whole[:6]
    assert len({tuple(draw_prefix(MIRRORED, s, 6)) for s in range(8)}) > 1


def test_check_openings_refuses_each_bad_argument():
    from nuzero_amd.scs_positions import check_openings
    A, LIMIT = 300, 40
    good = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12]])
    a, k = check_openings(good, None, A, LIMIT)
    assert a.dtype == np.int32 and a.flags.c_contiguous and np.array_equal(a, good) and k.tolist() == [3, 3, 3, 3]
    a, k = check_openings(good, [0, 1, 2, 3], A, LIMIT)
    assert k.dtype == np.int32 and k.tolist() == [0, 1, 2, 3]
    assert a.tolist() == [[0, 0, 0], [4, 0, 0], [7, 8, 0], [10, 11, 12]]       # entries past a match's plies are not read
    # an action outside a match's plies may be anything
    loose = good.copy()
    loose[1, 2] = -7
    check_openings(loose, [3, 2, 3, 3], A, LIMIT)
    bad = good.copy()
    bad[3, 2] = A
    with pytest.raises(ValueError, match=r"match 3, ply 2: action 300 outside 0 \.\. 299"):
        check_openings(bad, None, A, LIMIT)
    bad = good.copy()
    bad[2, 0] = -1
    with pytest.raises(ValueError, match=r"match 2, ply 0: action -1"):
        check_openings(bad, None, A, LIMIT)
    with pytest.raises(ValueError, match=r"match 1: an opening of 4 plies.*ply 3 is not there"):
        check_openings(good, [3, 4, 3, 3], A, LIMIT)
    with pytest.raises(ValueError, match=r"match 0: an opening of -1 plies"):
        check_openings(good, [-1, 3, 3, 3], A, LIMIT)
    with pytest.raises(ValueError, match="at most 2"):
        check_openings(good, None, A, 2)
    with pytest.raises(ValueError, match="2-D"):
        check_openings([1, 2, 3], None, A, LIMIT)
    with pytest.raises(ValueError, match="integers"):
        check_openings(good.astype(np.float32), None, A, LIMIT)
    with pytest.raises(ValueError, match="one integer per match"):
        check_openings(good, [1, 2], A, LIMIT)


def test_agent_results_under_both_assignments():
    from nuzero_amd.scs_positions import agent_results
    outcomes = np.array([1, 1, -1, 0, 1, -1, 0, 0])
    # a plain round: agent 1 moves for player index 1, so a terminal value of +1 (index 0 won) is agent 2's win
    assert agent_results(outcomes, False) == {"agent1_wins": 2, "agent2_wins": 3, "draws": 3, "unfinished": 0, "matches": 8}
    assert agent_results(outcomes, True) == {"agent1_wins": 3, "agent2_wins": 2, "draws": 3, "unfinished": 0, "matches": 8}
    per_match = np.array([True, False, True, False, False, False, True, True])
    assert agent_results(outcomes, per_match) == {"agent1_wins": 2, "agent2_wins": 3, "draws": 3, "unfinished": 0, "matches": 8}
    done = np.array([True] * 6 + [False, False])
    assert agent_results(outcomes, False, done) == {"agent1_wins": 2, "agent2_wins": 3, "draws": 1, "unfinished": 2, "matches": 8}
    with pytest.raises(ValueError):
        agent_results([2], False)


class _Scripted:
    """A play_match agent that plays a list of actions and notes the player index it is asked to move for."""

    def __init__(self, script):
        self.script, self.moved_for = script, set()

    def new_game(self):
        pass

    def choose_action(self, game):
        self.moved_for.add(int(game.get_current_player()))
        return self.script[game.length]


def test_the_winner_mapping_is_the_oracles():
    """Pinned against oracle games played to their end (uniformly random games of two_types_6x5: seed 9 ends +1, seed
    38 ends -1): play_match seats its first agent on player index 1, and a terminal value of +1 is index 0's win -- it
    holds a larger share of the opponent's victory points -- so it is the SECOND agent's."""
    from nuzero_amd.scs_positions import agent_results
    from oracle.agents import play_match
    for seed, value in ((9, 1), (38, -1)):
        script = random_game(TWO_TYPES, seed)
        g = oracle_game(TWO_TYPES)
        a1, a2 = _Scripted(script), _Scripted(script)
        assert [int(a) for a in play_match(g, a1, a2)] == script and g.is_terminal()
        assert a1.moved_for == {1} and a2.moved_for == {0}             # agent 1 moves for player index 1
        assert g.terminal_value == value
        vp = g.cfg.vp                                                  # who won by the rules, counted here
        share0 = sum(g.owner[r][k] == 0 for (r, k) in vp[1]) / len(vp[1])
        share1 = sum(g.owner[r][k] == 1 for (r, k) in vp[0]) / len(vp[0])
        index0_won = share0 > share1
        assert index0_won == (value == 1) and share0 != share1
        plain, exchanged = agent_results([g.terminal_value], False), agent_results([g.terminal_value], True)
        # plain seats: index 0 is agent 2's side; exchanged seats: agent 1 moved for index 0
        assert (plain["agent1_wins"], plain["agent2_wins"]) == ((0, 1) if index0_won else (1, 0))
        assert (exchanged["agent1_wins"], exchanged["agent2_wins"]) == ((1, 0) if index0_won else (0, 1))
