"""Floors on what the pinned directed walks (tests/scs_directed.py) reach, on the CPU oracle alone.

Each floor is a condition on the INPUTS of tests/test_gpu_scs_directed.py, not a measurement of the device: the device
tests compare the rule forms with the oracle along these walks, and they are worth what the walks visit.  No GPU."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import scs_directed as sd          # noqa: E402


def test_the_fixture_is_the_shape_the_device_tests_rely_on():
    g = sd.new_game("directed_6x5")
    c = g.cfg
    assert (c.rows, c.cols, c.turns, c.stacking) == (6, 5, 4, 3)
    assert (c.channels, c.planes, c.num_actions) == (105, 30, 900)
    assert len(g.unit_order) == 32 and [len(c.vp[0]), len(c.vp[1])] == [2, 3]
    kinds = {(u.attack, u.defense, u.mov_allowance) for u in g.unit_order}
    assert kinds == {(2, 1, 3), (2, 2, 2), (2, 2, 3), (1, 3, 2), (1, 1, 2)}
    mods = {t[:2] for row in c.terrain for t in row}
    assert (0.3, 1) in mods and (1, 1.5) in mods              # a modifier that is no power of two


def test_pinned_walks_reach_every_situation():
    total = sd.pinned_situations()
    print(dict(sorted(total.items())))
    for name in sd.SITUATIONS:
        assert total[name] >= 3, (name, total[name])
    for name in ("strongest_by_second", "strongest_by_third", "strongest_by_tie"):
        assert total[name] >= 5, (name, total[name])
    assert total["largest_legal_set"] > 64


def test_no_pinned_combat_depends_on_the_float32_transit_of_the_modifiers():
    """The device's game descriptions carry the terrain modifiers as float32, the oracle sums the YAML's doubles: 0.3
    differs, and a combat whose sums meet exactly (2 + 2 + 1 attack from 0.3 tiles against 1 defense on a 1.5 tile) is a
    tie on one side and a win on the other.  The pinned walks hold no such combat, so the device
    tests compare what both sides define alike; the counter itself tells the constructed case apart."""
    for w in sd.PINNED + [sd.PER_GAME]:
        assert w.situations()["result_differs_with_float32_modifiers"] == 0, w.label
    assert sd.pinned_situations()["result_tie"] >= 3               # exact meetings do occur, on representable sums
    import numpy as np
    exact = sum(x * 0.3 for x in (2, 2, 1))
    single = sum(x * float(np.float32(0.3)) for x in (2, 2, 1))
    assert exact == 1 * 1.5 and single > 1 * 1.5


def test_every_directed_game_places_unit_31_and_ends():
    for w in sd.DIRECTED:
        for g in w.games():
            assert g.situations["unit_31_placed"] == 1 and g.terminal and not g.dead_end, w.label
    outcomes = [g.outcome for w in sd.DIRECTED for g in w.games()]
    assert outcomes.count(1) >= 3 and outcomes.count(-1) >= 3


def test_capped_walks_stop_at_their_cap_with_large_legal_sets():
    for w in sd.EDGE:
        if w.cap:
            assert all(len(g.actions) <= w.cap for g in w.games()) and any(not g.terminal for g in w.games()), w.label
    assert sd.EDGE[0].name == "many_units_10x10" and sd.EDGE[0].situations()["largest_legal_set"] > 128
    assert sd.EDGE[1].name == "many_units_5x6" and sd.EDGE[1].situations()["largest_legal_set"] > 64


def test_dead_end_walks_end_on_a_live_position_without_a_legal_action():
    assert {w.name for w in sd.DEAD_ENDS} == {"two_types_6x5", "one_type_6x5"}
    for w in sd.DEAD_ENDS:
        for g in w.games():
            assert g.dead_end and not g.terminal and len(g.final_legal) == 0 and len(g.actions) > 20, w.label
            # the position itself: a placement whose every arrival tile the enemy holds
            game = sd.new_game(w.name)
            for a in g.actions:
                game.step_index(a)
            assert game.sub_phase == 0 and not game.terminal and not game.possible_actions().any()
            unit = game.reinf[game.player][game.turn][0]
            assert all(game.owner[r][k] == (game.player ^ 1) for (r, k) in unit.arrival), w.label


def test_the_uniform_walk_never_asks_the_second_or_third_key():
    """Why the directed walks exist: the walk of test_scs_device_rules_equal_oracle on two_types_6x5 (48 games in
    lock-step on RandomState(7)) has no "strongest unit" comparison that the second or the third key decides."""
    s = sd.uniform_lockstep_situations("two_types_6x5", 48, seed=7)
    print(dict(sorted(s.items())))
    assert s["strongest_by_second"] == 0 and s["strongest_by_third"] == 0
    assert s["attackers_1"] + s["attackers_2"] + s["attackers_3"] + s["attackers_4+"] > 0      # it does fight
