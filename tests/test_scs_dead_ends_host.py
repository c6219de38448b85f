"""What the oracle alone must show for tests/test_gpu_scs_dead_ends.py to mean anything (CPU, no device): floors on
what the cases of tests/scs_dead_ends.py reach -- conditions on the tests' inputs, not measurements of the device --,
oracle/search.py's semantics at a live node without a legal action stated as assertions, and the float32 oracle
network's distance from its float64 form on the dead-end leaves of the network cases."""
import os
import sys
from collections import Counter

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import scs_dead_ends as de                                          # noqa: E402
import scs_directed as sd                                           # noqa: E402
from scs_dead_ends import PLAYS_ON, REACHES, STARTS_ON              # noqa: E402


def test_every_case_ends_as_it_says():
    for case in de.CASES:
        out = de.oracle_run(case)
        assert de.ending_of(out) == case.ending, de.case_id(case)
        assert len(out["trace"]) <= 4 and case.sims <= 48 and case.moves <= 4
        assert out["simulations"] == case.sims * (len(out["trace"]) + int(out["dead_end_root"]))


def test_the_cases_reach_what_the_device_tests_need():
    total, depths = Counter(), set()
    outs = [(c, de.oracle_run(c)) for c in de.CASES]
    for _, out in outs:
        total.update(out["situations"])
        depths |= out["depths"]
    assert total["dead_end_evaluations"] >= 100
    assert total["re_evaluations"] >= 50 and total["dead_end_re_evaluations"] >= 50
    assert {1, 2, 3} <= depths
    reach = [c for c, out in outs if de.ending_of(out)[0] == REACHES and len(out["trace"]) >= 1]
    on = [c for c, out in outs if de.ending_of(out)[0] == PLAYS_ON and len(out["trace"]) >= 3
          and out["situations"]["childless_visited_at_reroot"] >= 1]
    start = [c for c, out in outs if de.ending_of(out)[0] == STARTS_ON]
    assert len(reach) >= 3 and len(on) >= 2 and len(start) >= 1
    assert any(c.training for c in reach) and any(c.training for c in on)
    # all four walks, both modes, every evaluation; the network cases on the fixture the persistent route admits
    assert {c.walk.label for c in de.CASES} == {w.label for w in sd.DEAD_ENDS}
    assert {c.training for c in de.CASES} == {True, False}
    assert {c.evaluation for c in de.CASES} >= {"flat", "net"}
    assert all(c.walk.name == "one_type_6x5" for c in de.CASES if c.evaluation == "net")
    assert total["dead_end_root_children"] >= 3 and total["dead_end_nodes"] >= 10
    assert total["moves_after_first_dead_end"] >= 10
    # what the cache test's hit floor stands on: the cases the library routes play (network, evaluation, not started on
    # the dead end) re-evaluate dead-end nodes
    library = [out for c, out in outs if c.evaluation == "net" and not c.training and c.back > 0]
    assert len(library) >= 3 and sum(o["situations"]["dead_end_re_evaluations"] for o in library) >= 50


def test_the_table_of_the_issue_is_among_the_cases():
    """47 of 48 and 43 of 48 first-move evaluations on the dead end from one ply back (evaluate_image); with the network
    from two plies back of one_type_6x5 seed 49: 28 in the first move's search, 60 after two moves."""
    def dead_in_move(out, m, sims):
        return sum(1 for e in out["evaluations"][m * sims:(m + 1) * sims] if e["dead_end"])
    t71, o20, o49 = (de.oracle_run(de.CASES[i]) for i in (0, 1, 5))
    assert (de.CASES[0].walk, de.CASES[0].back, de.CASES[0].evaluation) == (de.T71, 1, "flat")
    assert (de.CASES[1].walk, de.CASES[1].back, de.CASES[1].evaluation) == (de.O20, 1, "flat")
    assert (de.CASES[5].walk, de.CASES[5].back, de.CASES[5].evaluation) == (de.O49, 2, "net")
    assert dead_in_move(t71, 0, 48) == 47 and dead_in_move(o20, 0, 48) == 43
    assert dead_in_move(o49, 0, 32) == 28 and dead_in_move(o49, 0, 32) + dead_in_move(o49, 1, 32) == 60


def _dead_end_game(walk=de.O20):
    game = sd.new_game(walk.name)
    for a in walk.games()[0].actions:
        game.step_index(int(a))
    assert not game.is_terminal() and not game.possible_actions().any()
    return game


def test_an_expansion_without_legal_actions_appends_no_child_and_returns_the_evaluation():
    from oracle import search as osearch
    game = _dead_end_game()
    A = game.get_num_actions()
    explorer = osearch.Explorer(de.search_config(4), False, np.random.RandomState(1))
    node = osearch.Node(0)
    probs = np.full(A, 1.0 / A, np.float32)
    for n in range(1, 4):                               # every visit evaluates again and counts as an expansion
        assert explorer.evaluate(node, game, lambda g: (probs, np.float32(0.375))) == 0.375
        assert node.children == [] and not node.expanded() and node.terminal_value is None
        assert node.to_play == game.get_current_player()
        assert explorer.counters.expansions == n


def test_root_noise_on_a_childless_root_draws_nothing():
    from oracle import search as osearch
    rs = np.random.RandomState(11)
    before = rs.get_state()
    explorer = osearch.Explorer(de.search_config(4), True, rs)
    explorer.add_exploration_noise(osearch.Node(0))
    after = rs.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]


@pytest.mark.parametrize("training", [False, True])
def test_a_search_on_a_dead_end_root_evaluates_it_sims_times_and_raises_in_select_action(training):
    from oracle import search as osearch
    game = _dead_end_game(de.T71)
    A = game.get_num_actions()
    calls = []

    def ev(g):
        calls.append(g.get_length())
        return np.full(A, 1.0 / A, np.float32), np.float32(0.5)
    rs = np.random.RandomState(3)
    twin = np.random.RandomState(3)
    explorer = osearch.Explorer(de.search_config(6), training, rs)
    root = osearch.Node(0)
    with pytest.raises(IndexError) as err:
        explorer.run_mcts(game, ev, root)
    assert err.traceback[-1].name == "max_action" and any(t.name == "select_action" for t in err.traceback)
    assert calls == [game.get_length()] * 6 and root.visit_count == 6 and root.value_sum == 3.0 and root.children == []
    assert explorer.counters.simulations == 6 and explorer.counters.expansions == 6
    if training:                                        # no gamma draw, the two uniforms of select_action
        twin.random_sample(); twin.random_sample()
    assert np.array_equal(rs.get_state()[1], twin.get_state()[1]) and rs.get_state()[2] == twin.get_state()[2]


def test_the_float32_oracle_network_is_within_2e_6_of_float64_on_the_dead_end_leaves():
    """REF32_SHARE of tests/boardnet_cases.py: the float32 oracle may use a fifth of the project's 1e-5 (ORACLE_NET_TOL),
    which leaves a float32-accurate device the usual 5x."""
    import torch
    from scipy.special import softmax
    from boardnet_cases import REF32_SHARE
    from scs_replay import ORACLE_NET_TOL
    bound = REF32_SHARE * ORACLE_NET_TOL
    assert bound == pytest.approx(2e-6)
    cfg = sd.new_game("one_type_6x5").cfg
    r32, r64 = de.oracle_net(cfg), de.oracle_net(cfg, torch.float64)
    seen, worst = set(), [0.0, 0.0]
    for case in de.CASES:
        if case.evaluation != "net":
            continue
        for e in de.oracle_run(case)["evaluations"]:
            key = e["image"].tobytes()
            if not e["dead_end"] or key in seen:
                continue
            seen.add(key)
            (l32, v32), (l64, v64) = r32.inference(e["image"][None], None), r64.inference(e["image"][None], None)
            dp = float(np.max(np.abs(softmax(np.asarray(l32, np.float64).reshape(-1)) - softmax(np.asarray(l64).reshape(-1)))))
            dv = abs(float(np.asarray(v32).reshape(-1)[0]) - float(np.asarray(v64).reshape(-1)[0]))
            worst = [max(worst[0], dp), max(worst[1], dv)]
    print("distinct dead-end leaves", len(seen), "worst probability / value difference", worst)
    assert len(seen) >= 10
    assert worst[0] < bound and worst[1] < bound, worst
