"""Evaluation matches, the part that needs no GPU: the C ABI of nz_scs_match_* loads, ScsMatch refuses what the
library cannot play before it touches a device, and tests/match_replay.py -- the oracle replay the GPU tests
(tests/test_gpu_scs_match.py) rest on -- reproduces an oracle match from recorded evaluations alone."""
import copy
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
CONFIGS = os.path.join(HERE, "golden", "scs_configs")


def search_cfg(sims, keep=True):
    return {"Simulation": {"mcts_simulations": sims, "keep_subtree": keep}, "UCT": {"pb_c_base": 10000, "pb_c_init": 1.15},
            "Exploration": {"number_of_softmax_moves": 0, "epsilon_softmax_exploration": 0.04,
                            "epsilon_random_exploration": 0.001, "value_factor": 1,
                            "root_exploration_distribution": "gamma", "root_exploration_fraction": 0.2,
                            "root_dist_alpha": 0.15, "root_dist_beta": 1}}


def test_match_symbols_load():
    import ctypes
    from nuzero_amd import _lib
    for name in ("nz_scs_match_play", "nz_scs_match_result"):
        assert hasattr(_lib.lib, name), name
        assert name in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.ScsMatchTally) == 7 * 8
    # null handles are refused, not followed
    assert _lib.lib.nz_scs_match_play(None, None, None, None, 0, None) == _lib.NZ_ERR_ARG
    assert _lib.lib.nz_scs_match_result(None, None, None, None, None) == _lib.NZ_ERR_ARG
    import nuzero_amd
    from nuzero_amd.tester import ScsMatch, ScsTester
    assert nuzero_amd.ScsMatch is ScsMatch and nuzero_amd.ScsTester is ScsTester


def test_scsmatch_refuses_before_any_gpu_call(monkeypatch):
    from nuzero_amd import scs, tester
    from nuzero_amd.scs import ScsGameConfig

    def no_engine(*a, **k):
        raise AssertionError("an engine was created: the refusal must come first")
    monkeypatch.setattr(scs, "ScsSelfPlay", no_engine)
    path = os.path.join(CONFIGS, "mirrored_5x5.yml")
    with pytest.raises(ValueError, match="keep_subtree"):
        tester.ScsMatch(path, search_cfg(8), search_cfg(8, keep=False), 4)
    with pytest.raises(ValueError, match="keep_subtree"):
        tester.ScsMatch(path, search_cfg(8, keep=False), search_cfg(8), 4)
    with pytest.raises(ValueError, match="do not explore"):
        tester.ScsMatch(path, search_cfg(8), search_cfg(8), 4, training=True)
    with pytest.raises(ValueError, match="configs differ"):
        tester.ScsMatch((path, os.path.join(CONFIGS, "two_types_6x5.yml")), search_cfg(8), search_cfg(8), 4)
    with pytest.raises(ValueError, match="configs differ"):                       # same board, another game
        tester.ScsMatch((ScsGameConfig(path), ScsGameConfig(os.path.join(CONFIGS, "late_reinforcements_5x5.yml"))),
                        search_cfg(8), search_cfg(8), 4)
    with pytest.raises(ValueError, match="n_matches"):
        tester.ScsMatch(path, search_cfg(8), search_cfg(8), 0)
    with pytest.raises(AssertionError, match="an engine was created"):            # a sound pair gets that far
        tester.ScsMatch((path, path), search_cfg(8), search_cfg(8), 4)


def _oracle_match(path, sims1, sims2):
    from match_replay import RecordingEvaluator
    from oracle.agents import MctsAgentRef, play_match
    from oracle.scs import ScsConfig, ScsGame
    from scs_eval import evaluate_image
    game = ScsGame(ScsConfig(path))
    A = game.cfg.num_actions
    ev = lambda g: evaluate_image(g.state_image()[0], A)
    r1, r2 = RecordingEvaluator(ev), RecordingEvaluator(ev)
    actions = play_match(game, MctsAgentRef(search_cfg(sims1), r1), MctsAgentRef(search_cfg(sims2), r2))
    return [int(a) for a in actions], game, r1.arrays(), r2.arrays()


@pytest.mark.parametrize("config,sims1,sims2", [("mirrored_5x5.yml", 12, 7), ("late_reinforcements_5x5.yml", 6, 10)])
def test_match_replay_reproduces_an_oracle_match_from_recorded_evaluations(config, sims1, sims2):
    from match_replay import replay_match
    path = os.path.join(CONFIGS, config)
    actions, game, rec1, rec2 = _oracle_match(path, sims1, sims2)
    assert len(rec1[2]) > len(actions) and len(rec2[2]) > len(actions)
    out = replay_match((path, search_cfg(sims1), search_cfg(sims2), rec1, rec2))
    assert out["actions"] == actions
    assert out["length"] == game.length == len(actions) and out["terminal_value"] == game.terminal_value
    assert out["lookups"] == out["recorded"] == (len(rec1[2]), len(rec2[2]))
    assert out["unused"] == ([], [])


def test_match_replay_never_computes_an_evaluation():
    from match_replay import MissingEvaluation, RecordedEvaluations, replay_match
    path = os.path.join(CONFIGS, "mirrored_5x5.yml")
    actions, game, rec1, rec2 = _oracle_match(path, 8, 8)
    cut = len(rec2[2]) // 2                        # agent 2's list loses one row: its look-up must miss
    short = tuple(np.delete(a, cut, axis=0) for a in rec2)
    with pytest.raises(MissingEvaluation, match="agent 2"):
        replay_match((path, search_cfg(8), search_cfg(8), rec1, short))
    with pytest.raises(MissingEvaluation, match="agent 1"):   # the agents' lists are not interchangeable
        replay_match((path, search_cfg(8), search_cfg(5), rec1, rec2))
    # a surplus row is reported, not ignored
    extra = tuple(np.concatenate([a, a[-1:]]) for a in rec1)
    out = replay_match((path, search_cfg(8), search_cfg(8), extra, rec2))
    assert out["actions"] == actions and out["unused"] == ([len(rec1[2])], [])
    # an empty list answers nothing
    empty = RecordedEvaluations(np.zeros((0, 2), np.uint64), np.zeros((0, 4), np.float32), np.zeros((0,), np.float32))
    with pytest.raises(MissingEvaluation):
        empty(copy.deepcopy(game))
