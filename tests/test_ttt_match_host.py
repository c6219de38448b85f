"""Tic-Tac-Toe evaluation matches, the part that needs no GPU: the C ABI of nz_engine_match_play loads and refuses null
handles, TttMatch / TttAgentMatch / TttTester refuse what the library cannot play before any GPU call, and the random
mover's rule restated in numpy on a 3x3 mask agrees with RandomState.randint.  (The refusals that need two real engines --
one engine on both sides, different game counts, a training engine, no weights -- are in tests/test_gpu_ttt_match.py.)"""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from ttt_match_ref import random_move_on_mask, search_cfg   # noqa: E402


def test_ttt_match_symbols_load():
    from nuzero_amd import _lib
    for name in ("nz_engine_match_play", "nz_engine_match_streams"):
        assert hasattr(_lib.lib, name), name
        assert name in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.TttMatchResult) == 8 * 8
    assert (_lib.NZ_AGENT_MCTS, _lib.NZ_AGENT_POLICY, _lib.NZ_AGENT_RANDOM) == (0, 1, 2)
    import nuzero_amd
    from nuzero_amd.tester import TttAgentMatch, TttMatch, TttTester
    assert nuzero_amd.TttMatch is TttMatch and nuzero_amd.TttAgentMatch is TttAgentMatch and nuzero_amd.TttTester is TttTester


def test_null_handles_and_missing_seeds_are_refused_not_followed():
    from nuzero_amd import _lib
    play, err = _lib.lib.nz_engine_match_play, lambda: _lib.lib.nz_last_error(None).decode()
    seeds = np.arange(4, dtype=np.uint32)
    sp = ctypes.c_void_p(seeds.ctypes.data)
    for k1 in (_lib.NZ_AGENT_MCTS, _lib.NZ_AGENT_POLICY):           # an MCTS or policy side without an engine
        assert play(None, k1, None, _lib.NZ_AGENT_RANDOM, None, sp, None, None) == _lib.NZ_ERR_ARG
        assert "side 1" in err() and "needs an engine" in err()
        assert play(None, _lib.NZ_AGENT_RANDOM, None, k1, sp, None, None, None) == _lib.NZ_ERR_ARG
        assert "side 2" in err() and "needs an engine" in err()
    assert play(None, _lib.NZ_AGENT_RANDOM, None, _lib.NZ_AGENT_RANDOM, None, sp, None, None) == _lib.NZ_ERR_ARG
    assert "side 1" in err() and "seeds" in err()
    assert play(None, _lib.NZ_AGENT_RANDOM, None, _lib.NZ_AGENT_RANDOM, sp, None, None, None) == _lib.NZ_ERR_ARG
    assert "side 2" in err() and "seeds" in err()
    assert play(None, _lib.NZ_AGENT_RANDOM, None, _lib.NZ_AGENT_RANDOM, sp, sp, None, None) == _lib.NZ_ERR_ARG
    assert "two random sides" in err()
    assert play(None, 7, None, _lib.NZ_AGENT_RANDOM, None, sp, None, None) == _lib.NZ_ERR_ARG
    assert "unknown agent kind" in err()
    assert _lib.lib.nz_engine_match_streams(None, 0, None, None) == _lib.NZ_ERR_ARG


class _FakeEngine:
    """Stands where SelfPlayEngine would: building it is allowed (the refusals of play() need an object), anything that
    would reach the GPU is not."""
    made = 0

    def __init__(self, search_config, n_games, training=True, device=0):
        assert training is False
        type(self).made += 1
        self._h, self.device = None, None

    def _no(self, *a, **k):
        raise AssertionError("a GPU call was made: the refusal must come first")
    set_weights = set_table = _no

    def close(self):
        pass


@pytest.fixture
def no_gpu(monkeypatch):
    from nuzero_amd import _lib, engine

    class Lib:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was called: the refusal must come first")
    monkeypatch.setattr(engine, "SelfPlayEngine", _FakeEngine)
    monkeypatch.setattr(_lib, "lib", Lib())
    _FakeEngine.made = 0


def test_constructors_refuse_before_any_engine(no_gpu):
    from nuzero_amd import tester
    cfg = search_cfg(8)
    with pytest.raises(ValueError, match="keep_subtree"):
        tester.TttMatch(cfg, search_cfg(8, keep=False), 4)
    with pytest.raises(ValueError, match="keep_subtree"):
        tester.TttAgentMatch(("mcts", search_cfg(8, keep=False)), ("random",), 4)
    with pytest.raises(ValueError, match="n_matches"):
        tester.TttMatch(cfg, cfg, 0)
    with pytest.raises(ValueError, match="two random agents"):
        tester.TttAgentMatch(("random",), ("random",), 4)
    with pytest.raises(ValueError, match="agent spec"):
        tester.TttAgentMatch(("scripted",), ("random",), 4)
    with pytest.raises(ValueError, match="two search configs"):
        tester.TttMatch(cfg, ("policy",), 4)
    with pytest.raises(ValueError, match="share one engine"):         # an MCTS agent owns its trees
        tester.TttAgentMatch(("mcts", cfg), ("policy",), 4, share_policy_engine=True)
    assert _FakeEngine.made == 0
    m = tester.TttAgentMatch(("policy",), ("policy",), 4, share_policy_engine=True)
    assert _FakeEngine.made == 1 and m.engines[0] is m.engines[1]
    m = tester.TttAgentMatch(("mcts", cfg), ("random",), 4)
    assert m.engines[1] is None and m.kinds == ("mcts", "random")


def test_play_refuses_before_any_gpu_call(no_gpu):
    from nuzero_amd import tester
    cfg = search_cfg(8)
    table = np.zeros((3 ** 9, 10), np.float32)
    weights = {"w": np.zeros((4, 2, 3, 3), np.float32)}
    m = tester.TttAgentMatch(("mcts", cfg), ("random",), 4)
    with pytest.raises(ValueError, match="agent 1: a mcts agent needs a network"):
        m.play(None, None, agent_seeds=range(4))
    with pytest.raises(ValueError, match="pass agent_seeds"):
        m.play(table, None)
    with pytest.raises(ValueError, match="agent 2: 3 agent_seeds for 4 matches"):
        m.play(table, None, agent_seeds=range(3))
    with pytest.raises(ValueError, match="Seed must be between"):
        m.play(table, None, agent_seeds=[0, 1, 2, -1])
    with pytest.raises(ValueError, match="a table has shape"):
        m.play(np.zeros((100, 10), np.float32), None, agent_seeds=range(4))
    with pytest.raises(ValueError, match="net must be"):
        m.play("weights.pt", None, agent_seeds=range(4))
    with pytest.raises(ValueError, match=r"\(state_dict, set_weights kwargs\)"):
        m.play((weights, 64), None, agent_seeds=range(4))
    with pytest.raises(AssertionError, match="a GPU call was made"):   # a sound call gets that far
        m.play(table, None, agent_seeds=range(4))
    m = tester.TttAgentMatch(("random",), ("policy",), 4)
    with pytest.raises(ValueError, match="agent 2: a policy agent needs a network"):
        m.play(None, None, agent_seeds=range(4))
    m = tester.TttMatch(cfg, cfg, 4)
    with pytest.raises(ValueError, match="agent 2: a mcts agent needs a network"):
        m.play(weights, None)
    m = tester.TttAgentMatch(("policy",), ("policy",), 4, share_policy_engine=True)
    with pytest.raises(ValueError, match="the same net"):
        m.play(table, table.copy())
    t = tester.TttTester()
    with pytest.raises(ValueError, match="pass agent_seeds"):
        t.Test_using_agents(("policy",), table, ("random",), None, 4)
    with pytest.raises(ValueError, match="keep_subtree"):
        t.test_using_agents(search_cfg(8, keep=False), weights, ("random",), None, 4, agent_seeds=range(4))


def test_random_rule_on_a_3x3_mask_agrees_with_randint():
    """k = randint(n): masked rejection on 32-bit words, n == 1 draws nothing; then the k-th empty cell in ascending
    index.  n = 1..9 over 1000 seeds, on masks with n cells of the 3x3 board, several draws per stream."""
    pick = np.random.RandomState(7)
    for n in range(1, 10):
        for seed in range(1000):
            cells = np.sort(pick.permutation(9)[:n])
            mask = np.zeros(9, bool)
            mask[cells] = True
            mine, theirs = np.random.RandomState(seed), np.random.RandomState(seed)
            for _ in range(3):
                assert random_move_on_mask(mine, mask) == cells[theirs.randint(n)], (n, seed)
            a, b = mine.get_state(), theirs.get_state()
            assert a[2] == b[2] and np.array_equal(a[1], b[1]), (n, seed)       # the same words consumed
            if n == 1:
                assert a[2] == 624                                                # nothing drawn: never twisted
