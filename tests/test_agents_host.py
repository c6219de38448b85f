"""Evaluation matches against scripted agents (nz_scs_agent_match_*, nuzero_amd.tester.ScsAgentMatch), the part that
needs no GPU: the C ABI loads and refuses null arguments, ScsAgentMatch / ScsTester refuse what the library cannot play
before they touch a device, and tests/agents_ref.py -- the agents' CPU restatement the GPU tests
(tests/test_gpu_scs_agents.py) replay against -- draws what numpy's RandomState.randint draws."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
CONFIGS = os.path.join(HERE, "golden", "scs_configs")
MIRRORED = os.path.join(CONFIGS, "mirrored_5x5.yml")
RANDOMIZED = os.path.join(CONFIGS, "randomized_5x5.yml")

from test_match_host import search_cfg          # noqa: E402


def test_agent_match_symbols_load_and_refuse_null_arguments():
    import ctypes
    from nuzero_amd import _lib
    for name in ("nz_scs_agent_match_play", "nz_scs_agent_match_result", "nz_scs_agent_match_decisions",
                 "nz_scs_agent_record", "nz_scs_agent_record_read"):
        assert hasattr(_lib.lib, name), name
        assert name in _lib.SIGNATURES
    assert (_lib.NZ_AGENT_MCTS, _lib.NZ_AGENT_POLICY, _lib.NZ_AGENT_RANDOM) == (0, 1, 2)
    assert ctypes.sizeof(_lib.ScsAgent) == 24
    assert _lib.lib.nz_scs_agent_match_play(None, None, None, 0, None) == _lib.NZ_ERR_ARG
    a = _lib.ScsAgent(kind=_lib.NZ_AGENT_RANDOM, net=None, seeds_host=None)
    assert _lib.lib.nz_scs_agent_match_play(None, ctypes.byref(a), ctypes.byref(a), 0, None) == _lib.NZ_ERR_ARG
    assert _lib.lib.nz_scs_agent_match_result(None, None, None, None) == _lib.NZ_ERR_ARG
    assert _lib.lib.nz_scs_agent_match_decisions(None, 0, None, None, None, None) == _lib.NZ_ERR_ARG
    assert _lib.lib.nz_scs_agent_record(None, 0, None, 0, 0) == _lib.NZ_ERR_ARG
    assert _lib.lib.nz_scs_agent_record_read(None, 0, 0, None, None, None, None) == _lib.NZ_ERR_ARG
    import nuzero_amd
    from nuzero_amd.tester import ScsAgentMatch
    assert nuzero_amd.ScsAgentMatch is ScsAgentMatch


class _NoEngine:
    """Stands in for ScsSelfPlay: built without a GPU, and any use of it is the test's failure."""

    def __init__(self, *a, **k):
        pass

    def __getattr__(self, name):
        raise AssertionError(f"the engine was used ({name}): the refusal must come first")


def test_agent_match_refuses_before_any_gpu_call(monkeypatch):
    from nuzero_amd import scs, tester

    def no_engine(*a, **k):
        raise AssertionError("an engine was created: the refusal must come first")
    monkeypatch.setattr(scs, "ScsSelfPlay", no_engine)
    with pytest.raises(ValueError, match="use ScsMatch"):
        tester.ScsAgentMatch(MIRRORED, ("mcts", search_cfg(8)), ("mcts", search_cfg(8)), 4)
    with pytest.raises(ValueError, match="keep_subtree"):
        tester.ScsAgentMatch(MIRRORED, ("mcts", search_cfg(8, keep=False)), ("random",), 4)
    with pytest.raises(ValueError, match="keep_subtree"):
        tester.ScsAgentMatch(MIRRORED, ("policy",), ("mcts", search_cfg(8, keep=False)), 4)
    with pytest.raises(ValueError, match="agent spec"):
        tester.ScsAgentMatch(MIRRORED, ("scripted",), ("random",), 4)
    with pytest.raises(ValueError, match="n_matches"):
        tester.ScsAgentMatch(MIRRORED, ("policy",), ("random",), 0)
    with pytest.raises(AssertionError, match="an engine was created"):            # a sound pair gets that far
        tester.ScsAgentMatch(MIRRORED, ("mcts", search_cfg(8)), ("random",), 4)
    # the tester routes two MCTS specs to ScsMatch (whose own refusals stand) and everything else to ScsAgentMatch
    t = tester.ScsTester(MIRRORED)
    with pytest.raises(ValueError, match="keep_subtree"):
        t.test_using_agents(("mcts", search_cfg(8)), None, ("mcts", search_cfg(8, keep=False)), None, 4)
    with pytest.raises(ValueError, match="keep_subtree"):
        t.test_using_agents(search_cfg(8, keep=False), None, ("random",), None, 4, agent_seeds=range(4))

    # play(): an object whose engine must not be touched
    monkeypatch.setattr(scs, "ScsSelfPlay", _NoEngine)
    net = object()
    m = tester.ScsAgentMatch(MIRRORED, ("mcts", search_cfg(8)), ("random",), 4)
    with pytest.raises(ValueError, match="agent_seeds"):
        m.play(net, None)
    with pytest.raises(ValueError, match="needs a network"):
        m.play(None, None, agent_seeds=range(4))
    with pytest.raises(ValueError, match="3 agent_seeds for 4 matches"):
        m.play(net, None, agent_seeds=range(3))
    with pytest.raises(ValueError, match="Seed must be between"):
        m.play(net, None, agent_seeds=[0, 1, 2, -1])
    m = tester.ScsAgentMatch(MIRRORED, ("random",), ("policy",), 4)
    with pytest.raises(ValueError, match="agent 2: a policy agent needs a network"):
        m.play(None, None, agent_seeds=range(4))
    m = tester.ScsAgentMatch(MIRRORED, ("random",), ("random",), 4)
    with pytest.raises(ValueError, match="agent 2: 5 agent_seeds"):
        m.play(None, None, agent_seeds=(range(4), range(5)))
    from nuzero_amd.scs import ScsGameConfig
    m = tester.ScsAgentMatch(ScsGameConfig(RANDOMIZED, per_game=True), ("policy",), ("random",), 4)
    with pytest.raises(ValueError, match="pass seeds"):
        m.play(net, None, agent_seeds=range(4))
    with pytest.raises(ValueError, match="2 seeds for 4 matches"):
        m.play(net, None, seeds=[1, 2], agent_seeds=range(4))


@pytest.mark.parametrize("seed", [0, 1, 12345, 2 ** 32 - 1])
def test_random_rule_restatement_draws_what_randint_draws(seed):
    from agents_ref import legacy_randint
    mine, ref = np.random.RandomState(seed), np.random.RandomState(seed)
    for rounds in range(12):                                  # ~ 800 draws: past the first twist of the state
        for n in range(1, 65):
            before = mine.get_state()[2]
            assert legacy_randint(mine, n) == int(ref.randint(n)), (seed, rounds, n)
            if n == 1:
                assert mine.get_state()[2] == before          # nothing drawn
            a, b = mine.get_state(), ref.get_state()
            assert a[2] == b[2] and np.array_equal(a[1], b[1]), (seed, rounds, n)


def test_agent_refs_play_a_match_on_the_oracle():
    """RandomAgentRef / PolicyAgentRef are agents of oracle.agents.play_match: the random side takes the k-th legal
    action in ascending index, the policy side the first maximum among the legal ones; a round is a function of the
    seed."""
    from agents_ref import PolicyAgentRef, RandomAgentRef
    from oracle.agents import play_match
    from oracle.scs import ScsConfig, ScsGame

    class Spy(RandomAgentRef):
        def choose_action(self, game):
            legal = np.flatnonzero(np.asarray(game.possible_actions()).reshape(-1))
            twin = np.random.RandomState()
            twin.set_state(self.rs.get_state())
            a = super().choose_action(game)
            assert a == int(legal[int(twin.randint(len(legal)))])
            return a

    def flat(game):                                           # equal probabilities: every decision is a tie
        A = game.get_num_actions()
        return np.full((A,), 1.0 / A, np.float32), 0.0

    game = ScsGame(ScsConfig(MIRRORED))
    rnd, pol = Spy(77), PolicyAgentRef(flat)
    actions = play_match(game, pol, rnd)
    assert game.is_terminal() and len(actions) == game.length == len(rnd.actions) + len(pol.actions)
    g2 = ScsGame(ScsConfig(MIRRORED))
    for a in actions:
        legal = np.flatnonzero(np.asarray(g2.possible_actions()).reshape(-1))
        if g2.get_current_player() == 1:
            assert a == legal[0]                              # the tie goes to the lowest flat action index
        g2.step_index(a)
    again = play_match(ScsGame(ScsConfig(MIRRORED)), PolicyAgentRef(flat), RandomAgentRef(77))
    assert again == actions
    other = play_match(ScsGame(ScsConfig(MIRRORED)), PolicyAgentRef(flat), RandomAgentRef(78))
    assert other != actions
