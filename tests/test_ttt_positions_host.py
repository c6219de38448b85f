"""Tic-Tac-Toe start positions, the part that needs no GPU: nuzero_amd.ttt_positions (openings, the 4,520 reachable
non-terminal positions, perfect play) against a walk and a minimax over oracle/ttt.py, the C ABI of nz_engine_reset_to /
nz_engine_match_play_from / nz_engine_policy_actions loads and refuses null arguments, and TttAgentMatch / TttTester
refuse what cannot be played before any engine call.  (Refusals that need real engines: tests/test_gpu_ttt_positions.py.)"""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from nuzero_amd import ttt_positions as tp   # noqa: E402
from ttt_positions_ref import board_of, minimax_on_the_oracle, search_cfg, walk_positions   # noqa: E402

REACHABLE = [1, 9, 72, 252, 756, 1260, 1520, 1140, 390, 78]
PLAYABLE = [1, 9, 72, 252, 756, 1140, 1372, 696, 222, 0]
_cache = {}


def walked():
    if "walk" not in _cache:
        _cache["walk"] = walk_positions()
    return _cache["walk"]


def test_counts_and_order_against_a_walk_over_the_oracle_game():
    games = walked()
    by_stones, playable = [0] * 10, [[] for _ in range(10)]
    for code, g in games.items():
        by_stones[g.length] += 1
        if not g.is_terminal():
            playable[g.length].append(code)
    assert by_stones == REACHABLE and sum(by_stones) == 5478
    assert [len(p) for p in playable] == PLAYABLE and sum(PLAYABLE) == 4520
    for k in range(9):
        got = tp.openings(k)
        assert got.dtype == np.uint32
        codes = [tp.ttt_code(b) for b in got]
        assert codes == sorted(playable[k]), k                        # the same set, in ascending code order
        for b, c in zip(got, codes):
            assert int(b) == board_of(games[c]) and tp.is_playable(b) == (True, None)
            assert bin(int(b)).count("1") == k
    every = tp.reachable_nonterminal()
    assert every.dtype == np.uint32 and len(every) == 4520
    codes = [tp.ttt_code(b) for b in every]
    assert codes == sorted(c for p in playable for c in p)
    assert codes == [games[c].code() for c in codes]                  # ttt_code is oracle.ttt.TicTacToe.code
    with pytest.raises(ValueError, match="0 .. 8 stones"):
        tp.openings(9)
    assert len(tp.openings(0)) == 1 and int(tp.openings(0)[0]) == 0


def test_perfect_play_against_a_minimax_on_the_oracle_game():
    values, masks = tp.perfect_play()
    want = minimax_on_the_oracle()
    assert len(want) == 5478 and values.shape == masks.shape == (3 ** 9,)
    for code, (v, m) in want.items():
        assert (int(values[code]), int(masks[code])) == (v, m), code
    unreached = np.ones(3 ** 9, bool)
    unreached[list(want)] = False
    assert not values[unreached].any() and not masks[unreached].any()
    code = lambda acts: tp.ttt_code(tp.board_from_actions(acts))
    assert values[0] == 0 and masks[0] == 0x1FF                       # a draw, and every first move keeps it
    assert masks[code([4])] == sum(1 << a for a in (0, 2, 6, 8)) and values[code([4])] == 0
    assert masks[code([0])] == 1 << 4 and values[code([0])] == 0
    free = 0
    for b in tp.reachable_nonterminal():
        b = int(b)
        free += int(masks[tp.ttt_code(b)]) == (~(b | (b >> 16)) & 0x1FF)
    assert free == 1329                                               # positions where every legal move is optimal


def test_board_from_actions():
    assert int(tp.board_from_actions([])) == 0
    assert int(tp.board_from_actions([4, 0, 8])) == (1 << 4) | (1 << 8) | (1 << 16)
    with pytest.raises(ValueError, match="taken"):
        tp.board_from_actions([4, 4])
    with pytest.raises(ValueError, match="0 .. 8"):
        tp.board_from_actions([9])
    with pytest.raises(ValueError, match="game is over"):
        tp.board_from_actions([0, 3, 1, 4, 2, 5])


@pytest.mark.parametrize("board,words", [
    (1 << 9, "outside the stone sets"),
    (1 << 31, "outside the stone sets"),
    ((1 << 4) | (1 << 20), "both players"),
    ((1 << 0) | (1 << 1), "neither 0 nor 1"),                         # two stones of player one, none of player two
    (1 << 16, "neither 0 nor 1"),                                     # player two moved first
    (0o007 | (0o030 << 16), "has a line"),
    (0o030 | (1 << 8) | (0o007 << 16), "has a line"),
    (0b101001110 | (0b010110001 << 16), "no cell is empty"),          # a drawn full board
])
def test_is_playable_names_the_condition(board, words):
    ok, why = tp.is_playable(board)
    assert not ok and words in why
    with pytest.raises(ValueError, match=r"start board 1 \(0x%08x\) is not playable: .*%s" % (board, words)):
        tp.check_start_boards([0, board, 1 << 9])


def test_the_c_abi_loads_and_refuses_null_arguments():
    from nuzero_amd import _lib
    lib, err = _lib.lib, lambda: _lib.lib.nz_last_error(None).decode()
    for name in ("nz_engine_reset_to", "nz_engine_match_play_from", "nz_engine_policy_actions"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    boards = np.zeros(4, np.uint32)
    bp = ctypes.c_void_p(boards.ctypes.data)
    assert lib.nz_engine_reset_to(None, bp, None) == _lib.NZ_ERR_ARG and "NULL engine" in err()
    assert lib.nz_engine_reset_to(None, None, None) == _lib.NZ_ERR_ARG
    assert lib.nz_engine_policy_actions(None, bp, 4, bp, None) == _lib.NZ_ERR_ARG and "NULL engine" in err()
    assert lib.nz_engine_policy_actions(None, None, 4, None, None) == _lib.NZ_ERR_ARG
    # with and without start boards: nz_engine_match_play's refusals, in the same words, and they come first
    seeds = np.arange(4, dtype=np.uint32)
    sp = ctypes.c_void_p(seeds.ctypes.data)
    M, P, R = _lib.NZ_AGENT_MCTS, _lib.NZ_AGENT_POLICY, _lib.NZ_AGENT_RANDOM
    bad = np.full(4, 1 << 9, np.uint32)
    cases = [((None, M, None, R, None, sp), "side 1: an MCTS or policy side needs an engine"),
             ((None, R, None, P, sp, None), "side 2: an MCTS or policy side needs an engine"),
             ((None, R, None, R, None, sp), "side 1: a random side needs agent seeds"),
             ((None, R, None, R, sp, sp), "two random sides"),
             ((None, 7, None, R, None, sp), "side 1: unknown agent kind 7")]
    for args, words in cases:
        assert lib.nz_engine_match_play(*args, None, None) == _lib.NZ_ERR_ARG
        want = err()
        assert words in want
        for start in (None, bp, ctypes.c_void_p(bad.ctypes.data)):
            assert lib.nz_engine_match_play_from(*args, start, None, None) == _lib.NZ_ERR_ARG
            assert err() == want
    import nuzero_amd
    assert nuzero_amd.ttt_positions is tp


class _FakeEngine:
    """Stands where SelfPlayEngine would (as in tests/test_ttt_match_host.py): building it is counted, anything that
    would reach the GPU is refused."""
    made = 0

    def __init__(self, search_config, n_games, training=True, device=0):
        assert training is False
        type(self).made += 1
        self._h, self.device = None, None

    def _no(self, *a, **k):
        raise AssertionError("a GPU call was made: the refusal must come first")
    set_weights = set_table = reset = search = apply = policy_actions = _no

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


def test_play_refuses_start_boards_before_any_gpu_call(no_gpu):
    from nuzero_amd import tester
    cfg = search_cfg(8)
    table = np.zeros((3 ** 9, 10), np.float32)
    two = tp.openings(2)[:4]
    m = tester.TttAgentMatch(("mcts", cfg), ("policy",), 4)
    with pytest.raises(ValueError, match="3 start_boards for 4 matches"):
        m.play(table, table, start_boards=two[:3])
    with pytest.raises(ValueError, match=r"start board 2 \(0x00000003\) is not playable: .*neither 0 nor 1"):
        m.play(table, table, start_boards=[0, 0, 3, 0])
    with pytest.raises(ValueError, match="start boards 0 and 3 hold 2 and 3 stones"):
        m.play(table, table, start_boards=list(two[:3]) + [tp.openings(3)[0]])
    with pytest.raises(ValueError, match="agent 2: a policy agent needs a network"):     # the earlier refusals stand
        m.play(table, None, start_boards=two)
    with pytest.raises(AssertionError, match="a GPU call was made"):                     # a sound call gets that far
        m.play(table, table, start_boards=two)
    m = tester.TttMatch(cfg, cfg, 4)
    with pytest.raises(ValueError, match="start boards 0 and 1 hold 0 and 1 stones"):
        m.play(table, table, start_boards=[0, 1, 0, 0])


def test_the_tester_refuses_before_any_engine(no_gpu):
    from nuzero_amd import tester
    cfg = search_cfg(8)
    table = np.zeros((3 ** 9, 10), np.float32)
    t = tester.TttTester()
    with pytest.raises(ValueError, match="a random agent has no move to score"):
        t.score_against_perfect_play(("random",), None)
    with pytest.raises(ValueError, match="needs a network"):
        t.score_against_perfect_play(cfg, None)
    with pytest.raises(ValueError, match="a table has shape"):
        t.score_against_perfect_play(("policy",), np.zeros((9, 10), np.float32))
    with pytest.raises(ValueError, match="keep_subtree"):
        t.score_against_perfect_play(search_cfg(8, keep=False), table)
    with pytest.raises(ValueError, match="two random agents"):
        t.test_from_openings(("random",), None, ("random",), None, agent_seeds=range(72))
    with pytest.raises(ValueError, match="0 .. 8 stones"):
        t.test_from_openings(cfg, table, ("policy",), table, plies=9)
    assert _FakeEngine.made == 0
    with pytest.raises(ValueError, match="agent 2: 4 agent_seeds for 72 matches"):
        t.test_from_openings(cfg, table, ("random",), None, agent_seeds=range(4))
    with pytest.raises(AssertionError, match="a GPU call was made"):                     # sound calls get that far
        t.test_from_openings(cfg, table, ("policy",), table)
    with pytest.raises(AssertionError, match="a GPU call was made"):
        t.score_against_perfect_play(("policy",), table)


def test_the_tester_keeps_both_colour_assignments(no_gpu):
    """test_from_openings plays a pairing and then the same pairing with the sides exchanged: the tester keeps both
    matches, so a second call between two different agents builds no engine; another pairing closes both."""
    from nuzero_amd import tester
    cfg = search_cfg(8)
    t = tester.TttTester()
    assert t.opening_rounds is None
    a = t._match_of(cfg, ("policy",), 4)
    b = t._match_of(("policy",), cfg, 4)
    assert a is not b and _FakeEngine.made == 4
    assert t._match_of(cfg, ("policy",), 4) is a and t._match_of(("policy",), cfg, 4) is b
    assert t._match_of(("policy",), cfg, 4) is b and _FakeEngine.made == 4
    c = t._match_of(cfg, ("random",), 4)
    assert c is not a and t._exchanged is None and _FakeEngine.made == 5
    assert t._match_of(cfg, cfg, 4) is t._match_of(cfg, cfg, 4) and t._exchanged is None      # its own exchange
    t.close()
    assert t._match is None and t._exchanged is None
