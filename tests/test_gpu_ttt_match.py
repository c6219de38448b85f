"""Tic-Tac-Toe evaluation matches played inside the library (nz_engine_match_play; TttMatch / TttAgentMatch /
TttTester): 64 matches at 25 simulations per move.

Exact replay: both sides read a table evaluator of seeded random numbers, so oracle/agents.py play_match on oracle/ttt.py
with MctsAgentRef and the policy / random restatements of tests/agents_ref.py reads the very same float32 numbers and must
play the very same games.  The oracle games are computed once per pairing and shared."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from ttt_match_ref import expected_record, oracle_match, random_move_on_mask, random_table, search_cfg   # noqa: E402

pytestmark = pytest.mark.gpu

N, SIMS = 64, 25
SEEDS = list(range(5000, 5000 + N))
CFG = search_cfg(SIMS)
PAIRINGS = {
    "mcts_vs_random": (("mcts", CFG), ("random",)),
    "random_vs_mcts": (("random",), ("mcts", CFG)),
    "policy_vs_random": (("policy",), ("random",)),
    "mcts_vs_policy": (("mcts", CFG), ("policy",)),
}
_cache = {}


def tables():
    if "tables" not in _cache:
        _cache["tables"] = (random_table(101), random_table(202))
        for t in _cache["tables"]:
            t.setflags(write=False)
    return _cache["tables"]


def oracle_games(name):
    """The N oracle matches of a pairing (side i reads table i; a random side of match j is RandomState(SEEDS[j]))."""
    if name not in _cache:
        t1, t2 = tables()
        s1, s2 = PAIRINGS[name]
        _cache[name] = [oracle_match(s1 if s1[0] != "random" else ("random", SEEDS[j]), t1,
                                     s2 if s2[0] != "random" else ("random", SEEDS[j]), t2) for j in range(N)]
    return _cache[name]


def nets_of(specs, t1, t2):
    return tuple(None if s[0] == "random" else t for s, t in zip(specs, (t1, t2)))


def check_against(r, games, specs):
    actions, lengths, outcomes, tally = expected_record(games)
    assert np.array_equal(r["actions"], actions)
    assert np.array_equal(r["lengths"], lengths) and np.array_equal(r["outcomes"], outcomes)
    assert (r["p1_wins"], r["p2_wins"], r["draws"], r["unfinished"]) == tally
    for i, s in enumerate(specs):
        if s[0] == "mcts":
            assert r["agent_actions"][i] is None and r["agent_n_legal"][i] is None
            continue
        assert np.array_equal(r["agent_actions"][i], np.array([g["sides"][i]["agent_actions"] for g in games], np.int32)), i
        assert np.array_equal(r["agent_n_legal"][i], np.array([g["sides"][i]["agent_n_legal"] for g in games], np.int32)), i


@pytest.mark.parametrize("name", list(PAIRINGS))
def test_exact_replay_on_the_oracle(name):
    from nuzero_amd.tester import TttAgentMatch
    specs = PAIRINGS[name]
    t1, t2 = tables()
    games = oracle_games(name)
    m = TttAgentMatch(specs[0], specs[1], N)
    try:
        r = m.play(*nets_of(specs, t1, t2), agent_seeds=SEEDS if ("random",) in specs else None)
        check_against(r, games, specs)
        for i, s in enumerate(specs):
            if s[0] == "mcts":               # the MCTS side's own engine followed every match to its end
                ex = m.engines[i].export(states=False)
                assert np.array_equal(ex["actions"], r["actions"]) and np.array_equal(ex["outcomes"], r["outcomes"])
    finally:
        m.close()


def test_matches_with_a_random_side_differ_and_deterministic_pairings_do_not():
    """A condition on the fixed seeds and tables (checked on the oracle alone when they were chosen): the 64
    MCTS-vs-random matches are not copies of one game; MCTS against the bare policy is one game 64 times."""
    assert len({tuple(g["actions"]) for g in oracle_games("mcts_vs_random")}) > 1
    assert len({tuple(g["actions"]) for g in oracle_games("mcts_vs_policy")}) == 1
    from nuzero_amd.tester import TttAgentMatch
    t1, t2 = tables()
    m = TttAgentMatch(("mcts", CFG), ("random",), N)
    try:
        r = m.play(t1, None, agent_seeds=SEEDS)
        assert len({tuple(row) for row in r["actions"].tolist()}) > 1
    finally:
        m.close()


def test_a_mover_with_one_legal_cell_draws_nothing():
    """random vs MCTS: the random side moves at the ninth ply of a match that gets there, with one empty cell; every
    match's stream must be left exactly where the restatement's is (key and position)."""
    from nuzero_amd.tester import TttAgentMatch
    t1, t2 = tables()
    games = oracle_games("random_vs_mcts")
    ninth = [j for j, g in enumerate(games) if g["length"] == 9]
    assert ninth, "no match of these seeds reaches the ninth ply"
    m = TttAgentMatch(("random",), ("mcts", CFG), N)
    try:
        r = m.play(None, t2, agent_seeds=SEEDS)
        keys, pos = m.random_streams(0)
        with pytest.raises(Exception, match="no random side"):
            m.random_streams(1)
    finally:
        m.close()
    for j in ninth:
        assert r["agent_n_legal"][0][j, 8] == 1 and r["agent_actions"][0][j, 8] == games[j]["actions"][8]
    for j, g in enumerate(games):
        assert pos[j] == g["sides"][0]["pos"], j
        assert np.array_equal(keys[j], g["sides"][0]["keys"]), j


def test_policy_ties_go_to_the_lowest_legal_cell():
    """An all-zero table: every probability equal, so each side plays the lowest empty cell: 0 1 2 3 4 5 6, and
    player 1 completes 2-4-6."""
    from nuzero_amd.tester import TttAgentMatch
    zero = np.zeros((3 ** 9, 10), np.float32)
    m = TttAgentMatch(("policy",), ("policy",), N)
    try:
        r = m.play(zero, zero)
    finally:
        m.close()
    want = np.array([0, 1, 2, 3, 4, 5, 6, -1, -1], np.int32)
    assert np.array_equal(r["actions"], np.tile(want, (N, 1)))
    assert (r["lengths"] == 7).all() and (r["outcomes"] == 1).all()
    assert (r["p1_wins"], r["p2_wins"], r["draws"], r["unfinished"]) == (N, 0, 0, 0)
    assert np.array_equal(r["agent_actions"][0], np.tile(np.array([0, -1, 2, -1, 4, -1, 6, -1, -1], np.int32), (N, 1)))
    assert np.array_equal(r["agent_n_legal"][1], np.tile(np.array([0, 8, 0, 6, 0, 4, 0, 0, 0], np.int32), (N, 1)))


def _weights(seed):
    from nuzero_amd.weights import synthetic_recurrent_net_weights
    return synthetic_recurrent_net_weights(seed, 2, 1, 64, 2, True)


def test_two_policy_sides_on_one_shared_engine():
    """Real RecurrentNet weights through the stand-alone network route: one engine for both policy sides gives what two
    engines with the same weights give, and that is the game of the network's own masked argmax."""
    from nuzero_amd.tester import TttAgentMatch
    w = _weights(0)
    shared, apart = TttAgentMatch(("policy",), ("policy",), N, share_policy_engine=True), TttAgentMatch(("policy",), ("policy",), N)
    try:
        assert shared.engines[0] is shared.engines[1] and apart.engines[0] is not apart.engines[1]
        a, b = shared.play(w, w, recurrent_iterations=2), apart.play(w, w, recurrent_iterations=2)
        for key in ("actions", "lengths", "outcomes"):
            assert np.array_equal(a[key], b[key]), key
        for key in ("agent_actions", "agent_n_legal"):
            for i in range(2):
                assert np.array_equal(a[key][i], b[key][i]), (key, i)
        assert [a[k] for k in ("p1_wins", "p2_wins", "draws", "unfinished")] == [b[k] for k in ("p1_wins", "p2_wins", "draws", "unfinished")]
        # the same game from net_forward's probabilities, move by move on the host
        from oracle import ttt as ottt
        game, want = ottt.TicTacToe(), []
        while not game.is_terminal():
            _, _, probs = apart.engines[0].net_forward(game.state_image())
            p = probs.cpu().numpy().reshape(-1)
            mask = game.possible_actions().reshape(-1) != 0
            want.append(int(np.argmax(np.where(mask, p, -np.inf))))
            game.step_index(want[-1])
        assert a["actions"][0, :len(want)].tolist() == want and (a["actions"] == a["actions"][0]).all()
        assert a["lengths"][0] == len(want) and a["outcomes"][0] == game.terminal_value
    finally:
        shared.close()
        apart.close()


def _engine(weights):
    from nuzero_amd.engine import SelfPlayEngine
    e = SelfPlayEngine(CFG, N, training=False)
    e.set_weights(weights, recurrent_iterations=2)
    return e


def _ply_by_ply(e1, e2, seeds):
    """Today's loop of search / apply / last_actions (the low-level form): e1 plays player 1;
    e2 an engine, or None for a random mover drawn by numpy on the host."""
    engines = [e for e in (e1, e2) if e is not None]
    for e in engines:
        e.reset()
    rs = [np.random.RandomState(s) for s in seeds] if e2 is None else None
    boards = np.zeros((N, 9), np.int32)
    actions = np.full((N, 9), -1, np.int32)
    for ply in range(9):
        alive = e1.alive().cpu().numpy() != 0
        if not alive.any():
            break
        for e in engines:
            e.search()
        mover = e1 if ply % 2 == 0 else e2
        if mover is not None:
            mover.apply()
            a = mover.last_actions()
            for e in engines:
                if e is not mover:
                    e.apply(actions=a)
            a = a.cpu().numpy()
        else:
            a = np.full((N,), -1, np.int32)
            for j in np.flatnonzero(alive):
                a[j] = random_move_on_mask(rs[j], boards[j] == 0)
            e1.apply(actions=a)
        for j in np.flatnonzero(alive):
            actions[j, ply] = a[j]
            boards[j, a[j]] = 1 + ply % 2
    assert e1.live_games() == 0
    return actions


def test_same_games_as_the_ply_by_ply_route():
    """Real RecurrentNet weights (two different sets): MCTS vs MCTS and MCTS vs random through nz_engine_match_play play
    the action lists of the Python loop over nz_engine_search / _apply / _last_actions."""
    from nuzero_amd.tester import TttAgentMatch, TttMatch
    w1, w2 = _weights(0), _weights(1)
    e1, e2 = _engine(w1), _engine(w2)
    try:
        want_mm = _ply_by_ply(e1, e2, None)
        want_mr = _ply_by_ply(e1, None, SEEDS)
    finally:
        e1.close()
        e2.close()
    assert (want_mm == want_mm[0]).all() and len({tuple(r) for r in want_mr.tolist()}) > 1
    m = TttMatch(CFG, CFG, N)
    try:
        r = m.play(w1, w2, recurrent_iterations=2)
        assert np.array_equal(r["actions"], want_mm)
        assert r["p1_wins"] + r["p2_wins"] + r["draws"] == N and r["unfinished"] == 0
    finally:
        m.close()
    m = TttAgentMatch(("mcts", CFG), ("random",), N)
    try:
        r = m.play(w1, None, agent_seeds=SEEDS, recurrent_iterations=2)
        assert np.array_equal(r["actions"], want_mr)
        assert np.array_equal(r["lengths"], (want_mr >= 0).sum(1))
    finally:
        m.close()


def test_lifecycle_rounds_repeat():
    """Two plays on the same engines with the same seeds give identical records; so does a play after a self-play round
    on a different engine of the same process; and TttTester counts the same games."""
    from nuzero_amd.engine import SelfPlayEngine
    from nuzero_amd.tester import TttAgentMatch, TttTester
    t1, t2 = tables()
    games = oracle_games("mcts_vs_random")
    m = TttAgentMatch(("mcts", CFG), ("random",), N)
    try:
        first = m.play(t1, None, agent_seeds=SEEDS)
        other = m.play(t1, None, agent_seeds=[s + 1000 for s in SEEDS])
        assert not np.array_equal(first["actions"], other["actions"])           # the streams are rebuilt from the seeds
        again = m.play(t1, None, agent_seeds=SEEDS)
        sp = SelfPlayEngine(CFG, 16, training=True)
        sp.set_table(t2)
        sp.play(base_seed=3)
        assert (sp.export(states=False)["lengths"] >= 5).all()
        sp.close()
        third = m.play(t1, None, agent_seeds=SEEDS)
    finally:
        m.close()
    for r in (first, again, third):
        check_against(r, games, PAIRINGS["mcts_vs_random"])
    t = TttTester()
    try:
        got = t.Test_using_agents(CFG, t1, ("random",), None, N, agent_seeds=SEEDS)
        assert got == expected_record(games)[3][:3]
        got = t.test_using_agents(("policy",), t1, ("random",), None, N, agent_seeds=SEEDS)
        assert got == expected_record(oracle_games("policy_vs_random"))[3][:3]
    finally:
        t.close()


def test_refusals_that_need_real_engines():
    """NZ_ERR_ARG with a message, before any launch: one engine on both sides (unless both are policy sides), engines
    with different game counts, a training engine, a side without weights or table, an engine passed for a random side."""
    from nuzero_amd import _lib
    from nuzero_amd.engine import SelfPlayEngine
    t1, _ = tables()
    a, b = SelfPlayEngine(CFG, 8, training=False), SelfPlayEngine(CFG, 8, training=False)
    c, tr = SelfPlayEngine(CFG, 4, training=False), SelfPlayEngine(CFG, 8, training=True)
    seeds = np.arange(8, dtype=np.uint32)
    sp = ctypes.c_void_p(seeds.ctypes.data)
    M, P, R = _lib.NZ_AGENT_MCTS, _lib.NZ_AGENT_POLICY, _lib.NZ_AGENT_RANDOM

    def refused(e1, k1, e2, k2, s1, s2, words):
        st = _lib.lib.nz_engine_match_play(e1._h if e1 else None, k1, e2._h if e2 else None, k2, s1, s2, None, None)
        assert st == _lib.NZ_ERR_ARG, words
        msg = _lib.lib.nz_last_error((e1 or e2)._h).decode()
        assert words in msg, msg
    try:
        refused(a, M, b, M, None, None, "side 1: no network")
        a.set_table(t1)
        refused(a, M, b, P, None, None, "side 2: no network")
        b.set_table(t1)
        c.set_table(t1)
        tr.set_table(t1)
        refused(a, M, a, M, None, None, "same engine")
        refused(a, M, a, P, None, None, "same engine")
        refused(a, P, a, M, None, None, "same engine")
        refused(a, M, c, M, None, None, "8 and 4 games")
        refused(c, P, a, M, None, None, "4 and 8 games")
        refused(tr, M, b, M, None, None, "side 1: a training engine")
        refused(a, M, tr, P, None, None, "side 2: a training engine")
        refused(a, M, None, R, None, None, "side 2: a random side needs agent seeds")
        refused(a, M, b, R, None, sp, "side 2: a random side takes no engine")
        # nothing was launched or reset: the refused engines still play, and two policy sides may share one
        tally = (ctypes.c_int64 * 4)()
        res = _lib.TttMatchResult(tally4_host=tally)
        assert _lib.lib.nz_engine_match_play(a._h, P, a._h, P, None, None, ctypes.byref(res), None) == _lib.NZ_OK
        assert sum(tally) == 8 and tally[3] == 0
        assert _lib.lib.nz_engine_match_play(a._h, M, None, R, None, sp, ctypes.byref(res), None) == _lib.NZ_OK
        assert sum(tally) == 8 and tally[3] == 0
    finally:
        for e in (a, b, c, tr):
            e.close()
