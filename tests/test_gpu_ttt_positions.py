"""Tic-Tac-Toe searches and evaluation matches from given positions (nz_engine_reset_to, nz_engine_match_play_from,
nz_engine_policy_actions; SelfPlayEngine.reset(boards), TttAgentMatch.play(start_boards=...), TttTester).

Everything is exact equality against the CPU oracle: the sides read the table evaluators random_table(101) /
random_table(202) at 25 simulations, so oracle/agents.py play_match and oracle/search.py Explorer on an oracle game stepped
to the position read the very same float32 numbers.  Oracle results are computed once and shared."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from nuzero_amd import ttt_positions as tp   # noqa: E402
from ttt_positions_ref import (expected_record_from, gpu_table, images_of, minimax_on_the_oracle, oracle_match_from,   # noqa: E402
                               oracle_search_at, random_table, search_cfg)

pytestmark = pytest.mark.gpu

SIMS = 25
CFG = search_cfg(SIMS)
PAIRINGS = {
    "mcts_vs_mcts": (("mcts", CFG), ("mcts", CFG)),
    "mcts_vs_policy": (("mcts", CFG), ("policy",)),
    "policy_vs_random": (("policy",), ("random",)),
    "mcts_vs_random": (("mcts", CFG), ("random",)),
    "random_vs_mcts": (("random",), ("mcts", CFG)),
}
START_SETS = {"two": 2, "three": 3, "eight": 8}       # the 72 / 252 (side 2 moves first) / 222 (one ply left) positions
_cache = {}


def tables():
    if "tables" not in _cache:
        _cache["tables"] = (random_table(101), random_table(202))
        for t in _cache["tables"]:
            t.setflags(write=False)
    return _cache["tables"]


def seeds_for(n):
    return list(range(7000, 7000 + n))


def with_seeds(spec, seed):
    return ("random", seed) if spec[0] == "random" else spec


def oracle_round(specs, t1, t2, plies, key):
    """The oracle matches of a pairing from every opening of `plies` plies (a random side of match j: seeds_for(n)[j])."""
    if key not in _cache:
        boards = tp.openings(plies)
        seeds = seeds_for(len(boards))
        _cache[key] = [oracle_match_from(b, with_seeds(specs[0], seeds[j]), t1, with_seeds(specs[1], seeds[j]), t2)
                       for j, b in enumerate(boards)]
    return _cache[key]


def oracle_searches():
    """oracle_search_at on every reachable non-terminal position, table 101."""
    if "searches" not in _cache:
        from oracle import search as osearch
        ev = osearch.table_evaluator(tables()[0])
        _cache["searches"] = [oracle_search_at(b, CFG, ev) for b in tp.reachable_nonterminal()]
    return _cache["searches"]


def nets_of(specs, t1, t2):
    return tuple(None if s[0] == "random" else t for s, t in zip(specs, (t1, t2)))


# ---- 1. a search from every position ----------------------------------------------------------------------------------------
def test_search_from_every_position_equals_the_oracle():
    """One engine of 4,520 games (no multiple of the 16 games of a workgroup): reset(boards), search(), apply().  Record
    0 -- the first decision made at the position -- holds the oracle's visit counts, action and child count from a fresh
    root; lengths count the plies since; hist_board[0] is the given board."""
    from nuzero_amd.engine import SelfPlayEngine
    boards = tp.reachable_nonterminal()
    want = oracle_searches()
    e = SelfPlayEngine(CFG, len(boards), training=False)
    try:
        e.set_table(tables()[0])
        e.reset(boards)
        e.search()
        e.apply()
        last = e.last_actions().cpu().numpy()
        r = e.export()
    finally:
        e.close()
    assert np.array_equal(r["actions"][:, 0], np.array([w[0] for w in want], np.int32))
    assert np.array_equal(last, r["actions"][:, 0]) and (r["actions"][:, 1:] == -1).all()
    assert np.array_equal(r["visits"][:, 0], np.stack([w[1] for w in want]))
    assert np.array_equal(r["n_children"][:, 0], np.array([w[2] for w in want], np.int32))
    assert (r["tree_size"][:, 0] == SIMS).all()
    assert (r["lengths"] == 1).all()
    assert np.array_equal(r["outcomes"], np.array([w[4] if w[3] else 0 for w in want], np.int32))
    assert np.array_equal(r["states"][:, 0], images_of(boards)) and not r["states"][:, 1:].any()


def test_search_from_positions_on_a_real_network():
    """The 64-wide RecurrentNet of tests/test_gpu_ttt_match.py on the lock-step network route, on the 222 eight-stone and
    the 72 two-stone positions in one engine (mixed plies): the actions equal the oracle's on the engine's own
    net_forward outputs."""
    from nuzero_amd.engine import SelfPlayEngine
    from nuzero_amd.weights import synthetic_recurrent_net_weights
    from oracle import search as osearch
    boards = np.concatenate([tp.openings(8), tp.openings(2)])
    e = SelfPlayEngine(CFG, len(boards), training=False)
    try:
        e.set_weights(synthetic_recurrent_net_weights(0, 2, 1, 64, 2, True), recurrent_iterations=2)
        table = gpu_table(e)
        e.reset(boards)
        e.search()
        e.apply()
        got = e.last_actions().cpu().numpy()
    finally:
        e.close()
    ev = osearch.table_evaluator(table)
    assert got.tolist() == [oracle_search_at(b, CFG, ev)[0] for b in boards]


# ---- 2. matches from positions ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", list(START_SETS))
@pytest.mark.parametrize("name", list(PAIRINGS))
def test_matches_from_positions_equal_the_oracle(name, start):
    from nuzero_amd.tester import TttAgentMatch
    specs, k = PAIRINGS[name], START_SETS[start]
    t1, t2 = tables()
    boards = tp.openings(k)
    n = len(boards)
    games = oracle_round(specs, t1, t2, k, (name, start))
    m = TttAgentMatch(specs[0], specs[1], n)
    try:
        r = m.play(*nets_of(specs, t1, t2), agent_seeds=seeds_for(n) if ("random",) in specs else None, start_boards=boards)
        streams = {i: m.random_streams(i) for i, s in enumerate(specs) if s[0] == "random"}
        exports = {i: m.engines[i].export(states=False) for i, s in enumerate(specs) if s[0] == "mcts"}
    finally:
        m.close()
    actions, lengths, outcomes, tally = expected_record_from(games)
    assert (actions[:, :k] == -1).all() and (lengths > k).all()
    assert np.array_equal(r["actions"], actions)
    assert np.array_equal(r["lengths"], lengths) and np.array_equal(r["outcomes"], outcomes)
    assert (r["p1_wins"], r["p2_wins"], r["draws"], r["unfinished"]) == tally
    assert np.array_equal(r["start_boards"], boards)
    for i, s in enumerate(specs):
        if s[0] == "mcts":
            assert r["agent_actions"][i] is None and r["agent_n_legal"][i] is None
            ex = exports[i]                                  # the engine counts from the position: the record shifted by k
            assert np.array_equal(ex["actions"][:, :9 - k], r["actions"][:, k:]) and (ex["actions"][:, 9 - k:] == -1).all()
            assert np.array_equal(ex["lengths"], lengths - k) and np.array_equal(ex["outcomes"], outcomes)
            continue
        assert np.array_equal(r["agent_actions"][i], np.array([g["sides"][i]["agent_actions"] for g in games], np.int32)), i
        assert np.array_equal(r["agent_n_legal"][i], np.array([g["sides"][i]["agent_n_legal"] for g in games], np.int32)), i
        if s[0] == "random":
            keys, pos = streams[i]
            assert np.array_equal(pos, np.array([g["sides"][i]["pos"] for g in games], np.int32))
            assert np.array_equal(keys, np.stack([g["sides"][i]["keys"] for g in games]))
            if k == 8:                                       # one legal cell: nothing is drawn, the stream never twisted
                mine = r["agent_n_legal"][i][:, 8]
                assert ((mine == 1) | (mine == 0)).all() and (pos == 624).all()


def test_openings_make_deterministic_matches_differ():
    """A condition on the fixed tables, on the oracle alone: from the empty board MCTS against MCTS is one game; the 72
    two-ply openings give more than one continuation and all three outcomes."""
    t1, t2 = tables()
    games = oracle_round(PAIRINGS["mcts_vs_mcts"], t1, t2, 2, ("mcts_vs_mcts", "two"))
    assert len({tuple(g["actions"]) for g in games}) > 1
    assert {g["terminal_value"] for g in games} == {1, -1, 0}


# ---- 3. nothing changes without positions -----------------------------------------------------------------------------------
def _plain_match_play(m, seeds, n):
    """nz_engine_match_play itself on the engines of a TttAgentMatch(("mcts", cfg), ("random",))."""
    import torch
    from nuzero_amd import _lib
    dev = m.engines[0].device
    new = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    actions, lengths, outcomes, aa, an = new(n, 9), new(n), new(n), [new(n, 9), new(n, 9)], [new(n, 9), new(n, 9)]
    tally = (ctypes.c_int64 * 4)()
    res = _lib.TttMatchResult(actions=actions.data_ptr(), lengths=lengths.data_ptr(), outcomes=outcomes.data_ptr(),
                              agent_actions=(ctypes.c_void_p * 2)(*[t.data_ptr() for t in aa]),
                              agent_n_legal=(ctypes.c_void_p * 2)(*[t.data_ptr() for t in an]), tally4_host=tally)
    s = np.asarray(seeds, np.uint32)
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(_lib.lib.nz_engine_match_play(m.engines[0]._h, _lib.NZ_AGENT_MCTS, None, _lib.NZ_AGENT_RANDOM, None,
                                                 ctypes.c_void_p(s.ctypes.data), ctypes.byref(res), stream), m.engines[0]._h)
    return {"actions": actions.cpu().numpy(), "lengths": lengths.cpu().numpy(), "outcomes": outcomes.cpu().numpy(),
            "agent_actions": aa[1].cpu().numpy(), "agent_n_legal": an[1].cpu().numpy(), "tally": list(tally)}


def _same_round(r, plain):
    for key in ("actions", "lengths", "outcomes"):
        assert np.array_equal(r[key], plain[key]), key
    assert np.array_equal(r["agent_actions"][1], plain["agent_actions"])
    assert np.array_equal(r["agent_n_legal"][1], plain["agent_n_legal"])
    assert [r["p1_wins"], r["p2_wins"], r["draws"], r["unfinished"]] == plain["tally"]


def test_nothing_changes_without_positions():
    from nuzero_amd.tester import TttAgentMatch
    n = 64
    seeds = seeds_for(n)
    t1, _ = tables()
    m = TttAgentMatch(("mcts", CFG), ("random",), n)
    try:
        m.engines[0].set_table(t1)
        plain = _plain_match_play(m, seeds, n)
        assert len({tuple(a) for a in plain["actions"].tolist()}) > 1 and sum(plain["tally"]) == n
        none = m.play(t1, None, agent_seeds=seeds)
        assert none["start_boards"] is None
        _same_round(none, plain)
        _same_round(m.play(t1, None, agent_seeds=seeds, start_boards=[0] * n), plain)
        from_two = m.play(t1, None, agent_seeds=seeds, start_boards=tp.openings(2)[:n])
        assert (from_two["actions"][:, :2] == -1).all() and not np.array_equal(from_two["actions"], plain["actions"])
        _same_round(m.play(t1, None, agent_seeds=seeds), plain)          # no state leaks through the reset
    finally:
        m.close()


def test_reset_after_positions_is_the_empty_board_again():
    from nuzero_amd.engine import SelfPlayEngine
    n = 72
    t1, _ = tables()
    used, fresh = SelfPlayEngine(CFG, n, training=False), SelfPlayEngine(CFG, n, training=False)
    try:
        for e in (used, fresh):
            e.set_table(t1)
        used.reset(tp.openings(2))
        used.search()
        used.apply()
        for e in (used, fresh):                                          # reset() itself: the empty board again
            e.reset()
            e.search()
            e.apply()
        first = [e.export(trace=True) for e in (used, fresh)]
        used.reset()
        used.play_lockstep(base_seed=11)
        fresh.play_lockstep(base_seed=11)
        a, b = used.export(trace=True), fresh.export(trace=True)
    finally:
        used.close()
        fresh.close()
    assert (b["lengths"] >= 5).all() and (first[1]["lengths"] == 1).all()
    for key in first[0]:
        assert np.array_equal(first[0][key], first[1][key]), key
    assert not first[1]["states"][:, 0].any()                            # record 0 was made at the empty board
    for key in a:
        assert np.array_equal(a[key], b[key]), key


# ---- 4. the tester from openings ------------------------------------------------------------------------------------------------
def test_from_openings_counts_both_colour_assignments_per_agent():
    from nuzero_amd.tester import TttTester
    t1, t2 = tables()
    specs = PAIRINGS["mcts_vs_mcts"]
    first = oracle_round(specs, t1, t2, 2, ("mcts_vs_mcts", "two"))
    second = oracle_round(specs, t2, t1, 2, ("mcts_vs_mcts exchanged", "two"))      # agent 2 plays side 1
    v1 = np.array([g["terminal_value"] for g in first])
    v2 = np.array([g["terminal_value"] for g in second])
    want = (int((v1 > 0).sum() + (v2 < 0).sum()), int((v1 < 0).sum() + (v2 > 0).sum()), int((v1 == 0).sum() + (v2 == 0).sum()))
    t = TttTester()
    try:
        got = t.test_from_openings(CFG, t1, CFG, t2, plies=2)
        rounds = t.opening_rounds
    finally:
        t.close()
    assert got == want and sum(got) == 144
    assert np.array_equal(rounds[0]["actions"], expected_record_from(first)[0])
    assert np.array_equal(rounds[1]["actions"], expected_record_from(second)[0])


# ---- 5. the score against perfect play ------------------------------------------------------------------------------------------
def _tables_from_perfect_play():
    """Two policy tables by position code: uniform mass on the optimal moves; all mass on the lowest legal non-optimal
    cell where there is one (else uniform on the legal cells, all of which are optimal)."""
    _, masks = tp.perfect_play()
    good, bad = np.zeros((3 ** 9, 10), np.float32), np.zeros((3 ** 9, 10), np.float32)
    for b in tp.reachable_nonterminal():
        b = int(b)
        code, legal = tp.ttt_code(b), ~(b | (b >> 16)) & 0x1FF
        best = int(masks[code])
        opt = [a for a in range(9) if (best >> a) & 1]
        good[code, opt] = 1.0 / len(opt)
        worse = [a for a in range(9) if ((legal & ~best) >> a) & 1]
        if worse:
            bad[code, worse[0]] = 1.0
        else:
            bad[code, opt] = 1.0 / len(opt)
    return good, bad


def test_policy_score_against_perfect_play():
    from nuzero_amd.tester import TttTester
    good, bad = _tables_from_perfect_play()
    solved = minimax_on_the_oracle()
    boards = tp.reachable_nonterminal()
    free = [solved[tp.ttt_code(b)][1] == (~(int(b) | (int(b) >> 16)) & 0x1FF) for b in boards]
    assert sum(free) == 1329
    t = TttTester()
    try:
        s = t.score_against_perfect_play(("policy",), good)
        assert s["positions"] == 4520 and s["optimal"] == 4520 and s["is_optimal"].all()
        assert np.array_equal(s["boards"], boards)
        assert s["by_ply"].tolist() == [[c, c] for c in (1, 9, 72, 252, 756, 1140, 1372, 696, 222)]
        s = t.score_against_perfect_play(("policy",), bad)
        assert s["optimal"] == 1329 and s["is_optimal"].tolist() == free
    finally:
        t.close()


def test_mcts_score_against_perfect_play():
    from nuzero_amd.tester import TttTester
    want = oracle_searches()
    solved = minimax_on_the_oracle()
    boards = tp.reachable_nonterminal()
    t = TttTester()
    try:
        s = t.score_against_perfect_play(("mcts", CFG), tables()[0])
    finally:
        t.close()
    assert s["actions"].tolist() == [w[0] for w in want]
    ok = [bool((solved[tp.ttt_code(b)][1] >> w[0]) & 1) for b, w in zip(boards, want)]
    assert s["is_optimal"].tolist() == ok and s["optimal"] == sum(ok) and s["positions"] == 4520
    by_ply = np.zeros((9, 2), np.int64)
    for b, o in zip(boards, ok):
        by_ply[bin(int(b)).count("1")] += (1, int(o))
    assert np.array_equal(s["by_ply"], by_ply)


# ---- 6. refusals that need real engines -----------------------------------------------------------------------------------------
def test_refusals_that_need_real_engines():
    """Before any launch, with the index or the counts named: a training engine, n_slots != n_games, unplayable boards
    through the bare C ABI, mixed stone counts; afterwards the engines still play."""
    from nuzero_amd import _lib
    from nuzero_amd.engine import SelfPlayEngine
    lib = _lib.lib
    t1, _ = tables()
    n = 8
    a, b = SelfPlayEngine(CFG, n, training=False), SelfPlayEngine(CFG, n, training=False)
    tr, part = SelfPlayEngine(CFG, n, training=True), SelfPlayEngine(CFG, n, training=False, n_slots=4)
    M, P, R = _lib.NZ_AGENT_MCTS, _lib.NZ_AGENT_POLICY, _lib.NZ_AGENT_RANDOM
    two = tp.openings(2)[:n].copy()
    ptr = lambda arr: ctypes.c_void_p(arr.ctypes.data)
    msg = lambda e: lib.nz_last_error(e._h).decode()
    bad = two.copy()
    bad[5] = 0o007 | (0o030 << 16)                                          # player one already has the top row
    mixed = two.copy()
    mixed[3] = tp.openings(3)[0]
    import torch
    out_dev = torch.zeros((n + 1,), dtype=torch.int32, device=a.device)
    out = ctypes.c_void_p(out_dev.data_ptr())
    try:
        for e in (a, b, tr, part):
            e.set_table(t1)
        with pytest.raises(_lib.NzError, match="training engine"):
            tr.reset(two)
        assert lib.nz_engine_reset_to(tr._h, ptr(two), None) == _lib.NZ_ERR_ARG
        with pytest.raises(_lib.NzError, match="n_slots == n_games"):
            part.reset(two)
        assert lib.nz_engine_reset_to(part._h, ptr(two), None) == _lib.NZ_ERR_STATE
        with pytest.raises(ValueError, match="3 boards for 8 games"):
            a.reset(two[:3])
        assert lib.nz_engine_reset_to(a._h, None, None) == _lib.NZ_ERR_ARG and "NULL boards" in msg(a)
        assert lib.nz_engine_reset_to(a._h, ptr(bad), None) == _lib.NZ_ERR_ARG
        assert "start board 5 (0x00180007) is not playable" in msg(a) and "has a line" in msg(a)
        assert lib.nz_engine_match_play_from(a._h, M, b._h, M, None, None, ptr(bad), None, None) == _lib.NZ_ERR_ARG
        assert "start board 5 (0x00180007) is not playable" in msg(a) and msg(b) == msg(a)
        assert lib.nz_engine_match_play_from(a._h, M, b._h, P, None, None, ptr(mixed), None, None) == _lib.NZ_ERR_ARG
        assert "start boards 0 and 3 hold 2 and 3 stones" in msg(a)
        # nz_engine_match_play's own refusals come first, boards or not
        assert lib.nz_engine_match_play_from(a._h, M, tr._h, M, None, None, ptr(bad), None, None) == _lib.NZ_ERR_ARG
        assert "side 2: a training engine" in msg(a)
        assert lib.nz_engine_match_play_from(part._h, M, b._h, M, None, None, ptr(two), None, None) == _lib.NZ_ERR_ARG
        assert "side 1: a match engine needs n_slots == n_games" in msg(b)
        assert lib.nz_engine_policy_actions(a._h, ptr(bad), n, out, None) == _lib.NZ_ERR_ARG
        assert "start board 5" in msg(a)
        assert lib.nz_engine_policy_actions(a._h, ptr(two), n + 1, out, None) == _lib.NZ_ERR_ARG
        assert "9 positions" in msg(a)
        assert lib.nz_engine_policy_actions(a._h, ptr(two), n, None, None) == _lib.NZ_ERR_ARG
        # the library's check and ttt_positions.is_playable give the same verdict in the same words
        rs = np.random.RandomState(3)
        words = [1 << 9, 1 << 31, (1 << 4) | (1 << 20), 3, 1 << 16, 0o030 | (1 << 8) | (0o007 << 16), 0b101001110 | (0b010110001 << 16)]
        words += [int(w) for w in rs.randint(0, 1 << 32, 100, dtype=np.uint64)]
        words += [int(p1) | (int(p2) << 16) for p1, p2 in rs.randint(0, 512, (400, 2))] + [0] + [int(w) for w in two[:3]]
        verdicts = set()
        for w in words:
            ok, why = tp.is_playable(w)
            one = np.array([w], np.uint32)
            st = lib.nz_engine_policy_actions(a._h, ptr(one), 1, out, None)
            assert (st == _lib.NZ_OK) == ok, hex(w)
            assert ok or msg(a) == f"start board 0 (0x{w:08x}) is not playable: {why}"
            verdicts.add(why)
        assert len(verdicts) == 6                                            # every condition, and playable ones
        # nothing was launched or reset: the refused engines still play, from positions and from the empty board
        tally = (ctypes.c_int64 * 4)()
        res = _lib.TttMatchResult(tally4_host=tally)
        assert lib.nz_engine_match_play_from(a._h, M, b._h, M, None, None, ptr(two), ctypes.byref(res), None) == _lib.NZ_OK
        assert sum(tally) == n and tally[3] == 0
        assert lib.nz_engine_match_play(a._h, M, b._h, P, None, None, ctypes.byref(res), None) == _lib.NZ_OK
        assert sum(tally) == n and tally[3] == 0
        assert a.policy_actions(two[:5]).cpu().numpy().tolist() == [
            int(np.argmax(np.where([(int(x) | (int(x) >> 16)) >> c & 1 == 0 for c in range(9)], t1[tp.ttt_code(x), :9], -np.inf)))
            for x in two[:5]]
    finally:
        for e in (a, b, tr, part):
            e.close()
