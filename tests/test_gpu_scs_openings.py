"""SCS evaluation matches from opening positions (nz_scs_search_reset_to, nz_scs_match_play_from,
nz_scs_agent_match_play_from, nz_scs_openings_draw / _expand; nuzero_amd.scs_positions, ScsTester.test_from_openings).

The reference is tests/scs_openings_ref.py: oracle/scs.py stepped through the prefix, numpy's own RandomState for the
drawn openings, a breadth-first enumeration deduplicated on the state image, and oracle/agents.py play_match started
at the prefix's position and fed the evaluations the DEVICE agents recorded (it never computes one itself), so every
action, length and outcome must equal the device's, every recorded row must be asked for and none may be missing.
Small shapes: 5x5 maps, ConvNet / ResNet of 32 filters, 16 and 8 simulations.  Needs a GPU."""
import os
import sys
from ctypes import byref, c_void_p

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
pytestmark = pytest.mark.gpu
CONFIGS = os.path.join(HERE, "golden", "scs_configs")
MIRRORED = os.path.join(CONFIGS, "mirrored_5x5.yml")
RANDOMIZED = os.path.join(CONFIGS, "randomized_5x5.yml")
TWO_TYPES = os.path.join(CONFIGS, "two_types_6x5.yml")

from test_gpu_scs_configs import a1_search, _net          # noqa: E402
from scs_openings_ref import (apply_prefix, draw_prefix, enumerate_openings, legal_actions, oracle_game, random_game,      # noqa: E402
                              replay_agent_match_from, replay_match_from, run_jobs, status_row)
from scs_replay import image_mix_digest                   # noqa: E402

SIMS1, SIMS2 = 16, 8
N = 10                                                    # matches of the mixed rounds
MIXED_PLIES = [0, 1, 2, 4, 0, 1, 2, 4, 1, 2]
MAX_BATCH = 64                                            # the 55 two-ply positions of mirrored_5x5 fit one network


def _pack(prefixes, width=None):
    width = max([len(p) for p in prefixes] + [1]) if width is None else width
    a = np.zeros((len(prefixes), width), np.int32)
    for g, p in enumerate(prefixes):
        a[g, :len(p)] = p
    return a, np.array([len(p) for p in prefixes], np.int32)


def _mixed_prefixes(path, plies, first_seed, map_seeds=None):
    return [draw_prefix(path, first_seed + g, k, None if map_seeds is None else map_seeds[g]) for g, k in enumerate(plies)]


def _raw_openings(actions, n_plies, max_plies):
    """An nz_scs_openings straight from arrays: what the Python surface would refuse reaches the library."""
    from nuzero_amd import _lib
    a = np.ascontiguousarray(actions, np.int32)
    k = np.ascontiguousarray(n_plies, np.int32) if n_plies is not None else None
    return _lib.ScsOpenings(actions=a.ctypes.data, n_plies=k.ctypes.data if k is not None else None, max_plies=max_plies), (a, k)


@pytest.fixture(scope="module")
def nets():
    from nuzero_amd.scs import ScsGameConfig
    cfg = ScsGameConfig(MIRRORED)
    net1, _ = _net(cfg, "convnet", 32, 2, seed=811, gain=2.0, max_batch=MAX_BATCH)
    net2, _ = _net(cfg, "resnet", 32, 2, seed=822, gain=2.0, max_batch=MAX_BATCH)
    yield {"cfg": cfg, "nets": (net1, net2), "search": (a1_search(SIMS1), a1_search(SIMS2))}
    net1.close(); net2.close()


def _record_all(m, games):
    for a, sims in zip(m.agents, (SIMS1, SIMS2)):
        a.persistent(1)
        a.record(games, sims * (a.MAX_MOVES + 1))


def _stop_recording(m):
    for a in m.agents:
        a.record([], 0)
        a.persistent(-1)


@pytest.fixture(scope="module")
def mixed_round(nets):
    """Check 4's round: 10 matches from openings of 0, 1, 2 and 4 plies, persistent route, every evaluation recorded;
    and the plain round of the same match object."""
    from nuzero_amd.tester import ScsMatch
    (net1, net2), (s1, s2) = nets["nets"], nets["search"]
    m = ScsMatch(nets["cfg"], s1, s2, N)
    prefixes = _mixed_prefixes(MIRRORED, MIXED_PLIES, 300)
    start, n_plies = _pack(prefixes)
    _record_all(m, range(N))
    r = m.play(net1, net2, start_actions=start, n_plies=n_plies)
    assert m.agents[0].persistent() and m.agents[1].persistent()
    recs = (m.agents[0].records(), m.agents[1].records())
    status = (m.agents[0].status(), m.agents[1].status())
    exports = (m.agents[0].export(), m.agents[1].export())
    _stop_recording(m)
    plain = m.play(net1, net2)
    yield {"m": m, "r": r, "recs": recs, "status": status, "exports": exports, "prefixes": prefixes, "start": start, "n_plies": n_plies, "plain": plain}
    m.close()


def _same_round(ra, rb, label):
    for k in ("actions", "lengths", "outcomes", "finished"):
        assert ra[k].shape == rb[k].shape and np.array_equal(ra[k], rb[k]), (label, k)
    for k in ("matches", "p1_wins", "p2_wins", "draws", "unfinished", "length_sum", "length_max"):
        assert ra[k] == rb[k], (label, k)


def _check_replays(r, outs, games, prefixes, label):
    assert len(outs) == len(games)
    for g, out in zip(games, outs):
        n, k = int(r["lengths"][g]), len(prefixes[g])
        print(f"{label}: match {g}: opening of {k} plies, {n} decisions, outcome {r['outcomes'][g]}, evaluations asked for "
              f"{out['lookups']} of {out['recorded']} recorded")
        assert r["actions"][g, :k].tolist() == list(prefixes[g]), (label, g)        # the opening at its decision numbers
        assert out["actions"] == r["actions"][g, :n].tolist(), (label, g)
        assert (r["actions"][g, n:] == -1).all(), (label, g)
        assert out["length"] == n and out["terminal_value"] == r["outcomes"][g], (label, g)
        assert out["lookups"] == out["recorded"], (label, g, out["lookups"], out["recorded"])
        assert out["unused"] == ([], []), (label, g)


# ---- 1. reset_to equals the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [MIRRORED, RANDOMIZED], ids=["mirrored_5x5", "randomized_5x5_per_game"])
def test_reset_to_equals_the_oracle(path):
    from nuzero_amd.scs import ScsGameConfig
    from nuzero_amd.tester import ScsMatch
    G, per_game = 16, path == RANDOMIZED
    cfg = ScsGameConfig(path, per_game=True) if per_game else ScsGameConfig(path)
    map_seeds = [7300 + g for g in range(G)] if per_game else None
    prefixes = _mixed_prefixes(path, [g % 7 for g in range(G)], 40, map_seeds)          # 0 to 6 plies
    start, n_plies = _pack(prefixes)
    net1, _ = _net(cfg, "convnet", 32, 2, seed=811, gain=2.0, max_batch=G)
    net2, _ = _net(cfg, "resnet", 32, 2, seed=822, gain=2.0, max_batch=G)
    m = ScsMatch(cfg, a1_search(SIMS1), a1_search(SIMS2), G)
    e = m.agents[0]
    if per_game:
        e.set_games(map_seeds)
    e.reset_to(start, n_plies)
    games = [apply_prefix(oracle_game(path, None if not per_game else map_seeds[g]), prefixes[g]) for g in range(G)]
    assert e.status().tolist() == [status_row(g) for g in games]
    assert e.last_actions().cpu().numpy().tolist() == [p[-1] if p else -1 for p in prefixes]
    ex = e.export()
    for g, p in enumerate(prefixes):                       # records by decision number; nobody searched these plies
        assert ex["actions"][g, :len(p)].tolist() == p and (ex["actions"][g, len(p):] == -1).all()
        assert (ex["n_children"][g] == 0).all() and (ex["tree_size"][g] == 0).all()
    assert ex["simulations"] == 0
    # one search on the persistent route: the first evaluation each agent consumes is its fresh root's, the position itself
    _record_all(m, range(G))
    r = m.play(net1, net2, seeds=map_seeds, max_moves=1, start_actions=start, n_plies=n_plies)
    assert m.agents[0].persistent() and m.agents[1].persistent()
    assert r["lengths"].tolist() == [len(p) + 1 for p in prefixes] and r["unfinished"] == G
    for a in m.agents:
        recs = a.records()
        for g in range(G):
            assert recs[g][0][0].tolist() == image_mix_digest(games[g].state_image()[0]).tolist(), g
    _stop_recording(m)
    m.close(); net1.close(); net2.close()


# ---- 2. the device draw equals the reference's prefixes bit for bit ------------------------------------------------------------
# Opening seed 179 on mirrored_5x5, and 1130 on randomized_5x5's map of seed 8130, pass a position with exactly one
# legal action at their eighth ply (found by searching the fixtures with the reference): randint draws nothing there, which
# shows in the plies after it -- so those two rounds are also drawn to 10 plies.
@pytest.mark.parametrize("path,opening_seeds,map_seeds", [
    (MIRRORED, [179] + list(range(60, 75)), None),
    (RANDOMIZED, [1130] + list(range(80, 95)), [8130] + list(range(7400, 7415)))], ids=["mirrored_5x5", "randomized_5x5_per_game"])
def test_the_device_draw_equals_the_reference(path, opening_seeds, map_seeds):
    from nuzero_amd.scs import ScsGameConfig, ScsSelfPlay
    from nuzero_amd.scs_positions import random_openings
    G = len(opening_seeds)
    cfg = ScsGameConfig(path, per_game=True) if map_seeds else ScsGameConfig(path)
    e = ScsSelfPlay(cfg, a1_search(1), G, training=False)
    if map_seeds:
        e.set_games(map_seeds)
    before = e.status()
    for plies in (8, 10):
        n_legal = [[] for _ in range(G)]
        want = [draw_prefix(path, opening_seeds[g], plies, map_seeds[g] if map_seeds else None, n_legal[g]) for g in range(G)]
        if plies == 8:
            assert n_legal[0][7] == 1, n_legal[0]          # the fixture's single-action position is on the way
        actions, n_plies = random_openings(e, opening_seeds, plies)
        assert actions.dtype == np.int32 and actions.shape == (G, plies) and n_plies.tolist() == [plies] * G
        assert actions.tolist() == want
    assert np.array_equal(e.status(), before)              # drawing touches no game of the engine
    assert len({tuple(w) for w in want}) > 1
    e.close()


# ---- 3. all_openings equals the reference ----------------------------------------------------------------------------------------
def test_all_openings_equals_the_reference():
    from nuzero_amd._lib import NZ_ERR_STATE, NzError
    from nuzero_amd.scs import ScsGameConfig, ScsSelfPlay
    from nuzero_amd.scs_positions import all_openings, expand_openings
    e = ScsSelfPlay(ScsGameConfig(MIRRORED), a1_search(1), 1, training=False)
    for plies, count in ((1, 10), (2, 55), (3, 550)):
        got = all_openings(e, plies)
        want = enumerate_openings(MIRRORED, plies)         # the sequences, their order, the kept representatives
        assert got.dtype == np.int32 and got.shape == (count, plies) and [tuple(s) for s in got.tolist()] == want
    raw = all_openings(e, 2, distinct=False)
    assert [tuple(s) for s in raw.tolist()] == enumerate_openings(MIRRORED, 2, distinct=False) and len(raw) == 100
    assert all_openings(e, 0).shape == (1, 0)
    # the keys are the digests of the oracle's planes
    counts, children, keys = expand_openings(e, np.zeros((1, 0), np.int32))
    assert counts.tolist() == [10] and len(children) == 10
    for (a,), key in zip(children.tolist(), keys):
        g = apply_prefix(oracle_game(MIRRORED), [a])
        assert key.tolist() == image_mix_digest(g.state_image()[0]).tolist()
    with pytest.raises(ValueError, match="550 openings of 3 plies"):
        all_openings(e, 3, limit=100)
    first = int(children[0][0])                            # a frontier that is not a legal sequence is refused
    legal = set(legal_actions(apply_prefix(oracle_game(MIRRORED), [first])).tolist())
    illegal = next(a for a in range(e.cfg.num_actions) if a not in legal)
    with pytest.raises(NzError, match=rf"prefix 1, ply 1: action {illegal}: the action is not legal"):
        expand_openings(e, np.array([[first, first], [first, illegal]], np.int32))
    e.close()
    e = ScsSelfPlay(ScsGameConfig(TWO_TYPES), a1_search(1), 1, training=False)
    got = all_openings(e, 3)
    assert [tuple(s) for s in got.tolist()] == enumerate_openings(TWO_TYPES, 3) and len(got) == 18
    e.close()
    # per-game maps: one frontier belongs to one map
    e = ScsSelfPlay(ScsGameConfig(RANDOMIZED, per_game=True), a1_search(1), 2, training=False)
    e.set_games([7500, 7501])
    with pytest.raises(NzError, match="per-game maps") as err:
        all_openings(e, 1)
    assert err.value.code == NZ_ERR_STATE
    e.close()


# ---- 4. ScsMatch from mixed openings equals the oracle ---------------------------------------------------------------------------
def test_matches_from_mixed_openings_equal_the_oracle(mixed_round, nets):
    x, (s1, s2) = mixed_round, nets["search"]
    r, (rec1, rec2) = x["r"], x["recs"]
    assert r["unfinished"] == 0 and r["finished"].all() and r["matches"] == N
    outs = run_jobs(replay_match_from, [(MIRRORED, x["prefixes"][g], s1, s2, rec1[g], rec2[g]) for g in range(N)])
    _check_replays(r, outs, range(N), x["prefixes"], "mixed openings")           # every match, none left out
    out = r["outcomes"]
    assert (r["p1_wins"], r["p2_wins"], r["draws"]) == (int((out == 1).sum()), int((out == -1).sum()), int((out == 0).sum()))
    assert np.array_equal(*x["status"]) and np.array_equal(x["status"][0][:, 6], r["lengths"])
    e1, e2 = x["exports"]                                  # both engines' own records are the match record
    T = r["actions"].shape[1]
    assert np.array_equal(e1["actions"][:, :T], r["actions"]) and np.array_equal(e2["actions"][:, :T], r["actions"])
    for g, p in enumerate(x["prefixes"]):                  # the opening's plies were searched by nobody
        assert (e1["n_children"][g, :len(p)] == 0).all() and (e1["n_children"][g, len(p):int(r["lengths"][g])] > 0).all()


def test_wave_by_wave_route_and_the_null_cases(mixed_round, nets):
    x, (net1, net2) = mixed_round, nets["nets"]
    m = x["m"]
    for a in m.agents:
        a.persistent(0)
    rw = m.play(net1, net2, start_actions=x["start"], n_plies=x["n_plies"])
    assert m.agents[0].persistent() is False and m.agents[1].persistent() is False
    for a in m.agents:
        a.persistent(-1)
    _same_round(x["r"], rw, "wave by wave")
    assert np.array_equal(m.agents[0].status(), m.agents[1].status())
    # no openings, and openings of no plies, are the plain round
    _same_round(x["plain"], m.play(net1, net2, start_actions=None), "start_actions=None")
    _same_round(x["plain"], m.play(net1, net2, start_actions=x["start"], n_plies=np.zeros(N, np.int32)), "all-zero n_plies")
    # max_moves counts the round's own decisions, not the opening's plies
    part = m.play(net1, net2, start_actions=x["start"], n_plies=x["n_plies"], max_moves=3)
    assert part["lengths"].tolist() == [k + 3 for k in MIXED_PLIES] and part["unfinished"] == N
    assert all(np.array_equal(part["actions"][g, :k + 3], x["r"]["actions"][g, :k + 3]) for g, k in enumerate(MIXED_PLIES))


# ---- 5. ScsAgentMatch from openings ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pairing", ["mcts_vs_random", "random_vs_mcts", "policy_vs_random"])
def test_agent_matches_from_openings_equal_the_reference(pairing, nets):
    from nuzero_amd.tester import ScsAgentMatch
    net, search = nets["nets"][0], a1_search(SIMS1)
    agent_seeds = list(range(640, 640 + N))
    prefixes = _mixed_prefixes(MIRRORED, MIXED_PLIES, 900)
    start, n_plies = _pack(prefixes)
    kinds = {"mcts_vs_random": ("mcts", "random"), "random_vs_mcts": ("random", "mcts"), "policy_vs_random": ("policy", "random")}[pairing]
    spec = {"mcts": ("mcts", search), "policy": ("policy",), "random": ("random",)}
    m = ScsAgentMatch(nets["cfg"], spec[kinds[0]], spec[kinds[1]], N)
    if "mcts" in kinds:
        m.engine.persistent(1)
        m.engine.record(range(N), SIMS1 * (m.engine.MAX_MOVES + 1))
    else:
        m.record(0, range(N), m.engine.MAX_MOVES)
    r = m.play(*[net if k != "random" else None for k in kinds], agent_seeds=agent_seeds, start_actions=start, n_plies=n_plies)
    assert r["unfinished"] == 0 and r["finished"].all()
    recs = m.engine.records() if "mcts" in kinds else m.records(0)
    ref = {"mcts": lambda g: ("mcts", search, recs[g]), "policy": lambda g: ("policy", recs[g]), "random": lambda g: ("random", agent_seeds[g])}
    outs = run_jobs(replay_agent_match_from, [(MIRRORED, prefixes[g], ref[kinds[0]](g), ref[kinds[1]](g)) for g in range(N)])
    for g, out in enumerate(outs):
        n, k = int(r["lengths"][g]), len(prefixes[g])
        assert out["actions"] == r["actions"][g, :n].tolist() and (r["actions"][g, n:] == -1).all(), (pairing, g)
        assert out["length"] == n and out["terminal_value"] == r["outcomes"][g], (pairing, g)
        movers = np.array(out["movers"])                   # of the match's own decisions, k .. n
        for i, side in enumerate(out["sides"]):
            assert side["lookups"] == side["recorded"] and side["unused"] == [], (pairing, g, i)
            if kinds[i] == "mcts":
                continue
            mine = movers == i
            dev_a, dev_n = r["agent_actions"][i][g], r["agent_n_legal"][i][g]
            assert (dev_a[:k] == -1).all() and (dev_n[:k] == 0).all(), (pairing, g, i)      # nobody's decisions: the opening
            assert np.array_equal(dev_a[k:n][mine], side["agent_actions"]), (pairing, g, i)
            assert np.array_equal(dev_n[k:n][mine], side["n_legal"]), (pairing, g, i)        # a fresh stream after the opening
            assert (dev_a[k:n][~mine] == -1).all() and (dev_a[n:] == -1).all(), (pairing, g, i)
    assert len({r["actions"][g].tobytes() for g in range(N)}) >= 2
    m.close()


# ---- 6. per-game maps -----------------------------------------------------------------------------------------------------------
def test_matches_from_drawn_openings_on_per_game_maps():
    from nuzero_amd.scs import ScsGameConfig
    from nuzero_amd.scs_positions import random_openings
    from nuzero_amd.tester import ScsMatch
    G, sample = 16, [0, 5, 10, 15]
    cfg = ScsGameConfig(RANDOMIZED, per_game=True)
    net1, _ = _net(cfg, "convnet", 32, 2, seed=811, gain=2.0, max_batch=G)
    net2, _ = _net(cfg, "resnet", 32, 2, seed=822, gain=2.0, max_batch=G)
    s1, s2 = a1_search(SIMS1), a1_search(SIMS2)
    m = ScsMatch(cfg, s1, s2, G)
    map_seeds, opening_seeds = list(range(7600, 7600 + G)), list(range(20, 20 + G))
    m.agents[0].set_games(map_seeds)
    start, n_plies = random_openings(m.agents[0], opening_seeds, 3)               # every match's opening on its OWN map
    prefixes = [draw_prefix(RANDOMIZED, opening_seeds[g], 3, map_seeds[g]) for g in range(G)]
    assert start.tolist() == prefixes and n_plies.tolist() == [3] * G
    _record_all(m, sample)
    r = m.play(net1, net2, seeds=map_seeds, start_actions=start, n_plies=n_plies)
    assert r["unfinished"] == 0 and np.array_equal(m.agents[0].status(), m.agents[1].status())
    rec1, rec2 = m.agents[0].records(), m.agents[1].records()
    t, v = m.agents[0].game_maps
    outs = run_jobs(replay_match_from, [(RANDOMIZED, prefixes[g], s1, s2, rec1[g], rec2[g], map_seeds[g], (t[g], v[g])) for g in sample])
    _check_replays(r, outs, sample, prefixes, "per-game maps")                    # (oracle_game holds the map to the seed)
    _stop_recording(m)
    m.close(); net1.close(); net2.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engines_as_after_a_reset(mixed_round, nets):
    import torch
    from nuzero_amd import _lib
    from nuzero_amd._lib import NZ_ERR_ARG, NzError, lib
    x, (net1, net2) = mixed_round, nets["nets"]
    m = x["m"]
    a1, a2 = m.agents
    A, M = nets["cfg"].num_actions, a1.MAX_MOVES
    a1.reset(); a2.reset()
    fresh = a1.status()
    stream = lambda: c_void_p(torch.cuda.current_stream().cuda_stream)

    def refused(call, pattern):
        with pytest.raises(NzError, match=pattern) as err:
            a1._check(call())
        assert err.value.code == NZ_ERR_ARG
        assert np.array_equal(a1.status(), fresh) and np.array_equal(a2.status(), fresh)
        assert (a1.export()["actions"] == -1).all()

    good = [draw_prefix(MIRRORED, 50 + g, 3) for g in range(N)]
    # an illegal action at ply 2 of match 3 (in range, but not a legal action of that position)
    g3 = apply_prefix(oracle_game(MIRRORED), good[3][:2])
    legal = set(legal_actions(g3).tolist())
    illegal = next(a for a in range(A) if a not in legal)
    bad = [list(p) for p in good]
    bad[3][2] = illegal
    start, n_plies = _pack(bad)
    with pytest.raises(NzError, match=rf"match 3, ply 2: action {illegal}: the action is not legal") as err:
        a1.reset_to(start, n_plies)
    assert err.value.code == NZ_ERR_ARG and np.array_equal(a1.status(), fresh) and (a1.export()["actions"] == -1).all()
    with pytest.raises(NzError, match=rf"match 3, ply 2: action {illegal}") as err:       # the same through a match: both engines
        m.play(net1, net2, start_actions=start, n_plies=n_plies)
    assert err.value.code == NZ_ERR_ARG
    assert np.array_equal(a1.status(), fresh) and np.array_equal(a2.status(), fresh)
    # what the Python surface refuses itself goes to the library raw: an action out of range, n_plies above max_plies
    out_of_range, _ = _pack(good)
    out_of_range[6, 1] = A
    o, keep = _raw_openings(out_of_range, n_plies, 3)
    refused(lambda: lib.nz_scs_search_reset_to(a1._h, byref(o), stream()), rf"match 6, ply 1: action {A} outside")
    refused(lambda: lib.nz_scs_match_play_from(a1._h, net1._h, a2._h, net2._h, byref(o), 0, stream()), rf"match 6, ply 1: action {A} outside")
    long_plies = n_plies.copy()
    long_plies[2] = 4
    o, keep = _raw_openings(_pack(good)[0], long_plies, 3)
    refused(lambda: lib.nz_scs_search_reset_to(a1._h, byref(o), stream()), r"match 2: an opening of 4 plies.*ply 3")
    o, keep = _raw_openings(np.zeros((N, 1), np.int32), None, M + 1)
    refused(lambda: lib.nz_scs_search_reset_to(a1._h, byref(o), stream()), rf"openings of {M + 1} plies")
    with pytest.raises(ValueError, match="match 6, ply 1"):                                # and the Python surface's own refusal
        a1.reset_to(out_of_range, n_plies)
    # a prefix that runs past the end of a game: a whole reference-played random game plus one action
    whole = random_game(MIRRORED, 5)
    past = [list(p) for p in good]
    past[7] = whole + [0]
    start, n_plies = _pack(past)
    with pytest.raises(NzError, match=rf"match 7, ply {len(whole)}: action 0: the game was over before the prefix ended") as err:
        a1.reset_to(start, n_plies)
    assert err.value.code == NZ_ERR_ARG and np.array_equal(a1.status(), fresh) and (a1.export()["actions"] == -1).all()
    # the whole game itself is a sound opening: the match is over where it starts
    past[7] = whole
    start, n_plies = _pack(past)
    a1.reset_to(start, n_plies)
    assert a1.status()[7].tolist() == status_row(apply_prefix(oracle_game(MIRRORED), whole))
    # and a plain round afterwards is the fixture's
    _same_round(x["plain"], m.play(net1, net2), "a plain round after the refusals")


# ---- 8. test_from_openings on the 55 two-ply positions of mirrored_5x5 -----------------------------------------------------------
def test_tester_plays_every_two_ply_position_with_both_colours(nets):
    from nuzero_amd.scs_positions import agent_results
    from nuzero_amd.tester import ScsMatch, ScsTester
    (net1, net2), (s1, s2) = nets["nets"], nets["search"]
    want = enumerate_openings(MIRRORED, 2)
    assert len(want) == 55
    sample = [0, 7, 15, 23, 31, 39, 47, 54]
    t = ScsTester(nets["cfg"])
    exchanged, plain = t._match_of(s2, s1, 55), t._match_of(s1, s2, 55)           # built here so that their evaluations are recorded
    for m, sims in ((plain, (SIMS1, SIMS2)), (exchanged, (SIMS2, SIMS1))):
        for a, n in zip(m.agents, sims):
            a.persistent(1)
            a.record(sample, n * (a.MAX_MOVES + 1))
    tally = t.test_from_openings(s1, net1, s2, net2, plies=2)
    assert t._match[1] is exchanged and t._exchanged[1] is plain                  # the two rounds ran on these engines
    r1, r2 = t.opening_rounds
    start, n_plies = t.openings
    assert [tuple(s) for s in start.tolist()] == want and n_plies is None
    for r in (r1, r2):
        assert r["matches"] == 55 and r["unfinished"] == 0 and r["finished"].all()
        assert np.array_equal(r["actions"][:, :2], start)
    # the per-agent tally is the recount from the two rounds' outcomes: +1 is player index 0's win, the side agent 2 of a
    # round moves for -- s2's agent in round 1, s1's agent in the exchanged round
    o1, o2 = r1["outcomes"], r2["outcomes"]
    assert tally == {"agent1_wins": int((o1 == -1).sum() + (o2 == 1).sum()), "agent2_wins": int((o1 == 1).sum() + (o2 == -1).sum()),
                     "draws": int((o1 == 0).sum() + (o2 == 0).sum()), "unfinished": 0, "matches": 110}
    assert tally["agent1_wins"] == r1["p2_wins"] + r2["p1_wins"] and tally["agent2_wins"] == r1["p1_wins"] + r2["p2_wins"]
    both = {k: agent_results(o1, False)[k] + agent_results(o2, True)[k] for k in tally}
    assert both == tally
    # the point of the feature: the matches of a round are not copies of one game
    for r in (r1, r2):
        assert len({r["actions"][g, 2:].tobytes() for g in range(55)}) >= 2
    # eight matches of each round on the oracle
    for m, r, (sa, sb), label in ((plain, r1, (s1, s2), "round 1"), (exchanged, r2, (s2, s1), "exchanged round")):
        ra, rb = m.agents[0].records(), m.agents[1].records()
        outs = run_jobs(replay_match_from, [(MIRRORED, list(want[g]), sa, sb, ra[g], rb[g]) for g in sample])
        _check_replays(r, outs, sample, want, label)
        _stop_recording(m)
    # the exchanged round is the round of an ScsMatch built with the agents exchanged
    other = ScsMatch(nets["cfg"], s2, s1, 55)
    _same_round(r2, other.play(net2, net1, start_actions=start), "an ScsMatch with the agents exchanged")
    other.close()
    # caller's openings and one round only
    one = t.test_from_openings(s1, net1, s2, net2, openings=start, both_colours=False)
    assert one == agent_results(o1, False) and len(t.opening_rounds) == 1
    _same_round(r1, t.opening_rounds[0], "the caller's openings")
    t.close()
