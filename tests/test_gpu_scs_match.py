"""SCS evaluation matches played inside the library (nz_scs_match_play, nuzero_amd.tester.ScsMatch): two MCTS agents,
each with its own search config, board net and trees, many matches at once, the whole move loop on the device.

Exactness: every match is replayed on the CPU oracle (oracle/agents.py play_match, Tester.py:62-118) by
tests/match_replay.py, which feeds each oracle agent the evaluations the corresponding DEVICE agent recorded
(nz_scs_search_record on the persistent route) and never computes one itself -- actions, length and outcome must
equal the device's, every recorded evaluation must be asked for, none may be missing.  The recorded evaluations
themselves are held to oracle/net.py within 1e-5 (BASELINE.json's north_star, as tests/test_gpu_scs_persist.py).
The wave-by-wave route, per-game maps, the inference cache and a mixed round are compared with that.  Needs a GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
pytestmark = pytest.mark.gpu
CONFIGS = os.path.join(HERE, "golden", "scs_configs")
MIRRORED = os.path.join(CONFIGS, "mirrored_5x5.yml")
RANDOMIZED = os.path.join(CONFIGS, "randomized_5x5.yml")
LATE = os.path.join(CONFIGS, "late_reinforcements_5x5.yml")

from test_gpu_scs_configs import a1_search, _net          # noqa: E402

SIMS1, SIMS2 = 48, 24
N = 12


def _in_step(m):
    """The two engines hold the same games (check 6 of the issue: after every round)."""
    s1, s2 = m.agents[0].status(), m.agents[1].status()
    assert np.array_equal(s1, s2)
    return s1


def _same_round(ra, rb, label):
    assert np.array_equal(ra["lengths"], rb["lengths"]) and np.array_equal(ra["outcomes"], rb["outcomes"]), label
    assert ra["actions"].shape == rb["actions"].shape and np.array_equal(ra["actions"], rb["actions"]), label
    for k in ("matches", "p1_wins", "p2_wins", "draws", "unfinished", "length_sum", "length_max"):
        assert ra[k] == rb[k], (label, k)


def _tally_is_the_count(r, n):
    assert r["matches"] == n and len(r["outcomes"]) == n
    assert r["p1_wins"] + r["p2_wins"] + r["draws"] + r["unfinished"] == n
    assert r["length_sum"] == int(r["lengths"].sum()) and r["length_max"] == int(r["lengths"].max())


def _check_replays(r, outs, games, label):
    for g, out in zip(games, outs):
        n = int(r["lengths"][g])
        print(f"{label}: match {g}: {n} decisions, outcome {r['outcomes'][g]}, evaluations asked for {out['lookups']} "
              f"of {out['recorded']} recorded")
        assert out["actions"] == r["actions"][g, :n].tolist(), (label, g)
        assert (r["actions"][g, n:] == -1).all(), (label, g)
        assert out["length"] == n and out["terminal_value"] == r["outcomes"][g], (label, g)
        assert out["lookups"] == out["recorded"], (label, g, out["lookups"], out["recorded"])
        assert out["unused"] == ([], []), (label, g)


@pytest.fixture(scope="module")
def mirrored_round():
    """Check 1's round: ConvNet(32, 3) against ResNet(32, 2) on mirrored_5x5, 12 matches, persistent route, every
    evaluation of both agents recorded."""
    from nuzero_amd.scs import ScsGameConfig
    from nuzero_amd.tester import ScsMatch
    cfg = ScsGameConfig(MIRRORED)
    net1, w1 = _net(cfg, "convnet", 32, 3, seed=101, gain=2.0, max_batch=N)
    net2, w2 = _net(cfg, "resnet", 32, 2, seed=202, gain=2.0, max_batch=N)
    s1, s2 = a1_search(SIMS1), a1_search(SIMS2)
    m = ScsMatch(cfg, s1, s2, N)
    for a, sims in zip(m.agents, (SIMS1, SIMS2)):
        a.persistent(1)
        a.record(range(N), sims * (a.MAX_MOVES + 1))
    r = m.play(net1, net2)
    assert m.agents[0].persistent() and m.agents[1].persistent()
    st = _in_step(m)
    recs = (m.agents[0].records(), m.agents[1].records())
    for a in m.agents:
        a.record([], 0)
        a.persistent(-1)
    yield {"m": m, "nets": (net1, net2), "weights": (w1, w2), "search": (s1, s2), "r": r, "recs": recs, "status": st}
    m.close(); net1.close(); net2.close()


def test_matches_equal_the_oracle_on_the_agents_own_evaluations(mirrored_round):
    from match_replay import replay_matches
    from test_gpu_scs_persist import _oracle_net_on_leaves
    x = mirrored_round
    r, (rec1, rec2), (s1, s2) = x["r"], x["recs"], x["search"]
    assert r["unfinished"] == 0 and (x["status"][:, 4] == 1).all()
    assert np.array_equal(x["status"][:, 6], r["lengths"]) and np.array_equal(x["status"][:, 5], r["outcomes"])
    outs = replay_matches([(MIRRORED, s1, s2, rec1[g], rec2[g]) for g in range(N)])
    _check_replays(r, outs, range(N), "mirrored")          # every match, none left out
    _tally_is_the_count(r, N)
    assert r["p1_wins"] == int((r["outcomes"] == 1).sum()) and r["p2_wins"] == int((r["outcomes"] == -1).sum())
    assert r["draws"] == int((r["outcomes"] == 0).sum())
    # each agent's record against ITS network on root positions along the match
    for recs, w, arch, depth in ((rec1, x["weights"][0], "convnet", 3), (rec2, x["weights"][1], "resnet", 2)):
        for g in (0, N - 1):
            _oracle_net_on_leaves(MIRRORED, w, arch, depth, False, r, g, recs, 12)


def test_wave_by_wave_route_plays_the_same_matches_and_a_mixed_round_runs(mirrored_round):
    from nuzero_amd.scs import ScsGameConfig
    x = mirrored_round
    m, (net1, net2) = x["m"], x["nets"]
    for a in m.agents:
        a.persistent(0)
    rw = m.play(net1, net2)
    assert m.agents[0].persistent() is False and m.agents[1].persistent() is False
    _in_step(m)
    _same_round(x["r"], rw, "wave by wave")
    # agent 1 persistent, agent 2 a RecurrentNet (no per-wavefront form): to the end, each on its own route
    for a in m.agents:
        a.persistent(-1)
    net_r, _ = _net(ScsGameConfig(MIRRORED), "recurrent", 32, 1, seed=303, gain=1.0, iters=2, max_batch=N)
    rm = m.play(net1, net_r)
    assert m.agents[0].persistent() is True and m.agents[1].persistent() is False
    st = _in_step(m)
    assert rm["unfinished"] == 0 and (st[:, 4] == 1).all()
    _tally_is_the_count(rm, N)
    net_r.close()


def test_matches_on_per_game_maps():
    from match_replay import replay_matches
    from nuzero_amd._lib import NzError
    from nuzero_amd.scs import ScsGameConfig
    from nuzero_amd.tester import ScsMatch
    G, base = 256, 7000
    cfg = ScsGameConfig(RANDOMIZED, per_game=True)
    net1, _ = _net(cfg, "convnet", 32, 3, seed=111, gain=2.0, max_batch=G)
    net2, _ = _net(cfg, "resnet", 32, 2, seed=222, gain=2.0, max_batch=G)
    s1, s2 = a1_search(SIMS1), a1_search(SIMS2)
    m = ScsMatch(cfg, s1, s2, G)
    sample = [0, 85, 170, 255]
    seeds = list(range(base, base + G))
    for a, sims in zip(m.agents, (SIMS1, SIMS2)):
        a.persistent(1)
        a.record(sample, sims * (a.MAX_MOVES + 1))
    r = m.play(net1, net2, seeds=seeds)
    _in_step(m)
    assert r["unfinished"] == 0
    assert len({r["actions"][g].tobytes() for g in range(G)}) >= 2, "the maps are not reaching the matches"
    _tally_is_the_count(r, G)
    out = r["outcomes"]
    assert (r["p1_wins"], r["p2_wins"], r["draws"]) == (int((out == 1).sum()), int((out == -1).sum()), int((out == 0).sum()))
    rec1, rec2 = m.agents[0].records(), m.agents[1].records()
    t, v = m.agents[0].game_maps
    t2, v2 = m.agents[1].game_maps
    assert np.array_equal(t, t2) and np.array_equal(v, v2)
    outs = replay_matches([(RANDOMIZED, s1, s2, rec1[g], rec2[g], seeds[g], (t[g], v[g])) for g in sample])
    _check_replays(r, outs, sample, "per-game maps")
    # a pair of engines that do not hold the same maps is refused
    for a in m.agents:
        a.record([], 0)
    m.agents[1].set_games([s + 1 for s in seeds])
    from ctypes import c_void_p
    import torch
    from nuzero_amd._lib import lib
    a1, a2 = m.agents
    with pytest.raises(NzError, match="different maps"):
        a1._check(lib.nz_scs_match_play(a1._h, net1._h, a2._h, net2._h, 0, c_void_p(torch.cuda.current_stream().cuda_stream)))
    m.close(); net1.close(); net2.close()


def test_hand_over_with_mixed_movers_stops_both_engines_at_the_same_decision():
    from nuzero_amd.scs import ScsGameConfig
    from nuzero_amd.tester import ScsMatch
    G = 6
    cfg = ScsGameConfig(LATE)
    net1, _ = _net(cfg, "convnet", 32, 3, seed=121, gain=2.0, max_batch=G)
    net2, _ = _net(cfg, "resnet", 32, 2, seed=232, gain=2.0, max_batch=G)
    m = ScsMatch(cfg, a1_search(SIMS1), a1_search(SIMS2), G)
    full = m.play(net1, net2)
    st_full = _in_step(m)
    assert full["unfinished"] == 0 and (st_full[:, 4] == 1).all()
    part = m.play(net1, net2, max_moves=7)
    st = _in_step(m)                                        # both engines at the same decision
    assert (st[:, 6] == 7).all() and (part["lengths"] == 7).all()
    assert part["unfinished"] == int((st[:, 4] == 0).sum()) == G
    assert part["p1_wins"] == part["p2_wins"] == part["draws"] == 0
    assert part["actions"].shape == (G, 7) and np.array_equal(part["actions"], full["actions"][:, :7])
    # the phases of this config make one player decide several times in a row: the mover is not simply alternating,
    # and both engines recorded the very actions of the match record
    e1, e2 = m.agents[0].export(), m.agents[1].export()
    assert np.array_equal(e1["actions"][:, :7], part["actions"]) and np.array_equal(e2["actions"][:, :7], part["actions"])
    from oracle.scs import ScsConfig, ScsGame
    og, movers = ScsGame(ScsConfig(LATE)), []
    for a in full["actions"][0, :int(full["lengths"][0])]:
        movers.append(og.get_current_player())
        og.step_index(int(a))
    assert og.is_terminal() and og.terminal_value == full["outcomes"][0]
    assert any(movers[i] == movers[i + 1] for i in range(6)), movers[:7]
    m.close(); net1.close(); net2.close()


def test_inference_caches_are_results_neutral_and_stay_per_agent(mirrored_round):
    x = mirrored_round
    m, (net1, net2) = x["m"], x["nets"]
    a1, a2 = m.agents
    a1.cache(64)
    a2.cache(64)
    rc = m.play(net1, net2)
    _in_step(m)
    _same_round(x["r"], rc, "cache on both")
    c1, c2 = a1.cache_stats(), a2.cache_stats()
    assert c1["size"] == c2["size"] == 64 and c1["hits"] > 0 and c2["hits"] > 0
    assert 0 < c1["entries"] <= 64 and 0 < c2["entries"] <= 64
    # agent 1 alone: agent 2 has no table, so nothing agent 1 stores can reach it
    a1.cache(64)
    a2.cache(0)
    before = a2.cache_stats()
    r1 = m.play(net1, net2)
    _in_step(m)
    _same_round(x["r"], r1, "cache on agent 1 only")
    c1, c2 = a1.cache_stats(), a2.cache_stats()
    assert c1["hits"] > 0 and 0 < c1["entries"] <= 64
    assert c2["entries"] == 0 and c2["size"] == 0 and c2["hits"] == before["hits"] and c2["misses"] == before["misses"]
    a1.cache(0)


def test_tester_wrapper_counts_wins(mirrored_round):
    from nuzero_amd.tester import ScsTester
    x = mirrored_round
    t = ScsTester(MIRRORED)
    got = t.Test_using_agents(x["search"][0], x["nets"][0], x["search"][1], x["nets"][1], N)
    assert got == (x["r"]["p1_wins"], x["r"]["p2_wins"], x["r"]["draws"]) and sum(got) == N
    t._match[1].close()
