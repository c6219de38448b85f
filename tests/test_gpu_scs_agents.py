"""SCS evaluation matches against scripted agents, played inside the library (nz_scs_agent_match_play,
nuzero_amd.tester.ScsAgentMatch): the bare policy, a random mover and at most one MCTS agent on ONE engine.

Exactness: every match is replayed on the CPU oracle (oracle/agents.py play_match) with tests/agents_ref.py's
restatements of the two scripted agents; the oracle's MCTS and policy agents are fed the evaluations the DEVICE agents
recorded (nz_scs_search_record on the persistent route, nz_scs_agent_record) and never compute one themselves, so
every action, length and outcome must equal the device's, every recorded evaluation must be asked for and none may be
missing.  The policy agent's recorded rows are held to BoardNet.forward on the oracle's own state images within 1e-5,
the project's network tolerance (BASELINE.json's north_star).  Needs a GPU."""
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

from test_gpu_scs_configs import a1_search, _net          # noqa: E402

N, SIMS = 8, 16
MAP_SEEDS = list(range(9100, 9100 + N))
AGENT_SEEDS = list(range(500, 500 + N))


def _convnet(cfg, seed, zero_policy=False):
    """ConvNet(32 filters, 2 layers), fixed-seed weights."""
    net, w = _net(cfg, "convnet", 32, 2, seed=seed, gain=2.0, max_batch=N)
    if zero_policy:                                           # all logits equal: every probability is the same float
        w["policy_head.layers.2.weight"][:] = 0.0
        net.set_weights(w, 1)
    return net, w


def _check_replays(r, outs, label):
    assert len(outs) == N                                     # every match, none left out
    for g, out in enumerate(outs):
        n = int(r["lengths"][g])
        print(f"{label}: match {g}: {n} decisions, outcome {r['outcomes'][g]}, evaluations asked for "
              f"{[s['lookups'] for s in out['sides']]} of {[s['recorded'] for s in out['sides']]} recorded")
        assert out["actions"] == r["actions"][g, :n].tolist(), (label, g)
        assert (r["actions"][g, n:] == -1).all(), (label, g)
        assert out["length"] == n and out["terminal_value"] == r["outcomes"][g], (label, g)
        movers = np.array(out["movers"])
        for i, side in enumerate(out["sides"]):
            assert side["lookups"] == side["recorded"] and side["unused"] == [], (label, g, i)
            if r["agent_actions"][i] is None:                 # the MCTS side
                continue
            mine = movers == i                                # the decisions this scripted side took
            dev_a, dev_n = r["agent_actions"][i][g], r["agent_n_legal"][i][g]
            assert np.array_equal(dev_a[:n][mine], side["agent_actions"]), (label, g, i)
            assert np.array_equal(dev_a[:n][mine], r["actions"][g, :n][mine]), (label, g, i)
            assert np.array_equal(dev_n[:n][mine], side["n_legal"]), (label, g, i)
            assert (dev_a[:n][~mine] == -1).all() and (dev_a[n:] == -1).all() and (dev_n[:n][~mine] == 0).all(), (label, g, i)
            if "probs" in side:
                assert np.array_equal(r["agent_probs"][i][g][:n][mine], np.array(side["probs"], np.float32)), (label, g, i)


def _tally_is_the_count(r):
    assert r["matches"] == N and r["p1_wins"] + r["p2_wins"] + r["draws"] + r["unfinished"] == N
    out = r["outcomes"]
    done = r["unfinished"] == 0
    if done:
        assert (r["p1_wins"], r["p2_wins"], r["draws"]) == (int((out == 1).sum()), int((out == -1).sum()), int((out == 0).sum()))
    assert r["length_sum"] == int(r["lengths"].sum()) and r["length_max"] == int(r["lengths"].max())


def _same_round(ra, rb, label):
    for k in ("actions", "lengths", "outcomes"):
        assert np.array_equal(ra[k], rb[k]), (label, k)
    for k in ("matches", "p1_wins", "p2_wins", "draws", "unfinished", "length_sum", "length_max"):
        assert ra[k] == rb[k], (label, k)
    for i in range(2):
        for k in ("agent_actions", "agent_n_legal"):
            assert (ra[k][i] is None) == (rb[k][i] is None) and (ra[k][i] is None or np.array_equal(ra[k][i], rb[k][i])), (label, k, i)


@pytest.fixture(scope="module", params=[1, 2], ids=["mcts_is_player_1", "mcts_is_player_2"])
def mcts_vs_random(request):
    """(a)'s rounds: MCTS (16 simulations) against a random mover on per-game maps, persistent route, every
    evaluation of the MCTS agent recorded."""
    from nuzero_amd.scs import ScsGameConfig
    from nuzero_amd.tester import ScsAgentMatch
    side = request.param
    cfg = ScsGameConfig(RANDOMIZED, per_game=True)
    net, _ = _convnet(cfg, 31)
    search = a1_search(SIMS)
    specs = (("mcts", search), ("random",)) if side == 1 else (("random",), ("mcts", search))
    nets = (net, None) if side == 1 else (None, net)
    m = ScsAgentMatch(cfg, specs[0], specs[1], N)
    m.engine.persistent(1)
    m.engine.record(range(N), SIMS * (m.engine.MAX_MOVES + 1))
    r = m.play(nets[0], nets[1], seeds=MAP_SEEDS, agent_seeds=AGENT_SEEDS)
    assert m.engine.persistent()
    recs = m.engine.records()
    m.engine.record([], 0)
    m.engine.persistent(-1)
    yield {"m": m, "nets": nets, "side": side, "search": search, "r": r, "recs": recs, "maps": m.engine.game_maps}
    m.close(); net.close()


def test_mcts_against_random_equals_the_oracle(mcts_vs_random):
    from agents_ref import replay_agent_matches
    x = mcts_vs_random
    r, t, v = x["r"], *x["maps"]
    assert r["unfinished"] == 0
    _tally_is_the_count(r)
    jobs = []
    for g in range(N):
        mcts, rnd = ("mcts", x["search"], x["recs"][g]), ("random", AGENT_SEEDS[g])
        jobs.append((RANDOMIZED,) + ((mcts, rnd) if x["side"] == 1 else (rnd, mcts)) + (MAP_SEEDS[g], (t[g], v[g])))
    _check_replays(r, replay_agent_matches(jobs), f"MCTS as player {x['side']} against random")
    assert len({r["actions"][g].tobytes() for g in range(N)}) >= 2, "maps and streams are not reaching the matches"
    # the engine's own record is the match record
    e = x["m"].engine.export()
    assert np.array_equal(e["actions"][:, :r["actions"].shape[1]], r["actions"])


def test_wave_by_wave_route_plays_the_same_matches(mcts_vs_random):
    x = mcts_vs_random
    m = x["m"]
    m.engine.persistent(0)
    rw = m.play(x["nets"][0], x["nets"][1], seeds=MAP_SEEDS, agent_seeds=AGENT_SEEDS)
    assert m.engine.persistent() is False
    m.engine.persistent(-1)
    _same_round(x["r"], rw, "wave by wave")


def test_policy_against_random_runs_no_simulation_and_equals_the_oracle():
    import torch
    from agents_ref import replay_agent_matches
    from nuzero_amd.scs import ScsGameConfig
    from nuzero_amd.tester import ScsAgentMatch
    cfg = ScsGameConfig(RANDOMIZED, per_game=True)
    net, _ = _convnet(cfg, 41)
    m = ScsAgentMatch(cfg, ("policy",), ("random",), N)
    m.record(0, range(N), m.engine.MAX_MOVES)
    r = m.play(net, None, seeds=MAP_SEEDS, agent_seeds=AGENT_SEEDS)
    assert r["unfinished"] == 0 and (m.engine.status()[:, 4] == 1).all()       # full games
    _tally_is_the_count(r)
    e = m.engine.export()
    assert e["simulations"] == 0 and e["expansions"] == 0                    # no search ran at all
    assert np.array_equal(e["actions"][:, :r["actions"].shape[1]], r["actions"])
    recs = m.records(0)
    t, v = m.engine.game_maps
    outs = replay_agent_matches([(RANDOMIZED, ("policy", recs[g]), ("random", AGENT_SEEDS[g]), MAP_SEEDS[g], (t[g], v[g]))
                                 for g in range(N)], workers=1)
    _check_replays(r, outs, "policy against random")
    assert len({r["actions"][g].tobytes() for g in range(N)}) >= 2
    # independently: each recorded row is the network on the ORACLE position's state image
    worst_p = worst_v = 0.0
    for g, out in enumerate(outs):
        imgs = np.stack(out["sides"][0]["images"])
        dig, probs, values = recs[g]
        assert len(imgs) == len(probs) > 0
        for i in range(0, len(imgs), N):                                      # (the net holds N positions)
            p, val = net.forward(torch.from_numpy(np.ascontiguousarray(imgs[i:i + N])).cuda())
            worst_p = max(worst_p, float(np.abs(p.cpu().numpy() - probs[i:i + N]).max()))
            worst_v = max(worst_v, float(np.abs(val.cpu().numpy() - values[i:i + N]).max()))
    print(f"policy rows against BoardNet.forward on the oracle's images: probs {worst_p:.3g}, value {worst_v:.3g}")
    assert worst_p < 1e-5 and worst_v < 1e-5, (worst_p, worst_v)
    m.close(); net.close()


def test_policy_against_policy_on_one_shared_net_equals_the_oracle():
    """Both sides are the bare policy of ONE network object, whose input rows hold one side's positions at a time: on
    per-game maps the movers of one decision differ from match to match, so both sides evaluate in the same decision.
    Every recorded row is the network on the oracle's own position, and a round with two network objects of the same
    weights plays the same matches."""
    import torch
    from agents_ref import replay_agent_matches
    from nuzero_amd.scs import ScsGameConfig
    from nuzero_amd.tester import ScsAgentMatch
    cfg = ScsGameConfig(RANDOMIZED, per_game=True)
    net, _ = _convnet(cfg, 91)
    twin, _ = _convnet(cfg, 91)
    m = ScsAgentMatch(cfg, ("policy",), ("policy",), N)
    for side in (0, 1):
        m.record(side, range(N), m.engine.MAX_MOVES)
    r = m.play(net, net, seeds=MAP_SEEDS)
    assert r["unfinished"] == 0 and m.engine.export()["simulations"] == 0
    _tally_is_the_count(r)
    recs = [m.records(0), m.records(1)]
    t, v = m.engine.game_maps
    outs = replay_agent_matches([(RANDOMIZED, ("policy", recs[0][g]), ("policy", recs[1][g]), MAP_SEEDS[g], (t[g], v[g]))
                                 for g in range(N)], workers=1)
    _check_replays(r, outs, "policy against policy, one net")
    T = int(r["lengths"].min())
    movers = np.array([out["movers"][:T] for out in outs])
    assert (movers != movers[0]).any(), "every decision has one mover in all matches: the sides never share a decision"
    worst_p = worst_v = 0.0
    for g, out in enumerate(outs):
        for side in (0, 1):
            imgs = np.stack(out["sides"][side]["images"])
            _, probs, values = recs[side][g]
            assert len(imgs) == len(probs) > 0
            for i in range(0, len(imgs), N):                                  # (the net holds N positions)
                p, val = net.forward(torch.from_numpy(np.ascontiguousarray(imgs[i:i + N])).cuda())
                worst_p = max(worst_p, float(np.abs(p.cpu().numpy() - probs[i:i + N]).max()))
                worst_v = max(worst_v, float(np.abs(val.cpu().numpy() - values[i:i + N]).max()))
    print(f"shared net: policy rows against BoardNet.forward on the oracle's images: probs {worst_p:.3g}, value {worst_v:.3g}")
    assert worst_p < 1e-5 and worst_v < 1e-5, (worst_p, worst_v)
    _same_round(r, m.play(net, twin, seeds=MAP_SEEDS), "two network objects of the same weights")
    m.close(); net.close(); twin.close()


@pytest.mark.parametrize("mcts_side", [1, 2])
def test_mcts_against_policy_with_two_nets_equals_the_oracle(mcts_side):
    """(c): the oracle's MctsAgentRef follows the policy agent's move with update_subtree; its next search consumes the
    device engine's recorded evaluations in order, so a tree that differed after a forced move would miss a look-up."""
    from agents_ref import replay_agent_matches
    from nuzero_amd.scs import ScsGameConfig
    from nuzero_amd.tester import ScsAgentMatch
    cfg = ScsGameConfig(RANDOMIZED, per_game=True)
    net_m, _ = _convnet(cfg, 51)
    net_p, _ = _convnet(cfg, 62)
    search = a1_search(SIMS)
    specs = (("mcts", search), ("policy",)) if mcts_side == 1 else (("policy",), ("mcts", search))
    nets = (net_m, net_p) if mcts_side == 1 else (net_p, net_m)
    m = ScsAgentMatch(cfg, specs[0], specs[1], N)
    m.engine.persistent(1)
    m.engine.record(range(N), SIMS * (m.engine.MAX_MOVES + 1))
    m.record(2 - mcts_side, range(N), m.engine.MAX_MOVES)
    r = m.play(nets[0], nets[1], seeds=MAP_SEEDS)
    assert r["unfinished"] == 0
    _tally_is_the_count(r)
    rec_m, rec_p = m.engine.records(), m.records(2 - mcts_side)
    t, v = m.engine.game_maps
    jobs = []
    for g in range(N):
        a_m, a_p = ("mcts", search, rec_m[g]), ("policy", rec_p[g])
        jobs.append((RANDOMIZED,) + ((a_m, a_p) if mcts_side == 1 else (a_p, a_m)) + (MAP_SEEDS[g], (t[g], v[g])))
    _check_replays(r, replay_agent_matches(jobs), f"MCTS as player {mcts_side} against policy")
    m.close(); net_m.close(); net_p.close()


def test_a_tie_goes_to_the_lowest_legal_index():
    from nuzero_amd.scs import ScsGameConfig
    from nuzero_amd.tester import ScsAgentMatch
    from oracle.scs import ScsConfig, ScsGame
    cfg = ScsGameConfig(MIRRORED)
    net, _ = _convnet(cfg, 71, zero_policy=True)
    m = ScsAgentMatch(cfg, ("random",), ("policy",), N)
    m.record(1, range(N), m.engine.MAX_MOVES)
    r = m.play(None, net, agent_seeds=AGENT_SEEDS)
    assert r["unfinished"] == 0
    recs = m.records(1)
    decided = 0
    for g in range(N):
        probs = recs[g][1]
        assert len(probs) > 0 and (probs == probs[:, :1]).all()              # the tie is real: one float everywhere
        og = ScsGame(ScsConfig(MIRRORED))
        for i in range(int(r["lengths"][g])):
            a = int(r["actions"][g, i])
            if og.get_current_player() != 1:                                  # the policy agent (player index 0) decides
                legal = np.flatnonzero(np.asarray(og.possible_actions()).reshape(-1))
                assert a == legal[0] == r["agent_actions"][1][g, i], (g, i)
                assert r["agent_n_legal"][1][g, i] == len(legal)
                decided += 1
            og.step_index(a)
        assert og.is_terminal() and og.terminal_value == r["outcomes"][g]
    assert decided >= N
    m.close(); net.close()


def test_max_moves_stops_both_sides_and_a_second_round_is_the_same():
    from nuzero_amd.scs import ScsGameConfig
    from nuzero_amd.tester import ScsAgentMatch
    cfg = ScsGameConfig(RANDOMIZED, per_game=True)
    net, _ = _convnet(cfg, 81)
    m = ScsAgentMatch(cfg, ("mcts", a1_search(SIMS)), ("random",), N)
    full = m.play(net, None, seeds=MAP_SEEDS, agent_seeds=AGENT_SEEDS)
    assert full["unfinished"] == 0
    part = m.play(net, None, seeds=MAP_SEEDS, agent_seeds=AGENT_SEEDS, max_moves=7)
    st = m.engine.status()
    assert (st[:, 6] == 7).all() and (part["lengths"] == 7).all() and (st[:, 4] == 0).all()
    assert part["unfinished"] == N and part["p1_wins"] == part["p2_wins"] == part["draws"] == 0
    assert part["actions"].shape == (N, 7) and np.array_equal(part["actions"], full["actions"][:, :7])
    assert np.array_equal(part["agent_actions"][1], full["agent_actions"][1][:, :7])
    assert np.array_equal(part["agent_n_legal"][1], full["agent_n_legal"][1][:, :7])
    assert np.array_equal(m.engine.export()["actions"][:, :7], part["actions"])   # the engine stopped at the same decision
    again = m.play(net, None, seeds=MAP_SEEDS, agent_seeds=AGENT_SEEDS)          # the streams are rebuilt from the seeds
    _same_round(full, again, "second round")
    other = m.play(net, None, seeds=MAP_SEEDS, agent_seeds=[s + 1000 for s in AGENT_SEEDS])
    assert not np.array_equal(other["actions"], full["actions"])
    # the tester's wrapper counts the same wins through the same route
    from nuzero_amd.tester import ScsTester
    t = ScsTester(cfg)
    got = t.test_using_agents(("mcts", a1_search(SIMS)), net, ("random",), None, N, seeds=MAP_SEEDS, agent_seeds=AGENT_SEEDS)
    assert got == (full["p1_wins"], full["p2_wins"], full["draws"]) and sum(got) == N
    t._match[1].close()
    m.close(); net.close()
