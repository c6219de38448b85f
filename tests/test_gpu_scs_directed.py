"""Every device form of the SCS rules against the oracle on directed play (tests/scs_directed.py; the floors on what
the walks reach are tests/test_scs_directed_host.py's).

  (a) the one-lane `Scs` class (nz_scs_step / _legal_mask / _state_image / _status) in lock-step with the oracle;
  (b) the one-wavefront step, admission and image (scs_step_wave<true>, scs_admit_wave, scs_state_image_wave<false>)
      through the compact replay buffer, fed rounds built by hand from the oracle;
  (c) the one-wavefront legal set (wave_legal) through nz_scs_openings_expand at every depth of a walk;
  (d) the search's own forms (scs_step_wave<false>, scs_legal_mask_wave, the staged images) from positions deep in
      directed play, replayed on the oracle from the evaluations the device consumed.

Every comparison is exact: integer rules, images of small integers and exactly representable fractions.  Wall time on
an MI355X: 2.0 s for the longest case of (a), 0.6 s for (c) on directed_6x5, 1.1 s for (d), under 0.2 s for every other
case.  Needs a GPU."""
import os
import sys
from ctypes import c_void_p

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
pytestmark = pytest.mark.gpu

import scs_directed as sd                                          # noqa: E402
from test_gpu_scs_configs import a1_search                         # noqa: E402

FIXED_MAP_WALKS = sd.PINNED
SIMS = 16


def _ids(walks):
    return [w.label for w in walks]


def _device_config(walk):
    from nuzero_amd.scs import ScsGameConfig
    if walk.map_seeds is not None:
        return ScsGameConfig(sd.config_path(walk.name), per_game=True)
    return ScsGameConfig(sd.config_path(walk.name))


def _image_diff(got, want):
    """Where two state images differ, for an assertion's message: (channel, tile, device value, oracle value), the first few."""
    c, r, k = np.nonzero(got != want)
    return [(int(a), (int(b), int(d)), float(got[a, b, d]), float(want[a, b, d])) for a, b, d in list(zip(c, r, k))[:12]]


def _status(og):
    return (og.player, og.sub_phase, og.stage, og.turn, int(og.terminal), og.terminal_value, og.length)


# ---- (a) the one-lane form ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", FIXED_MAP_WALKS + [sd.PER_GAME], ids=_ids(FIXED_MAP_WALKS + [sd.PER_GAME]))
def test_one_lane_rules_equal_the_oracle_on_directed_play(walk):
    """ScsBatch plays the walk's games in lock-step with the oracle, the oracle's policy choosing: status tuple, legal
    mask and state image at every ply and in the position each game stops in.  At a dead end the device says "not
    terminal" with an all-zero mask, as the oracle does, and the game stops there."""
    from nuzero_amd.scs import ScsBatch
    games = walk.games()
    G = len(games)
    cfg = _device_config(walk)
    batch = ScsBatch(cfg, G)
    if walk.map_seeds is not None:
        terrain, vp = cfg.draw_games(list(walk.map_seeds))[:2]
        batch.set_maps(terrain, vp)
    oracle = [sd.new_game(walk.name, g.map_seed) for g in games]
    if walk.map_seeds is not None:
        for i, og in enumerate(oracle):                            # the device plays on the oracle's own maps
            assert np.array_equal(np.array(og.cfg.terrain, np.float32).reshape(-1, 3), terrain[i])
    compared = 0
    for m in range(max(len(g.actions) for g in games) + 1):
        st = batch.status().cpu().numpy()
        mask = batch.legal_mask().cpu().numpy()
        img = batch.state_image().cpu().numpy()
        actions = np.full(G, -1, np.int32)
        for i, (g, og) in enumerate(zip(games, oracle)):
            if m > len(g.actions):
                continue
            assert tuple(st[i]) == _status(og), (walk.label, i, m, tuple(st[i]), _status(og))
            assert np.array_equal(mask[i], og.possible_actions()), (walk.label, i, m)
            want = og.state_image()[0]
            assert np.array_equal(img[i], want), (walk.label, i, m, _image_diff(img[i], want))
            compared += 1
            if m < len(g.actions):
                actions[i] = g.actions[m]
                og.step_index(g.actions[m])
            elif g.dead_end:
                assert st[i][4] == 0 and not mask[i].any(), (walk.label, i, m)
            elif g.terminal:
                assert st[i][4] == 1 and st[i][5] == g.outcome and not mask[i].any(), (walk.label, i, m)
        if (actions >= 0).any():
            batch.step(actions)
    assert compared == sum(len(g.actions) + 1 for g in games)
    batch.close()


# ---- (b) wave step, admission and image through the compact replay buffer -----------------------------------------------
def _visits(n):
    return 1 + (7 * np.arange(n, dtype=np.int64)) % 5


def _hand_built_round(games, max_children):
    """What a search engine exports of a round, built from the oracle's walks: the child list of ply m is the legal
    set in ascending order with visits 1 + (7 j) % 5 (distinct across the 64-lane strides of a long list); every ply
    gets its own slot."""
    G, M = len(games), max(1, max(len(g.actions) for g in games))
    r = {"actions": np.zeros((G, M), np.int32), "lengths": np.array([len(g.actions) for g in games], np.int32),
         "outcomes": np.array([g.outcome if g.terminal else 0 for g in games], np.int32),
         "child_action": np.zeros((G, M, max_children), np.int32), "child_visit": np.zeros((G, M, max_children), np.int32),
         "n_children": np.zeros((G, M), np.int32), "dst": np.full((G, M), -1, np.int64)}
    slot = 0
    for i, g in enumerate(games):
        r["actions"][i, :len(g.actions)] = g.actions
        for m, legal in enumerate(g.legal):
            assert len(legal) <= max_children
            r["n_children"][i, m] = len(legal)
            r["child_action"][i, m, :len(legal)] = legal
            r["child_visit"][i, m, :len(legal)] = _visits(len(legal))
            r["dst"][i, m] = slot
            slot += 1
    return r, slot


@pytest.mark.parametrize("walk", FIXED_MAP_WALKS + [sd.PER_GAME], ids=_ids(FIXED_MAP_WALKS + [sd.PER_GAME]))
def test_wave_step_admission_and_image_equal_the_oracle_through_the_compact_buffer(walk):
    """nz_scs_replay_check_games accepts every walk (scs_admit_wave on every played action, scs_step_wave<true> on
    every transition) and names the game and length of a flipped outcome; after the save, one gather of all slots gives
    the oracle's image of the position before each ply (scs_state_image_wave<false>), the policy
    float32(float64(visits) / float64(sum)) at the legal actions and the outcome as value; check() stays clean.  The
    per-game case plays randomized_5x5 on the maps its seeds draw."""
    import torch
    from nuzero_amd._lib import NzError, lib
    from nuzero_amd.replay_scs import ScsReplayBuffer
    from nuzero_amd.scs import ScsSelfPlay
    games = walk.games()
    G = len(games)
    cfg = _device_config(walk)
    probe = ScsSelfPlay(cfg, a1_search(1), 1, training=False)
    max_children = probe.MAX_CHILDREN
    probe.close()
    if walk.name == "directed_6x5":
        assert max_children == 128
    r, total = _hand_built_round(games, max_children)
    assert total == sum(len(g.actions) for g in games)
    buf = ScsReplayBuffer(1, 8, cfg, total, max_children)          # capacity: the total number of plies
    assert buf.capacity == total
    buf.register(0, cfg)
    dev = buf.device
    d = {k: torch.from_numpy(v).to(dev) for k, v in r.items()}
    terrain = vp = None
    if walk.map_seeds is not None:
        t, v = cfg.draw_games(list(walk.map_seeds))[:2]
        terrain, vp = torch.from_numpy(np.ascontiguousarray(t)).to(dev), torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    ptr = lambda t: c_void_p(t.data_ptr()) if t is not None else None
    M = int(r["actions"].shape[1])

    def check_games(outcomes):
        buf._check(lib.nz_scs_replay_check_games(buf._h, 0, G, ptr(d["actions"]), M, ptr(d["lengths"]), ptr(outcomes),
                                                 ptr(terrain), ptr(vp), buf._stream()))

    check_games(d["outcomes"])
    finished = [i for i, g in enumerate(games) if g.terminal]
    if finished:
        i = max(finished, key=lambda k: abs(games[k].outcome))     # a decisive game where the walk has one
        bad = d["outcomes"].clone()
        bad[i] = -games[i].outcome if games[i].outcome else 1
        with pytest.raises(NzError, match=rf"game {i}, move {len(games[i].actions)}: the game ended with another outcome"):
            check_games(bad)
    buf._check(lib.nz_scs_replay_save(buf._h, 0, G, ptr(d["actions"]), M, ptr(d["lengths"]), ptr(d["outcomes"]), ptr(terrain),
                                      ptr(vp), ptr(d["child_action"]), ptr(d["child_visit"]), ptr(d["n_children"]), max_children,
                                      ptr(d["dst"]), M, buf._stream()))
    got = buf._gather(np.arange(total, dtype=np.int64))
    buf.check()
    states, policies, values = got.states.cpu().numpy(), got.policies.cpu().numpy(), got.values.cpu().numpy()
    assert (got.game_index.cpu().numpy() == 0).all()
    slot, longest = 0, 0
    for i, g in enumerate(games):
        og = sd.new_game(walk.name, g.map_seed)
        for m, a in enumerate(g.actions):
            image = og.state_image()[0]
            assert np.array_equal(states[slot], image), (walk.label, i, m, _image_diff(states[slot], image))
            legal = g.legal[m]
            v = _visits(len(legal))
            want = np.zeros(cfg.num_actions, np.float32)
            want[legal] = (v.astype(np.float64) / np.float64(v.sum())).astype(np.float32)
            assert np.array_equal(policies[slot], want), (walk.label, i, m)
            assert values[slot] == np.float32(r["outcomes"][i]), (walk.label, i, m)
            longest = max(longest, len(legal))
            og.step_index(a)
            slot += 1
    if walk.name in ("directed_6x5", "many_units_10x10", "many_units_5x6"):
        assert longest > 64                                        # child lists past one stride of the lanes
    buf.check()
    buf.close()


# ---- (c) the wave legal set through nz_scs_openings_expand --------------------------------------------------------------
EXPAND_SETS = {"directed_6x5": sd.DIRECTED, "two_types_6x5": [w for w in sd.DEAD_ENDS if w.name == "two_types_6x5"],
               "one_type_6x5": [w for w in sd.DEAD_ENDS if w.name == "one_type_6x5"]}


@pytest.mark.parametrize("name", list(EXPAND_SETS))
def test_wave_legal_set_equals_the_oracle_at_every_depth(name):
    """nz_scs_openings_expand with the walks' d-ply prefixes as the frontier, for every depth d up to the position each
    game stops in, children requested: the counts are the oracle's numbers of legal actions and the child prefixes'
    last actions the oracle's legal sets in ascending order.  At a dead end the count is 0 although the game is not
    over; at a game's end it is 0 because it is."""
    from nuzero_amd.scs import ScsGameConfig, ScsSelfPlay
    from nuzero_amd.scs_positions import expand_openings
    games = [g for w in EXPAND_SETS[name] for g in w.games()]
    e = ScsSelfPlay(ScsGameConfig(sd.config_path(name)), a1_search(1), 1, training=False)
    assert max(len(g.actions) for g in games) <= e.MAX_MOVES
    checked = 0
    for depth in range(max(len(g.actions) for g in games) + 1):
        rows = [g for g in games if len(g.actions) >= depth]
        frontier = np.array([g.actions[:depth] for g in rows], np.int32).reshape(len(rows), depth)
        want = [g.legal[depth] if depth < len(g.actions) else g.final_legal for g in rows]
        counts, children, _keys = expand_openings(e, frontier)
        assert counts.tolist() == [len(w) for w in want], (name, depth)
        assert children.shape == (sum(len(w) for w in want), depth + 1)
        at = 0
        for g, w in zip(rows, want):
            assert children[at:at + len(w), depth].tolist() == w.tolist(), (name, depth)
            assert (children[at:at + len(w), :depth] == np.array(g.actions[:depth], np.int32)).all(), (name, depth)
            at += len(w)
            checked += 1
    for g in games:
        assert len(g.final_legal) == 0 and (g.dead_end or g.terminal)
    if name != "directed_6x5":
        assert all(g.dead_end for g in games)
    assert checked == sum(len(g.actions) + 1 for g in games)
    e.close()


# ---- (d) the search's own forms, from positions deep in directed play ---------------------------------------------------
SEARCH_POSITIONS = [(0, 40), (1, 80), (2, 120), (3, 160), (0, 200), (0, 240)]       # (game of the advance walk, plies)


def test_searches_from_positions_deep_in_directed_play_equal_the_oracle():
    """Six positions at plies 40, 80, ... 240 of the directed_6x5 advance walk (reset_to), one searched move of 16
    simulations with the board net of the compact-replay tests.
    Host-evaluator route (wave_kernel, images in NCHW for the caller): every leaf evaluation is recorded and the oracle
    replays the move from them -- each consumed leaf's image in order, then the root statistics, bit for bit.
    Library route, wave by wave (images staged in the network's input rows): the same decision with the same root
    statistics.  The persistent route has no form for this shape (105 input planes on 30 cells do not fit a
    wavefront's share of LDS) and must say so before anything is launched."""
    from nuzero_amd._lib import NzError
    from nuzero_amd.scs import ScsGameConfig, ScsSelfPlay
    from nuzero_amd.tester import ScsMatch
    from scs_replay import LeafRecorder, assert_trace_equals_device, replay_games
    from test_gpu_scs_replay_compact import _net
    walk = sd.DIRECTED[0]
    assert walk.mode == "advance"
    games = walk.games()
    prefixes = [games[g].actions[:p] for g, p in SEARCH_POSITIONS]
    assert all(len(games[g].actions) > p for g, p in SEARCH_POSITIONS)
    G = len(prefixes)
    start = np.zeros((G, max(len(p) for p in prefixes)), np.int32)
    for i, p in enumerate(prefixes):
        start[i, :len(p)] = p
    n_plies = np.array([len(p) for p in prefixes], np.int32)
    path = sd.config_path(walk.name)
    cfg = ScsGameConfig(path)
    search = a1_search(SIMS)
    net1, net2 = _net(cfg, G), _net(cfg, G)
    # host-evaluator route
    sp = ScsSelfPlay(cfg, search, G, training=False)
    assert sp.MAX_CHILDREN == 128
    sp.reset_to(start, n_plies)
    rec = LeafRecorder(net1.evaluator(fixed_batch=G))
    sp.search(lambda images: rec(images, sp._leaf_game[:images.shape[0]]))
    sp.apply()
    r = sp.export()
    sp.close()
    assert r["lengths"].tolist() == [len(p) + 1 for p in prefixes]
    outs = replay_games([(path, search, 0, False) + rec.arrays(i) + (1, {"prefix": prefixes[i]}) for i in range(G)])
    for i, out in enumerate(outs):
        assert out["evaluations_used"] == out["evaluations_recorded"] > 0, i
        assert len(out["trace"]) == 1 and out["length"] == len(prefixes[i]) + 1, i
        assert r["actions"][i, :len(prefixes[i])].tolist() == prefixes[i], i
        assert assert_trace_equals_device(r, i, out, "directed", first=len(prefixes[i])) == 1
    # library route, wave by wave: both agents search the position with the same network and search config
    m = ScsMatch(cfg, search, search, G)
    for a in m.agents:
        a.persistent(0)
    rw = m.play(net1, net2, max_moves=1, start_actions=start, n_plies=n_plies)
    assert m.agents[0].persistent() is False and m.agents[1].persistent() is False
    assert rw["lengths"].tolist() == [len(p) + 1 for p in prefixes]
    for a in m.agents:
        ex = a.export()
        for i, p in enumerate(prefixes):
            k = len(p)
            assert ex["actions"][i, :k + 1].tolist() == r["actions"][i, :k + 1].tolist(), i
            c = int(r["n_children"][i, k])
            assert ex["n_children"][i, k] == c and ex["tree_size"][i, k] == r["tree_size"][i, k], i
            assert ex["root_value_sum"][i, k] == r["root_value_sum"][i, k], i
            for key in ("child_action", "child_visit", "child_prior", "child_value_sum"):
                assert np.array_equal(ex[key][i, k, :c], r[key][i, k, :c]), (key, i)
    # the persistent route refuses the shape on the host, before any launch
    for a in m.agents:
        a.persistent(1)
    with pytest.raises(NzError, match="persistent route requested but not available"):
        m.play(net1, net2, max_moves=1, start_actions=start, n_plies=n_plies)
    m.close(); net1.close(); net2.close()
