"""The compact SCS replay buffer (nuzero_amd.replay_scs.ScsReplayBuffer, C ABI nz_scs_replay_*): positions stored as
game states and rendered in the gather.  The reference is always the dense DeviceReplayBuffer fed the same device
records of the same round; both run the same rules code, so the comparison is exact (torch.equal on states, policies,
values and game indices) -- there is no tolerance to choose.  Needs a GPU."""
import os
import random
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
pytestmark = pytest.mark.gpu
CONFIGS = os.path.join(HERE, "golden", "scs_configs")

SEARCH = {"Simulation": {"mcts_simulations": 12, "keep_subtree": True}, "UCT": {"pb_c_base": 10000, "pb_c_init": 1.15},
          "Exploration": {"number_of_softmax_moves": 0, "epsilon_softmax_exploration": 0.04,
                          "epsilon_random_exploration": 0.001, "value_factor": 1,
                          "root_exploration_distribution": "gamma", "root_exploration_fraction": 0.2,
                          "root_dist_alpha": 0.2, "root_dist_beta": 1}}


def _path(name):
    return os.path.join(CONFIGS, name + ".yml")


def _net(cfg, max_batch):
    from nuzero_amd.boardnet import BoardNet
    from nuzero_amd.weights import synthetic_weights, convnet_param_shapes
    net = BoardNet("convnet", cfg.channels, cfg.planes, cfg.rows, cfg.cols, width=32, num_blocks=2, max_batch=max_batch)
    net.set_weights(synthetic_weights(4, convnet_param_shapes(cfg.channels, cfg.planes, 3, 32, 2), 2.0))
    return net


def _buffers(cfg, window, max_moves, max_children):
    from nuzero_amd.replay_device import DeviceReplayBuffer
    from nuzero_amd.replay_scs import ScsReplayBuffer
    dense = DeviceReplayBuffer(window, 8, (cfg.channels, cfg.rows, cfg.cols), cfg.num_actions, max_game_length=max_moves)
    compact = ScsReplayBuffer(window, 8, cfg, max_moves, max_children)
    return dense, compact


def _same_batch(got, want):
    import torch
    assert len(got) == len(want)
    assert torch.equal(got.states, want.states)
    assert torch.equal(got.policies, want.policies)
    assert torch.equal(got.values, want.values)
    assert torch.equal(got.game_index, want.game_index)
    assert got.keys == want.keys and got.counts == want.counts


def _same_contents(compact, dense):
    assert compact.len() == dense.len() and compact.played_games() == dense.played_games()
    _same_batch(compact.get_slice(0, compact.len()), dense.get_slice(0, dense.len()))


def _same_entries(got, want):
    import torch
    assert len(got) == len(want)
    for (s1, (v1, p1), g1), (s2, (v2, p2), g2) in zip(got, want):
        assert torch.equal(s1, s2) and v1 == v2 and g1 == g2
        assert np.array_equal(np.asarray(p1, np.float32), torch.tensor(p2).numpy())      # AlphaZero.py:901


def test_compact_buffer_equals_the_dense_one_through_evictions_shuffles_and_samples():
    """mirrored_5x5, six games through a window of four (evictions inside one batch): the whole buffer, slices after
    shuffles, samples in three modes and batches grouped by game index -- compact == dense == the host list."""
    from nuzero_amd.replay_buffer import ReplayBuffer
    from nuzero_amd.replay_device import late_heavy_probs
    from nuzero_amd.scs import ScsSelfPlay, ScsGameConfig, scs_game_records
    cfg = ScsGameConfig(_path("mirrored_5x5"))
    net = _net(cfg, 6)
    sp = ScsSelfPlay(cfg, SEARCH, 6)
    r = sp.play_native(net, range(20, 26))
    host = ReplayBuffer(4, 8)
    for rec in scs_game_records(sp, r):
        host.save_game(rec, 1)
    dense, compact = _buffers(cfg, 4, sp.MAX_MOVES, sp.MAX_CHILDREN)
    ex = sp.export_device()
    dense.save_scs_games(sp, ex, 1)
    lengths = compact.save_scs_games(sp, ex, 1)
    assert lengths.tolist() == r["lengths"].tolist()
    dense.check(); compact.check()
    assert compact.played_games() == 4 and compact.len() == host.len()
    assert compact.bytes_per_position * 4 <= (cfg.channels * 25 + cfg.num_actions + 2) * 4 and compact.capacity == dense.capacity
    _same_contents(compact, dense)
    _same_entries(compact.get_buffer(), dense.get_buffer())
    _same_entries(compact.get_buffer(), host.get_buffer())
    for seed in (1, 2):
        random.seed(seed); dense.shuffle()
        random.seed(seed); compact.shuffle()
        _same_batch(compact.get_slice(3, 35), dense.get_slice(3, 35))
    n = dense.len()
    for replace, probs in ((True, []), (False, []), (True, late_heavy_probs(n))):
        np.random.seed(5); want = dense.get_sample(32, replace, probs)
        np.random.seed(5); got = compact.get_sample(32, replace, probs)
        _same_batch(got, want)
        assert got.states.shape == (32, cfg.channels, 5, 5) and got.policies.shape == (32, cfg.num_actions) and got.states.is_cuda
    np.random.seed(9); want = dense.get_sample(32, True, [], group_by_game=True)
    np.random.seed(9); got = compact.get_sample(32, True, [], group_by_game=True)
    _same_batch(got, want)
    compact.check()
    dense.close(); compact.close(); sp.close(); net.close()


@pytest.mark.parametrize("route,n_games,n_trees", [("native", 6, 6), ("round", 10, 4)])
def test_records_carry_their_own_maps_through_shuffles_and_evictions(route, n_games, n_trees):
    """randomized_5x5, every game on its own map; two rounds with a shuffle between them through a window smaller than
    the first round, so the second round evicts shuffled positions of any game: contents equal the dense buffer's after
    each round.  ("round": 10 games over 4 trees, nz_scs_search_play_round.)"""
    from nuzero_amd.scs import ScsSelfPlay, ScsGameConfig
    cfg = ScsGameConfig(_path("randomized_5x5"), per_game=True)
    net = _net(cfg, n_trees)
    sp = ScsSelfPlay(cfg, SEARCH, n_trees)
    dense, compact = _buffers(cfg, n_games - 2, sp.MAX_MOVES, sp.MAX_CHILDREN)
    for rnd in range(2):
        seeds = range(300 + 50 * rnd, 300 + 50 * rnd + n_games)
        if route == "native":
            sp.play_native(net, seeds)
            ex = sp.export_device()
        else:
            ex = sp.play_round_device(net, seeds)
        assert len({t.tobytes() for t in sp.game_maps[0][:n_games]}) > 1
        dense.save_scs_games(sp, ex, 2)
        compact.save_scs_games(sp, ex, 2)
        dense.check(); compact.check()
        _same_contents(compact, dense)
        random.seed(7 + rnd); dense.shuffle()
        random.seed(7 + rnd); compact.shuffle()
        _same_contents(compact, dense)
    assert compact.index.full and compact.played_games() == n_games - 2
    dense.close(); compact.close(); sp.close(); net.close()


def test_two_descriptions_of_one_shape_share_a_buffer():
    """mirrored_5x5 under game index 0 and late_reinforcements_5x5 under 1: mixed batches equal the dense buffer's; a
    different description under an index in use, or one of another board shape, is refused and changes nothing."""
    from nuzero_amd._lib import NzError
    from nuzero_amd.scs import ScsSelfPlay, ScsGameConfig
    cfgs = [ScsGameConfig(_path(n)) for n in ("mirrored_5x5", "late_reinforcements_5x5")]
    assert (cfgs[0].channels, cfgs[0].num_actions) == (cfgs[1].channels, cfgs[1].num_actions)
    net = _net(cfgs[0], 6)
    sps = [ScsSelfPlay(c, SEARCH, 6) for c in cfgs]
    dense, compact = _buffers(cfgs[0], 20, max(s.MAX_MOVES for s in sps), max(s.MAX_CHILDREN for s in sps))
    exports = []
    for gi, sp in enumerate(sps):
        sp.play_native(net, range(40 + 10 * gi, 46 + 10 * gi))
        exports.append(sp.export_device())
        dense.save_scs_games(sp, exports[gi], gi)
        compact.save_scs_games(sp, exports[gi], gi)
    _same_contents(compact, dense)
    random.seed(3); dense.shuffle()
    random.seed(3); compact.shuffle()
    np.random.seed(4); want = dense.get_sample(48, True, [], group_by_game=True)
    np.random.seed(4); got = compact.get_sample(48, True, [], group_by_game=True)
    assert got.keys == [0, 1]
    _same_batch(got, want)
    before = compact.get_slice(0, compact.len())
    with pytest.raises(NzError, match="different description"):
        compact.save_scs_games(sps[1], exports[1], 0)
    with pytest.raises(NzError, match="tiles"):
        compact.register(2, ScsGameConfig(_path("many_units_5x6")))
    assert compact.len() == dense.len()
    _same_batch(compact.get_slice(0, compact.len()), before)
    compact.check()
    dense.close(); compact.close(); net.close()
    for sp in sps:
        sp.close()


@pytest.mark.parametrize("name,cap", [("reference_test_config", 40), ("many_units_5x6", None), ("many_units_10x10", None)])
def test_edge_shapes_equal_the_dense_buffer(name, cap):
    """Stacking 3 (105 image planes, 30 action planes) with games stopped before their end; boards of 30 and 100 tiles
    whose positions have more than 64 legal actions (lane loops over the child list, tile loops past one wavefront)."""
    from nuzero_amd.scs import ScsSelfPlay, ScsGameConfig
    cfg = ScsGameConfig(_path(name))
    net = _net(cfg, 6)
    sp = ScsSelfPlay(cfg, SEARCH, 6)
    r = sp.play_native(net, range(60, 66), max_moves=cap)
    longest = int(r["lengths"].max())
    if cap:
        assert cfg.stacking == 3 and cfg.channels == 105 and cfg.planes == 30
        assert (r["lengths"] == cap).all()                     # every game stops before its end
    else:
        assert max(int(r["n_children"][g, :r["lengths"][g]].max()) for g in range(6)) > 64
        assert cfg.rows * cfg.cols == (30 if name == "many_units_5x6" else 100)
    dense, compact = _buffers(cfg, 5, longest, sp.MAX_CHILDREN)
    ex = sp.export_device()
    dense.save_scs_games(sp, ex, 0)
    compact.save_scs_games(sp, ex, 0)
    dense.check(); compact.check()
    _same_contents(compact, dense)
    random.seed(1); dense.shuffle()
    random.seed(1); compact.shuffle()
    np.random.seed(2); want = dense.get_sample(40, True, [])
    np.random.seed(2); got = compact.get_sample(40, True, [])
    _same_batch(got, want)
    dense.close(); compact.close(); sp.close(); net.close()


def test_damaged_records_are_reported_and_nothing_is_stored():
    """An illegal action, an action outside the action space and a flipped outcome: each is an NzError naming game and
    move, before anything is stored -- never a step on an illegal action."""
    from nuzero_amd._lib import NzError
    from nuzero_amd.replay_scs import ScsReplayBuffer
    from nuzero_amd.scs import ScsBatch, ScsSelfPlay, ScsGameConfig
    cfg = ScsGameConfig(_path("mirrored_5x5"))
    net = _net(cfg, 6)
    sp = ScsSelfPlay(cfg, SEARCH, 6)
    r = sp.play_native(net, range(20, 26))
    ex = sp.export_device()
    compact = ScsReplayBuffer(100, 8, cfg, sp.MAX_MOVES, sp.MAX_CHILDREN)
    compact.save_scs_games(sp, ex, 1)
    before, n_before, games_before = compact.get_slice(0, compact.len()), compact.len(), compact.played_games()
    # an action whose bit is clear in the legal mask of game 2's position before move 3
    batch = ScsBatch(cfg, 6)
    for m in range(3):
        batch.step(r["actions"][:, m].astype(np.int32))
    mask = batch.legal_mask().cpu().numpy().reshape(6, -1)
    batch.close()
    assert mask[2, r["actions"][2, 3]] == 1
    illegal = int(np.nonzero(mask[2] == 0)[0][0])
    g_out = 5
    assert r["lengths"][g_out] < sp.MAX_MOVES                  # the game reached its end
    cases = []
    bad = dict(ex); bad["actions"] = ex["actions"].clone(); bad["actions"][2, 3] = illegal
    cases.append((bad, "game 2, move 3"))
    bad = dict(ex); bad["actions"] = ex["actions"].clone(); bad["actions"][4, 2] = cfg.num_actions + 5
    cases.append((bad, "game 4, move 2"))
    bad = dict(ex); bad["outcomes"] = ex["outcomes"].clone()
    bad["outcomes"][g_out] = -1 if int(r["outcomes"][g_out]) != -1 else 1
    cases.append((bad, f"game {g_out}, move {int(r['lengths'][g_out])}"))
    for bad, where in cases:
        with pytest.raises(NzError, match=where):
            compact.save_scs_games(sp, bad, 1)
        assert compact.len() == n_before and compact.played_games() == games_before
        _same_batch(compact.get_slice(0, compact.len()), before)
        compact.check()
    assert np.array_equal(compact.index.seq, np.arange(n_before))
    compact.close(); sp.close(); net.close()


def test_bad_slots_raise_the_error_word_and_leave_their_rows_alone():
    """A batch slot outside the buffer (flag 4) and a slot that was never saved (an empty record whose game index has no
    description, flag 16) are skipped -- their rows of the batch stay as they were -- and check() reports them, sticky."""
    import torch
    from nuzero_amd._lib import NzError, NZ_ERR_OVERFLOW
    from nuzero_amd.replay_scs import ScsReplayBuffer
    from nuzero_amd.scs import ScsSelfPlay, ScsGameConfig
    cfg = ScsGameConfig(_path("mirrored_5x5"))
    net = _net(cfg, 6)
    sp = ScsSelfPlay(cfg, SEARCH, 6)
    sp.play_native(net, range(20, 26))
    compact = ScsReplayBuffer(100, 8, cfg, sp.MAX_MOVES, sp.MAX_CHILDREN)
    compact.save_scs_games(sp, sp.export_device(), 1)
    compact.check()
    good = compact._gather(np.array([3, 4], np.int64))
    for bad_slot, flag in ((compact.capacity, 4), (-1, 4), (compact.capacity - 1, 16)):
        fresh = ScsReplayBuffer(100, 8, cfg, sp.MAX_MOVES, sp.MAX_CHILDREN)
        fresh.save_scs_games(sp, sp.export_device(), 1)
        got = fresh._gather(np.array([3, bad_slot, 4], np.int64))
        with pytest.raises(NzError, match=f"flag {flag}:") as e:
            fresh.check()
        assert e.value.code == NZ_ERR_OVERFLOW
        assert torch.equal(got.states[[0, 2]], good.states) and torch.equal(got.policies[[0, 2]], good.policies)
        with pytest.raises(NzError):
            fresh.check()
        fresh.close()
    compact.close(); sp.close(); net.close()


def test_gamer_fills_the_compact_buffer_as_it_fills_the_dense_one():
    """Gamer(..., records=False) picks the compact buffer up through save_scs_games: a round of 10 games over 4 trees on
    randomized_5x5 (every game on its own map) leaves the same positions as a second Gamer with the same seeds leaves
    in a DeviceReplayBuffer, and the same statistics."""
    import torch
    from nuzero_amd.gamer import Gamer
    from nuzero_amd.network import Network_Manager
    from nuzero_amd.scs import ScsSelfPlay, ScsGameConfig
    from nuzero_amd.weights import synthetic_weights, convnet_param_shapes

    class SCS_Game:                      # only the class name is looked at
        pass

    path = _path("randomized_5x5")
    cfg = ScsGameConfig(path, per_game=True)
    probe = ScsSelfPlay(cfg, SEARCH, 1)
    max_moves, max_children = probe.MAX_MOVES, probe.MAX_CHILDREN
    probe.close()
    model = {k: torch.from_numpy(v) for k, v in synthetic_weights(5, convnet_param_shapes(86, 21, 3, 32, 2), 2.0).items()}
    nm = Network_Manager(model)
    dense, compact = _buffers(cfg, 8, max_moves, max_children)
    stats = []
    for buf in (compact, dense):
        g = Gamer(buf, nm, SCS_Game, [path], 3, SEARCH, 1, "disabled", num_games=10, concurrent_games=4, base_seed=7700,
                  records=False)
        for _ in range(2):                                       # the second round evicts the first
            records, st = g.play_games()
            assert records == [] and len(st) == 10
            stats.append(st)
        g.engine.close()
    assert stats[0] == stats[2] and stats[1] == stats[3]
    dense.check(); compact.check()
    assert compact.played_games() == 8 and set(compact.get_slice(0, 5).game_index.tolist()) == {3}
    _same_contents(compact, dense)
    dense.close(); compact.close()


def test_checkpoints(tmp_path):
    """save_compact -> load_compact into a fresh buffer: the same buffer, games and samples; save_to_file writes the
    reference's layout, which the host ReplayBuffer loads; what cannot work raises and says where to go instead."""
    from nuzero_amd import ScsReplayBuffer
    from nuzero_amd.replay_buffer import ReplayBuffer
    from nuzero_amd.scs import ScsSelfPlay, ScsGameConfig, scs_game_records
    cfg = ScsGameConfig(_path("randomized_5x5"), per_game=True)
    net = _net(cfg, 6)
    sp = ScsSelfPlay(cfg, SEARCH, 6)
    compact = ScsReplayBuffer(4, 8, cfg, sp.MAX_MOVES, sp.MAX_CHILDREN)
    r = sp.play_native(net, range(80, 86))
    compact.save_scs_games(sp, sp.export_device(), 5)
    random.seed(11); compact.shuffle()
    compact.step_to_size_map[3] = (compact.len(), compact.played_games())
    compact.save_compact(tmp_path / "compact.pt")
    again = ScsReplayBuffer(4, 8, cfg, sp.MAX_MOVES, sp.MAX_CHILDREN)
    again.load_compact(tmp_path / "compact.pt")
    assert again.played_games() == compact.played_games() == 4 and again.index.full and again.step_to_size_map == {3: (compact.len(), 4)}
    _same_contents(again, compact)
    _same_entries(again.get_buffer(), compact.get_buffer())
    np.random.seed(6); want = compact.get_sample(16, False, [], group_by_game=True)
    np.random.seed(6); got = again.get_sample(16, False, [], group_by_game=True)
    _same_batch(got, want)
    other = ScsReplayBuffer(4, 8, cfg, sp.MAX_MOVES, sp.MAX_CHILDREN + 64)      # another record size: refused
    with pytest.raises(ValueError, match="bytes"):
        other.load_compact(tmp_path / "compact.pt")
    other.close()
    # a further round into the loaded buffer evicts as it does in the original
    sp.play_native(net, range(90, 96))
    ex = sp.export_device()
    compact.save_scs_games(sp, ex, 5); again.save_scs_games(sp, ex, 5)
    _same_contents(again, compact)
    # the reference's layout
    compact.save_to_file(tmp_path / "rb.pt", step=7)
    host = ReplayBuffer(4, 8)
    host.load_from_file(tmp_path / "rb.pt", 7)
    _same_entries(compact.get_buffer(), host.get_buffer())
    with pytest.raises(NotImplementedError, match="DeviceReplayBuffer"):
        again.load_from_file(tmp_path / "rb.pt", 7)
    with pytest.raises(NotImplementedError, match="DeviceReplayBuffer"):
        again.save_game(scs_game_records(sp, sp.export())[0], 5)
    again.check(); compact.check()
    again.close(); compact.close(); sp.close(); net.close()
