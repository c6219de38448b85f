"""SCS self-play with the board net in the plain-bf16 mode (BoardNet(precision="bf16")), on both search routes -- the
pattern of tests/test_gpu_scs_persist.py's test_persistent_route_equals_the_oracle_replay_and_the_wave_route:
  * the persistent route (wave_network<HEX, PREC_BF16> inside persist_kernel) and the wave-by-wave route
    (fused16_net_kernel<HEX, PREC_BF16> on the leaf batches) play the same games bit for bit;
  * the exact oracle replay on the evaluations the kernel recorded reproduces every action, count, prior and value sum
    (the search's correctness does not depend on the network's floats);
  * every recorded leaf's probabilities and value ARE nz_boardnet_forward's of the same planes, bit for bit (all games:
    the replay keeps every leaf's planes, tests/scs_planes_replay.py);
  * the games are not the float32 mode's games on the same seeds.
Needs a GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, "golden")

from test_gpu_scs_configs import a1_search, _same_games, _game_properties   # noqa: E402


def _net(cfg, arch, width, depth, seed, gain, hexnet, max_batch, precision):
    from nuzero_amd.boardnet import BoardNet
    from nuzero_amd.weights import synthetic_weights, hex_param_shapes, convnet_param_shapes, resnet_param_shapes
    shapes = (convnet_param_shapes(cfg.channels, cfg.planes, 3, width, depth) if arch == "convnet"
              else resnet_param_shapes(cfg.channels, cfg.planes, width, depth))
    w = synthetic_weights(seed, hex_param_shapes(shapes) if hexnet else shapes, gain)
    net = BoardNet(arch, cfg.channels, cfg.planes, cfg.rows, cfg.cols, width=width, num_blocks=depth, kernel_size=3,
                   max_batch=max_batch, hex=hexnet, precision=precision)
    net.set_weights(w, 1)
    return net, w


def _replay_every_game(path, search, seeds, recs, r, games, label):
    """The exact oracle replay of every game in `games` on its recorded evaluations (worker processes): the trace equals
    the device's.  Returns {game: the planes of its recorded leaves, in the order they were recorded}."""
    from scs_planes_replay import replay_games_keeping_planes
    from scs_replay import assert_trace_equals_device
    outs = replay_games_keeping_planes([(path, search, seeds[g]) + recs[g] for g in games])
    planes = {}
    for g, out in zip(games, outs):
        assert out["evaluations_used"] == len(recs[g][2]) == len(out["planes"]), (label, g)
        assert out["length"] == r["lengths"][g] and out["terminal_value"] == r["outcomes"][g], (label, g)
        assert assert_trace_equals_device(r, g, out, label) == r["lengths"][g], (label, g)
        planes[g] = out["planes"]
    return planes


def _leaves_are_forward(net_big, planes, rec, label):
    import torch
    _, probs, values = rec
    for at in range(0, len(planes), net_big.max_batch):
        x = torch.from_numpy(planes[at:at + net_big.max_batch]).cuda().contiguous()
        p, v = net_big.forward(x)
        assert np.array_equal(p.cpu().numpy().view(np.int32), probs[at:at + len(x)].view(np.int32)), (label, at, "probabilities")
        assert np.array_equal(v.cpu().numpy().view(np.int32), values[at:at + len(x)].view(np.int32)), (label, at, "values")


def _differ(ra, rb, G):
    """At least one move or prior differs between two exports of the same seeds."""
    for g in range(G):
        n = min(ra["lengths"][g], rb["lengths"][g])
        if ra["lengths"][g] != rb["lengths"][g] or not np.array_equal(ra["actions"][g, :n], rb["actions"][g, :n]):
            return True
        c = ra["n_children"][g, 0]
        if not np.array_equal(ra["child_prior"][g, 0, :c], rb["child_prior"][g, 0, :c]):
            return True
    return False


@pytest.mark.parametrize("arch,hexnet", [("convnet", False), ("resnet", False), ("convnet", True), ("resnet", True)])
def test_both_routes_in_bf16_mode(arch, hexnet):
    from nuzero_amd.scs import ScsSelfPlay, ScsGameConfig
    path = os.path.join(GOLDEN, "scs_configs", "late_reinforcements_5x5.yml" if arch == "convnet" else "mirrored_5x5.yml")
    cfg = ScsGameConfig(path)
    G = 12
    depth = 3 if arch == "convnet" else 2
    net, w = _net(cfg, arch, 32, depth, 43, 2.5, hexnet, G, "bf16")
    assert net.precision == "bf16"
    search = a1_search(48, number_of_softmax_moves=4, epsilon_softmax_exploration=0.1, epsilon_random_exploration=0.05,
                       root_exploration_fraction=0.25, root_dist_alpha=0.3)
    seeds = list(range(1900, 1900 + G))
    sp = ScsSelfPlay(cfg, search, G)
    sp.persistent(1)                                   # a play fails if the route is not available
    sp.record(range(G), 48 * (sp.MAX_MOVES + 1))
    rp = sp.play_native(net, seeds)
    assert sp.persistent() is True
    recs = sp.records()
    assert (rp["lengths"] > 10).all()
    assert rp["simulations"] == 48 * int(rp["lengths"].sum())
    assert rp["expansions"] == sum(len(v[2]) for v in recs.values())
    _game_properties(path, rp, range(G))
    # the exact oracle replay of every game on its recorded leaves, the leaves' planes kept
    planes = _replay_every_game(path, search, seeds, recs, rp, range(G), arch)
    # every recorded leaf of every game is nz_boardnet_forward of its planes (another handle, other batch slots)
    big, _ = _net(cfg, arch, 32, depth, 43, 2.5, hexnet, 256, "bf16")
    for g in range(G):
        _leaves_are_forward(big, planes[g], recs[g], (arch, hexnet, g))
    assert sum(len(planes[g]) for g in range(G)) == rp["expansions"]
    big.close()
    # the wave-by-wave route plays the same games
    sp.record([], 0)
    sp.persistent(0)
    rw = sp.play_native(net, seeds)
    assert sp.persistent() is False
    _same_games(rp, rw, [(g, g) for g in range(G)], arch)
    assert rw["expansions"] == rp["expansions"] and rw["simulations"] == rp["simulations"]
    net.close()
    # ... and they are not the float32 mode's games
    net32, _ = _net(cfg, arch, 32, depth, 43, 2.5, hexnet, G, "float32")
    r32 = sp.play_native(net32, seeds)
    assert _differ(rw, r32, G), "the bf16 mode played the float32 mode's games: is it on?"
    sp.close(); net32.close()


def test_bf16_mode_with_more_than_64_children():
    """many_units_5x6: the kernel variant that holds a node's children in chunks of 64 lanes, in the bf16 mode."""
    from nuzero_amd.scs import ScsSelfPlay, ScsGameConfig
    name, sims = "many_units_5x6", 16
    path = os.path.join(GOLDEN, "scs_configs", name + ".yml")
    cfg = ScsGameConfig(path)
    G = 6
    net, w = _net(cfg, "convnet", 32, 2, 47, 2.5, False, G, "bf16")
    search = a1_search(sims, number_of_softmax_moves=30, epsilon_softmax_exploration=0.1, epsilon_random_exploration=0.05,
                       root_exploration_fraction=0.25, root_dist_alpha=0.3)
    seeds = list(range(2300, 2300 + G))
    sp = ScsSelfPlay(cfg, search, G)
    assert sp.MAX_CHILDREN > 64
    sp.persistent(1)
    sp.record(range(G), sims * (sp.MAX_MOVES + 1))
    rp = sp.play_native(net, seeds)
    assert sp.persistent() is True
    assert int(rp["n_children"].max()) > 64
    recs = sp.records()
    _game_properties(path, rp, range(G))
    planes = _replay_every_game(path, search, seeds, recs, rp, range(G), name)
    big, _ = _net(cfg, "convnet", 32, 2, 47, 2.5, False, 256, "bf16")
    for g in range(G):
        _leaves_are_forward(big, planes[g], recs[g], (name, g))
    assert sum(len(planes[g]) for g in range(G)) == rp["expansions"]
    big.close()
    sp.record([], 0)
    sp.persistent(0)
    rw = sp.play_native(net, seeds)
    assert sp.persistent() is False
    _same_games(rp, rw, [(g, g) for g in range(G)], name)
    sp.close(); net.close()
