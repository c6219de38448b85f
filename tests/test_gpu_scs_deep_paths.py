"""Both SCS search routes against the CPU oracle on descents past 64 levels, and the exact size at which a game's tree
arena is full.  Cases and their choice: tests/scs_deep.py; what the oracle alone must show for them to mean anything:
tests/test_scs_deep_paths_host.py.

Whole games of `two_types_6x5` (host evaluator; 114-117 decisions) and `one_type_6x5` (network; 103 and 113) at 150
simulations with a peaked evaluation: per game 33 to 563 simulations run on paths longer than 64, and leaves that need
an evaluation occur at every path length from 60 to 70.
Nodes first backed up at level 64 and deeper later become roots, so their counts land in the records compared here.

Exercised now, on the code of scs_search.hip:
  * wave_kernel (host-evaluator route and the library's wave-by-wave route): the pending leaf taken from a lane
    (plen <= 64) and from path[plen - 1] (plen > 64), lanes < plen backed up from registers with the tail from memory
    (backup_tail from 64), and the terminal leaf's whole-path backup (backup_tail from 0) past its first stride -- 16
    terminal leaves on paths longer than 64 in the evaluation-mode case, 40 and 114 in the network case's games;
  * persist_leader: levels 0..63 in my_path, levels from 64 in path[], the backup from both, on pending and on
    terminal leaves (the same 40 and 114);
  * the arena check `base + k > half_cap` on all three routes, at the last size that fits and the first that does not,
    and the leader's and the helper's way out of the persistent kernel when it trips.
Still resting on reading the code:
  * levels 128 and up (the second stride of backup_tail): the longest path of any case is 87;
  * compact_kernel's own arena check, which cannot trigger (the subtree it copies comes from a half that fits).
With both tail backups taken out of scs_search.hip (tried once, not kept) the two host-evaluator tests and the
library-routes test fail, and every earlier test_gpu_scs*.py test still passes.
Needs a GPU."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, "golden")

import scs_deep                                                                         # noqa: E402
from scs_deep import deep_jobs, oracle_games, simulations_deeper_than                   # noqa: E402
from test_gpu_scs_configs import a1_search, _net, _same_games, _game_properties         # noqa: E402
from test_gpu_scs_persist import _replay_recorded, _oracle_net_on_leaves                # noqa: E402


def _host_evaluator(fn, num_actions):
    import torch

    def ev(images):
        out = [fn(im, num_actions) for im in images.cpu().numpy()]
        return (torch.from_numpy(np.stack([o[0] for o in out])), torch.from_numpy(np.array([o[1] for o in out], np.float32)))
    return ev


def _equals_the_oracle(r, g, out, label):
    """Game g of the device export `r` is the oracle's game `out`: `==` on everything, value sums included."""
    from scs_replay import assert_trace_equals_device
    assert r["lengths"][g] == out["length"], (label, g)
    if out["terminal"]:
        assert r["outcomes"][g] == out["terminal_value"], (label, g)
    assert assert_trace_equals_device(r, g, out, label) == len(out["trace"]) == out["length"]


@pytest.mark.parametrize("case", scs_deep.HOST_EVAL_CASES, ids=["training", "evaluation"])
def test_host_evaluator_route_equals_the_oracle_on_paths_past_64_levels(case):
    """ScsSelfPlay.play (wave_kernel, one host round trip per wave) with evaluate_image_peaked on both sides.  The arena
    is exactly as large as the oracle's peak node count says it must be (the evaluation-mode game keeps 48,356 nodes
    alive, twice what the default arena holds)."""
    from scs_eval import evaluate_image_peaked
    from nuzero_amd.scs import ScsSelfPlay, ScsGameConfig
    _, training, seeds = case
    outs = oracle_games(deep_jobs([case]))
    for out in outs:                                    # a run that stopped going deep must fail, not pass
        assert out["longest_path"] > 66 and simulations_deeper_than(out, 64) >= 20
    cfg = ScsGameConfig(scs_deep.CONFIG)
    search = scs_deep.deep_search()
    sp = ScsSelfPlay(cfg, search, len(seeds), training=training, nodes_per_game=2 * max(o["peak_nodes"] for o in outs))
    r = sp.play(_host_evaluator(evaluate_image_peaked, cfg.num_actions), list(seeds))
    sp.close()
    for g, out in enumerate(outs):
        _equals_the_oracle(r, g, out, case)
    _game_properties(scs_deep.CONFIG, r, range(len(seeds)))
    assert r["simulations"] == scs_deep.SIMS * int(r["lengths"].sum())


_LIBRARY = {}


def _library_games():
    """The network case on both library routes, played once for the tests below: (persistent route's export, its recorded
    evaluations, wave-by-wave route's export, search config, seeds, training, weights)."""
    if not _LIBRARY:
        from nuzero_amd.boardnet import BoardNet
        from nuzero_amd.scs import ScsSelfPlay, ScsGameConfig
        (_, training, seeds), = scs_deep.NET_CASES
        seeds, G = list(seeds), len(seeds)
        cfg = ScsGameConfig(scs_deep.NET_CONFIG)
        arch, width, depth, vact = scs_deep.NET
        w = scs_deep.peaked_net_weights(cfg.channels, cfg.planes)
        net = BoardNet(arch, cfg.channels, cfg.planes, cfg.rows, cfg.cols, width=width, num_blocks=depth,
                       value_activation=vact, kernel_size=3, max_batch=G)
        net.set_weights(w, 1)
        search = scs_deep.deep_search()
        sp = ScsSelfPlay(cfg, search, G, training=training)
        sp.persistent(1)                                   # a play fails if the route is not available
        sp.record(range(G), scs_deep.SIMS * (sp.MAX_MOVES + 1))
        rp = sp.play_native(net, seeds)
        assert sp.persistent() is True
        recs = sp.records()
        sp.record([], 0)
        sp.persistent(0)
        rw = sp.play_native(net, seeds)
        assert sp.persistent() is False
        sp.close(); net.close()
        _LIBRARY["games"] = (rp, recs, rw, search, seeds, training, w)
    return _LIBRARY["games"]


def test_library_routes_equal_the_oracle_replay_on_paths_past_64_levels():
    """The persistent route with the peaked network: the oracle replays both games from the evaluations the kernel itself
    recorded -- every consumed leaf's digest in order, which is what catches a wrongly chosen or wrongly backed-up deep
    node -- and the replay's own counters say that the paths went past 64 levels.  The wave-by-wave route plays the same
    games.  On `one_type_6x5`: the persistent route refuses `two_types_6x5` (105 input planes on 30 cells do not fit a
    wavefront's share of LDS; here 86)."""
    rp, recs, rw, search, seeds, training, _ = _library_games()
    G = len(seeds)
    assert rp["simulations"] == scs_deep.SIMS * int(rp["lengths"].sum())
    assert rp["expansions"] == sum(len(v[2]) for v in recs.values())
    _game_properties(scs_deep.NET_CONFIG, rp, range(G))
    outs = []
    moves = _replay_recorded(scs_deep.NET_CONFIG, search, seeds, rp, recs, range(G), "deep", training=training, outs_to=outs)
    assert moves == int(rp["lengths"].sum())
    for out in outs:                                    # a run that stopped going deep must fail, not pass
        assert out["longest_path"] > 66 and simulations_deeper_than(out, 64) >= 20
    assert sum(simulations_deeper_than(out, 64, terminal=True) for out in outs) > 0
    # the wave-by-wave route plays the same games
    _same_games(rp, rw, [(g, g) for g in range(G)], "deep")
    assert rw["expansions"] == rp["expansions"] and rw["simulations"] == rp["simulations"]


def test_the_peaked_network_is_the_oracle_network_within_1e_5_on_recorded_leaves():
    """The evaluations the persistent kernel recorded for root positions of game 0 against the oracle network
    (float32, oracle/net.py) at the project's 1e-5, so that the scaled net is covered as well as the search.  The
    float32 oracle is itself within 0.31e-5 of the float64 one on these games' root positions
    (tests/test_scs_deep_paths_host.py), which is what leaves a float32-accurate device room under the bound.
    Measured on an MI355X: 0.59e-5 on the probabilities, 6e-8 on the values."""
    rp, recs, _, _, _, _, w = _library_games()
    arch, _, depth, vact = scs_deep.NET
    print(_oracle_net_on_leaves(scs_deep.NET_CONFIG, w, arch, depth, False, rp, 0, recs, 12, value_activation=vact))


# ---- the arena limit ----------------------------------------------------------------------------------------------------
ARENA_CONFIG = os.path.join(GOLDEN, "scs_configs", "mirrored_5x5.yml")
ARENA_SIMS, ARENA_GAMES, ARENA_MOVES = 16, 3, 6


def _arena_search():
    return a1_search(ARENA_SIMS, number_of_softmax_moves=2, epsilon_softmax_exploration=0.1, epsilon_random_exploration=0.05,
                     root_exploration_fraction=0.25, root_dist_alpha=0.3)


def _overflow_flag(err):
    from nuzero_amd import _lib
    assert err.code == _lib.NZ_ERR_OVERFLOW, err
    found = re.search(r"flag (\d+)", str(err))
    assert found, err
    return int(found.group(1))


@pytest.mark.parametrize("route", ["host-evaluator", "wave", "persistent"])
def test_a_game_arena_holds_exactly_the_live_trees_peak_and_reports_one_node_less(route):
    """A half of a game's arena holds the live tree: after a move's search, 1 + the children of every expanded node
    reachable from the root (the oracle's peak_nodes; compaction keeps the new root's subtree, each expansion appends
    its children).  N = the largest over the games and moves played: with nodes_per_game = 2 N the games are those of a
    default-arena handle, with 2 N - 2 the play ends in NZ_ERR_OVERFLOW with flag 1 (arena full) -- on the persistent
    route together with flag 4: the game's leader wavefront leaves with simulations to go (its helper with it), and
    end_move_kernel reports the unfinished search."""
    from scs_eval import evaluate_image
    from scs_replay import replay_games
    from nuzero_amd._lib import NzError
    from nuzero_amd.scs import ScsSelfPlay, ScsGameConfig
    cfg = ScsGameConfig(ARENA_CONFIG)
    search = _arena_search()
    G = ARENA_GAMES
    seeds = list(range(3100, 3100 + G))
    net = None
    if route != "host-evaluator":
        net, _ = _net(cfg, "convnet", 32, 2, seed=43, gain=2.5, max_batch=G)

    def play(nodes_per_game, record=False):
        sp = ScsSelfPlay(cfg, search, G, nodes_per_game=nodes_per_game)
        try:
            if route == "host-evaluator":
                return sp.play(_host_evaluator(evaluate_image, cfg.num_actions), seeds, max_moves=ARENA_MOVES), None
            sp.persistent(1 if route == "persistent" or record else 0)
            if record:
                sp.record(range(G), ARENA_SIMS * (ARENA_MOVES + 1))
            r = sp.play_native(net, seeds, max_moves=ARENA_MOVES)
            assert sp.persistent() is (route == "persistent" or record)
            return r, (sp.records() if record else None)
        finally:
            sp.close()

    if route == "host-evaluator":
        r0, _ = play(None)
        outs = oracle_games([(ARENA_CONFIG, search, s, True, "flat", ARENA_MOVES) for s in seeds])
    else:
        # the replay needs the evaluations the persistent kernel records; the wave-by-wave route plays the same games
        rr, recs = play(None, record=True)
        outs = replay_games([(ARENA_CONFIG, search, seeds[g], True) + recs[g] + (ARENA_MOVES,) for g in range(G)])
        for out in outs:
            assert out["evaluations_used"] == out["evaluations_recorded"]
        r0 = rr if route == "persistent" else play(None)[0]
        _same_games(rr, r0, [(g, g) for g in range(G)], route)
    from scs_replay import assert_trace_equals_device
    for g, out in enumerate(outs):
        assert r0["lengths"][g] == ARENA_MOVES == assert_trace_equals_device(r0, g, out, route)
    n = max(out["peak_nodes"] for out in outs)
    assert n > ARENA_SIMS                              # (more than the roots' own children: the trees grew)
    fits, _ = play(2 * n)
    _same_games(r0, fits, [(g, g) for g in range(G)], route)
    with pytest.raises(NzError) as full:
        play(2 * n - 2)
    flag = _overflow_flag(full.value)
    assert flag & 1, flag
    if route == "persistent":
        assert flag & 4, flag
    if net is not None:
        net.close()
