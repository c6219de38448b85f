"""Lifecycle of the SCS search handle's buffer groups (nuzero_amd/csrc/scs_search.hip: cache, leaf recording, per-game
rows and draw buffers, round store, match buffers): replaced, grown, reused and released on ONE handle, every play must
equal the same play on a FRESH handle -- exported records compared with ==, no tolerance (the oracle-replay tests
establish that a fresh handle is right).  8 game slots, 8 simulations, 5x5 boards.  Needs a GPU."""
import os
import sys
from ctypes import byref, c_int32, c_void_p

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
pytestmark = pytest.mark.gpu
CONFIGS = os.path.join(HERE, "golden", "scs_configs")
MIRRORED = os.path.join(CONFIGS, "mirrored_5x5.yml")
RANDOMIZED = os.path.join(CONFIGS, "randomized_5x5.yml")

from test_gpu_scs_configs import a1_search, _net          # noqa: E402

G, SIMS, MOVES = 8, 8, 6
ZEROS = [0] * G


def _same(a, b, label):
    """The records of the decisions that were played: actions, and per decision the root's children."""
    assert np.array_equal(a["lengths"], b["lengths"]) and np.array_equal(a["outcomes"], b["outcomes"]), label
    assert a["actions"].shape == b["actions"].shape, label
    played = np.arange(a["actions"].shape[1])[None, :] < a["lengths"][:, None]
    assert played.any(), label
    assert np.array_equal(a["n_children"][played], b["n_children"][played]), label
    child = played[:, :, None] & (np.arange(a["child_visit"].shape[2])[None, None, :] < a["n_children"][:, :, None])
    assert np.array_equal(a["actions"][played], b["actions"][played]), label
    for k in ("child_action", "child_visit", "child_prior", "child_value_sum"):
        assert np.array_equal(a[k][child], b[k][child]), (label, k)


@pytest.fixture(scope="module")
def mirrored():
    from nuzero_amd.scs import ScsGameConfig
    cfg = ScsGameConfig(MIRRORED)
    net, _ = _net(cfg, "convnet", 32, 3, seed=11, gain=2.0)
    yield cfg, net
    net.close()


@pytest.fixture(scope="module")
def randomized():
    from nuzero_amd.scs import ScsGameConfig
    cfg = ScsGameConfig(RANDOMIZED, per_game=True)
    net, _ = _net(cfg, "convnet", 32, 3, seed=12, gain=2.0)
    yield cfg, net
    net.close()


def _engine(cfg, training=False):
    from nuzero_amd.scs import ScsSelfPlay
    return ScsSelfPlay(cfg, a1_search(SIMS), G, training=training)


def test_cache_resized_under_use(mirrored):
    cfg, net = mirrored
    fresh = {}
    for size in (1 << 12, 64, 0):
        f = _engine(cfg)
        f.cache(size)
        fresh[size] = f.play_native(net, ZEROS, max_moves=MOVES)
        f.close()
    sp = _engine(cfg)
    for size in (1 << 12, 64, 0, 1 << 12):
        sp.cache(size)
        out = sp.play_native(net, ZEROS, max_moves=MOVES)
        _same(out, fresh[size], f"cache({size})")
        assert sp.cache_stats()["size"] == size
    sp.close()


def _read_record(sp, slot, capacity):
    """nz_scs_search_record_read of one slot: (evaluations consumed, rows kept)."""
    from nuzero_amd._lib import lib
    A, count = sp.cfg.planes * sp.cfg.rows * sp.cfg.cols, c_int32(0)
    sp._check(lib.nz_scs_search_record_read(sp._h, slot, byref(count), None, None, None))
    n = min(count.value, capacity)
    dig, pr, va = np.zeros((n, 2), np.uint64), np.zeros((n, A), np.float32), np.zeros((n,), np.float32)
    sp._check(lib.nz_scs_search_record_read(sp._h, slot, byref(count), c_void_p(dig.ctypes.data), c_void_p(pr.ctypes.data),
                                            c_void_p(va.ctypes.data)))
    return count.value, dig, pr


def test_recording_on_off_on_with_another_capacity(mirrored):
    from nuzero_amd._lib import NzError
    cfg, net = mirrored
    f = _engine(cfg)
    f.persistent(1)
    want = f.play_native(net, ZEROS, max_moves=MOVES)
    f.close()
    sp = _engine(cfg)
    sp.persistent(1)
    for games, capacity in (([0, 3], 16), ([], 0), ([1], 4)):
        sp.record(games, capacity)
        _same(sp.play_native(net, ZEROS, max_moves=MOVES), want, f"record({games}, {capacity})")
        assert sp.persistent()
        for slot in range(len(games)):
            count, dig, pr = _read_record(sp, slot, capacity)
            print(f"record({games}, {capacity}) slot {slot}: {count} evaluations consumed, {len(dig)} kept")
            assert count > capacity and len(dig) == capacity          # 8 simulations x 6 moves: more than either capacity
            assert dig.any(axis=1).all() and np.allclose(pr.sum(axis=1), 1.0, atol=1e-4)
        with pytest.raises(NzError):                                    # no slot past the requested ones
            _read_record(sp, len(games), capacity)
    sp.close()


@pytest.mark.parametrize("on_device", [True, False])
def test_game_rows_and_draw_buffers_grow_and_are_reused(randomized, on_device):
    from nuzero_amd._lib import lib
    cfg, net = randomized
    rounds = [list(range(500, 500 + n)) for n in (8, 24, 8)]
    rounds[2] = list(range(900, 908))

    def play(sp, seeds):
        sp.draw_on_device = on_device
        return sp.play_round(net, seeds)

    sp = _engine(cfg, training=True)
    for seeds in rounds:
        f = _engine(cfg, training=True)
        _same(play(sp, seeds), play(f, seeds), f"{len(seeds)} games from seed {seeds[0]}")
        f.close()
    # no per-game maps any more: the description's one map, as an engine that never had any
    sp._check(lib.nz_scs_search_set_games(sp._h, 0, None, None, None, None))
    f, outs = _engine(cfg, training=True), []  # (the same description; the engines differ in their past only)
    seeds = np.arange(40, 40 + G, dtype=np.uint32)
    for e in (sp, f):
        e._check(lib.nz_scs_search_play_moves(e._h, net._h, c_void_p(seeds.ctypes.data), MOVES, e._stream()))
        outs.append(e.export())
    _same(outs[0], outs[1], "back to the description's map")
    sp.close(); f.close()


def test_round_store_growth(mirrored):
    cfg, net = mirrored
    fresh = {}
    for n in (16, 40):
        f = _engine(cfg, training=True)
        fresh[n] = f.play_round(net, range(100, 100 + n))
        f.close()
    sp = _engine(cfg, training=True)
    for n in (16, 40, 16):
        out = sp.play_round(net, range(100, 100 + n))
        assert out["actions"].shape[0] == n
        _same(out, fresh[n], f"round of {n}")
    sp.close()


def _same_match(ra, rb, label):
    for k in ("matches", "p1_wins", "p2_wins", "draws", "unfinished", "length_sum", "length_max"):
        assert ra[k] == rb[k], (label, k)
    assert np.array_equal(ra["lengths"], rb["lengths"]) and np.array_equal(ra["outcomes"], rb["outcomes"]), label
    assert ra["actions"].shape == rb["actions"].shape and np.array_equal(ra["actions"], rb["actions"]), label


def test_match_buffers_made_once_and_reused(mirrored):
    from nuzero_amd.tester import ScsMatch
    cfg, net1 = mirrored
    net2, _ = _net(cfg, "resnet", 32, 2, seed=13, gain=2.0)
    s1, s2 = a1_search(SIMS), a1_search(SIMS, pb_c_init=1.15)

    def fresh(sa, sb):
        m = ScsMatch(cfg, sa, sb, G)
        r = m.play(net1, net2, max_moves=MOVES)
        m.close()
        return r

    want = fresh(s1, s2)
    m = ScsMatch(cfg, s1, s2, G)
    for i in range(2):
        _same_match(m.play(net1, net2, max_moves=MOVES), want, f"round {i + 1} on one pair")
    # the handle that kept the match buffers now follows: agent 2 of another pair
    other = ScsMatch(cfg, s2, s1, G)
    other.agents[1].close()
    other.agents = (other.agents[0], m.agents[0])
    _same_match(other.play(net1, net2, max_moves=MOVES), fresh(s2, s1), "agent 1 as agent 2 of another pair")
    other.agents[0].close()
    m.close(); net2.close()


def test_nothing_left_behind(randomized):
    import torch
    cfg, net = randomized

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    def cycle():
        before = free()
        sp = _engine(cfg, training=True)
        sp.cache(1 << 12)
        sp.persistent(1)
        sp.record([0, 3], 16)
        sp.play_round(net, range(300, 316))        # drawn games, per-game rows, a 16-game round
        held = before - free()
        sp.close()
        return held

    readings, footprint = {}, 0
    for i in range(1, 13):
        held = cycle()
        if i in (2, 12):
            readings[i] = free()
        if i == 2:
            footprint = held                       # (cycle 1 also warms the tensor allocator up)
    print(f"free after cycle 2: {readings[2]}, after cycle 12: {readings[12]}, one handle holds {footprint} bytes")
    assert footprint > 0
    assert readings[12] >= readings[2] - footprint


def test_nothing_left_behind_with_the_network_handle(randomized):
    """The same with the network handle made and closed inside the cycle: every play asks the new handle for its
    per-wavefront program (persistent(1) stays set), which that handle builds, owns and releases."""
    import torch
    cfg, _ = randomized

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    def cycle():
        before = free()
        net, _ = _net(cfg, "convnet", 32, 3, seed=12, gain=2.0)
        sp = _engine(cfg, training=True)
        sp.cache(1 << 12)
        sp.persistent(1)
        sp.record([0, 3], 16)
        sp.play_round(net, range(300, 316))
        assert sp.persistent()
        held = before - free()
        sp.close()
        net.close()
        return held

    readings, footprint = {}, 0
    for i in range(1, 13):
        held = cycle()
        if i in (2, 12):
            readings[i] = free()
        if i == 2:
            footprint = held                       # (cycle 1 also warms the tensor allocator up)
    print(f"free after cycle 2: {readings[2]}, after cycle 12: {readings[12]}, search and network hold {footprint} bytes")
    assert footprint > 0
    assert readings[12] >= readings[2] - footprint
