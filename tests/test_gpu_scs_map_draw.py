"""Per-game "Randomized" SCS maps drawn by the library on the device (nz_scs_search_set_map_draw / _draw_games /
_drawn_games, nuzero_amd/csrc/scs_draw.hip): bit for bit what numpy draws on the host (ScsGameConfig.draw_games) --
maps, victory points, the streams' MT19937 state after the draws -- on the reference's presets and on synthetic
configs; the genuine SCS_Game's maps; the same games (and cache behaviour, hence the same rules rows and digests) on
both routes; the same Gamer rounds; refusals.  Needs a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, "golden")

from test_scs_map_draw_spec import PATH5, PATH10, SYNTHETIC, CONFIGS, _config, synthetic_config   # noqa: E402
from test_gpu_scs_configs import a1_search, _net, _same_games                                        # noqa: E402

SEEDS = [0, 1, 2 ** 31, 2 ** 32 - 1] + list(range(60000, 60000 + 4092))
SIMS = 24


def _engine(cfg, n_games=64):
    from nuzero_amd.scs import ScsSelfPlay
    return ScsSelfPlay(cfg, a1_search(8), n_games)


def _draw_equals_numpy(cfg, seeds):
    """Device draw == host draw: maps, victory points, keys and positions, and the streams go on alike.  Returns the
    host draw."""
    sp = _engine(cfg)
    streams = sp.set_games(seeds)
    host = cfg.draw_games(seeds)
    terrain, vp, keys, pos, host_streams = host
    t, v = sp.game_maps
    assert t.dtype == np.float32 and t.shape == (len(seeds), cfg.rows * cfg.cols, 3)
    assert v.dtype == np.int32 and v.shape == (len(seeds), len(cfg.vp), 2)
    assert np.array_equal(t, terrain) and np.array_equal(v, vp)
    k, p = sp.drawn_streams()
    assert np.array_equal(k, keys) and np.array_equal(p, pos)
    assert len(streams) == len(seeds)
    for g in (0, 3, len(seeds) - 1):
        assert streams[g].random_sample(5).tolist() == host_streams[g].random_sample(5).tolist()
    sp.close()
    return host


@pytest.mark.parametrize("path", [PATH5, PATH10])
def test_device_draw_equals_numpy_on_the_presets(path):
    from nuzero_amd.scs import ScsGameConfig
    terrain, vp, _, _, _ = _draw_equals_numpy(ScsGameConfig(path, per_game=True), SEEDS)
    assert len({t.tobytes() for t in terrain}) > 4000


@pytest.mark.parametrize("name", [n for n, _, _ in SYNTHETIC])
def test_device_draw_equals_numpy_on_synthetic_configs(name):
    cfg = synthetic_config(name)
    _, _, keys, _, _ = _draw_equals_numpy(cfg, SEEDS)
    if name == "10x10 past 624":                # the draws went past position 624: the key was twisted a second time
        for i, s in enumerate(SEEDS[:64]):
            rs = np.random.RandomState(s)
            rs.random_sample()
            assert not np.array_equal(rs.get_state()[1], keys[i]), s


def test_device_draw_gives_the_genuine_maps():
    """scs_pergame_kat.npz: the maps the genuine SCS_Game drew after np.random.seed(map_seed)."""
    from nuzero_amd.scs import ScsGameConfig
    kat = np.load(os.path.join(GOLDEN, "scs_pergame_kat.npz"))
    cfg = ScsGameConfig(PATH5, per_game=True)
    sp = _engine(cfg, 8)
    sp.set_games(kat["map_seed"].tolist())
    t, v = sp.game_maps
    n = len(kat["map_seed"])
    assert np.array_equal(t.reshape(n, 5, 5, 3), kat["terrain"].astype(np.float32))
    assert np.array_equal(v.reshape(n, 2, 2), kat["vp"].reshape(n, 2, 2))
    sp.close()


@pytest.mark.parametrize("route", [1, 0])
def test_same_games_after_the_device_draw(route):
    """play_native and a refill round (play_round_device: more games than trees) with a 64-entry inference cache, whose
    entries are replaced all the time and keyed on the map digests: the device draw plays exactly the games of the host
    draw -- the rules rows and the digests are the same."""
    from nuzero_amd.scs import ScsGameConfig, ScsSelfPlay
    cfg = ScsGameConfig(PATH5, per_game=True)
    G = 48
    seeds, round_seeds = list(range(5100, 5100 + G)), list(range(5300, 5300 + 130))
    net, _ = _net(cfg, "convnet", 32, 3, seed=75, gain=2.0, max_batch=G)
    out = {}
    for on_device in (False, True):
        sp = ScsSelfPlay(cfg, a1_search(SIMS), G)
        sp.draw_on_device = on_device
        sp.persistent(route)
        sp.cache(64)
        ra = sp.play_native(net, seeds)
        assert sp.persistent() is bool(route)
        st_a = sp.cache_stats()
        sp.cache_clear()
        rb = sp.play_round(net, round_seeds)
        maps = sp.game_maps
        out[on_device] = (ra, st_a, rb, sp.cache_stats(), maps)
        sp.close()
    net.close()
    (ha, hst_a, hb, hst_b, hmaps), (da, dst_a, db, dst_b, dmaps) = out[False], out[True]
    _same_games(ha, da, [(g, g) for g in range(G)], f"play_native route {route}")
    _same_games(hb, db, [(g, g) for g in range(len(round_seeds))], f"refill round route {route}")
    # (which of two games writing one entry of the small table wins depends on timing, so the split of hits and misses
    # is not reproducible from run to run; results are, and every evaluation is counted once)
    assert hst_a["hits"] + hst_a["misses"] == dst_a["hits"] + dst_a["misses"] == da["expansions"] and dst_a["hits"] > 0
    assert hst_b["hits"] + hst_b["misses"] == dst_b["hits"] + dst_b["misses"] == db["expansions"] and dst_b["hits"] > 0
    assert np.array_equal(hmaps[0], dmaps[0]) and np.array_equal(hmaps[1], dmaps[1])


def test_python_evaluator_loop_after_the_device_draw():
    """play() takes the games' RandomStates from set_games (built on first use after a device draw)."""
    from nuzero_amd.scs import ScsGameConfig, ScsSelfPlay
    cfg = ScsGameConfig(PATH5, per_game=True)
    G = 16
    seeds = list(range(700, 700 + G))
    net, _ = _net(cfg, "convnet", 32, 3, seed=11, gain=2.0, max_batch=G)
    res = []
    for on_device in (False, True):
        sp = ScsSelfPlay(cfg, a1_search(12), G)
        sp.draw_on_device = on_device
        res.append(sp.play(net.evaluator(), seeds, max_moves=6))
        sp.close()
    net.close()
    _same_games(res[0], res[1], [(g, g) for g in range(G)], "play()")


def _records_equal(ra, rb):
    assert len(ra) == len(rb)
    for a, b in zip(ra, rb):
        assert (a.length, a.terminal_value, a.action_history) == (b.length, b.terminal_value, b.action_history)
        assert a.child_policy == b.child_policy
        for m in range(a.length):
            assert np.array_equal(a.get_state_from_history(m).numpy(), b.get_state_from_history(m).numpy())


def test_gamer_rounds_equal_with_the_host_draw():
    """Two Gamers with the same base_seed on randomized_5x5, one forced to the host draw: two rounds each, identical
    records and statistics."""
    import torch
    from nuzero_amd.gamer import Gamer
    from nuzero_amd.network import Network_Manager
    from nuzero_amd.replay_buffer import ReplayBuffer
    from nuzero_amd.weights import synthetic_weights, convnet_param_shapes

    class SCS_Game:
        pass

    shapes = convnet_param_shapes(86, 21, 3, 32, 2)
    nm = Network_Manager({k: torch.from_numpy(v) for k, v in synthetic_weights(5, shapes, 2.0).items()})
    gamers = [Gamer(ReplayBuffer(100, 16), nm, SCS_Game, [PATH5], 3, a1_search(16), 1, "keyless", size_estimate=4096,
                    num_games=12, concurrent_games=4, base_seed=8100) for _ in range(2)]
    gamers[1].engine.draw_on_device = False
    for _ in range(2):
        (rd, sd), (rh, sh) = (g.play_games() for g in gamers)
        assert sd == sh
        _records_equal(rd, rh)
    assert gamers[0].engine._draws == 2 and gamers[1].engine._draws == 0


def test_refusals():
    from nuzero_amd import _lib
    from nuzero_amd.scs import ScsGameConfig, ScsSelfPlay
    cfg = ScsGameConfig(PATH5, per_game=True)
    sp = _engine(cfg)
    # the C ABI on its own (a caller without the Python layer): no spec yet, then specs it refuses
    seeds = np.arange(64, dtype=np.uint32)
    assert _lib.lib.nz_scs_search_draw_games(sp._h, 64, ctypes.c_void_p(seeds.ctypes.data), None) == _lib.NZ_ERR_STATE
    spec = _lib.ScsMapDraw(n_types=0, order=(ctypes.c_int32 * 2)(_lib.NZ_SCS_DRAW_VP, 0),
                           number_vp=(ctypes.c_int32 * 2)(11, 1), side_cols=(ctypes.c_int32 * 4)(0, 2, 3, 5))
    assert _lib.lib.nz_scs_search_set_map_draw(sp._h, ctypes.byref(spec)) == _lib.NZ_ERR_ARG
    assert b"11 victory points drawn, the description has 1" in _lib.lib.nz_scs_search_last_error(sp._h)
    spec.number_vp[0] = 1
    spec.side_cols[1] = 0
    assert _lib.lib.nz_scs_search_set_map_draw(sp._h, ctypes.byref(spec)) == _lib.NZ_ERR_ARG
    spec.order[0] = 0
    assert _lib.lib.nz_scs_search_set_map_draw(sp._h, ctypes.byref(spec)) == _lib.NZ_ERR_ARG
    assert b"nothing to draw" in _lib.lib.nz_scs_search_last_error(sp._h)
    assert _lib.lib.nz_scs_search_draw_games(sp._h, 64, ctypes.c_void_p(seeds.ctypes.data), None) == _lib.NZ_ERR_STATE
    # seeds numpy refuses; fewer games than the engine plays
    for bad in (2 ** 32, -1):
        with pytest.raises(ValueError, match="Seed must be between 0 and 2\\*\\*32 - 1"):
            sp.set_games(list(range(63)) + [bad])
    with pytest.raises(_lib.NzError, match="64 at a time"):
        sp.set_games(list(range(10)))
    # the engine still draws after the refusals
    sp.set_games(range(64))
    assert np.array_equal(sp.game_maps[0], cfg.draw_games(range(64))[0])
    sp.close()

    def too_many(d):
        d["Victory_points"]["number_vp"] = {"p1": 1, "p2": 11}
    for edit, msg in ((lambda d: d["Map"].update(distribution=[0.1, 0.15, 0.6, 0.1]), "probabilities do not sum to 1"),
                      (too_many, "player 2: 11 victory points on a side of 10 cells")):
        bad = _engine(ScsGameConfig(_config(PATH5, edit), per_game=True))
        with pytest.raises(ValueError, match=msg):
            bad.set_games(range(64))
        bad.close()
    fixed = ScsSelfPlay(ScsGameConfig(os.path.join(CONFIGS, "mirrored_5x5.yml")), a1_search(8), 64)
    with pytest.raises(ValueError, match="nothing to draw"):
        fixed.set_games(range(64))
    fixed.close()
