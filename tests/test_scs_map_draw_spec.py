"""The spec of the device map draw (ScsGameConfig.map_draw_spec, nz_scs_search_set_map_draw) and the algorithm the draw
kernel runs on it (nuzero_amd/csrc/scs_draw.hip), restated here in Python and held against numpy's own draw
(ScsGameConfig.draw_games): maps, victory points and the streams' state after the draws.  CPU only."""
import copy
import os

import numpy as np
import pytest
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
CONFIGS = os.path.join(HERE, "golden", "scs_configs")
PATH5 = os.path.join(CONFIGS, "randomized_5x5.yml")
PATH10 = os.path.join(CONFIGS, "randomized_10x10.yml")


class _Mt:
    """MT19937 as scs_draw.hip steps it: init_genrand, the twist when the position reaches 624, tempering."""

    def __init__(self, seed):
        self.key, s = [0] * 624, seed
        for i in range(624):
            self.key[i] = s
            s = (1812433253 * (s ^ (s >> 30)) + i + 1) & 0xFFFFFFFF
        self.pos, self.twists = 624, 0

    def u32(self):
        if self.pos == 624:
            k = self.key
            for i in range(624):
                y = (k[i] & 0x80000000) | (k[(i + 1) % 624] & 0x7FFFFFFF)
                k[i] = k[(i + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
            self.pos, self.twists = 0, self.twists + 1
        y = self.key[self.pos]
        self.pos += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        return y ^ (y >> 18)

    def double(self):
        a, b = self.u32() >> 5, self.u32() >> 6
        return (a * 67108864.0 + b) / 9007199254740992.0

    def randint(self, n):
        if n <= 1:
            return 0
        rng = n - 1
        mask = (1 << rng.bit_length()) - 1
        while True:
            v = self.u32() & mask
            if v <= rng:
                return v


def _kernel_draw(cfg, seed):
    """One game as the draw kernel draws it from map_draw_spec(): (terrain [tiles, 3], vp [k, 2], mt)."""
    sp = cfg.map_draw_spec()
    terrain, vp = cfg.terrain.copy(), cfg.vp.copy()
    mt = _Mt(seed)
    for section in sp["order"]:
        if section == "Map":
            for t in range(cfg.rows * cfg.cols):
                u = mt.double()
                idx = min(int(np.searchsorted(sp["cdf"], u, side="right")), len(sp["cdf"]) - 1)
                terrain[t] = sp["types"][idx]
        else:
            base = 0
            for side, (first, end) in enumerate(sp["side_cols"]):
                for i in range(sp["number_vp"][side]):
                    while True:
                        pt = (mt.randint(cfg.rows), first + mt.randint(end - first))
                        if pt not in [tuple(p) for p in vp[base:base + i].tolist()]:
                            break
                    vp[base + i] = pt
                base += sp["number_vp"][side]
    return terrain, vp, mt


def _config(path, edit=None):
    with open(path) as f:
        d = yaml.safe_load(f)
    if edit:
        edit(d)
    return d


def _vp_first(d):
    """The same config with "Victory_points" listed before "Map"."""
    out = {k: v for k, v in d.items() if k not in ("Map", "Victory_points")}
    out["Victory_points"] = d["Victory_points"]
    out["Map"] = d["Map"]
    d.clear()
    d.update(out)


def _many_vp(d):
    d["Victory_points"]["number_vp"] = {"p1": 40, "p2": 40}     # every cell of each side


def _one_column_side(d):
    """A 5 x 3 board: each side is one column (define_board_sides of an odd width)."""
    d["Board_dimensions"]["columns"] = 3
    d["Victory_points"]["number_vp"] = {"p1": 4, "p2": 5}


def _zero_type(d):
    d["Map"]["distribution"] = [0.3, 0.0, 0.45, 0.25]


def _map_only(d):
    d["Victory_points"] = {"creation_method": "Detailed", "vp_locations": {"p1": [[0, 0]], "p2": [[4, 4]]}}


def _vp_only(d):
    d["Map"] = {"creation_method": "Detailed", "map_configuration": [[3, 1, 2, 4, 3]] * 5}


# (name, path, edit): the synthetic configs the GPU test draws as well (tests/test_gpu_scs_map_draw.py)
SYNTHETIC = [("zero-probability type", PATH5, _zero_type), ("map only", PATH5, _map_only),
             ("victory points only", PATH5, _vp_only), ("victory points first", PATH5, _vp_first),
             ("one-column side", PATH5, _one_column_side), ("10x10 past 624", PATH10, _many_vp)]


def synthetic_config(name):
    from nuzero_amd.scs import ScsGameConfig
    path, edit = {n: (p, e) for n, p, e in SYNTHETIC}[name]
    return ScsGameConfig(_config(path, edit), per_game=True)


def test_spec_of_randomized_5x5():
    from nuzero_amd.scs import ScsGameConfig
    sp = ScsGameConfig(PATH5, per_game=True).map_draw_spec()
    assert sp["order"] == ("Map", "Victory_points") and sp["number_vp"] == (1, 1)
    assert sp["side_cols"] == ((0, 2), (3, 5))
    assert sp["types"].dtype == np.float32 and sp["types"].tolist() == [[0.5, 1, 2], [1, 2, 2], [1, 1, 1], [2, 1, 1]]
    p = np.array([0.1, 0.15, 0.65, 0.1])
    assert sp["cdf"].dtype == np.float64 and sp["cdf"].tolist() == (p.cumsum() / p.cumsum()[-1]).tolist()
    assert sp["cdf"][-1] == 1.0


def test_spec_of_a_uniform_map_and_vp_first():
    from nuzero_amd.scs import ScsGameConfig

    def edit(d):
        del d["Map"]["distribution"]
        _vp_first(d)
    sp = ScsGameConfig(_config(PATH5, edit), per_game=True).map_draw_spec()
    assert sp["order"] == ("Victory_points", "Map")
    assert sp["cdf"].tolist() == (np.array([0.25] * 4).cumsum() / np.array([0.25] * 4).sum()).tolist()


@pytest.mark.parametrize("seed", [0, 1, 7, 2 ** 31, 2 ** 32 - 1])
@pytest.mark.parametrize("path", [PATH5, PATH10])
def test_kernel_algorithm_equals_numpy_on_the_presets(path, seed):
    from nuzero_amd.scs import ScsGameConfig
    cfg = ScsGameConfig(path, per_game=True)
    terrain, vp, keys, pos, _ = cfg.draw_games([seed])
    t, v, mt = _kernel_draw(cfg, seed)
    assert np.array_equal(t, terrain[0]) and np.array_equal(v, vp[0])
    assert mt.key == keys[0].tolist() and mt.pos == pos[0]


@pytest.mark.parametrize("name", [n for n, _, _ in SYNTHETIC])
def test_kernel_algorithm_equals_numpy_on_synthetic_configs(name):
    cfg = synthetic_config(name)
    seeds = [0, 1, 2 ** 31, 2 ** 32 - 1] + list(range(100, 140))
    terrain, vp, keys, pos, _ = cfg.draw_games(seeds)
    wrapped = 0
    for i, s in enumerate(seeds):
        t, v, mt = _kernel_draw(cfg, s)
        assert np.array_equal(t, terrain[i]) and np.array_equal(v, vp[i]), (name, s)
        assert mt.key == keys[i].tolist() and mt.pos == pos[i], (name, s)
        wrapped += mt.twists > 1
    if name == "10x10 past 624":
        assert wrapped == len(seeds)          # every game's draws went past position 624: a second twist
    if name == "victory points only":
        assert np.array_equal(terrain, np.repeat(cfg.terrain[None], len(seeds), 0))
    if name == "map only":
        assert np.array_equal(vp, np.repeat(cfg.vp[None], len(seeds), 0))


def test_refuses_a_distribution_numpy_refuses():
    from nuzero_amd.scs import ScsGameConfig
    for dist, msg in (([0.1, 0.15, 0.6, 0.1], "probabilities do not sum to 1"),
                      ([0.5, -0.1, 0.5, 0.1], "probabilities are not non-negative"),
                      ([0.5, 0.5], "'a' and 'p' must have same size")):
        def edit(d):
            d["Map"]["distribution"] = dist
        cfg = ScsGameConfig(_config(PATH5, edit), per_game=True)
        with pytest.raises(ValueError, match=msg):
            cfg.map_draw_spec()
        with pytest.raises(ValueError, match=msg):        # what the reference (and the host draw) raises
            cfg.draw_games([0])


def test_refuses_more_victory_points_than_a_side_has_cells():
    from nuzero_amd.scs import ScsGameConfig

    def edit(d):
        d["Victory_points"]["number_vp"] = {"p1": 11, "p2": 1}       # side of player 1: 5 rows x 2 columns
    with pytest.raises(ValueError, match="player 1: 11 victory points on a side of 10 cells"):
        ScsGameConfig(_config(PATH5, edit), per_game=True).map_draw_spec()

    def edit_ok(d):
        d["Victory_points"]["number_vp"] = {"p1": 10, "p2": 10}
    assert ScsGameConfig(_config(PATH5, edit_ok), per_game=True).map_draw_spec()["number_vp"] == (10, 10)


def test_refuses_a_config_without_randomized_sections():
    from nuzero_amd.scs import ScsGameConfig
    cfg = ScsGameConfig(os.path.join(CONFIGS, "mirrored_5x5.yml"), per_game=True)
    assert not cfg.per_game
    with pytest.raises(ValueError, match="nothing to draw"):
        cfg.map_draw_spec()
    one_map = ScsGameConfig(PATH5, map_seed=3)
    with pytest.raises(ValueError, match="nothing to draw"):
        one_map.map_draw_spec()


def test_seed_range_is_numpys():
    from nuzero_amd.scs import _seed_array
    assert _seed_array([0, 1, 2 ** 32 - 1]).tolist() == [0, 1, 2 ** 32 - 1]
    assert _seed_array(np.arange(5, dtype=np.uint32)).dtype == np.uint32
    for bad in ([-1], [2 ** 32], [2 ** 70]):
        with pytest.raises(ValueError, match="Seed must be between 0 and 2\\*\\*32 - 1"):
            _seed_array(bad)
        with pytest.raises(ValueError, match="Seed must be between 0 and 2\\*\\*32 - 1"):
            np.random.RandomState(bad[0])


def test_spec_is_not_built_twice_and_leaves_the_config_alone():
    from nuzero_amd.scs import ScsGameConfig
    d = _config(PATH5)
    before = copy.deepcopy(d)
    cfg = ScsGameConfig(d, per_game=True)
    assert cfg.map_draw_spec() is cfg.map_draw_spec()
    assert d == before
