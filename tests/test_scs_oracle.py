"""oracle/scs.py against the SCS golden vectors made from the genuine reference
(tests/golden/make_golden_scs.py).  CPU only."""
import os

import numpy as np
import pytest

from oracle.scs import ScsConfig, ScsGame

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONFIGS = {
    "mirrored5": None,    # the reference's own mirrored_config_5.yml: restated below as data
    "late_reinf": os.path.join(GOLDEN, "scs_configs", "late_reinforcements_5x5.yml"),
    "ten_by_ten": os.path.join(GOLDEN, "scs_configs", "ten_by_ten.yml"),
    "two_types": os.path.join(GOLDEN, "scs_configs", "two_types_6x5.yml"),
}


@pytest.fixture(scope="module")
def kat():
    return dict(np.load(os.path.join(GOLDEN, "scs_kat.npz")))


def checksum_weights(n):
    i = np.arange(n, dtype=np.int64)
    return ((i * 2654435761) % 1000003).astype(np.float64) / 1000003.0


@pytest.mark.parametrize("name", ["late_reinf", "ten_by_ten", "two_types", "mirrored5"])
def test_scs_rules_against_reference(kat, name):
    path = CONFIGS[name] or os.path.join(GOLDEN, "scs_configs", "mirrored_5x5.yml")
    cfg = ScsConfig(path)
    planes, rows, cols, channels, stacking, turns = kat[f"{name}_shape"]
    assert (cfg.planes, cfg.rows, cfg.cols, cfg.channels, cfg.stacking, cfg.turns) == (planes, rows, cols, channels,
                                                                                       stacking, turns)
    game_ids, actions = kat[f"{name}_game"], kat[f"{name}_action"]
    legal, n_legal = kat[f"{name}_legal"], kat[f"{name}_n_legal"]
    images = {int(s): img for s, img in zip(kat[f"{name}_image_step"], kat[f"{name}_images"])}
    w = checksum_weights(channels * rows * cols)
    pos = 0
    g, last = None, -1
    n_images = 0
    for i in range(len(actions)):
        if game_ids[i] != last:
            if g is not None:
                _check_end(kat, name, last, g, images)
            g, last = ScsGame(cfg), int(game_ids[i])
        assert not g.is_terminal()
        assert (g.player, g.sub_phase, g.stage, g.turn) == (kat[f"{name}_player"][i], kat[f"{name}_sub_phase"][i],
                                                           kat[f"{name}_stage"][i], kat[f"{name}_turn"][i]), i
        mask = g.possible_actions()
        assert mask.dtype == np.int8 and mask.shape == (planes, rows, cols)
        idx = np.nonzero(mask.flatten())[0]
        assert idx.tolist() == legal[pos:pos + n_legal[i]].tolist(), i
        pos += n_legal[i]
        img = g.state_image()
        assert img.dtype == np.float32 and img.shape == (1, channels, rows, cols)
        assert float(np.sum(img.reshape(-1).astype(np.float64) * w)) == kat[f"{name}_checksum"][i], i
        if i in images:
            assert np.array_equal(img[0], images[i]), i
            n_images += 1
        g.step_index(int(actions[i]))
    _check_end(kat, name, last, g, images)
    assert n_images > 20


def _check_end(kat, name, gi, g, images):
    assert g.is_terminal()
    assert g.get_length() == kat[f"{name}_lengths"][gi] and g.get_terminal_value() == kat[f"{name}_values"][gi]
    assert np.array_equal(g.state_image()[0], images[-(gi + 1)])


def test_scs_search_against_reference():
    """oracle/search.py on oracle/scs.py vs MCTS games the genuine reference played on SCS
    (float32 priors, float64 after root noise, players 0/1 so Q is never negated)."""
    import gzip
    import json
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from scs_eval import evaluate_image
    from oracle import search as osearch
    with gzip.open(os.path.join(GOLDEN, "scs_search_kat.json.gz"), "rt") as f:
        kat = json.load(f)
    files = {"mirrored_config_5.yml": "mirrored_5x5.yml"}
    for name, case in kat.items():
        cfg = ScsConfig(os.path.join(GOLDEN, "scs_configs", files.get(case["config_file"], case["config_file"])))
        ev = lambda game: evaluate_image(game.state_image()[0], cfg.num_actions)
        for ref in case["games"]:
            game = ScsGame(cfg)
            trace = []
            osearch.play_game(game, ev, case["config"], np.random.RandomState(ref["seed"]),
                              training=case["training"], trace=trace)
            assert game.length == ref["length"] and game.terminal_value == ref["terminal_value"], name
            assert len(trace) == len(ref["moves"])
            for mine, theirs in zip(trace, ref["moves"]):
                for key in ("action", "root_visits", "root_value_sum", "child_actions", "child_visits",
                            "child_priors", "child_value_sums"):
                    assert mine[key] == theirs[key], (name, key)


def test_randomized_maps_against_reference():
    """"Randomized" maps and victory points (SCS_Game.py:1678-1738): what the genuine reference builds after
    np.random.seed(seed) (tests/golden/scs_random_maps.json, made by make_golden_scs_random.py) equals what the oracle
    and the product's host-side config build from map_seed=seed, for both of the reference's randomized configs."""
    import json
    from nuzero_amd.scs import ScsGameConfig
    from oracle.scs import ScsConfig
    with open(os.path.join(GOLDEN, "scs_random_maps.json")) as f:
        gold = json.load(f)
    assert set(gold) == {"randomized_5x5", "randomized_10x10"}
    for name, cases in gold.items():
        path = os.path.join(GOLDEN, "scs_configs", name + ".yml")
        with pytest.raises(Exception):
            ScsGameConfig(path)                               # no seed: refused, not guessed
        seen = set()
        for seed, want in cases.items():
            oc = ScsConfig(path, map_seed=int(seed))
            assert [[list(map(float, t)) for t in row] for row in oc.terrain] == want["terrain"], (name, seed)
            assert [list(map(list, side)) for side in oc.vp] == want["vp"], (name, seed)
            pc = ScsGameConfig(path, map_seed=int(seed))
            assert np.array_equal(pc.terrain.reshape(oc.rows, oc.cols, 3), np.array(want["terrain"], np.float32))
            assert pc.vp.tolist() == [list(p) for side in want["vp"] for p in side]
            seen.add(json.dumps(want["terrain"]))
        assert len(seen) == len(cases)                        # the seeds give different maps


def test_games_on_their_own_randomized_maps_against_reference():
    """A new "Randomized" map per game (Gamer.py:52 builds a game object per game; SCS_Game.py:1678-1738 draws its map
    at construction): 24 games the genuine SCS_Game played, each after np.random.seed(5000 + i) (scs_pergame_kat.npz,
    tests/golden/make_golden_scs_pergame.py) -- the oracle on the map it draws from the same seed, step by step."""
    kat = dict(np.load(os.path.join(GOLDEN, "scs_pergame_kat.npz")))
    path = os.path.join(GOLDEN, "scs_configs", "randomized_5x5.yml")
    planes, rows, cols, channels, stacking, turns = kat["shape"]
    w = checksum_weights(channels * rows * cols)
    images = {int(s): img for s, img in zip(kat["image_step"], kat["images"])}
    game_ids, actions, legal, n_legal = kat["game"], kat["action"], kat["legal"], kat["n_legal"]
    pos, g, last, n_images = 0, None, -1, 0

    def end(gi, g):
        assert g.is_terminal() and g.get_length() == kat["lengths"][gi] and g.get_terminal_value() == kat["values"][gi]
        assert np.array_equal(g.state_image()[0], images[-(gi + 1)])

    for i in range(len(actions)):
        if game_ids[i] != last:
            if g is not None:
                end(last, g)
            last = int(game_ids[i])
            cfg = ScsConfig(path, map_seed=int(kat["map_seed"][last]))
            assert np.array_equal(np.array(cfg.terrain, np.float64), kat["terrain"][last])
            assert [[list(p) for p in side] for side in cfg.vp] == kat["vp"][last].tolist()
            g = ScsGame(cfg)
        assert (g.player, g.sub_phase, g.stage, g.turn) == (kat["player"][i], kat["sub_phase"][i], kat["stage"][i], kat["turn"][i]), i
        idx = np.nonzero(g.possible_actions().flatten())[0]
        assert idx.tolist() == legal[pos:pos + n_legal[i]].tolist(), i
        pos += n_legal[i]
        img = g.state_image()
        assert float(np.sum(img.reshape(-1).astype(np.float64) * w)) == kat["checksum"][i], i
        if i in images:
            assert np.array_equal(img[0], images[i]), i
            n_images += 1
        g.step_index(int(actions[i]))
    end(last, g)
    assert n_images > 100 and len(set(kat["terrain"].reshape(24, -1).sum(1).tolist())) > 10


def test_search_on_per_game_maps_against_reference():
    """MCTS self-play where every game has its own map and ONE stream (np.random.seed(s); SCS_Game(config); play): the
    oracle draws the map from RandomState(s) and its Explorer goes on with the same stream."""
    import gzip
    import json
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from scs_eval import evaluate_image
    from oracle import search as osearch
    with gzip.open(os.path.join(GOLDEN, "scs_search_pergame_kat.json.gz"), "rt") as f:
        kat = json.load(f)
    path = os.path.join(GOLDEN, "scs_configs", "randomized_5x5.yml")
    for name, case in kat.items():
        for ref in case["games"]:
            rs = np.random.RandomState(ref["seed"])
            cfg = ScsConfig(path, map_seed=rs)
            assert np.array_equal(np.array(cfg.terrain, np.float64), np.array(ref["terrain"]))
            ev = lambda game: evaluate_image(game.state_image()[0], cfg.num_actions)
            game = ScsGame(cfg)
            trace = []
            osearch.play_game(game, ev, case["config"], rs, training=case["training"], trace=trace)
            assert game.length == ref["length"] and game.terminal_value == ref["terminal_value"], name
            assert len(trace) == len(ref["moves"])
            for mine, theirs in zip(trace, ref["moves"]):
                for key in ("action", "root_visits", "root_value_sum", "child_actions", "child_visits", "child_priors",
                            "child_value_sums"):
                    assert mine[key] == theirs[key], (name, key)


def _recorded_play(path, seed, config, training, evaluate):
    """Oracle self-play of the game with `seed` on its own map, recording every evaluation as the persistent kernel's
    test hook does: (128-bit digest of the leaf image, probabilities, value), in the order the search consumes them."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from scs_replay import image_mix_digest
    from oracle import search as osearch
    rs = np.random.RandomState(seed)
    cfg = ScsConfig(path, map_seed=rs)
    rec = []

    def ev(game):
        img = game.state_image()[0]
        p, v = evaluate(game, cfg)
        rec.append((image_mix_digest(img), np.asarray(p, np.float32), np.float32(v)))
        return rec[-1][1], rec[-1][2]

    game = ScsGame(cfg)
    osearch.play_game(game, ev, config, rs, training=training)
    return (np.stack([r[0] for r in rec]), np.stack([r[1] for r in rec]), np.array([r[2] for r in rec], np.float32)), game


def test_recorded_leaf_replay_on_per_game_maps():
    """tests/scs_replay.py in per-game mode (how the GPU tests replay the device's games on per-game maps): the
    evaluations of the scs_search_pergame_kat.json.gz games, recorded from the oracle's own play, replay to the genuine
    reference's traces move for move -- and only on the game's own map (the map of another seed fails at the first
    leaf image)."""
    import gzip
    import json
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from scs_eval import evaluate_image
    from scs_replay import replay_game
    with gzip.open(os.path.join(GOLDEN, "scs_search_pergame_kat.json.gz"), "rt") as f:
        kat = json.load(f)
    path = os.path.join(GOLDEN, "scs_configs", "randomized_5x5.yml")
    replayed = 0
    for name, case in kat.items():
        for ref in case["games"]:
            rec, _ = _recorded_play(path, ref["seed"], case["config"], case["training"],
                                    lambda game, cfg: evaluate_image(game.state_image()[0], cfg.num_actions))
            assert len(rec[2]) == ref["evaluations"], name
            job = (path, case["config"], ref["seed"], case["training"]) + rec + (None,)
            out = replay_game(job + ({"per_game": True},))
            assert out["evaluations_used"] == out["evaluations_recorded"] == ref["evaluations"], name
            assert out["length"] == ref["length"] and out["terminal"] and out["terminal_value"] == ref["terminal_value"]
            assert len(out["trace"]) == len(ref["moves"])
            for m, (mine, theirs) in enumerate(zip(out["trace"], ref["moves"])):
                for key in theirs:
                    assert mine[key] == theirs[key], (name, ref["seed"], m, key)
            replayed += 1
            with pytest.raises(AssertionError, match="leaf 0: the oracle's leaf image"):
                replay_game((path, case["config"], ref["seed"] + 1000) + job[3:] + ({"per_game": True},))
    assert replayed == sum(len(c["games"]) for c in kat.values())


def test_recorded_leaf_replay_holds_every_evaluation_to_the_oracle_network():
    """scs_replay's oracle-network option: evaluations the oracle network made on each leaf's own image replay (the
    largest difference is reported), and a game that consumed one evaluation of another position -- what a cache hit
    under a wrong key hands back -- fails at exactly that leaf although every image digest is right."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import torch
    from scs_replay import replay_game
    from nuzero_amd.weights import synthetic_weights, convnet_param_shapes
    from oracle.net import FeedForwardRef
    path = os.path.join(GOLDEN, "scs_configs", "randomized_5x5.yml")
    probe = ScsConfig(path, map_seed=0)
    w = synthetic_weights(3, convnet_param_shapes(probe.channels, probe.planes, 3, 8, 1), 2.0)
    ref = FeedForwardRef(w, "convnet", 1)

    def net(game, cfg):
        p, v = ref.inference(game.state_image(), None)
        return torch.softmax(torch.from_numpy(p.reshape(-1)), 0).numpy(), v.reshape(-1)[0]

    search = {"Simulation": {"mcts_simulations": 8, "keep_subtree": True}, "UCT": {"pb_c_base": 10000, "pb_c_init": 1.15},
              "Exploration": {"number_of_softmax_moves": 0, "epsilon_softmax_exploration": 0.04,
                              "epsilon_random_exploration": 0.001, "value_factor": 1,
                              "root_exploration_distribution": "gamma", "root_exploration_fraction": 0.2,
                              "root_dist_alpha": 0.15, "root_dist_beta": 1}}
    seed = 61
    (dig, probs, values), game = _recorded_play(path, seed, search, True, net)
    opts = {"per_game": True, "oracle_net": (w, "convnet", 1)}
    out = replay_game((path, search, seed, True, dig, probs, values, None, opts))
    assert out["evaluations_used"] == len(values) > 100 and out["length"] == game.length
    assert max(out["oracle_net_worst"]) < 1e-5
    # the same game played with ONE wrong evaluation, leaf k getting leaf k - 1's (a cache hit under a key that missed
    # what tells the two apart): its records are self-consistent, so the digest check alone replays them to the end
    k = next(i for i in range(40, len(values)) if np.max(np.abs(probs[i] - probs[i - 1])) > 1e-3)
    calls = [0]

    def wrong_once(game, cfg):
        calls[0] += 1
        return (probs[k - 1], values[k - 1]) if calls[0] == k + 1 else net(game, cfg)

    bad, _ = _recorded_play(path, seed, search, True, wrong_once)
    assert np.array_equal(bad[0][:k + 1], dig[:k + 1])
    out = replay_game((path, search, seed, True) + bad + (None, {"per_game": True}))
    assert out["evaluations_used"] == len(bad[2])
    with pytest.raises(AssertionError, match=f"leaf {k}: the evaluation the device consumed"):
        replay_game((path, search, seed, True) + bad + (None, opts))
