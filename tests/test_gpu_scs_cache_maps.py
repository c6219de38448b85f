"""The SCS inference cache on per-game maps (nz_scs_search_set_games + nz_scs_search_cache): the table is shared by the
engine's games, and two games on different maps reach equal ScsStates (every game starts from one) whose network inputs
differ in the terrain and victory-point planes.  The reference's KeylessCache hashes the state TENSOR, so it never hands
one map's evaluation to another; the device key must therefore cover the map as well as the state.  Checked here:
  * cache on == cache off, bit for bit, on both routes, with tables small enough to be replaced all the time, on maps
    that differ in a single field, across refills (a slot's next game brings its own map) and across rounds;
  * every evaluation the persistent kernel consumed, cache hits included, against the oracle network on the game's own
    image (tests/scs_replay.py with an oracle network);
  * games on EQUAL maps still share entries (the key is the map's content, not the game's row).
Needs a GPU."""
import copy
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, "golden")
PATH5 = os.path.join(GOLDEN, "scs_configs", "randomized_5x5.yml")
PATH10 = os.path.join(GOLDEN, "scs_configs", "randomized_10x10.yml")

from test_gpu_scs_configs import a1_search, _net, _same_games   # noqa: E402

SIMS = 30


def _play(cfg, net, seeds, route, entries, max_moves=None):
    """play_native of len(seeds) games on `route` (1 persistent, 0 wave by wave, -1 the default) with a table of
    `entries` (0: no cache).  Returns (export, cache statistics or None)."""
    from nuzero_amd.scs import ScsSelfPlay
    sp = ScsSelfPlay(cfg, a1_search(SIMS), len(seeds))
    sp.persistent(route)
    if entries:
        sp.cache(entries)
    r = sp.play_native(net, seeds, max_moves=max_moves)
    if route >= 0:
        assert sp.persistent() is bool(route)
    st = sp.cache_stats() if entries else None
    sp.close()
    return r, st


def _cache_neutral(cfg, net, seeds, route, entries, label, max_moves=None):
    """Cache on == cache off (every root statistic of every move), and the statistics add up."""
    ra, _ = _play(cfg, net, seeds, route, 0, max_moves)
    rb, st = _play(cfg, net, seeds, route, entries, max_moves)
    G = len(seeds)
    _same_games(ra, rb, [(g, g) for g in range(G)], label)
    assert rb["expansions"] == ra["expansions"] == st["hits"] + st["misses"], (label, st)
    assert st["size"] == entries
    print(f"[{label}] hits {st['hits']} misses {st['misses']} of {ra['expansions']} expansions", flush=True)
    return ra, rb, st


@pytest.mark.parametrize("entries", [64, 1 << 16])
@pytest.mark.parametrize("route", [1, 0])
def test_cache_is_results_neutral_on_per_game_maps(route, entries):
    """48 games, each on its own randomized 5 x 5 map, both routes; 64 entries force constant replacement."""
    from nuzero_amd.scs import ScsGameConfig
    cfg = ScsGameConfig(PATH5, per_game=True)
    G = 48
    net, _ = _net(cfg, "convnet", 32, 3, seed=71, gain=2.0, max_batch=G)
    _cache_neutral(cfg, net, list(range(3100, 3100 + G)), route, entries, f"randomized5 route {route} entries {entries}")
    net.close()


@pytest.mark.parametrize("arch", ["convnet", "recurrent"])
def test_cache_is_results_neutral_on_per_game_10x10_maps(arch):
    """Boards over 32 cells only take the wave-by-wave route: 16 games on their own randomized 10 x 10 maps, with a
    feed-forward and a recurrent network (the first 40 decisions of each game: the openings are where games meet)."""
    from nuzero_amd.scs import ScsGameConfig
    cfg = ScsGameConfig(PATH10, per_game=True)
    G = 16
    net, _ = _net(cfg, arch, 32, 2 if arch == "recurrent" else 3, seed=73, gain=2.0, iters=2, max_batch=G)
    _cache_neutral(cfg, net, list(range(3300, 3300 + G)), 0, 1 << 16, f"randomized10 {arch}", max_moves=40)
    net.close()


def _one_field_variants(cfg, seed):
    """Game 0's map and stream drawn from `seed`, then rows that share that stream and differ from row 0 in ONE field of
    the map: 1 a tile's attack modifier, 2 a tile's defense modifier, 3 a tile's movement cost (>= 1), 4 one of player
    0's victory points moved to another tile, 5 player 1's victory points only, 6 an exact copy of row 0."""
    terrain, vp, keys, pos, streams = type(cfg).draw_games(cfg, [seed])
    n = 7
    t, v = np.repeat(terrain, n, 0), np.repeat(vp, n, 0)
    tile = cfg.rows * cfg.cols // 2
    t[1, tile, 0] += 0.5
    t[2, tile, 1] += 0.5
    t[3, tile, 2] = 1.0 if t[0, tile, 2] != 1.0 else 2.0
    n0 = cfg.n_vp[0]

    def moved(points, i, col_range):
        taken = {tuple(p) for p in points.tolist()}
        r0, c0 = points[i]
        for dr in range(1, cfg.rows):
            for c in col_range:
                cand = ((r0 + dr) % cfg.rows, c)
                if cand not in taken:
                    return cand
        raise AssertionError("no free tile for a victory point")

    v[4, 0] = moved(v[4], 0, [int(v[0, 0, 1])])
    v[5, n0] = moved(v[5], n0, [int(v[0, n0, 1])])
    return (t, v, np.repeat(keys, n, 0), np.repeat(pos, n, 0), [copy.deepcopy(streams[0]) for _ in range(n)])


@pytest.mark.parametrize("route", [1, 0])
def test_cache_tells_maps_apart_that_differ_in_one_field(route):
    """Rows 1-5 share long openings with row 0 (same stream, maps one field apart): a key that misses any field the
    image reads hands them row 0's evaluations.  Row 6 (a copy of row 0) plays exactly row 0's game."""
    from nuzero_amd.scs import ScsGameConfig
    cfg = ScsGameConfig(PATH5, per_game=True)
    rows = _one_field_variants(cfg, 3500)
    assert len({(t.tobytes(), v.tobytes()) for t, v in zip(rows[0], rows[1])}) == 6
    cfg.draw_games = lambda seeds: rows
    net, _ = _net(cfg, "convnet", 32, 3, seed=75, gain=2.0, max_batch=7)
    ra, rb, st = _cache_neutral(cfg, net, [3500] * 7, route, 1 << 16, f"one field route {route}")
    for r in (ra, rb):
        _same_games(r, r, [(6, 0)], "copy of row 0")
        for g in range(1, 6):       # the changed field reaches the network input: the first priors differ
            c = r["n_children"][0, 0]
            assert not np.array_equal(r["child_prior"][g, 0, :c], r["child_prior"][0, 0, :c]), g
    assert st["hits"] > 0           # (row 6 on row 0's entries at least)
    net.close()


def test_recorded_evaluations_equal_the_oracle_network_on_each_games_own_image():
    """Persistent route, 64-entry table, every game recorded (nz_scs_search_record: every evaluation the search
    consumed, hits included): each game replays on the oracle on its own map with every evaluation within 1e-5 of the
    oracle network on that game's own image, and every root statistic equals the device's bit for bit.  Games 12-15
    repeat the seeds (hence the maps) of games 0-3, so hits that are legitimate happen as well."""
    from nuzero_amd.scs import ScsSelfPlay, ScsGameConfig
    from scs_replay import replay_games, assert_trace_equals_device
    cfg = ScsGameConfig(PATH5, per_game=True)
    G = 16
    net, w = _net(cfg, "convnet", 32, 3, seed=71, gain=2.0, max_batch=G)
    search = a1_search(SIMS)
    seeds = list(range(3700, 3712)) + list(range(3700, 3704))
    sp = ScsSelfPlay(cfg, search, G)
    sp.persistent(1)
    sp.cache(64)
    sp.record(range(G), SIMS * (sp.MAX_MOVES + 1))
    r = sp.play_native(net, seeds)
    assert sp.persistent() is True
    recs = sp.records()
    st = sp.cache_stats()
    sp.close(); net.close()
    assert r["expansions"] == sum(len(v[2]) for v in recs.values()) == st["hits"] + st["misses"]
    assert st["hits"] > 0
    print(f"[recorded persistent entries 64] hits {st['hits']} misses {st['misses']}", flush=True)
    opts = {"per_game": True, "oracle_net": (w, "convnet", 3)}
    outs = replay_games([(PATH5, search, seeds[g], True) + recs[g] + (None, opts) for g in range(G)])
    moves = 0
    for g, out in enumerate(outs):
        assert out["evaluations_used"] == out["evaluations_recorded"], g
        assert out["length"] == r["lengths"][g] and out["terminal"] and out["terminal_value"] == r["outcomes"][g], g
        assert max(out["oracle_net_worst"]) < 1e-5, (g, out["oracle_net_worst"])
        moves += assert_trace_equals_device(r, g, out, "recorded")
    assert moves == int(r["lengths"].sum())


@pytest.mark.parametrize("route", [1, 0])
def test_refill_switches_maps_under_the_cache(route):
    """A round of 48 games over 16 slots with the cache on: a slot's next game reads its own map row mid-round.  The
    round equals the same round without the cache and play_native with one slot per game."""
    from nuzero_amd.scs import ScsSelfPlay, ScsGameConfig
    cfg = ScsGameConfig(PATH5, per_game=True)
    N, S = 48, 16
    net, _ = _net(cfg, "convnet", 32, 3, seed=71, gain=2.0, max_batch=N)
    seeds = list(range(3900, 3900 + N))
    rounds = []
    for entries in (1 << 16, 0):
        sp = ScsSelfPlay(cfg, a1_search(SIMS), S)
        sp.persistent(route)
        if entries:
            sp.cache(entries)
        rounds.append(sp.play_round(net, seeds))
        assert sp.persistent() is bool(route)
        if entries:
            st = sp.cache_stats()
        sp.close()
    rn, _ = _play(cfg, net, seeds, route, 0)
    net.close()
    _same_games(rounds[0], rounds[1], [(g, g) for g in range(N)], "refill cache on / off")
    _same_games(rounds[0], rn, [(g, g) for g in range(N)], "refill / one slot per game")
    assert rounds[0]["expansions"] == rounds[1]["expansions"] == st["hits"] + st["misses"]
    print(f"[refill route {route}] hits {st['hits']} misses {st['misses']}", flush=True)


def test_table_kept_across_rounds_on_per_game_maps():
    """Seeds A, then seeds B on the kept table (no cache_clear): round B equals an uncached round B.  Then A again on
    the kept table: more hits than A's first round, the same games."""
    from nuzero_amd.scs import ScsSelfPlay, ScsGameConfig
    cfg = ScsGameConfig(PATH5, per_game=True)
    G = 48
    net, _ = _net(cfg, "convnet", 32, 3, seed=71, gain=2.0, max_batch=G)
    A, B = list(range(4100, 4100 + G)), list(range(4200, 4200 + G))
    plain_a, _ = _play(cfg, net, A, -1, 0)
    plain_b, _ = _play(cfg, net, B, -1, 0)
    sp = ScsSelfPlay(cfg, a1_search(SIMS), G)
    sp.cache(1 << 18)
    hits = []
    for seeds, plain, label in ((A, plain_a, "A"), (B, plain_b, "B"), (A, plain_a, "A again")):
        before = sp.cache_stats()["hits"]
        r = sp.play_native(net, seeds)
        hits.append(sp.cache_stats()["hits"] - before)
        _same_games(plain, r, [(g, g) for g in range(G)], label)
        assert r["expansions"] == plain["expansions"], label
    print(f"[kept table] hits per round A {hits[0]} B {hits[1]} A again {hits[2]}", flush=True)
    assert hits[2] > hits[0] and hits[2] > plain_a["expansions"] // 4
    sp.close(); net.close()


def test_games_on_equal_maps_share_entries():
    """The key is the map's CONTENT: a round where every row holds the same map (streams from distinct seeds) hits
    clearly more often than the same seeds on their own maps -- games on equal maps share positions, as with the
    reference's tensor-hashed cache.  The shared-map round is also results-neutral."""
    from nuzero_amd.scs import ScsGameConfig
    cfg = ScsGameConfig(PATH5, per_game=True)
    G = 48
    seeds = list(range(4400, 4400 + G))
    own = type(cfg).draw_games(cfg, seeds)

    def shared_map(s):
        assert list(s) == seeds
        t, v, keys, pos, streams = own
        return (np.repeat(t[:1], G, 0), np.repeat(v[:1], G, 0), keys, pos, streams)

    net, _ = _net(cfg, "convnet", 32, 3, seed=71, gain=2.0, max_batch=G)
    _, st_own = _play(cfg, net, seeds, -1, 1 << 16)
    cfg.draw_games = shared_map
    _, _, st_shared = _cache_neutral(cfg, net, seeds, -1, 1 << 16, "one map for all rows")
    net.close()
    print(f"[equal maps] hits {st_shared['hits']} against {st_own['hits']} on own maps", flush=True)
    # (measured: 11,327 against 8,300 -- the own-map hits are a game meeting its own positions again; a key on the
    # row rather than the map's content would leave the shared-map round at about that count too)
    assert st_shared["hits"] > 1.15 * st_own["hits"]
