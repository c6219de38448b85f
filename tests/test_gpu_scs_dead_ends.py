"""Every route of the SCS search against the oracle at live positions without a legal action ("Dead ends").
Cases and what the oracle alone shows of them: tests/scs_dead_ends.py, tests/test_scs_dead_ends_host.py.

  (a) host-evaluator route (ScsSelfPlay.search / apply, wave_kernel): every case, replayed on the oracle from the
      evaluations the device consumed -- re-evaluations of a dead-end node included --, the leaf mask of every leaf;
  (b) library routes through ScsMatch from the cases' positions (evaluation engines; a training search cannot start from a
      position on these routes): the persistent route recording its own evaluations, the wave-by-wave route bit-equal to
      it; on two_types_6x5, which the persistent route refuses, the wave-by-wave route against the host-evaluator route;
  (c) both with the inference cache at 64 and 65536 entries;
  (d) the arena's exact size for a game that plays on past dead ends;
  (e) a root without a legal action: flag 128, naming game and decision, beside a game that plays on.

Every comparison with the oracle is exact; the recorded evaluations are held to the float64 oracle network at 1e-5
(worst measured on an MI355X: 2.6e-9 on the probabilities, 1.1e-7 on the values).  Wall time on an MI355X: 1.9 s for
the first test (start-up), under 0.2 s for every other, 5.9 s for the file.  Needs a GPU."""
import os
import re
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
pytestmark = pytest.mark.gpu

import scs_dead_ends as de                                          # noqa: E402
import scs_directed as sd                                           # noqa: E402
from scs_dead_ends import PLAYS_ON, REACHES, STARTS_ON              # noqa: E402
from scs_replay import LeafRecorder, ORACLE_NET_TOL, assert_trace_equals_device      # noqa: E402
from test_gpu_scs_replay_compact import _net                        # noqa: E402

NO_LEGAL = "game {g}, decision {d}: the position has no legal action"


def _device_config(name):
    from nuzero_amd.scs import ScsGameConfig
    return ScsGameConfig(sd.config_path(name))


def _start(prefixes):
    start = np.zeros((len(prefixes), max(len(p) for p in prefixes)), np.int32)
    for i, p in enumerate(prefixes):
        start[i, :len(p)] = p
    return start, np.array([len(p) for p in prefixes], np.int32)


def _same_games(ra, rb, games, label):
    """_same_games of tests/test_gpu_scs_configs.py for games started behind an opening: the opening's plies hold actions
    only (their search records are not defined), so everything else is compared from the first searched decision on."""
    for g_a, g_b in games:
        n = ra["lengths"][g_a]
        assert n == rb["lengths"][g_b] and ra["outcomes"][g_a] == rb["outcomes"][g_b], (label, g_a)
        assert np.array_equal(ra["actions"][g_a, :n], rb["actions"][g_b, :n]), (label, g_a)
        first = int(np.flatnonzero(ra["n_children"][g_a, :n] > 0)[0]) if (ra["n_children"][g_a, :n] > 0).any() else n
        assert first == (int(np.flatnonzero(rb["n_children"][g_b, :n] > 0)[0]) if (rb["n_children"][g_b, :n] > 0).any() else n)
        for k in ("tree_size", "n_children", "bias", "root_value_sum"):
            assert np.array_equal(ra[k][g_a, first:n], rb[k][g_b, first:n]), (label, k, g_a)
        for m in range(first, n):
            c = ra["n_children"][g_a, m]
            for k in ("child_action", "child_visit", "child_prior", "child_value_sum"):
                assert np.array_equal(ra[k][g_a, m, :c], rb[k][g_b, m, :c]), (label, k, g_a, m)


def _flag(err):
    from nuzero_amd import _lib
    assert err.code == _lib.NZ_ERR_OVERFLOW, err
    return [int(f) for f in re.findall(r"flag (\d+)", str(err))]


def _image_evaluator(fn, num_actions):
    import torch

    def ev(images):
        out = [fn(im, num_actions) for im in images.cpu().numpy()]
        return (torch.from_numpy(np.stack([o[0] for o in out])).to(images.device),
                torch.from_numpy(np.array([o[1] for o in out], np.float32)).to(images.device))
    return ev


def _evaluator(evaluation, cfg, G):
    """(evaluator for ScsSelfPlay.search, the BoardNet behind it or None)."""
    from scs_eval import evaluate_image, evaluate_image_peaked
    if evaluation == "net":
        net = _net(cfg, G)
        return net.evaluator(fixed_batch=G), net
    return _image_evaluator({"flat": evaluate_image, "peaked": evaluate_image_peaked}[evaluation], cfg.num_actions), None


class HostRun:
    """Games on one ScsSelfPlay handle, moved as ScsSelfPlay.play moves them (root noise and select_action's uniforms
    drawn per game in the reference's order) from given positions, every consumed evaluation recorded with the leaf
    mask the search stored for it."""

    def __init__(self, name, cases, evaluation, nodes_per_game=None):
        from nuzero_amd.scs import ScsSelfPlay
        assert len({(c.sims, c.training) for c in cases}) == 1
        self.cases, self.cfg = cases, _device_config(name)
        self.search = de.search_config(cases[0].sims)
        self.sp = ScsSelfPlay(self.cfg, self.search, len(cases), training=cases[0].training, nodes_per_game=nodes_per_game)
        ev, self.net = _evaluator(evaluation, self.cfg, len(cases))
        self.rec = LeafRecorder(ev)
        self.masks = {g: [] for g in range(len(cases))}            # per game, per consumed evaluation: legal actions
        self.images = {g: [] for g in range(len(cases))}
        self.reset()

    def reset(self):
        self.sp.reset_to(*_start([de.prefix_of(c) for c in self.cases]))
        self.rngs = [np.random.RandomState(int(c.seed)) for c in self.cases]
        self.rec.records.clear()
        for g in self.masks:
            self.masks[g], self.images[g] = [], []

    def _leaves(self, images):
        sp = self.sp
        games = sp._leaf_game[:images.shape[0]]
        masks, ims = sp.leaf_masks(), images.cpu().numpy()
        for i, g in enumerate(games.cpu().numpy()):
            self.masks[int(g)].append(int(masks[g].sum()))
            self.images[int(g)].append(ims[i].copy())
        return self.rec(images, games)

    def move(self):
        """One searched move of every live game; returns the NzError of ending it, or None."""
        from nuzero_amd import _lib
        import torch
        from ctypes import c_void_p
        sp, ex, G = self.sp, self.search["Exploration"], len(self.cases)
        st = sp.status()
        noise = uni = None
        if sp.training:
            nchild = torch.empty((G,), dtype=torch.int32, device=sp.device)
            sp._check(_lib.lib.nz_scs_search_root_children(sp._h, c_void_p(nchild.data_ptr()), sp._stream()))
            nchild = nchild.cpu().numpy()
            noise, uni = np.zeros((G, sp.MAX_CHILDREN), np.float64), np.zeros((G, 3), np.float64)
            for g in range(G):
                if st[g, 4]:
                    continue
                rs, n = self.rngs[g], int(nchild[g])
                noise[g, :n] = rs.gamma(ex["root_dist_alpha"], ex["root_dist_beta"], n)
                assert st[g, 6] >= ex["number_of_softmax_moves"]
                u1, u2 = rs.random_sample(), rs.random_sample()
                uni[g, 0], uni[g, 1] = u1, u2
                if u1 < ex["epsilon_softmax_exploration"] or u2 < ex["epsilon_random_exploration"]:
                    uni[g, 2] = rs.random_sample()
        sp.search(self._leaves, noise)
        try:
            sp.apply(uniforms=uni)
        except _lib.NzError as e:
            return e
        return None

    def close(self):
        self.sp.close()
        if self.net is not None:
            self.net.close()


def _replay(case, arrays):
    out = de.run_case(case, recorded=arrays)
    assert out["evaluations_used"] == out["evaluations_recorded"], de.case_id(case)
    return out


def _check_leaves(run, g, out, label):
    """Every consumed leaf of game g: the stored mask has the oracle's number of legal actions -- none at a dead end --
    and a dead-end leaf's image is the oracle's."""
    assert len(run.masks[g]) == len(out["evaluations"]), label
    for i, e in enumerate(out["evaluations"]):
        assert run.masks[g][i] == e["n_legal"], (label, i)
        if e["dead_end"]:
            assert run.masks[g][i] == 0 and np.array_equal(run.images[g][i], e["image"]), (label, i)


# ---- (a) the host-evaluator route ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", de.CASES, ids=[de.case_id(c) for c in de.CASES])
def test_host_evaluator_route_equals_the_oracle_next_to_dead_ends(case):
    """One game per case, searched for case.moves moves or until a move ends on a root without children.  The oracle
    replays from the recorded evaluations; their number is the oracle's own count for the case, re-evaluations included."""
    t0 = time.perf_counter()
    label = de.case_id(case)
    run = HostRun(case.walk.name, [case], case.evaluation)
    first = len(de.prefix_of(case))
    err, played = None, 0
    for _ in range(case.moves):
        err = run.move()
        if err is not None:
            break
        played += 1
    r = run.sp.export()
    st = run.sp.status()
    out = _replay(case, run.rec.arrays(0))
    assert de.ending_of(out) == case.ending and len(out["trace"]) == played, label
    pure = de.oracle_run(case)
    if case.evaluation != "net":                          # (the same evaluator on both sides: the same search)
        assert out["evaluations_recorded"] == len(pure["evaluations"]), label
    assert out["situations"]["dead_end_evaluations"] > 0, label
    for key in ("dead_end_evaluations", "re_evaluations"):
        if case.evaluation != "net":
            assert out["situations"][key] == pure["situations"][key], (label, key)
    assert assert_trace_equals_device(r, 0, out, label, first=first) == played
    assert r["lengths"][0] == first + played and r["actions"][0, :first].tolist() == de.prefix_of(case), label
    assert r["simulations"] == out["simulations"] and r["expansions"] == out["expansions"], label
    _check_leaves(run, 0, out, label)
    if case.ending[0] == PLAYS_ON:
        assert err is None, label
    else:
        assert err is not None and _flag(err) == [128], (label, err)
        assert NO_LEGAL.format(g=0, d=first + played) in str(err), err
        assert st[0, 4] == 0 and st[0, 6] == first + played, label       # not terminal, nothing played
        if case.training:                                 # the stream stands where the oracle's stood when it raised
            want, got = out["rng_state"], run.rngs[0].get_state()
            assert np.array_equal(want[1], got[1]) and want[2:] == got[2:], label
    run.close()
    print(f"wall time {label}: {time.perf_counter() - t0:.2f} s")


# ---- (b), (c) the library routes ----------------------------------------------------------------------------------------
LIBRARY_CASES = [c for c in de.CASES if c.evaluation == "net" and not c.training and c.back > 0]
WAVE_ONLY_CASES = [c._replace(evaluation="net") for c in de.CASES if c.walk.name == "two_types_6x5" and not c.training and c.back > 0]
_WORST = [0.0, 0.0]


def _match_play(m, nets, case, route, record):
    """One ScsMatch round from the case's position on `route` (1 persistent, 0 wave by wave); -> (error or None, agent 1's
    export, its records or None, its cache hits in this round)."""
    from nuzero_amd._lib import NzError
    start, n_plies = _start([de.prefix_of(case)])
    for a in m.agents:
        a.persistent(route)
        a.record(range(1) if record else [], case.sims * (case.moves + 1) if record else 0)
    hits = m.agents[0].cache_stats()["hits"]
    err = None
    try:
        m.play(nets[0], nets[1], max_moves=case.moves, start_actions=start, n_plies=n_plies)
    except NzError as e:
        err = e
    for a in m.agents:
        assert a.persistent() is bool(route)
    recs = m.agents[0].records()[0] if record else None
    ex = [a.export() for a in m.agents]
    n = ex[0]["lengths"][0]
    assert n == ex[1]["lengths"][0]
    _same_games(ex[0], ex[1], [(0, 0)], de.case_id(case))             # both agents searched the same positions alike
    return err, ex[0], recs, m.agents[0].cache_stats()["hits"] - hits


def _check_dead_end_error(err, case, out, label):
    first = out["first"]
    if case.ending[0] == PLAYS_ON:
        assert err is None, (label, err)
    else:
        assert err is not None and _flag(err) == [128, 128], (label, err)
        assert NO_LEGAL.format(g=0, d=first + len(out["trace"])) in str(err), err


def _within_tolerance_of_float64(cfg_name, out, recs, label):
    """Every recorded leaf against the float64 oracle network on the oracle's own image of it."""
    import torch
    from scipy.special import softmax
    r64 = de.oracle_net(sd.new_game(cfg_name).cfg, torch.float64)
    done = {}
    for i, e in enumerate(out["evaluations"]):
        key = e["image"].tobytes()
        if key not in done:
            logits, v = r64.inference(e["image"][None], None)
            done[key] = (softmax(np.asarray(logits).reshape(-1)), float(np.asarray(v).reshape(-1)[0]))
        dp = float(np.max(np.abs(done[key][0] - recs[1][i])))
        dv = abs(done[key][1] - float(recs[2][i]))
        _WORST[0], _WORST[1] = max(_WORST[0], dp), max(_WORST[1], dv)
        assert dp < ORACLE_NET_TOL and dv < ORACLE_NET_TOL, (label, i, dp, dv)
    print(f"{label}: worst recorded-leaf error against the float64 network so far: probabilities {_WORST[0]:.3g}, "
          f"values {_WORST[1]:.3g}")


@pytest.mark.parametrize("cache", [0, 64, 1 << 16])
@pytest.mark.parametrize("case", LIBRARY_CASES, ids=[de.case_id(c) for c in LIBRARY_CASES])
def test_library_routes_equal_the_oracle_next_to_dead_ends(case, cache):
    """The persistent route records its own evaluations; the oracle replays from them, the wave-by-wave route plays the
    same game bit for bit, the counters are the oracle's.  With a cache the game is the uncached one (the oracle's replay
    is its own check of that), and a table that holds every position hits at least once per re-evaluation of a dead end
    (none in the case that plays on for four moves; tests/test_scs_dead_ends_host.py holds the library cases together
    to at least 50)."""
    from nuzero_amd.tester import ScsMatch
    t0 = time.perf_counter()
    label = f"{de.case_id(case)}-cache{cache}"
    cfg = _device_config(case.walk.name)
    search = de.search_config(case.sims)
    nets = (_net(cfg, 1), _net(cfg, 1))
    m = ScsMatch(cfg, search, search, 1)
    for a in m.agents:
        a.cache(cache)
    first = len(de.prefix_of(case))
    err_p, rp, recs, hits_p = _match_play(m, nets, case, 1, True)
    out = _replay(case, recs)
    assert de.ending_of(out) == case.ending, label
    assert out["situations"]["dead_end_evaluations"] > 0, label
    played = len(out["trace"])
    assert assert_trace_equals_device(rp, 0, out, label, first=first) == played and rp["lengths"][0] == first + played
    assert rp["simulations"] == out["simulations"] and rp["expansions"] == out["expansions"], label
    _check_dead_end_error(err_p, case, out, label)
    _within_tolerance_of_float64(case.walk.name, out, recs, label)
    for a in m.agents:
        a.cache_clear()
    err_w, rw, _, hits_w = _match_play(m, nets, case, 0, False)
    _same_games(rp, rw, [(0, 0)], label)
    assert rw["simulations"] == rp["simulations"] and rw["expansions"] == rp["expansions"], label
    _check_dead_end_error(err_w, case, out, label)
    if cache == 1 << 16:
        again = out["situations"]["dead_end_re_evaluations"]
        assert hits_p >= again and hits_w >= again, (label, again, hits_p, hits_w)
    if cache == 0:
        assert hits_p == 0 and hits_w == 0
    m.close()
    for n in nets:
        n.close()
    print(f"wall time {label}: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("cache", [0, 64, 1 << 16])
@pytest.mark.parametrize("case", WAVE_ONLY_CASES, ids=[de.case_id(c) for c in WAVE_ONLY_CASES])
def test_wave_route_equals_the_oracle_next_to_dead_ends_where_the_persistent_route_refuses(case, cache):
    """two_types_6x5 (105 input planes on 30 cells): the persistent route says so before anything is launched; the
    wave-by-wave route plays the game of the host-evaluator route with the same network, which the oracle replays."""
    from nuzero_amd._lib import NzError
    from nuzero_amd.tester import ScsMatch
    t0 = time.perf_counter()
    label = f"{de.case_id(case)}-cache{cache}"
    run = HostRun(case.walk.name, [case], "net")
    first = len(de.prefix_of(case))
    for _ in range(case.moves):
        if run.move() is not None:
            break
    rh = run.sp.export()
    out = _replay(case, run.rec.arrays(0))
    played = len(out["trace"])
    assert out["situations"]["dead_end_evaluations"] > 0, label
    assert assert_trace_equals_device(rh, 0, out, label, first=first) == played
    _within_tolerance_of_float64(case.walk.name, out, run.rec.arrays(0), label)
    cfg, search = run.cfg, run.search
    nets = (run.net, _net(cfg, 1))
    m = ScsMatch(cfg, search, search, 1)
    for a in m.agents:
        a.persistent(1)
    with pytest.raises(NzError, match="persistent route requested but not available"):
        m.play(nets[0], nets[1], max_moves=case.moves, start_actions=_start([de.prefix_of(case)])[0])
    for a in m.agents:
        a.cache(cache)
    err, rw, _, hits = _match_play(m, nets, case, 0, False)
    _same_games(rh, rw, [(0, 0)], label)
    assert rw["simulations"] == out["simulations"] and rw["expansions"] == out["expansions"], label
    if de.ending_of(out)[0] == PLAYS_ON:
        assert err is None, err
    else:
        assert err is not None and _flag(err) == [128, 128] and NO_LEGAL.format(g=0, d=first + played) in str(err), err
    if cache == 1 << 16:
        again = out["situations"]["dead_end_re_evaluations"]
        assert hits >= again, (label, again, hits)
    m.close(); nets[1].close(); run.close()
    print(f"wall time {label}: {time.perf_counter() - t0:.2f} s")


# ---- (d) the arena ------------------------------------------------------------------------------------------------------
ARENA_CASE = next(c for c in de.CASES if c.evaluation == "net" and not c.training and c.ending[0] == PLAYS_ON)


@pytest.mark.parametrize("route", ["host-evaluator", "wave", "persistent"])
def test_dead_end_expansions_add_no_node_to_the_arena(route):
    """The rule of tests/test_gpu_scs_deep_paths.py on a game that plays on past dead ends: N = the oracle's largest
    live tree over the moves played (1 + the children of every expanded node; a dead-end expansion adds none).  With
    nodes_per_game = 2 N the game is the default arena's, with 2 N - 2 the play ends with flag 1 (on the persistent route
    together with flag 4: the leader leaves with simulations to go)."""
    from nuzero_amd._lib import NzError
    from nuzero_amd.scs import ScsSelfPlay
    from nuzero_amd.tester import ScsMatch
    t0 = time.perf_counter()
    case = ARENA_CASE
    first = len(de.prefix_of(case))
    cfg, search = _device_config(case.walk.name), de.search_config(case.sims)

    def play(nodes_per_game):
        if route == "host-evaluator":
            run = HostRun(case.walk.name, [case], "net", nodes_per_game=nodes_per_game)
            try:
                for _ in range(case.moves):
                    err = run.move()
                    if err is not None:
                        raise err
                return run.sp.export(), run.rec.arrays(0)
            finally:
                run.close()
        nets = (_net(cfg, 1), _net(cfg, 1))
        m = ScsMatch(cfg, search, search, 1)
        if nodes_per_game is not None:
            for a in m.agents:
                a.close()
            m.agents = tuple(ScsSelfPlay(cfg, search, 1, training=False, nodes_per_game=nodes_per_game) for _ in range(2))
        try:
            err, r, recs, _ = _match_play(m, nets, case, 1 if route == "persistent" else 0, route == "persistent")
            if err is not None:
                raise err
            return r, recs
        finally:
            m.close()
            for n in nets:
                n.close()

    r0, recs = play(None)
    if recs is None:                                      # the wave-by-wave route records nothing: the persistent one's game
        m_recs = HostRun(case.walk.name, [case], "net")
        for _ in range(case.moves):
            assert m_recs.move() is None
        recs = m_recs.rec.arrays(0)
        _same_games(m_recs.sp.export(), r0, [(0, 0)], route)
        m_recs.close()
    out = _replay(case, recs)
    assert de.ending_of(out) == case.ending and out["situations"]["dead_end_evaluations"] > 0
    assert assert_trace_equals_device(r0, 0, out, route, first=first) == case.moves
    n = max(out["live_nodes"])
    assert n == out["peak_nodes"] and n > case.sims
    fits, _ = play(2 * n)
    _same_games(r0, fits, [(0, 0)], route)
    with pytest.raises(NzError) as full:
        play(2 * n - 2)
    flags = _flag(full.value)
    assert flags and all(f & 1 for f in flags), full.value
    if route == "persistent":
        assert all(f & 4 for f in flags) and not any(f & 128 for f in flags), full.value
    print(f"wall time arena-{route}: {time.perf_counter() - t0:.2f} s")


# ---- (e) a root without a legal action, beside a game that plays on -----------------------------------------------------
ROOT_CASES = {False: (de.Case(de.O49, 1, 32, False, 0, 2, "net", (REACHES, 1)), de.Case(de.O49, 3, 32, False, 0, 2, "net", (PLAYS_ON, 2))),
              True: (de.Case(de.O20, 1, 32, True, 21, 2, "flat", (REACHES, 1)), de.Case(de.O20, 3, 32, True, 22, 2, "flat", (PLAYS_ON, 2)))}


@pytest.mark.parametrize("training", [False, True], ids=["evaluation-net", "training-flat"])
def test_host_route_names_the_game_whose_root_has_no_legal_action(training):
    """Game 0 steps onto the dead end with its first move, game 1 plays on.  The second move's searches run (game 0:
    `sims` evaluations of its root), ending it fails with flag 128 naming game 0 and its decision, game 1 has completed
    both moves and game 0 its one; the training game's stream stands where the oracle's stood when it raised.  After
    reset_to the handle plays the first move of a fresh handle."""
    t0 = time.perf_counter()
    cases = ROOT_CASES[training]
    run = HostRun(cases[0].walk.name, list(cases), cases[0].evaluation)
    assert run.move() is None
    err = run.move()
    firsts = [len(de.prefix_of(c)) for c in cases]
    assert err is not None and _flag(err) == [128] and NO_LEGAL.format(g=0, d=firsts[0] + 1) in str(err), err
    r = run.sp.export()
    outs = [_replay(c, run.rec.arrays(g)) for g, c in enumerate(cases)]
    for g, (c, out) in enumerate(zip(cases, outs)):
        assert de.ending_of(out) == c.ending, g
        assert assert_trace_equals_device(r, g, out, "root", first=firsts[g]) == len(out["trace"]) == (1, 2)[g]
        assert r["lengths"][g] == firsts[g] + len(out["trace"])
        _check_leaves(run, g, out, ("root", g))
        if training:
            want, got = out["rng_state"], run.rngs[g].get_state()
            assert np.array_equal(want[1], got[1]) and want[2:] == got[2:], g
    assert [e["dead_end"] for e in outs[0]["evaluations"][-cases[0].sims:]] == [True] * cases[0].sims
    assert r["simulations"] == sum(o["simulations"] for o in outs) and r["expansions"] == sum(o["expansions"] for o in outs)
    # the same handle after reset_to, against a fresh one
    run.reset()
    assert run.move() is None
    again = run.sp.export()
    fresh = HostRun(cases[0].walk.name, list(cases), cases[0].evaluation)
    assert fresh.move() is None
    _same_games(again, fresh.sp.export(), [(0, 0), (1, 1)], "reset_to")
    assert again["lengths"].tolist() == [f + 1 for f in firsts]
    for g in range(2):
        assert assert_trace_equals_device(again, g, {"trace": outs[g]["trace"][:1]}, "reset_to", first=firsts[g]) == 1
    fresh.close(); run.close()
    print(f"wall time root-host-{training}: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("route", ["wave", "persistent"])
def test_match_names_the_game_whose_root_has_no_legal_action(route):
    """The two evaluation games above through ScsMatch.play(..., start_actions=...) on a library route: the round fails
    with flag 128 on both agents, naming match 0 and its decision; both agents' records up to the last completed move
    are the oracle's; the next round on the same handles is a fresh handle's."""
    from nuzero_amd._lib import NzError
    from nuzero_amd.tester import ScsMatch
    t0 = time.perf_counter()
    cases = ROOT_CASES[False]
    cfg, search = _device_config(cases[0].walk.name), de.search_config(cases[0].sims)
    nets = (_net(cfg, 2), _net(cfg, 2))
    start, n_plies = _start([de.prefix_of(c) for c in cases])
    firsts = n_plies.tolist()
    persist = 1 if route == "persistent" else 0

    def handles():
        m = ScsMatch(cfg, search, search, 2)
        for a in m.agents:
            a.persistent(persist)
        return m
    m = handles()
    m.agents[0].persistent(1)                             # the records come from a persistent agent 1 on either route
    m.agents[0].record(range(2), cases[0].sims * 3)
    with pytest.raises(NzError) as raised:
        m.play(nets[0], nets[1], max_moves=2, start_actions=start, n_plies=n_plies)
    err = raised.value
    assert _flag(err) == [128, 128] and NO_LEGAL.format(g=0, d=firsts[0] + 1) in str(err), err
    recs = m.agents[0].records()
    m.agents[0].record([], 0)
    outs = [_replay(c, recs[g]) for g, c in enumerate(cases)]
    for a in m.agents:
        ex = a.export()
        for g, (c, out) in enumerate(zip(cases, outs)):
            assert de.ending_of(out) == c.ending, g
            assert assert_trace_equals_device(ex, g, out, route, first=firsts[g]) == len(out["trace"]) == (1, 2)[g]
            assert ex["lengths"][g] == firsts[g] + len(out["trace"])
        assert ex["simulations"] == sum(o["simulations"] for o in outs) and ex["expansions"] == sum(o["expansions"] for o in outs)
    assert [e["dead_end"] for e in outs[0]["evaluations"][-cases[0].sims:]] == [True] * cases[0].sims
    # the same handles again, one move, against fresh ones
    m.agents[0].persistent(persist)
    m.play(nets[0], nets[1], max_moves=1, start_actions=start, n_plies=n_plies)
    fresh = handles()
    fresh.play(nets[0], nets[1], max_moves=1, start_actions=start, n_plies=n_plies)
    for a, b in zip(m.agents, fresh.agents):
        ra, rb = a.export(), b.export()
        _same_games(ra, rb, [(0, 0), (1, 1)], route)
        for g in range(2):
            assert assert_trace_equals_device(ra, g, {"trace": outs[g]["trace"][:1]}, route, first=firsts[g]) == 1
    fresh.close(); m.close()
    for n in nets:
        n.close()
    print(f"wall time root-match-{route}: {time.perf_counter() - t0:.2f} s")
