"""The per-wavefront board net of the persistent SCS route (wave_network<HEX, PREC> inside persist_kernel,
nuzero_amd/csrc/scs_search.hip) over its shapes -- tests/wavenet_cases.py: one-, three- and four-tile trunks, two K
groups, padded channels, boards of 16 and 18 cells, 67 and 105 state planes, 12 and 30 policy planes, depth 0 and 24,
1x1 weights, the relu value head, heads shared by shape -- and the route's admission rules.

Per admitted case 4 games are played on the persistent route with every leaf evaluation recorded, and
  (a) the exact oracle replay of every game on its recorded evaluations reproduces the device's trace, keeping every
      leaf's planes (tests/scs_planes_replay.py);
  (b) float32 cases: every recorded leaf is within 1e-5 of the FLOAT64 oracle on those planes (probabilities and value;
      tests/test_wavenet_ref_host.py shows the float32 oracle keeps to a fifth of that on these weights);
  (c) every recorded leaf IS nz_boardnet_forward of its planes, bit for bit, where the net has a one-launch form (DESIGN
      5c: "Same floats as the wave-by-wave route"); where it has none (no fused16_net_kernel program) the design claims no equal bits
      and the leaf is held to nz_boardnet_forward within FORMS_TOL.  bf16 cases: nz_boardnet_forward on those planes is also held to the
      float64 emulation of the mode (tests/bf16_net_ref.py) as tests/test_gpu_boardnet_bf16.py holds it;
  (d) the wave-by-wave route plays the same games from the same seeds (where the net has the fused16 form: the two
      routes share their floats through it, and without it no equal games are claimed);
  (e) heads run as two solo chains and heads shared layer by layer play the same games (NZ_SCS_PERSIST_NO_SOLO).
Per refusal case persistent(1) raises the reason, and the default falls back to the wave-by-wave route's games.

Needs a GPU."""
import numpy as np
import pytest

import boardnet_cases as bc
import wavenet_cases as wc
from test_gpu_boardnet_edges import FORMS_TOL
from test_gpu_scs_configs import a1_search, _same_games, _game_properties

pytestmark = pytest.mark.gpu
TOL = wc.TOL
G = 4
SIMS = 12
LEAF_FLOOR = 150
SEED0 = 4100


def _search():
    return a1_search(SIMS, number_of_softmax_moves=3, root_exploration_fraction=0.25, root_dist_alpha=0.3)


def _net(case, max_batch, precision=None):
    from nuzero_amd.boardnet import BoardNet
    k = wc.board_case(case)
    net = BoardNet(k.arch, k.in_channels, k.policy_channels, k.rows, k.cols, width=k.width, num_blocks=k.depth,
                   value_activation=k.value_activation, kernel_size=k.kernel_size, max_batch=max_batch, hex=k.hex,
                   precision=precision or case.precision)
    net.set_weights(bc.weights(k), 1)
    return net


def _selfplay(case):
    from nuzero_amd.scs import ScsSelfPlay, ScsGameConfig
    return ScsSelfPlay(ScsGameConfig(wc.fixture_path(case.fixture)), _search(), G)


def _seeds(case):
    return list(range(SEED0 + 16 * case.seed, SEED0 + 16 * case.seed + G))


def play_recorded(case):
    """4 games on the persistent route with every leaf recorded -> (export, records, planes per game): (a) is asserted
    here.  Shared with scripts/wavenet_edge_errors.py."""
    from scs_planes_replay import replay_games_keeping_planes
    from scs_replay import assert_trace_equals_device
    sp, net = _selfplay(case), _net(case, G)
    seeds, mm = _seeds(case), wc.max_moves(case)
    sp.persistent(1)
    sp.record(range(G), SIMS * (sp.MAX_MOVES + 1))
    r = sp.play_native(net, seeds, max_moves=mm)
    assert sp.persistent() is True
    recs = sp.records()
    chunked = sp.MAX_CHILDREN > 64
    sp.close(); net.close()
    outs = replay_games_keeping_planes([(wc.fixture_path(case.fixture), _search(), seeds[g]) + recs[g] + (mm,)
                                        for g in range(G)])
    planes = {}
    for g, out in enumerate(outs):
        assert out["evaluations_used"] == out["evaluations_recorded"] == len(out["planes"]) == len(recs[g][2]), (case.name, g)
        assert out["length"] == r["lengths"][g], (case.name, g)
        if mm is None:
            assert out["terminal"] and out["terminal_value"] == r["outcomes"][g], (case.name, g)
        assert assert_trace_equals_device(r, g, out, case.name) == r["lengths"][g], (case.name, g)
        planes[g] = out["planes"]
    leaves = sum(len(planes[g]) for g in range(G))
    assert leaves == r["expansions"], (case.name, leaves, r["expansions"])
    assert r["simulations"] == SIMS * int(r["lengths"].sum())
    assert leaves >= LEAF_FLOOR, (case.name, leaves)
    # (the kernel variant that holds a node's children in chunks of 64 lanes is chosen by the game's bound)
    assert chunked == (case.fixture == "many_units_5x6"), case.name
    return r, recs, planes


def leaf_arrays(recs, planes):
    """Every recorded leaf of every game, none left out: (planes [n, C, rows, cols], probs [n, A], values [n])."""
    x = np.concatenate([planes[g] for g in range(G)])
    p = np.concatenate([recs[g][1] for g in range(G)])
    v = np.concatenate([recs[g][2] for g in range(G)])
    assert len(x) == len(p) == len(v)
    return x, p, v


def float64_errors(case, x, p, v):
    """(device's, float32 oracle's) worst probability and value error against the float64 oracle on the leaves."""
    k = wc.board_case(case)
    w = bc.weights(k)
    want = bc.reference64(k, x, w)
    dev = bc.errors(None, p, v, want)
    _, p32, v32 = bc.reference32(k, x, w)
    return dev, bc.errors(None, p32, v32, want)


def _forward_all(net, x, want_logits=False):
    import torch
    outs = []
    for at in range(0, len(x), net.max_batch):
        got = net.forward(torch.from_numpy(x[at:at + net.max_batch]).cuda().contiguous(), want_logits=want_logits)
        outs.append([t.cpu().numpy() for t in got])
    return [np.concatenate(col) for col in zip(*outs)]


@pytest.mark.parametrize("name", [c.name for c in wc.ADMITTED])
def test_admitted_case(name):
    case = wc.BY_NAME[name]
    comp = wc.compile_case(case)
    assert comp.gate is None
    r, recs, planes = play_recorded(case)                                       # (a)
    x, p, v = leaf_arrays(recs, planes)
    assert np.isfinite(p).all() and np.isfinite(v).all()
    assert np.max(np.abs(p.astype(np.float64).sum(axis=1) - 1.0)) < 1e-5
    if case.precision == "float32":                                             # (b)
        dev, ref32 = float64_errors(case, x, p, v)
        print(f"{name}: {len(x)} leaves, against the float64 oracle: prob {dev['prob']:.2e} value {dev['value']:.2e} "
              f"(float32 oracle: prob {ref32['prob']:.2e} value {ref32['value']:.2e})")
        assert dev["prob"] < TOL and dev["value"] < TOL, (name, dev)
    # (c) the same floats as nz_boardnet_forward on a second handle
    big = _net(case, 64)
    assert big.fused()
    pf, vf = _forward_all(big, x)
    if comp.fused16:
        assert np.array_equal(pf.view(np.int32), p.view(np.int32)), (name, "probabilities")
        assert np.array_equal(vf.view(np.int32), v.view(np.int32)), (name, "values")
    else:
        # (by the restatement: the library does not say which one-launch form a handle has)
        assert "no fused16 form" in case.reaches
        dp, dv = float(np.abs(pf - p).max()), float(np.abs(vf - v).max())
        print(f"{name}: against nz_boardnet_forward (fused_net_kernel): prob {dp:.2e} value {dv:.2e}")
        assert dp < FORMS_TOL and dv < FORMS_TOL, (name, dp, dv)
    if case.precision == "bf16":
        import bf16_net_ref as br
        k = wc.board_case(case)
        w = bc.weights(k)
        lpv = lambda o: (o[2], o[0], o[1])                                      # forward's order -> (logits, probs, value)
        got = lpv(_forward_all(big, x, want_logits=True))
        emu, ref64 = br.emulate(k, x, w), bc.reference64(k, x, w)
        e_case, d_emu = br.distance(emu, ref64), br.distance(got, emu)
        f32 = _net(case, 64, "float32")
        d_f32 = br.distance(got, tuple(a.astype(np.float64) for a in lpv(_forward_all(f32, x, want_logits=True))))
        f32.close()
        print(f"{name}: to the float64 emulation {d_emu:.3e} (E_case {e_case:.3e}), to the float32 mode {d_f32:.3e}")
        assert d_emu <= e_case, (name, d_emu, e_case)
        assert d_f32 > 1e-4, (name, d_f32, "is the mode on?")
    big.close()
    # (d) the wave-by-wave route plays the same games -- where its leaf batches run fused16_net_kernel.  Without that form
    # they run fused_net_kernel, whose floats differ in the last bits (c), and so do the games after a few moves (seen on
    # the device at width 64): the wave route is then held to play whole legal games of its own.
    sp, net = _selfplay(case), _net(case, G)
    sp.persistent(0)
    rw = sp.play_native(net, _seeds(case), max_moves=wc.max_moves(case))
    assert sp.persistent() is False
    if comp.fused16:
        _same_games(r, rw, [(g, g) for g in range(G)], name)
        assert rw["expansions"] == r["expansions"] and rw["simulations"] == r["simulations"]
    else:
        _game_properties(wc.fixture_path(case.fixture), rw, range(G), full_games=wc.max_moves(case) is None)
        assert rw["simulations"] == SIMS * int(rw["lengths"].sum())
    sp.close(); net.close()


SOLO_AND_SHARED = [c.name for c in wc.ADMITTED if c.expect == "shared"] + ["w8_conv"]


@pytest.mark.parametrize("name", SOLO_AND_SHARED)
def test_solo_and_shared_heads_play_the_same_games(name, monkeypatch):
    """(e) NZ_SCS_PERSIST_NO_SOLO (read when a net's per-wavefront program is built) keeps every head layer split between
    the pair.  Which of the two programs the default is comes from the restatement: a case whose heads are shared by
    shape must be "shared" there (the variable then changes nothing: the odd path in head layers is what the case's
    other test has run), w8_conv must be "solo" (the variable then puts one-tile head layers on the odd path)."""
    case = wc.BY_NAME[name]
    assert wc.compile_case(case).verdict == case.expect
    assert wc.compile_case(case, no_solo=True).verdict == "shared"
    assert (name == "w8_conv") == (case.expect == "solo")
    out = []
    for no_solo in (False, True):
        if no_solo:
            monkeypatch.setenv("NZ_SCS_PERSIST_NO_SOLO", "1")
        sp, net = _selfplay(case), _net(case, G)
        sp.persistent(1)
        out.append(sp.play_native(net, _seeds(case), max_moves=wc.max_moves(case)))
        assert sp.persistent() is True
        sp.close(); net.close()
    _same_games(out[0], out[1], [(g, g) for g in range(G)], name)
    assert out[0]["expansions"] == out[1]["expansions"] and out[0]["simulations"] == out[1]["simulations"]


@pytest.mark.parametrize("name", [c.name for c in wc.REFUSED])
def test_refusal_case(name):
    from nuzero_amd._lib import NzError
    case = wc.BY_NAME[name]
    assert wc.compile_case(case).verdict == case.expect
    seeds = _seeds(case)
    sp, net = _selfplay(case), _net(case, G)
    sp.persistent(1)
    with pytest.raises(NzError, match=case.expect):
        sp.play_native(net, seeds, max_moves=1)
    sp.persistent(-1)
    rd = sp.play_native(net, seeds, max_moves=2)
    assert sp.persistent() is False
    sp.persistent(0)
    rw = sp.play_native(net, seeds, max_moves=2)
    assert sp.persistent() is False
    _same_games(rd, rw, [(g, g) for g in range(G)], name)
    assert rd["expansions"] == rw["expansions"]
    sp.close(); net.close()
