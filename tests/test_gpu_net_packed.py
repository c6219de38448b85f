"""The packed network pass on the GPU (net_packed_dev.hpp): a pass whose MFMA columns are (position, cell) pairs, for
engines of one to eight games per workgroup.

Its float arithmetic is net_tile's operation for operation, so everything is compared for equal bytes: the stand-alone
route (nz_net_forward_packed) against nz_net_forward on every non-terminal position, and whole rounds of the persistent
kernel with the packed pass against the same rounds with NZ_NET_PACKED=0 -- and against the C oracle fed with the
16-column network's outputs, as the other parity tests do."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PS = (1, 2, 3, 4, 7, 8)     # one tile with seven dead columns | two live columns in tile 1 | a position straddles tiles |
#                             the config-3 case | one dead column | five tiles
ENV = ("NZ_NET_PACKED", "NZ_SLOTS_PER_WG", "NZ_BURST_UNDER_NET", "NZ_SIMS_PER_CYCLE")


def _codes():
    from conftest import GOLDEN
    return np.load(os.path.join(GOLDEN, "net_kat.npz"))["codes"]


@functools.lru_cache(maxsize=None)
def _positions():
    """All 4,520 non-terminal positions as [N, 2, 3, 3] planes (4,520 is no multiple of 3 or 7: ragged last workgroup)."""
    from oracle import ttt as ottt
    codes = _codes()
    x = np.zeros((len(codes), 2, 3, 3), np.float32)
    for i, c in enumerate(codes):
        g = ottt.TicTacToe()
        g.board = ottt.board_from_code(int(c))
        x[i] = g.state_image()[0]
    assert len(x) == 4520
    return x


def _weights(arch, seed, width, blocks, recall, gain, k=3):
    from nuzero_amd import weights as W
    if arch == "recurrent":
        return W.synthetic_recurrent_net_weights(seed, 2, 1, width, blocks, recall, gain)
    if arch == "resnet":
        return W.synthetic_weights(seed, W.resnet_param_shapes(2, 1, width, blocks), gain)
    return W.synthetic_weights(seed, W.convnet_param_shapes(2, 1, k, width, blocks), gain)


# (id, arch, width, blocks, recall, iterations, value activation, kernel size, gain, logit scale)
NETS = [
    ("headline-g1", "recurrent", 64, 2, True, 2, "tanh", 3, 1.0, 1.0),
    ("headline-g3", "recurrent", 64, 2, True, 2, "tanh", 3, 3.0, 1.0),
    ("w16-i16", "recurrent", 16, 2, True, 16, "tanh", 3, 1.0, 1.0),
    ("w32-i3-tanh", "recurrent", 32, 2, True, 3, "tanh", 3, 3.0, 1.0),
    ("w64-i1-relu", "recurrent", 64, 2, True, 1, "relu", 3, 1.0, 1.0),
    ("no-recall", "recurrent", 64, 2, False, 2, "tanh", 3, 3.0, 1.0),
    ("w4", "recurrent", 4, 2, True, 2, "tanh", 3, 3.0, 1.0),
    ("w24", "recurrent", 24, 2, True, 2, "relu", 3, 1.0, 1.0),
    ("w40", "recurrent", 40, 2, True, 2, "tanh", 3, 3.0, 1.0),
    ("w48", "recurrent", 48, 1, True, 2, "tanh", 3, 1.0, 1.0),
    ("resnet", "resnet", 64, 2, False, 1, "tanh", 3, 3.0, 1.0),
    ("convnet-k3", "convnet", 64, 2, False, 1, "tanh", 3, 1.0, 1.0),
    ("convnet-k1", "convnet", 32, 3, False, 1, "relu", 1, 3.0, 1.0),
    ("large-logits", "recurrent", 64, 2, True, 2, "tanh", 3, 3.0, 30.0),
]


@pytest.mark.parametrize("net", NETS, ids=[n[0] for n in NETS])
def test_packed_forward_equals_the_16_column_forward(net):
    from nuzero_amd.engine import SelfPlayEngine
    from nuzero_amd.search_config import legacy_ttt_search_config
    _, arch, width, blocks, recall, iters, vact, k, gain, scale = net
    w = _weights(arch, 3, width, blocks, recall, gain, k)
    if scale != 1.0:                                         # 30 x the logits, no inf: the policy head's last conv
        w = dict(w)
        w["policy_head.layers.2.weight"] = w["policy_head.layers.2.weight"] * np.float32(scale)
    eng = SelfPlayEngine(legacy_ttt_search_config(10), 16)
    eng.set_weights(w, width=width, num_blocks=blocks, recall=recall, value_activation=vact, recurrent_iterations=iters,
                    arch=arch, kernel_size=k)
    x = _positions()
    want = [t.cpu().numpy() for t in eng.net_forward(x)]
    assert all(np.isfinite(a).all() for a in want)
    for P in PS:
        got = [t.cpu().numpy() for t in eng.net_forward(x, positions_per_pass=P)]
        for name, a, b in zip(("logits", "value", "probs"), got, want):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (P, name, int((a != b).sum()))
        for batch in (1, P + 1):
            got = [t.cpu().numpy() for t in eng.net_forward(x[100:100 + batch], positions_per_pass=P)]
            for name, a, b in zip(("logits", "value", "probs"), got, want):
                assert a.tobytes() == b[100:100 + batch].tobytes(), (P, batch, name)
    eng.close()


def test_packed_forward_rejects_other_sizes():
    from nuzero_amd._lib import NzError
    from nuzero_amd.engine import SelfPlayEngine
    from nuzero_amd.search_config import legacy_ttt_search_config
    eng = SelfPlayEngine(legacy_ttt_search_config(10), 16)
    eng.set_weights(_weights("recurrent", 0, 64, 2, True, 1.0))
    for P in (0, 9, 16):
        with pytest.raises(NzError):
            eng.net_forward(_positions()[:4], positions_per_pass=P)
    eng.close()


# ---- whole rounds ------------------------------------------------------------------------------------------------

def _config(kind, sims):
    from nuzero_amd.search_config import legacy_ttt_search_config
    cfg = legacy_ttt_search_config(sims)                     # the benchmark's search
    if kind == "explore":                                    # softmax moves and epsilon-random moves
        cfg["Exploration"]["number_of_softmax_moves"] = 3
        cfg["Exploration"]["epsilon_softmax_exploration"] = 0.1
        cfg["Exploration"]["epsilon_random_exploration"] = 0.2
    return cfg


@functools.lru_cache(maxsize=None)
def _round(packed, slots_per_wg, kind, sims, stamped=False, n_games=40, n_slots=24, seed=2200):
    """One round of the persistent kernel: every exported array, the counters, positions per pass, the 16-column
    network's table and (stamped) the phase stamps."""
    from nuzero_amd.engine import SelfPlayEngine
    saved = {k: os.environ.get(k) for k in ENV}
    try:
        for k in ENV:
            os.environ.pop(k, None)
        os.environ["NZ_NET_PACKED"] = str(packed)
        os.environ["NZ_SLOTS_PER_WG"] = str(slots_per_wg)
        eng = SelfPlayEngine(_config(kind, sims), n_games, n_slots=n_slots)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    eng.set_weights(_weights("recurrent", 1, 64, 2, True, 3.0))
    out = {"positions_per_pass": eng.positions_per_pass, "stamps": None}
    if stamped:
        eng.phase_stamps(True)
    eng.play(base_seed=seed)
    if stamped:
        out["stamps"] = eng.phase_stamps(False, read=True)
    out.update({k: np.asarray(v) for k, v in eng.export(trace=True).items()})
    out["counters"] = eng.counters()
    out["desync"] = eng.desync_count()
    out["live"] = eng.live_games()
    eng.close()
    return out


@functools.lru_cache(maxsize=None)
def _oracle(kind, sims, n_games=40, seed=2200):
    """The same round by the C oracle on the 16-column network's outputs."""
    from nuzero_amd.engine import SelfPlayEngine
    from oracle import cref
    eng = SelfPlayEngine(_config(kind, sims), 16)
    eng.set_weights(_weights("recurrent", 1, 64, 2, True, 3.0))
    codes = _codes()
    _, value, probs = eng.net_forward(_positions())
    table = np.zeros((3 ** 9, 10), np.float32)
    table[codes, :9] = probs.cpu().numpy()
    table[codes, 9] = value.cpu().numpy()
    eng.close()
    return cref.play_games(table, _config(kind, sims), [seed + g for g in range(n_games)])


ARRAYS = ("states", "visits", "actions", "lengths", "outcomes", "tree_size", "n_children", "bias", "child_prior",
          "child_value_sum", "root_value_sum")


def _same_bits(a, b):
    for k in ARRAYS:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
    assert a["counters"] == b["counters"] and a["desync"] == b["desync"] and a["live"] == b["live"] == 0


@pytest.mark.parametrize("kind,sims", [("bench", 30), ("explore", 64)])
@pytest.mark.parametrize("slots_per_wg", (1, 3, 4, 7))
def test_rounds_equal_the_16_column_pass_and_the_oracle(slots_per_wg, kind, sims):
    """40 games on 24 slots: slots refill, so rows die mid-round, and with 7 slots per workgroup the last workgroup
    holds 3 (24 is no multiple of 7): fewer live rows than P."""
    packed = _round(8, slots_per_wg, kind, sims)
    plain = _round(0, slots_per_wg, kind, sims)
    assert packed["positions_per_pass"] == slots_per_wg and plain["positions_per_pass"] == 16
    _same_bits(packed, plain)
    o = _oracle(kind, sims)
    for k in ("lengths", "outcomes", "actions", "visits", "tree_size", "n_children", "bias", "child_prior",
              "child_value_sum", "root_value_sum"):
        assert np.array_equal(packed[k], o[k]), k
    assert packed["counters"]["simulations"] == o["simulations"] and packed["counters"]["expansions"] == o["expansions"]


def test_positions_per_pass():
    """P for an engine that takes the packed pass; 16 for full workgroups, for NZ_NET_PACKED=0, and past the switch."""
    assert _round(8, 16, "bench", 30)["positions_per_pass"] == 16
    assert _round(0, 4, "bench", 30)["positions_per_pass"] == 16
    assert _round(3, 4, "bench", 30)["positions_per_pass"] == 16
    assert _round(4, 4, "bench", 30)["positions_per_pass"] == 4
    _same_bits(_round(8, 16, "bench", 30), _round(8, 4, "bench", 30))


def test_stamped_build_plays_the_same_games():
    stamped = _round(8, 4, "bench", 30, stamped=True)
    assert stamped["positions_per_pass"] == 4
    _same_bits(stamped, _round(0, 4, "bench", 30))
    s = stamped["stamps"]
    assert s["net_ticks_per_cycle"] > 0 and s["tree_ticks_per_cycle"] > 0 and s["workgroups"] == 6
    assert s["burst_passes_per_workgroup"] == 0 and s["burst_sims_per_workgroup"] == 0     # no wave sits a packed pass out
