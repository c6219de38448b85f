"""Whole-tile jobs of a stolen network pass (engine.hip solo_list, net_dev.hpp run_job<0x1FF>).

A wave that runs its SIMD partner's jobs too walks its solo list, in which the two cell halves of a tile are ONE job
over all nine output cells (NZ_BURST_WHOLE_TILE, default 1; 0: the two half-tile jobs back to back).  Per output cell
the accumulator sees the same MFMAs in the same order and the epilogue the same steps, so nothing may change: with waves
0-3 sitting out of EVERY pass (the hook NZ_BURST_UNDER_NET=2) every logit and value the search consumes comes from the
solo lists, and every exported array and counter must equal, bit for bit, the run with half-tile jobs and the run with
the switch off.

Two full workgroups (32 slots of 16), 64 games, 25 and 100 simulations.  Width 64 is where the trunk stages fuse:
ReLU and ReLU + residual (RecurrentNet, ResNet), the recall conv with its input planes and no activation, the projection
conv (input planes only), ELU (ConvNet: the plain whole-tile form); the narrower widths pair nothing up and run the
concatenated lists.  The value activation only reaches the head stages, which never fuse; both are run at width 64."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("states", "visits", "actions", "lengths", "outcomes", "tree_size", "n_children", "bias")
ENV = ("NZ_BURST_UNDER_NET", "NZ_BURST_WHOLE_TILE", "NZ_SLOTS_PER_WG", "NZ_BURST_BUDGET", "NZ_SIMS_PER_CYCLE")
ARCHS = ("recurrent", "recurrent-norecall", "resnet", "convnet")
NETS = [(a, w, "tanh") for a in ARCHS for w in (64, 48, 32, 16)] + [(a, 64, "relu") for a in ARCHS]


def _weights(arch, width):
    from nuzero_amd import weights as W
    if arch == "resnet":
        return W.synthetic_weights(1, W.resnet_param_shapes(2, 1, width, 2), 3.0)
    if arch == "convnet":
        return W.synthetic_weights(1, W.convnet_param_shapes(2, 1, 3, width, 2), 3.0)
    return W.synthetic_recurrent_net_weights(1, 2, 1, width, 2, arch == "recurrent", 3.0)


@functools.lru_cache(maxsize=None)
def _round(switch, whole_tile, arch, width, vact, sims, stamped=False, seed=4100):
    """One round of 64 games in 32 slots (two workgroups of 16): every exported array, the counters, the desync count and
    (stamped) the phase stamps."""
    from nuzero_amd.engine import SelfPlayEngine
    from nuzero_amd.search_config import legacy_ttt_search_config
    saved = {k: os.environ.get(k) for k in ENV}
    try:
        for k in ENV:
            os.environ.pop(k, None)
        os.environ["NZ_SLOTS_PER_WG"] = "16"
        if switch is not None:
            os.environ["NZ_BURST_UNDER_NET"] = str(switch)
        if whole_tile is not None:
            os.environ["NZ_BURST_WHOLE_TILE"] = str(whole_tile)
        eng = SelfPlayEngine(legacy_ttt_search_config(sims), 64, n_slots=32)
        eng.set_weights(_weights(arch, width), width=width, num_blocks=2, recall=arch == "recurrent", value_activation=vact,
                        arch=arch.split("-")[0])
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    stamps = None
    if stamped:
        eng.phase_stamps(True)
    eng.play(base_seed=seed)
    if stamped:
        stamps = eng.phase_stamps(False, read=True)
    out = {k: np.asarray(v) for k, v in eng.export().items()}
    out["counters"] = eng.counters()
    out["desync"] = eng.desync_count()
    out["stamps"] = stamps
    eng.close()
    return out


def _same_bits(a, b):
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
    assert a["counters"] == b["counters"] and a["desync"] == b["desync"]


@pytest.mark.parametrize("sims", (25, 100))
@pytest.mark.parametrize("net", NETS, ids=["-".join(str(x) for x in n) for n in NETS])
def test_every_pass_stolen_whole_tile_against_halves_and_switch_off(net, sims):
    off = _round(0, None, *net, sims)
    assert off["desync"] == 0 and off["counters"]["simulations"] > 0
    whole = _round(2, 1, *net, sims)
    halves = _round(2, 0, *net, sims)
    _same_bits(whole, halves)
    _same_bits(whole, off)
    _same_bits(halves, off)


def test_default_switches_steal_passes():
    """Nothing set: capped rows' waves sit out, their partners walk the solo lists with whole-tile jobs."""
    net = ("recurrent", 64, "tanh")
    stamped = _round(None, None, *net, 100, stamped=True)
    print(stamped["stamps"])
    assert stamped["stamps"]["burst_passes_per_workgroup"] > 0
    _same_bits(stamped, _round(0, None, *net, 100))
    _same_bits(_round(None, None, *net, 100), _round(0, None, *net, 100))

