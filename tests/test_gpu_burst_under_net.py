"""Simulations under the network pass (selfplay.hip burst_under_pass, net_dev.hpp net_tile `steal`).

With the switch on (NZ_BURST_UNDER_NET=1 at engine creation) a wave that holds a row at the per-cycle cap sits the
network pass out and goes on simulating, and the other wave of its SIMD runs both waves' jobs.  A row's simulations are
the same sequence whenever they run and the stolen jobs are the same jobs on the same operands, so every exported array
and every counter must equal the switch-off run bit for bit, and the games must equal the lock-step route's as in the
other parity tests.  The stamped build's counters show that the path ran.

Shapes: two full workgroups (16 slots each: passes with pending and capped rows side by side), one game per workgroup
(a capped row never meets a pending one: no wave may sit out), one full-width round (the benchmark's shape), and a run
with waves 0-3 sitting out of EVERY pass with no simulation budget at all widths and both value activations -- the
logits and values the search consumed then come from stolen jobs throughout."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("states", "visits", "actions", "lengths", "outcomes", "tree_size", "n_children", "bias")
ENV = ("NZ_BURST_UNDER_NET", "NZ_BURST_BUDGET", "NZ_SLOTS_PER_WG")


@functools.lru_cache(maxsize=None)
def _round(route, switch, budget, slots_per_wg, n_games, n_slots, sims, width=64, vact="tanh", stamped=False, seed=4100):
    """One round: every exported array, the counters, the desync count and (stamped) the phase stamps."""
    from nuzero_amd.engine import SelfPlayEngine
    from nuzero_amd.search_config import legacy_ttt_search_config
    from nuzero_amd.weights import synthetic_recurrent_net_weights
    saved = {k: os.environ.get(k) for k in ENV}
    try:
        for k, v in zip(ENV, (switch, budget, slots_per_wg)):
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = str(v)
        eng = SelfPlayEngine(legacy_ttt_search_config(sims), n_games, n_slots=n_slots)
        eng.set_weights(synthetic_recurrent_net_weights(1, 2, 1, width, 2, True, 3.0), width=width, value_activation=vact)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    stamps = None
    if route == "lockstep":
        eng.play_lockstep(base_seed=seed)
    else:
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


def _same_games(a, b):
    for k in ("lengths", "outcomes", "actions", "visits"):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("sims", (100, 25))
def test_two_full_workgroups(sims):
    shape = (16, 96, 32, sims)
    off = _round("persistent", 0, None, *shape)
    on = _round("persistent", 1, None, *shape)
    _same_bits(on, off)
    _same_games(on, _round("lockstep", None, None, None, 96, 96, sims))
    stamped = _round("persistent", 1, None, *shape, stamped=True)
    _same_bits(stamped, off)
    print(sims, stamped["stamps"])
    assert stamped["stamps"]["burst_passes_per_workgroup"] > 0 and stamped["stamps"]["burst_sims_per_workgroup"] > 0
    # switched off, nothing sits out
    quiet = _round("persistent", 0, None, *shape, stamped=True)
    assert quiet["stamps"]["burst_passes_per_workgroup"] == 0 and quiet["stamps"]["burst_sims_per_workgroup"] == 0


def test_one_game_per_workgroup():
    """32 slots spread over 32 workgroups: a workgroup's only row is either pending or capped, so no pass has a wave
    sitting out."""
    off = _round("persistent", 0, None, None, 96, 32, 100)
    on = _round("persistent", 1, None, None, 96, 32, 100)
    _same_bits(on, off)
    _same_games(on, _round("lockstep", None, None, None, 96, 96, 100))
    stamped = _round("persistent", 1, None, None, 96, 32, 100, stamped=True)
    _same_bits(stamped, off)
    assert stamped["stamps"]["burst_sims_per_workgroup"] == 0


def test_full_width_round():
    off = _round("persistent", 0, None, None, 4096, 4096, 100)
    on = _round("persistent", 1, None, None, 4096, 4096, 100)
    _same_bits(on, off)
    _same_games(on, _round("lockstep", None, None, None, 4096, 4096, 100))
    stamped = _round("persistent", 1, None, None, 4096, 4096, 100, stamped=True)
    _same_bits(stamped, off)
    assert stamped["stamps"]["burst_passes_per_workgroup"] > 0 and stamped["stamps"]["burst_sims_per_workgroup"] > 0


@pytest.mark.parametrize("vact", ("tanh", "relu"))
@pytest.mark.parametrize("width", (64, 48, 32, 16))
def test_stolen_jobs_compute_the_same_network(width, vact):
    """Waves 0-3 sit out of every pass and simulate nothing (budget 0): every logit and value the search consumes was
    computed with waves 4-7 running both lists.  The exported search records equal the switch-off run's."""
    shape = (16, 64, 32, 25)
    off = _round("persistent", 0, None, *shape, width=width, vact=vact)
    forced = _round("persistent", 2, "0,0", *shape, width=width, vact=vact)
    _same_bits(forced, off)
