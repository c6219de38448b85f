"""The compact SCS replay buffer's host side (C ABI nz_scs_replay_*): the record size is a condition on the layout, not
a measurement, and creation without a device fails loudly.  CPU only."""
import ctypes
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CONFIGS = os.path.join(HERE, "golden", "scs_configs")


def _cfg(name):
    from nuzero_amd.scs import ScsGameConfig
    return ScsGameConfig(os.path.join(CONFIGS, name + ".yml"))


def _dense_row(cfg):
    """Bytes of a position in the dense buffer: state image, policy over all actions, value, game index."""
    return (cfg.channels * cfg.rows * cfg.cols + cfg.num_actions + 2) * 4


@pytest.mark.parametrize("name,dense,limit", [("mirrored_5x5", 10708, 2677), ("ten_by_ten", 42808, 5351)])
def test_a_record_is_a_fraction_of_the_dense_row(name, dense, limit):
    """At most a quarter of the dense row on 5x5 and an eighth on 10x10, with the description's own children bound; on
    10x10 still with 256 children, the most the search engine's records hold (on 5x5 256 children alone are 2 KB: a
    record of 3,050 bytes, 28% of the dense row)."""
    from nuzero_amd.replay_scs import record_bytes
    cfg = _cfg(name)
    assert _dense_row(cfg) == dense and limit == dense // (4 if name == "mirrored_5x5" else 8)
    own = record_bytes(cfg)
    assert 640 < own <= limit
    assert own <= record_bytes(cfg, 256)
    if name == "ten_by_ten":
        assert record_bytes(cfg, 256) <= limit
    # the layout: 12 bytes of scalars, 12 per tile of terrain, 8 per child, the 640-byte state, 2 bytes per tile reserved
    # for victory points (a description may name every tile for either player), rounded up to whole words
    tiles = cfg.rows * cfg.cols
    assert record_bytes(cfg, 256) == (12 + 12 * tiles + 8 * 256 + 640 + 2 * tiles + 3) // 4 * 4
    assert record_bytes(cfg, 128) - record_bytes(cfg, 64) == 8 * 64


def test_record_bytes_depends_on_the_board_shape_only():
    """Two descriptions of one shape share a record size (they may share a buffer); another shape has another size."""
    from nuzero_amd.replay_scs import record_bytes
    a, b = record_bytes(_cfg("mirrored_5x5"), 64), record_bytes(_cfg("late_reinforcements_5x5"), 64)
    assert a == b
    assert record_bytes(_cfg("many_units_5x6"), 192) != record_bytes(_cfg("mirrored_5x5"), 192)


def test_record_bytes_refuses_a_children_bound_below_the_description():
    """many_units_5x6 has positions of more than 64 legal actions: records of 64 children cannot hold its games."""
    from nuzero_amd import _lib
    from nuzero_amd.replay_scs import record_bytes
    with pytest.raises(_lib.NzError, match="children"):
        record_bytes(_cfg("many_units_5x6"), 64)
    assert record_bytes(_cfg("many_units_5x6")) > 0


def test_create_without_a_device_fails_loudly():
    import torch
    from nuzero_amd import _lib
    if torch.cuda.is_available():
        return
    cfg = _cfg("mirrored_5x5")
    h = ctypes.c_void_p(0)
    st = _lib.lib.nz_scs_replay_create(ctypes.byref(h), 1000, 64, cfg.channels, cfg.rows, cfg.cols, cfg.num_actions, 0)
    assert st == _lib.NZ_ERR_HIP and not h.value
    assert b"no HIP device" in _lib.lib.nz_scs_replay_last_error(None)
    # sizes that are no SCS image shape are refused before the device is looked at
    st = _lib.lib.nz_scs_replay_create(ctypes.byref(h), 1000, 64, cfg.channels + 1, cfg.rows, cfg.cols, cfg.num_actions, 0)
    assert st == _lib.NZ_ERR_ARG and not h.value
    from nuzero_amd.replay_scs import ScsReplayBuffer
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        ScsReplayBuffer(4, 8, cfg, 100, 64)
