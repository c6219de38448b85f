"""Progressive epilogue of the fused network kernel (net_dev.hpp ProgEpi, engine.hip add_stage): an output cell that is
final before the K loop's last tap has its epilogue issued between the MFMAs of the remaining taps.

Host side (no GPU): the final-tap table and the hazard rule on the compiled job lists.  GPU side: `net_forward` on one
tile (16 positions) and on a partial tile (5) against the float32 reference network at the 1e-5 tolerance of the other
network tests, for networks that between them reach one- and two-K-group jobs, halves and quarters, the strip, the
residual and tanh forms and the jobs that keep the end-of-job epilogue; and one persistent round against the lock-step
route."""
import ctypes

import numpy as np
import pytest

import tttnet_cases

F = {k: i for i, k in enumerate(("wave", "stage", "og", "cells", "kgroups", "sslot", "src", "dst", "res", "act", "dtile",
                                 "extra", "progressive"))}
DST_POLICY, DST_VALUE, DST_STRIP = 2, 3, 4
STRIP_AREA = 2                      # read/write areas: the two activation buffers, then the strip

# (arch, width, num_blocks, recall, iterations, value_activation)
NETS = [("recurrent", w, 2, True, 2, va) for w in (16, 32, 48, 64) for va in ("tanh", "relu")]
NETS += [("resnet", 64, 2, False, 1, "tanh"), ("convnet", 64, 2, False, 1, "tanh")]
# the program shapes the host tests compile: those, and the shapes of tests/tttnet_cases.py (a seventh entry: the ConvNet
# trunk's kernel size).  The GPU test below keeps NETS: it has its own weights and tolerance.
PROGRAM_NETS = NETS + tttnet_cases.program_shapes()


def _program(arch, width, num_blocks, recall, iters, value_activation, kernel_size=3):
    from nuzero_amd import _lib
    nd = _lib.NetDesc(in_channels=2, policy_channels=1, width=width, num_blocks=num_blocks, recall=int(recall),
                      value_activation=_lib.NZ_ACT_RELU if value_activation == "relu" else _lib.NZ_ACT_TANH,
                      arch={"recurrent": _lib.NZ_ARCH_RECURRENT, "resnet": _lib.NZ_ARCH_RESNET,
                            "convnet": _lib.NZ_ARCH_CONVNET}[arch], kernel_size=kernel_size)
    n = ctypes.c_int32(0)
    _lib.check(_lib.lib.nz_net_program(ctypes.byref(nd), iters, None, 0, ctypes.byref(n)))
    rows = np.zeros((n.value, _lib.NZ_NET_JOB_FIELDS), np.int32)
    _lib.check(_lib.lib.nz_net_program(ctypes.byref(nd), iters, rows.ctypes.data_as(ctypes.c_void_p), n.value,
                                       ctypes.byref(n)))
    assert n.value == len(rows)
    return rows


def test_final_tap_table():
    """Tap index is 3 (dy + 1) + (dx + 1) with input cell = output cell + (dy, dx): the last tap whose input cell is on
    the board, worked out here from the geometry."""
    from nuzero_amd._lib import lib
    for o in range(9):
        oy, ox = divmod(o, 3)
        taps = [3 * (dy + 1) + (dx + 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                if 0 <= oy + dy < 3 and 0 <= ox + dx < 3]
        assert lib.nz_net_final_tap(o) == max(taps), o
    assert [lib.nz_net_final_tap(o) for o in range(9)] == [8, 8, 7, 8, 8, 7, 5, 5, 4]
    assert lib.nz_net_final_tap(9) == -1 and lib.nz_net_final_tap(-1) == -1


@pytest.mark.parametrize("net", PROGRAM_NETS, ids=lambda n: "-".join(str(x) for x in n))
def test_hazard_rule_on_compiled_programs(net):
    """A job flagged progressive writes an area that no job of its stage reads as an MFMA operand, has a cell that is
    final before tap 8, no input-plane step, and a buffer as destination."""
    from nuzero_amd._lib import lib
    rows = _program(*net)
    assert len(rows) > 0
    for stage in np.unique(rows[:, F["stage"]]):
        jobs = rows[rows[:, F["stage"]] == stage]
        reads = set()
        for j in jobs:
            if j[F["kgroups"]] > 0:
                reads.add(int(j[F["src"]]))
            if j[F["sslot"]] == -1:
                reads.add(STRIP_AREA)
        for j in jobs:
            if not j[F["progressive"]]:
                continue
            assert j[F["dst"]] in (0, 1) and int(j[F["dst"]]) not in reads, (stage, j)
            assert j[F["kgroups"]] >= 1 and not j[F["extra"]] and j[F["act"]] in (1, 2), (stage, j)
            assert any((j[F["cells"]] >> o) & 1 and lib.nz_net_final_tap(o) < 8 for o in range(9)), (stage, j)
    # network outputs and the strip keep the end-of-job epilogue
    assert not rows[np.isin(rows[:, F["dst"]], (DST_POLICY, DST_VALUE, DST_STRIP)), F["progressive"]].any()


def test_trunk_residual_jobs_are_progressive():
    """Every job of a residual conv on a group the kernel has the form for -- the late half {4,6,7,8} at four tiles, the
    quarters {5,7} and {2,6,8} at two -- is flagged (source: the other buffer; the residual is read by the wave that
    writes it), in the recurrent net and in the ResNet; the recall conv (input planes) is not; ELU (ConvNet) has no
    progressive form."""
    groups = (0x1D0, 0x0A0, 0x144)
    for net in (("recurrent", 64, 2, True, 2, "tanh"), ("resnet", 64, 2, False, 1, "tanh"), ("recurrent", 32, 1, True, 2, "relu")):
        rows = _program(*net)
        res = rows[(rows[:, F["res"]] >= 0) & np.isin(rows[:, F["cells"]], groups)]
        assert len(res) >= 4 and res[:, F["progressive"]].all(), net
        assert (rows[rows[:, F["res"]] >= 0][:, F["src"]] != rows[rows[:, F["res"]] >= 0][:, F["dst"]]).all()
        assert not rows[rows[:, F["extra"]] == 1, F["progressive"]].any()
    conv = _program("convnet", 64, 2, False, 1, "tanh")
    assert not conv[conv[:, F["act"]] == 3, F["progressive"]].any()
    # one- and two-K-group jobs, halves and quarters all occur among the flagged jobs of the test's networks
    flagged = np.concatenate([r[r[:, F["progressive"]] == 1] for r in (_program(*n) for n in PROGRAM_NETS)])
    assert set(flagged[:, F["kgroups"]]) == {1, 2}
    assert {0x1D0, 0x0A0, 0x144} <= set(flagged[:, F["cells"]])


def _weights(arch, width, num_blocks, recall):
    from nuzero_amd.weights import (synthetic_recurrent_net_weights, synthetic_weights, resnet_param_shapes,
                                    convnet_param_shapes)
    if arch == "recurrent":
        return synthetic_recurrent_net_weights(width, 2, 1, width, num_blocks, recall, 2.0)   # as test_gpu_head_stages
    shapes = resnet_param_shapes(2, 1, width, num_blocks) if arch == "resnet" else convnet_param_shapes(2, 1, 3, width, num_blocks)
    return synthetic_weights(width, shapes, 2.0)


def _boards(n):
    rs = np.random.RandomState(20)
    cells = rs.randint(0, 3, size=(n, 9))
    return np.stack([cells == 1, cells == 2], 1).astype(np.float32).reshape(n, 2, 3, 3)


@pytest.mark.gpu
def test_networks_match_reference_on_one_tile():
    from scipy.special import softmax
    from nuzero_amd.engine import SelfPlayEngine
    from nuzero_amd.search_config import legacy_ttt_search_config
    from oracle.net import RecurrentNetRef, FeedForwardRef
    x16 = _boards(16)
    eng = SelfPlayEngine(legacy_ttt_search_config(), 16)
    for arch, width, num_blocks, recall, iters, vact in NETS:
        w = _weights(arch, width, num_blocks, recall)
        eng.set_weights(w, width=width, num_blocks=num_blocks, recall=recall, value_activation=vact,
                        recurrent_iterations=iters, arch=arch)
        if arch == "recurrent":
            p_ref, v_ref = RecurrentNetRef(w, 2, 1, width, num_blocks, recall, vact).inference(x16, iters)
        else:
            p_ref, v_ref = FeedForwardRef(w, arch, num_blocks, vact).inference(x16)
        p_ref, v_ref = softmax(p_ref.reshape(16, 9).astype(np.float64), axis=1), v_ref.reshape(-1)
        for n in (16, 5):                       # one full tile; n_valid < 16
            _, value, probs = eng.net_forward(x16[:n])
            value, probs = value.cpu().numpy(), probs.cpu().numpy()
            dp, dv = np.abs(probs - p_ref[:n]).max(), np.abs(value - v_ref[:n]).max()
            print(arch, width, vact, n, "priors", dp, "value", dv)
            assert dp <= 1e-5 and dv <= 1e-5, (arch, width, vact, n, dp, dv)
    eng.close()


@pytest.mark.gpu
def test_persistent_round_equals_lockstep():
    """256 games on 16 slots, 25 simulations: the persistent kernel and the lock-step route (the stand-alone network
    kernel between tree kernels) play the same games from the same seeds."""
    from nuzero_amd.engine import SelfPlayEngine
    from nuzero_amd.search_config import legacy_ttt_search_config
    from nuzero_amd.weights import synthetic_recurrent_net_weights
    cfg = legacy_ttt_search_config(25)
    w = synthetic_recurrent_net_weights(1, 2, 1, 64, 2, True, 3.0)
    a = SelfPlayEngine(cfg, 256, n_slots=16)
    a.set_weights(w)
    a.play(base_seed=700)
    ra = a.export()
    assert a.desync_count() == 0
    a.close()
    b = SelfPlayEngine(cfg, 256)
    b.set_weights(w)
    b.play_lockstep(base_seed=700)
    rb = b.export()
    b.close()
    for k in ("lengths", "outcomes", "actions", "visits"):
        assert np.array_equal(ra[k], rb[k]), k
