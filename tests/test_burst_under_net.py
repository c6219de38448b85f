"""Job lists of a stealing network pass (engine.hip compile_net, net_dev.hpp net_tile `steal`; host only, no GPU).

In a pass that wave w ^ 4 sits out (selfplay.hip burst_under_pass), wave w runs, stage by stage, its own jobs and then
the other list's, and the sitting-out wave executes one barrier per stage-end flag of its own list.  Checked here on the
compiled programs of every network the GPU tests and the benchmark use:
  - all eight lists carry the same number of stage-end flags, and the merged walk ends each stage with the stolen list;
  - the jobs of waves w and w ^ 4 in a four-tile trunk stage write the same tile (the two output-cell
    halves of a tile go to the two waves of a SIMD); in the narrower and the head stages, where the dealer gives a
    wave several units or none, the property that lets any wave run any job of a stage holds instead: no job of a
    stage reads as an MFMA operand an area a job of the stage writes, and no two jobs write the same cell of a tile;
  - the weight ring's chain in merged order names the job actually run next."""
import ctypes

import numpy as np
import pytest

S = {k: i for i, k in enumerate(("wave", "index", "stage", "og", "kgroups", "w_off", "w_after", "dst", "dtile", "stage_end",
                                 "budget"))}
J = {k: i for i, k in enumerate(("wave", "stage", "og", "cells", "kgroups", "sslot", "src", "dst", "res", "act", "dtile",
                                 "extra", "progressive"))}
OG_NONE = 7
STRIP_AREA = 2

# (arch, width, num_blocks, recall, iterations, value_activation): the networks of the GPU tests; the benchmark's is
# the recurrent net at width 64 with tanh
NETS = [("recurrent", w, 2, True, 2, va) for w in (16, 32, 48, 64) for va in ("tanh", "relu")]
NETS += [("recurrent", 32, 1, True, 2, "relu"), ("resnet", 64, 2, False, 1, "tanh"), ("convnet", 64, 2, False, 1, "tanh")]
IDS = ["-".join(str(x) for x in n) for n in NETS]


def _desc(arch, width, num_blocks, recall, value_activation, kernel_size=3):
    from nuzero_amd import _lib
    return _lib.NetDesc(in_channels=2, policy_channels=1, width=width, num_blocks=num_blocks, recall=int(recall),
                        value_activation=_lib.NZ_ACT_RELU if value_activation == "relu" else _lib.NZ_ACT_TANH,
                        arch={"recurrent": _lib.NZ_ARCH_RECURRENT, "resnet": _lib.NZ_ARCH_RESNET,
                              "convnet": _lib.NZ_ARCH_CONVNET}[arch], kernel_size=kernel_size)


def _steal_order(net, wave):
    from nuzero_amd import _lib
    arch, width, num_blocks, recall, iters, vact, *k = net          # (a seventh entry: the ConvNet trunk's kernel size)
    nd = _desc(arch, width, num_blocks, recall, vact, *k)
    n, first = ctypes.c_int32(0), ctypes.c_int32(0)
    _lib.check(_lib.lib.nz_net_steal_order(ctypes.byref(nd), iters, wave, None, 0, ctypes.byref(n), ctypes.byref(first)))
    rows = np.zeros((n.value, _lib.NZ_NET_STEAL_FIELDS), np.int32)
    _lib.check(_lib.lib.nz_net_steal_order(ctypes.byref(nd), iters, wave, rows.ctypes.data_as(ctypes.c_void_p), n.value,
                                           ctypes.byref(n), ctypes.byref(first)))
    assert n.value == len(rows)
    return rows, first.value


def _program(net):
    from nuzero_amd import _lib
    arch, width, num_blocks, recall, iters, vact, *k = net          # (a seventh entry: the ConvNet trunk's kernel size)
    nd = _desc(arch, width, num_blocks, recall, vact, *k)
    n = ctypes.c_int32(0)
    _lib.check(_lib.lib.nz_net_program(ctypes.byref(nd), iters, None, 0, ctypes.byref(n)))
    rows = np.zeros((n.value, _lib.NZ_NET_JOB_FIELDS), np.int32)
    _lib.check(_lib.lib.nz_net_program(ctypes.byref(nd), iters, rows.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n)))
    return rows


@pytest.mark.parametrize("net", NETS, ids=IDS)
def test_every_wave_has_the_same_stage_ends(net):
    """A sitting-out wave executes one barrier per stage-end flag of its own list, its partner one per flag of the
    stolen list: the counts must agree over all eight lists, and each list's last job must carry the flag."""
    counts = {}
    for wave in range(8):
        rows, _ = _steal_order(net, wave)
        for lst in (wave, wave ^ 4):
            own = rows[rows[:, S["wave"]] == lst]
            assert list(own[:, S["index"]]) == list(range(len(own))), (wave, lst)      # every job of both lists, in order
            assert own[-1, S["stage_end"]] == 1
            counts.setdefault(lst, set()).add(int(own[:, S["stage_end"]].sum()))
    assert len(counts) == 8 and all(len(c) == 1 for c in counts.values())
    assert len({next(iter(c)) for c in counts.values()}) == 1, counts


@pytest.mark.parametrize("net", NETS, ids=IDS)
def test_merged_order_runs_own_then_stolen_jobs_of_each_stage(net):
    n_stages = None
    for wave in range(8):
        rows, _ = _steal_order(net, wave)
        stages = rows[:, S["stage"]]
        assert (np.diff(stages) >= 0).all() and stages[0] == 0
        n_stages = n_stages if n_stages is not None else int(stages[-1]) + 1
        assert int(stages[-1]) + 1 == n_stages
        for s in range(n_stages):
            r = rows[stages == s]
            k = int((r[:, S["wave"]] == wave).sum())
            assert 0 < k < len(r)
            assert (r[:k, S["wave"]] == wave).all() and (r[k:, S["wave"]] == wave ^ 4).all()
            # exactly the last job of either run ends the stage
            assert list(r[:k, S["stage_end"]]) == [0] * (k - 1) + [1]
            assert list(r[k:, S["stage_end"]]) == [0] * (len(r) - k - 1) + [1]
            assert len(set(r[:, S["budget"]])) == 1 and 0 <= r[0, S["budget"]] <= 16


@pytest.mark.parametrize("net", NETS, ids=IDS)
def test_weight_chain_names_the_job_run_next(net):
    """w_after of a job is the w_off of the next job of the merged order that reads weights through the ring (-1 after
    the last), and the ring starts with the first such job's."""
    for wave in range(8):
        rows, first = _steal_order(net, wave)
        readers = [i for i in range(len(rows)) if rows[i, S["og"]] != OG_NONE and rows[i, S["kgroups"]] > 0]
        assert first == (rows[readers[0], S["w_off"]] if readers else -1)
        for i in range(len(rows)):
            nxt = [r for r in readers if r > i]
            assert rows[i, S["w_after"]] == (rows[nxt[0], S["w_off"]] if nxt else -1), (wave, i)


def test_pairs_share_a_tile_in_four_tile_trunk_stages():
    """Width 64: every trunk stage gives waves w and w + 4 the two output-cell halves of tile w."""
    for net in (("recurrent", 64, 2, True, 2, "tanh"), ("resnet", 64, 2, False, 1, "tanh"), ("convnet", 64, 2, False, 1, "tanh")):
        rows = _program(net)
        n_stages = int(rows[:, J["stage"]].max()) + 1
        for s in range(n_stages - 4):                       # the four head stages come last
            jobs = rows[rows[:, J["stage"]] == s]
            assert len(jobs) == 8, (net, s)
            for w in range(4):
                a, b = jobs[jobs[:, J["wave"]] == w], jobs[jobs[:, J["wave"]] == w + 4]
                assert len(a) == 1 and len(b) == 1
                assert (a[0, J["dst"]], a[0, J["dtile"]]) == (b[0, J["dst"]], b[0, J["dtile"]]) and a[0, J["dtile"]] == w
                assert a[0, J["cells"]] | b[0, J["cells"]] == 0x1FF and a[0, J["cells"]] & b[0, J["cells"]] == 0


@pytest.mark.parametrize("net", NETS, ids=IDS)
def test_jobs_of_a_stage_are_independent(net):
    """What lets a wave run another wave's jobs of the same stage: no job of the stage reads, as an MFMA operand, an area
    that a job of the stage writes, and no two jobs write the same cell of the same tile of an area.  (The residual is
    read by the job that writes those very channels and cells.)"""
    rows = _program(net)
    for s in np.unique(rows[:, J["stage"]]):
        jobs = rows[rows[:, J["stage"]] == s]
        reads, written = set(), {}
        for j in jobs:
            if j[J["kgroups"]] > 0:
                reads.add(int(j[J["src"]]))
            if j[J["sslot"]] == -1:
                reads.add(STRIP_AREA)
        for j in jobs:
            area = STRIP_AREA if j[J["dst"]] == 4 else int(j[J["dst"]]) if j[J["dst"]] < 2 else 10 + int(j[J["dst"]])
            assert area not in reads, (s, j)
            key = (area, int(j[J["dtile"]]))
            assert written.get(key, 0) & int(j[J["cells"]]) == 0, (s, j)
            written[key] = written.get(key, 0) | int(j[J["cells"]])
            if j[J["res"]] >= 0:
                assert j[J["res"]] == j[J["dst"]] and j[J["res"]] != j[J["src"]]
