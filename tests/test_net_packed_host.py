"""The packed network pass on the host (engine.hip compile_net_packed, nz_net_packed_columns; no GPU).

A workgroup of P <= 8 games packs its 9 P live (position, cell) pairs into T = ceil(9 P / 16) tiles of 16 MFMA columns
(net_packed_dev.hpp).  Checked here: the column map, that a convolution done through it is the plain 'same'
convolution, the matrix-instruction count it gives, and that the compiled job lists compute every (conv application,
output tile, column tile) once, keep a stage's reads and writes apart, and give every wave the same barriers."""
import ctypes

import numpy as np
import pytest

import tttnet_cases

PS = list(range(1, 9))
F = {k: i for i, k in enumerate(("wave", "stage", "tensor", "nt", "tile0", "tiles", "kgroups", "src", "dst", "res", "act",
                                 "extra", "stage_end", "conv_tiles"))}

# (arch, width, num_blocks, recall, iterations, value_activation)
NETS = [("recurrent", 64, 2, True, 2, "tanh"), ("resnet", 64, 2, False, 1, "tanh"), ("convnet", 64, 2, False, 1, "tanh"),
        ("recurrent", 16, 2, True, 2, "tanh"), ("recurrent", 24, 2, True, 2, "relu"), ("recurrent", 48, 2, True, 2, "tanh")]
# and the shapes of tests/tttnet_cases.py (a seventh entry: the ConvNet trunk's kernel size)
NETS += tttnet_cases.program_shapes()
IDS = ["-".join(str(x) for x in n) for n in NETS]


def _columns(P):
    from nuzero_amd import _lib
    T = (9 * P + 15) // 16
    pos, cell = np.full(16 * T, 99, np.int32), np.full(16 * T, 99, np.int32)
    src = np.full((16 * T, 9), 99, np.int32)
    n = ctypes.c_int32(0)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    _lib.check(_lib.lib.nz_net_packed_columns(P, vp(pos), vp(cell), vp(src), 16 * T, ctypes.byref(n)))
    assert n.value == T
    return pos, cell, src


def _desc(arch, width, num_blocks, recall, value_activation, kernel_size=3):
    from nuzero_amd import _lib
    return _lib.NetDesc(in_channels=2, policy_channels=1, width=width, num_blocks=num_blocks, recall=int(recall),
                        value_activation=_lib.NZ_ACT_RELU if value_activation == "relu" else _lib.NZ_ACT_TANH,
                        arch={"recurrent": _lib.NZ_ARCH_RECURRENT, "resnet": _lib.NZ_ARCH_RESNET,
                              "convnet": _lib.NZ_ARCH_CONVNET}[arch], kernel_size=kernel_size)


def _program(net, P):
    from nuzero_amd import _lib
    arch, width, num_blocks, recall, iters, vact, *k = net
    nd = _desc(arch, width, num_blocks, recall, vact, *k)
    n = ctypes.c_int32(0)
    _lib.check(_lib.lib.nz_net_packed_program(ctypes.byref(nd), iters, P, None, 0, ctypes.byref(n)))
    rows = np.zeros((n.value, _lib.NZ_NET_PACKED_JOB_FIELDS), np.int32)
    _lib.check(_lib.lib.nz_net_packed_program(ctypes.byref(nd), iters, P, rows.ctypes.data_as(ctypes.c_void_p), n.value,
                                              ctypes.byref(n)))
    assert n.value == len(rows)
    return rows


def _applications(net):
    """The conv tensors in execution order, stage by stage (state_dict order; RecurrentNet.py:82-99, ConvNet.py:20-40,
    the two heads side by side)."""
    arch, _, blocks, recall, iters = net[:5]
    if arch == "convnet":
        trunk, n_trunk = [[i] for i in range(1 + blocks)], 1 + blocks
    else:
        first = 2 if recall else 1
        n_trunk = first + 2 * blocks
        trunk = [[0]]
        for _ in range(iters if arch == "recurrent" else 1):
            if recall:
                trunk.append([1])
            for b in range(blocks):
                trunk += [[first + 2 * b], [first + 2 * b + 1]]
    ph, vh = n_trunk, n_trunk + 2
    return trunk + [[ph, vh], [ph + 1, vh + 1], [vh + 2], [vh + 3]]


@pytest.mark.parametrize("P", PS)
def test_every_live_pair_sits_in_one_column(P):
    pos, cell, _ = _columns(P)
    live = pos >= 0
    assert np.array_equal(live, cell >= 0)
    pairs = sorted(zip(pos[live].tolist(), cell[live].tolist()))
    assert pairs == [(p, c) for p in range(P) for c in range(9)]
    assert int((~live).sum()) == 16 * ((9 * P + 15) // 16) - 9 * P
    assert np.all(pos[~live] == -1) and np.all(cell[~live] == -1)


@pytest.mark.parametrize("P", PS)
def test_tap_sources(P):
    """tap = 3 (dy + 1) + (dx + 1), source = cell + (dy, dx) on the board, else -1 (nz_net_final_tap's convention: the
    last tap that reaches a cell is the one with the largest in-board (dy, dx))."""
    from nuzero_amd import _lib
    pos, cell, src = _columns(P)
    for i in range(len(pos)):
        for tap in range(9):
            dy, dx = tap // 3 - 1, tap % 3 - 1
            y, x = cell[i] // 3 + dy, cell[i] % 3 + dx
            want = 3 * y + x if cell[i] >= 0 and 0 <= y < 3 and 0 <= x < 3 else -1
            assert src[i, tap] == want, (i, tap)
    for c in range(9):
        valid = [t for t in range(9) if src[c, t] >= 0]
        assert max(valid) == _lib.lib.nz_net_final_tap(c)


@pytest.mark.parametrize("P", PS)
def test_convolution_through_the_map(P):
    """One product per (column, tap): out[column] += w[tap] * x[pos, source cell]; a zero where the map says -1."""
    rng = np.random.RandomState(P)
    x = rng.standard_normal((P, 3, 3))
    w = rng.standard_normal((3, 3))
    want = np.zeros((P, 3, 3))
    padded = np.pad(x, ((0, 0), (1, 1), (1, 1)))
    for ky in range(3):
        for kx in range(3):
            want += w[ky, kx] * padded[:, ky:ky + 3, kx:kx + 3]          # cross-correlation, zero 'same' padding
    pos, cell, src = _columns(P)
    got = np.zeros((P, 9))
    flat = x.reshape(P, 9)
    n_products = 0
    for i in range(len(pos)):
        acc = 0.0
        for tap in range(9):
            frag = flat[pos[i], src[i, tap]] if src[i, tap] >= 0 else 0.0
            acc += w[tap // 3, tap % 3] * frag
            n_products += 1
        if pos[i] >= 0:
            got[pos[i], cell[i]] = acc
        else:
            assert acc == 0.0
    assert n_products == 9 * len(pos)
    assert np.allclose(got.reshape(P, 3, 3), want, rtol=0, atol=1e-13)


@pytest.mark.parametrize("P", PS)
def test_chain_count(P):
    """Six-MFMA chains per K group and output tile: 9 per column tile, below net_tile's 49."""
    rows = _program(NETS[0], P)
    work = rows[rows[:, F["tensor"]] >= 0]
    T = (9 * P + 15) // 16
    stage0 = work[(work[:, F["stage"]] == 2) & (work[:, F["nt"]] == 0)]          # one 64-channel trunk conv, one tile
    assert 9 * int(stage0[:, F["tiles"]].sum()) == 9 * T
    assert 9 * T == 9 * -(-9 * P // 16) and 9 * T < 49


@pytest.mark.parametrize("net", NETS, ids=IDS)
@pytest.mark.parametrize("P", (1, 2, 4, 5, 8))
def test_program_computes_everything_once(net, P):
    rows = _program(net, P)
    T = (9 * P + 15) // 16
    apps = _applications(net)
    work = rows[rows[:, F["tensor"]] >= 0]
    assert int(rows[:, F["stage_end"]].sum()) == 8 * len(apps)
    for s, tensors in enumerate(apps):
        st = work[work[:, F["stage"]] == s]
        assert sorted(set(st[:, F["tensor"]].tolist())) == sorted(tensors), s
        for tensor in tensors:
            jobs = st[st[:, F["tensor"]] == tensor]
            n_tiles = int(jobs[0, F["conv_tiles"]])
            done = [(int(j[F["nt"]]), t) for j in jobs for t in range(j[F["tile0"]], j[F["tile0"]] + j[F["tiles"]])]
            assert sorted(done) == [(nt, t) for nt in range(n_tiles) for t in range(T)], (s, tensor)
            assert np.all(jobs[:, F["tiles"]] >= 1) and np.all(jobs[:, F["tiles"]] <= 2)
    assert len(work[work[:, F["stage"]] >= len(apps)]) == 0


@pytest.mark.parametrize("net", NETS, ids=IDS)
@pytest.mark.parametrize("P", (1, 4, 8))
def test_stage_reads_and_writes_stay_apart(net, P):
    """No job of a stage reads, as an operand, an area a job of the stage writes; a residual is read by the job that
    writes the same elements (its own destination)."""
    rows = _program(net, P)
    work = rows[rows[:, F["tensor"]] >= 0]
    for s in set(work[:, F["stage"]].tolist()):
        st = work[work[:, F["stage"]] == s]
        reads = {int(j[F["src"]]) for j in st if j[F["kgroups"]] > 0}
        writes = {int(j[F["dst"]]) for j in st if j[F["dst"]] < 4}
        assert not (reads & writes), s
        for j in st:
            assert j[F["src"]] in range(4) and (j[F["dst"]] in range(4) or j[F["dst"]] in (8, 9))
            if j[F["res"]] >= 0:
                assert j[F["res"]] == j[F["dst"]]
        # two convs of a stage write different areas or outputs
        by_tensor = {int(t): {int(j[F["dst"]]) for j in st if j[F["tensor"]] == t} for t in set(st[:, F["tensor"]].tolist())}
        dsts = [d for v in by_tensor.values() for d in v]
        assert len(dsts) == len(set(dsts)), s


@pytest.mark.parametrize("net", NETS, ids=IDS)
@pytest.mark.parametrize("P", (1, 3, 8))
def test_every_wave_passes_the_same_barriers(net, P):
    rows = _program(net, P)
    n_stages = len(_applications(net))
    for wave in range(8):
        own = rows[rows[:, F["wave"]] == wave]
        assert int(own[:, F["stage_end"]].sum()) == n_stages
        assert own[-1, F["stage_end"]] == 1
        # the stage column counts the barriers passed before the job
        assert list(own[:, F["stage"]]) == [int(own[:i, F["stage_end"]].sum()) for i in range(len(own))]


def test_bad_arguments():
    from nuzero_amd import _lib
    nd = _desc("recurrent", 64, 2, True, "tanh")
    n = ctypes.c_int32(0)
    for P in (0, 9):
        assert _lib.lib.nz_net_packed_program(ctypes.byref(nd), 2, P, None, 0, ctypes.byref(n)) == _lib.NZ_ERR_ARG
    a = np.zeros(16 * 9, np.int32)
    vp = a.ctypes.data_as(ctypes.c_void_p)
    assert _lib.lib.nz_net_packed_columns(0, vp, vp, vp, 16, ctypes.byref(n)) == _lib.NZ_ERR_ARG
    assert _lib.lib.nz_net_packed_columns(4, vp, vp, vp, 16, ctypes.byref(n)) == _lib.NZ_ERR_ARG      # three tiles
