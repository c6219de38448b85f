"""The list a wave walks in a network pass it steals (engine.hip solo_list, NetProgram::solo_jobs; host only, no GPU).

Wave p walks its solo list when wave p ^ 4 sits the pass out: stage by stage p's jobs and then p ^ 4's, one barrier after
both, and where the two are the two cell halves of one tile of one conv, ONE job of group 0 (all nine cells) in their
place.  nz_net_solo_program returns the very rows the kernel walks; nz_net_steal_order the concatenated order they are
made of.  Checked on the networks of tests/test_burst_under_net.py and the shapes of tests/tttnet_cases.py:
  - per stage the solo list covers exactly the (destination, tile, cell) units of the two lists, each once, and has a
    group-0 job exactly where the pairing rule holds -- with a four-tile trunk (widths 52 to 64) in every trunk stage,
    and at widths 33 to 40 in the heads' first stage (HEAD_STAGE_FUSED);
  - one stage-end flag per stage, as many as each wave's own list carries (the sitting-out wave counts barriers off
    its own list);
  - the weight chain names the next job that reads weights;
  - with NZ_BURST_WHOLE_TILE=0 the list is the concatenated order job for job;
  - the hazard rule that lets a wave run any job of a stage holds for the solo lists, the whole-tile jobs flagged
    progressive where the late half was."""
import contextlib
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from test_burst_under_net import NETS as BURST_NETS, S, J, OG_NONE, STRIP_AREA, _desc, _steal_order, _program   # noqa: E402
import tttnet_cases   # noqa: E402

# and the shapes of tests/tttnet_cases.py (a seventh entry: the ConvNet trunk's kernel size)
NETS = BURST_NETS + tttnet_cases.program_shapes()
IDS = ["-".join(str(x) for x in n) for n in NETS]
# Where the two heads' first convs make four tiles (2 + 2: widths 33 to 40), add_stage cuts that stage's tiles in halves
# and deals wave p and p ^ 4 the two halves of one tile: the pairing rule holds there, in a HEAD stage, and the solo
# list has a whole-tile job with the value head's activation or the policy head's ReLU.  None of BURST_NETS has it.
HEAD_STAGE_FUSED = {n: {0} for n in NETS if 32 < n[1] <= 40}

# a solo row: the NZ_NET_JOB_FIELDS fields, then these
W_OFF, W_AFTER, STAGE_END = len(J), len(J) + 1, len(J) + 2
PAIR_FIELDS = ("kgroups", "src", "dst", "dtile", "res", "act", "extra", "sslot")
SWITCH = "NZ_BURST_WHOLE_TILE"


@contextlib.contextmanager
def _switch(value):
    saved = os.environ.get(SWITCH)
    os.environ.pop(SWITCH, None)
    if value is not None:
        os.environ[SWITCH] = str(value)
    try:
        yield
    finally:
        os.environ.pop(SWITCH, None)
        if saved is not None:
            os.environ[SWITCH] = saved


def _solo(net, wave, switch=None):
    from nuzero_amd import _lib
    arch, width, num_blocks, recall, iters, vact, *k = net
    nd = _desc(arch, width, num_blocks, recall, vact, *k)
    n, first = ctypes.c_int32(0), ctypes.c_int32(0)
    with _switch(switch):
        _lib.check(_lib.lib.nz_net_solo_program(ctypes.byref(nd), iters, wave, None, 0, ctypes.byref(n), ctypes.byref(first)))
        rows = np.zeros((n.value, _lib.NZ_NET_SOLO_FIELDS), np.int32)
        _lib.check(_lib.lib.nz_net_solo_program(ctypes.byref(nd), iters, wave, rows.ctypes.data_as(ctypes.c_void_p), n.value,
                                                ctypes.byref(n), ctypes.byref(first)))
    assert n.value == len(rows) and _lib.NZ_NET_SOLO_FIELDS == len(J) + 3
    return rows, first.value


def _own_jobs(net):
    """Every list's jobs that do work, per (wave, stage): nz_net_program's row with the job's w_off from
    nz_net_steal_order (the two agree on the order of a list's working jobs)."""
    prog = _program(net)
    out = {}
    for wave in range(8):
        order, _ = _steal_order(net, wave)
        mine = order[(order[:, S["wave"]] == wave) & (order[:, S["og"]] != OG_NONE)]
        rows = prog[prog[:, J["wave"]] == wave]
        assert len(mine) == len(rows)
        for o, r in zip(mine, rows):
            assert (o[S["og"]], o[S["kgroups"]], o[S["dst"]], o[S["dtile"]]) == (r[J["og"]], r[J["kgroups"]], r[J["dst"]], r[J["dtile"]])
            out.setdefault((wave, int(r[J["stage"]])), []).append((r, int(o[S["w_off"]])))
    return out


def _pairs_up(a, b):
    """The issue's pairing rule for the jobs of lists p and p ^ 4 in one stage."""
    if len(a) != 1 or len(b) != 1:
        return False
    (ra, wa), (rb, wb) = a[0], b[0]
    return ({int(ra[J["og"]]), int(rb[J["og"]])} == {5, 6} and wa == wb and
            all(ra[J[k]] == rb[J[k]] for k in PAIR_FIELDS))


def _units(rows):
    """(area, tile, cell) -> how many of `rows` (job rows) write it"""
    n = {}
    for r in rows:
        for cell in range(9):
            if (int(r[J["cells"]]) >> cell) & 1:
                key = (int(r[J["dst"]]), int(r[J["dtile"]]), cell)
                n[key] = n.get(key, 0) + 1
    return n


@pytest.mark.parametrize("net", NETS, ids=IDS)
def test_solo_list_covers_both_lists_and_fuses_paired_halves(net):
    own = _own_jobs(net)
    n_stages = 1 + max(s for _, s in own)
    fused_stages = set()
    for wave in range(8):
        rows, _ = _solo(net, wave)
        assert (np.diff(rows[:, J["stage"]]) >= 0).all() and rows[-1, J["stage"]] == n_stages - 1
        assert (rows[:, J["wave"]] == wave).all()
        for s in range(n_stages):
            a, b = own.get((wave, s), []), own.get((wave ^ 4, s), [])
            jobs = rows[(rows[:, J["stage"]] == s) & (rows[:, J["og"]] != OG_NONE)]
            want = _units([r for r, _ in a + b])
            assert all(v == 1 for v in want.values())
            assert _units(jobs) == want, (wave, s)
            whole = jobs[jobs[:, J["og"]] == 0]
            if _pairs_up(a, b):
                fused_stages.add(s)
                assert len(jobs) == 1 and len(whole) == 1 and whole[0, J["cells"]] == 0x1FF, (wave, s)
                ra, w_off = a[0]
                assert whole[0, W_OFF] == w_off and all(whole[0, J[k]] == ra[J[k]] for k in PAIR_FIELDS)
                assert whole[0, J["dst"]] < 2 and whole[0, J["sslot"]] >= 0      # the forms the kernel has for group 0
            else:
                assert len(whole) == 0, (wave, s)
                # the concatenation: p's jobs, then p ^ 4's, each as in its own list
                assert [tuple(r[2:len(J)]) for r in jobs] == [tuple(r[2:len(J)]) for r, _ in a + b], (wave, s)
                assert list(jobs[:, W_OFF]) == [w for _, w in a + b]
    width = net[1]
    head_fused = {n_stages - 4 + s for s in HEAD_STAGE_FUSED.get(net, ())}    # (empty for every net of BURST_NETS)
    if width > 48:                                                            # four tiles: 64, and 52 to 60 with padding
        assert fused_stages == set(range(n_stages - 4)) | head_fused, fused_stages   # every trunk stage; the four head stages come last
    else:
        assert fused_stages == head_fused, fused_stages                       # narrow trunks are cut in quarters


@pytest.mark.parametrize("switch", (None, 0))
@pytest.mark.parametrize("net", NETS, ids=IDS)
def test_one_stage_end_per_stage_as_in_the_own_lists(net, switch):
    for wave in range(8):
        rows, _ = _solo(net, wave, switch)
        order, _ = _steal_order(net, wave)
        for lst in (wave, wave ^ 4):
            own_ends = int(order[order[:, S["wave"]] == lst][:, S["stage_end"]].sum())
            assert int(rows[:, STAGE_END].sum()) == own_ends
        assert rows[-1, STAGE_END] == 1
        # the flag is what the stage column counts, and it closes every stage
        assert list(rows[:, J["stage"]]) == list(np.concatenate([[0], np.cumsum(rows[:, STAGE_END])[:-1]]))


@pytest.mark.parametrize("switch", (None, 0))
@pytest.mark.parametrize("net", NETS, ids=IDS)
def test_weight_chain_names_the_next_reader(net, switch):
    for wave in range(8):
        rows, first = _solo(net, wave, switch)
        readers = [i for i in range(len(rows)) if rows[i, J["og"]] != OG_NONE and rows[i, J["kgroups"]] > 0]
        assert first == (rows[readers[0], W_OFF] if readers else -1)
        for i in range(len(rows)):
            nxt = [r for r in readers if r > i]
            assert rows[i, W_AFTER] == (rows[nxt[0], W_OFF] if nxt else -1), (wave, i)


@pytest.mark.parametrize("net", NETS, ids=IDS)
def test_switch_off_is_the_concatenated_order(net):
    for wave in range(8):
        rows, first = _solo(net, wave, 0)
        order, order_first = _steal_order(net, wave)
        with _switch(0):
            order_off, _ = _steal_order(net, wave)
        assert np.array_equal(order, order_off)                       # nz_net_steal_order does not read the switch
        assert first == order_first and len(rows) == len(order)
        assert (rows[:, J["og"]] != 0).all()
        for k_solo, k_order in ((J["stage"], S["stage"]), (J["og"], S["og"]), (J["kgroups"], S["kgroups"]), (W_OFF, S["w_off"]),
                                (W_AFTER, S["w_after"]), (J["dst"], S["dst"]), (J["dtile"], S["dtile"])):
            assert list(rows[:, k_solo]) == list(order[:, k_order]), (wave, k_solo)
        # the walked list has its barrier after the second list's jobs only
        stolen_end = (order[:, S["wave"]] == wave ^ 4) & (order[:, S["stage_end"]] == 1)
        assert list(rows[:, STAGE_END]) == list(stolen_end.astype(np.int32))


@pytest.mark.parametrize("net", NETS, ids=IDS)
def test_jobs_of_a_solo_stage_are_independent(net):
    """test_burst_under_net.test_jobs_of_a_stage_are_independent on what a stolen pass runs on one SIMD pair -- waves
    p and p ^ 4's solo lists beside the other waves' own -- with the whole-tile jobs flagged progressive where the
    kernel has the form and the stage allows it."""
    prog = _program(net)
    progressive_whole = 0
    for wave in range(8):
        rows, _ = _solo(net, wave)
        rows = rows[rows[:, J["og"]] != OG_NONE]
        others = prog[(prog[:, J["wave"]] != wave) & (prog[:, J["wave"]] != wave ^ 4)]
        for s in np.unique(prog[:, J["stage"]]):
            jobs = np.concatenate([rows[rows[:, J["stage"]] == s][:, :len(J)], others[others[:, J["stage"]] == s]])
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
                if j[J["og"]] == 0:
                    form = (j[J["kgroups"]] >= 1 and not j[J["extra"]] and
                            (j[J["act"]] == 1 if j[J["res"]] >= 0 else j[J["act"]] in (1, 2)))
                    assert j[J["progressive"]] == (1 if form else 0), (s, j)
                    progressive_whole += int(j[J["progressive"]])
    # (ConvNet: ELU keeps the end-of-job epilogue; a net without residual blocks, or with zero iterations, has no trunk conv
    # without the input-plane step -- every net of BURST_NETS has blocks and iterations)
    has_block_convs = net[2] > 0 and (net[0] != "recurrent" or net[4] > 0)
    if net[1] == 64 and net[0] != "convnet" and has_block_convs:
        assert progressive_whole > 0
