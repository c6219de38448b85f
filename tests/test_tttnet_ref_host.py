"""What has to hold, before any device is involved, for tests/test_gpu_tttnet_edges.py to mean something
(cases: tests/tttnet_cases.py):

  * the float32 oracle -- the reference's own arithmetic -- stays within 0.2 of the 1e-5 tolerance of the float64 one on
    all 37 positions of every case, so the device is allowed 5x what the reference's own rounding costs;
  * the cases are neither flat nor saturated, so an absolute bound on probabilities and values has power;
  * the case table reaches the programs it claims to reach (nz_net_program, nz_net_solo_program, nz_net_packed_program);
  * in a bias-free net the all-zero position gives logits and a value of exactly 0, which the device test asserts bit
    for bit;
  * the inputs are what the table says: the first m positions of a draw of n are the draw of m.

No GPU."""
import ctypes

import numpy as np
import pytest

import tttnet_cases as tc

CASE_NAMES = [c.name for c in tc.CASES]
J = {k: i for i, k in enumerate(("wave", "stage", "og", "cells", "kgroups", "sslot", "src", "dst", "res", "act", "dtile",
                                 "extra", "progressive"))}
OG_NONE = 7
DST_STRIP = 4
SSLOT_SPLIT = -1
HALVES, QUARTERS = (5, 6), (1, 2, 3, 4)

_REF = {}


def _reference(case):
    if case.name not in _REF:
        x = tc.inputs(case, tc.MAX_BATCH)
        _REF[case.name] = (x, tc.reference64(case, x))
    return _REF[case.name]


# ---- the float32 oracle against the float64 one; sharpness -------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_float32_oracle_stays_within_a_fifth_of_the_tolerance(name):
    """On all 37 positions the reference's own float32 arithmetic is within 0.2 x 1e-5 of the float64 oracle on all three
    measures.  This is the cap that keeps the device tolerance honest: it is not relaxed for any case."""
    case = tc.BY_NAME[name]
    x, want = _reference(case)
    e = tc.errors(*tc.reference32(case, x), want)
    print(f"{name}: float32 vs float64 oracle, n = {len(x)}, gain {case.gain}: logit {e['logit']:.2e} "
          f"prob {e['prob']:.2e} value {e['value']:.2e}")
    bound = tc.REF32_SHARE * tc.TOL                         # 2e-6
    assert e["logit"] <= bound and e["prob"] <= bound and e["value"] <= bound, (name, e)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_cases_are_neither_flat_nor_saturated(name):
    """Over the 37 positions: largest probability in [0.2, 0.999], largest |value| in [0.2, 0.99], largest |logit| >= 2.
    A case excused by name in the table (flat_ok, with its measured figures there) gets the bound it records."""
    case = tc.BY_NAME[name]
    logits, probs, value = _reference(case)[1]
    pm, vm, lm = float(probs.max()), float(np.abs(value).max()), float(np.abs(logits).max())
    print(f"{name}: largest probability {pm:.4f}, largest |value| {vm:.4f}, largest |logit| {lm:.2f}")
    excuse = case.flat_ok or {}
    assert excuse.get("prob_min", 0.2) <= pm <= excuse.get("prob_max", 0.999), (name, pm)
    assert excuse.get("value_min", 0.2) <= vm <= excuse.get("value_max", 0.99), (name, vm)
    assert lm >= 2.0, (name, lm)
    if case.policy_scale is not None:
        assert lm >= 100.0, (name, lm)                      # the case is there for large logits


def test_only_large_logits_is_excused():
    assert [c.name for c in tc.CASES if c.flat_ok] == ["large_logits"]
    assert tc.BY_NAME["large_logits"].policy_scale == 30.0


# ---- the inputs ---------------------------------------------------------------------------------------------------------
def test_inputs_are_what_the_table_says():
    case = tc.BY_NAME["rec_blocks1"]
    x = tc.inputs(case, 37)
    assert x.shape == (37, 2, 3, 3) and x.dtype == np.float32
    assert not x[0].any() and (x[1] == 1.0).all()
    u = x[2:6]
    assert ((u >= 0) & (u < 1)).all() and len(np.unique(u)) == u.size
    # full mantissas: the low 8 bits of the floats are not all zero (a bf16, or a sum of two, would not hold them)
    assert (u.view(np.uint32) & 0xFF).astype(bool).mean() > 0.9
    boards = x[6:]
    assert set(np.unique(boards)) == {0.0, 1.0} and not (boards[:, 0] * boards[:, 1]).any()      # a cell is X or O, not both
    assert boards[:, 0].any() and boards[:, 1].any()
    for m in (1, 2, 5, 6, 7, 16, 36):
        assert np.array_equal(tc.inputs(case, m), x[:m])
    assert not np.array_equal(tc.inputs(tc.BY_NAME["rec_blocks0"], 37)[2:], x[2:])               # per-case draws


@pytest.mark.parametrize("name", CASE_NAMES)
def test_all_zero_position_gives_exact_zeros(name):
    """No conv has a bias, relu(0) = tanh(0) = elu(0) = 0: every logit and the value of position 0 are exactly 0 in both
    oracles, and its nine probabilities are equal."""
    case = tc.BY_NAME[name]
    x, (logits, probs, value) = _reference(case)
    assert not x[0].any()
    assert (logits[0] == 0).all() and value[0] == 0 and (probs[0] == probs[0, 0]).all()
    l32, p32, v32 = tc.reference32(case, x[:1])
    assert (l32[0] == 0).all() and v32[0] == 0 and (p32[0] == p32[0, 0]).all()


# ---- the table reaches what it claims -------------------------------------------------------------------------------------
def _desc(case):
    from nuzero_amd import _lib
    return _lib.NetDesc(in_channels=2, policy_channels=1, width=case.width, num_blocks=case.num_blocks,
                        recall=int(case.recall),
                        value_activation=_lib.NZ_ACT_RELU if case.value_activation == "relu" else _lib.NZ_ACT_TANH,
                        arch={"recurrent": _lib.NZ_ARCH_RECURRENT, "resnet": _lib.NZ_ARCH_RESNET,
                              "convnet": _lib.NZ_ARCH_CONVNET}[case.arch], kernel_size=case.kernel_size)


def _rows(call, fields):
    from nuzero_amd import _lib
    n = ctypes.c_int32(0)
    _lib.check(call(None, 0, ctypes.byref(n)))
    rows = np.zeros((n.value, fields), np.int32)
    _lib.check(call(rows.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n)))
    assert n.value == len(rows) > 0
    return rows


def _program(case):
    from nuzero_amd import _lib
    nd = _desc(case)
    return _rows(lambda *a: _lib.lib.nz_net_program(ctypes.byref(nd), case.iters, *a), _lib.NZ_NET_JOB_FIELDS)


def _solo(case, wave):
    from nuzero_amd import _lib
    nd, first = _desc(case), ctypes.c_int32(0)
    return _rows(lambda *a: _lib.lib.nz_net_solo_program(ctypes.byref(nd), case.iters, wave, *a, ctypes.byref(first)),
                 _lib.NZ_NET_SOLO_FIELDS)


def _packed(case, P):
    from nuzero_amd import _lib
    nd = _desc(case)
    return _rows(lambda *a: _lib.lib.nz_net_packed_program(ctypes.byref(nd), case.iters, P, *a),
                 _lib.NZ_NET_PACKED_JOB_FIELDS)


def _tiles(channels):
    return (channels + 15) // 16


def _expected(case):
    """From the description alone (RecurrentNet.py:82-99, ConvNet.py:20-40, the head schedule): the stages of a pass, and
    the head layout compile_net documents -- the value head's first conv into the side buffer's first tiles, the
    policy head's after them, past the fourth into the strip, which the policy head's second conv then reads split."""
    from nuzero_amd.weights import head_channels
    if case.arch == "convnet":
        trunk = 1 + case.num_blocks
    elif case.arch == "resnet":
        trunk = 1 + 2 * case.num_blocks
    else:
        trunk = 1 + case.iters * ((1 if case.recall else 0) + 2 * case.num_blocks)
    head_tiles = _tiles(head_channels(case.width, 1, 4)[1]) + _tiles(head_channels(case.width, 1, 2)[1])
    return {"stages": trunk + 4, "two_k": case.width > 32, "strip": head_tiles > 4, "tiles": _tiles(case.width)}


@pytest.mark.parametrize("name", CASE_NAMES)
def test_case_compiles_to_the_program_its_shape_asks_for(name):
    case = tc.BY_NAME[name]
    want = _expected(case)
    rows = _program(case)
    work = rows[rows[:, J["og"]] != OG_NONE]
    assert int(rows[:, J["stage"]].max()) + 1 == want["stages"]
    assert bool((work[:, J["kgroups"]] == 2).any()) == want["two_k"] and work[:, J["kgroups"]].max() <= 2
    assert (work[work[:, J["stage"]] == 0][:, J["kgroups"]] == 0).all()          # the projection reads the input planes only
    assert (work[work[:, J["stage"]] == 0][:, J["extra"]] == 1).all()
    assert bool((work[:, J["dst"]] == DST_STRIP).any()) == want["strip"]
    assert bool((work[:, J["sslot"]] == SSLOT_SPLIT).any()) == want["strip"]
    n_prog = int(work[:, J["progressive"]].sum())
    print(f"{name}: {want['stages']} stages, {len(work)} working jobs, K groups {sorted(set(work[:, J['kgroups']]))}, "
          f"strip {want['strip']}, {n_prog} progressive jobs")
    assert n_prog > 0
    # a trunk of four tiles is cut in halves, a narrower one in quarters
    trunk = work[work[:, J["stage"]] < want["stages"] - 4]
    assert set(trunk[:, J["og"]]) == set(HALVES if want["tiles"] == 4 else QUARTERS)
    assert int(trunk[:, J["dtile"]].max()) + 1 == want["tiles"]
    # the other two compilers take the shape too: every wave's solo list, and the packed program
    for wave in range(8):
        solo = _solo(case, wave)
        assert int(solo[:, len(J) + 2].sum()) == want["stages"]
        in_trunk = solo[solo[:, J["stage"]] < want["stages"] - 4]
        assert (in_trunk[:, J["og"]] == 0).all() if want["tiles"] == 4 else not (in_trunk[:, J["og"]] == 0).any()
    for P in (1, 3, 8):
        packed = _packed(case, P)
        assert int(packed[:, 12].sum()) == 8 * want["stages"]                     # stage_end: one per wave and stage


def test_table_spans_the_program_space():
    """What the cases compile to between them."""
    stages, kgroups, strip, progressive, tiles, acts = set(), set(), set(), [], set(), set()
    for case in tc.CASES:
        rows = _program(case)
        work = rows[rows[:, J["og"]] != OG_NONE]
        stages.add(int(rows[:, J["stage"]].max()) + 1)
        kgroups |= set(int(k) for k in work[:, J["kgroups"]])
        strip.add(bool((work[:, J["dst"]] == DST_STRIP).any()))
        progressive.append(int(work[:, J["progressive"]].sum()))
        tiles.add(_tiles(case.width))
        acts |= set(int(a) for a in work[:, J["act"]])
    assert min(stages) == 5 and max(stages) == 30
    assert kgroups == {0, 1, 2} and strip == {False, True} and tiles == {1, 2, 3, 4} and acts == {0, 1, 2, 3}
    assert min(progressive) >= 1 and max(progressive) >= 50, progressive
    by = tc.BY_NAME
    assert {c.width for c in tc.CASES} >= {4, 12, 20, 28, 36, 44, 52, 60, 64}
    assert {c.num_blocks for c in tc.CASES} >= {0, 1, 2, 3}
    assert by["rec_iters0"].iters == 0 and {c.kernel_size for c in tc.CASES} == {1, 3}
    assert any(c.arch == "recurrent" and not c.recall for c in tc.CASES)
    assert any(c.arch != "recurrent" and c.value_activation == "relu" for c in tc.CASES)


def test_added_cases_reach_the_forms_they_name():
    # rec_44: residual jobs in quarters at two K groups, flagged progressive; waves with two jobs in one trunk stage
    rows = _program(tc.BY_NAME["rec_44"])
    res = rows[(rows[:, J["res"]] >= 0)]
    assert len(res) and set(res[:, J["og"]]) <= set(QUARTERS) and (res[:, J["kgroups"]] == 2).all()
    assert res[:, J["progressive"]].any()
    recall = rows[(rows[:, J["extra"]] == 1) & (rows[:, J["kgroups"]] == 2)]
    assert len(recall) and set(recall[:, J["og"]]) == set(QUARTERS) and not recall[:, J["progressive"]].any()
    trunk = rows[(rows[:, J["stage"]] == 2) & (rows[:, J["og"]] != OG_NONE)]
    assert len(trunk) == 12 and max(np.bincount(trunk[:, J["wave"]])) == 2
    for other in tc.CASES:
        if other.name != "rec_44":
            r = _program(other)
            assert not ((r[:, J["res"]] >= 0) & (r[:, J["kgroups"]] == 2) & np.isin(r[:, J["og"]], QUARTERS)).any(), other.name
    # conv_56: 3x3 ELU in halves at two K groups; a stolen pass runs it as ONE whole-tile ELU job
    case = tc.BY_NAME["conv_56"]
    rows = _program(case)
    elu = rows[(rows[:, J["act"]] == 3) & (rows[:, J["kgroups"]] == 2)]
    assert len(elu) == 8 and set(elu[:, J["og"]]) == set(HALVES) and not elu[:, J["progressive"]].any()
    solo = _solo(case, 0)
    assert ((solo[:, J["og"]] == 0) & (solo[:, J["act"]] == 3) & (solo[:, J["kgroups"]] == 2)).any()
    for other in tc.CASES:
        if other.name != "conv_56" and other.kernel_size == 3:
            r = _program(other)
            assert not ((r[:, J["act"]] == 3) & (r[:, J["kgroups"]] == 2) & np.isin(r[:, J["og"]], HALVES)).any(), other.name
