"""What has to hold, before any device is involved, for tests/test_gpu_wavenet_edges.py to mean something (cases:
tests/wavenet_cases.py), as tests/test_boardnet_ref_host.py shows it for the board nets' own edge cases:

  * on 64 positions of seeded random play the float32 oracle -- the reference's own arithmetic -- stays within 0.2 of the
    1e-5 tolerance of the float64 oracle, so the device is allowed 5x what the reference's own rounding costs;
  * the cases are neither flat nor saturated there (that file's thresholds), so an absolute bound has power;
  * every case compiles, by the host restatement of the admission arithmetic, to what its `reaches` and `expect` claim:
    tile counts, K groups, solo or shared heads, which gate refuses;
  * the four small fixtures keep the properties they were written for.

No GPU."""
import numpy as np
import pytest

import boardnet_cases as bc
import wavenet_cases as wc

F32 = [c.name for c in wc.ADMITTED if c.precision == "float32"]
POSITIONS = 64
_REF = {}


def _reference(case):
    """(positions, weights, float64 (logits, probs, value)), computed once per case."""
    if case.name not in _REF:
        x = wc.random_positions(case, POSITIONS)
        k = wc.board_case(case)
        w = bc.weights(k)
        _REF[case.name] = (x, w, bc.reference64(k, x, w))
    return _REF[case.name]


@pytest.mark.parametrize("name", F32)
def test_float32_oracle_stays_within_a_fifth_of_the_tolerance(name):
    case = wc.BY_NAME[name]
    x, w, want = _reference(case)
    assert len(x) == POSITIONS
    e = bc.errors(*bc.reference32(wc.board_case(case), x, w), want)
    print(f"{name}: float32 vs float64 oracle, n = {len(x)}, gain {case.gain}: logit {e['logit']:.2e} "
          f"prob {e['prob']:.2e} value {e['value']:.2e}")
    bound = wc.REF32_SHARE * wc.TOL
    assert e["prob"] <= bound and e["value"] <= bound and e["logit"] <= bound, (name, e)


@pytest.mark.parametrize("name", F32)
def test_cases_are_neither_flat_nor_saturated(name):
    """Largest probability in [0.2, 0.999], largest |value| in [0.2, 0.99], largest |logit| >= 2: the thresholds of
    tests/test_boardnet_ref_host.py, no case excused."""
    case = wc.BY_NAME[name]
    _, _, (logits, probs, value) = _reference(case)
    pm, vm, lm = float(probs.max()), float(np.abs(value).max()), float(np.abs(logits).max())
    print(f"{name}: largest probability {pm:.4f}, largest |value| {vm:.4f}, largest |logit| {lm:.2f}")
    assert 0.2 <= pm <= 0.999, (name, pm)
    assert 0.2 <= vm <= 0.99, (name, vm)
    assert lm >= 2.0, (name, lm)


# ---- the table compiles to what it claims ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in wc.CASES])
def test_expect_is_the_restatements_verdict(name):
    case = wc.BY_NAME[name]
    comp = wc.compile_case(case)
    assert comp.verdict == case.expect, (name, comp)
    assert (comp.gate is None) == (case in wc.ADMITTED)
    if comp.gate is None:
        assert comp.lds_bytes <= wc.WAVE_LDS_BYTES and comp.workgroup_bytes <= wc.WORKGROUP_LDS_BYTES
        assert ("no fused16 form" in case.reaches) == (not comp.fused16), name
        if case.precision == "bf16":
            assert comp.fused16, "the plain-bf16 mode exists in the one-launch BF16 program only"


def _odd(layers):
    return [t for t, _ in layers if t & 1]


def test_case_table_reaches_the_paths_it_claims():
    """The cases that say so, one by one.  (tiles, K groups of 32 channels) per layer; a layer the pair of wavefronts
    shares with an odd tile count takes wave_layer_kloop<.., 1, ..> and wave_epilogue for its last tile."""
    by, comp = wc.BY_NAME, {c.name: wc.compile_case(c) for c in wc.CASES}
    trunk = lambda n: comp[n].layers[:comp[n].n_trunk]
    heads = lambda n: comp[n].layers[comp[n].n_trunk:]
    cells = lambda n: wc.board(by[n].fixture)[2] * wc.board(by[n].fixture)[3]
    # w8_conv: a one-tile trunk (all odd), hidden layer and logits wider than the trunk's real channels, solo heads; with
    # NZ_SCS_PERSIST_NO_SOLO the heads' one-tile layers are on the odd path as well
    assert [t for t, _ in trunk("w8_conv")] == [1, 1, 1] and comp["w8_conv"].verdict == "solo"
    assert heads("w8_conv")[:2] == [(1, 1), (2, 1)] and by["w8_conv"].width < 14
    shared = wc.compile_case(by["w8_conv"], no_solo=True)
    assert shared.verdict == "shared" and len(_odd(shared.layers)) == 8
    assert shared.lds_bytes == comp["w8_conv"].lds_bytes
    # w24_res: two tiles, 8 dead channels in the K group, a residual, 30 cells
    assert trunk("w24_res") == [(2, 3), (2, 1), (2, 1)] and comp["w24_res"].padded_channels == 8
    assert by["w24_res"].arch == "resnet" and cells("w24_res") == 30
    assert comp["d0_relu"].n_trunk == 1 and by["d0_relu"].value_activation == "relu"
    assert by["k1_conv"].kernel_size == 1 and not by["k1_conv"].hex and comp["k1_conv"].n_trunk == 4
    assert by["hex_w24"].hex and comp["hex_w24"].padded_channels == 8 and by["hex_w24"].arch == "resnet"
    # tiny_w64_res: four tiles, two K groups, no row in row tile 1, heads shared by shape with odd head layers
    assert trunk("tiny_w64_res")[1:] == [(4, 2)] * 4 and cells("tiny_w64_res") == 16
    assert comp["tiny_w64_res"].verdict == "shared" and _odd(heads("tiny_w64_res"))
    # tiny_w48_conv: pair + odd tile in the trunk, two K groups with 16 dead channels, 18 cells
    assert trunk("tiny_w48_conv")[1:] == [(3, 2)] * 3 and comp["tiny_w48_conv"].padded_channels == 16
    assert cells("tiny_w48_conv") == 18 and by["tiny_w48_conv"].value_activation == "relu"
    assert by["tiny_w40_hex"].hex and trunk("tiny_w40_hex")[1:] == [(3, 2)] * 2
    # 67 and 105 planes fit LDS on 16 cells and are refused for their half-filled K group alone
    assert wc.board("stack1_4x4")[:2] == (67, 12) and wc.board("stack3_4x4")[:2] == (105, 30)
    for n in ("refuse_67_planes", "refuse_105_planes_4x4"):
        assert comp[n].gate == "planes" and comp[n].lds_bytes <= wc.WAVE_LDS_BYTES
        assert comp[n].workgroup_bytes <= wc.WORKGROUP_LDS_BYTES
    assert trunk("refuse_105_planes_4x4")[0] == (2, 4)
    assert comp["chunked_w24"].padded_channels == 8
    assert len(comp["deep_w8"].layers) == 31
    assert trunk("tiny_w48_res_bf16")[1:] == [(3, 2)] * 4 and comp["tiny_w48_res_bf16"].verdict == "shared"
    assert {by[n].precision for n in ("tiny_w48_res_bf16", "w8_conv_bf16")} == {"bf16"}
    # every gate of boardnet_wave_program refuses at least once (no fixture meets the 160 KB gate past them)
    assert sorted(comp[c.name].gate for c in wc.REFUSED) == ["cells", "heads", "planes", "planes", "wave_lds", "wave_lds",
                                                              "width"]
    assert comp["refuse_w40_lds"].lds_bytes > wc.WAVE_LDS_BYTES
    # the trunks of the table: one, two, three and four tiles; one and two K groups; pairs with an odd tile
    assert {t for c in wc.ADMITTED for t, _ in trunk(c.name)} == {1, 2, 3, 4}
    assert sum(comp[c.name].verdict == "shared" for c in wc.ADMITTED) == 3


def test_admission_table_of_the_restatement():
    """The table DESIGN section 7 quotes: the largest board (cells) a feed-forward net of a width class fits at, by state
    planes (classes of 32 after padding: 49-64, 81-96, 113-128), and the gate that refuses the next larger one.  The
    160 KB gate is always the tighter of the two."""
    def largest(cin, planes, width):
        best, gate = 0, None
        for cells in range(1, 33):
            lds = wc.wave_lds_bytes(cells, cin, planes, width)
            wg = wc.PERSIST_RULES_BYTES + wc.PERSIST_GAMES * (wc.PERSIST_GAME_BYTES + (lds + 15) // 16 * 16)
            if lds <= wc.WAVE_LDS_BYTES and wg <= wc.WORKGROUP_LDS_BYTES:
                best = cells
            elif gate is None:
                gate = "wave_lds" if lds > wc.WAVE_LDS_BYTES else "workgroup_lds"
        return best, gate
    table = {(cin, w): largest(cin, planes, w) for cin, planes in ((64, 21), (86, 21), (128, 30)) for w in (32, 64)}
    print(table)
    assert table == {(64, 32): (32, None), (64, 64): (19, "workgroup_lds"),
                     (86, 32): (30, "workgroup_lds"), (86, 64): (18, "workgroup_lds"),
                     (128, 32): (24, "workgroup_lds"), (128, 64): (15, "workgroup_lds")}


# ---- the fixtures ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture,board", [("tiny_4x4", (86, 21, 4, 4)), ("tiny_3x6", (86, 21, 3, 6)),
                                           ("stack1_4x4", (67, 12, 4, 4)), ("stack3_4x4", (105, 30, 4, 4))])
def test_small_fixtures_keep_their_properties(fixture, board):
    """Planes and board as the table says; 100 games of seeded random play never reach a position without a legal
    action, offer at most 21, and stay short: over 3000 random games per fixture the lengths were 19-56 decisions (the
    bounds here leave a little room: another seed, not another game)."""
    from oracle.scs import ScsConfig, ScsGame
    assert wc.board(fixture) == board
    cfg = ScsConfig(wc.fixture_path(fixture))
    rs = np.random.RandomState(11)
    lengths, widest = [], 0
    for _ in range(100):
        g = ScsGame(cfg)
        while not g.is_terminal():
            legal = np.nonzero(g.possible_actions().reshape(-1))[0]
            assert len(legal) > 0, (fixture, g.length)
            widest = max(widest, len(legal))
            g.step_index(int(rs.choice(legal)))
        lengths.append(g.length)
    print(f"{fixture}: {min(lengths)}-{max(lengths)} decisions, at most {widest} legal actions")
    assert 18 <= min(lengths) and max(lengths) <= 60 and widest <= 21
