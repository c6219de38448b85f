"""What has to hold, before any device is involved, for tests/test_gpu_boardnet_edges.py to mean something
(cases: tests/boardnet_cases.py):

  * the float64 oracle (oracle/net.py with dtype=float64) agrees with an independent numpy convolution, so the shapes
    where F.conv2d(..., "same") is least exercised do not rest on torch alone;
  * the float32 oracle -- the reference's own arithmetic -- stays within 0.2 of the 1e-5 tolerance of the float64 one on
    every case, so the device is allowed 5x what the reference's own rounding costs;
  * the cases are neither flat nor saturated, so an absolute bound on probabilities and values has power;
  * the case table reaches the kernels it claims to reach.

No GPU."""
import numpy as np
import pytest

import boardnet_cases as bc
from nuzero_amd.weights import head_channels

CASE_NAMES = [c.name for c in bc.CASES]


# ---- an independent float64 network in numpy ------------------------------------------------------------------------
def _taps(case, w, names):
    """[(weight [cout, cin], dy per column parity (even, odd), dx)] of one convolution."""
    if case.hex:
        k0, k1 = (np.asarray(w[n], np.float64) for n in names)                # [o, i, 3, 1], [o, i, 2, 2]
        taps = [(k0[:, :, t, 0], (t - 1, t - 1), 0) for t in range(3)]         # N, centre, S of the own column
        for side, dx in ((0, -1), (1, 1)):                                     # odd columns sit half a cell lower
            taps.append((k1[:, :, 0, side], (-1, 0), dx))                      # upper neighbour: r - 1 (even) / r (odd)
            taps.append((k1[:, :, 1, side], (0, 1), dx))                       # lower neighbour: r (even) / r + 1 (odd)
        return taps
    k = np.asarray(w[names[0]], np.float64)
    half = k.shape[2] // 2
    return [(k[:, :, ky, kx], (ky - half, ky - half), kx - half) for ky in range(k.shape[2]) for kx in range(k.shape[3])]


def _conv(x, taps):
    n, cin, rows, cols = x.shape
    xp = np.zeros((n, cin, rows + 2, cols + 2))                                # explicit zero border
    xp[:, :, 1:-1, 1:-1] = x
    out = np.zeros((n, taps[0][0].shape[0], rows, cols))
    for wt, dy, dx in taps:
        for c in range(cols):
            src = xp[:, :, 1 + dy[c & 1]:1 + dy[c & 1] + rows, 1 + c + dx]      # [n, cin, rows]
            out[:, :, :, c] += np.einsum("oi,nir->nor", wt, src)
    return out


def _numpy_net(case, w, x):
    per = 2 if case.hex else 1
    names = list(w)
    convs = [names[i:i + per] for i in range(0, len(names), per)]
    pos = [0]

    def conv(t, at=None):
        i = pos[0] if at is None else at
        if at is None:
            pos[0] += 1
        return _conv(t, _taps(case, w, convs[i]))

    relu = lambda t: np.maximum(t, 0.0)
    elu = lambda t: np.where(t > 0, t, np.expm1(np.minimum(t, 0.0)))
    x = np.asarray(x, np.float64)
    if case.arch == "convnet":
        t = elu(conv(x))
        for _ in range(case.depth):
            t = elu(conv(t))
    elif case.arch == "resnet":
        t = relu(conv(x))
        for _ in range(case.depth):
            t = relu(conv(relu(conv(t))) + t)
    else:
        t = relu(conv(x))
        first = pos[0]
        for _ in range(case.iters):
            pos[0] = first
            if case.recall:
                t = conv(np.concatenate([t, x], 1))
            for _ in range(case.depth):
                t = relu(conv(relu(conv(t))) + t)
        pos[0] = first + (1 if case.recall else 0) + 2 * case.depth
    pc = head_channels(case.width, case.policy_channels, 2)
    vc = head_channels(case.width, 1, 4)
    at = pos[0]
    assert len(convs) == at + 6
    for i in range(2):
        assert np.asarray(w[convs[at + i][0]]).shape[:2] == (pc[i + 1], pc[i])
    for i in range(4):
        assert np.asarray(w[convs[at + 2 + i][0]]).shape[:2] == (vc[i + 1], vc[i])
    p = conv(relu(conv(t, at)), at + 1)
    act = np.tanh if case.value_activation == "tanh" else relu
    v = t
    for i in range(4):
        v = conv(v, at + 2 + i)
        if i != 3:
            v = act(v)
    return p.reshape(len(x), -1), np.tanh(v.mean(axis=(1, 2, 3)))


SMALL = [c.name for c in bc.CASES if c.rows * c.cols <= 40 and c.width <= 40]


@pytest.mark.parametrize("name", SMALL)
def test_float64_oracle_equals_an_independent_numpy_convolution(name):
    """1e-12 relative on logits and values, n = 5.  (For hex_odd both sides restate hexagdly's documented addressing:
    parity with hexagdly itself stays unpinned.)"""
    case = bc.BY_NAME[name]
    assert {"k1_scs", "k1_odd", "strip_row", "strip_col"} <= set(SMALL)
    x = bc.inputs(case, 5, offset=50)
    w = bc.weights(case)
    logits, _, value = bc.reference64(case, x, w)
    p, v = _numpy_net(case, w, x)
    el = np.max(np.abs(p - logits)) / np.max(np.abs(logits))
    ev = np.max(np.abs(v - value)) / np.max(np.abs(value))
    print(f"{name}: numpy vs float64 oracle, relative: logits {el:.2e} values {ev:.2e}")
    assert el < 1e-12 and ev < 1e-12, (name, el, ev)


# ---- the float32 oracle against the float64 one; sharpness -------------------------------------------------------------
def _host_batch(case):
    n = max(b for b in bc.all_batches(case) if b <= 37)
    return bc.inputs(case, max(bc.all_batches(case)))[:n]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_float32_oracle_stays_within_a_fifth_of_the_tolerance(name):
    """At the case's largest batch size up to 37 the reference's own float32 arithmetic is within 0.2 x 1e-5 of the
    float64 oracle on all three measures.  This is the cap that keeps the device tolerance honest: it is not relaxed
    for any case."""
    case = bc.BY_NAME[name]
    x = _host_batch(case)
    w = bc.weights(case)
    want = bc.reference64(case, x, w)
    e = bc.errors(*bc.reference32(case, x, w), want)
    print(f"{name}: float32 vs float64 oracle, n = {len(x)}, gain {case.gain}: logit {e['logit']:.2e} "
          f"prob {e['prob']:.2e} value {e['value']:.2e}")
    bound = bc.REF32_SHARE * bc.TOL
    assert e["logit"] <= bound and e["prob"] <= bound and e["value"] <= bound, (name, e)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_cases_are_neither_flat_nor_saturated(name):
    """Over the case's batch: largest probability in [0.2, 0.999], largest |value| in [0.2, 0.99], largest |logit| >= 2.
    A case excused by name in the table (flat_ok, with its measured figures there) gets the bound it records."""
    case = bc.BY_NAME[name]
    logits, probs, value = bc.reference64(case, _host_batch(case))
    pm, vm, lm = float(probs.max()), float(np.abs(value).max()), float(np.abs(logits).max())
    print(f"{name}: largest probability {pm:.4f}, largest |value| {vm:.4f}, largest |logit| {lm:.2f}")
    excuse = case.flat_ok or {}
    assert excuse.get("prob_min", 0.2) <= pm <= excuse.get("prob_max", 0.999), (name, pm)
    assert excuse.get("value_min", 0.2) <= vm <= excuse.get("value_max", 0.99), (name, vm)
    assert lm >= 2.0, (name, lm)


# ---- the table reaches what it claims -------------------------------------------------------------------------------------
def _pad16(c):
    return (c + 15) // 16 * 16


def _layers(case):
    """(coutp, c0p, c1p) of every convolution a forward pass launches, from the weight shapes (set_weights' op list)."""
    out = []
    for name, shape in bc.shapes(case)[::2 if case.hex else 1]:
        cout, cin = shape[0], shape[1]
        if case.arch == "recurrent" and case.recall and name.startswith("recur_module.0."):
            assert cin == case.width + case.in_channels
            out.append((_pad16(cout), _pad16(case.width), _pad16(case.in_channels)))
        else:
            out.append((_pad16(cout), _pad16(cin), 0))
    return out


def _has_wide_stream(coutp, c0p, c1p):        # pack(): the split form conv_wide_kernel reads
    return coutp % 128 == 0 and c0p % 32 == 0 and c1p % 32 == 0


def _has_bf16_stream(coutp):                  # pack(): the piece stream of fused16_net_kernel
    return coutp <= 64


def _dispatch(n, hw, coutp, c0p, c1p):
    """dispatch_conv's choice for one layer at batch size n: "wide" or (MT, NT)."""
    ntiles, kgt, groups = coutp // 16, (c0p + c1p) // 16, (n + 15) // 16
    wide_tiles = (groups + 15) // 16 * hw * (ntiles // 8)
    if _has_wide_stream(coutp, c0p, c1p) and wide_tiles >= 160 and groups >= 8:
        return "wide"
    if ntiles % 4 == 0:
        return (2, 4) if n >= 1024 and kgt >= 8 else (1, 4)
    if ntiles % 3 == 0:
        return (1, 3)
    if ntiles % 2 == 0:
        return (2, 2) if n >= 2048 else (1, 2)
    return (2, 1) if n >= 2048 else (1, 1)


def test_case_table_reaches_the_kernels_it_claims():
    """A statement about the TABLE, made with a restatement of dispatch_conv and pack (nuzero_amd/csrc/boardnet.hip).
    The C++ is the authority: when its rules change, this restatement has to be updated with it, or the table may stop
    reaching a kernel without this test noticing."""
    chosen, wide_fallback = set(), False
    k1 = widths_odd = fused16_all_narrow = False
    for case in bc.CASES:
        layers = _layers(case)
        hw = case.rows * case.cols
        for n in bc.all_batches(case):
            for layer in layers:
                d = _dispatch(n, hw, *layer)
                chosen.add(d)
                if _has_wide_stream(*layer) and d != "wide":
                    wide_fallback = True
        k1 |= case.kernel_size == 1 and not case.hex
        widths_odd |= case.width % 16 != 0
        if case.arch != "recurrent" and all(_has_bf16_stream(l[0]) for l in layers):
            fused16_all_narrow = True
    assert {(1, 1), (1, 2), (1, 3), (1, 4), (2, 1), (2, 2), (2, 4)} <= chosen, chosen
    assert "wide" in chosen and wide_fallback
    assert k1 and widths_odd and fused16_all_narrow
    # the cases that say so, one by one
    by = bc.BY_NAME
    hw = lambda c: c.rows * c.cols
    assert all(_dispatch(2060, hw(by["k1_scs"]), *l)[0] == 2 for l in _layers(by["k1_scs"]))
    assert (2, 1) in {_dispatch(2060, hw(by["rec_odd"]), *l) for l in _layers(by["rec_odd"])}
    assert (2, 4) in {_dispatch(1030, hw(by["rec_mt2"]), *l) for l in _layers(by["rec_mt2"])}
    assert (1030 + 15) // 16 % 2 == 1 and (2060 + 15) // 16 % 2 == 1            # a ragged pair of 16-groups
    assert (1, 3) in {_dispatch(37, hw(by["nt3"]), *l) for l in _layers(by["nt3"])}
    assert not all(_has_bf16_stream(l[0]) for l in _layers(by["nt3"]))
    assert (1, 1) in {_dispatch(37, hw(by["rec_64"]), *l) for l in _layers(by["rec_64"])} and hw(by["rec_64"]) == 64
    assert hw(by["rec_65"]) == 65
    for name, n in (("wide_nonsquare", 1040), ("wide_recall", 530)):
        c = by[name]
        assert "wide" in {_dispatch(n, hw(c), *l) for l in _layers(c)}
        assert "wide" not in {_dispatch(37, hw(c), *l) for l in _layers(c)}
        assert n % 256 != 0                                                       # a partly filled last tile
    assert any(l[2] > 0 and _dispatch(530, hw(by["wide_recall"]), *l) == "wide" for l in _layers(by["wide_recall"]))
    assert by["no_blocks_conv"].depth == 0 and by["no_blocks_res"].depth == 0


def test_head_schedule_never_reaches_zero_channels():
    """head_channels steps by (out - width) / layers, a multiple of 1/4 (value head) or 1/2 (policy head), so every
    partial sum is exact and the schedule ends exactly on `out` >= 1 without dipping below it: the library's refusal
    of a schedule that reaches 0 channels cannot be triggered with a positive width."""
    for width in range(1, 600):
        assert min(head_channels(width, 1, 4)) >= 1
        for planes in (1, 2, 3, 21, 30, 64, 1000):
            assert min(head_channels(width, planes, 2)) >= 1
