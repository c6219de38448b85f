"""A float64 emulation of the board nets' plain-bf16 mode (NZ_PREC_BF16, nuzero_amd/csrc/fused16_dev.hpp) on top of the
oracle nets, shared by tests/test_bf16_ref_host.py (what the emulation can and cannot pin, and the weight stream's
packing; no device) and tests/test_gpu_boardnet_bf16.py (the device layer by layer and as a whole).  A plain module: no
fixtures, nothing collected from it.

The mode: weights and every conv input are ONE bf16, rounded to nearest even; a layer accumulates in float32, adds the
residual -- the STORED (rounded) value --, activates, and stores one bf16; the last layers of the two heads (logits,
value plane) stay float32, and so do the softmax and tanh(mean).  The emulation does the same with float64 in the
place of float32, so it differs from the device by the float32 accumulation only -- which flips roundings: one flipped
activation is a 2^-8 relative step, far more than 1e-5 (test_bf16_ref_host.py measures it).

Sections, as nz_boardnet_forward_dump numbers them: 0 the rounded input, 1 + i the output of layer i, layers in
state_dict order (trunk, policy head, value head)."""
import collections

import numpy as np

import boardnet_cases as bc

FUSED16_CASES = ("k1_scs", "k1_odd", "strip_row", "strip_col", "two_by_two", "res_narrow", "no_blocks_conv", "hex_odd")

# src / res: section numbers; act: 0 none, 1 relu, 2 tanh, 3 elu (Fused16Op::act); rows32: the output stays float32
Layer = collections.namedtuple("Layer", ["index", "src", "res", "act", "rows32", "cout"])


def rne_bf16(x):
    """x (float64 or float32 array) rounded to the nearest bf16 value, ties to even; float64 out.  Normal numbers only
    (no overflow, no denormals: the nets' values are of order 1e-3 .. 1e2)."""
    x = np.asarray(x, np.float64)
    m, e = np.frexp(x)                        # x = m 2^e, 0.5 <= |m| < 1: eight significant bits = m 2^8 an integer
    return np.ldexp(np.rint(m * 256.0), e - 8)


def bf16_bits(x32):
    """The 16 bits of the bf16 nearest to each float32 (ties to even), by integer arithmetic -- weight_pack.hpp's
    bf16_rne for finite numbers."""
    b = np.ascontiguousarray(x32, np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint32) & 0xFFFF


def layers(case):
    """The conv layers in state_dict order (boardnet.hip fill_weights; ConvNet.py:52-57, ResNet.py:64-70,
    blocks.py:46-92,130-170)."""
    from oracle.net import head_channels
    assert case.arch in ("convnet", "resnet")
    out = []
    add = lambda src, res, act, rows32, cout: out.append(Layer(len(out), src, res, act, rows32, cout)) or len(out)
    W = case.width
    if case.arch == "convnet":
        t = add(0, None, 3, False, W)
        for _ in range(case.depth):
            t = add(t, None, 3, False, W)
    else:
        t = add(0, None, 1, False, W)
        for _ in range(case.depth):
            y = add(t, None, 1, False, W)
            t = add(y, t, 1, False, W)
    pc, vc = head_channels(W, case.policy_channels, 2), head_channels(W, 1, 4)
    p = add(t, None, 1, False, pc[1])
    add(p, None, 0, True, pc[2])
    vact = 1 if case.value_activation == "relu" else 2
    v = t
    for i in range(4):
        v = add(v, None, 0 if i == 3 else vact, i == 3, vc[i + 1])
    return out


def layer_weights(case, w):
    """Per layer the tensors of its conv: (weight,) square, (kernel0, kernel1) hexagonal -- state_dict order."""
    vals = [np.asarray(v) for v in w.values()]
    per = 2 if case.hex else 1
    return [tuple(vals[i * per:(i + 1) * per]) for i in range(len(vals) // per)]


def conv64(case, a, wt):
    """The layer's convolution in float64: a [n, C, rows, cols], wt the layer's tensors (any float dtype)."""
    import torch
    import torch.nn.functional as F
    from oracle.net import hex_conv2d
    a = torch.as_tensor(np.asarray(a, np.float64))
    if case.hex:
        return hex_conv2d(a, np.asarray(wt[0], np.float64), np.asarray(wt[1], np.float64), torch.float64).numpy()
    return F.conv2d(a, torch.as_tensor(np.asarray(wt[0], np.float64)), None, 1, "same").numpy()


def activate(y, act):
    if act == 1:
        return np.maximum(y, 0.0)
    if act == 2:
        return np.tanh(y)
    if act == 3:
        return np.where(y > 0, y, np.expm1(np.minimum(y, 0.0)))
    return y


def outputs(case, pol, val):
    """(logits [n, A], probs, value) from the policy planes [n, P, rows, cols] and the value plane [n, 1, rows, cols]."""
    logits = np.asarray(pol, np.float64).reshape(len(pol), -1)
    return logits, bc.softmax64(logits), np.tanh(np.asarray(val, np.float64).mean(axis=(1, 2, 3)))


def emulate(case, x, w=None, perturb=0.0, seed=0, residual_rounded=True, sections=False):
    """(logits, probs, value) of the mode in float64.  perturb: every value is multiplied by 1 + perturb u, u uniform in
    [-1, 1), before it is rounded (a stand-in for float32 accumulation).  residual_rounded=False takes the residual from
    the unrounded tensor (what the mode does NOT do; kept to show the difference)."""
    w = bc.weights(case) if w is None else w
    rs = np.random.RandomState(seed)
    wr = [tuple(rne_bf16(t) for t in wt) for wt in layer_weights(case, w)]
    stored = [rne_bf16(np.asarray(x, np.float64))]
    exact = [np.asarray(x, np.float64)]
    for L in layers(case):
        y = conv64(case, stored[L.src], wr[L.index])
        if L.res is not None:
            y = y + (stored[L.res] if residual_rounded else exact[L.res])
        y = activate(y, L.act)
        if perturb:
            y = y * (1.0 + perturb * (2.0 * rs.random_sample(y.shape) - 1.0))
        exact.append(y)
        stored.append(y if L.rows32 else rne_bf16(y))
    ls = layers(case)
    pol = stored[[L.index for L in ls if L.rows32][0] + 1]
    out = outputs(case, pol, stored[-1])
    return out + (stored,) if sections else out


def distance(got, want):
    """The worst of the project's three measures (boardnet_cases.errors) between two (logits, probs, value)."""
    return max(bc.errors(got[0], got[1], got[2], want).values())


def per_position(got, want):
    """The same per position: [n]."""
    gl, gp, gv = (np.asarray(a, np.float64) for a in got)
    wl, wp, wv = want
    scale = np.abs(wl).max(axis=1, keepdims=True) + 1.0
    return np.maximum(np.maximum((np.abs(gl - wl) / scale).max(axis=1), np.abs(gp - wp).max(axis=1)), np.abs(gv - wv))


def weight_stream(case, wt, cout, cin):
    """The one-piece weight stream of a layer, restated: uint32 [tile][tap][32-channel group][lane][4]; word j of lane l
    holds input channels 32 g + 8 (l >> 4) + 2 j (low half) and + 1 (high half) of output channel 16 tile + (l & 15)."""
    ntaps = 7 if case.hex else 9
    coutp, cinp = (cout + 15) // 16 * 16, (cin + 15) // 16 * 16
    kg = (cinp + 31) // 32
    dense = np.zeros((coutp, kg * 32, ntaps), np.float32)            # [co][ci][tap], zero where padding
    if case.hex:
        k0, k1 = (np.asarray(t, np.float32) for t in wt)             # [co][ci][3][1] (N, centre, S), [co][ci][2][2]
        dense[:cout, :cin, 0:3] = k0[:, :, :, 0]
        for tap, (lower, side) in zip((3, 4, 5, 6), ((0, 0), (1, 0), (0, 1), (1, 1))):     # NW, SW, NE, SE
            dense[:cout, :cin, tap] = k1[:, :, lower, side]
    else:
        k = np.asarray(wt[0], np.float32)
        if k.shape[-1] == 1:
            dense[:cout, :cin, 4] = k[:, :, 0, 0]
        else:
            dense[:cout, :cin, :] = k.reshape(cout, cin, 9)
    bits = bf16_bits(dense)
    lane = np.arange(64)
    out = np.zeros((coutp // 16, ntaps, kg, 64, 4), np.uint32)
    for nt in range(coutp // 16):
        for g in range(kg):
            for j in range(4):
                co, ci = nt * 16 + (lane & 15), g * 32 + (lane >> 4) * 8 + 2 * j
                out[nt, :, g, :, j] = (bits[co, ci, :] | (bits[co, ci + 1, :] << 16)).T
    return out


E_POSITIONS = 300
_E = {}


def e_case(name):
    """E_case: the emulation's worst distance from the float64 oracle over E_POSITIONS positions -- what rounding every
    stored number to bf16 costs the case, and the coarse bound the device's whole-network outputs are held to (a flipped
    rounding on the device moves a position by less: test_bf16_ref_host.py).  Computed once per process:
    {"E", "ref64", "emu", "x"}."""
    if name not in _E:
        case = bc.BY_NAME[name]
        x = bc.inputs(case, E_POSITIONS)
        ref64 = bc.reference64(case, x)
        emu = emulate(case, x)
        _E[name] = {"E": distance(emu, ref64), "ref64": ref64, "emu": emu, "x": x}
    return _E[name]
