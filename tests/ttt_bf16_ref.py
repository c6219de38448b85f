"""A float64 emulation of the Tic-Tac-Toe network's plain-bf16 mode (nz_engine_precision(e, NZ_PREC_BF16),
nuzero_amd/csrc/net_dev.hpp) on the nets of oracle/net.py, shaped like tests/bf16_net_ref.py and shared by
tests/test_ttt_bf16_ref_host.py (what the emulation can carry; no device) and tests/test_gpu_ttt_bf16.py (the device
layer by layer and as a whole).  A plain module: no fixtures, nothing collected from it.

The mode: weights, raw input planes and every stored activation are ONE bf16, rounded to nearest even; a conv
accumulates in float32, adds the residual -- the STORED (rounded) value --, activates, and stores one bf16; the last
layers of the two heads (logits, the value head's per-cell plane) stay float32, and so do the softmax and tanh(mean).
The emulation does the same with float64 in the place of float32, so it differs from the device by the float32
accumulation (and the device's tanh / expm1) only -- which flips roundings.

Sections: one per conv APPLICATION, in execution order (a recurrent net applies its recall conv and its blocks once per
iteration): Section(tensor, src, res, act, rows32, out) -- tensor: the conv in state_dict order; src / res: the
sections read (-1: the rounded input planes alone; a recall conv reads its source AND the planes); out: what was stored
(float64 [n, C, 3, 3]; rows32: unrounded)."""
import collections

import numpy as np

import tttnet_cases as tc
from bf16_net_ref import activate, bf16_bits, rne_bf16      # noqa: F401  (one statement of the rounding)

Section = collections.namedtuple("Section", ["tensor", "src", "res", "act", "rows32", "planes", "out"])

# the ten cases the layer test runs, and what each is there for
LAYER_CASES = ("rec_norecall_4", "res_20", "rec_blocks0", "rec_44", "conv_56", "conv_k1_40_b0", "rec_iters0", "rec_iters5",
               "res_64_relu", "large_logits")


def applications(case):
    """The conv applications in execution order: (tensor, src, res, act, rows32, planes) with src / res indices into
    this list (-1: none / the planes alone), act 0 none, 1 relu, 2 tanh, 3 elu (engine.hip trunk_stages, compile_net)."""
    out = []
    add = lambda tensor, src, res, act, rows32=False, planes=False: out.append((tensor, src, res, act, rows32, planes)) or len(out) - 1
    if case.arch == "convnet":
        t = add(0, -1, -1, 3, planes=True)
        for i in range(case.num_blocks):
            t = add(1 + i, t, -1, 3)
        trunk_tensors = 1 + case.num_blocks
    else:
        t = add(0, -1, -1, 1, planes=True)
        recall = case.arch == "recurrent" and case.recall
        first = 2 if recall else 1
        for _ in range(case.iters if case.arch == "recurrent" else 1):
            if recall:
                t = add(1, t, -1, 0, planes=True)
            for b in range(case.num_blocks):
                y = add(first + 2 * b, t, -1, 1)
                t = add(first + 2 * b + 1, y, t, 1)
        trunk_tensors = first + 2 * case.num_blocks
    ph, vh = trunk_tensors, trunk_tensors + 2
    p = add(ph, t, -1, 1)
    add(ph + 1, p, -1, 0, rows32=True)
    vact = 1 if case.value_activation == "relu" else 2
    v = t
    for i in range(4):
        v = add(vh + i, v, -1, 0 if i == 3 else vact, rows32=i == 3)
    return out


def conv64(a, wt):
    """A bias-free 'same' convolution in float64: a [n, C, 3, 3], wt [Cout, C, k, k]."""
    import torch
    import torch.nn.functional as F
    return F.conv2d(torch.as_tensor(np.asarray(a, np.float64)), torch.as_tensor(np.asarray(wt, np.float64)), None, 1, "same").numpy()


def outputs(pol, val):
    """(logits [n, 9], probs, value) from the policy plane [n, 1, 3, 3] and the value plane [n, 1, 3, 3]."""
    logits = np.asarray(pol, np.float64).reshape(len(pol), -1)
    return logits, tc.softmax64(logits), np.tanh(np.asarray(val, np.float64).mean(axis=(1, 2, 3)))


def emulate(case, x, w=None, sections=False):
    """(logits, probs, value) of the mode in float64; with sections=True also the list of Section."""
    w = tc.weights(case) if w is None else w
    wr = [rne_bf16(np.asarray(t)) for t in w.values()]
    xr = rne_bf16(np.asarray(x, np.float64))
    secs = []
    for tensor, src, res, act, rows32, planes in applications(case):
        a = xr if src < 0 else secs[src].out
        if planes and src >= 0:
            a = np.concatenate([a, xr], axis=1)                   # RecurrentNet.py:91: cat([thought, x])
        y = conv64(a, wr[tensor])
        if res >= 0:
            y = y + secs[res].out                                 # the stored value
        y = activate(y, act)
        secs.append(Section(tensor, src, res, act, rows32, planes, y if rows32 else rne_bf16(y)))
    pol = [s for s in secs if s.rows32][0].out
    out = outputs(pol, secs[-1].out)
    return out + (secs,) if sections else out


def distance(got, want):
    """The worst of the project's three measures (tttnet_cases.errors) between two (logits, probs, value)."""
    return max(tc.errors(got[0], got[1], got[2], want).values())


_E = {}


def e_case(name):
    """E_case: the emulation's worst distance from the float64 oracle on the case's 37 positions -- what rounding every
    stored number to bf16 costs the case, from the reference side alone; the bound the device's whole-network outputs
    are held to against the emulation.  Computed once per process: {"E", "ref64", "emu", "x"}."""
    if name not in _E:
        case = tc.BY_NAME[name]
        x = tc.inputs(case, tc.MAX_BATCH)
        ref64 = tc.reference64(case, x)
        emu = emulate(case, x)
        _E[name] = {"E": distance(emu, ref64), "ref64": ref64, "emu": emu, "x": x}
    return _E[name]


# ---- the kernel's summation order in float32 (net_dev.hpp kgroup / extra_planes) ---------------------------------------
TAPS = [(t // 3 - 1, t % 3 - 1) for t in range(9)]           # tap = 3 (dy + 1) + (dx + 1), input cell = output cell + (dy, dx)


def conv32_kernel_order(a, wt, n_main):
    """The conv as the kernel sums it, per output cell and channel one float32 accumulator: K groups of 32 main channels
    ascending, inside a K group taps 0 .. 8 ascending -- each (K group, tap) one MFMA, modelled as the exact sum of its 32
    products added to the accumulator with ONE float32 rounding --, then the input planes (channels n_main ..) tap by
    tap, one float32 MFMA of four products each.  a [n, C, 3, 3] and wt [Cout, C, k, k] hold bf16 values, so every
    product is exact in float32 (and in float64).  Returns float32 [n, Cout, 3, 3]."""
    a = np.asarray(a, np.float64)
    wt = np.asarray(wt, np.float64)
    if wt.shape[-1] == 1:                                       # a 1x1 conv is the centre tap (engine.hip set_weights)
        full = np.zeros(wt.shape[:2] + (3, 3))
        full[:, :, 1, 1] = wt[:, :, 0, 0]
        wt = full
    n, C = a.shape[:2]
    acc = np.zeros((n, wt.shape[0], 3, 3), np.float32)
    pad = np.zeros((n, C, 5, 5))
    pad[:, :, 1:4, 1:4] = a
    groups = [(g, min(g + 32, n_main)) for g in range(0, n_main, 32)] + ([(n_main, C)] if C > n_main else [])
    for lo, hi in groups:
        for t, (dy, dx) in enumerate(TAPS):
            shifted = pad[:, lo:hi, 1 + dy:4 + dy, 1 + dx:4 + dx]             # [n, c, oy, ox] = a[.., oy + dy, ox + dx]
            part = np.einsum("ncyx,oc->noyx", shifted, wt[:, lo:hi, t // 3, t % 3])
            acc = (acc.astype(np.float64) + part).astype(np.float32)
    return acc


def flipped_share(case, x, w=None):
    """Per conv application whose output is stored as bf16: the share of its values whose rounding differs between the
    float64 result and the kernel-order float32 result, both from the emulation's own stored inputs (numpy's float32
    tanh / expm1 stand in for the device's).  [(application index, share)]."""
    w = tc.weights(case) if w is None else w
    wr = [rne_bf16(np.asarray(t)) for t in w.values()]
    xr = rne_bf16(np.asarray(x, np.float64))
    secs = emulate(case, x, w, sections=True)[3]
    out = []
    for i, s in enumerate(secs):
        if s.rows32:
            continue
        a = xr if s.src < 0 else secs[s.src].out
        n_main = 0 if s.src < 0 else a.shape[1]
        if s.planes and s.src >= 0:
            a = np.concatenate([a, xr], axis=1)
        y = conv32_kernel_order(a, wr[s.tensor], n_main)
        if s.res >= 0:
            y = y + secs[s.res].out.astype(np.float32)
        with np.errstate(over="ignore"):
            y = {0: lambda v: v, 1: lambda v: np.maximum(v, np.float32(0)), 2: np.tanh,
                 3: lambda v: np.where(v > 0, v, np.expm1(np.minimum(v, np.float32(0))))}[s.act](y)
        assert y.dtype == np.float32
        out.append((i, float(np.mean(rne_bf16(y) != s.out))))
    return out


def weight_stream(wt, cin_main):
    """The mode's main weight stream of one conv tensor, restated: uint32 [tile][K group][tap][lane][4]; word j of lane l
    holds input channels 32 g + 8 (l >> 4) + 2 j (low half) and + 1 (high half) of output channel 16 tile + (l & 15), each
    weight rounded to nearest even, zero where padding (engine.hip pack_conv)."""
    k = np.asarray(wt, np.float32)
    cout, cin = k.shape[:2]
    ntiles, kg = (cout + 15) // 16, (cin_main + 31) // 32
    dense = np.zeros((ntiles * 16, kg * 32 + 2, 9), np.float32)
    if k.shape[-1] == 1:
        dense[:cout, :cin_main, 4] = k[:, :cin_main, 0, 0]
    else:
        dense[:cout, :cin_main, :] = k[:, :cin_main].reshape(cout, cin_main, 9)
    bits = bf16_bits(dense)
    lane = np.arange(64)
    out = np.zeros((ntiles, kg, 9, 64, 4), np.uint32)
    for nt in range(ntiles):
        for g in range(kg):
            for j in range(4):
                co, ci = nt * 16 + (lane & 15), g * 32 + (lane >> 4) * 8 + 2 * j
                out[nt, g, :, :, j] = (bits[co, ci, :] | (bits[co, ci + 1, :] << 16)).T
    return out
