"""The edge-shape cases the board nets (nz_boardnet_*, nuzero_amd/csrc/boardnet.hip) are held at, shared by
tests/test_boardnet_ref_host.py (which shows, without a device, that the float64 reference and these inputs can carry
a 1e-5 bound), tests/test_gpu_boardnet_edges.py (the device against the float64 reference) and
scripts/boardnet_edge_errors.py (the measured figures).  A plain module: no fixtures, nothing collected from it.

Every case names the kernels it is there to reach; test_boardnet_ref_host.py checks those claims against a
restatement of the library's dispatch rules."""
import collections

import numpy as np

TOL = 1e-5                    # BASELINE.json north_star; TOL of tests/test_gpu_boardnet.py
REF32_SHARE = 0.2             # the float32 oracle may use this share of TOL against the float64 one
STANDARD_BATCHES = (1, 15, 16, 17, 37)
SHARED_MAX_BATCH = 300        # the second handle every standard case runs on

Case = collections.namedtuple("Case", [
    "name", "arch", "hex", "in_channels", "policy_channels", "rows", "cols", "width", "depth", "recall",
    "value_activation", "iters", "kernel_size", "seed", "gain",
    "batches",        # batch sizes run with max_batch == n and on a handle with max_batch == SHARED_MAX_BATCH
    "big_batches",    # batch sizes run with max_batch == n and the one-launch form off (per-layer kernels)
    "reaches",        # what the case is in the table for
    "flat_ok",        # None, or the measured figures that excuse the case from the sharpness condition
])


def _case(name, arch, cin, planes, rows, cols, width, depth, k, gain, seed, reaches, recall=False, vact="tanh", iters=1,
          hex=False, batches=STANDARD_BATCHES, big=(), flat_ok=None):
    return Case(name, arch, hex, cin, planes, rows, cols, width, depth, recall, vact, iters, k, seed, gain,
                tuple(batches), tuple(big), reaches, flat_ok)


# Gains were settled on the CPU oracle alone, in steps of 0.5, until the sharpness condition and the float32 condition of
# test_boardnet_ref_host.py both held: no_blocks_res (largest probability 0.02 at 3.0, 0.18 at 4.0) and no_blocks_conv
# (0.04 at 3.0, 0.16 at 3.5) were raised, hex_odd (largest probability 1.0000 at 3.0) was lowered.  strip_col and
# wide_nonsquare hold at their starting gains with these seeds (largest probability 0.24 at 4.0 and 0.29 at 3.0, where
# other draws were flat), and the added res_narrow at 3.0 (0.36).
CASES = [
    _case("k1_scs", "convnet", 86, 21, 5, 5, 32, 2, 1, 3.0, 101, "pack k=1; fused16 and per-layer; MT=2 at n=2060",
          big=(2060,)),
    _case("k1_odd", "convnet", 7, 3, 4, 9, 24, 3, 1, 3.0, 102, "k=1, width not a multiple of 16, non-square board",
          vact="relu"),
    _case("strip_row", "convnet", 1, 1, 1, 7, 8, 1, 3, 6.0, 103, "one-row board, 1 input plane, 1 policy plane"),
    _case("strip_col", "resnet", 17, 5, 7, 1, 40, 2, 3, 4.0, 104,
          "one-column board, 3 tiles with 8 padded channels, residual on padding"),
    _case("two_by_two", "resnet", 3, 1, 2, 2, 20, 1, 3, 4.0, 105, "every cell a corner", vact="relu"),
    _case("res_narrow", "resnet", 5, 2, 3, 4, 12, 1, 3, 3.0, 116,
          "fused16 ResNet narrower than a 32-channel K group: trunk buffers past the input pieces, half-written rows"),
    _case("rec_odd", "recurrent", 33, 2, 3, 11, 24, 1, 3, 3.0, 106,
          "fused_net_kernel, two K sources with padding in both; MT=2 NT=1 at n=2060", recall=True, iters=3,
          big=(2060,)),
    _case("rec_64", "recurrent", 86, 21, 8, 8, 72, 2, 3, 2.5, 107, "hw = 64, five column tiles (NT = 1)", recall=True,
          vact="relu", iters=2),
    _case("rec_65", "recurrent", 5, 30, 13, 5, 16, 1, 3, 3.0, 108, "hw = 65, one column tile, policy planes > width",
          iters=2),
    _case("rec_mt2", "recurrent", 86, 21, 3, 5, 64, 1, 3, 3.0, 115,
          "conv_kernel<2,4>: four tiles, ten K groups, n >= 1024 with an odd count of 16-groups", recall=True, iters=2,
          batches=(), big=(1030, 37)),
    _case("nt3", "convnet", 86, 21, 7, 9, 96, 2, 3, 3.0, 109, "six tiles (NT = 3), no fused16 (coutp > 64)"),
    _case("no_blocks_res", "resnet", 86, 21, 5, 5, 80, 0, 3, 4.5, 110, "depth 0, five tiles"),
    _case("no_blocks_conv", "convnet", 86, 21, 5, 5, 32, 0, 3, 4.0, 111, "fused16 with n_trunk == 1"),
    _case("wide_nonsquare", "resnet", 86, 21, 4, 9, 128, 1, 3, 3.0, 112,
          "conv_wide_kernel on a non-square board, ragged last tile; n = 37: the same layers on conv_kernel",
          batches=(), big=(1040, 37)),
    _case("wide_recall", "recurrent", 86, 21, 3, 11, 256, 1, 3, 3.0, 113,
          "conv_wide_kernel, two sources, two 128-channel tiles; n = 37: the same layers on conv_kernel", recall=True,
          vact="relu", iters=2, batches=(), big=(530, 37),
          # no gain in steps of 0.5 is both sharp and unsaturated: at 2.5 the largest probability is 0.017 and the largest
          # |value| 0.51; at 3.0 they are 0.68 and 0.9935 (float32 oracle's value error there: 3.5e-8).  3.0 is kept.
          flat_ok={"value_max": 0.995}),
    _case("hex_odd", "convnet", 7, 3, 4, 9, 24, 2, 1, 2.5, 114, "7-tap form on the same edges (parity unpinned)",
          hex=True),
]
BY_NAME = {c.name: c for c in CASES}


def shapes(case):
    from nuzero_amd.weights import (convnet_param_shapes, hex_param_shapes, recurrent_net_param_shapes,
                                    resnet_param_shapes)
    if case.arch == "recurrent":
        s = recurrent_net_param_shapes(case.in_channels, case.policy_channels, case.width, case.depth, case.recall)
    elif case.arch == "resnet":
        s = resnet_param_shapes(case.in_channels, case.policy_channels, case.width, case.depth)
    else:
        s = convnet_param_shapes(case.in_channels, case.policy_channels, 3 if case.hex else case.kernel_size, case.width,
                                 case.depth)
    return hex_param_shapes(s) if case.hex else s


def weights(case, seed=None, gain=None):
    from nuzero_amd.weights import synthetic_weights
    return synthetic_weights(case.seed if seed is None else seed, shapes(case), case.gain if gain is None else gain)


def inputs(case, n, offset=0):
    """As the existing board-net tests draw them: 15 % binary planes, the last min(3, in_channels) planes uniform in
    [0, 1).  The two kinds come from two streams, so the first m positions of a draw of n are the draw of m."""
    rs = np.random.RandomState(2000 + case.seed + offset)
    x = (rs.random_sample((n, case.in_channels, case.rows, case.cols)) < 0.15).astype(np.float32)
    k = min(3, case.in_channels)
    rs = np.random.RandomState(7000 + case.seed + offset)
    x[:, -k:] = rs.random_sample((n, k, case.rows, case.cols)).astype(np.float32)
    return x


def all_batches(case):
    return tuple(sorted(set(case.batches) | set(case.big_batches)))


def oracle(case, w=None, dtype=None):
    import torch
    from oracle.net import FeedForwardRef, HexNetRef, RecurrentNetRef
    dtype = torch.float32 if dtype is None else dtype
    w = weights(case) if w is None else w
    if case.hex:
        return HexNetRef(w, case.arch, case.depth, case.recall, case.value_activation, dtype=dtype)
    if case.arch == "recurrent":
        return RecurrentNetRef(w, case.in_channels, case.policy_channels, case.width, case.depth, case.recall,
                               case.value_activation, dtype=dtype)
    return FeedForwardRef(w, case.arch, case.depth, case.value_activation, dtype=dtype)


def reference64(case, x, w=None):
    """(logits [n, A], probs [n, A], value [n]) of the float64 oracle, as float64 arrays."""
    import torch
    ref = oracle(case, w, torch.float64)
    with torch.no_grad():
        p, v = ref.forward(x, case.iters) if (case.hex or case.arch == "recurrent") else ref.forward(x)
    logits = p.numpy().reshape(len(x), -1)
    return logits, softmax64(logits), v.numpy().reshape(-1)


def reference32(case, x, w=None):
    """The same from the float32 oracle (the reference's own arithmetic), softmax in float32."""
    p, v = oracle(case, w).inference(x, case.iters)
    logits = p.reshape(len(x), -1)
    e = np.exp(logits - logits.max(axis=1, keepdims=True), dtype=np.float32)
    return logits, e / e.sum(axis=1, keepdims=True, dtype=np.float32), v.reshape(-1)


def softmax64(logits):
    logits = np.asarray(logits, np.float64)
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def errors(logits, probs, value, want):
    """The project's three measures against `want` = (logits, probs, value) of the float64 reference: logits relative to
    max|logit| + 1 of the position, probabilities absolute, values absolute.  Each the worst over the batch."""
    wl, wp, wv = want
    scale = np.abs(wl).max(axis=1, keepdims=True) + 1.0
    out = {"value": float(np.max(np.abs(np.asarray(value, np.float64) - wv)))}
    if logits is not None:
        out["logit"] = float(np.max(np.abs(np.asarray(logits, np.float64) - wl) / scale))
    if probs is not None:
        out["prob"] = float(np.max(np.abs(np.asarray(probs, np.float64) - wp)))
    return out
