"""The cases the fused 3x3 network pass (net_dev.hpp net_tile, net_packed_dev.hpp net_tile_packed, and the compilers
compile_net, solo_list and compile_net_packed of engine.hip) is held at over its program space, shared by
tests/test_tttnet_ref_host.py (which shows, without a device, that the float64 reference and these inputs can carry a
1e-5 bound and that the table reaches the programs it claims), tests/test_gpu_tttnet_edges.py (the device against the
float64 reference), scripts/tttnet_edge_errors.py (the measured figures) and the host checks of the compiled programs
(tests/test_solo_lists.py, tests/test_net_packed_host.py, tests/test_gpu_progressive_epilogue.py).  A plain module: no
fixtures, nothing collected from it."""
import collections

import numpy as np

from boardnet_cases import TOL, REF32_SHARE, softmax64, errors   # noqa: F401  (one statement of the bound and the measures)

BATCHES = (1, 15, 16, 17, 37)
MAX_BATCH = 37

Case = collections.namedtuple("Case", [
    "name", "arch", "width", "num_blocks", "recall", "iters", "value_activation", "kernel_size", "seed", "gain",
    "policy_scale",   # None, or a factor on the policy head's last conv
    "reaches",        # what the case is in the table for
    "flat_ok",        # None, or the measured figures that excuse the case from the sharpness condition
])


def _case(name, arch, width, blocks, recall, iters, vact, k, seed, gain, reaches, policy_scale=None, flat_ok=None):
    return Case(name, arch, width, blocks, bool(recall), iters, vact, k, seed, gain, policy_scale, reaches, flat_ok)


# Gains were settled on the CPU oracle alone, from 3.0 in steps of 0.5, until the sharpness condition and the float32
# condition of test_tttnet_ref_host.py both held.  Lowered to 2.5: rec_norecall_64 (largest probability 0.999 at 3.0),
# rec_norecall_20 (largest probability and largest |value| 1.000 at 3.0), rec_blocks3 (largest probability 1.000 at 3.0)
# and the added rec_44 (0.9995 and 0.993 at 3.0; 0.73 and 0.36 at 2.5; flat at 2.0).  Raised to 3.5: res_36_b0 (largest
# |logit| 1.7 at 3.0), conv_12 (1.8 at 3.0), conv_k1_4 (largest |value| 0.19 at 3.0).
# Two cases got another SEED, because no gain would do.  rec_iters5 with seed 208: flat at 2.0 (largest probability 0.15),
# largest |value| 0.16 at 2.5, saturated at 3.0 (largest probability 1.000, and the float32 oracle's value 2.8e-6 off);
# with seed 226 at 2.5 it is 0.73 and 0.28.  large_logits: with logits of several hundred the float32 oracle's own
# logits are some 1e-4 off in absolute terms, so wherever the two largest logits of a position are within a few units
# of each other its probabilities are up to 2.6e-5 off (seeds 219 to 231 at gain 3.0: eleven of thirteen miss 2e-6, at
# 2.0 and 2.5 seed 220 misses it too).  Seed 223 is the first after the table's whose positions keep the float32 oracle
# within the bound (2.9e-7; smallest gap between the two largest logits 5.1, so a second probability of 0.6 % is still
# there to be wrong).  The case is out of the probability window by construction; its figures are recorded.
CASES = [
    _case("rec_norecall_64", "recurrent", 64, 2, False, 2, "tanh", 3, 201, 2.5,
          "recall off at four tiles: halves, two K groups, no input-plane step after the projection; strip and split slot"),
    _case("rec_norecall_20", "recurrent", 20, 2, False, 3, "relu", 3, 202, 2.5,
          "recall off at two tiles with 12 padded channels, three iterations, relu value head"),
    _case("rec_norecall_4", "recurrent", 4, 1, False, 2, "tanh", 3, 203, 3.0,
          "the narrowest net: one tile with 12 padded channels, four waves with barrier-only jobs, one block"),
    _case("rec_blocks0", "recurrent", 36, 0, True, 3, "tanh", 3, 204, 3.0,
          "no blocks: the recall conv is the whole recurrent module, applied three times back to back; three tiles"),
    _case("rec_blocks1", "recurrent", 52, 1, True, 2, "relu", 3, 205, 3.0,
          "one block at four tiles with 12 padded channels; strip with 39 + 26 head channels"),
    _case("rec_blocks3", "recurrent", 28, 3, True, 2, "tanh", 3, 206, 2.5, "three blocks at two tiles; 2 + 1 head tiles"),
    _case("rec_iters0", "recurrent", 64, 2, True, 0, "tanh", 3, 207, 3.0,
          "zero iterations: projection and heads only, five stages; recall and block tensors packed but never run"),
    _case("rec_iters5", "recurrent", 12, 2, True, 5, "tanh", 3, 226, 2.5, "five iterations at one tile: 30 stages"),
    _case("res_4", "resnet", 4, 2, False, 1, "tanh", 3, 209, 3.0, "ResNet at one tile"),
    _case("res_20", "resnet", 20, 1, False, 1, "relu", 3, 210, 3.0, "ResNet at two tiles, relu value head"),
    _case("res_36_b0", "resnet", 36, 0, False, 1, "tanh", 3, 211, 3.5, "ResNet without blocks at three tiles: 2 + 2 head tiles"),
    _case("res_52_b3", "resnet", 52, 3, False, 1, "tanh", 3, 212, 3.0, "three residual blocks at four tiles with padding"),
    _case("res_64_relu", "resnet", 64, 2, False, 1, "relu", 3, 213, 3.0, "relu value head on a feed-forward net, full width"),
    _case("conv_12", "convnet", 12, 2, False, 1, "tanh", 3, 214, 3.5, "ELU at one tile"),
    _case("conv_44_relu", "convnet", 44, 1, False, 1, "relu", 3, 215, 3.0,
          "ELU in quarters of three tiles, two K groups; strip with 33 + 22 head channels (tiles of 1 and 6 live channels)"),
    _case("conv_60_b0", "convnet", 60, 0, False, 1, "tanh", 3, 216, 3.0, "the input-plane conv with ELU is the whole trunk"),
    _case("conv_k1_4", "convnet", 4, 3, False, 1, "tanh", 1, 217, 3.5, "k = 1 trunk at one tile, three layers"),
    _case("conv_k1_64", "convnet", 64, 2, False, 1, "relu", 1, 218, 3.0, "k = 1 trunk at full width, relu value head"),
    _case("conv_k1_40_b0", "convnet", 40, 0, False, 1, "tanh", 1, 219, 3.0, "k = 1 input-plane conv alone; 2 + 2 head tiles"),
    _case("large_logits", "recurrent", 64, 2, True, 2, "tanh", 3, 223, 3.0, "the softmax at logits 30 x as large (largest |logit| 329)",
          policy_scale=30.0, flat_ok={"prob_max": 1.0}),
    # added after reading add_stage: forms none of the above reaches
    _case("rec_44", "recurrent", 44, 2, True, 2, "relu", 3, 221, 2.5,
          "residual and recall jobs in QUARTERS at two K groups (three tiles: twelve units on eight waves, so waves hold "
          "two jobs of a stage), progressive quarters with two K groups"),
    _case("conv_56", "convnet", 56, 1, False, 1, "tanh", 3, 222, 3.0,
          "3x3 ELU in HALVES at two K groups (four tiles with 8 padded channels): the whole-tile ELU job of a stolen pass"),
]
BY_NAME = {c.name: c for c in CASES}


def net_tuple(case):
    """(arch, width, num_blocks, recall, iterations, value_activation, kernel_size): the shape as the host tests of the
    compiled programs list it."""
    return (case.arch, case.width, case.num_blocks, case.recall, case.iters, case.value_activation, case.kernel_size)


def program_shapes():
    """The distinct shapes of the table, in table order."""
    out = []
    for c in CASES:
        if net_tuple(c) not in out:
            out.append(net_tuple(c))
    return out


def shapes(case):
    from nuzero_amd.weights import convnet_param_shapes, recurrent_net_param_shapes, resnet_param_shapes
    if case.arch == "recurrent":
        return recurrent_net_param_shapes(2, 1, case.width, case.num_blocks, case.recall)
    if case.arch == "resnet":
        return resnet_param_shapes(2, 1, case.width, case.num_blocks)
    return convnet_param_shapes(2, 1, case.kernel_size, case.width, case.num_blocks)


def weights(case, seed=None, gain=None):
    from nuzero_amd.weights import synthetic_weights
    w = synthetic_weights(case.seed if seed is None else seed, shapes(case), case.gain if gain is None else gain)
    if case.policy_scale is not None:
        w["policy_head.layers.2.weight"] = w["policy_head.layers.2.weight"] * np.float32(case.policy_scale)
    return w


def inputs(case, n):
    """[n, 2, 3, 3] float32, n <= 37.  Position 0: both planes zero.  Position 1: both planes one (no legal board, but
    every tap is live).  Positions 2 to 5: uniform floats in [0, 1) with full mantissas.  The rest: random boards, each
    cell empty, X or O.  The kinds come from separate streams, so the first m positions of a draw of n are the draw of m."""
    assert 0 < n <= MAX_BATCH
    x = np.zeros((MAX_BATCH, 2, 3, 3), np.float32)
    x[1] = 1.0
    x[2:6] = np.random.RandomState(7000 + case.seed).random_sample((4, 2, 3, 3)).astype(np.float32)
    cells = np.random.RandomState(2000 + case.seed).randint(0, 3, size=(MAX_BATCH - 6, 3, 3))
    x[6:, 0] = cells == 1
    x[6:, 1] = cells == 2
    return x[:n].copy()


def oracle(case, w=None, dtype=None):
    import torch
    from oracle.net import FeedForwardRef, RecurrentNetRef
    dtype = torch.float32 if dtype is None else dtype
    w = weights(case) if w is None else w
    if case.arch == "recurrent":
        return RecurrentNetRef(w, 2, 1, case.width, case.num_blocks, case.recall, case.value_activation, dtype=dtype)
    return FeedForwardRef(w, case.arch, case.num_blocks, case.value_activation, dtype=dtype)


def reference64(case, x, w=None):
    """(logits [n, 9], probs [n, 9], value [n]) of the float64 oracle, as float64 arrays."""
    import torch
    ref = oracle(case, w, torch.float64)
    with torch.no_grad():
        p, v = ref.forward(x, case.iters) if case.arch == "recurrent" else ref.forward(x)
    logits = p.numpy().reshape(len(x), -1)
    return logits, softmax64(logits), v.numpy().reshape(-1)


def reference32(case, x, w=None):
    """The same from the float32 oracle (the reference's own arithmetic), softmax in float32."""
    p, v = oracle(case, w).inference(x, case.iters)
    logits = p.reshape(len(x), -1)
    e = np.exp(logits - logits.max(axis=1, keepdims=True), dtype=np.float32)
    return logits, e / e.sum(axis=1, keepdims=True, dtype=np.float32), v.reshape(-1)
