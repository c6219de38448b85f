"""What has to hold, before any device is involved, for tests/test_gpu_scs_deep_paths.py to mean something (cases:
tests/scs_deep.py): the oracle alone (oracle/search.py + oracle/scs.py) plays every case and reports, from its own
counters, how deep its descents went.  A path's length is its number of nodes, the root included: `plen` in the kernels.

For each case and each game:
  * paths of every length from 60 to 70 end in a leaf that needs an evaluation, so plen = 63, 64, 65 and 66 are all
    pending-leaf lengths (where the device routes switch from a path entry per lane to the tail in memory);
  * at least 20 simulations run on paths longer than 64.
These are conditions, not measurements: a case that does not meet them is replaced.

Printed (pytest -s): the longest path, the simulations and the terminal leaves on paths longer than 64, and the live
tree's peak node count per game.  Measured: terminal leaves past 64 levels do occur (16 in the evaluation-mode game of
the host evaluator, 40 and 114 in the network case's games, none in the others), so the whole-path backup of a terminal
leaf is walked past its first stride on the wave route and the register + tail backup on the persistent one.  No path
reaches 128 levels (the longest is 87; 89 on the reference's own test config with 300 simulations, 142 s of oracle
time): the second stride of the tail backup still rests on reading the code.

Also here: the float32 oracle of the peaked network against the float64 one (the room the device tests' 1e-5 has), the
measures themselves against a recount, and the peaked evaluator's stated properties.  No GPU."""
import numpy as np
import pytest

import scs_deep
from scs_deep import deep_jobs, oracle_games, pending_leaves, simulations_deeper_than

CASES = scs_deep.HOST_EVAL_CASES + scs_deep.NET_CASES


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-{'training' if c[1] else 'evaluation'}" for c in CASES])
def test_the_oracle_goes_past_64_levels_on_every_deep_case(case):
    oracle_games(deep_jobs(CASES))                  # every case's games side by side, once; then this case's own
    jobs = deep_jobs([case])
    for job, out in zip(jobs, oracle_games(jobs)):
        seed = job[2]
        deep, deep_terminal = simulations_deeper_than(out, 64), simulations_deeper_than(out, 64, terminal=True)
        print(f"\n{case[0]} training={case[1]} seed {seed}: {out['length']} decisions, longest path {out['longest_path']}, "
              f"{deep} simulations on paths > 64 ({deep_terminal} of them to a terminal leaf), "
              f"pending leaves at 60..70: {[pending_leaves(out, n) for n in range(60, 71)]}, peak nodes {out['peak_nodes']}")
        assert out["terminal"] and sum(out["path_lengths"].values()) == scs_deep.SIMS * out["length"]
        for n in range(60, 71):
            assert pending_leaves(out, n) > 0, (seed, n)
        assert deep >= 20, seed
        assert out["longest_path"] < 128        # (the module docstrings say so: a case that gets there widens the claim)


def test_the_float32_oracle_of_the_peaked_net_leaves_the_device_room():
    """The device tests hold the peaked network's probabilities to the float32 oracle at the project's 1e-5.  Logits of
    the size that makes the searches go deep (up to 130) cost float32 arithmetic precision: the comparison has room only
    if the float32 oracle itself stays within half the bound of the float64 one, so that a device as accurate as float32
    fits in the other half.  On every root position of both games: 0.31e-5 (a dense net that goes as deep: 1.4e-5;
    tests/scs_deep.py: peaked_net_weights)."""
    import torch
    from scipy.special import softmax
    from oracle.net import FeedForwardRef
    from oracle.scs import ScsConfig, ScsGame
    cfg = ScsConfig(scs_deep.NET_CONFIG)
    images = []
    for out in oracle_games(deep_jobs(scs_deep.NET_CASES)):
        game = ScsGame(cfg)
        for mv in out["trace"]:
            images.append(game.state_image()[0].copy())
            game.step_index(mv["action"])
    x = np.stack(images)
    arch, _, depth, vact = scs_deep.NET
    w = scs_deep.peaked_net_weights(cfg.channels, cfg.planes)
    p32, v32 = FeedForwardRef(w, arch, depth, vact).inference(x)
    p64, v64 = FeedForwardRef(w, arch, depth, vact, dtype=torch.float64).inference(x)
    dp = float(np.abs(softmax(p32.reshape(len(x), -1), axis=1) - softmax(p64.reshape(len(x), -1), axis=1)).max())
    dv = float(np.abs(v32 - v64).max())
    print(f"\n{len(x)} root positions, largest |logit| {np.abs(p64).max():.1f}: float32 oracle against float64, probabilities "
          f"{dp:.3g}, values {dv:.3g}; values {v64.min():.3f} .. {v64.max():.3f}")
    assert dp < 0.5e-5 and dv < 0.5e-5
    assert np.abs(p64).max() > 50 and v64.min() > 0.5                  # (peaked, and a positive value everywhere)


def test_path_and_node_measures_equal_a_recount():
    """Counters' histogram and peak node count on a short search, against a count made here: every simulation's path is
    one longer than the number of steps its scratch game took, and the live tree is the root plus every child list."""
    from oracle import search as osearch
    from oracle.scs import ScsConfig, ScsGame
    from scs_eval import evaluate_image_peaked
    game = ScsGame(ScsConfig(scs_deep.CONFIG))
    A = game.get_num_actions()
    steps, seen = [], []

    def ev(gm):
        seen.append(gm.length)
        return evaluate_image_peaked(gm.state_image()[0], A)

    search = scs_deep.deep_search(40)
    explorer = osearch.Explorer(search, True, np.random.RandomState(5))
    root = osearch.Node(0)
    peak = 0
    for move in range(4):
        before = len(seen)
        start = game.length
        action, chosen, _ = explorer.run_mcts(game, ev, root)
        steps += [d - start + 1 for d in seen[before:]]          # (no terminal leaf this early: every simulation evaluates)

        def count(n):
            return len(n.children) + sum(count(c) for c in n.children)
        peak = max(peak, 1 + count(root))
        assert osearch.live_nodes(root) == 1 + count(root)
        game.step_index(action)
        root = chosen
    c = explorer.counters
    assert c.simulations == 160 == len(steps) and not c.terminal_path_lengths
    assert c.path_lengths == {n: steps.count(n) for n in set(steps)}
    assert c.longest_path == max(steps) and c.peak_nodes == peak
    assert c.simulations_deeper_than(3) == sum(n > 3 for n in steps)


def test_the_peaked_evaluator_ranks_without_ties_and_stays_normal():
    from oracle.scs import ScsConfig, ScsGame
    from scs_eval import evaluate_image, evaluate_image_peaked
    game = ScsGame(ScsConfig(scs_deep.CONFIG))
    A = game.get_num_actions()
    img = game.state_image()[0]
    p, v = evaluate_image_peaked(img, A)
    assert p.dtype == np.float32 and p.shape == (A,) and isinstance(v, np.float32)
    assert len(np.unique(p)) == A and p.min() >= np.finfo(np.float32).tiny
    assert abs(float(p.sum(dtype=np.float64)) - 1.0) < 1e-5 and 0.89 <= float(v) <= 0.91
    legal = np.sort(p[np.nonzero(game.possible_actions().reshape(-1))[0]])[::-1]
    assert legal[0] > 0.5 * legal.sum()                         # the best legal action clearly dominates here
    p2, v2 = evaluate_image_peaked(img.copy(), A)                # a pure function of the image
    assert np.array_equal(p, p2) and v == v2
    assert np.array_equal(evaluate_image(img, A)[0], evaluate_image(img.copy(), A)[0])
