"""tests/replay_ref.py (the numpy model tests/test_gpu_replay_edges.py holds the replay kernels to) against what it
restates: the traces of the genuine ReplayBuffer class (tests/golden/replay_kat.json, `content`), the host list
(nuzero_amd/replay_buffer.py) through a batch that evicts its own earlier positions, torch.tensor(list of Python floats)
on counts whose sum needs 64 bits.  All comparisons are on bit patterns.  No GPU, no library."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import replay_ref  # noqa: E402
from replay_ref import ReplayModel, same_bits  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")


def test_model_equals_the_genuine_reference_contents():
    """The `content` case (five games through a window of three), games built as
    test_device_buffer_contents_equal_the_genuine_reference builds them, slots from ReplayIndex.save_games, ready-made
    float32 policies: identity, value, game index and policy_f32 of every entry."""
    from nuzero_amd.replay_device import ReplayIndex
    from test_gpu_replay_loss import _Game
    with open(os.path.join(GOLDEN, "replay_kat.json")) as f:
        case = json.load(f)["content"]
    rs = np.random.RandomState(case["seed"])
    games = [_Game(g, int(rs.randint(2, 6)), 9, rs) for g in range(5)]
    assert [len(g.state_history) for g in games] == case["lengths"]
    index, model = ReplayIndex(case["window"], 24), ReplayModel(24, 2, 9)
    for g in games:
        n = len(g.state_history)
        dst = index.save_games([n], g.gid % 2)
        states = torch.cat([g.get_state_from_history(i).reshape(1, -1) for i in range(n)], 0).numpy()
        policies = torch.tensor([g.make_target(i)[1] for i in range(n)]).numpy()          # AlphaZero.py:901
        model.append(states, None, policies, None, None, None, 0, [g.value], n, dst.reshape(-1), n, g.gid % 2)
    states, policies, values, gi = model.gather(index.seq)
    assert model.flags == 0 and len(index.seq) == len(case["content"])
    for i, want in enumerate(case["content"]):
        assert [int(states[i, 0]), int(states[i, 1]), int(gi[i])] == want["id"]
        assert values[i] == want["value"]
        assert same_bits(policies[i], np.asarray(want["policy_f32"], np.float32))


def test_model_equals_the_host_list_through_a_self_evicting_batch():
    """Window of 3 games; one batch of 40 games, which evicts its own earlier positions (ReplayIndex blanks them: of 295
    positions 30 are stored, 36 games are dropped whole), then 5 games under another game index.  The model, filled
    through ReplayIndex with dense visit counts and read in index.seq order, equals the host list fed GameRecords."""
    from nuzero_amd.gamer import GameRecord
    from nuzero_amd.replay_buffer import ReplayBuffer
    from nuzero_amd.replay_device import ReplayIndex
    W, T, A = replay_ref.SCHEDULE_WINDOW, replay_ref.SCHEDULE_T, replay_ref.SCHEDULE_A
    S = int(np.prod(replay_ref.SCHEDULE_SHAPE))
    host, index, model = ReplayBuffer(W, 32), ReplayIndex(W, W * T), ReplayModel(W * T, S, A)
    for n_batch, (game_index, lengths, states, visits, outcomes) in enumerate(replay_ref.schedule_batches()):
        G = len(lengths)
        for g in range(G):
            host.save_game(GameRecord(states[g], visits[g], np.zeros(T, np.int32), lengths[g], outcomes[g]), game_index)
        dst = np.full((G, T), -1, np.int64)
        kept = index.save_games(lengths, game_index)
        dst[:, :kept.shape[1]] = kept
        if n_batch == 0:
            assert G == 40 and int(lengths.sum()) == 295 and int((dst >= 0).sum()) == 30
            assert int((dst >= 0).any(axis=1).sum()) == 4
        model.append(states.reshape(G * T, S), visits.reshape(G * T, A), None, None, None, None, 0, outcomes, T,
                     dst.reshape(-1), G * T, game_index)
    got = model.gather(index.seq)
    want = host.get_buffer()
    assert model.flags == 0 and len(want) == len(index.seq) == 30
    assert sorted(set(got[3].tolist())) == [0, 1]
    for i, (state, (value, policy), game_index) in enumerate(want):
        assert same_bits(got[0][i], state.reshape(-1).numpy())
        assert same_bits(got[1][i], torch.tensor(policy).numpy())
        assert got[2][i] == value and got[3][i] == game_index


def test_dense_and_sparse_forms_give_the_same_bits():
    rs = np.random.RandomState(21)
    N, A, mc = 12, 300, 64
    visits = (rs.randint(1, 1000, (N, A)) * (rs.random_sample((N, A)) < 0.15)).astype(np.int32)
    visits[3] = 0                                     # a row without visits: zeros in both forms
    ca, cv = replay_ref.sparse_lists(rs, N, A, mc, np.zeros(N, int))
    counts = np.zeros(N, np.int32)
    for r in range(N):
        acts = rs.permutation(np.nonzero(visits[r])[0])[:mc - 2]
        visits[r][np.setdiff1d(np.arange(A), acts)] = 0
        zero = np.setdiff1d(np.arange(A), acts)[:2]          # two listed children nobody visited
        listed = np.concatenate([acts, zero])
        counts[r] = len(listed)
        ca[r, :len(listed)], cv[r, :len(listed)] = listed, visits[r][listed]
    states, slots = np.zeros((N, 1), np.float32), np.arange(N)
    dense, sparse = ReplayModel(N, 1, A), ReplayModel(N, 1, A)
    dense.append(states, visits, None, None, None, None, 0, np.zeros(N, np.int32), 1, slots, N, 0)
    sparse.append(states, None, None, ca, cv, counts, mc, np.zeros(N, np.int32), 1, slots, N, 0)
    assert dense.flags == 0 and sparse.flags == 0
    assert same_bits(dense.policies, sparse.policies)
    assert not dense.policies[3].any() and np.count_nonzero(dense.policies) == int(np.count_nonzero(visits)) > 100


def test_counts_whose_sum_needs_64_bits():
    """256 counts of 2**31 - 1 and a single 1: the total is above 2**32; the policy is torch.tensor of the quotients."""
    visits = np.full((1, 257), 2 ** 31 - 1, np.int32)
    visits[0, 100] = 1
    total = 256 * (2 ** 31 - 1) + 1
    assert total > 2 ** 32
    model = ReplayModel(1, 1, 257)
    model.append(np.zeros((1, 1), np.float32), visits, None, None, None, None, 0, [0], 1, [0], 1, 0)
    assert same_bits(model.policies[0], torch.tensor([int(v) / total for v in visits[0]]).numpy())
    assert model.policies[0, 100] > 0


def test_bad_input_raises_the_flags_and_is_skipped():
    model = ReplayModel(4, 2, 3)
    states = replay_ref.distinct_floats(np.random.RandomState(1), (4, 2), 1.0)
    ca = np.array([[0, 3], [1, -1], [2, 0], [1, 2]], np.int32)
    cv = np.array([[2, 2], [5, 5], [1, 3], [0, 0]], np.int32)
    model.append(states, None, None, ca, cv, [2, 2, 3, 2], 2, [1, -1], 2, [0, 4, 2, 3], 4, 6)
    assert model.flags == replay_ref.FLAG_SLOT | replay_ref.FLAG_ACTION
    assert model.policies.tolist() == [[0.5, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]]      # 2 / (2 + 2); count 3 > 2; 0 / 0
    assert model.values.tolist() == [1, 0, -1, -1] and model.game_index.tolist() == [6, 0, 6, 6]
    assert same_bits(model.states[[0, 2, 3]], states[[0, 2, 3]]) and not model.states[1].any()
    out = model.gather([3, 4, -1, 0], values_out=np.full(4, 9, np.float32))
    assert model.flags == 7 and out[2].tolist() == [-1, 9, 9, 1]


def test_the_grid_covers_every_pair():
    cases = replay_ref.pairwise_cases()
    factors = (replay_ref.STATE_FLOATS, replay_ref.NUM_ACTIONS, replay_ref.FORMS, replay_ref.N_ROWS,
               replay_ref.ROWS_PER_GAME)
    for i in range(len(factors)):
        for j in range(i + 1, len(factors)):
            assert {(c[i], c[j]) for c in cases} == {(a, b) for a in factors[i] for b in factors[j]}
    assert len(cases) <= 45 and cases == replay_ref.pairwise_cases()
