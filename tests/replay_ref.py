"""A plain numpy model of the device replay buffer (nuzero_amd/csrc/replay.hip, C ABI nz_replay_*): what every slot holds
after a sequence of nz_replay_append calls, what nz_replay_gather returns, and which error flags the kernels raise.  No
GPU, no library; plain Python loops over rows.  tests/test_replay_ref_host.py pins the model to the genuine ReplayBuffer
class's traces and to the host list; tests/test_gpu_replay_edges.py holds the kernels to the model, bit for bit.

The buffer moves data; its one computation is the policy target, visit / sum(visits) in double, rounded once to float32
(what torch.tensor(list of Python floats) gives, AlphaZero.py:901).  Rules on bad input, as include/nuzero_amd.h states
them: a slot at or beyond capacity raises flag 1 and the row is skipped; a listed child whose action is outside 0 .. A-1
raises flag 2 and is skipped (its visits still count in the row's sum); a child count outside 0 .. max_children raises flag
2 and counts as 0; a batch slot outside 0 .. capacity-1 raises flag 4 and leaves the output row alone.

Also here, shared by the two test files: the seeded inputs (distinct floats with special bit patterns among them), the
pairwise covering of the shape grid, and the games of the self-evicting schedule.
"""
import itertools

import numpy as np

FLAG_SLOT, FLAG_ACTION, FLAG_BATCH_SLOT = 1, 2, 4


class ReplayModel:
    def __init__(self, capacity, state_floats, num_actions):
        self.capacity, self.state_floats, self.num_actions = int(capacity), int(state_floats), int(num_actions)
        self.states = np.zeros((self.capacity, self.state_floats), np.float32)
        self.policies = np.zeros((self.capacity, self.num_actions), np.float32)
        self.values = np.zeros(self.capacity, np.float32)
        self.game_index = np.zeros(self.capacity, np.int32)
        self.flags = 0

    def append(self, states, visits, policies, child_action, child_visit, n_children, max_children, game_value,
               rows_per_game, dst_slot, n_rows, game_index):
        """nz_replay_append with host arrays: states [N, state_floats], one of visits [N, A] / policies [N, A] /
        (child_action, child_visit [N, max_children], n_children [N]), game_value [ceil(N / rows_per_game)], dst_slot [N]."""
        A = self.num_actions
        assert (visits is not None) + (policies is not None) + (child_action is not None) == 1 and rows_per_game > 0
        for r in range(int(n_rows)):
            slot = int(dst_slot[r])
            if slot < 0:
                continue
            if slot >= self.capacity:
                self.flags |= FLAG_SLOT
                continue
            self.states[slot] = states[r]
            if policies is not None:
                self.policies[slot] = policies[r]
            elif visits is not None:
                total = sum(int(v) for v in visits[r])
                for i in range(A):
                    v = int(visits[r][i])
                    self.policies[slot, i] = np.float32(np.float64(v) / np.float64(total)) if v != 0 else np.float32(0)
            else:
                k = int(n_children[r])
                if k < 0 or k > max_children:
                    self.flags |= FLAG_ACTION
                    k = 0
                total = sum(int(child_visit[r][i]) for i in range(k))
                self.policies[slot] = 0
                for i in range(k):
                    act, v = int(child_action[r][i]), int(child_visit[r][i])
                    if act < 0 or act >= A:
                        self.flags |= FLAG_ACTION
                        continue
                    self.policies[slot, act] = np.float32(np.float64(v) / np.float64(total)) if v != 0 else np.float32(0)
            self.values[slot] = np.float32(int(game_value[r // rows_per_game]))
            self.game_index[slot] = game_index

    def gather(self, slots, states_out=None, policies_out=None, values_out=None, game_index_out=None):
        """nz_replay_gather: the four outputs for the batch `slots`.  An output that is given is written in place (a row
        whose slot is out of range stays as it was); one that is not given is made here, zero-filled."""
        B = len(slots)
        if states_out is None:
            states_out = np.zeros((B, self.state_floats), np.float32)
        if policies_out is None:
            policies_out = np.zeros((B, self.num_actions), np.float32)
        if values_out is None:
            values_out = np.zeros(B, np.float32)
        if game_index_out is None:
            game_index_out = np.zeros(B, np.int32)
        for b in range(B):
            slot = int(slots[b])
            if slot < 0 or slot >= self.capacity:
                self.flags |= FLAG_BATCH_SLOT
                continue
            states_out[b] = self.states[slot]
            policies_out[b] = self.policies[slot]
            values_out[b] = self.values[slot]
            game_index_out[b] = self.game_index[slot]
        return states_out, policies_out, values_out, game_index_out


def same_bits(a, b):
    """Equal as bit patterns (float32 compared as uint32: NaN payloads and the sign of zero count)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    return bool(np.array_equal(a, b))


# -0.0, the smallest and the largest denormal, +inf, -inf, a quiet NaN with a payload, a negative NaN with another
SPECIAL_BITS = np.array([0x80000000, 0x00000001, 0x007FFFFF, 0x7F800000, 0xFF800000, 0x7FC12345, 0xFFC00001], np.uint32)


def distinct_floats(rs, shape, offset, specials=True):
    """Seeded float32 values, all distinct (a permutation of k / 4 + offset, exact in float32), with every 5th element
    replaced by one of SPECIAL_BITS in turn: a copy must keep each bit."""
    n = int(np.prod(shape))
    x = (rs.permutation(n).astype(np.float64) * 0.25 + offset).astype(np.float32)
    if specials:
        at = np.arange(0, n, 5)
        x.view(np.uint32)[at] = SPECIAL_BITS[np.arange(len(at)) % len(SPECIAL_BITS)]
    return x.reshape(shape)


# ---- the shape grid -----------------------------------------------------------------------------------------------
STATE_FLOATS = (1, 255, 256, 257, 513)
NUM_ACTIONS = (1, 2, 255, 256, 257, 600)
FORMS = ("dense", "ready", "sparse1", "sparse64", "sparse300")          # sparse<max_children>
N_ROWS = (1, 7, 300)
ROWS_PER_GAME = (1, 3, "all")                                             # "all": rows_per_game = n_rows


def pairwise_cases():
    """A pairwise covering of STATE_FLOATS x NUM_ACTIONS x FORMS x N_ROWS x ROWS_PER_GAME: every value of every factor
    meets every value of every other factor in at least one case.  Greedy and deterministic: always the case of the full
    product, in product order, that covers the most pairs not covered yet."""
    factors = (STATE_FLOATS, NUM_ACTIONS, FORMS, N_ROWS, ROWS_PER_GAME)
    product = list(itertools.product(*factors))
    pairs_of = lambda case: {(i, case[i], j, case[j]) for i in range(len(case)) for j in range(i + 1, len(case))}
    todo = set().union(*(pairs_of(c) for c in product))
    cases = []
    while todo:
        best = max(product, key=lambda c: len(pairs_of(c) & todo))     # max keeps the first of equals
        cases.append(best)
        todo -= pairs_of(best)
    return cases


def sparse_lists(rs, n_rows, A, max_children, counts, visit_low=0, visit_high=50):
    """Child lists for the sparse form: row r lists counts[r] children with distinct actions and visits in
    [visit_low, visit_high); the entries beyond are out-of-range garbage (actions and visits), which must be ignored."""
    ca = rs.choice([-7, A, A + 3, 2 ** 31 - 1, -2 ** 31], size=(n_rows, max_children)).astype(np.int32)
    cv = rs.choice([-5, 2 ** 31 - 1, 123456789], size=(n_rows, max_children)).astype(np.int32)
    for r in range(n_rows):
        k = int(counts[r])
        ca[r, :k] = rs.permutation(A)[:k]
        cv[r, :k] = rs.randint(visit_low, visit_high, size=k)
    return ca, cv


# ---- the self-evicting schedule (window of 3 games; a batch of 40 games, then 5 more under another game index) ------
SCHEDULE_WINDOW, SCHEDULE_T, SCHEDULE_SHAPE, SCHEDULE_A = 3, 12, (5, 7, 11), 300


def schedule_batches():
    """[(game_index, lengths [G], states [G, T, 5, 7, 11] f32, visits [G, T, 300] i32, outcomes [G] i32)]: 40 games of
    lengths RandomState(3).randint(1, 13, 40), of which a window of 3 games keeps 30 of 295 positions (the batch evicts its
    own earlier positions), then 5 games of 27 positions, so that 3 positions of the first batch stay.  Every position of a game has at least one visited action."""
    out = []
    for game_index, G, seed in ((1, 40, 3), (0, 5, 8)):
        rs = np.random.RandomState(seed)
        lengths = rs.randint(1, SCHEDULE_T + 1, G).astype(np.int32)
        states = distinct_floats(rs, (G, SCHEDULE_T) + SCHEDULE_SHAPE, 1000.0 * game_index, specials=False)
        visits = (rs.randint(1, 200, (G, SCHEDULE_T, SCHEDULE_A)) * (rs.random_sample((G, SCHEDULE_T, SCHEDULE_A)) < 0.1))
        visits[:, :, 17] += 1
        outcomes = rs.randint(-1, 2, G).astype(np.int32)
        out.append((game_index, lengths, states, visits.astype(np.int32), outcomes))
    return out
