"""The replay kernels (nuzero_amd/csrc/replay.hip: append_kernel, gather_kernel) at the raw C ABI (nz_replay_* through
nuzero_amd._lib.lib) against the numpy model tests/replay_ref.py (pinned to the genuine ReplayBuffer class and the host
list by tests/test_replay_ref_host.py), at the shapes and inputs the games never produce.  Needs a GPU.

Nothing here has a tolerance: the buffer moves data, and its one computation, visit / sum(visits) in double rounded once to
float32, is exactly specified.  Every comparison is on bit patterns (float32 as uint32), inputs carry -0.0, denormals,
+-inf and NaN payloads, and are distinct values, so that a misplaced element shows.

* grid: a pairwise covering (replay_ref.pairwise_cases) of state_floats 1 / 255 / 256 / 257 / 513 x num_actions 1 / 2 / 255 /
  256 / 257 / 600 x {dense visits, ready-made policies, child lists of max_children 1 / 64 / 300} x n_rows 1 / 7 / 300 x
  rows_per_game 1 / 3 / n_rows; child counts 0, 1 and max_children (capped at num_actions where max_children is larger: a
  row's children have distinct actions), list entries beyond the count are out-of-range garbage.  Each case fills every
  slot with one pattern, appends another with -1 rows, slot 0 and slot capacity - 1 (the neighbour of the flag word), and
  reads every slot back.
* every gather has 3 spare sentinel rows before and after each output, which must stay untouched.
* the error flags 1, 2, 4, each on a fresh handle: nz_replay_check returns NZ_ERR_OVERFLOW and names the flag, the valid
  rows of the same launch are right, every other slot is unchanged -- and the flag is STICKY: a second nz_replay_check
  reports it again (include/nuzero_amd.h says so; a caller that wants a clean handle makes a new one).
* no test depends on an access outside an allocation: the child-count cases pass views of the middle of larger tensors.
"""
import os
import random
import sys
from ctypes import byref, c_void_p

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import replay_ref  # noqa: E402
from replay_ref import ReplayModel, distinct_floats, same_bits, sparse_lists  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL_F, SENTINEL_I, MARGIN = np.float32(-12345.5), np.int32(-777), 3


def _lib():
    from nuzero_amd import _lib
    return _lib


def _up(x, dtype):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def _ptr(t):
    return None if t is None else c_void_p(t.data_ptr())


def _stream(stream=None):
    return c_void_p((stream or torch.cuda.current_stream()).cuda_stream)


class Dev:
    """A raw nz_replay handle with the model beside it: every append goes to both."""

    def __init__(self, capacity, state_floats, num_actions):
        L = _lib()
        self.h = c_void_p(0)
        assert L.lib.nz_replay_create(byref(self.h), capacity, state_floats, num_actions, 0) == L.NZ_OK
        self.capacity, self.S, self.A = capacity, state_floats, num_actions
        self.model = ReplayModel(capacity, state_floats, num_actions)
        self.keep = []                       # device tensors of launches that may still be in flight

    def close(self):
        _lib().lib.nz_replay_destroy(self.h)          # synchronises the device

    def error(self):
        return (_lib().lib.nz_replay_last_error(self.h) or b"").decode()

    def check(self, stream=None):
        return _lib().lib.nz_replay_check(self.h, _stream(stream))

    def append(self, states, game_value, rows_per_game, dst_slot, game_index, visits=None, policies=None, children=None,
               max_children=0, stream=None, device_children=None):
        """nz_replay_append on uploaded copies of the host arrays (device_children: (actions, visits, counts) device
        tensors to pass in place of uploads of `children`), the model likewise; returns the status."""
        ca, cv, nc = children if children is not None else (None, None, None)
        n_rows = len(dst_slot)
        d = [_up(states, np.float32), _up(visits, np.int32), _up(policies, np.float32), _up(ca, np.int32),
             _up(cv, np.int32), _up(nc, np.int32), _up(game_value, np.int32), _up(dst_slot, np.int64)]
        if device_children is not None:
            d[3:6] = device_children
        self.keep.append(d)
        st = _lib().lib.nz_replay_append(self.h, _ptr(d[0]), _ptr(d[1]), _ptr(d[2]), _ptr(d[3]), _ptr(d[4]), _ptr(d[5]),
                                         max_children, _ptr(d[6]), rows_per_game, _ptr(d[7]), n_rows, game_index,
                                         _stream(stream))
        if st == _lib().NZ_OK:
            self.model.append(states, visits, policies, ca, cv, nc, max_children, game_value, rows_per_game, dst_slot,
                              n_rows, game_index)
        return st

    def fill(self, rs, game_index=7):
        """Pattern A in every slot: distinct states and ready-made policies with the special bit patterns."""
        C = self.capacity
        st = self.append(distinct_floats(rs, (C, self.S), 1.0), rs.permutation(C) - C // 2, 1, rs.permutation(C),
                         game_index, policies=distinct_floats(rs, (C, self.A), 50000.0))
        assert st == _lib().NZ_OK

    def enqueue_gather(self, slots, null=(), stream=None, batch=None):
        """nz_replay_gather into outputs with MARGIN sentinel rows before and after the batch (the batch rows hold the
        sentinel too); `null`: names of the outputs passed as NULL."""
        B = len(slots)
        host = {"states": np.full((B + 2 * MARGIN, self.S), SENTINEL_F), "policies": np.full((B + 2 * MARGIN, self.A), SENTINEL_F),
                "values": np.full(B + 2 * MARGIN, SENTINEL_F), "game_index": np.full(B + 2 * MARGIN, SENTINEL_I)}
        dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
        slots_d = _up(slots, np.int64)
        self.keep.append((dev, slots_d))
        p = {k: None if k in null else _ptr(t[MARGIN:]) for k, t in dev.items()}
        st = _lib().lib.nz_replay_gather(self.h, _ptr(slots_d), B if batch is None else batch, p["states"], p["policies"],
                                         p["values"], p["game_index"], _stream(stream))
        assert st == _lib().NZ_OK, self.error()
        return slots, null, host, dev, batch

    def finish_gather(self, ticket):
        """After a synchronise: every output, margins included, against the model's."""
        slots, null, host, dev, batch = ticket
        B = len(slots)
        if batch is None:
            given = {k: v[MARGIN:MARGIN + B] for k, v in host.items() if k not in null}
            self.model.gather(slots, **{k + "_out": v for k, v in given.items()})
        for k in host:
            assert same_bits(dev[k].cpu().numpy(), host[k]), k

    def gather(self, slots, null=()):
        ticket = self.enqueue_gather(slots, null)
        torch.cuda.synchronize()
        self.finish_gather(ticket)

    def equals_model(self):
        self.gather(np.arange(self.capacity))


@pytest.fixture
def dev_factory():
    made = []

    def make(capacity, state_floats, num_actions):
        made.append(Dev(capacity, state_floats, num_actions))
        return made[-1]

    yield make
    for d in made:
        d.close()


def _slots_for(rs, n_rows, capacity):
    """dst_slot [n_rows]: distinct slots with capacity - 1 and (from two stored rows on) slot 0 among them, -1 rows between
    once there is more than one row."""
    n_store = min(max(1, n_rows - 2), capacity * 3 // 4)
    slots = np.concatenate([[capacity - 1, 0], 1 + rs.permutation(capacity - 2)])[:n_store]
    dst = np.full(n_rows, -1, np.int64)
    dst[np.sort(rs.permutation(n_rows)[:n_store])] = rs.permutation(slots)
    return dst


CASES = replay_ref.pairwise_cases()


@pytest.mark.parametrize("case_no", range(len(CASES)), ids=["-".join(str(x) for x in c) for c in CASES])
def test_append_and_gather_on_the_shape_grid(case_no, dev_factory):
    S, A, form, n_rows, rpg = CASES[case_no]
    rs = np.random.RandomState(100 + case_no)
    capacity = (8, 19, 64)[case_no % 3]
    rpg = n_rows if rpg == "all" else rpg
    dev = dev_factory(capacity, S, A)
    dev.fill(rs)
    dst = _slots_for(rs, n_rows, capacity)
    assert capacity - 1 in dst and (n_rows == 1 or (-1 in dst and 0 in dst))
    states = distinct_floats(rs, (n_rows, S), -100000.0)
    game_value = rs.permutation(2001)[:-(-n_rows // rpg)] - 1000
    kw = {}
    if form == "dense":
        visits = rs.randint(1, 50, (n_rows, A)) * (rs.random_sample((n_rows, A)) < 0.6)
        visits[np.arange(n_rows), rs.randint(0, A, n_rows)] += 1
        kw["visits"] = visits.astype(np.int32)
    elif form == "ready":
        kw["policies"] = distinct_floats(rs, (n_rows, A), -900000.0)
    else:
        mc = int(form[len("sparse"):])
        counts = np.full(n_rows, min(mc, A), np.int32)
        stored = np.nonzero(dst >= 0)[0]
        counts[stored] = np.array([min(mc, A), 0, 1])[np.arange(len(stored)) % 3]
        kw["children"] = sparse_lists(rs, n_rows, A, mc, counts, 1, 50) + (counts,)
        kw["max_children"] = mc
    assert dev.append(states, game_value, rpg, dst, 3, **kw) == _lib().NZ_OK
    dev.equals_model()
    assert dev.check() == _lib().NZ_OK and dev.model.flags == 0
    # the model did store pattern B where it should: the last slot is the row that named it
    r = int(np.nonzero(dst == capacity - 1)[0][0])
    assert same_bits(dev.model.states[capacity - 1], states[r]) and dev.model.values[capacity - 1] == game_value[r // rpg]


@pytest.mark.parametrize("capacity,S,A", [(8, 257, 600), (21, 1, 1)])
def test_gather_with_null_outputs_duplicates_and_batches_beyond_capacity(capacity, S, A, dev_factory):
    rs = np.random.RandomState(5)
    dev = dev_factory(capacity, S, A)
    dev.fill(rs)
    slots = np.concatenate([rs.randint(0, capacity, 3 * capacity - 4), [capacity - 1, capacity - 1, 0, 0]])
    assert len(slots) == 3 * capacity and len(set(slots.tolist())) < len(slots)
    dev.gather(slots)
    for name in ("states", "policies", "values", "game_index"):
        dev.gather(slots, null=(name,))
    dev.gather(slots, null=("states", "policies", "values", "game_index"))
    assert dev.check() == _lib().NZ_OK


def test_empty_calls_do_nothing(dev_factory):
    rs = np.random.RandomState(6)
    dev = dev_factory(16, 20, 9)
    dev.fill(rs)
    L = _lib()
    d = [_up(distinct_floats(rs, (4, 20), -7.0), np.float32), _up(distinct_floats(rs, (4, 9), -9.0), np.float32),
         _up([1, 1, 1, 1], np.int32), _up([0, 1, 15, 3], np.int64)]
    for n_rows in (0, -1, -2 ** 40):
        assert L.lib.nz_replay_append(dev.h, _ptr(d[0]), None, _ptr(d[1]), None, None, None, 0, _ptr(d[2]), 1, _ptr(d[3]),
                                      n_rows, 5, _stream()) == L.NZ_OK
    for batch in (0, -1, -2 ** 40):
        ticket = dev.enqueue_gather(np.array([0, 1, 15, 3]), batch=batch)
        torch.cuda.synchronize()
        dev.finish_gather(ticket)                # outputs: the sentinel everywhere
    dev.equals_model()
    assert dev.check() == L.NZ_OK


def test_calls_on_one_stream_run_in_order(dev_factory):
    """Two appends to overlapping slots and a gather on a side stream, nothing synchronised in between: the later append
    wins, the gather sees both."""
    rs = np.random.RandomState(7)
    dev = dev_factory(32, 513, 257)
    dev.fill(rs)
    first = (distinct_floats(rs, (20, 513), -1000.0), rs.permutation(20), 4, np.arange(0, 20), 1)
    second = (distinct_floats(rs, (20, 513), -90000.0), rs.permutation(20) + 50, 20, np.arange(29, 9, -1), 2)
    pol = [distinct_floats(rs, (20, 257), -5000.0), (rs.randint(0, 9, (20, 257))).astype(np.int32)]
    pol[1][:, 5] = 3
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert dev.append(*first, policies=pol[0], stream=side) == _lib().NZ_OK
    assert dev.append(*second, visits=pol[1], stream=side) == _lib().NZ_OK
    ticket = dev.enqueue_gather(np.arange(32), stream=side)
    side.synchronize()
    dev.finish_gather(ticket)
    assert same_bits(dev.model.states[10:20], second[0][19:9:-1]) and same_bits(dev.model.states[:10], first[0][:10])
    assert dev.check(side) == _lib().NZ_OK


def _large_counts(rs, n_rows, n):
    """Counts near 2**31 - 1: every row's total is above 2**32, no count is exact in float32's 24 bits."""
    v = rs.randint(2 ** 30, 2 ** 31 - 1, (n_rows, n)).astype(np.int64) | 1
    v[0] = 2 ** 31 - 1
    v[0, n // 2] = 1
    v[1:, 1::7] = rs.randint(1, 1000, v[1:, 1::7].shape)
    assert (v.sum(axis=1) > 2 ** 32).all()
    return v.astype(np.int32)


def test_large_counts_dense_and_sparse(dev_factory):
    """Visit sums above 2**32 (a 32-bit accumulator wraps, from 257 actions on within one thread's partial sum) and counts
    above 2**24 (a float32 division is off by an ulp): row 0 is 2**31 - 1 in all entries but one, which is 1."""
    rs = np.random.RandomState(8)
    for A in (257, 600):
        dev = dev_factory(8, 3, A)
        dev.fill(rs)
        visits = _large_counts(rs, 4, A)
        visits[3, ::3] = 0
        assert dev.append(distinct_floats(rs, (4, 3), -10.0), [1, -1], 2, [7, 0, -1, 3], 1, visits=visits) == _lib().NZ_OK
        dev.equals_model()
        want = torch.tensor([int(v) / int(visits[0].astype(np.int64).sum()) for v in visits[0]]).numpy()   # AlphaZero.py:901
        assert same_bits(dev.model.policies[7], want)
    dev = dev_factory(8, 3, 600)
    dev.fill(rs)
    mc = 300
    counts = np.array([300, 257, 300, 2], np.int32)
    ca, cv = sparse_lists(rs, 4, 600, mc, counts)
    big = _large_counts(rs, 4, mc)
    for r in range(4):
        cv[r, :counts[r]] = big[r, :counts[r]]
    cv[3, :2] = 2 ** 31 - 1, 2 ** 31 - 1          # two children make 2**32 - 2: an unsigned 32-bit sum would still do
    cv[1, 0] = 0
    assert dev.append(distinct_floats(rs, (4, 3), -10.0), [1, -1], 2, [0, 7, 2, 5], 1, children=(ca, cv, counts),
                      max_children=mc) == _lib().NZ_OK
    dev.equals_model()
    assert dev.check() == _lib().NZ_OK
    assert dev.model.policies[5, ca[3, 0]] == np.float32(0.5) and np.isfinite(dev.model.policies[[0, 7, 2, 5]]).all()


def test_rows_without_visits_store_zeros_never_nan(dev_factory):
    rs = np.random.RandomState(9)
    A, mc = 257, 64
    dev = dev_factory(8, 2, A)
    dev.fill(rs)                                         # pattern A's policies are not zero: the zeros must be written
    visits = rs.randint(0, 5, (4, A)).astype(np.int32)
    visits[[1, 3]] = 0
    assert dev.append(distinct_floats(rs, (4, 2), -10.0), [1, 0, -1, 1], 1, [7, 6, 0, 1], 1, visits=visits) == _lib().NZ_OK
    dev.equals_model()
    counts = np.array([mc, mc, 1, 5], np.int32)
    ca, cv = sparse_lists(rs, 4, A, mc, counts, 1, 9)
    cv[1, :mc] = 0
    cv[2, 0] = 0
    cv[3, :5] = 0, 4, 0, 0, 4
    assert dev.append(distinct_floats(rs, (4, 2), -20.0), [5, 6], 2, [2, 3, 4, 5], 1, children=(ca, cv, counts),
                      max_children=mc) == _lib().NZ_OK
    dev.equals_model()
    for slot in (6, 1, 3, 4):
        assert same_bits(dev.model.policies[slot], np.zeros(A, np.float32))
    assert np.count_nonzero(dev.model.policies[5]) == 2 and dev.check() == _lib().NZ_OK


FLAG_CASES = {
    "slot_at_capacity": (1, "slot", 0), "slot_2pow40": (1, "slot", 2 ** 40 - 16),
    "action_minus_1": (2, "action", -1), "action_A": (2, "action", None),
    "batch_slot_minus_1": (4, "batch", -1), "batch_slot_at_capacity": (4, "batch", 16),
    "n_children_minus_1": (2, "count", -1), "n_children_above_max": (2, "count", 65),
}


@pytest.mark.parametrize("name", list(FLAG_CASES))
def test_error_flags(name, dev_factory):
    """One bad row (or child, or batch slot) among good ones, on a fresh handle: nz_replay_check names the flag, twice (it
    is sticky); the good rows of the launch are stored / returned, the bad one is skipped as the header says, every other
    slot still holds pattern A."""
    L = _lib()
    flag, kind, bad = FLAG_CASES[name]
    rs = np.random.RandomState(10)
    C, S, A, mc, N = 16, 257, 300, 64, 6
    dev = dev_factory(C, S, A)
    dev.fill(rs)
    assert dev.check() == L.NZ_OK
    dst = np.array([15, 3, -1, 0, 9, 4], np.int64)
    counts = np.array([64, 1, 7, 0, 30, 64], np.int32)
    ca, cv = sparse_lists(rs, N, A, mc, counts, 1, 50)
    states, game_value = distinct_floats(rs, (N, S), -4000.0), [3, -2]
    device_children = None
    if kind == "slot":
        dst[4] = C + bad
    elif kind == "action":
        ca[4, 11] = A if bad is None else bad
    elif kind == "count":
        counts[4] = bad
        # the lists are the middle of larger tensors whose ends hold valid children: wherever a kernel that trusts the
        # count reads, it reads inside an allocation, and what it reads would show in the policy
        pad = np.stack([rs.permutation(A)[:2 * mc], rs.randint(1, 50, 2 * mc)]).astype(np.int32)
        wide = [_up(np.concatenate([pad[i, :mc], x.reshape(-1), pad[i, mc:]]), np.int32) for i, x in enumerate((ca, cv))]
        device_children = [w[mc:mc + N * mc] for w in wide] + [_up(counts, np.int32)]
        dev.keep.append(wide)
    if kind == "batch":
        assert dev.append(states, game_value, 3, dst, 2, children=(ca, cv, counts), max_children=mc) == L.NZ_OK
        assert dev.check() == L.NZ_OK
        dev.gather(np.array([3, 15, bad, 0, 15]))           # the bad row of every output keeps the sentinel
    else:
        assert dev.append(states, game_value, 3, dst, 2, children=(ca, cv, counts), max_children=mc,
                          device_children=device_children) == L.NZ_OK
    assert dev.model.flags == flag
    for _ in range(2):
        assert dev.check() == L.NZ_ERR_OVERFLOW
        assert f"flag {flag}:" in dev.error()
    dev.equals_model()
    assert dev.model.flags == flag
    if kind == "count":                                   # state, value and game index stored, the policy zeros
        assert same_bits(dev.model.states[9], states[4]) and dev.model.values[9] == -2 and dev.model.game_index[9] == 2
        assert same_bits(dev.model.policies[9], np.zeros(A, np.float32))
    if kind == "slot":
        assert dev.model.game_index[9] == 7               # the row went nowhere: pattern A


def test_append_and_gather_refuse_bad_arguments(dev_factory):
    """NZ_ERR_ARG with a message, nothing enqueued (the buffer still equals the model, which saw none of these)."""
    L = _lib()
    rs = np.random.RandomState(11)
    C, S, A, mc, N = 8, 5, 9, 4, 3
    dev = dev_factory(C, S, A)
    dev.fill(rs)
    counts = np.array([4, 1, 2], np.int32)
    ca, cv = sparse_lists(rs, N, A, mc, counts, 1, 9)
    t = {"h": dev.h, "states": _up(distinct_floats(rs, (N, S), -10.0), np.float32), "visits": _up(rs.randint(1, 9, (N, A)), np.int32),
         "policies": _up(distinct_floats(rs, (N, A), -20.0), np.float32), "ca": _up(ca, np.int32), "cv": _up(cv, np.int32),
         "nc": _up(counts, np.int32), "mc": mc, "values": _up([1, -1, 0], np.int32), "rpg": 1, "slots": _up([0, 7, 3], np.int64)}
    forms = {"dense": ("visits",), "ready": ("policies",), "sparse": ("ca", "cv", "nc")}

    def append(given, **change):
        a = dict(t, **change)
        for k in ("visits", "policies", "ca", "cv", "nc"):
            if k not in given:
                a[k] = None
        p = lambda k: a[k] if k == "h" else _ptr(a[k])
        st = L.lib.nz_replay_append(p("h"), p("states"), p("visits"), p("policies"), p("ca"), p("cv"), p("nc"), a["mc"],
                                    p("values"), a["rpg"], p("slots"), N, 4, _stream())
        return st, (L.lib.nz_replay_last_error(a["h"]) or b"").decode()

    # NULL pointers first: the handle's message is still empty, so a message found here was written by the refusal
    assert dev.error() == ""
    for form in forms.values():
        for null in ("states", "values", "slots"):
            st, msg = append(form, **{null: None})
            assert st == L.NZ_ERR_ARG and msg, (form, null)
    st, msg = append(forms["dense"], h=None)
    assert st == L.NZ_ERR_ARG and msg
    assert L.lib.nz_replay_gather(dev.h, None, 3, None, None, None, None, _stream()) == L.NZ_ERR_ARG and dev.error()
    assert L.lib.nz_replay_gather(None, _ptr(t["slots"]), 3, None, None, None, None, _stream()) == L.NZ_ERR_ARG
    assert L.lib.nz_replay_last_error(None)
    assert L.lib.nz_replay_check(None, _stream()) == L.NZ_ERR_ARG
    refused = [((), {}), (("visits", "policies"), {}), (("visits", "ca", "cv", "nc"), {}), (("policies", "ca", "cv", "nc"), {}),
               (("visits", "policies", "ca", "cv", "nc"), {}), (("ca", "nc"), {}), (("ca", "cv"), {}), (("ca",), {}),
               (forms["sparse"], {"mc": 0}), (forms["sparse"], {"mc": -1})]
    refused += [(form, {"rpg": rpg}) for form in forms.values() for rpg in (0, -1)]
    messages = set()
    for given, change in refused:
        st, msg = append(given, **change)
        assert st == L.NZ_ERR_ARG and msg, (given, change)
        messages.add(msg)
    assert len(messages) >= 3                             # forms, child lists, rows_per_game: each says what is wrong
    dev.equals_model()
    assert dev.check() == L.NZ_OK
    # and the same arguments unchanged are accepted
    st, _ = append(forms["sparse"])
    assert st == L.NZ_OK
    dev.model.append(t["states"].cpu().numpy(), None, None, ca, cv, counts, mc, [1, -1, 0], 1, [0, 7, 3], N, 4)
    dev.equals_model()


@pytest.mark.parametrize("sizes,status", [((0, 4, 4, 0), "NZ_ERR_ARG"), ((-1, 4, 4, 0), "NZ_ERR_ARG"), ((8, 0, 4, 0), "NZ_ERR_ARG"),
                                          ((8, -3, 4, 0), "NZ_ERR_ARG"), ((8, 4, 0, 0), "NZ_ERR_ARG"), ((8, 4, -1, 0), "NZ_ERR_ARG"),
                                          ((8, 4, 4, -1), "NZ_ERR_HIP")])
def test_create_refuses_bad_sizes_and_devices(sizes, status):
    L = _lib()
    torch.cuda.init()
    h = c_void_p(0)
    assert L.lib.nz_replay_create(byref(h), *sizes) == getattr(L, status)
    assert not h.value and L.lib.nz_replay_last_error(None)
    assert L.lib.nz_replay_create(None, 8, 4, 4, 0) == L.NZ_ERR_ARG


def test_surface_through_a_batch_that_evicts_its_own_positions():
    """DeviceReplayBuffer without an engine or a network: synthetic export tensors, a window of 3 games, one batch of 40
    games (which evicts its own earlier positions: rows of one launch would name the same slot if ReplayIndex did not
    blank them) and one of 5 -- buffer, shuffles, slices, samples and grouping == the host list fed the same games."""
    from nuzero_amd.gamer import GameRecord
    from nuzero_amd.replay_buffer import ReplayBuffer
    from nuzero_amd.replay_device import DeviceReplayBuffer, late_heavy_probs
    from test_gpu_replay_loss import _same_entries
    W, T, A = replay_ref.SCHEDULE_WINDOW, replay_ref.SCHEDULE_T, replay_ref.SCHEDULE_A
    host, dev = ReplayBuffer(W, 32), DeviceReplayBuffer(W, 32, replay_ref.SCHEDULE_SHAPE, A, max_game_length=T)
    for game_index, lengths, states, visits, outcomes in replay_ref.schedule_batches():
        for g in range(len(lengths)):
            host.save_game(GameRecord(states[g], visits[g], np.zeros(T, np.int32), lengths[g], outcomes[g]), game_index)
        export = {"states": torch.from_numpy(states).cuda(), "visits": torch.from_numpy(visits).cuda(),
                  "outcomes": torch.from_numpy(outcomes).cuda(), "lengths": torch.from_numpy(lengths).cuda()}
        dev.save_games_from_engine(None, game_index, export=export)
    n = host.len()
    assert dev.len() == n == 30 and dev.played_games() == host.played_games() == 3
    _same_entries(dev.get_buffer(), host.get_buffer())
    for seed in (1, 2):
        random.seed(seed); host.shuffle()
        random.seed(seed); dev.shuffle()
        _same_entries(dev.get_slice(3, 35).as_list(), host.get_slice(3, 35))
    for replace, probs in ((True, []), (False, []), (True, late_heavy_probs(n))):
        np.random.seed(5); want = host.get_sample(16, replace, probs)
        np.random.seed(5); got = dev.get_sample(16, replace, probs)
        _same_entries(got.as_list(), want)
        assert got.states.shape == (16,) + replay_ref.SCHEDULE_SHAPE and got.policies.shape == (16, A)
    np.random.seed(9); want = host.get_sample(24, True, [])
    np.random.seed(9); got = dev.get_sample(24, True, [], group_by_game=True)
    keys = sorted(set(e[2] for e in want))
    assert got.keys == keys == [0, 1]
    for (k, states, policies, values), key in zip(got.by_game(), keys):
        group = [e for e in want if e[2] == key]
        assert k == key and torch.equal(states.cpu(), torch.cat([e[0] for e in group], 0))
        assert torch.equal(policies.cpu(), torch.tensor([e[1][1] for e in group]))
        assert values.cpu().tolist() == [float(e[1][0]) for e in group]
    dev.check()
    dev.close()
