"""The Tic-Tac-Toe network's opt-in plain-bf16 mode (nz_engine_precision(e, NZ_PREC_BF16); net_dev.hpp net_tile<..,
PREC_BF16> in net_kernel and selfplay_kernel) on the cases of tests/tttnet_cases.py, at the C ABI.

  1. layer by layer, immune to rounding flips: nz_net_forward_dump hands out what the device held after every stage;
     every conv application is located through nz_net_program + nz_net_program_convs and recomputed in float64 from the
     device's OWN dumped sources, residual and planes (exact bf16 values) and the host-rounded weights; a stored value
     must be the bf16 (round to nearest even) of some y within delta of that result, delta = (products + 2) 2^-24
     sum |a| |w| (the float32 accumulation) + 3e-7 absolute for tanh_fast or 2^-22 relative for expm1f; at most 1 % of a
     layer's values may need the delta at all (tests/test_ttt_bf16_ref_host.py: the kernel's summation order flips
     under half of that); padded channels, rows past the batch and everything a stage does not write hold what the
     layout says;
  2. the whole network on all 22 cases at n = 1, 15, 16, 17, 37: within E_case (computed on the CPU from the reference
     side, ttt_bf16_ref.e_case) of the float64 emulation, finite, sums of 1, the all-zero position exactly 0, bit-exact
     across batch slots and batches, probs_dev NULL, guards;
  3. the default is untouched: bf16 -> float32 -> set_weights gives a fresh float32 engine's bytes, forward and round;
  4. rounds: the persistent kernel in bf16 mode under three environments plays the same bytes, those of the lock-step
     route and of the C oracle on the table nz_net_forward gives in bf16 mode; a ragged tile of 5 slots;
  5. what the mode refuses, and Gamer(net_precision="bf16") on Tic-Tac-Toe.
Needs a GPU."""
import os

import numpy as np
import pytest

import ttt_bf16_ref as tr
import tttnet_cases as tc
from test_gpu_tttnet_edges import ENV, N_GAMES, N_SLOTS, SEED, _Images, _config, _forward, _same_bytes, _set
from test_ttt_bf16_ref_host import program

pytestmark = pytest.mark.gpu
CASE_NAMES = [c.name for c in tc.CASES]
U32 = 2.0 ** -24
FLIP_CAP = 0.01
ROW = 2 * 9 * 64 + 9 * 16


def _engine(case=None, precision="bf16", n=16, sims=10, **kw):
    from nuzero_amd.engine import SelfPlayEngine
    from nuzero_amd.search_config import legacy_ttt_search_config
    eng = SelfPlayEngine(legacy_ttt_search_config(sims), n, precision=precision, **kw)
    if case is not None:
        _set(eng, case)
    return eng


# ---- 1. layer by layer ---------------------------------------------------------------------------------------------------
def _areas(flat):
    """One stage's dump [R, 1296] -> (buffers [2][R, 9, 64], strip [R, 9, 16]), float64."""
    R = flat.shape[0]
    f = flat.astype(np.float64)
    return [f[:, b * 576:(b + 1) * 576].reshape(R, 9, 64) for b in range(2)], f[:, 1152:].reshape(R, 9, 16)


def _nchw(a):
    """[R, 9 cells, C] -> [R, C, 3, 3]"""
    return np.ascontiguousarray(a.transpose(0, 2, 1)).reshape(a.shape[0], a.shape[2], 3, 3)


@pytest.mark.parametrize("name", tr.LAYER_CASES)
def test_every_layer_from_the_device_s_own_inputs(name):
    case = tc.BY_NAME[name]
    n = tc.MAX_BATCH
    x = tr.e_case(name)["x"]
    eng = _engine(case)
    d = {k: v.cpu().numpy() for k, v in eng.net_forward_dump(x).items()}
    eng.close()
    R = 16 * ((n + 15) // 16)
    acts, planes, vcells = d["acts"], d["planes"].astype(np.float64), d["vcells"].astype(np.float64)
    jobs, convs = program(case)
    n_stages = int(jobs[:, 1].max()) + 1
    assert acts.shape == (n_stages, R, ROW) and planes.shape == (R, 9, 4) and vcells.shape == (R, 9)
    # the rounded input planes; rows past the batch and planes 2, 3 are zero, and with them everything those rows hold
    assert np.array_equal(_nchw(planes[:n, :, :2]), tr.rne_bf16(x)), name
    assert not planes[n:].any() and not planes[:, :, 2:].any() and not acts[:, n:].any() and not vcells[n:].any(), name
    wts = [np.asarray(t, np.float64) for t in tc.weights(case).values()]
    wr = [tr.rne_bf16(t) for t in wts]
    prev_b, prev_s = [np.zeros((R, 9, 64)), np.zeros((R, 9, 64))], np.zeros((R, 9, 16))
    seen_logits = seen_value = False
    for s in range(n_stages):
        now_b, now_s = _areas(acts[s])
        written_b, written_s = [np.zeros((9, 64), bool), np.zeros((9, 64), bool)], np.zeros((9, 16), bool)
        rows = np.flatnonzero(jobs[:, 1] == s)
        for conv in sorted(set(convs[rows].tolist())):
            J = jobs[rows[convs[rows] == conv]]
            kgroups, sslot, src, res, act, extra = (int(J[0, i]) for i in (4, 5, 6, 8, 9, 11))
            assert all((J[:, i] == J[0, i]).all() for i in (4, 5, 6, 8, 9, 11)), (name, s, conv)
            cout, cin = wts[conv].shape[:2]
            cin_main = cin - (2 if extra else 0)
            assert (kgroups == (cin_main + 31) // 32) and (cin_main > 0 or extra), (name, s, conv)
            parts = []
            if cin_main:
                if sslot == -1:              # the split source slot: slots 6-7 of the buffer, then the strip
                    main = np.concatenate([prev_b[src][:, :, 48:64], prev_s], axis=2)
                else:
                    assert 8 * sslot + cin_main <= 64
                    main = prev_b[src][:, :, 8 * sslot:8 * sslot + 32 * kgroups] if 8 * sslot + 32 * kgroups <= 64 else \
                        np.concatenate([prev_b[src][:, :, 8 * sslot:], prev_b[src][:, :, :8 * sslot + 32 * kgroups - 64]], axis=2)
                assert np.isfinite(main).all(), (name, s, conv, "a K group's padding must read numbers")
                parts.append(main[:, :, :cin_main])
            if extra:
                parts.append(planes[:, :, :2])
            a = _nchw(np.concatenate(parts, axis=2))
            y = tr.conv64(a, wr[conv])
            s_abs = tr.conv64(np.abs(a), np.abs(wr[conv]))
            buffer_tiles = [int(j[10]) for j in J if j[7] < 2]
            base = min(buffer_tiles) if buffer_tiles else 0          # destination tile of output tile 0
            if res >= 0:
                assert base == 0 and (J[:, 7] < 2).all()
                r = _nchw(prev_b[res][:, :, :((cout + 15) // 16) * 16])[:, :cout]
                y, s_abs = y + r, s_abs + np.abs(r)
            delta = (9 * (32 * kgroups + 4 * extra) + 2) * U32 * s_abs
            want = tr.activate(y, act)
            if act == 2:
                delta = delta + 3e-7                                  # tanh_fast; its slope is at most 1
            elif act == 3:
                delta = delta + 2.0 ** -22 * np.abs(want)             # expm1f; slope at most 1
            checked = flipped = 0
            for j in J:
                mask, dst, dtile = int(j[3]), int(j[7]), int(j[10])
                cells = [o for o in range(9) if (mask >> o) & 1]
                nt = dtile - base if dst < 2 else (4 - base if dst == 4 else 0)
                live = min(16, cout - 16 * nt)
                assert live > 0, (name, s, conv, "a job past the conv's tiles")
                w_ = want[:, 16 * nt:16 * nt + live].reshape(R, live, 9)[:, :, cells]          # [R, ch, cell]
                dl = delta[:, 16 * nt:16 * nt + live].reshape(R, live, 9)[:, :, cells]
                if dst == 2:                  # logits, float32: [pos][9]
                    assert nt == 0 and live == 1
                    got = d["logits"].astype(np.float64)[:, cells]
                    assert (np.abs(got - w_[:n, 0]) <= dl[:n, 0] + U32 * np.abs(w_[:n, 0])).all(), (name, s, "logits")
                    seen_logits = True
                    continue
                if dst == 3:                  # the value head's per-cell staging, float32
                    assert nt == 0 and live == 1
                    assert (np.abs(vcells[:, cells] - w_[:, 0]) <= dl[:, 0] + U32 * np.abs(w_[:, 0])).all(), (name, s, "vcells")
                    seen_value = True
                    continue
                area, wr_mask = (now_s, written_s) if dst == 4 else (now_b[dst], written_b[dst])
                c0 = 0 if dst == 4 else 16 * dtile
                stored = area[:, cells, c0:c0 + 16].transpose(0, 2, 1)                            # [R, 16, cell]
                assert not wr_mask[cells, c0:c0 + 16].any(), (name, s, "two jobs write one place")
                wr_mask[np.ix_(cells, range(c0, c0 + 16))] = True
                assert not stored[:, live:].any(), (name, s, conv, "padded output channels hold 0")
                lo, hi = tr.rne_bf16(w_ - dl), tr.rne_bf16(w_ + dl)
                bad = (stored[:, :live] < lo) | (stored[:, :live] > hi)
                assert not bad.any(), (name, s, conv, int(bad.sum()), float(np.abs(stored[:, :live] - w_)[bad].max()))
                flipped += int((stored[:n, :live] != tr.rne_bf16(w_[:n])).sum())
                checked += stored[:n, :live].size
            if checked:
                assert flipped <= FLIP_CAP * checked, (name, s, conv, flipped, checked)
        # what no job of the stage writes keeps its bytes
        for b in range(2):
            assert np.array_equal(now_b[b][:, ~written_b[b]], prev_b[b][:, ~written_b[b]]), (name, s, b)
        assert np.array_equal(now_s[:, ~written_s], prev_s[:, ~written_s]), (name, s, "strip")
        prev_b, prev_s = now_b, now_s
    assert seen_logits and seen_value
    # the float32 tail: value = tanh_fast(mean of the staging), probs = softmax of the logits
    v_want = np.tanh(vcells[:n].mean(axis=1))
    v_tol = 3e-7 + 10 * U32 * np.abs(vcells[:n]).mean(axis=1) + U32
    assert (np.abs(d["value"].astype(np.float64) - v_want) <= v_tol).all(), name
    assert np.abs(d["probs"].astype(np.float64) - tc.softmax64(d["logits"].astype(np.float64))).max() < 1e-6, name


# ---- 2. the whole network ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_whole_network(name):
    case = tc.BY_NAME[name]
    e = tr.e_case(name)
    eng = _engine(case)
    assert eng.precision == "bf16" and eng.positions_per_pass == 16
    full = None
    for n in tc.BATCHES:
        images = _Images(e["x"][:n])
        got = _forward(eng, images)                       # (guards and the input are checked in there)
        l, p, v = got
        assert all(np.isfinite(a).all() for a in got), (name, n)
        assert np.max(np.abs(p.astype(np.float64).sum(axis=1) - 1.0)) < 1e-5, (name, n)
        dist = tr.distance(got, tuple(a[:n] for a in e["emu"]))
        print(f"{name} n={n}: to the float64 emulation {dist:.3e} (E_case {e['E']:.3e})")
        assert dist <= e["E"], (name, n, dist, e["E"])
        assert (l[0] == 0).all() and v[0] == 0 and (p[0] == p[0, 0]).all(), (name, n)
        if n == 17:
            _same_bytes(f"{name} probs_dev NULL", _forward(eng, images, probs=False), got)
        if n == tc.MAX_BATCH:
            full = got
    # the mode is on: the float32 mode is 1e-5 from the reference, this one is not
    assert tr.distance(full, e["ref64"]) > 10 * tc.TOL, name
    # the same position in other slots and batches: bit for bit
    order = np.array([5, 0, 16, 3, 3, 11, 36, 1, 20, 7, 9, 30, 2, 2, 8, 4, 35])
    _same_bytes(f"{name} slots", _forward(eng, _Images(e["x"][order])), [a[order] for a in full])
    for n in (1, 15, 16, 17):
        _same_bytes(f"{name} prefix {n}", _forward(eng, _Images(e["x"][:n])), [a[:n] for a in full])
    # the dump kernel computes the same outputs
    d = eng.net_forward_dump(e["x"])
    _same_bytes(f"{name} dump", [d[k].cpu().numpy() for k in ("logits", "probs", "value")], full)
    bf16_flops, _ = eng.net_matrix_flops_per_position()
    eng.close()
    f32 = _engine(case, precision="float32")
    assert f32.net_matrix_flops_per_position()[0] == 6 * bf16_flops
    f32.close()


# ---- 3. the default is untouched -------------------------------------------------------------------------------------------
def _round_of(eng):
    eng.play(base_seed=SEED)
    out = {k: np.asarray(v) for k, v in eng.export(trace=True).items()}
    out["counters"], out["desync"], out["live"] = eng.counters(), eng.desync_count(), eng.live_games()
    return out


def _same_round(tag, a, b):
    from test_gpu_net_packed import ARRAYS
    for k in ARRAYS:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (tag, k)
    assert a["counters"] == b["counters"] and a["desync"] == b["desync"] == 0 and a["live"] == b["live"] == 0, tag


@pytest.mark.parametrize("name", ["large_logits", "conv_56"])
def test_the_default_is_untouched(name):
    from nuzero_amd.engine import SelfPlayEngine
    case = tc.BY_NAME[name]
    x = tr.e_case(name)["x"]
    fresh = SelfPlayEngine(_config(), N_GAMES, n_slots=N_SLOTS)
    _set(fresh, case)
    back = SelfPlayEngine(_config(), N_GAMES, n_slots=N_SLOTS, precision="bf16")
    _set(back, case)
    bf = _forward(back, _Images(x))
    back.precision = "float32"
    assert back.precision == "float32" and back.positions_per_pass == fresh.positions_per_pass
    _set(back, case)
    base = _forward(fresh, _Images(x))
    _same_bytes(f"{name} forward", _forward(back, _Images(x)), base)
    assert tr.distance(bf, base) > 10 * tc.TOL, "the bf16 engine was in bf16 mode"
    for P in (3, 8):
        _same_bytes(f"{name} packed {P}", _forward(back, _Images(x), packed=P), base)
    _same_round(name, _round_of(back), _round_of(fresh))
    fresh.close(); back.close()


# ---- 4. rounds -------------------------------------------------------------------------------------------------------------
ROUTES = {"default": {}, "three slots a workgroup": {"NZ_SLOTS_PER_WG": "3"}, "burst switch 2": {"NZ_BURST_UNDER_NET": "2"}}


def _bf16_engine(case, env, n_slots=N_SLOTS):
    from nuzero_amd.engine import SelfPlayEngine
    saved = {k: os.environ.get(k) for k in ENV}
    try:
        for k in ENV:
            os.environ.pop(k, None)
        os.environ.update(env)
        eng = SelfPlayEngine(_config(), N_GAMES, n_slots=n_slots, precision="bf16")
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    _set(eng, case)
    return eng


def _oracle_round(eng):
    """The round by the C oracle on the table `eng`'s nz_net_forward gives for all 4,520 non-terminal positions."""
    from oracle import cref
    from test_gpu_net_packed import _codes, _positions
    codes = _codes()
    _, value, probs = eng.net_forward(_positions())
    table = np.zeros((3 ** 9, 10), np.float32)
    table[codes, :9] = probs.cpu().numpy()
    table[codes, 9] = value.cpu().numpy()
    assert np.isfinite(table).all()
    return cref.play_games(table, _config(), [SEED + g for g in range(N_GAMES)])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_rounds_equal_each_other_the_lock_step_route_and_the_oracle(name):
    case = tc.BY_NAME[name]
    rounds = {}
    for route, env in ROUTES.items():
        eng = _bf16_engine(case, env)
        assert eng.precision == "bf16" and eng.positions_per_pass == 16, (name, route)
        rounds[route] = _round_of(eng)
        if route == "default":
            o = _oracle_round(eng)
        eng.close()
    base = rounds["default"]
    assert base["desync"] == 0 and base["live"] == 0 and base["counters"]["simulations"] > 0
    for route in ROUTES:
        _same_round(f"{name} {route}", rounds[route], base)
    for k in ("lengths", "outcomes", "actions", "visits", "tree_size", "n_children", "bias", "child_prior",
              "child_value_sum", "root_value_sum"):
        assert np.array_equal(base[k], o[k]), (name, k)
    assert base["counters"]["simulations"] == o["simulations"] and base["counters"]["expansions"] == o["expansions"]
    # the lock-step route (as many slots as games) follows the mode
    lock = _bf16_engine(case, {}, n_slots=N_GAMES)
    lock.play_lockstep(base_seed=SEED)
    got = {k: np.asarray(v) for k, v in lock.export(trace=True).items()}
    from test_gpu_net_packed import ARRAYS
    for k in ARRAYS:
        assert got[k].tobytes() == base[k].tobytes(), (name, "lock-step", k)
    assert lock.counters() == base["counters"] and lock.live_games() == 0
    lock.close()


def test_a_ragged_tile_of_five_slots():
    case = tc.BY_NAME["large_logits"]
    base = _bf16_engine(case, {})
    ragged = _bf16_engine(case, {"NZ_SLOTS_PER_WG": "16"}, n_slots=5)
    assert ragged.positions_per_pass == 16
    _same_round("5 slots", _round_of(ragged), _round_of(base))
    base.close(); ragged.close()


# ---- 5. refusals and surface -------------------------------------------------------------------------------------------------
def _error_of(fn):
    from nuzero_amd._lib import NzError
    with pytest.raises(NzError) as ei:
        fn()
    return ei.value


def test_what_the_mode_refuses():
    from ctypes import byref, c_int32
    from nuzero_amd import _lib
    case = tc.BY_NAME["rec_44"]
    x = tr.e_case(case.name)["x"]
    eng = _engine(case, precision=None)
    assert eng.precision == "float32"
    err = _error_of(lambda: eng.net_forward_dump(x))
    assert err.code == _lib.NZ_ERR_STATE and "bf16" in str(err)
    assert _lib.lib.nz_engine_precision(eng._h, 7, None) == _lib.NZ_ERR_ARG
    cur = c_int32(-5)
    assert _lib.lib.nz_engine_precision(eng._h, -1, byref(cur)) == _lib.NZ_OK and cur.value == _lib.NZ_PREC_FLOAT32
    eng.precision = "float32"                      # the same mode: the weights stay
    eng.net_forward(x)
    eng.precision = "bf16"                         # a change of mode drops them
    for call in (lambda: eng.net_forward(x), lambda: eng.play(base_seed=1), lambda: eng.play_lockstep(base_seed=1),
                 lambda: eng.net_forward_dump(x)):
        err = _error_of(call)
        assert err.code == _lib.NZ_ERR_STATE and "nz_engine_set_weights" in str(err), str(err)
    _set(eng, case)
    eng.net_forward(x)
    err = _error_of(lambda: eng.net_forward(x, positions_per_pass=3))
    assert err.code == _lib.NZ_ERR_STATE and "float32 only" in str(err)
    err = _error_of(lambda: eng.net_forward_stamps(x))
    assert err.code == _lib.NZ_ERR_STATE and "float32 only" in str(err)
    with pytest.raises(ValueError):
        eng.precision = "fp8"
    assert eng.precision == "bf16"
    # a table evaluator is not the network's: it stays through a change of mode
    table = np.zeros((3 ** 9, 10), np.float32)
    table[:, :9] = 1.0 / 9
    eng.set_table(table)
    eng.precision = "float32"
    eng.play(base_seed=3)
    assert eng.live_games() == 0
    eng.close()


def test_gamer_plays_tic_tac_toe_in_bf16():
    from nuzero_amd.gamer import Gamer
    from nuzero_amd.network import Network_Manager
    from nuzero_amd.replay_buffer import ReplayBuffer
    from nuzero_amd.engine import SelfPlayEngine
    from nuzero_amd.weights import synthetic_recurrent_net_weights

    class tic_tac_toe:
        pass

    w = synthetic_recurrent_net_weights(5, 2, 1, 64, 2, True)
    cfg = _config()
    N, SLOTS = 48, 16
    g = Gamer(ReplayBuffer(10 ** 6, 64), Network_Manager(w), tic_tac_toe, [], 0, cfg, 2, "disabled", num_games=N,
              concurrent_games=SLOTS, base_seed=300, net_precision="bf16")
    assert g.engine.precision == "bf16"
    records, stats = g.play_games()
    eng = SelfPlayEngine(cfg, N, n_slots=SLOTS, precision="bf16")
    eng.set_weights(w, recurrent_iterations=2)
    eng.play(base_seed=300)
    r = eng.export()
    assert len(records) == N == len(stats)
    for i, rec in enumerate(records):
        assert rec.length == r["lengths"][i] and rec.terminal_value == r["outcomes"][i]
        assert rec.action_history == [int(t) for t in r["actions"][i][:rec.length]]
        for m in range(rec.length):
            v = r["visits"][i][m]
            assert rec.child_policy[m] == [int(c) / int(v.sum()) if c else 0 for c in v]
    assert g.buffer.len() == int(r["lengths"].sum())
    # and it is not the float32 round's network
    f32 = SelfPlayEngine(cfg, N, n_slots=SLOTS)
    f32.set_weights(w, recurrent_iterations=2)
    x = tr.e_case("large_logits")["x"]
    assert not np.array_equal(f32.net_forward(x)[0].cpu().numpy(), eng.net_forward(x)[0].cpu().numpy())
    eng.close(); f32.close()
    with pytest.raises(ValueError):
        Gamer(None, Network_Manager(w), tic_tac_toe, [], 0, cfg, 2, "disabled", num_games=N, net_precision="fp8")
