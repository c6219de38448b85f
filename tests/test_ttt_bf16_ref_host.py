"""What the float64 emulation of the Tic-Tac-Toe network's plain-bf16 mode (tests/ttt_bf16_ref.py) can carry, the
mode's weight stream, and the host-only surface of the mode -- no GPU.

tests/test_gpu_ttt_bf16.py leans on what is shown here for the cases of tests/tttnet_cases.py on their 37 positions:
  * E_case, the emulation's worst distance from the float64 oracle in tttnet_cases.errors' three measures, computed
    from the reference side alone: the bound the device's whole-network outputs are held to against the emulation, and
    far above the float32 mode's 1e-5, so the mode cannot be mistaken for it;
  * the share of a layer's stored values whose rounding a float32 accumulation in the kernel's summation order flips
    (a numpy restatement: ttt_bf16_ref.conv32_kernel_order) stays under HALF of the 1 % the layer test allows, for every
    case the layer test uses.  (A case that missed would get another seed in the case table below; none does.)
The figures are printed (pytest -s) and kept in DESIGN.md section 5 ("The plain-bf16 mode of the Tic-Tac-Toe network")."""
import ctypes

import numpy as np
import pytest

import ttt_bf16_ref as tr
import tttnet_cases as tc

FLIP_CAP = 0.01                 # tests/test_gpu_ttt_bf16.py: share of a layer's values that may need the margin
CASE_NAMES = [c.name for c in tc.CASES]


def _desc(case):
    from nuzero_amd import _lib
    return _lib.NetDesc(in_channels=2, policy_channels=1, width=case.width, num_blocks=case.num_blocks, recall=int(case.recall),
                        value_activation=_lib.NZ_ACT_RELU if case.value_activation == "relu" else _lib.NZ_ACT_TANH,
                        arch={"recurrent": _lib.NZ_ARCH_RECURRENT, "resnet": _lib.NZ_ARCH_RESNET,
                              "convnet": _lib.NZ_ARCH_CONVNET}[case.arch], kernel_size=case.kernel_size)


def program(case):
    """(rows of nz_net_program [n, 13], conv tensor of each row [n])."""
    from nuzero_amd import _lib
    nd, n = _desc(case), ctypes.c_int32(0)
    assert _lib.lib.nz_net_program(ctypes.byref(nd), case.iters, None, 0, ctypes.byref(n)) == _lib.NZ_OK
    jobs = np.zeros((n.value, _lib.NZ_NET_JOB_FIELDS), np.int32)
    convs = np.full(n.value, -9, np.int32)
    m = ctypes.c_int32(0)
    assert _lib.lib.nz_net_program(ctypes.byref(nd), case.iters, jobs.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(m)) == _lib.NZ_OK
    assert _lib.lib.nz_net_program_convs(ctypes.byref(nd), case.iters, convs.ctypes.data_as(ctypes.c_void_p), n.value,
                                         ctypes.byref(m)) == _lib.NZ_OK
    assert m.value == n.value
    return jobs, convs


@pytest.mark.parametrize("name", CASE_NAMES)
def test_e_case_is_far_from_the_float32_mode(name):
    e = tr.e_case(name)
    err = tc.errors(e["emu"][0], e["emu"][1], e["emu"][2], e["ref64"])
    print(f"\n{name}: E_case {e['E']:.3e}  (" + " ".join(f"{k} {err[k]:.2e}" for k in sorted(err)) + ")")
    assert all(np.isfinite(a).all() for a in e["emu"])
    assert e["E"] > 10 * tc.TOL, "the mode must be unmistakable beside the float32 mode's 1e-5"
    # the all-zero position: nothing to round
    assert not e["emu"][0][0].any() and e["emu"][2][0] == 0


@pytest.mark.parametrize("name", tr.LAYER_CASES)
def test_float32_accumulation_flips_few_roundings(name):
    case = tc.BY_NAME[name]
    shares = tr.flipped_share(case, tr.e_case(name)["x"])
    worst = max(s for _, s in shares)
    print(f"\n{name}: {len(shares)} stored layers, flipped roundings worst {100 * worst:.3f} % "
          f"(mean {100 * np.mean([s for _, s in shares]):.3f} %)")
    assert worst < FLIP_CAP / 2, (name, shares)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_applications_are_the_program_s_convs(name):
    """ttt_bf16_ref.applications lists the conv applications in the order the compiled program's stages run them:
    stage by stage the set of conv tensors (nz_net_program_convs) is the emulation's, the two heads side by side."""
    case = tc.BY_NAME[name]
    jobs, convs = program(case)
    assert (convs >= 0).all()
    by_stage = [sorted(set(convs[jobs[:, 1] == s].tolist())) for s in range(jobs[:, 1].max() + 1)]
    apps = [a[0] for a in tr.applications(case)]
    trunk, (p0, p1, v0, v1, v2, v3) = apps[:-6], apps[-6:]
    assert by_stage == [[t] for t in trunk] + [sorted([p0, v0]), sorted([p1, v1]), [v2], [v3]], name


@pytest.mark.parametrize("name", tr.LAYER_CASES)
def test_the_weight_stream_is_the_restated_packing(name):
    from nuzero_amd import _lib
    case = tc.BY_NAME[name]
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    seen_extra = False
    for i, t in enumerate(tc.weights(case).values()):
        t = np.ascontiguousarray(t, np.float32)
        cout, cin, k = t.shape[0], t.shape[1], t.shape[-1]
        cin_main = 0 if i == 0 else (cin - 2 if (case.arch == "recurrent" and case.recall and i == 1) else cin)
        n_main, n_extra = ctypes.c_int64(0), ctypes.c_int64(0)
        assert _lib.lib.nz_net_bf16_stream(vp(t), cout, cin, cin_main, k, None, 0, ctypes.byref(n_main), ctypes.byref(n_extra)) == _lib.NZ_OK
        want = tr.weight_stream(t, cin_main)
        assert n_main.value == want.size and n_extra.value == (9 * 64 * want.shape[0] if cin > cin_main else 0), (name, i)
        got = np.full(n_main.value + n_extra.value, 0xDEADBEEF, np.uint32)
        assert _lib.lib.nz_net_bf16_stream(vp(t), cout, cin, cin_main, k, vp(got), len(got), ctypes.byref(n_main),
                                           ctypes.byref(n_extra)) == _lib.NZ_OK
        assert np.array_equal(got[:n_main.value], want.reshape(-1)), (name, i)
        if n_extra.value:                                   # [tile][tap][lane]: plane lane >> 4 of output channel 16 tile + (lane & 15)
            seen_extra = True
            full = np.zeros((want.shape[0] * 16, 4, 9), np.float32)
            w9 = t.reshape(cout, cin, 9) if k == 3 else np.pad(t.reshape(cout, cin, 1), ((0, 0), (0, 0), (4, 4)))
            full[:cout, :cin - cin_main] = w9[:, cin_main:]
            lane = np.arange(64)
            ext = np.stack([full[nt * 16 + (lane & 15), lane >> 4, :].T for nt in range(want.shape[0])])   # [tile][tap][lane]
            assert np.array_equal(got[n_main.value:], (tr.bf16_bits(ext) << 16).astype(np.uint32).reshape(-1)), (name, i)
    assert seen_extra


def test_the_stream_is_a_third_of_the_float32_stream_and_refuses_what_it_cannot_pack():
    from nuzero_amd import _lib
    n_main, n_extra = ctypes.c_int64(0), ctypes.c_int64(0)
    w = np.zeros((64, 66, 3, 3), np.float32)
    p = w.ctypes.data_as(ctypes.c_void_p)
    assert _lib.lib.nz_net_bf16_stream(p, 64, 66, 64, 3, None, 0, ctypes.byref(n_main), ctypes.byref(n_extra)) == _lib.NZ_OK
    assert n_main.value == 4 * 2 * 9 * 64 * 4 and n_extra.value == 4 * 9 * 64        # (float32: 4 * 2 * 9 * 3 * 64 * 4)
    assert _lib.lib.nz_net_bf16_stream(p, 65, 66, 64, 3, None, 0, ctypes.byref(n_main), ctypes.byref(n_extra)) == _lib.NZ_ERR_ARG
    assert _lib.lib.nz_net_bf16_stream(p, 64, 66, 64, 2, None, 0, ctypes.byref(n_main), ctypes.byref(n_extra)) == _lib.NZ_ERR_ARG
