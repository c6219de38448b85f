"""What the float64 emulation of the board nets' plain-bf16 mode (tests/bf16_net_ref.py) can carry, and the packing of
the mode's weight stream -- on the host, no GPU.

The GPU tests (tests/test_gpu_boardnet_bf16.py) lean on two conditions that are shown here for every fused16 case of
tests/boardnet_cases.py, at 300 positions:
  * E_case, the emulation's worst distance from the float64 oracle, is far above 1e-4: the mode cannot be mistaken for
    the float32 mode (whose distance is below 1e-5);
  * an emulation whose every value is perturbed by 1e-6 (relative) before it is rounded -- a stand-in for the device's
    float32 accumulation -- stays within E_case of the unperturbed one, although most positions move by more than 1e-5:
    a flipped rounding is a 2^-8 step of one activation.  So E_case bounds the device's distance from the emulation,
    and nothing finer than a layer-by-layer check (which sees the device's own rounded inputs) can.
The figures are printed (pytest -s) and kept in DESIGN.md section 5b."""
import ctypes

import numpy as np
import pytest

import bf16_net_ref as br
import boardnet_cases as bc

PERTURB = 1e-6


def test_rne_bf16_is_round_to_nearest_even():
    # bf16 numbers of [1, 2) are 2^-7 apart; 1 + k 2^-8 is halfway between two of them for odd k: to the even significand
    x = 1.0 + np.arange(0, 16) * 2.0 ** -8
    want = 1.0 + np.array([0, 0, 2, 4, 4, 4, 6, 8, 8, 8, 10, 12, 12, 12, 14, 16]) * 2.0 ** -8
    assert np.array_equal(br.rne_bf16(x), want)
    assert np.array_equal(br.rne_bf16(-x), -want)
    r = np.random.RandomState(1).standard_normal(10000).astype(np.float32) * 3
    bits = br.bf16_bits(r)
    assert np.array_equal((bits << 16).astype(np.uint32).view(np.float32).astype(np.float64), br.rne_bf16(r))
    assert np.all(np.abs(br.rne_bf16(r) - r) <= np.abs(r) * 2.0 ** -8)          # half an ulp of 8 bits, at most


@pytest.mark.parametrize("name", br.FUSED16_CASES)
def test_the_emulation_carries_the_bounds_the_gpu_tests_use(name):
    case = bc.BY_NAME[name]
    e = br.e_case(name)
    E, ref64, emu, x = e["E"], e["ref64"], e["emu"], e["x"]
    med = float(np.median(br.per_position(emu, ref64)))
    pert = br.emulate(case, x, perturb=PERTURB, seed=5)
    moved = br.per_position(pert, emu)
    unrounded_res = br.distance(br.emulate(case, x, residual_rounded=False), emu)
    print(f"\n{name}: E_case {E:.3e} (median {med:.3e}); 1e-6 perturbation: {100 * np.mean(moved <= bc.TOL):.0f} % of positions "
          f"within 1e-5, worst {moved.max():.3e} = {moved.max() / E:.2f} E_case; residual unrounded instead: {unrounded_res:.3e}")
    assert E > 1e-3, "the mode must be unmistakable: ten times the 1e-4 the device test asks of it against float32 mode"
    assert moved.max() <= E, "a perturbed emulation leaves E_case: the coarse bound of the device test does not hold"


@pytest.mark.parametrize("name", br.FUSED16_CASES)
def test_the_weight_stream_is_the_restated_packing(name):
    from nuzero_amd import _lib
    case = bc.BY_NAME[name]
    w = bc.weights(case)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
    for L, wt in zip(br.layers(case), br.layer_weights(case, w)):
        cin = case.in_channels if L.src == 0 else br.layers(case)[L.src - 1].cout
        t0 = np.ascontiguousarray(wt[0], np.float32)
        t1 = np.ascontiguousarray(wt[1], np.float32) if case.hex else None
        assert t0.shape[0] == L.cout and t0.shape[1] == cin
        n = ctypes.c_int64(0)
        k = 1 if case.hex else t0.shape[-1]
        assert _lib.lib.nz_boardnet_bf16_stream(vp(t0), vp(t1), L.cout, cin, k, int(case.hex), None, 0, ctypes.byref(n)) == _lib.NZ_OK
        want = br.weight_stream(case, wt, L.cout, cin)
        assert n.value == want.size
        got = np.full(n.value, 0xDEADBEEF, np.uint32)
        assert _lib.lib.nz_boardnet_bf16_stream(vp(t0), vp(t1), L.cout, cin, k, int(case.hex), vp(got), n.value, ctypes.byref(n)) == _lib.NZ_OK
        assert np.array_equal(got, want.reshape(-1)), (name, L.index)
        assert np.count_nonzero(got) > 0


def test_the_stream_call_refuses_what_has_no_stream():
    from nuzero_amd import _lib
    n = ctypes.c_int64(0)
    w = np.zeros((96, 8, 3, 3), np.float32)
    st = _lib.lib.nz_boardnet_bf16_stream(w.ctypes.data_as(ctypes.c_void_p), None, 96, 8, 3, 0, None, 0, ctypes.byref(n))
    assert st == _lib.NZ_ERR_ARG and b"64" in _lib.lib.nz_boardnet_last_error(None)
