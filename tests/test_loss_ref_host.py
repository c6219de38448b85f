"""tests/loss_ref.py, the float64 reference of tests/test_gpu_loss_edges.py, against what it restates -- no GPU.

1. Against tests/golden/loss_kat.npz, the vectors of the genuine loss functions and the calculate_loss loop
   (tests/golden/make_golden_replay.py): every key -- losses, dlogits, dvalues -- of the three batches, the four
   policy forms and the two value forms.  The vectors were computed in float32 and the restatement in float64, so they
   differ by float32 rounding: 2.7e-7 at worst (losses relative, gradients over the largest entry); 1e-6 is asserted.
2. The hard inputs of the GPU test: on every case the float32 restatement's losses stay within 2e-6 relative of the
   float64 ones (1.6e-6 at worst, on the batch of 2048; 8e-7 on the others), so the bound the kernel is held to there
   is one the reference's own arithmetic meets.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import loss_ref  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
POLICY_KEYS = dict(zip(("ce", "ce_norm", "kld", "mse"), loss_ref.POLICY_FORMS))
VALUE_KEYS = {"se": "SE", "ae": "AE"}


@pytest.mark.parametrize("name", ["ttt", "scs", "one"])
def test_float64_restatement_equals_the_genuine_loss_functions(name):
    kat = np.load(os.path.join(GOLDEN, "loss_kat.npz"))
    seen = 0
    for pkey, (pname, norm) in POLICY_KEYS.items():
        for vkey, vname in VALUE_KEYS.items():
            key = f"{name}_{pkey}_{vkey}"
            if pkey == "ce_norm" and name == "one":
                assert key + "_losses" not in kat.files          # log(1) = 0: the reference divides by zero there
                continue
            losses, dlogits, dvalues = loss_ref.reference(kat[f"{name}_logits"], kat[f"{name}_values"],
                                                          kat[f"{name}_target_policies"], kat[f"{name}_target_values"],
                                                          pname, vname, norm, torch.float64)
            assert loss_ref.rel_err(kat[key + "_losses"], losses) <= 1e-6, key
            for got, want in ((dlogits, kat[key + "_dlogits"]), (dvalues, kat[key + "_dvalues"])):
                assert got.shape == want.shape, key
                assert loss_ref.max_abs_err(want, got) <= 1e-6 * np.abs(got).max(), key
            seen += 3
    # nothing in the file is left unchecked: 4 inputs per batch + 3 outputs per form
    assert seen + 4 == sum(k.startswith(name + "_") for k in kat.files)


def test_the_hard_inputs_are_what_they_claim():
    for (B, A) in loss_ref.SMALL_SHAPES + loss_ref.LARGE_SHAPES:
        lo = 256 * ((A - 1) // 256)
        for kind in loss_ref.TARGET_KINDS:
            t = loss_ref.make_targets(B, A, kind).astype(np.float32)
            assert t.shape == (B, A) and np.all(t >= 0) and np.allclose(t.sum(1), 1.0, atol=1e-6, rtol=0)
            nz = (t != 0).sum(1)
            assert np.all(nz >= 1)
            if kind == "onehot":
                assert np.all(nz == 1) and np.all(t.max(1) == 1.0)
            if kind == "dense":
                assert np.all(nz == A)
            if kind == "tail":
                assert np.all(t[:, :lo] == 0) and lo < A
            if kind in ("sparse", "tail"):
                assert np.all(nz <= 12)
        values, target_values = loss_ref.make_values(B, A)
        assert values.shape == (B, 1) and values.dtype == np.float32 and set(target_values.tolist()) <= {-1, 0, 1}
        assert values[0, 0] == target_values[0] and (B == 1 or np.all(values[1:, 0] != target_values[1:]))
        x = loss_ref.make_logits(B, A, "equal")
        assert np.all(x == np.float32(-3.25))
        assert np.all(loss_ref.make_logits(B, A, "offset1e4") > 9900.0)
        assert np.all(loss_ref.make_logits(B, A, "spike80").max(1) > 70.0)
    assert len(loss_ref.GRID) == 10 * 5 + 2 * 2 * 4


@pytest.mark.parametrize("B,A,logit_kind,target_kinds", loss_ref.GRID,
                         ids=[f"{B}x{A}-{lk}" + ("" if len(tks) > 1 else "-" + tks[0]) for B, A, lk, tks in loss_ref.GRID])
def test_float32_restatement_meets_the_loss_bound_on_the_hard_inputs(B, A, logit_kind, target_kinds):
    for tk, pname, norm, vname in loss_ref.grid_cases(B, A, target_kinds):
        case = (B, A, logit_kind, tk, pname, norm, vname)
        l64, dl64, dv64 = loss_ref.grid_reference(*case, torch.float64)
        l32, dl32, dv32 = loss_ref.grid_reference(*case, torch.float32)
        assert np.isfinite(l64).all() and np.isfinite(dl64).all() and np.isfinite(dv64).all(), case
        assert loss_ref.rel_err(l32, l64) <= 2e-6, (case, l32, l64)
