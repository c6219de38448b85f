"""The fused loss kernel (nuzero_amd/csrc/loss.hip, C ABI nz_loss_forward_backward, nuzero_amd/loss.py) against a float64
restatement of the reference's per-sample loop (tests/loss_ref.py, pinned to the genuine loss functions by
tests/test_loss_ref_host.py), at the shapes, logits and targets where such a kernel goes wrong.  Needs a GPU.

Shapes (B, A): one lane, two, one wave -1 / 0 / +1, one 256-thread stride -1 / 0 / +1, two strides + 1, the 10 x 10 SCS
action count (2100), batches of 300 and 2048 for the fixed-order sum kernel.  Logits: 2 N, 30 N, 2 N + 1e4, all equal,
N with +80 on one entry per row.  Targets: sparse visit fractions, one-hot, dense, non-zero in the last ragged stride
only.  Values tanh(N), sample 0's exactly on its target; targets in {-1, 0, 1}.  Every policy loss x SE / AE, CEL also
normalised by log(B).

Bounds (tests/loss_ref.py LOSS_BOUND, gradient_bounds): losses 2e-6 relative to float64 -- the float32 restatement
itself meets that on these inputs (tests/test_loss_ref_host.py); gradients: max |error| <= max(2e-6 of the largest
reference entry, 4 x the float32 restatement's own error on the case, 2e-6 x policy_scale).

scripts/loss_edge_errors.py records the kernel's worst errors on the same grid (profiles/loss_edge_errors.json);
DESIGN.md section 2 statement 12 says what has been measured.
"""
import os
import sys
from ctypes import c_void_p

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import loss_ref  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = -12345.5


def _ptr(t):
    return None if t is None else c_void_p(t.data_ptr())


def raw_loss(x, v, tp, tv, pname, vname, norm, grads=True, out=None, batch=None, actions=None, check=True):
    """nz_loss_forward_backward on device tensors x [B, A], v [B], tp [B, A], tv [B]; returns (status, losses3, dlogits,
    dvalues, workspace).  out = (losses3, dlogits, dvalues, workspace) to write into given tensors."""
    from nuzero_amd import _lib
    from nuzero_amd._lib import lib
    from nuzero_amd.loss import POLICY_LOSSES, VALUE_LOSSES
    B, A = (tp if x is None else x).shape
    if out is None:
        out = (torch.empty(3, device="cuda"), torch.empty_like(x) if grads else None,
               torch.empty_like(v) if grads else None, torch.empty(2 * B, device="cuda"))
    losses, dl, dv, work = out
    st = lib.nz_loss_forward_backward(_ptr(x), _ptr(v), _ptr(tp), _ptr(tv), B if batch is None else batch,
                                      A if actions is None else actions, POLICY_LOSSES.get(pname, pname),
                                      VALUE_LOSSES.get(vname, vname), int(norm), _ptr(losses), _ptr(dl), _ptr(dv),
                                      _ptr(work), c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    if check:
        assert st == _lib.NZ_OK, lib.nz_loss_last_error()
    return st, losses, dl, dv, work


def _device_inputs(B, A, logit_kind, target_kind):
    x, v, tp, tv = loss_ref.grid_inputs(B, A, logit_kind, target_kind)
    return (torch.tensor(x).cuda(), torch.tensor(v).cuda(), torch.tensor(tp.tolist()).cuda(),      # list: float32
            torch.tensor(tv).float().cuda())


@pytest.mark.parametrize("B,A,logit_kind,target_kinds", loss_ref.GRID,
                         ids=[f"{B}x{A}-{lk}" + ("" if len(tks) > 1 else "-" + tks[0]) for B, A, lk, tks in loss_ref.GRID])
def test_kernel_meets_the_float64_reference(B, A, logit_kind, target_kinds):
    """Every case of the grid, through calculate_loss + combined_loss.backward() and through the raw ABI."""
    from nuzero_amd.loss import calculate_loss
    failures, worst = [], [0.0, 0.0, 0.0]
    inputs = {tk: _device_inputs(B, A, logit_kind, tk) for tk in target_kinds}
    for tk, pname, norm, vname in loss_ref.grid_cases(B, A, target_kinds):
        case = (B, A, logit_kind, tk, pname, norm, vname)
        ref64 = loss_ref.grid_reference(*case, torch.float64)
        ref32 = loss_ref.grid_reference(*case, torch.float32)
        dl_bound, dv_bound = loss_ref.gradient_bounds(ref64, ref32, B, norm)
        x, v, tp, tv = inputs[tk]
        _, losses, dl, dv, _ = raw_loss(x, v.reshape(B), tp, tv, pname, vname, norm)
        x, v = x.detach().requires_grad_(), v.detach().requires_grad_()
        v_loss, p_loss, c_loss = calculate_loss((x, v), tp, tv, pname, vname, norm)
        c_loss.backward()
        assert x.grad.shape == x.shape and v.grad.shape == v.shape == (B, 1)
        for route, got_l, got_dl, got_dv in (("abi", losses, dl, dv.reshape(B, 1)),
                                             ("calculate_loss", torch.stack([v_loss, p_loss, c_loss]), x.grad, v.grad)):
            figures = (loss_ref.rel_err(got_l.detach().cpu().numpy(), ref64[0]),
                       loss_ref.max_abs_err(got_dl.cpu().numpy(), ref64[1]),
                       loss_ref.max_abs_err(got_dv.cpu().numpy(), ref64[2]))
            bounds = (loss_ref.LOSS_BOUND, dl_bound, dv_bound)
            worst = [max(w, f / b) for w, f, b in zip(worst, figures, bounds)]
            if not all(np.isfinite(f) and f <= b for f, b in zip(figures, bounds)):
                failures.append((route, case, "loss rel %.3g, dlogits %.3g, dvalues %.3g" % figures,
                                 "bounds %.3g, %.3g, %.3g" % bounds))
    print(f"{B}x{A} {logit_kind} {'/'.join(target_kinds)}: worst error / bound: losses {worst[0]:.3f}, "
          f"dlogits {worst[1]:.3f}, dvalues {worst[2]:.3f}")
    assert not failures, failures


@pytest.mark.parametrize("pname", ["CEL", "KLD", "MSE"])
def test_absolute_error_on_the_target_has_gradient_zero(pname):
    """d = t - v == 0 for sample 0: |d|'s subgradient is 0 there, as torch's abs backward has it -- exactly."""
    for (B, A) in ((3, 1), (4, 65), (300, 9)):
        x, v, tp, tv = _device_inputs(B, A, "normal2", "sparse")
        assert v[0, 0] == tv[0]
        _, losses, dl, dv, _ = raw_loss(x, v.reshape(B), tp, tv, pname, "AE", False)
        assert dv[0].item() == 0.0
        ref = loss_ref.grid_reference(B, A, "normal2", "sparse", pname, False, "AE", torch.float64)
        assert ref[2][0, 0] == 0.0 and np.array_equal(np.sign(dv.cpu().numpy()), np.sign(ref[2][:, 0]))


@pytest.mark.parametrize("logit_kind", loss_ref.LOGIT_KINDS)
def test_one_action_has_no_policy_loss(logit_kind):
    """A = 1: log_softmax is exactly 0 whatever the logit, so the cross entropy is exactly 0 and its gradient row is
    zeros (softmax 1 times the smoothed target's sum 1, minus the smoothed target 1)."""
    B, A = 3, 1
    x, v, tp, tv = _device_inputs(B, A, logit_kind, "onehot")
    for norm in (False, True):
        _, losses, dl, dv, _ = raw_loss(x, v.reshape(B), tp, tv, "CEL", "SE", norm)
        assert losses[1].item() == 0.0 and losses[2].item() == losses[0].item()
        assert torch.equal(dl, torch.zeros_like(dl))


def _wrapper_inputs():
    """logits [B, P, H, W] taken from a permuted tensor (not contiguous), values [B, 1]."""
    B, P, H, W = 5, 3, 4, 7
    rs = np.random.RandomState(23)
    x = torch.tensor((3.0 * rs.standard_normal((B, H, W, P)) + 50.0).astype(np.float32)).cuda().permute(0, 3, 1, 2)
    assert x.shape == (B, P, H, W) and not x.is_contiguous()
    v = torch.tensor(np.tanh(rs.standard_normal((B, 1))).astype(np.float32)).cuda()
    tp = loss_ref.make_targets(B, P * H * W, "sparse")
    tv = rs.randint(-1, 2, size=B)
    return x, v, tp, tv


@pytest.mark.parametrize("pname,vname,norm", [("CEL", "SE", True), ("KLD", "AE", False), ("MSE", "SE", False)])
def test_wrapper_differentiates_each_output(pname, vname, norm):
    """p_loss.backward() alone, v_loss.backward() alone and (0.5 v + 2 p + 3 c).backward() against float64 autograd of
    the same expression; gradients come back in the inputs' shapes."""
    from nuzero_amd.loss import calculate_loss
    x0, v0, tp, tv = _wrapper_inputs()
    B = x0.shape[0]
    tp_dev, tv_dev = torch.tensor(tp.tolist()).cuda(), torch.tensor(tv).float().cuda()
    for weights in ((0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (0.5, 2.0, 3.0)):
        x, v = x0.detach().requires_grad_(), v0.detach().requires_grad_()
        assert not x.is_contiguous()
        v_loss, p_loss, c_loss = calculate_loss((x, v), tp_dev, tv_dev, pname, vname, norm)
        (weights[0] * v_loss + weights[1] * p_loss + weights[2] * c_loss).backward()
        args = (x0.cpu().numpy(), v0.cpu().numpy(), tp, tv, pname, vname, norm)
        ref64 = loss_ref.reference(*args, torch.float64, weights)
        ref32 = loss_ref.reference(*args, torch.float32, weights)
        got_l = np.array([v_loss.item(), p_loss.item(), c_loss.item()])
        assert loss_ref.rel_err(got_l, ref64[0]) <= loss_ref.LOSS_BOUND, (weights, got_l, ref64[0])
        dl_bound, dv_bound = loss_ref.gradient_bounds(ref64, ref32, B, norm)
        if weights[1] == 0.0 and weights[2] == 0.0:
            assert x.grad is None or torch.equal(x.grad, torch.zeros_like(x))
            assert np.all(ref64[1] == 0.0)
        else:
            assert x.grad.shape == x0.shape == ref64[1].shape
            # the expression's weight on the policy loss scales every term of the bound
            err = loss_ref.max_abs_err(x.grad.cpu().numpy(), ref64[1])
            print(pname, weights, "dlogits error %.3g, bound %.3g" % (err, dl_bound))
            assert err <= max(dl_bound, 2e-6 * (weights[1] + weights[2]) * loss_ref.policy_scale(B, norm)), weights
        if weights[0] == 0.0 and weights[2] == 0.0:
            assert v.grad is None or torch.equal(v.grad, torch.zeros_like(v))
            assert np.all(ref64[2] == 0.0)
        else:
            assert v.grad.shape == v0.shape == ref64[2].shape == (B, 1)
            assert loss_ref.max_abs_err(v.grad.cpu().numpy(), ref64[2]) <= dv_bound, weights


def test_wrapper_on_a_side_stream_returns_the_same_bits():
    from nuzero_amd.loss import calculate_loss
    x0, v0, tp, tv = _wrapper_inputs()
    tp_dev, tv_dev = torch.tensor(tp.tolist()).cuda(), torch.tensor(tv).float().cuda()

    def run():
        x, v = x0.detach().requires_grad_(), v0.detach().requires_grad_()
        losses = calculate_loss((x, v), tp_dev, tv_dev, "CEL", "SE", True)
        losses[2].backward()
        return torch.stack([l.detach() for l in losses]), x.grad, v.grad

    torch.cuda.synchronize()
    want = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = run()
    side.synchronize()
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        assert torch.equal(g, w)


ABI_CASES = [(3, 257, "offset1e4", "tail", "CEL", False, "SE"), (2, 2100, "normal30", "dense", "MSE", False, "AE"),
             (300, 9, "normal2", "sparse", "KLD", False, "SE"), (4, 64, "spike80", "onehot", "CEL", True, "AE")]


@pytest.mark.parametrize("case", ABI_CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[4]}")
def test_abi_fixed_order_null_gradients_and_guard_rows(case):
    B, A, logit_kind, tk, pname, norm, vname = case
    x, v, tp, tv = _device_inputs(B, A, logit_kind, tk)
    v = v.reshape(B)
    # the header promises a fixed summation order: the same inputs twice give the same bits
    _, l1, dl1, dv1, _ = raw_loss(x, v, tp, tv, pname, vname, norm)
    _, l2, dl2, dv2, _ = raw_loss(x, v, tp, tv, pname, vname, norm)
    assert torch.equal(l1, l2) and torch.equal(dl1, dl2) and torch.equal(dv1, dv2)
    assert torch.isfinite(l1).all() and torch.isfinite(dl1).all() and torch.isfinite(dv1).all()
    # dlogits / dvalues may be NULL: the same losses to the bit
    _, l3, dl3, dv3, _ = raw_loss(x, v, tp, tv, pname, vname, norm, grads=False)
    assert dl3 is None and dv3 is None and torch.equal(l3, l1)
    # outputs as the middle rows of larger tensors: every element inside is written, nothing outside is
    bufs = [torch.full((3, n), SENTINEL, device="cuda") for n in (3, B * A, B, 2 * B)]
    out = (bufs[0][1], bufs[1][1].view(B, A), bufs[2][1], bufs[3][1])
    _, l4, dl4, dv4, work = raw_loss(x, v, tp, tv, pname, vname, norm, out=out)
    for buf in bufs:
        assert torch.all(buf[0] == SENTINEL) and torch.all(buf[2] == SENTINEL)
        assert torch.all(buf[1] != SENTINEL)
    assert torch.equal(l4, l1) and torch.equal(dl4, dl1) and torch.equal(dv4, dv1)
    # and with NULL gradients only the losses and the workspace
    bufs = [torch.full((3, n), SENTINEL, device="cuda") for n in (3, 2 * B)]
    raw_loss(x, v, tp, tv, pname, vname, norm, grads=False, out=(bufs[0][1], None, None, bufs[1][1]))
    for buf in bufs:
        assert torch.all(buf[0] == SENTINEL) and torch.all(buf[2] == SENTINEL) and torch.all(buf[1] != SENTINEL)
    assert torch.equal(bufs[0][1], l1)


def test_abi_rejects_bad_arguments():
    from nuzero_amd import _lib
    B, A = 4, 9
    x, v, tp, tv = _device_inputs(4, 64, "normal2", "sparse")
    x, tp, v = x[:, :A].contiguous(), tp[:, :A].contiguous(), v.reshape(B)
    sent = [torch.full((n,), SENTINEL, device="cuda") for n in (3, B * A, B, 2 * B)]
    out = (sent[0], sent[1].view(B, A), sent[2], sent[3])

    def status(**kw):
        args = dict(x=x, v=v, tp=tp, tv=tv, pname="CEL", vname="SE", norm=False, out=out, check=False)
        args.update(kw)
        return raw_loss(**args)[0]

    assert status() == _lib.NZ_OK
    for s in sent:
        s.fill_(SENTINEL)
    torch.cuda.synchronize()
    assert status(batch=0) == _lib.NZ_ERR_ARG and status(batch=-1) == _lib.NZ_ERR_ARG
    assert status(actions=0) == _lib.NZ_ERR_ARG and status(actions=-5) == _lib.NZ_ERR_ARG
    for bad in (-1, 3):
        assert status(pname=bad) == _lib.NZ_ERR_ARG
    for bad in (-1, 2):
        assert status(vname=bad) == _lib.NZ_ERR_ARG
    for name in ("x", "v", "tp", "tv"):
        assert status(**{name: None}, batch=B, actions=A) == _lib.NZ_ERR_ARG, name
    assert status(out=(None, out[1], out[2], out[3])) == _lib.NZ_ERR_ARG
    assert status(out=(out[0], out[1], out[2], None)) == _lib.NZ_ERR_ARG
    assert _lib.lib.nz_loss_last_error()
    # a rejected call launches nothing
    for s in sent:
        assert torch.all(s == SENTINEL)
