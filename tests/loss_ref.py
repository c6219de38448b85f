"""A plain restatement of AlphaZero.calculate_loss (Training/AlphaZero.py:891-921) in torch on the CPU with a `dtype`
argument, and the hard inputs the fused loss kernel (nuzero_amd/csrc/loss.hip) is held to.  No GPU.

`reference(..., dtype=torch.float64)` is the reference of tests/test_gpu_loss_edges.py; `dtype=torch.float32` is the
reference's OWN arithmetic (the genuine loop accumulates float32 tensors) and only measures how far that arithmetic
sits from float64.  tests/test_loss_ref_host.py pins the restatement to tests/golden/loss_kat.npz, the vectors of the
genuine loss functions (tests/golden/make_golden_replay.py).

The loop is the per-sample loop as make_golden_replay.py::calculate_loss drives it: torch.tensor(target list) rounds
the targets to float32 first, the sums are accumulated with `+=` in sample order, then `/ log(B)` when normalising,
then `/ B`.  Policy losses (AlphaZero.py:325-333, Utils/Functions/loss_functions.py:7-26), value losses
(loss_functions.py:28-33):
  CEL  nn.CrossEntropyLoss(label_smoothing=0.02) with probability targets
  KLD  nn.KLDivLoss() (reduction 'mean': over the A elements) on log_softmax(x)
  MSE  (t - softmax(x))^2 over the entries with t != 0, divided by their count
  SE   (t - v)^2          AE   |t - v|
"""
import functools
import math
import warnings

import numpy as np
import torch
import torch.nn.functional as F

POLICY_FORMS = (("CEL", False), ("CEL", True), ("KLD", False), ("MSE", False))     # (name, normalize_policy)
VALUE_FORMS = ("SE", "AE")


def policy_term(x, t, name):
    """One sample: x [A] logits, t [A] target, both of the working dtype."""
    if name == "CEL":
        return F.cross_entropy(x, t, label_smoothing=0.02)
    if name == "KLD":
        return F.kl_div(F.log_softmax(x, dim=0), t, reduction="mean")
    if name == "MSE":
        mask = t != 0
        d = t[mask] - F.softmax(x, dim=0)[mask]
        return (d * d).sum() / int(mask.sum())
    raise KeyError(name)


def value_term(v, t, name):
    if name == "SE":
        return (t - v) ** 2
    if name == "AE":
        return torch.abs(t - v)
    raise KeyError(name)


def calculate_loss(outputs, targets, batch_size, policy_loss, value_loss, normalize_policy, dtype):
    """The loop of AlphaZero.calculate_loss; targets = [(value, policy list)] as the replay buffer hands them out."""
    target_values, target_policies = list(zip(*targets))
    predicted_policies, predicted_values = outputs
    # torch.tensor(list of floats) is float32 (AlphaZero.py:901); all rows in one call, the same rounding
    target_policies = torch.tensor(target_policies, dtype=torch.float32).to(dtype).unbind(0)
    target_values = torch.tensor(target_values).to(dtype).unbind(0)
    p_sum = 0.0
    v_sum = 0.0
    for i in range(batch_size):
        p_sum += policy_term(torch.flatten(predicted_policies[i]), target_policies[i], policy_loss)
        v_sum += value_term(predicted_values[i], target_values[i], value_loss)
    if normalize_policy:
        p_sum /= math.log(len(targets))
    v_sum /= batch_size
    p_sum /= batch_size
    return v_sum, p_sum, p_sum + v_sum


def reference(logits, values, target_policies, target_values, policy_loss="CEL", value_loss="SE",
              normalize_policy=False, dtype=torch.float64, weights=(0.0, 0.0, 1.0)):
    """logits [B, ...] and values [B] or [B, 1] float32 arrays, target_policies [B, A] (any float type; rounded to
    float32 as the trainer does), target_values [B].  Returns (losses [3] = (value, policy, combined), dlogits, dvalues)
    as float64 arrays: the gradients of weights[0] * value + weights[1] * policy + weights[2] * combined, by autograd,
    in the shapes of `logits` and `values`."""
    lg = torch.tensor(np.asarray(logits, np.float32)).to(dtype).requires_grad_()
    vl = torch.tensor(np.asarray(values, np.float32)).to(dtype).requires_grad_()
    B = lg.shape[0]
    targets = list(zip(np.asarray(target_values).tolist(), np.asarray(target_policies).tolist()))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)          # nn.KLDivLoss()'s note on reduction='mean', per sample
        # (unbind: the samples as a tuple of rows -- indexing the batch tensor costs O(B * A) per sample in backward)
        v_loss, p_loss, c_loss = calculate_loss((lg.unbind(0), vl.reshape(B, 1).unbind(0)), targets, B, policy_loss,
                                                value_loss, normalize_policy, dtype)
        (weights[0] * v_loss + weights[1] * p_loss + weights[2] * c_loss).reshape(()).backward()
    losses = np.array([float(v_loss.detach()), float(p_loss.detach()), float(c_loss.detach())], np.float64)
    return losses, lg.grad.double().numpy(), vl.grad.double().numpy()


# ---- the hard inputs ------------------------------------------------------------------------------------------------
# (B, A): one lane, two lanes, one wave -1 / 0 / +1, one workgroup stride (256) -1 / 0 / +1, two strides + 1, the 10 x 10
# SCS action count (21 * 100 = 8 strides + 52); the batches of 300 and 2048 are for the fixed-order sum kernel.
SMALL_SHAPES = ((3, 1), (5, 2), (4, 63), (4, 64), (4, 65), (3, 255), (3, 256), (3, 257), (3, 513), (2, 2100))
LARGE_SHAPES = ((300, 9), (2048, 9))
LOGIT_KINDS = ("normal2", "normal30", "offset1e4", "equal", "spike80")
TARGET_KINDS = ("sparse", "onehot", "dense", "tail")
# (B, A, logit kind, target kinds): what one test case covers; a large batch takes one target kind per case, since the
# per-sample reference loop is what costs time there
GRID = [(B, A, lk, TARGET_KINDS) for (B, A) in SMALL_SHAPES for lk in LOGIT_KINDS] + \
       [(B, A, lk, (tk,)) for (B, A) in LARGE_SHAPES for lk in LOGIT_KINDS[:2] for tk in TARGET_KINDS]


def make_logits(B, A, kind):
    rs = np.random.RandomState([11, B, A, LOGIT_KINDS.index(kind)])
    n = rs.standard_normal((B, A))
    if kind == "normal2":
        x = 2.0 * n
    elif kind == "normal30":
        x = 30.0 * n
    elif kind == "offset1e4":
        x = 2.0 * n + 1e4
    elif kind == "equal":
        x = np.full((B, A), -3.25)
    else:                                            # N(0, 1) with +80 on one entry per row
        x = n
        x[np.arange(B), rs.randint(A, size=B)] += 80.0
    return x.astype(np.float32)


def _fractions(rs, A, idx):
    """Visit fractions on the entries `idx`, as the golden generator makes them: int / int in float64."""
    visits = rs.randint(1, 60, size=len(idx))
    pol = [0.0] * A
    for a, v in zip(idx, visits):
        pol[int(a)] = int(v) / int(visits.sum())
    return pol


def make_targets(B, A, kind):
    """[B, A] float64 (the trainer rounds them to float32).  sparse: at most 12 non-zeros (make_golden_replay.py);
    onehot; dense: every entry non-zero; tail: non-zero only in the last, ragged stride of the kernel's 256 threads,
    at indices >= 256 * floor((A - 1) / 256)."""
    rs = np.random.RandomState([13, B, A, TARGET_KINDS.index(kind)])
    rows = []
    for _ in range(B):
        if kind == "sparse":
            idx = rs.choice(A, size=int(rs.randint(1, min(A, 12) + 1)), replace=False)
        elif kind == "onehot":
            idx = [rs.randint(A)]
        elif kind == "dense":
            idx = np.arange(A)
        else:
            lo = 256 * ((A - 1) // 256)
            idx = lo + rs.choice(A - lo, size=int(rs.randint(1, min(A - lo, 12) + 1)), replace=False)
        rows.append(_fractions(rs, A, idx))
    return np.array(rows, np.float64)


def make_values(B, A):
    """values tanh(N) [B, 1] float32 -- sample 0's set exactly to its target, where |t - v| has subgradient 0 -- and
    targets in {-1, 0, 1}."""
    rs = np.random.RandomState([17, B, A])
    values = np.tanh(rs.standard_normal((B, 1))).astype(np.float32)
    target_values = rs.randint(-1, 2, size=B).astype(np.int32)
    values[0, 0] = target_values[0]
    return values, target_values


def grid_cases(B, A, target_kinds):
    """(target kind, policy loss, normalize_policy, value loss) of one entry of GRID: every policy loss x SE / AE, CEL
    also normalised by log(B); the two large batches with SE only."""
    vforms = VALUE_FORMS if (B, A) in SMALL_SHAPES else VALUE_FORMS[:1]
    return [(tk, pl, norm, vl) for tk in target_kinds for (pl, norm) in POLICY_FORMS for vl in vforms
            if not (norm and B == 1)]


@functools.lru_cache(maxsize=None)
def grid_inputs(B, A, logit_kind, target_kind):
    values, target_values = make_values(B, A)
    return make_logits(B, A, logit_kind), values, make_targets(B, A, target_kind), target_values


@functools.lru_cache(maxsize=None)
def grid_reference(B, A, logit_kind, target_kind, policy_loss, normalize_policy, value_loss, dtype):
    """reference() on a case of the grid, computed once per process and shared (treat the arrays as read-only)."""
    return reference(*grid_inputs(B, A, logit_kind, target_kind), policy_loss, value_loss, normalize_policy, dtype)


def rel_err(got, want):
    """Largest relative error of the three losses; an exact zero must be met exactly."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(got - want) / np.abs(want)
    return float(np.where(got == want, 0.0, r).max())


def max_abs_err(got, want):
    return float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max())


# ---- the bounds the kernel is held to against float64 ----------------------------------------------------------------
LOSS_BOUND = 2e-6        # relative, on each of the three losses: the project's bound, which the float32 restatement meets


def policy_scale(B, normalize_policy):
    return 1.0 / (B * math.log(B)) if normalize_policy else 1.0 / B


def gradient_bounds(ref64, ref32, B, normalize_policy):
    """(bound on max |dlogits - float64|, bound on max |dvalues - float64|) for one case; ref64 / ref32 are what
    reference() returned in float64 / float32.  dlogits, the largest of
      (a) 2e-6 of the largest reference entry: the project's rule;
      (b) 4 x the float32 restatement's own error on the same case (the factor is for another summation tree and the
          device's expf / logf against torch's; fixed before the kernel's figures were seen);
      (c) 2e-6 x policy_scale: every entry is policy_scale times an O(1) float32 quantity, and on saturated rows the
          whole gradient is ~1e-10, where float32 softmax itself is 100 % off.
    dvalues has no softmax in it: (a) and (b) only."""
    _, dl64, dv64 = ref64
    _, dl32, dv32 = ref32
    return (max(2e-6 * float(np.abs(dl64).max()), 4.0 * max_abs_err(dl32, dl64), 2e-6 * policy_scale(B, normalize_policy)),
            max(2e-6 * float(np.abs(dv64).max()), 4.0 * max_abs_err(dv32, dv64)))
