"""Errors of the fused loss kernel (nz_loss_forward_backward) on the hard inputs of tests/test_gpu_loss_edges.py
against the float64 restatement of the reference's loop (tests/loss_ref.py) -- next to the errors of that restatement
run in float32, the reference's own arithmetic.  Runs the grid once through the raw ABI and measures, per case,

    [loss rel, dlogits max abs, dvalues max abs]   of the kernel (under --label) and of the float32 restatement,
    [loss bound, dlogits bound, dvalues bound]     as the test computes them (loss_ref.gradient_bounds),

all against float64.  The file holds one record per (batch x actions, logit kind) -- 54 for the 1,664 cases: the number
of cases, and for the kernel and the float32 restatement the worst error and the worst error / bound per column over
the group's target kinds and loss forms, with the case that has the worst ratio.  --per-case writes one record per case
instead (some 320 kB: for looking at, not for committing).  --out is read first if it exists and only this label's
figures are replaced, so one file holds the kernel before and after a change (build the library at each state, run
with another --label).  No threshold is applied here; `outside_bounds` lists the cases a test would fail on.  Prints a
one-line JSON summary.

    python scripts/loss_edge_errors.py --label shifted_logits --kernel "xs = x - mx; logp = xs - logf(se)" \
        [--out profiles/loss_edge_errors.json]
"""
import argparse
import json
import os
import subprocess
import sys
from ctypes import c_void_p

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import loss_ref  # noqa: E402


def kernel(x, v, tp, tv, pname, vname, norm):
    from nuzero_amd import _lib
    from nuzero_amd._lib import lib
    from nuzero_amd.loss import POLICY_LOSSES, VALUE_LOSSES
    B, A = x.shape
    losses, dl, dv = torch.empty(3, device="cuda"), torch.empty_like(x), torch.empty(B, device="cuda")
    work = torch.empty(2 * B, device="cuda")
    st = lib.nz_loss_forward_backward(c_void_p(x.data_ptr()), c_void_p(v.data_ptr()), c_void_p(tp.data_ptr()),
                                      c_void_p(tv.data_ptr()), B, A, POLICY_LOSSES[pname], VALUE_LOSSES[vname], int(norm),
                                      c_void_p(losses.data_ptr()), c_void_p(dl.data_ptr()), c_void_p(dv.data_ptr()),
                                      c_void_p(work.data_ptr()), c_void_p(torch.cuda.current_stream().cuda_stream))
    if st != _lib.NZ_OK:
        raise _lib.NzError(st, (lib.nz_loss_last_error() or b"").decode())
    torch.cuda.synchronize()
    return losses.cpu().numpy(), dl.cpu().numpy(), dv.cpu().numpy().reshape(B, 1)


def errors(got, ref64):
    return [loss_ref.rel_err(got[0], ref64[0]), loss_ref.max_abs_err(got[1], ref64[1]),
            loss_ref.max_abs_err(got[2], ref64[2])]


def sig(values):
    return [float("%.3g" % v) for v in values]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", required=True, help="name of the kernel state measured, e.g. lse_order / shifted_logits")
    ap.add_argument("--kernel", default="", help="one line on what the kernel computes at this state")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_edge_errors.json"))
    ap.add_argument("--per-case", action="store_true", help="one record per case instead of one per (shape, logit kind)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("loss_edge_errors.py measures the kernel on the GPU; there is none")
    doc = {"cases": {}, "groups": {}, "runs": {}}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc["columns"] = ["loss rel", "dlogits max abs", "dvalues max abs"]
    doc["against"] = "float64 restatement of the reference's per-sample loop (tests/loss_ref.py)"
    doc["bounds_rule"] = ("losses 2e-6 relative; dlogits max(2e-6 of the largest reference entry, 4 x float32 "
                          "restatement's error, 2e-6 x policy_scale); dvalues max(2e-6 of the largest entry, 4 x float32)")

    outside, worst_ratio, groups = [], [0.0, 0.0, 0.0], {}
    by_logits = {lk: {"kernel": [0.0, 0.0], "float32": [0.0, 0.0]} for lk in loss_ref.LOGIT_KINDS}
    for B, A, lk, tks in loss_ref.GRID:
        for tk in tks:
            x, v, tp, tv = loss_ref.grid_inputs(B, A, lk, tk)
            dev = (torch.tensor(x).cuda(), torch.tensor(v).reshape(B).cuda(), torch.tensor(tp.tolist()).cuda(),
                   torch.tensor(tv).float().cuda())
            for _, pname, norm, vname in loss_ref.grid_cases(B, A, (tk,)):
                case = (B, A, lk, tk, pname, norm, vname)
                ref64 = loss_ref.grid_reference(*case, torch.float64)
                ref32 = loss_ref.grid_reference(*case, torch.float32)
                bounds = [loss_ref.LOSS_BOUND, *loss_ref.gradient_bounds(ref64, ref32, B, norm)]
                e_k, e_32 = errors(kernel(*dev, pname, vname, norm), ref64), errors(ref32, ref64)
                cid = f"{B}x{A}/{lk}/{tk}/{pname}{'/logB' if norm else ''}/{vname}"
                if a.per_case:
                    rec = doc["cases"].setdefault(cid, {})
                    rec["largest dlogits entry"] = float("%.3g" % np.abs(ref64[1]).max())
                    rec["bounds"], rec["float32"], rec[a.label] = sig(bounds), sig(e_32), sig(e_k)
                grp = groups.setdefault(f"{B}x{A}/{lk}", {"cases": 0})
                grp["cases"] += 1
                for who, e in ((a.label, e_k), ("float32", e_32)):
                    w = grp.setdefault(who, {"worst": [0.0] * 3, "worst_over_bound": [0.0] * 3, "at": None})
                    ratio = [x / b for x, b in zip(e, bounds)]
                    if w["at"] is None or max(ratio) > max(w["worst_over_bound"]):
                        w["at"] = cid
                    w["worst"] = [max(x, y) for x, y in zip(w["worst"], e)]
                    w["worst_over_bound"] = [max(x, y) for x, y in zip(w["worst_over_bound"], ratio)]
                if not all(np.isfinite(e) and e <= b for e, b in zip(e_k, bounds)):
                    outside.append(cid)
                worst_ratio = [max(w, e / b) for w, e, b in zip(worst_ratio, e_k, bounds)]
                # the issue's table: loss error, and gradient error over the largest entry, per logit kind
                scale = max(float(np.abs(ref64[1]).max()), 1e-300)
                for who, e in (("kernel", e_k), ("float32", e_32)):
                    w = by_logits[lk][who]
                    w[0], w[1] = max(w[0], e[0]), max(w[1], e[1] / scale)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                text=True).stdout.strip()
    except OSError:
        commit = ""
    summary = {"device": torch.cuda.get_device_name(0), "commit": commit or None, "kernel": a.kernel,
               "cases": sum(len(loss_ref.grid_cases(B, A, tks)) for B, A, _, tks in loss_ref.GRID),
               "outside_bounds": outside, "worst_error_over_bound": sig(worst_ratio),
               "worst_by_logits [loss rel, dlogits error / largest entry]": {k: {w: sig(e) for w, e in d.items()}
                                                                            for k, d in by_logits.items()}}
    doc["runs"][a.label] = summary
    for gid, grp in groups.items():                   # this label's and the float32 figures replace the file's
        rec = doc.setdefault("groups", {}).setdefault(gid, {})
        rec["cases"] = grp["cases"]
        for who in (a.label, "float32"):
            rec[who] = {"worst": sig(grp[who]["worst"]), "worst_over_bound": sig(grp[who]["worst_over_bound"]),
                        "at": grp[who]["at"]}
    print(json.dumps({a.label: summary}))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:                       # one group, or one case, per line
        f.write('{\n "columns": %s,\n "against": %s,\n "bounds_rule": %s,\n "runs": %s,\n' % (
            json.dumps(doc["columns"]), json.dumps(doc["against"]), json.dumps(doc["bounds_rule"]),
            json.dumps(doc["runs"], indent=1).replace("\n", "\n ")))
        for key in ("groups", "cases"):
            f.write(' %s: {\n' % json.dumps(key))
            f.write(",\n".join("  %s: %s" % (json.dumps(k), json.dumps(r)) for k, r in doc.get(key, {}).items()))
            f.write("\n }%s\n" % ("," if key == "groups" else ""))
        f.write("}\n")


if __name__ == "__main__":
    main()
