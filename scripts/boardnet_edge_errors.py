"""Measure the board nets (nz_boardnet_*) on the edge-shape cases of tests/boardnet_cases.py against the float64
oracle and write profiles/boardnet_edge_errors.json: per case, route (one-launch / per-layer) and batch size the worst
value of the project's three error measures, next to the float32 oracle's own figure on the same positions.

    python scripts/boardnet_edge_errors.py [--out profiles/boardnet_edge_errors.json]

Needs a GPU.  The file is only worth committing from a real device run."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402


def main():
    import torch
    import boardnet_cases as bc
    from nuzero_amd.boardnet import BoardNet
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "boardnet_edge_errors.json"))
    args = ap.parse_args()
    out = {"tolerance": bc.TOL, "reference": "oracle/net.py, dtype=float64",
           "measures": {"logit": "max |d logit| / (max |logit| of the position + 1)", "prob": "max |d probability|",
                        "value": "max |d value|"},
           "device": torch.cuda.get_device_name(0), "cases": {}}
    worst = 0.0
    for case in bc.CASES:
        x_all = bc.inputs(case, max(bc.all_batches(case)))
        want_all = bc.reference64(case, x_all)
        w = bc.weights(case)
        n32 = max(b for b in bc.all_batches(case) if b <= 37)
        ref32 = bc.errors(*bc.reference32(case, x_all[:n32], w), tuple(a[:n32] for a in want_all))
        runs = []
        plan = [(n, n, True) for n in case.batches] + [(n, bc.SHARED_MAX_BATCH, True) for n in case.batches]
        plan += [(n, n, False) for n in case.big_batches]
        for n, max_batch, one_launch in plan:
            net = BoardNet(case.arch, case.in_channels, case.policy_channels, case.rows, case.cols, width=case.width,
                           num_blocks=case.depth, recall=case.recall, value_activation=case.value_activation,
                           kernel_size=case.kernel_size, max_batch=max_batch, hex=case.hex)
            net.set_weights(w, case.iters)
            xd = torch.from_numpy(x_all[:n]).cuda()
            want = tuple(a[:n] for a in want_all)
            routes = (["one-launch"] if one_launch and net.fused() else []) + ["per-layer"]
            for route in routes:
                net.fused(route == "one-launch")
                probs, value, logits = net.forward(xd, want_logits=True)
                e = bc.errors(logits.cpu().numpy(), probs.cpu().numpy(), value.cpu().numpy(), want)
                runs.append({"n": n, "max_batch": max_batch, "route": route, **e})
                worst = max(worst, max(e.values()))
                print(f"{case.name:15s} n {n:5d} max_batch {max_batch:5d} {route:10s} " +
                      " ".join(f"{k} {v:.2e}" for k, v in sorted(e.items())), flush=True)
            net.close()
        out["cases"][case.name] = {"gain": case.gain, "reaches": case.reaches,
                                   "float32_oracle": {"n": n32, **ref32}, "runs": runs}
    out["worst_error"] = worst
    out["worst_ratio_to_tolerance"] = worst / bc.TOL
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"worst error {worst:.2e} = {worst / bc.TOL:.3f} of the tolerance -> {args.out}")
    assert np.isfinite(worst)


if __name__ == "__main__":
    main()
