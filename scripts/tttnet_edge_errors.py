"""Measure the fused 3x3 network pass (nz_net_forward, nz_net_forward_packed) on the cases of tests/tttnet_cases.py
against the float64 oracle and write profiles/tttnet_edge_errors.json: per case and batch size the worst value of the
project's three error measures, next to the float32 oracle's own figures on the 37 positions, one case per line.  The
packed pass is recorded as equal to nz_net_forward bit for bit, or not.

    python scripts/tttnet_edge_errors.py [--out profiles/tttnet_edge_errors.json]

The tolerance is not fitted to these figures: it stays 1e-5 (BASELINE.json north_star); the file records how much of it
the device uses.  Needs a GPU.  The file is only worth committing from a real device run."""
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
    import tttnet_cases as tc
    from nuzero_amd.engine import SelfPlayEngine
    from nuzero_amd.search_config import legacy_ttt_search_config
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tttnet_edge_errors.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tttnet_edge_errors.py measures the kernels on the GPU; there is none")
    out = {"tolerance": tc.TOL, "reference": "oracle/net.py, dtype=float64",
           "measures": {"logit": "max |d logit| / (max |logit| of the position + 1)", "prob": "max |d probability|",
                        "value": "max |d value|"},
           "columns": ["logit", "prob", "value"], "batch_sizes": list(tc.BATCHES),
           "packed_equal_bytes": "nz_net_forward_packed at P = 1, 3, 8 on the 37 positions has nz_net_forward's bytes",
           "device": torch.cuda.get_device_name(0)}
    cases = {}
    sig = lambda e: [float("%.3g" % e[k]) for k in ("logit", "prob", "value")]
    worst, worst_at, worst32 = 0.0, None, 0.0
    eng = SelfPlayEngine(legacy_ttt_search_config(10), 16)
    for case in tc.CASES:
        x_all = tc.inputs(case, tc.MAX_BATCH)
        want_all = tc.reference64(case, x_all)
        w = tc.weights(case)
        ref32 = tc.errors(*tc.reference32(case, x_all, w), want_all)
        worst32 = max(worst32, max(ref32.values()))
        eng.set_weights(w, width=case.width, num_blocks=case.num_blocks, recall=case.recall,
                        value_activation=case.value_activation, recurrent_iterations=case.iters, arch=case.arch,
                        kernel_size=case.kernel_size)
        device, packed_equal = {}, True
        for n in tc.BATCHES:
            logits, value, probs = (t.cpu().numpy() for t in eng.net_forward(x_all[:n]))
            e = tc.errors(logits, probs, value, tuple(a[:n] for a in want_all))
            device[str(n)] = sig(e)
            if n == tc.MAX_BATCH:
                for P in (1, 3, 8):
                    got = [t.cpu().numpy() for t in eng.net_forward(x_all[:n], positions_per_pass=P)]
                    packed_equal &= all(a.tobytes() == b.tobytes() for a, b in zip(got, (logits, value, probs)))
            if max(e.values()) > worst:
                worst, worst_at = max(e.values()), f"{case.name} n={n}"
            print(f"{case.name:16s} n {n:3d} " + " ".join(f"{k} {v:.2e}" for k, v in sorted(e.items())), flush=True)
        cases[case.name] = {"gain": case.gain, "seed": case.seed, "float32_oracle": sig(ref32), "device": device,
                            "packed_equal_bytes": packed_equal}
    eng.close()
    out["worst_error"] = worst
    out["worst_error_at"] = worst_at
    out["worst_ratio_to_tolerance"] = worst / tc.TOL
    out["worst_float32_oracle_error"] = worst32
    with open(args.out, "w") as f:                    # one case per line
        f.write(json.dumps(out, indent=1)[:-2] + ',\n "cases": {\n')
        f.write(",\n".join("  %s: %s" % (json.dumps(k), json.dumps(r)) for k, r in cases.items()))
        f.write("\n }\n}\n")
    print(f"worst error {worst:.2e} ({worst_at}) = {worst / tc.TOL:.3f} of the tolerance; float32 oracle's worst "
          f"{worst32:.2e} -> {args.out}")
    assert np.isfinite(worst)


if __name__ == "__main__":
    main()
