"""Measure the per-wavefront board net of the persistent SCS route on the cases of tests/wavenet_cases.py and write
profiles/wavenet_edge_errors.json: per admitted case the worst probability and value error of the recorded leaves
against the float64 oracle, the float32 oracle's own error on the same leaves, the leaf count and the admission verdict
(the host restatement's, which the play confirms); per refusal case the library's own message.

    python scripts/wavenet_edge_errors.py [--out profiles/wavenet_edge_errors.json]

Needs a GPU.  The file is only worth committing from a real device run."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    import torch
    import wavenet_cases as wc
    import test_gpu_wavenet_edges as t
    from nuzero_amd._lib import NzError
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "wavenet_edge_errors.json"))
    args = ap.parse_args()
    out = {"tolerance": wc.TOL, "reference": "oracle/net.py, dtype=float64",
           "measures": {"prob": "max |d probability|", "value": "max |d value|"},
           "leaves": f"every leaf evaluation of {t.G} games at {t.SIMS} simulations a move on the persistent route",
           "device": torch.cuda.get_device_name(0), "cases": {}, "refusals": {}}
    worst = 0.0
    for case in wc.ADMITTED:
        comp = wc.compile_case(case)
        r, recs, planes = t.play_recorded(case)
        x, p, v = t.leaf_arrays(recs, planes)
        dev, ref32 = t.float64_errors(case, x, p, v)
        if case.precision == "float32":
            worst = max(worst, dev["prob"], dev["value"])
        out["cases"][case.name] = {
            "fixture": case.fixture, "precision": case.precision, "gain": case.gain, "reaches": case.reaches,
            "verdict": comp.verdict, "lds_bytes": comp.lds_bytes, "workgroup_lds_bytes": comp.workgroup_bytes,
            "fused16_form": comp.fused16, "leaves": len(x), "moves": int(r["lengths"].sum()),
            "device": dev, "float32_oracle": ref32}
        print(f"{case.name:18s} {comp.verdict:6s} leaves {len(x):5d} prob {dev['prob']:.2e} value {dev['value']:.2e} "
              f"(float32 oracle: prob {ref32['prob']:.2e} value {ref32['value']:.2e})", flush=True)
    for case in wc.REFUSED:
        comp = wc.compile_case(case)
        sp, net = t._selfplay(case), t._net(case, t.G)
        sp.persistent(1)
        try:
            sp.play_native(net, t._seeds(case), max_moves=1)
            message = None
        except NzError as e:
            message = str(e)
        sp.close(); net.close()
        out["refusals"][case.name] = {"fixture": case.fixture, "width": case.width, "gate": comp.gate,
                                      "lds_bytes": comp.lds_bytes, "workgroup_lds_bytes": comp.workgroup_bytes,
                                      "message": message}
        print(f"{case.name:18s} {comp.gate:14s} {message}", flush=True)
    out["worst_float32_error"] = worst
    out["worst_ratio_to_tolerance"] = worst / wc.TOL
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"worst float32-case error {worst:.2e} = {worst / wc.TOL:.3f} of the tolerance -> {args.out}")


if __name__ == "__main__":
    main()
