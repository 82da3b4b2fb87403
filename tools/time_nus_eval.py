"""Times the nuScenes detection metric on the device per stage and end to end at the full synthetic val size
(6 019 samples, ~40 GT and up to 500 predictions each; tests/test_nus_eval_gpu.py:synthetic_val), and the numpy
restatement of the devkit (tests/nus_eval_reference.py) on the same data on the host.  DESIGN §2.12 quotes the output.

    python tools/time_nus_eval.py [--samples 6019] [--repeat 3] [--no-oracle]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cvpr2023-unidistill_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=6019)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--no-oracle", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_nus_eval.py needs a GPU")
    import nus_eval_reference as R
    import test_nus_eval_gpu as T
    from unidistill_amd import _lib
    dev = torch.device("cuda:0")
    data = T.synthetic_val(S=args.samples)
    P, G = int(data["pred_count"].sum()), len(data["gt"]["cls"])
    # the eval loop's batches, already on the device (the eval forward leaves pred_dicts there)
    batches = [(ids, [{k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in pd.items()} for pd in pds],
                torch.from_numpy(data["l2g"][ids]).to(dev)) for ids, pds in T._batches(data, 8)]
    stages = ["nus_eval.k_nus_pred_prep", "nus_eval.k_nus_match", "nus_eval.sort", "nus_eval.scans",
              "nus_eval.k_nus_curves"]
    runs = []
    for r in range(args.repeat + 1):                  # run 0 warms up
        ev = T._make_eval(data["gt"], data["ego"], dev)
        torch.cuda.synchronize()
        _lib.prof_enable(False)
        t0 = time.perf_counter()
        for ids, pds, l2g in batches:
            ev.add_batch(ids, pds, l2g)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        summary = ev.compute()                        # ends in the device -> host copy of the curves
        t2 = time.perf_counter()
        # per-stage kernel times in a separate pass (events on the stream)
        ev.reset()
        _lib.prof_enable(True)
        for s in stages:
            _lib.prof_read(s)
        for ids, pds, l2g in batches:
            ev.add_batch(ids, pds, l2g)
        ev.compute()
        st = {s.split(".")[1]: _lib.prof_read(s)[0] for s in stages}
        _lib.prof_enable(False)
        if r:
            runs.append({"add_batch_ms": (t1 - t0) * 1e3, "compute_ms": (t2 - t1) * 1e3, "stages_ms": st})
    out = {"samples": args.samples, "predictions": P, "gt": G, "batches": len(batches),
           "device_runs": runs, "mean_ap": summary["mean_ap"], "nd_score": summary["nd_score"]}
    if not args.no_oracle:
        t0 = time.perf_counter()
        pred = T._oracle_preds(data)
        ref, _, _ = R.evaluate(data["gt"], pred, data["ego"])
        out["oracle_host_s"] = time.perf_counter() - t0
        out["oracle_nd_score"] = ref["nd_score"]
        out["abs_diff_nd"] = abs(ref["nd_score"] - summary["nd_score"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
