"""What the bootstrap intervals cost (infer.py --bootstrap R), device against the numpy rule, on three generated sets (the seeded "float"
generator of the tests): 64 typical FSC-147 images (60 ground truths x 120 detections) at R = 200, 1286 images x 100 detections (the
validation split's image count, 20 ground truths each) at R = 1000 and one image of 3731 x 1100 (the data set's largest object count at the
evaluator's maxDets) at R = 1000.

  launch : cdetr_bootstrap_counts (one count column) and cdetr_bootstrap_ap (4 area ranges x 10 thresholds x 101 recall samples, the
           launches of one call added) alone, by HIP events, median of 50.  cdetr_bootstrap_gather, run once per matching, beside them.
  call   : the whole coco_ap.Matching.bootstrap call on the flags cdetr_coco_match left on the device (merged order on the host, its upload,
           the gather, the replicates, the copies back, the six numbers per replicate), wall time, best of --repeats after a warm-up.
  numpy  : the same call on the same flags on the host at R = 10, per replicate (every replicate re-accumulates the split four times).
  pass   : infer.infer with device_detections over tools/eval_batch_time.py's synthetic split (64 seeded-noise images of 384 x 576, seeded
           weights, --eval_batch_size 8, one engine) without and with --bootstrap 1000, best of --repeats after a warm-up pass.
The six numbers of the device route are asserted equal to the numpy rule's on the first 10 replicates.  No threshold is set: nobody had
measured either side before.

usage: python tools/bootstrap_time.py [--out profiles/bootstrap_time.json] [--repeats 5] [--no-pass]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

from counting_detr_amd import bootstrap as bs
from counting_detr_amd import coco_ap as ca
from counting_detr_amd import ops
import coco_ap_cases as cc


def make_set(rng, n, G, D, extent):
    gts, dts = {}, {}
    for i in range(n):
        gts[i], dts[i] = cc.float_image(rng, G, D, extent=extent)
    return gts, dts


def best_of(fn, repeats):
    best, out = None, None
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return out, best


def spread(ms):
    ms = sorted(ms)
    return {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1]}


def time_set(name, gts, dts, R, dev, launches, repeats):
    pack = ca.pack_images(gts, dts)
    N = len(pack["image_ids"])
    rng = np.random.default_rng(7)
    gt_counts = np.array([len(gts[i]) for i in pack["image_ids"]], dtype=np.int32)
    pred_counts = (gt_counts + rng.integers(-6, 7, N)).clip(0).astype(np.int32)
    with torch.cuda.device(dev):
        matching = ca.Matching.launch(pack, dev)
        order, image = bs.prepare(pack["dt_score"], pack["dt_off"])
        i = torch.from_numpy(np.concatenate([order, image]).astype(np.int32)).to(dev)
        P = len(order)
        rec = torch.from_numpy(ca.REC_THRS).to(dev)
        d_gt, d_pred = torch.from_numpy(gt_counts).to(dev), torch.from_numpy(pred_counts).reshape(N, 1).to(dev)
        words = ops.bootstrap_gather(matching.matched, matching.det_ignored, i[:P])             # warm-ups
        ops.bootstrap_counts(d_gt, d_pred, R, 0)
        ops.bootstrap_ap(words, i[P:], matching.npig, rec, R, 0)
        ms_gather, ms_counts, ms_ap = [], [], []
        for _ in range(launches):
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ops.bootstrap_gather(matching.matched, matching.det_ignored, i[:P], events=ev)
            ec = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ops.bootstrap_counts(d_gt, d_pred, R, 0, events=ec)
            pairs = []
            ops.bootstrap_ap(words, i[P:], matching.npig, rec, R, 0, events=pairs)
            torch.cuda.synchronize()
            ms_gather.append(ev[0].elapsed_time(ev[1]))
            ms_counts.append(ec[0].elapsed_time(ec[1]))
            ms_ap.append(sum(e0.elapsed_time(e1) for e0, e1 in pairs))
        matching.bootstrap(R, 0)
        six, call_s = best_of(lambda: matching.bootstrap(R, 0), repeats)
    host = ca.Matching(pack, matching.areas, *matching.host())
    t0 = time.perf_counter()
    want = host.bootstrap(10, 0)
    numpy_s = (time.perf_counter() - t0) / 10
    assert np.array_equal(six[:10], want, equal_nan=True), name
    t0 = time.perf_counter()
    bs.counting(gt_counts, pred_counts, 10, 0)
    numpy_counts_s = (time.perf_counter() - t0) / 10
    row = {"set": name, "images": N, "detections": int(pack["dt_off"][-1]), "replicates": R,
           "bootstrap_counts_launch_ms_hip_events": spread(ms_counts), "bootstrap_ap_launch_ms_hip_events": spread(ms_ap),
           "bootstrap_gather_launch_ms_hip_events": spread(ms_gather), "matching_bootstrap_call_s": call_s,
           "numpy_rule_ap_s_per_replicate": numpy_s, "numpy_rule_counts_s_per_replicate": numpy_counts_s, "six_equal_on_10_replicates": True,
           "AP_interval": [float(v) for v in np.quantile(six[:, 0], [0.025, 0.975])]}
    print(json.dumps(row), flush=True)
    return row


def time_pass(dev, repeats):
    import infer as infer_mod
    from counting_detr_amd import build_model, engine
    from counting_detr_amd.args import default_args
    from oracle.weights import seeded_state_dict
    from tools.eval_batch_time import shift_bias, write_split
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        write_split(os.path.join(tmp, "ds"), 64, 576, 384, np.random.default_rng(2026))
        args = default_args(device=str(dev))
        args.data_path, args.scale_factor, args.split, args.num_workers = os.path.join(tmp, "ds"), 32, "val", 0
        model, criterion, _ = build_model(args)
        model.load_state_dict(seeded_state_dict(), strict=True)
        model.to(dev); criterion.to(dev)
        model.eval()
        args.eval_batch_size = 1
        shift_bias(model, list(infer_mod.eval_loader(args, dev)[0]), dev, 8)
        out_dir = os.path.join(tmp, "out")
        os.makedirs(out_dir)
        args.eval_batch_size = 8
        loader, per_image = infer_mod.eval_loader(args, dev)
        batches = list(loader)
        gt_json = os.path.join(args.data_path, "instances_val.json")
        eng = engine.InferenceEngine(model, 0.5, device=dev)
        for R in (None, 1000):
            times, metrics = [], None
            for _ in range(repeats + 1):                                         # the first pass is the warm-up (graph captures)
                boot = None if R is None else infer_mod.Bootstrap(R, 0, gt_json, dev)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                metrics, _ = infer_mod.infer(model, criterion, batches, dev, out_dir, split="val", device_detections=True, gt_json=gt_json,
                                             per_image=per_image, engine=eng, bootstrap=boot)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            row = {"bootstrap": R, "images": sum(int(b["image"].shape[0]) for b in batches), "pass_s": min(times[1:]),
                   "pass_s_median": sorted(times[1:])[len(times[1:]) // 2], "all_s": times[1:], "warm_up_s": times[0], "MAE": metrics["MAE"],
                   "MAE_interval": None if R is None else [metrics["MAE_lo"], metrics["MAE_hi"]],
                   "AP_interval": None if R is None else [metrics["AP_lo"], metrics["AP_hi"]]}
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bootstrap_time.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--no-pass", action="store_true", help="leave the two device passes out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bootstrap_time: no GPU here -- the device side cannot be measured (nothing is written)")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2025)
    sets = [("64 images of 60 x 120", make_set(rng, 64, 60, 120, 400.0), 200),
            ("1286 images of 20 x 100", make_set(rng, 1286, 20, 100, 400.0), 1000),
            ("1 image of 3731 x 1100", make_set(rng, 1, 3731, 1100, 2500.0), 1000)]
    rows = [time_set(name, gts, dts, R, dev, a.launches, a.repeats) for name, (gts, dts), R in sets]
    passes = None if a.no_pass else time_pass(dev, a.repeats)
    res = {"what": "bootstrap replicates over images (infer.py --bootstrap R): cdetr_bootstrap_counts (one count column), cdetr_bootstrap_ap (4 area "
                   "ranges x 10 IoU thresholds x 101 recall samples; the launches of one call added) and cdetr_bootstrap_gather by HIP events "
                   "(median of %d), the whole coco_ap.Matching.bootstrap call on device flags (wall seconds, best of %d after a warm-up), the numpy "
                   "rule on the same flags at R = 10 (seconds per replicate), and infer.infer with device_detections over 64 synthetic images of "
                   "384 x 576 at --eval_batch_size 8 without and with 1000 replicates (best of %d after a warm-up pass).  No threshold: first "
                   "measurement of either side" % (a.launches, a.repeats, a.repeats),
           "device": torch.cuda.get_device_name(0), "rows": rows, "pass": passes}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
