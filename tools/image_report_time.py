"""What the per-image evaluation report costs (infer.py --image_report), device against host, on three generated sets (the seeded "float"
generator of the tests): 64 typical FSC-147 images (60 ground truths x 120 detections), one image of 3731 x 1100 (the data set's largest
object count at the evaluator's maxDets) and 1200 images x 100 detections (a whole split's worth of images, 20 ground truths each).

  launch : cdetr_coco_image_stats alone on the flags cdetr_coco_match left on the device, 4 area ranges x 10 thresholds x 3 cuts x 101 recall
           samples, by HIP events, median of 50 launches.
  store  : the whole coco_ap.image_stats_store call on an ops.DetectionStore that holds the set's detections in evaluation order (pack of the
           ground truths, copies, the matching launch, the statistics launch, one copy back), wall time, best of --repeats after a warm-up; the
           first call, which also pays the store's one copy to the host, is reported beside it.
  host   : coco_ap.stats_from_flags (numpy, the checker) on the same flags already on the host -- the matching itself is not in this number.
The statistics of the store route are asserted equal to the host's, the average precisions bit for bit.  No threshold is set: nobody had
measured either side before.

usage: python tools/image_report_time.py [--out profiles/image_report_time.json] [--repeats 3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

from counting_detr_amd import coco_ap as ca
from counting_detr_amd import ops
import coco_ap_cases as cc


def make_set(rng, n, G, D, extent):
    gts, dts = {}, {}
    for i in range(n):
        gts[i], dts[i] = cc.float_image(rng, G, D, extent=extent)
    return gts, dts


def store_of(pack, dev):
    """An ops.DetectionStore holding the pack's detections as cdetr_emit_detections would have left them: evaluation records in evaluation order,
    image k of the store = image k of the pack (no wire records: the report does not read them)."""
    B, per = len(pack["image_ids"]), np.diff(pack["dt_off"])
    store = ops.DetectionStore(B, max(int(per.max()), 1), dev)
    E = int(pack["dt_off"][-1])
    store.eval_boxes[:E].copy_(torch.from_numpy(pack["dt_boxes"]))
    store.eval_area[:E].copy_(torch.from_numpy(pack["dt_area"]))
    store.eval_score[:E].copy_(torch.from_numpy(pack["dt_score"]))
    store.eval_off[:B + 1].copy_(torch.from_numpy(pack["dt_off"]))
    store.counts[:B].copy_(torch.from_numpy(per.astype(np.int32)))
    store.first = B
    return store


def timed(fn, repeats):
    best, out = None, None
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return out, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_report_time.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_report_time: no GPU here -- the device side cannot be measured (nothing is written)")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2025)
    areas, cuts = tuple(ca.AREA_RNG), ca.MAX_DET_CUTS
    sets = [("64 images of 60 x 120", make_set(rng, 64, 60, 120, 400.0)),
            ("1 image of 3731 x 1100", make_set(rng, 1, 3731, 1100, 2500.0)),
            ("1200 images of 20 x 100", make_set(rng, 1200, 20, 100, 400.0))]
    rows = []
    for name, (gts, dts) in sets:
        pack = ca.pack_images(gts, dts)
        B = len(pack["image_ids"])
        with torch.cuda.device(dev):
            matching = ca.Matching.launch(pack, dev, areas)
            keep, (matched, ignored, npig) = (matching.matched, matching.det_ignored, matching.npig), matching.host()
            dt_off = torch.from_numpy(pack["dt_off"]).to(dev)
            d_cuts, rec = torch.tensor(cuts, dtype=torch.int32, device=dev), torch.from_numpy(ca.REC_THRS).to(dev)
            ops.coco_image_stats(keep[0], keep[1], dt_off, keep[2], d_cuts, rec)                      # warm-up
            ms = []
            for _ in range(a.launches):
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ops.coco_image_stats(keep[0], keep[1], dt_off, keep[2], d_cuts, rec, events=ev)
                torch.cuda.synchronize()
                ms.append(ev[0].elapsed_time(ev[1]))
            store = store_of(pack, dev)
            t0 = time.perf_counter()
            first = ca.image_stats_store(gts, store, pack["image_ids"])
            torch.cuda.synchronize()
            first_s = time.perf_counter() - t0
            got, store_s = timed(lambda: ca.image_stats_store(gts, store, pack["image_ids"]), a.repeats)
        t0 = time.perf_counter()
        want = ca.stats_from_flags(matched, ignored, pack["dt_off"], npig, cuts)
        host_s = time.perf_counter() - t0
        for g in (first, got):
            assert np.array_equal(g["tp"], want[0]) and np.array_equal(g["fp"], want[1]), name
            assert np.array_equal(g["ap"].view(np.int64), want[2].view(np.int64)), name
        ar = ca.average_recall(got)
        row = {"set": name, "images": B, "ground_truths": int(pack["gt_off"][-1]), "detections": int(pack["dt_off"][-1]),
               "launch_ms_hip_events_median": float(np.median(ms)), "launch_ms_hip_events_min_max": [float(min(ms)), float(max(ms))],
               "image_stats_store_s": store_s, "image_stats_store_first_call_with_the_stores_copy_s": first_s,
               "host_stats_from_flags_s": host_s, "statistics_equal": True, "AR1100": ar["AR1100"]}
        print(json.dumps(row), flush=True)
        rows.append(row)
    res = {"what": "the per-image evaluation statistics (infer.py --image_report): cdetr_coco_image_stats by HIP events (median of %d launches; 4 "
                   "area ranges x 10 IoU thresholds x 3 cuts x 101 recall samples), the whole coco_ap.image_stats_store call (ground-truth pack, "
                   "copies, the matching launch, the statistics launch, one copy back; wall seconds, best of %d after a first call) and "
                   "coco_ap.stats_from_flags in numpy on the same flags (the matching not included).  No threshold: first measurement of "
                   "either side" % (a.launches, a.repeats),
           "device": torch.cuda.get_device_name(0), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
