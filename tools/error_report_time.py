"""What the error breakdown costs (infer.py --error_report), device against host, on the three generated sets tools/image_report_time.py uses
(the seeded "float" generator of the tests): 64 typical FSC-147 images (60 ground truths x 120 detections), one image of 3731 x 1100 (the
data set's largest object count at the evaluator's maxDets) and 1200 images x 100 detections (a whole split's worth, 20 ground truths each).

  launch : cdetr_coco_errors alone on the packed boxes already on the device, by HIP events, median of 50 launches.
  store  : the whole coco_ap.match_store(...).errors() call on an ops.DetectionStore that holds the set's detections in evaluation order
           (pack of the ground truths, copies, the matching launch every reader shares, the breakdown's launch, one copy back), wall time,
           best of --repeats after a first call, which also pays the store's one copy to the host and is reported beside it.
  host   : error_report.classify (numpy, the rule and the checker) on the same pack.
The codes of the store route are asserted equal to the rule's, the IoUs bit for bit.  No threshold is set on any time.

usage: python tools/error_report_time.py [--out profiles/error_report_time.json] [--repeats 3]"""
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
from counting_detr_amd import error_report as er
from counting_detr_amd import ops
from image_report_time import make_set, store_of, timed

KEYS = ("dt_code", "dt_gt", "dt_iou", "gt_code", "gt_dt", "gt_iou", "counts")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "error_report_time.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("error_report_time: no GPU here -- the device side cannot be measured (nothing is written)")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2025)
    sets = [("64 images of 60 x 120", make_set(rng, 64, 60, 120, 400.0)),
            ("1 image of 3731 x 1100", make_set(rng, 1, 3731, 1100, 2500.0)),
            ("1200 images of 20 x 100", make_set(rng, 1200, 20, 100, 400.0))]
    rows = []
    for name, (gts, dts) in sets:
        pack = ca.pack_images(gts, dts)
        B = len(pack["image_ids"])
        with torch.cuda.device(dev):
            up = lambda k, t=None: torch.from_numpy(np.ascontiguousarray(pack[k] if t is None else pack[k].astype(t))).to(dev)   # noqa: E731
            args = (up("gt_boxes").reshape(-1), up("gt_area"), up("gt_ignore"), up("gt_off", np.int32), up("dt_boxes").reshape(-1), up("dt_area"),
                    up("dt_off", np.int32), int(pack["g_max"]), er.IOU_FG, er.IOU_BG, ca.AREA_RNG["all"])
            ops.coco_errors(*args)                                                                    # warm-up
            ms = []
            for _ in range(a.launches):
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ops.coco_errors(*args, events=ev)
                torch.cuda.synchronize()
                ms.append(ev[0].elapsed_time(ev[1]))
            store = store_of(pack, dev)
            t0 = time.perf_counter()
            first = ca.match_store(gts, store, pack["image_ids"]).errors()
            torch.cuda.synchronize()
            first_s = time.perf_counter() - t0
            got, store_s = timed(lambda: ca.match_store(gts, store, pack["image_ids"]).errors(), a.repeats)
        t0 = time.perf_counter()
        want = er.classify(pack)
        host_s = time.perf_counter() - t0
        for g in (first, got):
            for k in KEYS:
                x, y = np.ascontiguousarray(g[k]), np.ascontiguousarray(want[k])
                assert x.dtype == y.dtype and np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x, y.view(np.int64) if y.dtype == np.float64 else y), (name, k)
        row = {"set": name, "images": B, "ground_truths": int(pack["gt_off"][-1]), "detections": int(pack["dt_off"][-1]),
               "launch_ms_hip_events_median": float(np.median(ms)), "launch_ms_hip_events_min_max": [float(min(ms)), float(max(ms))],
               "match_store_errors_s": store_s, "match_store_errors_first_call_with_the_stores_copy_s": first_s,
               "host_classify_s": host_s, "codes_equal": True, "totals": dict(zip(er.COUNT_KEYS, want["counts"].sum(axis=0).tolist()))}
        print(json.dumps(row), flush=True)
        rows.append(row)
    res = {"what": "the error breakdown (infer.py --error_report): cdetr_coco_errors by HIP events (median of %d launches), the whole "
                   "coco_ap.match_store(...).errors() call (ground-truth pack, copies, the shared matching launch, the breakdown's launch, one copy "
                   "back; wall seconds, best of %d after a first call) and error_report.classify in numpy on the same pack.  No threshold on any "
                   "time" % (a.launches, a.repeats),
           "device": torch.cuda.get_device_name(0), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
