"""Box-AP evaluation, host path against device path, in one process on three generated sets (the same seeded generators as the tests'
"float" family): 64 typical FSC-147 images (60 ground truths x 120 detections), one crowded image of 1500 x 900, one of 3731 x 1100 (the
data set's largest object count at the evaluator's maxDets).  Host = coco_ap.summarize as it stands (interpreted matcher, four area ranges one
after the other).  Device = coco_ap.summarize(device=...): pack + copies + ONE cdetr_coco_match launch + vectorised tail, wall time around the
whole call after one warm-up, HIP events around the launch alone.  The six numbers of both paths are asserted equal.  Beside them, the
InferenceEngine's time for the same number of 384 x 576 images (bench.inference_leg), to show which of the two dominates an evaluation.

usage: python tools/coco_ap_time.py [--out profiles/coco_ap_time.json] [--repeats 3] [--no-inference]"""
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
import coco_ap_cases as cc


def make_set(rng, n, G, D, extent):
    gts, dts = {}, {}
    for i in range(n):
        gts[i], dts[i] = cc.float_image(rng, G, D, extent=extent)
    return gts, dts


def same(a, b):
    return all(a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])) for k in a)


def device_once(gts, dts, dev):
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pack = ca.pack_images(gts, dts)
    t1 = time.perf_counter()
    matched, ignored, npig = ca.match_on_device(pack, dev, tuple(ca.AREA_RNG), events=ev)
    t2 = time.perf_counter()
    for a in range(len(ca.AREA_RNG)):
        ca.accumulate(pack["dt_score"], matched[a], ignored[a], int(npig[a].sum()))
    t3 = time.perf_counter()
    return {"pack_s": t1 - t0, "copies_and_launch_s": t2 - t1, "tail_s": t3 - t2, "launch_ms_hip_events": ev[0].elapsed_time(ev[1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coco_ap_time.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-inference", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2024)
    sets = [("64 images of 60 x 120", 64, make_set(rng, 64, 60, 120, 400.0)),
            ("1 image of 1500 x 900", 1, make_set(rng, 1, 1500, 900, 1500.0)),
            ("1 image of 3731 x 1100", 1, make_set(rng, 1, 3731, 1100, 2500.0))]
    rows = []
    for name, n_img, (gts, dts) in sets:
        ca.summarize(gts, dts, device=dev)                                        # warm-up: library load, allocator, LDS attribute
        walls, parts = [], []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = ca.summarize(gts, dts, device=dev)
            walls.append(time.perf_counter() - t0)
            parts.append(device_once(gts, dts, dev))
        t0 = time.perf_counter()
        want = ca.summarize(gts, dts)
        host_s = time.perf_counter() - t0
        assert same(want, got), (name, want, got)
        best = parts[int(np.argmin([p["launch_ms_hip_events"] for p in parts]))]
        row = {"set": name, "images": n_img, "ground_truths": sum(len(v) for v in gts.values()), "detections": sum(len(v) for v in dts.values()),
               "host_summarize_s": host_s, "device_summarize_s": min(walls), "device_summarize_s_all": walls, "device_parts": best,
               "speedup": host_s / min(walls), "six_numbers_equal": True, "AP": want["AP"]}
        print(json.dumps(row), flush=True)
        rows.append(row)
    res = {"what": "coco_ap.summarize: host path (interpreted, 4 area ranges in turn) vs device path (pack + one cdetr_coco_match launch for "
                   "4 ranges x 10 thresholds + vectorised tail); wall seconds of the whole call, best of %d after a warm-up" % a.repeats,
           "device": torch.cuda.get_device_name(0), "rows": rows}
    if not a.no_inference:
        import bench
        leg = bench.inference_leg(dev, [(384, 576)], 2, "bf16x3", steps=20)
        rate = leg["shapes"][0]["graph"]["value"]
        res["inference"] = {"what": "engine.InferenceEngine, graph replay, 384 x 576, 2 images per launch", "images_per_s": rate,
                            "seconds_for_the_same_images": {r["set"]: r["images"] / rate for r in rows}}
    assert all(r["device_summarize_s"] < r["host_summarize_s"] for r in rows), "the device path must be faster on every row"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
