"""What a threshold sweep costs (infer.py --sweep_thresholds) against what it replaces.

  1  the cdetr_count_sweep call alone by HIP events: B = 8 images, Q = 900 and Q = 1728 queries, T = 1 / 9 / 32 thresholds (median of --calls
     calls after a warm-up; seeded probabilities);
  2  the whole device pass (infer.infer, device_detections=True: forward through the captured graphs, losses, emit, one copy, json dicts, box
     AP) over 64 synthetic 384 x 576 images, without a sweep and with a 9-point one (0.3:0.7:9) -- wall time, best of --repeats after a warm-up;
  3  the same 9 thresholds the only way there was before: 9 separate plain passes, `infer(threshold=t)` each.

The model is the seeded network with its class bias shifted to the median logit (about half the queries kept at 0.5, so the thresholds cut at
different places); the ground truth is the targets the batches carry.  The sweep's row of every threshold is asserted equal to that threshold's
plain pass.  No threshold is set on any of these numbers.

usage: python tools/threshold_sweep_time.py [--out profiles/threshold_sweep_time.json] [--repeats 3] [--calls 50] [--images 64]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import infer as infer_mod
from counting_detr_amd import ops
from counting_detr_amd import threshold_sweep as ts

COUNT_KEYS = ("MAE", "RMSE", "NAE", "SRE")
AP_KEYS = ("AP", "AP50", "AP75", "APs", "APm", "APl")


def kernel_rows(dev, calls):
    rows, rng = [], np.random.default_rng(7)
    for Q in (900, 1728):
        prob = torch.from_numpy(rng.random((8, Q), dtype=np.float32)).to(dev)
        for T in (1, 9, 32):
            sweep = ops.ThresholdSweep(8, np.linspace(0.1, 0.9, T) if T > 1 else [0.5], dev)
            events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
            for k in range(calls + 5):
                sweep.first = 0
                sweep.emit(prob, events=events[k - 5] if k >= 5 else None)
            torch.cuda.synchronize()
            ms = sorted(a.elapsed_time(b) for a, b in events)
            rows.append({"B": 8, "Q": Q, "T": T, "call_us_hip_events": {"median": ms[len(ms) // 2] * 1e3, "min": ms[0] * 1e3, "max": ms[-1] * 1e3}})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def make_split(n, dev, tmp):
    """n batches of one synthetic 384 x 576 image each (the dicts infer.infer reads) + the instances json of their targets."""
    g = torch.Generator().manual_seed(11)
    H, W = 384, 576
    rects = torch.tensor([[.10, .10, .20, .20], [.40, .40, .50, .55], [.70, .20, .80, .30]])
    batches, gt = [], {"images": [], "categories": [{"id": 1, "name": "fg"}], "annotations": []}
    for i in range(n):
        T = 20 + 7 * (i % 9)
        box = torch.cat([torch.rand(T, 2, generator=g) * 0.8 + 0.1, torch.rand(T, 2, generator=g) * 0.10 + 0.02], 1)
        batches.append({"image": torch.randn(1, 3, H, W, generator=g).to(dev), "mask": torch.zeros(1, H, W, dtype=torch.bool, device=dev),
                        "ex_rects": rects[None].to(dev), "targets": [{"boxes": box.to(dev), "labels": torch.zeros(T, dtype=torch.int64, device=dev)}],
                        "orig_size": torch.tensor([[H, W]]), "image_id": torch.tensor([i + 1])})
        gt["images"].append({"id": i + 1, "height": H, "width": W})
        for cx, cy, w, h in (box * torch.tensor([W, H, W, H])).tolist():
            gt["annotations"].append({"id": len(gt["annotations"]) + 1, "image_id": i + 1, "category_id": 1, "iscrowd": 0,
                                      "bbox": [cx - w / 2, cy - h / 2, w, h], "area": w * h})
    gt_json = os.path.join(tmp, "instances_val.json")
    with open(gt_json, "w") as f:
        json.dump(gt, f)
    return batches, gt_json


def best(fn, repeats):
    out, times = None, []
    for _ in range(repeats + 1):                                                # the first run is the warm-up (it captures the forward)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return out, min(times[1:]), times[1:]


def same(a, b, keys):
    return all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in keys)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "threshold_sweep_time.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--images", type=int, default=64)
    a = ap.parse_args()
    from counting_detr_amd import build_model
    from counting_detr_amd.args import default_args
    from counting_detr_amd.engine import InferenceEngine
    from counting_detr_amd.init import seeded_init_
    from counting_detr_amd.misc import NestedTensor
    dev = torch.device("cuda", 0)
    with torch.cuda.device(dev), tempfile.TemporaryDirectory() as tmp:
        kernel = kernel_rows(dev, a.calls)
        model, criterion, _ = build_model(default_args())
        seeded_init_(model)
        model.to(dev).eval()
        criterion.to(dev)
        batches, gt_json = make_split(a.images, dev, tmp)
        with torch.no_grad():
            b0 = batches[0]
            logit = model(NestedTensor(b0["image"], b0["mask"]), rects=b0["ex_rects"])[0]["pred_logits"][0, :, 0]
            for ce in {id(m): m for m in model.transformer.cls_embed}.values():
                ce.bias[0] -= logit.median()
        thresholds = ts.parse_spec("0.3:0.7:9", 0.5)
        engines = {t: InferenceEngine(model, t, device=dev) for t in thresholds}

        def one(t, sweep):
            s = ts.Sweep(thresholds, gt_json) if sweep else None
            m, _ = infer_mod.infer(model, criterion, batches, dev, tmp, split="val", threshold=t, device_detections=True, gt_json=gt_json,
                                   engine=engines[t], sweep=s)
            return m, s
        (plain, _), plain_s, plain_all = best(lambda: one(0.5, False), a.repeats)
        (swept, s), sweep_s, sweep_all = best(lambda: one(0.5, True), a.repeats)
        assert same(plain, swept, plain), (plain, swept)
        separate, sep_s = {}, 0.0
        for t in thresholds:
            (separate[t], _), sec, _ = best(lambda: one(t, False), a.repeats)
            sep_s += sec
        for row in s.report["rows"]:
            assert same(row, separate[row["threshold"]], COUNT_KEYS + AP_KEYS), row
        res = {"what": "cdetr_count_sweep by HIP events (median of %d calls); infer.infer(device_detections=True) over %d synthetic 384 x 576 images, "
                       "seeded model, wall time, best of %d after a warm-up: one plain pass, one pass with a 9-point sweep, and the 9 plain passes "
                       "that the sweep replaces (every row asserted equal to its plain pass)" % (a.calls, a.images, a.repeats),
               "device": torch.cuda.get_device_name(0), "count_sweep_call": kernel, "images": a.images, "thresholds": thresholds,
               "pass_s": {"plain": plain_s, "with_9_point_sweep": sweep_s, "nine_separate_plain_passes": sep_s, "plain_all": plain_all,
                          "with_sweep_all": sweep_all},
               "sweep_over_plain": sweep_s / plain_s, "separate_over_sweep": sep_s / sweep_s,
               "rows": s.report["rows"], "rows_equal_their_plain_passes": True}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["pass_s"]), "wrote", a.out)


if __name__ == "__main__":
    main()
