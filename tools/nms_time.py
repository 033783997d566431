"""cdetr_nms_suppress (infer.py --nms_iou) beside its numpy checker, and what the flag costs a device pass.

  launch = ops.nms_suppress on seeded, clustered detections (the generator of tests/nms_ref.py) by HIP events, median of 50 after a warm-up,
           beside nms.suppress on the same arrays (wall time, best of 3), the two outputs asserted equal, at
             B = 8, Q = 900  with 63 candidates an image (a typical FSC-147 batch: 300 positions x 3 patterns, triplets on one object),
             B = 1, Q = 1728 with 1352 candidates (a crowded image),
             B = 1, Q = 4096 with every query a candidate, once in one cluster (nearly everything goes in the first chunk) and once in 700 loose
                             clusters (about 2400 survivors: the O(n^2) pair tests of one workgroup on one CU);
  pass   = infer.infer with device_detections over tools/eval_batch_time.py's synthetic split (64 seeded-noise images of 384 x 576, seeded
           weights, the class bias shifted so that 8 images keep every query), --eval_batch_size 8, batches collated up front and one
           InferenceEngine kept across the repeats, with and without nms_iou = 0.5: wall time of the whole call, best of --repeats after a
           warm-up pass.

No threshold is set on any of these numbers: none of them existed before.

usage: python tools/nms_time.py [--out profiles/nms_time.json] [--repeats 5]"""
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

import infer as infer_mod
import nms_ref as ref
from counting_detr_amd import build_model, engine, nms, ops
from counting_detr_amd.args import default_args
from tools.eval_batch_time import shift_bias, write_split

SHAPES = (("B = 8, Q = 900, 63 candidates an image", 900, (63,) * 8, 21, 0.08, 0.5),
          ("B = 1, Q = 1728, 1352 candidates", 1728, (1352,), 450, 0.08, 0.5),
          ("B = 1, Q = 4096, all candidates, one cluster", 4096, (4096,), 1, 0.08, 0.5),
          ("B = 1, Q = 4096, all candidates, 700 loose clusters", 4096, (4096,), 700, 0.3, 0.6))


def time_launch(dev, reps=50):
    rows = []
    rng = np.random.default_rng(2027)
    for name, Q, counts, clusters, spread, iou in SHAPES:
        prob, boxes, hw = ref.batch(rng, Q, counts, clusters, spread=spread)
        host_s = []
        for _ in range(3):
            t0 = time.perf_counter()
            want = nms.suppress(prob, boxes, hw, 0.5, iou)
            host_s.append(time.perf_counter() - t0)
        d_prob, d_boxes, d_hw = (torch.from_numpy(a).to(dev) for a in (prob, boxes, hw))
        out, removed = torch.empty_like(d_prob), torch.empty(len(counts), dtype=torch.int32, device=dev)
        for _ in range(3):
            ops.nms_suppress(d_prob, d_boxes, d_hw, 0.5, iou, out=out, removed=removed)
        events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for ev in events:
            ops.nms_suppress(d_prob, d_boxes, d_hw, 0.5, iou, out=out, removed=removed, events=ev)
        torch.cuda.synchronize()
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in events)
        assert ref.same((out.cpu().numpy(), removed.cpu().numpy()), want), name
        row = {"shape": name, "iou": iou, "candidates": int(sum(counts)), "removed": int(want[1].sum()),
               "launch_ms_hip_events": {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1]}, "numpy_checker_ms": min(host_s) * 1e3,
               "outputs_equal": True}
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def time_pass(model, criterion, args, dev, out_dir, repeats):
    args.eval_batch_size = 8
    loader, per_image = infer_mod.eval_loader(args, dev)
    batches = list(loader)
    n = sum(int(b["image"].shape[0]) for b in batches)
    gt_json = os.path.join(args.data_path, "instances_val.json")
    eng = engine.InferenceEngine(model, 0.5, device=dev)
    rows = []
    for iou in (None, 0.5):
        times, metrics = [], None
        for _ in range(repeats + 1):                                             # the first pass is the warm-up (graph captures)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            metrics, _ = infer_mod.infer(model, criterion, batches, dev, out_dir, split="val", device_detections=True, gt_json=gt_json,
                                         per_image=per_image, engine=eng, nms_iou=iou)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        row = {"nms_iou": iou, "images": n, "batches": len(batches), "pass_s": min(times[1:]), "pass_s_median": sorted(times[1:])[len(times[1:]) // 2],
               "all_s": times[1:], "warm_up_s": times[0], "MAE": metrics["MAE"], "AP": metrics["AP"], "nms_removed": metrics.get("nms_removed")}
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nms_time.json"))
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nms_time: needs an MI355X (nothing is measured on the CPU)")
    from oracle.weights import seeded_state_dict
    dev = torch.device("cuda", 0)
    with torch.cuda.device(dev), tempfile.TemporaryDirectory() as tmp:
        launches = time_launch(dev)
        write_split(os.path.join(tmp, "ds"), 64, 576, 384, np.random.default_rng(2026))
        args = default_args(device=str(dev))
        args.data_path, args.scale_factor, args.split, args.num_workers = os.path.join(tmp, "ds"), 32, "val", 0
        model, criterion, _ = build_model(args)
        model.load_state_dict(seeded_state_dict(), strict=True)
        model.to(dev); criterion.to(dev)
        model.eval()
        args.eval_batch_size = 1
        kept, _ = shift_bias(model, list(infer_mod.eval_loader(args, dev)[0]), dev, 8)
        os.makedirs(os.path.join(tmp, "out"))
        passes = time_pass(model, criterion, args, dev, os.path.join(tmp, "out"), a.repeats)
    res = {"what": "cdetr_nms_suppress by HIP events (median of 50 launches after a warm-up) beside the numpy checker nms.suppress (wall, best of 3) "
                   "on seeded clustered detections, outputs asserted equal; and infer.infer with device_detections over 64 synthetic images of "
                   "384 x 576 at --eval_batch_size 8 (seeded weights, %d images keep every query, batches collated up front, one engine across "
                   "the repeats) without and with nms_iou = 0.5: wall time of the whole call, best of %d after a warm-up pass.  Unmeasured "
                   "before; no threshold is set." % (kept, a.repeats),
           "device": torch.cuda.get_device_name(0), "launch": launches, "pass": passes}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
