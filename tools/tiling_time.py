"""The three launches of tiled inference (infer.py --tiles) beside their numpy checker, and what the flag costs a device pass.

  launch = ops.tile_images, ops.exemplar_group_fwd and ops.tile_stitch by HIP events, median of 50 after a warm-up, beside tiling.tile_images /
           group_feature / stitch on the same arrays (wall time, best of 3), the outputs asserted equal, for
             a 384 x 576 image at 2x2, margin 32, scale 1 and scale 2,
             an 800 x 1344 image (the 800 x 1333 class at a multiple of 32) at 2x2, margin 32, scale 1,
           with Q = 900 queries a tile and the layer-4 map of the padded tile (stride 16, 2048 channels);
  pass   = infer.infer with device_detections over a synthetic split (32 seeded-noise images of 384 x 576, seeded weights, the class bias shifted
           to the first image's median logit), batches collated up front and one InferenceEngine kept across the repeats: untiled, --tiles 2x2,
           and --tiles 2x2 --tile_below P with P the median exemplar size of the split: wall time of the whole call, best of --repeats after a
           warm-up pass.

No threshold is set on any of these numbers: none of them existed before.  What tiling does to MAE on trained weights is NOT measured here.

usage: python tools/tiling_time.py [--out profiles/tiling_time.json] [--repeats 3]"""
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
from counting_detr_amd import build_model, engine, ops, tiling
from counting_detr_amd.args import default_args
from counting_detr_amd.misc import NestedTensor
from tools.eval_batch_time import write_split

SHAPES = (("384 x 576 at 2x2, scale 1", 384, 576, 1), ("384 x 576 at 2x2, scale 2", 384, 576, 2), ("800 x 1344 at 2x2, scale 1", 800, 1344, 1))
Q, C, K = 900, 2048, 3


def _timed(fn, reps=50):
    for _ in range(3):
        fn(None)
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for ev in events:
        fn(ev)
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in events)
    return {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1]}


def _best(fn, n=3):
    out, best = None, None
    for _ in range(n):
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return out, best * 1e3


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def time_launch(dev):
    rows = []
    rng = np.random.default_rng(2028)
    for name, H, W, S in SHAPES:
        plan = tiling.Plan(H, W, 2, 2, 32, S)
        T = plan.T
        image = rng.standard_normal((3, H, W)).astype(np.float32)
        (want_t, want_m), cut_ms = _best(lambda: tiling.tile_images(image, plan))
        d_image, d_rec, d_coef = (torch.from_numpy(a).to(dev) for a in (image, plan.records, plan.coef))
        tiles = torch.empty((T, 3, plan.Hm, plan.Wm), dtype=torch.float32, device=dev)
        mask = torch.empty((T, plan.Hm, plan.Wm), dtype=torch.bool, device=dev)
        cut = _timed(lambda ev: ops.tile_images(d_image, d_rec, plan.Hm, plan.Wm, tiles=tiles, mask=mask, events=ev))
        assert _bits_equal(tiles.cpu().numpy(), want_t) and np.array_equal(mask.cpu().numpy(), want_m), name
        # the layer-4 map of the padded tile batch and the image's three exemplars, each in the tile that owns it
        h, w = -(-plan.Hm // 16), -(-plan.Wm // 16)
        x = rng.standard_normal((T, h * w, C)).astype(np.float32)
        c, s = rng.uniform(0.1, 0.9, (K, 2)), rng.uniform(0.02, 0.08, (K, 2))
        rects = tiling.tile_rects(np.concatenate([c - s / 2, c + s / 2], 1).astype(np.float32), plan)
        extent = np.array([[-(-(y1 - y0) * S // 16), -(-(x1 - x0) * S // 16)] for x0, y0, x1, y1 in plan.boxes], dtype=np.float32)
        (want_pf, want_idx), pool_ms = _best(lambda: tiling.group_feature(x, rects, extent, h, w, T))
        d_x, d_rects, d_extent = torch.from_numpy(x).to(dev).view(T, h, w, C), torch.from_numpy(rects).to(dev), torch.from_numpy(extent).to(dev)
        got = {}
        pool = _timed(lambda ev: got.update(out=ops.exemplar_group_fwd(d_x, d_rects, d_extent, T, events=ev)))
        assert _bits_equal(got["out"][0].cpu().numpy(), want_pf) and np.array_equal(got["out"][1].cpu().numpy(), want_idx), name
        prob = rng.uniform(0, 1, (T, Q)).astype(np.float32)
        boxes, points = rng.uniform(0, 1, (T, Q, 4)).astype(np.float32), rng.uniform(0, 1, (T, Q, 2)).astype(np.float32)
        want, stitch_ms = _best(lambda: tiling.stitch(prob, boxes, points, plan))
        d_prob, d_boxes, d_points = (torch.from_numpy(a).to(dev) for a in (prob, boxes, points))
        out = tuple(torch.empty((1, plan.slots * Q) + tail, dtype=torch.float32, device=dev) for tail in ((), (4,), (2,)))
        stitch = _timed(lambda ev: ops.tile_stitch(d_prob, d_boxes, d_points, d_coef, plan.slots, H, W, out=out, events=ev))
        assert all(_bits_equal(o[0].cpu().numpy(), wnt) for o, wnt in zip(out, want)), name
        row = {"shape": name, "tiles": T, "padded_tile": [plan.Hm, plan.Wm], "kept_queries": int((~np.isnan(want[0])).sum()), "virtual_queries": plan.slots * Q,
               "tile_images_ms_hip_events": cut, "tile_images_numpy_ms": cut_ms, "tile_images_bytes": int(image.nbytes + tiles.numel() * 4 + mask.numel()),
               "exemplar_group_fwd_ms_hip_events": pool, "group_feature_numpy_ms": pool_ms,
               "tile_stitch_ms_hip_events": stitch, "stitch_numpy_ms": stitch_ms, "outputs_equal": True}
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def time_pass(model, criterion, args, dev, out_dir, repeats, below):
    loader, per_image = infer_mod.eval_loader(args, dev)
    batches = list(loader)
    n = sum(int(b["image"].shape[0]) for b in batches)
    gt_json = os.path.join(args.data_path, "instances_val.json")
    eng = engine.InferenceEngine(model, 0.5, device=dev)
    rows = []
    for name, tiles in (("untiled", None), ("--tiles 2x2", tiling.Tiling(2, 2)), (f"--tiles 2x2 --tile_below {below:.2f}", tiling.Tiling(2, 2, below=below))):
        times, metrics = [], None
        grouped = eng.stats.get("grouped_calls", 0)
        for _ in range(repeats + 1):                                             # the first pass is the warm-up (graph captures)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            metrics, _ = infer_mod.infer(model, criterion, batches, dev, out_dir, split="val", device_detections=True, gt_json=gt_json,
                                         per_image=per_image, engine=eng, tiles=tiles)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        row = {"run": name, "images": n, "tiled_images": (eng.stats.get("grouped_calls", 0) - grouped) // (repeats + 1), "pass_s": min(times[1:]),
               "pass_s_median": sorted(times[1:])[len(times[1:]) // 2], "all_s": times[1:], "warm_up_s": times[0], "MAE": metrics["MAE"],
               "AP": metrics["AP"]}
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiling_time.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--images", type=int, default=32)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tiling_time: needs an MI355X (nothing is measured on the CPU)")
    from oracle.weights import seeded_state_dict
    dev = torch.device("cuda", 0)
    with torch.cuda.device(dev), tempfile.TemporaryDirectory() as tmp:
        launches = time_launch(dev)
        write_split(os.path.join(tmp, "ds"), a.images, 576, 384, np.random.default_rng(2026))
        args = default_args(device=str(dev))
        args.data_path, args.scale_factor, args.split, args.num_workers, args.eval_batch_size = os.path.join(tmp, "ds"), 32, "val", 0, 1
        model, criterion, _ = build_model(args)
        model.load_state_dict(seeded_state_dict(), strict=True)
        model.to(dev); criterion.to(dev)
        model.eval()
        batches = list(infer_mod.eval_loader(args, dev)[0])
        sizes = [tiling.exemplar_size(b["ex_rects"][0].numpy(), b["image"].shape[2], b["image"].shape[3]) for b in batches]
        below = float(np.median(sizes))
        with torch.no_grad():
            b = batches[0]
            logit = model(NestedTensor(b["image"].to(dev), b["mask"].to(dev)), rects=b["ex_rects"].to(dev))[0]["pred_logits"][0, :, 0]
            for ce in {id(m): m for m in model.transformer.cls_embed}.values():
                ce.bias[0] -= logit.median()
        os.makedirs(os.path.join(tmp, "out"))
        passes = time_pass(model, criterion, args, dev, os.path.join(tmp, "out"), a.repeats, below)
    res = {"what": "ops.tile_images / exemplar_group_fwd / tile_stitch by HIP events (median of 50 launches after a warm-up) beside the numpy rule of "
                   "counting_detr_amd/tiling.py (wall, best of 3) on seeded arrays, outputs asserted equal; and infer.infer with device_detections "
                   "over %d synthetic images of 384 x 576 (seeded weights, 300 queries, batches collated up front, one engine across the repeats) "
                   "untiled, at 2x2 and at 2x2 with tile_below = the split's median exemplar size: wall time of the whole call, best of %d after a "
                   "warm-up pass.  Unmeasured before; no threshold is set.  The accuracy effect of tiling on trained weights is not measured." %
                   (a.images, a.repeats),
           "device": torch.cuda.get_device_name(0), "launch": launches, "pass": passes}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
