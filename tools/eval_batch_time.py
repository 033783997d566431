"""The stage-2 evaluation loop (infer.infer) at --eval_batch_size 1, 4, 8 and 16, host path and --device_detections path, and the launch behind
the per-image losses (cdetr_criterion_eval) beside B launches of the training kernel (cdetr_criterion_fwd on each image alone).

  split   = 64 seeded-noise PNGs of 384 x 576 (one size bucket) written as an FSC-147 validation split, 20 ... 200 targets per image; the model
            carries oracle.weights.seeded_state_dict with the class bias shifted into the gap under the 8 images with the highest logits (the
            seeded network gives all queries of an image nearly one logit: those 8 images keep every query, the others none);
  loop    = infer.infer over the split's batches, collated ONCE up front (decode and resize stay outside the window) and with ONE
            InferenceEngine kept across the repeats (its graphs are captured by the warm-up pass: a split of thousands of images replays);
            batch size 1 is the parent commit's loop unchanged (the batched criterion on one image), larger sizes take
            SetCriterion.per_image.  Wall time of the whole call (it ends in blocking copies), best of --repeats after the warm-up pass;
  launch  = Q = 576 queries, seeded predictions, 20 ... 200 targets per image, B = 1, 8, 16: ops.criterion_eval by HIP events beside B calls of ops.CriterionFn on one
            image each (events around the B calls; the interpreter's launch overhead is inside both), alternating over 50 rounds after a warm-up.  The match is outside both windows.

No threshold is set: none of these numbers existed before.

usage: python tools/eval_batch_time.py [--out profiles/eval_batch_time.json] [--repeats 7]"""
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
from counting_detr_amd import build_model, engine, ops
from counting_detr_amd.args import default_args
from counting_detr_amd.misc import NestedTensor

SIZES = (1, 4, 8, 16)


def write_split(root, n, w, h, rng):
    from PIL import Image
    os.makedirs(os.path.join(root, "images_384_VarV2"))
    anno, images, annotations, names = {}, [], [], []
    for k in range(n):
        name = f"{k + 1}.png"
        names.append(name)
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(root, "images_384_VarV2", name))
        t = int(rng.integers(20, 201))
        wh = rng.uniform(8.0, 40.0, (t, 2))
        xy = rng.uniform(1.0, [w - 42.0, h - 42.0], (t, 2))
        images.append({"id": k + 1, "file_name": name, "width": w, "height": h})
        for (x, y), (bw, bh) in zip(xy.tolist(), wh.tolist()):
            annotations.append({"id": len(annotations) + 1, "image_id": k + 1, "bbox": [x, y, bw, bh], "category_id": 1, "area": bw * bh, "iscrowd": 0})
        ex = [[[x, y], [x, y + bh], [x + bw, y + bh], [x + bw, y]] for (x, y), (bw, bh) in zip(xy[:3].tolist(), wh[:3].tolist())]
        anno[name] = {"box_examples_coordinates": ex, "points": (xy + wh / 2).tolist(), "H": h, "W": w}
    for fn, obj in (("annotation_FSC147_384.json", anno), ("Train_Test_Val_FSC_147.json", {"train": [], "val": names, "test": []}),
                    ("instances_val.json", {"images": images, "annotations": annotations, "categories": [{"id": 1, "name": "fg"}]})):
        with open(os.path.join(root, fn), "w") as f:
            json.dump(obj, f)


def shift_bias(model, batches, dev, keep_images):
    """Class bias into the gap under the `keep_images` images with the highest logits -> (kept images, width of the gap)."""
    with torch.no_grad():
        logit = torch.cat([model(NestedTensor(b["image"].to(dev), b["mask"].to(dev)), rects=b["ex_rects"].to(dev))[0]["pred_logits"][..., 0]
                           for b in batches]).double().cpu()
        lo, hi = logit.min(1).values, logit.max(1).values
        order = torch.argsort(lo)
        n = len(order)
        cuts = [(float(lo[order[n - c]]) - float(hi[order[:n - c]].max()), c) for c in range(max(keep_images // 2, 1), min(2 * keep_images, n - 1) + 1)]
        gap, keep_images = max(cuts)                                             # the widest gap among the cuts around the wanted one
        if gap <= 0.0:
            raise RuntimeError("eval_batch_time: no gap between the images' logits near this cut")
        k = n - keep_images
        below, above = float(hi[order[:k]].max()), float(lo[order[k]])
        for ce in {id(m): m for m in model.transformer.cls_embed}.values():
            ce.bias[0] -= 0.5 * (below + above)
    return keep_images, above - below


def time_loops(model, criterion, args, dev, out_dir, repeats):
    rows, engines = [], {}
    real_engine = engine.InferenceEngine

    def cached_engine(m, threshold=0.5, **kw):                                   # one engine (and its captured graphs) per configuration, across the repeats
        key = engines["key"]
        if key not in engines:
            engines[key] = real_engine(m, threshold, **kw)
        return engines[key]
    gt_json = os.path.join(args.data_path, "instances_val.json")
    first = None
    engine.InferenceEngine = cached_engine
    try:
        for B in SIZES:
            args.eval_batch_size = B
            loader, per_image = infer_mod.eval_loader(args, dev)
            batches = list(loader)
            n = sum(int(b["image"].shape[0]) for b in batches)
            for path, flag in (("host", False), ("device_detections", True)):
                engines["key"] = (B, path)
                times, metrics = [], None
                for _ in range(repeats + 1):                                     # the first pass is the warm-up (graph captures, lazily built tables)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    metrics, _ = infer_mod.infer(model, criterion, batches, dev, out_dir, split="val", device_detections=flag,
                                                 gt_json=gt_json if flag else None, per_image=per_image)
                    torch.cuda.synchronize()
                    times.append(time.perf_counter() - t0)
                if first is None:
                    first = metrics
                loss_dev = max(abs(metrics[k] - first[k]) / max(abs(first[k]), 1e-12) for k in first if k.startswith("loss_"))
                row = {"eval_batch_size": B, "path": path, "images": n, "batches": len(batches), "images_per_s": n / min(times[1:]),
                       "images_per_s_median": n / sorted(times[1:])[len(times[1:]) // 2], "images_per_s_worst": n / max(times[1:]), "all_s": times[1:],
                       "warm_up_s": times[0], "per_image_losses": per_image, "MAE": metrics["MAE"], "MAE_equals_batch_1": metrics["MAE"] == first["MAE"],
                       "largest_relative_loss_difference_to_batch_1": loss_dev}
                print(json.dumps(row), flush=True)
                rows.append(row)
                del engines[(B, path)]
    finally:
        engine.InferenceEngine = real_engine
    return rows


def time_launch(dev, Q=576, reps=50):
    from counting_detr_amd.anchor_detr import SetCriterion
    from counting_detr_amd.matcher import OriginalHungarianMatcher
    crit = SetCriterion(1, OriginalHungarianMatcher(2, 5, 2), {"loss_ce": 2, "loss_bbox": 5, "loss_giou": 2, "loss_variance": 2},
                        ["labels", "boxes", "cardinality", "vars"], focal_alpha=0.25)
    g = torch.Generator().manual_seed(7)
    rows = []
    for B in (1, 8, 16):
        outs = {"pred_logits": torch.randn(B, Q, 2, generator=g).to(dev), "pred_vars": (torch.rand(B, Q, 2, generator=g) * 0.5 + 0.05).to(dev),
                "pred_boxes": torch.cat([torch.rand(B, Q, 2, generator=g) * 0.8 + 0.1, torch.rand(B, Q, 2, generator=g) * 0.1 + 0.02], 2).to(dev)}
        sizes = [int(t) for t in torch.randint(20, 201, (B,), generator=g)]
        tg = [{"boxes": torch.cat([torch.rand(t, 2, generator=g) * 0.8 + 0.1, torch.rand(t, 2, generator=g) * 0.1 + 0.02], 1).to(dev),
               "labels": torch.zeros(t, dtype=torch.int64, device=dev)} for t in sizes]
        crit.per_image(outs, tg)
        idx_i, idx_j, plan = crit.last_match
        tb, tl = torch.cat([t["boxes"] for t in tg]), torch.cat([t["labels"] for t in tg])
        w6 = crit._weights6(dev, None)
        alone = []
        for b in range(B):                                                       # each image as a batch of one: its own plan, indices and normaliser
            p1 = ops.MatchPlan((sizes[b],), Q, dev)
            alone.append(({k: v[b:b + 1].contiguous() for k, v in outs.items()}, tg[b], p1, idx_i[b:b + 1, :p1.Mmax].contiguous(),
                          idx_j[b:b + 1, :p1.Mmax].contiguous(), torch.full((1,), float(max(sizes[b], 1)), device=dev)))

        def new():
            return ops.criterion_eval(outs["pred_logits"], outs["pred_boxes"], outs["pred_vars"], tb, tl, plan, idx_i, idx_j, 1, 0.25, w6)

        def old():
            return [ops.CriterionFn.apply(o["pred_logits"], o["pred_boxes"], o["pred_vars"], t["boxes"], t["labels"], p1, ii, jj, nb, 1, 0.25, w6)[0]
                    for o, t, p1, ii, jj, nb in alone]
        rows_new, vec_old = new(), torch.stack(old())
        worst = float(((rows_new[:, :6] - vec_old).abs() / vec_old.abs().clamp_min(1e-6)).max())
        fns = (("criterion_eval_one_launch", new), ("criterion_fwd_B_launches", old))
        for _ in range(5):
            for _, fn in fns:
                fn()
        ev = {name: [] for name, _ in fns}
        for _ in range(reps):                                                    # the two alternate inside one window
            for name, fn in fns:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                ev[name].append((e0, e1))
        torch.cuda.synchronize()
        ms = {}
        for name, pairs in ev.items():
            t = sorted(e0.elapsed_time(e1) for e0, e1 in pairs)
            ms[name] = {"median_ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1]}
        row = {"B": B, "Q": Q, "targets": sizes, "hip_events": ms, "largest_relative_difference_of_the_six_scalars": worst}
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_batch_time.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--size", type=int, nargs=2, default=[384, 576], help="height width")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_batch_time: needs an MI355X (nothing is measured on the CPU)")
    from oracle.weights import seeded_state_dict
    dev = torch.device("cuda", 0)
    with torch.cuda.device(dev), tempfile.TemporaryDirectory() as tmp:
        write_split(os.path.join(tmp, "ds"), a.images, a.size[1], a.size[0], np.random.default_rng(2026))
        args = default_args(device=str(dev))
        args.data_path, args.scale_factor, args.split, args.num_workers = os.path.join(tmp, "ds"), 32, "val", 0
        model, criterion, _ = build_model(args)
        model.load_state_dict(seeded_state_dict(), strict=True)
        model.to(dev); criterion.to(dev)
        model.eval()
        args.eval_batch_size = 1
        kept, gap = shift_bias(model, list(infer_mod.eval_loader(args, dev)[0]), dev, max(a.images // 8, 1))
        os.makedirs(os.path.join(tmp, "out"))
        loops = time_loops(model, criterion, args, dev, os.path.join(tmp, "out"), a.repeats)
        launches = time_launch(dev)
    res = {"what": "infer.infer over a synthetic validation split (seeded-noise images of one size, seeded weights, batches collated up front, one "
                   "InferenceEngine kept across the repeats) at --eval_batch_size 1 / 4 / 8 / 16, host loop and --device_detections loop: images/s of "
                   "the whole call, best of %d after a warm-up pass; batch size 1 is the parent commit's loop.  cdetr_criterion_eval (one launch "
                   "for B images) beside B launches of cdetr_criterion_fwd by HIP events, Q = 576, the two alternating in one window of 50 rounds; "
                   "the events enclose the Python calls, so both figures include the interpreter's launch overhead, which dominates the B calls.  "
                   "images_per_s is the best pass, images_per_s_median / _worst give the spread (all_s: every pass)." % a.repeats,
           "device": torch.cuda.get_device_name(0), "images": a.images, "image_hw": a.size, "images_keeping_all_queries": kept,
           "logit_gap_at_the_threshold": gap, "loops": loops, "launch": launches}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
