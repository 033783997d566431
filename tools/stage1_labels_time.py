"""The work between the stage-1 forward and pseudo_bbox_<split>.json / its score, host path against device path
(main_stage1.py --device_labels), on generated forward outputs.  No model runs: a stub hands seeded device tensors out as `pred_wh`, the
images are 8 x 8 placeholders; original sizes are 384 x 576 (h x w).

  host   = stage1.write_pseudo_labels as it stands by default (the parent commit's loop): per batch two .cpu() copies, then one dict per dot;
  device = write_pseudo_labels(device_labels=True): per batch one cdetr_emit_pseudo_labels call, after the last batch ONE copy of the store and
           the annotation dicts built from its wire array.

  (1) one batch of B = 8 images with 7 / 64 / 300 / 900 points each through either path (the whole call: store, loop, dicts, json file), and
      the emit call alone by HIP events and by the host time it takes to enqueue;
  (2) a label pass over 32 images (4 ragged batches of 8, 7 .. 900 points per image), both ways;
  (3) the scoring call on that pass: stage1.score_pseudo_labels through the annotation dicts (coco_ap.summarize(device=)) against
      score_pseudo_labels(store=) (coco_ap.summarize_store straight from device memory).
Wall time, best of --repeats after a warm-up, every window ends in a device synchronise or a blocking copy.  Both paths' files are asserted
byte-equal and the scores equal.  No threshold is set: none of this had been measured before.

usage: python tools/stage1_labels_time.py [--out profiles/stage1_labels_time.json] [--repeats 5]"""
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

from counting_detr_amd import ops, stage1

W, H = 576, 384


class Stub(torch.nn.Module):
    """The forward's place in the loop: returns the batch's prepared pred_wh (batches are recognised by their points tensor)."""

    def __init__(self):
        super().__init__()
        self.on_device = {}

    def forward(self, image, points, counts=None):
        return {"pred_wh": self.on_device[points.data_ptr()]}


def make_batches(rng, dev, counts_per_batch, first_id=1):
    """Ragged batches as data.collate_stage1_ragged yields them (host tensors) + per batch the device pred_wh; ground truth near the boxes."""
    batches, gt, im_id = [], {"images": [], "categories": [{"id": 1, "name": "fg"}], "annotations": []}, first_id
    for counts in counts_per_batch:
        B, N = len(counts), max(counts)
        pts = rng.uniform(0.05, 0.95, (B, N, 2)).astype(np.float32)
        wh = rng.uniform(0.02, 0.12, (B, N, 2)).astype(np.float32)
        ids = list(range(im_id, im_id + B))
        im_id += B
        for b, c in enumerate(counts):
            pts[b, c:] = 0.5
            gt["images"].append({"id": 1000 + ids[b], "file_name": f"{ids[b]}.png", "height": H, "width": W})
            for (px, py), (pw, ph) in zip(pts[b, :c], wh[b, :c]):
                w, h = float(pw) * W * 1.1, float(ph) * H * 0.9
                gt["annotations"].append({"id": len(gt["annotations"]) + 1, "image_id": 1000 + ids[b], "category_id": 1, "iscrowd": 0,
                                          "bbox": [float(px) * W - w / 2 + 1.0, float(py) * H - h / 2, w, h], "area": w * h})
        batches.append({"image": torch.zeros(B, 3, 8, 8), "points": torch.from_numpy(pts), "counts": torch.tensor(counts, dtype=torch.int32),
                        "orig_size": torch.tensor([[W, H]] * B), "im_id": torch.tensor(ids), "_wh": torch.from_numpy(wh).to(dev)})
    return batches, gt


class DeviceInputs:
    """A loader whose batches' points are already on the device (so that the stub can key on them) -- `.to(device)` is then a no-op in both
    paths, as it is for a data.Prefetcher's batches."""

    def __init__(self, batches, dev):
        self.batches = [{**{k: v for k, v in b.items() if k != "_wh"}, "points": b["points"].to(dev), "image": b["image"].to(dev)} for b in batches]
        self.stub = Stub()
        self.stub.on_device = {d["points"].data_ptr(): b["_wh"] for d, b in zip(self.batches, batches)}

    def loader(self):
        return list(self.batches)


def best(fn, repeats):
    out, times = None, []
    for _ in range(repeats + 1):                                                # the first run is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return out, min(times[1:]), times[1:]


def same(a, b):
    return a.keys() == b.keys() and all(a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])) for k in a)


def both_ways(inputs, tmp, dev, repeats):
    """write_pseudo_labels over the loader, host loop and device labels: -> (ann, store, host seconds, device seconds, all timings)."""
    h_dir, d_dir = os.path.join(tmp, "host"), os.path.join(tmp, "dev")
    h_ann, h_s, h_all = best(lambda: stage1.write_pseudo_labels(inputs.stub, inputs.loader(), "val", h_dir, device=dev), repeats)
    (d_ann, store), d_s, d_all = best(lambda: stage1.write_pseudo_labels(inputs.stub, inputs.loader(), "val", d_dir, device=dev, device_labels=True,
                                                                         return_store=True), repeats)
    with open(os.path.join(h_dir, "pseudo_bbox_val.json"), "rb") as f, open(os.path.join(d_dir, "pseudo_bbox_val.json"), "rb") as g:
        assert f.read() == g.read() and h_ann == d_ann
    return h_ann, store, h_s, d_s, {"host_all_s": h_all, "device_all_s": d_all}


def emit_alone(inputs, dev, repeats):
    """The emit call of the loader's first batch: device time by HIP events and the host time to enqueue it (medians)."""
    b = inputs.batches[0]
    B = b["points"].shape[0]
    args = (b["points"], inputs.stub.on_device[b["points"].data_ptr()], b["counts"].to(dev), b["orig_size"].to(device=dev, dtype=torch.int32))
    store = ops.PseudoLabelStore(B * (repeats + 2), int(b["counts"].sum()) * (repeats + 2), dev)
    ev_ms, host_us = [], []
    for _ in range(repeats + 2):
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        store.emit(*args, events=ev)
        host_us.append((time.perf_counter() - t0) * 1e6)
        torch.cuda.synchronize()
        ev_ms.append(ev[0].elapsed_time(ev[1]))
    store.finish()
    return sorted(ev_ms[1:])[len(ev_ms[1:]) // 2], sorted(host_us[1:])[len(host_us[1:]) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stage1_labels_time.json"))
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2026)
    res = {"what": "post-forward work of stage 1's label pass (stage1.write_pseudo_labels: host loop vs device_labels=True) and the scoring call "
                   "(score_pseudo_labels through the dicts with coco_ap.summarize(device=) vs store= through coco_ap.summarize_store); wall time, "
                   "best of %d after a warm-up; the emit call by HIP events.  Synthetic forward outputs (a stub in the model's place), original "
                   "size 384 x 576.  The host path is the parent commit's loop, unmeasured before." % a.repeats,
           "device": None, "one_batch_of_8": [], "pass_over_32_images": None, "scoring": None}
    with torch.cuda.device(dev), tempfile.TemporaryDirectory() as tmp:
        res["device"] = torch.cuda.get_device_name(0)
        for P in (7, 64, 300, 900):
            batches, _ = make_batches(rng, dev, [[P] * 8])
            inputs = DeviceInputs(batches, dev)
            _, _, h_s, d_s, all_s = both_ways(inputs, tmp, dev, a.repeats)
            ev_ms, enqueue_us = emit_alone(inputs, dev, a.repeats)
            row = {"points_per_image": P, "boxes": 8 * P, "whole_call_ms": {"host": h_s * 1e3, "device": d_s * 1e3, **all_s},
                   "emit_call": {"device_ms_hip_events_median": ev_ms, "host_enqueue_us_median": enqueue_us}, "files_byte_equal": True}
            print(json.dumps(row), flush=True)
            res["one_batch_of_8"].append(row)

        counts = [[int(c) for c in rng.integers(7, 901, 8)] for _ in range(4)]
        batches, gt = make_batches(rng, dev, counts)
        inputs = DeviceInputs(batches, dev)
        ann, store, h_s, d_s, all_s = both_ways(inputs, tmp, dev, a.repeats)
        res["pass_over_32_images"] = {"images": 32, "batches": 4, "boxes": len(ann["annotations"]), "seconds": {"host": h_s, "device": d_s, **all_s},
                                      "files_byte_equal": True}
        print(json.dumps(res["pass_over_32_images"]), flush=True)

        gj = os.path.join(tmp, "instances_val.json")
        with open(gj, "w") as f:
            json.dump(gt, f)
        via_json, json_s, _ = best(lambda: stage1.score_pseudo_labels(ann, gj, device=dev), a.repeats)

        def via_store_fn():
            store._host = None                                                  # pay the store's copy inside the window too
            return stage1.score_pseudo_labels(ann, gj, store=store)
        via_store, store_s, _ = best(via_store_fn, a.repeats)
        via_cached, cached_s, _ = best(lambda: stage1.score_pseudo_labels(ann, gj, store=store), a.repeats)
        assert same(via_json, via_store) and same(via_json, via_cached), (via_json, via_store)
        res["scoring"] = {"boxes": len(ann["annotations"]), "ground_truths": len(gt["annotations"]),
                          "seconds": {"dicts_then_summarize_device": json_s, "summarize_store_with_its_copy": store_s,
                                      "summarize_store_copy_already_made": cached_s},
                          "numbers_equal": True, "AP": via_json["AP"], "AP50": via_json["AP50"]}
        print(json.dumps(res["scoring"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
