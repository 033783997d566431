"""The work between the forward and the box AP, host path against device path (infer.py --device_detections), on generated forward outputs:
64 images of 384 x 576 with Q = 900 queries (about 60 kept each) and one image with Q = 1728 (more than 1100 kept: the cut bites).  No model
runs: prob / pred_boxes / reference points are seeded device tensors standing in for the captured forward's static outputs, the six losses
device scalars.

  host   = infer.py's loop body as it stands: three .cpu() copies per image, float() of every loss, one dict per detection;
  device = what infer._infer_device does instead: the losses into a device buffer, one cdetr_emit_detections call per image, then ONE copy of
           the store and the annotation dicts built from its arrays.

Wall time per image of each (best of --repeats after a warm-up, every window ends in a device synchronise or a blocking copy), the emit
call's own time by HIP events (count + emit kernels, median over the images), and the whole AP call: coco_ap.ap_from_json(device=) on the
written predictions json against coco_ap.summarize_store on the store.  Both paths' annotations and six AP numbers are asserted equal.
No threshold is set: the host path's per-image cost had not been measured before.

usage: python tools/detections_time.py [--out profiles/detections_time.json] [--repeats 5]"""
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

from counting_detr_amd import coco_ap as ca
from counting_detr_amd import ops


def make_set(rng, n, Q, hw, kept_frac, dev):
    """Seeded forward outputs of n images (one launch of B = 1 each) + a ground truth json body whose boxes sit near some predictions."""
    imgs, gt = [], {"images": [], "categories": [{"id": 1, "name": "fg"}], "annotations": []}
    for i in range(n):
        prob = np.where(rng.uniform(size=Q) < kept_frac, rng.uniform(0.5, 0.99, Q), rng.uniform(0.01, 0.49, Q)).astype(np.float32)
        boxes = np.concatenate([rng.uniform(0.05, 0.95, (Q, 2)), rng.uniform(0.02, 0.12, (Q, 2))], axis=1).astype(np.float32)
        pts = boxes[:, :2] + rng.uniform(-0.01, 0.01, (Q, 2)).astype(np.float32)
        imgs.append({"prob": torch.from_numpy(prob[None]).to(dev), "boxes": torch.from_numpy(boxes[None]).to(dev), "pts": torch.from_numpy(pts[None]).to(dev),
                     "hw": torch.tensor([list(hw)], dtype=torch.int32, device=dev), "ori": hw, "id": i + 1,
                     "losses": [torch.tensor(float(v), device=dev) for v in rng.uniform(0.1, 2.0, 6)]})
        gt["images"].append({"id": i + 1, "height": hw[0], "width": hw[1]})
        for q in np.nonzero(prob >= 0.5)[0][::2]:                               # every other kept query has a ground truth under it
            cx, cy, w, h = boxes[q] * np.array([hw[1], hw[0], hw[1], hw[0]])
            gt["annotations"].append({"id": len(gt["annotations"]) + 1, "image_id": i + 1, "category_id": 1, "iscrowd": 0,
                                      "bbox": [float(cx - w / 2) + 1.0, float(cy - h / 2), float(w), float(h)], "area": float(w * h)})
    return imgs, gt


def host_post(imgs, threshold=0.5):
    """infer.py's loop body after the forward, per image (the keep mask is the engine's, formed on the device)."""
    anns, loss_sum, counts, anno_id = [], 0.0, [], 1
    for im in imgs:
        for v in im["losses"]:
            loss_sum += float(v)
        ori_h, ori_w = im["ori"]
        kb = (im["prob"] >= threshold)[0]
        scores = im["prob"][0][kb].cpu().numpy()
        boxes = im["boxes"][0][kb].cpu().numpy().copy()
        pts = im["pts"][0][kb].cpu().numpy().copy()
        pts[..., 0] *= ori_w; pts[..., 1] *= ori_h
        boxes[..., 0] *= ori_w; boxes[..., 1] *= ori_h; boxes[..., 2] *= ori_w; boxes[..., 3] *= ori_h
        for sc, bx, pt in zip(scores, boxes, pts):
            x_cen, y_cen, w, h = bx
            anns.append({"id": anno_id, "image_id": im["id"], "area": int(w * h), "bbox": [int(x_cen), int(y_cen), int(w), int(h)], "category_id": 1,
                         "score": float(sc), "point": [int(pt[0]), int(pt[1])]})
            anno_id += 1
        counts.append(int(kb.sum()))
    return anns, counts, loss_sum


def device_post(imgs, dev, threshold=0.5, events=None):
    """infer._infer_device's work after the forward: per image the losses into a buffer and one emit call; one copy at the end."""
    Q = imgs[0]["prob"].shape[1]
    store = ops.DetectionStore(len(imgs), Q, dev, threshold=threshold, max_det=ca.MAX_DETS)
    loss_buf = torch.zeros((len(imgs), 6), dtype=torch.float64, device=dev)
    for k, im in enumerate(imgs):
        loss_buf[k].copy_(torch.stack([v.to(torch.float64) for v in im["losses"]]))
        store.emit(im["prob"], im["boxes"], im["pts"], im["hw"], events=events[k] if events else None)
    host = store.finish()
    loss_sum = 0.0
    for row in loss_buf.cpu().tolist():
        for v in row:
            loss_sum += v
    ann_image = [im["id"] for im, c in zip(imgs, np.diff(host["wire_off"]).tolist()) for _ in range(c)]
    wire, score = host["wire"].tolist(), host["score"].astype(np.float64).tolist()
    anns = [{"id": k + 1, "image_id": i, "area": w[4], "bbox": w[:4], "category_id": 1, "score": sc, "point": w[5:7]}
            for k, (i, w, sc) in enumerate(zip(ann_image, wire, score))]
    return anns, host["counts"].tolist(), loss_sum, store


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
    return all(a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])) for k in a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detections_time.json"))
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2025)
    sets = [("64 images of 384 x 576, Q = 900", make_set(rng, 64, 900, (384, 576), 0.07, dev)),
            ("1 image of 384 x 576, Q = 1728", make_set(rng, 1, 1728, (384, 576), 0.8, dev))]
    rows = []
    with torch.cuda.device(dev), tempfile.TemporaryDirectory() as tmp:
        for name, (imgs, gt) in sets:
            n = len(imgs)
            (h_anns, h_counts, h_loss), host_s, host_all = best(lambda: host_post(imgs), a.repeats)
            (d_anns, d_counts, d_loss, store), dev_s, dev_all = best(lambda: device_post(imgs, dev), a.repeats)
            assert h_anns == d_anns and h_counts == d_counts and h_loss == d_loss, name
            events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in imgs]
            device_post(imgs, dev, events=events)
            torch.cuda.synchronize()
            emit_ms = sorted(e0.elapsed_time(e1) for e0, e1 in events)
            pj, gj = os.path.join(tmp, "p.json"), os.path.join(tmp, "g.json")
            with open(pj, "w") as f:
                json.dump({"categories": gt["categories"], "images": gt["images"], "annotations": h_anns}, f)
            with open(gj, "w") as f:
                json.dump(gt, f)
            ids = [im["id"] for im in imgs]
            gt_by = ca.gt_from_json(gj, ids)
            ap_file, file_s, _ = best(lambda: ca.ap_from_json(pj, gj, device=dev), a.repeats)

            def store_ap():
                store._host = None                                              # pay the store's copy inside the window too
                return ca.summarize_store(gt_by, store, ids)
            ap_store, store_s, _ = best(store_ap, a.repeats)
            ap_store_cached, cached_s, _ = best(lambda: ca.summarize_store(gt_by, store, ids), a.repeats)
            assert same(ap_file, ap_store) and same(ap_file, ap_store_cached), (name, ap_file, ap_store)
            row = {"set": name, "images": n, "queries": int(imgs[0]["prob"].shape[1]), "detections": len(h_anns),
                   "evaluated_detections": int(store.finish()["eval_off"][-1]),
                   "post_forward_ms_per_image": {"host": host_s / n * 1e3, "device": dev_s / n * 1e3, "host_all_s": host_all, "device_all_s": dev_all},
                   "emit_call_ms_hip_events": {"median": emit_ms[len(emit_ms) // 2], "min": emit_ms[0], "max": emit_ms[-1]},
                   "ap_s": {"ap_from_json_device": file_s, "summarize_store_with_its_copy": store_s, "summarize_store_copy_already_made": cached_s},
                   "annotations_counts_losses_equal": True, "six_numbers_equal": True, "AP": ap_file["AP"], "AP50": ap_file["AP50"]}
            print(json.dumps(row), flush=True)
            rows.append(row)
    res = {"what": "post-forward work of infer.py per image (host loop vs --device_detections) and the box-AP call (ap_from_json(device=) on the "
                   "json vs summarize_store on the device-resident store); wall time, best of %d after a warm-up; the emit call by HIP events. "
                   "Synthetic forward outputs, no model in the window.  The host path is the parent commit's code, unmeasured before." % a.repeats,
           "device": torch.cuda.get_device_name(0), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
