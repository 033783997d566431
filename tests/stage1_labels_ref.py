"""A numpy restatement of cdetr_emit_pseudo_labels (include/cdetr_hip.h, csrc/stage1_labels.hip) in explicit fp32, integer and float64
arithmetic -- the checker of tests/test_stage1_labels_cpu.py (which pins it to stage1.write_pseudo_labels' host loop) and of
tests/test_stage1_labels_gpu.py (which compares the kernel with it, array_equal).  Not a test module; imported by both."""
import numpy as np

F32 = np.float32


def next_below(v):
    """The fp32 one step below v (towards -inf)."""
    return np.nextafter(F32(v), F32(-np.inf))


def emit_image(points, pred_wh, ori_w, ori_h, max_det, gt_xywh=None):
    """One image's valid rows: points f32 [P, 2], pred_wh f32 [P, 2] -> dict: wire int32 [P, 5] (cx, cy, w, h, area), pair_iou f64 [P],
    eval_boxes f64 [E, 4], eval_area f64 [E], eval_score f64 [E] with E = min(P, max_det)."""
    points, pred_wh = np.asarray(points, dtype=F32).reshape(-1, 2), np.asarray(pred_wh, dtype=F32).reshape(-1, 2)
    W, H = F32(int(ori_w)), F32(int(ori_h))
    xf, yf, wf, hf = points[:, 0] * W, points[:, 1] * H, pred_wh[:, 0] * W, pred_wh[:, 1] * H      # one fp32 multiply each
    assert xf.dtype == F32 and (wf * hf).dtype == F32
    wire = np.stack([np.trunc(v).astype(np.int64) for v in (xf, yf, wf, hf, wf * hf)], axis=1).reshape(-1, 5)
    assert (np.abs(wire) < 2 ** 31).all()
    cx, cy, w, h = (wire[:, k].astype(np.float64) for k in range(4))
    boxes = np.stack([cx - w / 2.0, cy - h / 2.0, w, h], axis=1).reshape(-1, 4)                   # from the ints, not truncated again
    iou = np.zeros(len(wire))
    if gt_xywh is not None:
        iou = pair_iou(boxes, np.asarray(gt_xywh, dtype=np.float64).reshape(-1, 4))
    E = min(len(wire), max_det)
    return {"wire": wire.astype(np.int32), "pair_iou": iou, "eval_boxes": boxes[:E], "eval_area": (w * h)[:E], "eval_score": np.ones(E)}


def pair_iou(dt, gt):
    """Row-wise IoU of xywh boxes by the operations of coco_ap.box_iou_xywh (its diagonal), float64."""
    da, ga = dt[:, 2] * dt[:, 3], gt[:, 2] * gt[:, 3]
    w = np.minimum(dt[:, 0] + dt[:, 2], gt[:, 0] + gt[:, 2]) - np.maximum(dt[:, 0], gt[:, 0])
    h = np.minimum(dt[:, 1] + dt[:, 3], gt[:, 1] + gt[:, 3]) - np.maximum(dt[:, 1], gt[:, 1])
    inter = np.clip(w, 0, None) * np.clip(h, 0, None)
    union = da + ga - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(union > 0, inter / union, 0.0)


def emit_store(batches, max_det):
    """A sequence of launches, each (points [B, R, 2], pred_wh [B, R, 2], counts [B] or None, orig_wh [B, 2] = (width, height), gt_xywh
    [B, R, 4] or None) -> what ops.PseudoLabelStore.finish returns after them (wire int32 [rows, 6] with the store image index in front),
    plus eval_boxes / eval_area (device-resident there)."""
    imgs = []
    for points, pred_wh, counts, orig_wh, gt in batches:
        for b in range(len(points)):
            c = points.shape[1] if counts is None else int(counts[b])
            imgs.append(emit_image(points[b, :c], pred_wh[b, :c], orig_wh[b][0], orig_wh[b][1], max_det, None if gt is None else gt[b, :c]))
    cat = lambda k, shape, dt: (np.concatenate([i[k] for i in imgs]) if imgs else np.zeros(0)).reshape(shape).astype(dt)      # noqa: E731
    counts = np.array([len(i["wire"]) for i in imgs], dtype=np.int32)
    index = np.repeat(np.arange(len(imgs), dtype=np.int32), counts)
    return {"counts": counts,
            "row_off": np.concatenate([[0], np.cumsum(counts)]).astype(np.int32),
            "eval_off": np.concatenate([[0], np.cumsum([len(i["eval_area"]) for i in imgs])]).astype(np.int32),
            "wire": np.concatenate([index[:, None], cat("wire", (-1, 5), np.int32)], axis=1), "pair_iou": cat("pair_iou", (-1,), np.float64),
            "eval_boxes": cat("eval_boxes", (-1, 4), np.float64), "eval_area": cat("eval_area", (-1,), np.float64),
            "eval_score": cat("eval_score", (-1,), np.float64)}


def same(a, b):
    """Equality of score dicts / lists with NaN == NaN (an undefined APm / APl is NaN on both sides)."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and a != a:
        return isinstance(b, float) and b != b
    return a == b


def truncation_rows():
    """Hand-made (point, wh, (width, height)) rows where one fp32 rounding decides an integer of the json:
    a product exactly on an integer (0.5 x 384), one fp32 step below an integer, and w * h near 10^6 where the fp32 rounding of the
    PRODUCT of the unrounded sizes decides int(area).  -> points f32 [K, 2], pred_wh f32 [K, 2], (width, height)."""
    W, H = 384, 1000
    pts = [(0.5, 0.5), (next_below(0.5), next_below(0.5)), (0.25, 0.125), (next_below(0.25), 0.999)]
    whs = [(0.5, 0.5), (next_below(0.5), next_below(0.5)),
           (F32(2000.0) / F32(W), F32(0.5)),                              # 2000 x 500 = 10^6 exactly: wider than the image, still a row
           (next_below(F32(1000.5) / F32(W)), next_below(F32(999.5) / F32(H)))]
    # sizes whose fp32 product sits within a few ulp (2^-4 at 10^6) of an integer
    for k in range(8):
        wf, hf = F32(1000.0) + F32(k) * F32(0.0625), F32(1000.0) - F32(k) * F32(0.0625)
        pts.append((0.3, 0.7))
        whs.append((wf / F32(W), hf / F32(H)))
    return np.array(pts, dtype=F32), np.array(whs, dtype=F32), (W, H)


def make_batch(rng, B, R, sizes, gt=True, hand=True):
    """Seeded inputs of one launch: points anywhere in the image, sizes up to 60 % of it (some corners cx - w/2 go negative), the hand-made
    truncation rows in front of image 0 (`hand`; its size is then truncation_rows' own), ground-truth boxes near the predicted ones so that
    the IoUs cover 0 .. 1.  -> points, pred_wh f32 [B, R, 2], orig_wh int32 [B, 2], gt_xywh f64 [B, R, 4] or None."""
    points = rng.uniform(0.0, 1.0, (B, R, 2)).astype(F32)
    pred_wh = rng.uniform(0.004, 0.6, (B, R, 2)).astype(F32)
    orig_wh = np.array([sizes[b % len(sizes)] for b in range(B)], dtype=np.int32)
    if hand:
        p, w, size = truncation_rows()
        k = min(len(p), R)
        points[0, :k], pred_wh[0, :k], orig_wh[0] = p[:k], w[:k], size
    gt_xywh = None
    if gt:
        wh = pred_wh.astype(np.float64) * orig_wh[:, None, :] * rng.uniform(0.5, 1.6, (B, R, 2))
        c = points.astype(np.float64) * orig_wh[:, None, :] + rng.uniform(-0.4, 0.4, (B, R, 2)) * wh
        gt_xywh = np.concatenate([c - wh / 2, wh], axis=2)
        gt_xywh[:, ::7] = np.round(gt_xywh[:, ::7])                   # some integer boxes, as FSC-147's are
        gt_xywh[:, 5::11, :2] += 5000.0                               # some disjoint pairs: IoU 0
    return points, pred_wh, orig_wh, gt_xywh
