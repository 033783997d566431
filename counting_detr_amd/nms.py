"""Greedy non-maximum suppression of duplicate detections (infer.py / main.py --nms_iou): the one rule and its host form.  Plain numpy, no
device.  On the device the same filter is cdetr_nms_suppress (ops.nms_suppress), one launch per forwarded batch.

THE RULE, stated once.  Suppression is a filter on `prob [B, Q]` that runs before anything else reads it:

  candidates of image b   the queries with fp32 prob[b, q] >= float32(threshold) (threshold_sweep.py's rule: a NaN is never a candidate);
                          `threshold` is the run's LOWEST threshold, --threshold or the first of a sweep;
  order                   descending prob, equal probabilities in ascending query order: the order of the evaluation records
                          (detections.hip's sort_key), NOT cut at max_det -- the cut comes later, on the survivors;
  box of a candidate      the evaluation box the matcher sees: coco_ap.reference_box([int(cx * W), int(cy * H), int(w * W), int(h * H)]), single
                          fp32 multiplies, truncation, reference_box in integers as detections.hip forms it, widened to float64;
  suppression             walking the order, a candidate is suppressed when its coco_ap.box_iou_xywh with some earlier SURVIVING candidate is
                          > iou: strict, in float64, the division performed.  A suppressed candidate suppresses nobody.  Where the union is not
                          positive the IoU is 0, so identical zero-area boxes never suppress each other;
  output                  prob_out = prob with every suppressed entry replaced by NaN -- every other entry keeps its own bits, NaNs, negative
                          zero and everything below the threshold included --, and removed [B] int32, the suppressed candidates per image;
  iou                     a finite number in [0, 1]: 1 suppresses nothing (the identity), 0 suppresses any positive overlap.

Why one pass serves a sweep: whether the candidate of rank k survives depends only on the survivors ranked before it, and the candidates of
a higher threshold are a prefix of the order.  So `suppress(prob, t_low)` restricted to prob >= t equals `suppress(prob, t)` there, for every
t >= t_low: the suppression at the sweep's lowest threshold is the suppression at each of its thresholds.
"""
import math

import numpy as np

from .coco_ap import box_iou_xywh


def check_iou(iou):
    """--nms_iou as a float: a finite number in [0, 1], ValueError otherwise."""
    try:
        v = float(iou)
    except (TypeError, ValueError):
        raise ValueError(f"--nms_iou: expected a number in [0, 1], got {iou!r}") from None
    if not math.isfinite(v) or not 0.0 <= v <= 1.0:
        raise ValueError(f"--nms_iou: expected a number in [0, 1], got {iou!r}")
    return v


def eval_boxes(boxes, ori_h, ori_w):
    """boxes fp32 [n, 4] normalised cxcywh of one image -> float64 [n, 4]: coco_ap.reference_box of the truncated fp32 products, in integers
    ([tdiv2(2 cx - w), tdiv2(2 cy - h), w, h], division truncating toward zero = int(cx - w / 2))."""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    scale = np.array([ori_w, ori_h, ori_w, ori_h], dtype=np.float32)
    cx, cy, w, h = ((boxes * scale).astype(np.int64)[:, k] for k in range(4))        # one fp32 multiply each, int() of each

    def tdiv2(v):
        return np.where(v >= 0, v // 2, -((-v) // 2))
    return np.stack([tdiv2(2 * cx - w), tdiv2(2 * cy - h), w, h], axis=1).astype(np.float64)


def suppress(prob, boxes, orig_hw, threshold, iou):
    """prob fp32 [B, Q], boxes fp32 [B, Q, 4] normalised cxcywh, orig_hw [B, 2] = (height, width) -> (prob_out fp32 [B, Q], removed int32 [B]):
    the rule above, the host form of cdetr_nms_suppress."""
    prob = np.ascontiguousarray(prob, dtype=np.float32)
    boxes = np.asarray(boxes, dtype=np.float32)
    orig_hw = np.asarray(orig_hw).reshape(-1, 2)
    if prob.ndim != 2 or boxes.shape != prob.shape + (4,) or orig_hw.shape[0] != prob.shape[0]:
        raise ValueError(f"nms.suppress: prob [B, Q], boxes [B, Q, 4], orig_hw [B, 2] expected, got {prob.shape}, {boxes.shape}, {orig_hw.shape}")
    iou, t32 = check_iou(iou), np.float32(threshold)
    if np.isnan(t32):
        raise ValueError(f"nms.suppress: a threshold must be a number, got {threshold!r}")
    out, removed = prob.copy(), np.zeros(prob.shape[0], dtype=np.int32)
    for b in range(prob.shape[0]):
        cand = np.flatnonzero(prob[b] >= t32)                               # ascending query order; a NaN compares false
        cand = cand[np.argsort(-prob[b, cand], kind="stable")]              # descending prob, -0 == +0, equal ones stay in query order
        bx = eval_boxes(boxes[b, cand], int(orig_hw[b, 0]), int(orig_hw[b, 1]))
        gone = np.zeros(len(cand), dtype=bool)
        for r in range(len(cand) - 1):
            if not gone[r]:                                                 # a survivor: everything behind it that it overlaps beyond `iou` goes
                gone[r + 1:] |= box_iou_xywh(bx[r + 1:], bx[r:r + 1])[:, 0] > iou
        out[b, cand[gone]] = np.nan
        removed[b] = int(gone.sum())
    return out, removed
