"""The independent yardstick of the suppression rule (counting_detr_amd/nms.py states it): a serial restatement, a Python loop over ranks that
calls coco_ap.box_iou_xywh on ONE pair at a time and shares no code with nms.py -- plus the seeded inputs the nms tests are made of."""
import numpy as np

from counting_detr_amd.coco_ap import box_iou_xywh, reference_box

NAN_BITS = 0x7FC12345                    # a NaN with a payload: it has to come through with its bits


def suppress(prob, boxes, orig_hw, threshold, iou):
    """-> (prob_out fp32 [B, Q], removed int32 [B]), one candidate and one pair at a time."""
    prob = np.asarray(prob, dtype=np.float32)
    out, removed = prob.copy(), np.zeros(prob.shape[0], dtype=np.int32)
    t32 = np.float32(threshold)
    for b in range(prob.shape[0]):
        H, W = np.float32(int(orig_hw[b][0])), np.float32(int(orig_hw[b][1]))
        cand = [q for q in range(prob.shape[1]) if prob[b, q] >= t32]
        cand.sort(key=lambda q: (-float(prob[b, q]), q))
        survivors = []
        for q in cand:
            cx, cy, w, h = (np.float32(v) for v in boxes[b][q])
            box = [float(v) for v in reference_box([int(cx * W), int(cy * H), int(w * W), int(h * H)])]
            if any(float(box_iou_xywh([box], [s])[0, 0]) > iou for s in survivors):
                out[b, q] = np.nan
                removed[b] += 1
            else:
                survivors.append(box)
    return out, removed


def same(got, want):
    """(prob_out, removed) pairs agree: equal NaN masks, the other entries bit for bit, `removed` equal."""
    (gp, gr), (wp, wr) = got, want
    gp, wp = np.asarray(gp), np.asarray(wp)
    if gp.dtype != np.float32 or gp.shape != wp.shape or not np.array_equal(np.isnan(gp), np.isnan(wp)):
        return False
    live = ~np.isnan(wp)
    return np.array_equal(gp.view(np.uint32)[live], wp.view(np.uint32)[live]) and np.array_equal(np.asarray(gr), np.asarray(wr)) \
        and np.asarray(gr).dtype == np.int32


def clustered(rng, Q, n_cand, n_clusters, threshold=0.5, spread=0.08):
    """One image: prob fp32 [Q] with exactly `n_cand` candidates at `threshold` (many on a coarse grid of scores, so equal scores occur; one ON
    the threshold), the rest below it with a NaN, a -0.0 and the value just under the threshold among them; boxes fp32 [Q, 4] normalised
    cxcywh around `n_clusters` centres (members of a cluster overlap heavily; n_clusters = 0: every box apart from every other)."""
    t32 = np.float32(threshold)
    prob = (rng.random(Q, dtype=np.float32) * t32 * np.float32(0.98)).astype(np.float32)
    below = [np.float32(np.nan), np.float32(-0.0), np.nextafter(t32, np.float32(-1))]
    cand = np.sort(rng.choice(Q, n_cand, replace=False))
    rest = np.setdiff1d(np.arange(Q), cand)
    for q, v in zip(rest, below):
        prob[q] = v
    if len(rest):
        prob[rest[:1]] = np.array([NAN_BITS], dtype=np.uint32).view(np.float32)
    score = t32 + (1 - t32) * rng.random(n_cand, dtype=np.float32)
    coarse = rng.random(n_cand) < 0.5
    score[coarse] = t32 + (1 - t32) * np.round(score[coarse] * 8) / 8
    if n_cand:
        score[rng.integers(n_cand)] = t32
    prob[cand] = np.clip(score, t32, 1).astype(np.float32)
    if n_clusters == 0:                     # a grid of disjoint cells
        side = int(np.ceil(np.sqrt(Q)))
        cell = 1.0 / side
        q = np.arange(Q)
        boxes = np.stack([(q % side + 0.5) * cell, (q // side + 0.5) * cell, np.full(Q, 0.5 * cell), np.full(Q, 0.5 * cell)], 1)
    else:
        centre = 0.15 + 0.7 * rng.random((n_clusters, 2))
        size = 0.06 + 0.08 * rng.random((n_clusters, 2))
        of = rng.integers(n_clusters, size=Q)
        boxes = np.concatenate([centre[of] + spread * size[of] * rng.standard_normal((Q, 2)), size[of] * (1 + spread * rng.standard_normal((Q, 2)))], 1)
    return prob, boxes.astype(np.float32)


def batch(rng, Q, counts, n_clusters, threshold=0.5, spread=0.08):
    """Images of `counts` candidates each -> prob [B, Q], boxes [B, Q, 4], orig_hw int32 [B, 2] (odd sizes, none square)."""
    rows = [clustered(rng, Q, n, n_clusters, threshold, spread) for n in counts]
    hw = np.array([[384 + 17 * b, 576 - 31 * b] for b in range(len(counts))], dtype=np.int32)
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), hw


# ---- the constructed cases: W = H = 64, so the normalised coordinates k / 64 are exact
def _image(entries, Q=None):
    """entries: (score, x, y, w, h) in pixels of a 64 x 64 image, x / y the left / top edge, even w / h -> prob [1, Q], boxes [1, Q, 4], hw."""
    Q = len(entries) if Q is None else Q
    prob, boxes = np.zeros((1, Q), dtype=np.float32), np.zeros((1, Q, 4), dtype=np.float32)
    for q, (s, x, y, w, h) in enumerate(entries):
        prob[0, q] = s
        boxes[0, q] = [(x + w / 2) / 64, (y + h / 2) / 64, w / 64, h / 64]
    return prob, boxes, np.array([[64, 64]], dtype=np.int32)


def constructed():
    """name -> (prob, boxes, orig_hw, threshold, iou, expected NaN mask of row 0 as a list of suppressed queries)."""
    just_under = float(np.nextafter(0.5, 0))
    pair = _image([(0.9, 10, 10, 6, 2), (0.8, 12, 10, 6, 2)])                                   # intersection 8, union 16
    chain = _image([(0.9, 10, 10, 6, 2), (0.8, 11, 10, 6, 2), (0.7, 12, 10, 6, 2)])             # IoU 10/14, 10/14, 8/16
    equal = _image([(0.75, 20, 20, 8, 8), (0.75, 20, 20, 8, 8)])
    flat = _image([(0.9, 30, 30, 0, 8), (0.8, 30, 30, 0, 8)])
    special = _image([(0.9, 10, 10, 6, 2), (np.nan, 10, 10, 6, 2), (-0.0, 10, 10, 6, 2), (0.25, 10, 10, 6, 2), (0.8, 10, 10, 6, 2)])
    special[0][0, 1] = np.array([NAN_BITS], dtype=np.uint32).view(np.float32)[0]
    return {"iou_exactly_half_kept": (*pair, 0.5, 0.5, []),
            "iou_exactly_half_suppressed_just_under": (*pair, 0.5, just_under, [1]),
            "chain_is_greedy": (*chain, 0.5, 0.5, [1]),                                         # B goes; C meets A at exactly 0.5 and survives
            "equal_scores_lower_query_survives": (*equal, 0.5, 0.5, [1]),
            "zero_area_boxes_never_suppress": (*flat, 0.5, 0.0, []),
            "special_values_pass_with_their_bits": (*special, 0.5, 0.5, [4])}
