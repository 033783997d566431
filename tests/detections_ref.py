"""A numpy restatement of cdetr_emit_detections (include/cdetr_hip.h, csrc/detections.hip) in explicit fp32 and integer arithmetic -- the checker
of tests/test_detections_cpu.py (which pins it to infer.py's host loop, coco_ap.reference_box and coco_ap.pack_images) and of
tests/test_detections_gpu.py (which compares the kernel with it, array_equal).  Not a test module; imported by both."""
import numpy as np

F32 = np.float32


def tdiv2(t):
    """Integer division by 2 truncating toward zero (numpy's // floors)."""
    t = np.asarray(t, dtype=np.int64)
    return np.where(t >= 0, t // 2, -((-t) // 2))


def emit_image(prob, boxes, points, ori_h, ori_w, threshold, max_det):
    """One image: prob f32 [Q], boxes f32 [Q, 4], points f32 [Q, 2] -> dict: q (kept queries, ascending), wire int32 [K, 7], score f32 [K],
    eval_q, eval_boxes f64 [E, 4], eval_area f64 [E], eval_score f64 [E]."""
    prob, boxes, points = np.asarray(prob, dtype=F32), np.asarray(boxes, dtype=F32), np.asarray(points, dtype=F32)
    with np.errstate(invalid="ignore"):
        q = np.nonzero(prob >= F32(threshold))[0]                              # a NaN compares false: dropped
    W, H = F32(int(ori_w)), F32(int(ori_h))
    b, p = boxes[q], points[q]
    fx, fy, fw, fh = b[:, 0] * W, b[:, 1] * H, b[:, 2] * W, b[:, 3] * H        # float32 array x float32 scalar: one fp32 multiply each
    assert fx.dtype == F32 and (fw * fh).dtype == F32
    cols = [np.trunc(v).astype(np.int64) for v in (fx, fy, fw, fh, fw * fh, p[:, 0] * W, p[:, 1] * H)]
    wire = np.stack(cols, axis=1).reshape(-1, 7)
    assert (np.abs(wire) < 2 ** 31).all()
    score = prob[q]
    order = np.argsort(-score.astype(np.float64), kind="stable")[:max_det]      # descending score, equal scores keep ascending q; the cut last
    cx, cy, w, h = (wire[order, k] for k in range(4))
    eval_boxes = np.stack([tdiv2(2 * cx - w), tdiv2(2 * cy - h), w, h], axis=1).reshape(-1, 4).astype(np.float64)
    return {"q": q, "wire": wire.astype(np.int32), "score": score, "eval_q": q[order], "eval_boxes": eval_boxes,
            "eval_area": (w * h).astype(np.float64), "eval_score": score[order].astype(np.float64)}


def emit_store(batches, threshold, max_det, wire_cap=None, eval_cap=None):
    """A sequence of launches, each (prob [B, Q], boxes [B, Q, 4], points [B, Q, 2], orig_hw [B, 2] = (height, width)) -> what
    ops.DetectionStore.finish returns after them, plus eval_boxes / eval_area (device-resident there) and the per-image dicts.

    wire_cap / eval_cap (records; None: room for everything): the kernel's rule for a store that may overflow.  A launch starts at the
    offsets the launch before it left; inside a launch an image lands behind the launch's earlier images, whether those fitted or not, and
    its next offsets are start + those counts + its own: they run on past a capacity, UNclamped.  An image that does not fit both sections
    writes nothing and ORs 1 (wire records) | 2 (evaluation records) into `status`; a launch whose start lies beyond a capacity writes
    nothing, repeats its start as every next offset and ORs 4.  `placed`: per image (first wire record, first evaluation record) or None;
    the concatenated record arrays hold the placed images only; `counts` are the images' own either way."""
    imgs, placed, status, wire_off, eval_off = [], [], 0, [0], [0]
    for prob, boxes, points, orig_hw in batches:
        sw, se = wire_off[-1], eval_off[-1]
        start_ok = (wire_cap is None or sw <= wire_cap) and (eval_cap is None or se <= eval_cap)
        w0, e0 = sw, se
        for b in range(len(prob)):
            im = emit_image(prob[b], boxes[b], points[b], orig_hw[b][0], orig_hw[b][1], threshold, max_det)
            imgs.append(im)
            w1, e1 = w0 + len(im["q"]), e0 + len(im["eval_q"])
            fits_w, fits_e = start_ok and (wire_cap is None or w1 <= wire_cap), start_ok and (eval_cap is None or e1 <= eval_cap)
            placed.append((w0, e0) if fits_w and fits_e else None)
            status |= 4 if not start_ok else (0 if fits_w else 1) | (0 if fits_e else 2)
            wire_off.append(w1 if start_ok else sw)
            eval_off.append(e1 if start_ok else se)
            w0, e0 = w1, e1
    put = [i for i, at in zip(imgs, placed) if at]
    cat = lambda k, shape, dt: (np.concatenate([i[k] for i in put]) if put else np.zeros(0)).reshape(shape).astype(dt)      # noqa: E731
    return {"counts": np.array([len(i["q"]) for i in imgs], dtype=np.int32),
            "wire_off": np.array(wire_off, dtype=np.int32), "eval_off": np.array(eval_off, dtype=np.int32),
            "wire": cat("wire", (-1, 7), np.int32), "score": cat("score", (-1,), F32),
            "eval_boxes": cat("eval_boxes", (-1, 4), np.float64), "eval_area": cat("eval_area", (-1,), np.float64),
            "eval_score": cat("eval_score", (-1,), np.float64), "images": imgs, "placed": placed, "status": status}


def make_case(rng, Q, hw, kept="some", ties=0, at_threshold=False, nan=False, negative_corner=True, threshold=0.5):
    """Seeded inputs of one image: probabilities around the threshold (`kept`: "some" / "all" / "none"), `ties` groups of equal scores at
    non-adjacent queries, optionally one probability exactly at the threshold and one NaN; boxes with centres anywhere in the image and sizes up
    to 60 % of it, so that some corners cx - w/2 go negative (`negative_corner`: at least one is forced)."""
    lo, hi = {"some": (0.2, 0.95), "all": (0.55, 0.99), "none": (0.01, 0.45)}[kept]
    prob = rng.uniform(lo, hi, Q).astype(F32)
    free = list(rng.permutation(Q))
    if kept == "some" and Q >= 2:
        prob[free[0]], prob[free[1]] = F32(0.9), F32(0.1)                     # at least one on each side
        free = free[2:]
    for _ in range(ties):
        if len(free) < 3:
            break
        grp = sorted(free[:3])
        free = free[3:]
        prob[grp] = F32(rng.uniform(0.6, 0.9))
    if at_threshold and free:
        prob[free.pop()] = F32(threshold)
    if nan and free:
        prob[free.pop()] = np.nan
    boxes = np.concatenate([rng.uniform(0.0, 1.0, (Q, 2)), rng.uniform(0.005, 0.6, (Q, 2))], axis=1).astype(F32)
    if negative_corner:
        k = int(np.nanargmax(prob))
        boxes[k] = np.array([0.02, 0.03, 0.5, 0.4], dtype=F32)                 # kept whenever anything is: overhangs the left and top edges
    points = rng.uniform(0.0, 1.0, (Q, 2)).astype(F32)
    return prob, boxes, points, np.array(hw, dtype=np.int32)
