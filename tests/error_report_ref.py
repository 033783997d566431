"""The error breakdown of counting_detr_amd/error_report.py restated serially: plain Python loops over the IoU matrix of one image, one
detection and one ground truth at a time, sharing no code with the module (the matrix is coco_ap.box_iou_xywh's, the greedy match the loop
of coco_ap._evaluate_image written out for one threshold).  tests/test_error_report_cpu.py holds the module to it."""
import numpy as np

from counting_detr_amd import coco_ap as ca


def classify_image(gts, dts, n=None, iou_fg=0.5, iou_bg=0.1, area_rng=(0.0, 1e10)):
    """gts: [{bbox, area, (iscrowd), (ignore)}] in original order; dts: [{bbox, area}] in evaluation order, the first `n` used.
    -> dict of lists: dt_code, dt_gt, dt_iou, gt_code, gt_dt, gt_iou, counts."""
    G, D = len(gts), len(dts)
    n = D if n is None else min(D, max(int(n), 0))
    ign = [bool(g.get("ignore", 0)) or bool(g.get("iscrowd", 0)) or g["area"] < area_rng[0] or g["area"] > area_rng[1] for g in gts]
    iou = ca.box_iou_xywh([d["bbox"] for d in dts[:n]], [g["bbox"] for g in gts]).tolist() if n and G else [[0.0] * G for _ in range(n)]
    order = [g for g in range(G) if not ign[g]] + [g for g in range(G) if ign[g]]          # non-ignored first, original order otherwise
    gtm, dtm = [-1] * G, [-1] * n
    for d in range(n):
        best, m = iou_fg, -1
        for g in order:
            if gtm[g] >= 0:
                continue
            if m > -1 and not ign[m] and ign[g]:
                break
            if iou[d][g] < best:
                continue
            best, m = iou[d][g], g
        if m > -1:
            dtm[d], gtm[m] = m, d
    dt_code, dt_gt, dt_iou = [255] * D, [-1] * D, [0.0] * D
    for d in range(n):
        best, bg = 0.0, -1
        for g in range(G):
            if not ign[g] and iou[d][g] > 0 and iou[d][g] >= best:
                best, bg = iou[d][g], g
        area = dts[d].get("area", dts[d]["bbox"][2] * dts[d]["bbox"][3])
        if dtm[d] >= 0 and not ign[dtm[d]]:
            dt_code[d] = 0
        elif dtm[d] >= 0 or area < area_rng[0] or area > area_rng[1]:
            dt_code[d] = 1
        elif best >= iou_fg:
            dt_code[d] = 2
        elif best >= iou_bg:
            dt_code[d] = 3
        else:
            dt_code[d] = 4
        if dtm[d] >= 0:
            dt_gt[d], dt_iou[d] = dtm[d], iou[d][dtm[d]]
        else:
            dt_gt[d], dt_iou[d] = bg, best
    gt_code, gt_dt, gt_iou = [3] * G, [-1] * G, [0.0] * G
    for g in range(G):
        for d in range(n):
            if iou[d][g] > gt_iou[g]:
                gt_iou[g], gt_dt[g] = iou[d][g], d
        if ign[g]:
            gt_code[g] = 1
        elif gtm[g] >= 0:
            gt_code[g], gt_dt[g] = 0, gtm[g]
        else:
            for d in range(n):
                if dt_code[d] == 3 and dt_gt[d] == g:
                    gt_code[g] = 2
    counts = [sum(1 for c in dt_code[:n] if c == k) for k in range(5)] + [sum(1 for c in gt_code if c == k) for k in range(4)]
    return {"dt_code": dt_code, "dt_gt": dt_gt, "dt_iou": dt_iou, "gt_code": gt_code, "gt_dt": gt_dt, "gt_iou": gt_iou, "counts": counts}


def classify(gt_by_img, dt_by_img, counts=None, iou_bg=0.1, max_det=ca.MAX_DETS):
    """The dicts of coco_ap.average_precision -> the arrays of error_report.classify on `pack_images` of them: images in sorted-id order,
    those with neither ground truth nor detection left out, detections by descending score (stable), cut at max_det."""
    ids = [i for i in sorted(set(gt_by_img) | set(dt_by_img)) if gt_by_img.get(i) or dt_by_img.get(i)]
    parts = []
    for b, i in enumerate(ids):
        dts = dt_by_img.get(i, [])
        dts = [dts[j] for j in sorted(range(len(dts)), key=lambda j: -dts[j]["score"])][:max_det]          # sorted is stable
        parts.append(classify_image(gt_by_img.get(i, []), dts, None if counts is None else counts[b], min(0.5, 1 - 1e-10), iou_bg))
    cat = lambda k, t: np.array([v for p in parts for v in p[k]], dtype=t)                  # noqa: E731
    return {"dt_code": cat("dt_code", np.uint8), "dt_gt": cat("dt_gt", np.int32), "dt_iou": cat("dt_iou", np.float64),
            "gt_code": cat("gt_code", np.uint8), "gt_dt": cat("gt_dt", np.int32), "gt_iou": cat("gt_iou", np.float64),
            "counts": np.array([p["counts"] for p in parts], dtype=np.int32).reshape(len(ids), 9)}


def same(got, want):
    """Two code dicts, field by field, the IoUs as float64 bits."""
    for k in ("dt_code", "dt_gt", "dt_iou", "gt_code", "gt_dt", "gt_iou", "counts"):
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype == np.float64:
            g, w = g.view(np.int64), w.view(np.int64)
        bad = int((g != w).sum())
        assert bad == 0, f"{k}: {bad} of {w.size} differ"
