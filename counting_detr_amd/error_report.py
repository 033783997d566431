"""WHY a detection failed: the single-class form of the TIDE error breakdown (Bolya et al., ECCV 2020) on one pack of coco_ap
(`pack_images` / `pack_store`), in numpy.  The evaluation says how good the model is (six AP numbers, MAE / RMSE), `--image_report` on which
images it fails, `--render_worst` shows them; this says what went wrong, because each cause has another fix:

  duplicate     the same object counted twice                       -> --nms_iou, fewer query patterns
  localisation  a box on an object, IoU < 0.5 with it               -> box loss weights, stage-1 pseudo-box quality
  background    a box on nothing                                    -> the threshold
  missed        no box anywhere near an object                      -> the threshold, the query count (--tiles)

The reference has nothing like it.  This module is the RULE and the checker: csrc/error_report.hip (cdetr_coco_errors, one launch for a
split) equals `classify` bit for bit (tests/test_error_report_cpu.py pins `classify` to a loop-by-loop restatement, _gpu.py the kernel to it).

THE RULE, per image, area range `all`, iou_fg = min(0.5, 1 - 1e-10) = coco_ap.IOU_THRS[0] as the matcher clips it, iou_bg = 0.1 (TIDE's):
  * a ground truth is ignored by `coco_ap._evaluate_image`'s rule; the greedy match at iou_fg is that function's at that threshold -> dtm[d]
    (ground-truth index in the image's original order, -1) and gtm[g];
  * best_iou[d], best_gt[d]: the largest `coco_ap.box_iou_xywh` of d over the NON-IGNORED ground truths, taken or not, the highest index
    among equal IoUs (the matcher's tie rule); (0.0, -1) when no such IoU is > 0;
  * detection codes: 0 TP matched to a non-ignored ground truth; 1 IGN `det_ignored` of the matching; unmatched otherwise: 2 DUP
    best_iou >= iou_fg, 3 LOC iou_bg <= best_iou < iou_fg, 4 BKG best_iou < iou_bg; 255 beyond the image's prefix (`counts`);
    dt_gt = the matched ground truth if matched, else best_gt; dt_iou = the IoU with it (0.0 with -1);
  * ground-truth codes: 0 HIT gtm >= 0 and not ignored; 1 IGN; 2 MISLOC not hit and the best_gt of at least one LOC detection; 3 MISSED;
    gt_iou = its largest IoU over the used detections, gt_dt = the matched detection if hit, else the lowest detection reaching gt_iou
    (-1 when gt_iou == 0);
  * counts[b] = (tp, ign_dt, dup, loc, bkg, hit, ign_gt, misloc, missed).
A DUP detection's best ground truth is taken: it is unmatched, so no free non-ignored ground truth has an IoU >= iou_fg with it, and its
best one has.

WHAT-IF AP50 (`what_if`, TIDE's dAP, host numpy on the codes on every route): AP50 of the merged list through `coco_ap._sample` with the
operations of `coco_ap.accumulate`, once as it is (`AP50_base`, which EQUALS the matching's own AP50) and once per cause with the flags
changed as if the cause were fixed: DUP / BKG detections ignored; per MISLOC ground truth its first LOC detection a true positive and every
other LOC detection ignored; npig less the MISSED count.
"""
import numpy as np

from . import coco_ap as ca

IOU_FG = float(min(ca.IOU_THRS[0], 1 - 1e-10))
IOU_BG = 0.1
TP, IGN, DUP, LOC, BKG, UNUSED = 0, 1, 2, 3, 4, 255
HIT, GT_IGN, MISLOC, MISSED = 0, 1, 2, 3
COUNT_KEYS = ("tp", "ign_dt", "dup", "loc", "bkg", "hit", "ign_gt", "misloc", "missed")
DAP_KEYS = ("dAP50_dup", "dAP50_loc", "dAP50_bkg", "dAP50_missed")
ERR_KEYS = ("err_dup", "err_loc", "err_bkg", "err_misloc", "err_missed")


def classify_image(gt_boxes, gt_area, gt_ignore, dt_boxes, dt_area, n=None, iou_fg=IOU_FG, iou_bg=IOU_BG, area_rng=ca.AREA_RNG["all"]):
    """The rule on one image: ground truths in their original order, detections in evaluation order, of which the first `n` are used.
    -> (dt_code u8 [D], dt_gt i32 [D], dt_iou f64 [D], gt_code u8 [G], gt_dt i32 [G], gt_iou f64 [G], counts i32 [9])."""
    gt_boxes, dt_boxes = np.asarray(gt_boxes, dtype=np.float64).reshape(-1, 4), np.asarray(dt_boxes, dtype=np.float64).reshape(-1, 4)
    gt_area, dt_area = np.asarray(gt_area, dtype=np.float64), np.asarray(dt_area, dtype=np.float64)
    G, D = len(gt_boxes), len(dt_boxes)
    n = D if n is None else min(D, max(int(n), 0))
    g_ig = np.asarray(gt_ignore, dtype=bool) | (gt_area < area_rng[0]) | (gt_area > area_rng[1])
    iou = ca.box_iou_xywh(dt_boxes[:n], gt_boxes)                                   # [n, G]
    dt_code, dt_gt, dt_iou = np.full(D, UNUSED, dtype=np.uint8), -np.ones(D, dtype=np.int32), np.zeros(D)
    gtm = -np.ones(G, dtype=np.int64)
    real = ~g_ig
    index = np.arange(G)
    for d in range(n):
        row = iou[d]
        # _evaluate_image at one threshold: the free non-ignored ground truth of highest IoU >= iou_fg, the highest index among equal IoUs;
        # only when there is none, by the same rule a free ignored one
        m = -1
        for group in (real, g_ig):
            cand = group & (gtm < 0) & (row >= iou_fg)
            if cand.any():
                m = int(index[cand & (row == row[cand].max())].max())
                break
        # the best overlap: every non-ignored ground truth, taken or not
        over = real & (row > 0)
        best_gt = int(index[over & (row == row[over].max())].max()) if over.any() else -1
        best_iou = float(row[best_gt]) if best_gt >= 0 else 0.0
        if m >= 0:
            gtm[m] = d
            dt_code[d], dt_gt[d], dt_iou[d] = (IGN if g_ig[m] else TP), m, row[m]
            continue
        dt_gt[d], dt_iou[d] = best_gt, best_iou
        if dt_area[d] < area_rng[0] or dt_area[d] > area_rng[1]:
            dt_code[d] = IGN
        elif best_iou >= iou_fg:
            dt_code[d] = DUP
        elif best_iou >= iou_bg:
            dt_code[d] = LOC
        else:
            dt_code[d] = BKG
    hit = (gtm >= 0) & real
    marked = np.zeros(G, dtype=bool)
    loc_gt = dt_gt[:n][(dt_code[:n] == LOC) & (dt_gt[:n] >= 0)]
    marked[loc_gt] = True
    gt_code = np.where(g_ig, GT_IGN, np.where(hit, HIT, np.where(marked, MISLOC, MISSED))).astype(np.uint8)
    if n and G:
        gt_iou = iou.max(axis=0)
        first = np.argmax(iou == gt_iou[None, :], axis=0)                           # the lowest detection reaching the maximum
        gt_dt = np.where(hit, gtm, np.where(gt_iou > 0, first, -1)).astype(np.int32)
    else:
        gt_iou, gt_dt = np.zeros(G), -np.ones(G, dtype=np.int32)
    used = dt_code[:n]
    counts = np.array([(used == c).sum() for c in (TP, IGN, DUP, LOC, BKG)] + [(gt_code == c).sum() for c in (HIT, GT_IGN, MISLOC, MISSED)],
                      dtype=np.int32)
    return dt_code, dt_gt, dt_iou, gt_code, gt_dt, np.asarray(gt_iou, dtype=np.float64), counts


def classify(pack, counts=None, iou_bg=IOU_BG, iou_fg=IOU_FG):
    """The rule on every image of a pack (host arrays: a `pack_images` pack) -> {"dt_code" u8 [Dtot], "dt_gt" i32 [Dtot], "dt_iou" f64 [Dtot],
    "gt_code" u8 [Gtot], "gt_dt" i32 [Gtot], "gt_iou" f64 [Gtot], "counts" i32 [B, 9]}, indices local to the image.  `counts` [B]: use only the
    first min(counts[b], segment) detections of pack image b."""
    gt_off, dt_off = np.asarray(pack["gt_off"], dtype=np.int64), np.asarray(pack["dt_off"], dtype=np.int64)
    B = len(gt_off) - 1
    parts = [classify_image(pack["gt_boxes"][gt_off[b]:gt_off[b + 1]], pack["gt_area"][gt_off[b]:gt_off[b + 1]],
                            pack["gt_ignore"][gt_off[b]:gt_off[b + 1]], pack["dt_boxes"][dt_off[b]:dt_off[b + 1]],
                            pack["dt_area"][dt_off[b]:dt_off[b + 1]], None if counts is None else counts[b], iou_fg, iou_bg) for b in range(B)]
    empty = (np.zeros(0, np.uint8), np.zeros(0, np.int32), np.zeros(0), np.zeros(0, np.uint8), np.zeros(0, np.int32), np.zeros(0))
    out = {k: np.concatenate([p[j] for p in parts] + [empty[j]]) for j, k in enumerate(("dt_code", "dt_gt", "dt_iou", "gt_code", "gt_dt", "gt_iou"))}
    out["counts"] = np.stack([p[6] for p in parts]).astype(np.int32) if B else np.zeros((0, 9), dtype=np.int32)
    return out


def _ap50(scores, tp, fp, npig):
    """AP50 x 100 of a merged list as `coco_ap.accumulate` and `_six` form it: stable merge by descending score, cumulative sums, `_sample`,
    the mean over the recall samples; NaN without a non-ignored ground truth."""
    if npig <= 0:
        return float("nan")
    order = np.argsort(-np.asarray(scores, dtype=np.float64), kind="mergesort")
    tps = np.cumsum(tp[order][None, :], axis=1, dtype=np.float64)
    fps = np.cumsum(fp[order][None, :], axis=1, dtype=np.float64)
    return ca._mean(ca._sample(tps, fps, int(npig))) * 100


def what_if(pack, codes):
    """TIDE's dAP at IoU 0.5, area `all`, from the codes of `classify` (or of the kernel) and the pack's scores ->
    {"AP50_base", "dAP50_dup", "dAP50_loc", "dAP50_bkg", "dAP50_missed"}: the base and, per cause, the changed AP50 minus the base."""
    code, dt_gt, gt_code = codes["dt_code"], codes["dt_gt"], codes["gt_code"]
    used = code != UNUSED
    scores = np.asarray(pack["dt_score"], dtype=np.float64)[used]
    code_u = code[used]
    npig = int((gt_code != GT_IGN).sum())
    tp, fp = code_u == TP, (code_u == DUP) | (code_u == LOC) | (code_u == BKG)
    base = _ap50(scores, tp, fp, npig)
    # the first LOC detection, in evaluation order, of every MISLOC ground truth becomes a true positive; every other LOC detection is ignored
    dt_off, gt_off = np.asarray(pack["dt_off"], dtype=np.int64), np.asarray(pack["gt_off"], dtype=np.int64)
    fixed = np.zeros(len(code), dtype=bool)
    for b in range(len(dt_off) - 1):
        seg = slice(int(dt_off[b]), int(dt_off[b + 1]))
        loc = np.flatnonzero(code[seg] == LOC)
        g = dt_gt[seg][loc]
        ok = g >= 0
        ok[ok] = gt_code[gt_off[b] + g[ok]] == MISLOC
        _, first = np.unique(g[ok], return_index=True)
        fixed[int(dt_off[b]) + loc[ok][first]] = True
    fixed = fixed[used]
    out = {"AP50_base": base,
           "dAP50_dup": _ap50(scores, tp, fp & (code_u != DUP), npig) - base,
           "dAP50_loc": _ap50(scores, tp | fixed, fp & (code_u != LOC), npig) - base,
           "dAP50_bkg": _ap50(scores, tp, fp & (code_u != BKG), npig) - base,
           "dAP50_missed": _ap50(scores, tp, fp, npig - int((gt_code == MISSED).sum())) - base}
    return out


def report(pack, codes, image_ids, split, threshold, iou_bg=IOU_BG, iou_fg=IOU_FG):
    """What infer.py --error_report writes to error_report_<split>.json, from the codes of one classification (host arrays) -> the dict
    {"split", "threshold", "iou_fg", "iou_bg", "max_dets", "totals", "dAP50", "rows", "order_by_dup", "order_by_loc", "order_by_bkg",
    "order_by_missed"}.  A row = one image of `image_ids` (the order the images were run): image_id, the nine counts, mean_iou_tp / mean_iou_loc of
    its detections (NaN without one); an image the pack left out -- neither ground truth nor detection -- has zeros.  order_by_*: image ids by
    descending count, ties in run order."""
    at = {int(i): b for b, i in enumerate(pack["image_ids"])}
    dt_off = np.asarray(pack["dt_off"], dtype=np.int64)
    rows = []
    for i in image_ids:
        b = at.get(int(i))
        row = {"image_id": int(i)}
        if b is None:
            row.update(dict.fromkeys(COUNT_KEYS, 0), mean_iou_tp=float("nan"), mean_iou_loc=float("nan"))
        else:
            code, iou = codes["dt_code"][dt_off[b]:dt_off[b + 1]], codes["dt_iou"][dt_off[b]:dt_off[b + 1]]
            row.update({k: int(v) for k, v in zip(COUNT_KEYS, codes["counts"][b])})
            for key, c in (("mean_iou_tp", TP), ("mean_iou_loc", LOC)):
                sel = iou[code == c]
                row[key] = float(np.cumsum(sel)[-1] / len(sel)) if len(sel) else float("nan")       # summed in evaluation order
        rows.append(row)
    order = lambda k: [r["image_id"] for r in sorted(rows, key=lambda r: -r[k])]           # noqa: E731  (sorted is stable: ties in run order)
    return {"split": split, "threshold": float(threshold), "iou_fg": float(iou_fg), "iou_bg": float(iou_bg), "max_dets": ca.MAX_DETS,
            "totals": {k: int(sum(r[k] for r in rows)) for k in COUNT_KEYS}, "dAP50": what_if(pack, codes), "rows": rows,
            "order_by_dup": order("dup"), "order_by_loc": order("loc"), "order_by_bkg": order("bkg"), "order_by_missed": order("missed")}


def metrics(rep):
    """The keys a pass's metrics gain from its report: err_dup / err_loc / err_bkg / err_misloc / err_missed (split totals) and the four dAP50_*."""
    out = {"err_" + k: rep["totals"][k] for k in ("dup", "loc", "bkg", "misloc", "missed")}
    out.update({k: rep["dAP50"][k] for k in DAP_KEYS})
    return out
