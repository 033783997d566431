"""Box AP of a prediction json against a COCO-style ground-truth json, without detectron2 / pycocotools (optional part).

The reference's offline evaluator (A2/eval_all.py:141-279, 285-312, 496-531) hands the predictions to pycocotools' `COCOeval`
(`iouType="bbox"`, `maxDets = [900, 1000, 1100]`, summary read at `maxDets[2]`) after turning each predicted `[cx, cy, w, h]` into
`[int(cx - w/2), int(cy - h/2), int(w), int(h)]` (A2/eval_all.py:165-169) and reports AP, AP50, AP75, APs, APm, APl x 100.
pycocotools is a third-party dependency that is neither vendored in the reference tree nor installed in this image (its version is
not pinned by the reference either), so this module restates its PUBLISHED algorithm (cocoeval.py: computeIoU / evaluateImg /
accumulate / summarize, bbox path, no crowd regions in FSC-147):

  * per image and category, detections by descending score (stable), at most maxDet of them; ground truths with `ignore` / `iscrowd`
    or an area outside the area range are "ignored" and sorted behind the others;
  * for each IoU threshold t in 0.50:0.05:0.95 a detection takes the still-unmatched ground truth of highest IoU >= min(t, 1 - 1e-10),
    preferring non-ignored ones (the scan stops at the first ignored ground truth once a non-ignored match is held); a detection
    matched to an ignored ground truth, or unmatched with an area outside the range, is ignored itself;
  * all images' detections merged by descending score (stable): cumulative tp / fp -> recall = tp / #non-ignored gt,
    precision = tp / (tp + fp + eps), made monotonically non-increasing from the right, sampled at the 101 recall thresholds 0:0.01:1
    with `searchsorted(recall, thr, side="left")` (0 beyond the reached recall);
  * AP = mean over thresholds and recall samples of the precision (entries of -1 = no ground truth are skipped).

PARITY UNPINNED: there is no pycocotools here to generate golden vectors from, and the reference holds no AP fixtures.  The tests
(`tests/test_coco_ap.py`) pin the restatement to hand-derived cases and to the invariants of the definition only.  It is host-side
post-processing on a json pair -- not part of the step `bench.py` measures.

ONE MATCHING, MANY READERS (`Matching`): the flags of a matching -- matched, det_ignored [A, T, D], npig [A, B], images side by side in
`pack_images` order -- are a value.  `Matching.of(gt, dt)` makes it with the host code below (`_evaluate_image`, untouched: the checker),
`Matching.of(gt, dt, device)` / `Matching.launch(pack, device)` with ONE `cdetr_coco_match` launch (csrc/coco_eval.hip) whose flags stay on
the device, `match_store` from an ops.DetectionStore (`pack_store` packs only the ground truths; the detections are read where
cdetr_emit_detections, csrc/detections.hip, left them in evaluation order) and `match_predictions` from a predictions dict as written.  Its
readings: `host()` (the flags in one copy, taken once), `six()` (`accumulate` = the tail of `average_precision` as array operations, the same
float64 operations in the same order: EQUAL numbers), `six_sweep(thresholds)`, `stats(cuts, counts)`, `errors(counts)` and `row50()` (render.py's overlays).
`summarize(device=)`, `summarize_store`, `summarize_store_sweep`, `image_stats` and `image_stats_store` are one maker and one reading each
(tests/test_matching_cpu.py, test_coco_ap_device_gpu.py, test_detections_gpu.py).

SCORE-THRESHOLD SWEEP (`six_sweep`, infer.py --sweep_thresholds): the six numbers at several score thresholds from ONE matching at the lowest of
them -- in evaluation order the detections a higher threshold keeps are a prefix, per image and after the merge, and a greedy match never
looks ahead (`accumulate_sweep`).  `summarize_sweep` filters and evaluates once per threshold on the host: slow, and the
checker (tests/test_threshold_sweep_cpu.py, _gpu.py).

PER-IMAGE STATISTICS (`stats`, infer.py --image_report): the list the reference's evaluator keeps per image (A2/eval_all.py:227-239, its `ap`
field left empty at line 181) and the counts behind COCOevalMaxDets.summarize's stats[6..11], AR at maxDets 900 / 1000 / 1100 and AR small /
medium / large.  The first `c` detections of an image are an evaluation at max_det = c (COCOeval matches once and slices afterwards), and an
image's own AP is `_sample` on its own list.  `stats_from_flags` states that in numpy and is the checker; device flags go through ONE
cdetr_coco_image_stats launch (csrc/coco_report.hip) where they lie: EQUAL numbers, the average precisions bit for bit
(tests/test_image_report_cpu.py, _gpu.py).  `average_recall`, `image_rows` and `image_report` turn the statistics into what is
printed and written.

ERROR BREAKDOWN (`errors`, infer.py --error_report): WHY a detection failed -- duplicate, localisation, background, missed -- as one more reading of a
`Matching`: counting_detr_amd/error_report.py states the rule in numpy (host flags), device flags go through ONE cdetr_coco_errors launch
(csrc/error_report.hip) on the boxes where they lie: EQUAL codes, the IoUs bit for bit (tests/test_error_report_cpu.py, _gpu.py).

BOOTSTRAP REPLICATES (`bootstrap`, infer.py --bootstrap R): HOW FAR the six numbers move when the images are resampled, as one more reading of a `Matching`:
counting_detr_amd/bootstrap.py states the rule in numpy (host flags) -- every detection accumulated once with its image's multiplicity as weight, which EQUALS
`accumulate` on the repeated lists --, device flags are packed where they lie by ONE cdetr_bootstrap_gather launch and the replicates run in cdetr_bootstrap_ap
(csrc/bootstrap.hip), one copy back per launch: EQUAL numbers (tests/test_bootstrap_cpu.py, _gpu.py).
"""
import json

import numpy as np

IOU_THRS = np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1, endpoint=True)
REC_THRS = np.linspace(0.0, 1.0, int(np.round((1.0 - 0.0) / 0.01)) + 1, endpoint=True)
AREA_RNG = {"all": (0.0, 1e5 ** 2), "small": (0.0, 32.0 ** 2), "medium": (32.0 ** 2, 96.0 ** 2), "large": (96.0 ** 2, 1e5 ** 2)}
MAX_DETS = 1100          # A2/eval_all.py:511-512: maxDets = [900, 1000, 1100], AP summarised at the last one
MAX_DET_CUTS = (900, 1000, 1100)        # COCOeval's maxDets: its AR numbers are read at each, its AP at the last


def reference_box(b):
    """[cx, cy, w, h] of the prediction json -> the [x, y, w, h] ints the reference feeds to COCOeval (A2/eval_all.py:165-169)."""
    cx, cy, w, h = b
    return [int(cx - w / 2), int(cy - h / 2), int(w), int(h)]


def box_iou_xywh(dt, gt, device=None):
    """IoU matrix [len(dt), len(gt)] of xywh boxes (pycocotools maskApi bbIou, no crowd).  `device`: a CUDA device = the same matrix, bit for
    bit, from cdetr_box_iou_xywh."""
    dt = np.asarray(dt, dtype=np.float64).reshape(-1, 4)
    gt = np.asarray(gt, dtype=np.float64).reshape(-1, 4)
    if device is not None:
        import torch
        from . import ops
        with torch.cuda.device(_cuda(device)):
            return ops.box_iou_xywh(torch.from_numpy(dt).to(device), torch.from_numpy(gt).to(device)).cpu().numpy()
    if len(dt) == 0 or len(gt) == 0:
        return np.zeros((len(dt), len(gt)))
    da, ga = dt[:, 2] * dt[:, 3], gt[:, 2] * gt[:, 3]
    w = np.minimum(dt[:, None, 0] + dt[:, None, 2], gt[None, :, 0] + gt[None, :, 2]) - np.maximum(dt[:, None, 0], gt[None, :, 0])
    h = np.minimum(dt[:, None, 1] + dt[:, None, 3], gt[None, :, 1] + gt[None, :, 3]) - np.maximum(dt[:, None, 1], gt[None, :, 1])
    inter = np.clip(w, 0, None) * np.clip(h, 0, None)
    union = da[:, None] + ga[None, :] - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = np.where(union > 0, inter / union, 0.0)
    return iou


def _evaluate_image(dts, gts, area_rng, max_det):
    """One (image, category, area range): -> (scores [D], matched [T, D] bool, det_ignored [T, D] bool, number of non-ignored gt)."""
    g_ig = np.array([bool(g.get("ignore", 0)) or bool(g.get("iscrowd", 0)) or g["area"] < area_rng[0] or g["area"] > area_rng[1] for g in gts],
                    dtype=bool)
    g_order = np.argsort(g_ig, kind="mergesort")                        # non-ignored first, original order otherwise
    gts = [gts[i] for i in g_order]
    g_ig = g_ig[g_order]
    d_order = np.argsort([-d["score"] for d in dts], kind="mergesort")[:max_det]
    dts = [dts[i] for i in d_order]
    ious = box_iou_xywh([d["bbox"] for d in dts], [g["bbox"] for g in gts])
    T, D, G = len(IOU_THRS), len(dts), len(gts)
    gtm = -np.ones((T, G), dtype=np.int64)
    dtm = -np.ones((T, D), dtype=np.int64)
    dt_ig = np.zeros((T, D), dtype=bool)
    for ti, t in enumerate(IOU_THRS):
        for di in range(D):
            best, m = min(t, 1 - 1e-10), -1
            for gi in range(G):
                if gtm[ti, gi] >= 0:                                    # taken (no crowd regions here)
                    continue
                if m > -1 and not g_ig[m] and g_ig[gi]:                 # holding a real match: ignored ones cannot replace it
                    break
                if ious[di, gi] < best:
                    continue
                best, m = ious[di, gi], gi
            if m == -1:
                continue
            dt_ig[ti, di] = g_ig[m]
            dtm[ti, di] = m
            gtm[ti, m] = di
    d_area = np.array([d.get("area", d["bbox"][2] * d["bbox"][3]) for d in dts], dtype=np.float64)
    out_of_range = (d_area < area_rng[0]) | (d_area > area_rng[1])
    dt_ig = dt_ig | ((dtm < 0) & out_of_range[None, :])
    return np.array([d["score"] for d in dts], dtype=np.float64), dtm >= 0, dt_ig, int((~g_ig).sum())


def pack_images(gt_by_img, dt_by_img, max_det=MAX_DETS):
    """The dict form of `average_precision`'s inputs -> packed arrays for `cdetr_coco_match` (host work, no device needed).  Images in
    sorted-id order, those with neither ground truth nor detection left out (as `average_precision` skips them); image b owns ground truths
    gt_off[b]:gt_off[b + 1] (original order) and detections dt_off[b]:dt_off[b + 1], the latter in EVALUATION order: descending score,
    stable (equal scores keep their input order), cut at `max_det` -- the `d_order` of `_evaluate_image`.
    -> dict: image_ids, gt_boxes f64 [G, 4], gt_area f64 [G], gt_ignore u8 [G] (ignore or iscrowd), gt_off i32 [B + 1], dt_boxes f64 [D, 4],
    dt_area f64 [D], dt_score f64 [D], dt_off i32 [B + 1], g_max (largest ground-truth count of one image)."""
    ids = [i for i in sorted(set(gt_by_img) | set(dt_by_img)) if gt_by_img.get(i) or dt_by_img.get(i)]
    gts = [gt_by_img.get(i, []) for i in ids]
    dts = []
    for i in ids:
        d = dt_by_img.get(i, [])
        dts.append([d[j] for j in np.argsort([-x["score"] for x in d], kind="mergesort")[:max_det]])
    flat_d = [d for dl in dts for d in dl]
    return {"image_ids": ids, **_pack_gts(gts),
            "dt_boxes": np.array([d["bbox"] for d in flat_d], dtype=np.float64).reshape(-1, 4),
            "dt_area": np.array([d.get("area", d["bbox"][2] * d["bbox"][3]) for d in flat_d], dtype=np.float64),
            "dt_score": np.array([d["score"] for d in flat_d], dtype=np.float64),
            "dt_off": np.concatenate([[0], np.cumsum([len(dl) for dl in dts])]).astype(np.int32)}


def _pack_gts(gts):
    """The ground-truth half of `pack_images`: the images' lists, in evaluation order of the images -> gt_boxes, gt_area, gt_ignore, gt_off, g_max."""
    flat_g = [g for gl in gts for g in gl]
    return {"gt_boxes": np.array([g["bbox"] for g in flat_g], dtype=np.float64).reshape(-1, 4),
            "gt_area": np.array([g["area"] for g in flat_g], dtype=np.float64),
            "gt_ignore": np.array([bool(g.get("ignore", 0)) or bool(g.get("iscrowd", 0)) for g in flat_g], dtype=np.uint8),
            "gt_off": np.concatenate([[0], np.cumsum([len(gl) for gl in gts])]).astype(np.int32),
            "g_max": max([len(gl) for gl in gts], default=0)}


def accumulate(scores, matched, ignored, npig):
    """The tail of `average_precision` as array operations: all images' detections (scores [N], flags [T, N], images concatenated in
    `pack_images` order) merged by descending score (stable), cumulative tp / fp, precision envelope = running maximum from the right,
    sampled at the 101 recall thresholds.  Same float64 operations in the same order as the loops there: the result is EQUAL, not close."""
    if npig == 0:
        return -np.ones((len(IOU_THRS), len(REC_THRS)))
    return _sample(*_merged_cumulative(scores, matched, ignored)[1:], npig)


def _merged_cumulative(scores, matched, ignored):
    """The head of `accumulate`: -> (scores in merged order [N], cumulative tp [T, N], cumulative fp [T, N]), float64.  The sums count flags, so
    a column prefix of them IS the cumulative sum of that prefix of the merged list (`accumulate_sweep`)."""
    T = len(IOU_THRS)
    scores = np.asarray(scores, dtype=np.float64)
    order = np.argsort(-scores, kind="mergesort")
    matched = np.asarray(matched, dtype=bool).reshape(T, -1)[:, order]
    ignored = np.asarray(ignored, dtype=bool).reshape(T, -1)[:, order]
    return (scores[order], np.cumsum(matched & ~ignored, axis=1, dtype=np.float64), np.cumsum(~matched & ~ignored, axis=1, dtype=np.float64))


def _sample(tps, fps, npig):
    """The tail of `accumulate`, shared with `accumulate_sweep`: cumulative tp / fp [T, N] of a merged list and its npig > 0 -> precision
    [T, R]: recall and precision, the envelope from the right, the 101-point sampling (zeros for an empty list)."""
    T, R = tps.shape[0], len(REC_THRS)
    precision = np.zeros((T, R))
    N = tps.shape[1]
    if N == 0:
        return precision
    rc = tps / npig
    pr = tps / (fps + tps + np.spacing(1))
    pr = np.maximum.accumulate(pr[:, ::-1], axis=1)[:, ::-1]
    for t in range(T):                                                     # thresholds, not detections: searchsorted is one-dimensional
        inds = np.searchsorted(rc[t], REC_THRS, side="left")
        precision[t] = np.where(inds < N, pr[t][np.minimum(inds, N - 1)], 0.0)
    return precision


def _cuda(device):
    import torch
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"coco_ap: device={device} -- the device path runs HIP kernels (device=None is the host path)")
    return device


class Matching:
    """The result of ONE matching over one pack: `pack` (`pack_images` / `pack_store`), the area ranges `areas` it was matched under and
    `_evaluate_image`'s flags, images side by side: matched, det_ignored [A, T, D] and npig [A, B] -- device tensors where the cdetr_coco_match
    launch left them (`device`: that CUDA device) or numpy arrays from the host matcher (`device` None).  `image_ids`: the images in the
    caller's own order (a store's), in which prefix lengths `counts` are given; the pack's by default.  Every reading below is of these flags:
    nothing is matched twice, and the flags come to the host at most once."""

    def __init__(self, pack, areas, matched, det_ignored, npig, image_ids=None):
        self.pack, self.areas, self.matched, self.det_ignored, self.npig = pack, tuple(areas), matched, det_ignored, npig
        self.image_ids = pack["image_ids"] if image_ids is None else image_ids
        self.device = None if isinstance(matched, np.ndarray) else matched.device
        self._host = (matched, det_ignored, npig) if self.device is None else None

    @classmethod
    def of(cls, gt_by_img, dt_by_img, device=None, areas=tuple(AREA_RNG), max_det=MAX_DETS):
        """The dicts of `average_precision` matched by the host matcher (`device` None: `_evaluate_image` per image and area range, the flags
        concatenated in `pack_images` order) or on a CUDA device (`launch`)."""
        pack, T = pack_images(gt_by_img, dt_by_img, max_det), len(IOU_THRS)
        if device is not None:
            return cls.launch(pack, device, areas)
        ids = pack["image_ids"]
        per = [[_evaluate_image(dt_by_img.get(i, []), gt_by_img.get(i, []), AREA_RNG[a], max_det) for i in ids] for a in areas]
        cat = lambda k: np.stack([np.concatenate([e[k].reshape(T, -1) for e in row] + [np.zeros((T, 0), dtype=bool)], axis=1) for row in per])   # noqa: E731
        return cls(pack, areas, cat(1), cat(2), np.array([[e[3] for e in row] for row in per], dtype=np.int64).reshape(len(areas), len(ids)))

    @classmethod
    def launch(cls, pack, device, areas=tuple(AREA_RNG), events=None, image_ids=None):
        """ONE `cdetr_coco_match` launch for every image of `pack` under the area ranges `areas`; nothing is copied back.  `events`: a pair of
        torch.cuda.Event recorded around the launch.  A pack that carries "dt_device" = (boxes f64 [D, 4], area f64 [D]) device tensors
        (`pack_store`) has its detections read from there; its dt_boxes / dt_area are not used.  A pack without an image launches nothing: empty
        host flags."""
        import torch
        from . import ops
        device = _cuda(device)
        A, T, B = len(areas), len(IOU_THRS), len(pack["image_ids"])
        dt_dev = pack.get("dt_device")
        if B == 0:
            return cls(pack, areas, np.zeros((A, T, 0), dtype=bool), np.zeros((A, T, 0), dtype=bool), np.zeros((A, 0), dtype=np.int64), image_ids)
        thrs = np.minimum(IOU_THRS, 1 - 1e-10)
        rng = np.array([AREA_RNG[a] for a in areas], dtype=np.float64).reshape(-1)
        G = len(pack["gt_area"])
        dt_host = (pack["dt_boxes"].reshape(-1), pack["dt_area"]) if dt_dev is None else (np.zeros(0), np.zeros(0))
        f64 = np.concatenate([pack["gt_boxes"].reshape(-1), pack["gt_area"], dt_host[0], dt_host[1], thrs, rng])
        i32 = np.concatenate([pack["gt_off"], pack["dt_off"]]).astype(np.int32)
        with torch.cuda.device(device):
            f = torch.from_numpy(f64).to(device)
            i = torch.from_numpy(i32).to(device)
            ig = torch.from_numpy(pack["gt_ignore"]).to(device)
            cuts = np.cumsum([0, 4 * G, G, len(dt_host[0]), len(dt_host[1]), T, 2 * A])
            gt_boxes, gt_area, dt_boxes, dt_area, d_thrs, d_rng = (f[cuts[k]:cuts[k + 1]] for k in range(6))
            if dt_dev is not None:
                dt_boxes, dt_area = dt_dev[0].reshape(-1), dt_dev[1]
            flags = ops.coco_match(gt_boxes, gt_area, ig, i[:B + 1], dt_boxes, dt_area, i[B + 1:], d_thrs, d_rng, int(pack["g_max"]), events=events)
        return cls(pack, areas, *flags, image_ids)

    def host(self):
        """-> (matched [A, T, D] bool, det_ignored [A, T, D] bool, npig [A, B] int) on the host: a launch's flags come in ONE copy of its single
        buffer, taken at the first call and kept."""
        if self._host is None:
            from . import ops
            self._host = ops.coco_flags_host(self.matched, self.det_ignored, self.npig)
        return self._host

    def precisions(self):
        """-> precision [T, R] per area range (`accumulate`)."""
        matched, ignored, npig = self.host()
        return [accumulate(self.pack["dt_score"], matched[a], ignored[a], int(npig[a].sum())) for a in range(len(self.areas))]

    def six(self):
        """-> the six numbers of `summarize` (a matching under the four ranges of AREA_RNG)."""
        return _six(dict(zip(self.areas, self.precisions())))

    def six_sweep(self, thresholds):
        """-> the six numbers per score threshold (`summarize_flags_sweep`: the detections a threshold keeps are a prefix, checked)."""
        matched, ignored, npig = self.host()
        return summarize_flags_sweep(self.pack["dt_score"], {a: (matched[k], ignored[k], int(npig[k].sum())) for k, a in enumerate(self.areas)}, thresholds)

    def pack_counts(self, counts):
        """Prefix lengths per image of `image_ids` (or None: whole segments) -> per image of the pack, 0 for an image `image_ids` does not name."""
        if counts is None:
            return None
        slot = {int(i): k for k, i in enumerate(self.image_ids)}
        return [int(counts[slot[i]]) if i in slot else 0 for i in self.pack["image_ids"]]

    def stats(self, cuts=MAX_DET_CUTS, counts=None):
        """-> the per-image statistics of `image_stats`, of the first counts[k] detections of image k of `image_ids` where `counts` is given.
        Host flags: `stats_from_flags`.  Device flags: ONE cdetr_coco_image_stats launch on them where they lie and one copy of the statistics
        back (and the 4 B ints of npig, unless the flags' host copy is there already)."""
        pack, counts = self.pack, self.pack_counts(counts)
        if self.device is None:
            matched, ignored, npig = self._host
            return _stats_dict(pack["image_ids"], *stats_from_flags(matched, ignored, pack["dt_off"], npig, cuts, counts), npig, cuts)
        import torch
        from . import ops
        npig = self._host[2] if self._host is not None else self.npig.cpu().numpy()
        B, M = len(pack["image_ids"]), len(cuts)
        i32 = np.concatenate([pack["dt_off"], np.asarray(cuts, dtype=np.int64), np.asarray([] if counts is None else counts, dtype=np.int64)])
        with torch.cuda.device(self.device):
            i = torch.from_numpy(i32.astype(np.int32)).to(self.device)
            rec = torch.from_numpy(REC_THRS).to(self.device)
            tp, fp, ap = ops.coco_image_stats(self.matched, self.det_ignored, i[:B + 1], self.npig, i[B + 1:B + 1 + M], rec,
                                              dt_cnt=None if counts is None else i[B + 1 + M:], host=True)
        return _stats_dict(pack["image_ids"], tp, fp, ap, npig, cuts)

    def errors(self, counts=None, iou_bg=0.1):
        """-> the codes of error_report.classify (a dict of host arrays) for the pack, at area range `all` and IoU IOU_THRS[0], of the first
        counts[k] detections of image k of `image_ids` where `counts` is given.  Host flags: the numpy rule itself.  Device flags: ONE
        cdetr_coco_errors launch (csrc/error_report.hip) on the boxes where they lie -- a store's detections are not moved, the packed ground
        truths go up again -- and one copy of the codes back: EQUAL arrays, the IoUs bit for bit."""
        from . import error_report as er
        pack, counts = self.pack, self.pack_counts(counts)
        if self.device is None:
            return er.classify(pack, counts, iou_bg)
        import torch
        from . import ops
        B, G = len(pack["image_ids"]), len(pack["gt_area"])
        dt_dev = pack.get("dt_device")
        dt_host = (pack["dt_boxes"].reshape(-1), pack["dt_area"]) if dt_dev is None else (np.zeros(0), np.zeros(0))
        f64 = np.concatenate([pack["gt_boxes"].reshape(-1), pack["gt_area"], dt_host[0], dt_host[1]])
        i32 = np.concatenate([pack["gt_off"], pack["dt_off"], np.asarray([] if counts is None else counts, dtype=np.int64)]).astype(np.int32)
        with torch.cuda.device(self.device):
            f = torch.from_numpy(f64).to(self.device)
            i = torch.from_numpy(i32).to(self.device)
            ig = torch.from_numpy(pack["gt_ignore"]).to(self.device)
            cuts = np.cumsum([0, 4 * G, G, len(dt_host[0]), len(dt_host[1])])
            gt_boxes, gt_area, dt_boxes, dt_area = (f[cuts[k]:cuts[k + 1]] for k in range(4))
            if dt_dev is not None:
                dt_boxes, dt_area = dt_dev[0].reshape(-1), dt_dev[1]
            return ops.coco_errors(gt_boxes, gt_area, ig, i[:B + 1], dt_boxes, dt_area, i[B + 1:2 * B + 2], int(pack["g_max"]), er.IOU_FG, iou_bg,
                                   AREA_RNG["all"], dt_cnt=None if counts is None else i[2 * B + 2:], host=True)

    def bootstrap(self, R, seed=0, counts=None, mult=None, chunk=None):
        """-> float64 [R, 6]: AP, AP50, AP75, APs, APm, APl (x 100, NaN where undefined) of R bootstrap replicates over the images of
        `image_ids` (counting_detr_amd/bootstrap.py states the rule; replicate r draws the same images as every other metric's replicate r),
        of the first counts[k] detections of image k where `counts` is given.  Host flags: the numpy rule, slow.  Device flags: the merged order
        goes up once, ONE cdetr_bootstrap_gather launch packs the flags where they lie and cdetr_bootstrap_ap (csrc/bootstrap.hip) runs the
        replicates, one copy back per launch of `chunk` replicates: EQUAL numbers.  `mult`: int [R, N] multiplicities in place of the draws
        (tests)."""
        from . import bootstrap as bs
        R, seed = bs.check_args(R, seed)
        pack, N, A = self.pack, len(self.image_ids), len(self.areas)
        if self.areas != tuple(AREA_RNG):
            raise RuntimeError(f"coco_ap: the six numbers need a matching under {tuple(AREA_RNG)}, this one has {self.areas}")
        slot = {int(i): k for k, i in enumerate(self.image_ids)}
        if any(i not in slot for i in pack["image_ids"]):
            raise RuntimeError("coco_ap: the pack holds images that `image_ids` does not name: the replicates draw from `image_ids`")
        if N == 0:
            return np.full((R, len(bs.AP_KEYS)), np.nan)
        at = np.array([slot[i] for i in pack["image_ids"]], dtype=np.int64)
        order, image = bs.prepare(pack["dt_score"], pack["dt_off"], self.pack_counts(counts))
        image = at[image] if len(image) else image
        if mult is not None:
            mult = np.asarray(mult, dtype=np.int64).reshape(R, N)
        if self.device is None:
            matched, ignored, npig = self._host
            npig_n = np.zeros((A, N), dtype=np.int64)
            npig_n[:, at] = npig
            m = bs.multiplicities(seed, R, N) if mult is None else mult
            return bs.six_table(bs.ap_precisions(bs.flag_words(matched, ignored, order), image, npig_n, m), self.areas)
        import torch
        from . import ops
        with torch.cuda.device(self.device):
            i = torch.from_numpy(np.concatenate([order, image, at]).astype(np.int32)).to(self.device)
            P, B = len(order), len(at)
            npig_n = self.npig
            if B != N or not np.array_equal(at, np.arange(N)):
                npig_n = torch.zeros((A, N), dtype=torch.int32, device=self.device)
                npig_n[:, i[2 * P:].long()] = self.npig
            words = ops.bootstrap_gather(self.matched, self.det_ignored, i[:P])
            rec = torch.from_numpy(REC_THRS).to(self.device)
            dm = None if mult is None else torch.from_numpy(mult.astype(np.int32)).to(self.device)
            return bs.six_table(ops.bootstrap_ap(words, i[P:2 * P], npig_n, rec, R, seed, mult=dm, chunk=chunk), self.areas)

    def row50(self):
        """-> (matched, det_ignored) [D] at area range `all`, IoU 0.5, row [0, 0] of the flags, for the renderer: views of the device tensors
        (no copy), or arrays."""
        return self.matched[0, 0], self.det_ignored[0, 0]


def match_on_device(pack, device, areas=("all", "small", "medium", "large"), events=None):
    """`Matching.launch` and its flags on the host -> (matched [A, T, D] bool, det_ignored [A, T, D] bool, npig [A, B] int)."""
    return Matching.launch(pack, device, areas, events).host()


def _device_precisions(gt_by_img, dt_by_img, areas, max_det, device):
    return Matching.of(gt_by_img, dt_by_img, device, areas, max_det).precisions()


def average_precision(gt_by_img, dt_by_img, area="all", max_det=MAX_DETS, device=None):
    """`precision[T, R]` (COCOeval.eval["precision"][:, :, k, a, m]) for one category; -1 everywhere when there is no ground truth.
    gt_by_img / dt_by_img: {image_id: [ {bbox: xywh, area, (iscrowd), (ignore)} ]} / {image_id: [ {bbox: xywh, score} ]}.
    `device`: a CUDA device = the matching on the device (one launch for all images), the same array."""
    if device is not None:
        return _device_precisions(gt_by_img, dt_by_img, (area,), max_det, device)[0]
    rng = AREA_RNG[area]
    scores, matched, ignored, npig = [], [], [], 0
    for img in sorted(set(gt_by_img) | set(dt_by_img)):
        g, d = gt_by_img.get(img, []), dt_by_img.get(img, [])
        if not g and not d:
            continue
        s, m, ig, n = _evaluate_image(d, g, rng, max_det)
        scores.append(s); matched.append(m); ignored.append(ig)
        npig += n
    T, R = len(IOU_THRS), len(REC_THRS)
    precision = -np.ones((T, R))
    if npig == 0:
        return precision
    scores = np.concatenate(scores) if scores else np.zeros(0)
    order = np.argsort(-scores, kind="mergesort")
    matched = np.concatenate(matched, axis=1)[:, order] if matched else np.zeros((T, 0), dtype=bool)
    ignored = np.concatenate(ignored, axis=1)[:, order] if ignored else np.zeros((T, 0), dtype=bool)
    tps = np.cumsum(matched & ~ignored, axis=1, dtype=np.float64)
    fps = np.cumsum(~matched & ~ignored, axis=1, dtype=np.float64)
    for t in range(T):
        tp, fp = tps[t], fps[t]
        rc = tp / npig
        pr = tp / (fp + tp + np.spacing(1))
        q = np.zeros(R)
        pr = pr.tolist()
        for i in range(len(pr) - 1, 0, -1):                             # precision envelope
            if pr[i] > pr[i - 1]:
                pr[i - 1] = pr[i]
        inds = np.searchsorted(rc, REC_THRS, side="left")
        for ri, pi in enumerate(inds):
            if pi < len(pr):
                q[ri] = pr[pi]
        precision[t] = q
    return precision


def _mean(p):
    p = p[p > -1]
    return float(np.mean(p)) if p.size else -1.0


def _six(by_area):
    """precision[T, R] per area range -> the six reported numbers (x 100, NaN when undefined)."""
    p_all = by_area["all"]
    vals = {"AP": _mean(p_all), "AP50": _mean(p_all[np.isclose(IOU_THRS, 0.5)]), "AP75": _mean(p_all[np.isclose(IOU_THRS, 0.75)]),
            "APs": _mean(by_area["small"]), "APm": _mean(by_area["medium"]), "APl": _mean(by_area["large"])}
    return {k: (v * 100 if v >= 0 else float("nan")) for k, v in vals.items()}


def summarize(gt_by_img, dt_by_img, max_det=MAX_DETS, device=None):
    """The six numbers of A2/eval_all.py:331 (x 100, NaN when undefined): AP, AP50, AP75, APs, APm, APl.
    `device`: a CUDA device = all four area ranges matched in one launch, the same six numbers."""
    if device is not None:
        by_area = dict(zip(AREA_RNG, _device_precisions(gt_by_img, dt_by_img, tuple(AREA_RNG), max_det, device)))
    else:
        by_area = {area: average_precision(gt_by_img, dt_by_img, area, max_det) for area in AREA_RNG}
    return _six(by_area)


def pack_store(gt_by_img, store, image_ids):
    """`pack_images` for detections that are already on the device in evaluation order (an ops.DetectionStore; image k of the store is
    `image_ids[k]`): the ground truths are packed on the host, the detections stay where they are.  Images in sorted-id order, those with neither
    ground truth nor detection left out, exactly as `pack_images` orders them; when that is not the store's own order the segments are
    gathered on the device with an index built from the store's offsets.  -> the pack of `match_on_device` with "dt_device" (and dt_score, dt_off
    on the host; no dt_boxes / dt_area)."""
    import torch
    host = store.finish()                                                  # the one copy (cached by the store)
    image_ids = [int(i) for i in image_ids]
    if len(image_ids) != store.first or len(set(image_ids)) != len(image_ids):
        raise RuntimeError(f"coco_ap: {len(image_ids)} image ids ({len(set(image_ids))} distinct) for a store of {store.first} images")
    off = host["eval_off"].astype(np.int64)
    slot = {i: k for k, i in enumerate(image_ids)}
    n_dt = lambda i: int(off[slot[i] + 1] - off[slot[i]]) if i in slot else 0                                  # noqa: E731
    ids = [i for i in sorted(set(gt_by_img) | set(image_ids)) if gt_by_img.get(i) or n_dt(i)]
    segs = [(int(off[slot[i]]), int(off[slot[i] + 1])) for i in ids if i in slot and n_dt(i)]
    E = int(off[store.first])
    in_place = sum(hi - lo for lo, hi in segs) == E and all(a[1] == b[0] for a, b in zip(segs, segs[1:])) and (not segs or segs[0][0] == 0)
    boxes, area, score = store.eval_boxes[:E], store.eval_area[:E], host["eval_score"]
    if not in_place:
        idx = np.concatenate([np.arange(lo, hi) for lo, hi in segs]) if segs else np.zeros(0, dtype=np.int64)
        di = torch.from_numpy(idx).to(store.buf.device)
        boxes, area = boxes.index_select(0, di), area.index_select(0, di)
        score = score[idx]
    return {"image_ids": ids, **_pack_gts([gt_by_img.get(i, []) for i in ids]), "dt_device": (boxes.contiguous(), area.contiguous()),
            "dt_score": np.ascontiguousarray(score), "dt_off": np.concatenate([[0], np.cumsum([n_dt(i) for i in ids])]).astype(np.int32)}


def match_store(gt_by_img, store, image_ids, device=None, max_det=MAX_DETS, sweep=None):
    """The ONE matching of an ops.DetectionStore filled by cdetr_emit_detections (infer.py --device_detections) -> a `Matching` under the four
    area ranges: the evaluation records go to cdetr_coco_match straight from device memory.  `image_ids[k]` = the image id of the store's image
    k (the order of `counts` in `Matching.stats`); `gt_by_img` as for `summarize` (`gt_from_json`); `device`: the store's own (default).
    `sweep`: the score thresholds a sweep will ask of the matching (`Matching.six_sweep`), refused here, before any device work, unless the
    store was emitted at the lowest of them."""
    if sweep is not None:
        t32 = np.asarray(list(sweep), dtype=np.float64).astype(np.float32)
        if len(t32) == 0 or np.isnan(t32).any() or np.float32(store.threshold) != t32.min():
            raise RuntimeError(f"coco_ap: a sweep over {t32.tolist()} needs a store emitted at its lowest threshold, this one was emitted at "
                               f"{store.threshold}")
    if store.max_det != max_det:
        raise RuntimeError(f"coco_ap: the store was cut at max_det = {store.max_det}, the summary asks for {max_det}")
    device = store.buf.device if device is None else _cuda(device)
    return Matching.launch(pack_store(gt_by_img, store, image_ids), device, image_ids=image_ids)


def summarize_store(gt_by_img, store, image_ids, device=None, max_det=MAX_DETS):
    """`summarize(..., device=)` for an ops.DetectionStore: the same six numbers as `ap_from_json(device=)` gives on the predictions json written
    from that store, without the json trip (`match_store`)."""
    return match_store(gt_by_img, store, image_ids, device, max_det).six()


def accumulate_sweep(scores, matched, ignored, npig, thresholds):
    """`accumulate` for every score threshold of `thresholds` from the flags of ONE matching at (or below) the lowest of them -> a list of
    precision [T, R].  In evaluation order the detections kept at threshold t are a prefix of every image's list (descending score, cut at
    max_det: min(count_t, max_det) of them), the greedy matching gives detection k flags that depend on the detections before it only, and
    the stable merge by score keeps the kept ones a prefix again: the first n_t = #{score >= float32(t)} columns of the cumulative sums.
    Only the envelope and the sampling (`_sample`) run per threshold."""
    if npig == 0:
        return [-np.ones((len(IOU_THRS), len(REC_THRS))) for _ in thresholds]
    merged, tps, fps = _merged_cumulative(scores, matched, ignored)
    s32 = merged.astype(np.float32)                     # the scores are fp32 probabilities widened: the cast is exact
    out = []
    for t in thresholds:
        n_t = int((s32 >= np.float32(t)).sum())
        if n_t and not (s32[:n_t] >= np.float32(t)).all():
            raise RuntimeError("coco_ap: the detections kept at a threshold are not a prefix of the merged list (NaN scores?)")
        out.append(_sample(tps[:, :n_t], fps[:, :n_t], npig))
    return out


def summarize_sweep(gt_by_img, dt_by_img, thresholds, max_det=MAX_DETS):
    """The six numbers per score threshold on the host, the slow and obvious way (the checker of `summarize_store_sweep`): `summarize` on
    the detections with float32(score) >= float32(t), once per threshold.  -> list of dicts, in the order of `thresholds`."""
    out = []
    for t in thresholds:
        t32 = np.float32(t)
        kept = {i: [d for d in dl if np.float32(d["score"]) >= t32] for i, dl in dt_by_img.items()}
        out.append(summarize(gt_by_img, kept, max_det=max_det))
    return out


def summarize_flags_sweep(scores, flags, thresholds):
    """The prefix route's summary: `flags` = {area: (matched [T, D], det_ignored [T, D], npig)} of one matching at the lowest threshold,
    `scores` [D] in the same (images concatenated) order -> the six numbers per threshold."""
    per_area = {a: accumulate_sweep(scores, m, ig, int(n), thresholds) for a, (m, ig, n) in flags.items()}
    return [_six({a: per_area[a][k] for a in per_area}) for k in range(len(thresholds))]


def summarize_store_sweep(gt_by_img, store, image_ids, thresholds, device=None, max_det=MAX_DETS):
    """`summarize_store` at every score threshold of `thresholds` from ONE cdetr_coco_match launch: the store was emitted at the lowest
    threshold (checked), the flags of every higher one are a prefix of what that launch returns (`accumulate_sweep`).  -> list of the six
    numbers, in the order of `thresholds`; each EQUALS `summarize_store` on a store emitted at that threshold."""
    return match_store(gt_by_img, store, image_ids, device, max_det, sweep=thresholds).six_sweep(thresholds)


# ------------------------------------------------------------------------------------------------- per-image statistics and average recall
def stats_from_flags(matched, ignored, dt_off, npig, cuts, counts=None):
    """The definition of cdetr_coco_image_stats in numpy (host only: the checker).  matched / ignored [A, T, D] of ONE matching (images side by
    side, image b owns dt_off[b]:dt_off[b + 1], evaluation order), npig [A, B], `cuts` = maxDets cuts, `counts` [B] = use only the first
    min(counts[b], segment) detections of image b.  -> tp, fp int32 [A, B, T, M]: true / false positives among the first min(cut, n) detections
    of the image -- COCOeval matches once over dt[:maxDets[-1]] and slices [:, :maxDet] afterwards, so these are the counts of an evaluation at
    max_det = cut --; ap float64 [A, B, T]: the image's OWN average precision (`_sample` on its own list, the R samples summed in index order),
    -1 where the image has no non-ignored ground truth."""
    matched, ignored = np.asarray(matched, dtype=bool), np.asarray(ignored, dtype=bool)
    A, T, _ = matched.shape
    dt_off = np.asarray(dt_off, dtype=np.int64)
    B, M, R = len(dt_off) - 1, len(cuts), len(REC_THRS)
    npig = np.asarray(npig).reshape(A, B)
    tp, fp, ap = np.zeros((A, B, T, M), dtype=np.int32), np.zeros((A, B, T, M), dtype=np.int32), -np.ones((A, B, T))
    for b in range(B):
        lo, n = int(dt_off[b]), int(dt_off[b + 1] - dt_off[b])
        if counts is not None:
            n = min(n, max(int(counts[b]), 0))
        for a in range(A):
            m, ig = matched[a, :, lo:lo + n], ignored[a, :, lo:lo + n]
            tps, fps = np.cumsum(m & ~ig, axis=1, dtype=np.float64), np.cumsum(~m & ~ig, axis=1, dtype=np.float64)
            for k, c in enumerate(cuts):
                c = min(max(int(c), 0), n)
                if c:
                    tp[a, b, :, k], fp[a, b, :, k] = tps[:, c - 1], fps[:, c - 1]
            if npig[a, b] > 0:
                ap[a, b] = np.cumsum(_sample(tps, fps, int(npig[a, b])), axis=-1)[..., -1] / R
    return tp, fp, ap


def _stats_dict(ids, tp, fp, ap, npig, cuts):
    return {"image_ids": list(ids), "tp": tp, "fp": fp, "ap": ap, "npig": np.asarray(npig, dtype=np.int64), "cuts": tuple(int(c) for c in cuts)}


def image_stats(gt_by_img, dt_by_img, cuts=MAX_DET_CUTS, device=None, max_det=MAX_DETS):
    """Per-image statistics of one evaluation -> {"image_ids" (sorted, images with neither ground truth nor detection left out), "tp", "fp"
    int32 [A, B, T, M], "ap" float64 [A, B, T] (-1: no non-ignored ground truth), "npig" [A, B], "cuts"}; A = the four area ranges of AREA_RNG
    in its order, T = IOU_THRS, M = `cuts`.  device=None: `_evaluate_image`'s flags and `stats_from_flags`, the host path and the checker.  A
    CUDA device: `pack_images`, ONE cdetr_coco_match launch, ONE cdetr_coco_image_stats launch on its flags where they lie, one copy of the
    statistics back (and the 4 B ints of npig) -- EQUAL numbers, `ap` bit for bit."""
    return Matching.of(gt_by_img, dt_by_img, device, max_det=max_det).stats(cuts)


def image_stats_store(gt_by_img, store, image_ids, cuts=MAX_DET_CUTS, counts=None):
    """`image_stats(device=)` for an ops.DetectionStore: the detections are read where cdetr_emit_detections left them.  `image_ids[k]` = the id
    of the store's image k, `counts[k]` = use only its first counts[k] detections (a threshold above the store's own keeps a prefix)."""
    return match_store(gt_by_img, store, image_ids).stats(cuts, counts)


def average_recall(stats):
    """The second half of COCOeval.summarize, stats[6..11] -> {"AR<cut>" for every cut, "ARs", "ARm", "ARl"} x 100, NaN when undefined.  Per
    area range and cut: recall[t] = sum_b tp / sum_b npig (-1 when no image has a non-ignored ground truth), the mean of the entries > -1.
    The AR<cut> keys are area `all`; ARs / ARm / ARl are read at the last cut.  (`accumulate`'s recall is the cumulative tp's last column
    over npig: the sum of the images' counts.)"""
    areas = list(AREA_RNG)
    npig = np.asarray(stats["npig"]).sum(axis=1)

    def ar(a, m):
        rec = stats["tp"][a, :, :, m].sum(axis=0, dtype=np.int64).astype(np.float64) / npig[a] if npig[a] > 0 else -np.ones(len(IOU_THRS))
        v = _mean(rec)
        return v * 100 if v >= 0 else float("nan")
    out = {f"AR{c}": ar(areas.index("all"), m) for m, c in enumerate(stats["cuts"])}
    out.update({k: ar(areas.index(a), len(stats["cuts"]) - 1) for k, a in (("ARs", "small"), ("ARm", "medium"), ("ARl", "large"))})
    return out


def image_rows(stats, count_gt, count_pred):
    """One dict per image: image_id, count_gt, count_pred, diff = count_gt - count_pred (the sign of L2/scripts/analyze_res.py), AP / AP50 / AP75 /
    APs / APm / APl of the image alone (x 100; NaN where it has no non-ignored ground truth in that range), tp50 / fp50 / fn50 (area `all`, IoU
    0.5, the last cut; fn50 = npig - tp50).  count_gt / count_pred: {image_id: count}, the rows following count_gt's order (an image the
    statistics left out -- neither ground truth nor detection -- gets NaN and zeros), or sequences beside stats["image_ids"]."""
    areas = list(AREA_RNG)
    ids = list(count_gt) if isinstance(count_gt, dict) else list(stats["image_ids"])
    if not isinstance(count_gt, dict):
        count_gt, count_pred = dict(zip(ids, count_gt)), dict(zip(ids, count_pred))
    at = {i: b for b, i in enumerate(stats["image_ids"])}
    t50, t75, last = int(np.argmax(np.isclose(IOU_THRS, 0.5))), int(np.argmax(np.isclose(IOU_THRS, 0.75))), len(stats["cuts"]) - 1
    pct = lambda v: v * 100 if v >= 0 else float("nan")                    # noqa: E731
    rows = []
    for i in ids:
        row = {"image_id": i, "count_gt": int(count_gt[i]), "count_pred": int(count_pred[i]), "diff": int(count_gt[i]) - int(count_pred[i])}
        b = at.get(i)
        if b is None:
            row.update({k: float("nan") for k in ("AP", "AP50", "AP75", "APs", "APm", "APl")}, tp50=0, fp50=0, fn50=0)
        else:
            ap = stats["ap"]
            a = areas.index("all")
            row.update({"AP": pct(_mean(ap[a, b])), "AP50": pct(float(ap[a, b, t50])), "AP75": pct(float(ap[a, b, t75])),
                        "APs": pct(_mean(ap[areas.index("small"), b])), "APm": pct(_mean(ap[areas.index("medium"), b])),
                        "APl": pct(_mean(ap[areas.index("large"), b]))})
            tp50 = int(stats["tp"][a, b, t50, last])
            row.update(tp50=tp50, fp50=int(stats["fp"][a, b, t50, last]), fn50=int(stats["npig"][a, b]) - tp50)
        rows.append(row)
    return rows


def image_report(stats, image_ids, count_gt, count_pred, split, threshold):
    """What infer.py --image_report writes to image_report_<split>.json: {"split", "threshold", "max_dets", "AR" (`average_recall`), "rows"
    (`image_rows`, in the order `image_ids` = the order the images were run), "order_by_ap" (image ids by ascending AP, NaN last, ties by id),
    "order_by_diff" (image ids by descending diff, ties by id)}."""
    rows = image_rows(stats, dict(zip(image_ids, count_gt)), dict(zip(image_ids, count_pred)))
    by_ap = sorted(rows, key=lambda r: (r["AP"] != r["AP"], 0.0 if r["AP"] != r["AP"] else r["AP"], r["image_id"]))
    by_diff = sorted(rows, key=lambda r: (-r["diff"], r["image_id"]))
    return {"split": split, "threshold": float(threshold), "max_dets": list(stats["cuts"]), "AR": average_recall(stats), "rows": rows,
            "order_by_ap": [r["image_id"] for r in by_ap], "order_by_diff": [r["image_id"] for r in by_diff]}


def gt_from_json(gt_json, ids):
    """{image_id: [ground truth dicts]} of `instances_<split>.json` for the images `ids`, as `ap_from_json` forms them."""
    with open(gt_json) as f:
        gt = json.load(f)
    ids, gt_by = set(ids), {}
    for a in gt.get("annotations", []):
        if a["image_id"] in ids:
            b = [float(v) for v in a["bbox"]]
            gt_by.setdefault(a["image_id"], []).append({"bbox": b, "area": float(a.get("area", b[2] * b[3])), "iscrowd": a.get("iscrowd", 0),
                                                        "ignore": a.get("ignore", 0)})
    return gt_by


def dt_from_predictions(pred, ids=None):
    """{image_id: [detections]} of a predictions dict (the wire format of infer.py / A2/infer.py:84-116) as the matcher sees them: the
    evaluation boxes (`reference_box`), their areas and scores, of the images `ids` (None: all)."""
    dt_by = {}
    for a in pred.get("annotations", []):
        if ids is None or a["image_id"] in ids:
            b = reference_box(a["bbox"])
            dt_by.setdefault(a["image_id"], []).append({"bbox": b, "score": float(a["score"]), "area": float(b[2] * b[3])})
    return dt_by


def match_predictions(pred, gt_json, image_ids, device=None, areas=tuple(AREA_RNG)):
    """The ONE matching of a predictions dict as written against the ground truth `gt_json` holds for `image_ids` -> a `Matching` (`device` None:
    the host matcher)."""
    return Matching.of(gt_from_json(gt_json, image_ids), dt_from_predictions(pred), device, areas)


def ap_from_json(pred_json, gt_json, image_ids=None, device=None):
    """AP of `predictions_<split>.json` against `instances_<split>.json`.  `device`: passed to `summarize`."""
    with open(pred_json) as f:
        pred = json.load(f)
    ids = set(image_ids) if image_ids is not None else {im["id"] for im in pred.get("images", [])} or {a["image_id"] for a in pred["annotations"]}
    return summarize(gt_from_json(gt_json, ids), dt_from_predictions(pred, ids), device=device)
