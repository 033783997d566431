"""Seeded inputs for the device box-AP tests (test_coco_ap_device_cpu.py / _gpu.py) and the statistics that show what they exercise.
Everything here runs on the host; the checker is coco_ap's host path."""
import numpy as np

from counting_detr_amd import coco_ap as ca

SIZES = (8, 16, 32, 48, 96, 128)          # areas sit ON the 32^2 / 96^2 bounds of the area ranges (32 x 32 = 8 x 128 = 1024, 96 x 96 = 9216)


def gt(b, **kw):
    d = {"bbox": [float(v) for v in b], "area": float(b[2] * b[3])}
    d.update(kw)
    return d


def dt(b, s):
    return {"bbox": [float(v) for v in b], "score": float(s), "area": float(b[2] * b[3])}


def tie_image(rng, G, D, grid=12, step=16, copies=0.3, crowd=0.1):
    """The "tie" family: integer boxes on a coarse grid, sizes from SIZES, `copies` of the ground truths overwritten by exact copies of
    others (equal IoUs between ground truths), ~`crowd` of them iscrowd, detections = ground truths shifted by -8 / 0 / +8 per axis with
    scores rounded to two decimals (repeated scores: the stable order decides)."""
    g = np.stack([rng.integers(0, grid, G) * step, rng.integers(0, grid, G) * step, rng.choice(SIZES, G), rng.choice(SIZES, G)], axis=1).astype(np.float64)
    if G > 1:
        dst = rng.random(G) < copies
        g[dst] = g[rng.integers(0, G, int(dst.sum()))]
    gts = [gt(b, iscrowd=int(rng.random() < crowd)) for b in g]
    dts = []
    for _ in range(D):
        b = g[rng.integers(0, G)].copy() if G else np.array([rng.integers(0, grid) * step, rng.integers(0, grid) * step, 16.0, 16.0])
        b[0] += rng.choice((-8, 0, 8))
        b[1] += rng.choice((-8, 0, 8))
        dts.append(dt(b, round(float(rng.random()), 2)))
    return gts, dts


def float_image(rng, G, D, extent=1200.0, jitter=0.15):
    """The "float" family: fractional ground truths (stage-1 pseudo boxes are not integers), detections = jittered copies plus a fifth of
    stray boxes, distinct scores.  A contraction of a * b + c into an FMA shows here and not on integer boxes."""
    wh = np.exp(rng.uniform(np.log(6.0), np.log(160.0), (G, 2)))
    xy = rng.uniform(0.0, extent, (G, 2))
    g = np.concatenate([xy, wh], axis=1)
    gts = [gt(b, iscrowd=int(rng.random() < 0.05)) for b in g]
    dts = []
    for _ in range(D):
        if G and rng.random() < 0.8:
            b = g[rng.integers(0, G)].copy()
            b[:2] += rng.normal(0.0, jitter, 2) * b[2:]
            b[2:] *= np.exp(rng.normal(0.0, jitter, 2))
        else:
            b = np.concatenate([rng.uniform(0.0, extent, 2), np.exp(rng.uniform(np.log(6.0), np.log(160.0), 2))])
        dts.append(dt(b, float(rng.random())))
    return gts, dts


def tie_family(seed=0, shapes=((200, 333), (120, 150), (64, 100), (333, 200))):
    rng = np.random.default_rng(seed)
    gts, dts = {}, {}
    for i, (G, D) in enumerate(shapes):
        gts[10 + i], dts[10 + i] = tie_image(rng, G, D)
    return gts, dts


def float_family(seed=1, shapes=((60, 120), (5, 40), (150, 90))):
    rng = np.random.default_rng(seed)
    gts, dts = {}, {}
    for i, (G, D) in enumerate(shapes):
        gts[100 + i], dts[100 + i] = float_image(rng, G, D, extent=400.0)
    return gts, dts


def host_flags(gts, dts, area, max_det=ca.MAX_DETS):
    """coco_ap._evaluate_image over the images of a set in `pack_images` order -> (scores [N], matched [T, N], ignored [T, N], npig per image)."""
    T = len(ca.IOU_THRS)
    s, m, ig, n = [np.zeros(0)], [np.zeros((T, 0), dtype=bool)], [np.zeros((T, 0), dtype=bool)], []
    for img in sorted(set(gts) | set(dts)):
        g, d = gts.get(img, []), dts.get(img, [])
        if not g and not d:
            continue
        si, mi, ii, ni = ca._evaluate_image(d, g, ca.AREA_RNG[area], max_det)
        s.append(si); m.append(mi.reshape(T, -1)); ig.append(ii.reshape(T, -1)); n.append(ni)
    return np.concatenate(s), np.concatenate(m, axis=1), np.concatenate(ig, axis=1), np.array(n, dtype=np.int64)


def tie_statistics(gts, dts):
    """What the tie family is meant to exercise, counted on the HOST path's own quantities."""
    thr = np.minimum(ca.IOU_THRS, 1 - 1e-10)
    shared, on_thr, repeated = 0, 0, 0
    for img in gts:
        iou = ca.box_iou_xywh([d["bbox"] for d in dts[img]], [g["bbox"] for g in gts[img]])
        best = iou.max(axis=1)
        shared += int(((best >= 0.5) & ((iou == best[:, None]).sum(axis=1) > 1)).sum())
        on_thr += int(np.isin(iou, thr).sum())
        sc = [d["score"] for d in dts[img]]
        repeated += len(sc) - len(set(sc))
    out = {"shared_best": shared, "on_threshold": on_thr, "repeated_scores": repeated}
    for area in ca.AREA_RNG:
        _, m, ig, _ = host_flags(gts, dts, area)
        out[area] = {"matched_ignored": int((m & ig).sum()), "unmatched_ignored": int((~m & ig).sum()),
                     "matches_first": int(m[0].sum()), "matches_last": int(m[-1].sum()), "first_differs_from_last": bool((m[0] != m[-1]).any())}
    return out


def assert_tie_bars(st):
    assert st["shared_best"] >= 50, st
    assert st["on_threshold"] >= 20, st
    assert st["repeated_scores"] >= 100, st
    for area in ("small", "medium", "large"):
        assert st[area]["matched_ignored"] > 0 and st[area]["unmatched_ignored"] > 0, (area, st)
    assert st["all"]["first_differs_from_last"], st


def matching_sets():
    """Small members of the two families for the readings of one coco_ap.Matching, each with an image of ground truths only and one of
    detections only (and one with neither in `tie`), and the empty set."""
    tie = tie_family(seed=3, shapes=((20, 60), (0, 7), (9, 0), (12, 30)))
    tie[0][99], tie[1][99] = [], []
    return {"tie": tie, "float": float_family(seed=5, shapes=((15, 40), (6, 0), (0, 12))), "empty": ({}, {})}


def same_six(a, b):
    assert list(a) == list(b) and all(a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])) for k in a), (a, b)


def same_stats(a, b):
    """Two dicts of coco_ap.image_stats, field by field; the average precisions as float64 bits."""
    assert a["image_ids"] == b["image_ids"] and a["cuts"] == b["cuts"] and np.array_equal(a["npig"], b["npig"])
    for k in ("tp", "fp", "ap"):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
    assert np.array_equal(a["tp"], b["tp"]) and np.array_equal(a["fp"], b["fp"])
    assert np.array_equal(np.ascontiguousarray(a["ap"]).view(np.int64), np.ascontiguousarray(b["ap"]).view(np.int64))
