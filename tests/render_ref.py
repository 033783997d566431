"""The drawing rule of counting_detr_amd/render.py restated as a PAINTER (not a test module; shared by tests/test_render_cpu.py and
tests/test_render_gpu.py): the bottom layer first, one primitive at a time, each written over what is there with slice assignments -- exemplars
(last of the file first), ground truths (last of the pack first), detection outlines (worst score first), detection dots (worst score first).
What is painted last stays on top, so a pixel ends with the colour of the first primitive of the priority list that covers it: the same image
as the product's first-hit formulation, reached the opposite way.  Python integers and math.floor; nothing is shared with render.py."""
import math

import numpy as np

STYLE = [[0, 255, 0, 1], [255, 0, 0, 1], [128, 128, 128, 1], [0, 0, 255, 1], [255, 255, 0, 2]]        # tp, fp, ignored, gt, exemplar
TP, FP, IGNORED, GT, EXEMPLAR = range(5)


def _int(v):
    """floor, clamped to [-2, 32768] in floating point, then an int (v finite or an infinity)."""
    if v == math.inf:
        return 32768
    if v == -math.inf:
        return -2
    return int(min(max(float(math.floor(v)), -2.0), 32768.0))


def corners(box):
    """[x, y, w, h] -> (x0, y0, x1, y1, cx, cy) or None when the box draws nothing."""
    x, y, w, h = (float(v) for v in box)
    if not all(math.isfinite(v) for v in (x, y, w, h)):
        return None
    x0, y0, x1, y1 = _int(x), _int(y), _int(x + w), _int(y + h)
    if x1 < x0 or y1 < y0:
        return None
    return x0, y0, x1, y1, _int(x + w * 0.5), _int(y + h * 0.5)


def _fill(img, x0, y0, x1, y1, rgb):
    """The inclusive rectangle clipped to the canvas <- rgb (nothing when it is empty)."""
    H, W = img.shape[:2]
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1)
    if x0 <= x1 and y0 <= y1:
        img[y0:y1 + 1, x0:x1 + 1] = rgb


def outline(img, c, t, rgb):
    """Four strips of thickness t inside the corners: top, bottom, left, right (they overlap at the corners and, for a large t, in the middle)."""
    x0, y0, x1, y1 = c[:4]
    if t < 1:
        return
    _fill(img, x0, y0, x1, min(y0 + t - 1, y1), rgb)
    _fill(img, x0, max(y1 - t + 1, y0), x1, y1, rgb)
    _fill(img, x0, y0, min(x0 + t - 1, x1), y1, rgb)
    _fill(img, max(x1 - t + 1, x0), y0, x1, y1, rgb)


def paint(canvas, dts, classes, gts, exs, style=STYLE, dot=1):
    """One canvas: dts / gts / exs = lists of [x, y, w, h] (detections in evaluation order), classes[i] = TP / FP / IGNORED -> a new array."""
    img = np.array(canvas, dtype=np.uint8, copy=True)
    for box in reversed(list(exs)):
        c = corners(box)
        if c is not None:
            outline(img, c, style[EXEMPLAR][3], style[EXEMPLAR][:3])
    for box in reversed(list(gts)):
        c = corners(box)
        if c is not None:
            outline(img, c, style[GT][3], style[GT][:3])
    dts, classes = list(dts), list(classes)
    for box, k in reversed(list(zip(dts, classes))):
        c = corners(box)
        if c is not None:
            outline(img, c, style[k][3], style[k][:3])
    if dot >= 0:
        for box, k in reversed(list(zip(dts, classes))):
            c = corners(box)
            if c is not None:
                _fill(img, c[4] - dot, c[5] - dot, c[4] + dot, c[5] + dot, style[k][:3])
    return img


def classes_of(matched50, ignored50):
    return [IGNORED if ig else (TP if m else FP) for m, ig in zip(np.asarray(matched50).tolist(), np.asarray(ignored50).tolist())]


def paint_pack(canvases, pack, matched50, ignored50, sel, dt_cnt=None, exemplars=None, style=STYLE, dot=1):
    """`render.render_images`' signature on the painter: pack = coco_ap.pack_images' dict."""
    cls = classes_of(matched50, ignored50)
    out = []
    for k, (canvas, b) in enumerate(zip(canvases, sel)):
        d0, d1 = int(pack["dt_off"][b]), int(pack["dt_off"][b + 1])
        if dt_cnt is not None:
            d1 = d0 + min(d1 - d0, max(int(dt_cnt[b]), 0))
        g0, g1 = int(pack["gt_off"][b]), int(pack["gt_off"][b + 1])
        out.append(paint(canvas, pack["dt_boxes"][d0:d1].tolist(), cls[d0:d1], pack["gt_boxes"][g0:g1].tolist(),
                         [] if exemplars is None else np.asarray(exemplars[k], dtype=np.float64).reshape(-1, 4).tolist(), style, dot))
    return out


def make_pack(per_image):
    """[(dts [n, 4], gts [m, 4])] -> the fields of a pack the renderers read (image ids 0 .. B - 1)."""
    dts = [np.asarray(d, dtype=np.float64).reshape(-1, 4) for d, _ in per_image]
    gts = [np.asarray(g, dtype=np.float64).reshape(-1, 4) for _, g in per_image]
    return {"image_ids": list(range(len(per_image))), "dt_boxes": np.concatenate(dts + [np.zeros((0, 4))]),
            "gt_boxes": np.concatenate(gts + [np.zeros((0, 4))]),
            "dt_off": np.concatenate([[0], np.cumsum([len(d) for d in dts])]).astype(np.int32),
            "gt_off": np.concatenate([[0], np.cumsum([len(g) for g in gts])]).astype(np.int32)}


def random_boxes(rng, H, W, m, margin=20.0, small=None):
    """m boxes with both corners drawn from [-margin, size + margin] (`small`: the second corner at most that far from the first instead), three
    in ten rounded to integers."""
    a = np.stack([rng.uniform(-margin, W + margin, m), rng.uniform(-margin, H + margin, m)], axis=1)
    if small is None:
        b = np.stack([rng.uniform(-margin, W + margin, m), rng.uniform(-margin, H + margin, m)], axis=1)
    else:
        b = a + rng.uniform(0.0, small, (m, 2))
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    out = np.concatenate([lo, hi - lo], axis=1)
    whole = rng.random(m) < 0.3
    out[whole] = np.round(out[whole])
    return out


def random_set(rng, sizes, n_max, margin=20.0, counts=None, small=None):
    """Seeded canvases of `sizes` = [(H, W)], each with 0 .. n_max primitives split between detections, ground truths and exemplars (or
    exactly counts[k] = (detections, ground truths, exemplars)) -> (canvases, pack, matched50, ignored50, exemplars)."""
    canvases, per, exs = [], [], []
    for k, (H, W) in enumerate(sizes):
        canvases.append(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
        if counts is None:
            n = int(rng.integers(0, n_max + 1))
            cut = np.sort(rng.integers(0, n + 1, 2))
            nd, ng, ne = int(cut[0]), int(cut[1] - cut[0]), n - int(cut[1])
        else:
            nd, ng, ne = counts[k]
        per.append((random_boxes(rng, H, W, nd, margin, small), random_boxes(rng, H, W, ng, margin, small)))
        exs.append(random_boxes(rng, H, W, ne, margin, small))
    pack = make_pack(per)
    D = len(pack["dt_boxes"])
    return canvases, pack, rng.random(D) < 0.5, rng.random(D) < 0.2, exs


# ------------------------------------------------------------------------------------------------------------ hand-written cases, 5 rows x 7 columns
# Expected pixels, written out by hand from the rule: '.' = the image's pixel, G = tp green, R = fp red, X = ignored grey, B = ground-truth
# blue, Y = exemplar yellow.  A case = (name, detections [(box, class)], ground truths, exemplars, dot, dt_cnt or None, style overrides, rows).
LETTER = {"G": (0, 255, 0), "R": (255, 0, 0), "X": (128, 128, 128), "B": (0, 0, 255), "Y": (255, 255, 0)}
HAND_H, HAND_W = 5, 7
NAN, INF = float("nan"), float("inf")
BLANK = [".......", ".......", ".......", ".......", "......."]
_TWO = [([1, 1, 3, 2], TP), ([2, 2, 3, 2], FP)]
HAND_CASES = [
    ("one box", [], [[1, 1, 3, 2]], [], -1, None, {}, [".......", ".BBBB..", ".B..B..", ".BBBB..", "......."]),
    ("fractional corners floor", [], [[1.9, 1.2, 2.2, 2.7]], [], -1, None, {}, [".......", ".BBBB..", ".B..B..", ".BBBB..", "......."]),
    ("cut by the left edge", [], [[-2, 1, 4, 2]], [], -1, None, {}, [".......", "BBB....", "..B....", "BBB....", "......."]),
    ("cut by the right edge", [], [[4, 1, 5, 2]], [], -1, None, {}, [".......", "....BBB", "....B..", "....BBB", "......."]),
    ("cut by the top edge", [], [[2, -1.5, 2, 3]], [], -1, None, {}, ["..B.B..", "..BBB..", ".......", ".......", "......."]),
    ("cut by the bottom edge", [], [[2, 3, 2, 5]], [], -1, None, {}, [".......", ".......", ".......", "..BBB..", "..B.B.."]),
    ("fully outside", [], [[10, 10, 3, 3], [-9, -9, 3, 3], [7, 0, 2, 2], [0, 5, 2, 2]], [], -1, None, {}, BLANK),
    ("w = h = 0", [], [[3, 2, 0, 0]], [], -1, None, {}, [".......", ".......", "...B...", ".......", "......."]),
    ("x1 < x0 and y1 < y0", [([3, 2, -2, 1], TP), ([3, 2, 1, -1.5], FP)], [], [], 1, None, {}, BLANK),
    ("a NaN and an inf field", [([NAN, 1, 2, 2], TP), ([1, 1, 2, INF], FP), ([1, -INF, 2, 2], TP)], [[1, 1, NAN, 2]], [[INF, 1, 2, 2]], 1, None, {}, BLANK),
    ("1e300", [], [[1e300, 1, 2, 2], [-1e300, -1e300, 2e300, 2e300], [1, 1, 1e308, 1e308]], [], -1, None, {},
     [".......", ".BBBBBB", ".B.....", ".B.....", ".B....."]),
    ("1e300 around the canvas at thickness 3", [], [], [[-1e300, -1e300, 2e300, 2e300]], -1, None, {EXEMPLAR: 3},
     ["YYYYYYY", "Y......", "Y......", "Y......", "Y......"]),
    ("thickness 3 fills a 4 x 4 box", [], [], [[1, 0, 3, 3]], -1, None, {EXEMPLAR: 3}, [".YYYY..", ".YYYY..", ".YYYY..", ".YYYY..", "......."]),
    ("thickness 1 leaves its hole", [], [], [[1, 0, 3, 3]], -1, None, {EXEMPLAR: 1}, [".YYYY..", ".Y..Y..", ".Y..Y..", ".YYYY..", "......."]),
    ("two overlapping detections", _TWO, [], [], -1, None, {}, [".......", ".GGGG..", ".GRRGR.", ".GGGGR.", "..RRRR."]),
    ("an ignored detection is grey whatever matched says", [([1, 1, 3, 2], IGNORED)], [], [], -1, None, {},
     [".......", ".XXXX..", ".X..X..", ".XXXX..", "......."]),
    ("a dot over another box's outline", [([1, 1, 4, 2], TP), ([2, 0, 2, 2], FP)], [], [], 0, None, {},
     ["..RRR..", ".GGRGG.", ".GRGRG.", ".GGGGG.", "......."]),
    ("a dot of radius 1 is a 3 x 3 square, clipped", [([-1, 2, 2.5, 4], FP)], [], [], 1, None, {},
     [".......", ".......", "RR.....", "RR.....", "RR....."]),
    ("detection over ground truth over exemplar", [([1, 1, 3, 2], TP)], [[0, 1, 3, 2]], [[1, 1, 3, 2]], -1, None, {},
     [".......", "BGGGG..", "BGYBG..", "BGGGG..", "......."]),
    ("dt_cnt 0", _TWO, [], [], -1, [0], {}, BLANK),
    ("dt_cnt partial", _TWO, [], [], -1, [1], {}, [".......", ".GGGG..", ".G..G..", ".GGGG..", "......."]),
    ("dt_cnt larger than the list", _TWO, [], [], -1, [5], {}, [".......", ".GGGG..", ".GRRGR.", ".GGGGR.", "..RRRR."]),
    ("dt_cnt negative", _TWO, [], [], -1, [-3], {}, BLANK),
]


def hand_canvas():
    y, x = np.mgrid[0:HAND_H, 0:HAND_W]
    return np.stack([10 + y, 40 + x, 90 + y * HAND_W + x], axis=2).astype(np.uint8)


def hand_expected(rows):
    img = hand_canvas()
    for y, row in enumerate(rows):
        assert len(row) == HAND_W and len(rows) == HAND_H
        for x, ch in enumerate(row):
            if ch != ".":
                img[y, x] = LETTER[ch]
    return img


def hand_inputs(case):
    """A hand case -> the arguments of `render_images` / `paint_pack`: (canvases, pack, matched50, ignored50, sel, dt_cnt, exemplars, style, dot)."""
    _, dts, gts, exs, dot, dt_cnt, thick, _ = case
    style = [list(s) for s in STYLE]
    for k, t in thick.items():
        style[k][3] = t
    pack = make_pack([([b for b, _ in dts], gts)])
    matched = np.array([c in (TP, IGNORED) for _, c in dts], dtype=bool)           # an ignored detection is a matched one here: grey all the same
    ignored = np.array([c == IGNORED for _, c in dts], dtype=bool)
    return [hand_canvas()], pack, matched, ignored, [0], dt_cnt, [np.asarray(exs, dtype=np.float64).reshape(-1, 4)], style, dot
