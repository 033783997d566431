"""Tiled inference past the query cap (infer.py / main.py --eval --tiles RxC): the one rule and its host form.  Plain numpy, no device.
On the device the same steps are cdetr_tile_images, cdetr_exemplar_group_fwd and cdetr_tile_stitch (ops.tile_images / exemplar_group_fwd /
tile_stitch); this file is the host path of infer.py and the checker of those kernels, bit for bit.

THE RULE, stated once.  An image of the resized size H x W is cut into overlapping tiles, every tile is forwarded as an image of its own,
conditioned on the exemplars of the WHOLE image, and each detection is kept only by the tile whose core holds its centre.  What comes out is one
virtual image of Qv = R * C * Q queries that everything after the forward reads as it reads Q queries today.

  geometry      integers, in pixels of the resized image, unit u = 32.  Along an axis of length L with n requested parts:
                n_eff = min(n, max(L // u, 1)); core bounds c_i = u * ((i * (L // u)) // n_eff) for i < n_eff and c_{n_eff} = L; core i =
                [c_i, c_{i+1}); tile i = [max(c_i - M, 0), min(c_{i+1} + M, L)).  The cores partition [0, L).  Tiles are numbered row-major,
                T = R_eff * C_eff <= R * C = `slots`.
  tile pixels   scale 1: the crop.  Scale 2: output sample j of an axis lies at source position x0 + j / 2 - 0.25, i.e. it takes the source pixel
                x0 + j // 2 with weight 0.75 and its left (j even) or right (j odd) neighbour with weight 0.25; neighbours come from the
                FULL image, clamped to the image, not to the crop.  Horizontal pass first, the vertical pass over its result; a pass is
                0.75f * a + 0.25f * b, every multiply and the add rounded to fp32 (no FMA).  The tiles of an image are zero-padded to
                their common maximum Hm x Wm, mask True on the padding, as data.collate pads.
  exemplars     a present exemplar (x2 >= 0) belongs to exactly one tile: the one whose core holds its centre ((x1 + x2) / 2 * W, (y1 + y2) / 2 *
                H), formed in float64 from the fp32 rect; a centre left of / above the image belongs to the first core, one right of / below
                it to the last.  Its rect in that tile is r * a + o per coordinate, one fp32 multiply and one fp32 add, with a = L / tile_len
                and o = -x0 / tile_len formed in float64 and rounded to fp32 once (x0 = 0 gives o = -0.0, and r + -0.0 has r's bits).  In every
                other tile the row is -1, absent.  A tile that is the whole image has a = 1, o = -0.0: its rects come through bit for bit.
  small images  --tile_below P: an image is tiled when the float64 mean over its present exemplars of sqrt(w_px * h_px) is < P, with
                w_px = (x2 - x1) * W and h_px = (y2 - y1) * H formed in float64 from the fp32 rect; an image without a present exemplar is
                not tiled.  Every other image runs as ONE tile, the whole image at scale 1, and still fills R * C * Q virtual queries.
  group feature all T tiles of an image are conditioned on one exemplar feature pf = (sum x[tile][cell]) * (1 / max(cnt, 1)): an fp32 running
                sum over the tiles in order and within a tile over k in order, present rows only, `cell` by exemplar_fwd_kernel's own
                expression from the tile's rect and the tile's un-padded extent in feature cells (`cell_of`).
  stitch        virtual query t * Q + q is query q of tile t.  Box centres and reference points become v * a + o, sizes v * a, in whole-image
                normalised coordinates: one fp32 multiply, one fp32 add, no FMA, with a = tile_len / L and o = x0 / L formed in float64 and
                rounded to fp32 once (x0 = 0: o = -0.0, which changes no bit).  A query keeps its prob iff its stitched centre times (float)W
                and (float)H lies in the tile's core, lo <= v < hi in fp32; the first core of an axis has lo = -inf and the last hi = +inf,
                and an infinite bound is no bound at all (so a NaN centre is kept only along an axis that has ONE core).  Otherwise prob
                becomes NaN, which no reader counts; a NaN prob stays NaN.  Virtual queries of tiles that do not exist (T < R * C) are NaN
                with zero boxes and points.  At 1x1 the stitch is the identity on every bit.

Objects that straddle a seam can be detected by both neighbours with centres on either side of it; both survive the stitch, and --nms_iou,
which runs after it, is the tool that removes one.
"""
import re

import numpy as np

UNIT = 32
MAX_VIRTUAL = 4096          # R * C * Q: what cdetr_emit_detections and cdetr_nms_suppress take
COEF = 8                    # fp32 per tile: ax, ox, ay, oy, lo_x, hi_x, lo_y, hi_y


def parse_tiles(text):
    """`RxC` -> (R, C), both at least 1; ValueError otherwise."""
    m = re.fullmatch(r"\s*(\d+)\s*[xX]\s*(\d+)\s*", str(text))
    if m is None or int(m.group(1)) < 1 or int(m.group(2)) < 1:
        raise ValueError(f"--tiles: expected RxC with R and C at least 1, got {text!r}")
    return int(m.group(1)), int(m.group(2))


def check_capacity(R, C, Q):
    """R * C * Q <= 4096, the query limit of the emit and the suppression kernels; ValueError naming the numbers."""
    if R * C * Q > MAX_VIRTUAL:
        raise ValueError(f"--tiles {R}x{C}: {R} * {C} tiles of {Q} queries (--num_query_position * --num_query_pattern) are {R * C * Q} virtual "
                         f"queries, more than the {MAX_VIRTUAL} the detection kernels take")


def axis(L, n, M):
    """-> (core bounds [n_eff + 1], tiles [(x0, x1)] * n_eff) along an axis of L pixels cut into n parts with margin M."""
    L, n, M = int(L), int(n), int(M)
    if L < 1 or n < 1 or M < 0:
        raise ValueError(f"tiling.axis: L = {L}, n = {n}, M = {M}")
    cells = L // UNIT
    n_eff = min(n, max(cells, 1))
    c = [UNIT * ((i * cells) // n_eff) for i in range(n_eff)] + [L]
    return c, [(max(c[i] - M, 0), min(c[i + 1] + M, L)) for i in range(n_eff)]


class Plan:
    """The tiles of one image size: H, W, R, C, M, S, `slots` = R * C, T, per tile (row-major) `boxes` [(x0, y0, x1, y1)] and `cores`
    [(cx0, cy0, cx1, cy1)], `grid` = (R_eff, C_eff), the padded tile size Hm x Wm, and the tables the kernels read:
    records int32 [T, 5], coef fp32 [T, 8], rect_coef fp32 [T, 4] = (ax, ox, ay, oy) of the exemplar rects."""

    def __init__(self, H, W, R, C, M=32, S=1, slots=None):
        if S not in (1, 2):
            raise ValueError(f"--tile_scale: 1 or 2, got {S!r}")
        self.H, self.W, self.R, self.C, self.M, self.S = int(H), int(W), int(R), int(C), int(M), int(S)
        self.slots = self.R * self.C if slots is None else int(slots)
        self.cy, ty = axis(self.H, self.R, self.M)
        self.cx, tx = axis(self.W, self.C, self.M)
        self.grid = (len(ty), len(tx))
        self.T = len(ty) * len(tx)
        if self.T > self.slots:
            raise ValueError(f"tiling.Plan: {self.T} tiles into {self.slots} slots")
        self.boxes = [(x0, y0, x1, y1) for (y0, y1) in ty for (x0, x1) in tx]
        self.cores = [(self.cx[j], self.cy[i], self.cx[j + 1], self.cy[i + 1]) for i in range(len(ty)) for j in range(len(tx))]
        self.Hm = max(y1 - y0 for _, y0, _, y1 in self.boxes) * self.S
        self.Wm = max(x1 - x0 for x0, _, x1, _ in self.boxes) * self.S
        self.records = np.array([[x0, y0, x1 - x0, y1 - y0, self.S] for x0, y0, x1, y1 in self.boxes], dtype=np.int32)
        f32, inf = np.float32, np.float32(np.inf)
        self.coef = np.zeros((self.T, COEF), dtype=np.float32)
        self.rect_coef = np.zeros((self.T, 4), dtype=np.float32)
        nr, nc = self.grid
        for t, ((x0, y0, x1, y1), (kx0, ky0, kx1, ky1)) in enumerate(zip(self.boxes, self.cores)):
            i, j = divmod(t, nc)
            self.coef[t] = (f32((x1 - x0) / self.W), _offset(x0, self.W), f32((y1 - y0) / self.H), _offset(y0, self.H),
                            -inf if j == 0 else f32(kx0), inf if j == nc - 1 else f32(kx1),
                            -inf if i == 0 else f32(ky0), inf if i == nr - 1 else f32(ky1))
            self.rect_coef[t] = (f32(self.W / (x1 - x0)), -abs(_offset(x0, x1 - x0)), f32(self.H / (y1 - y0)), -abs(_offset(y0, y1 - y0)))
        self.whole = self.T == 1 and self.S == 1          # the one tile is the image itself: nothing to cut

    def owner(self, cx, cy):
        """Tile whose core holds the point (cx, cy) in resized pixels (float64); outside the image: the nearest core."""
        j = sum(1 for b in self.cx[1:-1] if cx >= b)
        i = sum(1 for b in self.cy[1:-1] if cy >= b)
        return i * self.grid[1] + j


def _offset(x0, L):
    """x0 / L in float64 -> fp32, and -0.0 for x0 = 0: adding it changes no bit of the other operand."""
    return np.float32(-0.0) if x0 == 0 else np.float32(x0 / L)


def exemplar_size(rects, H, W):
    """The float64 mean over the present rows of sqrt(w_px * h_px) (None without a present row); rects fp32 [K, 4] normalised xyxy."""
    r = np.asarray(rects, dtype=np.float32).reshape(-1, 4).astype(np.float64)
    r = r[r[:, 2] >= 0]
    if r.shape[0] == 0:
        return None
    return float(np.mean(np.sqrt(((r[:, 2] - r[:, 0]) * W) * ((r[:, 3] - r[:, 1]) * H))))


class Tiling:
    """--tiles / --tile_margin / --tile_scale / --tile_below of one run: `plan_for(H, W, rects)` -> the Plan of an image (cached per size)."""

    def __init__(self, R, C, margin=32, scale=1, below=None):
        self.R, self.C, self.margin, self.scale = int(R), int(C), int(margin), int(scale)
        self.below = None if below is None else float(below)
        if self.R < 1 or self.C < 1 or self.margin < 0 or self.scale not in (1, 2):
            raise ValueError(f"Tiling: R = {R}, C = {C}, margin = {margin}, scale = {scale}")
        self._plans = {}

    def tiled(self, H, W, rects):
        if self.below is None:
            return True
        size = exemplar_size(rects, H, W)
        return size is not None and size < self.below

    def plan_for(self, H, W, rects):
        key = (int(H), int(W), self.tiled(H, W, rects))
        if key not in self._plans:
            self._plans[key] = Plan(H, W, self.R, self.C, self.margin, self.scale) if key[2] else Plan(H, W, 1, 1, 0, 1, slots=self.R * self.C)
        return self._plans[key]


def _up2(n_out, x0, L):
    """Scale 2 along one axis -> (near, far) source indices of the n_out output samples, clamped to the image."""
    j = np.arange(n_out)
    near = x0 + j // 2
    far = np.where(j % 2 == 0, near - 1, near + 1)
    return np.clip(near, 0, L - 1), np.clip(far, 0, L - 1)


def tile_images(image, plan):
    """image fp32 [3, H, W] -> (tiles fp32 [T, 3, Hm, Wm], mask bool [T, Hm, Wm]): the host form of cdetr_tile_images."""
    image = np.ascontiguousarray(image, dtype=np.float32)
    if image.shape != (3, plan.H, plan.W):
        raise ValueError(f"tiling.tile_images: image {image.shape} for a plan of {plan.H} x {plan.W}")
    tiles = np.zeros((plan.T, 3, plan.Hm, plan.Wm), dtype=np.float32)
    mask = np.ones((plan.T, plan.Hm, plan.Wm), dtype=bool)
    a, b = np.float32(0.75), np.float32(0.25)
    for t, (x0, y0, x1, y1) in enumerate(plan.boxes):
        if plan.S == 1:
            out = image[:, y0:y1, x0:x1]
        else:
            xn, xf = _up2(2 * (x1 - x0), x0, plan.W)
            yn, yf = _up2(2 * (y1 - y0), y0, plan.H)
            hp = a * image[:, :, xn] + b * image[:, :, xf]              # fp32 throughout: one rounding per multiply and per add
            out = a * hp[:, yn, :] + b * hp[:, yf, :]
        tiles[t, :, :out.shape[1], :out.shape[2]] = out
        mask[t, :out.shape[1], :out.shape[2]] = False
    return tiles, mask


def tile_rects(rects, plan):
    """rects fp32 [K, 4] normalised xyxy of the whole image (x2 < 0: absent) -> fp32 [T, K, 4]: every present exemplar in the tile that owns
    its centre, in that tile's coordinates, and -1 everywhere else."""
    rects = np.ascontiguousarray(rects, dtype=np.float32).reshape(-1, 4)
    out = np.full((plan.T,) + rects.shape, -1.0, dtype=np.float32)
    for k, r in enumerate(rects):
        if not r[2] >= 0:
            continue
        r64 = r.astype(np.float64)
        t = plan.owner((r64[0] + r64[2]) / 2 * plan.W, (r64[1] + r64[3]) / 2 * plan.H)
        ax, ox, ay, oy = plan.rect_coef[t]
        out[t, k] = (r[0] * ax + ox, r[1] * ay + oy, r[2] * ax + ox, r[3] * ay + oy)
    return out


def stitch(prob, boxes, points, plan):
    """prob fp32 [T, Q], boxes fp32 [T, Q, 4] cxcywh, points fp32 [T, Q, 2] of an image's tiles -> (prob [Qv], boxes [Qv, 4], points [Qv, 2])
    of the virtual image, Qv = plan.slots * Q: the host form of cdetr_tile_stitch."""
    prob = np.ascontiguousarray(prob, dtype=np.float32)
    boxes, points = np.asarray(boxes, dtype=np.float32), np.asarray(points, dtype=np.float32)
    T, Q = prob.shape
    if T != plan.T or boxes.shape != (T, Q, 4) or points.shape != (T, Q, 2):
        raise ValueError(f"tiling.stitch: prob [{plan.T}, Q], boxes [T, Q, 4], points [T, Q, 2] expected, got {prob.shape}, {boxes.shape}, {points.shape}")
    S = plan.slots
    vp = np.full((S, Q), np.nan, dtype=np.float32)
    vb, vpt = np.zeros((S, Q, 4), dtype=np.float32), np.zeros((S, Q, 2), dtype=np.float32)
    Wf, Hf, inf = np.float32(plan.W), np.float32(plan.H), np.float32(np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            ax, ox, ay, oy, lox, hix, loy, hiy = plan.coef[t]
            vb[t, :, 0], vb[t, :, 1] = boxes[t, :, 0] * ax + ox, boxes[t, :, 1] * ay + oy
            vb[t, :, 2], vb[t, :, 3] = boxes[t, :, 2] * ax, boxes[t, :, 3] * ay
            vpt[t, :, 0], vpt[t, :, 1] = points[t, :, 0] * ax + ox, points[t, :, 1] * ay + oy
            px, py = vb[t, :, 0] * Wf, vb[t, :, 1] * Hf
            own = np.ones(Q, dtype=bool)
            for v, lo, hi in ((px, lox, hix), (py, loy, hiy)):
                if lo != -inf:
                    own &= v >= lo
                if hi != inf:
                    own &= v < hi
            vp[t] = np.where(own, prob[t], np.float32(np.nan))
    return vp.reshape(S * Q), vb.reshape(S * Q, 4), vpt.reshape(S * Q, 2)


def cell_of(rect, hv, wv, h, w):
    """exemplar_fwd_kernel's own expression: rect fp32 xyxy normalised to an image whose un-padded extent is (hv, wv) feature cells (fp32) on an
    h x w map -> the cell of its centre; every operation in fp32, rounded once (the kernel's products are not fused), truncation toward zero."""
    f32 = np.float32
    x1, y1, x2, y2 = (f32(v) for v in rect)
    hv, wv = f32(hv), f32(wv)
    with np.errstate(invalid="ignore", over="ignore"):
        xc = min(max(int((x1 * wv + x2 * wv) / f32(2)), 0), w - 1)
        yc = min(max(int((y1 * hv + y2 * hv) / f32(2)), 0), h - 1)
    return yc * w + xc


def group_feature(x, rects, extent, h, w, G):
    """x fp32 [B, h * w, C], rects fp32 [B, K, 4] (x2 < 0: absent), extent fp32 [B, 2] = un-padded (rows, columns), B % G == 0 ->
    (pf fp32 [B, C], the same row for the G tiles of a group; idx int32 [B, K], cell or -1): the host form of cdetr_exemplar_group_fwd."""
    x, rects, extent = np.asarray(x, dtype=np.float32), np.asarray(rects, dtype=np.float32), np.asarray(extent, dtype=np.float32)
    B, P, C = x.shape
    K = rects.shape[1]
    if P != h * w or rects.shape != (B, K, 4) or extent.shape != (B, 2) or G < 1 or B % G:
        raise ValueError(f"tiling.group_feature: x {x.shape}, rects {rects.shape}, extent {extent.shape}, map {h} x {w}, G = {G}")
    pf, idx = np.zeros((B, C), dtype=np.float32), np.full((B, K), -1, dtype=np.int32)
    for g in range(B // G):
        acc, cnt = np.zeros(C, dtype=np.float32), 0
        for b in range(g * G, (g + 1) * G):
            for k in range(K):
                if rects[b, k, 2] >= 0:
                    idx[b, k] = cell_of(rects[b, k], extent[b, 0], extent[b, 1], h, w)
                    acc = acc + x[b, idx[b, k]]
                    cnt += 1
        pf[g * G:(g + 1) * G] = acc * (np.float32(1) / np.float32(max(cnt, 1)))
    return pf, idx
