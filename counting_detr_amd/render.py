"""Box overlays of evaluated images: the step the reference left half alive (its evaluators' `visualize_res` draws predicted boxes, their
centres and the ground truths with cv2.rectangle / cv2.circle and never saves them, L2/offline_lvis_evaluator.py:167-207; stage 2 has
--vis_pseudo and scripts/visualize_generated_data.py), for the images infer.py --image_report says the model fails on (infer.py
--render_worst K / --render_ids).  No OpenCV: the rule below is the whole painter.

THE RULE (integers, so that every route can be compared with ==)
  canvas    the image file at its original size, PIL.Image.open(...).convert("RGB"), uint8 [H, W, 3].
  box       [x, y, w, h] float64: a detection = the evaluation box the matcher saw (coco_ap.reference_box of the json box), a ground truth =
            its `bbox` of instances_<split>.json, an exemplar = [x1, y1, x2 - x1, y2 - y1] of annotation_FSC147_384.json.
  corners   x0 = floor(x), y0 = floor(y), x1 = floor(x + w), y1 = floor(y + h): one float64 operation each (no FMA), clamped in float64 to
            [-2, 32768] before the conversion to int.  A box with a non-finite field, x1 < x0 or y1 < y0 draws nothing.
  outline   of thickness t >= 1: the canvas pixels with x0 <= px <= x1, y0 <= py <= y1 and min(px - x0, x1 - px, py - y0, y1 - py) < t.
            What lies off the canvas is not there; a box larger than the canvas may draw no pixel; w = h = 0 draws one; a large t fills.
  dot       of radius r >= 0 (detections only; r < 0: none): |px - cx| <= r and |py - cy| <= r, cx = floor(x + w * 0.5), cy = floor(y + h * 0.5),
            clamped like the corners.
  class     of a detection, read at area range `all`, IoU 0.5: `ignored` when det_ignored, else `tp` when matched, else `fp`.  Only the
            first dt_cnt[b] detections of an image are drawn (a threshold above the store's own keeps a prefix of the evaluation order).
  priority  detection dots in evaluation order, detection outlines in evaluation order (best score on top), ground truths in pack order,
            exemplars in file order: a pixel takes the colour of the FIRST primitive of that list that covers it, opaque, else the image's.
  style     uint8 [5][4] = (r, g, b, thickness) of tp, fp, ignored, gt, exemplar, and the dot radius.

`render_images(device=None)` is the host implementation below (numpy; per primitive in priority order, only pixels nothing has claimed
yet -- the kernel's formulation); `device=` a CUDA device is ONE cdetr_render_boxes launch (csrc/render.hip; TILE_H x TILE_W pixels per
workgroup, CHUNK primitives per round), EQUAL byte for byte (tests/test_render_cpu.py, _gpu.py check both against a bottom-up painter,
tests/render_ref.py).  `select` picks the images, `write` the PNGs and index.json.
"""
import json
import os

import numpy as np

TP, FP, IGNORED, GT, EXEMPLAR = range(5)
CLASSES = ("tp", "fp", "ignored", "gt", "exemplar")
DEFAULT_STYLE = np.array([[0, 255, 0, 1], [255, 0, 0, 1], [128, 128, 128, 1], [0, 0, 255, 1], [255, 255, 0, 2]], dtype=np.uint8)
DEFAULT_DOT = 1
TILE_H, TILE_W, CHUNK = 16, 16, 256         # CDETR_RENDER_TILE_H / _TILE_W / _CHUNK of include/cdetr_hip.h (tests stand on their edges)
MAX_SIDE = 16384
LO, HI = -2.0, 32768.0


def _clamped_floor(v):
    return np.clip(np.floor(v), LO, HI).astype(np.int64)


def corners(boxes):
    """float64 [N, 4] xywh -> (x0, y0, x1, y1, cx, cy int64 [N], ok bool [N]): the integer corners and centres of the rule; `ok` False = the
    box draws nothing."""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    finite = np.isfinite(b).all(axis=1)
    b = np.where(finite[:, None], b, 0.0)
    with np.errstate(over="ignore"):
        x, y, w, h = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
        x0, y0, x1, y1 = _clamped_floor(x), _clamped_floor(y), _clamped_floor(x + w), _clamped_floor(y + h)
        cx, cy = _clamped_floor(x + w * 0.5), _clamped_floor(y + h * 0.5)
    return x0, y0, x1, y1, cx, cy, finite & (x1 >= x0) & (y1 >= y0)


def detection_classes(matched50, ignored50):
    """The flags of a segment -> TP / FP / IGNORED per detection."""
    m, ig = np.asarray(matched50).astype(bool), np.asarray(ignored50).astype(bool)
    return np.where(ig, IGNORED, np.where(m, TP, FP)).astype(np.int64)


def primitives(dt_boxes, dt_class, gt_boxes, ex_boxes, style=DEFAULT_STYLE, dot=DEFAULT_DOT):
    """One canvas's primitives in PRIORITY order -> (rect int64 [P, 4] = x0, y0, x1, y1; thickness int64 [P]; class int64 [P]); a dot is the
    filled square of its radius (thickness = radius + 1).  Boxes that draw nothing are left out."""
    style = np.asarray(style, dtype=np.uint8).reshape(5, 4)
    dt_class = np.asarray(dt_class, dtype=np.int64).reshape(-1)
    rect, thick, cls = [], [], []
    dx0, dy0, dx1, dy1, cx, cy, ok = corners(dt_boxes)
    if dot >= 0:
        rect.append(np.stack([cx - dot, cy - dot, cx + dot, cy + dot], axis=1)[ok])
        thick.append(np.full(int(ok.sum()), dot + 1, dtype=np.int64))
        cls.append(dt_class[ok])
    rect.append(np.stack([dx0, dy0, dx1, dy1], axis=1)[ok])
    thick.append(style[dt_class[ok], 3].astype(np.int64))
    cls.append(dt_class[ok])
    for boxes, c in ((gt_boxes, GT), (ex_boxes, EXEMPLAR)):
        x0, y0, x1, y1, _, _, ok = corners(boxes)
        rect.append(np.stack([x0, y0, x1, y1], axis=1)[ok])
        thick.append(np.full(int(ok.sum()), int(style[c, 3]), dtype=np.int64))
        cls.append(np.full(int(ok.sum()), c, dtype=np.int64))
    return np.concatenate(rect).reshape(-1, 4), np.concatenate(thick), np.concatenate(cls)


def paint_first_hit(canvas, rect, thick, cls, style=DEFAULT_STYLE):
    """The host implementation for one canvas: the primitives in priority order, each colouring the pixels of its band that no earlier one
    has claimed.  -> a new uint8 [H, W, 3]."""
    style = np.asarray(style, dtype=np.uint8).reshape(5, 4)
    out = np.array(canvas, dtype=np.uint8, copy=True)
    H, W = out.shape[:2]
    claimed = np.zeros((H, W), dtype=bool)
    for (x0, y0, x1, y1), t, c in zip(rect.tolist(), thick.tolist(), cls.tolist()):
        ax0, ay0, ax1, ay1 = max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1)
        if ax0 > ax1 or ay0 > ay1 or t < 1:
            continue
        band = np.ones((ay1 - ay0 + 1, ax1 - ax0 + 1), dtype=bool)
        hx0, hy0, hx1, hy1 = max(x0 + t, ax0), max(y0 + t, ay0), min(x1 - t, ax1), min(y1 - t, ay1)       # the hole: min(...) >= t
        if hx0 <= hx1 and hy0 <= hy1:
            band[hy0 - ay0:hy1 - ay0 + 1, hx0 - ax0:hx1 - ax0 + 1] = False
        view = claimed[ay0:ay1 + 1, ax0:ax1 + 1]
        band &= ~view
        out[ay0:ay1 + 1, ax0:ax1 + 1][band] = style[c, :3]
        view |= band
    return out


def _segment(off, b):
    return int(off[b]), int(off[b + 1])


def _check_inputs(canvases, sel, B, exemplars, dot):
    canvases = [np.ascontiguousarray(c, dtype=np.uint8) for c in canvases]
    sel = [int(s) for s in sel]
    if len(sel) != len(canvases) or (exemplars is not None and len(exemplars) != len(canvases)):
        raise ValueError(f"render: {len(canvases)} canvases, {len(sel)} entries of sel, {None if exemplars is None else len(exemplars)} exemplar lists")
    for c in canvases:
        if c.ndim != 3 or c.shape[2] != 3 or not (1 <= c.shape[0] <= MAX_SIDE and 1 <= c.shape[1] <= MAX_SIDE):
            raise ValueError(f"render: a canvas is uint8 [H, W, 3] with H, W in 1 .. {MAX_SIDE}, got {c.shape}")
    for s in sel:
        if not 0 <= s < B:
            raise ValueError(f"render: sel names image {s} of a pack of {B}")
    if int(dot) > MAX_SIDE:
        raise ValueError(f"render: dot radius {dot} (limit {MAX_SIDE})")
    ex = [np.zeros((0, 4))] * len(canvases) if exemplars is None else [np.asarray(e, dtype=np.float64).reshape(-1, 4) for e in exemplars]
    return canvases, sel, ex


def render_images(canvases, pack, matched50, ignored50, sel, dt_cnt=None, exemplars=None, style=DEFAULT_STYLE, dot=DEFAULT_DOT, device=None):
    """Overlays of K canvases -> a list of K uint8 [H, W, 3] arrays (new; the canvases are not written).
    canvases : K uint8 [H, W, 3] arrays; sel[k] = the index in `pack` of the image canvas k shows (an image may be shown twice).
    pack     : coco_ap.pack_images' / pack_store's dict (gt_boxes, gt_off, dt_off; dt_boxes, or "dt_device" for a store).
    matched50, ignored50 : [D] flags of the pack's detections at area range `all`, IoU 0.5 (row [0, 0] of the matcher's outputs): arrays, or
               device tensors where the matching left them (device route).
    dt_cnt   : [B] draw only the first dt_cnt[b] detections of pack image b; None = all.
    exemplars: K arrays [n, 4] xywh, or None.
    device=None: the host implementation (a pack without dt_boxes, a store's, cannot be drawn there).  A CUDA device: one
    cdetr_render_boxes launch; the canvases (and the small tables) go up, the overlays come back, EQUAL to the host's."""
    style = np.ascontiguousarray(style, dtype=np.uint8).reshape(5, 4)
    B = len(pack["image_ids"])
    canvases, sel, ex = _check_inputs(canvases, sel, B, exemplars, dot)
    if dt_cnt is not None and len(dt_cnt) != B:
        raise ValueError(f"render: dt_cnt has {len(dt_cnt)} entries for a pack of {B} images")
    if device is not None:
        return _render_on_device(canvases, pack, matched50, ignored50, sel, dt_cnt, ex, style, int(dot), device)
    if "dt_boxes" not in pack:
        raise ValueError("render: the host implementation needs the pack's dt_boxes (a store's pack is drawn on its device)")
    cls = detection_classes(matched50, ignored50)
    out = []
    for canvas, b, e in zip(canvases, sel, ex):
        d0, d1 = _segment(pack["dt_off"], b)
        if dt_cnt is not None:
            d1 = d0 + min(d1 - d0, max(int(dt_cnt[b]), 0))
        g0, g1 = _segment(pack["gt_off"], b)
        out.append(paint_first_hit(canvas, *primitives(pack["dt_boxes"][d0:d1], cls[d0:d1], pack["gt_boxes"][g0:g1], e, style, int(dot)), style))
    return out


def device_inputs(canvases, pack, matched50, ignored50, sel, dt_cnt, ex, style, dot, device):
    """The uploads of one cdetr_render_boxes launch -> (keyword arguments of ops.render_boxes, pix_off int64 [K + 1] on the host).  The
    canvases go up as one buffer, the small tables as one more, the ground-truth and exemplar boxes as a third; the detections' boxes are the
    pack's "dt_device" where there is one, and flags given as device tensors are used where they lie.  Call it under torch.cuda.device(device)."""
    import torch
    K, B = len(canvases), len(pack["image_ids"])
    sizes = np.array([c.shape[:2] for c in canvases], dtype=np.int32).reshape(K, 2)
    pix_off = np.concatenate([[0], np.cumsum([c.size for c in canvases])]).astype(np.int64)
    ex_off = np.concatenate([[0], np.cumsum([len(e) for e in ex])]).astype(np.int32)
    cnt = np.zeros(0, np.int32) if dt_cnt is None else np.clip(np.asarray(dt_cnt, dtype=np.int64), 0, 2 ** 31 - 1).astype(np.int32)
    i32 = np.concatenate([sizes.reshape(-1), np.asarray(sel, dtype=np.int32), pack["dt_off"].astype(np.int32), pack["gt_off"].astype(np.int32), ex_off, cnt])
    cuts = np.cumsum([0, 2 * K, K, B + 1, B + 1, K + 1, len(cnt)])
    dt_dev = pack.get("dt_device")
    G, E = len(pack["gt_boxes"]), int(ex_off[-1])
    f64 = np.concatenate([pack["gt_boxes"].reshape(-1)] + [e.reshape(-1) for e in ex] + [np.zeros(0) if dt_dev is not None else pack["dt_boxes"].reshape(-1)])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)                     # noqa: E731
    i, f = up(i32), up(f64.astype(np.float64))
    d_size, d_sel, d_dt_off, d_gt_off, d_ex_off, d_cnt = (i[cuts[j]:cuts[j + 1]] for j in range(6))
    flags = [x if isinstance(x, torch.Tensor) else up(np.asarray(x).astype(np.uint8)) for x in (matched50, ignored50)]
    return dict(pix=up(np.concatenate([c.reshape(-1) for c in canvases])), pix_off=up(pix_off), size=d_size.view(K, 2), sel=d_sel,
                dt_boxes=dt_dev[0] if dt_dev is not None else f[4 * G + 4 * E:].view(-1, 4), dt_off=d_dt_off, matched50=flags[0], ignored50=flags[1],
                gt_boxes=f[:4 * G].view(-1, 4), gt_off=d_gt_off, ex_boxes=f[4 * G:4 * G + 4 * E].view(-1, 4), ex_off=d_ex_off, style=up(style),
                dot=int(dot), dt_cnt=None if dt_cnt is None else d_cnt, sel_host=[int(s) for s in sel],
                max_hw=(int(sizes[:, 0].max()), int(sizes[:, 1].max()))), pix_off


def _render_on_device(canvases, pack, matched50, ignored50, sel, dt_cnt, ex, style, dot, device):
    import torch
    from . import ops
    from .coco_ap import _cuda
    device = _cuda(device)
    if not canvases:
        return []
    with torch.cuda.device(device):
        kwargs, pix_off = device_inputs(canvases, pack, matched50, ignored50, sel, dt_cnt, ex, style, dot, device)
        host = ops.render_boxes(**kwargs).cpu().numpy()                                     # the one copy back: the overlays
    return [host[pix_off[k]:pix_off[k + 1]].reshape(canvases[k].shape) for k in range(len(canvases))]


def select(report, k, ids=()):
    """The images to render from coco_ap.image_report's dict -> [{"image_id", "reasons"}]: the first `k` of order_by_ap (lowest AP first, NaN
    last), then the `k` rows of largest |diff| (ties in the order the images were run), then `ids`; an image named more than once keeps its
    first place and collects its reasons, a subset of ["ap", "diff", "id"] in that order."""
    k = max(int(k), 0)
    rows = report["rows"]
    known = {r["image_id"] for r in rows}
    for i in ids:
        if i not in known:
            raise ValueError(f"render: image id {i} is not in the report ({len(rows)} images)")
    by_diff = sorted(range(len(rows)), key=lambda j: (-abs(rows[j]["diff"]), j))
    picks = [(i, "ap") for i in report["order_by_ap"][:k]] + [(rows[j]["image_id"], "diff") for j in by_diff[:k]] + [(i, "id") for i in ids]
    out, at = [], {}
    for i, why in picks:
        if i not in at:
            at[i] = len(out)
            out.append({"image_id": i, "reasons": []})
        if why not in out[at[i]]["reasons"]:
            out[at[i]]["reasons"].append(why)
    return out


def exemplar_boxes(anno):
    """An annotation_FSC147_384.json entry -> its exemplars as float64 [n, 4] = x1, y1, x2 - x1, y2 - y1, in file order."""
    return np.array([[b[0][0], b[0][1], b[2][0] - b[0][0], b[2][1] - b[0][1]] for b in anno.get("box_examples_coordinates", [])],
                    dtype=np.float64).reshape(-1, 4)


def load_canvases(data_path, split, image_ids):
    """-> (canvases, file names, exemplars) of the images `image_ids` of a split: instances_<split>.json names the files under
    images_384_VarV2/, annotation_FSC147_384.json holds the exemplars."""
    from PIL import Image
    with open(os.path.join(data_path, "instances_" + split + ".json")) as f:
        names = {im["id"]: im["file_name"] for im in json.load(f)["images"]}
    with open(os.path.join(data_path, "annotation_FSC147_384.json")) as f:
        anno = json.load(f)
    files = [names[i] for i in image_ids]
    canvases = [np.asarray(Image.open(os.path.join(data_path, "images_384_VarV2", fn)).convert("RGB"), dtype=np.uint8) for fn in files]
    return canvases, files, [exemplar_boxes(anno.get(fn, {})) for fn in files]


def write(output_dir, split, threshold, picks, files, report, overlays, style=DEFAULT_STYLE, dot=DEFAULT_DOT):
    """render_<split>/<image_id>.png for every pick and render_<split>/index.json: {"split", "threshold", "style", "dot", "images":
    [{"image_id", "file_name", "png", "reasons", "row"}]}, `row` = the image's row of the report."""
    from PIL import Image
    out_dir = os.path.join(output_dir, "render_" + split)
    os.makedirs(out_dir, exist_ok=True)
    for old in os.listdir(out_dir):                                             # an earlier pass's overlays: the directory shows ONE pass
        if old == "index.json" or (old.endswith(".png") and old[:-4].lstrip("-").isdigit()):
            os.remove(os.path.join(out_dir, old))
    rows ={r["image_id"]: r for r in report["rows"]}
    images = []
    for p, fn, a in zip(picks, files, overlays):
        png = f"{p['image_id']}.png"
        Image.fromarray(a).save(os.path.join(out_dir, png))
        images.append({"image_id": p["image_id"], "file_name": fn, "png": png, "reasons": list(p["reasons"]), "row": rows[p["image_id"]]})
    with open(os.path.join(out_dir, "index.json"), "w") as handle:
        json.dump({"split": split, "threshold": float(threshold), "style": np.asarray(style).astype(int).tolist(), "dot": int(dot), "images": images},
                  handle)
    return out_dir
