"""FSC-147 readers + batched collate for the 2nd-stage step.

Sample semantics follow the reference's dataset classes field by field:
  train  A2/data/fsc147.py:12-102   pseudo-label COCO json `annotations/pseudo_bbox_<split>.json` (bbox = [cx, cy, w, h] in pixels),
                                    exemplar rectangles from `annotation_FSC147_384.json`, image resized to floor(w/32)*32 x
                                    floor(h/32)*32 with PIL's default filter, ToTensor + ImageNet normalisation, boxes / rects
                                    divided by (w, h, w, h);
  val    A2/data/fsc147.py:105-211  `instances_val.json` (bbox = [x1, y1, w, h]) -> centre boxes, points, xyxy boxes; resize to a
  test   A2/data/fsc147.py:214-351  multiple of `scale_factor` with BILINEAR.
Differences (MI355X-first): no pycocotools (the COCO json is indexed directly); any number of images per step
(`collate` pads to the batch maximum and builds the padding mask the model consumes, the reference is batch-1 only);
`Prefetcher` stages the next batch through pinned memory on a side stream while the current step runs (the pattern the
reference sketches in A1/datasets/data_prefetcher.py:23-79 and never uses).
Optional (`--device_preprocess`): readers built with raw=True only decode; `collate_raw` / `collate_stage1_raw` pack the un-resized uint8
pixels with Pillow's resampling coefficients (`resample_tables`), and `Prefetcher` turns them into the SAME image / mask tensors, bit
for bit, with one cdetr_image_prep launch on its stream (ops.image_prep).
"""
import functools
import json
import math
import os

import numpy as np
import torch
from PIL import Image
from torch.utils.data import Dataset

MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)


def to_normalized_tensor(img):
    """transforms.ToTensor() + Normalize(ImageNet) of a PIL image -> float32 [3,H,W] (A2/data/fsc147.py:22-24)."""
    a = np.array(img.convert("RGB"), dtype=np.uint8)
    t = torch.from_numpy(a).permute(2, 0, 1).to(torch.float32).div(255.0)
    return (t - torch.from_numpy(MEAN).view(3, 1, 1)) / torch.from_numpy(STD).view(3, 1, 1)


# ---- device-side resize + normalise + pad (csrc/image_prep.hip): what the host has to prepare -------------------------------------
# limits of the kernel's LDS tile, as include/cdetr_hip.h states them (CDETR_IMAGE_PREP_*; tests/test_image_prep_cpu.py compares)
IMAGE_PREP_TILE_H, IMAGE_PREP_MAX_TAPS, IMAGE_PREP_MAX_ROWS, IMAGE_PREP_RECORD_INTS = 32, 20, 160, 12
_PRECISION_BITS = 22                                                   # Pillow: 32 - 8 - 2


def _resample_filter(filter, x):
    """Pillow's bicubic (a = -0.5) / bilinear kernels (src/libImaging/Resample.c), operation by operation, on a float64 array."""
    x = np.abs(x)
    if filter == Image.BICUBIC:
        near = ((-0.5 + 2.0) * x - (-0.5 + 3.0)) * x * x + 1
        far = (((x - 5) * x + 8) * x - 4) * -0.5
        return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))
    if filter == Image.BILINEAR:
        return np.where(x < 1.0, 1.0 - x, 0.0)
    raise ValueError(f"resample_tables: filter {filter} is not resampled on the device (bicubic and bilinear are)")


@functools.lru_cache(maxsize=1024)
def resample_tables(in_size, out_size, filter):
    """Pillow's 8-bit resampling coefficients of one axis (precompute_coeffs + normalize_coeffs_8bpc of its C resampler) ->
    (bounds int32 [out, 2] = (first source sample, number of taps), coeffs int32 [out, ksize], 22 fractional bits; read-only arrays).
    in_size == out_size gives the identity table (one tap of 2^22): Pillow skips such an axis, the identity leaves the same bytes.
    Cached per argument triple: a dataset has few distinct sizes."""
    in_size, out_size, filter = int(in_size), int(out_size), int(filter)
    if in_size <= 0 or out_size <= 0:
        raise ValueError(f"resample_tables: sizes must be positive, got {in_size} -> {out_size}")
    if in_size == out_size:
        bounds = np.stack([np.arange(out_size), np.ones(out_size, dtype=np.int64)], axis=1).astype(np.int32)
        coeffs = np.full((out_size, 1), 1 << _PRECISION_BITS, dtype=np.int32)
    else:
        _resample_filter(filter, np.zeros(1))                          # refuses an unknown filter
        scale = in_size / out_size
        fs = max(scale, 1.0)
        support = (2.0 if filter == Image.BICUBIC else 1.0) * fs
        ksize = int(math.ceil(support)) * 2 + 1
        center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
        xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)            # (int): truncation towards zero
        xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
        x = np.arange(ksize, dtype=np.int64)[None, :]
        w = _resample_filter(filter, ((x + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * (1.0 / fs))
        w = np.where(x < xmax[:, None], w, 0.0)
        ww = np.zeros(out_size, dtype=np.float64)
        for k in range(ksize):                                         # left to right, as the C loop adds them (numpy.sum adds pairwise)
            ww = ww + w[:, k]
        w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
        q = w * float(1 << _PRECISION_BITS)
        coeffs = np.where(w < 0, -0.5 + q, 0.5 + q).astype(np.int64).astype(np.int32)
        bounds = np.stack([xmin, xmax], axis=1).astype(np.int32)
    bounds.setflags(write=False)
    coeffs.setflags(write=False)
    return bounds, coeffs


@functools.lru_cache(maxsize=1024)
def _tile_rows(in_size, out_size, filter):
    """Largest number of source rows that IMAGE_PREP_TILE_H consecutive output rows (one tile of the kernel) reach on this axis."""
    b = resample_tables(in_size, out_size, filter)[0].astype(np.int64)
    first = np.arange(0, out_size, IMAGE_PREP_TILE_H)
    last = np.minimum(first + IMAGE_PREP_TILE_H, out_size) - 1
    return int((b[last, 0] + b[last, 1] - b[first, 0]).max())


def image_prep_supports(in_wh, out_wh, filter):
    """Whether cdetr_image_prep resamples (in_w, in_h) -> (out_w, out_h) itself: bicubic or bilinear, taps and tile rows within the
    kernel's LDS tile (downscales up to 4x per axis, any upscale).  Anything else is resized on the host by collate_raw."""
    (iw, ih), (ow, oh) = in_wh, out_wh
    if filter not in (Image.BICUBIC, Image.BILINEAR) or min(iw, ih, ow, oh) <= 0:
        return (iw, ih) == (ow, oh) and min(iw, ih) > 0
    return (resample_tables(iw, ow, filter)[1].shape[1] <= IMAGE_PREP_MAX_TAPS and resample_tables(ih, oh, filter)[1].shape[1] <= IMAGE_PREP_MAX_TAPS
            and _tile_rows(ih, oh, filter) <= IMAGE_PREP_MAX_ROWS)


@functools.lru_cache(maxsize=1)
def norm_table():
    """fp32 [3, 256]: to_normalized_tensor's value of byte v in channel c -- computed BY to_normalized_tensor on the 256 grey levels,
    so the device's table lookup equals the host's arithmetic whatever rounding either would choose."""
    a = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)                 # a 1 x 256 RGB image, pixel v = (v, v, v)
    return to_normalized_tensor(Image.fromarray(a)).reshape(3, 256).contiguous()


def _raw_image(img, size, resample=None):
    """The image fields of a raw=True sample: `image_raw` (contiguous uint8 [h, w, 3] RGB, as decoded), `resize_to` (w, h) and `resample`
    (PIL filter) -- the resize the reader would have made -- and `host_resized`.  Modes RGB and L (replicated to RGB: resizing commutes
    with the replication) go to the device as decoded; any other mode (P, 1, RGBA, I;16, ...) is resized here by the reader's own PIL
    call and passed on with an identity `resize_to`."""
    host = img.mode not in ("RGB", "L")
    if host:
        img = img.resize(size) if resample is None else img.resize(size, resample)
        size = img.size
    a = np.ascontiguousarray(np.asarray(img.convert("RGB"), dtype=np.uint8))
    return {"image_raw": a, "resize_to": (int(size[0]), int(size[1])), "resample": int(Image.BICUBIC if resample is None else resample),
            "host_resized": host}


def _image_fields(img, size, resample, raw):
    """{"image": ...} of the default readers, or the raw=True fields; `resample` None = PIL's default filter (the training readers)."""
    if raw:
        return _raw_image(img, size, resample)
    return {"image": to_normalized_tensor(img.resize(size) if resample is None else img.resize(size, resample))}


class CocoIndex:
    """The four pycocotools.COCO calls the reference uses (getImgIds / loadImgs / getAnnIds / loadAnns / .imgs)."""

    def __init__(self, path):
        with open(path, "r") as f:
            d = json.load(f)
        self.imgs = {im["id"]: im for im in d.get("images", [])}
        self.anns = {}
        self._by_img = {}
        for a in d.get("annotations", []):
            self.anns[a["id"]] = a
            self._by_img.setdefault(a["image_id"], []).append(a["id"])

    def getImgIds(self):
        return list(self.imgs.keys())

    def loadImgs(self, ids):
        return [self.imgs[i] for i in ids]

    def getAnnIds(self, img_ids):
        out = []
        for i in img_ids:
            out += self._by_img.get(i, [])
        return out

    def loadAnns(self, ids):
        return [self.anns[i] for i in ids]


def _load_json(path):
    with open(path, "r") as f:
        return json.load(f)


def _exemplar_rects(anno):
    """box_examples_coordinates: four corner points per exemplar -> [x1, y1, x2, y2] (A2/data/fsc147.py:52-61)."""
    return np.array([[b[0][0], b[0][1], b[2][0], b[2][1]] for b in anno["box_examples_coordinates"]], dtype=np.float32)


class FSC147Dataset(Dataset):
    """Training split (A2/data/fsc147.py:12-102)."""

    def __init__(self, args, split="train", raw=False):
        data_path = args.data_path
        self.raw = raw
        self.coco = CocoIndex(os.path.join(data_path, "annotations", "pseudo_bbox_" + split + ".json"))
        self.images = self.coco.getImgIds()
        self.img_path = os.path.join(data_path, "images_384_VarV2")
        self.annotations = _load_json(os.path.join(data_path, "annotation_FSC147_384.json"))

    def __len__(self):
        return len(self.images)

    def __getitem__(self, index):
        img_info = self.coco.loadImgs([self.images[index]])[0]
        img_file = img_info["file_name"]
        img = Image.open(os.path.join(self.img_path, img_file))
        wh = img.size
        anns = self.coco.loadAnns(self.coco.getAnnIds([self.images[index]]))
        bboxes = np.array([a["bbox"] for a in anns], dtype=np.float32).reshape(-1, 4)
        ex_rects = _exemplar_rects(self.annotations[img_file])
        img_w, img_h = img.size
        image = _image_fields(img, (32 * int(img_w / 32), 32 * int(img_h / 32)), None, self.raw)      # :75-77 (PIL default filter)
        res = np.array([img_w, img_h, img_w, img_h], dtype=np.float32)
        bboxes = bboxes / res[None, :]
        xyxy = np.zeros_like(bboxes)
        xyxy[:, 0], xyxy[:, 1] = bboxes[:, 0] - bboxes[:, 2] / 2, bboxes[:, 1] - bboxes[:, 3] / 2
        xyxy[:, 2], xyxy[:, 3] = bboxes[:, 0] + bboxes[:, 2] / 2, bboxes[:, 1] + bboxes[:, 3] / 2
        return {**image, "boxes": bboxes, "ex_rects": ex_rects / res[None, :], "origin_wh": wh,
                "labels": torch.zeros([bboxes.shape[0]], dtype=torch.int64), "orig_size": np.array([img_h, img_w]),
                "xyxy_boxes": xyxy}


class FSC147EvalDataset(Dataset):
    """Validation / test split (A2/data/fsc147.py:105-211, :214-351): `instances_<split>.json` ground truth."""

    def __init__(self, args, split="val", raw=False):
        data_path = args.data_path
        self.raw = raw
        self.im_dir = os.path.join(data_path, "images_384_VarV2")
        self.scale_factor = args.scale_factor
        self.annotations = _load_json(os.path.join(data_path, "annotation_FSC147_384.json"))
        self.data_split = _load_json(os.path.join(data_path, "Train_Test_Val_FSC_147.json"))[split]
        self.label = CocoIndex(os.path.join(data_path, f"instances_{split}.json"))
        self.name2id = {v["file_name"]: v["id"] for v in self.label.imgs.values()}

    def __len__(self):
        return len(self.data_split)

    def __getitem__(self, idx):
        name = self.data_split[idx]
        im_id = self.name2id[name]
        annos = self.label.loadAnns(self.label.getAnnIds([im_id]))
        centers = np.array([[a["bbox"][0] + a["bbox"][2] / 2, a["bbox"][1] + a["bbox"][3] / 2] for a in annos], dtype=np.float32).reshape(-1, 2)
        whs = np.array([[a["bbox"][2], a["bbox"][3]] for a in annos], dtype=np.float32).reshape(-1, 2)
        xyxy = np.array([[a["bbox"][0], a["bbox"][1], a["bbox"][0] + a["bbox"][2], a["bbox"][1] + a["bbox"][3]] for a in annos],
                        dtype=np.float32).reshape(-1, 4)
        ex = _exemplar_rects(self.annotations[name])
        image = Image.open("{}/{}".format(self.im_dir, name))
        img_w, img_h = image.size
        res4 = np.array([img_w, img_h, img_w, img_h], dtype=np.float32)
        sf = self.scale_factor
        image = _image_fields(image, (sf * int(img_w / sf), sf * int(img_h / sf)), Image.BILINEAR, self.raw)
        return {"image_id": im_id, **image, "points": centers / res4[None, :2],
                "boxes": np.concatenate((centers, whs), axis=1) / res4[None, :], "orig_size": np.array([img_h, img_w]),
                "exemplar_boxes": ex / res4[None, :], "labels": np.zeros(centers.shape[0], dtype=np.int64),
                "xyxy_boxes": xyxy / res4[None, :]}


class FSCDLVISDataset(Dataset):
    """FSCD-LVIS train / test readers (BASELINE config 4; L2/data/fscd_lvis.py:12-100, :103-190): same network, different
    files -- `annotations_old/pseudo_lvis_<split>_cxcywh.json` (train) or `single_instances_<split>.json` (test), exemplars
    from `count_<split>.json` (first three [x, y, w, h] boxes, clipped to the image on the training split only), RGB convert."""

    def __init__(self, args, split="train", test=False, raw=False):
        data_path = args.data_path
        self.raw = raw
        name = ("single_instances_" + split + ".json") if test else ("pseudo_lvis_" + split + "_cxcywh.json")
        self.coco = CocoIndex(os.path.join(data_path, "annotations_old", name))
        self.image_ids = self.coco.getImgIds()
        self.img_path = os.path.join(data_path, "images", "all_images")
        self.count_anno = _load_json(os.path.join(data_path, "annotations_old", "count_" + split + ".json"))
        self.clip = not test

    def __len__(self):
        return len(self.image_ids)

    def __getitem__(self, idx):
        img_id = self.image_ids[idx]
        img_file = self.coco.loadImgs([img_id])[0]["file_name"]
        img = Image.open(os.path.join(self.img_path, img_file)).convert("RGB")
        wh = img.size
        anns = self.coco.loadAnns(self.coco.getAnnIds([img_id]))
        bboxes = np.array([a["bbox"] for a in anns], dtype=np.float32).reshape(-1, 4)
        ex = np.array([[x, y, x + w, y + h] for x, y, w, h in self.count_anno["annotations"][idx]["boxes"][:3]], dtype=np.float32)
        if self.clip:                                                                    # L2/data/fscd_lvis.py:60-63
            ex[:, 0] = np.clip(ex[:, 0], 0, wh[0] - 1); ex[:, 1] = np.clip(ex[:, 1], 0, wh[1] - 1)
            ex[:, 2] = np.clip(ex[:, 2], 0, wh[0] - 1); ex[:, 3] = np.clip(ex[:, 3], 0, wh[1] - 1)
        img_w, img_h = wh
        image = _image_fields(img, (32 * int(img_w / 32), 32 * int(img_h / 32)), None, self.raw)
        res = np.array([img_w, img_h, img_w, img_h], dtype=np.float32)
        bboxes = bboxes / res[None, :]
        return {**image, "boxes": bboxes, "ex_rects": ex / res[None, :], "origin_wh": wh,
                "labels": torch.zeros([bboxes.shape[0]], dtype=torch.int64), "orig_size": np.array([img_h, img_w])}


def _exemplar_centres_whs(anno):
    """box_examples_coordinates -> exemplar centres and sizes in pixels, float32 [K,2] each (A1/datasets/fscd_147.py:37-49)."""
    c, wh = [], []
    for b in anno["box_examples_coordinates"]:
        x1, y1, x2, y2 = b[0][0], b[0][1], b[2][0], b[2][1]
        c.append([(x1 + x2) / 2, (y1 + y2) / 2])
        wh.append([x2 - x1, y2 - y1])
    return np.array(c, dtype=np.float32).reshape(-1, 2), np.array(wh, dtype=np.float32).reshape(-1, 2)


class FSC147ExemplarDataset(Dataset):
    """1st-stage training / validation reader (A1/datasets/fscd_147.py:11-73, FSCD147_Exemplars): the exemplar boxes of an image as
    points (centres) + whs (sizes), both divided by the ORIGINAL image size; the image resized to floor(w/32)*32 x floor(h/32)*32 with
    BILINEAR, ToTensor + ImageNet normalisation."""

    def __init__(self, args, split="train", raw=False):
        data_path = args.data_path
        self.raw = raw
        self.im_dir = os.path.join(data_path, "images_384_VarV2")
        self.annotations = _load_json(os.path.join(data_path, "annotation_FSC147_384.json"))
        self.data_split = _load_json(os.path.join(data_path, "Train_Test_Val_FSC_147.json"))[split]

    def __len__(self):
        return len(self.data_split)

    def __getitem__(self, idx):
        im_id = self.data_split[idx]
        centres, whs = _exemplar_centres_whs(self.annotations[im_id])
        image = Image.open(os.path.join(self.im_dir, im_id))
        img_w, img_h = image.size
        image = _image_fields(image, (32 * int(img_w / 32), 32 * int(img_h / 32)), Image.BILINEAR, self.raw)
        res = np.array([img_w, img_h], dtype=np.float32)
        return {**image, "points": centres / res[None, :], "whs": whs / res[None, :],
                "labels": np.zeros(centres.shape[0], dtype=np.int64), "orig_size": np.array([img_w, img_h])}


class FSC147PointsDataset(Dataset):
    """Pseudo-label reader (A1/datasets/fscd_147.py:76-136, FSCD147_Points): every annotated dot of an image (normalised by the original
    size), the exemplar centres as `anchor_points`, orig_size = (width, height) and the numeric image id -- what
    stage1.write_pseudo_labels consumes.  Image resized to a multiple of `scale_factor` with BILINEAR."""

    def __init__(self, args, split="train", raw=False):
        data_path = args.data_path
        self.raw = raw
        self.im_dir = os.path.join(data_path, "images_384_VarV2")
        self.scale_factor = getattr(args, "scale_factor", 32)
        self.annotations = _load_json(os.path.join(data_path, "annotation_FSC147_384.json"))
        self.data_split = _load_json(os.path.join(data_path, "Train_Test_Val_FSC_147.json"))[split]

    def __len__(self):
        return len(self.data_split)

    def point_counts(self):
        """Annotated dots per image, in dataset order, without opening an image (sizes stage1's device label store)."""
        return [len(self.annotations[im_id]["points"]) for im_id in self.data_split]

    def __getitem__(self, idx):
        im_id = self.data_split[idx]
        anno = self.annotations[im_id]
        all_points = np.array(anno["points"], dtype=np.float32).reshape(-1, 2)
        centres, _ = _exemplar_centres_whs(anno)
        image = Image.open(os.path.join(self.im_dir, im_id))
        img_w, img_h = image.size
        res = np.array([img_w, img_h], dtype=np.float32)
        sf = self.scale_factor
        image = _image_fields(image, (sf * int(img_w / sf), sf * int(img_h / sf)), Image.BILINEAR, self.raw)
        return {"im_id": int(im_id[:-4]), **image, "points": all_points / res[None, :],
                "labels": np.zeros(all_points.shape[0], dtype=np.int64), "anchor_points": centres / res[None, :],
                "orig_size": np.array([img_w, img_h])}


class FSC147BoxPointsDataset(Dataset):
    """The 1st-stage view of a split that has box ground truth (A1/datasets/fscd_147.py:150-242, FSCD147_Test, with the split's own
    `instances_<split>.json`): the fields of FSC147PointsDataset with `points` = the centres of the ground-truth boxes (normalised by the
    original size with FSC147EvalDataset's arithmetic), plus `gt_xywh` float64 [P,4] = the json's [x1, y1, w, h] untouched and `image_id` =
    the json's image id -- what main_stage1.py --test forwards and pairs the predicted sizes with."""

    def __init__(self, args, split="val", raw=False):
        data_path = args.data_path
        self.raw = raw
        self.im_dir = os.path.join(data_path, "images_384_VarV2")
        self.scale_factor = getattr(args, "scale_factor", 32)
        self.annotations = _load_json(os.path.join(data_path, "annotation_FSC147_384.json"))
        self.data_split = _load_json(os.path.join(data_path, "Train_Test_Val_FSC_147.json"))[split]
        self.label = CocoIndex(os.path.join(data_path, f"instances_{split}.json"))
        self.name2id = {v["file_name"]: v["id"] for v in self.label.imgs.values()}

    def __len__(self):
        return len(self.data_split)

    def point_counts(self):
        """Ground-truth boxes per image, in dataset order, without opening an image (sizes stage1's device label store)."""
        return [len(self.label.getAnnIds([self.name2id[name]])) for name in self.data_split]

    def __getitem__(self, idx):
        name = self.data_split[idx]
        image_id = self.name2id[name]
        annos = self.label.loadAnns(self.label.getAnnIds([image_id]))
        centers = np.array([[a["bbox"][0] + a["bbox"][2] / 2, a["bbox"][1] + a["bbox"][3] / 2] for a in annos], dtype=np.float32).reshape(-1, 2)
        gt_xywh = np.array([a["bbox"] for a in annos], dtype=np.float64).reshape(-1, 4)
        anchors, _ = _exemplar_centres_whs(self.annotations[name])
        image = Image.open(os.path.join(self.im_dir, name))
        img_w, img_h = image.size
        res4 = np.array([img_w, img_h, img_w, img_h], dtype=np.float32)
        sf = self.scale_factor
        image = _image_fields(image, (sf * int(img_w / sf), sf * int(img_h / sf)), Image.BILINEAR, self.raw)
        return {"im_id": int(name[:-4]), "image_id": image_id, **image, "points": centers / res4[None, :2],
                "labels": np.zeros(centers.shape[0], dtype=np.int64), "anchor_points": anchors / res4[None, :2],
                "orig_size": np.array([img_w, img_h]), "gt_xywh": gt_xywh}


def collate_stage1(samples):
    """List of 1st-stage samples -> batch dict: images padded to the batch maximum with the padding mask (as `collate`), points and whs
    stacked to [B,N,2] (every image of a batch needs the same number N of exemplars / points: the step pairs query n with exemplar n),
    orig_size [B,2]; im_id [B] when the samples carry it."""
    _check_stage1_counts(samples)
    image, mask = _pad_images(samples)
    return {"image": image, "mask": mask, **_stage1_fields(samples)}


def _check_stage1_counts(samples):
    counts = [np.asarray(s["points"]).reshape(-1, 2).shape[0] for s in samples]
    if len(set(counts)) != 1:
        raise ValueError(f"collate_stage1: the images of a batch hold different numbers of points {counts}; batch them by count "
                         "(or use batch size 1, the reference's)")


def _pad_images(samples):
    """The samples' image tensors zero-padded to the batch maximum + the padding mask (True = padding)."""
    B = len(samples)
    Hm = max(s["image"].shape[1] for s in samples)
    Wm = max(s["image"].shape[2] for s in samples)
    image = torch.zeros((B, 3, Hm, Wm), dtype=torch.float32)
    mask = torch.ones((B, Hm, Wm), dtype=torch.bool)
    for b, s in enumerate(samples):
        _, h, w = s["image"].shape
        image[b, :, :h, :w] = s["image"]
        mask[b, :h, :w] = False
    return image, mask


def _stage1_fields(samples):
    """Everything of a 1st-stage batch but the image and its mask."""
    out = {"points": torch.stack([torch.as_tensor(s["points"], dtype=torch.float32).reshape(-1, 2) for s in samples]),
           "orig_size": torch.as_tensor(np.stack([np.asarray(s["orig_size"]) for s in samples]))}
    if "whs" in samples[0]:
        out["whs"] = torch.stack([torch.as_tensor(s["whs"], dtype=torch.float32).reshape(-1, 2) for s in samples])
    if "im_id" in samples[0]:
        out["im_id"] = torch.as_tensor([int(s["im_id"]) for s in samples])
    if "gt_xywh" in samples[0]:                # FSC147BoxPointsDataset
        out["gt_xywh"] = torch.stack([torch.as_tensor(s["gt_xywh"], dtype=torch.float64).reshape(-1, 4) for s in samples])
        out["image_id"] = torch.as_tensor([int(s["image_id"]) for s in samples])
    return out


RAGGED_POINT_FILL = 0.5        # padded points sit in the image centre: finite through inverse_sigmoid and the sine embeddings


def _stage1_ragged_fields(samples):
    """_stage1_fields for samples with different numbers of points: points / whs padded to the batch maximum N with (0.5, 0.5) / 0 and
    `counts` int32 [B] = each image's own number; rows n >= counts[b] of image b are padding."""
    pts = [torch.as_tensor(s["points"], dtype=torch.float32).reshape(-1, 2) for s in samples]
    counts = [p.shape[0] for p in pts]
    if min(counts) == 0:
        raise ValueError(f"collate_stage1_ragged: an image without points (counts {counts}); every image needs at least one")
    B, N = len(samples), max(counts)
    out = {"points": torch.full((B, N, 2), RAGGED_POINT_FILL, dtype=torch.float32), "counts": torch.tensor(counts, dtype=torch.int32),
           "orig_size": torch.as_tensor(np.stack([np.asarray(s["orig_size"]) for s in samples]))}
    for b, p in enumerate(pts):
        out["points"][b, :counts[b]] = p
    if "whs" in samples[0]:
        out["whs"] = torch.zeros((B, N, 2), dtype=torch.float32)
        for b, s in enumerate(samples):
            out["whs"][b, :counts[b]] = torch.as_tensor(s["whs"], dtype=torch.float32).reshape(-1, 2)
    if "im_id" in samples[0]:
        out["im_id"] = torch.as_tensor([int(s["im_id"]) for s in samples])
    if "gt_xywh" in samples[0]:                # FSC147BoxPointsDataset: the ground-truth boxes, padded with zeros like whs
        out["gt_xywh"] = torch.zeros((B, N, 4), dtype=torch.float64)
        for b, s in enumerate(samples):
            out["gt_xywh"][b, :counts[b]] = torch.as_tensor(s["gt_xywh"], dtype=torch.float64).reshape(-1, 4)
        out["image_id"] = torch.as_tensor([int(s["image_id"]) for s in samples])
    return out


def collate_stage1_ragged(samples):
    """`collate_stage1` for images with different numbers of points: the same image / mask, points and whs padded to the batch maximum
    (_stage1_ragged_fields) and `counts` [B] -- what Stage1Trainer.step(..., counts=) and stage1.write_pseudo_labels take."""
    fields = _stage1_ragged_fields(samples)
    image, mask = _pad_images(samples)
    return {"image": image, "mask": mask, **fields}


def collate_stage1_ragged_raw(samples):
    """`collate_stage1_ragged` for raw=True samples (see collate_raw)."""
    fields = _stage1_ragged_fields(samples)
    return {"raw": pack_raw(samples), **fields}


class SizeBucketBatchSampler(torch.utils.data.Sampler):
    """Batches of dataset indices whose images share ONE resized size, for batched pseudo-label generation: a padded image changes
    the key means (they run over padded rows and columns too, as in the reference's padded batches), so batches of one size keep the
    batched labels equal to the batch-1 labels up to arithmetic noise.  The sizes come from the image headers (no decode) through the
    dataset's own rule floor(w / sf) * sf; sizes in order of first appearance, dataset order within a size, the last batch of a size may
    be short: the same batches on every pass."""

    def __init__(self, dataset, batch_size):
        if batch_size < 1:
            raise ValueError(f"batch_size must be at least 1, got {batch_size}")
        sf = getattr(dataset, "scale_factor", 32)
        buckets = {}
        for idx, im_id in enumerate(dataset.data_split):
            with Image.open(os.path.join(dataset.im_dir, im_id)) as im:
                w, h = im.size
            buckets.setdefault((sf * int(w / sf), sf * int(h / sf)), []).append(idx)
        self.sizes = []
        self.batches = []
        for size, idxs in buckets.items():
            for i in range(0, len(idxs), batch_size):
                self.batches.append(idxs[i:i + batch_size])
                self.sizes.append(size)

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


def build_dataset_stage1(args, image_set="train", raw=False):
    return FSC147ExemplarDataset(args, split=image_set, raw=raw)


def build_points_dataset(args, image_set="train", raw=False):
    return FSC147PointsDataset(args, split=image_set, raw=raw)


def build_box_points_dataset(args, image_set="val", raw=False):
    return FSC147BoxPointsDataset(args, split=image_set, raw=raw)


def build_dataset(args, raw=False):
    if getattr(args, "dataset", "fsc147") == "fscd_lvis":
        return FSCDLVISDataset(args, split="train", raw=raw)
    return FSC147Dataset(args, raw=raw)


def build_test_dataset(args, image_set="val", raw=False):
    return FSC147EvalDataset(args, split="val" if image_set == "val" else "test", raw=raw)


def collate(samples):
    """List of dataset samples -> the step's batch dict: images padded to the batch maximum with the padding mask
    (NestedTensor convention: True = padding), exemplar rectangles [B,3,4], per-image target dicts."""
    image, mask = _pad_images(samples)
    return {"image": image, "mask": mask, **_stage2_fields(samples)}


def _stage2_fields(samples):
    """Everything of a 2nd-stage batch but the image and its mask."""
    rk = "ex_rects" if "ex_rects" in samples[0] else "exemplar_boxes"
    rl = [torch.as_tensor(s[rk], dtype=torch.float32).reshape(-1, 4)[:3] for s in samples]
    # FSCD-LVIS has "at most 3" exemplars (L2/data/fscd_lvis.py:53): absent rows are marked with -1 (backbone per_image mode skips them)
    rects = torch.stack([torch.cat([r, torch.full((3 - r.shape[0], 4), -1.0)]) if r.shape[0] < 3 else r for r in rl])
    targets = [{"boxes": torch.as_tensor(s["boxes"], dtype=torch.float32).reshape(-1, 4),
                "labels": torch.as_tensor(s["labels"], dtype=torch.int64).reshape(-1)} for s in samples]
    out = {"ex_rects": rects, "targets": targets,
           "orig_size": torch.as_tensor(np.stack([np.asarray(s["orig_size"]) for s in samples]))}
    if "image_id" in samples[0]:
        out["image_id"] = torch.as_tensor([int(s["image_id"]) for s in samples])
    return out


def pack_raw(samples):
    """raw=True samples -> the `raw` part of a batch, what cdetr_image_prep reads (include/cdetr_hip.h), all of it torch tensors or ints:
    `pixels` uint8 (every image's [h, w, 3] bytes, each start 16-byte aligned), `images` int32 [B, 12] (per image: byte offset, in_h, in_w,
    out_h, out_w, then offset of bounds / offset of coeffs / taps for the horizontal and the vertical axis), `tables` int32 (the
    resample_tables of the batch, each distinct one stored once), `lut` fp32 [3, 256] (norm_table), Hm, Wm (the padded size),
    max_taps, max_rows (what the kernel's tile must hold) and `device_resampled`: the number of images that reach the device as decoded.
    An image whose scale is outside the kernel's range (image_prep_supports) is resized here with PIL and packed with identity tables."""
    B = len(samples)
    records = np.zeros((B, IMAGE_PREP_RECORD_INTS), dtype=np.int32)
    arrays, tables, where = [], [], {}
    n_pix = n_tab = max_taps = max_rows = n_host = 0

    def table(in_size, out_size, filt):
        nonlocal n_tab, max_taps
        key = (in_size, out_size, filt if in_size != out_size else 0)
        if key not in where:
            bounds, coeffs = resample_tables(in_size, out_size, filt)
            where[key] = (n_tab, n_tab + bounds.size, coeffs.shape[1])
            tables.extend([bounds.reshape(-1), coeffs.reshape(-1)])
            n_tab += bounds.size + coeffs.size
        max_taps = max(max_taps, where[key][2])
        return where[key]

    for b, s in enumerate(samples):
        a, (ow, oh), filt = s["image_raw"], s["resize_to"], int(s["resample"])
        host = bool(s.get("host_resized", False))
        if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
            raise ValueError(f"pack_raw: image_raw must be uint8 [h, w, 3], got {a.dtype} {a.shape}")
        if not image_prep_supports((a.shape[1], a.shape[0]), (ow, oh), filt):
            a = np.asarray(Image.fromarray(a).resize((ow, oh), filt), dtype=np.uint8)
            host = True
        ih, iw = a.shape[:2]
        n_host += host
        records[b, :5] = (n_pix, ih, iw, oh, ow)
        records[b, 5:8] = table(iw, ow, filt)
        records[b, 8:11] = table(ih, oh, filt)
        max_rows = max(max_rows, _tile_rows(ih, oh, filt))
        arrays.append(a)
        n_pix += (a.size + 15) // 16 * 16
    if n_pix >= 2 ** 31 or n_tab >= 2 ** 31:
        raise ValueError(f"pack_raw: {n_pix} pixel bytes / {n_tab} table entries do not fit the int32 records")
    pixels = np.zeros(n_pix, dtype=np.uint8)
    for r, a in zip(records, arrays):
        pixels[r[0]:r[0] + a.size] = a.reshape(-1)
    return {"pixels": torch.from_numpy(pixels), "images": torch.from_numpy(records), "tables": torch.from_numpy(np.concatenate(tables)),
            "lut": norm_table(), "Hm": int(records[:, 3].max()), "Wm": int(records[:, 4].max()), "max_taps": max_taps, "max_rows": max_rows,
            "device_resampled": B - n_host}


def collate_raw(samples):
    """`collate` for raw=True samples: the same dict with `raw` (pack_raw) in the place of `image` and `mask`; Prefetcher puts those two
    back with one cdetr_image_prep launch, equal to `collate`'s bit for bit."""
    return {"raw": pack_raw(samples), **_stage2_fields(samples)}


def collate_stage1_raw(samples):
    """`collate_stage1` for raw=True samples (see collate_raw)."""
    _check_stage1_counts(samples)
    return {"raw": pack_raw(samples), **_stage1_fields(samples)}


class Prefetcher:
    """Iterates a DataLoader of collated batches one step ahead: the next batch is copied host -> device through pinned
    memory on a side stream while the current step computes; `next()` hands over device tensors after an event wait.
    A batch that holds `raw` (collate_raw / collate_stage1_raw) gets its `image` and `mask` from ops.image_prep, launched on the same
    side stream right after the copies; `images` / `device_resampled` count what has gone through it."""

    def __init__(self, loader, device, host_keys=()):
        self.loader, self.device, self.host_keys = loader, torch.device(device), tuple(host_keys)      # host_keys: also kept as `<key>_host`
        self.stream = torch.cuda.Stream(device=self.device) if self.device.type == "cuda" else None
        self.images = self.device_resampled = 0

    def _to_device(self, batch):
        def mv(t):
            if not torch.is_tensor(t):
                return t
            if self.stream is not None:
                t = t.pin_memory() if not t.is_pinned() else t
            return t.to(self.device, non_blocking=True)
        out = {k: mv(v) for k, v in batch.items() if k not in ("targets", "raw")}
        out.update({k + "_host": batch[k] for k in self.host_keys if k in batch})
        if "targets" in batch:
            out["targets"] = [{k: mv(v) for k, v in t.items()} for t in batch["targets"]]
        if "raw" in batch:                      # the un-resized pixels went across: resize + normalise + pad there, in this stream
            from . import ops
            out["image"], out["mask"] = ops.image_prep({k: mv(v) for k, v in batch["raw"].items()})
            self.images += out["image"].shape[0]
            self.device_resampled += batch["raw"]["device_resampled"]
        return out

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        it = iter(self.loader)

        def stage():
            try:
                b = next(it)
            except StopIteration:
                return None
            if self.stream is None:
                return self._to_device(b)
            with torch.cuda.stream(self.stream):
                return self._to_device(b)

        nxt = stage()
        while nxt is not None:
            if self.stream is not None:
                torch.cuda.current_stream(self.device).wait_stream(self.stream)
                for v in list(nxt.values()) + [x for t in nxt.get("targets", ()) for x in t.values()]:
                    if torch.is_tensor(v) and v.is_cuda:
                        v.record_stream(torch.cuda.current_stream(self.device))
            cur, nxt = nxt, stage()
            yield cur
