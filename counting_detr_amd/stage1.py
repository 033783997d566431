"""1st-stage Counting-DETR (point -> box pseudo-label generator) on the same MI355X kernels -- SURVEY.md row a15.

API mirror of A1/models/anchor_detr.py (A1 = src/CountDETR_147_1st_stage): `build(args) -> (model, criterion,
postprocessors)`, `model(samples, scaled_sample_points) -> {"pred_logits", "pred_wh", "pred_points"}` (:80-113),
`BoundingBoxCriterion` (:317-337: L1 on wh + mean(1 - GIoU) of boxes built from the GT points and the predicted wh; no
Hungarian matcher is involved in stage 1; `fused = True` computes it in one launch, ops.BBoxCriterionFn).  The model's output also
carries "pred_boxes" = the box head's [B,Q,4] output that "pred_points" / "pred_wh" are column views of (the fused criterion reads
the wh columns in place).  Differences to stage 2 (A1/models/transformer.py:60-214): the query embedding is
called `modify_pattern`, there is no variance head, the class bias has ONE element broadcast over 2 logits, the anchor
points are `defined` = the given points (Q = number of points), the backbone output goes through `input_proj` (no
exemplar aggregation).  State dict is key-compatible with the reference's stage-1 model.
"""
import torch
import torch.nn.functional as F
from torch import nn

from . import box_ops, ops
from .anchor_detr import PostProcess, _ProjGN
from .backbone import BackboneAgg
from .misc import NestedTensor, nested_tensor_from_tensor_list
from .transformer import Transformer


class AnchorDETRStage1(nn.Module):
    def __init__(self, backbone, transformer, num_feature_levels=1):
        super().__init__()
        assert num_feature_levels == 1
        self.transformer = transformer
        self.num_feature_levels = num_feature_levels
        self.input_proj = nn.ModuleList([_ProjGN(backbone.num_channels[0], transformer.d_model)])
        self.backbone = backbone

    def forward(self, samples, scaled_sample_points, counts=None):
        """counts (int32 device tensor [B]): a ragged batch -- scaled_sample_points [B,N,2] padded to the batch maximum N, image b's
        rows beyond counts[b] are padding (finite, don't-care outputs); rows below are what the image alone would give."""
        if not isinstance(samples, NestedTensor):
            samples = nested_tensor_from_tensor_list(samples)
        images, mask = samples.decompose()
        x = self.backbone.body.forward_nhwc(images)                          # NHWC [B,h,w,2048]
        if ops.AFTER_BACKBONE is not None:                                   # (a trainer's schedule hook, as in AnchorDETR.forward)
            ops.AFTER_BACKBONE()
        m = F.interpolate(mask[None].float(), size=x.shape[1:3]).to(torch.bool)[0]
        src = self.input_proj[0](x)
        (cls, xywh, _), _ = self.transformer(src, m, scaled_sample_points, counts)
        return {"pred_logits": cls[-1], "pred_wh": xywh[-1][..., 2:], "pred_points": xywh[-1][..., :2], "pred_boxes": xywh[-1]}


class BoundingBoxCriterion(nn.Module):
    """A1/models/anchor_detr.py:317-337.  `fused = False` (default): the reference's chain of tensor ops.  `fused = True`: one launch
    (ops.BBoxCriterionFn over outputs["pred_boxes"]) that also forms the weighted total -- what engine.Stage1Trainer uses.
    targets["counts"] (int32 [B], optional): a ragged batch; the loss is the one over the concatenation of every image's first
    counts[b] pairs (M = sum(counts)), padded rows take no part and receive no gradient."""

    def __init__(self, fused=False):
        super().__init__()
        self.weight_dict = {"loss_wh": 1, "loss_giou": 0.4}
        self.fused = bool(fused)

    def forward(self, outputs, targets):
        return self.forward_with_total(outputs, targets)[0]

    def forward_with_total(self, outputs, targets):
        """(loss dict, weighted total sum_k loss_k * weight_dict[k]) -- A1/engine.py's `losses`."""
        wd = self.weight_dict
        if self.fused:
            if "pred_boxes" not in outputs:
                raise KeyError("the fused BoundingBoxCriterion reads the box head's [B,Q,4] output: outputs['pred_boxes'] is missing")
            vec = ops.BBoxCriterionFn.apply(outputs["pred_boxes"], targets["points"], targets["whs"], wd["loss_wh"], wd["loss_giou"],
                                            targets.get("counts"))
            return {"loss_wh": vec[0], "loss_giou": vec[1]}, vec[2]
        loss_dict = self._composition(outputs, targets)
        return loss_dict, sum(loss_dict[k] * wd[k] for k in loss_dict if k in wd)

    def _composition(self, outputs, targets):
        tgt_points = targets["points"].flatten(0, 1)
        src_whs = outputs["pred_wh"].flatten(0, 1)
        tgt_whs = targets["whs"].flatten(0, 1)
        counts = targets.get("counts")
        if counts is not None:            # the valid pairs, concatenated (boolean row mask: padded values never enter a sum)
            N = targets["whs"].shape[1]
            valid = (torch.arange(N, device=counts.device)[None, :] < counts[:, None]).flatten()
            tgt_points, src_whs, tgt_whs = tgt_points[valid], src_whs[valid], tgt_whs[valid]
        src_boxes = torch.cat([tgt_points, src_whs], dim=-1)
        tgt_boxes = torch.cat([tgt_points, tgt_whs], dim=-1)
        giou = box_ops.generalized_box_iou_pairs(box_ops.box_cxcywh_to_xyxy(src_boxes), box_ops.box_cxcywh_to_xyxy(tgt_boxes))
        return {"loss_wh": F.l1_loss(src_whs, tgt_whs), "loss_giou": (1 - giou).sum() / tgt_whs.shape[0]}


def build(args):
    """A1/models/anchor_detr.py:375-409."""
    from . import _ffi
    _ffi.lib()
    if args.attention_type != "RCDA":
        raise NotImplementedError(f"stage 1 is implemented for attention_type 'RCDA' only, not {args.attention_type!r}")
    backbone = BackboneAgg(args.lr_backbone > 0, args.dilation)
    transformer = Transformer(d_model=args.hidden_dim, nhead=args.nheads, num_encoder_layers=args.enc_layers,
                              num_decoder_layers=args.dec_layers, dim_feedforward=args.dim_feedforward, dropout=args.dropout,
                              num_feature_levels=args.num_feature_levels, num_query_position=args.num_query_position,
                              num_query_pattern=args.num_query_pattern, spatial_prior=args.spatial_prior,
                              attention_type=args.attention_type, stage=1)
    transformer.all_layer_heads = False
    model = AnchorDETRStage1(backbone, transformer, args.num_feature_levels)
    criterion = BoundingBoxCriterion().to(torch.device(args.device))
    return model, criterion, {"bbox": PostProcess()}


@torch.no_grad()
def generate_pseudo_boxes(model, image, points, counts=None):
    """A1/engine.py:124-187 core: all GT dots in, one [cx, cy, w, h] pseudo box per dot out (normalised).  counts: a ragged batch
    (points [B,N,2] padded; image b's boxes are rows [:counts[b]], the rest is padding)."""
    model.eval()
    if counts is not None:
        return torch.cat([points, model(image, points, counts)["pred_wh"]], dim=-1)
    out = model(image, points)
    return torch.cat([points.reshape(1, -1, 2).expand(image.shape[0], -1, -1), out["pred_wh"]], dim=-1)


@torch.no_grad()
def write_pseudo_labels(model, loader, split, output_dir, device="cuda", device_labels=False, return_store=False):
    """The 1st-stage -> 2nd-stage hand-off file (A1/engine.py:124-187): for every image, one pseudo box per annotated dot,
    written as the COCO-style `pseudo_bbox_<split>.json` that the 2nd-stage training reader opens
    (A2/data/fsc147.py:18-19; counting_detr_amd.data.FSC147Dataset): bbox = [cx, cy, w, h] in original pixels (ints),
    file_name = "<im_id>.jpg", ids counted from 1.  `loader` yields dicts with image [1,3,H,W], points [1,P,2] (normalised),
    orig_size [1,2] = (width, height), im_id.  A batch that carries `counts` [B] (data.collate_stage1_ragged) may hold several
    images -- image [B,3,H,W], points [B,N,2] padded, orig_size [B,2], im_id a sequence: one forward per batch, image b contributes
    its first counts[b] rows, images and annotations in loader order.  Returns the annotation dict.
    device_labels=True: the loop below is replaced by one cdetr_emit_pseudo_labels call per batch into an ops.PseudoLabelStore and ONE
    copy back after the last batch (_device_label_pass); the SAME bytes are written.  return_store=True: -> (annotation dict, that store or
    None) -- the store also holds the boxes in the form coco_ap.summarize_store reads and, for batches that carry `gt_xywh`, the paired IoUs."""
    import json
    import os
    if device_labels:
        ann, store = _device_label_pass(model, loader, device)
        os.makedirs(output_dir, exist_ok=True)
        with open(os.path.join(output_dir, "pseudo_bbox_" + split + ".json"), "w") as handle:
            json.dump(ann, handle)
        return (ann, store) if return_store else ann
    model.eval()
    ann = {"categories": [{"name": "fg", "id": 1}], "images": [], "annotations": []}
    img_id = anno_id = 1
    for ret in loader:
        image, points = ret["image"].to(device), ret["points"].to(device)
        if ret.get("counts") is not None:
            counts = ret["counts"]
            wh = model(image, points, counts.to(device=device, dtype=torch.int32))["pred_wh"]
            rows = [int(c) for c in counts.tolist()]
            sizes = ret["orig_size"].reshape(len(rows), 2).tolist()
            pts_b, whs_b = points.cpu().numpy(), wh.cpu().numpy()
            per_image = [(sizes[b], pts_b[b, :rows[b]].copy(), whs_b[b, :rows[b]].copy(), ret["im_id"][b]) for b in range(len(rows))]
        else:
            wh = model(image, points)["pred_wh"]
            per_image = [(ret["orig_size"].reshape(-1).tolist(), points.reshape(-1, 2).cpu().numpy().copy(),
                          wh.reshape(-1, 2).cpu().numpy().copy(), ret["im_id"])]
        for size, pts, whs, im_id in per_image:                           # size = (width, height)
            whs[:, 0] *= size[0]; whs[:, 1] *= size[1]
            pts[:, 0] *= size[0]; pts[:, 1] *= size[1]
            for (x_cen, y_cen), (w, h) in zip(pts, whs):
                ann["annotations"].append({"id": anno_id, "image_id": img_id, "area": int(w * h),
                                           "bbox": [int(x_cen), int(y_cen), int(w), int(h)], "category_id": 1, "iscrowd": 0})
                anno_id += 1
            ann["images"].append({"id": img_id, "file_name": str(int(im_id)) + ".jpg", "height": int(size[1]), "width": int(size[0])})
            img_id += 1
    os.makedirs(output_dir, exist_ok=True)
    with open(os.path.join(output_dir, "pseudo_bbox_" + split + ".json"), "w") as handle:
        json.dump(ann, handle)
    return (ann, None) if return_store else ann


def _label_store_size(loader):
    """(images, rows) a PseudoLabelStore must hold for one pass over `loader`: from its dataset's `point_counts()` (a DataLoader, a
    data.Prefetcher around one, or anything else with `.dataset`), or from the batches themselves when `loader` is a list of them."""
    if isinstance(loader, _GtTap):
        loader = loader.loader
    ds = getattr(loader, "dataset", None) or getattr(getattr(loader, "loader", None), "dataset", None)
    if ds is not None and hasattr(ds, "point_counts"):
        counts = ds.point_counts()
        return len(counts), int(sum(counts))
    if isinstance(loader, (list, tuple)):
        n = rows = 0
        for ret in loader:
            c = ret.get("counts")
            B = 1 if c is None else int(c.numel())
            n += B
            rows += ret["points"].reshape(-1, 2).shape[0] if c is None else int(c.sum())
        return n, rows
    raise RuntimeError("write_pseudo_labels(device_labels=True): the store is sized from the loader's dataset (`point_counts()`), "
                       f"which {type(loader).__name__} does not offer")


@torch.no_grad()
def _device_label_pass(model, loader, device, max_det=None):
    """write_pseudo_labels' loop with the post-forward work on the device: per batch one forward and one `emit` (no copy back, nothing
    awaited), after the loop ONE `finish()`; the annotation dict is built from the wire array.  -> (annotation dict, store).  Image ids and
    original sizes are host values of the loader's batches; where a data.Prefetcher has already moved them to the device they are
    gathered after the loop in one more copy."""
    from . import coco_ap
    n_images, rows = _label_store_size(loader)
    store = ops.PseudoLabelStore(max(n_images, 1), rows, device, max_det=coco_ap.MAX_DETS if max_det is None else max_det)
    model.eval()
    im_ids, sizes = [], []
    for ret in loader:
        image, points = ret["image"].to(device), ret["points"].to(device)
        counts = ret.get("counts")
        if counts is not None:
            counts = counts.to(device=device, dtype=torch.int32)
            wh = model(image, points, counts)["pred_wh"]
        else:
            wh = model(image, points)["pred_wh"]
        B = wh.shape[0]
        points = points.reshape(-1, points.shape[-2], 2).expand(B, -1, -1)
        gt = ret.get("gt_xywh")
        if gt is not None:
            gt = gt.to(device=device, dtype=torch.float64).reshape(B, -1, 4).contiguous()
        store.emit(points.contiguous(), wh.contiguous(), counts, ret["orig_size"].reshape(B, 2).to(device=device, dtype=torch.int32).contiguous(), gt)
        im_ids.append(torch.as_tensor(ret["im_id"]).reshape(-1))
        sizes.append(ret["orig_size"].reshape(B, 2))
    host = store.finish()
    im_ids = torch.cat(im_ids).tolist() if im_ids else []
    sizes = torch.cat(sizes).tolist() if sizes else []
    ann = {"categories": [{"name": "fg", "id": 1}], "images": [], "annotations": []}
    ann["annotations"] = [{"id": k + 1, "image_id": r[0] + 1, "area": r[5], "bbox": [r[1], r[2], r[3], r[4]], "category_id": 1, "iscrowd": 0}
                          for k, r in enumerate(host["wire"].tolist())]
    ann["images"] = [{"id": k + 1, "file_name": str(int(im_id)) + ".jpg", "height": int(size[1]), "width": int(size[0])}
                     for k, (im_id, size) in enumerate(zip(im_ids, sizes))]
    return ann, store


def _stem(file_name):
    import os
    return int(os.path.splitext(os.path.basename(file_name))[0])


def evaluator_boxes(ann):
    """The pseudo json's annotations as the offline evaluator reads them (A1/offline_coco_evaluator.py:134-143 + COCO loadRes): bbox
    [cx, cy, w, h] -> a detection [cx - w/2, cy - h/2, w, h] of score 1.0, area w * h, formed from the ints of the file and not truncated
    again.  -> {pseudo image id: [detection dicts]} in file order."""
    out = {}
    for a in ann["annotations"]:
        cx, cy, w, h = a["bbox"]
        out.setdefault(a["image_id"], []).append({"bbox": [cx - w / 2, cy - h / 2, w, h], "score": 1.0, "area": float(w * h)})
    return out


def _gt_image_ids(ann, gt_json):
    """Pseudo image id -> the ground-truth image id whose file_name has the same integer stem (the pseudo file writes "<im_id>.jpg" whatever
    the real extension)."""
    import json
    with open(gt_json) as f:
        by_stem = {_stem(im["file_name"]): im["id"] for im in json.load(f).get("images", [])}
    missing = [im["file_name"] for im in ann["images"] if _stem(im["file_name"]) not in by_stem]
    if missing:
        raise KeyError(f"score_pseudo_labels: {gt_json} has no image for {missing[:5]}{' ...' if len(missing) > 5 else ''}")
    return {im["id"]: by_stem[_stem(im["file_name"])] for im in ann["images"]}


def score_pseudo_labels(ann, gt_json, device=None, store=None, max_det=None):
    """Box AP of a pseudo-label annotation dict (write_pseudo_labels' return value / the loaded pseudo_bbox_<split>.json) against
    `instances_<split>.json`, by the offline evaluator's conventions (evaluator_boxes; A1/offline_coco_evaluator.py needs detectron2).
    -> coco_ap.summarize's six numbers (AP, AP50, AP75, APs, APm, APl; x 100, NaN when undefined) + `images` and `boxes`.
    device=None: the host code of coco_ap, the checker; a CUDA device: the matching in one launch (coco_ap.summarize(device=)), EQUAL numbers;
    store= the ops.PseudoLabelStore the labels were emitted into: the same numbers through coco_ap.summarize_store, the detections read
    straight from device memory (the dict only names the images)."""
    from . import coco_ap
    max_det = coco_ap.MAX_DETS if max_det is None else int(max_det)
    to_gt = _gt_image_ids(ann, gt_json)
    gt_by = coco_ap.gt_from_json(gt_json, set(to_gt.values()))
    if store is not None:
        if store.first != len(ann["images"]):
            raise RuntimeError(f"score_pseudo_labels: a store of {store.first} images for {len(ann['images'])} pseudo images")
        six = coco_ap.summarize_store(gt_by, store, [to_gt[im["id"]] for im in ann["images"]], max_det=max_det)   # image k of the store = id k + 1
    else:
        dt_by = {to_gt[i]: d for i, d in evaluator_boxes(ann).items()}
        six = coco_ap.summarize(gt_by, dt_by, max_det=max_det, device=device)
    return {**six, "images": len(ann["images"]), "boxes": len(ann["annotations"])}


def score_box_pairs(pair_iou, row_off):
    """Pairwise quality of boxes predicted AT the ground-truth centres: pair_iou float64 [rows] = IoU of row r's box with its own ground-truth
    box, row_off [images + 1] = each image's rows.  -> {"pairs", "mean_iou", "iou50", "iou75" (share of pairs with IoU >= 0.5 / 0.75),
    "per_image_mean_iou"} in numpy float64; NaN where there is no pair.  The same code summarises the host IoUs (host_pair_iou) and the
    store's `pair_iou`: equal bits in, equal numbers out."""
    import numpy as np
    iou = np.ascontiguousarray(pair_iou, dtype=np.float64).reshape(-1)
    off = np.asarray(row_off, dtype=np.int64).reshape(-1)
    if off[-1] != iou.size:
        raise ValueError(f"score_box_pairs: {iou.size} pairs, offsets end at {int(off[-1])}")
    mean = lambda v: float(np.mean(v)) if v.size else float("nan")                                           # noqa: E731
    return {"pairs": int(iou.size), "mean_iou": mean(iou), "iou50": mean(iou >= 0.5), "iou75": mean(iou >= 0.75),
            "per_image_mean_iou": [mean(iou[a:b]) for a, b in zip(off[:-1], off[1:])]}


def host_pair_iou(ann, gt_rows):
    """The host checker of the store's `pair_iou`: per image (in file order) the diagonal of coco_ap.box_iou_xywh between its evaluator boxes
    and gt_rows[k] (float64 [P, 4], the row-aligned ground truth).  -> (pair_iou float64 [rows], row_off int64 [images + 1])."""
    import numpy as np
    from . import coco_ap
    dt_by = evaluator_boxes(ann)
    ious, off = [], [0]
    for im, gt in zip(ann["images"], gt_rows):
        dt = dt_by.get(im["id"], [])
        gt = np.asarray(gt, dtype=np.float64).reshape(-1, 4)
        if len(dt) != len(gt):
            raise ValueError(f"host_pair_iou: image {im['file_name']} has {len(dt)} boxes and {len(gt)} ground-truth rows")
        ious.append(np.diagonal(coco_ap.box_iou_xywh([d["bbox"] for d in dt], gt)).astype(np.float64))
        off.append(off[-1] + len(dt))
    return (np.concatenate(ious) if ious else np.zeros(0)), np.asarray(off, dtype=np.int64)


class _GtTap:
    """Iterates `loader` unchanged while keeping every batch's row-aligned ground truth (gt_xywh, counts) for host_pair_iou."""

    def __init__(self, loader):
        self.loader, self.rows = loader, []

    def __iter__(self):
        for ret in self.loader:
            self.rows.append((ret["gt_xywh"], ret.get("counts")))
            yield ret

    def per_image(self):
        out = []
        for gt, counts in self.rows:
            gt = gt.cpu().numpy().reshape(-1, gt.shape[-2], 4)
            n = [gt.shape[1]] * gt.shape[0] if counts is None else [int(c) for c in counts.tolist()]
            out += [gt[b, :n[b]] for b in range(gt.shape[0])]
        return out


def score_boxes_at_gt(model, loader, split, gt_json, output_dir, device="cuda", device_labels=False):
    """main_stage1.py --test for one split: the forward at the ground-truth box centres (`loader` over data.FSC147BoxPointsDataset), the boxes
    written as `pseudo_bbox_gtpoints_<split>.json` by write_pseudo_labels, and -> score_box_pairs of every box with its own ground truth +
    the six AP numbers of score_pseudo_labels.  device_labels=False: the host loop, host_pair_iou and coco_ap's host code;
    True: the store's pair_iou and coco_ap.summarize_store -- EQUAL numbers."""
    tap = _GtTap(loader)
    ann, store = write_pseudo_labels(model, tap, "gtpoints_" + split, output_dir, device=device, device_labels=device_labels, return_store=True)
    if store is not None:
        host = store.finish()
        pairs = score_box_pairs(host["pair_iou"], host["row_off"])
    else:
        pairs = score_box_pairs(*host_pair_iou(ann, tap.per_image()))
    six = score_pseudo_labels(ann, gt_json, store=store)
    return {**pairs, **{k: six[k] for k in ("AP", "AP50", "AP75", "APs", "APm", "APl")}}
