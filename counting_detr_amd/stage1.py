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
def write_pseudo_labels(model, loader, split, output_dir, device="cuda"):
    """The 1st-stage -> 2nd-stage hand-off file (A1/engine.py:124-187): for every image, one pseudo box per annotated dot,
    written as the COCO-style `pseudo_bbox_<split>.json` that the 2nd-stage training reader opens
    (A2/data/fsc147.py:18-19; counting_detr_amd.data.FSC147Dataset): bbox = [cx, cy, w, h] in original pixels (ints),
    file_name = "<im_id>.jpg", ids counted from 1.  `loader` yields dicts with image [1,3,H,W], points [1,P,2] (normalised),
    orig_size [1,2] = (width, height), im_id.  A batch that carries `counts` [B] (data.collate_stage1_ragged) may hold several
    images -- image [B,3,H,W], points [B,N,2] padded, orig_size [B,2], im_id a sequence: one forward per batch, image b contributes
    its first counts[b] rows, images and annotations in loader order.  Returns the annotation dict."""
    import json
    import os
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
    return ann
