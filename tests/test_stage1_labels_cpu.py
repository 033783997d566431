"""Host side of the stage-1 device labels path (main_stage1.py --device_labels / --score_labels / --test; cdetr_emit_pseudo_labels,
ops.PseudoLabelStore, stage1.score_pseudo_labels / score_box_pairs, data.FSC147BoxPointsDataset):
  (a) the numpy restatement the GPU tests compare the kernel with (tests/stage1_labels_ref.py) equals stage1.write_pseudo_labels' host loop
      and the evaluator rule of stage1.evaluator_boxes, on rows where one fp32 rounding decides an integer;
  (b) the reader on the tiny fixture against FSC147EvalDataset and the json;
  (c) the scoring functions on hand-made json;
  (d) the CLI flags, the ABI plumbing and the argument checks that happen before any launch.
No GPU needed."""
import argparse
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import abi_header
import stage1_labels_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
TINY = os.path.join(HERE, "golden", "fsc147_tiny")
F32 = np.float32


def host_loop(pts, whs, size):
    """stage1.write_pseudo_labels' per-image arithmetic, statement for statement (counting_detr_amd/stage1.py, `for size, pts, whs, im_id`)."""
    pts, whs = np.array(pts, dtype=F32), np.array(whs, dtype=F32)
    whs[:, 0] *= size[0]; whs[:, 1] *= size[1]
    pts[:, 0] *= size[0]; pts[:, 1] *= size[1]
    out = []
    for (x_cen, y_cen), (w, h) in zip(pts, whs):
        out.append([int(x_cen), int(y_cen), int(w), int(h), int(w * h)])
    return out


class FixedModel(torch.nn.Module):
    """Stands in for the stage-1 model on the host: pred_wh is handed in, whatever the image."""

    def __init__(self, wh_by_call):
        super().__init__()
        self.wh, self.calls = wh_by_call, 0

    def forward(self, image, points, counts=None):
        self.calls += 1
        return {"pred_wh": self.wh[self.calls - 1]}


def test_restatement_equals_the_host_loop_on_truncation_rows():
    pts, whs, size = ref.truncation_rows()
    want = host_loop(pts, whs, size)
    got = ref.emit_image(pts, whs, size[0], size[1], max_det=1100)
    assert got["wire"].tolist() == want
    # the hand-made rows do what they were made for
    assert want[0][:4] == [192, 500, 192, 500]                                      # 0.5 x 384 lands exactly on 192
    assert want[1][:4] == [191, 499, 191, 499]                                      # one fp32 step below: truncated to the integer below
    areas = [r[4] for r in want[4:]]
    exact = [int((1000.0 + k * 0.0625) * (1000.0 - k * 0.0625)) for k in range(8)]
    fp32 = [int(F32(F32(pts_w) * F32(384)) * F32(F32(pts_h) * F32(1000))) for pts_w, pts_h in whs[4:]]
    assert areas == fp32
    assert any(w[2] * w[3] != w[4] for w in want[4:]), "int(w) * int(h) must differ from int(fp32(wf * hf)) somewhere"
    assert len(set(areas)) > 1 and all(abs(a - e) <= 1 for a, e in zip(areas, exact))


def test_restatement_equals_the_host_loop_on_random_rows():
    rng = np.random.default_rng(5)
    for size in ((384, 576), (3000, 2000), (101, 70)):
        pts, whs = rng.uniform(0, 1, (300, 2)).astype(F32), rng.uniform(0.004, 0.6, (300, 2)).astype(F32)
        assert ref.emit_image(pts, whs, size[0], size[1], 1100)["wire"].tolist() == host_loop(pts, whs, size)


def test_restatement_evaluation_records_equal_the_evaluator_rule():
    """eval_boxes / eval_area / pair_iou of the restatement == stage1.evaluator_boxes on the json ints and coco_ap.box_iou_xywh's diagonal."""
    from counting_detr_amd import coco_ap, stage1
    rng = np.random.default_rng(6)
    points, pred_wh, orig_wh, gt = ref.make_batch(rng, 1, 40, [(384, 576)])
    got = ref.emit_image(points[0], pred_wh[0], orig_wh[0][0], orig_wh[0][1], max_det=25, gt_xywh=gt[0])
    ann = {"annotations": [{"image_id": 1, "bbox": r[:4], "area": r[4]} for r in got["wire"].tolist()]}
    dts = stage1.evaluator_boxes(ann)[1]
    assert all(isinstance(v, int) for d in ann["annotations"] for v in d["bbox"])
    assert np.array_equal(np.array([d["bbox"] for d in dts[:25]], dtype=np.float64), got["eval_boxes"])
    assert np.array_equal(np.array([d["area"] for d in dts[:25]]), got["eval_area"]) and len(got["eval_score"]) == 25
    assert any(d["bbox"][0] != int(d["bbox"][0]) for d in dts), "an odd width must leave a half-pixel corner (not truncated again)"
    diag = np.diagonal(coco_ap.box_iou_xywh([d["bbox"] for d in dts], gt[0]))
    assert np.array_equal(diag, got["pair_iou"]) and diag.max() > 0.5 and diag.min() == 0.0


def test_write_pseudo_labels_host_loop_matches_the_restatement(tmp_path):
    """The default path of stage1.write_pseudo_labels (a dense and a ragged batch) writes what the restatement's wire rows say."""
    from counting_detr_amd import stage1
    rng = np.random.default_rng(7)
    p0, w0, o0, _ = ref.make_batch(rng, 1, 21, [(384, 1000)], gt=False)
    p1, w1, o1, _ = ref.make_batch(rng, 2, 9, [(640, 480), (3000, 2000)], gt=False, hand=False)
    counts = np.array([9, 4], dtype=np.int32)
    loader = [{"image": torch.zeros(1, 3, 8, 8), "points": torch.from_numpy(p0), "orig_size": torch.from_numpy(o0).long(), "im_id": torch.tensor([7])},
              {"image": torch.zeros(2, 3, 8, 8), "points": torch.from_numpy(p1), "orig_size": torch.from_numpy(o1).long(),
               "im_id": torch.tensor([12, 3]), "counts": torch.from_numpy(counts)}]
    model = FixedModel([torch.from_numpy(w0), torch.from_numpy(w1)])
    ann = stage1.write_pseudo_labels(model, loader, "val", str(tmp_path), device="cpu")
    want = ref.emit_store([(p0, w0, None, o0, None), (p1, w1, counts, o1, None)], 1100)
    assert [[a["image_id"] - 1] + a["bbox"] + [a["area"]] for a in ann["annotations"]] == want["wire"].tolist()
    assert [a["id"] for a in ann["annotations"]] == list(range(1, 21 + 9 + 4 + 1))
    assert [im["file_name"] for im in ann["images"]] == ["7.jpg", "12.jpg", "3.jpg"]
    assert json.load(open(tmp_path / "pseudo_bbox_val.json")) == ann


def _args(**kw):
    a = argparse.Namespace(data_path=TINY, scale_factor=32)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("split,names,counts", [("val", ["3.png", "1.png"], [8, 6]), ("test", ["4.png"], [9])])
def test_box_points_reader_on_the_tiny_fixture(split, names, counts):
    from PIL import Image
    from counting_detr_amd import data
    ds, ev = data.FSC147BoxPointsDataset(_args(), split), data.FSC147EvalDataset(_args(), split)
    gt = json.load(open(os.path.join(TINY, f"instances_{split}.json")))
    ids = {im["file_name"]: im["id"] for im in gt["images"]}
    assert len(ds) == len(names) and ds.point_counts() == counts
    for k, name in enumerate(names):
        s, e = ds[k], ev[k]
        assert torch.equal(s["image"], e["image"])
        assert s["points"].dtype == np.float32 and torch.equal(torch.from_numpy(s["points"]), torch.from_numpy(e["points"]))
        rows = [a["bbox"] for a in gt["annotations"] if a["image_id"] == ids[name]]
        assert s["gt_xywh"].dtype == np.float64 and s["gt_xywh"].tolist() == rows and len(rows) == counts[k]
        assert tuple(s["orig_size"]) == Image.open(os.path.join(TINY, "images_384_VarV2", name)).size         # (w, h)
        assert s["im_id"] == int(name[:-4]) and s["image_id"] == ids[name] and s["labels"].shape == (counts[k],)
        assert set(data.FSC147PointsDataset(_args(), split)[k]) <= set(s)
    raw = data.FSC147BoxPointsDataset(_args(), split, raw=True)[0]
    assert "image_raw" in raw and "image" not in raw and raw["gt_xywh"].tolist() == ds[0]["gt_xywh"].tolist()


def test_collates_carry_gt_xywh_only_when_the_samples_do():
    from counting_detr_amd import data
    ds = data.FSC147BoxPointsDataset(_args(), "val")
    b = data.collate_stage1_ragged([ds[0], ds[1]])
    assert b["counts"].tolist() == [8, 6] and b["gt_xywh"].dtype == torch.float64 and tuple(b["gt_xywh"].shape) == (2, 8, 4)
    assert b["gt_xywh"][0].tolist() == ds[0]["gt_xywh"].tolist() and b["gt_xywh"][1, :6].tolist() == ds[1]["gt_xywh"].tolist()
    assert float(b["gt_xywh"][1, 6:].abs().sum()) == 0.0 and b["image_id"].tolist() == [3, 1] and b["im_id"].tolist() == [3, 1]
    d = data.collate_stage1([ds[1]])
    assert tuple(d["gt_xywh"].shape) == (1, 6, 4) and d["gt_xywh"][0].tolist() == ds[1]["gt_xywh"].tolist()
    pts = data.FSC147PointsDataset(_args(), "val")
    assert "gt_xywh" not in data.collate_stage1_ragged([pts[0], pts[1]]) and "gt_xywh" not in data.collate_stage1([pts[0]])
    assert pts.point_counts() == [8, 6]


# ---- scoring on hand-made json ---------------------------------------------------------------------------------------------------------
GT_BOXES = {3: [[10, 20, 30, 30], [100, 50, 20, 10], [200, 200, 100, 120]], 1: [[5, 5, 10, 10]]}   # integer [x1, y1, w, h], even sizes; none medium


def _gt_json(path, boxes=GT_BOXES, ext=".png"):
    gt = {"images": [{"id": i, "file_name": f"{i}{ext}", "width": 640, "height": 480} for i in boxes], "categories": [{"id": 1, "name": "fg"}],
          "annotations": []}
    for i, rows in boxes.items():
        for b in rows:
            gt["annotations"].append({"id": len(gt["annotations"]) + 1, "image_id": i, "bbox": b, "area": b[2] * b[3], "category_id": 1, "iscrowd": 0})
    with open(path, "w") as f:
        json.dump(gt, f)
    return str(path)


def _pseudo(boxes_by_stem):
    """A pseudo annotation dict as write_pseudo_labels builds it: ids from 1 in order, file_name "<stem>.jpg", bbox = [cx, cy, w, h] ints."""
    ann = {"categories": [{"name": "fg", "id": 1}], "images": [], "annotations": []}
    for k, (stem, rows) in enumerate(boxes_by_stem.items()):
        ann["images"].append({"id": k + 1, "file_name": f"{stem}.jpg", "height": 480, "width": 640})
        for b in rows:
            ann["annotations"].append({"id": len(ann["annotations"]) + 1, "image_id": k + 1, "area": b[2] * b[3], "bbox": list(b), "category_id": 1,
                                       "iscrowd": 0})
    return ann


def _centre_form(b):
    """[x1, y1, w, h] -> the [cx, cy, w, h] whose evaluator box is b again (integers for even sizes)."""
    return [b[0] + b[2] / 2, b[1] + b[3] / 2, b[2], b[3]]


same = ref.same


def test_exact_boxes_score_100_and_iou_1(tmp_path):
    """Integer ground-truth boxes reproduced exactly: AP 100, every paired IoU 1.0; the stem mapping joins "3.jpg" with "3.png"."""
    from counting_detr_amd import stage1
    boxes = GT_BOXES
    gt_json = _gt_json(tmp_path / "instances_val.json", boxes)
    ann = _pseudo({1: [[int(v) for v in _centre_form(b)] for b in boxes[1]], 3: [[int(v) for v in _centre_form(b)] for b in boxes[3]]})
    s = stage1.score_pseudo_labels(ann, gt_json)
    assert s["AP"] == pytest.approx(100.0, abs=1e-9) and s["AP50"] == pytest.approx(100.0, abs=1e-9) and s["AP75"] == pytest.approx(100.0, abs=1e-9)
    assert s["images"] == 2 and s["boxes"] == 4
    assert s["APs"] == pytest.approx(100.0, abs=1e-9) and s["APl"] == pytest.approx(100.0, abs=1e-9) and math.isnan(s["APm"])   # no medium ground truth
    assert same(s, stage1.score_pseudo_labels(ann, gt_json)) and not same(s, {**s, "APm": 0.0})
    iou, off = stage1.host_pair_iou(ann, [boxes[1], boxes[3]])
    assert off.tolist() == [0, 1, 4] and iou.tolist() == [1.0] * 4
    p = stage1.score_box_pairs(iou, off)
    assert p == {"pairs": 4, "mean_iou": 1.0, "iou50": 1.0, "iou75": 1.0, "per_image_mean_iou": [1.0, 1.0]}


def test_a_shifted_box_gives_its_hand_computed_iou(tmp_path):
    """One 20 x 10 box moved 4 px to the right: intersection 16 x 10 = 160, union 200 + 200 - 160 = 240, IoU 2/3 -- matched at the
    thresholds 0.50 .. 0.65 only."""
    from counting_detr_amd import coco_ap, stage1
    gt_json = _gt_json(tmp_path / "instances_val.json", {7: [[100, 50, 20, 10]], 8: [[10, 10, 40, 40]]})
    ann = _pseudo({7: [[114, 55, 20, 10]], 8: [[30, 30, 40, 40]]})
    iou, off = stage1.host_pair_iou(ann, [[[100, 50, 20, 10]], [[10, 10, 40, 40]]])
    assert iou.tolist() == [160.0 / 240.0, 1.0]
    p = stage1.score_box_pairs(iou, off)
    assert p["pairs"] == 2 and p["mean_iou"] == (160.0 / 240.0 + 1.0) / 2 and p["iou50"] == 1.0 and p["iou75"] == 0.5 and p["per_image_mean_iou"] == [160.0 / 240.0, 1.0]
    s = stage1.score_pseudo_labels(ann, gt_json)
    # two detections of score 1.0 in image order; at t <= 0.65 both match (precision 1 everywhere), above only the second does: the first is a
    # false positive AHEAD of it, recall reaches 0.5 at precision 1/2 and never gets past it: 51 of the 101 recall samples hold 0.5
    hi = 51 * 0.5 / 101
    assert s["AP50"] == pytest.approx(100.0) and s["AP75"] == pytest.approx(100 * hi) and s["AP"] == pytest.approx(100 * (4 * 1.0 + 6 * hi) / 10)
    assert len(coco_ap.IOU_THRS) == 10


def test_an_image_above_max_det_keeps_its_first_rows(tmp_path):
    """More boxes than max_det: the evaluator sees the first max_det in file order (all scores tie, the sort is stable)."""
    from counting_detr_amd import stage1
    gt_json = _gt_json(tmp_path / "instances_val.json", {2: [[0, 0, 10, 10], [50, 50, 10, 10]]})
    good, bad = [5, 5, 10, 10], [300, 300, 4, 4]
    first = stage1.score_pseudo_labels(_pseudo({2: [good, [55, 55, 10, 10], bad, bad, bad]}), gt_json, max_det=2)
    last = stage1.score_pseudo_labels(_pseudo({2: [bad, bad, bad, good, [55, 55, 10, 10]]}), gt_json, max_det=2)
    assert first["AP"] == pytest.approx(100.0) and first["boxes"] == 5 and last["AP"] == 0.0
    assert stage1.score_pseudo_labels(_pseudo({2: [bad, bad, bad, good, [55, 55, 10, 10]]}), gt_json)["AP50"] > 0.0      # the default cut keeps all five


def test_an_image_missing_from_the_ground_truth_is_an_error(tmp_path):
    from counting_detr_amd import stage1
    gt_json = _gt_json(tmp_path / "instances_val.json", {2: [[0, 0, 10, 10]]})
    with pytest.raises(KeyError, match="9.jpg"):
        stage1.score_pseudo_labels(_pseudo({9: [[5, 5, 10, 10]]}), gt_json)


def test_score_box_pairs_edges():
    from counting_detr_amd import stage1
    p = stage1.score_box_pairs(np.zeros(0), [0, 0])
    assert p["pairs"] == 0 and math.isnan(p["mean_iou"]) and math.isnan(p["per_image_mean_iou"][0])
    p = stage1.score_box_pairs([0.5, 0.75, 0.7499999, 0.0], [0, 0, 3, 4])
    assert p["iou50"] == 0.75 and p["iou75"] == 0.25 and math.isnan(p["per_image_mean_iou"][0]) and p["per_image_mean_iou"][2] == 0.0
    with pytest.raises(ValueError):
        stage1.score_box_pairs([0.5], [0, 2])


# ---- CLI and plumbing ---------------------------------------------------------------------------------------------------------------
def test_parser_flags_and_defaults():
    import inspect
    from counting_detr_amd import stage1
    from counting_detr_amd.args import get_args_parser_stage1
    p = get_args_parser_stage1()
    a = p.parse_args([])
    assert (a.device_labels, a.score_labels, a.test) == (False, False, False)
    a = p.parse_args(["--generate_pseudo_label", "--score_labels", "--device_labels"])
    assert a.device_labels and a.score_labels and a.generate_pseudo_label and not a.test
    assert p.parse_args(["--test", "--device_labels"]).test
    sig = inspect.signature(stage1.write_pseudo_labels)
    assert sig.parameters["device_labels"].default is False and sig.parameters["return_store"].default is False


def test_default_write_pseudo_labels_never_touches_the_device_path(tmp_path, monkeypatch):
    from counting_detr_amd import ops, stage1

    def refuse(*a, **k):
        raise AssertionError("the default label path must stay on the host loop")
    monkeypatch.setattr(ops, "PseudoLabelStore", refuse)
    monkeypatch.setattr(ops, "emit_pseudo_labels", refuse)
    loader = [{"image": torch.zeros(1, 3, 8, 8), "points": torch.full((1, 2, 2), 0.5), "orig_size": torch.tensor([[64, 32]]), "im_id": torch.tensor([4])}]
    ann, store = stage1.write_pseudo_labels(FixedModel([torch.full((1, 2, 2), 0.25)]), loader, "test", str(tmp_path), device="cpu", return_store=True)
    assert store is None and [a["bbox"] for a in ann["annotations"]] == [[32, 16, 16, 8]] * 2
    with pytest.raises(AssertionError, match="host loop"):
        stage1.write_pseudo_labels(FixedModel([torch.full((1, 2, 2), 0.25)]), loader, "test", str(tmp_path), device="cpu", device_labels=True)


def test_abi_header_struct_and_argument_checks():
    """The descriptor mirrors the header field by field; bad descriptors are refused before any launch (no GPU is touched)."""
    from counting_detr_amd import _ffi
    L = _ffi.lib()
    src = abi_header.source()
    assert "cdetr_emit_pseudo_labels" in _ffi.EXPORTS and hasattr(L, "cdetr_emit_pseudo_labels")
    assert re.search(r"^int cdetr_emit_pseudo_labels\(const cdetr_emit_pseudo_labels_desc\* d, void\* stream\);", src, flags=re.M)
    assert abi_header.field_names("cdetr_emit_pseudo_labels_desc") == [f[0] for f in _ffi.EmitPseudoLabelsDesc._fields_]
    assert ctypes.sizeof(_ffi.EmitPseudoLabelsDesc) == 8 * 4 + 14 * 8
    assert "stage1_labels.hip" in __import__("counting_detr_amd.build", fromlist=["SOURCES"]).SOURCES

    buf = (ctypes.c_double * 64)()
    addr = (ctypes.addressof(buf) + 15) & ~15

    def desc(**kw):
        d = _ffi.EmitPseudoLabelsDesc()
        d.B, d.R, d.N, d.first, d.max_det, d.row_cap, d.eval_cap = 2, 8, 4, 0, 1100, 16, 16
        for f in ("points", "pred_wh", "orig_wh", "img_counts", "row_off", "eval_off", "wire", "pair_iou", "eval_boxes", "eval_area", "eval_score", "status"):
            setattr(d, f, addr)
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    assert L.cdetr_emit_pseudo_labels(None, None) < 0 and b"cdetr_emit_pseudo_labels" in L.cdetr_last_error()
    for bad in (dict(B=0), dict(R=0), dict(N=0), dict(first=-1), dict(first=3), dict(max_det=-1), dict(row_cap=-1), dict(row_cap=(1 << 30) + 1),
                dict(points=None), dict(pred_wh=None), dict(orig_wh=None), dict(row_off=None), dict(status=None), dict(wire=None), dict(pair_iou=None),
                dict(eval_boxes=None), dict(wire=addr + 8), dict(points=addr + 4)):
        rc = L.cdetr_emit_pseudo_labels(ctypes.byref(desc(**bad)), None)
        assert rc < 0 and b"cdetr_emit_pseudo_labels" in L.cdetr_last_error(), bad
    assert L.cdetr_emit_pseudo_labels(ctypes.byref(desc(R=(1 << 20) + 1)), None) == -3                         # CDETR_ERR_UNSUPPORTED


def test_ops_emit_pseudo_labels_checks_its_tensors():
    from types import SimpleNamespace
    from counting_detr_amd import ops
    store = SimpleNamespace(buf=torch.zeros(1), N=2, max_det=1100, row_cap=16, eval_cap=16)
    p, w, c, o, g = torch.zeros(2, 4, 2), torch.zeros(2, 4, 2), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, 4, 4).double()
    with pytest.raises(RuntimeError, match="float32.*points"):
        ops.emit_pseudo_labels(p.double(), w, c, o, store, 0)
    with pytest.raises(RuntimeError, match="contiguous.*pred_wh"):
        ops.emit_pseudo_labels(p, torch.zeros(2, 4, 4)[..., 2:], c, o, store, 0)
    with pytest.raises(RuntimeError, match="int32.*counts"):
        ops.emit_pseudo_labels(p, w, c.long(), o, store, 0)
    with pytest.raises(RuntimeError, match="int32.*orig_wh"):
        ops.emit_pseudo_labels(p, w, c, o.long(), store, 0)
    with pytest.raises(RuntimeError, match="float64.*gt_xywh"):
        ops.emit_pseudo_labels(p, w, c, o, store, 0, gt_xywh=g.float())
    with pytest.raises(RuntimeError, match="expected, got"):
        ops.emit_pseudo_labels(p, w[:, :3].contiguous(), c, o, store, 0)
    with pytest.raises(RuntimeError, match="expected, got"):
        ops.emit_pseudo_labels(p, w, c[:1], o, store, 0)
    with pytest.raises(RuntimeError, match="expected, got"):
        ops.emit_pseudo_labels(p, w, c, o, store, 0, gt_xywh=g[:, :3].contiguous())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.emit_pseudo_labels(p, w, c, o, SimpleNamespace(**{**vars(store), **{k: p for k in (
            "counts", "row_off", "eval_off", "status", "wire", "pair_iou", "eval_boxes", "eval_area", "eval_score")}}), 0)     # host tensors: no host implementation
