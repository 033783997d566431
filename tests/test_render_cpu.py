"""counting_detr_amd/render.py without a GPU: the drawing rule against hand-written pixels and against the painter of tests/render_ref.py, the
choice of images, the command line, the C boundary of cdetr_render_boxes, and the host route of infer.py --render_worst end to end.  Every
comparison of pixels is == on uint8 arrays."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import abi_header
import eval_split as es
import render_ref as rr
from counting_detr_amd import coco_ap as ca
from counting_detr_amd import render


def same_images(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.uint8 and g.shape == w.shape, (k, g.dtype, g.shape, w.shape)
        bad = int((g != w).any(axis=2).sum())
        print(f"canvas {k} {w.shape}: {bad} pixels differ")
        assert bad == 0, k


# ----------------------------------------------------------------------------------------------------------------- 1. hand-written pixels
@pytest.mark.parametrize("case", rr.HAND_CASES, ids=[c[0] for c in rr.HAND_CASES])
def test_hand_written_pixels(case):
    canvases, pack, matched, ignored, sel, dt_cnt, exs, style, dot = rr.hand_inputs(case)
    want = [rr.hand_expected(case[-1])]
    before = canvases[0].copy()
    same_images(render.render_images(canvases, pack, matched, ignored, sel, dt_cnt=dt_cnt, exemplars=exs, style=style, dot=dot), want)
    same_images(rr.paint_pack(canvases, pack, matched, ignored, sel, dt_cnt=dt_cnt, exemplars=exs, style=style, dot=dot), want)
    assert np.array_equal(canvases[0], before)                                  # the canvas itself is not written


def test_default_style_is_the_stated_one():
    assert render.DEFAULT_STYLE.dtype == np.uint8 and render.DEFAULT_STYLE.tolist() == rr.STYLE and render.DEFAULT_DOT == 1
    assert render.CLASSES == ("tp", "fp", "ignored", "gt", "exemplar")


# ------------------------------------------------------------------------------------------------------------- 2. seeded sets, both formulations
@pytest.mark.parametrize("seed", range(8))
def test_host_implementation_equals_the_painter_on_seeded_sets(seed):
    rng = np.random.default_rng(500 + seed)
    sizes = [(int(rng.integers(1, 60)), int(rng.integers(1, 90))), (int(rng.integers(20, 70)), int(rng.integers(5, 40))), (33, 47)]
    canvases, pack, matched, ignored, exs = rr.random_set(rng, sizes, 300)
    sel = [int(s) for s in rng.permutation(3)] if seed % 2 else [0, 1, 2]
    canvases, exs = [canvases[s] for s in sel], [exs[s] for s in sel]
    dt_cnt = None if seed % 3 == 0 else [int(c) for c in rng.integers(0, 120, 3)]
    style = rr.STYLE if seed < 4 else [[0, 255, 0, 2], [255, 0, 0, 3], [128, 128, 128, 1], [0, 0, 255, 2], [255, 255, 0, 5]]
    dot = [1, 0, -1, 2][seed % 4]
    got = render.render_images(canvases, pack, matched, ignored, sel, dt_cnt=dt_cnt, exemplars=exs, style=style, dot=dot)
    want = rr.paint_pack(canvases, pack, matched, ignored, sel, dt_cnt=dt_cnt, exemplars=exs, style=style, dot=dot)
    same_images(got, want)
    drawn = sum(int((w != c).any(axis=2).sum()) for w, c in zip(want, canvases))
    print("primitives", len(pack["dt_boxes"]), len(pack["gt_boxes"]), sum(len(e) for e in exs), "pixels drawn", drawn)
    assert len(pack["dt_boxes"]) + len(pack["gt_boxes"]) + sum(len(e) for e in exs) == 0 or drawn > 0


def test_bad_inputs_are_refused():
    c, pack = [rr.hand_canvas()], rr.make_pack([([], [])])
    none = np.zeros(0, dtype=bool)
    with pytest.raises(ValueError, match="sel"):
        render.render_images(c, pack, none, none, [1])
    with pytest.raises(ValueError, match="sel"):
        render.render_images(c, pack, none, none, [-1])
    with pytest.raises(ValueError, match="canvas"):
        render.render_images([np.zeros((0, 4, 3), np.uint8)], pack, none, none, [0])
    with pytest.raises(ValueError, match="dt_cnt"):
        render.render_images(c, pack, none, none, [0], dt_cnt=[1, 2])
    with pytest.raises(ValueError, match="dt_boxes"):
        render.render_images(c, {k: v for k, v in pack.items() if k != "dt_boxes"}, none, none, [0])


# ------------------------------------------------------------------------------------------------------------------------------ 3. select
def _row(i, ap, diff):
    return {"image_id": i, "count_gt": 10, "count_pred": 10 - diff, "diff": diff, "AP": ap}


def _report(rows):
    by_ap = sorted(rows, key=lambda r: (r["AP"] != r["AP"], 0.0 if r["AP"] != r["AP"] else r["AP"], r["image_id"]))
    return {"rows": rows, "order_by_ap": [r["image_id"] for r in by_ap], "order_by_diff": [r["image_id"] for r in sorted(rows, key=lambda r: -r["diff"])]}


def test_select():
    nan = float("nan")
    # run order 7, 3, 9, 4, 8: AP ties between 3 and 9 (by id), NaN last; |diff| ties between 3 (-5) and 4 (+5): the order run decides
    rep = _report([_row(7, 50.0, 1), _row(3, 20.0, -5), _row(9, 20.0, 0), _row(4, nan, 5), _row(8, 10.0, -40)])
    assert rep["order_by_ap"] == [8, 3, 9, 7, 4]
    assert render.select(rep, 0) == []
    assert render.select(rep, 1) == [{"image_id": 8, "reasons": ["ap", "diff"]}]
    assert render.select(rep, 2) == [{"image_id": 8, "reasons": ["ap", "diff"]}, {"image_id": 3, "reasons": ["ap", "diff"]}]
    assert render.select(rep, 3) == [{"image_id": 8, "reasons": ["ap", "diff"]}, {"image_id": 3, "reasons": ["ap", "diff"]},
                                     {"image_id": 9, "reasons": ["ap"]}, {"image_id": 4, "reasons": ["diff"]}]
    full = render.select(rep, 50, ids=(4, 4))                                   # k larger than the split; NaN AP last among the `ap` picks
    assert [p["image_id"] for p in full] == [8, 3, 9, 7, 4] and all(p["reasons"][:2] == ["ap", "diff"] for p in full)
    assert full[-1]["reasons"] == ["ap", "diff", "id"] and full[0]["reasons"] == ["ap", "diff"]
    assert render.select(rep, 0, ids=(9, 7, 9)) == [{"image_id": 9, "reasons": ["id"]}, {"image_id": 7, "reasons": ["id"]}]
    assert render.select(rep, 1, ids=(8, 7)) == [{"image_id": 8, "reasons": ["ap", "diff", "id"]}, {"image_id": 7, "reasons": ["id"]}]
    with pytest.raises(ValueError, match="12"):
        render.select(rep, 1, ids=(12,))


# ------------------------------------------------------------------------------------------------------------------------------ 4. the parser
def test_parser():
    from counting_detr_amd.args import default_args, get_args_parser
    p = get_args_parser()
    plain = p.parse_args([])
    assert not hasattr(plain, "render_worst") and not hasattr(plain, "render_ids")
    assert not hasattr(default_args(), "render_worst") and not hasattr(default_args(), "render_ids")
    assert not hasattr(p.parse_args(["--image_report"]), "render_worst")
    a = p.parse_args(["--image_report", "--render_worst", "2"])
    assert a.render_worst == 2 and a.image_report is True and not hasattr(a, "render_ids")
    a = p.parse_args(["--render_ids", "3,17", "--image_report"])
    assert a.render_ids == [3, 17] and not hasattr(a, "render_worst")
    a = p.parse_args(["--image_report", "--render_worst", "4", "--render_ids", "5"])
    assert (a.render_worst, a.render_ids) == (4, [5])
    for bad, names in ((["--render_worst", "2"], ["--render_worst"]), (["--render_ids", "3"], ["--render_ids"]),
                       (["--render_worst", "2", "--render_ids", "3"], ["--render_worst", "--render_ids"])):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    with pytest.raises(SystemExit):
        p.parse_args(["--image_report", "--render_worst", "-1"])


def test_the_error_names_both_flags(capsys):
    import infer as infer_mod
    from counting_detr_amd.args import get_args_parser
    with pytest.raises(SystemExit):
        get_args_parser().parse_args(["--render_worst", "2"])
    err = capsys.readouterr().err
    assert "--render_worst" in err and "--image_report" in err
    ns = get_args_parser().parse_args([])
    assert infer_mod.build_render(ns) is None
    ns.render_worst = 2                                                         # a namespace made by hand meets the same check at start-up
    with pytest.raises(ValueError, match="--render_worst.*--image_report"):
        infer_mod.build_render(ns)
    ns.image_report = True
    r = infer_mod.build_render(ns)
    assert (r.worst, r.ids) == (2, ())


# ------------------------------------------------------------------------------------------------------------------------- 5. header and _ffi
@pytest.fixture(scope="module")
def L():
    from counting_detr_amd import _ffi
    from counting_detr_amd.build import build_lib
    build_lib(verbose=False)
    return _ffi.lib()


def test_entry_is_declared_exported_and_the_abi_stays(L):
    from counting_detr_amd import _ffi
    src = re.sub(r"/\*.*?\*/", "", abi_header.source(), flags=re.S)
    assert re.search(r"^int\s+cdetr_render_boxes\s*\(", src, flags=re.M)
    assert "cdetr_render_boxes" in _ffi.EXPORTS and hasattr(L, "cdetr_render_boxes") and len(L.cdetr_render_boxes.argtypes) == 26
    assert L.cdetr_abi_version() == 2
    defines = dict(re.findall(r"#define CDETR_RENDER_(TILE_H|TILE_W|CHUNK) (\d+)", abi_header.source()))
    assert (render.TILE_H, render.TILE_W, render.CHUNK) == (int(defines["TILE_H"]), int(defines["TILE_W"]), int(defines["CHUNK"]))
    assert "render.hip" in __import__("counting_detr_amd.build", fromlist=["SOURCES"]).SOURCES


def _call(L, K=1, B=1, D=0, G=0, E=0, max_h=8, max_w=8, dot=1, null=(), sel_host=None):
    """cdetr_render_boxes with pointers into one HOST buffer: every case below returns before any launch, nothing is dereferenced on a device."""
    buf = ctypes.create_string_buffer(4096)
    at = ctypes.addressof(buf)
    names = ["pix", "pix_off", "size", "sel", "sel_host", "dt_boxes", "dt_off", "dt_cnt", "matched", "det_ignored", "gt_boxes", "gt_off", "ex_boxes",
             "ex_off", "style"]
    ptrs = {n: at for n in names}
    ptrs["sel_host"] = None if sel_host is None else ctypes.addressof(sel_host)
    for n in null:
        ptrs[n] = None
    rc = L.cdetr_render_boxes(*[ptrs[n] for n in names], K, B, D, G, E, max_h, max_w, dot, 4096, None if "out" in null else at, None)
    return rc, L.cdetr_last_error()


def test_validation_happens_before_any_launch(L):
    assert _call(L, K=0, null=("pix", "pix_off", "size", "sel", "style", "out"))[0] == 0              # nothing to draw, nothing required
    for name in ("pix", "pix_off", "size", "sel", "style", "out"):
        rc, msg = _call(L, null=(name,))
        assert rc == -1 and b"cdetr_render_boxes" in msg, name
    for kw in (dict(D=1, null=("dt_boxes",)), dict(D=1, null=("matched",)), dict(D=1, null=("det_ignored",)), dict(D=1, null=("dt_off",)),
               dict(G=1, null=("gt_boxes",)), dict(G=2, null=("gt_off",)), dict(E=1, null=("ex_boxes",)), dict(E=1, null=("ex_off",)),
               dict(K=-1), dict(B=-1), dict(D=-1)):
        rc, msg = _call(L, **kw)
        assert rc == -1 and b"cdetr_render_boxes" in msg, kw
    for kw in (dict(max_h=0), dict(max_w=0), dict(max_h=16385), dict(max_w=16385), dict(max_h=-5), dict(K=65536)):
        rc, msg = _call(L, **kw)
        assert rc == -3 and b"cdetr_render_boxes" in msg, kw
    for sel, B in (([0, 3], 3), ([-1, 0], 3), ([0, 0], 0)):
        rc, msg = _call(L, K=2, B=B, sel_host=(ctypes.c_int32 * 2)(*sel))
        assert rc == -3 and b"sel" in msg, (sel, B)


def test_ops_render_boxes_checks_dtypes_shapes_and_devices():
    import torch
    from counting_detr_amd import ops
    u8, i32, i64, f64 = (lambda *s: torch.zeros(s, dtype=torch.uint8)), (lambda *s: torch.zeros(s, dtype=torch.int32)), \
        (lambda *s: torch.zeros(s, dtype=torch.int64)), (lambda *s: torch.zeros(s, dtype=torch.float64))
    good = dict(pix=u8(12), pix_off=i64(2), size=i32(1, 2), sel=i32(1), dt_boxes=f64(0, 4), dt_off=i32(2), matched50=u8(0), ignored50=u8(0),
                gt_boxes=f64(0, 4), gt_off=i32(2), ex_boxes=f64(0, 4), ex_off=i32(2), style=u8(5, 4))
    with pytest.raises(RuntimeError, match="float64.*dt_boxes"):
        ops.render_boxes(**{**good, "dt_boxes": torch.zeros((0, 4), dtype=torch.float32)})
    with pytest.raises(RuntimeError, match="int64.*pix_off"):
        ops.render_boxes(**{**good, "pix_off": i32(2)})
    with pytest.raises(RuntimeError, match="uint8.*matched50"):
        ops.render_boxes(**{**good, "matched50": torch.zeros(0, dtype=torch.bool)})
    with pytest.raises(RuntimeError, match="render_boxes: size"):
        ops.render_boxes(**{**good, "ex_off": i32(3)})
    with pytest.raises(RuntimeError, match="render_boxes: size"):
        ops.render_boxes(**{**good, "dt_cnt": i32(4)})
    with pytest.raises(RuntimeError, match="device tensors"):                     # no CPU fallback: the product path refuses host tensors
        ops.render_boxes(**good, sel_host=[0], max_hw=(2, 2))


# -------------------------------------------------------------------------------------------------- 6. the host route end to end, no model
def crafted_predictions(root, seed=5):
    """A predictions dict for tests/eval_split.py's five images: jittered copies of some ground truths (hits at IoU 0.5 and misses) and strays,
    in the wire format ([cx, cy, w, h] ints), plus what infer.py holds beside it after a pass."""
    rng = np.random.default_rng(seed)
    with open(os.path.join(root, "instances_val.json")) as f:
        inst = json.load(f)
    predictions = {"categories": [{"name": "fg", "id": 1}], "images": [], "annotations": []}
    image_ids, gt_counts, pred_counts = [], [], []
    for im in inst["images"]:
        gts = [a["bbox"] for a in inst["annotations"] if a["image_id"] == im["id"]]
        boxes = [[x + w / 2 + rng.normal(0, 0.8), y + h / 2 + rng.normal(0, 0.8), w, h] for x, y, w, h in gts[:-1]]
        boxes += [[rng.uniform(5, im["width"] - 5), rng.uniform(5, im["height"] - 5), rng.uniform(3, 15), rng.uniform(3, 15)] for _ in range(3)]
        if im["id"] == 4:
            boxes = []                                                          # an image without a detection
        for b in boxes:
            predictions["annotations"].append({"id": len(predictions["annotations"]) + 1, "image_id": im["id"], "area": int(b[2] * b[3]),
                                               "bbox": [int(v) for v in b], "category_id": 1, "score": round(float(rng.uniform(0.5, 1.0)), 2),
                                               "point": [int(b[0]), int(b[1])]})
        predictions["images"].append({"id": im["id"], "height": im["height"], "width": im["width"], "file_name": "None"})
        image_ids.append(im["id"]); gt_counts.append(len(gts)); pred_counts.append(len(boxes))
    return predictions, image_ids, gt_counts, pred_counts


def expected_overlay(root, predictions, image_id):
    """The painter on one image of the split, fed from the files and coco_ap's host matcher directly."""
    from PIL import Image
    with open(os.path.join(root, "instances_val.json")) as f:
        inst = json.load(f)
    with open(os.path.join(root, "annotation_FSC147_384.json")) as f:
        anno = json.load(f)
    name = {im["id"]: im["file_name"] for im in inst["images"]}[image_id]
    gts = [{"bbox": [float(v) for v in a["bbox"]], "area": float(a["area"]), "iscrowd": 0} for a in inst["annotations"] if a["image_id"] == image_id]
    dts = [{"bbox": ca.reference_box(a["bbox"]), "score": a["score"]} for a in predictions["annotations"] if a["image_id"] == image_id]
    for d in dts:
        d["area"] = float(d["bbox"][2] * d["bbox"][3])
    order = np.argsort([-d["score"] for d in dts], kind="mergesort")
    _, matched, ignored, _ = ca._evaluate_image(dts, gts, ca.AREA_RNG["all"], ca.MAX_DETS)
    T = len(ca.IOU_THRS)
    cls = rr.classes_of(matched.reshape(T, -1)[0], ignored.reshape(T, -1)[0])
    exs = [[b[0][0], b[0][1], b[2][0] - b[0][0], b[2][1] - b[0][1]] for b in anno[name]["box_examples_coordinates"]]
    canvas = np.asarray(Image.open(os.path.join(root, "images_384_VarV2", name)).convert("RGB"))
    return rr.paint(canvas, [dts[i]["bbox"] for i in order], cls, [g["bbox"] for g in gts], exs), cls, name


def test_host_route_end_to_end_without_a_model(tmp_path):
    from PIL import Image
    import infer as infer_mod
    root = es.write_split(tmp_path / "ds")
    predictions, image_ids, gt_counts, pred_counts = crafted_predictions(root)
    report = infer_mod.ImageReport(os.path.join(root, "instances_val.json"), None)
    report.split = "val"
    report.from_predictions(predictions, image_ids, gt_counts, pred_counts, 0.5)
    out = tmp_path / "out"
    os.makedirs(out)
    r = infer_mod.Render(root, 2, (4,))
    out_dir = r.from_predictions(predictions, image_ids, report, str(out), 0.5)
    assert out_dir == str(out / "render_val") == r.out_dir
    picks = render.select(report.report, 2, (4,))
    assert 3 <= len(picks) <= 5 and any(p["image_id"] == 4 and "id" in p["reasons"] for p in picks)
    assert sorted(os.listdir(out_dir)) == sorted(["index.json"] + [f"{p['image_id']}.png" for p in picks])
    seen = set()
    for p in picks:
        want, cls, _ = expected_overlay(root, predictions, p["image_id"])
        got = np.asarray(Image.open(os.path.join(out_dir, f"{p['image_id']}.png")))
        same_images([got], [want])
        seen |= {tuple(px) for px in got.reshape(-1, 3).tolist()} & {tuple(v[:3]) for v in rr.STYLE}
    assert {tuple(rr.STYLE[k][:3]) for k in (rr.TP, rr.FP, rr.GT, rr.EXEMPLAR)} <= seen         # hits, misses, ground truths and exemplars all show
    index = json.load(open(os.path.join(out_dir, "index.json")))
    assert list(index) == ["split", "threshold", "style", "dot", "images"]
    assert (index["split"], index["threshold"], index["style"], index["dot"]) == ("val", 0.5, rr.STYLE, 1)
    rows = {row["image_id"]: row for row in report.report["rows"]}
    names = dict(zip(range(1, 6), [im[0] for im in es.IMAGES]))
    for entry, p in zip(index["images"], picks):
        assert list(entry) == ["image_id", "file_name", "png", "reasons", "row"]
        assert entry["image_id"] == p["image_id"] and entry["reasons"] == p["reasons"] and entry["png"] == f"{p['image_id']}.png"
        assert entry["file_name"] == names[p["image_id"]]
        assert json.dumps(entry["row"]) == json.dumps(rows[p["image_id"]])
    # a second pass into the same directory leaves only its own files
    infer_mod.Render(root, 0, (1,)).from_predictions(predictions, image_ids, report, str(out), 0.5)
    assert sorted(os.listdir(out_dir)) == ["1.png", "index.json"]
