"""Host side of the device detections path (infer.py --device_detections; cdetr_emit_detections, ops.DetectionStore, coco_ap.pack_store):
what can be checked without a GPU.  tests/detections_ref.py restates the kernel's rules in numpy; here it is pinned to the code those rules
come from -- infer.py's literal per-detection loop (through json), coco_ap.reference_box, coco_ap.pack_images -- with array_equal.
tests/test_detections_gpu.py compares the kernel with the same checker."""
import ctypes
import json
import re

import numpy as np
import pytest
import torch

from counting_detr_amd import coco_ap as ca

import abi_header
import detections_ref as dr

HWS = [(384, 683), (512, 384), (300, 301), (768, 1024)]


@pytest.fixture(scope="module")
def L():
    from counting_detr_amd.build import build_lib
    build_lib(verbose=False)
    from counting_detr_amd import _ffi
    return _ffi.lib()


@pytest.fixture(scope="module")
def images():
    """Four images of 70 queries with ties, a probability at the threshold, a NaN and overhanging boxes; one image keeps nothing."""
    rng = np.random.default_rng(31)
    out = [dr.make_case(rng, 70, HWS[0], ties=3, at_threshold=True, nan=True), dr.make_case(rng, 70, HWS[1], ties=2),
           dr.make_case(rng, 70, HWS[2], kept="none"), dr.make_case(rng, 70, HWS[3], kept="all", ties=4)]
    return [tuple(a[None] for a in c) for c in out]            # each a launch of B = 1


def host_loop(prob, boxes_n, pts_n, ori_h, ori_w, image_id, anno_id, threshold=0.5):
    """infer.py's per-image body, statement for statement, on numpy arrays (what `.cpu().numpy()` hands it)."""
    keep = prob >= np.float32(threshold)
    scores = prob[keep]
    boxes = boxes_n[keep].copy()
    pts = pts_n[keep].copy()
    pts[..., 0] *= ori_w; pts[..., 1] *= ori_h
    boxes[..., 0] *= ori_w; boxes[..., 1] *= ori_h; boxes[..., 2] *= ori_w; boxes[..., 3] *= ori_h
    anns = []
    for sc, bx, pt in zip(scores, boxes, pts):
        x_cen, y_cen, w, h = bx
        anns.append({"id": anno_id, "image_id": image_id, "area": int(w * h),
                     "bbox": [int(x_cen), int(y_cen), int(w), int(h)], "category_id": 1,
                     "score": float(sc), "point": [int(pt[0]), int(pt[1])]})
        anno_id += 1
    return anns


def test_checker_equals_the_host_loop_through_json(images):
    ref = dr.emit_store(images, 0.5, ca.MAX_DETS)
    anns = []
    for n, (prob, boxes, pts, hw) in enumerate(images):
        with np.errstate(invalid="ignore"):
            anns += host_loop(prob[0], boxes[0], pts[0], int(hw[0][0]), int(hw[0][1]), 100 + n, len(anns) + 1)
    anns = json.loads(json.dumps({"annotations": anns}))["annotations"]
    assert len(anns) == len(ref["wire"]) == int(ref["wire_off"][-1]) and len(anns) > 100
    assert ref["counts"].tolist() == [sum(1 for a in anns if a["image_id"] == 100 + n) for n in range(len(images))] and ref["counts"][2] == 0
    assert np.array_equal(np.array([a["bbox"] + [a["area"]] + a["point"] for a in anns]), ref["wire"])
    assert np.array_equal(np.array([a["score"] for a in anns]), ref["score"].astype(np.float64))
    assert [a["id"] for a in anns] == list(range(1, len(anns) + 1))          # ids number the records by image and then by query
    # the conditions the cases are there for
    p0 = images[0][0][0]
    assert np.isnan(p0).sum() == 1 and (p0 == np.float32(0.5)).sum() == 1 and np.float32(0.5) in ref["images"][0]["score"]
    assert any((np.bincount(np.unique(i["score"], return_inverse=True)[1]) >= 3).any() for i in ref["images"] if len(i["score"]))
    w = ref["wire"].astype(np.int64)
    assert (w[:, 4] != w[:, 2] * w[:, 3]).any()                              # the area is NOT the product of the truncated sides


def test_checker_equals_reference_box_and_pack_images(images):
    for max_det in (ca.MAX_DETS, 5):
        ref = dr.emit_store(images, 0.5, max_det)
        dt_by = {}
        for n, im in enumerate(ref["images"]):
            for rec, sc in zip(im["wire"].tolist(), im["score"].astype(np.float64).tolist()):
                b = ca.reference_box(rec[:4])                                 # as ap_from_json forms a detection from an annotation
                dt_by.setdefault(100 + n, []).append({"bbox": b, "score": float(sc), "area": float(b[2] * b[3])})
        gts = {100 + n: [{"bbox": [1.0, 2.0, 3.0, 4.0], "area": 12.0}] for n in range(len(images))}
        pack = ca.pack_images(gts, dt_by, max_det)
        assert pack["image_ids"] == [100, 101, 102, 103]
        assert np.array_equal(pack["dt_off"], ref["eval_off"]) and pack["dt_off"].dtype == ref["eval_off"].dtype
        for k in ("boxes", "area", "score"):
            assert pack["dt_" + k].dtype == ref["eval_" + k].dtype and np.array_equal(pack["dt_" + k], ref["eval_" + k]), (k, max_det)
        assert (ref["eval_boxes"][:, :2] < 0).any()                           # a corner left of / above the image
        if max_det == 5:
            assert (np.diff(ref["eval_off"]) == [5, 5, 0, 5]).all() and (ref["counts"][[0, 1, 3]] > 5).all()
    assert dr.tdiv2([-3, -2, -1, 0, 1, 2, 3]).tolist() == [int(t / 2) for t in (-3, -2, -1, 0, 1, 2, 3)] == [-1, -1, 0, 0, 0, 1, 1]


def _fill(store, ref):
    """Put the checker's arrays into a (CPU) DetectionStore the way the kernel leaves them."""
    n, W, E = len(ref["counts"]), len(ref["wire"]), len(ref["eval_score"])
    store.counts[:n] = torch.from_numpy(ref["counts"])
    store.wire_off[:n + 1] = torch.from_numpy(ref["wire_off"])
    store.eval_off[:n + 1] = torch.from_numpy(ref["eval_off"])
    store.wire[:W, :7] = torch.from_numpy(ref["wire"])
    store.wire[:W, 7] = torch.from_numpy(ref["score"].view(np.int32).copy())
    store.eval_boxes[:E], store.eval_area[:E] = torch.from_numpy(ref["eval_boxes"]), torch.from_numpy(ref["eval_area"])
    store.eval_score[:E] = torch.from_numpy(ref["eval_score"])
    store.first = n


def test_store_layout_finish_and_pack_store_order(images):
    """ops.DetectionStore on CPU memory, filled from the checker: `finish` returns the arrays, `pack_store` orders the images like
    `pack_images` -- sorted ids, images with neither ground truth nor detection left out, a ground-truth-only image kept -- whether the store's
    own order is that order (no gather) or not (gather from the offsets)."""
    from counting_detr_amd import ops
    ref = dr.emit_store(images, 0.5, 5)
    for ids in ([100, 101, 102, 103], [103, 100, 102, 101]):
        store = ops.DetectionStore(6, 70, "cpu", max_det=5)
        assert store.wire_cap == 420 and store.eval_cap == 30 and int(store.wire_off[0]) == 0 and int(store.status[0]) == 0
        _fill(store, ref)
        host = store.finish()
        for k in ("counts", "wire_off", "eval_off", "wire", "score", "eval_score"):
            assert host[k].dtype == ref[k].dtype and np.array_equal(host[k], ref[k]), k
        dt_by = {}
        for n, im in enumerate(ref["images"]):
            for rec, sc in zip(im["wire"].tolist(), im["score"].astype(np.float64).tolist()):
                b = ca.reference_box(rec[:4])
                dt_by.setdefault(ids[n], []).append({"bbox": b, "score": float(sc), "area": float(b[2] * b[3])})
        gts = {ids[0]: [{"bbox": [1.0, 2.0, 3.0, 4.0], "area": 12.0}], 7: [{"bbox": [0.0, 0.0, 5.0, 5.0], "area": 25.0, "iscrowd": 1}]}
        want = ca.pack_images(gts, dt_by, 5)
        got = ca.pack_store(gts, store, ids)
        assert got["image_ids"] == want["image_ids"] == sorted([7] + [i for i in ids if i != ids[2]])      # ids[2] kept nothing and has no ground truth
        for k in ("gt_boxes", "gt_area", "gt_ignore", "gt_off", "dt_score", "dt_off"):
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
        assert got["g_max"] == want["g_max"]
        assert np.array_equal(got["dt_device"][0].numpy(), want["dt_boxes"]) and np.array_equal(got["dt_device"][1].numpy(), want["dt_area"])
    with pytest.raises(RuntimeError, match="image ids"):
        ca.pack_store(gts, store, ids[:3])
    store.status[0] = 1
    store._host = None
    with pytest.raises(RuntimeError, match="cdetr_emit_detections reported status 1"):
        store.finish()


@pytest.mark.parametrize("cls, args, kw, cuts", [
    ("DetectionStore", (6, 70), dict(max_det=5), [0, 16, 48, 80, 112, 352, 13792, 14752, 14992]),
    ("DetectionStore", (3, 257), dict(max_det=100), [0, 16, 32, 48, 64, 2464, 27136, 36736, 39136]),
    ("DetectionStore", (3, 70), dict(wire_cap=69, eval_cap=69), [0, 16, 32, 48, 64, 624, 2832, 5040, 5600]),
    ("DetectionStore", (1, 900), {}, [0, 16, 32, 48, 64, 7264, 36064, 64864, 72064]),
    ("PseudoLabelStore", (6, 533), {}, [0, 16, 48, 80, 112, 4384, 21440, 25712, 42768, 47040]),
    ("PseudoLabelStore", (2, 10), dict(max_det=4), [0, 16, 32, 48, 64, 128, 448, 528, 784, 848]),
    ("PseudoLabelStore", (1, 0), {}, [0, 16, 32, 48, 64, 64, 64, 64, 64, 64])])
def test_store_sections_are_cut_where_they_always_were(cls, args, kw, cuts):
    """The byte layout of both stores, pinned with literals: [status | counts | wire offsets | eval_off | eval_score | wire | (pair_iou) |
    eval_boxes | eval_area], every section 16-byte aligned, every member a view of its section, the head zeroed."""
    from counting_detr_amd import ops
    s = getattr(ops, cls)(*args, "cpu", **kw)
    assert s._cuts == cuts and s.buf.numel() == cuts[-1] and s.first == 0 and s._host is None
    N, E = s.N, s.eval_cap
    off, W = (s.wire_off, s.wire_cap) if cls == "DetectionStore" else (s.row_off, s.row_cap)
    assert E == 8 or kw.get("max_det") != 4
    members = [(s.status, (1,), torch.int32), (s.counts, (N,), torch.int32), (off, (N + 1,), torch.int32), (s.eval_off, (N + 1,), torch.int32),
               (s.eval_score, (E,), torch.float64), (s.wire, (W, 8), torch.int32)] + \
              ([(s.pair_iou, (W,), torch.float64)] if cls == "PseudoLabelStore" else []) + \
              [(s.eval_boxes, (E, 4), torch.float64), (s.eval_area, (E,), torch.float64)]
    assert len(members) == len(cuts) - 1
    for k, (t, shape, dt) in enumerate(members):
        assert tuple(t.shape) == shape and t.dtype == dt and t.is_contiguous(), k
        assert t.numel() * t.element_size() <= cuts[k + 1] - cuts[k] and (t.numel() == 0 or t.data_ptr() == s.buf.data_ptr() + cuts[k]), k
    assert not s.buf[:cuts[4]].any()


def test_entry_exported_declared_and_documented(L):
    from counting_detr_amd import _ffi, build
    src = abi_header.source()
    assert "cdetr_emit_detections" in _ffi.EXPORTS and hasattr(L, "cdetr_emit_detections")
    assert re.search(r"^int cdetr_emit_detections\(const cdetr_emit_detections_desc\* d, void\* stream\);", src, flags=re.M)
    assert "detections.hip" in build.SOURCES and L.cdetr_abi_version() == 2
    lines = [ln for ln in abi_header.struct_body("cdetr_emit_detections_desc").splitlines() if ln.strip()]
    assert all("/*" in ln and "*/" in ln for ln in lines), [ln for ln in lines if "/*" not in ln]      # every field carries its comment
    assert abi_header.field_names("cdetr_emit_detections_desc") == [f[0] for f in _ffi.EmitDetectionsDesc._fields_]
    assert ctypes.sizeof(_ffi.EmitDetectionsDesc) == 32 + 12 * 8


def test_bad_arguments_are_refused_before_any_launch(L):
    from counting_detr_amd import _ffi
    assert L.cdetr_emit_detections(None, None) < 0 and b"cdetr_emit_detections" in L.cdetr_last_error()
    raw = (ctypes.c_char * 64)()
    a16 = (ctypes.addressof(raw) + 15) & ~15                                   # a 16-byte aligned host address: never dereferenced

    def desc(**kw):
        d = _ffi.EmitDetectionsDesc()
        d.B, d.Q, d.N, d.first, d.max_det, d.wire_cap, d.eval_cap, d.threshold = 1, 900, 4, 0, 1100, 3600, 3600, 0.5
        for f, _ in _ffi.EmitDetectionsDesc._fields_[8:]:
            setattr(d, f, a16)                               # non-null: the size checks are what refuse
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    for bad in (dict(Q=4097), dict(B=65536), dict(B=-1), dict(Q=-5), dict(Q=0), dict(N=-1), dict(first=-1), dict(max_det=-1), dict(wire_cap=-1),
                dict(eval_cap=-2), dict(first=4), dict(B=3, first=2), dict(wire_cap=(1 << 30) + 1), dict(prob=None), dict(status=None), dict(wire=None),
                dict(eval_area=None), dict(wire=a16 + 8)):
        rc = L.cdetr_emit_detections(ctypes.byref(desc(**bad)), None)
        assert rc < 0 and b"cdetr_emit_detections" in L.cdetr_last_error(), bad
    assert L.cdetr_emit_detections(ctypes.byref(desc(Q=4097)), None) == -3 and b"4097" in L.cdetr_last_error()      # CDETR_ERR_UNSUPPORTED
    assert _ffi.EmitDetectionsDesc().B == 0 and L.cdetr_emit_detections(ctypes.byref(_ffi.EmitDetectionsDesc()), None) < 0


def test_wrappers_refuse_what_the_kernel_cannot_take():
    from counting_detr_amd import ops
    store = ops.DetectionStore(2, 8, "cpu")
    p, b, r, hw = torch.zeros(1, 8), torch.zeros(1, 8, 4), torch.zeros(1, 8, 2), torch.zeros(1, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="float32"):
        ops.emit_detections(p.double(), b, r, hw, store, 0)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.emit_detections(torch.zeros(1, 8, 2)[..., 0], b, r, hw, store, 0)
    with pytest.raises(RuntimeError, match="int32"):
        ops.emit_detections(p, b, r, hw.long(), store, 0)
    with pytest.raises(RuntimeError, match=r"orig_hw \[B, 2\]"):
        ops.emit_detections(p, b, r[:, :4], hw, store, 0)
    with pytest.raises(RuntimeError, match="Q = 7"):
        ops.emit_detections(p[:, :7].contiguous(), b[:, :7].contiguous(), r[:, :7].contiguous(), hw, store, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.emit_detections(p, b, r, hw, store, 0)                             # host tensors: there is no host implementation behind it
    store.first = 2
    with pytest.raises(RuntimeError, match="store of 2"):
        store.emit(p, b, r, hw)
    with pytest.raises(RuntimeError, match="bad sizes"):
        ops.DetectionStore(0, 8, "cpu")


def test_clis_have_the_switch_and_the_host_path_is_the_default():
    import inspect
    import infer as infer_mod
    from counting_detr_amd.args import get_args_parser
    assert get_args_parser().parse_args([]).device_detections is False
    assert get_args_parser().parse_args(["--device_detections"]).device_detections is True
    sig = inspect.signature(infer_mod.infer)
    assert sig.parameters["device_detections"].default is False and sig.parameters["gt_json"].default is None
    with pytest.raises(RuntimeError, match="HIP kernels"):
        infer_mod._infer_device(None, None, [], torch.device("cpu"), "unused", 0.5, None)
