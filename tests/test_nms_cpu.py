"""The suppression rule on the host: counting_detr_amd/nms.py against the serial restatement of tests/nms_ref.py, the constructed cases, the
prefix property that lets one pass serve a sweep, the --nms_iou flag, and a host-loop pass of infer.py on tests/golden/fsc147_tiny.  Every
comparison is exact."""
import json
import os

import numpy as np
import pytest
import torch

from counting_detr_amd import nms
from counting_detr_amd import threshold_sweep as ts

import nms_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("seed,Q,counts,clusters,iou", [(1, 96, (60, 0, 1), 5, 0.5), (2, 300, (130, 65, 300), 12, 0.5), (3, 200, (200, 64), 9, 0.3),
                                                       (4, 150, (129, 128), 7, 0.7), (5, 81, (81,), 0, 0.0)])
def test_suppress_equals_the_serial_restatement(seed, Q, counts, clusters, iou):
    rng = np.random.default_rng(seed)
    prob, boxes, hw = ref.batch(rng, Q, counts, clusters)
    got, want = nms.suppress(prob, boxes, hw, 0.5, iou), ref.suppress(prob, boxes, hw, 0.5, iou)
    share = want[1].sum() / max(sum(counts), 1)
    print("candidates", counts, "removed", want[1].tolist(), "share", share)
    assert ref.same(got, want)
    assert np.array_equal(np.isnan(got[0]).sum(1) - np.isnan(prob).sum(1), got[1])            # `removed` counts the new NaNs
    if clusters:
        assert share >= 1 / 3                      # clustered boxes: the test cannot pass with nothing suppressed
    else:
        assert share == 0                          # disjoint boxes: nothing goes even at iou = 0


@pytest.mark.parametrize("name", sorted(ref.constructed()))
def test_constructed_cases(name):
    prob, boxes, hw, threshold, iou, gone = ref.constructed()[name]
    out, removed = nms.suppress(prob, boxes, hw, threshold, iou)
    assert ref.same((out, removed), ref.suppress(prob, boxes, hw, threshold, iou))
    bits, was = out.view(np.uint32)[0], prob.view(np.uint32)[0]
    assert [q for q in range(prob.shape[1]) if bits[q] != was[q]] == gone and removed.tolist() == [len(gone)]
    assert all(np.isnan(out[0, q]) for q in gone)
    if name.startswith("special"):
        assert bits[1] == ref.NAN_BITS and bits[2] == 0x80000000 and out[0, 3] == np.float32(0.25)


def test_the_prefix_property_lets_one_pass_serve_a_sweep():
    rng = np.random.default_rng(11)
    prob, boxes, hw = ref.batch(rng, 400, (400, 250, 3), 14, threshold=0.1)
    sweep = ts.parse_spec("0.1:0.9:9")
    low, _ = nms.suppress(prob, boxes, hw, sweep[0], 0.5)
    differ = 0
    for t in sweep:
        at_t, removed = nms.suppress(prob, boxes, hw, t, 0.5)
        k = ts.kept(prob, t)
        assert np.array_equal(np.isnan(at_t)[k], np.isnan(low)[k]) and removed.sum() == np.isnan(at_t)[k].sum(), t
        assert np.array_equal(ts.kept(at_t, t), ts.kept(low, t))                               # what every reader downstream sees
        differ += int((np.isnan(at_t) != np.isnan(low)).sum())
    assert differ > 0 and np.isnan(low)[ts.kept(prob, sweep[-1])].any()                        # the passes do differ below their thresholds


def test_iou_one_is_the_identity_and_the_range_is_checked():
    rng = np.random.default_rng(12)
    prob, boxes, hw = ref.batch(rng, 120, (120, 40), 3)
    out, removed = nms.suppress(prob, boxes, hw, 0.5, 1.0)
    assert np.array_equal(out.view(np.uint32), prob.view(np.uint32)) and removed.tolist() == [0, 0] and out is not prob
    assert nms.suppress(prob, boxes, hw, 0.5, 0.5)[1].sum() > 0
    for bad in (-0.01, 1.01, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="nms_iou"):
            nms.suppress(prob, boxes, hw, 0.5, bad)
    with pytest.raises(ValueError, match="prob"):
        nms.suppress(prob, boxes[:, :-1], hw, 0.5, 0.5)


def test_the_flag_leaves_no_trace_when_absent_and_is_checked_when_parsed(capsys):
    from counting_detr_amd.args import get_args_parser
    parser = get_args_parser()
    assert not hasattr(parser.parse_args([]), "nms_iou")
    assert parser.parse_args(["--nms_iou", "0.5"]).nms_iou == 0.5 and parser.parse_args(["--nms_iou", "1"]).nms_iou == 1.0
    assert parser.parse_args(["--nms_iou", "0"]).nms_iou == 0.0
    for bad in ("1.5", "-0.1", "nan", "inf", "half"):
        with pytest.raises(SystemExit):
            parser.parse_args(["--nms_iou=" + bad])
        assert "--nms_iou" in capsys.readouterr().err


def test_the_descriptor_twin_names_the_header_fields_and_bad_arguments_come_back_as_errors():
    """The ctypes twin of cdetr_nms_suppress_desc against include/cdetr_hip.h, and the entry's argument checks, which run before any launch and
    so without a GPU: the limit Q <= 4096, the range of iou, a NaN threshold, null pointers."""
    import ctypes
    import abi_header
    from counting_detr_amd import _ffi
    d = _ffi.NmsSuppressDesc()
    assert abi_header.field_names("cdetr_nms_suppress_desc") == [f[0] for f in d._fields_]
    kinds = {"int32_t": ctypes.c_int32, "float": ctypes.c_float, "double": ctypes.c_double}
    for (name, base, pointer), (_, ctype) in zip(abi_header.struct_fields("cdetr_nms_suppress_desc"), d._fields_):
        assert ctype is (ctypes.c_void_p if pointer else kinds[base]), name
    assert "cdetr_nms_suppress" in _ffi.EXPORTS
    L = _ffi.lib()
    buf = (ctypes.c_char * 64)()
    where = ctypes.addressof(buf)

    def call(**kw):
        d = _ffi.NmsSuppressDesc()
        d.B, d.Q, d.threshold, d.iou = 1, 8, 0.5, 0.5
        d.prob, d.boxes, d.orig_hw, d.prob_out, d.removed = where, where, where, where + 32, where
        for k, v in kw.items():
            setattr(d, k, v)
        return L.cdetr_nms_suppress(ctypes.byref(d), None), L.cdetr_last_error().decode()
    for kw, word in (({"Q": 4097}, "4097"), ({"Q": 0}, "bad sizes"), ({"B": 65536}, "65536"), ({"iou": 1.5}, "iou"), ({"iou": -0.1}, "iou"),
                     ({"iou": float("nan")}, "iou"), ({"threshold": float("nan")}, "threshold"), ({"removed": None}, "null"), ({"prob_out": where}, "alias")):
        rc, msg = call(**kw)
        assert rc < 0 and "cdetr_nms_suppress" in msg and word in msg, (kw, rc, msg)


class _Engine:
    """Stands in for engine.InferenceEngine on the host: seeded, clustered detections per image instead of a forward."""

    def __init__(self, model, threshold, Q=90):
        self.model, self.threshold, self.Q, self.rng = model, threshold, Q, np.random.default_rng(5)

    def __call__(self, samples, rects, next_samples=None):
        B = samples.tensors.shape[0]
        rows = [ref.clustered(self.rng, self.Q, 40, 6, self.threshold) for _ in range(B)]
        prob = torch.from_numpy(np.stack([r[0] for r in rows]))
        outputs = {"pred_boxes": torch.from_numpy(np.stack([r[1] for r in rows])), "pred_logits": torch.zeros(B, self.Q, 2)}
        keep = prob >= self.threshold
        return keep.sum(-1), keep, outputs, outputs["pred_boxes"][..., :2].clone(), prob


class _Criterion(torch.nn.Module):
    def forward(self, outputs, targets):
        return {"loss_ce": torch.zeros(())}


def test_host_loop_pass_on_the_tiny_tree_writes_fewer_annotations(tmp_path):
    from torch.utils.data import DataLoader
    import infer as infer_mod
    from counting_detr_amd import data
    from counting_detr_amd.args import default_args
    from counting_detr_amd.engine import counting_metrics
    args = default_args()
    args.data_path, args.scale_factor = os.path.join(HERE, "golden", "fsc147_tiny"), 32
    vl = DataLoader(data.build_test_dataset(args, "val"), batch_size=1, shuffle=False, collate_fn=data.collate)
    model, out = torch.nn.Identity(), {}
    for name, iou in (("plain", None), ("nms", 0.5), ("one", 1.0)):
        os.makedirs(tmp_path / name)
        out[name] = infer_mod.infer(model, _Criterion(), vl, torch.device("cpu"), str(tmp_path / name), split="val", engine=_Engine(model, 0.5),
                                    nms_iou=iou)
    (m0, p0), (m1, p1), (m2, p2) = out["plain"], out["nms"], out["one"]
    print("plain", m0, "with --nms_iou 0.5", m1)
    assert "nms_removed" not in m0 and m2["nms_removed"] == 0 and {k: v for k, v in m2.items() if k != "nms_removed"} == m0 and p2 == p0
    n0, n1 = len(p0["annotations"]), len(p1["annotations"])
    assert m1["nms_removed"] >= n0 / 3 and n1 == n0 - m1["nms_removed"]
    assert json.load(open(tmp_path / "nms" / "predictions_val.json")) == p1
    ids = [im["id"] for im in p1["images"]]
    gt = [int(b["targets"][0]["boxes"].shape[0]) for b in vl]                                # the loop's own ground-truth counts, in its order
    counts = [sum(1 for a in p1["annotations"] if a["image_id"] == i) for i in ids]
    again = counting_metrics(counts, gt)
    assert all(m1[k] == again[k] for k in ("MAE", "RMSE", "NAE", "SRE")) and m1["MAE"] != m0["MAE"]
    kept_ids = {(a["image_id"], tuple(a["bbox"]), a["score"]) for a in p1["annotations"]}
    assert kept_ids < {(a["image_id"], tuple(a["bbox"]), a["score"]) for a in p0["annotations"]}       # survivors are a subset, fields untouched
