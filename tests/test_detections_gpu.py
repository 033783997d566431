"""cdetr_emit_detections (csrc/detections.hip) behind ops.DetectionStore, coco_ap.summarize_store and infer.py --device_detections, against
the numpy checker tests/detections_ref.py (pinned to the host path by tests/test_detections_cpu.py) and, end to end, against the host path
itself.  Every comparison is array_equal / ==: no tolerance, no case left out."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from counting_detr_amd import coco_ap as ca
from counting_detr_amd import ops

import detections_ref as dr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
HW3 = [(384, 683), (683, 384), (511, 1023)]                  # non-square, different per image
KEYS = ("counts", "wire_off", "eval_off", "wire", "score", "eval_score")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_store(batches, threshold=0.5, max_det=ca.MAX_DETS, n_images=None, **caps):
    """The launches of `batches` into one fresh store -> (store, finish() dict + the device-resident evaluation arrays)."""
    n = sum(len(b[0]) for b in batches)
    store = ops.DetectionStore(n if n_images is None else n_images, batches[0][0].shape[1], DEV, threshold=threshold, max_det=max_det, **caps)
    for prob, boxes, points, hw in batches:
        store.emit(T(prob), T(boxes), T(points), T(hw))
    host = dict(store.finish())
    E = int(host["eval_off"][-1])
    host["eval_boxes"], host["eval_area"] = store.eval_boxes[:E].cpu().numpy(), store.eval_area[:E].cpu().numpy()
    return store, host


def check(batches, threshold=0.5, max_det=ca.MAX_DETS):
    ref = dr.emit_store(batches, threshold, max_det)
    _, got = run_store(batches, threshold, max_det)
    for k in KEYS + ("eval_boxes", "eval_area"):
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (k, got[k].dtype, got[k].shape, ref[k].shape)
        bad = int((got[k] != ref[k]).sum())
        print(f"{k}: {bad} of {ref[k].size} differ")
        assert np.array_equal(got[k], ref[k]), k
    return ref


def batch(cases):
    return tuple(np.stack([c[k] for c in cases]) for k in range(4))


def both(make):
    """A case alone (B = 1) and as image 1 of a B = 3 launch with a different original size per image."""
    rng = np.random.default_rng(7)
    one = make(rng, HW3[0])
    refs = [check([batch([one])])]
    three = [make(rng, HW3[0]), make(rng, HW3[1]), make(rng, HW3[2])]
    refs.append(check([batch(three)]))
    return refs


@pytest.mark.parametrize("Q", [1, 64, 70, 257])
def test_sizes(Q):
    refs = both(lambda rng, hw: dr.make_case(rng, Q, hw, kept="some" if Q > 1 else "all"))
    if Q > 1:
        assert all(0 < c < Q for r in refs for c in r["counts"])
    else:
        assert all(r["counts"].tolist() == [1] * len(r["counts"]) for r in refs)
        check([batch([dr.make_case(np.random.default_rng(1), 1, HW3[0], kept="none")])])


def test_equal_scores_at_non_adjacent_queries():
    for r in both(lambda rng, hw: dr.make_case(rng, 130, hw, ties=6)):
        for im in r["images"]:
            s, q = im["eval_score"], im["eval_q"]
            same = np.nonzero(s[1:] == s[:-1])[0]
            assert len(same) >= 6 and (q[same + 1] > q[same] + 1).any() and (q[same + 1] > q[same]).all()      # ties, apart, in ascending query order


def test_probability_at_the_threshold_is_kept_and_a_nan_is_dropped():
    for r in both(lambda rng, hw: dr.make_case(rng, 70, hw, at_threshold=True, nan=True)):
        for im in r["images"]:
            assert (im["score"] == np.float32(0.5)).sum() == 1 and not np.isnan(im["score"]).any()
    rng = np.random.default_rng(3)
    c = dr.make_case(rng, 70, HW3[0], nan=True)
    assert np.isnan(c[0]).sum() == 1
    ref = check([batch([c])])
    assert ref["counts"][0] == int((c[0] >= np.float32(0.5)).sum())


def test_all_kept_and_none_kept():
    for r in both(lambda rng, hw: dr.make_case(rng, 70, hw, kept="all")):
        assert (r["counts"] == 70).all()
    for r in both(lambda rng, hw: dr.make_case(rng, 70, hw, kept="none")):
        assert (r["counts"] == 0).all() and r["wire_off"][-1] == 0 and r["eval_off"][-1] == 0
    rng = np.random.default_rng(4)                                           # an empty image between two full ones
    ref = check([batch([dr.make_case(rng, 70, HW3[0], kept="all"), dr.make_case(rng, 70, HW3[1], kept="none"), dr.make_case(rng, 70, HW3[2])])])
    assert ref["counts"][0] == 70 and ref["counts"][1] == 0 and ref["counts"][2] > 0


def test_boxes_whose_corner_goes_negative():
    for r in both(lambda rng, hw: dr.make_case(rng, 70, hw, negative_corner=True)):
        for im in r["images"]:
            assert (im["eval_boxes"][:, 0] < 0).any() and (im["eval_boxes"][:, 1] < 0).any()
            odd = (2 * im["wire"][:, 0].astype(np.int64) - im["wire"][:, 2]) % 2 == 1
            assert (odd & (2 * im["wire"][:, 0].astype(np.int64) < im["wire"][:, 2])).any()      # a negative ODD 2 cx - w: truncation differs from floor


def test_max_det_5_with_more_kept():
    rng = np.random.default_rng(5)
    one = [batch([dr.make_case(rng, 70, HW3[0], ties=3)])]
    three = [batch([dr.make_case(rng, 70, HW3[0], ties=3), dr.make_case(rng, 70, HW3[1], kept="none"), dr.make_case(rng, 70, HW3[2])])]
    for b in (one, three):
        ref = check(b, max_det=5)
        assert (ref["counts"][[0, -1]] > 5).all() and np.diff(ref["eval_off"])[[0, -1]].tolist() == [5, 5]


def test_max_det_1100_at_1728_queries():
    rng = np.random.default_rng(6)
    mk = lambda hw, kept: dr.make_case(rng, 1728, hw, kept=kept, ties=20, at_threshold=True, nan=True)      # noqa: E731
    ref = check([batch([mk(HW3[0], "all")])])
    assert ref["counts"][0] > 1100 and np.diff(ref["eval_off"]).tolist() == [1100]
    ref = check([batch([mk(HW3[0], "all"), mk(HW3[1], "some"), mk(HW3[2], "all")])])
    assert ref["counts"][0] > 1100 and ref["counts"][2] > 1100 and 0 < ref["counts"][1] < 1728
    assert np.diff(ref["eval_off"]).tolist() == [1100, min(int(ref["counts"][1]), 1100), 1100]
    ref = check([batch([dr.make_case(rng, 4096, HW3[2], kept="all", ties=10)])])                              # the largest Q the kernel takes
    assert ref["counts"][0] == 4096
    with pytest.raises(RuntimeError, match="cdetr_emit_detections.*4097"):
        c = batch([dr.make_case(rng, 4097, HW3[0])])
        ops.DetectionStore(1, 4097, DEV).emit(T(c[0]), T(c[1]), T(c[2]), T(c[3]))


def test_two_launches_into_one_store():
    rng = np.random.default_rng(8)
    first = batch([dr.make_case(rng, 257, HW3[k], ties=2) for k in range(3)])
    second = batch([dr.make_case(rng, 257, HW3[2 - k], at_threshold=True) for k in range(3)])
    ref1, ref = dr.emit_store([first], 0.5, 100), dr.emit_store([first, second], 0.5, 100)
    store = ops.DetectionStore(6, 257, DEV, max_det=100)
    assert store.emit(T(first[0]), T(first[1]), T(first[2]), T(first[3])) == 0
    h1 = {k: v.copy() for k, v in store.finish().items()}
    raw1 = store.buf.cpu().numpy().copy()
    assert store.emit(T(second[0]), T(second[1]), T(second[2]), T(second[3])) == 3 and store.first == 6
    h2 = store.finish()
    for k in KEYS:
        assert np.array_equal(h1[k], ref1[k]) and np.array_equal(h2[k], ref[k]), k
    assert h2["wire_off"][3] == ref1["wire_off"][3] > 0 and (np.diff(h2["wire_off"]) > 0).all()              # the offsets chain
    # the first launch's records are untouched, byte for byte, in every section of the store
    raw2, c = store.buf.cpu().numpy(), store._cuts
    W1, E1 = int(ref1["wire_off"][3]), int(ref1["eval_off"][3])
    for lo, n in ((c[4], 8 * E1), (c[5], 32 * W1), (c[6], 32 * E1), (c[7], 8 * E1)):
        assert np.array_equal(raw1[lo:lo + n], raw2[lo:lo + n])
    E = int(ref["eval_off"][-1])
    assert np.array_equal(store.eval_boxes[:E].cpu().numpy(), ref["eval_boxes"]) and np.array_equal(store.eval_area[:E].cpu().numpy(), ref["eval_area"])


def test_undersized_store_raises_and_writes_nothing_out_of_range():
    rng = np.random.default_rng(9)
    b = batch([dr.make_case(rng, 70, HW3[k], kept="all") for k in range(3)])
    for caps, word in ((dict(wire_cap=100, eval_cap=300), 1), (dict(wire_cap=300, eval_cap=100), 2), (dict(wire_cap=69, eval_cap=69), 3)):
        store = ops.DetectionStore(3, 70, DEV, **caps)
        c = store._cuts
        store.buf[c[4]:].fill_(0xA5)
        store.emit(T(b[0]), T(b[1]), T(b[2]), T(b[3]))
        with pytest.raises(RuntimeError, match=f"reported status {word}"):
            store.finish()
        raw = store.buf.cpu().numpy()
        fits = min(store.wire_cap, store.eval_cap) // 70                       # images that fit both sections are written in full
        ref = dr.emit_store([b], 0.5, ca.MAX_DETS)
        assert np.array_equal(raw[c[5]:c[5] + 32 * 70 * fits].view(np.int32).reshape(-1, 8)[:, :7], ref["wire"][:70 * fits])
        # nothing of an image that does not fit: the rest of each section, its padding and the section behind it still hold the fill
        for k, rec in ((4, 8), (5, 32), (6, 32), (7, 8)):
            assert (raw[c[k] + rec * 70 * fits:c[k + 1]] == 0xA5).all(), (caps, k)
        assert raw[c[1]:c[1] + 12].view(np.int32).tolist() == [70, 70, 70]     # the counts are still the images' own


GUARD = 8


def guarded_store(N, Q, wire_cap, eval_cap, threshold=0.5, max_det=ca.MAX_DETS):
    """What emit_detections needs of a DetectionStore, its arrays separate allocations with GUARD sentinel elements behind each."""
    size = {"status": 1, "counts": N, "wire_off": N + 1, "eval_off": N + 1, "wire": 8 * wire_cap, "eval_boxes": 4 * eval_cap, "eval_area": eval_cap,
            "eval_score": eval_cap}
    full = {k: torch.full((n + GUARD,), -777, dtype=torch.float64 if k.startswith("eval_") and k != "eval_off" else torch.int32, device=DEV)
            for k, n in size.items()}
    full["status"][0] = full["wire_off"][0] = full["eval_off"][0] = 0
    s = SimpleNamespace(N=N, Q=Q, threshold=threshold, max_det=max_det, wire_cap=wire_cap, eval_cap=eval_cap, buf=full["status"], full=full, size=size)
    for k, t in full.items():
        setattr(s, k, t[:size[k]])
    s.wire, s.eval_boxes = s.wire.view(-1, 8), s.eval_boxes.view(-1, 4)
    return s


def test_offsets_and_status_after_an_overflow():
    """Three calls of 3, 3 and 1 images, every query kept, into a store ONE record short of six images: images 0 .. 4 are in place; image 5
    fits neither section, writes nothing, sets 1 | 2 and leaves its next offsets running past the capacity, unclamped; the third call finds
    its start beyond the capacity, sets 4, repeats the offsets and writes nothing.  tests/detections_ref.emit_store restates the rule."""
    rng = np.random.default_rng(10)
    calls = [batch([dr.make_case(rng, 70, HW3[k], kept="all", ties=1) for k in range(B)]) for B in (3, 3, 1)]
    cap = 6 * 70 - 1
    ref = dr.emit_store(calls, 0.5, ca.MAX_DETS, wire_cap=cap, eval_cap=cap)
    assert ref["placed"] == [(70 * n, 70 * n) for n in range(5)] + [None, None] and ref["status"] == 7
    assert ref["wire_off"].tolist() == ref["eval_off"].tolist() == [0, 70, 140, 210, 280, 350, 420, 420] and ref["wire_off"][6] == cap + 1
    s = guarded_store(7, 70, cap, cap)
    first, words = 0, []
    for c in calls:
        ops.emit_detections(T(c[0]), T(c[1]), T(c[2]), T(c[3]), s, first)
        first += len(c[0])
        words.append(int(s.status[0]))
    print("status after each call", words)
    assert words == [0, 3, 7]
    for k, t in s.full.items():
        assert (t[s.size[k]:].cpu() == -777).all(), f"guard words behind {k} changed"
    assert s.counts.tolist() == ref["counts"].tolist() == [70] * 7
    assert s.wire_off.tolist() == ref["wire_off"].tolist() and s.eval_off.tolist() == ref["eval_off"].tolist()
    wire, n = s.wire.cpu().numpy(), 350
    assert np.array_equal(wire[:n, :7], ref["wire"]) and np.array_equal(wire[:n, 7].view(np.float32), ref["score"]) and len(ref["wire"]) == n
    for k in ("eval_boxes", "eval_area", "eval_score"):
        assert np.array_equal(getattr(s, k)[:n].cpu().numpy(), ref[k]), k
        assert (getattr(s, k)[n:].cpu() == -777).all(), k
    assert (s.wire[n:].cpu() == -777).all()


def _same(a, b):
    return set(a) == set(b) and all(a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])) for k in a)


def test_infer_end_to_end_on_the_tiny_set(tmp_path):
    """infer.infer on tests/golden/fsc147_tiny (val, instances_val.json) with the flag off and on: equal predictions_val.json bytes, equal metric
    dicts (losses included), the store path's six AP numbers equal to ap_from_json(device=) on the file, and a fixed number of Tensor.cpu calls.
    The class head's bias is shifted to the first image's median logit so that some of its queries are kept and some are not.  The seeded model's boxes are not
    trained: AP50 > 0 is asserted only if the host path itself finds a match (printed); the equality of the six numbers holds either way.  All
    ground truths of the set are small, so AP / AP50 / AP75 / APs are the defined numbers (asserted non-NaN) and APm / APl are NaN on every path."""
    from torch.utils.data import DataLoader
    import infer as infer_mod
    from counting_detr_amd import build_model, data
    from counting_detr_amd.args import default_args
    from counting_detr_amd.misc import NestedTensor
    from oracle.weights import seeded_state_dict
    args = default_args()
    args.data_path, args.scale_factor = os.path.join(HERE, "golden", "fsc147_tiny"), 32
    model, criterion, _ = build_model(args)
    model.load_state_dict(seeded_state_dict(), strict=True)
    model.to(DEV); criterion.to(DEV)
    model.eval()
    vl = DataLoader(data.build_test_dataset(args, "val"), batch_size=1, shuffle=False, collate_fn=data.collate)
    with torch.no_grad():
        logit = torch.cat([model(NestedTensor(b["image"].to(DEV), b["mask"].to(DEV)), rects=b["ex_rects"].to(DEV))[0]["pred_logits"][0, :, 0] for b in vl])
        for ce in {id(m): m for m in model.transformer.cls_embed}.values():
            ce.bias[0] -= logit[:logit.numel() // 2].median()                # the first image's median: about half of ITS queries are kept
    gt_json = os.path.join(args.data_path, "instances_val.json")
    out = {}
    calls = []
    real_cpu = torch.Tensor.cpu

    def counted(self, *a, **kw):
        calls.append(1)
        return real_cpu(self, *a, **kw)
    for name, flag in (("host", False), ("device", True)):
        os.makedirs(tmp_path / name)
        if flag:
            torch.Tensor.cpu = counted
        try:
            out[name] = infer_mod.infer(model, criterion, vl, torch.device(DEV), str(tmp_path / name), split="val", device_detections=flag,
                                        gt_json=gt_json if flag else None)
        finally:
            torch.Tensor.cpu = real_cpu
    n_cpu = len(calls)
    host_bytes, dev_bytes = (open(tmp_path / n / "predictions_val.json", "rb").read() for n in ("host", "device"))
    pj = json.loads(host_bytes)
    per_image = [sum(1 for a in pj["annotations"] if a["image_id"] == im["id"]) for im in pj["images"]]
    Q = logit.numel() // len(per_image)
    print("kept per image", per_image, "of", Q, "Tensor.cpu calls", n_cpu)
    assert len(per_image) == 2 and 0 < per_image[0] < Q
    assert host_bytes == dev_bytes
    assert out["host"][1] == out["device"][1]                                 # the returned predictions dict too
    ap_keys = ("AP", "AP50", "AP75", "APs", "APm", "APl")
    m_host, m_dev = dict(out["host"][0]), dict(out["device"][0])
    ap_store = {k: m_dev.pop(k) for k in ap_keys}
    print("host", m_host, "device", m_dev)
    assert m_host == m_dev and "loss_ce" in m_host and m_host["images"] == 2
    ap_file = ca.ap_from_json(str(tmp_path / "host" / "predictions_val.json"), gt_json, device=DEV)
    ap_host = ca.ap_from_json(str(tmp_path / "host" / "predictions_val.json"), gt_json)
    print("AP from the file", ap_file, "from the store", ap_store)
    assert _same(ap_file, ap_store) and _same(ap_host, ap_store)
    for k in ("AP", "AP50", "AP75", "APs"):                                   # every ground truth of the tiny set is small: APm / APl are NaN by definition
        assert not np.isnan(ap_file[k]) and not np.isnan(ap_store[k]), k
    assert np.isnan(ap_host["APm"]) and np.isnan(ap_host["APl"])
    if ap_host["AP50"] > 0:
        assert ap_store["AP50"] > 0
    # the copies do not grow with the images: the same loader twice over gives the same number of Tensor.cpu calls
    calls.clear()
    torch.Tensor.cpu = counted
    try:
        twice = [b for b in vl] + [dict(b, image_id=b["image_id"] + 1000) for b in vl]
        m4, p4 = infer_mod.infer(model, criterion, twice, torch.device(DEV), str(tmp_path / "device"), split="val", device_detections=True, gt_json=gt_json)
    finally:
        torch.Tensor.cpu = real_cpu
    assert m4["images"] == 4 and len(p4["images"]) == 4 and len(calls) == n_cpu == 4
    assert p4["annotations"][:len(pj["annotations"])] == pj["annotations"]


def test_infer_cli_with_the_flag_and_with_ap_on_host(tmp_path, capsys):
    """infer.py --device_detections on the tiny set: the emit call runs once per image and the AP is matched from the store by ONE
    cdetr_coco_match launch; with --ap_on_host beside it the written file goes through the interpreted ap_from_json instead (no launch) and
    prints the same numbers; both write the same predictions json.  The second run also takes its batches from the device-side image preparation
    (a data.Prefetcher whose sizes and ids are device tensors; the same image tensors bit for bit, tests/test_image_prep_gpu.py)."""
    import infer as infer_mod
    from counting_detr_amd.args import get_args_parser
    from oracle.weights import seeded_state_dict
    ckpt = tmp_path / "seeded.pth"
    torch.save({"model": seeded_state_dict()}, ckpt)
    calls = {"emit": 0, "match": 0}
    real_emit, real_match = ops.emit_detections, ops.coco_match

    def emit(*a, **kw):
        calls["emit"] += 1
        return real_emit(*a, **kw)

    def match(*a, **kw):
        calls["match"] += 1
        return real_match(*a, **kw)
    out = {}
    try:
        ops.emit_detections, ops.coco_match = emit, match
        for name, extra, want in (("store", [], {"emit": 2, "match": 1}), ("file", ["--ap_on_host", "--device_preprocess"], {"emit": 4, "match": 1})):
            args = get_args_parser().parse_args(["-dp", os.path.join(HERE, "golden", "fsc147_tiny"), "-o", str(tmp_path / name), "--split", "val",
                                                 "--resume", str(ckpt), "--no_aux_loss", "--num_query_pattern", "1", "--num_workers", "0",
                                                 "--device", DEV, "--device_detections"] + extra)
            capsys.readouterr()
            infer_mod.main(args)
            out[name] = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
            assert calls == want, (name, calls)
    finally:
        ops.emit_detections, ops.coco_match = real_emit, real_match
    print(out)
    assert out["store"]["images"] == 2 and set(out["store"]) == set(out["file"])
    assert all(out["store"][k] == out["file"][k] or (np.isnan(out["store"][k]) and np.isnan(out["file"][k])) for k in out["store"])
    assert all(k in out["store"] for k in ("AP", "AP50", "AP75", "APs", "APm", "APl", "MAE", "loss_ce"))
    assert open(tmp_path / "store" / "predictions_val.json", "rb").read() == open(tmp_path / "file" / "predictions_val.json", "rb").read()
