"""cdetr_emit_pseudo_labels (csrc/stage1_labels.hip) behind ops.PseudoLabelStore, coco_ap.summarize_store and main_stage1.py --device_labels /
--score_labels / --test, against the numpy restatement tests/stage1_labels_ref.py (pinned to the host loop by tests/test_stage1_labels_cpu.py)
and against the host path itself: everything EQUAL, no tolerance anywhere.
  (a) the kernel: ragged counts over two calls into one store (an image without rows, one row, more than two waves, one row past a
      workgroup), a dense call, original sizes up to 3000 x 2000, the hand-made truncation rows;
  (b) the max_det cut; (c) a store one record short: status word, nothing out of bounds;
  (d) main_stage1.py on the tiny fixture: the same bytes and EQUAL scores with and without --device_labels.
Needs an MI355X."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import stage1_labels_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
TINY = os.path.join(HERE, "golden", "fsc147_tiny")
ROWS_PER_WG = 256                      # PL_ROWS of csrc/stage1_labels.hip
R = ROWS_PER_WG + 1                    # one row past a workgroup; > 130: more than two waves
SIZES = [(3000, 2000), (384, 576), (101, 70)]


def dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def emit(store, batch, first=None):
    points, pred_wh, counts, orig_wh, gt = batch
    args = (dev(points), dev(pred_wh), dev(counts, torch.int32), dev(orig_wh, torch.int32))
    if first is None:
        return store.emit(*args, gt_xywh=dev(gt))
    from counting_detr_amd import ops
    return ops.emit_pseudo_labels(*args, store, first, gt_xywh=dev(gt))


def assert_store_equals(store, want):
    host = store.finish()
    for k in ("counts", "row_off", "eval_off", "wire", "eval_score"):
        assert host[k].dtype == want[k].dtype and np.array_equal(host[k], want[k]), k
    assert host["pair_iou"].dtype == np.float64 and host["pair_iou"].tobytes() == want["pair_iou"].tobytes()       # bit-equal
    E = int(want["eval_off"][-1])
    assert torch.equal(store.eval_boxes[:E].cpu(), torch.from_numpy(want["eval_boxes"]))
    assert torch.equal(store.eval_area[:E].cpu(), torch.from_numpy(want["eval_area"]))


@pytest.fixture(scope="module")
def two_calls():
    rng = np.random.default_rng(11)
    a = ref.make_batch(rng, 3, R, SIZES)
    b = ref.make_batch(rng, 3, R, SIZES[::-1], hand=False)
    return ((a[0], a[1], np.array([R, 1, 57], dtype=np.int32), a[2], a[3]),
            (b[0], b[1], np.array([0, 5, R], dtype=np.int32), b[2], b[3]))


def test_kernel_equals_the_restatement_over_two_calls(two_calls):
    from counting_detr_amd import ops
    want = ref.emit_store(two_calls, 1100)
    rows = int(want["row_off"][-1])
    assert rows == 2 * R + 1 + 57 + 5 and want["counts"].tolist() == [R, 1, 57, 0, 5, R]
    store = ops.PseudoLabelStore(6, rows, DEV)                          # exactly full after the second call
    assert emit(store, two_calls[0]) == 0 and emit(store, two_calls[1]) == 3 and store.first == 6
    assert_store_equals(store, want)
    host = store.finish()
    assert host["row_off"][3] == host["row_off"][4] and host["eval_off"][3] == host["eval_off"][4]              # the image without rows
    assert host is store.finish()                                                                               # cached: one copy
    iou = host["pair_iou"]
    assert iou.max() > 0.5 and (iou == 0.0).any() and ((iou > 0) & (iou < 0.5)).any()


def test_after_the_first_call_alone(two_calls):
    from counting_detr_amd import ops
    store = ops.PseudoLabelStore(6, 2 * R + 63, DEV)
    emit(store, two_calls[0])
    assert_store_equals(store, ref.emit_store(two_calls[:1], 1100))


def test_without_ground_truth_the_pairs_are_zero(two_calls):
    from counting_detr_amd import ops
    batch = two_calls[0][:4] + (None,)
    store = ops.PseudoLabelStore(3, R + 58, DEV)
    emit(store, batch)
    assert_store_equals(store, ref.emit_store([batch], 1100))
    assert not store.finish()["pair_iou"].any()


def test_dense_call_equals_counts_all_rows(two_calls):
    from counting_detr_amd import ops
    points, pred_wh, _, orig_wh, gt = two_calls[0]
    dense, full = ops.PseudoLabelStore(3, 3 * R, DEV), ops.PseudoLabelStore(3, 3 * R, DEV)
    emit(dense, (points, pred_wh, None, orig_wh, gt))
    emit(full, (points, pred_wh, np.full(3, R, dtype=np.int32), orig_wh, gt))
    assert_store_equals(dense, ref.emit_store([(points, pred_wh, None, orig_wh, gt)], 1100))
    a, b = dense.finish(), full.finish()
    assert all(np.array_equal(a[k], b[k]) for k in a) and torch.equal(dense.eval_boxes, full.eval_boxes) and torch.equal(dense.eval_area, full.eval_area)


def test_max_det_cuts_the_evaluation_records_only():
    from counting_detr_amd import ops
    rng = np.random.default_rng(12)
    points, pred_wh, orig_wh, gt = ref.make_batch(rng, 2, 7, SIZES, hand=False)
    batch = (points, pred_wh, np.array([7, 3], dtype=np.int32), orig_wh, gt)
    want = ref.emit_store([batch], 4)
    store = ops.PseudoLabelStore(2, 10, DEV, max_det=4)
    assert store.eval_cap == 8
    emit(store, batch)
    assert_store_equals(store, want)
    host = store.finish()
    assert host["eval_off"].tolist() == [0, 4, 7] and host["row_off"].tolist() == [0, 7, 10] and len(host["wire"]) == 10
    every = ref.emit_store([batch], 1100)                                # rows 0..3 of image 0 and 0..2 of image 1
    assert np.array_equal(want["eval_boxes"], np.concatenate([every["eval_boxes"][0:4], every["eval_boxes"][7:10]]))


GUARD = 8


def guarded_store(N, row_cap, eval_cap, max_det=1100):
    """A store whose arrays are separate allocations with GUARD sentinel elements behind each."""
    mk = lambda n, dt: torch.full((n + GUARD,), -777, dtype=dt, device=DEV)                                  # noqa: E731
    full = {"status": mk(1, torch.int32), "counts": mk(N, torch.int32), "row_off": mk(N + 1, torch.int32), "eval_off": mk(N + 1, torch.int32),
            "wire": mk(8 * row_cap, torch.int32), "pair_iou": mk(row_cap, torch.float64), "eval_boxes": mk(4 * eval_cap, torch.float64),
            "eval_area": mk(eval_cap, torch.float64), "eval_score": mk(eval_cap, torch.float64)}
    size = {"status": 1, "counts": N, "row_off": N + 1, "eval_off": N + 1, "wire": 8 * row_cap, "pair_iou": row_cap, "eval_boxes": 4 * eval_cap,
            "eval_area": eval_cap, "eval_score": eval_cap}
    full["status"][0] = full["row_off"][0] = full["eval_off"][0] = 0
    s = SimpleNamespace(N=N, row_cap=row_cap, eval_cap=eval_cap, max_det=max_det, buf=full["status"], full=full, size=size)
    for k, t in full.items():
        setattr(s, k, t[:size[k]])
    s.wire, s.eval_boxes = s.wire.view(-1, 8), s.eval_boxes.view(-1, 4)
    return s


def test_a_store_one_record_short_sets_the_status_word_and_stays_in_bounds(two_calls):
    from counting_detr_amd import ops
    want = ref.emit_store(two_calls, 1100)
    rows = int(want["row_off"][-1])
    s = guarded_store(6, rows - 1, rows - 1)
    emit(s, two_calls[0], first=0)
    emit(s, two_calls[1], first=3)
    torch.cuda.synchronize()
    for k, t in s.full.items():
        assert (t[s.size[k]:].cpu() == -777).all(), f"guard words behind {k} changed"
    assert int(s.status[0]) == 3                                         # the last image fits neither the wire nor the evaluation records
    fit = int(want["row_off"][5])                                        # everything before the last image is in place
    assert np.array_equal(s.row_off.cpu().numpy()[:6], want["row_off"][:6]) and int(s.row_off[6]) == rows - 1
    assert np.array_equal(s.wire[:fit, :6].cpu().numpy(), want["wire"][:fit])
    assert s.pair_iou[:fit].cpu().numpy().tobytes() == want["pair_iou"][:fit].tobytes()
    assert (s.wire[fit:].cpu() == -777).all() and (s.pair_iou[fit:].cpu() == -777).all() and (s.eval_boxes[fit:].cpu() == -777).all()

    short = ops.PseudoLabelStore(6, rows - 1, DEV)
    emit(short, two_calls[0])
    emit(short, two_calls[1])
    with pytest.raises(RuntimeError, match="cdetr_emit_pseudo_labels reported status 3"):
        short.finish()


def test_a_count_beyond_the_rows_is_reported_not_followed():
    from counting_detr_amd import ops
    rng = np.random.default_rng(13)
    points, pred_wh, orig_wh, gt = ref.make_batch(rng, 2, 5, SIZES, hand=False)
    s = guarded_store(2, 16, 16)
    emit(s, (points, pred_wh, np.array([6, 2], dtype=np.int32), orig_wh, gt), first=0)
    torch.cuda.synchronize()
    assert int(s.status[0]) == 8 and s.row_off.tolist() == [0, 0, 2]
    want = ref.emit_store([(points[1:], pred_wh[1:], np.array([2], dtype=np.int32), orig_wh[1:], gt[1:])], 1100)
    assert np.array_equal(s.wire[:2, 1:6].cpu().numpy(), want["wire"][:, 1:]) and (s.wire[2:].cpu() == -777).all()


# ---- end to end on the tiny fixture: a seeded random-init stage-1 model ------------------------------------------------------------------
@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    from oracle.weights import seeded_state_dict, stage1_schema
    path = tmp_path_factory.mktemp("stage1_labels") / "init.pth"
    torch.save({"model": seeded_state_dict(stage1_schema())}, path)
    return str(path)


def run_main(out, checkpoint, *flags):
    import main_stage1
    from counting_detr_amd.args import get_args_parser_stage1
    os.makedirs(out, exist_ok=True)
    args = get_args_parser_stage1().parse_args(["--data_path", TINY, "--output_dir", str(out), "--num_workers", "0", "--device", DEV,
                                                "--dataset_file", "fscd_147_point", "--resume", checkpoint, *flags])
    main_stage1.main(args)
    return out


def load(path):
    with open(path) as f:
        return json.load(f)


@pytest.mark.parametrize("batching", [(), ("--ragged_batches", "--batch_size", "2")], ids=["batch1", "ragged2"])
def test_generate_and_score_labels_host_and_device_agree(tmp_path, checkpoint, batching, capsys):
    host = run_main(tmp_path / "host", checkpoint, "--generate_pseudo_label", "--score_labels", *batching)
    text = capsys.readouterr().out
    assert "pseudo_bbox_train.json: not scored" in text and "pseudo_scores_val.json:" in text
    devd = run_main(tmp_path / "dev", checkpoint, "--generate_pseudo_label", "--score_labels", "--device_labels", *batching)
    for split, images, boxes in (("train", 2, 13), ("val", 2, 14), ("test", 1, 9)):
        a, b = (host / f"pseudo_bbox_{split}.json").read_bytes(), (devd / f"pseudo_bbox_{split}.json").read_bytes()
        assert a == b, split
        ann = json.loads(a)
        assert len(ann["images"]) == images and len(ann["annotations"]) == boxes
    assert not (host / "pseudo_scores_train.json").exists() and not (devd / "pseudo_scores_train.json").exists()
    for split, images, boxes in (("val", 2, 14), ("test", 1, 9)):
        a, b = load(host / f"pseudo_scores_{split}.json"), load(devd / f"pseudo_scores_{split}.json")
        assert ref.same(a, b), (a, b)
        assert a["images"] == images and a["boxes"] == boxes and set(a) == {"AP", "AP50", "AP75", "APs", "APm", "APl", "images", "boxes"}
        assert 0.0 <= a["AP"] <= 100.0


@pytest.mark.parametrize("batching", [(), ("--ragged_batches", "--batch_size", "2")], ids=["batch1", "ragged2"])
def test_box_scores_host_and_device_agree(tmp_path, checkpoint, batching):
    host = run_main(tmp_path / "host", checkpoint, "--test", *batching)
    devd = run_main(tmp_path / "dev", checkpoint, "--test", "--device_labels", *batching)
    for split, images, pairs in (("val", 2, 14), ("test", 1, 9)):
        a, b = load(host / f"box_scores_{split}.json"), load(devd / f"box_scores_{split}.json")
        assert ref.same(a, b), (a, b)
        assert a["pairs"] == pairs and len(a["per_image_mean_iou"]) == images and 0.0 <= a["mean_iou"] <= 1.0
        assert set(a) == {"pairs", "mean_iou", "iou50", "iou75", "per_image_mean_iou", "AP", "AP50", "AP75", "APs", "APm", "APl"}
        assert (host / f"pseudo_bbox_gtpoints_{split}.json").read_bytes() == (devd / f"pseudo_bbox_gtpoints_{split}.json").read_bytes()
    assert not (host / "pseudo_bbox_val.json").exists()                 # --test writes no training labels


def test_store_scores_and_pair_ious_equal_the_host_checkers(tmp_path, checkpoint):
    """One device pass over val at the ground-truth centres: the store's paired IoUs are bit-equal to the diagonal of coco_ap.box_iou_xywh,
    summarize_store on the store equals coco_ap.summarize on the host dicts (host code and device=), ONE emit per batch and no host loop."""
    import main_stage1
    from counting_detr_amd import coco_ap, data, ops, stage1
    from counting_detr_amd.args import get_args_parser_stage1
    args = get_args_parser_stage1().parse_args(["--data_path", TINY, "--num_workers", "0", "--device", DEV, "--ragged_batches", "--batch_size", "2"])
    model, _, _ = stage1.build(args)
    model.load_state_dict(torch.load(checkpoint)["model"], strict=True)
    model.to(DEV)
    calls, real = [], ops.emit_pseudo_labels
    ops.emit_pseudo_labels = lambda *a, **k: (calls.append(a[0].shape[0]), real(*a, **k))[1]
    try:
        ann, store = stage1.write_pseudo_labels(model, main_stage1.loader_for(args, "val", points=True, device=DEV, boxes=True), "gt_val", str(tmp_path),
                                                device=DEV, device_labels=True, return_store=True)
    finally:
        ops.emit_pseudo_labels = real
    assert calls == [1, 1] and store.first == 2                          # two resized sizes: two batches of one image
    ds = data.FSC147BoxPointsDataset(args, "val")
    iou, off = stage1.host_pair_iou(ann, [ds[k]["gt_xywh"] for k in range(len(ds))])
    host = store.finish()
    assert host["pair_iou"].tobytes() == iou.tobytes() and np.array_equal(host["row_off"], off)
    gt_json = os.path.join(TINY, "instances_val.json")
    on_host = stage1.score_pseudo_labels(ann, gt_json)
    assert ref.same(stage1.score_pseudo_labels(ann, gt_json, store=store), on_host)
    assert ref.same(stage1.score_pseudo_labels(ann, gt_json, device=DEV), on_host)
    to_gt = stage1._gt_image_ids(ann, gt_json)
    gt_by = coco_ap.gt_from_json(gt_json, set(to_gt.values()))
    dt_by = {to_gt[i]: d for i, d in stage1.evaluator_boxes(ann).items()}
    assert ref.same(coco_ap.summarize_store(gt_by, store, [to_gt[im["id"]] for im in ann["images"]]), coco_ap.summarize(gt_by, dt_by))
    assert [im["file_name"] for im in ann["images"]] == ["3.jpg", "1.jpg"] and to_gt == {1: 3, 2: 1}
