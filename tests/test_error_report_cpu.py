"""The error breakdown without a GPU (counting_detr_amd/error_report.py, coco_ap.Matching.errors on host flags, infer.py --error_report's
parser side, the C-ABI entry of csrc/error_report.hip): the numpy rule against the serial restatement of tests/error_report_ref.py on the
seeded families of tests/coco_ap_cases.py, hand-derived cases, the identities that tie the breakdown to the evaluation's own counts, and the
prefix property the sweep route rests on.  Every comparison is ==; IoUs are compared as float64 bits."""
import math
import os

import numpy as np
import pytest

from counting_detr_amd import coco_ap as ca
from counting_detr_amd import error_report as er

import coco_ap_cases as cc
import error_report_ref as ref


def _plus(family, seed):
    """A family of tests/coco_ap_cases.py plus an image without ground truth and one without detections."""
    gts, dts = family()
    rng = np.random.default_rng(seed)
    gts[900], dts[900] = [], cc.float_image(rng, 0, 7, extent=400.0)[1]
    gts[901], dts[901] = cc.float_image(rng, 6, 0, extent=400.0)[0], []
    return gts, dts


@pytest.fixture(scope="module", params=["tie", "float"])
def family(request):
    gts, dts = _plus(cc.tie_family if request.param == "tie" else cc.float_family, 5)
    matching = ca.Matching.of(gts, dts)
    return gts, dts, matching, matching.errors()


def test_constants():
    assert er.IOU_FG == 0.5 == min(ca.IOU_THRS[0], 1 - 1e-10) and er.IOU_BG == 0.1
    assert er.COUNT_KEYS == ("tp", "ign_dt", "dup", "loc", "bkg", "hit", "ign_gt", "misloc", "missed")


# ------------------------------------------------------------------------------------------------------------ the module against the loops
def test_module_equals_the_serial_restatement(family):
    gts, dts, matching, codes = family
    ref.same(codes, ref.classify(gts, dts))
    ref.same(er.classify(matching.pack), codes)
    assert codes["dt_code"].dtype == np.uint8 and codes["dt_gt"].dtype == np.int32 and codes["counts"].shape == (len(matching.pack["image_ids"]), 9)


def test_every_code_occurs_in_the_family(family):
    codes = family[3]
    assert set(np.unique(codes["dt_code"]).tolist()) == {0, 1, 2, 3, 4}, np.unique(codes["dt_code"], return_counts=True)
    assert set(np.unique(codes["gt_code"]).tolist()) == {0, 1, 2, 3}, np.unique(codes["gt_code"], return_counts=True)
    assert (codes["counts"].sum(axis=0) > 0).all()


def test_another_background_bar_moves_loc_and_bkg_only(family):
    gts, dts, matching, codes = family
    wide = matching.errors(iou_bg=0.3)
    ref.same(wide, ref.classify(gts, dts, iou_bg=0.3))
    c0, c1 = codes["counts"].sum(axis=0), wide["counts"].sum(axis=0)
    assert c1[3] < c0[3] and c1[3] + c1[4] == c0[3] + c0[4] and np.array_equal(c0[[0, 1, 2, 5, 6]], c1[[0, 1, 2, 5, 6]]) and c1[8] >= c0[8]


# ------------------------------------------------------------------------------------------------------------------------------ identities
def test_identities_against_the_matchings_own_counts(family):
    gts, dts, matching, codes = family
    stats = matching.stats()
    a, t, last = list(ca.AREA_RNG).index("all"), 0, len(stats["cuts"]) - 1
    assert stats["cuts"][last] == 1100 and ca.IOU_THRS[t] == 0.5
    c = codes["counts"]
    tp50, fp50 = stats["tp"][a, :, t, last], stats["fp"][a, :, t, last]
    fn50 = stats["npig"][a] - tp50
    assert np.array_equal(c[:, 0], tp50) and np.array_equal(c[:, 2] + c[:, 3] + c[:, 4], fp50) and np.array_equal(c[:, 7] + c[:, 8], fn50)
    assert np.array_equal(c[:, 0], c[:, 5])
    matched, ignored, _ = matching.host()
    assert np.array_equal(codes["dt_code"] == er.TP, matched[a, t] & ~ignored[a, t]) and np.array_equal(codes["dt_code"] == er.IGN, ignored[a, t])
    dap = er.what_if(matching.pack, codes)
    assert dap["AP50_base"] == matching.six()["AP50"]
    assert list(dap) == ["AP50_base", "dAP50_dup", "dAP50_loc", "dAP50_bkg", "dAP50_missed"]
    assert all(dap[k] >= 0 for k in er.DAP_KEYS) and dap["dAP50_missed"] > 0          # ignoring false positives / dropping misses never lowers AP
    # a DUP detection's best ground truth is taken
    pack = matching.pack
    for b in range(len(pack["image_ids"])):
        dseg, gseg = slice(pack["dt_off"][b], pack["dt_off"][b + 1]), slice(pack["gt_off"][b], pack["gt_off"][b + 1])
        dup = codes["dt_code"][dseg] == er.DUP
        assert (codes["dt_gt"][dseg][dup] >= 0).all() and (codes["gt_code"][gseg][codes["dt_gt"][dseg][dup]] == er.HIT).all()
        assert (codes["dt_iou"][dseg][dup] >= 0.5).all()
        loc = codes["dt_code"][dseg] == er.LOC
        assert ((codes["dt_iou"][dseg][loc] >= 0.1) & (codes["dt_iou"][dseg][loc] < 0.5)).all()


def test_prefix_lengths_equal_truncated_lists(family):
    """`classify(counts=c)` is the classification of every image's first c detections: the greedy match never looks ahead."""
    gts, dts, matching, full = family
    pack = matching.pack
    lens = np.diff(pack["dt_off"]).tolist()
    rng = np.random.default_rng(13)
    counts = [0, lens[1], lens[2] + 5] + [int(rng.integers(1, n)) if n > 1 else n for n in lens[3:]]
    assert all(gts.get(i) or min(c, n) for i, c, n in zip(pack["image_ids"], counts, lens))          # no image drops out of the pack
    got = matching.errors(counts)
    by_score = lambda d: [d[j] for j in np.argsort([-x["score"] for x in d], kind="mergesort")]        # noqa: E731
    cut = {i: by_score(dts.get(i, []))[:c] for i, c in zip(pack["image_ids"], counts)}
    want = ca.Matching.of(gts, cut).errors()
    assert want["counts"].shape == got["counts"].shape
    assert np.array_equal(got["counts"], want["counts"]) and not np.array_equal(got["counts"], full["counts"])
    for k in ("gt_code", "gt_dt", "gt_iou"):
        assert np.array_equal(got[k].view(np.int64) if k == "gt_iou" else got[k], want[k].view(np.int64) if k == "gt_iou" else want[k]), k
    used = got["dt_code"] != er.UNUSED
    assert int(used.sum()) == sum(min(c, n) for c, n in zip(counts, lens)) == len(want["dt_code"])
    assert np.array_equal(got["dt_code"][used], want["dt_code"]) and np.array_equal(got["dt_gt"][used], want["dt_gt"])
    assert np.array_equal(got["dt_iou"][used].view(np.int64), want["dt_iou"].view(np.int64))
    assert (got["dt_gt"][~used] == -1).all() and (got["dt_iou"][~used] == 0.0).all()
    ref.same(got, ref.classify(gts, dts, counts=counts))
    # the what-if numbers of the prefix are those of the truncated lists
    a, b = er.what_if(pack, got), er.what_if(ca.pack_images(gts, cut), want)
    assert all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a)


# ----------------------------------------------------------------------------------------------------------------------- hand-derived cases
def _one(gts, dts, **kw):
    m = ca.Matching.of({1: gts}, {1: dts})
    codes = m.errors(**kw)
    ref.same(codes, ref.classify({1: gts}, {1: dts}, **kw))
    return m, codes


def test_ious_exactly_on_the_two_bars():
    """[0,0,1,1] against [0,0,2,1] and [0,0,10,1]: IoU exactly 0.5 and exactly 0.1 -- `>=` makes the first TP and the second LOC, not BKG."""
    _, c = _one([cc.gt([0, 0, 1, 1])], [cc.dt([0, 0, 2, 1], 0.9), cc.dt([0, 0, 10, 1], 0.8)])
    assert c["dt_iou"].tolist() == [0.5, 0.1] and c["dt_code"].tolist() == [er.TP, er.LOC] and c["dt_gt"].tolist() == [0, 0]
    assert c["gt_code"].tolist() == [er.HIT] and c["gt_dt"].tolist() == [0] and c["gt_iou"].tolist() == [0.5]
    assert c["counts"].tolist() == [[1, 0, 0, 1, 0, 1, 0, 0, 0]]
    # without the first detection the ground truth is mislocalised
    _, c = _one([cc.gt([0, 0, 1, 1])], [cc.dt([0, 0, 10, 1], 0.8), cc.dt([5, 5, 1, 1], 0.7)])
    assert c["dt_code"].tolist() == [er.LOC, er.BKG] and c["dt_gt"].tolist() == [0, -1] and c["dt_iou"].tolist() == [0.1, 0.0]
    assert c["gt_code"].tolist() == [er.MISLOC] and c["gt_dt"].tolist() == [0] and c["counts"].tolist() == [[0, 0, 0, 1, 1, 0, 0, 1, 0]]


def test_two_identical_detections_on_one_ground_truth():
    m, c = _one([cc.gt([10, 10, 20, 20]), cc.gt([100, 100, 40, 40])],
                [cc.dt([10, 10, 20, 20], 0.9), cc.dt([10, 10, 20, 20], 0.8), cc.dt([100, 100, 40, 40], 0.7)])
    assert c["dt_code"].tolist() == [er.TP, er.DUP, er.TP] and c["dt_gt"].tolist() == [0, 0, 1] and c["dt_iou"].tolist() == [1.0, 1.0, 1.0]
    assert c["gt_code"].tolist() == [er.HIT, er.HIT] and c["gt_dt"].tolist() == [0, 2] and c["counts"].tolist() == [[2, 0, 1, 0, 0, 2, 0, 0, 0]]
    dap = er.what_if(m.pack, c)
    # tp, fp, tp: precision 1, 1/2, 2/3 -> envelope 1, 2/3, 2/3; recall 1/2, 1/2, 1: 51 samples at 1, 50 at 2/3; without the duplicate 100
    assert dap["AP50_base"] == pytest.approx(100 * (51 + 50 * 2 / 3) / 101, abs=1e-9) and dap["AP50_base"] + dap["dAP50_dup"] == pytest.approx(100.0, abs=1e-9)
    assert dap["dAP50_loc"] == dap["dAP50_bkg"] == dap["dAP50_missed"] == 0.0


def test_a_detection_on_a_crowd_ground_truth_is_ignored():
    _, c = _one([cc.gt([10, 10, 20, 20], iscrowd=1), cc.gt([100, 100, 40, 40])], [cc.dt([10, 10, 20, 20], 0.9), cc.dt([12, 10, 20, 20], 0.5)])
    assert c["dt_code"].tolist() == [er.IGN, er.BKG] and c["dt_gt"].tolist() == [0, -1] and c["dt_iou"].tolist() == [1.0, 0.0]
    assert c["gt_code"].tolist() == [er.GT_IGN, er.MISSED] and c["gt_dt"].tolist() == [0, -1] and c["gt_iou"][0] == 1.0
    assert c["counts"].tolist() == [[0, 1, 0, 0, 1, 0, 1, 0, 1]]


def test_only_ignored_ground_truths():
    m, c = _one([cc.gt([10, 10, 20, 20], iscrowd=1), cc.gt([50, 50, 20, 20], ignore=1)], [cc.dt([300, 300, 5, 5], 0.9), cc.dt([50, 50, 20, 20], 0.5)])
    assert c["dt_code"].tolist() == [er.BKG, er.IGN] and c["gt_code"].tolist() == [er.GT_IGN, er.GT_IGN]
    assert c["counts"].tolist() == [[0, 1, 0, 0, 1, 0, 2, 0, 0]]
    assert all(math.isnan(v) for v in er.what_if(m.pack, c).values())                      # no non-ignored ground truth: no AP


def test_no_ground_truth_and_no_detection():
    m, c = _one([], [cc.dt([1, 1, 5, 5], 0.9), cc.dt([2, 2, 5, 5], 0.8)])
    assert c["dt_code"].tolist() == [er.BKG, er.BKG] and c["dt_gt"].tolist() == [-1, -1] and len(c["gt_code"]) == 0
    assert c["counts"].tolist() == [[0, 0, 0, 0, 2, 0, 0, 0, 0]]
    m, c = _one([cc.gt([1, 1, 5, 5]), cc.gt([20, 20, 5, 5])], [])
    assert len(c["dt_code"]) == 0 and c["gt_code"].tolist() == [er.MISSED, er.MISSED] and c["gt_dt"].tolist() == [-1, -1]
    assert c["gt_iou"].tolist() == [0.0, 0.0] and c["counts"].tolist() == [[0, 0, 0, 0, 0, 0, 0, 0, 2]]
    dap = er.what_if(m.pack, c)
    assert dap["AP50_base"] == 0.0 and math.isnan(dap["dAP50_missed"])                     # every ground truth missed: nothing is left
    empty = ca.Matching.of({}, {}).errors()
    assert empty["counts"].shape == (0, 9) and len(empty["dt_code"]) == 0 and len(empty["gt_iou"]) == 0


def test_the_first_loc_detection_of_a_misloc_ground_truth_becomes_the_true_positive():
    """Two LOC detections on one ground truth (IoU 1/3 and 1/4) and a true positive elsewhere: fixing localisation turns the first into a
    true positive and drops the second, AP50 goes to 100."""
    g = [cc.gt([0, 0, 16, 16]), cc.gt([100, 100, 16, 16])]
    d = [cc.dt([100, 100, 16, 16], 0.9), cc.dt([8, 0, 16, 16], 0.8), cc.dt([0, 0, 16, 64], 0.7)]
    m, c = _one(g, d)
    assert c["dt_code"].tolist() == [er.TP, er.LOC, er.LOC] and c["dt_gt"].tolist() == [1, 0, 0] and c["dt_iou"].tolist() == [1.0, 8 * 16 / (2 * 256 - 128), 0.25]
    assert c["gt_code"].tolist() == [er.MISLOC, er.HIT] and c["gt_dt"].tolist() == [1, 0]
    dap = er.what_if(m.pack, c)
    assert dap["AP50_base"] + dap["dAP50_loc"] == pytest.approx(100.0, abs=1e-9) and dap["AP50_base"] == pytest.approx(100 * 51 / 101, abs=1e-9)


# ------------------------------------------------------------------------------------------------------------------------------ the report
def test_report_rows_totals_and_orders(family):
    gts, dts, matching, codes = family
    run = list(reversed(matching.pack["image_ids"])) + [77]                                 # run order; 77: an image with nothing on it
    rep = er.report(matching.pack, codes, run, "val", 0.5)
    assert list(rep) == ["split", "threshold", "iou_fg", "iou_bg", "max_dets", "totals", "dAP50", "rows", "order_by_dup", "order_by_loc",
                         "order_by_bkg", "order_by_missed"]
    assert (rep["split"], rep["threshold"], rep["iou_fg"], rep["iou_bg"], rep["max_dets"]) == ("val", 0.5, 0.5, 0.1, 1100)
    assert [r["image_id"] for r in rep["rows"]] == run and all(list(r) == ["image_id", *er.COUNT_KEYS, "mean_iou_tp", "mean_iou_loc"] for r in rep["rows"])
    assert [rep["totals"][k] for k in er.COUNT_KEYS] == codes["counts"].sum(axis=0).tolist()
    assert rep["rows"][-1]["tp"] == 0 and math.isnan(rep["rows"][-1]["mean_iou_tp"])
    by = {r["image_id"]: r for r in rep["rows"]}
    for k in ("dup", "loc", "bkg", "missed"):
        order = rep["order_by_" + k]
        vals = [by[i][k] for i in order]
        assert sorted(order) == sorted(run) and vals == sorted(vals, reverse=True)
        assert all(run.index(a) < run.index(b) for a, b in zip(order, order[1:]) if by[a][k] == by[b][k])       # ties in run order
    assert all(0.5 <= r["mean_iou_tp"] <= 1 for r in rep["rows"] if r["tp"]) and all(0.1 <= r["mean_iou_loc"] < 0.5 for r in rep["rows"] if r["loc"])
    met = er.metrics(rep)
    assert list(met) == list(er.ERR_KEYS) + list(er.DAP_KEYS) and met["err_misloc"] == rep["totals"]["misloc"] and met["dAP50_bkg"] == rep["dAP50"]["dAP50_bkg"]
    # main.py --eval_every: behind the existing test_* keys of the epoch's log line
    from counting_detr_amd.checkpoint import epoch_log_line
    line = epoch_log_line({"loss": 1.0}, {"MAE": 2.0, "AP50": 3.0, **met}, 4)
    assert list(line) == ["train_loss", "test_MAE", "test_AP50", *("test_" + k for k in met), "epoch"] and line["test_err_dup"] == rep["totals"]["dup"]


# ------------------------------------------------------------------------------------------------------------------------------ the parser
def test_parser_leaves_no_attribute_and_a_missing_instances_json_raises(tmp_path):
    import infer as infer_mod
    from counting_detr_amd.args import get_args_parser
    p = get_args_parser()
    assert not hasattr(p.parse_args([]), "error_report") and not hasattr(p.parse_args(["--image_report"]), "error_report")
    a = p.parse_args(["--error_report", "-dp", str(tmp_path), "--split", "val"])
    assert a.error_report is True and not hasattr(a, "image_report")                      # it does not need the image report
    assert infer_mod.build_error_report(p.parse_args(["-dp", str(tmp_path)])) is None
    with pytest.raises(FileNotFoundError, match="instances_val.json"):
        infer_mod.build_error_report(a)
    (tmp_path / "instances_val.json").write_text("{}")
    rep = infer_mod.build_error_report(a)
    assert rep.gt_json == os.path.join(str(tmp_path), "instances_val.json") and rep.device is None and rep.report is None


# --------------------------------------------------------------------------------------------------------------------------- header / _ffi
def test_entry_is_declared_exported_and_refuses_bad_arguments_before_any_launch():
    from counting_detr_amd import _ffi, build
    build.build_lib(verbose=False)
    assert "error_report.hip" in build.SOURCES
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cdetr_hip.h")).read()
    assert "int cdetr_coco_errors(" in src and "cdetr_coco_errors" in _ffi.EXPORTS
    L = _ffi.lib()
    call = lambda B, G, D, Gmax, fg=0.5: L.cdetr_coco_errors(None, None, None, None, None, None, None, None, B, G, D, Gmax, fg, 0.1, 0.0, 1e10,      # noqa: E731
                                                             None, None, None, None, None, None, None, None)
    assert call(-1, 0, 0, 0) == -1 and b"cdetr_coco_errors" in L.cdetr_last_error()
    assert call(1, 0, 0, 0, float("nan")) == -1 and b"cdetr_coco_errors" in L.cdetr_last_error()
    assert call(1, 0, 0, 4097) == -3 and b"4097" in L.cdetr_last_error()
    assert call(1, 0, 0, 4096) == -1 and b"null" in L.cdetr_last_error()                   # inside the limit: the null pointers are what is wrong
    assert call(0, 0, 0, 0) == 0                                                           # no image: nothing to do
