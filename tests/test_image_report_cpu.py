"""The per-image evaluation report without a GPU (coco_ap.image_stats / stats_from_flags / average_recall / image_rows, infer.py
--image_report's parser side, the C-ABI entry of csrc/coco_report.hip): hand-derived cases, and the two facts the device launch rests on,
checked against coco_ap's host path -- the counts of the first `c` detections of ONE matching at 1100 are the counts of an evaluation at
max_det = c, and an image's own AP needs nothing but its own list."""
import math
import os

import numpy as np
import pytest

from counting_detr_amd import coco_ap as ca

import abi_header
import coco_ap_cases as cc

AREAS = list(ca.AREA_RNG)
ALL = AREAS.index("all")
CUTS = (50, 100, 1100)


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
    return gts, dts, ca.image_stats(gts, dts, cuts=CUTS)


# ----------------------------------------------------------------------------------------------------------------------- hand-derived cases
G2 = [cc.gt([10, 10, 20, 20]), cc.gt([100, 100, 40, 40])]


def _row(gts, dts, cuts=ca.MAX_DET_CUTS):
    st = ca.image_stats({1: gts}, {1: dts}, cuts=cuts)
    return st, ca.image_rows(st, {1: len(gts)}, {1: len(dts)})[0]


def test_two_exact_copies_scored_highest():
    st, row = _row(G2, [cc.dt([10, 10, 20, 20], 0.9), cc.dt([100, 100, 40, 40], 0.8), cc.dt([300, 300, 10, 10], 0.1)])
    assert all(row[k] == pytest.approx(100.0, abs=1e-9) for k in ("AP", "AP50", "AP75"))
    assert row["APs"] == pytest.approx(100.0, abs=1e-9) and row["APm"] == pytest.approx(100.0, abs=1e-9) and math.isnan(row["APl"])
    assert (row["tp50"], row["fp50"], row["fn50"]) == (2, 1, 0)
    assert (row["image_id"], row["count_gt"], row["count_pred"], row["diff"]) == (1, 2, 3, -1)
    assert st["tp"].shape == (4, 1, 10, 3) and st["ap"].shape == (4, 1, 10) and st["cuts"] == ca.MAX_DET_CUTS == (900, 1000, 1100)


def test_the_stray_detection_scored_highest():
    """Order: stray, copy, copy.  Precision 0, 1/2, 2/3 -> envelope 2/3 everywhere; recall 0, 1/2, 1: the sample at recall 0 takes index 0,
    all 101 samples are 2/3 (less the eps of the definition), AP50 = 100 * 2/3.  At a cut of 1 only the stray is left: fp 1, tp 0."""
    st, row = _row(G2, [cc.dt([300, 300, 10, 10], 0.95), cc.dt([10, 10, 20, 20], 0.9), cc.dt([100, 100, 40, 40], 0.8)], cuts=(1, 2, 1100))
    want = 2.0 / (1.0 + 2.0 + np.spacing(1))
    assert row["AP50"] == pytest.approx(100.0 * 2 / 3, abs=1e-9) and abs(row["AP50"] - 100.0 * want) < 1e-11
    assert row["AP"] == pytest.approx(100.0 * 2 / 3, abs=1e-9)
    assert st["fp"][ALL, 0, :, 0].tolist() == [1] * 10 and st["tp"][ALL, 0, :, 0].tolist() == [0] * 10
    assert st["fp"][ALL, 0, :, 1].tolist() == [1] * 10 and st["tp"][ALL, 0, :, 1].tolist() == [1] * 10
    assert (row["tp50"], row["fp50"], row["fn50"]) == (2, 1, 0)


def test_image_without_ground_truth_and_image_without_detections():
    dts = [cc.dt([10, 10, 20, 20], 0.9), cc.dt([100, 100, 40, 40], 0.8), cc.dt([300, 300, 10, 10], 0.1)]
    st = ca.image_stats({2: G2}, {1: dts})
    assert st["image_ids"] == [1, 2]
    rows = ca.image_rows(st, {1: 0, 2: 2}, {1: 3, 2: 0})
    assert all(math.isnan(rows[0][k]) for k in ("AP", "AP50", "AP75", "APs", "APm", "APl"))
    assert (rows[0]["tp50"], rows[0]["fp50"], rows[0]["fn50"]) == (0, 3, 0)
    assert rows[1]["AP"] == 0.0 and rows[1]["AP50"] == 0.0 and (rows[1]["tp50"], rows[1]["fp50"], rows[1]["fn50"]) == (0, 0, 2)
    assert rows[1]["diff"] == 2 and rows[0]["diff"] == -3
    # both ground truths are small (400) and medium (1600): the ranges without one are NaN
    assert rows[1]["APs"] == 0.0 and rows[1]["APm"] == 0.0 and math.isnan(rows[1]["APl"])
    ar = ca.average_recall(st)
    assert set(ar) == {"AR900", "AR1000", "AR1100", "ARs", "ARm", "ARl"} and ar["AR1100"] == 0.0 and math.isnan(ar["ARl"])
    # an image the statistics left out (neither ground truth nor detection) still gets a row, and the rows follow count_gt's order
    rows = ca.image_rows(st, {7: 0, 2: 2, 1: 0}, {7: 0, 2: 0, 1: 3})
    assert [r["image_id"] for r in rows] == [7, 2, 1] and math.isnan(rows[0]["AP"]) and (rows[0]["tp50"], rows[0]["fp50"], rows[0]["fn50"]) == (0, 0, 0)


def test_report_orders():
    dts = [cc.dt([10, 10, 20, 20], 0.9), cc.dt([100, 100, 40, 40], 0.8), cc.dt([300, 300, 10, 10], 0.1)]
    gts = {1: [], 2: G2, 3: G2, 4: G2}
    st = ca.image_stats(gts, {1: dts, 3: dts, 4: dts[:1]})
    rep = ca.image_report(st, [4, 3, 2, 1], [2, 2, 2, 0], [1, 3, 0, 3], "val", 0.5)
    assert [r["image_id"] for r in rep["rows"]] == [4, 3, 2, 1]
    assert rep["order_by_ap"] == [2, 4, 3, 1]                      # 0, 50.x, 100, NaN last
    assert rep["order_by_diff"] == [2, 4, 3, 1]                    # 2, 1, -1, -3
    assert rep["split"] == "val" and rep["threshold"] == 0.5 and rep["max_dets"] == [900, 1000, 1100]
    assert rep["AR"]["AR1100"] == 100.0 * 3 / 6 and math.isnan(rep["AR"]["ARl"]) and list(rep["AR"]) == ["AR900", "AR1000", "AR1100", "ARs", "ARm", "ARl"]


# ------------------------------------------------------------------------------------------------------------------ definition-level checks
def test_per_image_ap_is_summarize_on_that_image_alone(family):
    gts, dts, st = family
    rows = ca.image_rows(st, {i: 0 for i in st["image_ids"]}, {i: 0 for i in st["image_ids"]})
    worst = 0.0
    for row in rows:
        i = row["image_id"]
        want = ca.summarize({i: gts[i]}, {i: dts[i]})
        for k in want:
            assert math.isnan(want[k]) == math.isnan(row[k]), (i, k)
            if not math.isnan(want[k]):
                worst = max(worst, abs(want[k] - row[k]))
    print("largest difference to summarize on the image alone (x100 scale)", worst)
    assert worst <= 1e-9


def test_prefix_cuts_are_evaluations_at_that_max_det(family):
    gts, dts, st = family
    for a, area in enumerate(AREAS):
        for m, cut in enumerate(CUTS):
            s, mt, ig, npig = cc.host_flags(gts, dts, area, max_det=cut)
            _, tps, fps = ca._merged_cumulative(s, mt, ig)
            assert np.array_equal(st["tp"][a, :, :, m].sum(axis=0), tps[:, -1]) and np.array_equal(st["fp"][a, :, :, m].sum(axis=0), fps[:, -1]), (area, cut)
            assert np.array_equal(st["npig"][a], npig)


def test_average_recall_from_the_host_flags_directly(family):
    gts, dts, st = family
    ar = ca.average_recall(st)
    assert list(ar) == ["AR50", "AR100", "AR1100", "ARs", "ARm", "ARl"]

    def direct(area, cut):
        s, mt, ig, npig = cc.host_flags(gts, dts, area, max_det=cut)
        if npig.sum() == 0:
            return float("nan")
        return float(np.mean(ca._merged_cumulative(s, mt, ig)[1][:, -1] / npig.sum())) * 100
    for key, area, cut in (("AR50", "all", 50), ("AR100", "all", 100), ("AR1100", "all", 1100), ("ARs", "small", 1100), ("ARm", "medium", 1100),
                           ("ARl", "large", 1100)):
        want = direct(area, cut)
        assert ar[key] == want or (math.isnan(ar[key]) and math.isnan(want)), key
    assert ar["AR50"] < ar["AR1100"]                                # the cut at 50 really removes matched detections


def test_counts_equal_truncated_flags(family):
    gts, dts, st = family
    flags = [cc.host_flags(gts, dts, area) for area in AREAS]
    matched, ignored = np.stack([f[1] for f in flags]), np.stack([f[2] for f in flags])
    npig = np.stack([f[3] for f in flags])
    ids = st["image_ids"]
    lens = [min(len(dts.get(i, [])), ca.MAX_DETS) for i in ids]
    dt_off = np.concatenate([[0], np.cumsum(lens)])
    full = ca.stats_from_flags(matched, ignored, dt_off, npig, CUTS)
    assert all(np.array_equal(x, st[k]) for x, k in zip(full, ("tp", "fp", "ap")))
    rng = np.random.default_rng(11)
    counts = [0, lens[1], lens[2] + 5] + [int(rng.integers(1, n)) if n > 1 else n for n in lens[3:]]
    kept = [min(c, n) for c, n in zip(counts, lens)]
    cols = np.concatenate([np.arange(dt_off[b], dt_off[b] + kept[b]) for b in range(len(ids))]).astype(np.int64)
    cut_off = np.concatenate([[0], np.cumsum(kept)])
    want = ca.stats_from_flags(matched[:, :, cols], ignored[:, :, cols], cut_off, npig, CUTS)
    got = ca.stats_from_flags(matched, ignored, dt_off, npig, CUTS, counts=counts)
    for w, g in zip(want, got):
        assert w.dtype == g.dtype and np.array_equal(w.view(np.int64) if w.dtype == np.float64 else w, g.view(np.int64) if g.dtype == np.float64 else g)
    assert not np.array_equal(got[2], full[2])


# ------------------------------------------------------------------------------------------------------------------------------ the parser
def test_parser_leaves_no_attribute_and_a_missing_instances_json_raises(tmp_path):
    import infer as infer_mod
    from counting_detr_amd.args import get_args_parser
    p = get_args_parser()
    assert not hasattr(p.parse_args([]), "image_report")
    a = p.parse_args(["--image_report", "-dp", str(tmp_path), "--split", "val"])
    assert a.image_report is True
    assert infer_mod.build_image_report(p.parse_args(["-dp", str(tmp_path)])) is None
    with pytest.raises(FileNotFoundError, match="instances_val.json"):
        infer_mod.build_image_report(a)
    (tmp_path / "instances_val.json").write_text("{}")
    rep = infer_mod.build_image_report(a)
    assert rep.gt_json == os.path.join(str(tmp_path), "instances_val.json") and rep.device is None and rep.report is None


# --------------------------------------------------------------------------------------------------------------------------- header / _ffi
def test_entry_is_declared_exported_and_refuses_bad_sizes_before_any_launch():
    from counting_detr_amd import _ffi
    from counting_detr_amd.build import build_lib
    build_lib(verbose=False)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cdetr_hip.h")).read()
    assert "int cdetr_coco_image_stats(" in src and "cdetr_coco_image_stats" in _ffi.EXPORTS
    assert abi_header.field_names("cdetr_coco_match_desc")[-3:] == ["matched", "det_ignored", "npig"]        # whose outputs the new entry reads
    L = _ffi.lib()
    assert L.cdetr_abi_version() == 2
    call = lambda B, A, T, D, M, R: L.cdetr_coco_image_stats(None, None, None, None, None, None, None, B, A, T, D, M, R, None, None, None, None)   # noqa: E731
    assert call(1, 4, 0, 0, 3, 101) == -1 and b"cdetr_coco_image_stats" in L.cdetr_last_error()
    for sizes in ((1, 4, 17, 0, 3, 101), (1, 4, 10, 0, 65, 101), (1, 4, 10, 0, 3, 257), (1, 65536, 10, 0, 3, 101)):
        assert call(*sizes) == -3 and b"cdetr_coco_image_stats" in L.cdetr_last_error(), sizes
    assert call(1, 4, 10, 0, 3, 101) == -1                          # inside the limits: the null pointers are what is wrong
    assert call(0, 4, 10, 0, 3, 101) == 0                           # no image: nothing to do
