"""cdetr_coco_image_stats (csrc/coco_report.hip) behind ops.coco_image_stats, coco_ap.image_stats / image_stats_store and infer.py
--image_report, against coco_ap.stats_from_flags -- numpy on the flags of coco_ap's HOST matcher, pinned to the definition by
tests/test_image_report_cpu.py.  Every comparison is ==; the average precisions are compared as float64 BITS."""
import contextlib
import ctypes
import io
import json
import os

import numpy as np
import pytest
import torch

import coco_ap_cases as cc
import detections_ref as dr
import eval_split as es
from counting_detr_amd import coco_ap as ca
from counting_detr_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AREAS = tuple(ca.AREA_RNG)
CUTS = (50, 100, 1100)
AR_KEYS = ("AR900", "AR1000", "AR1100", "ARs", "ARm", "ARl")
AP_KEYS = ("AP", "AP50", "AP75", "APs", "APm", "APl")


def T(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))).to(DEV)


def flags_of(gts, dts, areas=AREAS):
    """Host-made flags of a set -> (matched [A, T, D] bool, ignored [A, T, D] bool, dt_off [B + 1], npig [A, B])."""
    per = [cc.host_flags(gts, dts, a) for a in areas]
    ids = [i for i in sorted(set(gts) | set(dts)) if gts.get(i) or dts.get(i)]
    dt_off = np.concatenate([[0], np.cumsum([min(len(dts.get(i, [])), ca.MAX_DETS) for i in ids])])
    return np.stack([p[1] for p in per]), np.stack([p[2] for p in per]), dt_off, np.stack([p[3] for p in per]).reshape(len(areas), len(ids))


def same(got, want):
    for name, g, w in zip(("tp", "fp", "ap"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        if name == "ap":
            g, w = np.ascontiguousarray(g).view(np.int64), np.ascontiguousarray(w).view(np.int64)
        bad = int((g != w).sum())
        print(f"{name}: {bad} of {w.size} differ")
        assert bad == 0, name


def check(matched, ignored, dt_off, npig, cuts, counts=None):
    """Upload the flags, one launch, compare every output with stats_from_flags.  -> the checker's (tp, fp, ap)."""
    want = ca.stats_from_flags(matched, ignored, dt_off, npig, cuts, counts=counts)
    got = ops.coco_image_stats(T(matched, np.uint8), T(ignored, np.uint8), T(dt_off, np.int32), T(npig, np.int32), T(cuts, np.int32),
                               T(ca.REC_THRS), dt_cnt=None if counts is None else T(counts, np.int32), host=True)
    same(got, want)
    return want


@pytest.fixture(scope="module")
def families():
    return {"tie": flags_of(*cc.tie_family()), "float": flags_of(*cc.float_family())}


# --------------------------------------------------------------------------------------------------------- the kernel against the checker
@pytest.mark.parametrize("name", ["tie", "float"])
def test_families_at_four_ranges_and_ten_thresholds(families, name):
    f = families[name]
    assert f[0].shape[:2] == (4, 10)
    tp, fp, ap = check(*f, CUTS)
    assert (tp[..., 0] < tp[..., 2]).any() and (ap > 0).any() and (ap[0] < 1).any()       # the cuts cut, the precisions are not all 0 or 1
    check(*f, (1,))


def test_dt_cnt_zero_full_and_in_between(families):
    m, ig, dt_off, npig = families["tie"]
    lens = np.diff(dt_off)
    counts = [0, int(lens[1]), int(lens[2]) // 2, int(lens[3]) + 9]
    cut = check(m, ig, dt_off, npig, CUTS, counts=counts)
    full = ca.stats_from_flags(m, ig, dt_off, npig, CUTS)
    assert (cut[2][:, 0] == 0).all() and np.array_equal(cut[2][:, 1], full[2][:, 1]) and not np.array_equal(cut[2][:, 2], full[2][:, 2])
    assert np.array_equal(cut[2][:, 3], full[2][:, 3])
    check(families["float"][0], families["float"][1], families["float"][2], families["float"][3], (900, 1000, 1100), counts=[64, 1, 65])


@pytest.mark.parametrize("D", [0, 1, 63, 64, 65, 129])
def test_one_image_sets_around_the_chunk_of_64(D):
    rng = np.random.default_rng(100 + D)
    g, d = cc.float_image(rng, 5, D, extent=200.0)
    tp, fp, ap = check(*flags_of({1: g}, {1: d}), CUTS)
    if D == 0:
        assert (ap[0] == 0).all() and (tp == 0).all()                                      # ground truth, no detection: AP 0
    if D:                                                                                    # the same detections on an image without ground truth
        tp, fp, ap = check(*flags_of({1: []}, {1: d}), CUTS)
        assert (ap == -1).all() and (tp == 0).all() and fp[0, 0, 0, 2] == D
    else:                                                                                    # B = 1, Dtot = 0 and no ground truth anywhere
        tp, fp, ap = check(np.zeros((4, 10, 0), bool), np.zeros((4, 10, 0), bool), np.array([0, 0]), np.zeros((4, 1), np.int64), CUTS)
        assert (ap == -1).all()


def test_every_detection_ignored():
    rng = np.random.default_rng(3)
    D = 150
    matched = rng.random((2, 10, D)) < 0.5
    tp, fp, ap = check(matched, np.ones((2, 10, D), bool), np.array([0, 70, D]), np.array([[4, 0], [1, 9]]), CUTS)
    assert (tp == 0).all() and (fp == 0).all() and ap[0, 0].tolist() == [0.0] * 10 and ap[0, 1].tolist() == [-1.0] * 10


@pytest.mark.parametrize("npig", [3, 4, 7, 10, 100])
def test_recall_lands_on_and_beside_the_thresholds(npig):
    """Every ground truth matched, false positives in between: the recalls k / npig hit recall thresholds exactly (1/4, 1/2, 1/10, ...) or miss
    them by one rounding (3 / 10 against 0.3 of the linspace): `side="left"` at equality is what is tested."""
    rng = np.random.default_rng(npig)
    D = npig + 40
    matched = np.zeros((1, 10, D), bool)
    for t in range(10):
        matched[0, t, rng.permutation(D)[:npig]] = True
    tp, fp, ap = check(matched, np.zeros((1, 10, D), bool), np.array([0, D]), np.array([[npig]]), (D,))
    rc = np.arange(1, npig + 1) / npig
    assert np.isin(rc, ca.REC_THRS).sum() >= 1 and tp[0, 0, :, 0].tolist() == [npig] * 10 and (ap > 0).all() and (ap < 1).all()


def test_one_crowded_image_at_the_evaluators_cuts():
    rng = np.random.default_rng(8)
    g, d = cc.float_image(rng, 60, 1100, extent=500.0)
    tp, fp, ap = check(*flags_of({1: g}, {1: d}), ca.MAX_DET_CUTS)
    assert (tp[0, 0, :, 0] <= tp[0, 0, :, 2]).all() and (fp[0, 0, :, 0] < fp[0, 0, :, 2]).all() and tp[0, 0, 0, 2] > 30


def test_one_range_one_threshold_one_cut(families):
    m, ig, dt_off, npig = families["float"]
    check(m[2:3, 4:5], ig[2:3, 4:5], dt_off, npig[2:3], (100,))


# ------------------------------------------------------------------------------------------------------------------------------ the limits
@pytest.mark.parametrize("T_, M, R", [(17, 3, 101), (10, 65, 101), (10, 3, 257)])
def test_beyond_a_limit_nothing_is_launched_or_written(T_, M, R):
    from counting_detr_amd import _ffi
    D = 5
    flags = torch.zeros((1, T_, D), dtype=torch.uint8, device=DEV)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)                          # noqa: E731
    tp, fp = torch.full((T_ * M,), -7, dtype=torch.int32, device=DEV), torch.full((T_ * M,), -7, dtype=torch.int32, device=DEV)
    ap = torch.full((T_,), -7.0, dtype=torch.float64, device=DEV)
    dt_off, npig, cuts, rec = i32([0, D]), i32([[2]]), i32(list(range(1, M + 1))), torch.linspace(0, 1, R, dtype=torch.float64, device=DEV)
    rc = _ffi.lib().cdetr_coco_image_stats(flags.data_ptr(), flags.data_ptr(), dt_off.data_ptr(), None, npig.data_ptr(), cuts.data_ptr(), rec.data_ptr(),
                                           1, 1, T_, D, M, R, tp.data_ptr(), fp.data_ptr(), ap.data_ptr(), ctypes.c_void_p(0))
    torch.cuda.synchronize()
    assert rc == -3 and b"cdetr_coco_image_stats" in _ffi.lib().cdetr_last_error()
    assert (tp == -7).all() and (fp == -7).all() and (ap == -7.0).all()
    with pytest.raises(RuntimeError, match="cdetr_coco_image_stats.*rc=-3"):
        ops.coco_image_stats(flags, flags, dt_off, npig, cuts, rec)


def test_at_the_limits():
    """T = 16, M = 64, R = 256 (unsorted recall thresholds are fine for the kernel; the checker's are fixed, so only tp / fp are compared)."""
    rng = np.random.default_rng(4)
    D = 200
    m, ig = rng.random((1, 16, D)) < 0.6, rng.random((1, 16, D)) < 0.1
    cuts = list(range(1, 65))
    want = ca.stats_from_flags(m, ig, [0, 90, D], [[12, 30]], cuts)
    tp, fp, ap = ops.coco_image_stats(T(m, np.uint8), T(ig, np.uint8), T([0, 90, D], np.int32), T([[12, 30]], np.int32), T(cuts, np.int32),
                                      T(np.linspace(0.0, 1.0, 256)), host=True)
    assert np.array_equal(tp, want[0]) and np.array_equal(fp, want[1]) and ((ap >= 0) & (ap <= 1)).all()


# ------------------------------------------------------------------------------------------------------------------------------ the routes
def stats_same(a, b):
    assert a["image_ids"] == b["image_ids"] and a["cuts"] == b["cuts"] and np.array_equal(a["npig"], b["npig"])
    same([a[k] for k in ("tp", "fp", "ap")], [b[k] for k in ("tp", "fp", "ap")])


def test_device_route_and_store_route_equal_the_host_route():
    """A store filled by cdetr_emit_detections from seeded forward outputs (three images, ids out of order: the gathered pack); ground truths =
    some of each image's own evaluation boxes, jittered, so that there are matches at every IoU threshold and misses."""
    rng = np.random.default_rng(21)
    hw = [(384, 683), (683, 384), (511, 1023)]
    cases = [dr.make_case(rng, 257, hw[k], ties=2) for k in range(3)]
    batch = tuple(np.stack([c[k] for c in cases]) for k in range(4))
    store = ops.DetectionStore(3, 257, DEV)
    store.emit(*(T(x) for x in batch))
    host = store.finish()
    off = host["eval_off"]
    boxes, area = store.eval_boxes[:int(off[-1])].cpu().numpy(), store.eval_area[:int(off[-1])].cpu().numpy()
    image_ids = [7, 3, 11]
    gt_by, dt_by = {}, {}
    for k, i in enumerate(image_ids):
        lo, hi = int(off[k]), int(off[k + 1])
        dt_by[i] = [{"bbox": boxes[j].tolist(), "score": float(host["eval_score"][j]), "area": float(area[j])} for j in range(lo, hi)]
        pick = rng.permutation(np.arange(lo, hi))[:40]
        g = boxes[pick] + np.concatenate([rng.normal(0.0, 0.04, (len(pick), 2)) * boxes[pick, 2:], np.zeros((len(pick), 2))], axis=1)
        gt_by[i] = [cc.gt(b) for b in g if b[2] > 0 and b[3] > 0]
    gt_by[20] = [cc.gt([5.0, 5.0, 30.0, 30.0])]                                              # an image the store never saw: ground truth only
    want = ca.image_stats(gt_by, dt_by)
    assert want["image_ids"] == [3, 7, 11, 20] and (want["ap"][0] > 0).any() and (want["ap"][0, :3] < 1).all()
    stats_same(ca.image_stats(gt_by, dt_by, device=DEV), want)
    stats_same(ca.image_stats_store(gt_by, store, image_ids), want)
    matching = ca.match_store(gt_by, store, image_ids)                                       # the reporting matching: the six numbers and the statistics
    six, stats = matching.six(), matching.stats(ca.MAX_DET_CUTS)
    plain = ca.summarize_store(gt_by, store, image_ids)
    assert set(six) == set(plain) and all(six[k] == plain[k] or (np.isnan(six[k]) and np.isnan(plain[k])) for k in plain)
    stats_same(stats, want)
    # prefix lengths per store image: 0, everything and something in between
    lens = np.diff(off).tolist()
    counts = [lens[0] // 3, 0, lens[2] + 4]
    cut = ca.image_stats({i: g for i, g in gt_by.items()}, {i: dt_by[i][:c] for i, c in zip(image_ids, counts)})
    got = ca.image_stats_store(gt_by, store, image_ids, counts=counts)
    stats_same(got, cut)
    ar, ar_host = ca.average_recall(got), ca.average_recall(cut)
    assert all(ar[k] == ar_host[k] or (np.isnan(ar[k]) and np.isnan(ar_host[k])) for k in ar_host) and list(ar) == list(AR_KEYS)


# ------------------------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """infer.py on the five-image split of tests/eval_split.py with the seeded model of tests/test_eval_batches_gpu.py (class bias shifted
    into the gap under the three highest images): every run the comparisons below read, each once."""
    import infer as infer_mod
    from counting_detr_amd import build_model, data
    from counting_detr_amd.args import default_args, get_args_parser
    from counting_detr_amd.misc import NestedTensor
    from oracle.weights import seeded_state_dict
    root = tmp_path_factory.mktemp("image_report")
    args = default_args()
    args.data_path, args.scale_factor, args.split, args.num_workers, args.device = es.write_split(root / "ds"), 32, "val", 0, DEV
    model, _, _ = build_model(args)
    model.load_state_dict(seeded_state_dict(), strict=True)
    model.to(DEV)
    model.eval()
    ds = data.build_test_dataset(args, "val")
    with torch.no_grad():
        logit = torch.stack([model(NestedTensor(b["image"].to(DEV), b["mask"].to(DEV)), rects=b["ex_rects"].to(DEV))[0]["pred_logits"][0, :, 0]
                             for b in (data.collate([ds[i]]) for i in range(len(ds)))]).double().cpu()
        lo, hi = logit.min(1).values, logit.max(1).values
        order = torch.argsort(lo)
        for ce in {id(m): m for m in model.transformer.cls_embed}.values():
            ce.bias[0] -= 0.5 * (float(hi[order[1]]) + float(lo[order[2]]))
    ckpt = root / "shifted.pth"
    torch.save({"model": model.state_dict()}, ckpt)
    common = ["-dp", args.data_path, "--split", "val", "--resume", str(ckpt), "--no_aux_loss", "--num_query_pattern", "1", "--num_workers", "0",
              "--device", DEV]
    sweep = ["--sweep_thresholds", "0.3:0.7:3", "--threshold", "0.5"]
    out = {"root": root, "launches": {}}
    real = {"coco_match": ops.coco_match, "coco_image_stats": ops.coco_image_stats}
    calls = dict.fromkeys(real, 0)

    def counted(fn):
        def call(*a, **kw):
            calls[fn] += 1
            return real[fn](*a, **kw)
        return call
    for name, extra in (("plain", []), ("host1", ["--image_report"]), ("dev1", ["--image_report", "--device_detections"]),
                        ("host2", ["--image_report", "--eval_batch_size", "2"]),
                        ("dev2", ["--image_report", "--device_detections", "--eval_batch_size", "2"]),
                        ("host1_sweep", ["--image_report", *sweep]), ("dev1_sweep", ["--image_report", "--device_detections", *sweep])):
        buf = io.StringIO()
        calls.update(dict.fromkeys(calls, 0))
        try:
            ops.coco_match, ops.coco_image_stats = counted("coco_match"), counted("coco_image_stats")
            with contextlib.redirect_stdout(buf):
                infer_mod.main(get_args_parser().parse_args(common + ["-o", str(root / name)] + extra))
        finally:
            ops.coco_match, ops.coco_image_stats = real["coco_match"], real["coco_image_stats"]
        out[name] = json.loads(buf.getvalue().strip().splitlines()[-1])
        out["launches"][name] = dict(calls)
    return out


def test_the_store_route_matches_once_for_the_six_numbers_and_the_report(runs):
    print(runs["launches"])
    for name in ("dev1", "dev2", "dev1_sweep"):
        assert runs["launches"][name] == {"coco_match": 1, "coco_image_stats": 1}, name
    assert runs["launches"]["plain"] == {"coco_match": 1, "coco_image_stats": 0}            # the AP of the written file; no statistics launch
    assert runs["launches"]["host1"] == {"coco_match": 2, "coco_image_stats": 1}            # the file is matched for the AP and for the report


def _report(runs, name):
    return open(runs["root"] / name / "image_report_val.json", "rb").read()


def _eq(a, b):
    return a == b or (a != a and b != b)


def test_host_route_and_store_route_write_the_same_report(runs):
    host, dev = _report(runs, "host1"), _report(runs, "dev1")
    rep = json.loads(dev)
    print(rep)
    assert host == dev
    assert list(rep) == ["split", "threshold", "max_dets", "AR", "rows", "order_by_ap", "order_by_diff"]
    assert [r["image_id"] for r in rep["rows"]] == [1, 2, 3, 4, 5] and rep["threshold"] == 0.5 and rep["max_dets"] == [900, 1000, 1100]
    assert all(list(r) == ["image_id", "count_gt", "count_pred", "diff", *AP_KEYS, "tp50", "fp50", "fn50"] for r in rep["rows"])
    assert [r["count_gt"] for r in rep["rows"]] == [im[3] for im in es.IMAGES]
    assert all(r["tp50"] + r["fp50"] == min(r["count_pred"], 1100) and r["tp50"] + r["fn50"] == r["count_gt"] for r in rep["rows"])
    assert sorted(rep["order_by_ap"]) == sorted(rep["order_by_diff"]) == [1, 2, 3, 4, 5]
    diffs = {r["image_id"]: r["diff"] for r in rep["rows"]}
    assert [diffs[i] for i in rep["order_by_diff"]] == sorted(diffs.values(), reverse=True)
    assert all(_eq(runs["host1"][k], runs["dev1"][k]) and _eq(runs["dev1"][k], rep["AR"][k]) for k in AR_KEYS)
    assert set(runs["host1"]) == set(runs["dev1"]) and all(_eq(runs["host1"][k], runs["dev1"][k]) for k in AP_KEYS + ("MAE", "RMSE", "images"))


def test_batches_of_two_give_the_same_rows_by_image(runs):
    host, dev = json.loads(_report(runs, "host2")), json.loads(_report(runs, "dev2"))
    assert [r["image_id"] for r in dev["rows"]] == [i + 1 for b in es.BATCHES_AT_2 for i in b]        # the order they were run in
    by = lambda rep: {r["image_id"]: [(k, v) if v == v else (k, "nan") for k, v in r.items()] for r in rep["rows"]}      # noqa: E731
    assert by(host) == by(dev) and len(by(dev)) == 5
    assert all(_eq(runs["host2"][k], runs["dev2"][k]) for k in AR_KEYS + AP_KEYS)


def test_with_a_sweep_the_report_is_the_plain_pass_at_the_runs_threshold(runs):
    assert _report(runs, "dev1_sweep") == _report(runs, "dev1") and _report(runs, "host1_sweep") == _report(runs, "host1")
    assert all(_eq(runs["dev1_sweep"][k], runs["dev1"][k]) for k in AR_KEYS)
    sw = json.loads(open(runs["root"] / "dev1_sweep" / "threshold_sweep_val.json").read())
    kept = sum(r["count_pred"] for r in json.loads(_report(runs, "dev1"))["rows"])
    print("sweep rows", [(r["threshold"], r["MAE"]) for r in sw["rows"]], "kept at 0.5", kept)
    # the store of the sweep was emitted at 0.3 and holds more than 0.5 keeps: the report's prefix lengths really cut it
    assert len(sw["rows"]) == 3 and sw["rows"][0]["MAE"] > sw["rows"][1]["MAE"] and 0 < kept < 5 * 300


def test_without_the_flag_nothing_changes(runs):
    root = runs["root"]
    assert not os.path.exists(root / "plain" / "image_report_val.json") and os.path.exists(root / "host1" / "image_report_val.json")
    assert open(root / "plain" / "predictions_val.json", "rb").read() == open(root / "host1" / "predictions_val.json", "rb").read()
    with_flag = {k: v for k, v in runs["host1"].items() if k not in AR_KEYS}
    assert list(with_flag) == list(runs["plain"]) and all(_eq(with_flag[k], runs["plain"][k]) for k in with_flag)
    assert list(runs["host1"])[-6:] == list(AR_KEYS)
    assert open(root / "plain" / "results_val.txt").read() == json.dumps(runs["plain"]) + "\n"
