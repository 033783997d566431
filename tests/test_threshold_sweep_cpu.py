"""The threshold sweep without a GPU: the ABI of cdetr_count_sweep, the --sweep_thresholds spec, the prefix property that lets ONE COCO
matching at the lowest threshold serve every threshold (coco_ap.accumulate_sweep against the filter-then-evaluate checker
coco_ap.summarize_sweep), the choice of the best threshold and the checkpoint's "count_threshold" entry.  Every comparison is ==."""
import ctypes
import re

import numpy as np
import pytest
import torch

from counting_detr_amd import coco_ap as ca
from counting_detr_amd import threshold_sweep as ts

import abi_header
import threshold_sweep_ref as ref

AP_KEYS = ("AP", "AP50", "AP75", "APs", "APm", "APl")


@pytest.fixture(scope="module")
def L():
    from counting_detr_amd.build import build_lib
    build_lib(verbose=False)
    from counting_detr_amd import _ffi
    return _ffi.lib()


# ---------------------------------------------------------------------------------------------------------------------------------- ABI
def test_entry_exported_declared_and_in_the_build(L):
    from counting_detr_amd import _ffi, build
    assert "cdetr_count_sweep" in _ffi.EXPORTS and hasattr(L, "cdetr_count_sweep")
    assert re.search(r"^int cdetr_count_sweep\(const float\* prob, const float\* thresholds, int32_t B, int32_t Q, int32_t T, int32_t\* table, "
                     r"int32_t N, int32_t first,\s+void\* stream\);", abi_header.source(), flags=re.M)
    assert "threshold_sweep.hip" in build.SOURCES and L.cdetr_abi_version() == 2


def test_bad_sizes_are_refused_before_any_launch(L):
    """Host addresses that are never dereferenced: every call below must return before it launches."""
    raw = (ctypes.c_char * 64)()
    a = ctypes.addressof(raw)
    call = lambda B, Q, T, N, first, prob=a, thr=a, table=a: L.cdetr_count_sweep(prob, thr, B, Q, T, table, N, first, None)      # noqa: E731
    for args, rc in (((1, 8, 33, 4, 0), -3), ((65536, 8, 4, 70000, 0), -3), ((0, 8, 4, 4, 0), -1), ((1, 0, 4, 4, 0), -1), ((1, 8, 0, 4, 0), -1),
                     ((2, 8, 4, 4, 3), -1), ((1, 8, 4, 4, -1), -1), ((1, 8, 4, 2 ** 31 - 1, 2 ** 31 - 1), -1)):
        assert call(*args) == rc, args
        assert b"cdetr_count_sweep" in L.cdetr_last_error(), args
    assert call(1, 8, 4, 4, 0, prob=None) == -1 and call(1, 8, 4, 4, 0, thr=None) == -1 and call(1, 8, 4, 4, 0, table=None) == -1


# --------------------------------------------------------------------------------------------------------------------------- the rule, the spec
def test_rule_and_count_table_agree_with_the_restatement():
    rng = np.random.default_rng(3)
    thr = [0.25, 0.5, 0.5, 0.7]
    prob = np.stack([ref.probe_row(rng, 200, thr), ref.probe_row(rng, 200, thr, kind="equal")])
    assert np.isnan(prob).any()
    got, want = ts.count_table(prob, thr), ref.count_table(prob, thr)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(ts.kept(prob, 0.7), ref.kept(prob, 0.7)) and not ts.kept(np.float32("nan"), 0.0)
    assert ts.widen(0.3) == float(np.float32(0.3)) != 0.3 and ts.widen(0.5) == 0.5
    with pytest.raises(ValueError):
        ts.widen(float("nan"))


def test_spec_parsing():
    got = ts.parse_spec("0.3:0.7:9")
    assert got == ref.linspace_spec(0.3, 0.7, 9) and len(got) == 9 and got[0] == ref.widen(0.3) and got[-1] == ref.widen(0.7)
    assert ts.parse_spec("0.3:0.7:9", 0.5) == got                                      # 0.5 is one of the nine already
    assert ts.parse_spec("0.3:0.7:9", 0.42) == sorted(got + [ref.widen(0.42)])         # --threshold is merged in
    assert ts.parse_spec("0.7, 0.2,0.5") == [ref.widen(0.2), 0.5, ref.widen(0.7)]
    assert ts.parse_spec("0.6", 0.5) == [0.5, ref.widen(0.6)]
    near = float(np.nextafter(np.float64(0.3), 1.0))                                    # another double, the same fp32
    assert ts.parse_spec(f"0.3,{near!r},0.3") == [ref.widen(0.3)]
    assert len(ts.parse_spec("0:1:32")) == 32 and len(ts.parse_spec("0.1:0.9:31", 0.55)) == 32
    for bad in ("0:1:33", "0.1:0.9:32|0.55", ",".join(str(i / 40) for i in range(33)), "a,b", "0.1:0.9", "0.1:0.9:0", "", "nan"):
        spec, _, thr = bad.partition("|")
        with pytest.raises(ValueError):
            ts.parse_spec(spec, float(thr) if thr else None)
    assert ts.column(got, 0.5) == 4 and ts.column(got, 0.3) == 0
    with pytest.raises(ValueError):
        ts.column(got, 0.31)


def test_parser_flags():
    from counting_detr_amd.args import get_args_parser
    p = get_args_parser()
    import infer as infer_mod
    a = p.parse_args([])                                       # off by default: the namespace (what a checkpoint's "args" pickles) is what it was
    assert not any(hasattr(a, k) for k in ("threshold", "sweep_thresholds", "calibrate_threshold"))
    assert infer_mod.run_threshold(a) == 0.5 and infer_mod.build_sweep(a) is None
    a = p.parse_args(["--threshold", "0.35", "--sweep_thresholds", "0.3:0.7:9", "--calibrate_threshold", "mae"])
    assert a.threshold == 0.35 and a.sweep_thresholds == "0.3:0.7:9" and a.calibrate_threshold == "mae"
    assert p.parse_args(["--threshold", "ckpt"]).threshold == "ckpt"


# --------------------------------------------------------------------------------------------------------------------- the prefix property
SCORES = [0.05, 0.2, 0.2, 0.3, 0.35, 0.35, 0.5, 0.5, 0.5, 0.6, 0.7, 0.7, 0.85, 0.9]          # few values: many exact ties, many on a threshold
THRESHOLDS = [0.2, 0.35, 0.5, 0.6, 0.7, 0.9]


def make_pack(seed):
    """6 images (ids not in order): 0-40 ground truths, 0-60 detections each -- about half of them jittered ground-truth boxes, so that matches exist
    at several IoU thresholds --, scores from SCORES (fp32, widened) and their fp32 neighbours; image 11 has neither, image 5 only ground truth."""
    rng = np.random.default_rng(seed)
    gt_by, dt_by = {}, {}
    pool = np.array([ref.widen(s) for s in SCORES] + [float(np.nextafter(np.float32(0.5), np.float32(0))), float(np.nextafter(np.float32(0.5), np.float32(1)))])
    for img in (7, 3, 11, 5, 20, 1):
        n_gt = 0 if img == 11 else int(rng.integers(1 if img == 5 else 0, 41))
        n_dt = 0 if img in (11, 5) else int(rng.integers(0, 61))
        gts = []
        for _ in range(n_gt):
            side = float(rng.choice([12.0, 40.0, 120.0]))                          # small, medium and large ground truths
            w, h = side * rng.uniform(0.7, 1.3), side * rng.uniform(0.7, 1.3)
            b = [float(rng.uniform(0, 500)), float(rng.uniform(0, 500)), float(w), float(h)]
            gts.append({"bbox": b, "area": b[2] * b[3], "iscrowd": 0, "ignore": int(rng.random() < 0.05)})
        dts = []
        for _ in range(n_dt):
            if gts and rng.random() < 0.55:
                g = gts[int(rng.integers(len(gts)))]["bbox"]
                j = rng.normal(0, 0.08, 4)
                b = [g[0] + j[0] * g[2], g[1] + j[1] * g[3], g[2] * (1 + j[2]), g[3] * (1 + j[3])]
            else:
                b = [float(rng.uniform(0, 500)), float(rng.uniform(0, 500)), float(rng.uniform(5, 150)), float(rng.uniform(5, 150))]
            b = [float(int(v)) for v in b]
            dts.append({"bbox": b, "score": float(rng.choice(pool)), "area": b[2] * b[3]})
        if gts:
            gt_by[img] = gts
        if dts or img == 11:
            dt_by[img] = dts                                                   # image 11 is named and empty
    return gt_by, dt_by


def prefix_route(gt_by, dt_by, thresholds, max_det):
    """The six numbers per threshold from `_evaluate_image`'s flags at the LOWEST threshold alone, through coco_ap's prefix code."""
    low = ref.filter_detections(dt_by, min(thresholds))
    flags, scores = {}, None
    for area, rng in ca.AREA_RNG.items():
        s, m, ig, npig = [], [], [], 0
        for img in sorted(set(gt_by) | set(low)):
            g, d = gt_by.get(img, []), low.get(img, [])
            if not g and not d:
                continue
            si, mi, igi, n = ca._evaluate_image(d, g, rng, max_det)
            s.append(si); m.append(mi); ig.append(igi)
            npig += n
        T = len(ca.IOU_THRS)
        flags[area] = (np.concatenate(m, axis=1) if m else np.zeros((T, 0), bool), np.concatenate(ig, axis=1) if ig else np.zeros((T, 0), bool), npig)
        scores = np.concatenate(s) if s else np.zeros(0)
    return ca.summarize_flags_sweep(scores, flags, thresholds)


def same(a, b):
    return set(a) == set(b) and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a)


@pytest.mark.parametrize("seed,max_det", [(11, ca.MAX_DETS), (12, ca.MAX_DETS), (11, 20)])
def test_prefix_route_equals_filter_then_evaluate(seed, max_det):
    gt_by, dt_by = make_pack(seed)
    assert not gt_by.get(11) and not dt_by.get(11) and gt_by.get(5) and not dt_by.get(5)
    want = ca.summarize_sweep(gt_by, dt_by, THRESHOLDS, max_det=max_det)
    got = prefix_route(gt_by, dt_by, THRESHOLDS, max_det)
    counts = [sum(len(d) for d in ref.filter_detections(dt_by, t).values()) for t in THRESHOLDS]
    for t, w, g, c in zip(THRESHOLDS, want, got, counts):
        print(t, c, "filter-then-evaluate", w, "prefix", g)
    assert len(got) == len(want) == len(THRESHOLDS)
    assert all(same(w, g) for w, g in zip(want, got))
    # the reference rule itself must tell the thresholds apart, or the equality above would show nothing
    aps = [w["AP"] for w in want]
    assert all(a == a for a in aps)
    distinct = [k for k in range(len(THRESHOLDS)) if all(aps[k] != aps[j] and counts[k] != counts[j] for j in range(len(THRESHOLDS)) if j != k)]
    assert len(distinct) >= 3, (aps, counts)
    if max_det == 20:                                                          # the cut bites: some image keeps more than max_det at the lowest threshold
        assert max(len(d) for d in ref.filter_detections(dt_by, THRESHOLDS[0]).values()) > 20
    # each row is also plain `summarize` on the filtered detections (what summarize_sweep is made of)
    assert same(want[2], ca.summarize(gt_by, ref.filter_detections(dt_by, THRESHOLDS[2]), max_det=max_det))


def test_accumulate_is_unchanged_by_the_shared_tail():
    """`accumulate` against the loops of `average_precision` on one of the packs, and the degenerate shapes."""
    gt_by, dt_by = make_pack(11)
    pack = ca.pack_images(gt_by, dt_by)
    flags = []
    for img in pack["image_ids"]:
        flags.append(ca._evaluate_image(dt_by.get(img, []), gt_by.get(img, []), ca.AREA_RNG["all"], ca.MAX_DETS))
    m, ig = np.concatenate([f[1] for f in flags], 1), np.concatenate([f[2] for f in flags], 1)
    npig = sum(f[3] for f in flags)
    assert np.array_equal(ca.accumulate(pack["dt_score"], m, ig, npig), ca.average_precision(gt_by, dt_by))
    T, R = len(ca.IOU_THRS), len(ca.REC_THRS)
    assert np.array_equal(ca.accumulate(np.zeros(0), np.zeros((T, 0), bool), np.zeros((T, 0), bool), 0), -np.ones((T, R)))
    assert np.array_equal(ca.accumulate(np.zeros(0), np.zeros((T, 0), bool), np.zeros((T, 0), bool), 5), np.zeros((T, R)))
    sweep = ca.accumulate_sweep(pack["dt_score"], m, ig, npig, [0.0, 2.0])
    assert np.array_equal(sweep[0], ca.accumulate(pack["dt_score"], m, ig, npig)) and np.array_equal(sweep[1], np.zeros((T, R)))


def test_store_sweep_refuses_a_store_emitted_elsewhere():
    from types import SimpleNamespace
    store = SimpleNamespace(threshold=0.5, max_det=ca.MAX_DETS)
    with pytest.raises(RuntimeError, match="lowest threshold"):
        ca.summarize_store_sweep({}, store, [], [0.3, 0.5])
    with pytest.raises(RuntimeError, match="max_det"):
        ca.summarize_store_sweep({}, SimpleNamespace(threshold=ref.widen(0.3), max_det=5), [], [0.3, 0.5])


# ------------------------------------------------------------------------------------------------------------------------------- best, report
def test_best_selection():
    nan = float("nan")
    rows = [{"threshold": ref.widen(t), "MAE": mae, "RMSE": 1.0, "NAE": nan, "SRE": sre, "AP": ap}
            for t, mae, sre, ap in ((0.2, 3.0, nan, 10.0), (0.4, 2.0, 5.0, nan), (0.5, 2.5, 5.0, 30.0), (0.6, 2.0, 4.0, 30.0), (0.7, nan, 4.0, 12.0))]
    b = ts.best(rows)
    assert b["MAE"] == {"threshold": ref.widen(0.4), "value": 2.0}                      # 0.4 and 0.6 tie and fp32 puts 0.4 nearer to 0.5
    assert abs(ref.widen(0.4) - 0.5) < abs(ref.widen(0.6) - 0.5)
    assert b["RMSE"] == {"threshold": 0.5, "value": 1.0}                                # all equal: nearest to 0.5
    assert b["NAE"]["threshold"] is None and b["NAE"]["value"] != b["NAE"]["value"]     # NaN never wins
    assert b["SRE"] == {"threshold": ref.widen(0.6), "value": 4.0}                      # 0.6 and 0.7 tie; the NaN of 0.2 is out
    assert b["AP"] == {"threshold": 0.5, "value": 30.0}                                 # highest wins, the NaN does not
    for key, higher in (("MAE", False), ("RMSE", False), ("SRE", False), ("AP", True)):
        assert (b[key]["threshold"], b[key]["value"]) == ref.best(rows, key, higher), key
    assert ref.best(rows, "NAE", False) is None
    sym = [{"threshold": t, "MAE": 1.0, "RMSE": 1.0, "NAE": 1.0, "SRE": 1.0} for t in (0.25, 0.75)]
    got = ts.best(sym)
    assert got["MAE"]["threshold"] == 0.25 and "AP" not in got                          # equally near: the lower one; no AP column, no AP entry


def test_report_rows_are_the_plain_loops_floats():
    from counting_detr_amd.engine import counting_metrics
    rng = np.random.default_rng(5)
    thr = ts.parse_spec("0.3,0.5,0.7")
    prob = rng.random((7, 50), dtype=np.float32)
    gt = [0, 3, 25, 40, 12, 1, 50]
    table = ref.count_table(prob, thr)
    ap_rows = [{k: float(i) for k in AP_KEYS} for i in range(3)]
    rep = ts.report(thr, table, gt, ap_rows)
    assert rep["thresholds"] == thr and [r["threshold"] for r in rep["rows"]] == thr
    for k, row in enumerate(rep["rows"]):
        want = counting_metrics([int((prob[i] >= np.float32(thr[k])).sum()) for i in range(7)], gt)
        assert {m: row[m] for m in want} == want and row["AP"] == float(k)
        assert list(row) == ["threshold", "MAE", "RMSE", "NAE", "SRE", *AP_KEYS]
    assert set(rep["best"]) == {"MAE", "RMSE", "NAE", "SRE", "AP"} and rep["best"]["AP"] == {"threshold": thr[2], "value": 2.0}
    assert "AP" not in ts.report(thr, table, gt)["rows"][0]


# ---------------------------------------------------------------------------------------------------------------------------------- checkpoint
def test_count_threshold_round_trip(tmp_path):
    rows = [{"threshold": ref.widen(t), "MAE": m, "RMSE": m, "NAE": m, "SRE": m} for t, m in ((0.3, 4.0), (0.5, 2.0), (0.7, 1.5))]
    rep = {"thresholds": [r["threshold"] for r in rows], "rows": rows, "best": ts.best(rows)}
    entry = ts.calibration(rep, "mae", 3)
    assert entry == {"metric": "mae", "threshold": ref.widen(0.7), "value": 1.5, "epoch": 3}
    path = tmp_path / "c.pth"
    torch.save({"model": {}, "epoch": 3, "count_threshold": entry}, path)
    back = torch.load(path, map_location="cpu", weights_only=False)
    assert back["count_threshold"] == entry and ts.checkpoint_threshold(back, str(path)) == ref.widen(0.7)
    assert ts.calibration({"best": {"MAE": {"threshold": None, "value": float("nan")}}}, "mae", 0) is None


def test_threshold_ckpt_on_a_checkpoint_without_the_entry(tmp_path, monkeypatch):
    """infer.py --threshold ckpt --resume <a checkpoint main.py wrote without calibration>: an error that names the missing key, before any
    data is touched; old checkpoints still load through checkpoint.resume_model."""
    import counting_detr_amd
    import infer as infer_mod
    from counting_detr_amd import checkpoint as ckpt_io
    from counting_detr_amd.args import get_args_parser
    model = torch.nn.Linear(2, 2)
    path = tmp_path / "old.pth"
    torch.save({"model": model.state_dict(), "epoch": 0, "best": {"metric": "mae", "value": 1.0, "epoch": 0}}, path)
    ckpt, missing, skipped = ckpt_io.resume_model(torch.nn.Linear(2, 2), str(path), log=lambda *_: None)
    assert "count_threshold" not in ckpt and not missing and not skipped
    monkeypatch.setattr(counting_detr_amd, "build_model", lambda args: (torch.nn.Linear(2, 2), None, None))
    monkeypatch.setattr(infer_mod, "eval_loader", lambda *a: pytest.fail("the loader was built before the threshold was read"))
    args = get_args_parser().parse_args(["--threshold", "ckpt", "--resume", str(path), "--device", "cpu", "-o", str(tmp_path)])
    with pytest.raises(KeyError, match="count_threshold"):
        infer_mod.main(args)
    with pytest.raises(KeyError, match="count_threshold"):
        ts.checkpoint_threshold({"model": {}})
    args = get_args_parser().parse_args(["--threshold", "ckpt", "--device", "cpu", "-o", str(tmp_path)])
    with pytest.raises(ValueError, match="--resume"):
        infer_mod.main(args)
