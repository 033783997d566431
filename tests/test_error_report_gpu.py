"""cdetr_coco_errors (csrc/error_report.hip) behind ops.coco_errors, coco_ap.Matching.errors and infer.py --error_report, against the numpy
rule of counting_detr_amd/error_report.py, which tests/test_error_report_cpu.py pins to a serial restatement.  Every comparison is ==; the IoUs
are compared as float64 BITS.  Nothing here reads the reference tree."""
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
import error_report_ref as ref
import eval_split as es
from counting_detr_amd import coco_ap as ca
from counting_detr_amd import error_report as er
from counting_detr_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = ca.AREA_RNG["all"]


def T(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))).to(DEV)


def pack_of(images):
    """[(gts, dts)] -> a pack in the layout of coco_ap.pack_images that keeps EVERY image, the empty ones too (image b = entry b)."""
    dts = [[d[j] for j in np.argsort([-x["score"] for x in d], kind="mergesort")] for _, d in images]
    flat = [d for dl in dts for d in dl]
    return {"image_ids": list(range(len(images))), **ca._pack_gts([g for g, _ in images]),
            "dt_boxes": np.array([d["bbox"] for d in flat], dtype=np.float64).reshape(-1, 4),
            "dt_area": np.array([d["area"] for d in flat], dtype=np.float64), "dt_score": np.array([d["score"] for d in flat], dtype=np.float64),
            "dt_off": np.concatenate([[0], np.cumsum([len(dl) for dl in dts])]).astype(np.int32)}


def launch(pack, counts=None, iou_bg=0.1, g_max=None):
    return ops.coco_errors(T(pack["gt_boxes"].reshape(-1)), T(pack["gt_area"]), T(pack["gt_ignore"]), T(pack["gt_off"], np.int32),
                           T(pack["dt_boxes"].reshape(-1)), T(pack["dt_area"]), T(pack["dt_off"], np.int32),
                           int(pack["g_max"]) if g_max is None else g_max, er.IOU_FG, iou_bg, ALL,
                           dt_cnt=None if counts is None else T(counts, np.int32), host=True)


def check(pack, counts=None, iou_bg=0.1):
    """One launch on the pack, every output compared with the numpy rule.  -> the rule's codes."""
    want = er.classify(pack, counts, iou_bg)
    ref.same(launch(pack, counts, iou_bg), want)
    return want


def _plus(family, seed):
    gts, dts = family()
    rng = np.random.default_rng(seed)
    gts[900], dts[900] = [], cc.float_image(rng, 0, 7, extent=400.0)[1]
    gts[901], dts[901] = cc.float_image(rng, 6, 0, extent=400.0)[0], []
    return gts, dts


@pytest.fixture(scope="module")
def families():
    return {"tie": ca.pack_images(*_plus(cc.tie_family, 5)), "float": ca.pack_images(*_plus(cc.float_family, 5))}


# --------------------------------------------------------------------------------------------------------- the kernel against the checker
@pytest.mark.parametrize("name", ["tie", "float"])
def test_families_with_an_empty_image_on_either_side(families, name):
    want = check(families[name])
    assert set(np.unique(want["dt_code"]).tolist()) == {0, 1, 2, 3, 4} and set(np.unique(want["gt_code"]).tolist()) == {0, 1, 2, 3}
    check(families[name], iou_bg=0.3)


def test_hand_cases_in_one_batch():
    g2 = [cc.gt([10, 10, 20, 20]), cc.gt([100, 100, 40, 40])]
    images = [([cc.gt([0, 0, 1, 1])], [cc.dt([0, 0, 2, 1], 0.9), cc.dt([0, 0, 10, 1], 0.8)]),
              ([cc.gt([0, 0, 1, 1])], [cc.dt([0, 0, 10, 1], 0.8), cc.dt([5, 5, 1, 1], 0.7)]),
              (g2, [cc.dt([10, 10, 20, 20], 0.9), cc.dt([10, 10, 20, 20], 0.8), cc.dt([100, 100, 40, 40], 0.7)]),
              ([cc.gt([10, 10, 20, 20], iscrowd=1), cc.gt([100, 100, 40, 40])], [cc.dt([10, 10, 20, 20], 0.9), cc.dt([12, 10, 20, 20], 0.5)]),
              ([cc.gt([10, 10, 20, 20], iscrowd=1), cc.gt([50, 50, 20, 20], ignore=1)], [cc.dt([300, 300, 5, 5], 0.9), cc.dt([50, 50, 20, 20], 0.5)]),
              ([], [cc.dt([1, 1, 5, 5], 0.9), cc.dt([2, 2, 5, 5], 0.8)]),
              (g2, []),
              ([], []),
              ([cc.gt([0, 0, 16, 16]), cc.gt([100, 100, 16, 16])], [cc.dt([100, 100, 16, 16], 0.9), cc.dt([8, 0, 16, 16], 0.8), cc.dt([0, 0, 16, 64], 0.7)])]
    want = check(pack_of(images))
    assert want["dt_code"][:4].tolist() == [er.TP, er.LOC, er.LOC, er.BKG] and want["dt_iou"][:2].tolist() == [0.5, 0.1]
    assert want["counts"][2].tolist() == [2, 0, 1, 0, 0, 2, 0, 0, 0] and want["counts"][7].tolist() == [0] * 9
    for one in images:
        check(pack_of([one]))


@pytest.mark.parametrize("G", [0, 1, 63, 64, 65, 4096])
def test_sizes_around_the_block_of_64(G):
    """Ground-truth counts around a lane block and at the capacity, each against detection counts around the hand-over chunk and at the
    evaluator's maxDets, as ONE batch (G = 4096, D = 1100 is the crowded image at full size)."""
    rng = np.random.default_rng(300 + G)
    images = []
    for D in (0, 1, 63, 64, 65, 1100):
        images.append(cc.float_image(rng, G, D, extent=2500.0 if G > 100 else 300.0))
    pack = pack_of(images)
    assert pack["g_max"] == G and np.diff(pack["dt_off"]).tolist() == [0, 1, 63, 64, 65, 1100]
    want = check(pack)
    if G >= 63:
        assert (want["counts"][-1, [0, 2, 3, 4]] > 0).all(), want["counts"][-1]


def test_one_crowded_image_of_ties_at_full_size():
    """4096 x 1100 of the tie family: integer boxes on a coarse grid, copied ground truths, repeated scores -- equal IoUs in every 64-block."""
    rng = np.random.default_rng(41)
    pack = pack_of([cc.tie_image(rng, 4096, 1100, grid=40)])
    want = check(pack)
    assert (want["counts"][0] > 0).all(), want["counts"]


def test_prefix_lengths_zero_mid_segment_and_beyond(families):
    pack = families["tie"]
    lens = np.diff(pack["dt_off"]).tolist()
    counts = [0, lens[1] // 2, lens[2] + 9, 65, 3, -4]
    want = check(pack, counts)
    full = er.classify(pack)
    assert (want["dt_code"] == er.UNUSED).sum() == sum(lens) - sum(min(max(c, 0), n) for c, n in zip(counts, lens)) > 0
    assert want["counts"][0, :5].tolist() == [0] * 5 and np.array_equal(want["counts"][2], full["counts"][2])
    check(families["float"], [64, 1, 65, 200, 0])


def test_a_segment_outside_the_buffers_counts_as_empty():
    """Offsets that do not describe the launch's buffers are refused on the device before they address anything: the detections of image 1
    run past Dtot, its ground truths past Gtot -> both segments empty, their outputs untouched, image 0 as it is alone."""
    g, d = cc.float_image(np.random.default_rng(2), 9, 30, extent=200.0)
    pack = pack_of([(g, d), (g[:3], d[:5])])
    alone = er.classify(pack_of([(g, d)]))
    bad = dict(pack)
    bad["gt_off"], bad["dt_off"] = pack["gt_off"] + np.array([0, 0, 2], dtype=np.int32), pack["dt_off"] + np.array([0, 0, 3], dtype=np.int32)
    got = launch(bad)
    assert got["counts"].tolist() == [alone["counts"][0].tolist(), [0] * 9]
    for k in ("dt_code", "dt_gt", "gt_code", "gt_dt"):
        assert np.array_equal(got[k][:len(alone[k])], alone[k]), k


def test_the_tp_and_ign_pattern_is_row_0_0_of_the_matcher(families):
    for pack in families.values():
        matched, ignored, npig = ca.Matching.launch(pack, DEV, ("all",)).host()
        got = launch(pack)
        assert np.array_equal(got["dt_code"] == er.TP, matched[0, 0] & ~ignored[0, 0]) and np.array_equal(got["dt_code"] == er.IGN, ignored[0, 0])
        assert np.array_equal(got["counts"][:, 5] + got["counts"][:, 7] + got["counts"][:, 8], npig[0])


def test_beyond_the_capacity_nothing_is_launched_or_written():
    from counting_detr_amd import _ffi
    z = torch.zeros(8, dtype=torch.float64, device=DEV)
    off = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    ig = torch.zeros(1, dtype=torch.uint8, device=DEV)
    code = torch.full((2,), 7, dtype=torch.uint8, device=DEV)
    idx = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    iou = torch.full((2,), -7.0, dtype=torch.float64, device=DEV)
    counts = torch.full((9,), -7, dtype=torch.int32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                            # noqa: E731
    rc = _ffi.lib().cdetr_coco_errors(p(z), p(z), p(ig), p(off), p(z), p(z), p(off), None, 1, 1, 1, 4097, 0.5, 0.1, ALL[0], ALL[1],
                                      p(code), p(idx), p(iou), p(code[1:]), p(idx[1:]), p(iou[1:]), p(counts), ctypes.c_void_p(0))
    torch.cuda.synchronize()
    assert rc == -3 and b"cdetr_coco_errors" in _ffi.lib().cdetr_last_error() and b"4097" in _ffi.lib().cdetr_last_error()
    assert (code == 7).all() and (idx == -7).all() and (iou == -7.0).all() and (counts == -7).all()
    with pytest.raises(RuntimeError, match="cdetr_coco_errors.*rc=-3"):
        ops.coco_errors(z[:4], z[:1], ig, off, z[:4], z[:1], off, 4097, 0.5, 0.1, ALL)
    out = ops.coco_errors(z[:0], z[:0], ig[:0], off[:1], z[:0], z[:0], off[:1], 0, 0.5, 0.1, ALL, host=True)      # B = 0: nothing is launched
    assert out["counts"].shape == (0, 9) and len(out["dt_code"]) == 0


# ------------------------------------------------------------------------------------------------------------------------------ the routes
def test_device_route_and_store_route_equal_the_numpy_rule():
    """A store filled by cdetr_emit_detections from seeded forward outputs (three images, ids out of order: the gathered pack); ground truths =
    some of each image's own evaluation boxes, jittered or copied: the detections are read where the emit left them."""
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
        g = boxes[pick] + np.concatenate([rng.normal(0.0, 0.25, (len(pick), 2)) * boxes[pick, 2:], np.zeros((len(pick), 2))], axis=1)
        gt_by[i] = [cc.gt(b, iscrowd=int(n % 9 == 0)) for n, b in enumerate(g) if b[2] > 0 and b[3] > 0]
    gt_by[20] = [cc.gt([5.0, 5.0, 30.0, 30.0])]                                              # an image the store never saw: ground truth only
    rule = ca.Matching.of(gt_by, dt_by)
    want = rule.errors()
    print(want["counts"])
    assert rule.pack["image_ids"] == [3, 7, 11, 20] and want["counts"][:, 0].sum() > 0 and want["counts"][3].tolist() == [0] * 8 + [1]
    ref.same(ca.Matching.of(gt_by, dt_by, DEV).errors(), want)
    stored = ca.match_store(gt_by, store, image_ids)
    ref.same(stored.errors(), want)
    assert all(a == b or (a != a and b != b) for a, b in zip(er.what_if(stored.pack, want).values(), er.what_if(rule.pack, want).values()))
    assert er.what_if(stored.pack, want)["AP50_base"] == stored.six()["AP50"]
    # prefix lengths per store image: something in between, nothing, everything and more
    lens = np.diff(off).tolist()
    counts = [lens[0] // 3, 0, lens[2] + 4]
    cut = ca.Matching.of(gt_by, {i: dt_by[i][:c] for i, c in zip(image_ids, counts)}).errors()
    got = stored.errors(counts)
    assert np.array_equal(got["counts"], cut["counts"]) and np.array_equal(got["gt_code"], cut["gt_code"]) and np.array_equal(got["gt_dt"], cut["gt_dt"])
    used = got["dt_code"] != er.UNUSED
    assert np.array_equal(got["dt_code"][used], cut["dt_code"]) and np.array_equal(got["dt_iou"][used].view(np.int64), cut["dt_iou"].view(np.int64))


# ------------------------------------------------------------------------------------------------------------------------------ end to end
ERR_KEYS = er.ERR_KEYS + er.DAP_KEYS
AP_KEYS = ("AP", "AP50", "AP75", "APs", "APm", "APl")
RUNS = (("plain", []), ("host", ["--error_report"]), ("dev", ["--error_report", "--device_detections"]), ("aph", ["--error_report", "--ap_on_host"]),
        ("dev_both", ["--error_report", "--image_report", "--device_detections"]))
SWEEP = ["--sweep_thresholds", "0.3:0.7:3", "--threshold", "0.5"]
RUNS += tuple((n + "_sweep", x + SWEEP) for n, x in RUNS[1:4]) + tuple((n + "_nms", x + ["--nms_iou", "0.5"]) for n, x in RUNS[1:4])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """infer.py on the five-image split of tests/eval_split.py with the seeded model as tests/test_image_report_gpu.py shifts it (class bias
    into the gap under the three highest images): every run the comparisons below read, each once, at --eval_batch_size 1."""
    import infer as infer_mod
    from counting_detr_amd import build_model, data
    from counting_detr_amd.args import default_args, get_args_parser
    from counting_detr_amd.misc import NestedTensor
    from oracle.weights import seeded_state_dict
    root = tmp_path_factory.mktemp("error_report")
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
    out = {"root": root, "launches": {}}
    real = {"coco_match": ops.coco_match, "coco_image_stats": ops.coco_image_stats, "coco_errors": ops.coco_errors}
    calls = dict.fromkeys(real, 0)

    def counted(fn):
        def call(*a, **kw):
            calls[fn] += 1
            return real[fn](*a, **kw)
        return call
    for name, extra in RUNS:
        buf = io.StringIO()
        calls.update(dict.fromkeys(calls, 0))
        try:
            ops.coco_match, ops.coco_image_stats, ops.coco_errors = counted("coco_match"), counted("coco_image_stats"), counted("coco_errors")
            with contextlib.redirect_stdout(buf):
                infer_mod.main(get_args_parser().parse_args(common + ["-o", str(root / name)] + extra))
        finally:
            ops.coco_match, ops.coco_image_stats, ops.coco_errors = real["coco_match"], real["coco_image_stats"], real["coco_errors"]
        out[name] = json.loads(buf.getvalue().strip().splitlines()[-1])
        out["launches"][name] = dict(calls)
    return out


def _report(runs, name):
    return open(runs["root"] / name / "error_report_val.json", "rb").read()


def _eq(a, b):
    return a == b or (a != a and b != b)


def _same_metrics(runs, names):
    first = runs[names[0]]
    for n in names[1:]:
        assert set(runs[n]) == set(first), (n, set(runs[n]) ^ set(first))
        assert all(_eq(runs[n][k], first[k]) for k in ERR_KEYS + AP_KEYS + ("MAE", "RMSE", "images")), (n, runs[n], first)


def test_three_routes_write_the_same_report_and_metrics(runs):
    host = _report(runs, "host")
    rep = json.loads(host)
    print(rep)
    assert host == _report(runs, "dev") == _report(runs, "aph") == _report(runs, "dev_both")
    _same_metrics(runs, ("host", "dev", "aph"))
    assert list(rep) == ["split", "threshold", "iou_fg", "iou_bg", "max_dets", "totals", "dAP50", "rows", "order_by_dup", "order_by_loc",
                         "order_by_bkg", "order_by_missed"]
    assert [r["image_id"] for r in rep["rows"]] == [1, 2, 3, 4, 5] and (rep["threshold"], rep["iou_fg"], rep["iou_bg"], rep["max_dets"]) == (0.5, 0.5, 0.1, 1100)
    assert [r["hit"] + r["ign_gt"] + r["misloc"] + r["missed"] for r in rep["rows"]] == [im[3] for im in es.IMAGES]
    assert sum(r["tp"] + r["ign_dt"] + r["dup"] + r["loc"] + r["bkg"] for r in rep["rows"]) > 0
    assert all(r["tp"] == r["hit"] for r in rep["rows"])
    assert all(runs["dev"]["err_" + k] == rep["totals"][k] for k in ("dup", "loc", "bkg", "misloc", "missed"))
    assert all(_eq(runs["dev"][k], rep["dAP50"][k]) for k in er.DAP_KEYS) and _eq(rep["dAP50"]["AP50_base"], runs["dev"]["AP50"])
    assert list(runs["dev"])[-9:] == list(ERR_KEYS) == list(runs["host"])[-9:]


def test_one_launch_per_pass_and_one_matching_for_both_reports(runs):
    print(runs["launches"])
    assert runs["launches"]["dev"] == {"coco_match": 1, "coco_image_stats": 0, "coco_errors": 1}
    assert runs["launches"]["dev_sweep"] == {"coco_match": 1, "coco_image_stats": 0, "coco_errors": 1}
    assert runs["launches"]["dev_both"] == {"coco_match": 1, "coco_image_stats": 1, "coco_errors": 1}      # both reports read the one matching
    assert runs["launches"]["host"]["coco_errors"] == 1 and runs["launches"]["aph"] == dict.fromkeys(("coco_match", "coco_image_stats", "coco_errors"), 0)
    assert runs["launches"]["plain"]["coco_errors"] == 0
    both = runs["dev_both"]
    assert all(_eq(both[k], runs["dev"][k]) for k in ERR_KEYS + AP_KEYS) and "AR1100" in both and os.path.exists(runs["root"] / "dev_both" / "image_report_val.json")


def test_with_a_sweep_the_report_is_the_plain_pass_at_the_runs_threshold(runs):
    for n in ("host", "dev", "aph"):
        assert _report(runs, n + "_sweep") == _report(runs, n), n
        assert all(_eq(runs[n + "_sweep"][k], runs[n][k]) for k in ERR_KEYS), n
    sw = json.loads(open(runs["root"] / "dev_sweep" / "threshold_sweep_val.json").read())
    rows = json.loads(_report(runs, "dev"))["rows"]
    kept = sum(r["tp"] + r["ign_dt"] + r["dup"] + r["loc"] + r["bkg"] for r in rows)
    # the store of the sweep was emitted at 0.3 and holds more than 0.5 keeps: the report's prefix lengths really cut it
    assert len(sw["rows"]) == 3 and sw["rows"][0]["MAE"] > sw["rows"][1]["MAE"] and 0 < kept < 5 * 300


def test_with_nms_the_three_routes_agree_on_the_survivors(runs):
    assert _report(runs, "host_nms") == _report(runs, "dev_nms") == _report(runs, "aph_nms")
    _same_metrics(runs, ("host_nms", "dev_nms", "aph_nms"))
    assert runs["dev_nms"]["nms_removed"] == runs["host_nms"]["nms_removed"]
    print("nms_removed", runs["dev_nms"]["nms_removed"], "err_dup", runs["dev"]["err_dup"], "->", runs["dev_nms"]["err_dup"])


def test_without_the_flag_nothing_changes(runs):
    root = runs["root"]
    assert not os.path.exists(root / "plain" / "error_report_val.json") and os.path.exists(root / "host" / "error_report_val.json")
    assert sorted(os.listdir(root / "host")) == sorted(os.listdir(root / "plain") + ["error_report_val.json"])
    assert open(root / "plain" / "predictions_val.json", "rb").read() == open(root / "host" / "predictions_val.json", "rb").read()
    with_flag = {k: v for k, v in runs["host"].items() if k not in ERR_KEYS}
    assert list(with_flag) == list(runs["plain"]) and all(_eq(with_flag[k], runs["plain"][k]) for k in with_flag)
    assert not any(k.startswith("err_") or k.startswith("dAP50") for k in runs["plain"])
    assert open(root / "plain" / "results_val.txt").read() == json.dumps(runs["plain"]) + "\n"
