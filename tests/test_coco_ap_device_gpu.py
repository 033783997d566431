"""The device box-AP path (csrc/coco_eval.hip behind counting_detr_amd/coco_ap.py, `device=`) against coco_ap's HOST path -- the code the
device path leaves untouched.  IoUs are compared bit for bit and every matching flag for equality: no tolerance, no case left out.
The crowded images (1500 x 900, 3731 x 1100) are matched under all four area ranges on the device and compared under ONE on the host,
whose interpreted matcher needs 5 s / 15 s per range at these sizes."""
import json
import os

import numpy as np
import pytest
import torch

from counting_detr_amd import coco_ap as ca

import coco_ap_cases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AREAS = tuple(ca.AREA_RNG)


def check_set(gts, dts, host_areas=AREAS, max_det=ca.MAX_DETS, device=DEV):
    """One launch for the whole set under all four ranges; `_evaluate_image` per image and range of `host_areas`.  -> number of flags compared."""
    pack = ca.pack_images(gts, dts, max_det)
    matched, ignored, npig = ca.match_on_device(pack, device, AREAS)
    T, B, D = len(ca.IOU_THRS), len(pack["image_ids"]), len(pack["dt_score"])
    assert matched.shape == ignored.shape == (len(AREAS), T, D) and npig.shape == (len(AREAS), B)
    n = 0
    for area in host_areas:
        a = AREAS.index(area)
        for b, img in enumerate(pack["image_ids"]):
            s, m, ig, k = ca._evaluate_image(dts.get(img, []), gts.get(img, []), ca.AREA_RNG[area], max_det)
            lo, hi = pack["dt_off"][b], pack["dt_off"][b + 1]
            assert np.array_equal(pack["dt_score"][lo:hi], s)
            bad_m, bad_i = int((matched[a][:, lo:hi] != m.reshape(T, -1)).sum()), int((ignored[a][:, lo:hi] != ig.reshape(T, -1)).sum())
            print(f"image {img} ({len(gts.get(img, []))} x {hi - lo}) range {area}: matched differs in {bad_m}, det_ignored in {bad_i} of {T * (hi - lo)}, "
                  f"npig {int(npig[a, b])} / {k}")
            assert bad_m == 0 and bad_i == 0 and int(npig[a, b]) == k, (img, area)
            n += 2 * T * (hi - lo)
    return n


def test_iou_matrix_is_bit_equal_to_numpy():
    rng = np.random.default_rng(5)
    g, d = cc.float_image(rng, 500, 300, extent=600.0)
    gb, db = np.array([x["bbox"] for x in g]), np.array([x["bbox"] for x in d])
    assert (gb != np.round(gb)).all()                                            # fractional: a contracted a * b + c would show
    tg, td = cc.tie_image(rng, 90, 70)
    special_d = [[0, 0, 10, 10], [5, 0, 10, 10], [100, 100, 1, 1], [3.25, 4.5, 0.0, 7.0], [3.25, 4.5, 0.0, 0.0], [1e4, 1e4, 2.5, 2.5], [0.1, 0.2, 0.3, 0.7]]
    special_g = [[0, 0, 10, 10], [0, 0, 20, 20], [3.25, 4.5, 0.0, 0.0], [3.25, 4.5, 0.0, 7.0], [-50.5, -60.25, 10.0, 10.0], [0.1, 0.2, 0.3, 0.7], [0.4, 0.2, 0.3, 0.7]]
    dall = np.concatenate([db, np.array([x["bbox"] for x in td]), np.array(special_d, dtype=np.float64)])
    gall = np.concatenate([gb, np.array([x["bbox"] for x in tg]), np.array(special_g, dtype=np.float64)])
    want = ca.box_iou_xywh(dall, gall)
    got = ca.box_iou_xywh(dall, gall, device=DEV)
    assert ((want > 0) & (want < 1)).sum() > 1000 and (want == 0).sum() > 1000 and (want == 1).sum() >= 2      # overlapping, disjoint, identical
    uni = (dall[:, None, 2] * dall[:, None, 3] + gall[None, :, 2] * gall[None, :, 3])
    assert (uni == 0).any()                                                      # union == 0 -> 0 by the rule, not 0 / 0
    assert got.dtype == np.float64 and got.shape == want.shape
    print("IoU entries that differ:", int((got != want).sum()), "of", want.size, "max |diff|", float(np.abs(got - want).max()))
    assert np.array_equal(got, want)
    assert np.array_equal(got.view(np.uint64) & ~np.uint64(1 << 63), want.view(np.uint64) & ~np.uint64(1 << 63))   # same bits (the sign of a zero aside)
    for dd, gg in ((np.zeros((0, 4)), gall), (dall, np.zeros((0, 4))), (dall[:1], gall[:1]), (dall[:17], gall[:257])):
        assert np.array_equal(ca.box_iou_xywh(dd, gg, device=DEV), ca.box_iou_xywh(dd, gg))


def test_hand_derived_cases():
    s = 50 * 0.38 / 1.62
    gts = {1: [cc.gt([10, 10, 20, 20]), cc.gt([100, 100, 50, 60])],
           2: [cc.gt([5, 5, 120, 120])],
           7: [cc.gt([10, 10, 40, 40]), cc.gt([100, 100, 50, 50])],
           8: [cc.gt([0, 0, 10, 10])],
           9: [cc.gt([0, 0, 10, 10])],
           10: [cc.gt([0, 0, 10, 10]), cc.gt([2, 0, 10, 10])],
           11: [cc.gt([0, 0, 10, 10]), cc.gt([50, 50, 10, 10], iscrowd=1)],
           12: [cc.gt([0, 0, 10, 10]), cc.gt([100, 100, 200, 200])],
           13: [cc.gt([0, 0, 10, 10]), cc.gt([0, 0, 10, 10]), cc.gt([0, 0, 10, 10], ignore=1)]}      # equal IoUs: the highest index first
    dts = {1: [cc.dt([10, 10, 20, 20], 0.9), cc.dt([100, 100, 50, 60], 0.8)],
           2: [cc.dt([5, 5, 120, 120], 0.9)],
           7: [cc.dt([10, 10, 40, 40], 0.9), cc.dt([300, 300, 30, 30], 0.8), cc.dt([100 + s, 100, 50, 50], 0.7)],
           8: [cc.dt([0, 0, 10, 10], 0.5), cc.dt([0, 0, 10, 10], 0.9)],
           9: [cc.dt([0, 0, 10, 10], 0.5), cc.dt([200, 0, 10, 10], 0.9)],
           10: [cc.dt([2, 0, 10, 10], 0.9)],
           11: [cc.dt([0, 0, 10, 10], 0.9), cc.dt([50, 50, 10, 10], 0.8)],
           12: [cc.dt([0, 0, 10, 10], 0.9)],
           13: [cc.dt([0, 0, 10, 10], 0.9), cc.dt([0, 0, 10, 10], 0.9), cc.dt([0, 0, 10, 10], 0.9), cc.dt([0, 0, 10, 10], 0.9)]}
    assert check_set(gts, dts) > 0
    pack = ca.pack_images(gts, dts)
    m, ig, npig = ca.match_on_device(pack, DEV, ("all",))
    lo = pack["dt_off"][pack["image_ids"].index(7)]
    assert m[0][:, lo:lo + 3].tolist() == [[True, False, True]] * 3 + [[True, False, False]] * 7      # IoU 0.62: a hit up to t = 0.60
    lo = pack["dt_off"][pack["image_ids"].index(13)]
    assert m[0][0, lo:lo + 4].tolist() == [True, True, True, False] and ig[0][0, lo:lo + 4].tolist() == [False, False, True, False]
    for k, v in ca.summarize(gts, dts).items():
        w = ca.summarize(gts, dts, device=DEV)[k]
        assert w == v or (np.isnan(w) and np.isnan(v)), k


def test_tie_family():
    gts, dts = cc.tie_family()
    st = cc.tie_statistics(gts, dts)
    print(json.dumps(st))
    cc.assert_tie_bars(st)
    assert check_set(gts, dts) == 2 * 4 * 10 * sum(len(v) for v in dts.values())
    assert check_set(gts, dts, max_det=50) == 2 * 4 * 10 * sum(min(len(v), 50) for v in dts.values())      # max_det below D


def test_float_family():
    gts, dts = cc.float_family()
    assert check_set(gts, dts) > 0
    assert check_set(gts, dts, max_det=33) > 0


def test_sizes_from_empty_to_several_waves_in_one_launch():
    """0 x 5, 5 x 0, 1 x 1, 63 / 64 / 65 x 100 (one lane short of, exactly, one past a wave's width), 130 x 70 and 400 x 600 side by side:
    workgroups of very different length in one launch, in both families."""
    shapes = ((0, 5), (5, 0), (1, 1), (63, 100), (64, 100), (65, 100), (130, 70))
    rng = np.random.default_rng(11)
    gts, dts = {}, {}
    for i, (G, D) in enumerate(shapes):
        gts[i], dts[i] = cc.tie_image(rng, G, D)
        gts[50 + i], dts[50 + i] = cc.float_image(rng, G, D, extent=300.0)
    gts[99], dts[99] = cc.float_image(rng, 400, 600, extent=700.0)
    gts[98], dts[98] = cc.tie_image(rng, 257, 300, grid=20)
    assert check_set(gts, dts) == 2 * 4 * 10 * sum(len(v) for v in dts.values())
    # an image alone in its launch gives what it gives beside the others
    one = ca.match_on_device(ca.pack_images({3: gts[3]}, {3: dts[3]}), DEV)
    pack = ca.pack_images(gts, dts)
    b = pack["image_ids"].index(3)
    lo, hi = pack["dt_off"][b], pack["dt_off"][b + 1]
    allm = ca.match_on_device(pack, DEV)
    assert np.array_equal(one[0], allm[0][:, :, lo:hi]) and np.array_equal(one[1], allm[1][:, :, lo:hi]) and np.array_equal(one[2][:, 0], allm[2][:, b])


def test_crowded_tie_image_1500_x_900():
    rng = np.random.default_rng(21)
    g, d = cc.tie_image(rng, 1500, 900, grid=40)
    small, d_small = cc.tie_image(rng, 3, 4)
    assert check_set({1: g, 2: small}, {1: d, 2: d_small}, host_areas=("medium",)) == 2 * 10 * 904


def test_most_crowded_image_3731_x_1100():
    """FSC-147's largest object count with the evaluator's maxDets: 59 ground truths per lane, the LDS image at 118 KiB."""
    rng = np.random.default_rng(22)
    g, d = cc.float_image(rng, 3731, 1300, extent=2500.0)
    assert check_set({1: g}, {1: d}, host_areas=("all",)) == 2 * 10 * ca.MAX_DETS


def test_capacity_is_a_clean_error():
    from counting_detr_amd import ops
    z = torch.zeros(8, dtype=torch.float64, device=DEV)
    off = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="cdetr_coco_match.*capacity"):
        ops.coco_match(z[:4], z[:1], torch.zeros(1, dtype=torch.uint8, device=DEV), off, z[:4], z[:1], off, z[:1] + 0.5, z[:2], g_max=4097)
    rng = np.random.default_rng(23)                                              # the limit itself works: 64 ground truths in every lane
    g, d = cc.float_image(rng, 4096, 40, extent=3000.0)
    assert check_set({1: g}, {1: d}, host_areas=("all",)) == 2 * 10 * 40


def _same(a, b):
    return set(a) == set(b) and all(a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])) for k in a)


def test_summary_numbers_are_equal_end_to_end(tmp_path):
    gts, dts = cc.tie_family(seed=4, shapes=((80, 120), (40, 90), (0, 6), (7, 0)))
    g2, d2 = cc.float_family(seed=5)
    gts.update(g2); dts.update(d2)
    host = ca.summarize(gts, dts)
    dev = ca.summarize(gts, dts, device=DEV)
    print("host", host, "device", dev)
    assert _same(host, dev) and 0 < host["AP"] < 100
    assert _same(ca.summarize(gts, dts, max_det=20), ca.summarize(gts, dts, max_det=20, device=torch.device(DEV)))
    for area in AREAS:
        assert np.array_equal(ca.average_precision(gts, dts, area), ca.average_precision(gts, dts, area, device=DEV))
    only_small = {1: [cc.gt([0, 0, 10, 10])]}                                    # NaN where NaN: no medium / large ground truth
    host, dev = ca.summarize(only_small, {1: [cc.dt([0, 0, 10, 10], 0.9)]}), ca.summarize(only_small, {1: [cc.dt([0, 0, 10, 10], 0.9)]}, device=DEV)
    assert np.isnan(host["APm"]) and np.isnan(dev["APl"]) and _same(host, dev)
    assert _same(ca.summarize({}, {}), ca.summarize({}, {}, device=DEV))
    # the json pair in the reference's wire format: predictions carry [cx, cy, w, h]
    gt_json = {"images": [{"id": i} for i in gts], "categories": [{"id": 1, "name": "fg"}], "annotations": []}
    pr_json = {"images": [{"id": i} for i in gts], "categories": [{"id": 1, "name": "fg"}], "annotations": []}
    for i, gl in gts.items():
        for g in gl:
            gt_json["annotations"].append({"id": len(gt_json["annotations"]) + 1, "image_id": i, "category_id": 1, "bbox": g["bbox"], "area": g["area"],
                                           "iscrowd": g.get("iscrowd", 0)})
    for i, dl in dts.items():
        for d in dl:
            x, y, w, h = d["bbox"]
            pr_json["annotations"].append({"id": len(pr_json["annotations"]) + 1, "image_id": i, "category_id": 1, "bbox": [x + w / 2, y + h / 2, w, h],
                                           "score": d["score"], "point": [0, 0]})
    pj, gj = tmp_path / "p.json", tmp_path / "g.json"
    pj.write_text(json.dumps(pr_json)); gj.write_text(json.dumps(gt_json))
    host, dev = ca.ap_from_json(str(pj), str(gj)), ca.ap_from_json(str(pj), str(gj), device=DEV)
    print("json host", host, "device", dev)
    assert _same(host, dev) and 0 < host["AP"] < 100
    ids = list(gts)[:3]
    assert _same(ca.ap_from_json(str(pj), str(gj), image_ids=ids), ca.ap_from_json(str(pj), str(gj), image_ids=ids, device=DEV))


@pytest.mark.parametrize("name", ["tie", "float"])
def test_one_device_matching_answers_everything_as_the_host_matching_does(name):
    """ONE coco_ap.Matching on the device, asked for the six numbers, the sweep, the statistics (with prefix lengths), row [0, 0] and the six
    again: one cdetr_coco_match launch, one cdetr_coco_image_stats launch, two Tensor.cpu calls (the launch's buffer once, the statistics) and
    none when everything but the statistics is asked again; every answer equals the host matching's (tests/test_matching_cpu.py)."""
    from counting_detr_amd import ops
    gts, dts = cc.matching_sets()[name]
    thresholds, cuts = (0.0, 0.25, 0.5, 0.9, 2.0), (5, 20, 1100)
    host = ca.Matching.of(gts, dts)
    counts = [0, 1000] + [n // 2 for n in np.diff(host.pack["dt_off"]).tolist()[2:]]
    calls = {"coco_match": 0, "coco_image_stats": 0, "cpu": 0}
    real = {"coco_match": ops.coco_match, "coco_image_stats": ops.coco_image_stats, "cpu": torch.Tensor.cpu}

    def counted(fn):
        def call(*a, **kw):
            calls[fn] += 1
            return real[fn](*a, **kw)
        return call
    try:
        ops.coco_match, ops.coco_image_stats, torch.Tensor.cpu = counted("coco_match"), counted("coco_image_stats"), counted("cpu")
        m = ca.Matching.of(gts, dts, device=DEV)
        assert calls == {"coco_match": 1, "coco_image_stats": 0, "cpu": 0}                       # nothing is copied back at construction
        six, rows, stats, row, again = m.six(), m.six_sweep(thresholds), m.stats(cuts, counts), m.row50(), m.six()
        assert calls == {"coco_match": 1, "coco_image_stats": 1, "cpu": 2}
        second = m.six(), m.six_sweep(thresholds), m.row50(), m.host()
        assert calls == {"coco_match": 1, "coco_image_stats": 1, "cpu": 2}
    finally:
        ops.coco_match, ops.coco_image_stats, torch.Tensor.cpu = real["coco_match"], real["coco_image_stats"], real["cpu"]
    assert m.device == torch.device(DEV) and m.matched.is_cuda and m.pack["image_ids"] == host.pack["image_ids"] and m.areas == host.areas
    cc.same_six(six, host.six()); cc.same_six(again, six); cc.same_six(second[0], six)
    for got, want in zip(rows + second[1], host.six_sweep(thresholds) * 2):
        cc.same_six(got, want)
    cc.same_stats(stats, host.stats(cuts, counts))
    assert row[0].is_cuda and row[0].data_ptr() == m.matched.data_ptr() and row[1].data_ptr() == m.det_ignored.data_ptr()      # views: no copy
    for got, want in zip(row, host.row50()):
        assert np.array_equal(got.cpu().numpy().astype(bool), want)
    for got, want in zip(second[3], host.host()):
        assert got.shape == want.shape and np.array_equal(got, want)


def test_launches_are_stream_ordered_and_leave_no_state():
    a = cc.tie_family(seed=6, shapes=((150, 200), (10, 30)))
    b = cc.float_family(seed=7, shapes=((20, 15), (300, 500), (64, 64)))
    c = cc.tie_family(seed=8, shapes=((1, 3),))
    want = {k: [cc.host_flags(*s, area) for area in ("all", "medium")] for k, s in (("a", a), ("b", b), ("c", c))}
    side = torch.cuda.Stream(device=DEV)
    for k, s, stream in (("a", a, None), ("b", b, None), ("c", c, None), ("a", a, side), ("c", c, side), ("b", b, None), ("a", a, None)):
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(DEV)):
            m, ig, npig = ca.match_on_device(ca.pack_images(*s), DEV, ("all", "medium"))
        for i in range(2):
            _, wm, wi, wn = want[k][i]
            assert np.array_equal(m[i], wm) and np.array_equal(ig[i], wi) and np.array_equal(npig[i], wn), (k, i)
    torch.cuda.synchronize()


def test_infer_cli_prints_the_same_metrics_on_either_path(tmp_path, capsys):
    """infer.py on the tiny FSC-147-format set: the AP the CLI prints is the same six numbers with the device matcher (default) and with
    --ap_on_host; the device path really ran (its launch is counted)."""
    import infer as infer_mod
    from counting_detr_amd import ops
    from counting_detr_amd.args import get_args_parser
    from oracle.weights import seeded_state_dict
    here = os.path.dirname(os.path.abspath(__file__))
    ckpt = tmp_path / "seeded.pth"
    torch.save({"model": seeded_state_dict()}, ckpt)
    calls = []
    real = ops.coco_match

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    out = {}
    try:
        ops.coco_match = counted
        for name, extra in (("device", []), ("host", ["--ap_on_host"])):
            args = get_args_parser().parse_args(["-dp", os.path.join(here, "golden", "fsc147_tiny"), "-o", str(tmp_path / name), "--split", "val",
                                                 "--resume", str(ckpt), "--no_aux_loss", "--num_query_pattern", "1", "--num_workers", "0",
                                                 "--device", DEV] + extra)
            capsys.readouterr()
            infer_mod.main(args)
            out[name] = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
            n_calls = len(calls)
            assert n_calls == 1, (name, n_calls)                               # one launch for the split on the device path, none on the host path
    finally:
        ops.coco_match = real
    print(out)
    ap_keys = ("AP", "AP50", "AP75", "APs", "APm", "APl")
    assert all(k in out["device"] for k in ap_keys) and out["device"]["images"] == 2
    assert _same({k: out["device"][k] for k in ap_keys}, {k: out["host"][k] for k in ap_keys})
    for k in ("MAE", "RMSE", "NAE", "SRE", "images"):
        assert out["device"][k] == out["host"][k], k
    assert open(tmp_path / "device" / "predictions_val.json").read() == open(tmp_path / "host" / "predictions_val.json").read()
