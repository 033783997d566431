"""cdetr_nms_suppress (csrc/nms.hip) behind ops.nms_suppress against the host rule (counting_detr_amd/nms.py) and the serial restatement of
tests/nms_ref.py, then --nms_iou end to end: infer.py's host and device passes on tests/golden/fsc147_tiny with the seeded model of
tests/test_threshold_sweep_gpu.py.  Every comparison is exact: equal NaN masks, the other entries bit for bit, `removed` equal."""
import json
import os

import numpy as np
import pytest
import torch

from counting_detr_amd import nms, ops
from counting_detr_amd import threshold_sweep as ts

import nms_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
AP_KEYS = ("AP", "AP50", "AP75", "APs", "APm", "APl")
COUNT_KEYS = ("MAE", "RMSE", "NAE", "SRE")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(prob, boxes, hw, threshold, iou):
    """One launch into sentinel-filled outputs -> (prob_out, removed) on the host."""
    out = torch.full(prob.shape, -3.0, dtype=torch.float32, device=DEV)
    removed = torch.full((prob.shape[0],), -7, dtype=torch.int32, device=DEV)
    got = ops.nms_suppress(T(prob), T(boxes), T(hw), threshold, iou, out=out, removed=removed)
    assert got[0] is out and got[1] is removed
    return out.cpu().numpy(), removed.cpu().numpy()


# (Q, candidates per image, clusters; 0 clusters = every box apart from every other): Q at 1, 64, 65, 1024, 1025, 4096; candidate counts at the
# chunk edges 0, 1, 64, 65, 128, 129 and 4096 (one cluster: almost everything goes in the first chunk; many clusters: survivors in every
# chunk); three images with (0, 65, 1) in one launch.  The serial restatement costs one Python call per pair, which sets the cluster counts.
CASES = [(1, (0,), 1), (1, (1,), 1), (64, (64,), 1), (64, (1,), 3), (65, (65,), 4), (65, (64,), 0), (300, (0, 65, 1), 5), (1024, (128,), 9),
         (1024, (129,), 0), (1024, (1024,), 60), (1025, (129,), 11), (1025, (0,), 2), (4096, (4096,), 1), (4096, (4096,), 32), (4096, (65,), 6)]


@pytest.mark.parametrize("Q,counts,clusters", CASES)
def test_kernel_equals_the_rule_and_the_serial_restatement(Q, counts, clusters):
    rng = np.random.default_rng(100 * Q + 7 * sum(counts) + clusters)
    prob, boxes, hw = ref.batch(rng, Q, counts, clusters)
    iou = 0.5
    got = run(prob, boxes, hw, 0.5, iou)
    rule, serial = nms.suppress(prob, boxes, hw, 0.5, iou), ref.suppress(prob, boxes, hw, 0.5, iou)
    print("Q", Q, "candidates", counts, "removed", got[1].tolist(), "rule", rule[1].tolist(), "serial", serial[1].tolist())
    assert ref.same(got, rule) and ref.same(got, serial)
    assert np.array_equal(ts.kept(prob, 0.5).sum(1), counts)
    if clusters and max(counts) >= 64:
        assert got[1].sum() >= sum(counts) / 3          # clustered: a third or more goes
    if clusters == 0:
        assert got[1].sum() == 0                        # every candidate survives: 129 survivors walk through three chunks


def test_many_survivors_in_every_chunk_at_the_limit():
    """Q = 4096, all candidates, 700 loose clusters: more than two thousand survivors, hundreds in every quarter of the ranks, so every chunk
    pushes survivors forward (the serial restatement would need millions of calls here; the host rule is the checker)."""
    rng = np.random.default_rng(77)
    prob, boxes, hw = ref.batch(rng, 4096, (4096, 4096), 700, spread=0.3)
    got, rule = run(prob, boxes, hw, 0.5, 0.6), nms.suppress(prob, boxes, hw, 0.5, 0.6)
    print("removed", got[1].tolist(), "rule", rule[1].tolist())
    assert ref.same(got, rule) and (4096 - rule[1] >= 2000).all() and (rule[1] >= 4096 // 3).all()


@pytest.mark.parametrize("name", sorted(ref.constructed()))
def test_constructed_cases(name):
    prob, boxes, hw, threshold, iou, gone = ref.constructed()[name]
    out, removed = run(prob, boxes, hw, threshold, iou)
    assert ref.same((out, removed), nms.suppress(prob, boxes, hw, threshold, iou))
    assert ref.same((out, removed), ref.suppress(prob, boxes, hw, threshold, iou))
    bits, was = out.view(np.uint32)[0], prob.view(np.uint32)[0]
    assert [q for q in range(prob.shape[1]) if bits[q] != was[q]] == gone and removed.tolist() == [len(gone)]
    if name.startswith("special"):
        assert bits[1] == ref.NAN_BITS and bits[2] == 0x80000000


def test_iou_one_is_the_identity_and_iou_zero_takes_any_overlap():
    rng = np.random.default_rng(3)
    prob, boxes, hw = ref.batch(rng, 333, (333, 100), 8)
    out, removed = run(prob, boxes, hw, 0.5, 1.0)
    assert np.array_equal(out.view(np.uint32), prob.view(np.uint32)) and removed.tolist() == [0, 0]
    assert ref.same(run(prob, boxes, hw, 0.5, 0.0), nms.suppress(prob, boxes, hw, 0.5, 0.0))


def test_arguments_are_checked_before_any_launch():
    rng = np.random.default_rng(4)
    prob, boxes, hw = ref.batch(rng, 4097, (10,), 2)
    with pytest.raises(RuntimeError, match="cdetr_nms_suppress.*4097"):
        ops.nms_suppress(T(prob), T(boxes), T(hw), 0.5, 0.5)
    prob, boxes, hw = (T(a) for a in ref.batch(rng, 70, (10, 3), 2))
    with pytest.raises(ValueError, match="nms_iou"):
        ops.nms_suppress(prob, boxes, hw, 0.5, 1.5)
    with pytest.raises(RuntimeError, match="nms_suppress"):
        ops.nms_suppress(prob.double(), boxes, hw, 0.5, 0.5)
    with pytest.raises(RuntimeError, match="nms_suppress"):
        ops.nms_suppress(prob, boxes[:, :, :3].contiguous(), hw, 0.5, 0.5)
    with pytest.raises(RuntimeError, match="nms_suppress"):
        ops.nms_suppress(prob, boxes, hw.long(), 0.5, 0.5)
    with pytest.raises(RuntimeError, match="nms_suppress"):
        ops.nms_suppress(prob.t().contiguous().t(), boxes, hw, 0.5, 0.5)
    with pytest.raises(RuntimeError, match="must not be"):
        ops.nms_suppress(prob, boxes, hw, 0.5, 0.5, out=prob)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ end to end, fsc147_tiny
def _same(a, b):
    return set(a) == set(b) and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a)


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """The passes the end-to-end tests read, run once, on the seeded model of tests/test_threshold_sweep_gpu.py (class bias shifted to the
    first image's median logit; two more thresholds at the 30 % and 70 % quantiles of the probabilities), all with --nms_iou 0.5 but `raw`:
      host, device, device without the flag, host + sweep, device + sweep, a plain device pass at each threshold, and the report + overlays
      by the store route and by the --ap_on_host route."""
    from torch.utils.data import DataLoader
    import infer as infer_mod
    from counting_detr_amd import build_model, data
    from counting_detr_amd.args import default_args
    from counting_detr_amd.engine import InferenceEngine
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
        shift = logit[:logit.numel() // 2].median()
        for ce in {id(m): m for m in model.transformer.cls_embed}.values():
            ce.bias[0] -= shift
    engines = {0.5: InferenceEngine(model, 0.5, device=DEV)}
    fwd = [engines[0.5](NestedTensor(b["image"].to(DEV), b["mask"].to(DEV)), b["ex_rects"].to(DEV)) for b in vl]
    prob = np.concatenate([f[4].cpu().numpy() for f in fwd])
    lo, hi = (ts.widen(v) for v in np.quantile(prob, [0.3, 0.7]))
    gt_json = os.path.join(args.data_path, "instances_val.json")
    thresholds = ts.parse_spec(f"{lo!r},{hi!r}", 0.5)
    engines.update({t: InferenceEngine(model, t, device=DEV) for t in (lo, hi)})
    root = tmp_path_factory.mktemp("nms_tiny")
    out = {"thresholds": thresholds, "lo": lo, "hi": hi, "root": root, "model": model, "criterion": criterion, "args": args}

    def one(name, threshold, device_detections, sweep=False, nms_iou=0.5, report=None):
        os.makedirs(root / name)
        image_report = render = None
        if report is not None:
            image_report, render = infer_mod.ImageReport(gt_json, None if report == "host" else torch.device(DEV)), infer_mod.Render(args.data_path, 2)
        m, _ = infer_mod.infer(model, criterion, vl, torch.device(DEV), str(root / name), split="val", threshold=threshold,
                               device_detections=device_detections, gt_json=gt_json if device_detections else None, engine=engines[threshold],
                               sweep=ts.Sweep(thresholds, gt_json) if sweep else None, nms_iou=nms_iou, image_report=image_report, render=render)
        out[name] = m
    one("host", 0.5, False)
    one("device", 0.5, True)
    one("raw", 0.5, True, nms_iou=None)
    one("host_sweep", 0.5, False, sweep=True)
    one("device_sweep", 0.5, True, sweep=True)
    one("device_lo", lo, True)
    one("device_hi", hi, True)
    one("device_sweep_hi", hi, True, sweep=True)
    one("report_store", 0.5, True, report="device")
    one("report_host", 0.5, False, report="host")
    return out


def _annotations(root, name):
    return json.loads(open(root / name / "predictions_val.json").read())["annotations"]


def test_host_and_device_loops_write_the_same_file_and_metrics(tiny):
    root = tiny["root"]
    host, dev, raw = (open(root / n / "predictions_val.json", "rb").read() for n in ("host", "device", "raw"))
    print("host", tiny["host"], "device", tiny["device"], "without the flag", tiny["raw"])
    assert host == dev != raw
    n, n_raw = len(_annotations(root, "device")), len(_annotations(root, "raw"))
    assert tiny["device"]["nms_removed"] == n_raw - n > 0 and n > 0 and "nms_removed" not in tiny["raw"]
    assert _same(tiny["host"], {k: v for k, v in tiny["device"].items() if k not in AP_KEYS})      # the host loop itself reports no AP
    assert all(k in tiny["device"] for k in AP_KEYS + COUNT_KEYS + ("loss_ce", "images"))
    assert tiny["device"]["MAE"] != tiny["raw"]["MAE"]


def test_sweep_rows_equal_separate_plain_passes_with_the_flag(tiny):
    root = tiny["root"]
    host, dev = (open(root / n / "threshold_sweep_val.json", "rb").read() for n in ("host_sweep", "device_sweep"))
    assert host == dev
    assert open(root / "device_sweep" / "predictions_val.json", "rb").read() == open(root / "device" / "predictions_val.json", "rb").read()
    assert _same(tiny["device_sweep"], tiny["device"]) and _same(tiny["host_sweep"], tiny["host"])
    rows = {r["threshold"]: r for r in json.loads(dev)["rows"]}
    lo, hi = tiny["lo"], tiny["hi"]
    for name, t in (("device_lo", lo), ("device", 0.5), ("device_hi", hi)):
        plain = tiny[name]
        row = {k: v for k, v in rows[t].items() if k != "threshold"}
        print(t, "sweep row", row, "plain pass", {k: plain[k] for k in row}, "removed", plain["nms_removed"])
        assert _same(row, {k: plain[k] for k in row}), t
    removed = [tiny[name]["nms_removed"] for _, name in sorted(((lo, "device_lo"), (0.5, "device"), (hi, "device_hi")))]     # by ascending threshold
    assert removed[0] >= removed[1] >= removed[2] and removed[0] > removed[2] > 0                  # the thresholds cut the suppressed set too
    # a sweep whose own --threshold is its highest: the filter ran at the lowest, the file, the metrics and nms_removed are the highest's
    assert _same(tiny["device_sweep_hi"], tiny["device_hi"]) and tiny["device_hi"]["nms_removed"] < tiny["device"]["nms_removed"]
    assert open(root / "device_sweep_hi" / "predictions_val.json", "rb").read() == open(root / "device_hi" / "predictions_val.json", "rb").read()


def test_report_and_overlays_agree_between_the_store_and_the_host_route(tiny):
    root = tiny["root"]
    a, b = root / "report_store", root / "report_host"
    assert open(a / "image_report_val.json", "rb").read() == open(b / "image_report_val.json", "rb").read()
    files = sorted(os.listdir(a / "render_val"))
    assert files == sorted(os.listdir(b / "render_val")) and any(f.endswith(".png") for f in files)
    for f in files:
        assert open(a / "render_val" / f, "rb").read() == open(b / "render_val" / f, "rb").read(), f
    assert open(a / "predictions_val.json", "rb").read() == open(root / "device" / "predictions_val.json", "rb").read()
    rep = json.loads(open(a / "image_report_val.json").read())
    raw = len(_annotations(root, "raw"))
    assert sum(r["count_pred"] for r in rep["rows"]) == raw - tiny["device"]["nms_removed"]      # the report counts the survivors


def test_the_flag_reaches_the_pass_from_the_command_line(tiny, tmp_path):
    import infer as infer_mod
    from counting_detr_amd.args import get_args_parser
    args = get_args_parser().parse_args(["-dp", tiny["args"].data_path, "--split", "val", "-o", str(tmp_path), "--device", DEV, "--device_detections",
                                         "--nms_iou", "0.5", "--scale_factor", "32", "--num_workers", "0"])
    dl, per_image = infer_mod.eval_loader(args, torch.device(DEV))
    m = infer_mod.evaluate_split(tiny["model"], tiny["criterion"], dl, per_image, torch.device(DEV), args)
    print(m)
    assert _same(m, tiny["device"])
    assert open(tmp_path / "predictions_val.json", "rb").read() == open(tiny["root"] / "device" / "predictions_val.json", "rb").read()
