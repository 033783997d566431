"""cdetr_count_sweep (csrc/threshold_sweep.hip) behind ops.count_sweep / ops.ThresholdSweep against the numpy rule of
tests/threshold_sweep_ref.py, then the sweep end to end: infer.py's device and host passes on tests/golden/fsc147_tiny, and main.py
--calibrate_threshold followed by infer.py --threshold ckpt on the tree of tests/validate_tree.py.  Every comparison is == / array_equal."""
import json
import os

import numpy as np
import pytest
import torch

from counting_detr_amd import ops
from counting_detr_amd import threshold_sweep as ts

import threshold_sweep_ref as ref
import validate_tree as vt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = -7
AP_KEYS = ("AP", "AP50", "AP75", "APs", "APm", "APl")
COUNT_KEYS = ("MAE", "RMSE", "NAE", "SRE")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def thresholds_of(n):
    """n ascending fp32 thresholds; n = 2: two adjacent EQUAL values."""
    if n == 1:
        return np.array([0.5], dtype=np.float32)
    if n == 2:
        return np.array([0.4, 0.4], dtype=np.float32)
    return np.linspace(0.02, 0.98, n).astype(np.float32)


def rows_of(rng, B, Q, thr):
    kinds = ["mixed", "equal", "mixed"][:B] if B > 1 else ["mixed"]
    return np.stack([ref.probe_row(rng, Q, thr, kind=k) for k in kinds])


def run(prob, thr, N=None, first=0):
    """One launch into a sentinel-filled table -> the whole table on the host."""
    B = prob.shape[0]
    table = torch.full((B + first if N is None else N, len(thr)), SENTINEL, dtype=torch.int32, device=DEV)
    ops.count_sweep(T(prob), T(thr), table, first)
    return table.cpu().numpy()


@pytest.mark.parametrize("n_thr", [1, 2, 32])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Q", [1, 63, 64, 65, 300, 4097])
def test_kernel_equals_the_rule(Q, B, n_thr):
    rng = np.random.default_rng(1000 * Q + 10 * B + n_thr)
    thr = thresholds_of(n_thr)
    prob = rows_of(rng, B, Q, thr)
    want = ref.count_table(prob, thr)
    got = run(prob, thr)
    print("Q", Q, "B", B, "T", n_thr, "NaN", int(np.isnan(prob).sum()), "on a threshold", int(np.isin(prob, thr).sum()), "differ", int((got != want).sum()))
    assert got.dtype == np.int32 and np.array_equal(got, want)


def test_the_probe_rows_hold_every_edge():
    """What the cases above are made of, at the sizes where all of it fits: values on a threshold, both fp32 neighbours, 0, 1, NaN, an all-equal row."""
    rng = np.random.default_rng(4)
    for n_thr, Q in ((1, 65), (2, 65), (32, 300), (32, 4097)):
        thr = thresholds_of(n_thr)
        prob = rows_of(rng, 3, Q, thr)
        for t in thr:
            assert (prob[0] == t).any() and (prob[0] == np.nextafter(t, np.float32(-1))).any() and (prob[0] == np.nextafter(t, np.float32(2))).any()
        assert (prob[0] == 0).any() and (prob[0] == 1).any() and np.isnan(prob[0]).any() and (prob[1] == prob[1][0]).all()
        want = ref.count_table(prob, thr)
        assert np.array_equal(run(prob, thr), want)
        assert want[1].max() == Q and (n_thr < 32 or want[1].min() == 0)               # the all-equal row sits ON a threshold: kept there, not above


def test_first_row_offset_leaves_the_other_rows_alone():
    rng = np.random.default_rng(9)
    thr = thresholds_of(32)
    prob = rows_of(rng, 3, 300, thr)
    got = run(prob, thr, N=9, first=4)
    assert np.array_equal(got[4:7], ref.count_table(prob, thr))
    assert (got[:4] == SENTINEL).all() and (got[7:] == SENTINEL).all()


def test_limits_return_the_error_and_touch_nothing():
    rng = np.random.default_rng(2)
    prob = rng.random((2, 70), dtype=np.float32)
    for n_thr, N, first, B in ((33, 4, 0, 2), (4, 4, 3, 2), (4, 4, 0, 0)):
        table = torch.full((N, n_thr), SENTINEL, dtype=torch.int32, device=DEV)
        with pytest.raises(RuntimeError, match="cdetr_count_sweep"):
            ops.count_sweep(T(prob[:B]), T(np.linspace(0.1, 0.9, n_thr).astype(np.float32)), table, first)
        torch.cuda.synchronize()
        assert (table.cpu().numpy() == SENTINEL).all(), (n_thr, N, first, B)


def test_threshold_sweep_store_two_batches_one_copy():
    rng = np.random.default_rng(6)
    given = [0.7, 0.3, 0.5, float(np.nextafter(np.float64(0.3), 1.0)), 0.5]            # unsorted, with fp32 duplicates
    sweep = ops.ThresholdSweep(5, given, DEV)
    assert sweep.thresholds.dtype == np.float32 and sweep.thresholds.tolist() == [ref.widen(0.3), 0.5, ref.widen(0.7)]
    a, b = rows_of(rng, 3, 257, sweep.thresholds), rows_of(rng, 1, 257, sweep.thresholds)
    assert sweep.emit(T(a)) == 0 and sweep.emit(T(b)) == 3
    calls, real = [], torch.Tensor.cpu

    def counted(self, *args, **kw):
        calls.append(1)
        return real(self, *args, **kw)
    torch.Tensor.cpu = counted
    try:
        got = sweep.finish()
        again = sweep.finish()
    finally:
        torch.Tensor.cpu = real
    assert len(calls) == 1 and again is got
    assert got.shape == (4, 3) and np.array_equal(got, ref.count_table(np.concatenate([a, b]), sweep.thresholds))
    sweep.emit(T(b))
    with pytest.raises(RuntimeError, match="ThresholdSweep"):
        sweep.emit(T(b))
    with pytest.raises(RuntimeError, match="ThresholdSweep"):
        ops.ThresholdSweep(5, np.linspace(0, 1, 33), DEV)


# ------------------------------------------------------------------------------------------------------------------ end to end, fsc147_tiny
def _same(a, b):
    return set(a) == set(b) and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a)


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """The passes every end-to-end test reads, run once: the seeded model of tests/test_detections_gpu.py (class bias shifted to the first
    image's median logit), two thresholds taken from the 30 % and 70 % quantiles of the probabilities, then
      host+sweep, device+sweep, device plain at 0.5, device plain at each of the two thresholds."""
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
    # the probabilities the passes below see (the engine's own forward, the same floats pass after pass)
    prob = np.concatenate([engines[0.5](NestedTensor(b["image"].to(DEV), b["mask"].to(DEV)), b["ex_rects"].to(DEV))[4].cpu().numpy() for b in vl])
    lo, hi = (ref.widen(v) for v in np.quantile(prob, [0.3, 0.7]))
    gt_json = os.path.join(args.data_path, "instances_val.json")
    thresholds = ts.parse_spec(f"{lo!r},{hi!r}", 0.5)
    engines.update({t: InferenceEngine(model, t, device=DEV) for t in (lo, hi)})
    root = tmp_path_factory.mktemp("sweep_tiny")
    out = {"thresholds": thresholds, "lo": lo, "hi": hi, "prob": prob, "root": root}

    def one(name, threshold, device_detections, sweep):
        os.makedirs(root / name)
        m, _ = infer_mod.infer(model, criterion, vl, torch.device(DEV), str(root / name), split="val", threshold=threshold,
                               device_detections=device_detections, gt_json=gt_json if device_detections else None, engine=engines[threshold],
                               sweep=ts.Sweep(thresholds, gt_json) if sweep else None)
        out[name] = m
    one("host_sweep", 0.5, False, True)
    one("device_sweep", 0.5, True, True)
    one("device_plain", 0.5, True, False)
    one("device_lo", lo, True, False)
    one("device_hi", hi, True, False)
    return out


def test_device_pass_with_a_sweep_writes_and_reports_what_a_pass_without_it_does(tiny):
    root = tiny["root"]
    with_sweep, plain = (open(root / n / "predictions_val.json", "rb").read() for n in ("device_sweep", "device_plain"))
    assert with_sweep == plain and len(json.loads(plain)["annotations"]) > 0
    assert open(root / "host_sweep" / "predictions_val.json", "rb").read() == plain
    print("with the sweep", tiny["device_sweep"], "without", tiny["device_plain"])
    assert _same(tiny["device_sweep"], tiny["device_plain"]) and all(k in tiny["device_plain"] for k in AP_KEYS + COUNT_KEYS + ("loss_ce", "images"))
    assert not os.path.exists(root / "device_plain" / "threshold_sweep_val.json")
    host = dict(tiny["host_sweep"])                                                      # the host loop itself reports no AP
    assert _same(host, {k: v for k, v in tiny["device_plain"].items() if k not in AP_KEYS})


def test_host_and_device_sweeps_write_equal_reports(tiny):
    root = tiny["root"]
    host, dev = (open(root / n / "threshold_sweep_val.json", "rb").read() for n in ("host_sweep", "device_sweep"))
    print(dev.decode())
    assert host == dev
    rep = json.loads(dev)
    assert rep["thresholds"] == tiny["thresholds"] == [r["threshold"] for r in rep["rows"]] and len(rep["rows"]) == 3
    assert all(set(r) == {"threshold", *COUNT_KEYS, *AP_KEYS} for r in rep["rows"])
    assert set(rep["best"]) == {*COUNT_KEYS, "AP"}
    for key, higher in [(k, False) for k in COUNT_KEYS] + [("AP", True)]:
        win = ref.best(rep["rows"], key, higher)
        assert (rep["best"][key]["threshold"], rep["best"][key]["value"]) == win, key


def test_sweep_rows_equal_separate_plain_passes(tiny):
    rep = json.loads(open(tiny["root"] / "device_sweep" / "threshold_sweep_val.json").read())
    rows = {r["threshold"]: r for r in rep["rows"]}
    prob, lo, hi = tiny["prob"], tiny["lo"], tiny["hi"]
    counts = {t: int(ref.kept(prob, t).sum()) for t in (lo, 0.5, hi)}
    print("kept over the split", counts)
    assert lo < hi and 0.5 not in (lo, hi) and len(set(counts.values())) == 3           # the thresholds really cut the scores at different places
    for name, t in (("device_lo", lo), ("device_plain", 0.5), ("device_hi", hi)):
        plain = tiny[name]
        row = {k: v for k, v in rows[t].items() if k != "threshold"}
        print(t, "sweep row", row, "plain pass", {k: plain[k] for k in row})
        assert _same(row, {k: plain[k] for k in row}), t
    assert len({(rows[t]["MAE"], rows[t]["RMSE"]) for t in (lo, 0.5, hi)}) == 3         # and the counting metrics differ with them
    n_lo, n_hi = (len(json.loads(open(tiny["root"] / n / "predictions_val.json").read())["annotations"]) for n in ("device_lo", "device_hi"))
    assert n_lo == counts[lo] > n_hi == counts[hi]


# ------------------------------------------------------------------------------------------------------------------------- calibration
def test_calibration_goes_into_the_log_and_the_checkpoint_and_infer_reads_it_back(tmp_path):
    import infer as infer_mod
    import main as main_mod
    from counting_detr_amd.args import get_args_parser
    tree = vt.write_tree(tmp_path / "ds")
    out, out_i = tmp_path / "run", tmp_path / "infer"
    # One epoch on this tree leaves every probability of the seeded network between 0.02 and 0.04 (a seeded network gives its queries nearly equal
    # logits): at --threshold 0.02 every query counts, from 0.04 up none does and the MAE is the same -- the tie goes to the threshold nearest 0.5,
    # the sweep's highest, 0.3.  So the calibrated threshold is neither --threshold nor the default, and a pass that did not read it would show.
    run_at, spec = ref.widen(0.02), "0.02:0.3:15"
    common = ["--device", DEV, *vt.MODEL_FLAGS, "--device_detections", "--eval_batch_size", "2", "--sweep_thresholds", spec]
    main_mod.main(get_args_parser().parse_args(["-dp", tree, "-o", str(out), "--images_per_gpu", "2", "--seed", "2", "--epochs", "1", "--eval_every", "1",
                                                "--threshold", "0.02", "--calibrate_threshold", "mae", *common]))
    line = json.loads(open(out / "detr_retrain.txt").read().strip().splitlines()[-1])
    rep = json.loads(open(out / "threshold_sweep_val.json").read())
    keys = list(line)
    print({k: line[k] for k in keys if k.startswith("test_")})
    assert keys[-3:] == ["test_best_threshold", "test_best_mae", "epoch"] and keys[-4].startswith("test_")
    win = ref.best(rep["rows"], "MAE", False)
    print("MAE per threshold", [(r["threshold"], r["MAE"]) for r in rep["rows"]])
    assert (line["test_best_threshold"], line["test_best_mae"]) == win
    assert win[0] not in (0.5, run_at) and win[1] < line["test_MAE"]   # the calibration found something neither --threshold nor the default gives
    at_run = next(r for r in rep["rows"] if r["threshold"] == run_at)
    assert all(line["test_" + k] == at_run[k] or (at_run[k] != at_run[k]) for k in COUNT_KEYS + AP_KEYS)         # the test_* keys stay at --threshold
    ckpt = torch.load(out / "detr_retrain.pth", map_location="cpu", weights_only=False)
    assert ckpt["count_threshold"] == {"metric": "mae", "threshold": win[0], "value": win[1], "epoch": 0}
    assert ckpt["args"].threshold == 0.02 and ckpt["args"].calibrate_threshold == "mae"
    infer_mod.main(get_args_parser().parse_args(["-dp", tree, "-o", str(out_i), "--split", "val", "--resume", str(out / "detr_retrain.pth"),
                                                 "--threshold", "ckpt", *common]))
    m = json.loads(open(out_i / "results_val.txt").read())
    row = next(r for r in rep["rows"] if r["threshold"] == win[0])
    print("infer.py --threshold ckpt", m, "the calibrated row", row)
    assert all(m[k] == row[k] or (m[k] != m[k] and row[k] != row[k]) for k in COUNT_KEYS + AP_KEYS) and m["MAE"] == win[1]
    assert open(out_i / "threshold_sweep_val.json", "rb").read() == open(out / "threshold_sweep_val.json", "rb").read()
