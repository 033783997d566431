"""cdetr_bootstrap_counts / _gather / _ap (csrc/bootstrap.hip) behind ops.bootstrap_counts / bootstrap_gather / bootstrap_ap,
coco_ap.Matching.bootstrap and --bootstrap, against the numpy rule of counting_detr_amd/bootstrap.py -- which tests/test_bootstrap_cpu.py
pins to the literal expansion (tests/bootstrap_ref.py).  Every comparison is ==; the precision tables and the float sums as float64 BITS."""
import contextlib
import ctypes
import io
import json
import os

import numpy as np
import pytest
import torch

import bootstrap_ref as ref
import eval_split as es
from counting_detr_amd import bootstrap as bs
from counting_detr_amd import coco_ap as ca
from counting_detr_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AREAS = tuple(ca.AREA_RNG)


def T(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))).to(DEV)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def flags(seed, N, D, empty=(), tie=4):
    """Random flags of N images sharing D detections -> (matched, ignored [4, 10, D] bool, dt_score [D], dt_off [N + 1], npig [4, N]); scores are
    multiples of 1 / tie (tie = 1: all equal), descending inside an image; the images of `empty` have no detection."""
    rng = np.random.default_rng(seed)
    owner = np.sort(rng.choice([i for i in range(N) if i not in empty], D)) if D else np.zeros(0, dtype=np.int64)
    dt_off = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=N))])
    score = rng.integers(1, tie + 1, D) / tie
    for b in range(N):
        score[dt_off[b]:dt_off[b + 1]] = -np.sort(-score[dt_off[b]:dt_off[b + 1]])
    npig = rng.integers(0, 4, (4, N))
    npig[0] += 1
    return rng.random((4, 10, D)) < 0.55, rng.random((4, 10, D)) < 0.15, score, dt_off, npig


def check_ap(case, R, seed=0, mult=None, counts=None, chunk=None):
    """One gather and the replicates on the device against the rule -> the rule's precision [R, 4, 10, 101]."""
    matched, ignored, score, dt_off, npig = case
    N = len(dt_off) - 1
    order, image = bs.prepare(score, dt_off, counts)
    words = bs.flag_words(matched, ignored, order)
    m = bs.multiplicities(seed, R, N) if mult is None else np.asarray(mult)
    want = bs.ap_precisions(words, image, npig, m)
    dwords = ops.bootstrap_gather(T(matched, np.uint8), T(ignored, np.uint8), T(order, np.int32))
    assert np.array_equal(dwords.cpu().numpy().view(np.uint32), words)
    got = ops.bootstrap_ap(dwords, T(image, np.int32), T(npig, np.int32), T(ca.REC_THRS), R, seed,
                           mult=None if mult is None else T(mult, np.int32), chunk=chunk)
    assert got.shape == want.shape == (R, 4, 10, 101) and got.dtype == want.dtype
    bad = int((bits(got) != bits(want)).sum())
    print(f"precision: {bad} of {want.size} differ")
    assert bad == 0
    return want


def check_counts(gt, pred, R, seed=0, mult=None):
    m = bs.multiplicities(seed, R, len(gt)) if mult is None else np.asarray(mult)
    S, F = bs.count_sums(gt, pred, m)
    gS, gF = ops.bootstrap_counts(T(gt, np.int32), T(pred, np.int32), R, seed, mult=None if mult is None else T(mult, np.int32), host=True)
    assert gS.dtype == S.dtype and gS.shape == S.shape and np.array_equal(gS, S)
    assert gF.shape == F.shape and np.array_equal(bits(gF), bits(F))
    return S, F


# ----------------------------------------------------------------------------------------------------------- the AP kernel against the rule
@pytest.mark.parametrize("D", [0, 1, 63, 64, 65, 129])
def test_merged_lists_around_the_chunk_of_64(D):
    want = check_ap(flags(D, 5, D), 9, seed=D)
    assert (want[:, 0] >= 0).all()                                       # npig at `all` is positive on every image: never undefined
    if D == 0:
        assert set(np.unique(want)) <= {0.0, -1.0}


@pytest.mark.parametrize("N", [1, 2, 64, 65, 700])
def test_image_counts_around_the_wave_and_above_the_draw_loops_threads(N):
    want = check_ap(flags(N, N, 150, tie=7), 3, seed=11)
    assert (want > 0).any() and (want[want >= 0] <= 1).all()


@pytest.mark.parametrize("R", [1, 33])
def test_replicate_counts_and_a_chunk_boundary(R):
    case = flags(5, 9, 200)
    whole = check_ap(case, R, seed=3)
    if R > 1:
        assert np.array_equal(bits(check_ap(case, R, seed=3, chunk=8)), bits(whole))         # 8 + 8 + 8 + 8 + 1
        assert len({whole[r].tobytes() for r in range(R)}) > R // 2                            # the replicates differ


def test_all_scores_equal_and_images_without_detections_or_ground_truth():
    matched, ignored, score, dt_off, npig = flags(8, 6, 100, empty=(1, 4), tie=1)
    assert len(set(score)) == 1 and dt_off[2] == dt_off[1] and dt_off[5] == dt_off[4]
    npig[:, 2] = 0                                                      # an image with detections and no ground truth
    check_ap((matched, ignored, score, dt_off, npig), 17, seed=1)


def test_large_is_undefined_in_some_replicates_only():
    matched, ignored, score, dt_off, npig = flags(2, 7, 120)
    npig[3] = 0
    npig[3, 0] = 2                                                       # `large` ground truths on image 0 alone
    want = check_ap((matched, ignored, score, dt_off, npig), 33, seed=5)
    undefined = (want[:, 3] == -1).all(axis=(1, 2))
    assert 0 < undefined.sum() < 33 and not (want[:, 0] == -1).any()
    assert np.array_equal(undefined, bs.multiplicities(5, 33, 7)[:, 0] == 0)


def test_explicit_multiplicities_ones_zeros_and_heavy():
    case = flags(4, 5, 140)
    ones = check_ap(case, 1, mult=np.ones((1, 5), dtype=np.int64))
    for a in range(4):                                                   # m == 1: `accumulate` itself
        assert np.array_equal(bits(ones[0, a]), bits(ca.accumulate(case[2], case[0][a], case[1][a], int(case[4][a].sum()))))
    check_ap(case, 3, mult=np.array([[0, 0, 5, 0, 0], [3, 0, 0, 1, 1], [0, 0, 0, 0, 0]]))
    check_ap(case, 2, mult=np.array([[1, 2, 0, 1, 1], [2, 1, 1, 1, 0]]), counts=[3, 0, 1000, 10, 64])      # prefix lengths per image


# -------------------------------------------------------------------------------------------------------------------- the counts kernel
@pytest.mark.parametrize("N, Tc, R", [(1, 1, 1), (2, 32, 3), (64, 1, 33), (65, 32, 5), (700, 3, 9)])
def test_count_sums(N, Tc, R):
    rng = np.random.default_rng(N + Tc)
    gt = rng.integers(0, 400, N)
    gt[rng.random(N) < 0.2] = 0                                          # a ground-truth count of 0: no term in Sn / Ss
    gt[0] = 0 if N > 1 else 3
    S, F = check_counts(gt, rng.integers(0, 500, (N, Tc)), R, seed=N)
    assert (S[..., 1] >= S[..., 0]).all() and np.isfinite(F).all()


def test_count_sums_with_ones_are_counting_metrics_and_a_table_is_read_where_it_lies():
    from counting_detr_amd.engine import counting_metrics
    rng = np.random.default_rng(6)
    gt, pred = rng.integers(0, 90, 40), rng.integers(0, 99, (40, 4))
    S, F = check_counts(gt, pred, 1, mult=np.ones((1, 40), dtype=np.int64))
    got = bs.count_metrics(S, F, 40)
    for c in range(4):
        want = counting_metrics(pred[:, c].tolist(), gt.tolist())
        assert all(got[k][0, c] == want[k] for k in want)
    table = T(pred, np.int32)
    S2, F2 = ops.bootstrap_counts(T(gt, np.int32), table[:, 1:3], 5, 2, host=True)          # two columns of the table, not copied
    w = bs.count_sums(gt, pred[:, 1:3], bs.multiplicities(2, 5, 40))
    assert np.array_equal(S2, w[0]) and np.array_equal(bits(F2), bits(w[1]))
    check_counts(gt, pred, 2, mult=np.array([[0] * 40, [7] + [0] * 38 + [2]]))


# ------------------------------------------------------------------------------------------------------------------------------ the limits
def test_beyond_a_limit_nothing_is_launched_or_written():
    from counting_detr_amd import _ffi
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=DEV)                   # noqa: E731
    null = ctypes.c_void_p(0)
    for N, R, r0 in ((bs.MAX_IMAGES + 1, 1, 0), (4, bs.MAX_REPLICATES + 1, 0), (4, 2, bs.MAX_REPLICATES - 1)):
        out = torch.full((max(R, 1) * 4 * 10 * 101,), -7.0, dtype=torch.float64, device=DEV)
        S = torch.full((max(R, 1) * 2,), -7, dtype=torch.int64, device=DEV)
        rec = T(ca.REC_THRS)
        rc = _ffi.lib().cdetr_bootstrap_ap(None, None, i32(4, N).data_ptr(), None, rec.data_ptr(), 0, r0, R, N, 0, 4, 10, 101, float(np.spacing(1)),
                                           out.data_ptr(), null)
        assert rc == -3 and b"cdetr_bootstrap_ap" in _ffi.lib().cdetr_last_error() and b"limit" in _ffi.lib().cdetr_last_error()
        rc = _ffi.lib().cdetr_bootstrap_counts(i32(N).data_ptr(), i32(N, 1).data_ptr(), 1, None, 0, r0, R, N, 1, S.data_ptr(), out.data_ptr(), null)
        torch.cuda.synchronize()
        assert rc == -3 and b"cdetr_bootstrap_counts" in _ffi.lib().cdetr_last_error()
        assert (out == -7.0).all() and (S == -7).all()
    with pytest.raises(RuntimeError, match="limit 16384"):
        ops.bootstrap_counts(i32(bs.MAX_IMAGES + 1), i32(bs.MAX_IMAGES + 1, 1), 2, 0)
    with pytest.raises(RuntimeError, match="1 .. 10000"):
        ops.bootstrap_ap(i32(4, 0), i32(0), i32(4, 3), T(ca.REC_THRS), bs.MAX_REPLICATES + 1, 0)
    with pytest.raises(RuntimeError, match="rc=-3"):                    # T = 10 exactly: the flag word holds ten bits a side
        ops.bootstrap_gather(torch.zeros((1, 11, 5), dtype=torch.uint8, device=DEV), torch.zeros((1, 11, 5), dtype=torch.uint8, device=DEV), i32(5))


def test_at_the_image_limit():
    case = flags(1, bs.MAX_IMAGES, 300, tie=9)
    check_ap(case, 2, seed=4)
    rng = np.random.default_rng(0)
    check_counts(rng.integers(0, 50, bs.MAX_IMAGES), rng.integers(0, 50, (bs.MAX_IMAGES, 2)), 2, seed=4)


# ------------------------------------------------------------------------------------------------------------------ Matching.bootstrap
def test_matching_on_the_device_equals_the_host_rule_and_the_expansion():
    gt_by, dt_by, ids = ref.random_case(12, n_img=9, big=True)
    host, dev = ca.Matching.of(gt_by, dt_by), ca.Matching.of(gt_by, dt_by, DEV)
    host.image_ids = dev.image_ids = ids                                 # the run's images: two of them are in no pack
    assert len(host.pack["image_ids"]) < len(ids)
    want = host.bootstrap(33, seed=2)
    got = dev.bootstrap(33, seed=2, chunk=16)
    assert got.shape == (33, 6) and np.array_equal(got, want, equal_nan=True)
    assert 0 < np.isnan(want[:, 5]).sum() < 33 and not np.isnan(want[:, 0]).any()
    m = bs.multiplicities(2, 33, len(ids))
    assert np.array_equal(got[7], ref.expanded_six(host, m[7]), equal_nan=True)
    counts = [2, 0, 5, 1, 9, 9, 9, 3, 0]
    assert np.array_equal(dev.bootstrap(5, seed=1, counts=counts), host.bootstrap(5, seed=1, counts=counts), equal_nan=True)
    one = dev.bootstrap(1, mult=np.ones((1, len(ids)), dtype=np.int64))[0]
    assert np.array_equal(one, [dev.six()[k] for k in bs.AP_KEYS], equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------------------ end to end
ROUTES = {"file": [], "store": ["--device_detections"], "host": ["--ap_on_host"]}
VARIANTS = {"alone": [], "sweep": ["--sweep_thresholds", "0.3:0.7:3", "--threshold", "0.5"], "nms": ["--nms_iou", "0.5"],
            "reports": ["--image_report", "--error_report"]}
BOOT = ["--bootstrap", "40", "--bootstrap_seed", "5"]
BOOT_KEYS = [K + s for K in bs.COUNT_KEYS + bs.AP_KEYS for s in ("_lo", "_hi")]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """infer.py on the five-image split of tests/eval_split.py with the seeded model of tests/test_image_report_gpu.py (class bias shifted into
    the gap under the three highest images): every variant on every route with --bootstrap, and the store route without it; each run once."""
    import infer as infer_mod
    from counting_detr_amd import build_model, data
    from counting_detr_amd.args import default_args, get_args_parser
    from counting_detr_amd.misc import NestedTensor
    from oracle.weights import seeded_state_dict
    root = tmp_path_factory.mktemp("bootstrap")
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
    real = {"coco_match": ops.coco_match, "bootstrap_ap": ops.bootstrap_ap, "bootstrap_counts": ops.bootstrap_counts}
    calls = dict.fromkeys(real, 0)

    def counted(fn):
        def call(*a, **kw):
            calls[fn] += 1
            return real[fn](*a, **kw)
        return call
    todo = [("plain", ROUTES["store"])] + [(v + "_" + r, VARIANTS[v] + ROUTES[r] + BOOT) for v in VARIANTS for r in ROUTES]
    for name, extra in todo:
        buf = io.StringIO()
        calls.update(dict.fromkeys(calls, 0))
        try:
            for fn in real:
                setattr(ops, fn, counted(fn))
            with contextlib.redirect_stdout(buf):
                infer_mod.main(get_args_parser().parse_args(common + ["-o", str(root / name)] + extra))
        finally:
            for fn in real:
                setattr(ops, fn, real[fn])
        out[name] = json.loads(buf.getvalue().strip().splitlines()[-1])
        out["launches"][name] = dict(calls)
    return out


def _eq(a, b):
    return a == b or (a != a and b != b)


def _file(runs, name, what="bootstrap_val.json"):
    return open(runs["root"] / name / what, "rb").read()


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_the_three_routes_write_the_same_bytes_and_equal_metrics(runs, variant):
    file, store, host = (variant + "_" + r for r in ROUTES)
    rep = json.loads(_file(runs, store))
    print(variant, rep["metrics"], runs["launches"][store])
    assert _file(runs, file) == _file(runs, store) == _file(runs, host)
    assert set(runs[file]) == set(runs[store]) == set(runs[host]) and list(runs[store])[-20:] == BOOT_KEYS == list(runs[file])[-20:]
    for k in BOOT_KEYS + list(bs.COUNT_KEYS + bs.AP_KEYS) + ["images"]:
        assert _eq(runs[file][k], runs[store][k]) and _eq(runs[host][k], runs[store][k]), k
    assert list(rep)[:6] == ["split", "threshold", "replicates", "seed", "level", "metrics"] and ("sweep" in rep) == (variant == "sweep")
    assert (rep["split"], rep["threshold"], rep["replicates"], rep["seed"], rep["level"]) == ("val", 0.5, 40, 5, 0.95)
    assert list(rep["metrics"]) == list(bs.COUNT_KEYS + bs.AP_KEYS)
    for K, d in rep["metrics"].items():                                  # the file's values ARE the printed metrics
        assert _eq(d["value"], runs[store][K]) and _eq(d["lo"], runs[store][K + "_lo"]) and _eq(d["hi"], runs[store][K + "_hi"]), K
        assert d["undefined"] == 0 if K in bs.COUNT_KEYS else 0 <= d["undefined"] <= 40
    assert rep["metrics"]["MAE"]["lo"] < rep["metrics"]["MAE"]["hi"] and rep["metrics"]["MAE"]["se"] > 0
    assert rep["metrics"]["AP"]["lo"] <= rep["metrics"]["AP"]["hi"] and rep["metrics"]["AP"]["undefined"] < 40


def test_the_replicates_run_in_the_kernels_except_on_the_host_route(runs):
    print(runs["launches"])
    for v in VARIANTS:
        assert runs["launches"][v + "_store"]["bootstrap_ap"] == runs["launches"][v + "_store"]["bootstrap_counts"] == 1, v
        assert runs["launches"][v + "_file"]["bootstrap_ap"] == runs["launches"][v + "_file"]["bootstrap_counts"] == 1, v
        assert runs["launches"][v + "_host"]["bootstrap_ap"] == runs["launches"][v + "_host"]["bootstrap_counts"] == 0, v
        assert runs["launches"][v + "_store"]["coco_match"] == 1, v      # the store's one matching, shared with the reports
    assert runs["launches"]["reports_file"]["coco_match"] == 2          # the file is matched for the AP, and once for both reports and the replicates


def test_the_sweep_section(runs):
    rep = json.loads(_file(runs, "sweep_store"))
    sweep = json.loads(_file(runs, "sweep_store", "threshold_sweep_val.json"))
    rows = rep["sweep"]["rows"]
    assert [r["threshold"] for r in rows] == sweep["thresholds"] and len(rows) == 3
    for row, srow in zip(rows, sweep["rows"]):
        for K in bs.COUNT_KEYS:
            assert row[K]["value"] == srow[K] and list(row[K]) == ["value", "lo", "hi", "delta"] and list(row[K]["delta"]) == ["value", "lo", "hi"]
    assert rows[1]["MAE"]["delta"] == {"value": 0.0, "lo": 0.0, "hi": 0.0} and rows[0]["MAE"]["delta"]["value"] == rows[0]["MAE"]["value"] - rows[1]["MAE"]["value"]
    assert {K: rows[1][K][s] for K in bs.COUNT_KEYS for s in ("value", "lo", "hi")} == \
           {K: rep["metrics"][K][s] for K in bs.COUNT_KEYS for s in ("value", "lo", "hi")}
    for K in bs.COUNT_KEYS:
        best = sweep["best"][K]["threshold"]
        assert rep["sweep"]["best_vs_threshold"][K] == dict(threshold=best, **rows[sweep["thresholds"].index(best)][K]["delta"])
    # AP at the run's threshold reads a prefix of every image of the store emitted at the lowest one: the numbers of the run without the sweep
    assert json.dumps(rep["metrics"]) == json.dumps(json.loads(_file(runs, "alone_store"))["metrics"])


def test_without_the_flag_nothing_changes(runs):
    root = runs["root"]
    assert not os.path.exists(root / "plain" / "bootstrap_val.json")
    assert _file(runs, "plain", "predictions_val.json") == _file(runs, "alone_store", "predictions_val.json")
    with_flag = {k: v for k, v in runs["alone_store"].items() if k not in BOOT_KEYS}
    assert list(with_flag) == list(runs["plain"]) and all(_eq(with_flag[k], runs["plain"][k]) for k in with_flag)
    assert open(root / "plain" / "results_val.txt").read() == json.dumps(runs["plain"]) + "\n"
    assert _file(runs, "reports_store", "image_report_val.json") == _file(runs, "reports_file", "image_report_val.json")
