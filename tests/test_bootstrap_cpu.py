"""counting_detr_amd/bootstrap.py -- the draws, the weighted rule, the tail and the report -- against the literal expansion of
tests/bootstrap_ref.py (the lists repeated by multiplicity, handed to coco_ap.accumulate / _six and engine.counting_metrics), and the
--bootstrap flags.  No device: the kernel is held to this rule by tests/test_bootstrap_gpu.py."""
import json

import numpy as np
import pytest

import bootstrap_ref as ref
from counting_detr_amd import bootstrap as bs
from counting_detr_amd import coco_ap as ca
from counting_detr_amd.engine import counting_metrics


def same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def matching_of(seed, **kw):
    gt_by, dt_by, ids = ref.random_case(seed, **kw)
    m = ca.Matching.of(gt_by, dt_by)
    m.image_ids = ids                                                    # the run's images; those with neither ground truth nor detection are in no pack
    return m


# ------------------------------------------------------------------------------------------------------------------------------ the draws
@pytest.mark.parametrize("seed, r, N", [(0, 0, 1), (0, 0, 7), (1, 0, 7), (0, 9999, 1286), (2 ** 63 - 1, 3, 65), (12345, 17, 16384)])
def test_draws_equal_the_python_int_restatement(seed, r, N):
    d = bs.draws(seed, r, N)
    n = min(N, 300)
    assert d.dtype == np.int64 and d.shape == (N,) and d[:n].tolist() == ref.draws_int(seed, r, N)[:n] and 0 <= d.min() and d.max() < N


def test_multiplicities_sum_to_n_and_depend_on_seed_and_replicate():
    m = bs.multiplicities(3, 40, 1286)
    assert m.shape == (40, 1286) and m.dtype == np.int64 and (m.sum(axis=1) == 1286).all() and (m >= 0).all()
    assert np.array_equal(m, bs.multiplicities(3, 40, 1286)) and np.array_equal(m[5:9], bs.multiplicities(3, 4, 1286, first=5))
    assert len({row.tobytes() for row in m}) == 40 and not np.array_equal(m[0], bs.multiplicities(4, 1, 1286)[0])
    assert bs.draws(3, 1, 50).tolist() != bs.draws(3, 2, 50).tolist() != bs.draws(4, 2, 50).tolist()
    assert abs(m.mean() - 1) < 1e-12 and 0.9 < m.var() < 1.1         # Poisson-like: mean 1 exactly, variance 1 - 1 / N


# ------------------------------------------------------------------------------------------------------------------- the counting metrics
def test_with_ones_the_counting_metrics_are_counting_metrics():
    rng = np.random.default_rng(0)
    gt, pred = rng.integers(0, 3800, 60), rng.integers(0, 4000, (60, 5))
    gt[[3, 17]] = 0
    S, F = bs.count_sums(gt, pred, np.ones((1, 60), dtype=np.int64))
    got = bs.count_metrics(S, F, 60)
    for c in range(5):
        want = counting_metrics(pred[:, c].tolist(), gt.tolist())
        assert all(got[k][0, c] == want[k] for k in want), (c, want)


def test_counting_replicates_against_the_expanded_image_list():
    """MAE and RMSE are integer sums: EQUAL to counting_metrics on the repeated list.  NAE and SRE add float64 terms: the rule adds m * q once,
    the repeated list adds q m times, each a sum of at most 2N roundings of relative size 2^-53 on non-negative terms."""
    rng = np.random.default_rng(1)
    N = 50
    gt, pred = rng.integers(0, 200, N), rng.integers(0, 220, N)
    gt[4] = 0
    m = bs.multiplicities(9, 12, N)
    m[0] = 1
    m[1, :] = 0
    m[1, 7] = N                                                          # one image drawn N times
    S, F = bs.count_sums(gt, pred, m)
    got = bs.count_metrics(S, F, N)
    for r in range(12):
        want = ref.expanded_counting(gt, pred, m[r])
        assert got["MAE"][r, 0] == want["MAE"] and got["RMSE"][r, 0] == want["RMSE"]
        for k in ("NAE", "SRE"):
            assert abs(got[k][r, 0] - want[k]) <= 2 * N * 2.0 ** -53 * want[k]
    assert all(got[k][0, 0] == counting_metrics(pred.tolist(), gt.tolist())[k] for k in got)
    values, reps = bs.counting(gt, pred, 12, 9)
    assert values["MAE"].shape == (1,) and reps["SRE"].shape == (12, 1) and values["NAE"][0] == counting_metrics(pred.tolist(), gt.tolist())["NAE"]
    assert np.array_equal(reps["MAE"], bs.count_metrics(*bs.count_sums(gt, pred, bs.multiplicities(9, 12, N)), N)["MAE"])


# ---------------------------------------------------------------------------------------------------------------------------------- AP
@pytest.mark.parametrize("seed", range(6))
def test_with_ones_the_six_numbers_are_six(seed):
    m = matching_of(seed)
    one = m.bootstrap(1, mult=np.ones((1, len(m.image_ids)), dtype=np.int64))
    assert one.shape == (1, 6) and same(one[0], [m.six()[k] for k in bs.AP_KEYS])


@pytest.mark.parametrize("seed", range(12))
def test_the_rule_equals_the_expansion(seed):
    """Score ties (scores are quarters), images without detections, without ground truth and with neither, weights 0 and >= 2."""
    m = matching_of(100 + seed, n_img=7 + seed % 3, ties=seed % 4 != 3)
    N, R = len(m.image_ids), 10
    mult = bs.multiplicities(seed, R, N)
    assert (mult == 0).any() and (mult >= 2).any() and len(m.pack["image_ids"]) < N
    got = m.bootstrap(R, seed=seed)
    for r in range(R):
        assert same(got[r], ref.expanded_six(m, mult[r])), (seed, r)
    hand = np.array([[0] * N, [3] + [0] * (N - 1), [2] * N])
    got = m.bootstrap(3, mult=hand)
    for r in range(3):
        assert same(got[r], ref.expanded_six(m, hand[r]))
    assert np.isnan(got[0]).all()                                        # no image drawn: no ground truth anywhere


def test_the_precision_tables_equal_the_expansion_bit_for_bit_with_prefix_lengths():
    m = matching_of(31, n_img=8)
    N = len(m.image_ids)
    counts = [3, 0, 100, 1, 2, 5, 4, 0]
    order, image = bs.prepare(m.pack["dt_score"], m.pack["dt_off"], m.pack_counts(counts))
    slot = {i: k for k, i in enumerate(m.image_ids)}
    at = np.array([slot[i] for i in m.pack["image_ids"]])
    matched, ignored, npig = m.host()
    npig_n = np.zeros((4, N), dtype=np.int64)
    npig_n[:, at] = npig
    mult = bs.multiplicities(5, 6, N)
    got = bs.ap_precisions(bs.flag_words(matched, ignored, order), at[image], npig_n, mult)
    for r in range(6):
        want = ref.expanded_precision(m, mult[r], counts)
        assert got[r].shape == want.shape == (4, 10, 101) and np.array_equal(got[r].view(np.int64), want.view(np.int64))
    assert same(m.bootstrap(6, seed=5, counts=counts)[2], ref.expanded_six(m, mult[2], counts))


def test_large_is_undefined_in_some_replicates_and_all_in_none():
    m = matching_of(12, n_img=9, big=True)                               # ground truths of the range `large` on the first image alone
    got = m.bootstrap(33, seed=2)
    undefined = np.isnan(got[:, 5])
    assert 0 < undefined.sum() < 33 and not np.isnan(got[:, 0]).any()
    assert np.array_equal(undefined, bs.multiplicities(2, 33, 9)[:, 0] == 0)
    d = bs.interval(m.six()["APl"], got[:, 5])
    assert d["undefined"] == int(undefined.sum()) and d["lo"] <= d["hi"] and d["value"] == m.six()["APl"]
    assert bs.interval(m.six()["AP"], got[:, 0])["undefined"] == 0


# ------------------------------------------------------------------------------------------------------------------------------ the tail
def test_the_tail():
    v = np.array([3.0, 1.0, np.nan, 2.0, 10.0])
    d = bs.interval(7.5, v)
    lo, hi = np.quantile([3.0, 1.0, 2.0, 10.0], [0.025, 0.975], method="linear")
    assert d == {"value": 7.5, "lo": float(lo), "hi": float(hi), "se": float(np.std([3.0, 1.0, 2.0, 10.0], ddof=1)), "undefined": 1}
    one = bs.interval(1.0, [np.nan, 4.0])
    assert one["undefined"] == 1 and one["value"] == 1.0 and all(np.isnan(one[k]) for k in ("lo", "hi", "se"))
    none = bs.interval(float("nan"), [])
    assert none["undefined"] == 0 and np.isnan(none["lo"])
    flat = bs.interval(2.0, [2.0] * 9)
    assert flat["lo"] == flat["hi"] == 2.0 and flat["se"] == 0.0


def test_the_report_and_the_sweeps_paired_differences():
    from counting_detr_amd import threshold_sweep as ts
    rng = np.random.default_rng(2)
    N, R, thresholds = 30, 25, [ts.widen(t) for t in (0.3, 0.5, 0.7)]
    gt = rng.integers(1, 60, N)
    table = np.stack([gt + rng.integers(0, 9, N), gt + rng.integers(-2, 3, N), gt - rng.integers(0, 6, N)], axis=1).clip(0)
    values, reps = bs.counting(gt, table, R, 4)
    sweep = ts.report(thresholds, table, gt.tolist())
    sec = bs.sweep_section(thresholds, 0.5, values, reps, sweep["best"])
    assert [r["threshold"] for r in sec["rows"]] == thresholds
    for k, row in enumerate(sec["rows"]):
        for K in bs.COUNT_KEYS:
            assert row[K]["value"] == sweep["rows"][k][K] and list(row[K]) == ["value", "lo", "hi", "delta"]
            paired = bs.interval(values[K][k] - values[K][1], reps[K][:, k] - reps[K][:, 1])
            assert row[K]["delta"] == {x: paired[x] for x in ("value", "lo", "hi")}
        assert row["MAE"]["delta"] == ({"value": 0.0, "lo": 0.0, "hi": 0.0} if k == 1 else row["MAE"]["delta"])
    # paired: the interval of the difference is NOT the difference of the intervals
    row = sec["rows"][0]["MAE"]
    assert row["delta"]["lo"] != row["lo"] - sec["rows"][1]["MAE"]["lo"]
    best_t = sweep["best"]["MAE"]["threshold"]
    assert sec["best_vs_threshold"]["MAE"] == dict(threshold=best_t, **sec["rows"][ts.column(thresholds, best_t)]["MAE"]["delta"])
    rep = bs.report("val", 0.5, R, 4, {K: values[K][1] for K in bs.COUNT_KEYS}, {K: reps[K][:, 1] for K in bs.COUNT_KEYS}, sec)
    assert list(rep) == ["split", "threshold", "replicates", "seed", "level", "metrics", "sweep"] and rep["level"] == 0.95
    assert list(rep["metrics"]) == list(bs.COUNT_KEYS) and list(rep["metrics"]["MAE"]) == ["value", "lo", "hi", "se", "undefined"]
    assert rep["metrics"]["MAE"]["value"] == counting_metrics(table[:, 1].tolist(), gt.tolist())["MAE"]
    assert rep["metrics"]["MAE"]["lo"] <= rep["metrics"]["MAE"]["value"] <= rep["metrics"]["MAE"]["hi"]
    assert bs.metrics(rep) == {K + s: rep["metrics"][K][s[1:]] for K in bs.COUNT_KEYS for s in ("_lo", "_hi")}
    json.dumps(rep)


def test_the_pass_object_on_host_flags():
    """infer.Bootstrap on the host route: counting intervals alone, with AP from a matching, and with a sweep."""
    import infer
    from counting_detr_amd import threshold_sweep as ts
    m = matching_of(12, n_img=9, big=True)
    ids = m.image_ids
    gt_counts = [len(ref.random_case(12, n_img=9, big=True)[0].get(i, [])) for i in ids]
    pred_counts = [len(ref.random_case(12, n_img=9, big=True)[1].get(i, [])) for i in ids]
    b = infer.Bootstrap(20, 3)
    b.split = "val"
    got = b.run(ids, gt_counts, pred_counts, 0.5)
    assert list(got) == [K + s for K in bs.COUNT_KEYS for s in ("_lo", "_hi")] and list(b.report["metrics"]) == list(bs.COUNT_KEYS)
    assert b.report["metrics"]["MAE"]["value"] == counting_metrics(pred_counts, gt_counts)["MAE"] and "sweep" not in b.report
    got = b.run(ids, gt_counts, pred_counts, 0.5, matching=m)
    assert list(b.report["metrics"]) == list(bs.COUNT_KEYS + bs.AP_KEYS) and len(got) == 20
    six = m.six()
    assert all(same(b.report["metrics"][K]["value"], six[K]) for K in bs.AP_KEYS) and b.report["metrics"]["APl"]["undefined"] > 0
    assert b.report["replicates"] == 20 and b.report["seed"] == 3 and b.report["split"] == "val"
    sweep = ts.Sweep([0.25, 0.5])
    sweep.counts = np.stack([np.asarray(pred_counts) + 2, pred_counts], axis=1)
    sweep.report = ts.report(sweep.thresholds, sweep.counts, gt_counts)
    with_sweep = b.run(ids, gt_counts, pred_counts, 0.5, matching=m, sweep=sweep)
    assert with_sweep == got or all(same(with_sweep[k], got[k]) for k in got)              # the run's own threshold: the same replicates
    assert len(b.report["sweep"]["rows"]) == 2 and b.report["sweep"]["rows"][1]["MAE"]["delta"]["hi"] == 0.0


# ----------------------------------------------------------------------------------------------------------------------------- the flags
def test_argument_parsing(capsys):
    from counting_detr_amd.args import default_args, get_args_parser
    p = get_args_parser()
    base = ["-dp", "x"]
    ns = p.parse_args(base)
    assert not hasattr(ns, "bootstrap") and not hasattr(ns, "bootstrap_seed") and not hasattr(default_args(), "bootstrap")
    ns = p.parse_args(base + ["--bootstrap", "1000"])
    assert ns.bootstrap == 1000 and not hasattr(ns, "bootstrap_seed")
    ns = p.parse_args(base + ["--bootstrap", "1", "--bootstrap_seed", "7"])
    assert (ns.bootstrap, ns.bootstrap_seed) == (1, 7)
    assert p.parse_args(base + ["--bootstrap", "10000"]).bootstrap == 10000
    for bad in (["--bootstrap", "0"], ["--bootstrap", "10001"], ["--bootstrap", "-3"], ["--bootstrap", "1.5"], ["--bootstrap_seed", "7"],
                ["--bootstrap", "5", "--bootstrap_seed", "-1"]):
        with pytest.raises(SystemExit):
            p.parse_args(base + bad)
        assert "bootstrap" in capsys.readouterr().err
    with pytest.raises(ValueError, match="1 .. 10000"):
        bs.check_args(10001)
    import infer
    by_hand = default_args()
    by_hand.bootstrap_seed = 3                                           # a namespace built by hand meets the check when the pass is built
    with pytest.raises(ValueError, match="--bootstrap_seed needs --bootstrap"):
        infer.build_bootstrap(by_hand)
    assert infer.build_bootstrap(default_args()) is None
