"""Bootstrap confidence intervals over images for the counting metrics and box AP: THE RULE, stated once in numpy (no torch, no device), the
tail that turns replicates into intervals and the report written to bootstrap_<split>.json (infer.py / main.py --bootstrap R).

A replicate r of a split of N images draws N images with replacement; `draws` is a counter-based, integer-only generator (a splitmix64
finaliser of (seed, r, j), multiply-shift into 0 .. N - 1) that csrc/bootstrap.hip restates bit for bit, and its constants are written
HERE and nowhere else in Python.  `multiplicities` are the bincounts m[r, i], sum_i m[r, i] = N.  Replicate r uses the SAME m[r] for every
metric, so replicates are paired across metrics and across the thresholds of a sweep.

COUNTING METRICS (`count_sums`, `count_metrics`): with the integer err_i = |gt_i - pred_i| a replicate's sums are S1 = sum m_i err_i and
S2 = sum m_i err_i^2 (int64) and Sn = sum m_i (err_i / gt_i), Ss = sum m_i (err_i^2 / gt_i) (float64: every term is the product of the integer
weight and ONE division, 0 where gt_i == 0, and the terms are added one by one in image order).  The host forms MAE / RMSE / NAE / SRE from the
four sums with the expressions of engine.counting_metrics, the power ** 0.5 included; with m == 1 the result EQUALS counting_metrics.

AP (`prepare`, `ap_precision`): every detection is accumulated ONCE with weight m[its image]: cumulative tp / fp are integer weighted prefix
sums over the merged order, npig_r = sum m_i npig[a, i], positions of weight 0 are dropped and the tail is coco_ap._sample unchanged.  That
EQUALS coco_ap.accumulate on the literally duplicated lists (numpy.repeat of the merged order by weight): a copy of a detection only adds
positions whose precision is dominated, at equal or higher recall, by a position the weighted list already holds (tests/bootstrap_ref.py
is that expansion).  A replicate whose npig_r is 0 for an area range has that number undefined (-1 -> NaN, as today).

THE TAIL (`interval`): value = the run's own number; lo / hi = numpy.quantile(v, [a/2, 1 - a/2], method="linear") over the defined replicates
at level 0.95; se = numpy.std(v, ddof=1); undefined = the replicates dropped; lo / hi / se NaN with fewer than 2 defined.
"""
import numpy as np

GOLDEN = 0x9E3779B97F4A7C15             # splitmix64: the increment, and the seed's multiplier
MIX1 = 0xBF58476D1CE4E5B9
MIX2 = 0x94D049BB133111EB
MAX_IMAGES = 16384                      # csrc/bootstrap.hip: the multiplicities of one replicate are 64 KB of LDS
MAX_REPLICATES = 10000
LEVEL, ALPHA = 0.95, 0.05               # the level reported, and the a of the quantiles a / 2 and 1 - a / 2
COUNT_KEYS = ("MAE", "RMSE", "NAE", "SRE")
AP_KEYS = ("AP", "AP50", "AP75", "APs", "APm", "APl")


def check_args(R, seed=0):
    """The limits every route shares -> (R, seed) as ints."""
    R, seed = int(R), int(seed)
    if not 1 <= R <= MAX_REPLICATES:
        raise ValueError(f"bootstrap: R = {R} replicates, 1 .. {MAX_REPLICATES} expected")
    if not 0 <= seed < 2 ** 63:
        raise ValueError(f"bootstrap: seed = {seed}, 0 .. 2^63 - 1 expected")
    return R, seed


def draws(seed, r, N):
    """The N image indices replicate `r` draws under `seed` -> int64 [N].  uint64 arithmetic modulo 2^64 throughout."""
    with np.errstate(over="ignore"):
        x = np.full(N, (int(seed) * GOLDEN) % 2 ** 64, dtype=np.uint64) ^ (np.uint64(int(r) << 32) | np.arange(N, dtype=np.uint64))
        x = x + np.uint64(GOLDEN)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(MIX1)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(MIX2)
        x = x ^ (x >> np.uint64(31))
        return (((x >> np.uint64(32)) * np.uint64(N)) >> np.uint64(32)).astype(np.int64)


def multiplicities(seed, R, N, first=0):
    """-> int64 [R, N]: how often replicate first + r draws image i."""
    return np.stack([np.bincount(draws(seed, first + r, N), minlength=N) for r in range(R)]).reshape(R, N).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------------ counting metrics
def count_sums(gt, pred, m):
    """gt [N], pred [N, Tc] integer counts, m [R, N] -> (S int64 [R, Tc, 2] = S1, S2; F float64 [R, Tc, 2] = Sn, Ss)."""
    gt = np.asarray(gt, dtype=np.int64).reshape(-1)
    N = len(gt)
    pred, m = np.asarray(pred, dtype=np.int64).reshape(N, -1), np.asarray(m, dtype=np.int64).reshape(-1, N)
    err = np.abs(gt[:, None] - pred)
    S = np.stack([m @ err, m @ (err * err)], axis=-1)
    has = (gt > 0)[:, None]
    den = np.where(has, gt[:, None], 1).astype(np.float64)
    qn = np.where(has, err.astype(np.float64) / den, 0.0)
    qs = np.where(has, (err * err).astype(np.float64) / den, 0.0)
    F = np.zeros((m.shape[0], pred.shape[1], 2))
    mf = m.astype(np.float64)
    for i in range(N):                                  # image order: the sums are float64 and not associative
        F[:, :, 0] = F[:, :, 0] + mf[:, i, None] * qn[i][None, :]
        F[:, :, 1] = F[:, :, 1] + mf[:, i, None] * qs[i][None, :]
    return S, F


def count_metrics(S, F, N):
    """The four sums -> {"MAE", "RMSE", "NAE", "SRE"}: float64 arrays shaped like S[..., 0], by engine.counting_metrics' expressions (Python's
    own float power, one element at a time: numpy's array power takes another route for 0.5)."""
    S, F = np.asarray(S), np.asarray(F)
    shape = S.shape[:-1]
    s1, s2, sn, ss = S[..., 0].reshape(-1).tolist(), S[..., 1].reshape(-1).tolist(), F[..., 0].reshape(-1).tolist(), F[..., 1].reshape(-1).tolist()
    arr = lambda v: np.array(v, dtype=np.float64).reshape(shape)                  # noqa: E731
    return {"MAE": arr([float(a) / N for a in s1]), "RMSE": arr([(float(a) / N) ** 0.5 for a in s2]),
            "NAE": arr([a / N for a in sn]), "SRE": arr([(a / N) ** 0.5 for a in ss])}


# ---------------------------------------------------------------------------------------------------------------------------------- AP
def prepare(dt_score, dt_off, counts=None):
    """The merged order of a pack's detections, computed once -> (order int64 [P]: indices into the pack's detections by descending score,
    stable, those beyond an image's prefix length counts[b] left out; image int64 [P]: the pack image of every position)."""
    dt_off = np.asarray(dt_off, dtype=np.int64)
    image = np.repeat(np.arange(len(dt_off) - 1), np.diff(dt_off))
    order = np.argsort(-np.asarray(dt_score, dtype=np.float64), kind="mergesort")
    if counts is not None:
        rank = np.arange(len(image)) - dt_off[image]
        order = order[(rank < np.maximum(np.asarray(counts, dtype=np.int64), 0)[image])[order]]
    return order, image[order]


def flag_words(matched, ignored, order):
    """matched / det_ignored [A, T, D] -> uint32 [A, P] in merged order: bit t = a true positive at IoU threshold t (matched, not ignored),
    bit 16 + t = a false positive (unmatched, not ignored); the form the kernel streams."""
    matched, ignored = np.asarray(matched, dtype=bool)[:, :, order], np.asarray(ignored, dtype=bool)[:, :, order]
    T = matched.shape[1]
    sh = np.arange(T, dtype=np.uint32)[None, :, None]
    tp = ((matched & ~ignored).astype(np.uint32) << sh).sum(axis=1, dtype=np.uint32)
    fp = ((~matched & ~ignored).astype(np.uint32) << (sh + np.uint32(16))).sum(axis=1, dtype=np.uint32)
    return (tp | fp).reshape(matched.shape[0], len(order))


def ap_precision(words, image, npig, m, T=10):
    """ONE replicate: words uint32 [A, P] (`flag_words`), image [P], npig [A, B], m [B] -> precision float64 [A, T, 101], -1 where npig_r is 0."""
    from .coco_ap import REC_THRS, _sample
    words, npig, m = np.asarray(words, dtype=np.uint32), np.asarray(npig, dtype=np.int64), np.asarray(m, dtype=np.int64)
    A = words.shape[0]
    w = m[np.asarray(image, dtype=np.int64)]
    keep = w > 0
    out = -np.ones((A, T, len(REC_THRS)))
    sh = np.arange(T, dtype=np.uint32)[:, None]
    for a in range(A):
        npig_r = int((m * npig[a]).sum())
        if npig_r == 0:
            continue
        tp = ((words[a][None, :] >> sh) & np.uint32(1)).astype(np.int64) * w
        fp = ((words[a][None, :] >> (sh + np.uint32(16))) & np.uint32(1)).astype(np.int64) * w
        out[a] = _sample(np.cumsum(tp, axis=1)[:, keep].astype(np.float64), np.cumsum(fp, axis=1)[:, keep].astype(np.float64), npig_r)
    return out


def ap_precisions(words, image, npig, m):
    """`ap_precision` per row of m [R, B] -> [R, A, T, 101]: the numpy route (slow: every replicate re-accumulates the split)."""
    m = np.asarray(m, dtype=np.int64).reshape(-1, np.asarray(npig).shape[1])
    return np.stack([ap_precision(words, image, npig, m[r]) for r in range(len(m))]) if len(m) else np.zeros((0, len(words), 10, 101))


def six_table(precision, areas):
    """precision [R, A, T, 101] under the area ranges `areas` -> float64 [R, 6] in AP_KEYS order (coco_ap._six; NaN where undefined)."""
    from .coco_ap import _six
    out = np.empty((len(precision), len(AP_KEYS)))
    for r, p in enumerate(precision):
        six = _six(dict(zip(areas, p)))
        out[r] = [six[k] for k in AP_KEYS]
    return out


# ------------------------------------------------------------------------------------------------------------------------------ the tail
def interval(value, v, alpha=ALPHA):
    """The run's own `value` and its replicates v [R] -> {"value", "lo", "hi", "se", "undefined"}."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    ok = v[~np.isnan(v)]
    out = {"value": float(value), "lo": float("nan"), "hi": float("nan"), "se": float("nan"), "undefined": int(len(v) - len(ok))}
    if len(ok) >= 2:
        lo, hi = np.quantile(ok, [alpha / 2, 1 - alpha / 2], method="linear")
        out.update(lo=float(lo), hi=float(hi), se=float(np.std(ok, ddof=1)))
    return out


def _three(d):
    return {k: d[k] for k in ("value", "lo", "hi")}


def sweep_section(thresholds, threshold, values, reps, best=None):
    """The "sweep" entry: thresholds [Tc], the run's `threshold` (one of them), values / reps = {K: [Tc] / [R, Tc]} for the counting metrics ->
    {"rows": [{"threshold", K: {value, lo, hi, "delta": {value, lo, hi}}}], "best_vs_threshold": {K: delta at best[K]["threshold"]}}.  `delta`
    = the metric minus the metric at the run's threshold, replicate by replicate: the replicates are paired."""
    from .threshold_sweep import column
    c0 = column(thresholds, threshold)
    rows = []
    for k, t in enumerate(thresholds):
        row = {"threshold": float(t)}
        for K in COUNT_KEYS:
            v, rep = np.asarray(values[K], dtype=np.float64), np.asarray(reps[K], dtype=np.float64)
            row[K] = dict(_three(interval(v[k], rep[:, k])), delta=_three(interval(v[k] - v[c0], rep[:, k] - rep[:, c0])))
        rows.append(row)
    out = {"rows": rows, "best_vs_threshold": {}}
    for K in COUNT_KEYS:
        b = (best or {}).get(K)
        if b and b.get("threshold") is not None:
            out["best_vs_threshold"][K] = dict(threshold=float(b["threshold"]), **rows[column(thresholds, b["threshold"])][K]["delta"])
    return out


def report(split, threshold, R, seed, values, reps, sweep=None):
    """What --bootstrap writes to bootstrap_<split>.json: values = {K: the run's number}, reps = {K: [R] replicates} ->
    {"split", "threshold", "replicates", "seed", "level", "metrics": {K: `interval`}} (+ "sweep": `sweep_section`)."""
    out = {"split": split, "threshold": float(threshold), "replicates": int(R), "seed": int(seed), "level": LEVEL,
           "metrics": {K: interval(values[K], reps[K]) for K in values}}
    if sweep is not None:
        out["sweep"] = sweep
    return out


def metrics(report_):
    """The keys the run's metrics gain: <K>_lo / <K>_hi."""
    out = {}
    for K, d in report_["metrics"].items():
        out[K + "_lo"], out[K + "_hi"] = d["lo"], d["hi"]
    return out


def counting(gt, pred, R, seed, device_sums=None, mult=None):
    """Counting metrics of gt [N] / pred [N, Tc] and their replicates -> ({K: [Tc]}, {K: [R, Tc]}).  `device_sums`: a callable (gt, pred, R, seed,
    mult) -> (S, F) that launches the kernel instead of `count_sums`; `mult`: an explicit [R, N] table in place of the draws (tests)."""
    gt = np.asarray(gt, dtype=np.int64).reshape(-1)
    N = len(gt)
    pred = np.asarray(pred, dtype=np.int64).reshape(N, -1)
    S, F = count_sums(gt, pred, np.ones((1, N), dtype=np.int64))
    values = {K: v[0] for K, v in count_metrics(S, F, N).items()}
    if device_sums is not None:
        S, F = device_sums(gt, pred, R, seed, mult)
    else:
        S, F = count_sums(gt, pred, multiplicities(seed, R, N) if mult is None else mult)
    return values, count_metrics(S, F, N)
