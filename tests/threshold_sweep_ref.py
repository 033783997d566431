"""The counting-threshold rule restated in numpy, the checker of the threshold sweep (cdetr_count_sweep, ops.ThresholdSweep,
coco_ap.summarize_store_sweep, infer.py --threshold / --sweep_thresholds).  Nothing here imports the code under test.

THE RULE: a threshold is rounded to fp32 once, numpy.float32(t); a probability (fp32) is kept when prob >= t32; a NaN probability is never
kept.  Reports print the fp32 threshold widened to double.
"""
import numpy as np


def t32(t):
    return np.float32(t)


def widen(t):
    return float(np.float32(t))


def kept(prob, t):
    """bool array: the rule, element by element (numpy's >= is False for a NaN on either side)."""
    prob = np.asarray(prob)
    assert prob.dtype == np.float32, prob.dtype
    return prob >= t32(t)


def count_table(prob, thresholds):
    """prob fp32 [B, Q] -> int32 [B, T], [b, t] = #{q : prob[b, q] >= float32(thresholds[t])}."""
    prob = np.asarray(prob)
    out = np.zeros((prob.shape[0], len(thresholds)), dtype=np.int32)
    for k, t in enumerate(thresholds):
        out[:, k] = kept(prob, t).sum(axis=1)
    return out


def filter_detections(dt_by_img, t):
    """{image: [detection dicts]} -> the same with the detections whose fp32 score passes the rule, input order kept."""
    return {i: [d for d in dl if kept(np.float32(d["score"]), t)] for i, dl in dt_by_img.items()}


def linspace_spec(lo, hi, n):
    """`lo:hi:n`: n evenly spaced doubles, both ends included, each rounded to fp32; duplicates dropped, ascending, widened."""
    return sorted({widen(v) for v in np.linspace(lo, hi, n)})


def best(rows, key, higher):
    """The winning (threshold, value) of metric `key` over `rows`: NaN never wins, highest / lowest value, ties to the threshold nearest 0.5,
    then to the lower threshold.  None when every value is NaN."""
    win = None
    for r in rows:
        v, t = r[key], r["threshold"]
        if v != v:
            continue
        if win is None:
            win = (t, v)
            continue
        better = v > win[1] if higher else v < win[1]
        if v == win[1]:
            better = abs(t - 0.5) < abs(win[0] - 0.5) or (abs(t - 0.5) == abs(win[0] - 0.5) and t < win[0])
        if better:
            win = (t, v)
    return win


def probe_row(rng, Q, thresholds, kind="mixed"):
    """One row of Q fp32 probabilities built to sit on the rule's edges: values exactly on a threshold, the fp32 neighbours on both sides of
    one, 0, 1 and NaN, the rest uniform in [0, 1); `kind` "equal": every value the same (a threshold's own value)."""
    thr = np.asarray(thresholds, dtype=np.float32)
    if kind == "equal":
        return np.full(Q, thr[len(thr) // 2], dtype=np.float32)
    row = rng.random(Q, dtype=np.float32)
    special = []
    for t in thr:
        special += [t, np.nextafter(t, np.float32(-1)), np.nextafter(t, np.float32(2))]
    special += [np.float32(0), np.float32(1), np.float32("nan")]
    special = np.array(special, dtype=np.float32)
    if Q >= 3 * len(special):                                  # every special value, twice over at random places
        where = rng.choice(Q, size=2 * len(special), replace=False)
        row[where] = np.concatenate([special, special])
    else:                                                      # short rows: as many as fit, drawn at random
        where = rng.choice(Q, size=max(1, Q // 2), replace=False)
        row[where] = rng.choice(special, size=len(where))
    return row
