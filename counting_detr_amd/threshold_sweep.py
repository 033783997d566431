"""The counting threshold as something a user can move: the one rule, the `--sweep_thresholds` spec, the per-threshold report and the choice of
the best threshold (infer.py --threshold / --sweep_thresholds, main.py --calibrate_threshold).  Plain numpy / Python, no device.

THE RULE, stated once: a threshold is rounded to fp32 once, `numpy.float32(t)`; a query is kept when the fp32 `prob >= t32`; a NaN
probability is never kept.  For 0.5 this is the rule the project always had.  Everything that carries a threshold around carries the
fp32 value widened to double (`widen`), which every fp32 or fp64 comparison against an fp32 probability treats alike, and reports print it.

On the device the table of counts comes from cdetr_count_sweep (ops.ThresholdSweep), the AP of every threshold from one matching at the
lowest one (coco_ap.summarize_store_sweep); on the host `count_table` and coco_ap.summarize_sweep are the same numbers the slow way.
"""
import math

import numpy as np

MAX_THRESHOLDS = 32                     # cdetr_count_sweep's T
COUNT_KEYS = ("MAE", "RMSE", "NAE", "SRE")
AP_KEYS = ("AP", "AP50", "AP75", "APs", "APm", "APl")
CALIBRATE = {"mae": "MAE", "rmse": "RMSE", "nae": "NAE", "sre": "SRE", "ap": "AP"}


def widen(t):
    """float32(t) as a Python float."""
    t32 = np.float32(t)
    if np.isnan(t32):
        raise ValueError(f"a threshold must be a number, got {t!r}")
    return float(t32)


def kept(prob, t):
    """The rule on an array of probabilities -> bool array."""
    return np.asarray(prob, dtype=np.float32) >= np.float32(t)


def count_table(prob, thresholds):
    """prob [B, Q] -> int32 [B, T]: #{q : prob[b, q] >= float32(thresholds[t])}, the host form of cdetr_count_sweep."""
    prob = np.asarray(prob, dtype=np.float32)
    return np.stack([kept(prob, t).sum(-1) for t in thresholds], axis=-1).astype(np.int32).reshape(prob.shape[0], len(thresholds))


def parse_spec(spec, threshold=None):
    """`--sweep_thresholds SPEC` -> the ascending list of distinct thresholds (fp32 values widened).  SPEC = `lo:hi:n` (n evenly spaced values,
    both ends included) or a comma list; `threshold` (the run's --threshold) is always part of the set; values whose fp32 roundings
    coincide count once; more than 32 distinct values raise."""
    spec = str(spec).strip()
    try:
        if ":" in spec:
            lo, hi, n = spec.split(":")
            n = int(n)
            if n < 1:
                raise ValueError
            values = np.linspace(float(lo), float(hi), n).tolist() if n > 1 else [float(lo)]
        else:
            values = [float(v) for v in spec.split(",") if v.strip()]
    except ValueError:
        raise ValueError(f"--sweep_thresholds {spec!r}: expected lo:hi:n or a comma list of numbers") from None
    if threshold is not None:
        values.append(float(threshold))
    out = sorted({widen(v) for v in values})
    if not out or not all(math.isfinite(v) for v in out):
        raise ValueError(f"--sweep_thresholds {spec!r}: no finite threshold")
    if len(out) > MAX_THRESHOLDS:
        raise ValueError(f"--sweep_thresholds {spec!r}: {len(out)} distinct thresholds, at most {MAX_THRESHOLDS}")
    return out


def column(thresholds, t):
    """Index of threshold `t` in `thresholds` (compared as fp32)."""
    hits = [k for k, v in enumerate(thresholds) if np.float32(v) == np.float32(t)]
    if not hits:
        raise ValueError(f"threshold {t} is not in the sweep {list(thresholds)}")
    return hits[0]


def best(rows):
    """rows (dicts with "threshold" and metrics) -> {metric: {"threshold", "value"}} for MAE / RMSE / NAE / SRE (lowest wins) and, when the rows
    carry it, AP (highest wins).  A NaN never wins; among equal values the threshold nearest 0.5 wins, then the lower one.  A metric that is
    NaN in every row gets threshold None and value NaN."""
    out = {}
    for key, higher in [(k, False) for k in COUNT_KEYS] + [("AP", True)]:
        cand = [(float(r[key]), float(r["threshold"])) for r in rows if key in r and r[key] is not None and float(r[key]) == float(r[key])]
        if not any(key in r for r in rows):
            continue
        if not cand:
            out[key] = {"threshold": None, "value": float("nan")}
            continue
        v, t = min(cand, key=lambda c: (-c[0] if higher else c[0], abs(c[1] - 0.5), c[1]))
        out[key] = {"threshold": t, "value": v}
    return out


def report(thresholds, counts, gt_counts, ap_rows=None):
    """The content of threshold_sweep_<split>.json: `counts` [N, T] (column k = the counts at thresholds[k]), the images' ground-truth counts,
    optionally the six AP numbers per threshold.  The counting metrics are engine.counting_metrics on each column: the floats of the plain loop."""
    from .engine import counting_metrics
    counts = np.asarray(counts).reshape(len(gt_counts), len(thresholds))
    rows = []
    for k, t in enumerate(thresholds):
        row = {"threshold": widen(t)}
        row.update(counting_metrics(counts[:, k].tolist(), gt_counts))
        if ap_rows is not None:
            row.update(ap_rows[k])
        rows.append(row)
    return {"thresholds": [widen(t) for t in thresholds], "rows": rows, "best": best(rows)}


class Sweep:
    """What a pass needs to sweep (`infer.infer(sweep=)`) and what it leaves behind: `thresholds` (parse_spec's list), `gt_json` (the split's
    instances json or None: no AP columns); after the pass `report` (the dict written to threshold_sweep_<split>.json) and `counts` [N, T]."""

    def __init__(self, thresholds, gt_json=None):
        self.thresholds, self.gt_json = [widen(t) for t in thresholds], gt_json
        if self.thresholds != sorted(set(self.thresholds)) or not 1 <= len(self.thresholds) <= MAX_THRESHOLDS:
            raise ValueError(f"Sweep: 1 .. {MAX_THRESHOLDS} distinct ascending thresholds expected, got {self.thresholds}")
        self.report = self.counts = None


def checkpoint_threshold(ckpt, path="the checkpoint"):
    """`--threshold ckpt`: the calibrated threshold a checkpoint carries ("count_threshold": {"metric", "threshold", "value", "epoch"})."""
    entry = ckpt.get("count_threshold") if isinstance(ckpt, dict) else None
    if not entry or entry.get("threshold") is None:
        raise KeyError(f"--threshold ckpt: {path} has no \"count_threshold\" entry (written by main.py --eval_every N --sweep_thresholds SPEC "
                       f"--calibrate_threshold METRIC)")
    return widen(entry["threshold"])


def calibration(report_, metric, epoch):
    """The checkpoint's "count_threshold" entry from a pass's report, or None when the metric has no winner."""
    b = report_["best"].get(CALIBRATE[metric])
    if not b or b["threshold"] is None:
        return None
    return {"metric": metric, "threshold": b["threshold"], "value": b["value"], "epoch": int(epoch)}
