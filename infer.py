"""infer.py -- the reference's inference driver (A2/infer.py:27-122) + the counting part of its evaluator
(A2/eval_all.py:141-279) on the MI355X path.

For every image of the val / test split: forward, losses (logged), the counting rule `sigmoid(logit[..., 0]) >= 0.5`,
predictions written in the reference's wire format (COCO-style json: bbox = [cx, cy, w, h] ints in original pixels, `point` =
the query's reference point, one `images` entry per image) to <output_dir>/predictions_<split>.json, then MAE / RMSE / NAE /
SRE of the predicted counts against the ground-truth instance counts, and -- when the split's `instances_<split>.json` is there -- the box AP /
AP50 / AP75 / APs / APm / APl of A2/eval_all.py:285-331 from a dependency-free restatement of pycocotools' COCOeval
(counting_detr_amd/coco_ap.py; parity unpinned: there is no pycocotools in this image to check it against).  On a CUDA device the AP's
matching runs there (one cdetr_coco_match launch for the split); `--ap_on_host` keeps the interpreted host path, which gives the same numbers.

`--device_detections` (off by default; the host loop stays the checker): the detections leave the forward in the form the matcher reads.  One
cdetr_emit_detections call per image appends its wire records (the json's fields) and its evaluation records (reference_box + COCOeval's order) to
a device-resident store, the losses go to a device buffer, and nothing is copied or awaited inside the loop; after it, one copy of the store
writes the SAME predictions json byte for byte and the AP is matched from device memory without re-reading that file.

`--eval_batch_size B` (default 1: the loop above, one image per forward): the split is walked in batches of B images of ONE resized size
(data.SizeBucketBatchSampler: a padded image is not the image alone -- the key means run over padded cells), in bucket order.  The logged
losses stay what they are at batch 1, per-image quantities averaged over the split: `SetCriterion.per_image` gives every image the losses it
would get alone (one batched match + one cdetr_criterion_eval launch per batch), where the batched `forward` would normalise by the batch's
target count.  The json lists the images in the order they were run; AP and the counting metrics do not depend on it.

`--threshold T` (default 0.5) moves the counting rule's bar: `prob >= float32(T)` in fp32, a NaN never kept (threshold_sweep.py states the rule);
`--threshold ckpt` takes the threshold main.py --calibrate_threshold left in the --resume checkpoint.  `--sweep_thresholds SPEC` (lo:hi:n or a
comma list, at most 32 values, --threshold included) reports the counting metrics and the AP at every threshold from the SAME pass into
threshold_sweep_<split>.json ({"thresholds", "rows", "best"}); everything else the run writes and prints stays what it is without the flag.  On
the device path the store is emitted at the lowest threshold, one cdetr_count_sweep launch per batch counts every threshold, and ONE matching
gives every threshold's AP (the detections kept at a higher threshold are a prefix of the evaluation order: coco_ap.accumulate_sweep); on
the host path the same report comes from numpy and coco_ap.summarize_sweep, the slow checker.

`--image_report` says on WHICH images the model fails (the per-image list the reference's evaluator pickles, A2/eval_all.py:227-239, with the `ap`
field its line 181 left empty, and COCOeval's six recall numbers beside the six AP): the metrics gain AR900 / AR1000 / AR1100 / ARs / ARm / ARl
and image_report_<split>.json appears beside the predictions file ({"split", "threshold", "max_dets", "AR", "rows", "order_by_ap",
"order_by_diff"}; a row = image_id, count_gt, count_pred, diff, the image's own AP / AP50 / AP75 / APs / APm / APl, tp50 / fp50 / fn50).  On the
device path the flags of the split's one matching go through ONE cdetr_coco_image_stats launch where they lie; every other run forms the
same numbers from one matching of the written predictions (coco_ap.match_predictions; `--ap_on_host`: its host code, the checker).  With --sweep_thresholds the
report describes the run's own --threshold.  Without the flag nothing changes.

`--render_worst K` / `--render_ids 3,17` (both need --image_report; an error at start-up otherwise) SHOW those images -- the step the reference's
evaluators left half alive (`visualize_res` draws boxes, centres and ground truths with cv2 and its imwrite is commented out,
L2/offline_lvis_evaluator.py:167-207): render_<split>/<image_id>.png for the K images of lowest AP, the K of largest count error and the ids named,
and render_<split>/index.json ({"split", "threshold", "style", "dot", "images": [{"image_id", "file_name", "png", "reasons", "row"}]}), wherever the
predictions file is written.  Detections are green (true positive at IoU 0.5), red (false positive) or grey (ignored) with a centre dot, ground
truths blue, exemplars yellow; counting_detr_amd/render.py states the integer rule.  `--ap_on_host` draws with its numpy implementation from the
written predictions and the host matcher's flags (the checker); any other host-loop run matches the predictions on the device and draws there; with
`--device_detections` ONE cdetr_render_boxes launch reads the store's boxes and the flags of the split's one matching where they lie -- only the
chosen images' pixels go up, only the overlays come back.  Same PNG bytes on every route.  Without the flags nothing changes.

`--nms_iou T` (a number in [0, 1]; off without it) suppresses duplicate detections -- several query patterns of one anchor position firing on the same
object -- before anything counts them: per image the queries at or above the pass's lowest threshold are walked by descending score and one whose
evaluation box has an IoU > T with an earlier SURVIVING one is dropped (counting_detr_amd/nms.py states the rule).  It is a filter on `prob`: the
suppressed queries become NaN directly after the forward, which the counting rule, the emit, the sweep's count and the host loop never keep, so
--threshold, --sweep_thresholds, --image_report and --render_worst work on the survivors unchanged (greedy suppression is prefix-consistent: the
filter at a sweep's lowest threshold is the filter of each of its thresholds).  The host loop calls nms.suppress (numpy, the checker); with
--device_detections ONE cdetr_nms_suppress launch per batch does the same bit for bit.  The metrics gain nms_removed.  Without the flag nothing changes.

`--error_report` says WHY detections fail, the single-class form of the TIDE breakdown at IoU 0.5 (counting_detr_amd/error_report.py states the rule): an
unmatched detection is a duplicate (its best ground truth is taken), a localisation error (0.1 <= IoU < 0.5) or background; an unmatched ground truth is
mislocalised or missed.  The metrics gain err_dup / err_loc / err_bkg / err_misloc / err_missed and dAP50_dup / _loc / _bkg / _missed (what AP50 would gain if
the cause were fixed) and error_report_<split>.json appears beside the predictions file ({"split", "threshold", "iou_fg", "iou_bg", "max_dets", "totals",
"dAP50", "rows", "order_by_dup", "order_by_loc", "order_by_bkg", "order_by_missed"}).  It needs instances_<split>.json, not --image_report; with both, the two
reports read the same one matching.  With --device_detections ONE cdetr_coco_errors launch reads the store's boxes where they lie; any other run on a GPU packs
the written predictions for the same kernel; `--ap_on_host` is the numpy rule.  Same bytes on every route; with --sweep_thresholds the report describes the
run's own --threshold.  Without the flag nothing changes.

`--bootstrap R` (1 .. 10000; `--bootstrap_seed S`, default 0, an error without it) says HOW FAR the numbers move when the split is resampled: R bootstrap
replicates over images, the same draws for every metric (counting_detr_amd/bootstrap.py states the rule).  The metrics gain <K>_lo / <K>_hi, the 95 % interval,
for MAE / RMSE / NAE / SRE and -- where instances_<split>.json is there -- AP / AP50 / AP75 / APs / APm / APl, and bootstrap_<split>.json appears beside the
predictions file ({"split", "threshold", "replicates", "seed", "level", "metrics": {K: {"value", "lo", "hi", "se", "undefined"}}}; with --sweep_thresholds also
"sweep": every threshold's counting intervals, their paired differences to --threshold and "best_vs_threshold"; AP at the run's threshold only).  With
--device_detections the replicates read the split's one matching where its flags lie (cdetr_bootstrap_gather, cdetr_bootstrap_ap) and the sweep's count table
where it lies (cdetr_bootstrap_counts); any other run on a GPU matches the written predictions there for the same kernels; `--ap_on_host` is the numpy rule,
slow for AP.  Same bytes on every route.  Without the flag nothing changes.

`--tiles RxC` (`--tile_margin M`, default 32; `--tile_scale S`, 1 or 2, default 1; `--tile_below P`; off without --tiles, and nothing changes) counts PAST
the query cap: the model has Q queries, so no image can count more than Q objects.  Every image is cut into R x C overlapping tiles (cores on a
32-pixel grid that partition the image, each tile reaching M pixels beyond its core, optionally upsampled by 2), the tiles run as ONE grouped forward
in which every tile is conditioned on the exemplar feature pooled over all tiles of the image (cdetr_exemplar_group_fwd), and the stitch puts their
outputs back into whole-image coordinates as one virtual image of R * C * Q queries (at most 4096) in which a query keeps its prob only in the tile
whose core holds its centre -- everywhere else it is NaN (counting_detr_amd/tiling.py states the rule).  It is one more filter between the forward and
the first reader: the store, the sweep, the one matching, the reports, the intervals, the overlays and the predictions file work on [1, R * C * Q, .]
tensors unchanged, and --nms_iou, which runs after the stitch, removes the second detection of an object that straddles a seam.  --tile_below P
tiles only the images whose exemplars are small (mean sqrt(w h) in resized pixels < P, known on the host); the others run whole.  The losses are
not computed under --tiles (no loss_* / class_error / cardinality_error in the metrics); --eval_batch_size must be 1; 1x1 is the identity.  The host
loop cuts and stitches with tiling.py's numpy (the checker); with --device_detections one cdetr_tile_images and one cdetr_tile_stitch launch per image
do the same bit for bit, nothing awaited.  Whether tiling lowers MAE on trained FSC-147 weights is UNMEASURED.

  python infer.py -dp /data/FSC147 --split val --resume out/detr_retrain.pth -o out
  python infer.py -dp /data/FSC147 --split val --resume out/detr_retrain.pth -o out --device_detections
  python infer.py -dp /data/FSC147 --split val --resume out/detr_retrain.pth -o out --device_detections --tiles 2x2 --nms_iou 0.5
  python infer.py -dp /data/FSC147 --split val --resume out/detr_retrain.pth -o out --device_detections --tiles 2x2 --tile_scale 2 --tile_below 24
  python infer.py -dp /data/FSC147 --split val --resume out/detr_retrain.pth -o out --device_detections --error_report
  python infer.py -dp /data/FSC147 --split val --resume out/detr_retrain.pth -o out --device_detections --bootstrap 1000
  python infer.py -dp /data/FSC147 --split val --resume out/detr_retrain.pth -o out --device_detections --image_report
  python infer.py -dp /data/FSC147 --split val --resume out/detr_retrain.pth -o out --device_detections --image_report --render_worst 8
  python infer.py -dp /data/FSC147 --split val --resume out/detr_retrain.pth -o out --device_detections --image_report --render_ids 3,17
  python infer.py -dp /data/FSC147 --split val --resume out/detr_retrain.pth -o out --device_detections --sweep_thresholds 0.3:0.7:9
  python infer.py -dp /data/FSC147 --split test --resume out/detr_retrain.pth -o out --device_detections --threshold ckpt
  python infer.py -dp /data/FSC147 --split val --resume out/detr_retrain.pth -o out --device_detections --eval_batch_size 16
  python infer.py -dp /data/FSC147 --split val --resume out/detr_retrain.pth -o out --device_detections --nms_iou 0.5
"""
import json
import os

import torch

import counting_detr_amd
from counting_detr_amd import data
from counting_detr_amd.args import get_args_parser
from counting_detr_amd.coco_ap import MAX_DET_CUTS, MAX_DETS, gt_from_json, match_predictions, match_store, reference_box, summarize_sweep
from counting_detr_amd.engine import count_from_logits, counting_metrics
from counting_detr_amd.misc import NestedTensor


class ImageReport:
    """--image_report for one pass: where the box ground truth is, where the host route matches (`device`: a CUDA device, or None = coco_ap's
    interpreted host code) and, after the pass, `report` = coco_ap.image_report's dict (None for a pass without images)."""

    def __init__(self, gt_json, device=None):
        self.gt_json, self.device, self.split, self.report = gt_json, device, None, None

    def from_matching(self, matching, counts, image_ids, gt_counts, pred_counts, threshold):
        """The report of the images `image_ids` (in the order they were run) from the statistics of ONE coco_ap.Matching -> its AR numbers.
        `counts`: the prefix lengths of `Matching.stats` (None: every detection the matching saw)."""
        from counting_detr_amd.coco_ap import image_report
        self.report = image_report(matching.stats(MAX_DET_CUTS, counts), image_ids, gt_counts, pred_counts, self.split, threshold)
        return self.report["AR"]

    def from_predictions(self, predictions, image_ids, gt_counts, pred_counts, threshold):
        """`from_matching` for a predictions dict as written (`coco_ap.match_predictions`), matched where `device` says."""
        return self.from_matching(match_predictions(predictions, self.gt_json, image_ids, self.device), None, image_ids, gt_counts, pred_counts, threshold)

    def write(self, output_dir):
        if self.report is not None:
            with open(os.path.join(output_dir, "image_report_" + self.split + ".json"), "w") as handle:
                json.dump(self.report, handle)


class ErrorReport:
    """--error_report for one pass, beside ImageReport and with its three routes: where the box ground truth is, where the host route matches
    (`device`: a CUDA device, or None = the numpy rule of counting_detr_amd/error_report.py) and, after the pass, `report` = error_report.report's
    dict (None for a pass without images)."""

    def __init__(self, gt_json, device=None):
        self.gt_json, self.device, self.split, self.report = gt_json, device, None, None

    def from_matching(self, matching, counts, image_ids, threshold):
        """The report of the images `image_ids` (in the order they were run) from the `errors()` reading of ONE coco_ap.Matching -> the metrics'
        err_* and dAP50_* keys.  `counts`: the prefix lengths of `Matching.errors` (None: every detection the matching saw)."""
        from counting_detr_amd import error_report as er
        self.report = er.report(matching.pack, matching.errors(counts), image_ids, self.split, threshold)
        return er.metrics(self.report)

    def write(self, output_dir):
        if self.report is not None:
            with open(os.path.join(output_dir, "error_report_" + self.split + ".json"), "w") as handle:
                json.dump(self.report, handle)


class Bootstrap:
    """--bootstrap R for one pass, beside ImageReport / ErrorReport and with their three routes: `replicates` and `seed` of the draws, `gt_json`
    (the split's box ground truth, or None: counting intervals only), where the replicates run (`device`: a CUDA device = cdetr_bootstrap_counts
    / cdetr_bootstrap_ap, or None = the numpy rule of counting_detr_amd/bootstrap.py) and, after the pass, `report` = bootstrap.report's dict
    (None for a pass without images)."""

    def __init__(self, replicates, seed=0, gt_json=None, device=None):
        from counting_detr_amd.bootstrap import check_args
        (self.replicates, self.seed), self.gt_json, self.device, self.split, self.report = check_args(replicates, seed), gt_json, device, None, None

    def _device_sums(self, table):
        """The counting sums on `device`: the [N, T] int32 `table` ops.ThresholdSweep left there is read where it lies, else the counts go up."""
        def sums(gt, pred, R, seed, mult):
            import numpy as np
            from counting_detr_amd import ops
            with torch.cuda.device(self.device):
                p = table if table is not None else torch.from_numpy(np.ascontiguousarray(pred, dtype=np.int32)).to(self.device)
                return ops.bootstrap_counts(torch.from_numpy(gt.astype(np.int32)).to(self.device), p, R, seed, host=True)
        return sums if self.device is not None else None

    def run(self, image_ids, gt_counts, pred_counts, threshold, matching=None, counts=None, six=None, sweep=None, table=None):
        """The report of one pass -> the metrics' <K>_lo / <K>_hi keys.  The images in the order they were run: replicate r draws the same
        images for every metric.  `matching` (a coco_ap.Matching under the four area ranges whose `image_ids` are these, or None: no AP),
        `counts` its prefix lengths and `six` the run's own six numbers (None: `matching.six()`); `sweep` (a threshold_sweep.Sweep after its pass:
        counts [N, T] and report): the counting intervals of every threshold and their paired differences to `threshold`; `table`: the sweep's
        counts as the device tensor they were formed in."""
        import numpy as np
        from counting_detr_amd import bootstrap as bs
        from counting_detr_amd import threshold_sweep as ts
        R, seed, N = self.replicates, self.seed, len(gt_counts)
        pred, col = (np.asarray(pred_counts).reshape(N, 1), 0) if sweep is None else (np.asarray(sweep.counts).reshape(N, -1), ts.column(sweep.thresholds, threshold))
        values, reps = bs.counting(gt_counts, pred, R, seed, self._device_sums(table[:N] if table is not None and sweep is not None else None))
        section = bs.sweep_section(sweep.thresholds, threshold, values, reps, sweep.report["best"]) if sweep is not None else None
        values, reps = {K: values[K][col] for K in bs.COUNT_KEYS}, {K: reps[K][:, col] for K in bs.COUNT_KEYS}
        if matching is not None:
            six, table6 = matching.six() if six is None else six, matching.bootstrap(R, seed, counts)
            values.update({K: six[K] for K in bs.AP_KEYS})
            reps.update({K: table6[:, k] for k, K in enumerate(bs.AP_KEYS)})
        self.report = bs.report(self.split, threshold, R, seed, values, reps, section)
        return bs.metrics(self.report)

    def write(self, output_dir):
        if self.report is not None:
            with open(os.path.join(output_dir, "bootstrap_" + self.split + ".json"), "w") as handle:
                json.dump(self.report, handle)


class Render:
    """--render_worst K / --render_ids for one pass: the overlays of the images `render.select` picks from the pass's image report, written to
    render_<split>/ wherever the predictions file is (counting_detr_amd/render.py states the drawing rule).  `out_dir`: where the last pass
    wrote them (None: it wrote none)."""

    def __init__(self, data_path, worst=0, ids=()):
        self.data_path, self.worst, self.ids, self.out_dir = data_path, int(worst), tuple(ids), None

    def from_predictions(self, predictions, image_ids, image_report, output_dir, threshold):
        """`from_matching` for a predictions dict as written, matched at area range `all` where `image_report.device` says."""
        matching = match_predictions(predictions, image_report.gt_json, image_ids, image_report.device, ("all",))
        return self.from_matching(matching, None, image_report, output_dir, threshold)

    def from_matching(self, matching, counts, image_report, output_dir, threshold):
        """The overlays from what ONE coco_ap.Matching holds: the pack's boxes (a store's are read on its device), row [0, 0] of the flags where
        they lie and the prefix lengths `counts` (as for `ImageReport.from_matching`).  Host flags (--ap_on_host) are drawn by render.py's
        host implementation, the checker; device flags by one cdetr_render_boxes launch there."""
        from counting_detr_amd import render as rd
        pack, report = matching.pack, image_report.report
        picks = rd.select(report, self.worst, self.ids)
        canvases, files, exemplars = rd.load_canvases(self.data_path, image_report.split, [p["image_id"] for p in picks])
        at = {i: b for b, i in enumerate(pack["image_ids"])}
        drawn = [k for k, p in enumerate(picks) if p["image_id"] in at]             # an image with neither ground truth nor detection is not packed
        overlays = rd.render_images([canvases[k] for k in drawn], pack, *matching.row50(), [at[picks[k]["image_id"]] for k in drawn],
                                    dt_cnt=matching.pack_counts(counts), exemplars=[exemplars[k] for k in drawn], device=matching.device) if drawn else []
        by_pick = dict(zip(drawn, overlays))
        overlays = [by_pick[k] if k in by_pick else rd.paint_first_hit(canvases[k], *rd.primitives([], [], [], exemplars[k]))       # exemplars only
                    for k in range(len(picks))]
        self.out_dir = rd.write(output_dir, image_report.split, threshold, picks, files, report, overlays)
        return self.out_dir


@torch.no_grad()
def infer(model, criterion, data_loader, device, output_dir, split="test", threshold=0.5, graphs=True, device_detections=False, gt_json=None,
          per_image=False, engine=None, write_json=True, sweep=None, image_report=None, render=None, nms_iou=None, error_report=None,
          bootstrap=None, tiles=None):
    """-> (metrics dict, predictions dict); writes predictions_<split>.json like A2/infer.py:28-121.  The forward + counting rule
    runs through engine.InferenceEngine (pre-split weight images, one captured HIP graph per image shape; `graphs=False`: eager).
    `device_detections`: the post-forward work on the device (`_infer_device`): the same file, bytes and all, the same metrics; with `gt_json`
    (the split's instances json) the metrics also carry the box AP, matched from the device-resident detections.
    `per_image` (--eval_batch_size > 1): the loader yields batches of several images of one size; the losses are `criterion.per_image`'s, one
    value per image, summed image by image -- what the batch-1 loop logs.
    `engine`: an InferenceEngine of `model` made by the caller instead of a new one per call (main.py --eval_every: one engine riding on the
    trainer, engine.InferenceEngine(trainer=...), its captured forwards reused pass after pass; its weight images are brought up to date
    here, `engine.sync()`, before the first forward).  `write_json=False`: no predictions file is written or removed (the device path then
    returns None for the predictions dict instead of building it); the metrics are the same either way.
    `threshold`: rounded to fp32 once (threshold_sweep.widen), the rule everywhere below.  `sweep` (a threshold_sweep.Sweep whose thresholds
    include `threshold`): the same pass also forms the counts of every image at every threshold of the sweep -- and, with `sweep.gt_json`, the
    six AP numbers per threshold --, leaves them in `sweep.report` / `sweep.counts` and writes threshold_sweep_<split>.json; the returned
    metrics and the predictions file are those of a pass without it.
    `image_report` (an ImageReport): the metrics gain the six average-recall keys and image_report_<split>.json is written wherever the
    predictions file is; with `device_detections` and `gt_json` the statistics come from the store's ONE matching (one more launch),
    otherwise from the predictions as written.
    `render` (a Render; needs `image_report`): render_<split>/ with the overlays of the report's worst images is written wherever the
    predictions file is, drawn where the pass matched: from the store's one matching, else from the predictions as written.
    `nms_iou` (--nms_iou; None: off, and nothing changes): greedy suppression of duplicate detections (counting_detr_amd/nms.py states the
    rule).  Directly after the forward `prob` is replaced by the filtered tensor, suppressed queries NaN -- which no reader below counts --, at
    the pass's lowest threshold (`threshold`, or the sweep's first); the host loop calls nms.suppress, the device loop launches
    cdetr_nms_suppress once per batch.  The metrics gain `nms_removed`: the split's queries with raw prob >= `threshold` that were suppressed.
    `error_report` (an ErrorReport; None: off, and nothing changes): the metrics gain err_dup / err_loc / err_bkg / err_misloc / err_missed and the
    four dAP50_* numbers, and error_report_<split>.json is written wherever the predictions file is.  It reads the SAME one matching as
    `image_report` -- with `device_detections` and `gt_json` the store's (one cdetr_coco_errors launch on the boxes where they lie), otherwise
    one of the predictions as written -- and does not need an image report.
    `bootstrap` (a Bootstrap; None: off, and nothing changes): the metrics gain <K>_lo / <K>_hi for MAE / RMSE / NAE / SRE and, where
    `bootstrap.gt_json` is set, for the six AP numbers, and bootstrap_<split>.json is written wherever the predictions file is.  The AP
    replicates read the SAME one matching as the reports (with `device_detections` and `gt_json` the store's, its flags where they lie).
    `tiles` (--tiles; a tiling.Tiling, None: off, and nothing changes): every image is cut into overlapping tiles, the tiles run as ONE grouped
    forward conditioned on the image's pooled exemplars, and the stitch turns their outputs into `prob`, `pred_boxes` and `ref_points` of shape
    [1, R * C * Q, .] in whole-image coordinates, a query outside its tile's core NaN (counting_detr_amd/tiling.py states the rule) -- one more
    filter between the forward and the first reader, ahead of `nms_iou`.  The host loop cuts and stitches with tiling.py's numpy, the device loop
    with cdetr_tile_images / cdetr_tile_stitch.  The criterion is not called: a stitched set of queries is not a training output, the metrics
    carry no loss_* / class_error / cardinality_error.  One image per batch."""
    from counting_detr_amd import threshold_sweep as ts
    threshold = ts.widen(threshold)
    if nms_iou is not None:
        from counting_detr_amd import nms
        nms_iou = nms.check_iou(nms_iou)
    if render is not None:
        if image_report is None:
            raise ValueError("infer: --render_worst / --render_ids draw what --image_report lists: pass an ImageReport as well")
        render.out_dir = None
    if sweep is not None:
        ts.column(sweep.thresholds, threshold)              # raises unless the run's own threshold is one of the sweep's
    if image_report is not None:
        image_report.split, image_report.report = split, None
    if error_report is not None:
        error_report.split, error_report.report = split, None
    if bootstrap is not None:
        bootstrap.split, bootstrap.report = split, None
    output_path = os.path.join(output_dir, "predictions_" + split + ".json") if write_json else None
    if output_path is not None and os.path.isfile(output_path):
        os.remove(output_path)
    model.eval()
    criterion.eval()
    if engine is None:
        from counting_detr_amd.engine import InferenceEngine
        engine = InferenceEngine(model, threshold, graphs=graphs and torch.device(device).type == "cuda", device=device)
    elif engine.model is not model or ts.widen(engine.threshold) != threshold:
        raise ValueError("infer: the engine passed in was built for another model or threshold")
    elif getattr(engine, "trainer", None) is not None:
        engine.sync()                   # the epoch's last optimizer step came after the last refresh of the trainer's forward images
    if device_detections:
        out = _infer_device(engine, criterion, data_loader, torch.device(device), output_path, threshold, gt_json, per_image, sweep, image_report,
                            render, output_dir, nms_iou, error_report, bootstrap, tiles)
        _write_sweep(sweep, output_dir, split)
        if image_report is not None and output_path is not None:
            image_report.write(output_dir)
        if error_report is not None and output_path is not None:
            error_report.write(output_dir)
        if bootstrap is not None and output_path is not None:
            bootstrap.write(output_dir)
        return out
    predictions = {"categories": [{"name": "fg", "id": 1}], "images": [], "annotations": []}
    anno_id = 1
    pred_counts, gt_counts, loss_sum, n_img = [], [], {}, 0
    tables, dt_by, image_ids = [], {}, []           # sweep: count rows per batch, the detections kept at the sweep's lowest threshold
    nms_removed = 0
    def lookahead(loader):          # (batch on the device, the next batch's image tensor or None): the engine runs the next image's frozen
        prev = None                 # stage (stem + layer1) beside this image's encoder / decoder
        for cur in loader:
            cur = dict(cur)
            cur["image"], cur["mask"] = cur["image"].to(device), cur["mask"].to(device)
            if prev is not None:
                yield prev, cur["image"]
            prev = cur
        if prev is not None:
            yield prev, None

    for ret, next_image in lookahead(data_loader):
        image, mask = ret["image"], ret["mask"]
        rects = ret["ex_rects"].to(device)
        targets = [{k: v.to(device) for k, v in t.items()} for t in ret["targets"]]
        if tiles is None:
            _, keep, outputs, ref_points, prob = engine(NestedTensor(image, mask), rects, next_samples=next_image)      # forward + :75-81
        else:                                       # the tiles of this image as one grouped forward, stitched by the numpy rule
            outputs, ref_points, prob = _tiled_forward(engine, tiles, image, mask, ret, on_device=False)
            keep = prob >= threshold
        if nms_iou is not None:                     # the filter: everything below reads the suppressed queries as NaN
            raw = prob.cpu().numpy()
            kept_h, _ = nms.suppress(raw, outputs["pred_boxes"].cpu().numpy(), [[int(x) for x in hw] for hw in ret["orig_size"]],
                                     threshold if sweep is None else sweep.thresholds[0], nms_iou)
            nms_removed += int((ts.kept(raw, threshold) & ~ts.kept(kept_h, threshold)).sum())
            prob = torch.from_numpy(kept_h).to(prob.device)
            keep = prob >= threshold
        if tiles is not None:                       # no losses: the criterion describes whole-image training outputs
            pass
        elif per_image:
            for k, v in criterion.per_image(outputs, targets).items():
                for x in v.tolist():                # float(v[b]) in image order
                    loss_sum[k] = loss_sum.get(k, 0.0) + x
        else:
            loss_dict = criterion(outputs, targets)
            for k, v in loss_dict.items():
                loss_sum[k] = loss_sum.get(k, 0.0) + float(v) * len(targets)
        for b in range(image.shape[0]):
            ori_h, ori_w = [int(x) for x in ret["orig_size"][b]]
            image_id = int(ret["image_id"][b]) if "image_id" in ret else n_img
            kb = keep[b]
            if sweep is not None:                   # everything the lowest threshold keeps; the file takes those at `threshold`
                if b == 0:
                    prob_h = prob.cpu().numpy()
                    tables.append(ts.count_table(prob_h, sweep.thresholds))
                kb = torch.from_numpy(ts.kept(prob_h[b], sweep.thresholds[0])).to(prob.device)
            scores = prob[b][kb].cpu().numpy()
            boxes = outputs["pred_boxes"][b][kb].cpu().numpy().copy()
            pts = ref_points[b][kb].cpu().numpy().copy()
            pts[..., 0] *= ori_w; pts[..., 1] *= ori_h
            boxes[..., 0] *= ori_w; boxes[..., 1] *= ori_h; boxes[..., 2] *= ori_w; boxes[..., 3] *= ori_h
            for sc, bx, pt in zip(scores, boxes, pts):
                x_cen, y_cen, w, h = bx
                if sweep is not None:
                    box = reference_box([int(x_cen), int(y_cen), int(w), int(h)])
                    dt_by.setdefault(image_id, []).append({"bbox": box, "score": float(sc), "area": float(box[2] * box[3])})
                    if not ts.kept(sc, threshold):
                        continue
                predictions["annotations"].append({"id": anno_id, "image_id": image_id, "area": int(w * h),
                                                   "bbox": [int(x_cen), int(y_cen), int(w), int(h)], "category_id": 1,
                                                   "score": float(sc), "point": [int(pt[0]), int(pt[1])]})
                anno_id += 1
            predictions["images"].append({"id": image_id, "height": ori_h, "width": ori_w, "file_name": "None"})
            pred_counts.append(int(kb.sum()) if sweep is None else int(tables[-1][b, ts.column(sweep.thresholds, threshold)]))
            gt_counts.append(int(targets[b]["boxes"].shape[0]))
            image_ids.append(image_id)
            n_img += 1
    if output_path is not None:
        with open(output_path, "w") as handle:
            json.dump(predictions, handle)
    metrics = {k: v / max(n_img, 1) for k, v in loss_sum.items()}
    if n_img:       # images without objects contribute to MAE / RMSE only (the reference divides by the count, A2/eval_all.py:264-265)
        metrics.update(counting_metrics(pred_counts, gt_counts))
    metrics["images"] = n_img
    if nms_iou is not None:
        metrics["nms_removed"] = nms_removed
    if sweep is not None and n_img:
        import numpy as np
        ap_rows = None
        if sweep.gt_json is not None:
            ap_rows = summarize_sweep(gt_from_json(sweep.gt_json, image_ids), dt_by, sweep.thresholds)
        sweep.counts = np.concatenate(tables)
        sweep.report = ts.report(sweep.thresholds, sweep.counts, gt_counts, ap_rows)
    _write_sweep(sweep, output_dir, split)
    boot_ap = bootstrap is not None and bootstrap.gt_json is not None and n_img
    matching = None
    if image_report is not None and n_img:
        matching = match_predictions(predictions, image_report.gt_json, image_ids, image_report.device)       # once, for the reports and the overlays
        metrics.update(image_report.from_matching(matching, None, image_ids, gt_counts, pred_counts, threshold))
        if output_path is not None:
            image_report.write(output_dir)
            if render is not None:
                render.from_matching(matching, None, image_report, output_dir, threshold)
    if error_report is not None and n_img:
        if image_report is None:                # no statistics asked for: the breakdown reads the boxes, one area range carries them (the replicates need four)
            matching = match_predictions(predictions, error_report.gt_json, image_ids, error_report.device, *(() if boot_ap else (("all",),)))
        metrics.update(error_report.from_matching(matching, None, image_ids, threshold))
        if output_path is not None:
            error_report.write(output_dir)
    if bootstrap is not None and n_img:
        if boot_ap and matching is None:
            matching = match_predictions(predictions, bootstrap.gt_json, image_ids, bootstrap.device)
        if boot_ap:
            matching.image_ids = image_ids      # the images the replicates draw from, in the order they were run
        metrics.update(bootstrap.run(image_ids, gt_counts, pred_counts, threshold, matching if boot_ap else None, sweep=sweep))
        if output_path is not None:
            bootstrap.write(output_dir)
    return metrics, predictions


def _write_sweep(sweep, output_dir, split):
    """threshold_sweep_<split>.json of a pass that swept (nothing otherwise)."""
    if sweep is not None and sweep.report is not None:
        with open(os.path.join(output_dir, "threshold_sweep_" + split + ".json"), "w") as handle:
            json.dump(sweep.report, handle)


def _num_images(data_loader):
    """Images a loader will yield (the device store is allocated once, up front)."""
    inner = getattr(data_loader, "loader", data_loader)                 # data.Prefetcher wraps the DataLoader
    if hasattr(inner, "dataset"):
        return len(inner.dataset)
    if isinstance(inner, (list, tuple)):
        return sum(int(b["image"].shape[0]) for b in inner)
    raise RuntimeError("infer: device_detections needs the number of images up front (a DataLoader, a data.Prefetcher or a list of batches)")


def _infer_device(engine, criterion, data_loader, device, output_path, threshold, gt_json, per_image=False, sweep=None, image_report=None,
                  render=None, output_dir=None, nms_iou=None, error_report=None, bootstrap=None, tiles=None):
    """The loop of `infer` with nothing coming back to the host inside it.  Per batch: forward, losses into row i of a device buffer (`per_image`:
    cdetr_criterion_eval's [B, 7] rows into B rows, one per image), one
    cdetr_emit_detections call into an ops.DetectionStore (wire records in query order + evaluation records in COCOeval's order), original sizes
    and image ids into a device table.  After the loop: one copy each of the store, the table and the loss buffer; the json is written from the
    store's arrays (same bytes as the host loop's file), the losses are summed in Python in the same order (same floats), the counts are the
    store's.  Everything that needs the box ground truth then reads ONE coco_ap.Matching of the store (`match_store`; the file is not read
    back): the six AP numbers (`gt_json`), the report's statistics and the overlays.
    `sweep`: the store is emitted at the sweep's LOWEST threshold and one cdetr_count_sweep call per batch (ops.ThresholdSweep) sits beside the
    emit; after the loop one more copy brings the [N, T] table.  The file takes the wire records with score >= `threshold` (query order, ids
    from 1: the bytes of a pass without the sweep), the counts are the table's column at `threshold`, the AP of every threshold is a
    reading of that matching (`six_sweep`), the returned six numbers being its row at `threshold`, and the report and the overlays take the
    prefix of every image that `threshold` keeps, min(its count there, max_det).
    Without `gt_json` the report and the overlays are formed from the predictions dict as written (`match_predictions`, once for both).
    `nms_iou`: one cdetr_nms_suppress launch per batch at the store's threshold replaces `prob` before the emit and the sweep's count read it;
    the number of suppressed queries with raw prob >= `threshold` is accumulated in a device scalar and read after the loop.
    `tiles`: one cdetr_tile_images launch cuts the image, the tiles run as one grouped forward, one cdetr_tile_stitch launch leaves prob / boxes
    / points of R * C * Q virtual queries where the suppression and the emit read them; the store is sized for that many queries; no losses."""
    import numpy as np
    from counting_detr_amd import ops
    from counting_detr_amd import threshold_sweep as ts
    if device.type != "cuda":
        raise RuntimeError(f"infer: device_detections runs HIP kernels, device={device} has none (the default is the host path)")
    N = _num_images(data_loader)
    store = meta = loss_buf = loss_keys = table = nms_removed = None
    n_targets, gt_counts, n_img, n_batch = [], [], 0, 0
    with torch.cuda.device(device):
        for ret in data_loader:
            image, mask = ret["image"].to(device), ret["mask"].to(device)
            rects = ret["ex_rects"].to(device)
            targets = [{k: v.to(device) for k, v in t.items()} for t in ret["targets"]]
            if tiles is None:
                _, _, outputs, ref_points, prob = engine(NestedTensor(image, mask), rects)
                loss_dict = criterion.per_image(outputs, targets) if per_image else criterion(outputs, targets)
            else:
                outputs, ref_points, prob = _tiled_forward(engine, tiles, image, mask, ret, on_device=True)
                loss_dict = {}
            B, Q = prob.shape
            if store is None:
                store = ops.DetectionStore(N, Q, device, threshold=threshold if sweep is None else sweep.thresholds[0], max_det=MAX_DETS)
                table = ops.ThresholdSweep(N, sweep.thresholds, device) if sweep is not None else None
                meta = torch.zeros((N, 3), dtype=torch.int64, device=device)                # ori_h, ori_w, image id
                loss_keys = list(loss_dict)
                loss_buf = torch.zeros((N, len(loss_keys)), dtype=torch.float64, device=device)      # fp32 -> fp64 is exact: float(v) of the host loop
            if n_img + B > N or list(loss_dict) != loss_keys:
                raise RuntimeError(f"infer: the loader yields more than its {N} images, or the criterion changed its losses")
            if not per_image:
                if loss_keys:
                    loss_buf[n_batch].copy_(torch.stack([v.detach().reshape(()).to(torch.float64) for v in loss_dict.values()]))
                n_targets.append(len(targets))
                n_batch += 1
            else:
                loss_buf[n_batch:n_batch + B].copy_(torch.stack(list(loss_dict.values()), 1))      # [B, keys]: the kernel's rows, one per image
                n_targets += [1] * B
                n_batch += B
            rows = meta[n_img:n_img + B]
            rows[:, :2].copy_(torch.as_tensor(ret["orig_size"]).reshape(B, 2), non_blocking=True)
            if "image_id" in ret:
                rows[:, 2].copy_(torch.as_tensor(ret["image_id"]).reshape(B), non_blocking=True)
            else:
                rows[:, 2].copy_(torch.arange(n_img, n_img + B))
            prob, pred_boxes, orig_hw = prob.contiguous(), outputs["pred_boxes"].contiguous(), rows[:, :2].to(torch.int32)
            if nms_iou is not None:                 # the filter: the emit and the count below read the suppressed queries as NaN
                raw = prob
                prob, removed = ops.nms_suppress(raw, pred_boxes, orig_hw, store.threshold, nms_iou)
                if nms_removed is None:
                    nms_removed = torch.zeros((), dtype=torch.int64, device=device)
                # at the store's own threshold `removed` is the number; under a sweep only those the run's threshold would have kept count
                nms_removed += removed.sum() if sweep is None else ((raw >= threshold) & ~(prob >= threshold)).sum()
            store.emit(prob, pred_boxes, ref_points.reshape(B, Q, 2).contiguous(), orig_hw)
            if table is not None:
                table.emit(prob)
            gt_counts += [int(t["boxes"].shape[0]) for t in targets]
            n_img += B
        predictions = {"categories": [{"name": "fg", "id": 1}], "images": [], "annotations": []}
        loss_sum, pred_counts, image_ids = {}, [], []
        if n_img:
            host = store.finish()
            meta_h = meta[:n_img].cpu().tolist()
            for row, n_t in zip(loss_buf[:n_batch].cpu().tolist(), n_targets):
                for k, v in zip(loss_keys, row):
                    loss_sum[k] = loss_sum.get(k, 0.0) + v * n_t
            pred_counts = host["counts"].tolist()
            image_ids = [m[2] for m in meta_h]
            wire_np, score_np, per_image = host["wire"], host["score"], np.diff(host["wire_off"]).tolist()
            if sweep is not None:                   # the store holds what the lowest threshold keeps: the file and the counts are `threshold`'s
                col = ts.column(sweep.thresholds, threshold)
                sweep.counts = table.finish()
                pred_counts = sweep.counts[:, col].tolist()
                at_thr = ts.kept(score_np, threshold)
                owner = np.repeat(np.arange(n_img), per_image)
                wire_np, score_np, per_image = wire_np[at_thr], score_np[at_thr], np.bincount(owner[at_thr], minlength=n_img).tolist()
        if n_img and output_path is not None:
            ann_image = [i for i, c in zip(image_ids, per_image) for _ in range(c)]
            wire, score = wire_np.tolist(), score_np.astype(np.float64).tolist()
            predictions["annotations"] = [{"id": k + 1, "image_id": i, "area": w[4], "bbox": w[:4], "category_id": 1, "score": sc, "point": w[5:7]}
                                          for k, (i, w, sc) in enumerate(zip(ann_image, wire, score))]
            predictions["images"] = [{"id": m[2], "height": m[0], "width": m[1], "file_name": "None"} for m in meta_h]
        if output_path is not None:
            with open(output_path, "w") as handle:
                json.dump(predictions, handle)
        else:
            predictions = None
        metrics = {k: v / max(n_img, 1) for k, v in loss_sum.items()}
        if n_img:
            metrics.update(counting_metrics(pred_counts, gt_counts))
        metrics["images"] = n_img
        if nms_iou is not None:
            metrics["nms_removed"] = int(nms_removed) if nms_removed is not None else 0
        ap_json = sweep.gt_json if sweep is not None and sweep.gt_json is not None else gt_json
        matching = counts = ap_rows = None
        if ap_json is not None and n_img:                   # the store's ONE matching: everything below reads it
            matching = match_store(gt_from_json(ap_json, image_ids), store, image_ids, sweep=sweep.thresholds if sweep is not None else None)
        if sweep is not None and n_img:
            if matching is not None:                        # the report and the overlays describe `threshold`: a prefix of every image of the store
                ap_rows, counts = matching.six_sweep(sweep.thresholds), np.minimum(sweep.counts[:, col], MAX_DETS)
            sweep.report = ts.report(sweep.thresholds, sweep.counts, gt_counts, ap_rows if sweep.gt_json is not None else None)
        if matching is not None and gt_json is not None:
            metrics.update(matching.six() if ap_rows is None else ap_rows[col])
        boot_ap = bootstrap is not None and bootstrap.gt_json is not None and n_img
        six = None if ap_rows is None else ap_rows[col]
        if (image_report is not None or error_report is not None or boot_ap) and n_img:
            if gt_json is None:                             # no device matching asked for: the reports are formed from the predictions as written
                if predictions is None:
                    raise RuntimeError("infer: a report without the device matching (gt_json) is formed from the predictions file: write_json=False")
                src = image_report if image_report is not None else error_report if error_report is not None else bootstrap
                areas = () if image_report is not None or boot_ap else (("all",),)      # the breakdown alone reads the boxes: one area range carries them
                matching, counts, six = match_predictions(predictions, src.gt_json, image_ids, src.device, *areas), None, None
                matching.image_ids = image_ids
            if image_report is not None:
                metrics.update(image_report.from_matching(matching, counts, image_ids, gt_counts, pred_counts, threshold))
                if render is not None and output_path is not None:
                    render.from_matching(matching, counts, image_report, output_dir, threshold)
            if error_report is not None:
                metrics.update(error_report.from_matching(matching, counts, image_ids, threshold))
        if bootstrap is not None and n_img:
            metrics.update(bootstrap.run(image_ids, gt_counts, pred_counts, threshold, matching if boot_ap else None, counts, six, sweep,
                                         table.table if table is not None else None))
    return metrics, predictions


def _tiled_forward(engine, tiles, image, mask, ret, on_device):
    """One image under --tiles -> (outputs {"pred_boxes": [1, Qv, 4]}, ref_points [1, Qv, 2], prob [1, Qv]) on the image's device, Qv = R * C * Q:
    the plan of this image (its size and, under --tile_below, its exemplars, known on the host), the tile batch and the tile rects, ONE grouped
    forward, the stitch.  `on_device`: cdetr_tile_images and cdetr_tile_stitch, nothing awaited; else tiling.py's numpy rule, the checker.  An
    image whose plan is one whole-image tile is forwarded as it is."""
    from counting_detr_amd import tiling
    if image.shape[0] != 1:
        raise ValueError(f"infer: --tiles runs one image per batch, the loader gave {image.shape[0]} (--eval_batch_size must be 1)")
    rects_h = ret.get("ex_rects_host", ret["ex_rects"])[0].cpu().numpy()          # the loader's own host tensor: no device is asked
    plan = tiles.plan_for(image.shape[2], image.shape[3], rects_h)
    device, T = image.device, plan.T
    trects = torch.from_numpy(tiling.tile_rects(rects_h, plan)).to(device, non_blocking=True)
    if on_device:                                   # the plan's two small tables go up once per image size
        from counting_detr_amd import ops
        tables = plan.__dict__.setdefault("_tables", {})
        if device not in tables:
            tables[device] = (torch.from_numpy(plan.records).to(device), torch.from_numpy(plan.coef).to(device))
        records, coef = tables[device]
    if plan.whole:
        timg, tmask = image, mask
    elif on_device:
        timg, tmask = ops.tile_images(image[0].contiguous(), records, plan.Hm, plan.Wm)
    else:
        t_h, m_h = tiling.tile_images(image[0].cpu().numpy(), plan)
        timg, tmask = torch.from_numpy(t_h).to(device), torch.from_numpy(m_h).to(device)
    _, _, touts, tref, tprob = engine(NestedTensor(timg, tmask), trects, group=T)
    Q = tprob.shape[1]
    if on_device:
        prob, boxes, points = ops.tile_stitch(tprob.contiguous(), touts["pred_boxes"].contiguous(), tref.reshape(T, Q, 2).contiguous(), coef,
                                              plan.slots, plan.H, plan.W)
    else:
        p_h, b_h, r_h = tiling.stitch(tprob.cpu().numpy(), touts["pred_boxes"].cpu().numpy(), tref.reshape(T, Q, 2).cpu().numpy(), plan)
        prob, boxes, points = (torch.from_numpy(a)[None].to(device) for a in (p_h, b_h, r_h))
    return {"pred_boxes": boxes}, points, prob


def counting_metrics_from_json(pred_json, gt_json, threshold=0.5):
    """MAE / RMSE / NAE / SRE from a predictions json and the split's `instances_<split>.json` (A2/eval_all.py:141-270:
    predicted count = #annotations with score >= threshold per image, ground truth = #instances)."""
    with open(pred_json) as f:
        pred = json.load(f)
    gt = data.CocoIndex(gt_json)
    cnt = {im["id"]: 0 for im in pred["images"]}
    for a in pred["annotations"]:
        if a["score"] >= threshold:
            cnt[a["image_id"]] = cnt.get(a["image_id"], 0) + 1
    ids = sorted(cnt)
    return counting_metrics([cnt[i] for i in ids], [len(gt.getAnnIds([i])) for i in ids])


def eval_loader(args, device):
    """-> (loader of the evaluation split, per_image).  --eval_batch_size 1 (the default): one image per batch in dataset order, batched losses
    (the reference's loop).  B > 1: batches of up to B images of one resized size in bucket order (data.SizeBucketBatchSampler), per-image losses."""
    from torch.utils.data import DataLoader
    raw = bool(getattr(args, "device_preprocess", False))               # workers decode only; resize + normalise + pad on the device
    ds = data.build_test_dataset(args, image_set=args.split, raw=raw)
    collate_fn = data.collate_raw if raw else data.collate
    B = int(getattr(args, "eval_batch_size", 1))
    if B < 1:
        raise ValueError(f"--eval_batch_size must be at least 1, got {B}")
    if B > 1:
        dl = DataLoader(ds, batch_sampler=data.SizeBucketBatchSampler(ds, B), collate_fn=collate_fn, num_workers=args.num_workers)
    else:
        dl = DataLoader(ds, batch_size=1, shuffle=False, collate_fn=collate_fn, num_workers=args.num_workers)
    if raw:                                                             # --tiles plans on the host: the exemplar rects also stay there
        dl = data.Prefetcher(dl, device, host_keys=("ex_rects",)) if hasattr(args, "tiles") else data.Prefetcher(dl, device)
    return dl, B > 1


def run_threshold(args):
    """--threshold as the number the pass uses (fp32, widened); `ckpt` has been replaced by the checkpoint's value before (`main`)."""
    from counting_detr_amd.threshold_sweep import widen
    t = getattr(args, "threshold", 0.5)
    if t == "ckpt":
        raise ValueError("--threshold ckpt: only infer.py reads the threshold from the --resume checkpoint")
    return widen(t)


def build_sweep(args):
    """--sweep_thresholds -> a threshold_sweep.Sweep for one pass (--threshold merged in; AP columns when instances_<split>.json is there), or None."""
    if not getattr(args, "sweep_thresholds", None):
        return None
    from counting_detr_amd.threshold_sweep import Sweep, parse_spec
    gt_json = os.path.join(args.data_path, "instances_" + args.split + ".json")
    return Sweep(parse_spec(args.sweep_thresholds, run_threshold(args)), gt_json if os.path.isfile(gt_json) else None)


def evaluate_split(model, criterion, dl, per_image, device, args, engine=None, write_json=True, sweep=None):
    """One pass over `dl` (eval_loader) -> the metrics this file prints: mean losses, MAE / RMSE / NAE / SRE, `images`, and the six AP numbers
    when the split's instances json is there.  `engine` / `write_json`: see `infer` (main.py --eval_every passes its riding engine); the
    file is written regardless when the AP has to be read back from it (no --device_detections, or --ap_on_host).  --threshold and
    --sweep_thresholds act here; `sweep`: the caller's own `build_sweep(args)`, whose report it reads after the pass."""
    gt_json = os.path.join(args.data_path, "instances_" + args.split + ".json")
    on_device = bool(getattr(args, "device_detections", False))
    ap_in_loop = on_device and os.path.isfile(gt_json) and not getattr(args, "ap_on_host", False)      # matched from the device-resident detections
    ap_from_file = os.path.isfile(gt_json) and not ap_in_loop
    threshold = run_threshold(args)
    if sweep is None:
        sweep = build_sweep(args)
    report = build_image_report(args, device)
    render = build_render(args)
    errors = build_error_report(args, device)
    boot = build_bootstrap(args, device)
    tiles = build_tiling(args)
    metrics, _ = infer(model, criterion, dl, device, args.output_dir, split=args.split, threshold=threshold, device_detections=on_device,
                       gt_json=gt_json if ap_in_loop else None, per_image=per_image, engine=engine, write_json=write_json or ap_from_file,
                       sweep=sweep, image_report=report, render=render, nms_iou=getattr(args, "nms_iou", None), error_report=errors,
                       bootstrap=boot, tiles=tiles)
    if ap_from_file:
        from counting_detr_amd.coco_ap import ap_from_json
        # the matching runs on the device the detections came from (one cdetr_coco_match launch); --ap_on_host: the interpreted path, same numbers
        ap_device = device if device.type == "cuda" and not getattr(args, "ap_on_host", False) else None
        ar = {k: metrics.pop(k) for k in (report.report["AR"] if report is not None and report.report else ())}      # the AR keys follow the AP keys
        if errors is not None and errors.report:                                                                      # and the breakdown's follow those
            from counting_detr_amd.error_report import metrics as error_metrics
            ar.update({k: metrics.pop(k) for k in error_metrics(errors.report)})
        if boot is not None and boot.report:                                                                          # and the intervals come last
            from counting_detr_amd.bootstrap import metrics as bootstrap_metrics
            ar.update({k: metrics.pop(k) for k in bootstrap_metrics(boot.report)})
        metrics.update(ap_from_json(os.path.join(args.output_dir, "predictions_" + args.split + ".json"), gt_json, device=ap_device))
        metrics.update(ar)
    return metrics


def build_image_report(args, device=None):
    """--image_report -> an ImageReport for one pass, or None without the flag.  The report needs the split's box ground truth: a missing
    instances_<split>.json is an error here, before anything runs.  `device`: where a pass that does not match from the device store forms
    its statistics (a CUDA device unless --ap_on_host)."""
    if not getattr(args, "image_report", False):
        return None
    gt_json = os.path.join(args.data_path, "instances_" + args.split + ".json")
    if not os.path.isfile(gt_json):
        raise FileNotFoundError(f"--image_report needs the split's box ground truth: {gt_json} is not there")
    on_device = device is not None and torch.device(device).type == "cuda" and not getattr(args, "ap_on_host", False)
    return ImageReport(gt_json, torch.device(device) if on_device else None)


def build_error_report(args, device=None):
    """--error_report -> an ErrorReport for one pass, or None without the flag, as `build_image_report`: a missing instances_<split>.json is an
    error here, before anything runs; `device`: where a pass that does not read the device store classifies (a CUDA device unless --ap_on_host)."""
    if not getattr(args, "error_report", False):
        return None
    gt_json = os.path.join(args.data_path, "instances_" + args.split + ".json")
    if not os.path.isfile(gt_json):
        raise FileNotFoundError(f"--error_report needs the split's box ground truth: {gt_json} is not there")
    on_device = device is not None and torch.device(device).type == "cuda" and not getattr(args, "ap_on_host", False)
    return ErrorReport(gt_json, torch.device(device) if on_device else None)


def build_bootstrap(args, device=None):
    """--bootstrap R / --bootstrap_seed S -> a Bootstrap for one pass, or None without the flag.  The AP intervals appear where
    instances_<split>.json is there; without it only the counting intervals do, which is not an error.  `device`: where the replicates run
    (a CUDA device unless --ap_on_host: the numpy rule, slow for AP)."""
    if not hasattr(args, "bootstrap"):
        from counting_detr_amd.args import check_bootstrap_flags
        check_bootstrap_flags(args)
        return None
    gt_json = os.path.join(args.data_path, "instances_" + args.split + ".json")
    on_device = device is not None and torch.device(device).type == "cuda" and not getattr(args, "ap_on_host", False)
    return Bootstrap(args.bootstrap, getattr(args, "bootstrap_seed", 0), gt_json if os.path.isfile(gt_json) else None,
                     torch.device(device) if on_device else None)


def build_tiling(args):
    """--tiles RxC / --tile_margin / --tile_scale / --tile_below -> a tiling.Tiling for one pass, or None without --tiles.  The flags are
    checked again here (the parser says so first; a namespace built by hand meets it here)."""
    from counting_detr_amd.args import check_tile_flags
    check_tile_flags(args)
    if not hasattr(args, "tiles"):
        return None
    from counting_detr_amd.tiling import Tiling
    R, C = args.tiles
    return Tiling(R, C, getattr(args, "tile_margin", 32), getattr(args, "tile_scale", 1), getattr(args, "tile_below", None))


def build_render(args):
    """--render_worst K / --render_ids -> a Render for one pass, or None without either flag.  Both draw what --image_report lists: without
    it this is an error (the parser says so first; a namespace built by hand meets it here)."""
    if not hasattr(args, "render_worst") and not hasattr(args, "render_ids"):
        return None
    from counting_detr_amd.args import check_render_flags
    check_render_flags(args)
    return Render(args.data_path, getattr(args, "render_worst", 0), getattr(args, "render_ids", ()))


def main(args):
    device = torch.device(args.device)
    build_render(args)
    build_image_report(args)                                            # --image_report without instances_<split>.json: an error before anything is built
    build_error_report(args)                                            # --error_report likewise
    build_bootstrap(args)                                               # --bootstrap_seed without --bootstrap, R out of range: likewise
    build_tiling(args)                                                  # --tile_* without --tiles, too many virtual queries: likewise
    model, criterion, _ = counting_detr_amd.build_model(args)
    model.to(device)
    if args.resume:
        ckpt = torch.load(args.resume, map_location="cpu", weights_only=False)
        model.load_state_dict(ckpt["model"], strict=True)
    if getattr(args, "threshold", 0.5) == "ckpt":                       # the threshold main.py --calibrate_threshold left in the checkpoint
        from counting_detr_amd.threshold_sweep import checkpoint_threshold
        if not args.resume:
            raise ValueError("--threshold ckpt needs --resume: the threshold is read from that checkpoint")
        args.threshold = checkpoint_threshold(ckpt, args.resume)
    dl, per_image = eval_loader(args, device)
    os.makedirs(args.output_dir, exist_ok=True)
    metrics = evaluate_split(model, criterion, dl, per_image, device, args)
    print(json.dumps(metrics))
    with open(os.path.join(args.output_dir, "results_" + args.split + ".txt"), "w") as f:
        f.write(json.dumps(metrics) + "\n")


if __name__ == "__main__":
    main(get_args_parser().parse_args())
