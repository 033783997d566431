"""The reference's CLI (A2/main.py:17-135): same flag names and defaults, so scripts written for the reference's
main.py keep working.  `default_args(**overrides)` builds the namespace programmatically."""
import argparse


def get_args_parser():
    p = _CheckedParser("Counting-DETR 2nd stage (MI355X)", add_help=True)
    p.add_argument("-dp", "--data_path", type=str, default="./FSC147/")
    p.add_argument("-o", "--output_dir", type=str, default="./outputs/anchor_detr")
    p.add_argument("-ts", "--test_split", type=str, default="val", choices=["val_PartA", "val_PartB", "test_PartA", "test_PartB", "test", "val"])
    p.add_argument("--lr", default=1e-4, type=float)
    p.add_argument("--lr_backbone_names", default=["backbone"], type=str, nargs="+")
    p.add_argument("--lr_backbone", default=1e-5, type=float)
    p.add_argument("--lr_linear_proj_names", default=[], type=str, nargs="+")
    p.add_argument("--lr_linear_proj_mult", default=0.1, type=float)
    p.add_argument("--batch_size", default=1, type=int)
    p.add_argument("--weight_decay", default=1e-4, type=float)
    p.add_argument("--epochs", default=30, type=int)
    p.add_argument("--lr_drop", default=20, type=int)
    p.add_argument("--lr_drop_epochs", default=None, type=int, nargs="+")
    p.add_argument("--clip_max_norm", default=0.1, type=float)
    p.add_argument("--sgd", action="store_true", help="torch.optim.SGD(momentum=0.9) over the same lr groups instead of AdamW (A2/main.py:185-186)")
    p.add_argument("--frozen_weights", type=str, default=None)
    p.add_argument("--backbone", default="resnet50", type=str)
    p.add_argument("--dilation", default=True, type=lambda s: str(s).lower() not in ("0", "false", "no"))
    p.add_argument("--num_feature_levels", default=1, type=int)
    p.add_argument("--enc_layers", default=6, type=int)
    p.add_argument("--dec_layers", default=6, type=int)
    p.add_argument("--dim_feedforward", default=1024, type=int)
    p.add_argument("--hidden_dim", default=256, type=int)
    p.add_argument("--dropout", default=0.0, type=float)
    p.add_argument("--nheads", default=8, type=int)
    p.add_argument("--num_query_position", default=300, type=int)
    p.add_argument("--num_query_pattern", default=3, type=int)
    p.add_argument("--spatial_prior", default="learned", choices=["learned", "grid", "defined"], type=str)
    p.add_argument("--attention_type", default="RCDA", choices=["RCDA", "nn.MultiheadAttention"], type=str)
    p.add_argument("--masks", action="store_true")
    p.add_argument("--no_aux_loss", dest="aux_loss", action="store_false")
    p.add_argument("--cost_class", default=2, type=float)
    p.add_argument("--cost_bbox", default=5, type=float)
    p.add_argument("--cost_giou", default=2, type=float)
    p.add_argument("--mask_loss_coef", default=1, type=float)
    p.add_argument("--dice_loss_coef", default=1, type=float)
    p.add_argument("--cls_loss_coef", default=2, type=float)
    p.add_argument("--bbox_loss_coef", default=5, type=float)
    p.add_argument("--giou_loss_coef", default=2, type=float)
    p.add_argument("--focal_alpha", default=0.25, type=float)
    p.add_argument("--variance_loss_coef", default=2, type=float)
    p.add_argument("--device", default="cuda")
    p.add_argument("--seed", default=42, type=int)
    p.add_argument("--resume", default="")
    p.add_argument("--auto_resume", default=False, action="store_true")
    p.add_argument("--start_epoch", default=0, type=int)
    p.add_argument("--eval", action="store_true")
    p.add_argument("--num_workers", default=2, type=int)
    p.add_argument("--scale_factor", default=32, type=int, help="val / test images are resized to a multiple of this (A2/infer.py)")
    p.add_argument("--split", default="val", type=str, help="infer.py: val or test")
    p.add_argument("--cache_mode", default=False, action="store_true")
    p.add_argument("--ap_on_host", action="store_true",
                   help="infer.py: box AP through coco_ap's interpreted host path instead of the device matcher (same numbers, minutes on crowded splits)")
    p.add_argument("--device_detections", action="store_true",
                   help="infer.py / main.py --eval: threshold, scaling, truncation and COCOeval's ordering of the detections on the device "
                        "(cdetr_emit_detections, one call per image, one copy back per split); the same predictions json byte for byte, the box "
                        "AP matched from device memory without re-reading it (--ap_on_host: ap_from_json on the written file)")
    p.add_argument("--eval_batch_size", default=1, type=int,
                   help="infer.py / main.py --eval: images per forward.  1: the reference's loop.  More: batches of images of ONE resized size "
                        "(bucket order), the logged losses stay per-image quantities (SetCriterion.per_image, one cdetr_criterion_eval launch per batch)")
    # additions of this build (the reference hard-codes batch 1 on one GPU)
    p.add_argument("--dataset", default="fsc147", choices=["fsc147", "fscd_lvis"], help="reader used without --synthetic")
    p.add_argument("--images_per_gpu", default=2, type=int, help="local batch of the data-parallel trainer")
    p.add_argument("--synthetic", action="store_true", help="train on seeded synthetic tensors (no dataset needed)")
    p.add_argument("--steps_per_epoch", default=20, type=int, help="synthetic mode only")
    p.add_argument("--synthetic_size", default=[800, 800], type=int, nargs=2, help="synthetic mode only: image H W")
    p.add_argument("--pretrained_backbone", default="", type=str,
                   help="torchvision-layout ResNet-50 state dict (the reference hard-codes pretrained_models/resnet50-0676ba61.pth)")
    p.add_argument("--resume_skip_mismatch", action="store_true",
                   help="--resume: drop checkpoint keys whose shape differs (e.g. an Anchor-DETR COCO class head) instead of raising")
    p.add_argument("--resume_optimizer", action="store_true",
                   help="--resume: ALSO restore AdamW moments, StepLR state and the epoch counter from the checkpoint (continue an "
                        "interrupted run).  Default: model weights only and training starts at --start_epoch, exactly like the "
                        "reference (A2/main.py:195-209), which fine-tunes from a full detector checkpoint this way")
    p.add_argument("--no_resume_optimizer", dest="resume_optimizer", action="store_false", help="(default; kept for scripts of round 2)")
    p.add_argument("--no_graph_cache", dest="graph_cache", action="store_false",
                   help="train with the stream-ordered step instead of cached HIP graphs (one per padded image size / target-capacity class)")
    p.add_argument("--graph_cache_size", default=32, type=int, help="captured steps kept alive (least recently used is dropped)")
    p.add_argument("--graph_layout", default="chain", choices=["chain", "single"],
                   help="captured step: chain = linear graphs + side-stream graphs (host cost 0.3 ms per step); single = round 3's two graphs with "
                        "in-graph branches (8.7 ms of host time per step)")
    p.add_argument("--no_frozen_prefetch", dest="frozen_prefetch", action="store_false",
                   help="run the frozen stem + layer1 of a batch inside its own step instead of beside the previous step's Hungarian solve")
    p.add_argument("--captured_allreduce", action="store_true",
                   help="world_size > 1: the four gradient buckets' all-reduces as captured graphs on the exchange stream instead of host-issued "
                        "RCCL calls (untested on N > 1 GPUs: for the first multi-GPU A/B)")
    p.add_argument("--bwd_precision", default=None, choices=["bf16", "bf16x2", "bf16x3"],
                   help="arithmetic of the backward contractions (default bf16 = 1 MFMA per product, gradient error 4.7e-3 of its norm; "
                        "bf16x3 = the forward's split arithmetic, 1.6e-3; DESIGN section 3).  Same as CDETR_PRECISION_BWD=3/2/1")
    p.add_argument("--exemplar_mode", default="per_image", choices=["per_image", "reference"],
                   help="per_image: image b is conditioned on its own exemplars; reference: rects[0] for the whole batch "
                        "(A2/models/backbone.py:122 -- exact only at batch 1)")
    p.add_argument("--device_preprocess", action="store_true",
                   help="the DataLoader workers only decode; resize (PIL-exact), normalisation and padding run on the device in one launch per "
                        "batch (cdetr_image_prep) -- the same image / mask tensors bit for bit")
    p.add_argument("--eval_every", default=0, type=int,
                   help="main.py: validate on --split after every N-th epoch and after the last one, on the trainer's own weight images "
                        "(engine.InferenceEngine(trainer=...): no graph of the trainer or the engine is dropped); the epoch's log line gains "
                        "test_<k>.  0 = off.  Honours --eval_batch_size / --device_preprocess; --device_detections is the intended combination")
    p.add_argument("--keep_best", default="mae", choices=["mae", "ap", "loss"],
                   help="with --eval_every: the epoch whose pass has the lowest MAE / lowest loss / highest AP is also saved to "
                        "detr_retrain_best.pth (a tie keeps the earlier epoch; ap needs instances_<split>.json)")
    # the three flags below leave NO attribute behind when they are not given (argparse.SUPPRESS): a run without them sees the namespace -- and
    # writes the checkpoint's "args" -- it always did; readers use getattr(args, name, default), threshold 0.5 and no sweep being the defaults
    p.add_argument("--threshold", default=argparse.SUPPRESS, type=_threshold,
                   help="infer.py / main.py --eval / --eval_every: a query counts (and becomes a detection) when the fp32 sigmoid(logit) >= "
                        "float32(T); default 0.5.  infer.py also takes `ckpt`: the calibrated threshold the --resume checkpoint carries")
    p.add_argument("--sweep_thresholds", default=argparse.SUPPRESS, type=str, metavar="SPEC",
                   help="infer.py / main.py --eval / --eval_every: also report counts and AP at these thresholds from the same pass, into "
                        "threshold_sweep_<split>.json.  SPEC = lo:hi:n (n evenly spaced values, both ends) or a comma list; at most 32 distinct "
                        "fp32 values, --threshold included.  With --device_detections: one cdetr_count_sweep launch per batch, one matching per split")
    p.add_argument("--calibrate_threshold", default=argparse.SUPPRESS, choices=["mae", "rmse", "nae", "sre", "ap"],
                   help="main.py with --eval_every and --sweep_thresholds: the sweep's best threshold for this metric goes into the epoch's log "
                        "line (test_best_threshold, test_best_<metric>) and into every checkpoint written afterwards (count_threshold)")
    # like the three above: no attribute when it is not given
    p.add_argument("--image_report", action="store_true", default=argparse.SUPPRESS,
                   help="infer.py / main.py --eval / --eval_every: also say on WHICH images the model fails -- image_report_<split>.json beside the "
                        "predictions file (per image: counts, diff, its own AP numbers, tp / fp / fn at IoU 0.5; the images ordered by AP and by "
                        "diff) and six average-recall keys (AR900, AR1000, AR1100, ARs, ARm, ARl) in the metrics.  Needs instances_<split>.json.  "
                        "With --device_detections: one cdetr_coco_image_stats launch on the flags of the split's one matching")
    # the two below: no attribute when they are not given; both need --image_report (checked when the command line is parsed)
    p.add_argument("--render_worst", default=argparse.SUPPRESS, type=int, metavar="K",
                   help="infer.py / main.py --eval / --eval_every, with --image_report: draw the K images of lowest AP and the K of largest count "
                        "error -- render_<split>/<image_id>.png (detections green = true positive at IoU 0.5, red = false positive, grey = ignored, "
                        "with centre dots; ground truths blue, exemplars yellow) and render_<split>/index.json, beside the predictions file.  On "
                        "a CUDA device one cdetr_render_boxes launch; --ap_on_host: the host painter, the same bytes")
    p.add_argument("--render_ids", default=argparse.SUPPRESS, type=_id_list, metavar="ID,ID",
                   help="with --image_report: also draw the images with these ids (a comma list); usable without --render_worst")
    # like the flags above: no attribute when it is not given
    p.add_argument("--nms_iou", default=argparse.SUPPRESS, type=_nms_iou, metavar="T",
                   help="infer.py / main.py --eval / --eval_every: greedy suppression of duplicate detections ahead of everything that reads the "
                        "probabilities -- walking each image's queries by descending score, one whose box overlaps an earlier SURVIVING one with "
                        "IoU > T is dropped (counting_detr_amd/nms.py states the rule).  T in [0, 1]; 1 suppresses nothing.  Works with --threshold, "
                        "--sweep_thresholds, --image_report and --render_worst; the metrics gain nms_removed.  With --device_detections: one "
                        "cdetr_nms_suppress launch per batch")
    p.add_argument("--error_report", action="store_true", default=argparse.SUPPRESS,
                   help="infer.py / main.py --eval / --eval_every: also say WHY detections fail -- the single-class TIDE breakdown at IoU 0.5: "
                        "duplicate, localisation (0.1 <= IoU < 0.5), background and missed (counting_detr_amd/error_report.py states the rule).  "
                        "error_report_<split>.json beside the predictions file (per image: the counts and mean IoUs; the images ordered by each "
                        "cause; what AP50 would gain if a cause were fixed) and err_dup / err_loc / err_bkg / err_misloc / err_missed, dAP50_dup / "
                        "_loc / _bkg / _missed in the metrics.  Needs instances_<split>.json, not --image_report.  On a CUDA device one "
                        "cdetr_coco_errors launch for the split; --ap_on_host: the numpy rule, the same file")
    # the two below: no attribute when they are not given; --bootstrap_seed needs --bootstrap (checked when the command line is parsed)
    p.add_argument("--bootstrap", default=argparse.SUPPRESS, type=_replicates, metavar="R",
                   help="infer.py / main.py --eval / --eval_every: also say how far the numbers move when the split is resampled -- R (1 .. 10000) "
                        "bootstrap replicates over images (counting_detr_amd/bootstrap.py states the rule): MAE / RMSE / NAE / SRE and, where "
                        "instances_<split>.json is there, AP / AP50 / AP75 / APs / APm / APl gain <K>_lo / <K>_hi (the 95 %% interval) in the metrics, "
                        "and bootstrap_<split>.json beside the predictions file holds value / lo / hi / se per metric; with --sweep_thresholds "
                        "also every threshold's counting intervals and its paired difference to --threshold.  On a CUDA device the replicates "
                        "run in cdetr_bootstrap_counts / cdetr_bootstrap_ap; --ap_on_host: the numpy rule, the same file, SLOW for AP (about 0.1 s "
                        "per replicate and area range on a split of 1286 images)")
    p.add_argument("--bootstrap_seed", default=argparse.SUPPRESS, type=_seed, metavar="S",
                   help="with --bootstrap: the seed of the replicates' draws (default 0); the same seed draws the same images on every route")
    # the four below: no attribute when they are not given; the last three need --tiles (checked when the command line is parsed)
    p.add_argument("--tiles", default=argparse.SUPPRESS, type=_tiles, metavar="RxC",
                   help="infer.py / main.py --eval: count past the query cap -- every image is cut into R x C overlapping tiles, the tiles are "
                        "forwarded as one batch conditioned on the exemplars of the whole image, and each detection is kept by the tile whose "
                        "core holds its centre (counting_detr_amd/tiling.py states the rule).  Everything after the forward reads one image of "
                        "R * C * Q queries, at most 4096; 1x1 is the identity.  The losses are not computed (no loss_* keys in the metrics); "
                        "needs --eval_batch_size 1, not with --eval_every.  --nms_iou removes the duplicates of objects on a seam.  With "
                        "--device_detections: cdetr_tile_images + cdetr_tile_stitch per image.  The effect on accuracy is unmeasured")
    p.add_argument("--tile_margin", default=argparse.SUPPRESS, type=_margin, metavar="M",
                   help="with --tiles: pixels of the resized image a tile reaches beyond its core on every inner side (default 32)")
    p.add_argument("--tile_scale", default=argparse.SUPPRESS, type=int, choices=[1, 2], metavar="S",
                   help="with --tiles: 2 upsamples every tile bilinearly by 2 before the forward (default 1)")
    p.add_argument("--tile_below", default=argparse.SUPPRESS, type=float, metavar="P",
                   help="with --tiles: tile only the images whose exemplars are small -- mean sqrt(w * h) of the exemplars in resized pixels "
                        "< P; every other image runs whole")
    return p


class _CheckedParser(argparse.ArgumentParser):
    """The 2nd-stage parser with the checks that span two flags: they fail when the command line is parsed, before anything is built."""

    def parse_known_args(self, args=None, namespace=None):
        ns, rest = super().parse_known_args(args, namespace)
        check_render_flags(ns, self.error)
        check_bootstrap_flags(ns, self.error)
        check_tile_flags(ns, self.error)
        return ns, rest


def check_render_flags(ns, fail=None):
    """--render_worst / --render_ids draw what --image_report lists: without it the run stops at start-up."""
    given = [f for f in ("render_worst", "render_ids") if hasattr(ns, f)]
    if given and not getattr(ns, "image_report", False):
        msg = " / ".join("--" + f for f in given) + " needs --image_report: the images to draw are chosen from its report"
        if fail is None:
            raise ValueError(msg)
        fail(msg)
    if hasattr(ns, "render_worst") and ns.render_worst < 0:
        msg = f"--render_worst must not be negative, got {ns.render_worst}"
        if fail is None:
            raise ValueError(msg)
        fail(msg)


def check_bootstrap_flags(ns, fail=None):
    """--bootstrap_seed seeds the draws of --bootstrap: without it the run stops at start-up."""
    if hasattr(ns, "bootstrap_seed") and not hasattr(ns, "bootstrap"):
        msg = "--bootstrap_seed needs --bootstrap R: it seeds the replicates' draws"
        if fail is None:
            raise ValueError(msg)
        fail(msg)


def check_tile_flags(ns, fail=None):
    """--tiles and what goes with it: the three companion flags need it; R * C * Q <= 4096; one image per forward; not inside training."""
    def stop(msg):
        if fail is None:
            raise ValueError(msg)
        fail(msg)
    given = [f for f in ("tile_margin", "tile_scale", "tile_below") if hasattr(ns, f)]
    if not hasattr(ns, "tiles"):
        if given:
            stop(" / ".join("--" + f for f in given) + " needs --tiles RxC: it describes how the tiles are cut")
        return
    from .tiling import check_capacity
    R, C = ns.tiles
    try:
        check_capacity(R, C, int(getattr(ns, "num_query_position", 300)) * int(getattr(ns, "num_query_pattern", 3)))
    except ValueError as e:
        stop(str(e))
    if getattr(ns, "tile_scale", 1) not in (1, 2):
        stop(f"--tile_scale must be 1 or 2, got {ns.tile_scale}")
    if getattr(ns, "tile_margin", 32) < 0:
        stop(f"--tile_margin must not be negative, got {ns.tile_margin}")
    if int(getattr(ns, "eval_batch_size", 1)) > 1:
        stop(f"--tiles forwards the tiles of ONE image as a batch: not with --eval_batch_size {ns.eval_batch_size}")
    if int(getattr(ns, "eval_every", 0)) > 0:
        stop("--tiles with --eval_every: validation inside training is not built for tiles; evaluate the checkpoint with infer.py or main.py --eval")


def _tiles(text):
    """--tiles: `RxC` -> (R, C), both at least 1 (argparse turns the error into a usage error)."""
    from .tiling import parse_tiles
    try:
        return parse_tiles(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def _margin(text):
    """--tile_margin: an integer >= 0."""
    try:
        M = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected an integer, got {text!r}") from None
    if M < 0:
        raise argparse.ArgumentTypeError(f"expected a margin of at least 0 pixels, got {M}")
    return M


def _replicates(text):
    """--bootstrap: an integer in 1 .. 10000 (argparse turns the error into a usage error)."""
    from .bootstrap import MAX_REPLICATES
    try:
        R = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected an integer, got {text!r}") from None
    if not 1 <= R <= MAX_REPLICATES:
        raise argparse.ArgumentTypeError(f"expected 1 .. {MAX_REPLICATES} replicates, got {R}")
    return R


def _seed(text):
    """--bootstrap_seed: an integer in 0 .. 2^63 - 1."""
    try:
        S = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected an integer, got {text!r}") from None
    if not 0 <= S < 2 ** 63:
        raise argparse.ArgumentTypeError(f"expected 0 .. 2^63 - 1, got {S}")
    return S


def _id_list(text):
    """--render_ids: `3,17` -> [3, 17]."""
    return [int(t) for t in text.split(",") if t.strip()]


def _nms_iou(text):
    """--nms_iou: a finite number in [0, 1] (argparse turns the ValueError into a usage error)."""
    from .nms import check_iou
    try:
        return check_iou(float(text))
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def _threshold(text):
    """--threshold: a number, or `ckpt`."""
    return "ckpt" if text == "ckpt" else float(text)


def get_args_parser_stage1():
    """The 1st-stage CLI (A1/main.py:27-132): A1's flags and defaults -- `defined` spatial prior and num_query_pattern 1 as the shipped
    scripts pass them (A1/scripts/weakly_supervise_fscd_147.sh), epochs 30, lr_drop 20, seed 42 -- plus this build's additions."""
    p = argparse.ArgumentParser("Counting-DETR 1st stage (MI355X)", add_help=True)
    p.add_argument("--lr", default=1e-4, type=float)
    p.add_argument("--lr_backbone_names", default=["backbone"], type=str, nargs="+")
    p.add_argument("--lr_backbone", default=1e-5, type=float)
    p.add_argument("--lr_linear_proj_names", default=[], type=str, nargs="+")
    p.add_argument("--lr_linear_proj_mult", default=0.1, type=float)
    p.add_argument("--batch_size", default=1, type=int,
                   help="images per step (the reference: 1; more need equal exemplar counts, or --ragged_batches)")
    p.add_argument("--ragged_batches", action="store_true",
                   help="batches may mix images with different numbers of points (padded, per-image counts on the device): training and --eval "
                        "with any --batch_size; --generate_pseudo_label runs --batch_size same-sized images per forward")
    p.add_argument("--weight_decay", default=1e-4, type=float)
    p.add_argument("--epochs", default=30, type=int)
    p.add_argument("--lr_drop", default=20, type=int)
    p.add_argument("--lr_drop_epochs", default=None, type=int, nargs="+")
    p.add_argument("--clip_max_norm", default=0.1, type=float)
    p.add_argument("--sgd", action="store_true", help="(not supported: AdamW only)")
    p.add_argument("--vis_pseudo", action="store_true", help="(accepted for script compatibility; no visualisation is written)")
    p.add_argument("--frozen_weights", type=str, default=None)
    p.add_argument("--backbone", default="resnet50", type=str)
    p.add_argument("--dilation", default=True, type=lambda s: str(s).lower() not in ("0", "false", "no"))
    p.add_argument("--num_feature_levels", default=1, type=int)
    p.add_argument("--enc_layers", default=6, type=int)
    p.add_argument("--dec_layers", default=6, type=int)
    p.add_argument("--dim_feedforward", default=1024, type=int)
    p.add_argument("--hidden_dim", default=256, type=int)
    p.add_argument("--dropout", default=0.0, type=float)
    p.add_argument("--nheads", default=8, type=int)
    p.add_argument("--num_query_position", default=300, type=int)
    p.add_argument("--num_query_pattern", default=1, type=int)
    p.add_argument("--spatial_prior", default="defined", choices=["learned", "grid", "defined"], type=str)
    p.add_argument("--attention_type", default="RCDA", choices=["RCDA", "nn.MultiheadAttention"], type=str)
    p.add_argument("--masks", action="store_true")
    p.add_argument("--dataset_file", default="fscd_147", choices=["fscd_147", "fscd_147_point"])
    p.add_argument("--data_path", default="./FSC147/", type=str)
    p.add_argument("--output_dir", default="./outputs/fscd_147_1st_stage", type=str)
    p.add_argument("--device", default="cuda")
    p.add_argument("--seed", default=42, type=int)
    p.add_argument("--resume", default="")
    p.add_argument("--auto_resume", default=False, action="store_true")
    p.add_argument("--start_epoch", default=0, type=int)
    p.add_argument("--eval", action="store_true", help="validation loss of the model (A1/engine.py evaluate), then exit")
    p.add_argument("--generate_pseudo_label", action="store_true", help="write pseudo_bbox_{train,val,test}.json, then exit")
    p.add_argument("--num_workers", default=2, type=int)
    p.add_argument("--cache_mode", default=False, action="store_true")
    p.add_argument("--scale_factor", default=32, type=int)
    # additions of this build
    p.add_argument("--synthetic", action="store_true", help="train on seeded synthetic batches (no dataset needed)")
    p.add_argument("--steps_per_epoch", default=20, type=int, help="synthetic mode only")
    p.add_argument("--synthetic_size", default=[384, 576], type=int, nargs=2, help="synthetic mode only: image H W")
    p.add_argument("--print_freq", default=100, type=int, help="the loss is read back every this many steps")
    p.add_argument("--no_graph_cache", dest="graph_cache", action="store_false",
                   help="train with the stream-ordered step instead of cached HIP graphs (one per padded image size / points shape)")
    p.add_argument("--graph_cache_size", default=32, type=int)
    p.add_argument("--device_preprocess", action="store_true",
                   help="the DataLoader workers only decode; resize (PIL-exact), normalisation and padding run on the device in one launch per "
                        "batch (cdetr_image_prep) -- the same image / mask tensors bit for bit")
    p.add_argument("--test", action="store_true",
                   help="for val and test: forward at the centres of the ground-truth boxes of instances_<split>.json and score every predicted "
                        "box against its own ground truth (mean IoU, share of IoU >= 0.5 / 0.75) and as detections (box AP): "
                        "box_scores_<split>.json, then exit")
    p.add_argument("--score_labels", action="store_true",
                   help="with --generate_pseudo_label: box AP of pseudo_bbox_{val,test}.json against instances_<split>.json "
                        "(the offline evaluator's conventions): pseudo_scores_<split>.json")
    p.add_argument("--device_labels", action="store_true",
                   help="with --generate_pseudo_label or --test: the labels leave the forward on the device (cdetr_emit_pseudo_labels, one call "
                        "per batch, one copy back per split); the same json byte for byte, the scores read from device memory")
    p.add_argument("--eval_every", default=0, type=int,
                   help="validate (the loss of --eval, on the live weights) after every N-th epoch and after the last one; the epoch's line in "
                        "log.txt gains test_loss / test_loss_wh / test_loss_giou.  0 = off")
    p.add_argument("--keep_best", default="loss", choices=["loss"],
                   help="with --eval_every: the epoch with the lowest validation loss is also saved to checkpoint_best.pth")
    return p


def default_args(**kw):
    a = get_args_parser().parse_args([])
    a.aux_loss = False            # the shipped scripts all pass --no_aux_loss (A2/scripts/var_wh_laplace_600.sh:7)
    a.num_query_pattern = 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a
