"""main.py -- CLI of the reference's 2nd-stage trainer (A2/main.py:17-258) on the MI355X path.

Same flags, same driver behaviour: build_model -> 3 lr groups / AdamW (SGD, momentum 0.9, with --sgd) / StepLR(lr_drop) -> optional --resume (model
weights only, keys filtered like A2/main.py:195-209) -> per epoch train_one_epoch, scheduler step, checkpoint
{"model","optimizer","lr_scheduler","epoch","args"} to <output_dir>/detr_retrain.pth (+ numbered copies), JSON log line.
Differences: any number of images per GPU (--images_per_gpu), data-parallel over the GPUs of a node under torchrun
(RCCL), and --synthetic (seeded tensors; FSC-147 is not available in this environment -- with a dataset, pass a
DataLoader yielding the reference's sample dicts to `train_one_epoch`).  Without --synthetic the FSC-147 reader of
counting_detr_amd/data.py feeds the step (batched collate + pinned-memory prefetch); with --device_preprocess the workers only decode
and the resize / normalisation / padding of a batch is one launch on the prefetch stream (same tensors bit for bit).
--eval_every N: the validation call the reference left commented out (A2/main.py "Evaluate ...").  After every N-th epoch and the last one rank 0
walks --split through infer.py's loop on the live weights (an InferenceEngine riding on the trainer: no graph is dropped on either side), the
epoch's log line gains test_<k>, and --keep_best {mae,ap,loss} also saves the best epoch to detr_retrain_best.pth ("best" in every checkpoint).
--threshold T / --sweep_thresholds SPEC reach that pass and --eval (infer.py); with --calibrate_threshold {mae,rmse,nae,sre,ap} the sweep's best
threshold follows the test_* keys as test_best_threshold / test_best_<metric> (the test_* keys themselves stay at --threshold) and every checkpoint
written from then on carries "count_threshold": {"metric", "threshold", "value", "epoch"}, which `infer.py --threshold ckpt` reads.
--image_report reaches the same passes (infer.py): six average-recall keys behind the AP keys, image_report_<split>.json wherever the predictions file is written.
--render_worst K / --render_ids (with --image_report) reach them too: render_<split>/ with the box overlays of the report's worst images, beside that file.
--error_report reaches them too: WHY detections fail (duplicate / localisation / background / missed, counting_detr_amd/error_report.py) -- err_* and dAP50_*
in the metrics (test_err_* / test_dAP50_* in the epoch log), error_report_<split>.json wherever the predictions file is written.
--bootstrap R [--bootstrap_seed S] reaches them too: HOW FAR the numbers move when the split is resampled (counting_detr_amd/bootstrap.py) -- <K>_lo / <K>_hi in
the metrics (test_<K>_lo / _hi in the epoch log), bootstrap_<split>.json wherever the predictions file is written; --keep_best and --calibrate_threshold decide as before.
--nms_iou T reaches them too: greedy suppression of duplicate detections ahead of everything that counts them (counting_detr_amd/nms.py), nms_removed in the metrics.

  python main.py --synthetic --no_aux_loss --num_query_pattern 1 --epochs 1 -o /tmp/out
  python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 main.py --synthetic --no_aux_loss ...
"""
import json
import os
import time
from pathlib import Path

import torch

import counting_detr_amd
from counting_detr_amd import checkpoint as ckpt_io
from counting_detr_amd import misc as utils
from counting_detr_amd.args import get_args_parser
from counting_detr_amd.engine import Trainer, count_objects, counting_metrics, train_one_epoch


class SyntheticLoader:
    """Seeded stand-in for FSC147Dataset + DataLoader: yields the step's sample dict (images already on the device)."""

    def __init__(self, args, device, steps, size=(800, 800), targets=(37, 120)):
        self.args, self.device, self.steps, self.size, self.targets = args, device, steps, size, targets

    def __iter__(self):
        B = self.args.images_per_gpu
        H, W = self.size
        rects = torch.tensor([[.10, .10, .20, .20], [.40, .40, .50, .55], [.70, .20, .80, .30]], device=self.device)
        for it in range(self.steps):
            g = torch.Generator().manual_seed(1000003 * utils.get_rank() + it)
            tg = []
            for b in range(B):
                T = self.targets[b % len(self.targets)]
                box = torch.cat([torch.rand(T, 2, generator=g) * 0.8 + 0.1, torch.rand(T, 2, generator=g) * 0.10 + 0.02], 1)
                tg.append({"boxes": box.to(self.device), "labels": torch.zeros(T, dtype=torch.int64, device=self.device)})
            yield {"image": torch.randn(B, 3, H, W, generator=g).to(self.device), "ex_rects": rects[None].repeat(B, 1, 1),
                   "targets": tg}

    def __len__(self):
        return self.steps


class Validator:
    """--eval_every: one pass over --split (infer.py's loop and metrics) on the weights as they stand, between two epochs.  The engine rides on
    the trainer (engine.InferenceEngine(trainer=...)): the trainer's forward weight images, nothing invalidated -- the trainer's captured
    steps and the engine's captured forwards both live on from pass to pass.  Engine and loader are built once."""

    def __init__(self, trainer, criterion, args, device):
        import infer as _infer
        from counting_detr_amd.engine import InferenceEngine
        self._infer, self.trainer, self.criterion, self.args, self.device = _infer, trainer, criterion, args, device
        self.loader, self.per_image = _infer.eval_loader(args, device)
        self.engine = InferenceEngine(trainer.model, _infer.run_threshold(args), graphs=device.type == "cuda", device=device, trainer=trainer)
        self.sweep = None                                               # --sweep_thresholds: the last pass's threshold_sweep.Sweep (its report)

    def run(self, write_json=True):
        try:
            self.sweep = self._infer.build_sweep(self.args)
            return self._infer.evaluate_split(self.trainer.model, self.criterion, self.loader, self.per_image, self.device, self.args,
                                              engine=self.engine, write_json=write_json, sweep=self.sweep)
        finally:
            self.trainer.model.train()
            self.criterion.train()


def main(args):
    utils.init_distributed_mode(args)
    os.makedirs(args.output_dir, exist_ok=True)
    if getattr(args, "image_report", False) and not args.synthetic and (args.eval or args.eval_every > 0):
        import infer as _infer
        _infer.build_image_report(args)         # without instances_<split>.json: an error now, not after the epochs
    if getattr(args, "error_report", False) and not args.synthetic and (args.eval or args.eval_every > 0):
        import infer as _infer
        _infer.build_error_report(args)         # likewise
    device = torch.device(args.device if not getattr(args, "distributed", False) else f"cuda:{args.gpu}")
    # every rank builds the SAME initial weights (the init draws from the global RNG); only the data order is rank-specific.
    # Trainer additionally broadcasts rank 0's parameters and buffers (what DistributedDataParallel does at construction).
    torch.manual_seed(args.seed)
    # arithmetic of the backward contractions: handed to the trainer, which owns its arithmetic (ops.arithmetic) -- no module global is flipped
    bwd_precision = {"bf16": 3, "bf16x2": 2, "bf16x3": 1}[args.bwd_precision] if getattr(args, "bwd_precision", None) else None
    model, criterion, _ = counting_detr_amd.build_model(args)
    model.to(device)
    if args.pretrained_backbone:                                        # A2/models/backbone.py:153-155 -> resnet.py:292-297
        n = ckpt_io.load_backbone_pretrained(model, args.pretrained_backbone)
        print(f"backbone: {n} tensors from {args.pretrained_backbone}")

    checkpoint = None
    if args.auto_resume and not args.resume:                            # A1/main.py:217-221: continue from the output directory's last checkpoint
        last = os.path.join(args.output_dir, "detr_retrain.pth")
        if os.path.isfile(last):
            args.resume = last
    if args.resume:                                                     # A2/main.py:195-209
        checkpoint, _, _ = ckpt_io.resume_model(model, args.resume, skip_mismatch=args.resume_skip_mismatch)

    trainer = Trainer(model, criterion, args, device=device, precision_bwd=bwd_precision)           # 3 lr groups + flat AdamW or --sgd SGD (A2/main.py:157-189); syncs replicas; owns its arithmetic
    if utils.is_main_process():
        print(f"optimizer: {trainer.optimizer_name}" + (" (momentum 0.9)" if trainer.sgd else "") + f", lr {args.lr}, backbone lr {args.lr_backbone}, "
              f"weight decay {args.weight_decay}, clip {args.clip_max_norm}")
    if checkpoint is not None and (args.resume_optimizer or args.auto_resume) and checkpoint.get("optimizer"):
        # opt-in (the reference loads weights only and starts at --start_epoch, A2/main.py:195-209): continue an interrupted run
        trainer.load_state_dict(checkpoint["optimizer"], checkpoint.get("lr_scheduler"))
        resumed = int(checkpoint.get("epoch", -1)) + 1
        if resumed > args.start_epoch:
            print(f"resume: optimizer state restored, continuing at epoch {resumed} (checkpoint epoch {resumed - 1})")
            args.start_epoch = resumed
    # --eval_every: validation inside the run, on the trainer's own weight images (engine.InferenceEngine(trainer=...)), + the best checkpoint
    keeper = validator = last_metrics = count_threshold = None
    calibrate = getattr(args, "calibrate_threshold", None)
    if calibrate and not (args.eval_every > 0 and getattr(args, "sweep_thresholds", None)):
        raise SystemExit("--calibrate_threshold picks from a validation pass's sweep: it needs --eval_every N and --sweep_thresholds SPEC")
    if args.eval_every > 0:
        if args.synthetic:
            raise SystemExit("--eval_every validates on a dataset split: not with --synthetic")
        if calibrate == "ap" and not os.path.isfile(os.path.join(args.data_path, "instances_" + args.split + ".json")):
            raise SystemExit("--calibrate_threshold ap needs the split's box ground truth (instances_<split>.json): it is not there")
        if checkpoint is not None and (args.resume_optimizer or args.auto_resume):
            count_threshold = checkpoint.get("count_threshold")          # a resumed run keeps the calibration until its next calibrated pass
        keeper = ckpt_io.BestKeeper(args.keep_best, os.path.isfile(os.path.join(args.data_path, "instances_" + args.split + ".json")))
        if checkpoint is not None and (args.resume_optimizer or args.auto_resume):
            keeper.load(checkpoint.get("best"))           # a resumed run never overwrites a better detr_retrain_best.pth with a worse one
    if args.start_epoch >= args.epochs:
        print(f"nothing to train: start epoch {args.start_epoch} >= --epochs {args.epochs}")
    torch.manual_seed(args.seed + 1 + utils.get_rank())                 # data-side RNG (synthetic batches, augmentation)
    sampler = None
    if args.synthetic:
        loader = SyntheticLoader(args, device, args.steps_per_epoch, size=tuple(args.synthetic_size))
    else:                                                               # A2/main.py:146-147 (+ batching, sharding, prefetch)
        from torch.utils.data import DataLoader, DistributedSampler
        from counting_detr_amd import data
        raw = bool(getattr(args, "device_preprocess", False))            # workers decode only; the Prefetcher launches cdetr_image_prep
        ds = data.build_dataset(args, raw=raw)
        sampler = DistributedSampler(ds, shuffle=True, seed=args.seed) if getattr(args, "distributed", False) else None
        dl = DataLoader(ds, batch_size=args.images_per_gpu, shuffle=(sampler is None), sampler=sampler,
                        collate_fn=data.collate_raw if raw else data.collate, num_workers=args.num_workers, drop_last=True, pin_memory=False)
        loader = data.Prefetcher(dl, device)
    print("Start training")
    start = time.time()
    output_dir = Path(args.output_dir)
    for epoch in range(args.start_epoch, args.epochs):
        if sampler is not None:
            sampler.set_epoch(epoch)           # a different shuffle (and rank sharding) every epoch
        stats = train_one_epoch(trainer, loader, epoch, print_freq=10)
        trainer.lr_scheduler_step()
        paths = [output_dir / "detr_retrain.pth"]
        if (epoch + 1) % args.lr_drop == 0 or (epoch + 1) % 10 == 0:
            paths.append(output_dir / f"detr_retrain_{epoch:04}.pth")
        test_stats = None
        if keeper is not None and ckpt_io.validation_due(epoch, args.eval_every, args.epochs):
            if utils.is_main_process():        # rank 0 validates (the whole split), the other ranks wait in the barrier below
                if validator is None:          # built once: the engine's captured forwards and the loader serve every later pass
                    validator = Validator(trainer, criterion, args, device)
                last_metrics = validator.run(write_json=epoch + 1 == args.epochs)      # the run leaves the last pass's predictions file
                test_stats = {"loss": ckpt_io.weighted_loss(last_metrics, criterion.weight_dict), **last_metrics}
                if keeper.update(test_stats, epoch):
                    paths.append(output_dir / "detr_retrain_best.pth")
                if calibrate:   # the sweep's best threshold of this pass: behind the test_* keys, and into the checkpoints from here on
                    from counting_detr_amd.threshold_sweep import calibration
                    found = calibration(validator.sweep.report, calibrate, epoch) if validator.sweep.report else None
                    if found is not None:
                        count_threshold = found
                        test_stats["best_threshold"], test_stats["best_" + calibrate] = found["threshold"], found["value"]
            if utils.is_dist_avail_and_initialized():
                torch.distributed.barrier()
        if utils.is_main_process():            # only rank 0 pays for the host copy of the moments
            ckpt = {"model": model.state_dict(), "optimizer": trainer.state_dict(), "lr_scheduler": trainer.lr_scheduler_state_dict(),
                    "epoch": epoch, "args": args}
            if keeper is not None:
                ckpt["best"] = keeper.state()
            if count_threshold is not None:
                ckpt["count_threshold"] = dict(count_threshold)
            for p in paths:
                torch.save(ckpt, p)
        if utils.is_main_process():
            with (output_dir / "detr_retrain.txt").open("a") as f:
                f.write(json.dumps(ckpt_io.epoch_log_line(stats, test_stats, epoch)) + "\n")
    print("time: ", time.time() - start)
    if args.eval and last_metrics is not None:                          # --eval_every already ran this pass after the last epoch
        print("counting metrics ({}): {}".format(args.split, json.dumps(last_metrics)))
    elif args.eval and not args.synthetic:                              # counting evaluation on the validation split (A2/infer.py)
        if utils.is_main_process():
            import infer as _infer
            dl, per_image = _infer.eval_loader(args, device)           # --eval_batch_size: batches of one resized size, per-image losses
            on_device = bool(getattr(args, "device_detections", False))      # post-forward work + box AP on the device (infer.py)
            gt_json = os.path.join(args.data_path, "instances_" + args.split + ".json")
            metrics, _ = _infer.infer(model, criterion, dl, device, args.output_dir, split=args.split, threshold=_infer.run_threshold(args),
                                      device_detections=on_device, gt_json=gt_json if on_device and os.path.isfile(gt_json) else None,
                                      per_image=per_image, sweep=_infer.build_sweep(args), image_report=_infer.build_image_report(args, device),
                                      render=_infer.build_render(args), nms_iou=getattr(args, "nms_iou", None),
                                      error_report=_infer.build_error_report(args, device), bootstrap=_infer.build_bootstrap(args, device),
                                      tiles=_infer.build_tiling(args))
            print("counting metrics ({}): {}".format(args.split, json.dumps(metrics)))
    if args.eval and args.synthetic:                                    # counting rule + MAE on the synthetic shard
        pred, gt = [], []
        for ret in SyntheticLoader(args, device, 2):
            counts, _, _, _ = count_objects(model, ret["image"], ret["ex_rects"])
            pred += [int(c) for c in counts]
            gt += [len(t["boxes"]) for t in ret["targets"]]
        print("counting metrics (synthetic):", counting_metrics(pred, gt))


if __name__ == "__main__":
    a = get_args_parser().parse_args()
    if a.output_dir:
        Path(a.output_dir).mkdir(parents=True, exist_ok=True)
    main(a)
