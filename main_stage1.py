"""main_stage1.py -- CLI of the reference's 1st-stage trainer (A1/main.py, A1 = src/CountDETR_147_1st_stage) on the MI355X path.

Same flags, same driver: stage1.build -> three lr groups / AdamW / StepLR(lr_drop) + clip 0.1 (engine.Stage1Trainer) -> optional --resume
(model weights, `transformer.pattern.weight` filtered, so the COCO Anchor-DETR checkpoint loads) -> per epoch train_one_epoch, scheduler
step, checkpoint {"model","optimizer","lr_scheduler","epoch","args"} to <output_dir>/checkpoint.pth (+ checkpoint<epoch:04>.pth at lr_drop
and every 10 epochs), one JSON line per epoch in log.txt.
  --eval                   validation loss (A1/engine.py evaluate) of the model, then exit (A1's own --eval then unpacks a COCO evaluator
                           that evaluate never returns and crashes: not reproduced)
  --generate_pseudo_label  load --resume and write pseudo_bbox_{train,val,test}.json (the 2nd stage's training labels), then exit
  --score_labels           with --generate_pseudo_label: box AP of the val / test files against instances_<split>.json (the offline
                           evaluator's conventions, stage1.score_pseudo_labels) -> pseudo_scores_<split>.json
  --test                   load --resume, forward val / test at the centres of their ground-truth boxes and score every predicted box against
                           its own ground truth (stage1.score_boxes_at_gt) -> box_scores_<split>.json, then exit (A1's own --test reads
                           outputs["pred_boxes"] through a PostProcess the 1st-stage model does not feed: not reproduced)
  --device_labels          with either of the two: one cdetr_emit_pseudo_labels call per batch instead of the per-annotation host loop, one
                           copy back per split, the scores straight from device memory; the same files byte for byte
  --eval_every N           the validation loss of --eval after every N-th epoch and after the last, on the live weights: test_loss /
                           test_loss_wh / test_loss_giou in the epoch's log line; the epoch with the lowest loss is also saved to
                           checkpoint_best.pth and every checkpoint carries "best" = {"metric", "value", "epoch"} (--keep_best loss)
  --auto_resume            continue from <output_dir>/checkpoint.pth: weights, AdamW moments, StepLR state and the next epoch
  --synthetic              seeded batches, no dataset
  --ragged_batches         batches may mix images with different numbers of points (padded to the batch maximum, per-image counts read by
                           the kernels): training with any --batch_size on a real split, --eval likewise, and --generate_pseudo_label
                           runs --batch_size images of one resized size per forward
Differences: any number of images per step (--batch_size; the reference trains batch 1) -- with equal exemplar counts, or any counts
with --ragged_batches -- and the step runs as cached HIP graphs (--no_graph_cache: stream-ordered).  --sgd and multi-GPU training are
not supported.

  python main_stage1.py --data_path ./FSC147/ --output_dir ./outputs/fscd_147_1st_stage --resume ./pretrained_models/AnchorDETR_r50_c5.pth
  python main_stage1.py --data_path ./FSC147/ --output_dir ./outputs/fscd_147_1st_stage --dataset_file fscd_147_point \\
      --generate_pseudo_label --resume ./outputs/fscd_147_1st_stage/checkpoint.pth
"""
import json
import os
import time
from pathlib import Path

import torch

from counting_detr_amd import checkpoint as ckpt_io
from counting_detr_amd import stage1
from counting_detr_amd.args import get_args_parser_stage1
from counting_detr_amd.engine import Stage1Trainer, train_one_epoch


class SyntheticLoader:
    """Seeded stand-in for FSC147ExemplarDataset + DataLoader: yields the step's batch dict (on the device)."""

    def __init__(self, args, device, steps, size=(384, 576), npts=3):
        self.args, self.device, self.steps, self.size, self.npts = args, device, steps, size, npts

    def __iter__(self):
        B = self.args.batch_size
        H, W = self.size
        for it in range(self.steps):
            g = torch.Generator().manual_seed(1000003 + it)
            yield {"image": torch.randn(B, 3, H, W, generator=g).to(self.device),
                   "points": (torch.rand(B, self.npts, 2, generator=g) * 0.6 + 0.2).to(self.device),
                   "whs": (torch.rand(B, self.npts, 2, generator=g) * 0.15 + 0.03).to(self.device)}

    def __len__(self):
        return self.steps


def to_device(loader, device):
    for b in loader:
        yield {k: (v.to(device, non_blocking=True) if torch.is_tensor(v) else v) for k, v in b.items()}


def loader_for(args, split, points=False, shuffle=False, device=None, boxes=False):
    """The split's DataLoader (host tensors).  --device_preprocess: its workers only decode and a data.Prefetcher on `device` yields device
    batches whose image / mask come from one cdetr_image_prep launch -- the same tensors bit for bit.  boxes=True (with points): the
    points are the centres of the split's ground-truth boxes (data.FSC147BoxPointsDataset)."""
    from torch.utils.data import DataLoader
    from counting_detr_amd import data
    raw = bool(getattr(args, "device_preprocess", False))
    ragged = bool(getattr(args, "ragged_batches", False))
    if points and boxes:
        ds = data.build_box_points_dataset(args, split, raw=raw)
    else:
        ds = data.build_points_dataset(args, split, raw=raw) if points else data.build_dataset_stage1(args, split, raw=raw)
    if ragged:
        collate_fn = data.collate_stage1_ragged_raw if raw else data.collate_stage1_ragged
    else:
        collate_fn = data.collate_stage1_raw if raw else data.collate_stage1
    if points and ragged:                      # pseudo labels: --batch_size images of ONE resized size per forward, in a fixed order
        dl = DataLoader(ds, batch_sampler=data.SizeBucketBatchSampler(ds, args.batch_size), collate_fn=collate_fn, num_workers=args.num_workers)
    else:
        dl = DataLoader(ds, batch_size=1 if points else args.batch_size, shuffle=shuffle, collate_fn=collate_fn, num_workers=args.num_workers,
                        drop_last=shuffle)
    return data.Prefetcher(dl, device) if raw else dl


@torch.no_grad()
def evaluate(model, criterion, loader, device):
    """A1/engine.py evaluate: mean over the batches of the validation losses (loss = weighted total, loss_wh, loss_giou)."""
    from counting_detr_amd.misc import NestedTensor
    model.eval()
    acc, n = None, 0
    for ret in to_device(loader, device):
        counts = ret.get("counts")             # --ragged_batches: the model and the criterion see each image's own points only
        out = model(NestedTensor(ret["image"], ret["mask"]), ret["points"], counts)
        targets = {"points": ret["points"], "whs": ret["whs"]}
        if counts is not None:
            targets["counts"] = counts
        ld, total = criterion.forward_with_total(out, targets)
        v = torch.stack([total, ld["loss_wh"], ld["loss_giou"]])
        acc = v if acc is None else acc + v
        n += 1
    model.train()
    if n == 0:
        return {}
    acc = (acc / n).tolist()
    return {"loss": acc[0], "loss_wh": acc[1], "loss_giou": acc[2], "batches": n}


def write_scores(path, scores):
    """Print a score dict and write it as json (NaN for an undefined number, as json.dump spells it)."""
    print(f"{path.name}:", json.dumps(scores))
    with open(path, "w") as f:
        json.dump(scores, f)


def main(args):
    device = torch.device(args.device)
    torch.manual_seed(args.seed)
    model, criterion, _ = stage1.build(args)
    model.to(device)
    criterion.fused = True                     # one launch (ops.BBoxCriterionFn); the validation loss goes through it as well
    output_dir = Path(args.output_dir)
    os.makedirs(output_dir, exist_ok=True)
    if args.auto_resume:                       # A1/main.py:218-222
        if not args.resume:
            args.resume = str(output_dir / "checkpoint.pth")
        if not os.path.isfile(args.resume):
            args.resume = ""

    if args.generate_pseudo_label or args.test:  # A1/main.py:247-286: the checkpoint as it is (strict=False), then the splits
        ckpt = ckpt_io._read(args.resume)
        missing, unexpected = model.load_state_dict(ckpt["model"] if "model" in ckpt else ckpt, strict=False)
        ckpt_io.invalidate_caches(model)
        if missing:
            print("Missing Keys: {}".format(missing))
        if unexpected:
            print("Unexpected Keys: {}".format(unexpected))
        if args.test:
            for split in ("val", "test"):
                scores = stage1.score_boxes_at_gt(model, loader_for(args, split, points=True, device=device, boxes=True), split,
                                                  os.path.join(args.data_path, f"instances_{split}.json"), args.output_dir, device=device,
                                                  device_labels=args.device_labels)
                write_scores(output_dir / f"box_scores_{split}.json", scores)
            return
        for split in ("train", "val", "test"):
            ann, store = stage1.write_pseudo_labels(model, loader_for(args, split, points=True, device=device), split, args.output_dir,
                                                    device=device, device_labels=args.device_labels, return_store=True)
            print(f"pseudo_bbox_{split}.json: {len(ann['images'])} images, {len(ann['annotations'])} boxes")
            if not args.score_labels:
                continue
            gt_json = os.path.join(args.data_path, f"instances_{split}.json")
            if split == "train" or not os.path.isfile(gt_json):
                print(f"pseudo_bbox_{split}.json: not scored, the split has no box ground truth (instances_{split}.json)")
                continue
            write_scores(output_dir / f"pseudo_scores_{split}.json", stage1.score_pseudo_labels(ann, gt_json, store=store))
        return

    checkpoint = None
    if args.resume:                            # A1/main.py:224-239 (weights; transformer.pattern.weight filtered)
        checkpoint, _, _ = ckpt_io.resume_model(model, args.resume)

    if args.eval:
        stats = evaluate(model, criterion, loader_for(args, "val", device=device), device)
        print("validation:", json.dumps(stats))
        return

    trainer = Stage1Trainer(model, criterion, args, device=device)
    if checkpoint is not None and args.auto_resume and checkpoint.get("optimizer"):
        trainer.load_state_dict(checkpoint["optimizer"], checkpoint.get("lr_scheduler"))
        resumed = int(checkpoint.get("epoch", -1)) + 1
        if resumed > args.start_epoch:
            print(f"resume: optimizer state restored, continuing at epoch {resumed}")
            args.start_epoch = resumed
    keeper = val_loader = None
    if args.eval_every > 0:                    # the loss of --eval on the live weights, between epochs (+ checkpoint_best.pth)
        if args.synthetic:
            raise SystemExit("--eval_every validates on the val split: not with --synthetic")
        keeper = ckpt_io.BestKeeper(args.keep_best)
        if checkpoint is not None and args.auto_resume:
            keeper.load(checkpoint.get("best"))
        val_loader = loader_for(args, "val", device=device)       # the loader --eval builds (--ragged_batches honoured), built once
    torch.manual_seed(args.seed + 1)
    n_parameters = sum(p.numel() for p in model.parameters() if p.requires_grad)
    print("Start training")
    start = time.time()
    for epoch in range(args.start_epoch, args.epochs):
        if args.synthetic:
            loader = SyntheticLoader(args, device, args.steps_per_epoch, size=tuple(args.synthetic_size))
        else:
            loader = to_device(loader_for(args, "train", shuffle=True, device=device), device)
        stats = train_one_epoch(trainer, loader, epoch, print_freq=args.print_freq)
        trainer.lr_scheduler_step()
        paths = [output_dir / "checkpoint.pth"]
        if (epoch + 1) % args.lr_drop == 0 or (epoch + 1) % 10 == 0:
            paths.append(output_dir / f"checkpoint{epoch:04}.pth")
        test_stats = None
        if keeper is not None and ckpt_io.validation_due(epoch, args.eval_every, args.epochs):
            # eager, no weight mirror in force, nothing invalidated: the trainer's captured steps stay (evaluate leaves the model in train mode)
            test_stats = {k: v for k, v in evaluate(model, criterion, val_loader, device).items() if k.startswith("loss")}
            if keeper.update(test_stats, epoch):
                paths.append(output_dir / "checkpoint_best.pth")
        ckpt = {"model": model.state_dict(), "optimizer": trainer.state_dict(), "lr_scheduler": trainer.lr_scheduler_state_dict(),
                "epoch": epoch, "args": args}
        if keeper is not None:
            ckpt["best"] = keeper.state()
        for p in paths:
            torch.save(ckpt, p)
        with (output_dir / "log.txt").open("a") as f:
            f.write(json.dumps(ckpt_io.epoch_log_line(stats, test_stats, epoch, n_parameters=n_parameters)) + "\n")
    print("Training time {:.1f} s".format(time.time() - start))


if __name__ == "__main__":
    a = get_args_parser_stage1().parse_args()
    if a.output_dir:
        Path(a.output_dir).mkdir(parents=True, exist_ok=True)
    main(a)
