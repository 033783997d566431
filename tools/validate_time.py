"""What validation inside a training run costs (main.py --eval_every), and what the only alternative before it cost.

  tree     = the tree of tests/validate_tree.py (four training images of two sizes, five validation images of two sizes) enlarged by
             repetition (--times, default 8: 32 training and 40 validation images); seeded weights (init.seeded_init_), Q = 100;
  epoch    = engine.train_one_epoch over main.py's loader (batches of two, shuffled, data.Prefetcher), wall time with a device
             synchronisation on both sides; the first epoch captures the step graphs and is reported apart;
  pass     = main.Validator.run (infer.py's loop through an InferenceEngine riding on the trainer, --device_detections) at
             --eval_batch_size 1 and 8: wall time and engine captures of the first and of the second pass, then the `graph_captures` and the
             wall time of the training epoch that follows;
  parent   = a plain InferenceEngine(model) built between two epochs (checkpoint.invalidate_caches: the trainer's graphs and mirror go), one
             pass through it, then the next epoch's `graph_captures` and wall time.

No threshold is set on any time: none of these numbers existed before.

usage: python tools/validate_time.py [--out profiles/validate_time.json] [--times 8]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch


def enlarge(root, times):
    """Every image of the tree `times` times over (copies under new names and ids), in all of its json files."""
    def load(fn):
        with open(os.path.join(root, fn)) as f:
            return json.load(f)
    anno, split = load("annotation_FSC147_384.json"), load("Train_Test_Val_FSC_147.json")
    cocos = {fn: load(fn) for fn in ("instances_val.json", os.path.join("annotations", "pseudo_bbox_train.json"))}
    for r in range(1, times):
        for part in ("train", "val"):
            for name in [n for n in split[part] if not n.startswith("r")]:
                new = f"r{r}_{name}"
                shutil.copy(os.path.join(root, "images_384_VarV2", name), os.path.join(root, "images_384_VarV2", new))
                anno[new] = anno[name]
                split[part].append(new)
        for coco in cocos.values():
            for im in [im for im in coco["images"] if not im["file_name"].startswith("r")]:
                coco["images"].append({**im, "id": im["id"] + 1000 * r, "file_name": f"r{r}_{im['file_name']}"})
            n0 = len([a for a in coco["annotations"] if a["image_id"] < 1000])
            for a in coco["annotations"][:n0]:
                coco["annotations"].append({**a, "id": a["id"] + 100000 * r, "image_id": a["image_id"] + 1000 * r})
    for fn, obj in (("annotation_FSC147_384.json", anno), ("Train_Test_Val_FSC_147.json", split), *cocos.items()):
        with open(os.path.join(root, fn), "w") as f:
            json.dump(obj, f)
    return len(split["train"]), len(split["val"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validate_time.json"))
    ap.add_argument("--times", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("validate_time: needs an MI355X (nothing is measured on the CPU)")
    import infer as infer_mod
    import main as main_mod
    import validate_tree as vt
    from torch.utils.data import DataLoader
    from counting_detr_amd import build_model, data
    from counting_detr_amd.args import get_args_parser
    from counting_detr_amd.engine import InferenceEngine, Trainer, train_one_epoch
    from counting_detr_amd.init import seeded_init_
    dev = torch.device("cuda", 0)
    quiet = lambda *x: None      # noqa: E731
    with torch.cuda.device(dev), tempfile.TemporaryDirectory() as tmp:
        root = vt.write_tree(os.path.join(tmp, "ds"))
        n_train, n_val = enlarge(root, a.times)
        args = get_args_parser().parse_args(["-dp", root, "-o", os.path.join(tmp, "out"), "--images_per_gpu", "2", "--device", str(dev), "--seed", "2",
                                             "--device_detections", "--eval_every", "1", *vt.MODEL_FLAGS])
        os.makedirs(args.output_dir)
        torch.manual_seed(args.seed)
        model, criterion, _ = build_model(args)
        seeded_init_(model)
        model.to(dev)
        trainer = Trainer(model, criterion, args, device=dev)
        torch.manual_seed(args.seed + 1)
        loader = data.Prefetcher(DataLoader(data.build_dataset(args), batch_size=args.images_per_gpu, shuffle=True, collate_fn=data.collate,
                                            num_workers=0, drop_last=True), dev)
        epoch_no = [0]

        def epoch():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stats = train_one_epoch(trainer, loader, epoch_no[0], print_freq=10 ** 9, log=quiet)
            torch.cuda.synchronize()
            epoch_no[0] += 1
            return {"wall_s": time.perf_counter() - t0, "steps": stats["graph_steps"], "graph_captures": stats["graph_captures"]}

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        res = {"first_epoch": epoch(), "epoch": epoch(), "passes": []}
        print(json.dumps(res), flush=True)
        for B in (1, 8):
            args.eval_batch_size = B
            val = main_mod.Validator(trainer, criterion, args, dev)
            row = {"eval_batch_size": B, "images": n_val}
            for name in ("first_pass", "second_pass"):
                c0 = val.engine.stats["captures"]
                wall, metrics = timed(lambda: val.run(write_json=False))
                row[name] = {"wall_s": wall, "engine_captures": val.engine.stats["captures"] - c0, "images": metrics["images"]}
            row["epoch_after"] = epoch()
            print(json.dumps(row), flush=True)
            res["passes"].append(row)
        # the parent's only alternative: a plain engine on the model being trained, built between two epochs
        args.eval_batch_size = 8
        dl, per_image = infer_mod.eval_loader(args, dev)
        build_s, plain = timed(lambda: InferenceEngine(model, device=dev))
        c0 = plain.stats["captures"]
        pass_s, metrics = timed(lambda: infer_mod.evaluate_split(model, criterion, dl, per_image, dev, args, engine=plain, write_json=False))
        model.train()
        criterion.train()
        res["plain_engine_between_epochs"] = {"eval_batch_size": 8, "build_s": build_s, "pass_s": pass_s, "engine_captures": plain.stats["captures"] - c0,
                                              "images": metrics["images"], "epoch_after": epoch(), "epoch_after_that": epoch()}
        print(json.dumps(res["plain_engine_between_epochs"]), flush=True)
    res = {"what": "main.py --eval_every on the tree of tests/validate_tree.py repeated %d times (%d training, %d validation images; two image "
                   "sizes each, seeded weights, Q = 100, batches of two): wall time of a training epoch (engine.train_one_epoch, device "
                   "synchronised on both sides), of a validation pass through an InferenceEngine riding on the trainer (main.Validator, "
                   "--device_detections) at --eval_batch_size 1 and 8, first pass (captures its forwards) and second, and the graph captures "
                   "and wall time of the epoch after; then the same for a plain InferenceEngine(model) built between two epochs, which "
                   "invalidates the trainer's graphs and mirror.  One run, no repeats: the times are single samples." % (a.times, n_train, n_val),
           "device": torch.cuda.get_device_name(0), **res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
