"""Image preparation, host path against device path (--device_preprocess), on generated FSC-147-format JPEG sets: 683 x 384 files (resized to
672 x 384 by the training reader) and 1350 x 810 files (1344 x 800, the detection-size class).  Recorded, no threshold:
  * host ms per image by stage on one worker (one thread, in this process): decode, resize, to_normalized_tensor, padding into the batch for
    the host path; decode, RGB bytes, packing for the device path;
  * H2D bytes per batch of 2 on either path;
  * cdetr_image_prep's time for a batch of 2 (HIP events around the launch, best of --repeats after a warm-up), both sizes;
  * loader-only images/s at --num_workers 2: DataLoader + collate + Prefetcher (copies; on the device path also the kernel), nothing consumed;
  * beside it the trainer's step rate at 384 x 672 (bench.extra_shape: graph replay, 2 images per step).
The batches of both paths are asserted torch.equal.

usage: python tools/image_prep_time.py [--out profiles/image_prep_time.json] [--images 64] [--repeats 20] [--no-step-rate]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch
from PIL import Image
from torch.utils.data import DataLoader

from counting_detr_amd import data, ops
import image_prep_ref as ref


def photo_like(h, w, seed):
    """Smooth structure + mild noise: a JPEG of it decodes at a photograph's cost, not at white noise's."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    a = np.stack([127 + 90 * np.sin(xx / (17 + 5 * c) + seed) * np.cos(yy / (23 - 4 * c)) for c in range(3)], axis=2)
    return Image.fromarray((a + rng.normal(0, 6, a.shape)).clip(0, 255).astype(np.uint8))


def best_ms(fn, n):
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def host_stages(path, n):
    """ms per image of each stage of either path, one thread."""
    def opened():
        im = Image.open(path)
        im.load()
        return im
    im = opened()
    w, h = im.size
    size = (32 * int(w / 32), 32 * int(h / 32))
    r = im.resize(size)
    t = data.to_normalized_tensor(r)
    host = {"decode": best_ms(opened, n), "bicubic_resize": best_ms(lambda: im.resize(size), n),
            "to_normalized_tensor": best_ms(lambda: data.to_normalized_tensor(r), n),
            "pad_into_the_batch": best_ms(lambda: ref.host_batch([{"image": t}, {"image": t}]), n) / 2}
    s = data._raw_image(im, size, None)
    dev = {"decode": host["decode"], "rgb_bytes": best_ms(lambda: data._raw_image(im, size, None), n),
           "pack_into_the_batch": best_ms(lambda: data.pack_raw([s, s]), n) / 2}
    host["total"], dev["total"] = sum(host.values()), sum(dev.values())
    return {"source": [h, w], "resized": [size[1], size[0]], "host_path_ms_per_image": host, "device_path_ms_per_image": dev}


def kernel_time(path, dev, repeats):
    im = Image.open(path)
    w, h = im.size
    s = data._raw_image(im, (32 * int(w / 32), 32 * int(h / 32)), None)
    raw = data.pack_raw([s, s])
    h2d_dev = sum(v.numel() * v.element_size() for v in raw.values() if torch.is_tensor(v))
    want_i, want_m = ref.host_batch([{"image": data.to_normalized_tensor(im.resize(s["resize_to"]))}] * 2)
    h2d_host = want_i.numel() * 4 + want_m.numel()
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in raw.items()}
    image, mask = ops.image_prep(d)
    assert torch.equal(image.cpu(), want_i) and torch.equal(mask.cpu(), want_m)
    ms = []
    for _ in range(repeats):
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ops.image_prep(d, events=ev)
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    out_bytes = image.numel() * 4 + mask.numel()
    k = float(np.median(ms))
    return {"batch": 2, "source": [h, w], "output": list(image.shape[2:]), "kernel_ms_median": k, "kernel_ms_min": float(min(ms)), "repeats": repeats,
            "h2d_bytes_host_path": h2d_host, "h2d_bytes_device_path": h2d_dev, "h2d_ratio": h2d_dev / h2d_host,
            "kernel_GB_per_s_read_plus_written": (raw["pixels"].numel() + out_bytes) / k / 1e6, "equal_to_host_path": True}


def loader_rate(root, dev, raw, workers, epochs=3):
    a = argparse.Namespace(data_path=root, scale_factor=32)
    ds = data.FSC147Dataset(a, raw=raw)
    dl = DataLoader(ds, batch_size=2, shuffle=False, collate_fn=data.collate_raw if raw else data.collate, num_workers=workers, drop_last=True,
                    persistent_workers=workers > 0)
    p = data.Prefetcher(dl, dev)
    for _ in p:                                      # warm-up epoch: worker start, file cache, pinned allocations
        pass
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for _ in range(epochs):
        for b in p:
            n += b["image"].shape[0]
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_prep_time.json"))
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--num_workers", type=int, default=2)
    ap.add_argument("--no-step-rate", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.set_num_threads(1)
    res = {"what": "image preparation per batch: host path (PIL resize + to_normalized_tensor in the workers, collate pads, fp32 copy) vs device "
                   "path (workers decode, uint8 copy, one cdetr_image_prep launch); both paths' batches torch.equal",
           "device": torch.cuda.get_device_name(0), "host_cpus_usable": len(os.sched_getaffinity(0)), "sizes": []}
    with tempfile.TemporaryDirectory() as tmp:
        for tag, (h, w) in (("fsc147", (384, 683)), ("detection", (810, 1350))):
            root = os.path.join(tmp, tag)
            n = a.images if tag == "fsc147" else max(a.images // 4, 8)
            ref.write_fsc147(root, [photo_like(h, w, i) for i in range(n)], name_fmt="{}.jpg")
            first = os.path.join(root, "images_384_VarV2", "1.jpg")
            row = {"set": tag, "files": n, **host_stages(first, a.repeats), "kernel": kernel_time(first, dev, a.repeats)}
            row["loader_only_images_per_s"] = {"num_workers": a.num_workers, "host_path": loader_rate(root, dev, False, a.num_workers),
                                               "device_path": loader_rate(root, dev, True, a.num_workers)}
            print(json.dumps(row), flush=True)
            res["sizes"].append(row)
    if not a.no_step_rate:
        import bench
        leg = bench.extra_shape(dev, 384, 672, 300, "learned", (37, 120), 2, "bf16x3", steps=10)
        res["trainer_step"] = {"what": "Trainer graph replay, 384 x 672, 2 images per step, 300 queries (bench.extra_shape)", "images_per_s": leg["value"],
                               "ms_per_step": leg["ms_per_step"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
