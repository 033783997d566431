"""cdetr_image_prep (csrc/image_prep.hip) against the HOST path -- PIL's resize, to_normalized_tensor, collate -- with torch.equal on image
and mask: no tolerance.  The equality tests route no image to the host and say so (device_resampled == number of images); the routing
tests are separate and named as such.  tests/test_image_prep_cpu.py holds the tables and the numpy restatement to the same target."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import image_prep_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TINY = os.path.join(HERE, "golden", "fsc147_tiny")
LVIS = os.path.join(HERE, "golden", "fscd_lvis_tiny")


def _device(raw):
    from counting_detr_amd import ops
    image, mask = ops.image_prep({k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in raw.items()})
    torch.cuda.synchronize()
    return image.cpu(), mask.cpu()


def _equal_to_host(items, expect_routed=0):
    """items: [(pixels uint8 [h, w, 3] or [h, w], (out_h, out_w), filter)] -> one batch on the device == the host path's batch."""
    from counting_detr_amd import data
    raw = data.pack_raw([ref.raw_sample(a, o, f) for a, o, f in items])
    assert raw["device_resampled"] == len(items) - expect_routed, (raw["device_resampled"], len(items))
    want_i, want_m = ref.host_batch([ref.host_sample(a, o, f) for a, o, f in items])
    image, mask = _device(raw)
    assert image.dtype == torch.float32 and mask.dtype == torch.bool and image.shape == want_i.shape and mask.shape == want_m.shape
    assert torch.equal(mask, want_m), [(a.shape, o, f) for a, o, f in items]
    assert torch.equal(image, want_i), ([(a.shape, o, f) for a, o, f in items], int((image != want_i).sum()))
    return want_m


@pytest.mark.parametrize("filt", [ref.BICUBIC, ref.BILINEAR])
def test_every_size_case_equals_the_host_path(filt):
    for n, (ih, iw, oh, ow) in enumerate(ref.size_cases()):
        _equal_to_host([(ref.seeded_pixels(ih, iw, seed=n), (oh, ow), filt)])


def test_mode_l_equals_the_host_path():
    for n, (ih, iw, oh, ow) in enumerate([(384, 511, 384, 480), (65, 97, 64, 96), (500, 333, 160, 96), (65, 97, 208, 312), (64, 64, 64, 64)]):
        for filt in (ref.BICUBIC, ref.BILINEAR):
            _equal_to_host([(ref.seeded_pixels(ih, iw, seed=70 + n, channels=1), (oh, ow), filt)])


def test_mixed_size_batch_of_four_with_padding():
    items = [(ref.seeded_pixels(384, 683, seed=1), (384, 672), ref.BICUBIC),
             (ref.seeded_pixels(397, 384, seed=2), (384, 384), ref.BICUBIC),
             (ref.seeded_pixels(500, 333, seed=3), (480, 320), ref.BILINEAR),
             (ref.seeded_pixels(65, 97, seed=4, channels=1), (64, 96), ref.BICUBIC)]
    mask = _equal_to_host(items)
    assert mask.shape == (4, 480, 672) and mask.any() and not mask[:, :64, :96].any()
    assert [int((~m).sum()) for m in mask] == [384 * 672, 384 * 384, 480 * 320, 64 * 96]


def test_two_times_downscale_and_upscale():
    _equal_to_host([(ref.seeded_pixels(768, 1024, seed=5), (384, 512), ref.BICUBIC), (ref.seeded_pixels(768, 1024, seed=6), (384, 512), ref.BILINEAR)])
    _equal_to_host([(ref.seeded_pixels(384, 683, seed=7), (800, 1333), ref.BICUBIC), (ref.seeded_pixels(100, 100, seed=8), (320, 320), ref.BILINEAR)])


def test_sizes_that_are_no_multiple_of_four():
    """Wm % 4 != 0: the scalar stores; padded rows and columns that end inside a tile and inside a 4-column group."""
    _equal_to_host([(ref.seeded_pixels(50, 71, seed=9), (45, 67), ref.BICUBIC), (ref.seeded_pixels(90, 40, seed=10), (77, 33), ref.BILINEAR)])
    _equal_to_host([(ref.seeded_pixels(50, 71, seed=11), (33, 66), ref.BICUBIC), (ref.seeded_pixels(90, 40, seed=12), (65, 130), ref.BILINEAR)])


def test_g15_on_the_device(golden):
    from counting_detr_amd import data
    z = golden("g15_image_prep.npz")
    lut = data.norm_table().numpy()
    samples = {}
    for i in range(int(z["n"])):
        a, (oh, ow), filt = z[f"in{i}"], z[f"to{i}"].tolist(), int(z[f"filter{i}"])
        if not data.image_prep_supports(a.shape[1::-1], (ow, oh), filt):
            continue                                                    # the 5x downscale: test_routing_* below
        samples[i] = ref.raw_sample(a, (oh, ow), filt)
        raw = data.pack_raw([samples[i]])
        assert raw["device_resampled"] == 1
        image, mask = _device(raw)
        want = np.stack([lut[c][z[f"out{i}"][:, :, c]] for c in range(3)])
        assert np.array_equal(image[0].numpy(), want) and not mask.any(), i
    raw = data.pack_raw([samples[i] for i in z["batch"].tolist()])
    assert raw["device_resampled"] == len(z["batch"])
    image, mask = _device(raw)
    assert np.array_equal(image.numpy(), z["batch_image"]) and np.array_equal(mask.numpy(), z["batch_mask"])


def test_output_buffers_are_fully_written():
    """No fill launch precedes the kernel: over memory that held other values every element of image and mask is (re)written."""
    from counting_detr_amd import data, ops
    items = [(ref.seeded_pixels(50, 71, seed=13), (40, 64), ref.BICUBIC), (ref.seeded_pixels(97, 60, seed=14), (96, 56), ref.BICUBIC)]
    raw = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in data.pack_raw([ref.raw_sample(*it) for it in items]).items()}
    want_i, want_m = ref.host_batch([ref.host_sample(*it) for it in items])
    for _ in range(3):
        junk = [torch.full((2 * 3 * 96 * 64,), float("nan"), device=DEV), torch.full((2 * 96 * 64,), 7, dtype=torch.uint8, device=DEV)]
        del junk                                                        # the caching allocator hands these blocks to the next same-size request
        image, mask = ops.image_prep(raw)
        assert torch.equal(image.cpu(), want_i) and torch.equal(mask.view(torch.uint8).cpu(), want_m.view(torch.uint8))


def test_on_a_side_stream():
    from counting_detr_amd import data, ops
    items = [(ref.seeded_pixels(384, 683, seed=15), (384, 672), ref.BICUBIC)] * 2
    raw = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in data.pack_raw([ref.raw_sample(*it) for it in items]).items()}
    want_i, want_m = ref.host_batch([ref.host_sample(*it) for it in items])
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        image, mask = ops.image_prep(raw)
    s.synchronize()
    assert torch.equal(image.cpu(), want_i) and torch.equal(mask.cpu(), want_m)


def test_routing_unsupported_scale_is_resized_on_the_host_and_still_equal():
    from counting_detr_amd import _ffi, data, ops
    items = [(ref.seeded_pixels(400, 90, seed=21), (64, 64), ref.BICUBIC), (ref.seeded_pixels(70, 90, seed=22), (64, 64), ref.BICUBIC)]
    _equal_to_host(items, expect_routed=1)
    # the kernel itself refuses what its tile cannot hold, before any launch
    raw = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in data.pack_raw([ref.raw_sample(*items[1])]).items()}
    with pytest.raises(RuntimeError, match="cdetr_image_prep.*taps"):
        ops.image_prep({**raw, "max_taps": data.IMAGE_PREP_MAX_TAPS + 1})
    assert _ffi.lib().cdetr_last_error()


def test_routing_palette_and_rgba_files_through_the_prefetcher(tmp_path):
    from PIL import Image
    from torch.utils.data import DataLoader
    from counting_detr_amd import data
    rgb = Image.fromarray(ref.seeded_pixels(70, 101, seed=11))
    rgba = Image.fromarray(np.concatenate([ref.seeded_pixels(70, 101, seed=12), ref.seeded_pixels(70, 101, seed=13)[:, :, :1]], axis=2), "RGBA")
    root = str(tmp_path / "ds")
    ref.write_fsc147(root, [rgb.convert("P", palette=Image.Palette.ADAPTIVE), rgba, rgb, rgb])
    a = argparse.Namespace(data_path=root, scale_factor=32)
    want = list(DataLoader(data.FSC147Dataset(a), batch_size=2, shuffle=False, collate_fn=data.collate))
    p = data.Prefetcher(DataLoader(data.FSC147Dataset(a, raw=True), batch_size=2, shuffle=False, collate_fn=data.collate_raw), DEV)
    got = list(p)
    torch.cuda.synchronize()
    assert (p.images, p.device_resampled) == (4, 2) and len(got) == len(want) == 2
    for g, w in zip(got, want):
        assert torch.equal(g["image"].cpu(), w["image"]) and torch.equal(g["mask"].cpu(), w["mask"])
        ref.assert_batches_equal(g, w)


def _loaders(raw):
    from counting_detr_amd import data
    a, al = argparse.Namespace(data_path=TINY, scale_factor=32), argparse.Namespace(data_path=LVIS)
    c2, c1 = (data.collate_raw, data.collate_stage1_raw) if raw else (data.collate, data.collate_stage1)
    return [("fsc147 train", data.FSC147Dataset(a, raw=raw), 2, c2, 0), ("fsc147 val", data.FSC147EvalDataset(a, split="val", raw=raw), 1, c2, 2),
            ("fsc147 test", data.FSC147EvalDataset(a, split="test", raw=raw), 1, c2, 0),
            ("lvis train", data.FSCDLVISDataset(al, split="train", raw=raw), 2, c2, 0), ("lvis test", data.FSCDLVISDataset(al, split="test", test=True, raw=raw), 1, c2, 0),
            ("stage1 train", data.FSC147ExemplarDataset(a, split="train", raw=raw), 2, c1, 0), ("stage1 val", data.FSC147ExemplarDataset(a, split="val", raw=raw), 2, c1, 2),
            ("points train", data.FSC147PointsDataset(a, split="train", raw=raw), 1, c1, 0), ("points test", data.FSC147PointsDataset(a, split="test", raw=raw), 1, c1, 0)]


def test_prefetcher_epoch_equals_the_default_loader_on_the_tiny_datasets():
    """An epoch of each tiny dataset, all five readers: Prefetcher over the raw loader == the default loader, batch by batch, field by
    field; every image went through the kernel as decoded."""
    from torch.utils.data import DataLoader
    from counting_detr_amd import data
    n_batches = 0
    for (name, ds, bs, col, workers), (_, rds, _, rcol, _) in zip(_loaders(False), _loaders(True)):
        want = list(DataLoader(ds, batch_size=bs, shuffle=False, collate_fn=col))
        p = data.Prefetcher(DataLoader(rds, batch_size=bs, shuffle=False, collate_fn=rcol, num_workers=workers), DEV)
        assert len(p) == len(want)
        got = list(p)
        torch.cuda.synchronize()
        assert len(got) == len(want) >= 1, name
        assert p.images == p.device_resampled == len(ds), (name, p.images, p.device_resampled)
        for g, w in zip(got, want):
            assert g["image"].is_cuda and g["mask"].is_cuda and g["mask"].dtype == torch.bool and "raw" not in g, name
            assert torch.equal(g["image"].cpu(), w["image"]) and torch.equal(g["mask"].cpu(), w["mask"]), name
            ref.assert_batches_equal(g, w)
            n_batches += 1
    assert n_batches >= 9


def _run(script, argv, timeout=900):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return p.stdout


def test_main_and_infer_run_with_device_preprocess(tmp_path):
    from oracle.weights import seeded_state_dict
    ckpt = tmp_path / "seeded.pth"
    torch.save({"model": seeded_state_dict()}, ckpt)
    out = tmp_path / "train"
    common = ["-dp", TINY, "--no_aux_loss", "--num_query_pattern", "1", "--num_workers", "0", "--device", DEV, "--device_preprocess"]
    txt = _run("main.py", common + ["-o", str(out), "--images_per_gpu", "2", "--epochs", "1", "--resume", str(ckpt), "--eval", "--split", "val"])
    log = json.loads((out / "detr_retrain.txt").read_text().splitlines()[-1])
    losses = {k: v for k, v in log.items() if k.startswith("train_loss")}
    assert losses and all(np.isfinite(v) for v in losses.values()), log
    val = json.loads(txt.split("counting metrics (val):", 1)[1].strip().splitlines()[0])
    assert val["images"] == 2 and all(np.isfinite(v) for k, v in val.items() if k.startswith("loss")), val
    # infer.py: the same metrics with and without the flag (the tensors it feeds the model are equal)
    res = {}
    for tag, extra in (("device", ["--device_preprocess"]), ("host", [])):
        o = tmp_path / tag
        txt = _run("infer.py", [a for a in common if a != "--device_preprocess"] + extra + ["-o", str(o), "--split", "val", "--resume", str(ckpt)])
        res[tag] = json.loads(txt.strip().splitlines()[-1])
        assert res[tag]["images"] == 2 and all(np.isfinite(v) for k, v in res[tag].items() if k.startswith("loss")), res[tag]
    for k in ("MAE", "RMSE", "NAE", "SRE", "images"):
        assert res["device"][k] == res["host"][k], k
    assert (tmp_path / "device" / "predictions_val.json").read_text() == (tmp_path / "host" / "predictions_val.json").read_text()


def test_main_stage1_runs_with_device_preprocess(tmp_path):
    out = tmp_path / "s1"
    common = ["--data_path", TINY, "--output_dir", str(out), "--num_workers", "0", "--print_freq", "1", "--device_preprocess"]
    _run("main_stage1.py", common + ["--epochs", "1", "--batch_size", "2"])
    log = json.loads((out / "log.txt").read_text().splitlines()[-1])
    assert np.isfinite(log["train_loss"]), log
    txt = _run("main_stage1.py", common + ["--eval", "--resume", str(out / "checkpoint.pth")])
    val = json.loads(txt.split("validation:", 1)[1].strip().splitlines()[0])
    assert np.isfinite(val["loss"]) and val["batches"] == 2
    _run("main_stage1.py", common + ["--dataset_file", "fscd_147_point", "--generate_pseudo_label", "--resume", str(out / "checkpoint.pth")])
    host = tmp_path / "s1_host"
    _run("main_stage1.py", ["--data_path", TINY, "--output_dir", str(host), "--num_workers", "0", "--dataset_file", "fscd_147_point",
                            "--generate_pseudo_label", "--resume", str(out / "checkpoint.pth")])
    for split in ("train", "val", "test"):                               # the same images and dots in the same order as the host path writes
        got, want = json.loads((out / f"pseudo_bbox_{split}.json").read_text()), json.loads((host / f"pseudo_bbox_{split}.json").read_text())
        assert got["images"] == want["images"] and len(got["annotations"]) == len(want["annotations"]) > 0, split
