"""Host side of the device image preparation (--device_preprocess; data.resample_tables / raw=True readers / collate_raw, the C-ABI entry
of csrc/image_prep.hip): what can be checked without a GPU.  The target is the HOST path -- PIL's resize, to_normalized_tensor, collate --
and the bar is equality: the coefficient tables + the numpy restatement of the kernel (tests/image_prep_ref.py) reproduce it byte for
byte, so tests/test_image_prep_gpu.py only has to hold the kernel to the same tensors.  No tolerance appears anywhere."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import abi_header
import image_prep_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TINY = os.path.join(HERE, "golden", "fsc147_tiny")
LVIS = os.path.join(HERE, "golden", "fscd_lvis_tiny")


def _tables(ih, iw, oh, ow, filt):
    from counting_detr_amd import data
    return data.resample_tables(iw, ow, filt) + data.resample_tables(ih, oh, filt)


@pytest.mark.parametrize("filt", [ref.BICUBIC, ref.BILINEAR])
def test_tables_and_restatement_equal_pil(filt):
    cases = ref.size_cases()
    assert len(cases) >= 20
    for n, (ih, iw, oh, ow) in enumerate(cases):
        a = ref.seeded_pixels(ih, iw, seed=n)
        want = np.asarray(Image.fromarray(a).resize((ow, oh), filt))
        got = ref.resize_u8(a, *_tables(ih, iw, oh, ow, filt))
        assert got.shape == want.shape and np.array_equal(got, want), ((ih, iw, oh, ow, filt), int((got != want).sum()))


def test_mode_l_resized_then_replicated_equals_replicated_then_resized():
    for n, (ih, iw, oh, ow) in enumerate([(384, 511, 384, 480), (65, 97, 64, 96), (500, 333, 160, 96), (65, 97, 208, 312), (64, 64, 64, 64)]):
        g = ref.seeded_pixels(ih, iw, seed=70 + n, channels=1)
        for filt in (ref.BICUBIC, ref.BILINEAR):
            want = np.asarray(Image.fromarray(g).resize((ow, oh), filt).convert("RGB"))
            s = ref.raw_sample(g, (oh, ow), filt)
            assert s["image_raw"].shape == (ih, iw, 3) and not s["host_resized"]
            assert np.array_equal(ref.resize_u8(s["image_raw"], *_tables(ih, iw, oh, ow, filt)), want), (ih, iw, oh, ow, filt)


def test_tables_shape_cache_and_identity():
    from counting_detr_amd import data
    b, c = data.resample_tables(683, 672, ref.BICUBIC)
    assert b.dtype == np.int32 and c.dtype == np.int32 and b.shape == (672, 2) and c.shape == (672, 2 * 3 + 1)      # ceil(2 * 683 / 672) * 2 + 1
    assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= 683).all() and (b[:, 1] <= c.shape[1]).all()
    assert (c.sum(axis=1) - (1 << 22)).__abs__().max() <= c.shape[1]              # each row sums to one, up to the taps' roundings
    assert data.resample_tables(683, 672, ref.BICUBIC)[0] is b                   # cached per argument triple
    assert data.resample_tables(1813, 512, ref.BILINEAR)[1].shape == (512, 2 * 4 + 1)
    ib, ic = data.resample_tables(64, 64, ref.BICUBIC)
    assert ib.tolist() == [[i, 1] for i in range(64)] and ic.tolist() == [[1 << 22]] * 64
    with pytest.raises(ValueError):
        data.resample_tables(64, 32, int(Image.NEAREST))
    with pytest.raises(ValueError):
        data.resample_tables(0, 32, ref.BICUBIC)


def test_norm_table_is_to_normalized_tensor():
    from counting_detr_amd import data
    lut = data.norm_table()
    assert lut.dtype == torch.float32 and lut.shape == (3, 256)
    a = ref.seeded_pixels(40, 56, seed=5)
    want = data.to_normalized_tensor(Image.fromarray(a))
    got = torch.stack([lut[c][torch.from_numpy(a[:, :, c].astype(np.int64))] for c in range(3)])
    assert torch.equal(got, want)


def test_limits_mirror_the_header():
    from counting_detr_amd import data
    src = open(os.path.join(ROOT, "include", "cdetr_hip.h")).read()
    for name, val in (("TILE_H", data.IMAGE_PREP_TILE_H), ("MAX_TAPS", data.IMAGE_PREP_MAX_TAPS), ("MAX_ROWS", data.IMAGE_PREP_MAX_ROWS),
                      ("RECORD_INTS", data.IMAGE_PREP_RECORD_INTS)):
        assert int(re.search(r"#define CDETR_IMAGE_PREP_" + name + r" (\d+)", src).group(1)) == val, name
    # the range the header states: downscales up to 4x per axis and any upscale, both filters
    for filt in (ref.BICUBIC, ref.BILINEAR):
        for i, o in ((4 * 333, 333), (1536, 384), (1813, 512), (683, 672), (65, 800), (7, 1333), (1, 64)):
            assert data.image_prep_supports((i, i), (o, o), filt), (i, o, filt)
    assert not data.image_prep_supports((5 * 96, 100), (96, 100), ref.BICUBIC)
    assert not data.image_prep_supports((100, 5 * 96), (100, 96), ref.BICUBIC)
    assert data.image_prep_supports((100, 96), (100, 96), int(Image.NEAREST)) and not data.image_prep_supports((100, 96), (50, 48), int(Image.NEAREST))


def test_g15_equals_tables_and_restatement(golden):
    from counting_detr_amd import data
    z = golden("g15_image_prep.npz")
    n = int(z["n"])
    assert n >= 6
    samples, routed = [], 0
    for i in range(n):
        a, (oh, ow), filt = z[f"in{i}"], z[f"to{i}"].tolist(), int(z[f"filter{i}"])
        s = ref.raw_sample(a, (oh, ow), filt)
        samples.append(s)
        if data.image_prep_supports(a.shape[1::-1], (ow, oh), filt):
            got = ref.resize_u8(s["image_raw"], *_tables(a.shape[0], a.shape[1], oh, ow, filt))
            assert np.array_equal(got, z[f"out{i}"]), i
        else:
            routed += 1
        raw = data.pack_raw([s])                                      # ... and through the packed form, whichever way it was routed
        image, mask = ref.run(raw)
        lut = data.norm_table().numpy()
        want = np.stack([lut[c][z[f"out{i}"][:, :, c]] for c in range(3)])
        assert np.array_equal(image[0], want) and not mask.any(), i
    assert routed == 1                                                # the 5x downscale
    raw = data.pack_raw([samples[i] for i in z["batch"].tolist()])
    image, mask = ref.run(raw)
    assert raw["device_resampled"] == len(z["batch"])
    assert image.dtype == z["batch_image"].dtype and np.array_equal(image, z["batch_image"]) and np.array_equal(mask, z["batch_mask"])
    assert mask.any() and not mask.all()                              # the batch has padding


def _args(path):
    return argparse.Namespace(data_path=path, scale_factor=32)


def _readers(raw):
    from counting_detr_amd import data
    return {"FSC147Dataset": ([data.FSC147Dataset(_args(TINY), raw=raw)], data.collate_raw if raw else data.collate),
            "FSC147EvalDataset": ([data.FSC147EvalDataset(_args(TINY), split=s, raw=raw) for s in ("val", "test")], data.collate_raw if raw else data.collate),
            "FSCDLVISDataset": ([data.FSCDLVISDataset(_args(LVIS), split="train", raw=raw), data.FSCDLVISDataset(_args(LVIS), split="test", test=True, raw=raw)],
                                data.collate_raw if raw else data.collate),
            "FSC147ExemplarDataset": ([data.FSC147ExemplarDataset(_args(TINY), split=s, raw=raw) for s in ("train", "val")],
                                      data.collate_stage1_raw if raw else data.collate_stage1),
            "FSC147PointsDataset": ([data.FSC147PointsDataset(_args(TINY), split=s, raw=raw) for s in ("train", "val", "test")],
                                    data.collate_stage1_raw if raw else data.collate_stage1)}


def _batches(ds, one_by_one):
    idx = [[i] for i in range(len(ds))] if one_by_one else [list(range(len(ds)))]
    return idx + ([] if one_by_one or len(ds) < 2 else [[i] for i in range(len(ds))])


@pytest.mark.parametrize("reader", ["FSC147Dataset", "FSC147EvalDataset", "FSCDLVISDataset", "FSC147ExemplarDataset", "FSC147PointsDataset"])
def test_raw_reader_collate_and_restatement_equal_the_default_path(reader):
    """raw=True reader -> collate_raw -> restatement == default reader -> collate, on the tiny datasets: image and mask equal, every
    other sample and batch field equal; no image is resized on the host."""
    (dss, col), (rdss, rcol) = _readers(False)[reader], _readers(True)[reader]
    n_img = 0
    for ds, rds in zip(dss, rdss):
        assert len(ds) == len(rds) >= 1
        for i in range(len(ds)):                                       # sample level: same fields but the image's
            s, r = ds[i], rds[i]
            assert set(r) - {"image_raw", "resize_to", "resample", "host_resized"} == set(s) - {"image"}
            assert r["image_raw"].dtype == np.uint8 and r["image_raw"].flags["C_CONTIGUOUS"] and r["image_raw"].shape[2] == 3
            assert tuple(r["resize_to"]) == (s["image"].shape[2], s["image"].shape[1]) and not r["host_resized"]
            for k in set(s) - {"image"}:
                assert np.array_equal(np.asarray(s[k]), np.asarray(r[k])), k
        for idx in _batches(ds, one_by_one=reader == "FSC147PointsDataset"):          # the points reader: different dot counts per image
            want, got = col([ds[i] for i in idx]), rcol([rds[i] for i in idx])
            assert "image" not in got and "mask" not in got
            ref.assert_batches_equal(got, want)
            image, mask = ref.run(got["raw"])
            assert got["raw"]["device_resampled"] == len(idx)
            assert image.dtype == np.float32 and np.array_equal(image, want["image"].numpy()) and np.array_equal(mask, want["mask"].numpy()), idx
            n_img += len(idx)
    assert n_img >= 2


def test_the_tiny_batches_have_padding_and_both_filters():
    """What the reader test above relies on: the tiny training batch mixes sizes (so the mask is not trivial) and the readers cover both filters."""
    from counting_detr_amd import data
    b = data.collate_raw([s for s in data.FSC147Dataset(_args(TINY), raw=True)])
    _, mask = ref.run(b["raw"])
    assert mask.any() and not mask.all()
    filters = {int(data.FSC147Dataset(_args(TINY), raw=True)[0]["resample"]), int(data.FSC147EvalDataset(_args(TINY), raw=True)[0]["resample"])}
    assert filters == {ref.BICUBIC, ref.BILINEAR}


def test_routing_palette_and_rgba_images_go_through_the_host(tmp_path):
    """Modes other than RGB / L are resized by the reader's own PIL call and passed on with identity tables: still equal."""
    from counting_detr_amd import data
    rgb = Image.fromarray(ref.seeded_pixels(70, 101, seed=11))
    rgba = Image.fromarray(np.concatenate([ref.seeded_pixels(70, 101, seed=12), ref.seeded_pixels(70, 101, seed=13)[:, :, :1]], axis=2), "RGBA")
    grey = Image.fromarray(ref.seeded_pixels(70, 101, seed=14, channels=1))
    root = str(tmp_path / "ds")
    ref.write_fsc147(root, [rgb.convert("P", palette=Image.Palette.ADAPTIVE), rgba, grey, rgb])
    for cls, col, rcol in ((data.FSC147Dataset, data.collate, data.collate_raw), (data.FSC147EvalDataset, data.collate, data.collate_raw),
                           (data.FSC147ExemplarDataset, data.collate_stage1, data.collate_stage1_raw)):
        ds, rds = cls(_args(root)), cls(_args(root), raw=True)
        assert [rds[i]["host_resized"] for i in range(4)] == [True, True, False, False]
        assert [tuple(rds[i]["image_raw"].shape[:2]) for i in range(4)] == [(64, 96), (64, 96), (70, 101), (70, 101)]
        want, got = col([ds[i] for i in range(4)]), rcol([rds[i] for i in range(4)])
        ref.assert_batches_equal(got, want)
        assert got["raw"]["device_resampled"] == 2
        image, mask = ref.run(got["raw"])
        assert np.array_equal(image, want["image"].numpy()) and np.array_equal(mask, want["mask"].numpy())


def test_routing_scales_beyond_the_tile_are_resized_by_collate_raw():
    from counting_detr_amd import data
    a = ref.seeded_pixels(400, 90, seed=21)                            # 6.25x down on one axis
    ok = ref.seeded_pixels(70, 90, seed=22)
    samples = [ref.raw_sample(a, (64, 64), ref.BICUBIC), ref.raw_sample(ok, (64, 64), ref.BICUBIC)]
    assert not samples[0]["host_resized"]                             # the reader passes it on: the scale is collate_raw's to judge
    raw = data.pack_raw(samples)
    assert raw["device_resampled"] == 1 and raw["images"][0, 1:5].tolist() == [64, 64, 64, 64] and raw["max_taps"] <= data.IMAGE_PREP_MAX_TAPS
    image, mask = ref.run(raw)
    want_i, want_m = ref.host_batch([ref.host_sample(a, (64, 64), ref.BICUBIC), ref.host_sample(ok, (64, 64), ref.BICUBIC)])
    assert np.array_equal(image, want_i.numpy()) and np.array_equal(mask, want_m.numpy())


def test_pack_raw_layout():
    from counting_detr_amd import data
    ss = [ref.raw_sample(ref.seeded_pixels(37, 53, seed=1), (32, 48), ref.BICUBIC), ref.raw_sample(ref.seeded_pixels(37, 53, seed=2), (32, 48), ref.BICUBIC),
          ref.raw_sample(ref.seeded_pixels(64, 41, seed=3), (64, 40), ref.BILINEAR)]
    raw = data.pack_raw(ss)
    assert {k: (v.dtype, v.is_contiguous()) for k, v in raw.items() if torch.is_tensor(v)} == \
        {"pixels": (torch.uint8, True), "images": (torch.int32, True), "tables": (torch.int32, True), "lut": (torch.float32, True)}
    assert all(isinstance(raw[k], int) for k in ("Hm", "Wm", "max_taps", "max_rows", "device_resampled"))
    rec = raw["images"].tolist()
    assert (raw["Hm"], raw["Wm"]) == (64, 48) and [r[0] % 16 for r in rec] == [0, 0, 0] and rec[0][5:11] == rec[1][5:11]       # equal tables stored once
    assert rec[2][8:11] == [rec[2][8], rec[2][8] + 2 * 64, 1]                                                                   # unchanged axis: identity
    assert raw["pixels"].numel() < sum(s["image_raw"].size for s in ss) + 48
    assert raw["max_taps"] == 7 and raw["max_rows"] <= data.IMAGE_PREP_MAX_ROWS
    # a quarter of the bytes of the fp32 batch, as the un-resized pixels are 3 B each against 12 B per resized pixel
    assert raw["pixels"].numel() + 4 * raw["tables"].numel() < 3 * 64 * 48 * 3 * 4


def test_collate_raw_survives_worker_processes():
    from torch.utils.data import DataLoader
    from counting_detr_amd import data
    rds = data.FSC147Dataset(_args(TINY), raw=True)
    want = data.collate_raw([rds[i] for i in range(2)])
    got = next(iter(DataLoader(rds, batch_size=2, shuffle=False, collate_fn=data.collate_raw, num_workers=2)))
    ref.assert_batches_equal(got, want)
    for k, v in want["raw"].items():
        assert torch.equal(got["raw"][k], v) if torch.is_tensor(v) else got["raw"][k] == v, k


def test_prefetcher_keeps_todays_path_for_batches_without_raw():
    from torch.utils.data import DataLoader
    from counting_detr_amd import data
    dl = DataLoader(data.FSC147ExemplarDataset(_args(TINY)), batch_size=2, shuffle=False, collate_fn=data.collate_stage1)
    p = data.Prefetcher(dl, "cpu")                                      # a 1st-stage batch has no targets
    got = list(p)
    assert len(got) == 1 and torch.equal(got[0]["image"], next(iter(dl))["image"]) and p.images == 0
    rdl = DataLoader(data.FSC147ExemplarDataset(_args(TINY), raw=True), batch_size=2, shuffle=False, collate_fn=data.collate_stage1_raw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):         # the raw path has no host implementation in the product
        list(data.Prefetcher(rdl, "cpu"))


@pytest.fixture(scope="module")
def L():
    from counting_detr_amd.build import build_lib
    build_lib(verbose=False)
    from counting_detr_amd import _ffi
    return _ffi.lib()


def test_entry_exported_and_declared(L):
    from counting_detr_amd import _ffi, build
    src = abi_header.source()
    assert "cdetr_image_prep" in _ffi.EXPORTS and hasattr(L, "cdetr_image_prep")
    assert re.search(r"^int cdetr_image_prep\(const cdetr_image_prep_desc\* d, void\* stream\);", src, flags=re.M)
    assert abi_header.field_names("cdetr_image_prep_desc") == [f[0] for f in _ffi.ImagePrepDesc._fields_]
    assert "image_prep.hip" in build.SOURCES and L.cdetr_abi_version() == 2


def test_bad_descriptors_are_refused_before_any_launch(L):
    from counting_detr_amd import _ffi
    d = _ffi.ImagePrepDesc()
    assert L.cdetr_image_prep(ctypes.byref(d), None) < 0 and b"cdetr_image_prep" in L.cdetr_last_error()
    assert L.cdetr_image_prep(None, None) < 0 and b"cdetr_image_prep" in L.cdetr_last_error()
    buf = (ctypes.c_uint8 * 64)()
    base = (ctypes.addressof(buf) + 15) & ~15

    def good():
        g = _ffi.ImagePrepDesc()
        g.B, g.Hm, g.Wm, g.max_taps, g.max_rows, g.pixel_bytes, g.table_ints = 1, 32, 32, 7, 40, 3072, 500
        for f in ("pixels", "images", "tables", "lut", "image", "mask"):
            setattr(g, f, base)
        return g
    for field, value, word in (("B", 0, b"bad sizes"), ("B", 70000, b"bad sizes"), ("Wm", -4, b"bad sizes"), ("pixel_bytes", 0, b"buffer sizes"),
                               ("table_ints", 2 ** 31, b"buffer sizes"), ("lut", None, b"null pointer"), ("mask", None, b"null pointer"),
                               ("image", base + 4, b"aligned"), ("max_taps", 21, b"21 taps"), ("max_rows", 161, b"161 staged rows"),
                               ("max_taps", 0, b"must be positive")):
        g = good()
        setattr(g, field, value)
        rc = L.cdetr_image_prep(ctypes.byref(g), None)
        msg = L.cdetr_last_error()
        assert rc < 0 and b"cdetr_image_prep" in msg and word in msg, (field, value, rc, msg)


def test_cli_flag_defaults_off():
    from counting_detr_amd.args import get_args_parser, get_args_parser_stage1
    for parser in (get_args_parser, get_args_parser_stage1):
        assert parser().parse_args([]).device_preprocess is False
        assert parser().parse_args(["--device_preprocess"]).device_preprocess is True
