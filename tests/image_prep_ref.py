"""Checker of the device image preparation (csrc/image_prep.hip, data.collate_raw): a numpy restatement of what cdetr_image_prep computes
from the `raw` part of a batch -- Pillow's two 8-bit resampling passes from the packed coefficient tables, the normalisation table
lookup, the zero padding and the padding mask -- plus the case list the CPU and the GPU tests share and the host path they compare with.
Not product code: nothing under counting_detr_amd imports it."""
import json
import os

import numpy as np
import torch
from PIL import Image

BICUBIC, BILINEAR = int(Image.BICUBIC), int(Image.BILINEAR)

# (in_h, in_w) of the readers' images, each resized as the readers do (floor to a multiple of 32 and of 8), then the scale cases:
# downscales up to 3.5x, upscales to 800 x 800, 800 x 1333 and by 3.2, and the identity
READER_SIZES = [(384, 511), (384, 683), (397, 384), (500, 333), (1200, 1813), (384, 1023), (65, 97), (97, 131)]
SCALE_CASES = [((384, 683), (192, 320)),        # 2x down (2.0 / 2.13)
               ((500, 333), (160, 96)),         # 3.1x / 3.5x down
               ((1200, 1813), (352, 520)),      # 3.4x / 3.5x down
               ((384, 511), (800, 800)),        # up, aspect changed
               ((384, 683), (800, 1333)),       # up to the detection size
               ((65, 97), (208, 312)),          # 3.2x up
               ((384, 512), (384, 512)),        # identity on both axes
               ((64, 64), (64, 64)),
               ((97, 128), (96, 128))]          # one axis unchanged


def size_cases():
    """[(in_h, in_w, out_h, out_w)] without repeats."""
    out = []
    for h, w in READER_SIZES:
        for sf in (32, 8):
            out.append((h, w, sf * (h // sf), sf * (w // sf)))
    out += [(a, b, c, d) for (a, b), (c, d) in SCALE_CASES]
    return list(dict.fromkeys(out))


def seeded_pixels(h, w, seed, channels=3):
    """uint8 [h, w, channels] (or [h, w] for channels = 1): smooth ramps + noise + saturated patches, so that the bicubic overshoot is clamped
    at both ends somewhere."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([(yy * (3 + c) + xx * (5 - c)) % 256 for c in range(channels)], axis=2).astype(np.int64)
    a = (a + rng.randint(-40, 41, a.shape)).clip(0, 255)
    for _ in range(6):
        y, x = rng.randint(0, h), rng.randint(0, w)
        a[y:y + max(h // 9, 2), x:x + max(w // 7, 2)] = 255 * rng.randint(0, 2)
    a = a.astype(np.uint8)
    return a if channels == 3 else a[:, :, 0]


def resample_axis1(src, bounds, coeffs):
    """One pass of Pillow's 8-bit resampler along axis 1 of uint8 [R, n_in, C] -> uint8 [R, n_out, C]."""
    s = src.astype(np.int64)
    out = np.empty((src.shape[0], bounds.shape[0], src.shape[2]), dtype=np.uint8)
    for i in range(bounds.shape[0]):
        first, n = int(bounds[i, 0]), int(bounds[i, 1])
        acc = (1 << 21) + (s[:, first:first + n, :] * coeffs[i, :n].astype(np.int64)[None, :, None]).sum(axis=1)
        assert np.abs(acc).max() < 2 ** 31                           # the C code (and the kernel) accumulate in int32
        out[:, i, :] = np.clip(acc >> 22, 0, 255)
    return out


def resize_u8(a, hb, hc, vb, vc):
    """uint8 [in_h, in_w, 3] -> uint8 [out_h, out_w, 3]: horizontal pass into uint8, then the vertical pass over that."""
    mid = resample_axis1(a, hb, hc)
    return resample_axis1(mid.transpose(1, 0, 2), vb, vc).transpose(1, 0, 2)


def run(raw):
    """The `raw` dict of data.pack_raw -> (image float32 [B, 3, Hm, Wm], mask bool [B, Hm, Wm]) as numpy arrays."""
    pixels, records, tables = raw["pixels"].numpy(), raw["images"].numpy(), raw["tables"].numpy()
    lut = raw["lut"].numpy().reshape(3, 256)
    B, Hm, Wm = records.shape[0], raw["Hm"], raw["Wm"]
    image = np.zeros((B, 3, Hm, Wm), dtype=np.float32)
    mask = np.ones((B, Hm, Wm), dtype=bool)
    for b, (off, ih, iw, oh, ow, hb, hc, hk, vb, vc, vk, _) in enumerate(records.tolist()):
        a = pixels[off:off + ih * iw * 3].reshape(ih, iw, 3)
        out = resize_u8(a, tables[hb:hb + 2 * ow].reshape(ow, 2), tables[hc:hc + ow * hk].reshape(ow, hk),
                        tables[vb:vb + 2 * oh].reshape(oh, 2), tables[vc:vc + oh * vk].reshape(oh, vk))
        for c in range(3):
            image[b, c, :oh, :ow] = lut[c][out[:, :, c]]
        mask[b, :oh, :ow] = False
    return image, mask


def raw_sample(a, out_hw, filt):
    """What a raw=True reader returns for the decoded RGB (uint8 [h, w, 3]) or grey (uint8 [h, w], mode L) image `a`."""
    from counting_detr_amd import data
    return data._raw_image(Image.fromarray(a), (out_hw[1], out_hw[0]), filt)


def host_sample(a, out_hw, filt):
    """What the default readers make of the same image: PIL resize + to_normalized_tensor."""
    from counting_detr_amd import data
    return {"image": data.to_normalized_tensor(Image.fromarray(a).resize((out_hw[1], out_hw[0]), filt))}


def host_batch(samples):
    """(image, mask) torch tensors of data.collate's padding for {"image": ...} samples."""
    from counting_detr_amd import data
    b = data.collate_stage1([{**s, "points": np.zeros((1, 2), np.float32), "orig_size": np.zeros(2, np.int64)} for s in samples])
    return b["image"], b["mask"]


def assert_batches_equal(got, want, skip=("image", "mask", "raw")):
    """Every field of two collated batches but the image part: same keys, equal tensors (targets: list of dicts)."""
    assert set(got) - set(skip) == set(want) - set(skip), (sorted(got), sorted(want))
    for k in set(want) - set(skip):
        if k == "targets":
            assert len(got[k]) == len(want[k])
            for tg, tw in zip(got[k], want[k]):
                assert set(tg) == set(tw)
                for kk in tw:
                    assert tg[kk].dtype == tw[kk].dtype and torch.equal(tg[kk].cpu(), tw[kk].cpu()), (k, kk)
        else:
            assert got[k].dtype == want[k].dtype and torch.equal(got[k].cpu(), want[k].cpu()), k


def write_fsc147(root, images, name_fmt="{}.png"):
    """An FSC-147-format training + validation set around the given PIL images (any mode): images_384_VarV2/, three exemplar boxes and
    two dots per image, pseudo boxes, instances_val.json, the split file."""
    os.makedirs(os.path.join(root, "images_384_VarV2"))
    os.makedirs(os.path.join(root, "annotations"))
    anno, ims, anns, names = {}, [], [], []
    for i, im in enumerate(images):
        name = name_fmt.format(i + 1)
        w, h = im.size
        im.save(os.path.join(root, "images_384_VarV2", name))
        ex = [[[x, y], [x, y + 0.2 * h], [x + 0.1 * w, y + 0.2 * h], [x + 0.1 * w, y]] for x, y in ((0.1 * w, 0.2 * h), (0.5 * w, 0.3 * h), (0.3 * w, 0.6 * h))]
        anno[name] = {"box_examples_coordinates": ex, "points": [[0.25 * w, 0.25 * h], [0.7 * w, 0.6 * h]]}
        ims.append({"id": i + 1, "file_name": name, "width": w, "height": h})
        for j in range(2):
            anns.append({"id": 2 * i + j + 1, "image_id": i + 1, "category_id": 1, "iscrowd": 0, "area": 48.0,
                         "bbox": [0.2 * w + 9 * j, 0.3 * h + 5 * j, 6.0, 8.0]})
        names.append(name)
    coco = {"images": ims, "annotations": anns, "categories": [{"id": 1, "name": "fg"}]}
    json.dump(anno, open(os.path.join(root, "annotation_FSC147_384.json"), "w"))
    json.dump(coco, open(os.path.join(root, "annotations", "pseudo_bbox_train.json"), "w"))
    json.dump(coco, open(os.path.join(root, "instances_val.json"), "w"))
    json.dump({"train": names, "val": names, "test": names}, open(os.path.join(root, "Train_Test_Val_FSC_147.json"), "w"))
