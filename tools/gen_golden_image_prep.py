"""Writes tests/golden/g15_image_prep.npz: small seeded uint8 images with what the HOST path makes of them -- PIL's resize of each
(`out<i>`), and data.collate's padded, normalised batch and mask of three of them -- recorded with the Pillow of the machine that ran this.
tests/test_image_prep_cpu.py / _gpu.py hold the coefficient tables, the numpy restatement and the kernel to these bytes, so a different
Pillow on another host cannot move the target unnoticed.

  python tools/gen_golden_image_prep.py
"""
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (in_h, in_w, out_h, out_w, filter, channels)
CASES = [(37, 53, 32, 40, Image.BICUBIC, 3),       # the readers' floor to a multiple of 8
         (50, 31, 24, 48, Image.BICUBIC, 3),       # down on one axis, up on the other
         (20, 20, 16, 16, Image.BILINEAR, 3),
         (70, 45, 20, 16, Image.BILINEAR, 3),      # 3.5x / 2.8x down
         (16, 24, 40, 56, Image.BICUBIC, 3),       # 2.5x / 2.3x up
         (33, 47, 32, 40, Image.BICUBIC, 1),       # mode L
         (24, 32, 24, 32, Image.BICUBIC, 3),       # identity
         (165, 41, 32, 40, Image.BICUBIC, 3)]      # 5.2x down: beyond the kernel's tile, resized on the host by collate_raw
BATCH = (1, 2, 6)                                  # padded to 24 x 48


def main():
    import image_prep_ref as ref
    from counting_detr_amd import data
    out = {"n": np.array(len(CASES)), "batch": np.array(BATCH), "pillow": np.array(PIL.__version__)}
    samples = []
    for i, (ih, iw, oh, ow, filt, ch) in enumerate(CASES):
        a = ref.seeded_pixels(ih, iw, seed=150 + i, channels=ch)
        r = Image.fromarray(a).resize((ow, oh), filt)
        out[f"in{i}"], out[f"to{i}"], out[f"filter{i}"] = a, np.array([oh, ow]), np.array(int(filt))
        out[f"out{i}"] = np.asarray(r.convert("RGB"), dtype=np.uint8)
        samples.append({"image": data.to_normalized_tensor(r)})
    image, mask = ref.host_batch([samples[i] for i in BATCH])
    out["batch_image"], out["batch_mask"] = image.numpy(), mask.numpy()
    path = os.path.join(ROOT, "tests", "golden", "g15_image_prep.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
