"""infer.py --eval_batch_size on the five-image split of tests/eval_split.py (seeded weights): the host loop against the --device_detections
loop at batch size 2 (exact: both consume the same forward outputs), batch size 2 against the same bucket order run one image at a time (the
bars of tests/test_stage1_ragged_gpu.py for batched versus single), and the default path (batch size 1: the batched criterion, no
cdetr_criterion_eval launch, the bytes of a plain batch-1 loader).

The class bias is shifted into a gap BETWEEN logits.  The seeded (untrained) network gives every query of an image nearly the same logit: in
the CPU oracle's forward the 300 logits of an image span 6e-4 ... 2e-3, the images lie 2e-2 ... 1e-1 apart, so a threshold inside an image's
cluster would put all of its queries (20 % of the split) within 1e-3 of it in probability.  The shift is therefore the middle of the gap
under the three highest images (oracle: 0.018 wide, images 1, 2 and 5 kept whole, one of each batch of two): no batch-1 probability lies
within 1e-3 of the threshold (share of left-out queries in the CPU oracle's forward: 0 of 1500; the test prints and bounds the device's), and the
count comparison leaves nothing out."""
import json
import os

import numpy as np
import pytest
import torch

import eval_split as es
from counting_detr_amd import coco_ap as ca
from counting_detr_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AP_KEYS = ("AP", "AP50", "AP75", "APs", "APm", "APl")
THRESHOLD = 0.5


def _same(a, b):
    return set(a) == set(b) and all(a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])) for k in a)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The split, the shifted model and the three runs every comparison reads: host loop and device loop at batch size 2, host loop over the same
    bucket order one image at a time; each with the forward's probabilities and boxes as the loop saw them."""
    import infer as infer_mod
    from counting_detr_amd import build_model, data
    from counting_detr_amd.args import default_args
    from counting_detr_amd.engine import InferenceEngine
    from counting_detr_amd.misc import NestedTensor
    from oracle.weights import seeded_state_dict
    root = tmp_path_factory.mktemp("eval_batches")
    args = default_args()
    args.data_path, args.scale_factor, args.split, args.num_workers, args.device = es.write_split(root / "ds"), 32, "val", 0, DEV
    model, criterion, _ = build_model(args)
    model.load_state_dict(seeded_state_dict(), strict=True)
    model.to(DEV); criterion.to(DEV)
    model.eval()
    ds = data.build_test_dataset(args, "val")
    single = [data.collate([ds[i]]) for b in es.BATCHES_AT_2 for i in b]                  # the bucket order, one image per batch
    with torch.no_grad():
        logit = torch.stack([model(NestedTensor(b["image"].to(DEV), b["mask"].to(DEV)), rects=b["ex_rects"].to(DEV))[0]["pred_logits"][0, :, 0]
                             for b in single]).double().cpu()
        lo, hi = logit.min(1).values, logit.max(1).values
        order = torch.argsort(lo)
        below, above = float(hi[order[1]]), float(lo[order[2]])                            # the gap under the three highest images
        print("logit spans", [(round(float(a), 5), round(float(b), 5)) for a, b in zip(lo, hi)], "gap", above - below)
        assert above - below > 0.01, "the threshold needs a gap between the images' logits (see the module docstring)"
        for ce in {id(m): m for m in model.transformer.cls_embed}.values():
            ce.bias[0] -= 0.5 * (below + above)
    gt_json = os.path.join(args.data_path, "instances_val.json")
    args.eval_batch_size = 2
    real_call = InferenceEngine.__call__
    runs = {}
    for name, flag, batched in (("host2", False, True), ("device2", True, True), ("single", False, False)):
        seen = []

        def call(self, *a, _seen=seen, **kw):
            out = real_call(self, *a, **kw)
            _seen.append((out[4].clone(), out[2]["pred_boxes"].clone()))
            return out
        os.makedirs(root / name)
        loader = infer_mod.eval_loader(args, torch.device(DEV))[0] if batched else single
        InferenceEngine.__call__ = call
        try:
            metrics, preds = infer_mod.infer(model, criterion, loader, torch.device(DEV), str(root / name), split="val", device_detections=flag,
                                             gt_json=gt_json if flag else None, per_image=batched)
        finally:
            InferenceEngine.__call__ = real_call
        runs[name] = {"metrics": metrics, "preds": preds, "bytes": open(root / name / "predictions_val.json", "rb").read(),
                      "prob": torch.cat([s[0] for s in seen]).cpu().numpy(), "boxes": torch.cat([s[1] for s in seen]).cpu().numpy(),
                      "batches": [int(s[0].shape[0]) for s in seen]}
    return {"root": root, "args": args, "model": model, "criterion": criterion, "gt_json": gt_json, "runs": runs, "ds": ds}


def test_host_loop_and_device_loop_agree_exactly_at_batch_size_two(world):
    host, dev = world["runs"]["host2"], world["runs"]["device2"]
    assert host["batches"] == dev["batches"] == [len(b) for b in es.BATCHES_AT_2]
    assert host["bytes"] == dev["bytes"] and host["preds"] == dev["preds"]
    assert [im["id"] for im in host["preds"]["images"]] == [i + 1 for b in es.BATCHES_AT_2 for i in b]      # the order they were run in
    m_host, m_dev = dict(host["metrics"]), dict(dev["metrics"])
    ap_store = {k: m_dev.pop(k) for k in AP_KEYS}
    print("host", m_host, "device", m_dev)
    assert _same(m_host, m_dev) and m_host["images"] == 5 and all(k in m_host for k in es.LOSS_KEYS + ("MAE", "RMSE"))
    ap_file = ca.ap_from_json(str(world["root"] / "host2" / "predictions_val.json"), world["gt_json"], device=DEV)
    print("AP from the file", ap_file, "from the store", ap_store)
    assert _same(ap_file, ap_store)


def test_batch_size_two_against_one_image_at_a_time(world):
    two, one = world["runs"]["host2"], world["runs"]["single"]
    assert one["batches"] == [1] * 5
    assert [im for im in two["preds"]["images"]] == [im for im in one["preds"]["images"]]
    np.testing.assert_allclose(two["prob"], one["prob"], rtol=1e-3, atol=1e-4, err_msg="probabilities")
    np.testing.assert_allclose(two["boxes"], one["boxes"], rtol=1e-3, atol=1e-4, err_msg="boxes")
    near = np.abs(one["prob"] - THRESHOLD) <= 1e-3                                         # left out of the count comparison
    share = float(near.mean())
    keep2, keep1 = two["prob"] >= THRESHOLD, one["prob"] >= THRESHOLD
    print("left-out share", share, "kept per image", keep1.sum(1).tolist(), "largest probability difference", float(np.abs(two["prob"] - one["prob"]).max()))
    assert share <= 0.02
    assert ((keep2 & ~near).sum(1) == (keep1 & ~near).sum(1)).all() and (keep2 == keep1)[~near].all()
    assert 0 < keep1.sum() < keep1.size                                                    # some images kept, some not
    # the written integers, query by query (the json lists an image's kept queries in query order)
    def by_query(run, keep):
        ids = [im["id"] for im in run["preds"]["images"]]
        keys = [(ids[b], int(q)) for b in range(keep.shape[0]) for q in np.nonzero(keep[b])[0]]
        assert len(keys) == len(run["preds"]["annotations"]) and [k[0] for k in keys] == [a["image_id"] for a in run["preds"]["annotations"]]
        return dict(zip(keys, run["preds"]["annotations"]))
    a2, a1 = by_query(two, keep2), by_query(one, keep1)
    common = sorted(set(a2) & set(a1))
    assert len(common) >= int((keep1 & ~near).sum())
    for key in common:
        x, y = a2[key], a1[key]
        assert all(abs(p - q) <= 1 for p, q in zip(x["bbox"] + x["point"], y["bbox"] + y["point"])) and abs(x["area"] - y["area"]) <= 1, (x, y)
        np.testing.assert_allclose(x["score"], y["score"], rtol=1e-3, atol=1e-4)
    for k in es.LOSS_KEYS:
        print(k, two["metrics"][k], one["metrics"][k])
        np.testing.assert_allclose(two["metrics"][k], one["metrics"][k], rtol=1e-3, err_msg=k)
    if not near.any():
        for k in ("MAE", "RMSE", "NAE", "SRE"):
            assert two["metrics"][k] == one["metrics"][k], k


def test_default_path_and_the_cli(world, tmp_path, capsys, monkeypatch):
    """--eval_batch_size 1: the bytes of infer.infer over a plain batch-1 loader, and ops.criterion_eval is never called.  --eval_batch_size 2
    with --device_detections --device_preprocess: one cdetr_criterion_eval and one emit call per batch, the bytes of the device loop above (the
    raw batches carry several images; the image tensors are the host's bit for bit)."""
    from torch.utils.data import DataLoader
    import infer as infer_mod
    from counting_detr_amd import data
    from counting_detr_amd.args import get_args_parser
    ckpt = tmp_path / "shifted.pth"
    torch.save({"model": world["model"].state_dict()}, ckpt)
    calls = {"criterion_eval": 0, "emit_detections": 0}
    for name in calls:
        real = getattr(ops, name)

        def counted(*a, _real=real, _name=name, **kw):
            calls[_name] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(ops, name, counted)
    common = ["-dp", world["args"].data_path, "--split", "val", "--resume", str(ckpt), "--no_aux_loss", "--num_query_pattern", "1", "--num_workers", "0",
              "--device", DEV]
    os.makedirs(tmp_path / "plain")
    plain = DataLoader(world["ds"], batch_size=1, shuffle=False, collate_fn=data.collate)
    m_plain, _ = infer_mod.infer(world["model"], world["criterion"], plain, torch.device(DEV), str(tmp_path / "plain"), split="val")
    capsys.readouterr()
    infer_mod.main(get_args_parser().parse_args(common + ["-o", str(tmp_path / "cli1"), "--eval_batch_size", "1"]))
    m_cli = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert calls == {"criterion_eval": 0, "emit_detections": 0}
    assert open(tmp_path / "cli1" / "predictions_val.json", "rb").read() == open(tmp_path / "plain" / "predictions_val.json", "rb").read()
    assert all(m_cli[k] == v or (np.isnan(v) and np.isnan(m_cli[k])) for k, v in m_plain.items())
    infer_mod.main(get_args_parser().parse_args(common + ["-o", str(tmp_path / "cli2"), "--eval_batch_size", "2", "--device_detections", "--device_preprocess"]))
    m_cli2 = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert calls == {"criterion_eval": 3, "emit_detections": 3}
    assert open(tmp_path / "cli2" / "predictions_val.json", "rb").read() == world["runs"]["device2"]["bytes"]
    assert _same(m_cli2, world["runs"]["device2"]["metrics"])
