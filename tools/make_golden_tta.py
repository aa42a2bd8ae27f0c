#!/usr/bin/env python
"""Writes tests/golden/tta_multiquery_cases.npz: what the libraries reid/extract_feature.py calls compute on the seeded cases of
tests/tta_ref.py.  Runs on the CPU from Pillow, torch, numpy and scikit-learn; torchvision's TenCrop is restated with Image.crop /
Image.transpose (tests/tta_ref.py cites the formulas).

  <geometry>_resized      Pillow's Resize((RH, RW)) of every source image, uint8 [B, RH, RW, 3]
  <geometry>_crops_u8     (small geometries) Pillow's own ten crops, uint8 [B, 10, CH, CW, 3]
  <geometry>_tencrop      (small geometries) the crops after ToTensor + Normalize with torch's own float32 ops, [B, 10, 3, CH, CW]
  mean_<case>             torch's x.view(B, n, -1).mean(1) on the CPU
  pool_<case>_y / _max / _avg   sklearn.preprocessing.normalize of every group's rows, np.max / np.mean(axis=0) of them -- stored as
                          int16 distances, in float32 steps, from the float32 rounding of tta_ref's float64 restatement
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tta_ref as ref  # noqa: E402


def torch_normalize(crops_u8):
    """ToTensor (uint8 HWC -> float CHW .div(255)) and Normalize (.sub_(mean).div_(std)) as torchvision writes them, in torch"""
    x = torch.from_numpy(np.ascontiguousarray(crops_u8)).permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255)
    mean = torch.as_tensor(ref.MEAN, dtype=torch.float32).view(-1, 1, 1); std = torch.as_tensor(ref.STD, dtype=torch.float32).view(-1, 1, 1)
    return x.sub_(mean).div_(std).numpy()


def main():
    from sklearn.preprocessing import normalize
    out = {}
    for name, (B, h, w, resize, crop, _) in ref.GEOMETRIES.items():
        src = ref.source_images(name)
        resized = np.stack([ref.pil_resize(im, resize) for im in src])
        out[name + "_resized"] = resized
        if name in ref.FULL:
            crops = np.stack([ref.ten_crop_pil(im, crop) for im in resized])
            out[name + "_crops_u8"] = crops
            out[name + "_tencrop"] = np.stack([torch_normalize(c) for c in crops])
    for name in ref.MEAN_CASES:
        x = torch.from_numpy(ref.mean_inputs(name))
        bs, n = x.shape[:2]
        out["mean_" + name] = x.view(bs, n, -1).mean(1).numpy()
        frac64 = float((out["mean_" + name] != x.double().mean(1).float().numpy()).mean())
        D = x.shape[2]
        print("mean %s: equal to the sequential float32 sum / n: %s; with the last %d columns in the scalar loop's order: %s; differs from "
              "the rounded float64 mean on %.0f %% of the elements"
              % (name, np.array_equal(out["mean_" + name], ref.sequential_mean(x.numpy())), ref.mean_tail(D),
                 np.array_equal(out["mean_" + name], ref.torch_mean(x.numpy(), ref.mean_tail(D))), 100 * frac64))
    for name in ref.POOL_CASES:
        x, names, queries = ref.pool_case(name)
        groups = ref.group_rows(names, queries)
        t = ref.normalize64(x)
        tmax, tavg = ref.pool64(t, groups)
        y = np.zeros_like(x)
        hmax, havg = [], []
        for g in groups:                       # the script's loop per query: the rows of its key, normalize, max and mean over axis 0
            multi = normalize(np.ascontiguousarray(x[g]))      # a float32 block (see tests/tta_ref.py on the script's list)
            y[g] = multi
            hmax.append(np.max(multi, axis=0)); havg.append(np.mean(multi, axis=0))
        hmax, havg = np.array(hmax), np.array(havg)
        assert y.dtype == np.float32 and hmax.dtype == np.float32 and havg.dtype == np.float32
        for tag, rec, t64 in (("y", y, t), ("max", hmax, tmax), ("avg", havg, tavg)):
            steps = ref.pack_steps(rec, t64)
            assert np.array_equal(ref.unpack_steps(steps, t64).view(np.uint32), rec.view(np.uint32))
            out["pool_%s_%s" % (name, tag)] = steps
            print("pool %s %s: at most %d float32 steps from float32(t)" % (name, tag, int(np.abs(steps).max())))
    path = ref.GOLDEN
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (os.path.relpath(path, ROOT), len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
