#!/usr/bin/env python3
"""Generate tests/golden/lovasz_kats.npz by running the REFERENCE's lovasz_softmax (head_seg/loss_lovasz.py) on CPU, called the way the
reference model calls it with segment.use_lovasz (model.py:207-210): lovasz_softmax(F.softmax(seg, 1), gt_seg.long(), ignore=255).

Only data is written: logits, targets (as given to HydraNet.cal_loss: int64 or float32), the loss and logits.grad per case.  The logits are
continuous random values, so no two errors tie and the reference's unstable sort gives a well-defined gradient.
Run:  python tests/golden/make_golden_lovasz.py"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/model/head_seg/loss_lovasz.py"
sys.dont_write_bytecode = True


def _reference():
    spec = importlib.util.spec_from_file_location("ref_loss_lovasz", REF)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.lovasz_softmax


def _cases(g):
    def labels(shape, values):
        return torch.tensor(values)[torch.randint(0, len(values), shape, generator=g)]

    out = {}
    # ignore pixels (a 255 block and scattered ones) + an absent class (3)
    t = labels((2, 6, 7), [0, 1, 2, 4])
    t[0, :2, :3] = 255
    t[1, 4, 1::2] = 255
    out["ignore_absent"] = (torch.randn(2, 5, 6, 7, generator=g) * 2.0, t)
    # a single present class (everything else ignored)
    t = torch.full((1, 5, 8), 255, dtype=torch.int64)
    t[0, 1:4, 2:6] = 3
    out["single_class"] = (torch.randn(1, 5, 5, 8, generator=g) * 2.0, t)
    # labels out of range (7, 9: background for every class), with ignore pixels
    t = labels((2, 5, 6), [0, 1, 2, 3, 4, 7, 9, 255])
    out["out_of_range"] = (torch.randn(2, 5, 5, 6, generator=g) * 2.0, t)
    # float32 class ids (what to_gpu delivers); the reference sees gt_seg.long()
    t = labels((2, 4, 9), [0, 1, 2, 3, 255]).to(torch.float32)
    out["float_target"] = (torch.randn(2, 4, 4, 9, generator=g) * 2.0, t)
    # three classes, no ignore pixels
    out["plain_c3"] = (torch.randn(2, 3, 7, 5, generator=g) * 2.0, labels((2, 7, 5), [0, 1, 2]))
    return out


def main():
    lovasz_softmax = _reference()
    g = torch.Generator().manual_seed(20261015)
    rec = {}
    for name, (logits, target) in _cases(g).items():
        x = logits.clone().requires_grad_(True)
        loss = lovasz_softmax(F.softmax(x, dim=1), target.long(), ignore=255)
        loss.backward()
        rec[f"{name}/logits"] = logits.numpy().astype(np.float32)
        rec[f"{name}/target"] = target.numpy()
        rec[f"{name}/loss"] = np.array(float(loss.detach()), dtype=np.float64)
        rec[f"{name}/grad"] = x.grad.numpy().astype(np.float64)
    np.savez_compressed(os.path.join(HERE, "lovasz_kats.npz"), **rec)
    print("wrote", sorted({k.split("/")[0] for k in rec}))


if __name__ == "__main__":
    main()
