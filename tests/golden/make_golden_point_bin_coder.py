"""Record encode_torch / decode_torch of the reference's PointBinResidualCoder into point_bin_coder.npz (read by
tests/test_point_head_cpu.py).

Usage: python tests/golden/make_golden_point_bin_coder.py /path/to/reference/checkout

Inputs are fixed here: random boxes plus headings on bin edges, negative and > 2 pi headings; encodings with tied bin
scores (the first maximum wins).  Both use_mean_size settings are recorded; the reference's .cuda() of mean_size is
redirected to the CPU."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_sa_keys as sa_keys  # noqa: E402

BINS = 12
MEAN_SIZE = [[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]]


def inputs():
    rng = np.random.default_rng(0)
    n = 64
    boxes = np.zeros((n, 8), np.float32)
    boxes[:, 0:3] = rng.uniform(-40, 70, (n, 3))
    boxes[:, 3:6] = rng.uniform(0.3, 5.0, (n, 3))
    boxes[:, 6] = rng.uniform(-7.0, 14.0, n)
    step = 2 * np.pi / BINS
    edges = np.array([0.0, step / 2, -step / 2, 3 * step / 2, np.pi, -np.pi, 2 * np.pi, 2 * np.pi + step / 2,
                      4 * np.pi - 1e-3, -2 * np.pi - step / 2, 11 * step + step / 2, 1e-7], np.float32)
    boxes[:len(edges), 6] = edges
    boxes[-1, 3] = 0.0                                # clamped to 1e-5
    boxes[:, 7] = rng.integers(1, 4, n)
    points = (boxes[:, 0:3] + rng.uniform(-2, 2, (n, 3))).astype(np.float32)
    classes = boxes[:, 7].astype(np.int64)
    enc = rng.standard_normal((n, 6 + 2 * BINS)).astype(np.float32)
    enc[:8, 6:6 + BINS] = 0.5                         # all bins tied
    enc[8:16, 6 + 3] = enc[8:16, 6 + 7] = 9.0         # two bins tied above the rest
    return boxes[:, :7].copy(), points, classes, enc


def main(ref_root):
    sa_keys.install_stubs(ref_root)
    torch.Tensor.cuda = lambda self, *a, **k: self
    from pcdet.utils import box_coder_utils as ref
    boxes, points, classes, enc = inputs()
    out = dict(boxes=boxes, points=points, classes=classes, enc=enc)
    for mean in (False, True):
        tag = "mean" if mean else "plain"
        coder = ref.PointBinResidualCoder(use_mean_size=mean, angle_bin_num=BINS, mean_size=MEAN_SIZE)
        cls_t = torch.from_numpy(classes)
        out["encode_" + tag] = coder.encode_torch(torch.from_numpy(boxes.copy()), torch.from_numpy(points),
                                                  cls_t).numpy()
        out["decode_" + tag] = coder.decode_torch(torch.from_numpy(enc), torch.from_numpy(points), cls_t).numpy()
    np.savez_compressed(os.path.join(HERE, "point_bin_coder.npz"), **out)
    print("wrote", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
