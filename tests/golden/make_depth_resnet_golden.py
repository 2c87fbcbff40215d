"""Regenerate tests/golden/depth_resnet.npz and tests/golden/depth_resnet_keys.txt:  python tests/golden/make_depth_resnet_golden.py

Everything comes from our own restatement (tests/depth_resnet_ref.py): the network of the reference's depth encoder lives in
habitat-lab, which is not part of the reference tree, so there is no reference program to record.  Per case of
depth_resnet_ref.CASES: the fp64 output on the seeded images with the seeded weights, the restatement's own CPU distance from
it in fp32 and under bfloat16 autocast (rel-L2 and max-abs / absmax), and the fraction of zeros in the output.  The bf16 gate of
tests/test_gpu_depth_resnet.py is a multiple of the recorded bfloat16 figure.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main():
    from tests import depth_resnet_ref as R
    with open(os.path.join(HERE, "depth_resnet_keys.txt"), "w") as f:
        for k, s in R.shapes().items():
            f.write(f"{k} {s}\n")
    out = {}
    for case in R.CASES:
        y = R.run(case).numpy()
        out[case + "_out"] = y
        out[case + "_zero_fraction"] = np.array(float((y == 0).mean()))
        report = [f"{case}: {y.shape}, |y| max {np.abs(y).max():.3f}, zeros {float((y == 0).mean()):.3f}"]
        for tag, got in (("fp32", R.run(case, torch.float32)), ("bf16", R.run(case, torch.float32, autocast=True))):
            out[f"{case}_{tag}_rel_l2"] = np.array(R.rel_l2(got.numpy(), y))
            out[f"{case}_{tag}_max_rel"] = np.array(R.max_rel(got.numpy(), y))
            report.append(f"  {tag}: rel-L2 {R.rel_l2(got.numpy(), y):.3e} max-abs/absmax {R.max_rel(got.numpy(), y):.3e}")
        print("\n".join(report), flush=True)
    path = os.path.join(HERE, "depth_resnet.npz")
    np.savez_compressed(path, **out)
    print("depth_resnet.npz", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1 << 20


if __name__ == "__main__":
    main()
