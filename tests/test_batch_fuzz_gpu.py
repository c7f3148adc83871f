"""Seeded random sweep of the batched (percnn_pi_batch_*) and ensemble (percnn_pi_ensemble_*) rollouts against the plain-C
oracle looped over the samples: the shape lists of test_fuzz_gpu.py (extents 2, 3, 5, odd widths -> scalar kernels and
unaligned per-sample bases, 100, 129, 3D down to 2 x 2 x 4), every block kind (poly, 2, 4, 8, generic 3 / 6 / 16 -> the
hidden-channel chunks of the ensemble gradient pass), both types, B in {2, 3, 5, 8}, rollout lengths around the tile
kernels' K, and every kind of frame mask.  State and adjoint fields bit-identical per sample, gradients (rows, or their
float64 sum for the shared block) to reduction round-off."""
import numpy as np
import pytest

from util import MASK_KINDS, batch_case_id, check_case, make_case

pytestmark = pytest.mark.gpu

W2 = [4, 6, 8, 12, 20, 24, 28, 32, 36, 44, 48, 52, 64, 96, 100, 132, 256]        # the lists of test_fuzz_gpu._cases()
H2 = [2, 3, 5, 8, 17, 23, 24, 25, 31, 32, 33, 40, 47, 48, 49, 64, 70, 100, 129]
Z3, Y3, X3 = [2, 3, 5, 8, 12], [2, 4, 5, 8, 16], [4, 6, 8, 20, 64, 128, 256]
# odd row lengths (the lists above have none in 2D and none in 3D rows): scalar kernels, and with float32 an odd n puts the
# base of every other sample off 16 bytes
W2_ODD = [3, 5, 7, 33, 101]
X3_ODD = [3, 5, 9, 33]


def _cases():
    rs = np.random.RandomState(20250214)
    out = []
    for i in range(150):
        ndim = 2 if i % 3 else 3
        odd = i % 5 == 0
        if ndim == 2:
            shape = (int(rs.choice(H2)), int(rs.choice(W2_ODD if odd else W2)))
        else:
            shape = (int(rs.choice(Z3)), int(rs.choice(Y3)), int(rs.choice(X3_ODD if odd else X3)))
        hc = int(rs.choice([0, 0, 2, 3, 4, 6, 8, 16]))
        dtype = np.float32 if rs.rand() < 0.6 else np.float64
        B = int(rs.choice([2, 3, 5, 8]))
        T = int(rs.choice([1, 2, 3, 4, 5, 7, 8, 9, 13]))
        mask = MASK_KINDS[int(rs.choice([0, 0, 0, 1, 1, 2, 2, 3, 4]))]
        out.append(make_case(i, shape, hc, dtype, B, T, mask))
    return out


def _large2d_cases():
    """more than 128 tiles of 32 x 32 per sample: default dispatch on the 32 x 32 fused-moments sweep (float32 poly; 384^2,
    416 x 352, 500 x 396), the 32 x 40 tiles (544^2, 640 x 260 forward) and the 40 x 40 tiles of the sweep (576 x 608), ragged
    edges, next to the split schedule of the other block kinds and of float64; T around multiples of K = 4"""
    shapes = [(384, 384), (416, 352), (500, 396), (640, 260), (544, 544), (576, 608)]
    Ts = [4, 7, 8, 5, 3, 9, 4, 8, 6, 5, 7, 4]
    out = []
    for i in range(12):
        hc = [0, 0, 0, 0, 0, 0, 8, 0, 2, 0, 0, 4][i]
        dtype = np.float64 if i in (7, 11) else np.float32
        mask = ("none", "random", "top")[i % 3]
        out.append(make_case(300 + i, shapes[i % 6], hc, dtype, 2 + i % 2, Ts[i], mask))
    return out


def all_cases():
    return _cases() + _large2d_cases()


@pytest.mark.parametrize("case", all_cases(), ids=batch_case_id)
def test_random_batched_and_ensemble_rollout_vs_oracle(case, hip_device):
    check_case(case, hip_device)
