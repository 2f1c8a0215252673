"""The affinity stage without a GPU: the restatement (tests/affinity_ref.py) against fixtures written by the reference's own
``ExtractAffinityLabelInRadius`` and ``get_indices_of_pairs`` (tests/golden/make_affinity_golden.py) bit for bit, the sparse step
iteration against the dense matrix power in float64, and the ABI's names."""
import os

import numpy as np
import pytest
import torch

import abi_checks
import affinity_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SQUARE = ("r5_9", "r5_28", "r3_6", "r2_3")
INDEX_ONLY = ("r5_12x17", "r3_6x7", "r5_5x75")
ABI = ("acr_aff_pairs", "acr_aff_pair_codes", "acr_aff_loss_ws_bytes", "acr_aff_loss_fwd", "acr_aff_loss_bwd", "acr_aff_walk_weights",
       "acr_aff_walk_resident", "acr_aff_walk_ws_bytes", "acr_aff_walk")


def gold(tag):
    return np.load(os.path.join(GOLD, "affinity_%s.npz" % tag))


@pytest.mark.parametrize("tag", SQUARE)
def test_masks_and_indices_equal_the_reference(tag):
    g = gold(tag)
    radius, label = int(g["radius"]), torch.from_numpy(g["label"])
    bg, fg, neg = R.pair_masks(label, radius)
    for name, m in (("bg", bg), ("fg", fg), ("neg", neg)):
        assert g[name].any(), name                            # the fixture exercises every mask
        assert np.array_equal(m.numpy().astype(np.uint8), g[name]), name
    frm, to = R.pair_indices(radius, *label.shape)
    assert np.array_equal(frm.numpy(), g["idx_from"]) and np.array_equal(to.reshape(-1).numpy(), g["idx_to"])
    codes, counts = R.pair_codes(label[None], radius, 1)
    assert np.array_equal(codes[0].numpy(), g["bg"] + 2 * g["fg"] + 3 * g["neg"])
    assert counts.tolist() == [int(g["bg"].sum()), int(g["fg"].sum()), int(g["neg"].sum())]


@pytest.mark.parametrize("tag", INDEX_ONLY)
def test_indices_of_non_square_grids_equal_the_reference(tag):
    g = gold(tag)
    h, w = (int(v) for v in g["hw"])
    frm, to = R.pair_indices(int(g["radius"]), h, w)
    assert np.array_equal(frm.numpy(), g["idx_from"]) and np.array_equal(to.reshape(-1).numpy(), g["idx_to"])


def test_geometry_counts_and_refusals():
    assert len(R.search_dist(5)) == 34 and len(R.search_dist(3)) == 12 and len(R.search_dist(2)) == 4
    assert R.search_dist(5)[:5] == [(0, 1), (0, 2), (0, 3), (0, 4), (1, -4)]
    frm, to = R.pair_indices(5, 9, 9)
    assert frm.numel() == 5 and tuple(to.shape) == (34, 5)     # a single from-column
    for h, w in ((4, 20), (20, 8)):
        with pytest.raises(ValueError):
            R.pair_indices(5, h, w)
    from acr_wsss_amd import affinity as A
    assert A.search_dist(5) == R.search_dist(5)
    assert A._geometry(56, 56, 5) == (34, 52 * 48)
    for args in ((4, 20, 5), (20, 8, 5), (20, 20, 1), (20, 20, 6)):
        with pytest.raises(ValueError):
            A._geometry(*args)


def test_subsampling_rule():
    m = torch.arange(16 * 24, dtype=torch.int64).view(1, 16, 24)
    g = R.subsample(m, 8)
    assert g.tolist() == [[[0, 8, 16], [192, 200, 208]]]
    with pytest.raises(ValueError):
        R.subsample(m[:, :15], 8)


@pytest.mark.parametrize("radius,h,w,K", [(5, 9, 9, 1), (5, 12, 17, 3), (3, 6, 7, 2)])
def test_step_iteration_equals_the_dense_power_in_float64(radius, h, w, K):
    g = torch.Generator().manual_seed(h * w)
    P, N = len(R.search_dist(radius)), (h - radius + 1) * (w - 2 * radius + 2)
    aff = torch.rand(P, N, generator=g, dtype=torch.float64) * 0.9 + 0.1
    scores = torch.rand(K, h, w, generator=g, dtype=torch.float64)
    T = R.transition(aff, h, w, radius, 2)
    assert torch.equal(T > 0, T.t() > 0)                                               # the support is symmetric
    assert float((T.sum(0) - 1).abs().max()) <= 1e-15                                  # column-stochastic
    for steps in (0, 1, 2, 16):
        dense = R.walk_dense(aff, scores, radius, 2, None, steps)
        sparse = R.walk_steps(aff, scores, radius, 2, steps)
        err = float((dense - sparse).abs().max())
        print("R %d, %d x %d, %d steps: max|dense - steps| = %.3e" % (radius, h, w, steps, err))
        assert err <= 1e-14
    assert float((R.walk_dense(aff, scores, radius, 2, 4) - R.walk_steps(aff, scores, radius, 2, 16)).abs().max()) <= 1e-14
    assert torch.equal(R.walk_steps(aff, scores, radius, 2, 0), scores)


def test_loss_restatement_edge_cases():
    g = torch.Generator().manual_seed(1)
    label = torch.from_numpy(gold("r5_9")["label"])[None]
    codes, counts = R.pair_codes(label, 5, 1)
    feat = torch.full((1, 3, 9, 9), 0.25, dtype=torch.float64)
    loss, bg, fg, neg, aff = R.aff_loss(feat, codes, counts, 5)
    assert torch.equal(aff, torch.ones_like(aff))
    assert abs(float(bg) - -np.log(1 + 1e-5) * float(counts[0]) / (float(counts[0]) + 1e-5)) <= 1e-15
    none = torch.full_like(label, 255)
    c0, n0 = R.pair_codes(none, 5, 1)
    assert not c0.any() and n0.tolist() == [0, 0, 0]
    out = R.aff_loss(torch.rand(1, 3, 9, 9, generator=g, dtype=torch.float64), c0, n0, 5)
    assert all(float(v) == 0.0 for v in out[:4])


def test_abi_names_in_signatures_and_header():
    from acr_wsss_amd import _lib
    for name in ABI:
        assert name in _lib.SIGNATURES, name
        assert name in abi_checks.PROTOTYPES, name
    assert "affinity.hip" in open(os.path.join(ROOT, "acr_wsss_amd", "csrc", "Makefile")).read()


def test_argument_errors_without_a_gpu():
    from acr_wsss_amd import affinity as A
    with pytest.raises(ValueError):
        A.pair_codes(torch.zeros(1, 16, 16), 5, 8)                 # not uint8
    with pytest.raises(ValueError):
        A.pair_codes(torch.zeros(1, 2, 3, 4, dtype=torch.uint8), 5, 8)
    with pytest.raises(ValueError):
        A.pair_affinity(torch.zeros(2, 3, 9), 5)
    with pytest.raises(ValueError):
        A.random_walk(torch.zeros(1, 34, 5), torch.zeros(1, 9, 9), logt=8)
