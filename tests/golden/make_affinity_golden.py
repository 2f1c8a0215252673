#!/usr/bin/env python3
"""Pin the pair labels and pair indices of the affinity stage against the REFERENCE's own code.

Build container only (the reference tree does not travel; ``ACR_REFERENCE`` names it):   python tests/golden/make_affinity_golden.py
writes tests/golden/affinity_<tag>.npz (data only, a few KB each).

What runs, imported UNMODIFIED under ``make_data_golden.install_stubs`` (tool/imutils.py imports cv2, pydensecrf and torchvision at
module top; none is called here): ``tool.torchutils.ExtractAffinityLabelInRadius`` (:107-157) on seeded grid-sized label maps, and
``tool.pyutils.get_indices_of_pairs`` (:125-159).  The reference class takes one ``cropsize``: it is square-only, so the non-square
grids are pinned by the index arrays alone (to = from + dy w + dx).  Labels are drawn from {0, 0, 1, 2, 255}: every mask is
non-empty (asserted)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_data_golden import REF, install_stubs  # noqa: E402

SQUARE = {"r5_9": (5, 9), "r5_28": (5, 28), "r3_6": (3, 6), "r2_3": (2, 3)}             # tag -> (radius, size)
INDEX_ONLY = {"r5_12x17": (5, 12, 17), "r3_6x7": (3, 6, 7), "r5_5x75": (5, 5, 75)}      # tag -> (radius, h, w)


def main():
    install_stubs()
    sys.path.insert(0, REF)
    from tool.pyutils import get_indices_of_pairs                  # the reference, unmodified
    from tool.torchutils import ExtractAffinityLabelInRadius
    for seed, (tag, (radius, size)) in enumerate(sorted(SQUARE.items())):
        rng = np.random.RandomState(100 + seed)
        for _ in range(64):                                        # redraw until every mask has a pair (tiny grids)
            label = rng.choice(np.array([0, 0, 1, 2, 255], dtype=np.uint8), size=(size, size))
            bg, fg, neg = ExtractAffinityLabelInRadius(cropsize=size, radius=radius)(label)
            if bg.any() and fg.any() and neg.any():
                break
        assert bg.any() and fg.any() and neg.any(), tag
        frm, to = get_indices_of_pairs(radius, (size, size))
        assert bg.dtype == fg.dtype == neg.dtype == np.float32 and set(np.unique(np.stack([bg, fg, neg]))) <= {0.0, 1.0}
        np.savez_compressed(os.path.join(HERE, "affinity_%s.npz" % tag), radius=np.int32(radius), label=label, bg=bg.astype(np.uint8),
                            fg=fg.astype(np.uint8), neg=neg.astype(np.uint8), idx_from=frm.astype(np.int64), idx_to=to.astype(np.int64))
        print(tag, label.shape, bg.shape, int(bg.sum()), int(fg.sum()), int(neg.sum()))
    for tag, (radius, h, w) in sorted(INDEX_ONLY.items()):
        frm, to = get_indices_of_pairs(radius, (h, w))
        np.savez_compressed(os.path.join(HERE, "affinity_%s.npz" % tag), radius=np.int32(radius), hw=np.array([h, w], np.int32),
                            idx_from=frm.astype(np.int64), idx_to=to.astype(np.int64))
        print(tag, frm.shape, to.shape)


if __name__ == "__main__":
    main()
