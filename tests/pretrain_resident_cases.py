"""Shared cases of the resident pre-training set's tests (CPU and GPU): 13 sentences over 6 images as ``InputExample``s."""
import os

import numpy as np

from helpers import GOLDEN

N_IMG, N_Q = 6, 13
IMG_OF = [0, 5, 2, 0, 3, 1, 4, 2, 0, 5, 3, 3, 1]  # the image of every sample: every image is shared or at least used


def tok():
    from xggm_amd.lxrt.tokenization import BertTokenizer
    return BertTokenizer(os.path.join(GOLDEN, "vocab_small.txt"), do_lower_case=True)


def words():
    return [w for w in open(os.path.join(GOLDEN, "vocab_small.txt")).read().split() if w.isalpha()][:40]


def make_examples(O, F, K, T, n_answers=29, seed=0, n_img=N_IMG, img_of=IMG_OF):
    """``InputExample``s whose images are shared by several sentences; sample 0 has a sentence longer than T - 2 words,
    sample 1 the empty sentence; label dicts have 0, 1, .. K keys (sample 0: K keys in DESCENDING id order, so that the
    insertion order is not the sorted one)"""
    from xggm_amd.pretrain.lxmert_pretrain import InputExample
    rng = np.random.default_rng([seed, O, F, K, T])
    w = words()
    imgs = [(rng.standard_normal((O, F)).astype(np.float32), rng.random((O, 4), dtype=np.float32),
             rng.integers(0, 1600, O).astype(np.int64), rng.random(O, dtype=np.float32),
             rng.integers(0, 400, O).astype(np.int64), rng.random(O, dtype=np.float32)) for _ in range(n_img)]
    out = []
    for q, i in enumerate(img_of):
        n_words = T + 3 if q == 0 else (0 if q == 1 else int(rng.integers(1, max(2, T - 2))))
        sent = " ".join(rng.choice(w, size=n_words)) if n_words else ""
        used = K if q == 0 else q % (K + 1)
        keys = sorted((int(x) for x in rng.choice(n_answers, size=used, replace=False)), reverse=(q == 0))
        label = {k: float(np.float32(rng.random())) for k in keys} if used else (None if q % 2 else {})
        f, b, ol, oc, al, ac = imgs[i]
        out.append(InputExample("img%d_vqa_%03d" % (i, q), sent, (f, b), (ol, oc), (al, ac), 1, label))
    return out
