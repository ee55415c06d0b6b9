"""Generate tests/golden/pretrain_swap.npz by running the REFERENCE's own ``LXMERTTorchDataset.__getitem__``
(src/pretrain/lxmert_data.py:148-199, the matched-sentence swap at :173-183) on a recorded stream of draws.
    python tests/golden/make_pretrain_swap_golden.py <path to the reference's src directory>
The reference's module cannot be imported -- it pulls in the flag parser and the tsv readers -- so the class definition is
taken out of the file with ``ast`` at generation time and executed in a stub namespace; nothing of it is copied.  The object
is made with ``__new__`` (no data files) and ``data``, ``imgid2img``, ``task_matched`` and ``raw_dataset`` are filled by
hand.  The namespace's ``random`` pops recorded float32 draws: ``random()`` returns the next one, ``randint(0, n - 1)``
returns ``floor(u * n)`` of the next one (evaluated in Python floats, i.e. in double).  Per example the consumed draws are
laid out as ``u_swap [B]`` and ``u_pick [B, R]`` (R = 8; the slots the reference did not consume hold seeded draws nobody
looks at), together with the index of the sentence the example came back with and its ``is_matched``.

6 examples (items 0..5) over 3 images, a pool of P = 7 sentences (the flattened data set), T = 7 over the 81-word
vocabulary; one sentence is longer than T - 2 words.  The recorded stream holds
  row 0: u = 0.5 exactly (``0.5 < 0.5`` is false: stays matched);
  row 1: the largest float32 below 0.5 (swapped);
  row 2: two picks that hit the example's own image, then one that succeeds;
  row 3: the largest float32 below 1 as the pick draw: index P - 1;
  row 4: not swapped;  row 5: u = 0 and a pick draw of 0: index 0.
A pick draw whose float32 product ``u * P`` rounds up to P while the double product stays below it does not exist: for
u <= 1 - 2^-24 the exact product is at most P - P 2^-24, and with 2^e < P < 2^(e+1) the float32 spacing below P is
2^(e-23) < P 2^-23, so the product lies more than half a spacing below P and rounds down (a power of two gives an exact
product).  Checked below for P = 7; an exhaustive scan over every float32 in [0, 1) finds no u at all for which
floor(u * 7) differs between float32 and double.  Row 3 is the nearest case there is: the draw that comes closest to the
end of the pool.

Gates (the script fails otherwise): every row consumed at most R - 1 re-draws; the recorded decisions follow the rule of
xggm_pretrain_swap in include/xggm.h."""
import ast
import collections
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
B, T, P, R = 6, 7, 7, 8
SEED = 23
IMG = ["imgA", "imgA", "imgB", "imgB", "imgC", "imgC", "imgA"]  # image of pool sentence j; examples are items 0..5
SENTS = ["what is the man hold ##ing woman", "woman", "is the man", "what man", "the woman is hold ##ing", "man is", "what is"]


class Tokenizer:
    def __init__(self, path):
        self.vocab = collections.OrderedDict((w.rstrip("\n"), i) for i, w in enumerate(open(path, encoding="utf-8")))

    def tokenize(self, s):
        return s.split()

    def convert_tokens_to_ids(self, toks):
        return [self.vocab[t] for t in toks]


class Draws:
    """``random`` of the reference's module: a queue of recorded float32 draws"""

    def __init__(self):
        self.queue, self.picks = collections.deque(), []

    def random(self):
        return float(self.queue.popleft())

    def randint(self, lo, hi):
        assert lo == 0
        u = self.queue.popleft()
        self.picks.append(u)
        return int(float(u) * (hi + 1))


def load_reference(src, draws):
    path = os.path.join(src, "pretrain", "lxmert_data.py")
    tree = ast.parse(open(path).read(), path)
    body = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "LXMERTTorchDataset"]
    assert len(body) == 1
    example = lambda uid, sent, visual_feats, obj_labels, attr_labels, is_matched, label: types.SimpleNamespace(
        uid=uid, sent=sent, visual_feats=visual_feats, obj_labels=obj_labels, attr_labels=attr_labels, is_matched=is_matched, label=label)
    ns = dict(Dataset=object, LXMERTDataset=object, args=types.SimpleNamespace(task_matched=True, tiny=False, fast=False),
              random=draws, np=np, InputExample=example)
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns["LXMERTTorchDataset"]


def rule(u_swap, u_pick, img, pool_img, rate=0.5):
    """the contract of xggm_pretrain_swap in numpy -> (sentence index, is_matched, exhausted)"""
    n, p = len(u_swap), len(pool_img)
    idx, matched, exhausted = np.arange(n, dtype=np.int64), np.ones(n, dtype=np.int64), 0
    for b in range(n):
        if not float(u_swap[b]) < rate:
            continue
        for r in range(u_pick.shape[1]):
            j = min(int(float(u_pick[b, r]) * p), p - 1)
            if pool_img[j] != img[b]:
                idx[b], matched[b] = j, 0
                break
        else:
            exhausted += 1
    return idx, matched, exhausted


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    tok = Tokenizer(os.path.join(HERE, "vocab_small.txt"))
    r = np.random.default_rng(SEED)
    assert len(set(SENTS)) == P == len(IMG) and len(SENTS[0].split()) > T - 2
    pool_ids, pool_mask = np.zeros((P, T), dtype=np.int64), np.zeros((P, T), dtype=np.int64)
    for j, s in enumerate(SENTS):
        w = [tok.vocab["[CLS]"]] + tok.convert_tokens_to_ids(tok.tokenize(s)[:T - 2]) + [tok.vocab["[SEP]"]]
        pool_ids[j, :len(w)], pool_mask[j, :len(w)] = w, 1
    keys = {name: k for k, name in enumerate(sorted(set(IMG)))}
    pool_img = np.array([keys[i] for i in IMG], dtype=np.int64)
    top, half = np.nextafter(np.float32(1), np.float32(0)), np.float32(0.5)
    assert float(np.float32(top * np.float32(P))) < P and int(float(top) * P) == P - 1  # see the docstring: no fp32 draw reaches P
    f = np.float32
    # (u_swap, the pick draws the reference is expected to consume); pool indices by image: A = {0, 1, 6}, B = {2, 3}, C = {4, 5}
    rows = [(half, []),
            (np.nextafter(half, f(0)), [f(0.45)]),             # example 1 (imgA) -> index 3 (imgB)
            (f(0.1), [f(0.30), f(0.43), f(0.75)]),             # example 2 (imgB): 2 (own), 3 (own), then 5 (imgC)
            (f(0.3), [top]),                                   # example 3 (imgB) -> index 6 (imgA)
            (f(0.9), []),
            (f(0.0), [f(0.0)])]                                # example 5 (imgC) -> index 0 (imgA)
    draws = Draws()
    cls = load_reference(sys.argv[1], draws)
    ds = cls.__new__(cls)
    O = 2
    ds.task_matched = True
    ds.raw_dataset = types.SimpleNamespace(answer_table=types.SimpleNamespace(ans2id=lambda a: 0))
    ds.data = [dict(uid="%s_vqa_%03d" % (IMG[j], j), img_id=IMG[j], sent=SENTS[j]) for j in range(P)]
    ds.imgid2img = {name: dict(num_boxes=O, features=r.standard_normal((O, 4), dtype=np.float32), boxes=(50 * r.random((O, 4))).astype(np.float32),
                               objects_id=np.zeros(O, dtype=np.int64), objects_conf=np.ones(O, dtype=np.float32),
                               attrs_id=np.zeros(O, dtype=np.int64), attrs_conf=np.ones(O, dtype=np.float32), img_h=60, img_w=60)
                    for name in keys}
    u_swap, u_pick = np.zeros(B, dtype=np.float32), r.random((B, R), dtype=np.float32)
    sent_index, matched, n_picks = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    for b, (u, picks) in enumerate(rows):
        draws.queue, draws.picks = collections.deque([u] + picks), []
        ex = ds[b]
        assert not draws.queue, "row %d: the reference consumed fewer draws than recorded" % b
        assert len(draws.picks) <= R and len(draws.picks) - 1 <= R - 1, "row %d needs more than R - 1 re-draws" % b
        u_swap[b], n_picks[b] = u, len(draws.picks)
        u_pick[b, :len(draws.picks)] = draws.picks
        sent_index[b], matched[b] = SENTS.index(ex.sent), ex.is_matched
    img = pool_img[:B]
    want = rule(u_swap, u_pick, img, pool_img)
    assert want[2] == 0 and (want[0] == sent_index).all() and (want[1] == matched).all(), (want, sent_index, matched)
    assert matched.tolist() == [1, 0, 0, 0, 1, 0] and sent_index.tolist() == [0, 3, 5, 6, 4, 0] and n_picks.tolist() == [0, 1, 3, 1, 0, 1]
    assert all(pool_img[sent_index[b]] != img[b] for b in range(B) if matched[b] == 0)
    data = dict(pool_ids=pool_ids, pool_mask=pool_mask, pool_img=pool_img, u_swap=u_swap, u_pick=u_pick, sent_index=sent_index,
                is_matched=matched, n_picks=n_picks, cfg=np.array([B, T, P, R], dtype=np.int64), rate=np.array([0.5]))
    path = os.path.join(HERE, "pretrain_swap.npz")
    np.savez_compressed(path, **data)
    print("wrote %s: %d arrays, %d bytes" % (path, len(data), os.path.getsize(path)))


if __name__ == "__main__":
    main()
