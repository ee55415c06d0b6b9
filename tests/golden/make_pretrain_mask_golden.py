"""Generate tests/golden/pretrain_mask.npz by running the REFERENCE's own ``random_word``, ``random_feat`` and
``convert_example_to_features`` (src/pretrain/lxmert_pretrain.py:76-215) on recorded draws.
    python tests/golden/make_pretrain_mask_golden.py <path to the reference's src directory>
The reference's module cannot be imported -- it builds its data sets at import (:50-53) -- so the three definitions are
taken out of the file with ``ast`` at generation time and executed in a stub namespace; nothing of it is copied.  The
namespace provides ``args`` with the two rates, a whitespace tokenizer over tests/golden/vocab_small.txt, a ``random`` whose
``.random()`` pops the recorded draw of the current position and whose ``.choice(seq)`` returns ``seq[int(u2 * len(seq))]``
with that position's pick draw, and ``train_tuple.torchdset.random_feat()`` returning ``pool[int(u2 * P)]``.

Two batches of B = 3, T = 8, O = 5, F = 24 over the 81-word vocabulary, a pool of 7 rows.  Sentences: one longer than T - 2
words (cut to the full length L = T), an empty one ([CLS][SEP] alone, L = 2) and a single word (L = 3).  Draws are float32.
Batch 0 puts on the 7 eligible word positions and on 7 object rows: 0 and the float32 neighbours on both sides of ``rate``,
``0.8 rate`` and ``0.9 rate`` (the last float32 for which the reference's comparison is true, and its successor); the
largest float32 below 1 is the pick draw of a replaced word and of a replaced row (index V - 1 / P - 1).  Ineligible word
positions carry the draw 0, which would mask them if they were looked at.  Batch 1: word draws inside every interval (seven
positions are too few to leave to a seed), seeded object draws.  Answers: several keys, one
key, no label | ``is_matched = 0`` with a label, an empty dict, several keys.  The several-keys case is
``np.random.multinomial`` in the reference, whose stream cannot be fed from outside: those entries alone come from the
float64 restatement (tests/pretrain_mask_ref.py) on the recorded ``u_ans``.

Gates: all four word outcomes and all four object outcomes occur in EACH batch, and the restatement reproduces everything
the reference returned; a draw set that fails is replaced, the gates are never dropped."""
import ast
import collections
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pretrain_mask_ref as R  # noqa: E402

B, T, O, F, P = 3, 8, 5, 24, 7
WORD_RATE, OBJ_RATE = 0.15, 0.15
SEED = 11
WANTED = ("random_word", "random_feat", "convert_example_to_features")
SENTS = ["what is the man hold ##ing woman", "", "woman"]
LABELS = [[{3: 0.3, 7: 0.6, 11: 1.0}, {5: 1.0}, None], [{4: 0.9}, {}, {2: 0.5, 9: 0.25}]]
MATCHED = [[1, 1, 1], [0, 1, 1]]
K = 3


class Tokenizer:
    def __init__(self, path):
        self.vocab = collections.OrderedDict((w.rstrip("\n"), i) for i, w in enumerate(open(path, encoding="utf-8")))

    def tokenize(self, s):
        return s.split()

    def convert_tokens_to_ids(self, toks):
        return [self.vocab[t] for t in toks]


class Draws:
    """``random`` of the reference: one (u, u2) pair per decision, in the order the reference asks"""

    def __init__(self):
        self.queue, self.pick = collections.deque(), None

    def random(self):
        u, self.pick = self.queue.popleft()
        return u

    def choice(self, seq):
        return seq[int(self.pick * len(seq))]


def load_reference(src, tok, draws, pool):
    path = os.path.join(src, "pretrain", "lxmert_pretrain.py")
    tree = ast.parse(open(path).read(), path)
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANTED]
    assert sorted(n.name for n in body) == sorted(WANTED)
    ns = dict(args=types.SimpleNamespace(word_mask_rate=WORD_RATE, obj_mask_rate=OBJ_RATE), random=draws, np=np,
              InputExample=object, InputFeatures=lambda **kw: types.SimpleNamespace(**kw),
              train_tuple=types.SimpleNamespace(torchdset=types.SimpleNamespace(
                  random_feat=lambda: pool[int(draws.pick * len(pool))])))
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns["convert_example_to_features"]


def edge_draws(rate):
    below = lambda th: (lambda x: x / rate < th)
    e8, e9 = R.fp32_edges(below(0.8), 0.8 * rate), R.fp32_edges(below(0.9), 0.9 * rate)
    er = R.fp32_edges(lambda x: x < rate, rate)
    return np.array([0.0, e8[0], e8[1], e9[0], e9[1], er[0], er[1]], dtype=np.float32)


def spread(r, shape, rate):
    """seeded draws that land in each of the four intervals of ``rate`` about equally often (uniform draws would put 1.5 % of
    them into the replace interval: too few for 15 rows)"""
    lo = np.array([0.0, 0.8 * rate, 0.9 * rate, rate])
    hi = np.array([0.8 * rate, 0.9 * rate, rate, 1.0])
    k = r.integers(0, 4, size=shape)
    return (lo[k] + (0.05 + 0.9 * r.random(shape)) * (hi[k] - lo[k])).astype(np.float32)


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    tok = Tokenizer(os.path.join(HERE, "vocab_small.txt"))
    V = len(tok.vocab)
    r = np.random.default_rng(SEED)
    feats = r.standard_normal((B, O, F), dtype=np.float32)
    pool = r.standard_normal((P, F), dtype=np.float32)
    boxes = r.random((B, O, 4), dtype=np.float32)
    ids, mask = np.zeros((B, T), dtype=np.int64), np.zeros((B, T), dtype=np.int64)
    for b, s in enumerate(SENTS):
        w = [tok.vocab["[CLS]"]] + tok.convert_tokens_to_ids(tok.tokenize(s)[:T - 2]) + [tok.vocab["[SEP]"]]
        ids[b, :len(w)], mask[b, :len(w)] = w, 1
    assert sorted(mask.sum(1).tolist()) == [2, 3, T]
    eligible = [(b, t) for b in range(B) for t in range(1, T - 1) if mask[b, t] == 1 and mask[b, t + 1] == 1]
    assert len(eligible) == 7
    top = np.nextafter(np.float32(1), np.float32(0))
    data = dict(input_ids=ids, input_mask=mask, feats=feats, pool=pool,
                cfg=np.array([B, T, O, F, P, K, V, tok.vocab["[MASK]"]], dtype=np.int64),
                rates=np.array([WORD_RATE, OBJ_RATE], dtype=np.float64))
    draws = Draws()
    convert = load_reference(sys.argv[1], tok, draws, pool)
    for c in range(2):
        d = dict(u_word=np.zeros((B, T), dtype=np.float32), u_word_pick=r.random((B, T), dtype=np.float32),
                 u_obj=spread(r, (B, O), OBJ_RATE), u_obj_pick=r.random((B, O), dtype=np.float32),
                 u_ans=r.random(B, dtype=np.float32))
        if c == 0:
            ew, eo = edge_draws(WORD_RATE), edge_draws(OBJ_RATE)
            for (b, t), u in zip(eligible, ew):
                d["u_word"][b, t] = u
            d["u_word_pick"][eligible[2]] = top  # the first replaced word: index V - 1
            d["u_obj"].reshape(-1)[1:8] = eo     # rows 1..7; the rest stays seeded
            d["u_obj_pick"].reshape(-1)[3] = top  # the first replaced row: pool row P - 1
            d["u_ans"][0] = 0.2
        else:
            for (b, t), u in zip(eligible, (0.6, 0.128, 0.03, 0.14, 0.2, 0.11, 0.131)):  # interior of every interval
                d["u_word"][b, t] = np.float32(u)
            d["u_ans"][2] = top
        lab_ids, lab_scores = np.full((B, K), -1, dtype=np.int64), np.zeros((B, K), dtype=np.float32)
        for b, lab in enumerate(LABELS[c]):
            for j, (k, v) in enumerate((lab or {}).items()):
                lab_ids[b, j], lab_scores[b, j] = k, v
        matched = np.array(MATCHED[c], dtype=np.int64)
        want = R.corrupt(ids, mask, feats, matched, lab_ids, lab_scores, d, WORD_RATE, OBJ_RATE, V, tok.vocab["[MASK]"], pool)
        assert set(want["word_kind"][want["word_kind"] >= 0].tolist()) == {0, 1, 2, 3}, "word outcomes: replace the draws"
        assert set(want["obj_kind"].reshape(-1).tolist()) == {0, 1, 2, 3}, "object outcomes: replace the draws"
        if c == 0:
            assert (want["input_ids"] == V - 1).any() and any((row == pool[P - 1]).all() for row in want["masked_feat"].reshape(-1, F))
        got = {k: [] for k in ("input_ids", "masked_lm_labels", "masked_feat", "feat_mask", "ans")}
        for b in range(B):
            L = int(mask[b].sum())
            draws.queue = collections.deque([(float(d["u_word"][b, t]), float(d["u_word_pick"][b, t])) for t in range(1, L - 1)]
                                            + [(float(d["u_obj"][b, o]), float(d["u_obj_pick"][b, o])) for o in range(O)])
            ex = types.SimpleNamespace(sent=SENTS[b], visual_feats=(feats[b], boxes[b]), obj_labels=(None, None),
                                       attr_labels=(None, None), is_matched=int(matched[b]),
                                       label={k: float(np.float32(v)) for k, v in LABELS[c][b].items()} if LABELS[c][b] is not None else None)
            f = convert(ex, T, tok)
            assert not draws.queue and f.input_mask == mask[b].tolist() and f.obj_labels["feat"][0] is ex.visual_feats[0]
            several = LABELS[c][b] is not None and len(LABELS[c][b]) > 1 and matched[b] == 1
            assert several or f.ans == want["ans"][b]  # every other answer case IS the reference's
            got["input_ids"].append(f.input_ids), got["masked_lm_labels"].append(f.lm_label_ids)
            got["masked_feat"].append(f.visual_feats[0]), got["feat_mask"].append(f.obj_labels["feat"][1])
            got["ans"].append(want["ans"][b] if several else f.ans)
        out = dict(input_ids=np.array(got["input_ids"], dtype=np.int64), masked_lm_labels=np.array(got["masked_lm_labels"], dtype=np.int64),
                   masked_feat=np.stack(got["masked_feat"]).astype(np.float32), feat_mask=np.stack(got["feat_mask"]).astype(np.float32),
                   ans=np.array(got["ans"], dtype=np.int64))
        for k, v in out.items():  # the restatement reproduces the reference: integers equal, features bit-equal
            assert v.dtype == want[k].dtype and v.tobytes() == want[k].tobytes(), k
            data["b%d.out.%s" % (c, k)] = v
        for k, v in d.items():
            data["b%d.%s" % (c, k)] = v
        data["b%d.label_ids" % c], data["b%d.label_scores" % c], data["b%d.is_matched" % c] = lab_ids, lab_scores, matched
    path = os.path.join(HERE, "pretrain_mask.npz")
    np.savez_compressed(path, **data)
    assert os.path.getsize(path) < os.path.getsize(os.path.join(HERE, "pretrain.npz"))
    print("wrote %s: %d arrays, %d bytes" % (path, len(data), os.path.getsize(path)))


if __name__ == "__main__":
    main()
