"""WordPiece tokenisation with the reference's class names (src/lxrt/tokenization.py:72-348).

The reference resolves ``bert-base-uncased`` to a vocabulary URL; offline the vocabulary must
be a local ``vocab.txt`` (one token per line, line number = id).  The algorithm is BERT's
published one: clean + lower-case + strip accents + split punctuation/CJK, then greedy
longest-match-first WordPiece with the ``##`` continuation prefix.

``DeviceTokenizer`` runs the same conversion for a whole list of sentences in one launch (contract:
xggm_tokenize_wordpiece in include/xggm.h) from tables built here: ``code_point_table`` and ``host_tables``.
``Restatement`` restates the kernel in Python from the same tables -- the reference the kernel's algorithm is tested
against on the CPU, NOT a fallback.
"""
import collections
import os
import unicodedata

import numpy as np


def load_vocab(vocab_file):
    vocab = collections.OrderedDict()
    with open(vocab_file, "r", encoding="utf-8") as f:
        for idx, line in enumerate(f):
            tok = line.rstrip("\n")
            if tok:
                vocab[tok.strip()] = idx
    return vocab


def whitespace_tokenize(text):
    text = text.strip()
    return text.split() if text else []


def _is_punct(ch):
    cp = ord(ch)
    if 33 <= cp <= 47 or 58 <= cp <= 64 or 91 <= cp <= 96 or 123 <= cp <= 126:
        return True
    return unicodedata.category(ch).startswith("P")


def _is_cjk(cp):
    return (0x4E00 <= cp <= 0x9FFF or 0x3400 <= cp <= 0x4DBF or 0x20000 <= cp <= 0x2A6DF or 0x2A700 <= cp <= 0x2B73F
            or 0x2B740 <= cp <= 0x2B81F or 0x2B820 <= cp <= 0x2CEAF or 0xF900 <= cp <= 0xFAFF
            or 0x2F800 <= cp <= 0x2FA1F)


class BasicTokenizer(object):
    """ref: src/lxrt/tokenization.py:174-288"""

    def __init__(self, do_lower_case=True, never_split=("[UNK]", "[SEP]", "[PAD]", "[CLS]", "[MASK]")):
        self.do_lower_case = do_lower_case
        self.never_split = never_split

    def tokenize(self, text):
        cleaned = []
        for ch in text:
            cp = ord(ch)
            if cp == 0 or cp == 0xFFFD or (unicodedata.category(ch) in ("Cc", "Cf") and ch not in "\t\n\r"):
                continue
            if ch in " \t\n\r" or unicodedata.category(ch) == "Zs":
                cleaned.append(" ")
            elif _is_cjk(cp):
                cleaned.extend((" ", ch, " "))
            else:
                cleaned.append(ch)
        out = []
        for tok in whitespace_tokenize("".join(cleaned)):
            if tok in self.never_split:
                out.append(tok)
                continue
            if self.do_lower_case:
                tok = "".join(c for c in unicodedata.normalize("NFD", tok.lower()) if unicodedata.category(c) != "Mn")
            word = []
            for ch in tok:
                if _is_punct(ch):
                    if word:
                        out.append("".join(word))
                        word = []
                    out.append(ch)
                else:
                    word.append(ch)
            if word:
                out.append("".join(word))
        return out


class WordpieceTokenizer(object):
    """greedy longest-match-first; ref: src/lxrt/tokenization.py:291-348"""

    def __init__(self, vocab, unk_token="[UNK]", max_input_chars_per_word=100):
        self.vocab = vocab
        self.unk_token = unk_token
        self.max_input_chars_per_word = max_input_chars_per_word

    def tokenize(self, text):
        out = []
        for token in whitespace_tokenize(text):
            if len(token) > self.max_input_chars_per_word:
                out.append(self.unk_token)
                continue
            pieces, start, bad = [], 0, False
            while start < len(token):
                end = len(token)
                cur = None
                while start < end:
                    sub = token[start:end]
                    if start > 0:
                        sub = "##" + sub
                    if sub in self.vocab:
                        cur = sub
                        break
                    end -= 1
                if cur is None:
                    bad = True
                    break
                pieces.append(cur)
                start = end
            out.extend([self.unk_token] if bad else pieces)
        return out


class BertTokenizer(object):
    """ref: src/lxrt/tokenization.py:72-171"""

    def __init__(self, vocab_file, do_lower_case=True, max_len=None,
                 never_split=("[UNK]", "[SEP]", "[PAD]", "[CLS]", "[MASK]")):
        if not os.path.isfile(vocab_file):
            raise ValueError("Can't find a vocabulary file at path '{}' (no download offline)".format(vocab_file))
        self.vocab = load_vocab(vocab_file)
        self.ids_to_tokens = collections.OrderedDict([(ids, tok) for tok, ids in self.vocab.items()])
        self.basic_tokenizer = BasicTokenizer(do_lower_case=do_lower_case, never_split=never_split)
        self.wordpiece_tokenizer = WordpieceTokenizer(vocab=self.vocab)
        self.max_len = max_len if max_len is not None else int(1e12)

    def tokenize(self, text):
        return [sub for tok in self.basic_tokenizer.tokenize(text) for sub in self.wordpiece_tokenizer.tokenize(tok)]

    def convert_tokens_to_ids(self, tokens):
        ids = [self.vocab[t] for t in tokens]
        if len(ids) > self.max_len:
            raise ValueError("Token indices sequence length is longer than the specified maximum sequence length "
                             "for this BERT model ({} > {}).".format(len(ids), self.max_len))
        return ids

    def convert_ids_to_tokens(self, ids):
        return [self.ids_to_tokens[i] for i in ids]

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, cache_dir=None, *inputs, **kwargs):
        path = pretrained_model_name_or_path
        if os.path.isdir(path):
            path = os.path.join(path, "vocab.txt")
        return cls(path, *inputs, **kwargs)


# ----------------------------------------------------------------------------- tokenising on the device
ACT_KEEP, ACT_DROP, ACT_SPACE, ACT_CJK, ACT_HOST = 0, 1, 2, 3, 4  # bits 0-2 of a code point's table entry
MAX_WORD, MAX_NEVER = 100, 8                                      # XGGM_TOKENIZE_MAX_WORD / _MAX_NEVER (include/xggm.h)
HASH_MUL, HASH_MUL_INV = 0x9E3779B97F4A7C15, 0xF1DE83E19937733D   # XGGM_TOKENIZE_HASH_MUL / _INV: inverses modulo 2^64
_M64 = (1 << 64) - 1
N_CODE_POINTS = 0x110000
_cp_table_cache = None


def fold_of(ch):
    """what ``BasicTokenizer`` makes of ONE character of a lower-cased token: lower, NFD, drop Mn"""
    return [c for c in unicodedata.normalize("NFD", ch.lower()) if unicodedata.category(c) != "Mn"]


def needs_host(cp, fold):
    """the two effects of the host's fold that are no function of one code point: U+03A3 lower-cases by context (final
    sigma), and a surviving character of non-zero combining class may be reordered by NFD against a neighbour of its kind"""
    return cp == 0x3A3 or any(unicodedata.combining(c) != 0 for c in fold)


def code_point_table():
    """-> (table uint32 [0x110000], ext uint32 [n_ext]) from the running interpreter's ``unicodedata``; the entry layout is
    the one of xggm_tokenize_wordpiece in include/xggm.h: bits 0-2 action, 3-4 length nf of the folded sequence, 5-7
    punctuation flag per folded character, 8-28 the folded code point (nf == 1) or an index into ``ext`` (nf > 1)."""
    global _cp_table_cache
    if _cp_table_cache is not None:
        return _cp_table_cache
    cat_of, nfd = unicodedata.category, unicodedata.normalize
    table = (np.arange(N_CODE_POINTS, dtype=np.uint32) << 8) | np.uint32(1 << 3)  # keep, folds to itself, no punctuation
    ext = []
    for cp in range(N_CODE_POINTS):
        ch = chr(cp)
        cat = cat_of(ch)
        if (cat[0] not in "CZMP" or cat in ("Cn", "Co")) and cp > 127 and cp != 0xFFFD and not _is_cjk(cp) and nfd("NFD", ch.lower()) == ch:
            continue  # the common case, already in place
        if cp == 0 or cp == 0xFFFD or (cat in ("Cc", "Cf") and ch not in "\t\n\r"):
            table[cp] = ACT_DROP
            continue
        if ch in " \t\n\r" or cat == "Zs" or ch.isspace():  # U+2028 / U+2029 survive the cleaning and split in str.split()
            table[cp] = ACT_SPACE
            continue
        fold = fold_of(ch)
        if len(fold) > 3:
            raise ValueError("code point U+%04X folds to %d characters, the table holds 3" % (cp, len(fold)))
        act = ACT_HOST if needs_host(cp, fold) else (ACT_CJK if _is_cjk(cp) else ACT_KEEP)
        e = act | (len(fold) << 3)
        for f, c in enumerate(fold):
            if _is_punct(c):
                e |= 1 << (5 + f)
        if len(fold) == 1:
            e |= ord(fold[0]) << 8
        elif len(fold) > 1:
            e |= len(ext) << 8
            ext.extend(ord(c) for c in fold)
        table[cp] = e
    _cp_table_cache = (table, np.asarray(ext, dtype=np.uint32))
    return _cp_table_cache


def piece_hash(cps):
    """the polynomial hash of xggm_tokenize_wordpiece over code points, modulo 2^64"""
    h = 0
    for c in cps:
        h = (h * HASH_MUL + c + 1) & _M64
    return h


def build_hash_table(entries, capacity=None):
    """``entries``: [(code points, id, offset into the blob)] -> uint32 [capacity, 4] slots {hash >> 32, id, offset, length},
    id 0xFFFFFFFF (-1) = empty.  Open addressing, linear probing from (h ^ (h >> 32)) & (capacity - 1).  ``capacity``: a
    power of two that leaves at least one slot empty (default: the first one >= 2 x entries); an insert that finds no room,
    or a key that is already present, raises."""
    if capacity is None:
        capacity = 16
        while capacity < 2 * len(entries):
            capacity *= 2
    capacity = int(capacity)
    if capacity < 1 or capacity & (capacity - 1):
        raise ValueError("build_hash_table: capacity %d is not a power of two" % capacity)
    if len(entries) >= capacity:
        raise ValueError("build_hash_table: %d entries do not fit %d slots (one stays empty)" % (len(entries), capacity))
    slots = np.zeros((capacity, 4), dtype=np.uint32)
    slots[:, 1] = 0xFFFFFFFF
    used, keys = [False] * capacity, set()
    for cps, idx, off in entries:
        cps = tuple(cps)
        if not cps or cps in keys:
            raise ValueError("build_hash_table: empty or repeated key %r" % (cps,))
        if not 0 <= idx < (1 << 31):
            raise ValueError("build_hash_table: id %d outside int32" % idx)
        keys.add(cps)
        h = piece_hash(cps)
        i = (h ^ (h >> 32)) & (capacity - 1)
        for _ in range(capacity):
            if not used[i]:
                break
            i = (i + 1) & (capacity - 1)
        else:
            raise ValueError("build_hash_table: no free slot for %r" % (cps,))
        used[i] = True
        slots[i] = (h >> 32, idx, off, len(cps))
    return slots


def host_tables(tokenizer, capacity=None):
    """the tables of xggm_tokenize_wordpiece for a ``BertTokenizer`` as numpy arrays under the kernel's names, built from
    ``tokenizer.vocab`` (the dict: duplicate and blank lines of the file resolve as they do on the host)."""
    basic = tokenizer.basic_tokenizer
    if not basic.do_lower_case:
        raise ValueError("DeviceTokenizer: only do_lower_case=True is implemented on the device")
    wp = tokenizer.wordpiece_tokenizer
    if wp.max_input_chars_per_word != MAX_WORD or wp.vocab is not tokenizer.vocab:
        raise ValueError("DeviceTokenizer: max_input_chars_per_word must be %d and the WordPiece vocabulary the tokenizer's" % MAX_WORD)
    vocab = tokenizer.vocab
    for t in ("[CLS]", "[SEP]", wp.unk_token):
        if t not in vocab:
            raise ValueError("DeviceTokenizer: the vocabulary lacks %s" % t)
    never = list(basic.never_split)
    if len(never) > MAX_NEVER or any(not t for t in never):
        raise ValueError("DeviceTokenizer: at most %d non-empty never_split tokens, got %r" % (MAX_NEVER, never))
    blob, init, cont = [], [], []
    for tok, idx in vocab.items():
        cps = [ord(c) for c in tok]
        if not cps:
            continue
        init.append((cps, idx, len(blob)))
        if tok.startswith("##") and len(cps) > 2:
            cont.append((cps[2:], idx, len(blob) + 2))
        blob.extend(cps)
    table, ext = code_point_table()
    never_off = np.zeros(len(never) + 1, dtype=np.int32)
    never_off[1:] = np.cumsum([len(t) for t in never])
    return dict(cp_table=table, cp_ext=ext if len(ext) else np.zeros(1, dtype=np.uint32),
                init_slots=build_hash_table(init, capacity), cont_slots=build_hash_table(cont, capacity),
                blob=np.asarray(blob if blob else [0], dtype=np.uint32),
                never_cps=np.asarray([ord(c) for t in never for c in t] or [0], dtype=np.uint32), never_off=never_off,
                cls_id=int(vocab["[CLS]"]), sep_id=int(vocab["[SEP]"]), unk_id=int(vocab[wp.unk_token]),
                n_ext=len(ext), n_blob=len(blob), never_end=int(never_off[-1]), vocab_size=max(vocab.values()) + 1)


def decode_utf8(b, p, end):
    """strict UTF-8 at b[p] inside [p, end) -> (code point, bytes consumed); consumed 0: malformed or cut off"""
    b0 = b[p]
    if b0 < 0x80:
        return b0, 1
    lo, hi = 0x80, 0xBF
    if 0xC2 <= b0 <= 0xDF:
        need, cp = 1, b0 & 0x1F
    elif 0xE0 <= b0 <= 0xEF:
        need, cp = 2, b0 & 0x0F
        lo = 0xA0 if b0 == 0xE0 else lo
        hi = 0x9F if b0 == 0xED else hi
    elif 0xF0 <= b0 <= 0xF4:
        need, cp = 3, b0 & 0x07
        lo = 0x90 if b0 == 0xF0 else lo
        hi = 0x8F if b0 == 0xF4 else hi
    else:
        return 0, 0
    if p + need >= end:
        return 0, 0
    for i in range(1, need + 1):
        c = b[p + i]
        if c < lo or c > hi:
            return 0, 0
        lo, hi = 0x80, 0xBF
        cp = (cp << 6) | (c & 0x3F)
    return cp, need + 1


class Restatement:
    """the kernel of csrc/tokenize.hip step by step in Python, reading the SAME tables (``host_tables``) with the same
    table lookups, rolling hash and probing.  ``row(data, T)`` -> (token ids with [CLS] / [SEP], not padded; flag)."""

    def __init__(self, tables):
        self.t = tables
        self.trace = None  # a list: ``wordpiece`` appends every word it is handed (the stream ``BasicTokenizer`` produces)
        self.cp_table, self.cp_ext = tables["cp_table"].tolist(), tables["cp_ext"].tolist()
        self.slots = {False: tables["init_slots"].tolist(), True: tables["cont_slots"].tolist()}
        self.blob = tables["blob"].tolist()
        self.n_blob = tables["n_blob"]
        off, cps = tables["never_off"].tolist(), tables["never_cps"].tolist()
        self.never = [cps[off[k]:off[k + 1]] for k in range(len(off) - 1)]

    def lookup(self, cont, h, w, s, e):
        slots = self.slots[cont]
        cap = len(slots)
        tag, n = h >> 32, e - s
        i = (h ^ (h >> 32)) & (cap - 1)
        for _ in range(cap):
            key, idx, off, length = slots[i]
            if idx == 0xFFFFFFFF:
                return -1
            if key == tag and length == n and off + n <= self.n_blob and self.blob[off:off + n] == w[s:e]:
                return idx
            i = (i + 1) & (cap - 1)
        return -1

    def wordpiece(self, w, n, out, L):
        """``w``: the stored code points (at most MAX_WORD), ``n``: the word's length"""
        if n == 0 or len(out) >= L:
            return
        if self.trace is not None:
            self.trace.append("".join(map(chr, w)))
        if n > MAX_WORD:
            out.append(self.t["unk_id"])
            return
        s, pieces = 0, []
        while s < n:
            h = piece_hash(w[s:n])
            e, idx = n, -1
            while e > s:
                idx = self.lookup(s > 0, h, w, s, e)
                if idx >= 0:
                    break
                h = ((h - (w[e - 1] + 1)) * HASH_MUL_INV) & _M64
                e -= 1
            if idx < 0:
                out.append(self.t["unk_id"])
                return
            pieces.append(idx)
            s = e
        out.extend(pieces[:L - len(out)])

    def row(self, data, T):
        tab, L = self.cp_table, T - 2
        p, end, out, host, fresh = 0, len(data), [], 0, True
        w, n = [], 0

        def flush():
            nonlocal w, n
            self.wordpiece(w, n, out, L)
            w, n = [], 0

        while p < end and len(out) < L:
            cp, nb = decode_utf8(data, p, end)
            if nb == 0:
                host = 1
                p += 1
                continue
            ent = tab[cp]
            act = ent & 7
            if act == ACT_HOST:
                host, act = 1, ACT_KEEP
            if act == ACT_DROP:
                p += nb
                continue
            if act == ACT_SPACE:
                flush()
                fresh = True
                p += nb
                continue
            if act == ACT_KEEP and fresh and self.never:
                alive = [k for k, t in enumerate(self.never) if t[0] == cp]
                if alive:
                    q, j = p + nb, 1
                    while alive and q < end:
                        c2, nb2 = decode_utf8(data, q, end)
                        if nb2 == 0:
                            host = 1
                            q += 1
                            continue
                        act2 = tab[c2] & 7
                        if act2 == ACT_DROP:
                            q += nb2
                            continue
                        if act2 in (ACT_SPACE, ACT_CJK):
                            break
                        alive = [k for k in alive if j < len(self.never[k]) and self.never[k][j] == c2]
                        j += 1
                        q += nb2
                    hit = [k for k in alive if len(self.never[k]) == j]
                    if hit:
                        w, n = list(self.never[hit[-1]][:MAX_WORD]), j
                        flush()
                        p = q
                        continue
            if act == ACT_CJK:
                flush()
            nf, payload = (ent >> 3) & 3, ent >> 8
            for f in range(nf):
                c = payload if nf == 1 else self.cp_ext[payload + f]
                if ent >> (5 + f) & 1:
                    flush()
                    w, n = [c], 1
                    flush()
                else:
                    if n < MAX_WORD:
                        w.append(c)
                    n += 1
            fresh = act == ACT_CJK
            if act == ACT_CJK:
                flush()
            p += nb
        flush()
        return [self.t["cls_id"]] + out + [self.t["sep_id"]], host


def pack_sentences(sents):
    """-> (the sentences' UTF-8 as one uint8 array, int64 offsets [n + 1], the rows strict UTF-8 cannot encode -- lone
    surrogates --, which are packed empty and belong to the host).  ``str.strip()`` is not applied: what it removes is
    whitespace to the kernel as well."""
    n = len(sents)
    lens = np.zeros(n + 1, dtype=np.int64)
    joined = "".join(sents)
    host_rows = []
    if joined.isascii():
        data = joined.encode("ascii")
        lens[1:] = np.fromiter(map(len, sents), dtype=np.int64, count=n)
    else:
        enc = []
        for i, s in enumerate(sents):
            try:
                enc.append(s.encode("utf-8"))
            except UnicodeEncodeError:
                enc.append(b"")
                host_rows.append(i)
        data = b"".join(enc)
        lens[1:] = np.fromiter(map(len, enc), dtype=np.int64, count=n)
    return np.frombuffer(data, dtype=np.uint8), np.cumsum(lens), host_rows


class DeviceTokenizer(object):
    """a ``BertTokenizer`` whose batch conversions run on the device: ``encode`` / ``features`` pack the sentences, copy them
    once, tokenise all of them in ONE launch (``ops.tokenize_wordpiece``) and read back only the number of rows the kernel
    handed to the host -- rows with a ``HOST`` code point (``needs_host``) -- which are re-tokenised by the wrapped
    tokenizer and patched in.  ``tokenize`` / ``convert_tokens_to_ids`` / ``vocab`` are the wrapped tokenizer's, so the
    object can stand wherever a tokenizer is expected."""

    def __init__(self, tokenizer, device):
        import torch
        self.tokenizer, self.device = tokenizer, torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DeviceTokenizer: %s is no GPU (no CPU fallback)" % (device,))
        self.vocab, self.ids_to_tokens = tokenizer.vocab, tokenizer.ids_to_tokens
        self.host = host_tables(tokenizer)
        self.tables = {k: (torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).to(self.device)
                           if isinstance(v, np.ndarray) else v) for k, v in self.host.items()}
        self.last_host_rows = 0

    def tokenize(self, text):
        return self.tokenizer.tokenize(text)

    def convert_tokens_to_ids(self, tokens):
        return self.tokenizer.convert_tokens_to_ids(tokens)

    def convert_ids_to_tokens(self, ids):
        return self.tokenizer.convert_ids_to_tokens(ids)

    def host_ids(self, sent, T):
        return self.tokenizer.convert_tokens_to_ids(["[CLS]"] + self.tokenizer.tokenize(sent.strip())[:T - 2] + ["[SEP]"])

    def _run(self, sents, T, block):
        import torch
        from .. import ops
        sents, T = list(sents), int(T)
        n = len(sents)
        if n < 1 or T < 2:
            raise ValueError("DeviceTokenizer: %d sentences, max_seq_length %d" % (n, T))
        data, offsets, host_rows = pack_sentences(sents)
        buf = np.empty(8 * (n + 1) + len(data), dtype=np.uint8)  # offsets, then bytes: ONE host-to-device copy
        buf[:8 * (n + 1)] = offsets.view(np.uint8)
        buf[8 * (n + 1):] = data
        dev = torch.from_numpy(buf).to(self.device)
        out = ops.tokenize_wordpiece(dev[8 * (n + 1):], dev[:8 * (n + 1)].view(torch.int64), offsets, T, self.tables,
                                     outputs=("block", "flags", "flagged") if block else ("ids", "len", "flags", "flagged"))
        if int(out["flagged"].item()):  # the one read-back of the common case
            host_rows = sorted(set(host_rows) | set(torch.nonzero(out["flags"]).view(-1).tolist()))
        self.last_host_rows = len(host_rows)
        if host_rows:
            rows = np.zeros((len(host_rows), T), dtype=np.int64)
            lens = np.zeros(len(host_rows), dtype=np.int64)
            for k, i in enumerate(host_rows):
                ids = self.host_ids(sents[i], T)
                rows[k, :len(ids)], lens[k] = ids, len(ids)
            at = torch.tensor(host_rows, dtype=torch.int64, device=self.device)
            rows_d, lens_d = torch.from_numpy(rows).to(self.device), torch.from_numpy(lens).to(self.device)
            if block:
                out["block"][0].index_copy_(0, at, rows_d)
                out["block"][1].index_copy_(0, at, (torch.arange(T, device=self.device)[None, :] < lens_d[:, None]).long())
            else:
                out["ids"].index_copy_(0, at, rows_d.int())
                out["len"].index_copy_(0, at, lens_d.int())
        return out

    def encode(self, sents, max_seq_length):
        """-> (ids int32 [n, T], len int32 [n]) on the device: [CLS] tokens[:T - 2] [SEP], zero padded -- the q_ids / q_len
        layout of the resident stores"""
        out = self._run(sents, max_seq_length, False)
        return out["ids"], out["len"]

    def features(self, sents, max_seq_length):
        """-> (input_ids, input_mask, segment_ids) int64 [n, T] on the device: what ``SentenceBatcher.__call__`` returns"""
        b = self._run(sents, max_seq_length, True)["block"]
        return b[0], b[1], b[2]
