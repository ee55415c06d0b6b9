"""64-bit fingerprints of ranges of the training state: the summary the replica drift guard (dist.ReplicaGuard)
compares across data-parallel ranks, and a way to compare two runs by eye (``state_fingerprint``).

ONE definition (the contract is the comment of ``xggm_fingerprint_spans`` in include/xggm.h), two implementations:
the HIP kernel for device tensors (``ops.fingerprint_spans``) and ``fingerprint_host`` below, its numpy restatement,
for CPU tensors -- the transport-level tests of the guard run over gloo on CPU tensors, as those of ``dist`` do.  The
host version is not a fallback of the model: a CUDA tensor never goes through it.
"""
import numpy as np
import torch

GOLD = 0x9E3779B9
MIXMUL = 0x7FEB352D
# one salt per buffer of the arena: equal bits in two buffers (all-zero moments, say) still give different words
SALT = {"params": 0x70617261, "m": 0x6D6F6D31, "v": 0x6D6F6D32, "shadow": 0x73686477}
_CHUNK = 1 << 22  # words per numpy step (temporaries of a few tens of MB)


def _words(x):
    """the little-endian 32-bit words of an array / CPU tensor (whole 4-byte words only)"""
    if torch.is_tensor(x):
        if x.is_cuda:
            raise RuntimeError("fingerprint_host takes CPU data; device tensors go through fingerprint() (the HIP kernel)")
        if x.numel() == 0:
            return np.zeros(0, dtype="<u4")
        x = x.detach().contiguous().reshape(-1).view(torch.uint8).numpy()
    b = np.ascontiguousarray(x).reshape(-1).view(np.uint8)
    if b.size % 4:
        raise ValueError("fingerprint: %d bytes is not a whole number of 32-bit words" % b.size)
    return b.view("<u4")


def fingerprint_host(x, salt=0):
    """the fingerprint of the bytes of ``x`` (numpy array or CPU tensor of any dtype) as a Python int in [0, 2^64)"""
    w = _words(x)
    salt = np.uint32(int(salt) & 0xFFFFFFFF)
    acc = np.uint64(0)
    with np.errstate(over="ignore"):
        for a in range(0, w.size, _CHUNK):
            c = w[a:a + _CHUNK]
            # the index mod 2^32: uint32 arithmetic wraps exactly as the contract asks
            i = (np.arange(a, a + c.size, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
            x32 = (c ^ (i * np.uint32(GOLD) + salt)) * np.uint32(MIXMUL)
            x32 ^= x32 >> np.uint32(15)
            odd = (i << np.uint32(1)) | np.uint32(1)  # 2 * (i mod 2^31) + 1
            acc = acc + np.sum(x32.astype(np.uint64) * odd.astype(np.uint64), dtype=np.uint64)
    return int(acc)


def _as_int64(v):
    """a uint64 value as the int64 with the same bits (torch has no usable uint64 collectives)"""
    return v - (1 << 64) if v >= (1 << 63) else v


def fingerprint_table(items, max_workgroups=0):
    """``items``: [(flat tensor, start, end, salt)] element ranges, all tensors on one device -> int64 tensor
    [len(items)] on that device holding the fingerprints' bit patterns.  Device tensors: ONE call of the kernel for the
    whole table."""
    if not items:
        return torch.empty(0, dtype=torch.int64)
    dev = items[0][0].device
    for t, s, e, _ in items:
        if t.device != dev or t.dim() != 1 or not t.is_contiguous() or not 0 <= s <= e <= t.numel():
            raise ValueError("fingerprint: flat contiguous tensors of one device and ranges inside them are required")
        if ((e - s) * t.element_size()) % 4 or (s * t.element_size()) % 4:
            raise ValueError("fingerprint: range [%d, %d) of a %s tensor is not made of whole 32-bit words" % (s, e, t.dtype))
    if dev.type == "cuda":
        from . import ops
        spans = [(t.data_ptr() + s * t.element_size(), (e - s) * t.element_size(), salt) for t, s, e, salt in items]
        return ops.fingerprint_spans(spans, dev, max_workgroups=max_workgroups)
    return torch.tensor([_as_int64(fingerprint_host(t[s:e], salt)) for t, s, e, salt in items], dtype=torch.int64)


def fingerprint(tensor, ranges, salt=0, max_workgroups=0):
    """fingerprints of the element ranges [(start, end)] of a flat tensor (fp32, bf16, uint8 / e4m3 ...; every range a
    whole number of 32-bit words) -> int64 tensor [len(ranges)] on the tensor's device"""
    out = fingerprint_table([(tensor, int(s), int(e), salt) for s, e in ranges], max_workgroups)
    return out.to(tensor.device) if not ranges else out


def hex64(v):
    return "0x%016x" % (int(v) & 0xFFFFFFFFFFFFFFFF)


def state_fingerprint(model, level="state"):
    """{buffer: {arena group: "0x..."}} of ONE process's arena: what a run can print to be compared with another run
    (a resume, a second build, a determinism check) without keeping both states in memory.  ``level``: "weights" = what
    the forward reads (the bf16 shadow, or the fp32 masters in fp32 mode); "state" = fp32 masters, both BertAdam
    moments and the shadow.  Under the sharded update "state" first makes the masters and moments whole
    (ParamArena.gather_sharded_state: a collective there)."""
    from .runtime import runtime_of
    arena = runtime_of(model).arena
    if level not in ("weights", "state"):
        raise ValueError("level must be 'weights' or 'state'")
    if level == "state":
        arena.gather_sharded_state()
    elif arena.zero1 is not None:
        arena.zero1.wait_pending()
    bufs = ["shadow" if arena.shadow is not None else "params"] if level == "weights" else \
        ["params", "m", "v"] + (["shadow"] if arena.shadow is not None else [])
    items = [(getattr(arena, b), G.start, G.end, SALT[b]) for b in bufs for G in arena.groups.values()]
    words = fingerprint_table(items).cpu().tolist()
    names = list(arena.groups)
    return {b: {g: hex64(words[i * len(names) + j]) for j, g in enumerate(names)} for i, b in enumerate(bufs)}
