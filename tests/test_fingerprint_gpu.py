"""The fingerprint kernel (xggm_fingerprint_spans) against its numpy restatement, bit for bit, and the single-process
helper ``state_fingerprint`` on the tiny model."""
import numpy as np
import pytest
import torch

from xggm_amd import synth
from helpers import batch_tensors

pytestmark = pytest.mark.gpu
DEV = "cuda"
M64 = 0xFFFFFFFFFFFFFFFF


def _host(t, ranges, salt):
    from xggm_amd.fingerprint import fingerprint
    return fingerprint(t.cpu(), ranges, salt)


def _random(n_bytes, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n_bytes,), generator=g, dtype=torch.uint8)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.uint8])
def test_kernel_equals_the_host_restatement(dt):
    from xggm_amd.fingerprint import fingerprint
    item = torch.empty(0, dtype=dt).element_size()
    raw = _random((64 << 20) + 64, 3)
    t = raw.view(dt).to(DEV)
    el = lambda nbytes: nbytes // item  # noqa: E731
    # 0, 4 bytes, one wave's worth of 16-byte loads minus a word, 1 Mi + 8 elements, 64 Mi bytes
    lengths = [0, 4, 64 * 16 - 4, (1 << 20) * item + 8 * item, 64 << 20]
    for nbytes in lengths:
        for off in (0, 4, 8, 12, 20):  # starts that are 4-byte but not 16-byte aligned, too
            if nbytes == 64 << 20 and off not in (0, 12):
                continue
            r = [(el(off), el(off + nbytes))]
            got = fingerprint(t, r, salt=77)
            assert got.dtype == torch.int64 and got.is_cuda
            assert torch.equal(got.cpu(), _host(raw.view(dt), r, 77)), (dt, nbytes, off)
    # 1, 2 and 28 ranges of mixed sizes in one call, an empty one in the middle
    rng = np.random.default_rng(5)
    for n in (1, 2, 28):
        rs, o = [], 4
        for i in range(n):
            nb = 0 if (n > 1 and i == n // 2) else int(rng.choice([4, 1020, 4096, 65536 + 4, 1 << 20])) + 4 * int(rng.integers(0, 8))
            rs.append((el(o), el(o + nb)))
            o += nb + 4 * int(rng.integers(0, 5))
        got = fingerprint(t, rs, salt=n)
        assert torch.equal(got.cpu(), _host(raw.view(dt), rs, n)), (dt, n)
        if n > 1:
            assert int(got[n // 2]) == 0
    # more ranges than one grid holds
    rs = [(el(8 * i), el(8 * i + 4 * (i % 7))) for i in range(150)]
    assert torch.equal(fingerprint(t, rs, salt=1).cpu(), _host(raw.view(dt), rs, 1))


def test_grid_shape_does_not_enter():
    from xggm_amd.fingerprint import fingerprint
    raw = _random(24 << 20, 9)
    t = raw.view(torch.float32).to(DEV)
    rs = [(1, 1 + (1 << 20) + 3), (2 << 20, 2 << 20), (3 << 20, (3 << 20) + 5), (4 << 20, 6 << 20)]
    want = _host(raw.view(torch.float32), rs, 4)
    for wgs in (1, 7, 0, 4096):
        assert torch.equal(fingerprint(t, rs, 4, max_workgroups=wgs).cpu(), want), wgs


def test_every_single_bit_flip_changes_its_word_and_no_other():
    from xggm_amd.fingerprint import fingerprint
    raw = _random(48 << 20, 21)
    t = raw.to(DEV)
    n = 16 << 20
    rs = [(0, n), (n, 2 * n), (2 * n, 3 * n)]
    base = fingerprint(t, rs, 6).cpu()
    g = torch.Generator().manual_seed(99)
    where = torch.randint(0, n, (64,), generator=g).tolist()
    bits = torch.randint(0, 8, (64,), generator=g).tolist()
    for byte, bit in zip(where, bits):
        t[n + byte] ^= (1 << bit)
        got = fingerprint(t, rs, 6).cpu()
        assert got[1] != base[1] and got[0] == base[0] and got[2] == base[2], (byte, bit)
        t[n + byte] ^= (1 << bit)
    assert torch.equal(fingerprint(t, rs, 6).cpu(), base)


def test_inside_a_captured_graph_and_with_patterned_buffers():
    """no host synchronisation, no allocation, no state besides the arguments: the call replays; and every output word
    is written, no workspace word is read that the call did not write.  The pattern written into the workspace and the
    -1 preset of the output before every replay stand in for a run under XGGM_POISON_EMPTY=1, whose poison only reaches
    floating-point buffers and so could not touch the int64 buffers of this path."""
    from xggm_amd import ops
    from xggm_amd.fingerprint import fingerprint, fingerprint_host, _as_int64
    raw = _random(6 << 20, 31)
    t = raw.view(torch.bfloat16).to(DEV)
    rs = [(0, 1 << 20), (1 << 20, 1 << 20), ((1 << 20) + 2, (3 << 20) - 6)]
    fingerprint(t, rs, 8)  # the eager call that makes the workspace
    for ws in ops._FP_WS.values():
        ws.fill_(0x5A5A5A5A5A5A5A5A)
    spans = [(t.data_ptr() + 2 * s, 2 * (e - s), 8) for s, e in rs]
    out = torch.full((3,), -1, device=DEV, dtype=torch.int64)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.fingerprint_spans(spans, t.device, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), _host(raw.view(torch.bfloat16), rs, 8))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.fingerprint_spans(spans, t.device, out=out)
    for k in range(3):
        t[(k * 7919) % (1 << 20)] = float(k + 1)
        t[(2 << 20) + k] = -float(k + 1)
        out.fill_(-1)
        graph.replay()
        eager = fingerprint(t, rs, 8)
        assert torch.equal(out, eager), k
        host = t.cpu()
        assert [int(x) for x in out.cpu()] == [_as_int64(fingerprint_host(host[s:e], 8)) for s, e in rs]
    assert int(out[1]) == 0
    # a later call with the largest grid the wrapper takes must not replace the workspace the graph captured
    ws0 = ops._FP_WS[t.device].data_ptr()
    assert torch.equal(fingerprint(t, rs, 8, max_workgroups=ops.FP_MAX_WORKGROUPS), eager)
    assert ops._FP_WS[t.device].data_ptr() == ws0
    out.fill_(-1)
    graph.replay()
    assert torch.equal(out, eager)
    with pytest.raises(ValueError):
        fingerprint(t, rs, 8, max_workgroups=ops.FP_MAX_WORKGROUPS + 1)
    # a workspace of the caller's own (calls that may run side by side on two streams)
    mine = ops.fingerprint_workspace(t.device)
    mine.fill_(0x5A5A5A5A5A5A5A5A)
    assert torch.equal(ops.fingerprint_spans(spans, t.device, ws=mine), eager)


def _tiny_trainer(seed_w=5, seed_rt=11):
    from oracle import shapes
    from test_model_gpu import build_model
    from xggm_amd.engine import CapturedTrainer
    from xggm_amd.vqa.vqacpv2 import make_optimizer
    cfg = dict(shapes.TINY, l_layers=2, x_layers=2, r_layers=1)
    m = build_model(cfg, 29, seed=seed_w, dt=torch.bfloat16)
    m.seed = seed_rt
    opt = make_optimizer(m, 1e-4, 40)
    b = batch_tensors(synth.vqa_batch(4, A=29, F=cfg["feat_dim"], vocab=cfg["vocab"], seed=3), DEV)
    return m, opt, CapturedTrainer(m, opt, b, sigma=1.0, warmup_iters=1)


def test_state_fingerprint_of_the_tiny_model(tmp_path):
    from xggm_amd.fingerprint import state_fingerprint
    from xggm_amd.vqa.vqacpv2 import save_training_state, load_training_state
    m1, o1, t1 = _tiny_trainer()
    m2, o2, t2 = _tiny_trainer()
    for br in ("rel", "node", "rel"):
        t1.iteration(br)
        t2.iteration(br)
    f1, f2 = state_fingerprint(m1), state_fingerprint(m2)
    assert f1 == f2 and set(f1) == {"params", "m", "v", "shadow"} and set(f1["params"]) == set(m1.arena().groups)
    assert all(v.startswith("0x") and len(v) == 18 for d in f1.values() for v in d.values())
    assert state_fingerprint(m1, "weights") == {"shadow": f1["shadow"]}
    assert f1["params"]["enc_main"] != f1["m"]["enc_main"]
    t2.iteration("node")
    f2 = state_fingerprint(m2)
    assert f2 != f1 and f2["params"]["enc_main"] != f1["params"]["enc_main"] and f2["shadow"]["logit_fc"] != f1["shadow"]["logit_fc"]
    # a checkpoint of the longer run, loaded into a fresh model, gives the same words
    path = str(tmp_path / "state.pt")
    save_training_state(path, m2, o2)
    m3, o3, _ = _tiny_trainer(seed_w=6, seed_rt=12)
    assert state_fingerprint(m3) != f2
    load_training_state(path, m3, o3)
    assert state_fingerprint(m3) == f2
