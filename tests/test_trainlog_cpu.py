"""Host side of the device-resident training log (xggm_train_log_append, engine.TrainLog): the boundary, the refusals
that happen before any launch, and the pure helpers.  No kernel runs here."""
import ctypes
import re

import pytest
import torch


def test_entry_point_is_exported_declared_and_cited():
    from xggm_amd import _lib
    assert "xggm_train_log_append" in _lib.parse_header()
    assert len(_lib.parse_header()["xggm_train_log_append"]) == 7
    assert hasattr(_lib.lib, "xggm_train_log_append")
    src = open(_lib.HEADER_PATH).read()
    # the comment in front of the declaration names the reference lines the log replaces
    m = re.search(r"/\* ---- training log.*?\*/(?=\s*#define XGGM_TRAINLOG_COLS)", src, flags=re.S)
    assert m is not None
    for cite in ("src/vqa/vqacpv2.py:179", "src/vqa/vqacpv2.py:256-270"):
        assert cite in m.group(0), cite
    assert re.search(r"#define XGGM_TRAINLOG_COLS\s+8\b", src) and re.search(r"#define XGGM_TRAINLOG_KINDS\s+4\b", src)


def test_ctypes_struct_matches_the_header_field_by_field():
    from xggm_amd import _lib, ops, trainlog
    src = open(_lib.HEADER_PATH).read()
    m = re.search(r"typedef struct xggm_train_log \{(.*?)\} xggm_train_log;", src, flags=re.S)
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    decls = [f.split() for f in body.split(";") if f.strip()]
    fields = [d[-1].lstrip("*") for d in decls]
    assert fields == [n for n, _ in ops.TrainLogDesc._fields_]
    assert fields == ["values", "steps", "kinds", "cursor", "sums", "counts", "first_bad", "capacity"]
    for d, (name, ct) in zip(decls, ops.TrainLogDesc._fields_):
        is_ptr = "*" in "".join(d)
        assert ct is (ctypes.c_void_p if is_ptr else ctypes.c_int64), name
        if not is_ptr:
            assert d[0] == "int64_t", name
    assert ctypes.sizeof(ops.TrainLogDesc) == 64
    assert (ops.TRAINLOG_COLS, ops.TRAINLOG_KINDS) == (8, 4) == (trainlog.COLS, trainlog.KINDS)


def test_bad_arguments_are_refused_before_any_launch():
    """an error code and a message, and nothing is enqueued (the pointers below are never dereferenced: no GPU is needed
    to be refused)"""
    from xggm_amd import _lib, ops
    L = _lib.lib
    fake = 0x1000  # aligned, never touched
    d = ops.TrainLogDesc(fake, fake, fake, fake, fake, fake, fake, 4)
    src = (ctypes.c_void_p * 9)(*([fake] * 9))
    S = ctypes.cast(src, ctypes.c_void_p)

    def refused(*args):
        rc = L.xggm_train_log_append(*args)
        assert rc != 0 and b"xggm_train_log_append" in L.xggm_last_error(), args
        return L.xggm_last_error()

    D = ctypes.addressof(d)
    assert b"n = 0" in refused(S, None, 0, 0, None, D, None)
    assert b"n = 9" in refused(S, None, 9, 0, None, D, None)
    assert b"kind = -1" in refused(S, None, 3, -1, None, D, None)
    assert b"kind = 4" in refused(S, None, 3, 4, None, D, None)
    refused(None, None, 3, 0, None, D, None)
    refused(S, None, 3, 0, None, None, None)
    e = ops.TrainLogDesc.from_buffer_copy(d)
    e.capacity = 0
    assert b"capacity = 0" in refused(S, None, 3, 0, None, ctypes.addressof(e), None)
    for field in ("cursor", "values", "sums", "kinds", "counts", "first_bad"):
        e = ops.TrainLogDesc.from_buffer_copy(d)
        setattr(e, field, None)
        assert field.encode() in refused(S, None, 3, 0, None, ctypes.addressof(e), None)
    e = ops.TrainLogDesc.from_buffer_copy(d)
    e.sums = fake + 4
    assert b"aligned" in refused(S, None, 3, 0, None, ctypes.addressof(e), None)
    e = ops.TrainLogDesc.from_buffer_copy(d)
    e.values = fake + 2
    assert b"aligned" in refused(S, None, 3, 0, None, ctypes.addressof(e), None)
    assert b"aligned" in refused(S, None, 3, 0, fake + 4, D, None)  # the step counter


def test_wrapper_rejects_cpu_tensors_wide_columns_and_too_many():
    from xggm_amd import ops
    from xggm_amd.engine import TrainLog

    class Log:  # never reached: the columns are checked first
        capacity = 4

    one = torch.zeros(())
    with pytest.raises(RuntimeError, match="GPU"):
        ops.train_log_append(Log, 0, [one])
    with pytest.raises(RuntimeError, match="GPU"):
        ops.train_log_append(Log, 0, [None, torch.zeros(1)])
    with pytest.raises(ValueError, match="column 1 .*ONE fp32 value"):
        ops.train_log_append(Log, 0, [None, torch.zeros(2)])
    with pytest.raises(ValueError, match="ONE fp32 value"):
        ops.train_log_append(Log, 0, [torch.zeros((), dtype=torch.float64)])
    with pytest.raises(ValueError, match="9 columns"):
        ops.train_log_append(Log, 0, [one] * 9)
    with pytest.raises(ValueError, match="0 columns"):
        ops.train_log_append(Log, 0, [])
    with pytest.raises(ValueError, match="factors"):
        ops.train_log_append(Log, 0, [one, one], mul=[1.0])
    with pytest.raises(RuntimeError, match="GPU"):
        TrainLog(4, "cpu")
    with pytest.raises(ValueError, match="capacity"):
        TrainLog(0, "cuda")
    assert (TrainLog.LOSS, TrainLog.BCE, TrainLog.KL, TrainLog.DSM, TrainLog.GRAD_NORM, TrainLog.LR_SCALE) == tuple(range(6))
    assert (TrainLog.PLAIN, TrainLog.REL, TrainLog.NODE) == (0, 1, 2)


def test_unroll_of_the_ring():
    from xggm_amd.trainlog import unroll
    assert unroll(0, 4) == []
    assert unroll(3, 4) == [0, 1, 2]
    assert unroll(4, 4) == [0, 1, 2, 3]
    assert unroll(11, 4) == [3, 0, 1, 2]
    assert unroll(5, 1) == [0]
    with pytest.raises(ValueError):
        unroll(1, 0)


def test_decode_of_a_read_back_log():
    """the int64 words of ``TrainLog.read``'s one transfer: a ring of 3 that has wrapped once (5 records)"""
    from xggm_amd import trainlog as T
    cap = 3
    w = torch.zeros(T.words(cap), dtype=torch.int64)
    assert T.words(cap) == T.HEADER + cap + cap * 4 + 2 and T.HEADER == 38
    w[0], w[1] = 5, -1
    w[2:6] = torch.tensor([2, 2, 1, 0])
    w[6:38].view(torch.float64).view(4, 8)[1, 2] = 0.5
    steps = w[38:41]
    values = w[41:53].view(torch.float32).view(cap, 8)
    kinds = w[53:].view(torch.int32)[:cap]
    for r in range(5):  # record r: kind r % 3, columns 0 and r % 8 present
        row = r % cap
        steps[row] = 100 + r
        values[row] = 0
        values[row, 0], values[row, r] = float(r), -float(r)
        kinds[row] = (r % 3) | (((1 << 0) | (1 << r)) << 8)
    rec = T.decode_packed(w, cap)
    assert int(rec["cursor"]) == 5 and int(rec["first_bad"]) == -1
    assert rec["steps"].tolist() == [102, 103, 104] and rec["kinds"].tolist() == [2, 0, 1]
    assert rec["values"][:, 0].tolist() == [2.0, 3.0, 4.0] and rec["values"].dtype == torch.float32
    assert rec["present"].dtype == torch.bool and rec["present"].shape == (3, 8)
    assert [row.nonzero().flatten().tolist() for row in rec["present"]] == [[0, 2], [0, 3], [0, 4]]
    assert rec["counts"].tolist() == [2, 2, 1, 0] and float(rec["sums"][1, 2]) == 0.5 and rec["sums"].dtype == torch.float64
    w[0] = 2  # not wrapped yet: rows 0 and 1
    assert T.decode_packed(w, cap)["values"].shape == (2, 8)
    w[0] = 0
    empty = T.decode_packed(w, cap)
    assert empty["values"].shape == (0, 8) and empty["present"].shape == (0, 8) and empty["steps"].shape == (0,)
