"""``--optim`` (src/param.py:9-31) without a GPU: the flag, the names, torch's constructor defaults, the refused flags,
the exported symbols and the argument checks that run before any launch."""
import ctypes

import pytest
import torch

from xggm_amd import _lib, optim as xo, param

PAIRS = [("Adam", torch.optim.Adam), ("AdamW", torch.optim.AdamW), ("Adamax", torch.optim.Adamax), ("SGD", torch.optim.SGD),
         ("RMSprop", torch.optim.RMSprop)]


def test_get_optimizer_maps_the_reference_names():
    assert param.get_optimizer("rms") is xo.RMSprop
    assert param.get_optimizer("adam") is xo.Adam
    assert param.get_optimizer("adamw") is xo.AdamW
    assert param.get_optimizer("adamax") is xo.Adamax
    assert param.get_optimizer("sgd") is xo.SGD
    assert param.get_optimizer("bert") == "bert"
    with pytest.raises(AssertionError, match="lion"):
        param.get_optimizer("lion")


def test_optim_flag_binds_args_optimizer():
    assert param.build_parser().parse_args([]).optim == "bert"
    assert param.parse_args([]).optimizer == "bert"
    a = param.parse_args(["--optim", "adamax"])
    assert a.optim == "adamax" and a.optimizer is xo.Adamax
    param.parse_args([])


@pytest.mark.parametrize("name,ref", PAIRS)
def test_constructor_defaults_are_torchs(name, ref):
    w = torch.nn.Parameter(torch.zeros(3))
    ours, theirs = getattr(xo, name)([w]).defaults, ref([w]).defaults
    common = set(ours) & set(theirs)
    assert {"lr", "weight_decay"} <= common and len(common) >= 4
    assert {k: ours[k] for k in common} == {k: theirs[k] for k in common}
    if name == "AdamW":
        assert ours["weight_decay"] == 0.01 and ours["decoupled_weight_decay"] is True


@pytest.mark.parametrize("name,kw", [
    ("Adam", dict(amsgrad=True)), ("Adam", dict(foreach=True)), ("Adam", dict(fused=True)), ("Adam", dict(capturable=True)),
    ("Adam", dict(maximize=True)), ("AdamW", dict(amsgrad=True)), ("AdamW", dict(fused=False)),
    ("Adamax", dict(foreach=False)), ("Adamax", dict(maximize=True)), ("Adamax", dict(capturable=True)),
    ("SGD", dict(maximize=True)), ("SGD", dict(foreach=True)), ("SGD", dict(fused=True)),
    ("RMSprop", dict(centered=True)), ("RMSprop", dict(capturable=True)), ("RMSprop", dict(maximize=True)),
    ("RMSprop", dict(foreach=True))])
def test_refused_flags_raise(name, kw):
    w = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError, match=list(kw)[0]):
        getattr(xo, name)([w], **kw)


def test_invalid_hyper_parameters_raise_as_in_torch():
    w = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError):
        xo.Adam([w], lr=-1.0)
    with pytest.raises(ValueError):
        xo.Adamax([w], betas=(1.0, 0.999))
    with pytest.raises(ValueError):
        xo.SGD([w], nesterov=True)
    with pytest.raises(ValueError):
        xo.RMSprop([w], momentum=-0.1)


def test_library_exports_the_new_symbols():
    decl = _lib.parse_header()
    for name in ("xggm_optim_multi", "xggm_sched_step_ex"):
        assert name in decl and hasattr(_lib.lib, name)
    src = open(_lib.HEADER_PATH).read()
    assert "src/param.py:9-31" in src and "src/vqa/vqacpv2.py:141" in src


def test_struct_mirrors_have_the_c_layout():
    """xggm_optim_args = xggm_adam_args + {int, pointer, 5 doubles, int}; xggm_sched_entry = {2 int, int64, 3 doubles}"""
    from xggm_amd import ops
    assert ctypes.sizeof(ops.SchedEntry) == 40
    assert ctypes.sizeof(ops.OptimArgs) == ctypes.sizeof(ops.AdamArgs) + 64
    assert ops.OptimArgs.rule.offset == ctypes.sizeof(ops.AdamArgs)


def test_null_or_empty_argument_block_is_rejected_before_any_launch():
    from xggm_amd import ops
    lib = _lib.lib
    assert lib.xggm_optim_multi(None, 1, None, None) != 0 and "no spans" in _lib.last_error()
    arr = (ops.OptimArgs * 1)()
    assert lib.xggm_optim_multi(ctypes.cast(arr, ctypes.c_void_p), 0, None, None) != 0
    assert lib.xggm_optim_multi(ctypes.cast(arr, ctypes.c_void_p), 1, None, None) != 0  # null p / g / m / v, n = 0
    assert "bad arguments" in _lib.last_error()
    arr[0].rule = 17
    assert lib.xggm_optim_multi(ctypes.cast(arr, ctypes.c_void_p), 1, None, None) != 0 and "unknown rule" in _lib.last_error()
    ent = (ops.SchedEntry * 1)()
    assert lib.xggm_sched_step_ex(None, None, None, ctypes.cast(ent, ctypes.c_void_p), 1, None) != 0
    assert "bad arguments" in _lib.last_error()


def test_bertadam_accepts_the_reference_schedules():
    from xggm_amd.lxrt.optimization import BertAdam
    w = torch.nn.Parameter(torch.zeros(3))
    for s in ("warmup_cosine", "warmup_constant", "warmup_linear"):
        assert BertAdam([w], lr=1e-3, warmup=0.1, t_total=10, schedule=s).defaults["schedule"] == s


def test_foreign_optimiser_is_named():
    from xggm_amd.lxrt.optimization import require_arena_aware
    w = torch.nn.Parameter(torch.zeros(3))
    require_arena_aware(xo.Adamax([w]))
    with pytest.raises(TypeError, match="xggm_amd.optim"):
        require_arena_aware(torch.optim.Adamax([w]))
