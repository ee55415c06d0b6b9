"""Generate tests/golden/softmax_loss.npz: the REFERENCE's ``Focal`` (src/module/vqa_debias_loss_functions.py:74-81) and
``torch.nn.CrossEntropyLoss(ignore_index=-1)`` (what src/gqa/gqa_ood.py:116 constructs for --mceLoss) in float64 on the CPU.
    python tests/golden/make_softmax_loss_golden.py <path to the reference's src directory>
The reference file is loaded by path, never copied.  Inputs come from ``xggm_amd.synth.debias_case`` (seeded, not stored).
Cross-entropy's class of a row is the first index of the maximum of its soft scores, or -1 (ignored) when that maximum is
<= 0.  Per case and kind the file holds the loss, d_logit and, for cross-entropy, the labels.  Every d_logit is stored
WHOLE -- the largest has 9387 elements.  (The every-97th-element sample with per-row sums that debias.npz keeps for its
big cases does not carry over to Focal: a row that holds a +-30 logit has a gradient that is the cancelling remainder of
terms a thousand times larger, and on a sample that misses the few large entries, or on a row sum over the row's abs-sum,
the reference's own float32 run misses the gate below at nearly every seed -- 35 of 36 tried at (5, 1842), 6 of 7 at
(3, 3129) -- while it passes on the whole gradient.  A measure the reference's float32 run cannot pass measures nothing.)

A gate on the INPUTS: for every stored case the reference's own float32 run has to agree with its float64 run within
GATE = 1e-5 -- half of the project's fp32 bar (tests/test_kernels_gpu.py: tol(F32) = 2e-5) -- on the relative loss error and
on rel_err(d_logit).  Focal's +1e-5 floor kills the gradient of a row that holds a +-30 logit; such a case would measure
nothing.  A seed that fails the gate is replaced by another seed, the bar is never widened.  Both figures of every case are
recorded in ``meta_json``."""
import importlib.util
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from xggm_amd import synth  # noqa: E402

GATE = 1e-5
IGNORE = -1
# name -> (kinds, B, A, seed, variant)
#   variant "all_ignored": every soft score set to 0, so cross-entropy ignores every row
#   variant "label_index": the classes are handed over as int64 [B], entry 1 set to ignore_index (stored as <name>.label_index)
CASES = {
    "a": (("focal", "ce"), 1, 1, 21, None),
    "b": (("focal", "ce"), 2, 5, 21, None),
    "c": (("focal", "ce"), 3, 263, 22, None),
    "d": (("focal", "ce"), 3, 3129, 21, None),
    "e": (("focal", "ce"), 5, 1842, 21, None),
    "f": (("focal", "ce"), 2, 4097, 21, None),
    "g": (("focal", "ce"), 130, 64, 21, None),
    "h": (("ce",), 2, 7, 21, "all_ignored"),
    "i": (("ce",), 3, 3129, 21, "label_index"),
}


def load_reference(src):
    if not hasattr(inspect, "getargspec"):  # the reference's to_json uses the pre-3.11 name
        def getargspec(f):
            s = inspect.getfullargspec(f)
            return type("ArgSpec", (), dict(args=s.args, varargs=s.varargs, keywords=s.varkw, defaults=s.defaults))
        inspect.getargspec = getargspec
    spec = importlib.util.spec_from_file_location("ref_debias", os.path.join(src, "module", "vqa_debias_loss_functions.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def case_inputs(name):
    """float32 numpy inputs of a case: logits, labels, bias and the cross-entropy classes (int64; -1: ignored)"""
    _, B, A, seed, variant = CASES[name]
    x = synth.debias_case(B, A, 0, seed)
    if variant == "all_ignored":
        x["labels"] = np.zeros_like(x["labels"])
    y = torch.from_numpy(x["labels"])
    mx, arg = y.max(1)
    assert np.array_equal(arg.numpy(), x["labels"].argmax(1))  # torch's tie rule: the first index of the maximum
    cls = torch.where(mx > 0, arg, torch.full_like(arg, IGNORE))
    if variant == "label_index":
        cls[1] = IGNORE
    x["classes"] = cls.numpy().astype(np.int64)
    return x


def run(ref, kind, x, dt):
    logits = torch.from_numpy(x["logits"]).to(dt).requires_grad_(True)
    if kind == "focal":
        loss = ref.Focal()(None, logits, torch.from_numpy(x["bias"]).to(dt), torch.from_numpy(x["labels"]).to(dt))
    else:
        loss = torch.nn.CrossEntropyLoss(ignore_index=IGNORE)(logits, torch.from_numpy(x["classes"]))
    loss.backward()
    return loss.detach().double(), logits.grad.double()


def rel_err(a, b):
    return float((a - b).norm() / (b.norm() + 1e-30))


def run_case(ref, name):
    kinds, B, A, seed, variant = CASES[name]
    x = case_inputs(name)
    out, gate = {}, {}
    if variant is None and (B, A) == (2, 5):
        assert (x["classes"] == IGNORE).sum() == 1  # one row without a positive score: cross-entropy ignores it
    for kind in kinds:
        loss, dl = run(ref, kind, x, torch.float64)
        loss32, dl32 = run(ref, kind, x, torch.float32)
        tag = "%s.%s" % (name, kind)
        if variant == "all_ignored":
            # what torch does with no valid row is RECORDED, not assumed: today a NaN loss and an all-zero gradient
            assert bool(torch.isnan(loss)) == bool(torch.isnan(loss32)) and torch.equal(dl, dl32)
            g_loss, g_grad = 0.0, 0.0
        else:
            assert torch.isfinite(loss)
            g_loss = abs(float(loss32) - float(loss)) / abs(float(loss)) if float(loss) != 0.0 else abs(float(loss32))
            g_grad = rel_err(dl32, dl)
        assert g_loss <= GATE and g_grad <= GATE, "case %s fails the input gate (%.2e, %.2e): choose another seed" % (tag, g_loss, g_grad)
        gate[kind] = dict(loss=g_loss, d_logit=g_grad)
        out[tag + ".loss"] = np.float64(loss.item())
        out[tag + ".d_logit"] = dl.numpy().astype(np.float32)
        if kind == "ce":
            out[tag + ".labels"] = x["classes"]
            for r in np.nonzero(x["classes"] == IGNORE)[0]:
                assert not dl[r].any()  # ignored rows: an exactly zero gradient
    if variant == "label_index":
        out[name + ".label_index"] = x["classes"]
    return out, gate


def contract(ref):
    """the reference's ``Focal``: base class, constructor, to_json() and state_dict keys"""
    c = ref.Focal
    assert "__init__" not in c.__dict__  # no constructor of its own
    m = c()
    try:
        js = [list(kv) for kv in m.to_json().items()]
    except (NotImplementedError, ValueError):
        # the reference inspects nn.Module.__init__, whose signature is (*args, **kwargs) on current PyTorch, which
        # getargspec refuses (it was (self) when the reference was written): the name only
        js = [["name", "Focal"]]
    return dict(Focal=dict(defaults=[], positional=[], to_json=js, state_dict=list(m.state_dict().keys()),
                           base=[b.__name__ for b in c.__mro__[1:2]]))


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = load_reference(sys.argv[1])
    data, gates = {}, {}
    for name in CASES:
        out, gates[name] = run_case(ref, name)
        data.update(out)
    meta = dict(cases={k: dict(kinds=list(v[0]), B=v[1], A=v[2], seed=v[3], variant=v[4], gate=gates[k])
                       for k, v in CASES.items()},
                gate=GATE, ignore_index=IGNORE, contract=contract(ref))
    data["meta_json"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "softmax_loss.npz")
    np.savez_compressed(path, **data)
    worst = {k: max(g[k] for c in gates.values() for g in c.values()) for k in ("loss", "d_logit")}
    print("wrote %s: %d arrays, %d bytes; float32-vs-float64 of the reference, worst case: loss %.2e, d_logit %.2e (gate %.0e)"
          % (path, len(data), os.path.getsize(path), worst["loss"], worst["d_logit"], GATE))


if __name__ == "__main__":
    main()
