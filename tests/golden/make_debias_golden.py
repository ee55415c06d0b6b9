"""Generate tests/golden/debias.npz by running the REFERENCE's debias losses (src/module/vqa_debias_loss_functions.py) in
float64 on the CPU.
    python tests/golden/make_debias_golden.py <path to the reference's src directory>
The reference file is loaded by path, never copied.  Inputs come from ``xggm_amd.synth.debias_case`` (seeded, not
stored); the file holds, per case: the loss, the gradients of bias_lin.weight / bias_lin.bias / smooth_param, d_hidden and
d_logit (whole for the small cases; every 97th element plus per-row sums and abs-sums for the big ones).

For the two scalar gradients (bias_lin.bias, smooth_param) -- cancelling sums over all B x A elements -- the file also holds
the sum of the ABSOLUTE values of their per-element terms, the scale a summation error is measured against.  Those terms
come from the closed form (the docstring of ``terms``); the script asserts that the closed form's sums equal the
reference's autograd gradients to 1e-9 before it writes anything, so the closed form is checked against the reference too.

``<case>.bf16`` entries: hidden and bias_lin are rounded to bfloat16 before the reference sees them (what a bf16 model
hands the loss)."""
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

# name -> (kind, B, A, Hd, constructor kwargs, bias_max, seed, also in bf16, d_logit stored whole)
CASES = {
    "a": ("LearnedMixin", 3, 3129, 768, dict(w=0.36), None, 11, True, False),
    "b": ("LearnedMixin", 1, 1, 1024, dict(w=0.36), None, 12, False, True),
    "c": ("LearnedMixin", 5, 1842, 768, dict(w=0.36, smooth=False, constant_smooth=0.1), None, 13, True, True),
    "d": ("LearnedMixin", 33, 3129, 768, dict(w=0.36), None, 14, True, False),
    "e": ("BiasProduct", 3, 3129, 0, dict(), None, 15, False, True),
    "f": ("BiasProduct", 2, 5, 0, dict(smooth=False, constant_smooth=0.05), None, 16, False, True),
    "g": ("ReweightByInvBias", 3, 3129, 0, dict(), 0.99, 17, False, True),
    "h": ("ReweightByInvBias", 2, 7, 0, dict(), 0.99, 18, False, True),
}
STRIDE = 97


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


def bf16_round(x):
    return torch.from_numpy(x).to(torch.bfloat16).float().numpy()


def terms(kind, kw, x, sp):
    """closed form in float64: per-element terms of d bias_lin.bias and d smooth_param.
    p = log(b + s), q = log(1 - b + s), e = g (p - q), d = z + e, te = dL/de = (sigmoid(d) - y) / B - w e sigmoid(e)
    sigmoid(-e) / (B A);  d bias_lin.bias = sum te (p - q) sigmoid(pre_r);  d smooth_param = sum te g (1 / (b + s) - 1 / (1 -
    b + s)) sigmoid'(smooth_param)"""
    z, y, b = (torch.from_numpy(x[k]).double() for k in ("logits", "labels", "bias"))
    B, A = z.shape
    s = float(kw.get("constant_smooth", 0.0))
    sg = None
    if sp is not None:
        sg = torch.sigmoid(torch.tensor(float(sp), dtype=torch.float64))
        s = s + sg
    if kind == "LearnedMixin":
        pre = torch.from_numpy(x["hidden"]).double() @ torch.from_numpy(x["lin_w"]).double().t() + float(x["lin_b"][0])
        g, w = torch.nn.functional.softplus(pre), float(kw["w"])
    else:
        pre, g, w = None, torch.ones(B, 1, dtype=torch.float64), 0.0
    p, q = torch.log(b + s), torch.log(1 - b + s)
    e = g * (p - q)
    te = (torch.sigmoid(z + e) - y) / B - w * e * torch.sigmoid(e) * torch.sigmoid(-e) / (B * A)
    t_b = te * (p - q) * torch.sigmoid(pre) if pre is not None else None
    t_s = te * g * (1 / (b + s) - 1 / (1 - b + s)) * sg * (1 - sg) if sg is not None else None
    return t_b, t_s


def run_case(ref, name, bf16):
    kind, B, A, Hd, kw, bias_max, seed, _, whole = CASES[name]
    x = synth.debias_case(B, A, Hd, seed, bias_max)
    if bf16:
        for k in ("hidden", "lin_w", "lin_b"):
            x[k] = bf16_round(x[k])
    loss_mod = getattr(ref, kind)(**kw).double()
    if Hd:
        assert loss_mod.bias_lin.in_features == 1024  # the reference's hard-coded width
        loss_mod.bias_lin = torch.nn.Linear(Hd, 1).double()
        with torch.no_grad():
            loss_mod.bias_lin.weight.copy_(torch.from_numpy(x["lin_w"]).double())
            loss_mod.bias_lin.bias.copy_(torch.from_numpy(x["lin_b"]).double())
    logits = torch.from_numpy(x["logits"]).double().requires_grad_(True)
    hidden = torch.from_numpy(x["hidden"]).double().requires_grad_(True) if Hd else None
    loss = loss_mod(hidden, logits, torch.from_numpy(x["bias"]).double(), torch.from_numpy(x["labels"]).double())
    assert torch.isfinite(loss)
    loss.backward()
    tag = name + (".bf16" if bf16 else "")
    out = {tag + ".loss": np.float64(loss.item())}
    dl = logits.grad
    if whole:
        out[tag + ".d_logit"] = dl.numpy().astype(np.float32)
    else:
        out[tag + ".d_logit_every97"] = dl.reshape(-1)[::STRIDE].numpy().astype(np.float32)
        out[tag + ".d_logit_rowsum"] = dl.sum(1).numpy()
        out[tag + ".d_logit_rowabs"] = dl.abs().sum(1).numpy()
    sp = getattr(loss_mod, "smooth_param", None)
    if kind != "ReweightByInvBias":
        t_b, t_s = terms(kind, kw, x, None if sp is None else sp.item())
    else:
        t_b = t_s = None
    if Hd:
        out[tag + ".d_hidden"] = hidden.grad.numpy().astype(np.float32)
        out[tag + ".d_lin_w"] = loss_mod.bias_lin.weight.grad.numpy().astype(np.float32)
        out[tag + ".d_lin_b"] = loss_mod.bias_lin.bias.grad.numpy()
        out[tag + ".d_lin_b_abs"] = np.float64(t_b.abs().sum().item())
        assert abs(t_b.sum().item() - loss_mod.bias_lin.bias.grad.item()) <= 1e-9 * out[tag + ".d_lin_b_abs"], tag
    if sp is not None:
        out[tag + ".d_smooth"] = sp.grad.numpy()
        out[tag + ".d_smooth_abs"] = np.float64(t_s.abs().sum().item())
        assert abs(t_s.sum().item() - sp.grad.item()) <= 1e-9 * out[tag + ".d_smooth_abs"], tag
    return out


def contract(ref):
    """class names, constructor defaults, to_json() and state_dict keys of the reference's classes"""
    out = {}
    for cls, args in (("Plain", ()), ("ReweightByInvBias", ()), ("BiasProduct", ()), ("LearnedMixin", (0.36,))):
        c = getattr(ref, cls)
        m = c(*args)
        sig = inspect.signature(c.__init__) if "__init__" in c.__dict__ else None
        try:
            js = list(m.to_json().items())
        except (NotImplementedError, ValueError):
            # classes without an __init__ of their own: the reference inspects nn.Module.__init__, whose signature is
            # annotated (*args, **kwargs) on current PyTorch, which getargspec refuses (it was (self) when the reference
            # was written): name only
            assert sig is None
            js = [["name", cls]]
        out[cls] = dict(defaults=[] if sig is None else [[k, p.default] for k, p in sig.parameters.items()
                                                         if k != "self" and p.default is not p.empty],
                        positional=[] if sig is None else [k for k, p in sig.parameters.items()
                                                           if k != "self" and p.default is p.empty],
                        to_json=[list(kv) for kv in js], state_dict=list(m.state_dict().keys()),
                        base=[b.__name__ for b in c.__mro__[1:2]])
    return out


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = load_reference(sys.argv[1])
    data = {}
    for name, spec in CASES.items():
        data.update(run_case(ref, name, False))
        if spec[7]:
            data.update(run_case(ref, name, True))
    meta = dict(cases={k: dict(kind=v[0], B=v[1], A=v[2], Hd=v[3], kwargs=v[4], bias_max=v[5], seed=v[6], bf16=v[7], whole=v[8])
                       for k, v in CASES.items()}, stride=STRIDE, contract=contract(ref))
    data["meta_json"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "debias.npz")
    np.savez_compressed(path, **data)
    print("wrote %s: %d arrays, %d bytes" % (path, len(data), os.path.getsize(path)))


if __name__ == "__main__":
    main()
