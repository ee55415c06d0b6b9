"""Flag namespace with the reference's names and defaults (src/param.py:34-123).  The
reference parses ``sys.argv`` at import time; here ``args`` is a plain namespace that
``parse_args(argv)`` can refresh, so importing the package never touches the command line."""
import argparse


def get_optimizer(optim):
    """the reference's ``--optim`` names (src/param.py:9-31) bound to this package's arena-aware classes of the same
    names (``xggm_amd.optim``: the ``torch.optim`` rules on the fused device update); ``'bert'`` stays the string the
    trainers turn into ``BertAdam`` (src/vqa/vqacpv2.py:113-128)."""
    names = {'rms': 'RMSprop', 'adam': 'Adam', 'adamw': 'AdamW', 'adamax': 'Adamax', 'sgd': 'SGD'}
    if optim in names:
        from . import optim as xo  # (imports the compiled library: only when an optimiser is asked for)
        return getattr(xo, names[optim])
    if 'bert' in optim:
        return 'bert'  # bound later, as in the reference
    assert False, "Please add your optimizer %s in the list." % optim


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--bs", dest="batch_size", type=int, default=8)
    p.add_argument("--optim", default="bert")
    p.add_argument("--lr", type=float, default=1e-5)
    p.add_argument("--epochs", type=int, default=4)
    p.add_argument("--seed", type=int, default=9595)
    p.add_argument("--llayers", type=int, default=9)
    p.add_argument("--xlayers", type=int, default=5)
    p.add_argument("--rlayers", type=int, default=5)
    p.add_argument("--gnn", type=str, default="GCN")
    p.add_argument("--num_layer", type=int, default=2)
    p.add_argument("--sigma", type=float, default=1.0)
    p.add_argument("--delta", type=int, default=5)
    p.add_argument("--fromScratch", dest="from_scratch", action="store_const", default=False, const=True)
    p.add_argument("--multiGPU", action="store_const", default=False, const=True)
    p.add_argument("--mceLoss", dest="mce_loss", action="store_const", default=False, const=True)  # src/param.py:78
    # LXMERT pre-training tasks, src/param.py:91-100 (``pretrain.lxmert_pretrain.LXMERT``)
    p.add_argument("--taskMatched", dest="task_matched", action="store_const", default=False, const=True)
    p.add_argument("--taskMaskLM", dest="task_mask_lm", action="store_const", default=False, const=True)
    p.add_argument("--taskObjPredict", dest="task_obj_predict", action="store_const", default=False, const=True)
    p.add_argument("--taskQA", dest="task_qa", action="store_const", default=False, const=True)
    p.add_argument("--visualLosses", dest="visual_losses", default="obj,attr,feat", type=str)
    p.add_argument("--output", type=str, default="snap/test")
    p.add_argument("--wordMaskRate", dest="word_mask_rate", default=0.15, type=float)  # src/param.py:102-105
    p.add_argument("--objMaskRate", dest="obj_mask_rate", default=0.15, type=float)
    p.add_argument("--vocab", dest="vocab_path", type=str, default=None,
                   help="local BERT vocab.txt (the reference downloads it; offline it must be given)")
    return p


def parse_args(argv=None):
    global args
    args = build_parser().parse_args(argv or [])
    args.optimizer = get_optimizer(args.optim)  # src/param.py:121
    return args


args = parse_args([])
