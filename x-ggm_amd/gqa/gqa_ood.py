"""GQA-OOD iteration (src/gqa/gqa_ood.py:165-292): GGM pass first (KL weight 12), plain
pass second.  Thin front-end over xggm_amd.vqa.vqacpv2."""
from ..vqa.vqacpv2 import (loss_func, compute_kl_loss, BCEWithLogitsLoss, plain_pass, ggm_pass, predict, evaluate,  # noqa: F401
                           train_iteration as _train_iteration, make_optimizer, attach_debias_loss,  # noqa: F401
                           answer_prior_table, make_answer_loss, FineTuner, val_schedule)  # noqa: F401


def train_iteration(model, optim, bce_loss, batch, delta=5, sigma=1.0, branch=None, clip=5.0, train_log=None):
    return _train_iteration(model, optim, bce_loss, batch, delta=delta, sigma=sigma, order="gqa", branch=branch,
                            clip=clip, train_log=train_log)


class GQA(FineTuner):
    """``class GQA`` of src/gqa/gqa_ood.py:70-431: GGM pass first, KL weight 12, validation at twice the training batch
    size (:82), ``total_loss`` over the number of answers (:290), six more writer tags whose sources the reference never
    updates (:159-161: they are written as 0.), no blank line in front of the epoch's Valid line (:368) and a ``load`` that
    strips ``.module`` and loads non-strictly (:425-431)."""

    order = "gqa"
    valid_factor = 2
    extra_tags = ('Train/node_gen/all_loss', 'Train/node_gen/dis_loss', 'Train/node_gen/grad_loss',
                  'Train/repr_gen/all_loss', 'Train/repr_gen/dis_loss', 'Train/repr_gen/grad_loss')

    def _total_iters_line(self, t_total):
        return "Total Iters: %d" % t_total

    def _loss_divisor(self, trainer):
        """``total_loss += loss / logit.size(1)`` (src/gqa/gqa_ood.py:290)"""
        return trainer.static["target"].shape[1]

    def _epoch_lines(self, epoch, train_score, valid_score, best_valid):
        s = f"\nEpoch {epoch}: Train {train_score:.2f}\n"
        if valid_score is not None:
            s += f"Epoch {epoch}: Valid {valid_score * 100.:.2f}\n" + f"Epoch {epoch}: Best {best_valid * 100.:.2f}\n"
        return s

    def _print_lr(self):
        pass

    def load(self, path):
        import torch
        print("Load model from %s" % path)
        state_dict = torch.load("%s.pth" % path, map_location="cpu", weights_only=True)
        for key in list(state_dict.keys()):
            if '.module' in key:
                state_dict[key.replace('.module', '')] = state_dict.pop(key)
        self.model.load_state_dict(state_dict, strict=False)
