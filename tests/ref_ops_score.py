"""The CPU test double (tests/ref_ops.py) plus the op `Engine.score` adds to the engine's vocabulary."""
import torch

from tests.ref_ops import RefOps


class RefOpsScore(RefOps):
    def seq_logprob(self, logits, labels, score, n_valid, T):
        """score[r] = Σ_t log softmax(logits[r·T + t])[labels[r·T + t]] over the labels in [0, V), n_valid[r] their count"""
        V = logits.shape[1]
        valid = (labels >= 0) & (labels < V)
        lp = torch.log_softmax(logits.float(), -1).gather(1, labels.clamp(0, V - 1)[:, None])[:, 0]
        score.copy_(torch.where(valid, lp, torch.zeros_like(lp)).view(-1, T).sum(1))
        n_valid.copy_(valid.view(-1, T).sum(1).to(n_valid.dtype))
