"""Linear-chain CRF over per-token tag scores, in plain torch.

A path y of a sentence of n tokens scores ``start[y_0] + sum_t logits[t, y_t] + sum_{t>=1} trans[y_{t-1}, y_t] +
end[y_{n-1}]``; ``trans[i, j]`` is the score of tag i followed by tag j.  ``Crf.nll`` and ``Crf.decode`` run on any
device and dtype and use no in-tree kernel: they are the CPU path of PyBiLstmCrf and, in fp64, the reference of the
GPU kernels (csrc/kernels/crf.hip, reached through engine/tagger.py), which compute the same loss on the same scale.
"""
import torch


class Crf(torch.nn.Module):
    def __init__(self, num_tags: int):
        super().__init__()
        self.trans = torch.nn.Parameter(torch.empty(num_tags, num_tags).uniform_(-0.1, 0.1))
        self.start = torch.nn.Parameter(torch.empty(num_tags).uniform_(-0.1, 0.1))
        self.end = torch.nn.Parameter(torch.empty(num_tags).uniform_(-0.1, 0.1))

    def nll(self, logits_blk, tags, lens):
        """sum_b (logZ_b - score_b(tags_b)) / #tokens: logits_blk [B, L, tags], tags [B, L] (read for t < lens[b]),
        lens [B].  The per-token scale is that of the softmax cross-entropy it replaces."""
        B, L, _ = logits_blk.shape
        dev = logits_blk.device
        lens = torch.as_tensor(lens, device=dev).long()
        tags = torch.as_tensor(tags, device=dev).long().clamp(min=0)
        steps = torch.arange(L, device=dev)[None, :] < lens[:, None]            # [B, L]: token t exists
        alpha = self.start + logits_blk[:, 0]
        for t in range(1, L):
            nxt = torch.logsumexp(alpha[:, :, None] + self.trans[None], dim=1) + logits_blk[:, t]
            alpha = torch.where(steps[:, t, None], nxt, alpha)
        log_z = torch.logsumexp(alpha + self.end, dim=1)
        emit = logits_blk.gather(2, tags[:, :, None]).squeeze(2) * steps
        score = self.start[tags[:, 0]] + emit.sum(1) + self.end[tags.gather(1, (lens - 1).clamp(min=0)[:, None])[:, 0]]
        if L > 1:
            score = score + (self.trans[tags[:, :-1], tags[:, 1:]] * steps[:, 1:]).sum(1)
        return ((log_z - score) * (lens > 0)).sum() / lens.sum().clamp(min=1)

    @torch.no_grad()
    def decode(self, logits_blk, lens):
        """The best path of every sentence: int64 [B, L], -1 for t >= lens[b]."""
        B, L, _ = logits_blk.shape
        dev = logits_blk.device
        lens = torch.as_tensor(lens, device=dev).long()
        score = self.start + logits_blk[:, 0]
        back = []
        for t in range(1, L):
            best, arg = (score[:, :, None] + self.trans[None]).max(dim=1)       # over the previous tag
            score = torch.where((t < lens)[:, None], best + logits_blk[:, t], score)
            back.append(arg)
        cur = (score + self.end).argmax(dim=1)                                  # the tag of token lens[b] - 1
        out = torch.full((B, L), -1, dtype=torch.long, device=dev)
        for t in range(L - 1, -1, -1):
            here = t < lens
            out[:, t] = torch.where(here, cur, out[:, t])
            if t > 0:
                cur = torch.where(here, back[t - 1].gather(1, cur[:, None])[:, 0], cur)
        return out
