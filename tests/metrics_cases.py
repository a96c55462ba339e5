"""Inputs and CPU yardsticks of the loss / prec@k meter tests (tests/test_gpu_metrics.py).

Labels are PLANTED: random labels give no top-5 hit at K = 1000 and would test nothing.  Row b gets
  b % 3 == 0: the class at stable-sorted position 0 (the argmax),
  b % 3 == 1: the class at stable-sorted position 1 + (b // 3) % 6 -- it straddles k = 5,
  otherwise : a random class.
The expected values are stated here from the definitions, not taken from any implementation under test:
  rank = #{j : x_j > x_l} + #{j < l : x_j == x_l}   (position of the label in a stable descending sort)."""
import functools

import torch

SEED = 21
SHAPES = [(9, 1), (5, 7), (8, 257), (37, 1000), (64, 16), (3, 65536), (300, 16), (1, 1000)]


@functools.lru_cache(maxsize=None)
def planted(B, K, dtype):
    """(logits of ``dtype`` on the CPU, int64 labels); cached -- callers must not modify them."""
    g = torch.Generator().manual_seed(SEED)
    logits = (torch.randn(B, K, generator=g) * 3).to(dtype)
    order = torch.sort(logits.float(), dim=1, descending=True, stable=True).indices
    labels = torch.randint(0, K, (B,), generator=g)
    for b in range(B):
        if b % 3 == 0:
            labels[b] = order[b, 0]
        elif b % 3 == 1:
            labels[b] = order[b, min(1 + (b // 3) % 6, K - 1)]
    return logits, labels


def stable_rank(logits, labels):
    """The stable-rule rank of valid labels, on the CPU (NaN-free logits)."""
    x = logits.float()
    xl = x.gather(1, labels.view(-1, 1))
    idx = torch.arange(x.shape[1]).view(1, -1)
    return ((x > xl).sum(1) + ((x == xl) & (idx < labels.view(-1, 1))).sum(1)).to(torch.int32)


def label_has_twin(logits, labels):
    """Rows where another logit equals the label's logit bit for bit (torch.topk may order those either way)."""
    x = logits.float()
    return (x == x.gather(1, labels.view(-1, 1))).sum(1) > 1


def topk_hits(logits, labels, k):
    """The reference's own definition (train_util.py:59-61): label among output.topk(k, 1, True, True), fp32 on the CPU."""
    _, pred = logits.float().topk(min(k, logits.shape[1]), 1, True, True)
    return (pred == labels.view(-1, 1)).any(1)


def ce_fp64(logits, labels):
    return torch.nn.functional.cross_entropy(logits.double(), labels, reduction="none")
