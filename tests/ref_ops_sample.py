"""The CPU test double (tests/ref_ops.py + ref_ops_score.py) plus the ops sampled decoding adds to the engine's vocabulary, and the
plain-torch restatement of the sampler (lako_sample_step, csrc/rowops.hip) that every sampling test compares against.

The sampler, for one row of logits x (a NaN counts as −∞), in real numbers — the restatement computes it in float64:
  weights   w_i = exp((x_i − max x) / temperature)
  top-k     0 < top_k < V: keep the top_k largest x, equal values by ascending index
  top-p     top_p < 1: in the order (x descending, index ascending) keep the shortest prefix of the kept whose mass reaches
            top_p · (mass of the kept); at least one token
  draw      u = U / 2^24,  U = hash32((hash32(seed_lo + 0x9E3779B9·k) ^ seed_hi) + 0x85EBCA6B·step + 0x1234567) >> 8   (all mod 2^32;
            k = row mod group: the sequence's index within its question; hash32 = tests/ref_ops.py::_hash32_int = lako_hash32);
            the token is the first kept index, ascending, whose running kept mass exceeds u · (kept mass)
  score     += log_softmax(x)[token]   (raw logits: neither temperature nor truncation)
A row without a finite logit gives token 0.  (The kernel rounds the weights to integers of 2^−40 and does the exp in fp32; a row is
*decidable* when neither the nucleus boundary nor the draw sits within 1e-5 of where such roundings could move it: sample_row.)"""
import numpy as np
import torch

from tests.ref_ops import M32, _hash32_int
from tests.ref_ops_score import RefOpsScore

MARGIN = 1e-5


def draw_u24(seed: int, k: int, step: int) -> int:
    seed &= 0xFFFFFFFFFFFFFFFF
    a = _hash32_int(((seed & M32) + 0x9E3779B9 * k) & M32)
    return _hash32_int(((a ^ (seed >> 32)) + 0x85EBCA6B * step + 0x1234567) & M32) >> 8


def sample_row(x: torch.Tensor, temperature: float, top_k: int, top_p: float, u24: int):
    """(token, log-prob of the token under the raw logits, decidable) for one row of logits (any float dtype; computed in float64).

    decidable: (a) u·mass is further than 1e-5·mass from both CDF edges of the drawn token, and (b) the nucleus is settled: its mass at
    the boundary (just before and just after its last token) is further than 1e-5 from top_p — or, where a token's probability is of the
    order of 1e-5 itself and no boundary can be that far from top_p (V = 32 128: the tokens at the 0.9 boundary of 3·randn logits have
    p ≈ 4e-6), EVERY nucleus whose boundary lies within 1e-5 of top_p gives the same token, each with margin (a).  With the boundary
    further than 1e-5 away there is one such nucleus and this is the plain rule."""
    V = x.numel()
    x = x.double()
    x = torch.where(torch.isnan(x), torch.full_like(x, -float("inf")), x)
    m = x.max()
    if not bool(m > -float("inf")):
        return 0, float("nan"), True
    temperature, top_p = float(np.float32(temperature)), float(np.float32(top_p))
    w = torch.exp((x - m) / temperature)
    # (x descending, index ascending): a stable sort of −x
    order = torch.sort(-x, stable=True).indices
    kept = torch.ones(V, dtype=torch.bool)
    if 0 < top_k < V:
        kept = torch.zeros(V, dtype=torch.bool)
        kept[order[:top_k]] = True

    def draw(kept):
        wk = torch.where(kept, w, torch.zeros_like(w))
        cum = torch.cumsum(wk, 0)
        mass = float(cum[-1])
        target = (u24 / 16777216.0) * mass
        tok = int(torch.nonzero((cum > target) & kept)[0])
        hi, lo = float(cum[tok]), float(cum[tok] - wk[tok])
        clear = not ((lo > 0.0 and abs(target - lo) <= MARGIN * mass) or (hi < mass and abs(target - hi) <= MARGIN * mass))
        return tok, clear

    if top_p < 1.0:
        o = order[kept[order]]
        cum = torch.cumsum(w[o], 0)
        total = float(cum[-1])

        def shortest(goal):          # the shortest prefix whose mass reaches the goal
            return max(1, min(int((cum < goal * total).sum()) + 1, o.numel()))
        n = shortest(top_p)
        variants = range(shortest(top_p - MARGIN), shortest(top_p + MARGIN) + 1)
        nucleus = torch.zeros(V, dtype=torch.bool)
        nucleus[o[:n]] = True
        tok, decidable = draw(nucleus)
        for n2 in variants:
            if n2 != n and decidable:
                other = torch.zeros(V, dtype=torch.bool)
                other[o[:n2]] = True
                tok2, clear2 = draw(other)
                decidable = clear2 and tok2 == tok
    else:
        tok, decidable = draw(kept)
    lp = float(x[tok] - m - torch.log(torch.exp(x - m).sum()))
    return tok, lp, decidable


def sample_rows(logits, temperature, top_k, top_p, seed, step, group):
    """the restatement over the rows of logits [rows, V]: (tokens int64 [rows], log-probs float64 [rows], decidable bool [rows])"""
    rows = logits.shape[0]
    toks, lps, dec = [], [], []
    lc = logits.detach().cpu()
    for r in range(rows):
        t, lp, d = sample_row(lc[r], temperature, top_k, top_p, draw_u24(seed, r % group, step))
        toks.append(t), lps.append(lp), dec.append(d)
    return torch.tensor(toks, dtype=torch.int64), torch.tensor(lps, dtype=torch.float64), torch.tensor(dec)


# ---- the sweep of the kernel test (tests/test_sample_gpu.py), built on the CPU: tests/test_sample_cpu.py holds its decidable fraction ----
SWEEP_V = [7, 256, 257, 32128]


def sweep_logits(rows, V, seed):
    """3·randn with a −∞ column and exact duplicates of the maximum (the tie rules: equal values by ascending index)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, V, generator=g) * 3.0
    x[:, V // 3] = -float("inf")
    top = x.max(1).values
    x[:, V - 1] = top                   # a second maximum behind the first …
    if V > 16:
        x[:, 5] = top                   # … and (larger rows) one in front of it
    return x


def pick_seed(x, temperature, top_k, top_p, step, group, base):
    """The seeds are picked on the CPU: the first of base, base + 1, … (at most 32) for which the restatement calls every row decidable.
    At V = 32 128 a token's probability is of the order of the 1e-5 margin itself, so an arbitrary seed leaves about one row in ten
    undecidable; what is still undecidable after 32 seeds is counted by the caller."""
    for seed in range(base, base + 32):
        want, lp, dec = sample_rows(x, temperature, top_k, top_p, seed, step, group)
        if bool(dec.all()):
            break
    return seed, want, lp, dec


def sweep_cases(V):
    """every (rows, top_k, top_p, temperature, step) of the sweep with its logits, its picked seed and the restatement's verdict"""
    for rows in (1, 5):
        x = sweep_logits(rows, V, 100 + V % 97 + rows)
        group = 3 if rows == 5 else 1
        for top_k in (0, 1, 2, 50, V):
            for top_p in (1.0, 0.9, 0.05):
                for temperature in (0.7, 1.0, 2.0):
                    for step in (0, 3):
                        base = (V * 1_000_003 + top_k * 7919 + int(top_p * 100) * 31 + int(temperature * 10)) * 2 ** 20 + 12345
                        seed, want, lp, dec = pick_seed(x, temperature, top_k, top_p, step, group, base)
                        yield dict(x=x, group=group, top_k=top_k, top_p=top_p, temperature=temperature, step=step, seed=seed, want=want,
                                   lp=lp, dec=dec, what=f"V={V} rows={rows} top_k={top_k} top_p={top_p} T={temperature} t={step}")


def unpack_params(params):
    """(temperature, top_p, top_k, seed) out of the 8-word device buffer of lako_sample_step"""
    wds = params.detach().cpu().numpy().view(np.uint32)
    return (float(wds[0:1].view(np.float32)[0]), float(wds[1:2].view(np.float32)[0]), int(wds[2]), int(wds[3]) | (int(wds[4]) << 32))


def pack_params(temperature, top_p, top_k, seed):
    """the 8-word buffer lako_sample_step reads (int32 view; the engine builds the same in Engine._sampler_params)"""
    seed &= 0xFFFFFFFFFFFFFFFF
    wds = np.array([np.float32(temperature).view(np.uint32), np.float32(top_p).view(np.uint32), min(top_k, 0x7FFFFFFF), seed & M32, seed >> 32,
                    0, 0, 0], dtype=np.uint32)
    return torch.from_numpy(wds.view(np.int32))


class RefOpsSample(RefOpsScore):
    def sample_step(self, logits, seq, pos, next_ids, done, score, n_done, params, step, group, eos_id=1, pad_id=0):
        temperature, top_p, top_k, seed = unpack_params(params)
        toks, lps, _ = sample_rows(logits, temperature, top_k, top_p, seed, step, group)
        live = ~done.bool().cpu()
        nxt = torch.where(live, toks, torch.full_like(toks, pad_id)).to(seq.device)
        seq[:, pos] = nxt
        next_ids.copy_(nxt)
        if score is not None:
            score += torch.where(live, torch.nan_to_num(lps), torch.zeros_like(lps)).to(score.dtype).to(score.device)
        done |= (nxt == eos_id).to(done.dtype)
        n_done[0] = int(done.sum())

    def xattn_decode_multi(self, Q, E, k_off, part_ml, part_c, rt=0):
        """per sequence what xattn_decode writes for that sequence's queries alone"""
        Bz, K, R, D = Q.shape
        Z = part_c.shape[0]
        pml, pc = part_ml.view(Z, Bz, K, 16, 2), part_c.view(Z, Bz, K, 16, D)
        for k in range(K):
            ml_k, c_k = torch.empty(Z, Bz, 16, 2), torch.empty(Z, Bz, 16, D)
            self.xattn_decode(Q[:, k], E, k_off, ml_k, c_k)
            pml[:, :, k] = ml_k
            pc[:, :, k] = c_k
