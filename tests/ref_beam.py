"""Beam search over a `logits(b, rows)` callable, written out plainly and independently of the engine: the semantics of transformers 5.15
`_beam_search` as FiDT5.generate(num_beams=K) states them.

Per question: K running hypotheses (one to begin with: the start token — HF's K − 1 further initial beams carry −1e9 and never enter the
2K best of step 0) and a finished list of at most K.  Step t (n = t + 1 tokens generated after it): every continuation scores
running score + log_softmax(logits)[v]; the 2K best are taken, by score descending and flat index beam·V + v ascending; a candidate ends
with EOS or at the last step (t + 2 == max_length); the first K that do not end run on; an ending one among the first K is offered with
score / n**length_penalty while the question is open (and, with early_stopping, while the list is not full); the list keeps its best K,
old before new on ties; the question closes once the list is full and best running / n**length_penalty <= the list's worst.  Decoding
ends when no question is open, or early_stopping and every list is full, or at the last step; until then closed questions keep
stepping."""
import torch

from oracle import fid_t5_oracle as O


def oracle_logits(w, dims, input_ids, attention_mask):
    """logits(b, rows int64 [k, n]) → [k, V]: the next-token logits of the oracle's FiD-T5 (fp32, as the oracle computes) for question b
    after each of the k prefixes"""
    enc, enc_mask = O.fid_encode(w, dims, input_ids, attention_mask, False)

    def logits(b, rows):
        k = rows.shape[0]
        h = O.decoder_stack(w, dims, rows, enc[b:b + 1].expand(k, -1, -1), enc_mask[b:b + 1].expand(k, -1), False)
        return (h[:, -1] * dims.d_model ** -0.5) @ w["shared.weight"].t()
    return logits


def beam_search(logits, B, K, max_length, length_penalty=1.0, early_stopping=False, eos=1, start=0, dtype=torch.float64):
    """The search's own arithmetic (log-softmax, running sums) in `dtype`.  → per question the finished list, best first: [(tokens (start token first, EOS last if it ended with one), normalised score, raw
    sum of log-probabilities)]"""
    run = [[([start], None)] for _ in range(B)]         # (tokens, score tensor)
    fin = [[] for _ in range(B)]
    is_open = [True] * B
    for t in range(max_length - 1):
        n, last = t + 1, t + 2 == max_length
        for b in range(B):
            rows = torch.tensor([r[0] for r in run[b]], dtype=torch.int64)
            lg = logits(b, rows)
            lp = torch.log_softmax(lg.to(dtype), -1)
            V = lp.shape[1]
            prev = torch.stack([r[1] if r[1] is not None else lp.new_zeros(()) for r in run[b]])
            acc = (prev[:, None] + lp).reshape(-1)
            top = torch.sort(-acc, stable=True).indices[:2 * K].tolist()
            accept = is_open[b] and not (early_stopping and len(fin[b]) == K)
            nxt = []
            for j, flat in enumerate(top):
                k, v = divmod(flat, V)
                toks = run[b][k][0] + [v]
                if v == eos or last:
                    if j < K and accept:
                        sc = float(acc[flat]) / n ** length_penalty
                        at = next((i for i, f in enumerate(fin[b]) if sc > f[1]), len(fin[b]))
                        fin[b].insert(at, (toks, sc, float(acc[flat])))
                        del fin[b][K:]
                elif len(nxt) < K:
                    nxt.append((toks, acc[flat]))
            if nxt:
                run[b] = nxt
                if len(fin[b]) == K and float(nxt[0][1]) / n ** length_penalty <= min(f[1] for f in fin[b]):
                    is_open[b] = False
        if not any(is_open) or (early_stopping and all(len(f) == K for f in fin)) or last:
            break
    return fin
