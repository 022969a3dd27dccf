"""The CPU test double (tests/ref_ops_sample.py) plus the three ops beam search adds to the engine's vocabulary, restated in plain
torch / Python: what tests/test_beam_gpu.py compares lako_beam_rows, lako_beam_merge and lako_beam_gather (csrc/beam.hip) against.

The rules are those of include/lako_hip.h.  rows: per row the C best logits in the order (x descending, index ascending; a NaN counts as
−∞) as (run + log_softmax(x)[token], token) — the log-softmax in float64, rounded to fp32, the sum in fp32.  merge: the question's 2K
best candidates by (acc descending, flat index k·V + token ascending); the first K that do not end run on; an ending candidate (EOS, or
the last step) among the first K of the 2K is offered with acc / pos**length_penalty (fp32) unless the question is closed, or
early_stopping is set and all K slots were filled before the step; the finished set keeps the best K of (old ∪ offers), old before new
on ties; then open &= not (all filled and run[0] / pos**length_penalty <= min finished); n_done += K if the question is done."""
import numpy as np
import torch

from tests.ref_ops_sample import RefOpsSample


def rows_ref(logits, run, C):
    """→ (acc fp32 [rows, C], token int32 [rows, C])"""
    x = logits.detach().cpu().double()
    x = torch.where(torch.isnan(x), torch.full_like(x, -float("inf")), x)
    m = x.max(1, keepdim=True).values
    lse = m + torch.log(torch.exp(x - m).sum(1, keepdim=True))
    order = torch.sort(-x, dim=1, stable=True).indices[:, :C]
    xv = torch.gather(x, 1, order)
    lp = torch.where(xv > -float("inf"), xv - lse, torch.full_like(xv, -float("inf")))
    return run.detach().cpu().float()[:, None] + lp.float(), order.to(torch.int32)


def pack_beam_params(length_penalty, early_stopping):
    """the 8-word buffer lako_beam_merge reads (int32 view; the engine builds the same in Engine._beam_params)"""
    wds = np.array([np.float32(length_penalty).view(np.uint32), int(bool(early_stopping)), 0, 0, 0, 0, 0, 0], dtype=np.uint32)
    return torch.from_numpy(wds.view(np.int32))


def unpack_beam_params(params):
    wds = params.detach().cpu().numpy().view(np.uint32)
    return float(wds[0:1].view(np.float32)[0]), bool(wds[1])


def merge_ref(cand_acc, cand_tok, seq_src, fin_src, pos, last, run, fin_score, fin_raw, fin_len, fin_filled, open_, length_penalty,
              early_stopping, eos_id=1, pad_id=0):
    """One step for every question, on CPU tensors; nothing is modified.  → dict of the new state: seq, fin, run, next_ids, parent,
    fin_score, fin_raw, fin_len, fin_filled, open, n_done (the sum over the questions)"""
    BK, C = cand_acc.shape
    K = C // 2
    B, ld = BK // K, seq_src.shape[1]
    f32 = np.float32
    norm = f32(np.power(f32(pos), f32(length_penalty)))
    out = dict(seq=torch.zeros_like(seq_src), fin=torch.zeros_like(fin_src), run=run.clone(), next_ids=torch.zeros(BK, dtype=torch.int64),
               parent=torch.zeros(BK, dtype=torch.int32), fin_score=fin_score.clone(), fin_raw=fin_raw.clone(), fin_len=fin_len.clone(),
               fin_filled=fin_filled.clone(), open=open_.clone(), n_done=0)
    out["seq"].copy_(seq_src)         # (columns behind pos are the kernel's to leave alone: the caller compares [0, pos])
    acc_all = torch.nan_to_num(cand_acc.float(), nan=-float("inf"), posinf=float("inf"), neginf=-float("inf")).numpy()
    for b in range(B):
        cands = [(-float(acc_all[b * K + k, j]), k, int(cand_tok[b * K + k, j])) for k in range(K) for j in range(C)]
        top = sorted(cands)[:C]
        fin = [dict(score=f32(fin_score[b * K + k]), raw=f32(fin_raw[b * K + k]), len=int(fin_len[b * K + k]),
                    row=fin_src[b * K + k].clone()) for k in range(K) if bool(fin_filled[b * K + k])]
        accept = bool(open_[b]) and not (early_stopping and len(fin) == K)
        nxt = []
        for j, (nacc, k, tok) in enumerate(top):
            ends = tok == eos_id or bool(last)
            if not ends:
                if len(nxt) < K:
                    nxt.append((f32(-nacc), k, tok))
            elif j < K and accept:
                sc = f32(-nacc) / norm
                row = torch.full((ld,), pad_id, dtype=torch.int64)
                row[:pos] = seq_src[b * K + k, :pos]
                row[pos] = tok
                at = next((i for i, f in enumerate(fin) if sc > f["score"]), len(fin))
                fin.insert(at, dict(score=sc, raw=f32(-nacc), len=pos + 1, row=row))
                del fin[K:]
        for j in range(C):
            if len(nxt) < K:
                nxt.append((f32(-top[j][0]), top[j][1], top[j][2]))
        for j, (acc, k, tok) in enumerate(nxt):
            r = b * K + j
            out["run"][r], out["next_ids"][r], out["parent"][r] = float(acc), tok, b * K + k
            out["seq"][r, :pos] = seq_src[b * K + k, :pos]
            out["seq"][r, pos] = tok
        for k in range(K):
            r = b * K + k
            if k < len(fin):
                out["fin_score"][r], out["fin_raw"][r], out["fin_len"][r] = float(fin[k]["score"]), float(fin[k]["raw"]), fin[k]["len"]
                out["fin_filled"][r] = 1
                out["fin"][r] = fin[k]["row"]
            else:       # an unfilled slot keeps what it held
                out["fin"][r] = fin_src[r]
        filled = len(fin) == K
        is_open = bool(open_[b])
        if filled and nxt[0][0] / norm <= min(f["score"] for f in fin):
            is_open = False
        out["open"][b] = int(is_open)
        if (not is_open) or (early_stopping and filled) or bool(last):
            out["n_done"] += K
    return out


class RefOpsBeam(RefOpsSample):
    def beam_rows(self, logits, run, cand_acc, cand_tok):
        acc, tok = rows_ref(logits, run, cand_acc.shape[1])
        cand_acc.copy_(acc)
        cand_tok.copy_(tok)

    def beam_merge(self, cand_acc, cand_tok, seq_src, seq_dst, fin_src, fin_dst, pos, last, run, next_ids, parent, fin_score, fin_raw, fin_len,
                   fin_filled, open_, n_done, params, eos_id=1, pad_id=0):
        lpen, early = unpack_beam_params(params)
        o = merge_ref(cand_acc, cand_tok, seq_src, fin_src, pos, last, run, fin_score, fin_raw, fin_len, fin_filled, open_, lpen, early,
                      eos_id, pad_id)
        seq_dst[:, :pos + 1] = o["seq"][:, :pos + 1]
        fin_dst.copy_(o["fin"])
        for dst, key in ((run, "run"), (next_ids, "next_ids"), (parent, "parent"), (fin_score, "fin_score"), (fin_raw, "fin_raw"),
                         (fin_len, "fin_len"), (fin_filled, "fin_filled"), (open_, "open")):
            dst.copy_(o[key])
        n_done[0] += o["n_done"]

    def beam_gather(self, src, dst, parent, n_pos, col0, width):
        dst[:, :, :n_pos, col0:col0 + width] = src[:, parent.long(), :n_pos, col0:col0 + width]
