"""tests/golden/beam_hf.npz: what transformers' own beam search returns for the reference FiD-T5 on the weights and inputs of
tests/golden/tiny_eos.npz.  Runs on the CPU, where the reference and transformers are installed.  Only data is written: HF's token rows
(−1 behind the returned width), its `sequences_scores`, the case table (K, length_penalty, early_stopping, max_length) and per case the
smallest gap between adjacent returned scores of a question.  A case is recorded only if tests/ref_beam.py reproduces it with its arithmetic in float64 and
in float32 (tokens up to the first EOS, scores within 1e-4); at least six must remain."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import transformers  # noqa: E402

from oracle.make_fixtures import build_reference  # noqa: E402
from tests.ref_beam import beam_search, oracle_logits  # noqa: E402
from tests.util_golden import load_case  # noqa: E402

CASES = [(2, 1.0, False, 8), (3, 1.0, False, 8), (4, 1.0, False, 8), (3, 0.0, False, 8), (3, 2.0, False, 8), (3, 1.0, True, 8),
         (4, 1.0, False, 4)]


def upto_eos(row, eos=1):
    row = [int(v) for v in row if v >= 0]
    return row[:row.index(eos) + 1] if eos in row[1:] else row


def main():
    z, dims, w = load_case("tiny_eos")
    ids, mask = torch.from_numpy(z["input_ids"]), torch.from_numpy(z["attention_mask"])
    B, N, _ = ids.shape
    model = build_reference(dims, w).eval()
    logits = oracle_logits(w, dims, ids, mask)
    out, kept = {}, []
    for K, lpen, early, ML in CASES:
        model.encoder.n_passages = N
        with torch.no_grad():
            hf = transformers.T5ForConditionalGeneration.generate(
                model, input_ids=ids.view(B, -1), attention_mask=mask.view(B, -1), max_length=ML, num_beams=K, num_return_sequences=K,
                length_penalty=lpen, early_stopping=early, do_sample=False, return_dict_in_generate=True, output_scores=True)
        seqs, scores = hf.sequences.view(B, K, -1), hf.sequences_scores.view(B, K).float()
        ok = True
        for dtype in (torch.float64, torch.float32):
            fin = beam_search(logits, B, K, ML, lpen, early, dtype=dtype)
            for b in range(B):
                for k in range(K):
                    same = k < len(fin[b]) and fin[b][k][0] == upto_eos(seqs[b, k].tolist()) and abs(fin[b][k][1] - float(scores[b, k])) <= 1e-4
                    ok = ok and same
        lens = sorted({len(upto_eos(r.tolist())) for r in seqs.reshape(B * K, -1)})
        gap = float((scores[:, :-1] - scores[:, 1:]).min())
        print(f"K={K} length_penalty={lpen} early_stopping={early} max_length={ML}: width {seqs.shape[2]}, lengths {lens}, "
              f"smallest score gap {gap:.3e}, tests/ref_beam.py reproduces it: {ok}")
        if not ok:
            continue
        i = len(kept)
        kept.append((K, lpen, float(early), ML))
        tok = np.full((B, K, ML), -1, dtype=np.int64)
        tok[:, :, :seqs.shape[2]] = seqs.numpy()
        out[f"tokens_{i}"], out[f"scores_{i}"], out[f"gap_{i}"] = tok, scores.numpy(), np.float64(gap)
    assert len(kept) >= 6, f"only {len(kept)} cases reproduced"
    out["cases"] = np.array(kept, dtype=np.float64)
    path = os.path.join(ROOT, "tests", "golden", "beam_hf.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(kept)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
