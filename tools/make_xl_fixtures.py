"""Generate the T5-3B / Flan-T5-XL golden fixtures tests/golden/xl3b_mid.npz and xlv11_mid.npz by RUNNING THE REFERENCE ITSELF.

Run in the build container only, next to oracle/make_fixtures.py (it needs the reference tree, which never travels to the GPU box):

    python tools/make_xl_fixtures.py

Two reduced-depth shapes with the per-layer widths of the real models where they are affordable on a CPU:
  xl3b_mid   t5-3b form:   ReLU, tied head, d_model 1024, d_kv 128, 8 heads, d_ff 512, vocab 256, 2 + 2 layers
  xlv11_mid  flan-t5-xl:   gated-GELU, untied head, d_model 2048, d_kv 64, 32 heads, d_ff 512, vocab 256, 2 + 2 layers

What runs: the reference's own `FiDT5` (src/model.py) and `set_optim` (src/util.py) through the harness of oracle/make_fixtures.py
(ReLU) and tools/make_gated_fixtures.py (gated, untied).  Like gated_mid, each file stores its weight seed (the ReLU case:
oracle.fid_t5_oracle.init_weights, the gated case: tests/util_gated.init_gated_weights, with per-tensor sums to check the
regeneration) instead of the weights, the loss and logits, every gradient's norm and a fixed sample of 512 of its elements, three
optimizer steps' losses, gradient norms and weight samples, greedy tokens and the step-0 cross-attention scores with the fact scores
of the stream-2 layout.  Only data is written.
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from oracle import make_fixtures as MF  # noqa: E402  (the harness: reference import + its three patches)
from oracle import fid_t5_oracle as O  # noqa: E402
from tests.util_gated import init_gated_weights  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_gated_fixtures", os.path.join(HERE, "make_gated_fixtures.py"))
MG = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MG)

ru = MF.ru


def weights_of(dims, gated, seed):
    return init_gated_weights(dims, seed) if gated else O.init_weights(dims, seed=seed)


def reference(dims, weights, gated):
    return MG.build_reference(dims, weights) if gated else MF.build_reference(dims, weights)


def make_case(name, dims, gated, B, N, L, T, seed):
    weights = weights_of(dims, gated, seed)
    ids, mask, labels = O.synthetic_batch(B, N, L, T, dims.vocab_size, seed=seed + 100)
    names = sorted(weights)
    g = torch.Generator().manual_seed(seed + 5)
    sample_idx = {k: torch.randint(0, weights[k].numel(), (min(MG.SAMPLE, weights[k].numel()),), generator=g).numpy() for k in names}
    out = dict(input_ids=ids.numpy(), attention_mask=mask.numpy(), labels=labels.numpy(), gated=np.array(int(gated)),
               dims=np.array([dims.vocab_size, dims.d_model, dims.d_kv, dims.d_ff, dims.num_layers,
                              dims.num_decoder_layers, dims.num_heads, dims.num_buckets, dims.max_distance]),
               w_seed=np.array(seed), w_sums=np.array([float(weights[k].double().sum()) for k in names]))
    out.update({"idx/" + k: sample_idx[k] for k in names})

    model = reference(dims, weights, gated)
    model.train()
    res = model(input_ids=ids, attention_mask=mask, labels=labels)
    res[0].backward()
    out.update(loss=np.array(res[0].item(), dtype=np.float64), logits=res.logits.detach().numpy())
    grads = MG.named(model, grad=True)
    if not gated:
        grads.pop("lm_head.weight", None)      # tied: the head IS shared (its gradient is in shared.weight)
    assert set(grads) == set(names), sorted(set(names) ^ set(grads))
    MG.store(out, "g/", grads, False, sample_idx)
    out["grad_norm"] = np.array(float(np.sqrt(sum(float((v.astype(np.float64) ** 2).sum()) for v in grads.values()))))
    model.zero_grad()

    opt = types.SimpleNamespace(optim="adamw", lr=1e-2, weight_decay=1e-2, scheduler="linear", scheduler_steps=None,
                                total_steps=10, warmup_steps=2, fixed_lr=False)
    optimizer, scheduler = ru.set_optim(opt, model)      # src/util.py:230-245
    losses, norms = [], []
    for k in range(3):
        bi, bm, bl = O.synthetic_batch(B, N, L, T, dims.vocab_size, seed=seed + 200 + k)
        tl = model(input_ids=bi, attention_mask=bm, labels=bl)[0]
        tl.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)))   # train_reader.py:76
        optimizer.step()
        scheduler.step()
        model.zero_grad()
        losses.append(tl.item())
    w3 = MG.named(model)
    if not gated:
        w3.pop("lm_head.weight", None)
    MG.store(out, "w_step3/", w3, False, sample_idx)
    out["train_losses"] = np.array(losses)
    out["train_gnorms"] = np.array(norms)
    out["train_hparams"] = np.array([opt.lr, opt.weight_decay, 1.0, opt.warmup_steps, opt.total_steps])

    # greedy generate + step-0 cross-attention scores (oracle/make_fixtures.py)
    model = reference(dims, weights, gated)
    model.eval()
    model.config.num_layers = dims.num_decoder_layers      # (see tools/make_gated_fixtures.py)
    qk, hooks = {}, []
    for li, blk in enumerate(model.decoder.block):
        att = blk.layer[1].EncDecAttention

        def _keep(kind, li):
            def hook(m, i, o):                           # first call = decode step 0; must return None
                qk.setdefault((kind, li), o.detach())
            return hook
        hooks.append(att.q.register_forward_hook(_keep("q", li)))
        hooks.append(att.k.register_forward_hook(_keep("k", li)))
    with torch.no_grad():
        for ml in (4, 12):
            out[f"gen_{ml}"] = model.generate(input_ids=ids, attention_mask=mask, max_length=ml).numpy()
    for h in hooks:
        h.remove()
    H, dk = dims.num_heads, dims.d_kv
    flat_mask = mask.view(B, -1)
    per_layer = []
    for li in range(dims.num_decoder_layers):
        q = qk[("q", li)].view(B, -1, H, dk).transpose(1, 2)
        k = qk[("k", li)].view(B, -1, H, dk).transpose(1, 2)
        s = torch.einsum("bnqd,bnkd->bnqk", q, k)
        s = s + torch.zeros(B, 1, 1, N * L).masked_fill(~flat_mask[:, None, None, :], torch.finfo(torch.float32).min)
        per_layer.append(s)
        model.decoder.block[li].layer[1].EncDecAttention.score_storage = s
    out["cross_scores"] = torch.cat(per_layer, dim=2).numpy()       # [B, H, n_layers, N·L]
    assert N == 2
    for style in ("mean", "max", "21mean"):
        for half in ("no", "yes"):
            o2 = types.SimpleNamespace(stream=2, n_context=5, use_last_half_layer_attention=half, attention_score_style=style)
            out[f"fact_scores_{style}_{half}"] = model.get_crossattention_scores(o2, ids, None, mask).numpy()   # src/model.py:143-204
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    np.savez_compressed(path, **out)
    print(name, "loss", out["loss"], "gnorm", out["grad_norm"], "gen", out["gen_12"].tolist(), f"{os.path.getsize(path)} B")


if __name__ == "__main__":
    torch.manual_seed(0)
    make_case("xl3b_mid", O.T5Dims(vocab_size=256, d_model=1024, d_kv=128, d_ff=512, num_layers=2, num_decoder_layers=2, num_heads=8,
                                   dropout=0.0), gated=False, B=2, N=2, L=24, T=6, seed=31)
    make_case("xlv11_mid", O.T5Dims(vocab_size=256, d_model=2048, d_kv=64, d_ff=512, num_layers=2, num_decoder_layers=2, num_heads=32,
                                    dropout=0.0), gated=True, B=2, N=2, L=24, T=6, seed=33)
