"""Generate the T5 v1.1 golden fixtures tests/golden/gated_*.npz by RUNNING THE REFERENCE ITSELF.

Run in the build container only, next to oracle/make_fixtures.py (it needs the reference tree, which never travels to the GPU box):

    python tools/make_gated_fixtures.py

What runs: the reference's own `FiDT5` (src/model.py) and `set_optim` (src/util.py) with the same three harness patches as
oracle/make_fixtures.py (imported from there), on a `T5Config(feed_forward_proj="gated-gelu", tie_word_embeddings=False)`.

transformers 5.x reads `tie_word_embeddings=False` as "do not rescale the decoder output" but still ties `lm_head` to `shared`.
The published v1.1 semantics (transformers 4.x, the real Flan-T5 checkpoints) have an untied head, so after construction `lm_head`
gets its own parameter; the script asserts that it is not `shared` and that the logits follow it.

gated_tiny stores everything.  gated_mid (d 768, f 2048) would be ≈100 MB per weight set, so it stores its weight seed
(tests/util_gated.init_gated_weights, with per-tensor sums to check the regeneration), every gradient's norm and a fixed sample
of 512 of its elements, and the same for the weights after three optimizer steps.  Only data is written.
"""
from __future__ import annotations

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

import transformers  # noqa: E402

rm, ru = MF.rm, MF.ru
SAMPLE = 512


def build_reference(dims: O.T5Dims, weights: dict):
    cfg = transformers.T5Config(
        vocab_size=dims.vocab_size, d_model=dims.d_model, d_kv=dims.d_kv, d_ff=dims.d_ff,
        num_layers=dims.num_layers, num_decoder_layers=dims.num_decoder_layers, num_heads=dims.num_heads,
        relative_attention_num_buckets=dims.num_buckets, relative_attention_max_distance=dims.max_distance,
        dropout_rate=0.0, layer_norm_epsilon=dims.eps, feed_forward_proj="gated-gelu", tie_word_embeddings=False,
        decoder_start_token_id=0, pad_token_id=0, eos_token_id=1)
    cfg._attn_implementation = "eager"
    assert cfg.is_gated_act and cfg.dense_act_fn == "gelu_new" and not cfg.scale_decoder_outputs
    model = rm.FiDT5(cfg)
    sd = {k: v.clone() for k, v in weights.items() if k != "lm_head.weight"}
    sd["encoder.embed_tokens.weight"] = sd["shared.weight"]
    sd["decoder.embed_tokens.weight"] = sd["shared.weight"]
    sd["lm_head.weight"] = sd["shared.weight"]
    model.load_t5(sd)                                   # src/model.py:79-82
    model.lm_head.weight = torch.nn.Parameter(weights["lm_head.weight"].clone())      # untie (see the module docstring)
    assert model.lm_head.weight.data_ptr() != model.shared.weight.data_ptr()
    return model


def plain(wrapped: str):
    if wrapped in ("encoder.encoder.embed_tokens.weight", "decoder.embed_tokens.weight"):
        return None
    if wrapped.startswith("encoder.encoder."):
        wrapped = "encoder." + wrapped[len("encoder.encoder."):]
    return wrapped.replace(".module.layer.", ".layer.")


def named(model, grad=False):
    out = {}
    for k, p in model.named_parameters():
        pk = plain(k)
        if pk is None:
            continue
        t = p.grad if grad else p
        if t is not None:
            out[pk] = t.detach().numpy().copy()
    return out


def store(out, prefix, tensors, full, sample_idx):
    for k, v in tensors.items():
        if full:
            out[prefix + k] = v
        else:
            out["norm_" + prefix + k] = np.array(float(np.sqrt((v.astype(np.float64) ** 2).sum())))
            out["s_" + prefix + k] = v.reshape(-1)[sample_idx[k]]


def make_case(name, dims, B, N, L, T, seed, full, eos_row=False):
    weights = init_gated_weights(dims, seed)
    ids, mask, labels = O.synthetic_batch(B, N, L, T, dims.vocab_size, seed=seed + 100)
    if eos_row:                     # an early EOS: target of length 2, then ignored positions
        labels[0, 1] = 1
        labels[0, 2:] = -100
    names = sorted(weights)
    g = torch.Generator().manual_seed(seed + 5)
    sample_idx = {k: torch.randint(0, weights[k].numel(), (min(SAMPLE, weights[k].numel()),), generator=g).numpy() for k in names}
    out = dict(input_ids=ids.numpy(), attention_mask=mask.numpy(), labels=labels.numpy(),
               dims=np.array([dims.vocab_size, dims.d_model, dims.d_kv, dims.d_ff, dims.num_layers,
                              dims.num_decoder_layers, dims.num_heads, dims.num_buckets, dims.max_distance]))
    if full:
        out.update({"w/" + k: v.numpy() for k, v in weights.items()})
    else:
        out["w_seed"] = np.array(seed)
        out["w_sums"] = np.array([float(weights[k].double().sum()) for k in names])
        out.update({"idx/" + k: sample_idx[k] for k in names})

    model = build_reference(dims, weights)
    model.train()
    res = model(input_ids=ids, attention_mask=mask, labels=labels)
    res[0].backward()
    out.update(loss=np.array(res[0].item(), dtype=np.float64), logits=res.logits.detach().numpy())
    grads = named(model, grad=True)
    assert set(grads) == set(names), sorted(set(names) ^ set(grads))
    store(out, "g/", grads, full, sample_idx)
    out["grad_norm"] = np.array(float(np.sqrt(sum(float((v.astype(np.float64) ** 2).sum()) for v in grads.values()))))
    model.zero_grad()
    # the logits follow the untied head (not `shared`)
    with torch.no_grad():
        base = model(input_ids=ids, attention_mask=mask, labels=labels).logits.clone()
        model.lm_head.weight.mul_(2.0)
        assert torch.allclose(model(input_ids=ids, attention_mask=mask, labels=labels).logits, 2 * base, rtol=1e-4, atol=1e-5)
        model.lm_head.weight.mul_(0.5)

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
    assert model.lm_head.weight.data_ptr() != model.shared.weight.data_ptr()
    store(out, "w_step3/", named(model), full, sample_idx)
    out["train_losses"] = np.array(losses)
    out["train_gnorms"] = np.array(norms)
    out["train_hparams"] = np.array([opt.lr, opt.weight_decay, 1.0, opt.warmup_steps, opt.total_steps])

    model = build_reference(dims, weights)
    model.eval()
    with torch.no_grad():
        # (transformers 5 sizes generate's key / value cache by config.num_layers — the ENCODER's count; the stacks are built, so
        # the decoder's count there only sizes the cache)
        model.config.num_layers = dims.num_decoder_layers
        for ml in (4, 12):
            out[f"gen_{ml}"] = model.generate(input_ids=ids, attention_mask=mask, max_length=ml).numpy()
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", name + ".npz"), **out)
    print(name, "loss", out["loss"], "gnorm", out["grad_norm"], "gen", out["gen_12"].tolist())


if __name__ == "__main__":
    torch.manual_seed(0)
    make_case("gated_tiny", O.T5Dims(vocab_size=64, d_model=32, d_kv=32, d_ff=48, num_layers=2, num_decoder_layers=2, num_heads=2,
                                     dropout=0.0), B=2, N=3, L=8, T=5, seed=21, full=True)
    make_case("gated_mid", O.T5Dims(vocab_size=512, d_model=768, d_kv=64, d_ff=2048, num_layers=1, num_decoder_layers=2, num_heads=12,
                                    dropout=0.0), B=2, N=3, L=40, T=6, seed=23, full=False, eos_row=True)
