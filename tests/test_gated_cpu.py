"""T5 v1.1 / Flan-T5 readers (gated-GELU feed-forward, untied LM head) on the CPU: configuration, parameter layout, checkpoints,
and the engine's schedule through the CPU test double (tests/util_gated.GatedRefOps) against the reference's gated_tiny fixture."""
import json
import types

import numpy as np
import pytest
import torch

from lako_amd import FiDConfig, FiDT5
from lako_amd import util as U
from lako_amd.engine import Engine, build_layout
from lako_amd.model import plain_name, wrapped_name
from oracle import fid_t5_oracle as O
from tests.util_gated import GatedRefOps, gated_cfg, gelu_new, gelu_new_grad, load_gated
from tests.util_golden import group

HF_FLAN = dict(vocab_size=64, d_model=32, d_kv=32, d_ff=48, num_layers=2, num_decoder_layers=2, num_heads=2,
               feed_forward_proj="gated-gelu", tie_word_embeddings=False, model_type="t5")


def test_from_hf_accepts_gated_gelu_and_rejects_the_rest():
    cfg = FiDConfig.from_hf(HF_FLAN)
    assert cfg.feed_forward_proj == "gated-gelu" and cfg.tie_word_embeddings is False and cfg.gated
    for ff in ("gated-silu", "gelu", "silu"):
        with pytest.raises(ValueError, match="feed-forward"):
            FiDConfig.from_hf(dict(HF_FLAN, feed_forward_proj=ff))
    v10 = FiDConfig.from_hf(dict(HF_FLAN, feed_forward_proj="relu", tie_word_embeddings=None))
    assert v10.feed_forward_proj == "relu" and v10.tie_word_embeddings and not v10.gated
    d = json.loads(cfg.to_json())
    assert d["feed_forward_proj"] == "gated-gelu" and d["tie_word_embeddings"] is False
    assert FiDConfig.from_hf(d) == cfg


def test_named_v1_1_sizes():
    for name, (dm, ff, H, nl) in {"v1_1-small": (512, 1024, 6, 8), "v1_1-base": (768, 2048, 12, 12),
                                  "v1_1-large": (1024, 2816, 16, 24)}.items():
        c = FiDConfig.named(name)
        assert (c.d_model, c.d_ff, c.num_heads, c.num_layers, c.num_decoder_layers, c.d_kv, c.vocab_size) == (dm, ff, H, nl, nl, 64, 32128)
        assert c.feed_forward_proj == "gated-gelu" and not c.tie_word_embeddings
    assert FiDConfig.named("base").feed_forward_proj == "relu" and FiDConfig.named("base").tie_word_embeddings


def _old_layout(cfg):
    """the v1.0 block table as the layout was built before the gated form existed: (name, shape, members, transposed), in order"""
    d, f, inner, H, nb = cfg.d_model, cfg.d_ff, cfg.inner_dim, cfg.num_heads, cfg.relative_attention_num_buckets
    out = [("dec.final_ln", (d,), [("decoder.final_layer_norm.weight", 0, d)], False)]
    for i in range(cfg.num_decoder_layers):
        p = f"decoder.block.{i}.layer."
        out += [(f"dec.{i}.qkv", (3 * inner, d), [(p + f"0.SelfAttention.{n}.weight", j * inner, inner) for j, n in enumerate("qkv")], True),
                (f"dec.{i}.o", (d, inner), [(p + "0.SelfAttention.o.weight", 0, d)], True),
                (f"dec.{i}.ln1", (d,), [(p + "0.layer_norm.weight", 0, d)], False),
                (f"dec.{i}.cq", (inner, d), [(p + "1.EncDecAttention.q.weight", 0, inner)], True),
                (f"dec.{i}.co", (d, inner), [(p + "1.EncDecAttention.o.weight", 0, d)], True),
                (f"dec.{i}.ln2", (d,), [(p + "1.layer_norm.weight", 0, d)], False),
                (f"dec.{i}.wi", (f, d), [(p + "2.DenseReluDense.wi.weight", 0, f)], True),
                (f"dec.{i}.wo", (d, f), [(p + "2.DenseReluDense.wo.weight", 0, d)], True),
                (f"dec.{i}.ln3", (d,), [(p + "2.layer_norm.weight", 0, d)], False)]
    out.append(("dec.rel", (nb, H), [("decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight", 0, nb)], False))
    kv = []
    for i in range(cfg.num_decoder_layers):
        p = f"decoder.block.{i}.layer.1.EncDecAttention."
        kv += [(p + "k.weight", 2 * i * inner, inner), (p + "v.weight", (2 * i + 1) * inner, inner)]
    out.append(("dec.kv_all", (cfg.num_decoder_layers * 2 * inner, d), kv, True))
    out.append(("enc.final_ln", (d,), [("encoder.final_layer_norm.weight", 0, d)], False))
    for i in reversed(range(cfg.num_layers)):
        p = f"encoder.block.{i}.layer."
        out += [(f"enc.{i}.qkv", (3 * inner, d), [(p + f"0.SelfAttention.{n}.weight", j * inner, inner) for j, n in enumerate("qkv")], True),
                (f"enc.{i}.o", (d, inner), [(p + "0.SelfAttention.o.weight", 0, d)], True),
                (f"enc.{i}.ln1", (d,), [(p + "0.layer_norm.weight", 0, d)], False),
                (f"enc.{i}.wi", (f, d), [(p + "1.DenseReluDense.wi.weight", 0, f)], True),
                (f"enc.{i}.wo", (d, f), [(p + "1.DenseReluDense.wo.weight", 0, d)], True),
                (f"enc.{i}.ln2", (d,), [(p + "1.layer_norm.weight", 0, d)], False)]
    out.append(("enc.rel", (nb, H), [("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight", 0, nb)], False))
    out.append(("shared", (cfg.vocab_size, d), [("shared.weight", 0, cfg.vocab_size)], True))
    return out


@pytest.mark.parametrize("size", ["tiny", "small", "base", "large"])
def test_relu_layout_is_unchanged(size):
    cfg = FiDConfig.named(size)
    blocks = build_layout(cfg)
    assert [(b.name, b.shape, b.members, b.transpose) for b in blocks] == _old_layout(cfg)
    off = toff = 0
    for b in blocks:       # offsets: each block at the previous one's end rounded up to 64 elements
        assert b.off == off and (b.toff == toff if b.transpose else b.toff == -1)
        off += -(-b.numel // 64) * 64
        if b.transpose:
            toff += -(-b.numel // 64) * 64


def test_gated_layout():
    cfg = FiDConfig.from_hf(HF_FLAN)
    by = {b.name: b for b in build_layout(cfg)}
    f, d = cfg.d_ff, cfg.d_model
    wi = by["enc.1.wi"]
    assert wi.shape == (2 * f, d) and wi.transpose
    assert wi.members == [("encoder.block.1.layer.1.DenseReluDense.wi_0.weight", 0, f),
                          ("encoder.block.1.layer.1.DenseReluDense.wi_1.weight", f, f)]
    assert by["dec.0.wi"].members[1] == ("decoder.block.0.layer.2.DenseReluDense.wi_1.weight", f, f)
    assert by["lm_head"].shape == (cfg.vocab_size, d) and by["lm_head"].transpose and build_layout(cfg)[0].name == "lm_head"


def test_gelu_new_grad_matches_autograd():
    x = torch.linspace(-9, 9, 2001, dtype=torch.float64, requires_grad=True)
    gelu_new(x).sum().backward()
    torch.testing.assert_close(gelu_new_grad(x.detach()), x.grad)
    torch.testing.assert_close(gelu_new(x.detach()), torch.nn.functional.gelu(x.detach(), approximate="tanh"))


def build(name="gated_tiny", dropout=0.0, ops=None):
    z, dims, w = load_gated(name)
    model = FiDT5(gated_cfg(dims, dropout), dtype=torch.float32, _ops=ops or GatedRefOps())
    model.load_t5(w)
    return z, dims, w, model


def test_state_dict_names_and_round_trip(tmp_path):
    z, dims, w, model = build()
    sd = model.state_dict()
    assert sd["lm_head.weight"].data_ptr() != sd["shared.weight"].data_ptr()
    assert "encoder.encoder.block.0.module.layer.1.DenseReluDense.wi_0.weight" in sd
    assert "decoder.block.1.layer.2.DenseReluDense.wi_1.weight" in sd
    for k, v in w.items():
        assert torch.equal(sd[wrapped_name(k)], v), k
    model.save_pretrained(str(tmp_path / "wrapped"))
    m2 = FiDT5.from_pretrained(str(tmp_path / "wrapped"), dtype=torch.float32, _ops=GatedRefOps())
    assert m2.config == model.config
    for k, v in w.items():
        assert torch.equal(m2.state_dict()[wrapped_name(k)], v), k
    # a plain HF directory: config.json + pytorch_model.bin with plain names and the tied embedding aliases
    hf = tmp_path / "flan"
    hf.mkdir()
    (hf / "config.json").write_text(json.dumps(dict(HF_FLAN, architectures=["T5ForConditionalGeneration"])))
    plain = {k: v.clone() for k, v in w.items()}
    plain["encoder.embed_tokens.weight"] = plain["decoder.embed_tokens.weight"] = plain["shared.weight"]
    torch.save(plain, hf / "pytorch_model.bin")
    m3 = FiDT5.from_pretrained(str(hf), dtype=torch.float32, _ops=GatedRefOps())
    m3.unwrap_encoder()
    for k, v in w.items():
        assert torch.equal(m3.state_dict()[k], v), k
    # an untied checkpoint without its head is incomplete
    del plain["lm_head.weight"]
    with pytest.raises(KeyError, match="lm_head"):
        FiDT5(gated_cfg(dims), dtype=torch.float32, _ops=GatedRefOps()).load_t5(plain)


def test_forward_backward_vs_reference():
    z, dims, w, model = build()
    ids, mask, labels = (torch.from_numpy(z[k]) for k in ("input_ids", "attention_mask", "labels"))
    model.train()
    out = model(input_ids=ids, attention_mask=mask, labels=labels)
    assert abs(out[0].item() - float(z["loss"])) < 2e-5
    torch.testing.assert_close(out.logits, torch.from_numpy(z["logits"]), atol=5e-5, rtol=1e-4)
    out[0].backward()
    g = group(z, "g/")
    params = {plain_name(n): p for n, p in model.named_parameters()}
    assert set(params) == set(g) and "lm_head.weight" in g
    for k, p in params.items():
        torch.testing.assert_close(p.grad, g[k], atol=5e-5, rtol=2e-4, msg=lambda m, k=k: f"{k}: {m}")


def test_train_steps_and_generate_vs_reference():
    z, dims, w, model = build()
    B, N, L = z["input_ids"].shape
    T = z["labels"].shape[1]
    lr, wd, clip, warm, total = z["train_hparams"].tolist()
    opt = types.SimpleNamespace(optim="adamw", lr=lr, weight_decay=wd, scheduler="linear", scheduler_steps=None,
                                total_steps=int(total), warmup_steps=int(warm), fixed_lr=False)
    model.eval()
    ids, mask = torch.from_numpy(z["input_ids"]), torch.from_numpy(z["attention_mask"])
    for ml in (4, 12):
        assert model.generate(ids, mask, ml).tolist() == z[f"gen_{ml}"].tolist()
    optimizer, scheduler = U.set_optim(opt, model)
    model.train()
    for k in range(3):
        bi, bm, bl = O.synthetic_batch(B, N, L, T, dims.vocab_size, seed=21 + 200 + k)
        loss = model(input_ids=bi, attention_mask=bm, labels=bl)[0]
        loss.backward()
        gn = U.clip_grad_norm_(model, clip)
        optimizer.step()
        scheduler.step()
        model.zero_grad()
        assert abs(loss.item() - z["train_losses"][k]) < 3e-5
        assert abs(gn.item() - z["train_gnorms"][k]) < 1e-3 * max(1.0, z["train_gnorms"][k])
    ref = group(z, "w_step3/")
    for n, p in model.named_parameters():
        torch.testing.assert_close(p.detach(), ref[plain_name(n)], atol=3e-5, rtol=2e-4, msg=lambda m, n=n: f"{n}: {m}")


def test_set_checkpoint_and_dropout_recompute_match():
    """dropout on: the recomputed encoder (set_checkpoint) regenerates the gated activation's mask: identical gradients"""
    grads = []
    for ckpt in (False, True):
        z, dims, w, model = build(dropout=0.1)
        model.set_checkpoint(ckpt)
        model.train()
        ids, mask, labels = (torch.from_numpy(z[k]) for k in ("input_ids", "attention_mask", "labels"))
        model(input_ids=ids, attention_mask=mask, labels=labels)[0].backward()
        grads.append(model._engine.G.clone())
    torch.testing.assert_close(grads[0], grads[1], atol=1e-6, rtol=1e-5)


def test_fp8_is_refused_for_gated_configs():
    cfg = FiDConfig.from_hf(HF_FLAN)
    ops = GatedRefOps()
    ops.gemm_nt_mx = lambda *a, **k: None      # (the refusal is about the FFN, not the op set)
    with pytest.raises(ValueError, match="gated"):
        Engine(cfg, ops, "cpu", dtype=torch.bfloat16, fp8=True)
