"""T5-3B (d_kv 128) and Flan-T5-XL (d_model 2048, 32 heads) readers on the CPU: named sizes and parameter counts, HF configs, and the
engine's schedule through the fp32 test double against the reference's fixtures (tools/make_xl_fixtures.py)."""
import json
import types

import numpy as np
import pytest
import torch

from lako_amd import FiDConfig
from lako_amd.engine import Engine, build_layout, layout_sizes
from tests.ref_ops import RefOps
from tests.util_gated import GatedRefOps
from tests.util_xl import build_xl, check_grads, train_three_steps

# config.json of t5-3b and google/flan-t5-xl (the fields the reader reads)
HF_T5_3B = dict(d_ff=16384, d_kv=128, d_model=1024, decoder_start_token_id=0, dropout_rate=0.1, eos_token_id=1,
                feed_forward_proj="relu", initializer_factor=1.0, is_encoder_decoder=True, layer_norm_epsilon=1e-06,
                model_type="t5", n_positions=512, num_decoder_layers=24, num_heads=32, num_layers=24, pad_token_id=0,
                relative_attention_num_buckets=32, vocab_size=32128, architectures=["T5WithLMHeadModel"])
HF_FLAN_XL = dict(d_ff=5120, d_kv=64, d_model=2048, decoder_start_token_id=0, dropout_rate=0.1, eos_token_id=1,
                  feed_forward_proj="gated-gelu", initializer_factor=1.0, is_encoder_decoder=True, layer_norm_epsilon=1e-06,
                  model_type="t5", n_positions=512, num_decoder_layers=24, num_heads=32, num_layers=24, pad_token_id=0,
                  relative_attention_max_distance=128, relative_attention_num_buckets=32, tie_word_embeddings=False,
                  vocab_size=32128, architectures=["T5ForConditionalGeneration"])


def test_named_xl_sizes_and_parameter_counts():
    c = FiDConfig.named("3b")
    assert (c.d_model, c.d_kv, c.d_ff, c.num_heads, c.num_layers, c.num_decoder_layers, c.vocab_size) == (1024, 128, 16384, 32, 24, 24, 32128)
    assert c.feed_forward_proj == "relu" and c.tie_word_embeddings and c.inner_dim == 4096
    x = FiDConfig.named("v1_1-xl")
    assert (x.d_model, x.d_kv, x.d_ff, x.num_heads, x.num_layers, x.num_decoder_layers, x.vocab_size) == (2048, 64, 5120, 32, 24, 24, 32128)
    assert x.feed_forward_proj == "gated-gelu" and not x.tie_word_embeddings
    assert layout_sizes(build_layout(c))[0] == 2_851_598_336
    assert layout_sizes(build_layout(x))[0] == 2_849_757_184
    for big in ("11b", "v1_1-xxl"):
        with pytest.raises(ValueError, match="unknown model size"):
            FiDConfig.named(big)


@pytest.mark.parametrize("hf,named", [(HF_T5_3B, "3b"), (HF_FLAN_XL, "v1_1-xl")], ids=["t5-3b", "flan-t5-xl"])
def test_from_hf_round_trips(hf, named):
    cfg = FiDConfig.from_hf(hf)
    assert cfg == FiDConfig.named(named)
    assert FiDConfig.from_hf(json.loads(cfg.to_json())) == cfg


def test_engine_accepts_d_kv_128_and_refuses_the_rest():
    small = dict(vocab_size=64, d_model=256, d_ff=64, num_layers=1, num_decoder_layers=1, num_heads=2)
    Engine(FiDConfig(d_kv=128, **small), RefOps(), "cpu", dtype=torch.float32)
    for dk in (16, 96, 256):
        with pytest.raises(ValueError, match="32, 64 or 128"):
            Engine(FiDConfig(d_kv=dk, **small), RefOps(), "cpu", dtype=torch.float32)


def test_fp8_is_refused_for_d_kv_128():
    cfg = FiDConfig(vocab_size=64, d_model=256, d_kv=128, d_ff=64, num_layers=1, num_decoder_layers=1, num_heads=2)
    ops = RefOps()
    ops.gemm_nt_mx = lambda *a, **k: None
    with pytest.raises(ValueError, match="d_kv=128"):
        Engine(cfg, ops, "cpu", dtype=torch.bfloat16, fp8=True)


CASES = ["xl3b_mid", "xlv11_mid"]


def build(name):
    return build_xl(name, torch.float32, ops=GatedRefOps() if name == "xlv11_mid" else RefOps())


@pytest.mark.parametrize("name", CASES)
def test_forward_backward_vs_reference(name):
    z, dims, gated, model = build(name)
    ids, mask, labels = (torch.from_numpy(z[k]) for k in ("input_ids", "attention_mask", "labels"))
    model.train()
    out = model(input_ids=ids, attention_mask=mask, labels=labels)
    assert abs(out[0].item() - float(z["loss"])) < 2e-5
    torch.testing.assert_close(out.logits, torch.from_numpy(z["logits"]), atol=5e-5, rtol=1e-4)
    out[0].backward()
    check_grads(z, model, rel=2e-4, tol=dict(atol=5e-5, rtol=2e-4))


@pytest.mark.parametrize("name", CASES)
def test_train_steps_vs_reference(name):
    """(weights: Adam divides by sqrt(v) + 1e-6, so elements whose gradients are rounding noise move by rounding noise times lr — at the
    XL width the update of such elements differs by up to 6e-5 from the reference's; test_engine_cpu.py loosens its tiny_eos step alike)"""
    z, dims, gated, model = build(name)
    train_three_steps(name, z, dims, model, lambda t: t, loss_tol=3e-5, gn_tol=1e-3, w_tol=dict(atol=1e-4, rtol=2e-4))


@pytest.mark.parametrize("name", CASES)
def test_generate_and_scores_vs_reference(name):
    z, dims, gated, model = build(name)
    ids, mask = torch.from_numpy(z["input_ids"]), torch.from_numpy(z["attention_mask"])
    model.eval()
    for ml in (4, 12):
        assert model.generate(input_ids=ids, attention_mask=mask, max_length=ml).tolist() == z[f"gen_{ml}"].tolist()
    model.overwrite_forward_crossattention()
    model.reset_score_storage()
    model.generate(input_ids=ids, attention_mask=mask, max_length=4)
    ref = torch.from_numpy(z["cross_scores"])
    keep = mask.view(mask.shape[0], 1, 1, -1).expand_as(ref)
    torch.testing.assert_close(model._score_storage[keep], ref[keep], atol=5e-5, rtol=1e-4)
    for style in ("mean", "max", "21mean"):
        for half in ("no", "yes"):
            o = types.SimpleNamespace(stream=2, n_context=5, use_last_half_layer_attention=half, attention_score_style=style)
            np.testing.assert_allclose(model.get_crossattention_scores(o, ids, None, mask).numpy(), z[f"fact_scores_{style}_{half}"],
                                       rtol=2e-5, atol=2e-6)
