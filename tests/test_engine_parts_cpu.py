"""The parts forward_loss, score and generate share (Engine._batch, _cross_keys, _dec_chains' whole-batch chain) on a host without a GPU,
through the fp32 test double: what a trace of the ops at tiny shapes would not show."""
import pytest
import torch

from lako_amd import FiDT5
from tests.test_engine_cpu import build, cfg_of
from tests.util_golden import load_case


@pytest.fixture(scope="module", autouse=True)
def global_rng_as_found():
    """FiDT5() draws its initial weights from torch's global generator: hand the generator back as this module found it, so that a
    test that runs later and builds a model without seeding sees the stream it saw before this file existed"""
    state = torch.get_rng_state()
    yield
    torch.set_rng_state(state)


def test_the_batch_prologue_keeps_the_padded_layout_when_asked():
    """Engine._batch, the prologue forward_loss, score and generate share: by default the valid tokens only; `keep_padding` (generate while
    the cross-attention scores are captured) gives the padded layout with the mask kept as the encoder's key mask and clears `_all_valid`
    — also right after an all-valid batch, whose flag must not leak — and the encoder output at the valid positions is the same."""
    z, dims, w, model = build("tiny_a")
    ids, mask = torch.from_numpy(z["input_ids"]), torch.from_numpy(z["attention_mask"])
    B, N, L = ids.shape
    eng = model._get_engine()
    eng.refresh_shadows()
    ws = eng._workspace(("prologue",))
    bt, enc_out, kv = eng._batch(ws, ids, mask, None)
    assert bt.rag is not None and bt.rag.M == int(mask.sum()) < mask.numel() and eng._row_cap == {bt.rag.M: B * N * L}
    assert bt.enc_ids.numel() == bt.rag.M and bt.xa is None and not eng.xattn_active and kv is not None
    packed = enc_out.clone()
    full, _, _ = eng._batch(ws, ids.clamp(min=2), torch.ones_like(mask), None)
    assert full.rag is None and full.enc_mask is None and eng._all_valid
    kept, enc_out, kv = eng._batch(ws, ids, mask, None, keep_padding=True)
    assert kept.rag is None and not eng._all_valid and eng._row_cap == {}
    assert kept.enc_mask is kept.mask_u8 and kept.enc_ids is kept.ids and kept.ids.numel() == B * N * L
    assert torch.equal(kept.mask_u8, mask.reshape(B * N, L).to(torch.uint8)) and tuple(enc_out.shape) == (B * N * L, dims.d_model)
    torch.testing.assert_close(enc_out[mask.reshape(-1)], packed, atol=5e-5, rtol=1e-4)
    assert eng._cross_keys(kept)[:2] == (B, N * L) and eng._cross_keys(bt)[:2] == (1, bt.rag.M)


def test_backward_uses_the_key_descriptor_forward_stored(monkeypatch):
    """forward_loss stores the cross-attention's key descriptor on the context (and the chains hold that very dict); backward derives
    nothing again: with the environment switched to another layout between the two calls, and the descriptor's builder made to fail,
    the gradients are those of the undisturbed step bit for bit."""
    z, dims, w, model = build("tiny_a", dropout=0.1)
    ids, mask, labels = (torch.from_numpy(z[k]) for k in ("input_ids", "attention_mask", "labels"))
    model.train()
    model(input_ids=ids, attention_mask=mask, labels=labels)[0].backward()
    eng = model._engine
    want = eng.G.clone()
    model.zero_grad()
    eng.step_count = 0            # the same dropout masks again
    loss = model(input_ids=ids, attention_mask=mask, labels=labels)[0]
    kb, kt, ckw = eng.ctx.cross
    assert eng.ctx.rag is not None and (kb, kt) == (1, eng.ctx.rag.M) and ckw["k_off"] is eng.ctx.rag.soff
    assert all(ch["ckw"] is ckw and (ch["kv_b"], ch["kv_t"]) == (kb, kt) for ch in eng.ctx.chains)
    monkeypatch.setenv("LAKO_UNPAD", "0")
    monkeypatch.setenv("LAKO_XATTN", "0")

    def no_second_derivation(*a, **k):
        raise AssertionError("backward derived the key descriptor again")
    monkeypatch.setattr(eng, "_cross_keys", no_second_derivation)
    loss.backward()
    assert torch.equal(eng.G, want)


def test_score_runs_the_whole_batch_as_one_chain_without_dropout(monkeypatch):
    """`score` takes its chain record from _dec_chains: ONE chain over all samples, no dropout — on a model in training mode with
    dropout configured and LAKO_DEC_CHAINS=2 set, which cuts the same batch in two in forward_loss — for the full chunk and the tail."""
    from tests.ref_ops_score import RefOpsScore
    monkeypatch.setenv("LAKO_DEC_CHAINS", "2")
    z, dims, w = load_case("tiny_eos")
    model = FiDT5(cfg_of(dims, 0.1), dtype=torch.float32, _ops=RefOpsScore())
    model.load_t5(w)
    model.train()
    ids, mask, labels = (torch.from_numpy(z[k]) for k in ("input_ids", "attention_mask", "labels"))
    B, T = ids.shape[0], 4
    assert B >= 4
    model(input_ids=ids, attention_mask=mask, labels=labels)
    eng = model._engine
    assert len(eng.ctx.chains) == 2 and eng.ctx.chains[1]["dr"](7) is not None
    seen, inner = [], eng._dec_layer_fwd
    monkeypatch.setattr(eng, "_dec_layer_fwd", lambda ws, i, ch, *a, **k: (seen.append(ch), inner(ws, i, ch, *a, **k))[1])
    cand = torch.randint(2, dims.vocab_size, (B, 3, T), generator=torch.Generator().manual_seed(3))
    model.score(ids, mask, cand, candidate_chunk=2)
    assert len(seen) == 2 * dims.num_decoder_layers
    for ch, c in zip(seen[::dims.num_decoder_layers], (2, 1)):
        assert (ch["c"], ch["b0"], ch["b1"], ch["B"], ch["r0"], ch["r1"], ch["kv_r"]) == (0, 0, B, B, 0, B * c * T, None)
        assert all(ch["dr"](site) is None for site in (3, 4, 4000, 4013))
