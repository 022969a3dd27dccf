"""The parts forward_loss, score and generate share (Engine._batch, _cross_keys, _dec_chains' whole-batch chain) and the parts of backward
(its plan of switches, the one feed-forward backward, the chain records it only reads) on a host without a GPU, through the fp32 test
double: what a trace of the ops at tiny shapes would not show."""
import pytest
import torch

from lako_amd import FiDT5
from tests.ref_ops import RefOps
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


# ---- backward in parts ------------------------------------------------------------------------------------------------------------
def step(name="tiny_a", env=None, checkpoint=False, legacy=False, before_backward=None):
    """one forward + backward with dropout 0.1 and the masks of step 0 on a freshly built model → (engine, loss, its context)"""
    import contextlib
    import dataclasses

    from tools.op_trace import environment
    z, dims, w = load_case(name)
    cfg = cfg_of(dims, 0.1)
    with environment(env or {}) if env else contextlib.nullcontext():
        torch.manual_seed(0)
        model = FiDT5(dataclasses.replace(cfg, legacy_cross_bias=True) if legacy else cfg, dtype=torch.float32, _ops=RefOps())
        if not legacy:      # (the fixtures have no cross-attention table: the seeded initial weights)
            model.load_t5(w)
        model.set_checkpoint(checkpoint)
        model.train()
        loss = model(**{k: torch.from_numpy(z[k]) for k in ("input_ids", "attention_mask", "labels")})[0]
        eng = model._engine
        ctx = eng.ctx
        if before_backward is not None:
            before_backward(eng)
        loss.backward()
    return eng, loss.detach().clone(), ctx


@pytest.fixture(scope="module")
def default_step():
    eng, loss, _ = step()
    return loss, eng.G.clone()


@pytest.mark.parametrize("env,checkpoint", [({"LAKO_FUSE_DROP": "0"}, False), ({"LAKO_DEC_HB_DEFER": "0"}, False),
                                            ({"LAKO_DEC_DEFER_DW": "0"}, False), ({"LAKO_ENC_DW_GROUP": "1"}, False),
                                            ({"LAKO_ENC_DW_SPLIT": "2"}, False), ({}, True)],
                         ids=["fuse_drop0", "hb_defer0", "defer_dw0", "enc_dw_group1", "enc_dw_split2", "checkpoint"])
def test_every_schedule_of_backward_gives_the_default_schedules_gradients_bit_for_bit(env, checkpoint, default_step):
    """the A/B switches and set_checkpoint only move launches: on the double (fp32, the same dropout masks) loss and G are `torch.equal`
    to the default schedule's — measured so on the commit before backward was cut into parts, hence no tolerance"""
    eng, loss, _ = step(env=env, checkpoint=checkpoint)
    assert torch.equal(loss, default_step[0])
    assert torch.equal(eng.G, default_step[1])


def test_the_encoder_and_the_decoder_reach_the_one_feed_forward_backward():
    """one call per encoder layer, which may ask for the library's gated routes, and one per decoder layer, which may not"""
    seen = []

    def spy(eng):
        inner = eng._ffn_bwd
        eng._ffn_bwd = lambda *a, library_gated, **k: (seen.append(library_gated), inner(*a, library_gated=library_gated, **k))[1]
    eng, _, _ = step(before_backward=spy)
    Ld, Le = eng.cfg.num_decoder_layers, eng.cfg.num_layers
    assert seen == [False] * Ld + [True] * Le and Ld == Le == 2


@pytest.mark.parametrize("name,legacy,env", [("tiny_a", False, None), ("tiny_a", True, None), ("tiny_eos", True, {"LAKO_DEC_CHAINS": "2"})],
                         ids=["tiny_a", "legacy_cross_bias", "legacy_cross_bias-two_chains"])
def test_backward_leaves_the_chain_records_as_forward_loss_made_them(name, legacy, env):
    """the chains belong to forward_loss: backward hands the head-batched list and legacy_cross_bias's gradient table to the layers as
    arguments — no chain gains a key, and `ckw` stays the very object forward_loss stored (with one chain: the context's descriptor)"""
    before = {}

    def snapshot(eng):
        before.update(keys=[sorted(ch) for ch in eng.ctx.chains], ckw=[ch["ckw"] for ch in eng.ctx.chains],
                      items=[dict(ch["ckw"]) for ch in eng.ctx.chains])
    eng, _, ctx = step(name, env=env, legacy=legacy, before_backward=snapshot)
    assert len(ctx.chains) == (2 if env else 1) and (eng.dec_xrel is not None) == legacy
    assert [sorted(ch) for ch in ctx.chains] == before["keys"] and "hb" not in ctx.chains[0]
    for ch, ckw, items in zip(ctx.chains, before["ckw"], before["items"]):
        assert ch["ckw"] is ckw and "drel" not in ckw and sorted(ckw) == sorted(items) and all(ckw[k] is items[k] for k in items)
    if not env:
        assert ctx.chains[0]["ckw"] is ctx.cross[2]
    if legacy:      # (and the table's gradient did arrive)
        assert float(eng.dec_xrel.g.abs().max()) > 0


def test_backward_reads_its_switches_once_when_it_is_called(monkeypatch):
    """Engine._bwd_plan is the one place backward reads the environment (LAKO_TN_SLABS stays in _tn_scratch): a switch set between
    forward_loss and backward takes effect, and once the plan exists every further read of a LAKO_* name fails"""
    import os
    applied, reads = [], []

    def guard(eng):
        monkeypatch.setenv("LAKO_FUSE_DROP", "0")
        plan, real, apply = eng._bwd_plan, os.environ.get, eng.ops.dropout_apply

        def no_switch(key, default=None):
            reads.append(key)
            if key.startswith("LAKO_") and key != "LAKO_TN_SLABS":
                raise AssertionError(f"backward read {key} after it had made its plan")
            return real(key, default)

        def plan_then_guard(ctx):
            bw = plan(ctx)
            monkeypatch.setattr(os.environ, "get", no_switch)
            os.environ.get("PATH")      # (the call the engine makes goes through the guard)
            return bw
        monkeypatch.setattr(eng, "_bwd_plan", plan_then_guard)
        monkeypatch.setattr(eng.ops, "dropout_apply", lambda *a, **k: (applied.append(1), apply(*a, **k))[1], raising=False)
    try:
        eng, _, _ = step(before_backward=guard)
    finally:
        monkeypatch.undo()
    assert reads[0] == "PATH" and set(reads[1:]) <= {"LAKO_TN_SLABS"}
    # LAKO_FUSE_DROP=0 as read at the backward call: one dropout_apply per residual branch, 2 per encoder and 3 per decoder layer
    assert len(applied) == 2 * eng.cfg.num_layers + 3 * eng.cfg.num_decoder_layers
