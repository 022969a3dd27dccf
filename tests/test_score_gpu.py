"""-m gpu: candidate scoring on the HIP path — lako_seq_logprob against torch in float64, and FiDT5.score against the same model's
per-candidate `forward` logits (the only way to score an answer without it: log_softmax → gather → masked sum)."""
import pytest
import torch

from lako_amd import FiDConfig, FiDT5
from oracle import fid_t5_oracle as O
from tests.test_kernels_gpu import close
from tests.util_golden import load_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# fp32 engine: the bound of the fp32 parity tests (tests/test_parity_gpu.py: logits within atol 1e-3, rtol 1e-3)
F32_TOL = dict(atol=1e-3, rtol=1e-3)
# bf16 engine: 1.5 × the largest |score − per-candidate forward| measured on the MI355X over the four bf16 runs of
# test_model_scores_match_per_candidate_forward (LAKO_XATTN=1: default chunk 4.7684e-7, candidate_chunk=2 4.7684e-7; LAKO_XATTN=0: 9.9468e-3 and 0.0): 9.9468e-3.  The projected
# attention kernel tiles Lq = C·T = 20 query rows differently from Lq = T = 4, so its bf16 probabilities round differently; on the
# encoder-state path the same kernels see the same rows.  DESIGN.md §3 "Candidate scoring"
SCORE_BF16_MEASURED = 9.9468e-3
SCORE_BF16_BOUND = 1.5 * SCORE_BF16_MEASURED


@pytest.fixture(scope="module", autouse=True)
def global_rng_as_found():
    """FiDT5() draws its initial weights from torch's global generator and the model tests seed it: hand the generator back as this
    module found it, so that a test that runs later and builds a model without seeding (tests/test_xl_gpu.py: three bf16 AdamW steps
    whose loss must fall) sees the stream it saw before this file existed"""
    state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(DEV)      # (torch.manual_seed seeds the device's generator too)
    yield
    torch.set_rng_state(state)
    torch.cuda.set_rng_state(dev_state, DEV)


@pytest.fixture(scope="module")
def ops():
    from lako_amd.ops import HipOps
    return HipOps()


# ---- the kernel ------------------------------------------------------------------------------------------------------------
def kernel_case(R, T, V):
    """logits with row 0 shifted by +80, row 1 by −80 and (more than two valid rows) row 2 with a single dominant logit at its label;
    labels covering 0 and V − 1, an ignored token in the middle of sequence 1 (T >= 3) and the last sequence ignored altogether"""
    g = torch.Generator().manual_seed(1000 * R + 10 * T + V % 7)
    logits = torch.randn(R * T, V, generator=g) * 3.0
    labels = torch.randint(0, V, (R, T), generator=g)
    flat, n_rows = labels.view(-1), (R - 1) * T            # rows of the sequences that keep valid labels
    flat[n_rows - 1] = V - 1
    if n_rows > 1:
        flat[0] = 0
    labels[R - 1] = -100                                   # a sequence without any valid label: 0 / 0
    if T >= 3:
        labels[1, T // 2] = -100                           # an ignored token between two valid ones
    logits[0] += 80.0
    logits[1] -= 80.0
    if n_rows > 2:
        logits[2, int(flat[2])] = 60.0                     # log-prob ≈ 0
    return logits.to(DEV), labels.to(DEV)


def kernel_ref(logits, labels, T):
    lp = torch.log_softmax(logits.double(), -1)
    valid = labels.view(-1) != -100
    pick = lp.gather(1, labels.view(-1).clamp(min=0)[:, None])[:, 0]
    score = torch.where(valid, pick, torch.zeros_like(pick)).view(-1, T).sum(1).float()
    return score, valid.view(-1, T).sum(1).to(torch.int32)


@pytest.mark.parametrize("R,T,V", [(3, 5, 32128), (2, 1, 520), (7, 3, 8)])
def test_seq_logprob_against_float64(ops, R, T, V):
    logits, labels = kernel_case(R, T, V)
    want, n_want = kernel_ref(logits, labels, T)
    outs = []
    for _ in range(2):
        score = torch.full((R + 5,), 7777.0, device=DEV)
        n_valid = torch.full((R + 5,), -7, dtype=torch.int32, device=DEV)
        ops.seq_logprob(logits, labels.view(-1), score[:R], n_valid[:R], T)
        torch.cuda.synchronize()
        assert torch.equal(score[R:], torch.full((5,), 7777.0, device=DEV)) and torch.equal(n_valid[R:].cpu(), torch.full((5,), -7, dtype=torch.int32))
        outs.append((score[:R].clone(), n_valid[:R].clone()))
    print(f"seq_logprob {R}x{T}x{V}: max |err| {float((outs[0][0] - want).abs().max()):.3e} (scale {float(want.abs().max()):.3e})")
    assert torch.equal(outs[0][1], n_want)
    assert float(outs[0][0][R - 1]) == 0.0 and int(outs[0][1][R - 1]) == 0
    close(outs[0][0], want, torch.float32, f"seq_logprob {R}x{T}x{V}")
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])       # the same launch twice: the same bits
    if (R - 1) * T > 2:                                                                       # the dominant-logit row: log-prob ≈ 0
        assert abs(float(torch.log_softmax(logits[2].double(), -1)[labels.view(-1)[2]])) < 1e-6


def test_seq_logprob_ignores_labels_outside_the_vocabulary(ops):
    """a label outside [0, V) other than −100 is the caller's error: treated as ignored, never read out of bounds"""
    V, T = 16, 4
    logits = (torch.randn(2 * T, V, generator=torch.Generator().manual_seed(5)) * 2.0).to(DEV)
    labels = torch.tensor([[3, V, 5, -1], [V + 100, -100, -7, 2 ** 40]], device=DEV)
    good = torch.tensor([[3, -100, 5, -100], [-100, -100, -100, -100]], device=DEV)
    want, n_want = kernel_ref(logits, good, T)
    score, n_valid = torch.empty(2, device=DEV), torch.empty(2, dtype=torch.int32, device=DEV)
    ops.seq_logprob(logits, labels.view(-1), score, n_valid, T)
    assert torch.equal(n_valid, n_want) and n_want.tolist() == [2, 0]
    close(score, want, torch.float32, "seq_logprob out-of-range labels")


# ---- the model ---------------------------------------------------------------------------------------------------------------
def candidates_of(B, C, T, V, seed, first=None):
    g = torch.Generator().manual_seed(seed)
    cand = torch.randint(2, V, (B, C, T), generator=g)
    if first is not None:
        cand[:, 0] = first
    cand[:, 1, T - 1:] = -100
    cand[:, 2, 1:] = -100
    cand[0, 3, 2:] = -100
    cand[:, C - 1] = -100
    return cand


def forward_scores(model, ids, mask, cand):
    """the per-candidate way: one `forward` per candidate, log_softmax of its logits → gather → masked sum (a candidate without any
    valid token scores 0 by definition and needs no forward)"""
    B, C, T = cand.shape
    score, n = torch.zeros(B, C, device=cand.device), torch.zeros(B, C, dtype=torch.int32, device=cand.device)
    with torch.no_grad():
        for c in range(C):
            lab = cand[:, c].contiguous()
            valid = lab != -100
            if not bool(valid.any()):
                continue
            logits = model(input_ids=ids, attention_mask=mask, labels=lab).logits
            lp = torch.log_softmax(logits.float(), -1).gather(2, lab.clamp(min=0)[..., None])[..., 0]
            score[:, c] = torch.where(valid, lp, torch.zeros_like(lp)).sum(1)
            n[:, c] = valid.sum(1)
    return score, n


def check_scores(runs, want, dtype, what):
    """runs: {name: scores}.  Every figure is printed before anything is asserted"""
    diffs = {k: float((got - want).abs().max()) for k, got in runs.items()}
    for k, diff in diffs.items():
        print(f"{what} {k}: max |score − per-candidate forward| = {diff:.4e} (largest |score| {float(want.abs().max()):.3f})")
    for k, got in runs.items():
        if dtype == torch.float32:
            torch.testing.assert_close(got, want, **F32_TOL)
        else:
            assert diffs[k] <= SCORE_BF16_BOUND, (what, k, diffs[k], SCORE_BF16_BOUND)


@pytest.mark.parametrize("xattn", ["1", "0"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_model_scores_match_per_candidate_forward(dt, xattn, monkeypatch):
    """B = 2, N = 3, L = 24 with ragged passage lengths, C = 5, T = 4 on a two-layer model the encoder-state cross-attention takes
    (d_kv 64, d_model 128) — in bf16 with LAKO_XATTN=1; the fp32 engine and LAKO_XATTN=0 run the projected formulation, Lq = C·T"""
    monkeypatch.setenv("LAKO_DTYPE", dt)
    monkeypatch.setenv("LAKO_XATTN", xattn)
    dtype = torch.float32 if dt == "f32" else torch.bfloat16
    torch.manual_seed(17)
    cfg = FiDConfig(vocab_size=64, d_model=128, d_kv=64, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2, dropout_rate=0.0)
    model = FiDT5(cfg).cuda().eval()
    assert model.compute_dtype == dtype
    B, N, L, C, T = 2, 3, 24, 5, 4
    ids, mask, labels = (t.to(DEV) for t in O.synthetic_batch(B, N, L, T, cfg.vocab_size, seed=23))
    assert 0 < int(mask.sum()) < B * N * L
    cand = candidates_of(B, C, T, cfg.vocab_size, 29, first=labels.cpu()).to(DEV)
    want, n = forward_scores(model, ids, mask, cand)
    eng = model._engine
    got = model.score(ids, mask, cand)
    assert eng.xattn_active == (dt == "bf16" and xattn == "1")
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, C) and bool(torch.isfinite(got).all())
    assert torch.equal(got[:, C - 1], torch.zeros(B, device=DEV))
    check_scores({"default chunk": got, "chunk=2": model.score(ids, mask, cand, candidate_chunk=2)}, want, dtype, f"score {dt} xattn={xattn}")
    sc, nv = eng.score(ids, mask, cand)
    assert torch.equal(nv, n) and torch.equal(sc, got)
    assert torch.equal(model.score(ids, mask, cand, normalize=True), got / n.clamp(min=1))
    # a training step in flight is left alone
    model.train()
    loss = model(input_ids=ids, attention_mask=mask, labels=labels)[0]
    ctx = eng.ctx
    assert torch.equal(model.score(ids, mask, cand), got) and eng.ctx is ctx and eng.step_count == 0
    loss.backward()
    assert eng.step_count == 1 and bool(torch.isfinite(eng.G).all())


@pytest.mark.parametrize("name", ["gated_mid", "xl3b_mid"])
def test_wide_and_gated_models_score_like_their_forward(name):
    """Flan-T5 shapes (gated-GELU feed-forward, untied LM head, d_model 768) and T5-3B's head dim 128 at reduced depth, fp32 engine"""
    if name == "gated_mid":
        from tests.util_gated import gated_cfg, load_gated
        z, dims, w = load_gated(name)
        model = FiDT5(gated_cfg(dims), dtype=torch.float32)
        model.load_t5(w)
        model = model.cuda()
    else:
        from tests.util_xl import build_xl
        z, dims, _, model = build_xl(name, torch.float32, device="cuda")
    model.eval()
    ids, mask, labels = (torch.from_numpy(z[k]).to(DEV) for k in ("input_ids", "attention_mask", "labels"))
    T = 4
    cand = candidates_of(ids.shape[0], 5, T, dims.vocab_size, 31, first=labels[:, :T].cpu()).to(DEV)
    want, n = forward_scores(model, ids, mask, cand)
    check_scores({"default chunk": model.score(ids, mask, cand), "chunk=2": model.score(ids, mask, cand, candidate_chunk=2)}, want,
                 torch.float32, f"score {name}")


def test_the_greedy_answer_outscores_itself_with_another_first_token():
    """sanity: the greedy output of `generate` (start token stripped, −100 after EOS) scores at least as high as the same sequence
    with its first token replaced"""
    z, dims, w = load_case("tiny_eos")
    from tests.test_parity_gpu import cfg_of
    model = FiDT5(cfg_of(dims), dtype=torch.float32)
    model.load_t5(w)
    model = model.cuda().eval()
    ids, mask = (torch.from_numpy(z[k]).to(DEV) for k in ("input_ids", "attention_mask"))
    T, B, V = 4, ids.shape[0], dims.vocab_size
    toks = model.generate(input_ids=ids, attention_mask=mask, max_length=T + 1)[:, 1:]
    greedy = torch.full((B, T), -100, dtype=torch.int64, device=DEV)
    greedy[:, :toks.shape[1]] = toks
    after_eos = ((greedy == dims_eos(model)).cumsum(1) - (greedy == dims_eos(model)).long()) > 0
    greedy[after_eos] = -100
    cand = greedy[:, None, :].repeat(1, 4, 1)
    for k in range(1, 4):
        cand[:, k, 0] = (greedy[:, 0] + 7 * k) % (V - 2) + 2          # another first token (never pad / EOS)
        assert not bool((cand[:, k, 0] == greedy[:, 0]).any())
    sc = model.score(ids, mask, cand)
    print("greedy vs replaced first token:", sc.tolist())
    assert bool((sc[:, :1] >= sc[:, 1:]).all()), sc.tolist()


def dims_eos(model):
    return model.config.eos_token_id
