"""`FiDT5.score` / `Engine.score` on a host without a GPU: the orchestration (one encoder pass, the [b, c, t] row order with c·T
cross-attention rows per sample, chunking over the candidates, isolation from a training step in flight) driven through the fp32 test
double and compared with the oracle run once per candidate; the argument checks of the Python surface; and the refusals of
lako_seq_logprob, which the built library makes on the host before any launch."""
import ctypes as C
import os
import subprocess

import pytest
import torch

from lako_amd import FiDT5, _lib
from oracle import fid_t5_oracle as O
from tests.ref_ops_score import RefOpsScore
from tests.test_engine_cpu import cfg_of
from tests.util_golden import load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the bound of the fp32 double-versus-oracle comparisons of tests/test_engine_cpu.py (logits, encoder output, scores)
TOL = dict(atol=5e-5, rtol=1e-4)


@pytest.fixture(scope="module", autouse=True)
def global_rng_as_found():
    """FiDT5() draws its initial weights from torch's global generator: hand the generator back as this module found it, so that a
    test that runs later and builds a model without seeding sees the stream it saw before this file existed"""
    state = torch.get_rng_state()
    yield
    torch.set_rng_state(state)


def build(dropout=0.0, **over):
    z, dims, w = load_case("tiny_a")
    cfg = cfg_of(dims, dropout)
    for k, v in over.items():
        setattr(cfg, k, v)
    model = FiDT5(cfg, dtype=torch.float32, _ops=RefOpsScore())
    if not over:
        model.load_t5(w)
    ids, mask, labels = (torch.from_numpy(z[k]) for k in ("input_ids", "attention_mask", "labels"))
    return z, dims, w, model, ids, mask, labels


def candidates_of(labels, V, T=4):
    """[B, 5, T]: the fixture's labels (their first T tokens), three random tails of differing length, one candidate all −100"""
    B = labels.shape[0]
    g = torch.Generator().manual_seed(11)
    cand = torch.randint(2, V, (B, 5, T), generator=g)
    cand[:, 0] = labels[:, :T]
    cand[:, 1, 3:] = -100
    cand[:, 2, 1:] = -100
    cand[0, 3, 2:] = -100
    cand[:, 4] = -100
    cand[1, 3, 0], cand[2, 3, 1] = 0, V - 1
    return cand


def oracle_scores(w, dims, ids, mask, cand):
    """the oracle once per candidate: log_softmax → gather → masked sum"""
    B, Cn, T = cand.shape
    score, n = torch.zeros(B, Cn), torch.zeros(B, Cn, dtype=torch.int32)
    for c in range(Cn):
        _, logits = O.fid_forward(w, dims, ids, mask, cand[:, c].contiguous())
        valid = cand[:, c] != -100
        lp = torch.log_softmax(logits.float(), -1).gather(2, cand[:, c].clamp(min=0)[..., None])[..., 0]
        score[:, c] = torch.where(valid, lp, torch.zeros_like(lp)).sum(1)
        n[:, c] = valid.sum(1)
    return score, n


@pytest.fixture(scope="module")
def case():
    z, dims, w, model, ids, mask, labels = build()
    cand = candidates_of(labels, dims.vocab_size)
    with torch.no_grad():
        want, n = oracle_scores(w, dims, ids, mask, cand)
    return dict(z=z, dims=dims, w=w, ids=ids, mask=mask, labels=labels, cand=cand, want=want, n=n)


def test_scores_match_the_oracle_run_per_candidate(case):
    _, _, _, model, ids, mask, _ = build()
    cand, want, n = case["cand"], case["want"], case["n"]
    B = ids.shape[0]
    model.train()                     # eval semantics whatever .training says (the config's dropout is 0 here; see the test below)
    got = model.score(ids, mask, cand)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, 5)
    torch.testing.assert_close(got, want, **TOL)
    assert torch.equal(got[:, 4], torch.zeros(B))                     # no valid label: 0
    sc, nv = model._engine.score(ids, mask, cand)
    assert nv.dtype == torch.int32 and torch.equal(nv, n)
    torch.testing.assert_close(model.score(ids, mask, cand, normalize=True), want / n.clamp(min=1), **TOL)
    for chunk in (1, 2, 5):
        torch.testing.assert_close(model.score(ids, mask, cand, candidate_chunk=chunk), want, **TOL)
    # one list for every question: [C, T] is broadcast
    shared = cand[1]
    with torch.no_grad():
        want_shared, _ = oracle_scores(case["w"], case["dims"], ids, mask, shared[None].expand(B, -1, -1))
    torch.testing.assert_close(model.score(ids, mask, shared), want_shared, **TOL)
    # 2-D (already flattened) inputs reuse the remembered n_passages; no mask = all valid
    torch.testing.assert_close(model.score(ids.view(B, -1), mask.view(B, -1), cand), want, **TOL)
    with torch.no_grad():
        want_all, _ = oracle_scores(case["w"], case["dims"], ids, torch.ones_like(mask), cand)
    torch.testing.assert_close(model.score(ids, None, cand), want_all, **TOL)


def test_the_fixtures_own_labels_score_what_its_recorded_logits_say(case):
    """the fixture's labels at their full length (T = 5) against the logits the reference recorded for them"""
    _, _, _, model, ids, mask, labels = build()
    logits = torch.from_numpy(case["z"]["logits"])
    valid = labels != -100
    lp = torch.log_softmax(logits, -1).gather(2, labels.clamp(min=0)[..., None])[..., 0]
    want = torch.where(valid, lp, torch.zeros_like(lp)).sum(1)
    torch.testing.assert_close(model.score(ids, mask, labels[:, None, :])[:, 0], want, **TOL)


def test_the_encoder_runs_once_per_call(case):
    _, _, _, model, ids, mask, _ = build()
    model.score(ids, mask, case["cand"])              # builds the engine
    eng, calls = model._engine, []
    inner = eng._encode
    eng._encode = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    got = model.score(ids, mask, case["cand"], candidate_chunk=2)       # C = 5 in chunks of 2, 2, 1
    assert len(calls) == 1
    torch.testing.assert_close(got, case["want"], **TOL)


def test_a_score_call_between_forward_and_backward_leaves_the_step_alone(case):
    """dropout on, training mode: the gradients of forward → score → backward equal those of forward → backward bit for bit, the step
    counter moves only with the backward, and `score` itself draws no dropout mask"""
    grads, scores = [], []
    for with_score in (True, False):
        _, _, w, model, ids, mask, labels = build(dropout=0.1)
        model.train()
        loss = model(input_ids=ids, attention_mask=mask, labels=labels)[0]
        eng = model._engine
        assert eng.step_count == 0
        if with_score:
            ctx = eng.ctx
            scores.append(model.score(ids, mask, case["cand"]))
            scores.append(model.score(ids, mask, case["cand"], candidate_chunk=2))
            assert eng.step_count == 0 and eng.ctx is ctx
        loss.backward()
        assert eng.step_count == 1
        grads.append(eng.G.clone())
    assert torch.equal(grads[0], grads[1])
    assert float(grads[0].abs().max()) > 0
    torch.testing.assert_close(scores[0], case["want"], **TOL)          # no dropout in `score`
    torch.testing.assert_close(scores[1], case["want"], **TOL)


def test_python_side_errors(case):
    _, dims, _, model, ids, mask, _ = build()
    bad = case["cand"].clone()
    bad[0, 1, 0] = dims.vocab_size
    with pytest.raises(ValueError, match="candidates"):
        model.score(ids, mask, bad)
    bad[0, 1, 0] = -1
    with pytest.raises(ValueError, match="candidates"):
        model.score(ids, mask, bad)
    with pytest.raises(ValueError, match="candidates"):
        model.score(ids, mask, case["cand"][:2])                      # neither [B, C, T] nor [C, T]
    fresh = build()[3]
    with pytest.raises(ValueError, match="n_passages"):
        fresh.score(ids.view(ids.shape[0], -1), mask.view(ids.shape[0], -1), case["cand"])
    legacy = build(legacy_cross_bias=True)[3]
    with pytest.raises(ValueError, match="legacy_cross_bias"):
        legacy.score(ids, mask, case["cand"])


# ---- the C-ABI entry ---------------------------------------------------------------------------------------------------
OK, E_BADARG, E_ALIGN = 0, -1, -2


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["bash", os.path.join(ROOT, "lako_amd", "csrc", "build.sh")], check=True)
    _lib._lib = None
    return _lib.load()


def test_seq_logprob_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "lako_hip.h")).read()
    assert "int lako_seq_logprob(const float* logits, const int64_t* labels, float* score, int32_t* n_valid, int64_t R, int T," in header
    assert "lako_seq_logprob" in _lib.SIGNATURES and len(_lib.SIGNATURES["lako_seq_logprob"]) == 8


def test_seq_logprob_refuses_bad_arguments_before_any_launch(L):
    """pointer VALUES that are never dereferenced, a null stream: every refusal happens on the host"""
    lg, lb, sc, nv = (C.c_void_p(0x100000000000 + i * 0x010000000000) for i in range(4))
    call = L.lako_seq_logprob
    for args in ((None, lb, sc, nv), (lg, None, sc, nv), (lg, lb, None, nv), (lg, lb, sc, None)):
        assert call(*args, 3, 5, 32128, None) == E_BADARG
    for R, T, V in ((0, 5, 32128), (-1, 5, 32128), (3, 0, 32128), (3, -2, 32128), (3, 5, 0), (3, 5, -4)):
        assert call(lg, lb, sc, nv, R, T, V, None) == E_BADARG, (R, T, V)
    buf = C.create_string_buffer(256)
    assert L.lako_last_error(buf, 256) > 0 and b"lako_seq_logprob" in buf.value
    assert call(C.c_void_p(lg.value + 4), lb, sc, nv, 3, 5, 32128, None) == E_ALIGN       # logits not 16-byte aligned
    assert call(C.c_void_p(lg.value + 8), lb, sc, nv, 3, 5, 32128, None) == E_ALIGN
    for V in (32127, 32130, 6):
        assert call(lg, lb, sc, nv, 3, 5, V, None) == E_ALIGN, V                          # V % 4 != 0
    assert call(None, lb, sc, nv, 3, 5, 6, None) == E_BADARG                              # null pointers come first
