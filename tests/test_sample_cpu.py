"""Sampled decoding (`FiDT5.generate(do_sample=True, …, num_return_sequences=K)`) on a host without a GPU: the orchestration — K decoder
rows per question over ONE copy of the question's encoder states, the sampler's parameters, the scores, the argument checks — driven
through the fp32 test double (tests/ref_ops_sample.py, which holds the torch restatement of lako_sample_step) and compared with the
reference's recorded greedy tokens (top_k = 1 makes every sampled row the greedy decode) and with `FiDT5.score`."""
import json
import os

import pytest
import torch

from lako_amd import FiDT5
from tests.ref_ops import RefOps
from tests.ref_ops_sample import SWEEP_V, RefOpsSample, draw_u24, sample_row, sweep_cases
from tests.test_engine_cpu import CASES, cfg_of
from tests.util_golden import load_case

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module", autouse=True)
def global_rng_as_found():
    """FiDT5() draws its initial weights from torch's global generator (and seed=None draws a seed from it): hand it back as found"""
    state = torch.get_rng_state()
    yield
    torch.set_rng_state(state)


def build(name, ops=None, **over):
    z, dims, w = load_case(name)
    cfg = cfg_of(dims)
    for k, v in over.items():
        setattr(cfg, k, v)
    model = FiDT5(cfg, dtype=torch.float32, _ops=ops or RefOpsSample())
    if not over:
        model.load_t5(w)
    model.eval()
    return z, model, torch.from_numpy(z["input_ids"]), torch.from_numpy(z["attention_mask"])


def as_candidates(tokens, B, K, eos=1):
    """generated rows [B·K, n] (start token first) → candidates [B, K, n − 1] with −100 after each row's EOS"""
    cand = tokens[:, 1:].clone()
    is_eos = cand == eos
    after = (is_eos.cumsum(1) - is_eos.long()) > 0
    cand[after] = -100
    return cand.view(B, K, -1)


@pytest.mark.parametrize("name", CASES)
def test_top_k_1_makes_every_sampled_row_the_reference_greedy_decode(name):
    """K = 3 rows per question over the question's one set of encoder states; the early-EOS rows of tiny_eos included"""
    z, model, ids, mask = build(name)
    for ml, seed in ((4, 0), (12, 123456789012345)):
        toks = model.generate(ids, mask, ml, do_sample=True, top_k=1, num_return_sequences=3, seed=seed)
        want = torch.from_numpy(z[f"gen_{ml}"])
        assert toks.dtype == torch.int64 and tuple(toks.shape) == (3 * ids.shape[0], want.shape[1])
        assert torch.equal(toks.view(ids.shape[0], 3, -1), want[:, None].expand(-1, 3, -1))


@pytest.mark.parametrize("route", ["projected", "unfused", "one_pass"])
def test_the_three_cross_attention_routes_decode_the_same_rows(route, monkeypatch):
    """the double takes the encoder-state routes too: K·H rows per sample through the unfused ops, K tiles through xattn_decode_multi"""
    if route != "projected":
        monkeypatch.setenv("LAKO_XATTN_GENERATE", "1")
        monkeypatch.setenv("LAKO_XATTN_DECODE", "0" if route == "unfused" else "1")
    z, model, ids, mask = build("mid_a")
    toks = model.generate(ids, mask, 12, do_sample=True, top_k=1, num_return_sequences=3, seed=1)
    assert model._engine.xattn_active == (route != "projected")
    assert torch.equal(toks.view(ids.shape[0], 3, -1), torch.from_numpy(z["gen_12"])[:, None].expand(-1, 3, -1))


@pytest.mark.parametrize("name", ["tiny_a", "tiny_eos"])
def test_returned_scores_are_what_score_gives_for_the_same_sequences(name):
    z, model, ids, mask = build(name)
    B = ids.shape[0]
    toks, sc = model.generate(ids, mask, 12, do_sample=True, temperature=1.5, top_k=0, top_p=0.9, num_return_sequences=4, seed=7,
                              return_scores=True)
    assert sc.dtype == torch.float32 and tuple(sc.shape) == (B, 4) and toks.shape[0] == 4 * B
    want = model.score(ids, mask, as_candidates(toks, B, 4))
    print(f"{name}: sampled max |score - model.score| {float((sc - want).abs().max()):.3e}")
    assert float((sc - want).abs().max()) <= 1e-5
    # greedy with scores: the tokens are the greedy decode's
    gt, gs = model.generate(ids, mask, 12, return_scores=True)
    assert torch.equal(gt, torch.from_numpy(z["gen_12"])) and tuple(gs.shape) == (B, 1)
    want = model.score(ids, mask, as_candidates(gt, B, 1))
    print(f"{name}: greedy max |score - model.score| {float((gs - want).abs().max()):.3e}")
    assert float((gs - want).abs().max()) <= 1e-5


def test_seeds_decide_the_tokens_and_a_question_does_not_see_its_batch():
    """The draw of row (b, k) at step t is a hash of (seed, k, t): the kernel is told K and hashes r mod K, so question b's rows do not
    depend on b — cut the batch to question b alone and its K rows come out unchanged."""
    z, model, ids, mask = build("mid_a")
    B, K = ids.shape[0], 3
    kw = dict(do_sample=True, temperature=2.0, num_return_sequences=K)
    a = model.generate(ids, mask, 12, seed=11, **kw)
    assert torch.equal(a, model.generate(ids, mask, 12, seed=11, **kw))
    assert not torch.equal(a, model.generate(ids, mask, 12, seed=12, **kw))
    rows = a.view(B, K, -1)
    assert len({tuple(r.tolist()) for r in rows[0]}) > 1                    # temperature 2: a question's rows differ from each other
    for b in range(B):
        alone = model.generate(ids[b:b + 1], mask[b:b + 1], 12, seed=11, **kw)
        n = min(alone.shape[1], rows.shape[2])                              # (a batch runs until its last row ends: compare what both hold)
        assert torch.equal(alone[:, :n], rows[b, :, :n])
        assert not bool(alone[:, n:].any()) and not bool(rows[b, :, n:].any())
    # seed=None draws the seed from torch's global generator: reproducible through torch.manual_seed
    torch.manual_seed(5)
    c = model.generate(ids, mask, 12, **kw)
    torch.manual_seed(5)
    assert torch.equal(c, model.generate(ids, mask, 12, **kw))


def test_argument_errors_raise_before_anything_runs():
    class Untouchable:
        def __getattr__(self, n):
            raise AssertionError(f"op {n} reached")
    z, model, ids, mask = build("tiny_a")
    model._get_engine().ops = Untouchable()
    bad = [dict(do_sample=True, temperature=0.0), dict(do_sample=True, temperature=-1.0), dict(do_sample=True, top_p=0.0),
           dict(do_sample=True, top_p=1.5), dict(do_sample=True, top_k=-1), dict(do_sample=True, num_return_sequences=0),
           dict(num_return_sequences=2)]
    for kw in bad:
        with pytest.raises(ValueError):
            model.generate(ids, mask, 4, **kw)
    model.overwrite_forward_crossattention()
    model.reset_score_storage()
    with pytest.raises(ValueError, match="captured"):
        model.generate(ids, mask, 4, do_sample=True)
    z, legacy, ids, mask = build("tiny_a", legacy_cross_bias=True)
    legacy._get_engine().ops = Untouchable()
    with pytest.raises(ValueError, match="legacy_cross_bias"):
        legacy.generate(ids, mask, 4, do_sample=True, num_return_sequences=2)


@pytest.mark.parametrize("V", SWEEP_V)
def test_the_kernel_sweep_leaves_out_at_most_one_row_in_a_hundred(V):
    """the sweep tests/test_sample_gpu.py compares the kernel on, with the seeds it picks: the restatement alone must call at least 99 %
    of its rows decidable (undecidable rows are not compared with the kernel)"""
    cases = list(sweep_cases(V))
    total, undecided = sum(c["want"].numel() for c in cases), sum(int((~c["dec"]).sum()) for c in cases)
    print(f"V={V}: {total} rows, {undecided} undecidable")
    assert total == 540 and undecided <= 0.01 * total


class _Log:
    """records the name of every op the engine calls"""
    def __init__(self, inner):
        self._i, self.names = inner, []

    def __getattr__(self, n):
        v = getattr(self._i, n)
        if callable(v) and not n.startswith("_") and not n.endswith("_ok"):
            def w(*a, **k):
                self.names.append(n)
                return v(*a, **k)
            return w
        return v


def test_a_default_generate_issues_the_ops_it_issued_before_sampling_existed():
    """tests/golden/generate_default_ops.json: the op names of `generate(ids, mask, max_length)` recorded with this very proxy on the
    commit before sampled decoding (plain RefOps, which has no sample_step at all)"""
    with open(os.path.join(GOLDEN, "generate_default_ops.json")) as fh:
        want = json.load(fh)
    for name, ml in (("tiny_a", 4), ("tiny_eos", 12)):
        ops = _Log(RefOps())
        z, model, ids, mask = build(name, ops=ops)
        ops.names.clear()
        toks = model.generate(ids, mask, ml)
        assert ops.names == want[f"{name}_{ml}"]
        assert toks.tolist() == z[f"gen_{ml}"].tolist()
        assert all(len(k) == 5 for k in model._engine._ws_cache if k[0] == "gen")      # the workspace key of before


def engine_call_ops():
    """{call: op names} of a training step with dropout, a sampled generate with K = 3 and scores, and a chunked score on tiny_a"""
    ops = _Log(RefOpsSample())
    z, model, ids, mask = build("tiny_a", ops=ops)
    model.config.dropout_rate = 0.1
    got = {}
    ops.names.clear()
    model.train()
    model(input_ids=ids, attention_mask=mask, labels=torch.from_numpy(z["labels"]))[0].backward()
    model.eval()
    got["forward_backward"] = list(ops.names)
    ops.names.clear()
    model.generate(ids, mask, 6, do_sample=True, top_k=3, num_return_sequences=3, seed=7, return_scores=True)
    got["generate_sampled"] = list(ops.names)
    ops.names.clear()
    cand = torch.randint(2, model.config.vocab_size, (ids.shape[0], 3, 4), generator=torch.Generator().manual_seed(29))
    cand[:, 1, 3:] = -100
    model.score(ids, mask, cand, candidate_chunk=2)      # a full chunk and the smaller tail chunk
    got["score"] = list(ops.names)
    return got


def test_the_engines_public_calls_issue_the_ops_they_issued_before_the_engine_was_cut_into_parts():
    """tests/golden/engine_ops.json: the op names of engine_call_ops() recorded with this very proxy on the commit before
    forward_loss / score / generate came to share their batch prologue, decoder set-up and norm + projection helper"""
    with open(os.path.join(GOLDEN, "engine_ops.json")) as fh:
        want = json.load(fh)
    got = engine_call_ops()
    assert sorted(got) == sorted(want)
    for call, names in got.items():
        assert names == want[call], call


@pytest.mark.parametrize("fixture", ["tiny_a", "tiny_eos", "gated_tiny", "legacy_cross_bias"])
def test_backward_issues_the_ops_it_issued_before_it_was_cut_into_parts(fixture):
    """tests/golden/engine_bwd_ops.json: the op names of one forward + backward under every switch and state that makes backward branch
    (tools/op_trace.py's backward variants, the places of the gradient hook's notifications among them), recorded with the tool's own
    proxy on the commit before Engine.backward came to be a sequence of parts with one feed-forward backward for both stacks"""
    from tools.op_trace import BWD_FIXTURES, cpu_backward_matrix, read_names
    want = {key: names for key, names in read_names(os.path.join(GOLDEN, "engine_bwd_ops.json")).items()
            if key.startswith(fixture + "|") or "+" + fixture in key}
    got = {key: [r[0] for r in rec["ops"]] for key, rec in cpu_backward_matrix({}, names_only=True, only=fixture).items()}
    assert fixture in BWD_FIXTURES and sorted(got) == sorted(want) and len(got) == {"tiny_a": 12, "tiny_eos": 12, "gated_tiny": 1}.get(fixture, 2)
    assert fixture not in ("tiny_a", "tiny_eos") or sum("grad_ready" in names for names in got.values()) == 2
    for key, names in got.items():
        assert names == want[key], key


def test_the_restatement_follows_the_definition_on_a_hand_made_row():
    x = torch.tensor([0.0, 2.0, 2.0, -float("inf"), 1.0, float("nan")])
    # top_k = 1: the first of the two maxima, whatever the draw
    assert all(sample_row(x, 1.0, 1, 1.0, u)[0] == 1 for u in (0, 2 ** 23, 2 ** 24 - 1))
    # top_k = 2: both maxima, half the mass each
    assert sample_row(x, 1.0, 2, 1.0, 2 ** 23 - 1)[0] == 1 and sample_row(x, 1.0, 2, 1.0, 2 ** 23)[0] == 2
    # a nucleus of 0.05: at least one token, the first maximum
    assert sample_row(x, 1.0, 0, 0.05, 2 ** 24 - 1)[0] == 1
    # no truncation: the last draw lands on the last token with mass (index 4), never on −∞ / NaN
    assert sample_row(x, 1.0, 0, 1.0, 2 ** 24 - 1)[0] == 4 and sample_row(x, 1.0, 0, 1.0, 0)[0] == 0
    tok, lp, _ = sample_row(x, 0.7, 0, 1.0, 0)
    assert abs(lp - float(torch.log_softmax(torch.tensor([0.0, 2.0, 2.0, 1.0], dtype=torch.float64), 0)[0])) < 1e-12
    assert sample_row(torch.full((4,), float("nan")), 1.0, 0, 1.0, 5)[0] == 0
    assert draw_u24(1, 0, 0) != draw_u24(1, 1, 0) != draw_u24(1, 1, 1) and 0 <= draw_u24(2 ** 63 + 5, 7, 3) < 2 ** 24
