"""Beam search (`FiDT5.generate(num_beams=K)`) on a host without a GPU: the engine's orchestration — K beams as K decoder rows over one
encoder pass, cache sets alternating by step parity, the finished set read back once — on the CPU test double (tests/ref_ops_beam.py),
against what transformers' own beam search returned for the reference model (tests/golden/beam_hf.npz, written by
tools/make_beam_fixture.py).  The kernels themselves are compared with the same double in tests/test_beam_gpu.py."""
import json
import os

import numpy as np
import pytest
import torch

from lako_amd import FiDT5
from tests.ref_beam import beam_search, oracle_logits
from tests.ref_ops_beam import RefOpsBeam
from tests.test_engine_cpu import cfg_of
from tests.util_golden import GOLDEN, load_case

HF = np.load(os.path.join(GOLDEN, "beam_hf.npz"))
CASES = [(i, int(c[0]), float(c[1]), bool(c[2]), int(c[3])) for i, c in enumerate(HF["cases"])]


@pytest.fixture(scope="module", autouse=True)
def global_rng_as_found():
    state = torch.get_rng_state()
    yield
    torch.set_rng_state(state)


def build(name="tiny_eos", **over):
    z, dims, w = load_case(name)
    cfg = cfg_of(dims)
    for k, v in over.items():
        setattr(cfg, k, v)
    model = FiDT5(cfg, dtype=torch.float32, _ops=RefOpsBeam())
    if not over:
        model.load_t5(w)
    model.eval()
    return z, model, torch.from_numpy(z["input_ids"]), torch.from_numpy(z["attention_mask"])


def check_against_hf(i, K, lpen, toks, raw, eos=1, pad=0, tol=1e-4):
    """tokens up to and including the first EOS as HF's, pad behind it, HF's width, raw / len**length_penalty within tol of HF's score"""
    want, want_sc = HF[f"tokens_{i}"], HF[f"scores_{i}"]
    B = want.shape[0]
    width = int((want >= 0).sum(-1).max())
    assert toks.dtype == torch.int64 and tuple(toks.shape) == (B * K, width), (tuple(toks.shape), width)
    assert raw.dtype == torch.float32 and tuple(raw.shape) == (B, K)
    worst = 0.0
    for b in range(B):
        for k in range(K):
            row = [int(v) for v in want[b, k] if v >= 0]
            n = row.index(eos, 1) + 1 if eos in row[1:] else len(row)
            got = toks[b * K + k].tolist()
            assert got[:n] == row[:n], (b, k, got, row)
            assert all(v == pad for v in got[n:]), (b, k, got)
            worst = max(worst, abs(float(raw[b, k]) / (n - 1) ** lpen - float(want_sc[b, k])))
    assert worst <= tol, worst
    return worst


@pytest.mark.parametrize("i,K,lpen,early,ML", CASES)
def test_the_engine_reproduces_transformers_beam_search(i, K, lpen, early, ML):
    z, model, ids, mask = build()
    toks, raw = model.generate(ids, mask, ML, num_beams=K, num_return_sequences=K, length_penalty=lpen, early_stopping=early,
                               return_scores=True)
    worst = check_against_hf(i, K, lpen, toks, raw)
    print(f"K={K} length_penalty={lpen} early_stopping={early} max_length={ML}: max |raw / len**lp - HF score| {worst:.3e}")
    # the returned raw sums are what score gives for the returned sequences
    cand = toks[:, 1:].clone()
    is_eos = cand == 1
    cand[(is_eos.cumsum(1) - is_eos.long()) > 0] = -100
    sc = model.score(ids, mask, cand.view(ids.shape[0], K, -1))
    assert float((sc - raw).abs().max()) <= 1e-4


def test_the_plain_restatement_agrees_with_the_fixture():
    """tests/ref_beam.py, the independent float64 statement of the semantics, on the oracle's logits"""
    z, dims, w = load_case("tiny_eos")
    ids, mask = torch.from_numpy(z["input_ids"]), torch.from_numpy(z["attention_mask"])
    logits = oracle_logits(w, dims, ids, mask)
    i, K, lpen, early, ML = CASES[1]
    fin = beam_search(logits, ids.shape[0], K, ML, lpen, early)
    for b in range(ids.shape[0]):
        for k in range(K):
            row = [int(v) for v in HF[f"tokens_{i}"][b, k] if v >= 0]
            n = row.index(1, 1) + 1 if 1 in row[1:] else len(row)
            assert fin[b][k][0] == row[:n] and abs(fin[b][k][1] - float(HF[f"scores_{i}"][b, k])) <= 1e-4


def test_fewer_returned_sequences_are_the_first_rows_and_one_beam_is_greedy():
    z, model, ids, mask = build()
    B, K = ids.shape[0], 4
    full, fs = model.generate(ids, mask, 8, num_beams=K, num_return_sequences=K, return_scores=True)
    for R in (1, 2):
        part, ps = model.generate(ids, mask, 8, num_beams=K, num_return_sequences=R, return_scores=True)
        want = full.view(B, K, -1)[:, :R]
        width = int((want != 0).sum(-1).max()) + 1          # (pad is 0 and sits only in column 0 and behind a row's end)
        assert tuple(part.shape) == (B * R, width)
        assert torch.equal(part.view(B, R, -1), want[:, :, :width]) and not bool(want[:, :, width:].any())
        assert torch.equal(ps, fs[:, :R])
    assert tuple(model.generate(ids, mask, 8, num_beams=K).shape)[0] == B          # R defaults to 1: the best hypothesis
    for ml in (4, 12):
        assert torch.equal(model.generate(ids, mask, ml, num_beams=1), torch.from_numpy(z[f"gen_{ml}"]))


def test_a_question_alone_and_inside_a_batch_returns_the_same_hypotheses():
    z, model, ids, mask = build()
    B, K = ids.shape[0], 3
    toks, raw = model.generate(ids, mask, 8, num_beams=K, num_return_sequences=K, return_scores=True)
    rows = toks.view(B, K, -1)
    for b in range(B):
        alone, ar = model.generate(ids[b:b + 1], mask[b:b + 1], 8, num_beams=K, num_return_sequences=K, return_scores=True)
        n = alone.shape[1]                                  # (a batch is cropped to ITS longest row)
        assert torch.equal(alone, rows[b, :, :n]) and not bool(rows[b, :, n:].any())
        assert float((ar[0] - raw[b]).abs().max()) <= 1e-5


def test_the_settings_live_in_device_memory_and_the_state_is_rebuilt_per_call():
    """two calls with other settings through one workspace, then the first again: the same result as a fresh model's"""
    z, model, ids, mask = build()
    a = model.generate(ids, mask, 8, num_beams=3, num_return_sequences=3, length_penalty=2.0)
    model.generate(ids, mask, 8, num_beams=3, num_return_sequences=3, length_penalty=0.0, early_stopping=True)
    assert torch.equal(a, model.generate(ids, mask, 8, num_beams=3, num_return_sequences=3, length_penalty=2.0))


def test_argument_errors_raise_before_anything_runs():
    class Untouchable:
        def __getattr__(self, n):
            raise AssertionError(f"op {n} reached")
    z, model, ids, mask = build("tiny_a")
    model._get_engine().ops = Untouchable()
    bad = [dict(num_beams=17), dict(num_beams=0), dict(num_beams=2, do_sample=True), dict(num_beams=2, num_return_sequences=3),
           dict(num_beams=2, early_stopping="never"), dict(num_beams=2, early_stopping=1), dict(num_return_sequences=2)]
    for kw in bad:
        with pytest.raises(ValueError):
            model.generate(ids, mask, 4, **kw)
    small = build("tiny_a", vocab_size=8)[1]
    small._get_engine().ops = Untouchable()
    with pytest.raises(ValueError, match="vocab_size"):
        small.generate(ids % 8, mask, 4, num_beams=5)
    model.overwrite_forward_crossattention()
    model.reset_score_storage()
    with pytest.raises(ValueError, match="captured"):
        model.generate(ids, mask, 4, num_beams=2)
    z, legacy, ids, mask = build("tiny_a", legacy_cross_bias=True)
    legacy._get_engine().ops = Untouchable()
    with pytest.raises(ValueError, match="legacy_cross_bias"):
        legacy.generate(ids, mask, 4, num_beams=2)


@pytest.fixture
def generation_defaults_as_found():
    found = FiDT5.generation_defaults
    yield
    FiDT5.generation_defaults = found


def spy_on_generate(model, seen):
    """record the decoding arguments that reach the engine"""
    eng = model._get_engine()
    plain = eng.generate

    def spy(*a, **kw):
        seen.append({k: v for k, v in kw.items() if k in ("num_beams", "length_penalty", "num_return_sequences")})
        return plain(*a, **kw)
    eng.generate = spy


def test_the_training_drivers_evaluation_decodes_with_the_beams_it_is_given(generation_defaults_as_found):
    """train_reader.py --num_beams K --length_penalty p: the flags parse (defaults: the greedy decode) into the model's generation
    defaults, and its evaluate() scores the best hypothesis of a beam search with those settings"""
    import train_reader
    from lako_amd.options import Options
    chain = lambda: Options().add_reader_options().add_optim_options().add_decode_options()      # noqa: E731  (train_reader.py's)
    opt = chain().parse([])
    assert (opt.num_beams, opt.length_penalty) == (1, 1.0) and FiDT5.generation_defaults == {}
    z, model, ids, mask = build()
    best = model.generate(ids, mask, 50, num_beams=3, length_penalty=2.0)
    labels = torch.full((ids.shape[0], best.shape[1]), -100, dtype=torch.int64)
    labels[:, :best.shape[1] - 1] = best[:, 1:]             # the beam search's best hypotheses as the gold answers
    batch = dict(idx=None, ids=ids, mask=mask, labels=labels, lens=None)
    seen = []
    spy_on_generate(model, seen)
    opt = chain().parse(["--num_beams", "3", "--length_penalty", "2"])
    assert (opt.num_beams, opt.length_penalty) == (3, 2.0) and FiDT5.generation_defaults == dict(num_beams=3, length_penalty=2.0)
    opt.is_distributed = False
    assert train_reader.evaluate(model, [batch], opt) == 1.0
    assert torch.equal(model.generate(ids, mask, 50, num_beams=1), torch.from_numpy(z["gen_12"]))      # an explicit argument wins
    opt = chain().parse([])                                  # one beam: the call the driver always made
    opt.is_distributed = False
    train_reader.evaluate(model, [batch], opt)
    assert [s_.get("num_beams", 1) for s_ in seen] == [3, 1, 1] and seen[0]["length_penalty"] == 2.0 and seen[2] == {}


def test_the_evaluation_driver_takes_the_flags_and_refuses_them_with_score_capture(tmp_path, generation_defaults_as_found):
    """test_reader.py --num_beams K --length_penalty p (its option chain): evaluate() decodes with the beams and scores the best hypothesis
    — one answer per question; with --write_crossattention_scores the flags are refused when they are parsed, before anything runs, and
    a model that captures scores refuses beams too"""
    import copy
    import importlib.util
    import types

    from torch.utils.data import DataLoader, SequentialSampler

    from lako_amd import FiDConfig
    from lako_amd.data import Collator, Dataset
    from lako_amd.options import Options
    from tests.stub_tokenizer import StubTokenizer
    from tests.test_data_pipeline import EXAMPLES
    spec = importlib.util.spec_from_file_location("reader_eval", os.path.join(os.path.dirname(__file__), "..", "test_reader.py"))
    tr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tr)
    chain = lambda: Options().add_reader_options().add_eval_options().add_optim_options()        # noqa: E731  (test_reader.py's)
    opt = chain().parse([])
    assert (opt.num_beams, opt.length_penalty) == (1, 1.0) and FiDT5.generation_defaults == {}
    with pytest.raises(ValueError, match="write_crossattention_scores"):
        chain().parse(["--num_beams", "2", "--write_crossattention_scores"])
    with pytest.raises(ValueError, match="num_beams"):
        chain().parse(["--num_beams", "0"])
    assert FiDT5.generation_defaults == {}
    chain().parse(["--write_crossattention_scores"])        # alone it stays what it was

    cfg = FiDConfig(vocab_size=64, d_model=32, d_kv=32, d_ff=64, num_layers=2, num_decoder_layers=2, num_heads=2, dropout_rate=0.0)
    model = FiDT5(cfg, dtype=torch.float32, seed=3, _ops=RefOpsBeam())
    seen = []
    spy_on_generate(model, seen)
    results = {}
    for flags in ([], ["--num_beams", "4", "--length_penalty", "0.5"]):
        parsed = chain().parse(flags)
        opt = types.SimpleNamespace(n_context=2, fact_use_way="concate", use_fact="yes", stream=2, write_results=True,
                                    write_crossattention_scores=False, ans_attention="no", attention_score_style="mean",
                                    use_last_half_layer_attention="no", dataset="okvqa", model_size="tiny", per_gpu_batch_size=2,
                                    text_maxlength=24, is_distributed=False, eval_data="dev.json", version="v1", device="cpu",
                                    num_beams=parsed.num_beams, length_penalty=parsed.length_penalty)
        ds = Dataset(copy.deepcopy(EXAMPLES), opt)
        tok = StubTokenizer()
        dl = DataLoader(ds, sampler=SequentialSampler(ds), batch_size=2, collate_fn=Collator(24, tok, stream=2))
        out = tmp_path / f"beams{parsed.num_beams}"
        em, stem_em, inc_em, total = tr.evaluate(model, ds, dl, tok, opt, str(out))
        assert total == 3                                    # one scored answer per question: the best hypothesis
        results[parsed.num_beams] = json.load(open(out / "test_results" / os.listdir(out / "test_results")[0]))
    assert [s_.get("num_beams", 1) for s_ in seen] == [1, 1, 4, 4] and seen[2]["length_penalty"] == 0.5 and seen[0] == {}
    assert len(results[4]) == 3 and all(isinstance(r["answer"], str) for r in results[4])
    # what the driver decoded is the best hypothesis of the same call made by hand
    batch = next(iter(dl))
    by_hand = model.generate(input_ids=batch[3], attention_mask=batch[4], max_length=50, num_beams=4, length_penalty=0.5)
    assert tok.batch_decode(by_hand, skip_special_tokens=True) == [r["answer"] for r in results[4][:2]]
    # a model that captures the cross-attention scores refuses beams, whichever way they arrive
    model.overwrite_forward_crossattention()
    model.reset_score_storage()
    with pytest.raises(ValueError, match="captured"):
        model.generate(input_ids=batch[3], attention_mask=batch[4], max_length=50)


def test_further_argument_errors(generation_defaults_as_found):
    class Untouchable:
        def __getattr__(self, n):
            raise AssertionError(f"op {n} reached")
    z, model, ids, mask = build("tiny_a")
    model._get_engine().ops = Untouchable()
    for kw in (dict(num_beams="many"), dict(num_beams=2.5), dict(num_beams=None, length_penalty="x"), dict(num_beams=True)):
        FiDT5.generation_defaults = dict(num_beams=2) if kw["num_beams"] is None else {}
        with pytest.raises(ValueError):
            model.generate(ids, mask, 4, **kw)
    FiDT5.generation_defaults = {}
