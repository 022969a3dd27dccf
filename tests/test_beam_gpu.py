"""-m gpu: beam search on the HIP path — lako_beam_rows + lako_beam_merge against their restatement (tests/ref_ops_beam.py) on the same
logits and state, lako_beam_gather against index_select, and FiDT5.generate(num_beams=K) against transformers' beam search
(tests/golden/beam_hf.npz), against itself across the eager / capture / replay calls and the three cross-attention routes, and against
FiDT5.score."""
import numpy as np
import pytest
import torch

from tests.ref_ops_beam import merge_ref, pack_beam_params, rows_ref
from tests.test_beam_cpu import CASES, check_against_hf
from tests.test_sample_cpu import as_candidates
from tests.test_sample_gpu import d512_model, fixture_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
NAN = float("nan")
MARGIN = 1e-4           # no two values the rules compare are closer than this (the seeds are picked for it, on the CPU)
SCORE_RTOL = 2e-6
LD = 9                  # token columns of the kernel tests: max_length 9, so that step 7 is the last
STEPS = (0, 4, 7)       # the first, a middle and the last step
SWEEP = [(V, K, B) for V in (7, 256, 257, 32128, 40000) for K in (2, 3, 4, 8, 16) if 2 * K <= V for B in (1, 3)]


@pytest.fixture(scope="module", autouse=True)
def global_rng_as_found():
    state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(DEV)
    yield
    torch.set_rng_state(state)
    torch.cuda.set_rng_state(dev_state, DEV)


@pytest.fixture(scope="module")
def ops():
    from lako_amd.ops import HipOps
    return HipOps()


# ---- lako_beam_rows + lako_beam_merge ----------------------------------------------------------------------------------------------
def beam_logits(rows, V, g):
    """3·randn with a −∞ column, a NaN, exact duplicates of the maximum (the ascending-index tie rule) and, in every other row, EOS (id 1)
    right behind them — so that ending candidates reach the first K"""
    x = torch.randn(rows, V, generator=g) * 3.0
    top = x.max(1).values
    x[:, V - 1] = top                       # a second maximum behind the first …
    if V > 16:
        x[:, 5] = top                       # … and one in front of it
        x[:, V // 3] = -INF
        x[:, V // 2] = NAN
    x[::2, 1] = top[::2] - 0.25
    return x


def beam_state(B, K, step, g):
    """running scores sorted best first ([0, −1e9, …] at step 0), token rows, and a finished set per question: none filled / K − 1 filled /
    all filled and the question closed (B = 3), or all filled and still open (B = 1)"""
    BK, pos = B * K, step + 1
    run = -torch.sort(torch.rand(B, K, generator=g) * 4.0 + 0.5, dim=1).values
    if step == 0:
        run = torch.full((B, K), -1.0e9)
        run[:, 0] = 0.0
    seq = torch.zeros(BK, LD, dtype=torch.int64)
    seq[:, 1:pos] = torch.randint(2, 7, (BK, pos - 1), generator=g)
    fin = torch.randint(2, 7, (BK, LD), generator=g)
    fin_score = -torch.sort(torch.rand(B, K, generator=g) * 3.0 + 0.05, dim=1).values
    fin_raw = fin_score * 3.0
    fin_len = torch.randint(2, LD + 1, (BK,), generator=g).to(torch.int32)
    filled = torch.zeros(B, K, dtype=torch.uint8)
    open_ = torch.ones(B, dtype=torch.uint8)
    if B == 1:
        filled[0] = 1
    else:
        filled[1, :K - 1] = 1
        filled[2] = 1
        open_[2] = 0
    empty = ~filled.reshape(BK).bool()               # an unfilled slot is all zero, as the engine leaves it
    fin[empty] = 0
    fin_len[empty] = 0
    fin_score, fin_raw = fin_score.reshape(BK).clone(), fin_raw.reshape(BK).clone()
    fin_score[empty] = 0.0
    fin_raw[empty] = 0.0
    return dict(run=run.reshape(BK).float(), seq=seq, fin=fin, fin_score=fin_score.reshape(BK).float(), fin_raw=fin_raw.reshape(BK).float(),
                fin_len=fin_len, fin_filled=filled.reshape(BK), open=open_)


def decidable(acc, tok, st, K, pos, lpen, last, eos=1):
    """Every comparison of the merge has a margin.  (a) Adjacent candidates among the best 2K + 1 are further apart than MARGIN, unless they
    are exact duplicates inside one row, which the index rule orders (both sides compute them to the same bits).  (b) Every one of the
    best 2K, normalised, is further than MARGIN from every filled finished score: that covers the offers against the finished set and
    the best running beam against an old worst score.  (c) The comparison that closes a question, best running beam against the worst
    finished score, where that worst score is an offer of this very step: two different candidates over the same norm, so their
    distance is that of (a) divided by the norm — asserted here as such, MARGIN / norm (norm <= 64; the values are of order 1 and fp32
    resolves 1e-7 of them)."""
    B = acc.shape[0] // K
    C = 2 * K
    norm = float(np.float32(pos) ** np.float32(lpen))
    for b in range(B):
        cands = sorted((-float(a), k, int(t)) for k in range(K) for a, t in zip(acc[b * K + k].tolist(), tok[b * K + k].tolist()))
        for (a0, k0, _), (a1, k1, _) in zip(cands[:C], cands[1:C + 1]):
            if not (a1 - a0 > MARGIN or (a0 == a1 and k0 == k1)):
                return False
        fs = st["fin_score"][b * K:(b + 1) * K][st["fin_filled"][b * K:(b + 1) * K].bool()].tolist()
        for a, _, _ in cands[:C]:
            if any(abs(-a / norm - f) <= MARGIN for f in fs):
                return False
        ends = [last or t == eos for _, _, t in cands[:C]]
        best = next((c for c, e in zip(cands[:C], ends) if not e), cands[0])
        for j, (c, e) in enumerate(zip(cands[:K], ends[:K])):
            if e and c is not best and not (abs(c[0] - best[0]) / norm > MARGIN / norm or (c[0] == best[0] and c[1] == best[1])):
                return False
    return True


def build_case(V, K, B):
    """logits, states and the restatement's verdicts for every (step, early_stopping, length_penalty) of one (V, K, B); the seed is the
    first of 32 for which every one of them is decidable — none is skipped"""
    for seed in range(32):
        g = torch.Generator().manual_seed(1000 * V + 10 * K + B + 7919 * seed)
        x = beam_logits(B * K, V, g)
        subs, ok = [], True
        for step in STEPS:
            st = beam_state(B, K, step, g)
            acc, tok = rows_ref(x, st["run"], 2 * K)
            for lpen in (0.0, 1.0, 2.0):
                ok = ok and decidable(acc, tok, st, K, step + 1, lpen, step == STEPS[-1])
                for early in (False, True):
                    want = merge_ref(acc, tok, st["seq"], st["fin"], step + 1, step == STEPS[-1], st["run"], st["fin_score"], st["fin_raw"],
                                     st["fin_len"], st["fin_filled"], st["open"], lpen, early)
                    subs.append((step, lpen, early, st, acc, tok, want))
        if ok:
            return x, subs
    raise AssertionError(f"V={V} K={K} B={B}: no decidable seed among 32")


def close(got, want, what):
    got, want = got.cpu().double(), want.cpu().double()
    same = (got == want) | ((got - want).abs() <= SCORE_RTOL * want.abs())
    assert bool(same.all()), (what, got.tolist(), want.tolist())
    fin = torch.isfinite(want) & (want != 0)
    return float(((got - want).abs() / want.abs())[fin].max()) if bool(fin.any()) else 0.0


@pytest.mark.parametrize("V,K,B", SWEEP)
def test_rows_and_merge_follow_the_restatement(ops, V, K, B):
    x, subs = build_case(V, K, B)
    BK, C = B * K, 2 * K
    xd = x.to(DEV)
    worst = 0.0
    for step, lpen, early, st, acc, tok, want in subs:
        what = f"V={V} K={K} B={B} step={step} length_penalty={lpen} early_stopping={early}"
        pos, last = step + 1, step == STEPS[-1]
        d = {k: v.clone().to(DEV) for k, v in st.items()}
        cacc, ctok = torch.full((BK + 2, C), 77.0, device=DEV), torch.full((BK + 2, C), 77, dtype=torch.int32, device=DEV)
        ops.beam_rows(xd, d["run"], cacc[1:-1], ctok[1:-1])
        assert bool((cacc[0] == 77).all() and (cacc[-1] == 77).all() and (ctok[0] == 77).all() and (ctok[-1] == 77).all()), what
        assert torch.equal(ctok[1:-1].cpu(), tok), what
        worst = max(worst, close(cacc[1:-1], acc, what + " candidates"))
        seq_dst = torch.full((BK, LD), -3, dtype=torch.int64, device=DEV)
        fin_dst = torch.full((BK, LD), -3, dtype=torch.int64, device=DEV)
        nxt, parent = torch.full((BK,), -5, dtype=torch.int64, device=DEV), torch.full((BK,), -5, dtype=torch.int32, device=DEV)
        nd = torch.tensor([-7, 0, -7], dtype=torch.int32, device=DEV)
        ops.beam_merge(cacc[1:-1], ctok[1:-1], d["seq"], seq_dst, d["fin"], fin_dst, pos, last, d["run"], nxt, parent, d["fin_score"], d["fin_raw"],
                       d["fin_len"], d["fin_filled"], d["open"], nd[1:2], pack_beam_params(lpen, early).to(DEV), 1, 0)
        torch.cuda.synchronize()
        assert torch.equal(nxt.cpu(), want["next_ids"]) and torch.equal(parent.cpu(), want["parent"]), what
        assert torch.equal(seq_dst[:, :pos + 1].cpu(), want["seq"][:, :pos + 1]) and bool((seq_dst[:, pos + 1:] == -3).all()), what
        assert torch.equal(fin_dst.cpu(), want["fin"]), what
        assert torch.equal(d["fin_len"].cpu(), want["fin_len"]) and torch.equal(d["fin_filled"].cpu(), want["fin_filled"]), what
        assert torch.equal(d["open"].cpu(), want["open"]) and nd.cpu().tolist() == [-7, want["n_done"], -7], what
        assert torch.equal(d["seq"].cpu(), st["seq"]) and torch.equal(d["fin"].cpu(), st["fin"]), what + ": a source row was written"
        for key in ("run", "fin_score", "fin_raw"):
            worst = max(worst, close(d[key], want[key], f"{what} {key}"))
    print(f"V={V} K={K} B={B}: {len(subs)} steps, worst relative score difference {worst:.3e}")


def test_rows_with_few_or_no_finite_logits(ops):
    """a NaN counts as −∞; −∞ entries are taken only when the finite ones run out, lowest index first, with −∞ as their score; a row
    without a finite logit gives indices 0 … C − 1"""
    for V in (257, 32128, 40000):
        x = torch.full((4, V), -INF)
        x[0, [3, V - 2, 40]] = torch.tensor([1.0, 2.0, 1.0])       # three finite, two of them equal
        x[1] = NAN
        x[2, ::2] = NAN
        x[2, 1::2] = torch.randn(x[2, 1::2].shape, generator=torch.Generator().manual_seed(V))
        x[3] = torch.randn(V, generator=torch.Generator().manual_seed(V + 1))
        x[3, 7] = NAN
        run = torch.tensor([-1.0, -2.0, -3.0, 0.0])
        acc, tok = rows_ref(x, run, 6)
        cacc, ctok = torch.zeros(4, 6, device=DEV), torch.zeros(4, 6, dtype=torch.int32, device=DEV)
        ops.beam_rows(x.to(DEV), run.to(DEV), cacc, ctok)
        assert tok[0].tolist() == [V - 2, 3, 40, 0, 1, 2] and tok[1].tolist() == [0, 1, 2, 3, 4, 5]
        assert torch.equal(ctok.cpu(), tok), (V, ctok.tolist(), tok.tolist())
        assert not bool(torch.isnan(cacc).any())
        assert bool((cacc[0, 3:] == -INF).all()) and bool((cacc[1] == -INF).all()) and bool(torch.isfinite(cacc[2:]).all())
        close(cacc, acc, f"V={V}")


# ---- lako_beam_gather ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inner", [64, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_gather_is_index_select_on_the_first_positions(ops, inner, dtype):
    Ld, rows, ML = 2, 6, 9
    g = torch.Generator().manual_seed(inner)
    src = torch.randn(Ld, rows, ML, 3 * inner, generator=g).to(dtype).to(DEV)
    for t in (0, 4, 7):
        for parent in ([0, 1, 2, 3, 4, 5], [1, 0, 0, 5, 5, 3], torch.randint(0, rows, (rows,), generator=g).tolist()):
            big = torch.full((Ld + 2, rows, ML, 3 * inner), 77.0, dtype=dtype, device=DEV)
            dst = big[1:-1]
            dst[:, :, t + 1:] = NAN
            before = big.clone()
            p = torch.tensor(parent, dtype=torch.int32, device=DEV)
            ops.beam_gather(src, dst, p, t + 1, inner, 2 * inner)
            torch.cuda.synchronize()
            want = before.clone()
            want[1:-1, :, :t + 1, inner:] = src[:, p.long(), :t + 1, inner:]
            # bit for bit, guards, the q columns and the NaN positions behind t included
            assert torch.equal(big.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                               want.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)), (inner, dtype, t, parent)


# ---- the model -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,K,lpen,early,ML", CASES)
def test_generate_reproduces_transformers_beam_search_fp32(i, K, lpen, early, ML):
    """tiny_eos in fp32, every recorded case, three calls: eager warm-up of the mode, graph capture, pure replay — bit for bit the same,
    HF's tokens, and raw / len**length_penalty within 1e-4 of HF's sequences_scores (the fp32 bound of tests/test_sample_gpu.py)"""
    z, model, ids, mask = fixture_model("tiny_eos")
    calls = [model.generate(ids, mask, ML, num_beams=K, num_return_sequences=K, length_penalty=lpen, early_stopping=early, return_scores=True)
             for _ in range(3)]
    for toks, raw in calls[1:]:
        assert torch.equal(toks, calls[0][0]) and torch.equal(raw.view(torch.int32), calls[0][1].view(torch.int32))
    graphs = model._get_engine()._ws_cache[("gen", ids.shape[0], ids.shape[1], ids.shape[2], ML, K, "b")]["g.graphs"]
    assert any(len(g_["steps"]) > 0 for g_ in graphs.values()), "no step graph was captured"
    worst = check_against_hf(i, K, lpen, calls[0][0].cpu(), calls[0][1].cpu())
    print(f"K={K} length_penalty={lpen} early_stopping={early} max_length={ML}: max |raw / len**lp - HF score| {worst:.3e}")


# bf16 on gen_d512 (top-1 / top-2 logit gaps > 1): |returned raw score − FiDT5.score(returned tokens)| per route, over all K returned
# hypotheses.  Each bound is 1.5 × the difference measured on the MI355X for that route (the convention of tests/test_sample_gpu.py;
# FiDT5.score is unchanged by beam search); DESIGN.md §3 "Beam search" quotes the same table.
BEAM_BF16_MEASURED = {"one_pass": 1.8978e-4, "unfused": 4.7684e-6, "projected": 2.8310e-3}
BEAM_ROUTES = {"one_pass": (2, {}), "unfused": (4, {}), "projected": (4, dict(LAKO_XATTN_GENERATE="0"))}


def test_bf16_routes_best_hypothesis_graphs_and_scores(monkeypatch):
    """K = 2 takes the one-pass cross-attention kernel, K = 4 the unfused ones, LAKO_XATTN_GENERATE=0 the projected route: on each the
    best hypothesis is the fixture's greedy decode, the replayed call returns what the eager one did, and the returned scores are what
    FiDT5.score gives for the returned tokens within the route's bound"""
    model, ids, mask, want, ML = d512_model()
    B = ids.shape[0]
    eng = model._get_engine()
    diffs = {}
    for route, (K, env) in BEAM_ROUTES.items():
        monkeypatch.setenv("LAKO_XATTN_GENERATE", "1")
        monkeypatch.delenv("LAKO_XATTN_DECODE", raising=False)
        for k_, v_ in env.items():
            monkeypatch.setenv(k_, v_)
        monkeypatch.setenv("LAKO_GEN_GRAPH", "0")
        eager, es = model.generate(ids, mask, ML, num_beams=K, num_return_sequences=K, return_scores=True)
        monkeypatch.setenv("LAKO_GEN_GRAPH", "1")
        for _ in range(3):
            toks, sc = model.generate(ids, mask, ML, num_beams=K, num_return_sequences=K, return_scores=True)
        assert eng.xattn_active == (route != "projected")
        assert torch.equal(toks, eager) and torch.equal(sc, es), route
        best = toks.view(B, K, -1)[:, 0].cpu()
        n = min(best.shape[1], want.shape[1])
        assert torch.equal(best[:, :n], want[:, :n]) and not bool(best[:, n:].any()) and not bool(want[:, n:].any()), (route, best.tolist())
        diffs[route] = float((sc - model.score(ids, mask, as_candidates(toks, B, K))).abs().max())
        print(f"{route} K={K}: max |generate score - model.score| {diffs[route]:.4e}, largest |score| {float(sc.abs().max()):.3f}")
    for route, v_ in diffs.items():
        assert v_ <= 1.5 * BEAM_BF16_MEASURED[route], (route, v_)
