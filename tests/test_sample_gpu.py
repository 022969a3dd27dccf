"""-m gpu: sampled decoding on the HIP path — lako_sample_step against the torch restatement of the sampler in float64
(tests/ref_ops_sample.py) with token equality, the distribution of its draws, lako_xattn_decode_multi bit for bit against
lako_xattn_decode run per sequence, and FiDT5.generate(do_sample=True, …) against the fixtures' greedy tokens, against itself across
the eager / graph-replay and the three cross-attention routes, and against FiDT5.score."""
import math
import os

import numpy as np
import pytest
import torch

from lako_amd import FiDConfig, FiDT5
from lako_amd._lib import XK_DECODE_MULTI, LakoError
from tests.ref_ops_sample import SWEEP_V, pack_params, pick_seed, sample_rows, sweep_cases, sweep_logits
from tests.test_sample_cpu import as_candidates
from tests.test_xattn_gates_gpu import GUARD, NAN, encoder_states, inside, offsets, rel_l2, rnd, untouched
from tests.util_golden import load_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
INF = float("inf")


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


# ---- lako_sample_step ------------------------------------------------------------------------------------------------------------
class Step:
    """one launch over guarded buffers: seq [rows, 6] inside a window of guard words, score likewise"""
    def __init__(self, ops, logits, done=None, score0=None):
        self.ops, self.rows = ops, logits.shape[0]
        rows = self.rows
        self.logits = logits.to(DEV).contiguous()
        self.seq, self.seq_big, self.seq_sl = inside(torch.zeros(rows, 6, dtype=torch.int64, device=DEV), [(2, 2), (1, 1)], 77)
        self.score, self.score_big, self.score_sl = inside(torch.zeros(rows, device=DEV) if score0 is None else score0.to(DEV), [(3, 3)], GUARD)
        self.nxt = torch.full((rows,), -5, dtype=torch.int64, device=DEV)
        self.done = torch.zeros(rows, dtype=torch.uint8, device=DEV) if done is None else done.to(DEV)
        self.nd = torch.full((3,), -7, dtype=torch.int32, device=DEV)

    def run(self, temperature, top_k, top_p, seed, step, group, pos=3, eos=1, pad=0):
        params = pack_params(temperature, top_p, top_k, seed).to(DEV)
        # score is a window of a bigger buffer: hand the kernel a contiguous view of exactly `rows` floats
        self.ops.sample_step(self.logits, self.seq, pos, self.nxt, self.done, self.score, self.nd[1:2], params, step, group, eos, pad)
        torch.cuda.synchronize()
        return self.seq[:, pos].cpu()

    def guards_intact(self, pos, what):
        c = self.seq_big.clone()
        assert bool((c[self.seq_sl][:, [p for p in range(6) if p != pos]] == 0).all()), f"{what}: another position of seq was written"
        c[self.seq_sl] = 77
        assert bool((c == 77).all()), f"{what}: a word around seq was written"
        untouched(self.score_big, self.score_sl, f"{what} score")
        assert self.nd[0] == -7 and self.nd[2] == -7, f"{what}: a word around n_done was written"


@pytest.mark.parametrize("V", SWEEP_V)
def test_sample_step_draws_the_restatements_token(ops, V):
    """every (rows, top_k, top_p, temperature, step) of the sweep.  A row is compared when the restatement calls it decidable: its draw
    further than 1e-5·mass from both CDF edges of the drawn token, and its nucleus boundary further than 1e-5 from top_p (the kernel's
    exp is fp32).  At V = 32 128 the tokens at the 0.9 boundary have p ≈ 4e-6, so no boundary can be 1e-5 away from top_p; there a row
    also counts as decidable when EVERY nucleus whose boundary lies within 1e-5 of top_p gives the same token
    (tests/ref_ops_sample.py::sample_row) — more rows are compared, and every row the plain rule compares still is.  First the
    restatement alone: at most 1 % of the rows may be undecidable (tests/test_sample_cpu.py holds the same without a GPU); then the
    kernel, token for token."""
    cases = list(sweep_cases(V))
    total, undecided = sum(c["want"].numel() for c in cases), sum(int((~c["dec"]).sum()) for c in cases)
    print(f"V={V}: {total} rows, {undecided} undecidable")
    assert undecided <= 0.01 * total
    worst_lp = 0.0
    for c in cases:
        x, want, lp, dec, what = c["x"], c["want"], c["lp"], c["dec"], c["what"]
        rows = x.shape[0]
        st = Step(ops, x)
        got = st.run(c["temperature"], c["top_k"], c["top_p"], c["seed"], c["step"], c["group"])
        st.guards_intact(3, what)
        assert bool(((got >= 0) & (got < V)).all()), (what, got.tolist())
        assert bool((x[torch.arange(rows), got] > -INF).all()), f"{what}: a token with logit -inf was drawn"
        assert torch.equal(got[dec], want[dec]), (what, got.tolist(), want.tolist(), dec.tolist())
        same = got == want
        err = (st.score.cpu().double() - lp)[same].abs()
        worst_lp = max(worst_lp, float(err.max()) if err.numel() else 0.0)
        assert st.nxt.cpu().tolist() == got.tolist() and int(st.nd[1]) == int((got == 1).sum())
        assert st.done.cpu().tolist() == (got == 1).to(torch.uint8).tolist()
    print(f"V={V}: worst |log-prob - float64| {worst_lp:.3e}")
    assert worst_lp <= 1e-5


def test_sample_step_done_rows_nan_rows_and_the_row_that_does_not_fit_lds(ops):
    V = 32128
    x = sweep_logits(4, V, 9)
    x[2] = NAN                                              # a row of NaNs: id 0, never an out-of-range id
    x[3, ::2] = NAN                                         # NaNs count as −∞: never drawn
    done = torch.tensor([0, 1, 0, 0], dtype=torch.uint8)
    st = Step(ops, x, done=done, score0=torch.tensor([0.5, 0.25, 0.0, -1.0]))
    got = st.run(1.0, 0, 1.0, 77, 2, 4, pad=9)
    st.guards_intact(3, "done / NaN rows")
    want, lp, dec = sample_rows(x, 1.0, 0, 1.0, 77, 2, 4)
    assert dec[0] and dec[3]
    assert got.tolist() == [int(want[0]), 9, 0, int(want[3])] and int(want[3]) % 2 == 1
    sc = st.score.cpu()
    assert sc[1] == 0.25 and sc[2] == 0.0                   # a done row leaves its score alone
    assert abs(float(sc[0]) - (0.5 + float(lp[0]))) <= 1e-5 and abs(float(sc[3]) - (-1.0 + float(lp[3]))) <= 1e-5
    assert st.done.cpu().tolist() == [int(want[0] == 1), 1, 0, int(want[3] == 1)]
    # V = 40 001: the row (160 004 bytes) does not fit next to the histograms and is re-read from L2 — the same tokens
    V = 40001
    x = sweep_logits(3, V, 10)
    for top_k, top_p in ((0, 1.0), (50, 0.9), (0, 0.05)):
        seed, want, lp, dec = pick_seed(x, 0.7, top_k, top_p, 1, 3, 5)
        st = Step(ops, x)
        got = st.run(0.7, top_k, top_p, seed, 1, 3)
        st.guards_intact(3, f"V={V}")
        assert bool(dec.all()) and torch.equal(got, want), (top_k, top_p, got.tolist(), want.tolist())
        assert float((st.score.cpu().double() - lp).abs().max()) <= 1e-5


def test_sample_step_frequencies_follow_the_softmax(ops):
    """V = 7, 8192 rows × steps 0…3 of fixed logits, temperature 1, no truncation: each token's frequency within
    5·sqrt(p(1 − p)/n) of its softmax probability (five standard deviations of a binomial frequency), −∞ never"""
    logit = torch.tensor([0.0, 1.0, 2.0, -1.0, 0.5, -INF, 1.5])
    rows, steps = 8192, 4
    x = logit[None].expand(rows, -1).contiguous()
    counts = torch.zeros(7, dtype=torch.int64)
    for step in range(steps):
        st = Step(ops, x)
        got = st.run(1.0, 0, 1.0, 2024, step, rows, eos=-1)
        counts += torch.bincount(got, minlength=7)
    n = rows * steps
    p = torch.softmax(logit.double(), 0)
    freq = counts.double() / n
    for i in range(7):
        bound = 5.0 * math.sqrt(float(p[i]) * (1.0 - float(p[i])) / n)
        print(f"token {i}: p {float(p[i]):.5f} frequency {float(freq[i]):.5f} |diff| / bound {abs(float(freq[i] - p[i])) / bound if bound else 0.0:.3f}")
    assert int(counts[5]) == 0
    for i in range(7):
        assert abs(float(freq[i] - p[i])) <= 5.0 * math.sqrt(float(p[i]) * (1.0 - float(p[i])) / n), (i, float(freq[i]), float(p[i]))


# ---- lako_xattn_decode_multi -------------------------------------------------------------------------------------------------------
MULTI_LENS = {1: [200], 3: [33, 1, 200]}                 # per-sample key counts (with the lens of the K sweep below: 1, 31, 32, 33, 200)
MULTI_LENS_ALT = {1: [31], 3: [32, 31, 1]}


def expected_rt(D, K):
    return min({512: 4, 768: 4, 1024: 2}[D], max(c for c in (1, 2, 4) if c <= K))


@pytest.mark.parametrize("K", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("D", [512, 768, 1024])
def test_decode_multi_writes_the_single_tile_kernels_bits(ops, D, K):
    """K sequences per sample through xdecode_kernel<KS, RT> (the rule's RT, and RT forced to 1 and 2): the partials of every sequence
    equal, bit for bit, lako_xattn_decode's for that sequence alone; the combine against float64 within the decode bound of
    tests/test_xattn_gates_gpu.py (context rel_l2 < 1e-2 against the direct form).  Z = 5 leaves most ranges of the short samples empty;
    E has row stride D + 8 and NaN rows around it, Q NaN rows past H and NaN columns past D."""
    for H in (6, 12, 16):
        for B, lens in ((1, (MULTI_LENS if H != 12 else MULTI_LENS_ALT)[1]), (3, (MULTI_LENS if H != 6 else MULTI_LENS_ALT)[3])):
            Z = 5
            k_off, _, ko, _ = offsets(lens)
            E = encoder_states(ko[-1], D, seed=D + K)
            Q = inside(rnd(B, K, H, D, dtype=BF, scale=0.08, seed=2 + H), [(0, 0), (0, 0), (1, 16 - H + 2), (0, 8)], NAN)[0]
            Wv = rnd(H * 64, D, dtype=BF, scale=0.05, seed=3)
            # the reference partials: one single-tile launch per sequence
            ref_ml = torch.empty(Z, B, K, 16, 2, device=DEV)
            ref_c = torch.empty(Z, B, K, 16, D, device=DEV)
            for k in range(K):
                ml1, c1 = torch.full((Z, B, 16, 2), GUARD, device=DEV), torch.full((Z, B, 16, D), GUARD, device=DEV)
                ops.xattn_decode(Q[:, k], E, k_off, ml1, c1)
                ref_ml[:, :, k], ref_c[:, :, k] = ml1, c1
            for rt in (0, 1, 2):
                what = f"decode_multi D={D} H={H} K={K} B={B} rt={rt}"
                pml, mlbig, mlsl = inside(torch.full((Z, B * K, 16, 2), GUARD, device=DEV), [(1, 1), (0, 0), (0, 0), (0, 0)], GUARD)
                pc, pcbig, pcsl = inside(torch.full((Z, B * K, 16, D), GUARD, device=DEV), [(1, 1), (0, 0), (0, 0), (0, 0)], GUARD)
                pl = ops.xattn_decode_multi_plan(Q, E, k_off, pml, pc, rt)
                want_rt = rt or expected_rt(D, K)
                stage = 32 * D * 2
                stages = 3 if 3 * stage + want_rt * 16384 <= 160 * 1024 else 2
                assert (pl.kernel, pl.ks, pl.nt, pl.stages, pl.lds) == (XK_DECODE_MULTI, D // 256, want_rt, stages, stages * stage + want_rt * 16384), pl
                assert (pl.gx, pl.gy, pl.gz, pl.block) == (Z, B, -(-K // want_rt), 512), pl
                ops.xattn_decode_multi(Q, E, k_off, pml, pc, rt)
                torch.cuda.synchronize()
                untouched(mlbig, mlsl, f"{what} part_ml")
                untouched(pcbig, pcsl, f"{what} part_c")
                assert torch.equal(pml.view(Z, B, K, 16, 2).view(torch.int32), ref_ml.view(torch.int32)), f"{what}: part_ml bits differ"
                assert torch.equal(pc.view(Z, B, K, 16, D).view(torch.int32), ref_c.view(torch.int32)), f"{what}: part_c bits differ"
                if rt:
                    continue
                ctx = torch.full((B * K, H * 64), GUARD, dtype=BF, device=DEV)
                ops.xattn_decode_combine(pml, pc, Wv, ctx, H)
                torch.cuda.synchronize()
                wv = Wv.double().view(H, 64, D)
                worst = 0.0
                for b, n in enumerate(lens):
                    e = E[ko[b]:ko[b + 1]].double()
                    for k in range(K):
                        s = Q[b, k].double() @ e.T
                        direct = torch.einsum("hc,hjc->hj", torch.softmax(s, -1) @ e, wv)
                        got = ctx[b * K + k].double().view(H, 64)
                        assert bool(torch.isfinite(got).all()), what
                        worst = max(worst, rel_l2(got, direct))
                print(f"{what}: worst ctx rel_l2 against the direct form {worst:.2e}")
                assert worst < 1e-2, (what, worst)


def test_decode_multi_refusals_reach_python_through_launch_and_plan(ops):
    """(the whole refusal table runs on the CPU, tests/test_sample_plan_cpu.py; here: both entries raise through HipOps)"""
    D, H, K, B, Z = 1024, 12, 4, 1, 2
    k_off, _, ko, _ = offsets([40])
    E, Q = encoder_states(ko[-1], D), rnd(B, K, H, D, dtype=BF)
    pml, pc = torch.zeros(Z, B * K, 16, 2, device=DEV), torch.zeros(Z, B * K, 16, D, device=DEV)
    for fn in (ops.xattn_decode_multi, ops.xattn_decode_multi_plan):
        with pytest.raises(LakoError):
            fn(Q, E, k_off, pml, pc, 4)                     # RT = 4 is not built at D = 1024
        with pytest.raises(LakoError):
            fn(Q, E, k_off, pml, pc, 3)
        with pytest.raises(LakoError):
            fn(rnd(B, K, 17, D, dtype=BF), E, k_off, pml, pc)
    assert bool((pml == 0).all()) and bool((pc == 0).all())


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def fixture_model(name, dtype=torch.float32):
    from tests.test_parity_gpu import cfg_of
    z, dims, w = load_case(name)
    model = FiDT5(cfg_of(dims), dtype=dtype)
    model.load_t5(w)
    return z, model.cuda().eval(), torch.from_numpy(z["input_ids"]).to(DEV), torch.from_numpy(z["attention_mask"]).to(DEV)


def d512_model():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_d512.npz"))
    names = ("vocab_size", "d_model", "d_kv", "d_ff", "num_layers", "num_decoder_layers", "num_heads")
    cfg = FiDConfig(dropout_rate=0.0, **{k: int(v) for k, v in zip(names, z["dims"])})
    w = {k[2:]: torch.from_numpy(z[k]).view(torch.bfloat16).float() for k in z.files if k.startswith("w.")}
    m = FiDT5(cfg, dtype=torch.bfloat16)
    m.load_t5(w)
    return m.cuda().eval(), torch.from_numpy(z["ids"]).to(DEV), torch.from_numpy(z["mask"]).to(DEV), torch.from_numpy(z["tokens"]), int(z["max_length"])


@pytest.mark.parametrize("name", ["tiny_a", "tiny_fact", "mid_a", "tiny_eos"])
def test_top_k_1_rows_are_the_fixtures_greedy_tokens_fp32(name):
    z, model, ids, mask = fixture_model(name)
    B = ids.shape[0]
    for ml in (4, 12):
        want = torch.from_numpy(z[f"gen_{ml}"])
        for rnd_ in range(3):                               # eager warm-up of the mode, graph capture, pure replay
            toks, sc = model.generate(ids, mask, ml, do_sample=True, top_k=1, num_return_sequences=3, seed=rnd_, return_scores=True)
            assert torch.equal(toks.cpu().view(B, 3, -1), want[:, None].expand(-1, 3, -1)), (name, ml, rnd_)
        ref = model.score(ids, mask, as_candidates(toks, B, 3))
        diff = float((sc - ref).abs().max())
        print(f"{name} max_length {ml} fp32: max |generate score - model.score| {diff:.3e}")
        assert diff <= 1e-4
    # sampled, with the truncations on
    toks, sc = model.generate(ids, mask, 12, do_sample=True, temperature=1.5, top_p=0.9, num_return_sequences=4, seed=7, return_scores=True)
    diff = float((sc - model.score(ids, mask, as_candidates(toks, B, 4))).abs().max())
    print(f"{name} sampled fp32: max |generate score - model.score| {diff:.3e}")
    assert diff <= 1e-4
    gt, gs = model.generate(ids, mask, 12, return_scores=True)                 # greedy with scores: the greedy tokens
    assert torch.equal(gt.cpu(), torch.from_numpy(z["gen_12"])) and tuple(gs.shape) == (B, 1)
    assert float((gs - model.score(ids, mask, as_candidates(gt, B, 1))).abs().max()) <= 1e-4


def test_a_sampled_call_adds_no_host_sync():
    """torch's sync debug mode turns any synchronising torch call into an error (tests/test_drivers_gpu.py's pattern); generate's own
    waits are event waits on a finished step (LAG steps behind), which the mode does not count — the greedy call shows that first"""
    z, model, ids, mask = fixture_model("mid_a")
    lens = mask.sum(-1).to(torch.int32).cpu()
    kw = dict(do_sample=True, temperature=1.2, top_k=20, top_p=0.9, num_return_sequences=3, seed=3, return_scores=True)
    for _ in range(3):                                       # allocations, LDS attributes, graph capture
        model.generate(ids, mask, 12, passage_lengths=lens)
        first = model.generate(ids, mask, 12, passage_lengths=lens, **kw)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        model.generate(ids, mask, 12, passage_lengths=lens)
        again = model.generate(ids, mask, 12, passage_lengths=lens, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


# bf16: every (route, regime) has its own bound, 1.5 × the difference measured on the MI355X for that route and regime (FiDT5.score is
# unchanged from the commit before sampled decoding; eager and replayed calls measured the same figure, and the larger of the two is
# compared).  The regimes, on gen_d512 with K = 3:
#   greedy     top_k = 1 — |score| <= 0.003, the fixture's model is sure of its answers;
#   moderate   temperature 2.5, top_k 40, top_p 0.95 — |score| up to 36.5, a quarter of the tokens differ from the greedy ones, bf16
#              amplification small: the regime that pins the bf16 projected and one-pass formulations with K distinct rows per question;
#   hot        temperature 5, top_k 40, top_p 0.95 / 0.8 — |score| up to 113, answers the model finds very unlikely, where the bf16 roundings of different
#              formulations of the cross-attention are amplified (FiDT5.score runs the unfused encoder-state kernels: that route sees
#              the same kernels on the same rows);
#   agreement  greedy scores of a route against the projected route's eager call.
# DESIGN.md §3 "Sampled decoding" quotes the same table.
SCORE_BF16_MEASURED = {
    ("projected", "greedy"): 4.8822e-6, ("unfused", "greedy"): 8.5536e-7, ("one_pass", "greedy"): 1.4326e-6,
    ("projected", "moderate"): 4.1641e-2, ("unfused", "moderate"): 2.8610e-6, ("one_pass", "moderate"): 4.0436e-4,
    ("projected", "hot"): 1.0467, ("unfused", "hot"): 3.8147e-6, ("one_pass", "hot"): 4.2505e-1,
    ("projected", "agreement"): 0.0, ("unfused", "agreement"): 4.6408e-6, ("one_pass", "agreement"): 3.4496e-6,
}
ROUTES = {"projected": dict(LAKO_XATTN_GENERATE="0"), "unfused": dict(LAKO_XATTN_DECODE="0"), "one_pass": {}}


def test_bf16_routes_graphs_and_scores(monkeypatch):
    """gen_d512 (bf16; d_model 512, 8 heads, 4 questions × 10 passages × 200 tokens; its tokens are the fp32 oracle's greedy decode):
    K = 3 rows of top_k = 1 equal the fixture on every cross-attention route, eager and replayed; sampled tokens (temperature, top-k,
    top-p) are the same eager and replayed, and calls with other seeds and top_p replay the SAME graph objects; generate's scores agree
    with FiDT5.score of the same tokens, and the routes with each other, within the bound of their own (route, regime)."""
    model, ids, mask, want, ML = d512_model()
    B, K = ids.shape[0], 3
    eng = model._get_engine()
    diffs, scores, sampled, largest, moved = {}, {}, {}, {}, {}

    def against_score(toks, sc):
        return float((sc - model.score(ids, mask, as_candidates(toks, B, K))).abs().max())

    def note(route, regime, value):
        diffs[route, regime] = max(diffs.get((route, regime), 0.0), value)

    for route, env in ROUTES.items():
        for k_, v_ in {"LAKO_XATTN_GENERATE": "1", "LAKO_XATTN_DECODE": "1", **env}.items():
            monkeypatch.setenv(k_, v_)
        for graph in ("0", "1"):
            monkeypatch.setenv("LAKO_GEN_GRAPH", graph)
            for rnd_ in range(3 if graph == "1" else 1):    # graph: eager warm-up of the mode, capture, pure replay
                toks, sc = model.generate(ids, mask, ML, do_sample=True, top_k=1, num_return_sequences=K, seed=rnd_, return_scores=True)
                assert torch.equal(toks.cpu().view(B, K, -1), want[:, None].expand(-1, K, -1)), (route, graph, rnd_)
            assert eng.xattn_active == (route != "projected")
            scores[route, graph] = sc
            note(route, "greedy", against_score(toks, sc))
            # sampled: eager first (graph = 0), then the replayed graphs must give the same tokens for the same seed
            kw = dict(do_sample=True, top_k=40, num_return_sequences=K, return_scores=True)
            if graph == "1":      # the step graphs the three calls above left behind, per mode of this workspace
                graphs = eng._ws_cache[("gen", B, ids.shape[1], ids.shape[2], ML, K, "s")]["g.graphs"]
                before = {m_: dict(g_["steps"]) for m_, g_ in graphs.items()}
                assert any(len(v_) > 0 for v_ in before.values()), "no step graph was captured"
            runs = [("moderate", model.generate(ids, mask, ML, seed=4, temperature=2.5, top_p=0.95, **kw)),
                    ("hot", model.generate(ids, mask, ML, seed=5, temperature=5.0, top_p=0.95, **kw)),
                    ("hot", model.generate(ids, mask, ML, seed=6, temperature=5.0, top_p=0.8, **kw))]
            if graph == "0":
                sampled[route] = [t_ for _, (t_, _) in runs]
            else:                 # other sampler settings replay the SAME graph objects, and give the eager call's tokens
                for m_, steps in before.items():
                    assert all(graphs[m_]["steps"][t] is g_ for t, g_ in steps.items()), (route, m_)
                assert all(torch.equal(t_, e_) for (_, (t_, _)), e_ in zip(runs, sampled[route])), route
            for regime, (t_, s_) in runs:
                note(route, regime, against_score(t_, s_))
                largest[regime] = max(largest.get(regime, 0.0), float(s_.abs().max()))
                n = min(t_.shape[1], want.shape[1])
                moved[regime] = max(moved.get(regime, 0.0), float((t_.cpu().view(B, K, -1)[:, :, :n] != want[:, None, :n]).float().mean()))
    ref = scores["projected", "0"]
    for (route, graph), sc in scores.items():
        note(route, "agreement", float((sc - ref).abs().max()))
    assert not torch.equal(sampled["one_pass"][1], sampled["one_pass"][2])      # another seed: other tokens
    for (route, regime), v_ in sorted(diffs.items()):
        print(f"gen_d512 bf16 {route} {regime}: {v_:.4e} (measured {SCORE_BF16_MEASURED[route, regime]})")
    print(f"gen_d512 bf16 largest |score|: greedy {float(ref.abs().max()):.3f}, " + ", ".join(
        f"{r_} {largest[r_]:.1f} ({100 * moved[r_]:.0f} % of the tokens differ from the greedy ones)" for r_ in ("moderate", "hot")))
    for key, v_ in diffs.items():
        assert SCORE_BF16_MEASURED[key] is not None and v_ <= 1.5 * SCORE_BF16_MEASURED[key], (key, v_, SCORE_BF16_MEASURED[key])
