"""T5-3B / Flan-T5-XL readers on the MI355X: the generic attention kernels at d_head 128, the wide-row RMSNorm backward (1024 < d <= 4096),
and the HIP engine against the reference's xl fixtures (tools/make_xl_fixtures.py) and, at full size, against the oracle."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from lako_amd import FiDConfig, FiDT5
from lako_amd import util as U
from lako_amd.model import plain_name
from lako_amd.ops import HipOps
from oracle import fid_t5_oracle as O
from tests.ref_ops import RefOps
from tests.test_kernels_gpu import close, rnd
from tests.util_xl import build_xl, check_grads, train_three_steps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def ops():
    return HipOps()


@pytest.fixture(scope="module")
def ref():
    return RefOps()


# ------------------------------------------------------------------------------------------------
# attention, d_head 128
ATTN128 = [
    # name, Bn, H, Lq, Lk, bias, mask, causal, causal_off, drop
    ("enc_pad", 2, 3, 200, 200, True, True, False, 0, None),     # one fully padded row (below)
    ("enc_drop", 2, 2, 150, 150, True, True, False, 0, (0.1, 31, 3)),
    ("enc_nomask", 2, 2, 256, 256, True, False, False, 0, None),
    ("dec_self", 4, 4, 9, 9, True, False, True, 0, (0.1, 32, 4)),
    ("decode_step", 3, 4, 1, 11, True, False, True, 10, None),    # the KV-cached step: query at position 10 of 11 keys
    ("cross_4000", 2, 2, 5, 4000, False, True, False, 0, None),   # key split over 4 000 keys, several chunks
    ("cross_drop", 2, 2, 20, 300, False, True, False, 0, (0.1, 33, 5)),
]


def make_case(case, T):
    name, Bn, H, Lq, Lk, bias, mask, causal, coff, drop = case
    dk, inner = 128, H * 128
    if Lq == Lk and not causal:
        qkv = rnd(Bn, Lq, 3 * inner, dtype=T, seed=61, scale=0.3)
        q, k, v = (qkv[:, :, i * inner:(i + 1) * inner].view(Bn, Lq, H, dk) for i in range(3))
    else:
        q = rnd(Bn, Lq, H, dk, dtype=T, seed=62, scale=0.3)
        kv = rnd(Bn, Lk, 2 * inner, dtype=T, seed=63, scale=0.3)
        k, v = kv[:, :, :inner].view(Bn, Lk, H, dk), kv[:, :, inner:].view(Bn, Lk, H, dk)
    rel, rel_off = None, 0
    if bias:
        R = Lq + Lk - 1 + coff
        rel, rel_off = rnd(H, R, seed=64), Lq - 1 + coff
    km = None
    if mask:
        g = torch.Generator().manual_seed(5)
        lens = torch.randint(max(1, Lk // 2), Lk + 1, (Bn,), generator=g)
        km = torch.arange(Lk)[None, :] < lens[:, None]
        km[Bn - 1] = False
        km = km.to(torch.uint8).to(DEV)
    return q, k, v, dict(rel_bias=rel, rel_off=rel_off, key_mask=km, causal=causal, causal_off=coff, drop=drop)


def zeros_as(t, dtype=None):
    """zeros with the strides of `t` (a gradient must share the layout of its forward tensor, packed Q/K/V views included)"""
    return torch.empty_strided(t.shape, t.stride(), dtype=dtype or t.dtype, device=t.device).zero_()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", ATTN128, ids=[c[0] for c in ATTN128])
def test_attention_d128(ops, ref, dt, case):
    """forward (output, statistics, captured scores) and backward (dq, dk, dv, drel) against the fp32 test double, with the bounds of
    the d_head 64 cases in test_kernels_gpu.py"""
    T = DT[dt]
    q, k, v, kw = make_case(case, T)
    Bn, Lq, H, dk = q.shape
    Lk = k.shape[1]
    out, outr = torch.zeros(Bn, Lq, H, dk, dtype=T, device=DEV), torch.zeros(Bn, Lq, H, dk, device=DEV)
    st, stg = torch.zeros(Bn, H, Lq, 4, device=DEV), torch.zeros(Bn, H, Lq, 4, device=DEV)
    sc, scr = torch.zeros(Bn, H, Lq, Lk, device=DEV), torch.zeros(Bn, H, Lq, Lk, device=DEV)
    ops.attn_fwd(q, k, v, out, stg, scores_out=sc, **kw)
    ref.attn_fwd(q, k, v, outr, st, scores_out=scr, **kw)
    close(sc, scr, T, f"scores {case[0]} {dt}")
    close(stg[..., 0], st[..., 0], T, f"rowmax {case[0]} {dt}")
    close(stg[..., 1], st[..., 1], T, f"1/rowsum {case[0]} {dt}", k=2)
    close(out, outr, T, f"out {case[0]} {dt}")
    # without capture: the same output
    out2 = torch.zeros_like(out)
    ops.attn_fwd(q, k, v, out2, torch.zeros_like(stg), **kw)
    close(out2, outr, T, f"out (no capture) {case[0]} {dt}")
    dout = rnd(Bn, Lq, H, dk, dtype=T, seed=65)
    o_in = outr.to(T)
    dq, dk_, dv = (zeros_as(t) for t in (q, k, v))
    dqr, dkr, dvr = (torch.zeros(t.shape, device=DEV) for t in (q, k, v))
    rel = kw["rel_bias"]
    drel, drelr = (torch.zeros_like(rel), torch.zeros_like(rel)) if rel is not None else (None, None)
    ops.attn_bwd(q, k, v, o_in, dout, st, dq, dk_, dv, drel=drel, **kw)
    ref.attn_bwd(q, k, v, o_in, dout, st, dqr, dkr, dvr, drel=drelr, **kw)
    close(dq, dqr, T, f"dq {case[0]} {dt}", k=2)
    close(dk_, dkr, T, f"dk {case[0]} {dt}", k=2)
    close(dv, dvr, T, f"dv {case[0]} {dt}", k=2)
    if rel is not None:
        close(drel, drelr, T, f"drel {case[0]} {dt}", k=4)


@pytest.mark.parametrize("kind", ["self", "cross"])
def test_attention_d128_ragged_equals_padded(ops, kind):
    """fp32, ragged q_off / k_off over packed rows = the padded call with a key mask, bit for bit, including an empty sequence"""
    T, H, dk = torch.float32, 2, 128
    inner = H * dk
    if kind == "cross":
        Bn, Lq, Lmax, lens = 3, 6, 150, [150, 37, 96]
    else:
        Bn, Lmax, lens = 4, 70, [70, 33, 0, 48]
        Lq = Lmax
    off = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=DEV)
    km = (torch.arange(Lmax, device=DEV)[None] < torch.tensor(lens, device=DEV)[:, None]).to(torch.uint8)
    heads = lambda t, c0: t[:, :, c0:c0 + inner].unflatten(2, (H, dk))      # noqa: E731

    def pack(tp):
        return torch.cat([tp[b, :lens[b]] for b in range(Bn)], 0)[None].contiguous()

    bias = {}
    if kind == "cross":
        q_p = rnd(Bn, Lq, inner, dtype=T, seed=71, scale=0.3)
        kv_p = rnd(Bn, Lmax, 2 * inner, dtype=T, seed=72, scale=0.3)
        args_p = (heads(q_p, 0), heads(kv_p, 0), heads(kv_p, inner))
        args_r = (heads(q_p, 0), heads(pack(kv_p), 0), heads(pack(kv_p), inner))
        rag = dict(k_off=off, max_k=Lmax)
        out_shape_r = (Bn, Lq, inner)
    else:
        qkv_p = rnd(Bn, Lmax, 3 * inner, dtype=T, seed=73, scale=0.3)
        args_p = tuple(heads(qkv_p, c) for c in (0, inner, 2 * inner))
        args_r = tuple(heads(pack(qkv_p), c) for c in (0, inner, 2 * inner))
        rag = dict(q_off=off, k_off=off, max_q=Lmax, max_k=Lmax)
        bias = dict(rel_bias=rnd(H, 2 * Lmax - 1, seed=74), rel_off=Lmax - 1)
        out_shape_r = (1, int(off[-1]), inner)
    out_p, st_p = torch.zeros(Bn, Lq, inner, device=DEV), torch.zeros(Bn, H, Lq, 4, device=DEV)
    ops.attn_fwd(*args_p, out_p.unflatten(2, (H, dk)), st_p, key_mask=km, **bias)
    out_r, st_r = torch.zeros(out_shape_r, device=DEV), torch.zeros_like(st_p)
    ops.attn_fwd(*args_r, out_r.unflatten(2, (H, dk)), st_r, **bias, **rag)
    assert torch.equal(out_r, out_p if kind == "cross" else pack(out_p))
    dout_p = rnd(Bn, Lq, inner, dtype=T, seed=75)
    if kind == "cross":
        dq_p, dkv_p = torch.zeros_like(q_p), torch.zeros_like(kv_p)
        ops.attn_bwd(*args_p, out_p.unflatten(2, (H, dk)), dout_p.unflatten(2, (H, dk)), st_p, heads(dq_p, 0), heads(dkv_p, 0),
                     heads(dkv_p, inner), key_mask=km)
        dq_r, dkv_r = torch.zeros_like(q_p), torch.zeros_like(pack(kv_p))
        ops.attn_bwd(*args_r, out_r.unflatten(2, (H, dk)), dout_p.unflatten(2, (H, dk)), st_r, heads(dq_r, 0), heads(dkv_r, 0),
                     heads(dkv_r, inner), **rag)
        assert torch.equal(dq_r, dq_p) and torch.equal(dkv_r, pack(dkv_p))
    else:
        dout_p = dout_p * km[:, :, None].to(T)
        dqkv_p, dqkv_r = torch.zeros_like(qkv_p), torch.zeros_like(pack(qkv_p))
        ops.attn_bwd(*args_p, out_p.unflatten(2, (H, dk)), dout_p.unflatten(2, (H, dk)), st_p, heads(dqkv_p, 0), heads(dqkv_p, inner),
                     heads(dqkv_p, 2 * inner), key_mask=km, **bias)
        ops.attn_bwd(*args_r, out_r.unflatten(2, (H, dk)), pack(dout_p).unflatten(2, (H, dk)), st_r, heads(dqkv_r, 0),
                     heads(dqkv_r, inner), heads(dqkv_r, 2 * inner), **bias, **rag)
        assert torch.equal(dqkv_r, pack(dqkv_p))


def test_attention_other_head_sizes_still_refused(ops):
    for dk in (96, 256):
        q = torch.zeros(1, 16, 1, dk, device=DEV)
        with pytest.raises(Exception, match="d_head"):
            ops.attn_fwd(q, q, q, torch.zeros_like(q), torch.zeros(1, 1, 16, 4, device=DEV))


# ------------------------------------------------------------------------------------------------
# RMSNorm backward, 1024 < d <= 4096
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("d", [1536, 2048, 4096])
@pytest.mark.parametrize("rows", [1, 37, 70001])
def test_rmsnorm_bwd_wide(ops, ref, dt, d, rows):
    T = DT[dt]
    x = rnd(rows, d, dtype=T, seed=81)
    w = 1.0 + 0.1 * rnd(d, seed=82)
    rs = torch.empty(rows, device=DEV)
    ref.rmsnorm_fwd(x, w, torch.empty(rows, d, device=DEV), rs, 1e-6, None)
    dy, dres = rnd(rows, d, dtype=T, seed=83), rnd(rows, d, dtype=T, seed=84)
    for drop in (None, (0.1, 5, 9)):
        for mode in ("none", "out_of_place", "in_place"):
            dr = None if mode == "none" else dres.clone()
            dx = dr if mode == "in_place" else torch.empty_like(x)
            dxr, dw, dwr = torch.empty(rows, d, device=DEV), torch.ones(d, device=DEV), torch.ones(d, device=DEV)
            ref.rmsnorm_bwd(dy, x, w, rs, dres if dr is not None else None, dxr, dwr, drop)
            ops.rmsnorm_bwd(dy, x, w, rs, dr, dx, dw, drop)
            close(dx, dxr, T, f"dx d={d} rows={rows} {mode} drop={drop}", tight=True)
            close(dw, dwr, torch.float32, f"dw d={d} rows={rows}", k=20 if rows < 1000 else 200)
            # the second, dropped output = lako_dropout_apply of the rounded dx, bit for bit
            dr2 = None if mode == "none" else dres.clone()
            dx2 = dr2 if mode == "in_place" else torch.empty_like(x)
            dd = torch.empty_like(x)
            ops.rmsnorm_bwd(dy, x, w, rs, dr2, dx2, torch.ones(d, device=DEV), drop, dx_drop=dd, drop_out=(0.2, 11, 12))
            want = torch.empty_like(x)
            ops.dropout_apply(dx, want, (0.2, 11, 12))
            assert torch.equal(dx2, dx) and torch.equal(dd, want)


def test_rmsnorm_bwd_wide_limits(ops):
    x = torch.zeros(4, 4104, device=DEV)
    with pytest.raises(Exception, match="4096"):
        ops.rmsnorm_bwd(x, x, torch.ones(4104, device=DEV), torch.ones(4, device=DEV), None, torch.empty_like(x),
                        torch.zeros(4104, device=DEV))


_DET_CHILD = r"""
import sys, json, hashlib, torch
sys.path.insert(0, {root!r})
from lako_amd.ops import HipOps
from tests.test_xl_gpu import make_case, zeros_as, ATTN128
ops, dev = HipOps(), torch.device("cuda:0")
def digest(*ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()
def run():
    res = []
    for T in (torch.float32, torch.bfloat16):
        for case in ATTN128:
            q, k, v, kw = make_case(case, T)
            Bn, Lq, H, dk = q.shape
            out, st = torch.zeros(Bn, Lq, H, dk, dtype=T, device=dev), torch.zeros(Bn, H, Lq, 4, device=dev)
            ops.attn_fwd(q, k, v, out, st, **kw)
            dout = torch.ones_like(out) * 0.1
            dq, dk_, dv = (zeros_as(t) for t in (q, k, v))
            drel = torch.zeros_like(kw["rel_bias"]) if kw["rel_bias"] is not None else None
            ops.attn_bwd(q, k, v, out, dout, st, dq, dk_, dv, drel=drel, **kw)
            res.append(digest(out, st, dq, dk_, dv, *([drel] if drel is not None else [])))
        for d in (1536, 4096):
            g = torch.Generator().manual_seed(d)
            x, dy = (torch.randn(70001, d, generator=g).to(dev, T) for _ in range(2))
            w, rs = torch.ones(d, device=dev), torch.ones(70001, device=dev) * 0.9
            dx, dw = torch.empty_like(x), torch.zeros(d, device=dev)
            ops.rmsnorm_bwd(dy, x, w, rs, None, dx, dw, (0.1, 3, 4))
            res.append(digest(dx, dw))
    return res
print(json.dumps([run(), run()]))
"""


def test_deterministic_mode_repeats_bit_for_bit():
    """LAKO_DETERMINISTIC=1 in a child process: d_head 128 attention (bias gradient in fixed point) and the wide RMSNorm backward
    (norm-weight gradient in fixed point) give bit-identical outputs over two runs"""
    r = subprocess.run([sys.executable, "-c", _DET_CHILD.format(root=ROOT)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, LAKO_DETERMINISTIC="1"), cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    a, b = json.loads(r.stdout.strip().splitlines()[-1])
    assert a == b


# ------------------------------------------------------------------------------------------------
# the HIP engine against the reference's fixtures
def to_dev(t):
    return torch.as_tensor(t).to(DEV)


CASES = ["xl3b_mid", "xlv11_mid"]


@pytest.mark.parametrize("name", CASES)
def test_fp32_vs_reference(name):
    z, dims, gated, model = build_xl(name, torch.float32, device="cuda")
    ids, mask, labels = (to_dev(z[k]) for k in ("input_ids", "attention_mask", "labels"))
    model.train()
    out = model(input_ids=ids, attention_mask=mask, labels=labels)
    ref = float(z["loss"])
    assert abs(out[0].item() - ref) < 1e-3 * max(1.0, abs(ref)), (out[0].item(), ref)
    torch.testing.assert_close(out.logits.cpu(), torch.from_numpy(z["logits"]), atol=1e-3, rtol=1e-3)
    out[0].backward()
    check_grads(z, model, rel=1e-3, tol=dict(atol=1e-3, rtol=1e-3))
    model.zero_grad()
    model.eval()
    for ml in (4, 12):
        assert model.generate(input_ids=ids, attention_mask=mask, max_length=ml).cpu().tolist() == z[f"gen_{ml}"].tolist()
    model.overwrite_forward_crossattention()
    model.reset_score_storage()
    model.generate(input_ids=ids, attention_mask=mask, max_length=4)
    sref = torch.from_numpy(z["cross_scores"])
    keep = mask.cpu().view(mask.shape[0], 1, 1, -1).expand_as(sref)
    torch.testing.assert_close(model._score_storage.cpu()[keep], sref[keep], atol=1e-3, rtol=1e-3)
    _, _, _, model = build_xl(name, torch.float32, device="cuda")
    train_three_steps(name, z, dims, model, to_dev, loss_tol=1e-3, gn_tol=2e-3, w_tol=dict(atol=1e-3, rtol=1e-3))


@pytest.mark.parametrize("name", CASES)
def test_bf16_vs_reference(name):
    """bf16: loss within 3 %, every gradient's norm within 5 % and its sample's direction cosine > 0.98 (the bounds of the gated
    fixtures' bf16 test)"""
    z, dims, gated, model = build_xl(name, torch.bfloat16, device="cuda")
    ids, mask, labels = (to_dev(z[k]) for k in ("input_ids", "attention_mask", "labels"))
    model.train()
    out = model(input_ids=ids, attention_mask=mask, labels=labels)
    ref = float(z["loss"])
    assert abs(out[0].item() - ref) < 0.03 * max(1.0, abs(ref)), (out[0].item(), ref)
    out[0].backward()
    check_grads(z, model, rel=0.05, cos_min=0.98)


@pytest.mark.parametrize("name", CASES)
def test_modes_unpadded_checkpoint_graph(name, monkeypatch):
    """fp32: unpadded = padded; set_checkpoint(True) = off (bf16, dropout on); graph-replayed generate = eager"""
    z, dims, gated, model = build_xl(name, torch.float32, device="cuda")
    ids, mask, labels = (to_dev(z[k]) for k in ("input_ids", "attention_mask", "labels"))
    model.train()
    res = []
    for flag in ("0", "1"):
        monkeypatch.setenv("LAKO_UNPAD", flag)
        model.zero_grad()
        out = model(input_ids=ids, attention_mask=mask, labels=labels)
        assert (model._engine.ctx.rag is not None) == (flag == "1")
        out[0].backward()
        res.append((out[0].item(), model._engine.G.clone()))
    monkeypatch.delenv("LAKO_UNPAD")
    assert abs(res[0][0] - res[1][0]) < 1e-5
    assert (res[1][1] - res[0][1]).abs().max().item() < 1e-4 * res[0][1].abs().max().item()
    grads = []
    for ckpt in (False, True):
        _, _, _, m = build_xl(name, torch.bfloat16, dropout=0.1, seed=3, device="cuda")
        m.set_checkpoint(ckpt)
        m.train()
        m(input_ids=ids, attention_mask=mask, labels=labels)[0].backward()
        grads.append(m._engine.G.clone())
    assert (grads[0] - grads[1]).abs().max().item() <= 1e-3 * grads[0].abs().max().item()
    model.eval()
    monkeypatch.setenv("LAKO_GEN_GRAPH", "0")
    eager = model.generate(input_ids=ids, attention_mask=mask, max_length=10).clone()
    monkeypatch.setenv("LAKO_GEN_GRAPH", "1")
    for _ in range(3):              # warm-up, capture, replay
        assert torch.equal(model.generate(input_ids=ids, attention_mask=mask, max_length=10), eager)


# ------------------------------------------------------------------------------------------------
# full size
def test_full_3b_fp32_vs_oracle():
    """named("3b"), fp32, B1 N2 L130 T8: loss, logits and every per-tensor gradient norm against the oracle (fp32 torch on the GPU)"""
    cfg = FiDConfig.named("3b", dropout_rate=0.0)
    dims = O.T5Dims(vocab_size=cfg.vocab_size, d_model=cfg.d_model, d_kv=cfg.d_kv, d_ff=cfg.d_ff, num_layers=cfg.num_layers,
                    num_decoder_layers=cfg.num_decoder_layers, num_heads=cfg.num_heads, dropout=0.0)
    w = {k: v.to(DEV) for k, v in O.init_weights(dims, seed=7).items()}
    ids, mask, labels = O.synthetic_batch(1, 2, 130, 8, dims.vocab_size, seed=8)
    model = FiDT5(cfg, dtype=torch.float32)
    model.load_t5(w)
    model = model.cuda().train()
    out = model(input_ids=ids.cuda(), attention_mask=mask.cuda(), labels=labels.cuda())
    out[0].backward()
    got_norms = {plain_name(n): float(p.grad.double().norm()) for n, p in model.named_parameters()}
    loss_mine, logits_mine = out[0].item(), out.logits.float()
    del model, out
    torch.cuda.empty_cache()
    leaves = {k: v.requires_grad_(True) for k, v in w.items()}
    with torch.device(DEV):             # (the oracle builds its masks and position tables with the default device)
        ref_loss, ref_logits = O.fid_forward(leaves, dims, ids.cuda(), mask.cuda(), labels.cuda(), training=False)
        ref_loss.backward()
    assert abs(loss_mine - ref_loss.item()) < 1e-3 * max(1.0, abs(ref_loss.item())), (loss_mine, ref_loss.item())
    torch.testing.assert_close(logits_mine, ref_logits.detach().float(), atol=2e-3, rtol=2e-3)
    for k, v in leaves.items():
        if k in got_norms:
            rn = float(v.grad.double().norm())
            assert abs(got_norms[k] - rn) <= 2e-3 * rn + 1e-6, (k, got_norms[k], rn)


@pytest.mark.parametrize("size", ["v1_1-xl", "3b"])
def test_full_size_bf16_steps_and_generate(size):
    """three AdamW steps on one fixed batch: finite, decreasing loss; then generate(max_length=8) runs"""
    cfg = FiDConfig.named(size, dropout_rate=0.0)
    model = FiDT5(cfg, dtype=torch.bfloat16, seed=1)
    model.reset_parameters()
    if not cfg.tie_word_embeddings:     # HF's untied-head init (std 1) puts the first logits at std ≈ √d_model ≈ 45: loss ≈ 200, and
        with torch.no_grad():           # AdamW steps on it overshoot; the tied head's d_model^-½ rescale gives a trainable start
            model._params_by_plain["lm_head.weight"].mul_(cfg.d_model ** -0.5)
        model._mark_stale()
    model = model.cuda().train()
    ids, mask, labels = (t.cuda() for t in O.synthetic_batch(2, 4, 130, 8, cfg.vocab_size, seed=9))
    opt = types.SimpleNamespace(optim="adamw", lr=1e-5, weight_decay=0.0, scheduler="fixed", scheduler_steps=None,
                                total_steps=10, warmup_steps=0, fixed_lr=True)
    optimizer, scheduler = U.set_optim(opt, model)
    losses = []
    for _ in range(3):
        loss = model(input_ids=ids, attention_mask=mask, labels=labels)[0]
        loss.backward()
        U.clip_grad_norm_(model, 1.0)
        optimizer.step()
        scheduler.step()
        model.zero_grad()
        losses.append(loss.item())
    assert all(np.isfinite(losses)) and losses[0] > losses[1] > losses[2], losses
    model.eval()
    toks = model.generate(input_ids=ids, attention_mask=mask, max_length=8)
    assert toks.shape[0] == 2 and toks.shape[1] <= 8
