"""T5 v1.1 / Flan-T5 readers on the MI355X: the gated-GELU kernels (lako_gated_gelu_fwd / _bwd) against torch, and the HIP engine with
the gated feed-forward and the untied LM head against the reference's fixtures (tools/make_gated_fixtures.py)."""
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
from tests.ref_ops import keep_mask
from tests.util_gated import gated_cfg, gelu_new, gelu_new_grad, load_gated
from tests.util_golden import group

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
SEED = {"gated_tiny": 21, "gated_mid": 23}


def dev(*ts):
    return [torch.as_tensor(t).to(DEV) for t in ts]


@pytest.fixture(scope="module")
def ops():
    return HipOps()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,f", [(37, 40), (256, 2048), (5, 8)])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_gated_gelu_kernels_vs_torch(ops, dtype, M, f, p):
    g = torch.Generator().manual_seed(M * 7 + f)
    pre = (torch.randn(M, 2 * f, generator=g) * 2.0).to(DEV, dtype)
    dh = torch.randn(M, f, generator=g).to(DEV, dtype)
    drop = (p, 1234, 102) if p > 0 else None
    h = torch.empty(M, f, device=DEV, dtype=dtype)
    dpre = torch.empty(M, 2 * f, device=DEV, dtype=dtype)
    ops.gated_gelu_fwd(pre, h, drop)
    ops.gated_gelu_bwd(dh, pre, dpre, drop)
    a, b, y = pre[:, :f].double().cpu(), pre[:, f:].double().cpu(), dh.double().cpu()
    keep = torch.ones(M, f, dtype=torch.bool)
    scale = 1.0
    if drop is not None:            # the lako_keep4 recipe at index m·f + n
        keep, scale = keep_mask(drop, torch.arange(M * f, dtype=torch.int64).view(M, f))
    want_h = torch.where(keep, gelu_new(a) * b * scale, torch.zeros_like(a))
    yk = torch.where(keep, y * scale, torch.zeros_like(y))
    want_da, want_db = yk * b * gelu_new_grad(a), yk * gelu_new(a)
    tol = dict(atol=2e-5, rtol=2e-5) if dtype == torch.float32 else dict(atol=2e-2, rtol=1e-2)
    torch.testing.assert_close(h.double().cpu(), want_h, **tol)
    torch.testing.assert_close(dpre[:, :f].double().cpu(), want_da, **tol)
    torch.testing.assert_close(dpre[:, f:].double().cpu(), want_db, **tol)
    if drop is not None:           # the mask itself: dropped elements are exactly zero, kept ones are not (a, b ≠ 0 a.s.)
        hc = h.cpu()
        assert (hc[~keep] == 0).all() and (hc[keep & (want_h.abs() > 1e-2)] != 0).all()


def test_gated_gelu_launch_checks(ops):
    pre = torch.zeros(4, 2 * 12, device=DEV)
    with pytest.raises(Exception, match="multiple of 8"):
        ops.gated_gelu_fwd(pre, torch.zeros(4, 12, device=DEV))
    with pytest.raises(Exception, match="pre"):
        ops.gated_gelu_fwd(torch.zeros(4, 20, device=DEV), torch.zeros(4, 16, device=DEV))


def build(name, dtype, dropout=0.0, seed=0):
    z, dims, w = load_gated(name)
    model = FiDT5(gated_cfg(dims, dropout), dtype=dtype, seed=seed)
    model.load_t5(w)
    return z, dims, w, model.cuda()


def check_grads(z, model, full_tol=None, cos_min=None):
    """every parameter gradient: element-wise (tiny: all elements; mid: norm + the stored sample), or by direction (bf16)"""
    full = "g/shared.weight" in z.files
    names = {plain_name(n): p for n, p in model.named_parameters()}
    for k, p in names.items():
        got = p.grad.detach().cpu().double().flatten()
        assert torch.isfinite(got).all(), k
        if full:
            ref = torch.from_numpy(z["g/" + k]).double().flatten()
        else:
            ref = torch.from_numpy(z["s_g/" + k]).double()
            rn = float(z["norm_g/" + k])
            gn = float(got.norm())
            assert abs(gn - rn) <= (1e-3 if cos_min is None else 0.05) * max(rn, 1e-6) + 1e-7, (k, gn, rn)
            got = got[torch.from_numpy(z["idx/" + k]).long()]
        if cos_min is None:
            torch.testing.assert_close(got, ref, **full_tol, msg=lambda m, k=k: f"{k}: {m}")
        elif ref.norm() > 1e-3 * np.sqrt(ref.numel()):
            cos = float(torch.dot(ref, got) / (ref.norm() * got.norm() + 1e-30))
            assert cos > cos_min, f"{k}: cosine {cos:.4f}"


@pytest.mark.parametrize("name", ["gated_tiny", "gated_mid"])
def test_fp32_vs_reference(name):
    z, dims, w, model = build(name, torch.float32)
    ids, mask, labels = dev(z["input_ids"], z["attention_mask"], z["labels"])
    model.train()
    out = model(input_ids=ids, attention_mask=mask, labels=labels)
    ref = float(z["loss"])
    assert abs(out[0].item() - ref) < 1e-3 * max(1.0, abs(ref)), (out[0].item(), ref)
    torch.testing.assert_close(out.logits.cpu(), torch.from_numpy(z["logits"]), atol=1e-3, rtol=1e-3)
    out[0].backward()
    check_grads(z, model, full_tol=dict(atol=1e-3, rtol=1e-3))
    model.zero_grad()
    model.eval()
    for ml in (4, 12):
        assert model.generate(input_ids=ids, attention_mask=mask, max_length=ml).cpu().tolist() == z[f"gen_{ml}"].tolist()
    B, N, L = z["input_ids"].shape
    T = z["labels"].shape[1]
    lr, wd, clip, warm, total = z["train_hparams"].tolist()
    opt = types.SimpleNamespace(optim="adamw", lr=lr, weight_decay=wd, scheduler="linear", scheduler_steps=None,
                                total_steps=int(total), warmup_steps=int(warm), fixed_lr=False)
    optimizer, scheduler = U.set_optim(opt, model)
    model.train()
    for k in range(3):
        bi, bm, bl = dev(*O.synthetic_batch(B, N, L, T, dims.vocab_size, seed=SEED[name] + 200 + k))
        loss = model(input_ids=bi, attention_mask=bm, labels=bl)[0]
        loss.backward()
        gn = U.clip_grad_norm_(model, clip)
        optimizer.step()
        scheduler.step()
        model.zero_grad()
        assert abs(loss.item() - z["train_losses"][k]) < 1e-3 * max(1.0, z["train_losses"][k])
        assert abs(gn.item() - z["train_gnorms"][k]) < 2e-3 * max(1.0, z["train_gnorms"][k])
    for n, p in model.named_parameters():
        k = plain_name(n)
        got = p.detach().cpu().flatten()
        if "w_step3/" + k in z.files:
            want = torch.from_numpy(z["w_step3/" + k]).flatten()
        else:
            got, want = got[torch.from_numpy(z["idx/" + k]).long()], torch.from_numpy(z["s_w_step3/" + k])
        torch.testing.assert_close(got, want, atol=1e-3, rtol=1e-3, msg=lambda m, k=k: f"{k}: {m}")


@pytest.mark.parametrize("name", ["gated_tiny", "gated_mid"])
def test_bf16_vs_reference(name):
    """bf16 bounds: loss within 3 %, every gradient's direction cosine > 0.98 (mid: on the stored sample, norm within 5 %)"""
    z, dims, w, model = build(name, torch.bfloat16)
    ids, mask, labels = dev(z["input_ids"], z["attention_mask"], z["labels"])
    model.train()
    out = model(input_ids=ids, attention_mask=mask, labels=labels)
    ref = float(z["loss"])
    assert abs(out[0].item() - ref) < 0.03 * max(1.0, abs(ref)), (out[0].item(), ref)
    out[0].backward()
    check_grads(z, model, cos_min=0.98)


def test_modes_unpadded_checkpoint_graph(monkeypatch):
    """gated_mid shapes, fp32: unpadded = padded (dropout off); set_checkpoint(True) = off (dropout on: the recomputed
    activation regenerates its mask); graph-replayed generate = eager"""
    z, dims, w, model = build("gated_mid", torch.float32, dropout=0.0)
    ids, mask, labels = dev(z["input_ids"], z["attention_mask"], z["labels"])
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
        _, _, _, m = build("gated_mid", torch.bfloat16, dropout=0.1, seed=3)
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
    assert model._engine._workspace(("gen",) + tuple(ids.shape) + (10,))["g.graphs"]


def test_fp8_refused_for_gated():
    z, dims, w = load_gated("gated_tiny")
    model = FiDT5(gated_cfg(dims), dtype=torch.bfloat16, fp8=True).cuda()
    ids, mask, labels = dev(z["input_ids"], z["attention_mask"], z["labels"])
    with pytest.raises(ValueError, match="gated"):
        model(input_ids=ids, attention_mask=mask, labels=labels)


_DET_CHILD = r"""
import hashlib, json, os, sys, torch
sys.path.insert(0, {root!r})
from lako_amd import FiDT5, util as U
from oracle import fid_t5_oracle as O
from tests.util_gated import gated_cfg, load_gated
import types
out = []
for fuse in ("1", "1", "0"):      # twice with the fused encoder epilogues, once with the standalone kernels
    os.environ["LAKO_FUSE_GATED"] = fuse
    z, dims, w = load_gated("gated_mid")
    m = FiDT5(gated_cfg(dims, 0.1), dtype=torch.bfloat16, seed=5)
    m.load_t5(w)
    m = m.cuda().train()
    opt = types.SimpleNamespace(optim="adamw", lr=1e-3, weight_decay=1e-2, scheduler="linear", scheduler_steps=None, total_steps=10,
                                warmup_steps=0, fixed_lr=False)
    o, s = U.set_optim(opt, m)
    losses = []
    for k in range(1):
        bi, bm, bl = (t.cuda() for t in O.synthetic_batch(2, 3, 40, 6, dims.vocab_size, seed=300 + k))
        loss = m(input_ids=bi, attention_mask=bm, labels=bl)[0]
        loss.backward()
        grads = hashlib.sha1(m._engine.G.cpu().numpy().tobytes()).hexdigest()
        U.clip_grad_norm_(m, 1.0)
        o.step(); s.step(); m.zero_grad()
        losses.append(loss.item().hex())
    out.append(dict(losses=losses, grads=grads, w=hashlib.sha1(m._engine.P.cpu().numpy().tobytes()).hexdigest()))
print(json.dumps(out))
"""


def test_deterministic_mode_repeats_bit_for_bit_and_fused_equals_standalone():
    """LAKO_DETERMINISTIC=1, bf16, dropout on, gated_mid shapes (ragged encoder rows): a training step repeats bit for bit, and the fused
    encoder epilogues (LAKO_FUSE_GATED=1) give bit for bit the loss, gradients and updated weights of the standalone kernels (=0)"""
    r = subprocess.run([sys.executable, "-c", _DET_CHILD.format(root=ROOT)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, LAKO_DETERMINISTIC="1"), cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    a, b, c = json.loads(r.stdout.strip().splitlines()[-1])
    assert a == b
    assert a == c


@pytest.mark.parametrize("M", [512, 333])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_fused_gated_epilogues_bit_identical(ops, M, p):
    """encoder shapes (d 768, f 2048), 256-aligned and ragged M: pre and h of the fused forward product, and dpre of the fused backward
    product, equal the same four-wave product (gemm_nt_four, what LAKO_FUSE_GATED=0 runs) + the standalone kernel bit for bit"""
    d, f = 768, 2048
    g = torch.Generator().manual_seed(M + int(p * 10))
    xn = (torch.randn(M, d, generator=g)).to(DEV, torch.bfloat16)
    wi = (torch.randn(2 * f, d, generator=g) * d ** -0.5).to(DEV, torch.bfloat16)
    dy = (torch.randn(M, d, generator=g)).to(DEV, torch.bfloat16)
    wo_t = (torch.randn(f, d, generator=g) * f ** -0.5).to(DEV, torch.bfloat16)
    drop = (p, 99, 110) if p > 0 else None
    assert ops.gated_fused_ok(xn, wi, f)
    pre0, h0 = torch.empty(M, 2 * f, device=DEV, dtype=torch.bfloat16), torch.empty(M, f, device=DEV, dtype=torch.bfloat16)
    ops.gemm_nt_four(xn, wi, pre0)
    ops.gated_gelu_fwd(pre0, h0, drop)
    pre1, h1 = torch.full_like(pre0, 7.0), torch.full_like(h0, 7.0)
    from lako_amd._lib import NT_FOUR, NT_FOUR_GATED
    old = ops.tuning.nt_variant
    ops.tuning.nt_variant = 9           # (what gemm_nt_four runs under)
    assert (ops.gemm_nt_plan(xn, wi, pre0).kernel, ops.gemm_nt_plan(xn, wi, pre0).tile_rows) == (NT_FOUR, 256)
    ops.tuning.nt_variant = old
    assert ops.gemm_nt_gated_plan(xn, wi, pre1, h1, drop).kernel == NT_FOUR_GATED
    ops.gemm_nt_gated(xn, wi, pre1, h1, drop)
    assert torch.equal(pre0, pre1) and torch.equal(h0, h1)
    dh = torch.empty(M, f, device=DEV, dtype=torch.bfloat16)
    ops.gemm_nt_four(dy, wo_t, dh)
    dpre0 = torch.empty_like(pre0)
    ops.gated_gelu_bwd(dh, pre0, dpre0, drop)
    dpre1 = torch.full_like(pre0, 7.0)
    assert ops.gemm_nt_gated_plan(dy, wo_t, dpre1, pre0, drop, backward=True).kernel == NT_FOUR_GATED
    ops.gemm_nt_gated(dy, wo_t, dpre1, pre0, drop, backward=True)
    assert torch.equal(dpre0, dpre1)


def test_train_reader_driver_v1_1(tmp_path):
    """The checkpoint path of train_reader.py for a v1.1 model: a trained v1_1-small model written by util.save (what the driver calls —
    like the reference it writes only when the dev score improves, which synthetic batches never do) → train_reader.py --model_size v1_1-small
    resumes from it (util.load) → FiDT5.from_pretrained (test_reader.py's loader) gives back a gated, untied model with the trained weights"""
    cfg = FiDConfig.named("v1_1-small", dropout_rate=0.0)
    m = FiDT5(cfg, dtype=torch.bfloat16, seed=1).cuda().train()
    opt = types.SimpleNamespace(optim="adamw", lr=1e-3, weight_decay=1e-4, scheduler="linear", scheduler_steps=None, total_steps=6,
                                warmup_steps=0, fixed_lr=False)
    optimizer, scheduler = U.set_optim(opt, m)
    ids, mask, labels = dev(*O.synthetic_batch(2, 3, 40, 6, cfg.vocab_size, seed=9))
    m(input_ids=ids, attention_mask=mask, labels=labels)[0].backward()
    optimizer.step()
    scheduler.step()
    U.save(m, optimizer, scheduler, 1, 0.0, opt, str(tmp_path / "manual"), "step-1")
    ck = tmp_path / "manual" / "checkpoint" / "latest"
    base = [sys.executable, os.path.join(ROOT, "train_reader.py"), "--per_gpu_batch_size", "2", "--n_context", "3",
            "--text_maxlength", "40", "--optim", "adamw", "--scheduler", "linear", "--lr", "1e-3", "--epochs", "1",
            "--synthetic", "2,3,40,6", "--steps", "3", "--checkpoint_dir", str(tmp_path), "--name", "run"]
    r = subprocess.run(base + ["--model_size", "v1_1-small", "--model_path", str(ck)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "model loaded from" in r.stderr and "samples/s" in r.stderr
    back = FiDT5.from_pretrained(os.path.realpath(str(ck)), dtype=torch.bfloat16)
    assert back.config.gated and not back.config.tie_word_embeddings
    sd, want = back.state_dict(), {k: v.detach().cpu() for k, v in m.state_dict().items()}
    assert sd["lm_head.weight"].data_ptr() != sd["shared.weight"].data_ptr()
    assert not torch.equal(sd["lm_head.weight"], sd["shared.weight"])
    for k, v in want.items():
        assert torch.equal(sd[k], v), k
    back = back.cuda().eval()
    assert back.generate(input_ids=ids, attention_mask=mask, max_length=6).shape[0] == 2
