"""-m gpu: both sides of the attention dispatch gates, on real memory.

tests/test_attn_plan_cpu.py pins WHICH kernels every gate selects; this file runs the calls, at the smallest shapes at which each gate flips.
Every call is
  1. planned: HipOps.attn_fwd_plan / attn_bwd_plan (the plan the launch consumes) must name the kernels the side is about;
  2. compared with the fp32 double (tests/ref_ops.py attn_fwd / attn_bwd) under the bounds of tests/test_kernels_gpu.py::test_attention;
  3. guarded: out, dq, dk, dv and the bias gradient sit inside larger buffers of a NaN bit pattern no result can equal, and every bit outside
     their windows must survive;
  4. poisoned: q, k, v, dO and O sit inside NaN-filled buffers: an over-read that reaches an accumulator makes an output non-finite."""
import os
import subprocess
import sys

import pytest
import torch

from lako_amd._lib import (ATTN_BWD_DKV, ATTN_BWD_DQ, ATTN_ENC_BWD_DKV, ATTN_ENC_BWD_DQ, ATTN_ENC_BWD_DQ_P, ATTN_ENC_BWD_FUSED, ATTN_ENC_FWD,
                           ATTN_ENC_FWD_C, ATTN_FWD)
from tests.ref_ops import RefOps
from tests.test_gemm_gates_gpu import untouched_outside, window
from tests.test_kernels_gpu import close, fast_bwd_kernels, planned, rnd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF, F32 = torch.bfloat16, torch.float32
GENERIC = [ATTN_BWD_DQ, ATTN_BWD_DKV]
PER_ITEM = [ATTN_ENC_BWD_DQ, ATTN_ENC_BWD_DKV]
FUSED = [ATTN_ENC_BWD_FUSED]


@pytest.fixture(scope="module")
def ops():
    from lako_amd.ops import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def ref():
    return RefOps()


def heads(rows_per_seq, Bn, H, dk, *, fill, seed=0):
    """a contiguous [Bn, rows, H, dk] bf16 view inside a poisoned (operands: NaN, outputs: guard pattern) buffer -> (view, 2-D window, buffer)"""
    w, buf = window(Bn * rows_per_seq, H * dk, BF, fill=fill, seed=seed)
    if fill == "nan":
        w.mul_(0.5)
    return w.view(Bn, rows_per_seq, H, dk), w, buf


def run_attn(ops, ref, what, Bn, H, Lq, Lk, *, fwd, bwd, bias="enc", drop=None, ring=None, dma_stage=None):
    """forward and backward of one bf16 / d_head 64 attention without mask: plans == (fwd, bwd), numbers, guards"""
    dk = 64
    q, _, _ = heads(Lq, Bn, H, dk, fill="nan", seed=1)
    k, _, _ = heads(Lk, Bn, H, dk, fill="nan", seed=2)
    v, _, _ = heads(Lk, Bn, H, dk, fill="nan", seed=3)
    kw = dict(drop=drop)
    if bias is not None:        # "enc": the encoder's table; "long": one entry more (indices are clamped: the generic kernels)
        kw.update(rel_bias=rnd(H, Lq + Lk - 1 + (bias == "long"), seed=4), rel_off=Lq - 1)
    out, outw, outbuf = heads(Lq, Bn, H, dk, fill="guard")
    stg, st = torch.zeros(Bn, H, Lq, 4, device=q.device), torch.zeros(Bn, H, Lq, 4, device=q.device)
    outr = torch.zeros(Bn, Lq, H, dk, device=q.device)
    pl = planned(ops.attn_fwd_plan, [fwd], q, k, v, out, stg, **kw)
    assert pl.launch[0].drop == (drop is not None and fwd != ATTN_FWD)
    ops.attn_fwd(q, k, v, out, stg, **kw)
    ref.attn_fwd(q, k, v, outr, st, **kw)
    untouched_outside(outw, outbuf, f"{what} out")
    close(stg[..., 0], st[..., 0], BF, f"{what} rowmax")
    close(stg[..., 1], st[..., 1], BF, f"{what} 1/rowsum", k=2)
    close(out, outr, BF, f"{what} out")
    # backward, fed the reference's forward products (as test_attention: the comparison isolates the backward kernels)
    dout, _, _ = heads(Lq, Bn, H, dk, fill="nan", seed=5)
    dout.mul_(2.0)
    o_in, o_w, _ = heads(Lq, Bn, H, dk, fill="nan", seed=6)
    o_in.copy_(outr)
    grads = [heads(L, Bn, H, dk, fill="guard") for L in (Lq, Lk, Lk)]
    (dq, dk_, dv) = (g[0] for g in grads)
    dqr, dkr, dvr = (torch.zeros(t.shape, device=q.device) for t in (q, k, v))
    drel = drelr = drelw = drelbuf = None
    if bias is not None:
        drelw, drelbuf = window(H, kw["rel_bias"].shape[1], F32, fill="guard")
        drel = drelw.zero_()
        drelr = torch.zeros_like(kw["rel_bias"])
    pl = planned(ops.attn_bwd_plan, bwd, q, k, v, o_in, dout, st, dq, dk_, dv, drel=drel, **kw)
    if ring is not None and pl.kernels == FUSED:
        assert pl.launch[0].ring == ring
    if dma_stage is not None and pl.kernels[-1] == ATTN_ENC_BWD_DKV:
        assert pl.launch[1].dma_stage == dma_stage
    ops.attn_bwd(q, k, v, o_in, dout, st, dq, dk_, dv, drel=drel, **kw)
    ref.attn_bwd(q, k, v, o_in, dout, st, dqr, dkr, dvr, drel=drelr, **kw)
    for (g, w, buf), want, nm in zip(grads, (dqr, dkr, dvr), ("dq", "dk", "dv")):
        untouched_outside(w, buf, f"{what} {nm}")
        close(g, want, BF, f"{what} {nm}", k=2)
    if drel is not None:
        untouched_outside(drelw, drelbuf, f"{what} drel")
        close(drel, drelr, BF, f"{what} drel", k=4)


# (id, environment, Bn, H, Lq, Lk, extra, forward kernel, backward kernels [default mode]) — the two or three sides of a gate next to each other
GATES = [
    # at most 256 keys
    ("keys_256", {}, 1, 2, 256, 256, {}, ATTN_ENC_FWD_C, PER_ITEM),
    ("keys_257", {}, 1, 2, 257, 257, {}, ATTN_FWD, GENERIC),
    # the one-pass backward holds 224 key rows
    ("bwd_keys_224", {}, 2, 2, 224, 224, dict(drop=(0.1, 19, 9)), ATTN_ENC_FWD_C, FUSED),
    ("bwd_keys_225", {}, 2, 2, 225, 225, dict(drop=(0.1, 19, 9)), ATTN_ENC_FWD_C, PER_ITEM),
    # one query block over more than 64 keys: the generic key-split mode
    ("q16_k64", {}, 2, 2, 16, 64, {}, ATTN_ENC_FWD_C, FUSED),
    ("q16_k65", {}, 2, 2, 16, 65, {}, ATTN_FWD, GENERIC),
    ("q17_k65", {}, 2, 2, 17, 65, {}, ATTN_ENC_FWD_C, FUSED),
    ("q16_k256", {}, 2, 2, 16, 256, {}, ATTN_FWD, GENERIC),     # (its bias gradient: the widest key range the dQ pass cuts into two chunks)
    # the encoder's bias table | one that needs index clamping | none
    ("bias_encoder", {}, 2, 2, 40, 40, {}, ATTN_ENC_FWD_C, FUSED),
    ("bias_longer", {}, 2, 2, 40, 40, dict(bias="long"), ATTN_FWD, GENERIC),
    ("bias_none", {}, 2, 2, 40, 40, dict(bias=None), ATTN_ENC_FWD_C, FUSED),
    # the persistent dQ pass from 1024 (sequence, head) items on
    ("dq_items_1024", dict(LAKO_ATTN_PERSIST="2"), 256, 4, 40, 40, dict(dma_stage=1), ATTN_ENC_FWD_C, [ATTN_ENC_BWD_DQ_P, ATTN_ENC_BWD_DKV]),
    ("dq_items_1023", dict(LAKO_ATTN_PERSIST="2"), 341, 3, 40, 40, dict(dma_stage=1), ATTN_ENC_FWD_C, PER_ITEM),
    # the slab ring of the one-pass backward
    ("ring_4", dict(LAKO_ATTN_FUSED_NST="4"), 2, 2, 64, 64, dict(drop=(0.1, 7, 8), ring=4), ATTN_ENC_FWD_C, FUSED),
    ("ring_3", dict(LAKO_ATTN_FUSED_NST="3"), 2, 2, 64, 64, dict(drop=(0.1, 7, 8), ring=3), ATTN_ENC_FWD_C, FUSED),
]


@pytest.mark.parametrize("gate", GATES, ids=[g[0] for g in GATES])
def test_attention_gate(ops, ref, gate, monkeypatch):
    what, env, Bn, H, Lq, Lk, extra, fwd, bwd = gate
    monkeypatch.setenv("LAKO_ATTN_PERSIST", env.get("LAKO_ATTN_PERSIST", "18"))
    monkeypatch.setenv("LAKO_ATTN_FUSED_NST", env.get("LAKO_ATTN_FUSED_NST", "4"))
    if fwd != ATTN_FWD:         # a fast-path side: the same kernels as the rule test_kernels_gpu.py states (which also knows LAKO_DETERMINISTIC)
        want = fast_bwd_kernels(ops, os.environ["LAKO_ATTN_PERSIST"], Bn, H, Lk)
        assert want == bwd or ops.det
        bwd = want
    if os.environ.get("LAKO_ATTN_FWD_DMA") == "0" and fwd == ATTN_ENC_FWD_C:
        fwd = ATTN_ENC_FWD
    run_attn(ops, ref, what, Bn, H, Lq, Lk, fwd=fwd, bwd=bwd, **extra)


def test_register_staging_forms(ops, ref, monkeypatch):
    """LAKO_ATTN_FWD_DMA=0 / LAKO_ATTN_DKV_DMA=0 (read once per process: test_register_staging_forms_in_a_child_process sets them): the
    per-item forward and dK/dV pass that stage their LDS images through registers; without the variables, the LDS-DMA forms"""
    monkeypatch.setenv("LAKO_ATTN_PERSIST", "0")
    fwd = ATTN_ENC_FWD if os.environ.get("LAKO_ATTN_FWD_DMA") == "0" else ATTN_ENC_FWD_C
    dma = 0 if os.environ.get("LAKO_ATTN_DKV_DMA") == "0" else 1
    bwd = fast_bwd_kernels(ops, "0", 2, 3, 100)
    run_attn(ops, ref, f"staging fwd {fwd} dkv dma {dma}", 2, 3, 100, 100, fwd=fwd, bwd=bwd, drop=(0.1, 3, 4), dma_stage=dma)
    run_attn(ops, ref, f"staging fwd {fwd} dkv dma {dma} odd", 3, 2, 37, 37, fwd=fwd, bwd=bwd, dma_stage=dma)


def test_register_staging_forms_in_a_child_process():
    env = dict(os.environ, LAKO_ATTN_FWD_DMA="0", LAKO_ATTN_DKV_DMA="0")
    env.pop("LAKO_DETERMINISTIC", None)      # (that mode never runs the fast path's dK/dV pass)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider", "-k",
                        "test_register_staging_forms and not child"], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "1 passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-1500:]
