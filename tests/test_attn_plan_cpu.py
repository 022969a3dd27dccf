"""The attention dispatch as a decision table, checked on a host without a GPU.

lako_attn_fwd_plan / lako_attn_bwd_plan go through the validation and the decision code of lako_attn_fwd / lako_attn_bwd and launch nothing
(include/lako_hip.h "plan queries"), so every gate can be pinned here with pointer VALUES that are never dereferenced.  The expected kernels
are what the written contract says — the comment on lako_attn_fwd_t ("bf16 / d_head 64 / <= 256 keys / no key mask / no causal mask / no
score capture takes the fast path"), DESIGN.md §3's attention rows and the comments at the gates in csrc/attn_enc.hip (why one query block
over more than 64 keys goes to the generic key-split mode, why the one-pass backward stops at 224 key rows, which passes LAKO_ATTN_PERSIST
makes persistent and from how many (sequence, head) items) — not a reading of attn_fwd_plan: a gate that drifts (too tight: the fast kernel
is silently no longer used; too loose: a kernel takes a shape its LDS layout does not hold) fails a row here, where the result-only GPU tests
keep passing.  Byte counts are not pinned; every plan is checked structurally instead (check_plan)."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from lako_amd import _lib
from lako_amd._lib import (ATTN_BWD_DKV, ATTN_BWD_DQ, ATTN_ENC_BWD_DKV, ATTN_ENC_BWD_DKV_P, ATTN_ENC_BWD_DQ, ATTN_ENC_BWD_DQ_P,
                           ATTN_ENC_BWD_FUSED, ATTN_ENC_FWD, ATTN_ENC_FWD_C, ATTN_ENC_FWD_P, ATTN_FWD, LAKO_BF16, LAKO_F32, AttnBwd, AttnFwd,
                           AttnPlan)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_BADARG, E_ALIGN, E_UNSUPPORTED = 0, -1, -2, -4
LDS_MAX = 163840        # bytes of LDS one gfx950 workgroup can allocate
OFFS_MAX = 64           # csrc/attn_shared.h: batch rows per workgroup (+1) whose ragged offsets are staged in LDS
DET_SLOTS = 16384       # csrc/det.h: fixed-point slots of the deterministic bias gradient

# never dereferenced: far apart, 4 KiB aligned
PQ, PK, PV, PO, PDO, PLSE, PDQ, PDK, PDV, PREL, PDREL, PMASK, PSC, PQOFF, PKOFF = (0x100000000000 + i * 0x010000000000 for i in range(15))
GENERIC_BWD = [ATTN_BWD_DQ, ATTN_BWD_DKV]
PERSISTENT = (ATTN_ENC_FWD_P, ATTN_ENC_BWD_DQ_P, ATTN_ENC_BWD_DKV_P, ATTN_ENC_BWD_FUSED)


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["bash", os.path.join(ROOT, "lako_amd", "csrc", "build.sh")], check=True)
    _lib._lib = None
    return _lib.load()


@pytest.fixture(autouse=True)
def _default_per_call_knobs(monkeypatch):
    monkeypatch.delenv("LAKO_ATTN_PERSIST", raising=False)
    monkeypatch.delenv("LAKO_ATTN_FUSED_NST", raising=False)


def env_is_zero(name):
    """the library's reading of a switch-off knob: set, and atoi() of it is 0"""
    v = os.environ.get(name)
    if v is None:
        return False
    try:
        return int(v) == 0
    except ValueError:
        return True


def cdiv(a, b):
    return -(-a // b)


def mk(Bn, H, Lq, Lk, *, dk=64, dtype=LAKO_BF16, bias="enc", mask=False, causal=False, capture=False, p=0.0, layout="padded", drel=True,
       token_stride=None):
    """(lako_attn_fwd_t, lako_attn_bwd_t) of one attention over fake operands.  bias: "enc" = the encoder's table (R = Lq + Lk - 1,
    rel_off = Lq - 1), None, or (R, rel_off).  layout: "padded" (q | k | v columns of one [Bn, L, 3·H·dk] buffer when Lq == Lk, else q and
    k | v buffers), "ragged" (q_off and k_off), "q_only" / "k_only" (one offset array), "odd_batch" (padded, batch stride = whole rows + 8).
    token_stride: {"q" | "k" | "v" | "o": elements} overrides one tensor's token stride (its batch stride stays that many whole rows)"""
    inner = H * dk
    if Lq == Lk:
        qst = kst = 3 * inner
    else:
        qst, kst = inner, 2 * inner
    qsb, ksb = Lq * qst, Lk * kst
    if layout == "odd_batch":
        qsb, ksb = qsb + 8, ksb + 8
    f, b = AttnFwd(), AttnBwd()
    for s in (f, b):
        s.q, s.k, s.v, s.lse = PQ, PK, PV, PLSE
        s.q_stride_b, s.q_stride_t, s.o_stride_b, s.o_stride_t = qsb, qst, Lq * inner, inner
        s.k_stride_b, s.k_stride_t, s.v_stride_b, s.v_stride_t = ksb, kst, ksb, kst
        for t, st in (token_stride or {}).items():
            setattr(s, t + "_stride_t", st)
            setattr(s, t + "_stride_b", (Lq if t in "qo" else Lk) * st)
        if bias is not None:
            s.rel_bias = PREL
            s.R, s.rel_off = (Lq + Lk - 1, Lq - 1) if bias == "enc" else bias
        if mask:
            s.key_mask = PMASK
        s.causal = int(causal)
        s.Bn, s.H, s.Lq, s.Lk, s.d_head, s.dtype = Bn, H, Lq, Lk, dk, dtype
        s.drop = _lib.Dropout(p, 5, 6)
        if layout in ("ragged", "q_only"):
            s.q_off = PQOFF
        if layout in ("ragged", "k_only"):
            s.k_off = PKOFF
    f.out = PO
    if capture:
        f.scores_out = PSC
    b.out, b.dout, b.dq_out, b.dk_out, b.dv_out = PO, PDO, PDQ, PDK, PDV
    if bias is not None and drel:
        b.drel = PDREL
    return f, b


def check_plan(pl, s):
    """what must hold for ANY plan of the call `s`, whichever kernels it names"""
    assert 1 <= pl.n_launches <= 2
    for l in pl.launches:
        assert 0 < l.lds <= LDS_MAX, l
        assert l.block in (256, 512, 1024) and l.gx >= 1 and l.gy >= 1 and l.gz >= 1, l
        assert l.chunk_rows % 32 == 0 and 32 <= l.chunk_rows <= 256, l
        assert l.bn_per_wg <= OFFS_MAX - 1, l
        assert l.ring == 0 or (l.kernel == ATTN_ENC_BWD_FUSED and l.ring in (3, 4)), l
        if l.ring == 4:
            assert l.lds <= 160 * 1024, l
        if l.kernel in PERSISTENT:      # one workgroup per CU walking the sequences of one head: whole heads, at most the 256 CUs
            assert (l.gy, l.gz) == (1, 1) and l.gx % s.H == 0 and s.H <= l.gx <= max(256, s.H) and l.gx // s.H <= s.Bn, l
        elif l.kernel == ATTN_ENC_BWD_DQ:        # every query block of a sequence in one workgroup, bn_per_wg sequences each
            assert (l.gx, l.gy) == (1, s.H) and l.bn_per_wg >= 1 and l.gz * l.bn_per_wg >= s.Bn, l
        else:                                    # a grid over (16-row blocks, heads, sequences) that covers all of them
            rows = s.Lk if l.kernel in (ATTN_BWD_DKV, ATTN_ENC_BWD_DKV) else s.Lq
            gx, gy, gz = (l.grid_x, s.H, l.grid_z) if l.grid_x > 0 else (l.gx, l.gy, l.gz)
            if l.grid_x > 0:
                assert l.kernel == ATTN_BWD_DQ and (l.gy, l.gz) == (1, 1) and l.gx >= gx * gy * gz, l
            assert l.blocks_per_wg >= 1 and gx * l.blocks_per_wg >= cdiv(rows, 16) and gy == s.H, l
            assert gz * max(l.bn_per_wg, 1) >= s.Bn, l
        if l.kernel >= ATTN_ENC_FWD:
            assert l.drop == (s.drop.p > 0) and (l.R, l.rel_off) == (s.Lq + s.Lk - 1, s.Lq - 1), l   # the encoder's indexing, table or not
            assert l.drel == (1 if getattr(s, "drel", None) else 0), l
        else:
            assert (l.R, l.rel_off) == ((s.R, s.rel_off) if s.rel_bias else (0, s.rel_off)), l


def fwd_plan(L, f):
    pl = AttnPlan()
    rc = L.lako_attn_fwd_plan(C.byref(f), C.byref(pl))
    if rc == OK:
        assert pl.n_launches == 1
        check_plan(pl, f)
    else:
        assert bytes(pl) == bytes(C.sizeof(pl)), "a refused query leaves a zeroed plan"
    return rc, pl


def bwd_plan(L, b):
    pl = AttnPlan()
    rc = L.lako_attn_bwd_plan(C.byref(b), C.byref(pl))
    if rc == OK:
        check_plan(pl, b)
    else:
        assert bytes(pl) == bytes(C.sizeof(pl)), "a refused query leaves a zeroed plan"
    return rc, pl


def kernels(L, *a, **kw):
    """(forward kernel, [backward kernels]) of one call"""
    f, b = mk(*a, **kw)
    (rcf, pf), (rcb, pb) = fwd_plan(L, f), bwd_plan(L, b)
    assert rcf == OK and rcb == OK, (rcf, rcb)
    return pf.kernels[0], pb.kernels


def is_fast(L, *a, **kw):
    """True: forward and backward on the fast path; False: both on the generic kernels (anything else fails)"""
    kf, kb = kernels(L, *a, **kw)
    fast = kf >= ATTN_ENC_FWD
    assert kf == ATTN_FWD or fast
    assert all(k >= ATTN_ENC_BWD_DQ for k in kb) if fast and not L.lako_deterministic() else True
    if not fast:
        assert kb == GENERIC_BWD
    return fast


def two_pass(L, *expected):
    """the backward kernels of a fast-path call whose one-pass kernel does not apply: the named two passes — in LAKO_DETERMINISTIC mode the
    generic kernels (the fast path's two-pass kernels add their bias gradient by float atomics in arrival order: DESIGN.md §4)"""
    return GENERIC_BWD if L.lako_deterministic() else list(expected)


needs_fast = pytest.mark.skipif(env_is_zero("LAKO_ATTN_FAST"), reason="LAKO_ATTN_FAST=0: everything on the generic kernels (test_knob_fast)")


# ---- the fast-path gate: one row per term, both sides ---------------------------------------------------------------------------------
@needs_fast
def test_fast_path_gate(L):
    assert is_fast(L, 2, 4, 200, 200)                                            # bf16, d_head 64, the encoder's bias table, <= 256 keys
    assert not is_fast(L, 2, 4, 200, 200, dtype=LAKO_F32)
    assert not is_fast(L, 2, 4, 200, 200, dk=32) and not is_fast(L, 2, 4, 200, 200, dk=128)
    assert not is_fast(L, 2, 4, 200, 200, causal=True)
    assert not is_fast(L, 2, 4, 200, 200, mask=True)
    assert is_fast(L, 2, 4, 256, 256) and not is_fast(L, 2, 4, 256, 257) and not is_fast(L, 2, 4, 257, 256)
    assert is_fast(L, 2, 4, 200, 200, bias=None)
    assert not is_fast(L, 2, 4, 200, 200, bias=(400, 199)) and not is_fast(L, 2, 4, 200, 200, bias=(399, 198))   # R, rel_off: a table that needs clamping
    # one query block over many keys is the generic key-split mode's
    assert is_fast(L, 2, 4, 16, 64) and not is_fast(L, 2, 4, 16, 65) and is_fast(L, 2, 4, 17, 65)
    assert is_fast(L, 21845, 3, 40, 40) and not is_fast(L, 16384, 4, 40, 40)     # Bn·H 65535 | 65536
    # score capture exists in the forward only: that call alone leaves the fast path
    f, _ = mk(2, 4, 200, 200, capture=True)
    assert fwd_plan(L, f)[1].kernels == [ATTN_FWD] and fwd_plan(L, f)[1].launch[0].capture == 1
    assert fwd_plan(L, mk(2, 4, 200, 200, dtype=LAKO_F32)[0])[1].launch[0].capture == 0


# ---- forward ----------------------------------------------------------------------------------------------------------------------------
@needs_fast
def test_forward_kernels(L, monkeypatch):
    fk = lambda *a, **kw: fwd_plan(L, mk(*a, **kw)[0])[1].kernels[0]      # noqa: E731
    per_item = ATTN_ENC_FWD if env_is_zero("LAKO_ATTN_FWD_DMA") else ATTN_ENC_FWD_C
    assert fk(320, 12, 200, 200, layout="ragged", p=0.1) == per_item            # the default (18) keeps the forward per item
    monkeypatch.setenv("LAKO_ATTN_PERSIST", "1")
    assert fk(256, 4, 40, 40) == ATTN_ENC_FWD_P and fk(341, 3, 40, 40) == per_item          # Bn·H 1024 | 1023
    assert fk(4, 257, 40, 40) == per_item and fk(4, 256, 40, 40) == ATTN_ENC_FWD_P          # one workgroup per CU: at most 256 heads
    monkeypatch.setenv("LAKO_ATTN_PERSIST", "9")                                           # bit 8: small launches too
    assert fk(2, 4, 40, 40) == ATTN_ENC_FWD_P and fk(2, 257, 40, 40) == per_item
    monkeypatch.setenv("LAKO_ATTN_PERSIST", "14")                                          # every bit but the forward's
    assert fk(256, 4, 40, 40) == per_item
    f, _ = mk(2, 4, 200, 200, p=0.1)
    assert fwd_plan(L, f)[1].launch[0].drop == 1 and fwd_plan(L, mk(2, 4, 200, 200)[0])[1].launch[0].drop == 0


# ---- backward ---------------------------------------------------------------------------------------------------------------------------
@needs_fast
def test_backward_default_kernels(L):
    bk = lambda *a, **kw: bwd_plan(L, mk(*a, **kw)[1])[1]      # noqa: E731
    pl = bk(2, 2, 224, 224, layout="ragged")
    assert pl.kernels == [ATTN_ENC_BWD_FUSED] and pl.n_launches == 1             # the one-pass kernel holds up to 224 key rows
    assert bk(2, 2, 225, 225, layout="ragged").kernels == two_pass(L, ATTN_ENC_BWD_DQ, ATTN_ENC_BWD_DKV)
    assert bk(2, 2, 193, 193, layout="ragged").kernels == [ATTN_ENC_BWD_FUSED] and bk(2, 2, 192, 192).kernels == [ATTN_ENC_BWD_FUSED]
    # beyond it: the persistent dQ pass from 1024 (sequence, head) items on, the dK/dV pass per item with its images by LDS-DMA
    big, small = bk(256, 4, 225, 225, layout="ragged"), bk(341, 3, 225, 225, layout="ragged")
    assert big.kernels == two_pass(L, ATTN_ENC_BWD_DQ_P, ATTN_ENC_BWD_DKV) and small.kernels == two_pass(L, ATTN_ENC_BWD_DQ, ATTN_ENC_BWD_DKV)
    if not L.lako_deterministic():
        want = 0 if env_is_zero("LAKO_ATTN_DKV_DMA") else 1
        assert big.launch[1].dma_stage == want and small.launch[1].dma_stage == want and big.launch[0].dma_stage == 0
    # config 2 of the benchmark: 320 passages x 12 heads of <= 200 tokens, ragged, dropout 0.1
    pl = bk(320, 12, 200, 200, layout="ragged", p=0.1)
    assert pl.kernels == [ATTN_ENC_BWD_FUSED] and pl.launch[0].drop == 1 and pl.launch[0].ring in (3, 4) and pl.launch[0].drel == 1
    assert (pl.launch[0].rq, pl.launch[0].rk) == (0, 0)                          # ragged: rows come from the offsets
    assert bk(320, 12, 200, 200, layout="ragged", bias=None).launch[0].drel == 0 and bk(320, 12, 200, 200, layout="ragged", drel=False).launch[0].drel == 0


@needs_fast
def test_backward_layouts_of_the_one_pass_kernel(L):
    """one addressing form, row offset x token stride: ragged with BOTH offset arrays, or padded with batch strides of whole rows"""
    bk = lambda *a, **kw: bwd_plan(L, mk(*a, **kw)[1])[1]      # noqa: E731
    assert bk(2, 2, 200, 200, layout="ragged").kernels == [ATTN_ENC_BWD_FUSED]
    pl = bk(3, 2, 200, 200, layout="padded")
    assert pl.kernels == [ATTN_ENC_BWD_FUSED] and (pl.launch[0].rq, pl.launch[0].rk) == (200, 200)      # rows per sequence
    pl = bk(3, 2, 100, 200, layout="padded")
    assert pl.kernels == [ATTN_ENC_BWD_FUSED] and (pl.launch[0].rq, pl.launch[0].rk) == (100, 200)
    for layout in ("odd_batch", "q_only", "k_only"):
        assert bk(3, 2, 200, 200, layout=layout).kernels == two_pass(L, ATTN_ENC_BWD_DQ, ATTN_ENC_BWD_DKV), layout


@needs_fast
def test_token_strides_beyond_the_32_bit_range(L, monkeypatch):
    """the LDS-DMA forms and the persistent kernels address 256 rows of a tensor through one 32-bit buffer descriptor: 256 x the token stride
    in bytes must stay below 2^31 (bf16: fewer than 2^22 elements) — k and v in the forward and the dQ pass, q and dO / O in the dK/dV pass,
    all four in the one-pass backward.  Beyond it the register-staging forms run."""
    if L.lako_deterministic():
        return
    far, near = 1 << 22, (1 << 22) - 8
    per_item = ATTN_ENC_FWD if env_is_zero("LAKO_ATTN_FWD_DMA") else ATTN_ENC_FWD_C
    dma = 0 if env_is_zero("LAKO_ATTN_DKV_DMA") else 1
    for t in "qkvo":
        monkeypatch.setenv("LAKO_ATTN_PERSIST", "18")
        assert bwd_plan(L, mk(2, 4, 200, 200, token_stride={t: near})[1])[1].kernels == [ATTN_ENC_BWD_FUSED], t
        pl = bwd_plan(L, mk(2, 4, 200, 200, token_stride={t: far})[1])[1]
        assert pl.kernels == [ATTN_ENC_BWD_DQ, ATTN_ENC_BWD_DKV] and pl.launch[1].dma_stage == (dma if t in "kv" else 0), t
        assert fwd_plan(L, mk(2, 4, 200, 200, token_stride={t: far})[0])[1].kernels == [ATTN_ENC_FWD if t in "kv" else per_item], t
        monkeypatch.setenv("LAKO_ATTN_PERSIST", "15")
        assert fwd_plan(L, mk(2, 4, 200, 200, token_stride={t: near})[0])[1].kernels == [ATTN_ENC_FWD_P], t
        assert fwd_plan(L, mk(2, 4, 200, 200, token_stride={t: far})[0])[1].kernels == [ATTN_ENC_FWD if t in "kv" else ATTN_ENC_FWD_P], t
        assert bwd_plan(L, mk(2, 4, 200, 200, token_stride={t: near})[1])[1].kernels == [ATTN_ENC_BWD_DQ_P, ATTN_ENC_BWD_DKV_P], t
        want = [ATTN_ENC_BWD_DQ, ATTN_ENC_BWD_DKV_P] if t in "kv" else [ATTN_ENC_BWD_DQ_P, ATTN_ENC_BWD_DKV]
        assert bwd_plan(L, mk(2, 4, 200, 200, token_stride={t: far})[1])[1].kernels == want, t


@needs_fast
def test_backward_kernels_the_gpu_tests_select(L, monkeypatch):
    """LAKO_ATTN_PERSIST 0 / 15 / 16 and LAKO_ATTN_FUSED_NST 3 / 4 as tests/test_kernels_gpu.py sets them (read on every call)"""
    bk = lambda *a, **kw: bwd_plan(L, mk(*a, **kw)[1])[1]      # noqa: E731
    det = bool(L.lako_deterministic())
    monkeypatch.setenv("LAKO_ATTN_PERSIST", "0")
    if not det:       # (the deterministic mode takes the one-pass kernel wherever it applies: test_knob_deterministic)
        assert bk(2, 12, 200, 200).kernels == [ATTN_ENC_BWD_DQ, ATTN_ENC_BWD_DKV] and bk(256, 4, 40, 40).kernels == [ATTN_ENC_BWD_DQ, ATTN_ENC_BWD_DKV]
    monkeypatch.setenv("LAKO_ATTN_PERSIST", "15")
    if not det:
        assert bk(2, 12, 200, 200).kernels == [ATTN_ENC_BWD_DQ_P, ATTN_ENC_BWD_DKV_P] and bk(2, 2, 256, 256).kernels == [ATTN_ENC_BWD_DQ_P, ATTN_ENC_BWD_DKV_P]
        assert bk(2, 257, 40, 40).kernels == [ATTN_ENC_BWD_DQ, ATTN_ENC_BWD_DKV]
    monkeypatch.setenv("LAKO_ATTN_PERSIST", "2")
    assert bk(256, 4, 225, 225).kernels == two_pass(L, ATTN_ENC_BWD_DQ_P, ATTN_ENC_BWD_DKV)
    assert bk(341, 3, 225, 225).kernels == two_pass(L, ATTN_ENC_BWD_DQ, ATTN_ENC_BWD_DKV)
    monkeypatch.setenv("LAKO_ATTN_PERSIST", "7")
    assert bk(256, 4, 40, 40).kernels == two_pass(L, ATTN_ENC_BWD_DQ_P, ATTN_ENC_BWD_DKV_P)
    assert bk(45, 12, 200, 200, layout="ragged").kernels == two_pass(L, ATTN_ENC_BWD_DQ, ATTN_ENC_BWD_DKV)
    monkeypatch.setenv("LAKO_ATTN_PERSIST", "16")
    for nst in ("4", "3"):
        monkeypatch.setenv("LAKO_ATTN_FUSED_NST", nst)
        for case in ((2, 12, 200, 200), (3, 3, 200, 200), (2, 4, 37, 37), (2, 2, 130, 130), (2, 2, 224, 224)):
            pl = bk(*case)
            assert pl.kernels == [ATTN_ENC_BWD_FUSED], case
            assert pl.launch[0].ring == 3 if nst == "3" else pl.launch[0].ring in (3, 4)
        assert bk(2, 4, 37, 37).launch[0].ring == int(nst)                        # a short sequence: four stages fit
        # 256 keys are 256 key rows: past the one-pass kernel, and bits 2 / 4 are clear — the per-item two-pass kernels
        assert bk(1, 2, 256, 256).kernels == two_pass(L, ATTN_ENC_BWD_DQ, ATTN_ENC_BWD_DKV)
        assert bk(2, 257, 40, 40).kernels == two_pass(L, ATTN_ENC_BWD_DQ, ATTN_ENC_BWD_DKV)      # more heads than CUs


def test_decoder_attention_runs_the_generic_kernels(L):
    """decoder self-attention (causal) and cross-attention (`dec_self`, `cross`, `decode_step` of tests/test_kernels_gpu.py::ATTN_CASES);
    one query block (Lq <= 16) splits the KEYS over the workgroup's four waves and merges them through LDS"""
    assert kernels(L, 4, 12, 7, 7, causal=True) == (ATTN_FWD, GENERIC_BWD)
    assert kernels(L, 3, 4, 5, 600, bias=None, mask=True) == (ATTN_FWD, GENERIC_BWD)
    assert kernels(L, 4, 8, 1, 23, bias=(99, 27)) == (ATTN_FWD, GENERIC_BWD)
    for case, kw in (((3, 4, 5, 600), dict(bias=None, mask=True)), ((4, 8, 1, 23), dict(bias=(99, 27)))):
        Bn, H, Lq, Lk = case
        one, two = mk(Bn, H, Lq, Lk, **kw), mk(Bn, H, 17, Lk, **kw)               # one query block | two: same chunk, same table
        f1, f2 = fwd_plan(L, one[0])[1].launch[0], fwd_plan(L, two[0])[1].launch[0]
        q1, q2 = bwd_plan(L, one[1])[1].launch[0], bwd_plan(L, two[1])[1].launch[0]
        assert f1.gx == 1 and q1.gx == 1 and f1.chunk_rows == f2.chunk_rows and q1.chunk_rows == q2.chunk_rows
        assert f1.lds > f2.lds and q1.lds > q2.lds, "the merge scratch of the key-split mode"
    # the key-split mode sums its bias gradient by LDS atomics, which the dQ pass does when the keys take more than one chunk: with a bias
    # gradient, one query block over 65 ... 256 keys gets two chunks; without one, or with two query blocks, one chunk holds all keys
    def chunk(Lq, Lk, **kw):
        l = bwd_plan(L, mk(2, 2, Lq, Lk, mask=True, **kw)[1])[1].launch[0]
        assert l.kernel == ATTN_BWD_DQ
        return l.chunk_rows
    for Lk in (65, 96, 97, 256):
        assert Lk / 2 <= chunk(16, Lk) < Lk <= chunk(16, Lk, drel=False) == chunk(17, Lk), Lk
    # the dQ pass with a bias gradient walks several batch rows per workgroup once there are more than ~1024 workgroups
    q = bwd_plan(L, mk(320, 12, 200, 200, mask=True)[1])[1].launch[0]
    assert q.kernel == ATTN_BWD_DQ and q.blocks_per_wg == 4 and 1 < q.bn_per_wg <= OFFS_MAX - 1 and q.grid_x == cdiv(200, 64)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_carry_the_codes_of_the_launching_calls(L):
    """every refusal happens before the first launch, so the launching entry point can be called with a null stream on this host"""
    def both(f=None, b=None):
        out = []
        if f is not None:
            rc = fwd_plan(L, f)[0]
            assert rc != OK and L.lako_attn_fwd(C.byref(f), None) == rc
            out.append(rc)
        if b is not None:
            rc = bwd_plan(L, b)[0]
            assert rc != OK and L.lako_attn_bwd(C.byref(b), None) == rc
            out.append(rc)
        return out

    pl = AttnPlan()
    assert L.lako_attn_fwd_plan(None, C.byref(pl)) == E_BADARG and L.lako_attn_bwd_plan(None, C.byref(pl)) == E_BADARG
    f, b = mk(2, 4, 40, 40)
    assert L.lako_attn_fwd_plan(C.byref(f), None) == E_BADARG and L.lako_attn_bwd_plan(C.byref(b), None) == E_BADARG
    assert L.lako_attn_fwd(None, None) == E_BADARG and L.lako_attn_bwd(None, None) == E_BADARG
    assert both(*mk(0, 4, 40, 40)) == [E_BADARG] * 2 and both(*mk(2, 65536, 40, 40)) == [E_BADARG] * 2
    assert both(*mk(2, 4, 40, 40, dtype=2)) == [E_BADARG] * 2
    assert both(*mk(2, 4, 40, 40, dk=48)) == [E_UNSUPPORTED] * 2
    assert both(*mk(2, 4, 40, 40, bias=(5000, 39))) == [E_BADARG] * 2
    assert both(*mk(2, 4, 40, 40, p=1.0)) == [E_BADARG] * 2
    assert both(*mk(60000, 60000, 40, 40, p=0.1)) == [E_UNSUPPORTED] * 2         # dropout block index past 32 bits
    f, b = mk(2, 4, 40, 40)
    f.q_stride_t += 4
    b.k_stride_t += 4
    assert both(f, b) == [E_ALIGN] * 2                                           # token strides: multiples of 16 bytes
    f, b = mk(2, 4, 40, 40)
    f.k += 8
    b.k += 8
    assert both(f) == [E_ALIGN] and bwd_plan(L, b)[0] == OK                      # (only the forward checks the operand pointers)
    f, _ = mk(2, 4, 40, 40)
    f.out += 4
    assert both(f) == [E_ALIGN]
    assert both(mk(2, 4, 40, 40, capture=True, layout="ragged")[0]) == [E_BADARG]
    assert both(*mk(2, 4, 40, 40, mask=True, layout="k_only")) == [E_BADARG] * 2
    _, b = mk(2, 4, 40, 40)
    b.dk_out = None
    assert both(b=b) == [E_BADARG]
    _, b = mk(2, 4, 40, 40, bias=None)
    b.drel = PDREL
    assert both(b=b) == [E_BADARG]                                               # a bias gradient without a bias


# ---- the knobs that are read once per process: each test tells from the environment which side it is on, the last one runs the other
# ---- side of each in a child process -----------------------------------------------------------------------------------------------------
def test_knob_fast(L):
    kf, kb = kernels(L, 2, 4, 200, 200, layout="ragged")
    if env_is_zero("LAKO_ATTN_FAST"):
        assert (kf, kb) == (ATTN_FWD, GENERIC_BWD)
    else:
        assert kf >= ATTN_ENC_FWD and kb == [ATTN_ENC_BWD_FUSED]


@needs_fast
def test_knob_fwd_dma(L):
    want = ATTN_ENC_FWD if env_is_zero("LAKO_ATTN_FWD_DMA") else ATTN_ENC_FWD_C
    assert fwd_plan(L, mk(2, 4, 200, 200)[0])[1].kernels == [want] and fwd_plan(L, mk(2, 4, 37, 37, p=0.1)[0])[1].kernels == [want]


@needs_fast
def test_knob_dkv_dma(L, monkeypatch):
    if L.lako_deterministic():
        return                  # the two-pass kernels of the fast path are not taken in that mode (test_knob_deterministic)
    monkeypatch.setenv("LAKO_ATTN_PERSIST", "0")
    pl = bwd_plan(L, mk(2, 4, 200, 200)[1])[1]
    assert pl.kernels == [ATTN_ENC_BWD_DQ, ATTN_ENC_BWD_DKV] and pl.launch[1].dma_stage == (0 if env_is_zero("LAKO_ATTN_DKV_DMA") else 1)


@needs_fast
def test_knob_deterministic(L, monkeypatch):
    det = os.environ.get("LAKO_DETERMINISTIC", "")[:1] == "1"
    assert bool(L.lako_deterministic()) == det
    bk = lambda *a, **kw: bwd_plan(L, mk(*a, **kw)[1])      # noqa: E731
    big = (2, 12, 700, 700)                  # H·R = 12 x 1399 > 16 384 slots
    assert 12 * 1399 > DET_SLOTS
    for persist in ("18", "0", "15"):
        monkeypatch.setenv("LAKO_ATTN_PERSIST", persist)
        if det:
            assert bk(2, 12, 200, 200)[1].kernels == [ATTN_ENC_BWD_FUSED]            # wherever it applies, whatever the mask says
            assert bk(2, 2, 225, 225)[1].kernels == GENERIC_BWD                      # never the fast path's two-pass kernels
            rc, _ = bk(*big)
            assert rc == E_UNSUPPORTED and L.lako_attn_bwd(C.byref(mk(*big)[1]), None) == E_UNSUPPORTED
            assert bk(*big, drel=False)[0] == OK
        else:
            assert bk(2, 2, 225, 225)[1].kernels[1] in (ATTN_ENC_BWD_DKV, ATTN_ENC_BWD_DKV_P)
            assert bk(*big)[0] == OK and bk(*big)[1].kernels == GENERIC_BWD


def test_once_per_process_knobs_in_child_processes():
    """LAKO_ATTN_FAST, LAKO_ATTN_FWD_DMA, LAKO_ATTN_DKV_DMA and LAKO_DETERMINISTIC are read once per process: the knob tests above, once
    more in one child process per knob with the setting this process does not have"""
    det = os.environ.get("LAKO_DETERMINISTIC", "")[:1] == "1"
    for name, value, want in (("LAKO_ATTN_FAST", "1" if env_is_zero("LAKO_ATTN_FAST") else "0", "test_knob_fast"),
                              ("LAKO_ATTN_FWD_DMA", "1" if env_is_zero("LAKO_ATTN_FWD_DMA") else "0", "test_knob_fwd_dma"),
                              ("LAKO_ATTN_DKV_DMA", "1" if env_is_zero("LAKO_ATTN_DKV_DMA") else "0", "test_knob_dkv_dma"),
                              ("LAKO_DETERMINISTIC", "0" if det else "1", "test_knob_deterministic")):
        env = dict(os.environ, **{name: value})
        if name != "LAKO_ATTN_FAST":
            env["LAKO_ATTN_FAST"] = "1"
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-p", "no:cacheprovider", "-k", want],
                           env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0 and "1 passed" in r.stdout and "skipped" not in r.stdout, (name, value, r.stdout[-3000:] + r.stderr[-1000:])
