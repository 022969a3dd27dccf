"""The GEMM dispatch as a decision table, checked on a host without a GPU.

lako_gemm_nt_plan / lako_gemm_nt_mx_plan / lako_gemm_tn_plan / lako_gemm_tn_grouped_plan go through the validation and the decision code
of their launching entry points and launch nothing (include/lako_hip.h "plan queries"), so every gate of the dispatch can be pinned here
with pointer VALUES that are never dereferenced.  The expected kernels are what the written contract says — the comments on lako_tuning_t
and LAKO_EPI_* in include/lako_hip.h, DESIGN.md, README.md — not a reading of nt_plan: a gate that drifts (too tight: a fast kernel is
silently no longer used; too loose: a kernel takes a call whose epilogue it ignores) fails a row of this table, where the result-only
GPU tests would keep passing."""
import ctypes as C
import itertools
import os
import subprocess

import pytest
import torch

from lako_amd import _lib
from lako_amd._lib import (EPI_ATOMIC, EPI_AUXMASK, EPI_GATED, EPI_GATED_BWD, EPI_NORM_A, EPI_RELU, EPI_RESID, LAKO_BF16, LAKO_F32,
                           LAKO_FP8_E4M3, NT_128, NT_EIGHT, NT_EIGHT_256x128, NT_FOUR, NT_FOUR_BY_128, NT_FOUR_GATED, NT_MX_EIGHT,
                           NT_MX_FOUR, NT_REFUSED, NT_RING, NT_SKINNY, NT_SKINNY_NORM, GemmNT, GemmPlan, GemmTNItem, GemmTNPlan, Tuning)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_BADARG, E_ALIGN, E_UNSUPPORTED = 0, -1, -2, -4

# never dereferenced: far apart, 4 KiB aligned
PA, PB, PC, PR, PX, PW, PS = (0x100000000000 + i * 0x010000000000 for i in range(7))
ME = 47757          # rows of the encoder GEMMs of BASELINE config 2 (README.md)


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["bash", os.path.join(ROOT, "lako_amd", "csrc", "build.sh")], check=True)
    _lib._lib = None
    return _lib.load()


@pytest.fixture(autouse=True)
def _no_env_tuning(monkeypatch):
    monkeypatch.delenv("LAKO_TUNING", raising=False)


def tuning(L, **knobs):
    t = Tuning()
    assert L.lako_tuning_init(C.byref(t)) == 0
    for k, v in knobs.items():
        assert L.lako_tuning_set(C.byref(t), ("gemm_" + k).encode(), v) == 0, k
    return t


def nt(M, N, K, *, tu, dt_in=LAKO_BF16, dt_out=LAKO_BF16, alpha=1.0, flags=0, p=0.0, lda=None, ldb=None, ldc=None, ldr=None, ldaux=None,
       c_off=0, r_off=0, x_off=0, norm=False, aux=None):
    """a lako_gemm_nt_t over fake operands; *_off in BYTES from a 4 KiB aligned address"""
    g = GemmNT()
    g.A, g.B, g.C = PA, PB, PC + c_off
    g.M, g.N, g.K = M, N, K
    g.lda, g.ldb, g.ldc = lda or K, ldb or K, ldc or N
    g.in_dtype, g.out_dtype, g.alpha, g.flags = dt_in, dt_out, alpha, flags
    if flags & EPI_RESID:
        g.resid, g.ldr = PR + r_off, ldr or N
    if flags & (EPI_AUXMASK | EPI_GATED | EPI_GATED_BWD):
        g.aux, g.ldaux = (PX + x_off) if aux is None else aux, ldaux or N
    g.aux_scale = 1.0
    g.drop = _lib.Dropout(p, 5, 6)
    g.tuning = C.addressof(tu)
    if norm:
        g.flags |= EPI_NORM_A
        g.norm_w, g.norm_eps, g.norm_out, g.norm_ld, g.norm_rstd = PW, 1e-6, PS, K, PS + (1 << 30)
    g._keep = tu
    return g


def plan(L, g):
    out = GemmPlan()
    rc = L.lako_gemm_nt_plan(C.byref(g), C.byref(out))
    if rc != OK:
        assert out.kernel == NT_REFUSED and out.tile_rows == 0, "a refused query leaves a zeroed plan"
    return rc, out


def cdiv(a, b):
    return -(-a // b)


# the four epilogues the training step uses (tests/test_kernels_gpu.py runs every NT test over them)
EPIS = {"plain": dict(), "relu+drop": dict(flags=EPI_RELU, p=0.1), "resid+drop": dict(flags=EPI_RESID, p=0.1), "aux": dict(flags=EPI_AUXMASK)}
# (name, N, K, epilogue): README.md "all five encoder shapes" (profiles/r06z_gemm_vs_vendor_47757.txt) with the epilogues the step gives them
ENCODER = [("qkv", 2304, 768, "plain"), ("o+res", 768, 768, "resid+drop"), ("wi", 3072, 768, "relu+drop"), ("wo", 768, 3072, "resid+drop"),
           ("dx_qkv", 768, 2304, "plain")]


def four_wave_rows(M, N, K):
    """include/lako_hip.h nt_four: "256- or 192-row tiles, whichever needs less time for the launch's rounds of the chip"; the price is the
    one DESIGN.md / the tile-height note state: rounds of 256 tiles, a tile costs 4.5 µs + (K / 64) · (1.32 | 0.99) µs"""
    cost = lambda bm, step: cdiv(cdiv(M, bm) * cdiv(N, 256), 256) * (4.5 + step * (K // 64))     # noqa: E731
    return 192 if cost(192, 0.99) < cost(256, 1.32) else 256


# ------------------------------------------------------------------------------------------------------------------------------------
def test_encoder_shapes_run_on_the_four_wave_kernel(L):
    """README.md / DESIGN.md: the encoder's products run on gemm_nt4_kernel.  Tile height: 47 757 x 768 outputs are 561 tiles of 256 rows
    = 3 rounds against 747 of 192 rows = 3 shorter ones -> 192-row tiles."""
    assert cdiv(ME, 256) * 3 == 561 and cdiv(ME, 192) * 3 == 747
    tu = tuning(L)
    for name, N, K, epi in ENCODER:
        rc, pl = plan(L, nt(ME, N, K, tu=tu, **EPIS[epi]))
        assert rc == OK and pl.kernel == NT_FOUR and pl.head_rows == 0, (name, pl)
        assert pl.tile_rows == four_wave_rows(ME, N, K), (name, pl)
        if N == 768:
            assert pl.tile_rows == 192, (name, pl)
        assert (pl.side_lds, pl.wide_epi, pl.queue, pl.eight_phase, pl.skinny_steps) == (0, 0, 0, 0, 0), (name, pl)


def test_encoder_shapes_without_the_four_wave_kernel(L):
    """gemm_nt_four = 0, "the eight-wave kernels of rounds 1-5": 288-row tiles where they save a round or the tail launch — at N = 768 that is
    498 tiles in two rounds of the chip and no tail launch."""
    assert cdiv(ME, 288) * 3 == 498 <= 2 * 256
    tu = tuning(L, nt_four=0)
    for name, N, K, epi in ENCODER:
        rc, pl = plan(L, nt(ME, N, K, tu=tu, **EPIS[epi]))
        assert rc == OK and pl.kernel == NT_EIGHT and pl.tile_rows in (256, 288), (name, pl)
        if N == 768:
            assert (pl.tile_rows, pl.head_rows) == (288, 0), (name, pl)
        # an epilogue with one side operand stages it through LDS, a plain one leaves through the wide epilogue (lako_tuning_t)
        side = epi in ("resid+drop", "aux")
        assert (pl.side_lds, pl.wide_epi) == ((1, 0) if side else (0, 1)), (name, pl)


def test_encoder_shapes_tail_split(L):
    """gemm_nt_four = 0, gemm_nt_tile288 = 0: the rows of the full rounds of 256² tiles on the eight-wave 256² kernel, the rest on a second
    launch with 128² tiles — when the last round would be less than half full (nt_tail_split); at most one 128² tile per CU -> the ring."""
    tu = tuning(L, nt_four=0, nt_tile288=0)
    seen_tail = 0
    for name, N, K, epi in ENCODER:
        rc, pl = plan(L, nt(ME, N, K, tu=tu, **EPIS[epi]))
        tn, tiles = cdiv(N, 256), cdiv(ME, 256) * cdiv(N, 256)
        full_rows = (tiles // 256) * 256 // tn          # tile-rows covered by the full rounds
        rest = tiles - full_rows * tn
        assert rc == OK, name
        if rest < 128:
            seen_tail += 1
            assert pl.head_tile == 256 and pl.head_rows == full_rows * 256 and pl.head_rows % 256 == 0 and 0 < pl.head_rows < ME, (name, pl)
            tail_tiles = cdiv(ME - pl.head_rows, 128) * cdiv(N, 128)
            assert pl.kernel == (NT_RING if tail_tiles <= 256 else NT_128), (name, pl, tail_tiles)
            side = epi in ("resid+drop", "aux")
            assert (pl.head_side_lds, pl.head_wide_epi) == ((1, 0) if side else (0, 1)), (name, pl)
        else:
            assert (pl.kernel, pl.tile_rows, pl.head_rows) == (NT_EIGHT, 256, 0), (name, pl)
    assert seen_tail >= 3       # the three N = 768 products: 561 tiles = 2 rounds + 51


def test_encoder_shapes_with_the_ticket_queue(L):
    """gemm_nt_queue = 1: "the persistent 256x256 kernel pulls its tiles from per-XCD ticket counters" — the 256-row eight-wave kernel, QUEUE
    instantiation, for the big launch of every encoder product (the four-wave and the 288-row kernels have a static tile order)."""
    tu = tuning(L, nt_queue=1)
    for name, N, K, epi in ENCODER:
        rc, pl = plan(L, nt(ME, N, K, tu=tu, **EPIS[epi]))
        assert rc == OK, name
        if pl.head_rows:
            assert (pl.head_tile, pl.head_queue, pl.head_eight_phase) == (256, 1, 0) and pl.kernel in (NT_RING, NT_128) and pl.queue == 0, (name, pl)
        else:
            assert (pl.kernel, pl.tile_rows, pl.queue) == (NT_EIGHT, 256, 1), (name, pl)


def test_decoder_shapes(L):
    """lako_tuning_t.nt_skinny: M <= 256 on the split-K kernel (32² tiles by default); the LM head (N = 32 128, fp32 logits) is not a
    skinny problem: 251 tiles of 128², at most one per CU -> the ring.  K-step buckets: a wave unrolls ceil(K / 32 / 8) steps in 4 | 8 | 16."""
    tu = tuning(L)
    for (M, N, K), epi in itertools.product([(128, 2304, 768), (128, 768, 768), (128, 3072, 768), (128, 768, 3072), (16, 768, 768), (256, 4096, 1024)], EPIS):
        rc, pl = plan(L, nt(M, N, K, tu=tu, **EPIS[epi]))
        assert rc == OK and (pl.kernel, pl.tile_rows, pl.head_rows) == (NT_SKINNY, 32, 0), (M, N, K, epi, pl)
        per = cdiv(K // 32, 8)
        assert pl.skinny_steps == (4 if per <= 4 else 8 if per <= 8 else 16), (K, pl)
    for K, steps in ((128, 4), (1024, 4), (1056, 8), (2048, 8), (2080, 16), (4096, 16)):
        assert plan(L, nt(128, 768, K, tu=tu))[1].skinny_steps == steps, K
    for sk, side in ((2, 64), (3, 32), (4, 16)):
        assert plan(L, nt(128, 768, 768, tu=tuning(L, nt_skinny=sk)))[1].tile_rows == side
    rc, pl = plan(L, nt(128, 32128, 768, tu=tu, dt_out=LAKO_F32))
    assert rc == OK and pl.kernel == NT_RING, pl
    rc, pl = plan(L, nt(128, 32128, 768, tu=tu, dt_out=LAKO_F32, flags=EPI_ATOMIC))
    assert rc == OK and pl.kernel == NT_RING, pl


NORM_REFUSED_TUNINGS = [dict(nt_queue=1), dict(nt_tile288=0), dict()]      # tests/test_kernels_gpu.py::test_gemm_nt_norm_refused_before_any_launch


def test_fused_norm_taken_and_refused(L):
    """LAKO_EPI_NORM_A: "Only where the M <= 256 kernel runs (bf16, K % 32 == 0, K <= 1024): LAKO_E_UNSUPPORTED otherwise, nothing launched" """
    tu = tuning(L)
    for M, N, K in ((128, 2304, 768), (256, 768, 1024), (16, 768, 128), (37, 776, 512)):
        rc, pl = plan(L, nt(M, N, K, tu=tu, norm=True))
        assert rc == OK and (pl.kernel, pl.tile_rows, pl.skinny_steps) == (NT_SKINNY_NORM, 32, 4), (M, N, K, pl)
    for M, N, K in ((128, 768, 2048), (128, 768, 1056), (257, 768, 768), (300, 768, 768), (128, 4104, 768), (128, 768, 1000)):
        assert plan(L, nt(M, N, K, tu=tu, norm=True))[0] == E_UNSUPPORTED, (M, N, K)
    assert plan(L, nt(128, 768, 768, tu=tu, norm=True, dt_in=LAKO_F32, dt_out=LAKO_F32))[0] == E_UNSUPPORTED
    assert plan(L, nt(128, 768, 768, tu=tuning(L, nt_skinny=0), norm=True))[0] == E_UNSUPPORTED
    for knobs in NORM_REFUSED_TUNINGS:
        for variant in (-1, 0, 2, 4, 8, 9):
            assert plan(L, nt(5600, 3072, 768, tu=tuning(L, nt_variant=variant, **knobs), norm=True))[0] == E_UNSUPPORTED, (knobs, variant)


# ---- one row per term of every predicate: a call that differs from a taken call in that term only ---------------------------------------
BIG = dict(M=16500, N=1032, K=384)         # 65 x 5 = 325 tiles of 256²: more than a round of the chip
HUGE = 1 << 23                             # a row stride whose 128- / 256-row offsets no longer fit 32 bits (elements of 2 bytes)


def four(L, tu, **kw):
    a = dict(BIG)
    a.update(kw)
    return plan(L, nt(a.pop("M"), a.pop("N"), a.pop("K"), tu=tu, **a))


FOUR_TAKEN = {  # every epilogue the header's nt_four comment lists
    "plain": dict(), "alpha alone": dict(alpha=0.5), "relu": dict(flags=EPI_RELU), "dropout": dict(p=0.1), "relu+dropout": dict(flags=EPI_RELU, p=0.1),
    "resid": dict(flags=EPI_RESID), "resid+dropout": dict(flags=EPI_RESID, p=0.1), "aux": dict(flags=EPI_AUXMASK),
    "ldc wide": dict(ldc=1040), "ldr wide": dict(flags=EPI_RESID, ldr=1040), "ldaux wide": dict(flags=EPI_AUXMASK, ldaux=1040),
    "K = 256": dict(K=256), "lda wide": dict(lda=392, ldb=400),
}
FOUR_DECLINED = {  # one term off each
    "fp32 in": dict(dt_in=LAKO_F32), "fp32 out": dict(dt_out=LAKO_F32), "K % 128": dict(K=320), "K % 128 (448)": dict(K=448), "K < 256": dict(K=128),
    "atomic": dict(dt_out=LAKO_F32, flags=EPI_ATOMIC),
    "N % 8": dict(N=1028), "ldc % 8": dict(ldc=1036), "C 8-byte aligned": dict(c_off=8), "lda beyond 32-bit offsets": dict(lda=HUGE), "ldb beyond 32-bit offsets": dict(ldb=HUGE),
    "alpha with relu": dict(alpha=0.5, flags=EPI_RELU), "alpha with dropout": dict(alpha=0.5, p=0.1), "alpha with resid": dict(alpha=0.5, flags=EPI_RESID),
    "alpha with aux": dict(alpha=0.5, flags=EPI_AUXMASK),
    "resid + aux": dict(flags=EPI_RESID | EPI_AUXMASK), "relu + resid": dict(flags=EPI_RELU | EPI_RESID), "relu + aux": dict(flags=EPI_RELU | EPI_AUXMASK),
    "aux + dropout": dict(flags=EPI_AUXMASK, p=0.1),
    "ldr % 8": dict(flags=EPI_RESID, ldr=1036), "resid + 2 bytes": dict(flags=EPI_RESID, r_off=2), "resid + 8 bytes": dict(flags=EPI_RESID, r_off=8),
    "ldr beyond 32-bit offsets": dict(flags=EPI_RESID, ldr=HUGE),
    "ldaux % 8": dict(flags=EPI_AUXMASK, ldaux=1036), "aux + 2 bytes": dict(flags=EPI_AUXMASK, x_off=2), "aux + 8 bytes": dict(flags=EPI_AUXMASK, x_off=8),
    "ldaux beyond 32-bit offsets": dict(flags=EPI_AUXMASK, ldaux=HUGE), "ldc beyond 32-bit offsets": dict(ldc=HUGE),
}


@pytest.mark.parametrize("variant,rows", [(9, 256), (3, 192)])
def test_four_wave_gate_forced(L, variant, rows):
    """nt_variant 9 / 3 force the 256- / 192-row four-wave kernel; "shapes and epilogues they do not take run on variant 2": the eight-wave
    256² kernel — named, not merely "something else" """
    tu = tuning(L, nt_variant=variant)
    for name, kw in FOUR_TAKEN.items():
        rc, pl = four(L, tu, **kw)
        assert rc == OK and (pl.kernel, pl.tile_rows, pl.head_rows) == (NT_FOUR, rows, 0), (name, pl)
    for name, kw in FOUR_DECLINED.items():
        rc, pl = four(L, tu, **kw)
        assert rc == OK and (pl.kernel, pl.tile_rows, pl.head_rows) == (NT_EIGHT, 256, 0), (name, pl)
    for knobs in (dict(nt_four=0), dict(nt_queue=1)):       # forcing the variant is what counts, as the header says
        rc, pl = four(L, tuning(L, nt_variant=variant, **knobs))
        assert (pl.kernel, pl.tile_rows) == (NT_FOUR, rows), (knobs, pl)


def test_four_wave_gate_default_plan(L):
    """the same terms where the choice is the library's: a taken call is four-wave at the height the rounds of the chip favour, a declined one
    runs "as with gemm_nt_four = 0" — the plan must equal that tuning's plan field for field"""
    tu, tu0 = tuning(L), tuning(L, nt_four=0)
    for name, kw in FOUR_TAKEN.items():
        rc, pl = four(L, tu, **kw)
        a = dict(BIG, **{k: v for k, v in kw.items() if k in ("M", "N", "K")})
        assert rc == OK and (pl.kernel, pl.tile_rows, pl.head_rows) == (NT_FOUR, four_wave_rows(a["M"], a["N"], a["K"]), 0), (name, pl)
    for name, kw in FOUR_DECLINED.items():
        (rc, pl), (rc0, pl0) = four(L, tu, **kw), four(L, tu0, **kw)
        assert rc == rc0 == OK and pl.kernel != NT_FOUR and bytes(pl) == bytes(pl0), (name, pl, pl0)
        if kw.get("dt_in") != LAKO_F32:      # bf16 operands and more than a round of 256² tiles: the eight-wave 256-column kernel does the bulk
            # (with a tail split the head IS the eight-wave kernel; the tail's few rows run on small tiles, pinned in test_tail_split_threshold)
            bulk = (NT_EIGHT, pl.head_tile) if pl.head_rows else (pl.kernel, pl.tile_rows)
            assert bulk[0] == NT_EIGHT and bulk[1] in (256, 288), (name, pl)
    assert four(L, tuning(L, nt_queue=1))[1].kernel != NT_FOUR


def test_four_wave_dropout_index_bound(L):
    """the four-wave kernels index dropout quads in 32 bits: (row0 + M + 256) · N must stay below 2^34 — a matrix nobody can allocate in a
    test (2^24 rows x 1024 columns of bf16 = 32 GiB), so the bound is only reachable here.  Without dropout the same call is taken."""
    tu = tuning(L, nt_variant=9)
    N, K = 1024, 256
    edge = (1 << 34) // N - 256                   # first M that no longer fits
    for M, p, want in ((edge - 1, 0.1, NT_FOUR), (edge, 0.1, NT_EIGHT), (edge, 0.0, NT_FOUR), (edge + 4096, 0.1, NT_EIGHT)):
        for flags in (0, EPI_RELU, EPI_RESID):
            if p == 0.0 and flags == 0 or p > 0:
                rc, pl = plan(L, nt(M, N, K, tu=tu, p=p, flags=flags))
                assert rc == OK and (pl.kernel, pl.tile_rows) == (want, 256), (M, p, flags, pl)


def test_chip_filling_boundary(L):
    """nt_four: "problems of at least one round of 256x256 tiles" — 255 tiles is not one, 256 and 257 are"""
    tu = tuning(L)
    for tiles_m, tn, want in ((255, 1, False), (256, 1, True), (257, 1, True), (51, 5, False), (52, 5, True), (127, 2, False), (128, 2, True)):
        for M in (tiles_m * 256, tiles_m * 256 - 255):
            rc, pl = plan(L, nt(M, 256 * tn, 384, tu=tu))
            assert rc == OK and (pl.kernel == NT_FOUR) == want, (tiles_m, tn, M, pl)
            if not want:      # "big tiles once there is enough work to fill the chip with them (>= 1 tile per CU), else 128x128"
                assert pl.kernel == NT_128 and pl.head_rows == 0, (tiles_m, tn, pl)


def test_tail_split_threshold(L):
    """nt_tail_split: "rows beyond the full rounds of 256x256 tiles go to a second launch with small tiles", "only when the last round would be
    less than half full": a last round of 127 tiles splits, one of 128 does not (eight-wave kernels, 288-row tiles off)"""
    tu = tuning(L, nt_four=0, nt_tile288=0)
    for last, split in ((127, True), (128, False), (1, True), (255, False)):
        M = (256 + last) * 256
        rc, pl = plan(L, nt(M, 256, 384, tu=tu))
        assert rc == OK and (pl.head_rows > 0) == split, (last, pl)
        if split:
            # (the tail is a problem of its own: a few 128² tiles, or the M <= 256 kernel when it is that short)
            assert (pl.head_rows, pl.head_tile) == (256 * 256, 256) and pl.kernel == (NT_SKINNY if last == 1 else NT_RING if last * 2 * 2 <= 256 else NT_128), (last, pl)
        else:
            assert (pl.kernel, pl.tile_rows) == (NT_EIGHT, 256), (last, pl)
    rc, pl = plan(L, nt((256 + 127) * 256, 256, 384, tu=tuning(L, nt_four=0, nt_tile288=0, nt_tail_split=0)))
    assert (pl.kernel, pl.tile_rows, pl.head_rows) == (NT_EIGHT, 256, 0), pl
    # the atomic epilogue accumulates: it is never split
    rc, pl = plan(L, nt((256 + 127) * 256, 256, 384, tu=tu, dt_out=LAKO_F32, flags=EPI_ATOMIC))
    assert rc == OK and pl.head_rows == 0, pl


def test_tile288_gate(L):
    """variant 8 = 288 x 256 / 8 waves, bf16 in and out, static tile order; everything else on 256-row tiles"""
    for kw, rows in ((dict(), 288), (dict(flags=EPI_RESID, p=0.1), 288), (dict(flags=EPI_AUXMASK), 288), (dict(flags=EPI_RELU, p=0.1), 288),
                     (dict(dt_in=LAKO_F32), 256), (dict(dt_out=LAKO_F32), 256), (dict(dt_out=LAKO_F32, flags=EPI_ATOMIC), 256)):
        rc, pl = four(L, tuning(L, nt_variant=8), **kw)
        assert rc == OK and (pl.kernel, pl.tile_rows) == (NT_EIGHT, rows), (kw, pl)
    rc, pl = four(L, tuning(L, nt_variant=8, nt_queue=1))
    assert (pl.kernel, pl.tile_rows) == (NT_EIGHT, 256), pl


SKINNY = dict(M=128, N=768, K=768)
SKINNY_TAKEN = {"plain": dict(), "K = 128": dict(K=128), "K = 4096": dict(K=4096), "K % 32 == 0": dict(K=160), "fp32 out": dict(dt_out=LAKO_F32),
                "resid": dict(flags=EPI_RESID, p=0.1, alpha=0.5), "aux": dict(flags=EPI_AUXMASK), "relu+resid": dict(flags=EPI_RELU | EPI_RESID),
                "wide rows": dict(lda=776, ldb=784, ldc=776)}
SKINNY_DECLINED = {"K % 32": dict(K=776), "K % 32 (72)": dict(K=72), "K < 128": dict(K=96), "K > 4096": dict(K=4128), "N % 8": dict(N=772), "ldc % 8": dict(ldc=772),
                   "C 8-byte aligned": dict(c_off=8), "A beyond 32-bit offsets": dict(lda=1 << 24), "B beyond 32-bit offsets": dict(ldb=1 << 22, N=776),
                   "atomic": dict(dt_out=LAKO_F32, flags=EPI_ATOMIC), "ldr % 8": dict(flags=EPI_RESID, ldr=772), "resid + 2 bytes": dict(flags=EPI_RESID, r_off=2),
                   "resid + 8 bytes": dict(flags=EPI_RESID, r_off=8), "ldaux % 8": dict(flags=EPI_AUXMASK, ldaux=772), "aux + 2 bytes": dict(flags=EPI_AUXMASK, x_off=2),
                   "aux + 8 bytes": dict(flags=EPI_AUXMASK, x_off=8), "fp32 in": dict(dt_in=LAKO_F32, dt_out=LAKO_F32)}


def skinny(L, tu, **kw):
    a = dict(SKINNY)
    a.update(kw)
    return plan(L, nt(a.pop("M"), a.pop("N"), a.pop("K"), tu=tu, **a))


@pytest.mark.parametrize("variant", [5, -1])
def test_skinny_gate(L, variant):
    """variant 5 / M <= 256: the split-K kernel; "it falls back to the ring when K is not a multiple of 32" — and for every other term"""
    tu = tuning(L, nt_variant=variant)
    for name, kw in SKINNY_TAKEN.items():
        rc, pl = skinny(L, tu, **kw)
        assert rc == OK and (pl.kernel, pl.tile_rows) == (NT_SKINNY, 32), (name, pl)
    for name, kw in SKINNY_DECLINED.items():
        rc, pl = skinny(L, tu, **kw)
        assert rc == OK and pl.kernel == NT_RING and pl.skinny_steps == 0, (name, pl)


def test_skinny_wanted_boundaries(L):
    """the library's own choice: M <= 256 rows and N <= 4096 columns (the decoder), tuning nt_skinny on"""
    tu = tuning(L)
    for M, N, want in ((256, 768, True), (257, 768, False), (128, 4096, True), (128, 4104, False), (1, 8, True)):
        rc, pl = plan(L, nt(M, N, 768, tu=tu))
        assert rc == OK and (pl.kernel == NT_SKINNY) == want, (M, N, pl)
        if not want:
            assert pl.kernel == NT_RING, (M, N, pl)      # few tiles: the ring
    assert plan(L, nt(128, 768, 768, tu=tuning(L, nt_skinny=0)))[1].kernel == NT_RING
    assert plan(L, nt(128, 768, 768, tu=tuning(L, nt_skinny=0, nt_ring=0)))[1].kernel == NT_128
    assert plan(L, nt(300, 768, 768, tu=tuning(L, nt_variant=5)))[1].kernel == NT_SKINNY      # forced: whatever the shape


def test_side_operand_and_wide_epilogue_gates(L):
    """lako_tuning_t.nt_side_lds: "residual / aux operand of a 256x256 tile staged through LDS" — exactly one side operand, bf16 in and out,
    16-byte granular rows everywhere, else the operand is read from global memory in the accumulator layout; nt_wide_epi: "LDS-transposed
    epilogue with 16-byte stores for plain bf16 outputs", else stores from the accumulator layout"""
    for variant in (2, 7, 8):
        tu = tuning(L, nt_variant=variant)
        for side, ld, off in ((EPI_RESID, "ldr", "r_off"), (EPI_AUXMASK, "ldaux", "x_off")):
            for kw, want in ((dict(), 1), (dict(p=0.1), 1), ({ld: 1040}, 1), (dict(ldc=1040), 1),
                             (dict(N=1028), 0), (dict(ldc=1036), 0), ({ld: 1036}, 0), (dict(c_off=8), 0), ({off: 2}, 0), ({off: 8}, 0), ({off: 16}, 1),
                             (dict(ldc=HUGE), 0), ({ld: HUGE}, 0), (dict(dt_out=LAKO_F32), 0), (dict(dt_in=LAKO_F32, dt_out=LAKO_F32), 0)):
                rc, pl = four(L, tu, flags=side, **kw)
                assert rc == OK and pl.kernel == NT_EIGHT and (pl.side_lds, pl.wide_epi) == (want, 0), (variant, side, kw, pl)
            rc, pl = four(L, tuning(L, nt_variant=variant, nt_side_lds=0), flags=side)
            assert (pl.kernel, pl.side_lds) == (NT_EIGHT, 0), pl
        assert four(L, tu, flags=EPI_RESID | EPI_AUXMASK)[1].side_lds == 0
        for kw, want in ((dict(), 1), (dict(alpha=0.5), 1), (dict(flags=EPI_RELU, p=0.1), 1), (dict(ldc=1040), 1), (dict(N=1028), 0), (dict(ldc=1036), 0),
                         (dict(c_off=8), 0), (dict(flags=EPI_RESID), 0), (dict(flags=EPI_AUXMASK), 0), (dict(dt_out=LAKO_F32), 0), (dict(dt_in=LAKO_F32), 0),
                         (dict(dt_out=LAKO_F32, flags=EPI_ATOMIC), 0)):
            rc, pl = four(L, tu, **kw)
            assert rc == OK and pl.kernel == NT_EIGHT and pl.wide_epi == want, (variant, kw, pl)
        assert four(L, tuning(L, nt_variant=variant, nt_wide_epi=0))[1].wide_epi == 0
    # kernels without these epilogues never report them
    for variant in (0, 1, 4, 6, 9):
        pl = four(L, tuning(L, nt_variant=variant), flags=EPI_RESID)[1]
        assert (pl.side_lds, pl.wide_epi) == (0, 0), (variant, pl)
        assert four(L, tuning(L, nt_variant=variant))[1].wide_epi == 0, variant


def test_queue_and_eight_phase_gates(L):
    """nt_queue: the 256-row eight-wave kernel with several K-steps per tile, several tiles per workgroup and a persistent grid — "on shapes where
    the queue does not apply (one round; K of one K-step) the launch falls back to the strided kernel"; nt_pp: "the 8-phase loop of the
    256x256 / 8-wave bf16 kernel (K >= 128)" """
    q = dict(nt_variant=2, nt_queue=1)
    for (M, N, K), knobs, kw, want in (((70000, 768, 768), {}, {}, 1), ((40000, 2304, 192), {}, {}, 1), ((70000, 768, 128), {}, {}, 1), ((5000, 768, 64), {}, {}, 0),
                                       ((70000, 768, 64), {}, {}, 0), ((1000, 768, 768), {}, {}, 0), ((65536, 256, 768), {}, {}, 0), ((65537, 256, 768), {}, {}, 1),
                                       ((70000, 768, 768), dict(nt_persistent=0), {}, 0), ((70000, 768, 768), {}, dict(flags=EPI_RESID), 1),
                                       ((70000, 768, 768), {}, dict(dt_out=LAKO_F32), 0), ((70000, 768, 768), dict(nt_variant=7), {}, 0),
                                       ((70000, 768, 768), dict(nt_variant=8), {}, 1)):      # (variant 8 under the queue runs 256-row tiles: test_tile288_gate)
        rc, pl = plan(L, nt(M, N, K, tu=tuning(L, **dict(q, **knobs)), **kw))
        assert rc == OK and pl.kernel == NT_EIGHT and (pl.queue, pl.eight_phase) == (want, 0), (M, N, K, knobs, kw, pl)
    pp = dict(nt_variant=2, nt_pp=1)
    for (M, N, K), knobs, kw, want in (((2048, 768, 768), {}, {}, 1), ((256, 256, 128), {}, {}, 1), ((515, 264, 72), {}, {}, 0), ((515, 264, 64), {}, {}, 0),
                                       ((2048, 768, 768), dict(nt_variant=7), {}, 0), ((2048, 768, 768), dict(nt_variant=8), {}, 0),
                                       ((2048, 768, 768), dict(nt_pp=0), {}, 0), ((2048, 768, 768), {}, dict(dt_out=LAKO_F32), 0),
                                       ((2048, 768, 768), {}, dict(flags=EPI_AUXMASK), 1)):
        rc, pl = plan(L, nt(M, N, K, tu=tuning(L, **dict(pp, **knobs)), **kw))
        assert rc == OK and pl.kernel == NT_EIGHT and (pl.eight_phase, pl.queue) == (want, 0), (M, N, K, knobs, kw, pl)


# variant -> (own kernel, tile rows or None, a shape + arguments that reach it), (documented fallback, rows, shape + arguments) or None
FORCED = {
    0: ((NT_128, None, (700, 520, 200, {})), None),
    1: ((NT_EIGHT_256x128, None, (700, 520, 200, {})), None),
    2: ((NT_EIGHT, 256, (700, 520, 200, {})), None),
    3: ((NT_FOUR, 192, (1024, 768, 768, {})), (NT_EIGHT, 256, (700, 520, 200, {}))),              # K % 128
    4: ((NT_RING, None, (2048, 2304, 768, {})), None),
    5: ((NT_SKINNY, 32, (128, 768, 768, {})), (NT_RING, None, (128, 768, 72, {}))),               # K % 32
    6: ((NT_FOUR_BY_128, None, (700, 520, 200, {})), (NT_128, None, (700, 520, 200, dict(dt_in=LAKO_F32)))),
    7: ((NT_EIGHT, 192, (700, 520, 200, {})), (NT_EIGHT, 256, (700, 520, 200, dict(dt_out=LAKO_F32)))),
    8: ((NT_EIGHT, 288, (700, 520, 200, {})), (NT_EIGHT, 256, (700, 520, 200, dict(dt_out=LAKO_F32)))),
    9: ((NT_FOUR, 256, (1024, 768, 768, {})), (NT_EIGHT, 256, (128, 768, 72, {}))),               # K % 128, K < 256
}


@pytest.mark.parametrize("variant", sorted(FORCED))
def test_forced_variants(L, variant):
    """lako_tuning_t.nt_variant 0-9: each id plans its own kernel on a shape it takes and the documented fallback on one it does not"""
    tu = tuning(L, nt_variant=variant)
    for case in FORCED[variant]:
        if case is None:
            continue
        kernel, rows, (M, N, K, kw) = case
        rc, pl = plan(L, nt(M, N, K, tu=tu, **kw))
        assert rc == OK and pl.kernel == kernel and pl.head_rows == 0 and (rows is None or pl.tile_rows == rows), (variant, case, pl)


GATED = dict(M=1024, K=768, f=2048)


def gated(tu, backward=False, **kw):
    a = dict(GATED, **kw)
    f, K, M = a.pop("f"), a.pop("K"), a.pop("M")
    a.setdefault("ldc", 2 * f)
    a.setdefault("ldaux", 2 * f if backward else f)
    a.setdefault("flags", EPI_GATED_BWD if backward else EPI_GATED)
    return nt(M, f if backward else 2 * f, K, tu=tu, **a)


@pytest.mark.parametrize("backward", [False, True])
def test_fused_gated_gate(L, backward):
    """LAKO_EPI_GATED / _BWD: "The only flag of the call; bf16, alpha = 1, f % 128 == 0, K % 128 == 0, K >= 256; LAKO_E_UNSUPPORTED otherwise,
    nothing launched", ldc = 2f, ldaux = f (forward) / 2f (backward), 16-byte aligned operands"""
    tu = tuning(L)
    for kw in (dict(), dict(K=256), dict(f=128), dict(p=0.1), dict(M=16), dict(lda=776, ldb=784)):
        rc, pl = plan(L, gated(tu, backward, **kw))
        assert rc == OK and (pl.kernel, pl.tile_rows, pl.head_rows) == (NT_FOUR_GATED, 256, 0), (kw, pl)
    me = EPI_GATED_BWD if backward else EPI_GATED
    for name, kw in {"f % 128": dict(f=2112), "K % 128": dict(K=832), "K < 256": dict(K=128), "alpha": dict(alpha=0.5), "with relu": dict(flags=me | EPI_RELU),
                     "with resid": dict(flags=me | EPI_RESID), "both": dict(flags=EPI_GATED | EPI_GATED_BWD), "ldc": dict(ldc=2 * 2048 + 8), "ldaux": dict(ldaux=3 * 2048),
                     "no side": dict(aux=0), "C 8-byte aligned": dict(c_off=8), "side 8-byte aligned": dict(x_off=8), "fp32": dict(dt_in=LAKO_F32, dt_out=LAKO_F32),
                     "fp32 out": dict(dt_out=LAKO_F32)}.items():
        rc, pl = plan(L, gated(tu, backward, **kw))
        assert rc == E_UNSUPPORTED, (name, rc, pl)


def test_gated_fused_ok_mirrors_the_library(L):
    """HipOps.gated_fused_ok is what the engine asks before it calls gemm_nt_gated; a disagreement with gated_nt4_ok surfaces as LAKO_E_UNSUPPORTED
    raised from inside a training step.  Over (f, K, contiguity, dtype): the mirror says yes exactly where the library takes the call."""
    from lako_amd.ops import HipOps
    tu = tuning(L)
    for f, K, pad, dt in itertools.product((128, 192, 1024, 2048, 2112, 2816), (128, 256, 320, 512, 768, 832, 1024), (0, 8), (torch.bfloat16, torch.float32)):
        for backward in (False, True):
            M, N = 512, (f if backward else 2 * f)
            A = torch.empty(M, K + pad, dtype=dt, device="meta")[:, :K]
            B = torch.empty(N, K, dtype=dt, device="meta")
            code = LAKO_BF16 if dt == torch.bfloat16 else LAKO_F32
            rc, pl = plan(L, gated(tu, backward, M=M, K=K, f=f, lda=A.stride(0), ldb=B.stride(0), dt_in=code, dt_out=code))
            mirror = HipOps.gated_fused_ok(A, B, f)
            if pad == 0:
                assert mirror == (rc == OK), (f, K, dt, backward, rc)
            else:       # the mirror asks for contiguous operands, the library for 16-byte rows only: it may be the stricter one, never the looser
                assert not mirror and (rc == OK) == (dt == torch.bfloat16 and f % 128 == 0 and K % 128 == 0 and K >= 256), (f, K, dt, backward, rc)


def mx(M, N, K, *, tu, **kw):
    g = nt(M, N, K, tu=tu, dt_in=LAKO_FP8_E4M3, **kw)
    return g


def mx_plan(L, g, sa=PW, sb=PS):
    out = GemmPlan()
    rc = L.lako_gemm_nt_mx_plan(C.byref(g), sa, sb, C.byref(out))
    return rc, out


def test_mx_gate(L):
    """lako_tuning_t.nt_four: "lako_gemm_nt_mx follows the same key: non-zero = the four-wave MX kernel where K % 512 == 0 and the launch fills the
    chip"; the epilogues are those of the bf16 four-wave kernel; variants 3 / 9 force the tile height"""
    tu = tuning(L)
    for (M, N, K), kw, want in (((70000, 768, 1024), {}, NT_MX_FOUR), ((70000, 768, 512), {}, NT_MX_FOUR), ((70000, 768, 768), {}, NT_MX_EIGHT),
                                ((70000, 768, 640), {}, NT_MX_EIGHT), ((65536, 256, 1024), {}, NT_MX_FOUR), ((65280, 256, 1024), {}, NT_MX_EIGHT),
                                ((70000, 768, 1024), dict(flags=EPI_RELU, p=0.1), NT_MX_FOUR), ((70000, 768, 1024), dict(flags=EPI_RESID, p=0.1), NT_MX_FOUR),
                                ((70000, 768, 1024), dict(flags=EPI_AUXMASK), NT_MX_FOUR), ((70000, 768, 1024), dict(flags=EPI_RELU | EPI_RESID), NT_MX_EIGHT),
                                ((70000, 768, 1024), dict(flags=EPI_AUXMASK, p=0.1), NT_MX_EIGHT), ((70000, 768, 1024), dict(alpha=0.5, p=0.1), NT_MX_EIGHT),
                                ((70000, 768, 1024), dict(alpha=0.5), NT_MX_FOUR), ((70000, 768, 1024), dict(flags=EPI_RESID, r_off=8), NT_MX_EIGHT),
                                ((70000, 768, 1024), dict(flags=EPI_RESID, ldr=772), NT_MX_EIGHT), ((70000, 768, 1024), dict(flags=EPI_AUXMASK, x_off=2), NT_MX_EIGHT)):
        rc, pl = mx_plan(L, mx(M, N, K, tu=tu, **kw))
        assert rc == OK and pl.kernel == want and pl.head_rows == 0, (M, N, K, kw, pl)
        if want == NT_MX_EIGHT:
            assert pl.tile_rows == 256 and pl.wide_epi == (0 if kw.get("flags", 0) & (EPI_RESID | EPI_AUXMASK) else 1), (kw, pl)
    assert mx_plan(L, mx(70000, 768, 1024, tu=tuning(L, nt_four=0)))[1].kernel == NT_MX_EIGHT
    assert mx_plan(L, mx(70000, 768, 1024, tu=tuning(L, nt_queue=1)))[1].kernel == NT_MX_FOUR       # "nt_queue is not consulted"
    for variant, rows in ((9, 256), (3, 192)):
        pl = mx_plan(L, mx(70000, 768, 1024, tu=tuning(L, nt_variant=variant)))[1]
        assert (pl.kernel, pl.tile_rows) == (NT_MX_FOUR, rows), pl
    # validation agrees with the launching entry point's: N % 8, 16-byte C, K % 128, null scales
    assert mx_plan(L, mx(70000, 772, 1024, tu=tu))[0] == E_BADARG and mx_plan(L, mx(70000, 768, 1024, tu=tu, c_off=8))[0] == E_ALIGN
    assert mx_plan(L, mx(70000, 768, 1000, tu=tu))[0] == E_BADARG and mx_plan(L, mx(70000, 768, 1024, tu=tu), sa=None)[0] == E_BADARG
    assert mx_plan(L, mx(70000, 768, 1024, tu=tu, dt_out=LAKO_F32))[0] == E_BADARG


def test_mx_scale_cols_mirrors_the_header():
    """lako_mx_quantize: scales [rows, 4, KSP] bytes with KSP = ceil(K / 128) rounded up to a multiple of 4"""
    from lako_amd.ops import HipOps
    for K in (128, 256, 512, 640, 768, 1024, 3072, 4096 + 128):
        assert HipOps.mx_scale_cols(K) == 4 * (cdiv(cdiv(K, 128), 4) * 4), K


def test_engine_fp8_choice_is_accepted_by_the_library(L):
    """the engine gives a weight an fp8 shadow — and then calls gemm_nt_mx on it from inside a training step — where its K is a multiple of 128
    (Engine._fp8_blocks: the encoder's QKV and FFN-in projections and the decoder's stacked cross K/V projection; ReLU models with d_kv 64).
    Over the model sizes that qualify and the row counts of the step: lako_gemm_nt_mx takes every product the engine sends it, and refuses
    (K % 128) exactly what the engine keeps in bf16."""
    from lako_amd.config import FiDConfig
    tu = tuning(L)
    for size in ("tiny", "small", "base", "large"):
        cfg = FiDConfig.named(size)
        inner = cfg.num_heads * cfg.d_kv
        weights = {"qkv": (3 * inner, cfg.d_model, {}), "wi": (cfg.d_ff, cfg.d_model, dict(flags=EPI_RELU, p=0.1)),
                   "kv_all": (cfg.num_decoder_layers * 2 * inner, cfg.d_model, {})}
        for name, (n, k, epi) in weights.items():
            engine_fp8 = k % 128 == 0
            for M in (1, 128, 4000, ME, 16 * 20 * 200):
                rc, pl = mx_plan(L, mx(M, n, k, tu=tu, **epi))
                assert (rc == OK) == engine_fp8 and (not engine_fp8 or pl.kernel in (NT_MX_FOUR, NT_MX_EIGHT)), (size, name, M, n, k, rc, pl)
                # the four-wave MX kernel on the launches that fill the chip, where K is whole groups of four K-steps
                if engine_fp8:
                    assert (pl.kernel == NT_MX_FOUR) == (k % 512 == 0 and cdiv(M, 256) * cdiv(n, 256) >= 256), (size, name, M, pl)


def test_queries_return_the_launching_calls_codes(L):
    """the query returns what the launching call returns before its first launch: both are given the same refused struct (nothing can be
    launched from it, so calling the launching entry point is safe on a host without a GPU) and must agree, message included"""
    tu = tuning(L)
    def msg():
        buf = C.create_string_buffer(512)
        L.lako_last_error(buf, 512)
        return buf.value
    bad = {"M = 0": (nt(0, 768, 768, tu=tu), E_BADARG), "K rows not 16 bytes": (nt(128, 768, 770, tu=tu), E_BADARG), "N % 4": (nt(128, 770, 768, tu=tu), E_BADARG),
           "ldc % 4": (nt(128, 768, 768, tu=tu, ldc=770), E_BADARG), "C 4-byte aligned": (nt(128, 768, 768, tu=tu, c_off=4), E_ALIGN),
           "ldr % 4": (nt(128, 768, 768, tu=tu, flags=EPI_RESID, ldr=770), E_BADARG), "ldaux % 4": (nt(128, 768, 768, tu=tu, flags=EPI_AUXMASK, ldaux=770), E_BADARG),
           "atomic into bf16": (nt(128, 768, 768, tu=tu, flags=EPI_ATOMIC), E_BADARG), "dropout p = 1": (nt(128, 768, 768, tu=tu, p=1.0), E_BADARG),
           "bad dtype": (nt(128, 768, 768, tu=tu, dt_in=7), E_BADARG), "norm, K = 2048": (nt(128, 768, 2048, tu=tu, norm=True), E_UNSUPPORTED),
           "norm, fp32": (nt(128, 768, 768, tu=tu, norm=True, dt_in=LAKO_F32), E_UNSUPPORTED), "gated, f % 128": (gated(tu, f=2112), E_UNSUPPORTED)}
    for name, (g, want) in bad.items():
        rc, _ = plan(L, g)
        m1 = msg()
        rc2 = L.lako_gemm_nt(C.byref(g), None)
        assert rc == rc2 == want and m1 == msg() and m1, (name, rc, rc2, m1)
    assert L.lako_gemm_nt_plan(None, C.byref(GemmPlan())) == E_BADARG and L.lako_gemm_nt_plan(C.byref(nt(128, 768, 768, tu=tu)), None) == E_BADARG
    g = mx(70000, 772, 1024, tu=tu)
    assert mx_plan(L, g)[0] == L.lako_gemm_nt_mx(C.byref(g), PW, PS, None) == E_BADARG
    # accepted at the far side of the fast kernels' alignment gates (INTEGRATION.md offers these to outside callers)
    for kw in (dict(N=772), dict(ldc=772), dict(c_off=8), dict(flags=EPI_RESID, r_off=2), dict(flags=EPI_AUXMASK, x_off=6), dict(K=776), dict(flags=EPI_RESID, ldr=772)):
        assert skinny(L, tu, **kw)[0] == OK, kw


# ---- weight gradients ------------------------------------------------------------------------------------------------------------------
def tn_items(shapes, K, ld_pad=0):
    arr = (GemmTNItem * len(shapes))()
    for i, (it, (M, N)) in enumerate(zip(arr, shapes)):
        it.a, it.b, it.c = PA + i * (1 << 34), PB + i * (1 << 34), PC + i * (1 << 34)
        it.M, it.N, it.lda, it.ldb, it.ldc, it.alpha, it.rows_out = M, N, M + ld_pad, N + ld_pad, N, 1.0, 0
    return arr


def tn_grouped(L, shapes, K, split_k=0, tu=None, ws=None, ws_bytes=0, dt=LAKO_BF16):
    arr = tn_items(shapes, K)
    out = GemmTNPlan()
    rc = L.lako_gemm_tn_grouped_plan(arr, len(shapes), K, dt, split_k, C.byref(tu) if tu is not None else None, ws, ws_bytes, C.byref(out))
    return rc, out, arr


T5_BASE_LAYER = [(2304, 768), (768, 768), (3072, 768), (768, 3072)]          # dW of QKV, o, wi, wo: 27 + 9 + 36 + 36 tiles of 256²
T5_LARGE_LAYER = [(3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096)]    # 48 + 16 + 64 + 64


def test_tn_grouped_plan(L):
    """lako_gemm_tn_grouped: "108 tiles (a T5-base layer's four weight gradients) -> 2 splits; 192 tiles (T5-large) -> 4 splits"; split_k 1 = one
    contributor, -1 = plain read-modify-write, -2 = overwrite; with a workspace the K-splits meet in slabs, without it by float atomics; the
    four-wave kernel (tuning tn_four) takes "K ranges of at least 128 rows, no slab reduction"; -3 = hybrid: "1 296 tiles = five rounds of
    full-K tiles + 16 tiles x 16 pieces"; shapes the 256² kernel does not take (fp32, M or N < 256) run one lako_gemm_tn per item.
    LAKO_DETERMINISTIC=1 (read once per process; test_tn_plans_in_the_other_mode runs this table under the other setting): "every float
    accumulation shared between workgroups is order-independent (one-contributor splits)" — no hybrid schedule, the library's K-splits only
    through the workspace slabs (summed in split order), one contributor per element without a workspace."""
    det = bool(L.lako_deterministic())
    tu = tuning(L)
    L.lako_gemm_tn_grouped_workspace.restype = C.c_int64
    for shapes, tiles, splits in ((T5_BASE_LAYER, 108, 2), (T5_LARGE_LAYER, 192, 4)):
        one = (1, cdiv(ME, 64) * 64, tiles)                   # (split_k, k_chunk, grid) of one contributor per element
        rc, pl, _ = tn_grouped(L, shapes, ME, tu=tu)
        assert rc == OK and (pl.per_item, pl.big, pl.tiles, pl.full_tiles, pl.slabs, pl.atomics, pl.out_mode, pl.four) == (0, 1, tiles, 0, 0, 1, 0, 1), pl
        if det:
            assert (pl.split_k, pl.k_chunk, pl.grid) == one, pl
        else:
            assert pl.split_k == splits and pl.k_chunk % 64 == 0 and pl.k_chunk * (splits - 1) < ME <= pl.k_chunk * splits and pl.grid == tiles * splits, pl
        # the slab path (either mode): the library's cut, the pieces summed in order through the caller's workspace; not the four-wave kernel
        need = L.lako_gemm_tn_grouped_workspace(tn_items(shapes, ME), len(shapes), ME, LAKO_BF16, 0, C.byref(tu))
        assert need == tiles * splits * 65536 * 4 + cdiv(tiles, 64) * 256
        rc, pl, _ = tn_grouped(L, shapes, ME, tu=tu, ws=PS, ws_bytes=need)
        assert rc == OK and (pl.split_k, pl.slabs, pl.atomics, pl.four, pl.grid) == (splits, 1, 0, 0, tiles * splits), pl
        for ws, nbytes in ((PS, need - 1), (PS + 8, need), (None, need)):       # too small / misaligned / absent: no slabs
            pl = tn_grouped(L, shapes, ME, tu=tu, ws=ws, ws_bytes=nbytes)[1]
            assert (pl.slabs, pl.atomics, pl.four, pl.split_k) == (0, 1, 1, 1 if det else splits), pl
        for sk, mode, atomics in ((1, 0, 1), (-1, 1, 0), (-2, 2, 0)):             # one contributor by request: the same in both modes
            rc, pl, _ = tn_grouped(L, shapes, ME, split_k=sk, tu=tu, ws=PS, ws_bytes=need)
            assert rc == OK and (pl.split_k, pl.k_chunk, pl.grid, pl.out_mode, pl.atomics, pl.slabs, pl.four) == one + (mode, atomics, 0, 1), (sk, pl)
        # a split the caller or the tuning names: kept where its pieces may meet by atomics, one contributor in the deterministic mode
        assert tn_grouped(L, shapes, ME, split_k=3, tu=tu)[1].split_k == (1 if det else 3)
        assert tn_grouped(L, shapes, ME, tu=tuning(L, tn_split=5))[1].split_k == (1 if det else 5)
        need3 = L.lako_gemm_tn_grouped_workspace(tn_items(shapes, ME), len(shapes), ME, LAKO_BF16, 3, C.byref(tu))
        pl = tn_grouped(L, shapes, ME, split_k=3, tu=tu, ws=PS, ws_bytes=need3)[1]
        assert need3 == tiles * 3 * 65536 * 4 + cdiv(tiles, 64) * 256 and (pl.split_k, pl.slabs, pl.atomics) == (3, 1, 0), pl
        assert tn_grouped(L, shapes, ME, tu=tuning(L, tn_four=0))[1].four == 0
        assert tn_grouped(L, shapes, ME, tu=tuning(L, nt_glds=0))[1].four == 0      # the four-wave kernel stages by global_load_lds only
    # hybrid: the encoder's weight gradients of all 12 layers
    rc, pl, _ = tn_grouped(L, T5_BASE_LAYER * 12, ME, split_k=-3, tu=tu)
    if det:       # "no hybrid schedule (its short units meet by float atomics)"
        assert rc == OK and (pl.tiles, pl.full_tiles, pl.split_k, pl.slabs, pl.grid) == (1296, 0, 1, 0, 1296), pl
    else:
        assert rc == OK and (pl.tiles, pl.full_tiles, pl.split_k, pl.slabs, pl.atomics, pl.four) == (1296, 1280, 16, 0, 1, 1), pl
        assert pl.grid == 1280 + 16 * 16
    # "the pieces of a hybrid launch add by atomics: it never asks for a workspace"; in the deterministic mode the call is the library's own choice
    ws = lambda sk: L.lako_gemm_tn_grouped_workspace(tn_items(T5_BASE_LAYER * 12, ME), 48, ME, LAKO_BF16, sk, C.byref(tu))     # noqa: E731
    assert ws(-3) == (ws(0) if det else 0)
    # K ranges under 128 rows: the four-wave kernel declines (one piece per tile: the same in both modes)
    for K, four in ((256, 1), (128, 1), (127, 0), (64, 0)):
        rc, pl, _ = tn_grouped(L, [(256, 256)], K, split_k=1, tu=tu)
        assert rc == OK and (pl.big, pl.four, pl.split_k) == (1, four, 1), (K, pl)
    for K, four in ((1024, 1), (1100, 1), (1030, 0)):      # four pieces of 256 / 320 / 320 rows: the last has 256 / 140 / 70
        rc, pl, _ = tn_grouped(L, [(256, 256)], K, split_k=4, tu=tu)
        assert rc == OK and pl.big == 1 and (pl.split_k, pl.four) == ((1, 1) if det else (4, four)), (K, pl)
    # one launch per item
    for shapes, dt, knobs in (([(128, 768)], LAKO_BF16, {}), ([(768, 768), (768, 248)], LAKO_BF16, {}), ([(768, 768)], LAKO_F32, {}), ([(768, 768)], LAKO_BF16, dict(tn_big=0))):
        rc, pl, _ = tn_grouped(L, shapes, 1024, tu=tuning(L, **knobs), dt=dt)
        first_big = int(dt == LAKO_BF16 and shapes[0] == (768, 768) and not knobs)      # (the fields describe item 0's own launch)
        assert rc == OK and (pl.per_item, pl.big, pl.four, pl.slabs, pl.atomics, pl.full_tiles) == (1, first_big, first_big, 0, 1, 0), pl
        if det:
            assert pl.split_k == 1, pl
    # refusals agree with the launching entry point
    for n, K, sk in ((0, 1024, 0), (49, 1024, 0), (1, 0, 0), (1, 1024, -4)):
        arr = tn_items([(256, 256)] * max(n, 1), K)
        out = GemmTNPlan()
        L.lako_gemm_tn_grouped.restype = C.c_int
        assert L.lako_gemm_tn_grouped_plan(arr, n, K, LAKO_BF16, sk, None, None, 0, C.byref(out)) == L.lako_gemm_tn_grouped(arr, n, K, LAKO_BF16, sk, None, None, 0, None) == E_BADARG
    arr = tn_items([(256, 256), (256, 256)], 1024)
    arr[1].c = arr[0].c
    assert L.lako_gemm_tn_grouped_plan(arr, 2, 1024, LAKO_BF16, -1, None, None, 0, C.byref(GemmTNPlan())) == E_BADARG      # overlapping exclusive outputs
    arr = tn_items([(768, 768), (768, 260)], 1024)                                                                          # N rows not 16 bytes
    assert L.lako_gemm_tn_grouped_plan(arr, 2, 1024, LAKO_BF16, 0, None, None, 0, C.byref(GemmTNPlan())) == E_BADARG
    assert L.lako_gemm_tn_grouped_plan(arr, 2, 1024, LAKO_BF16, 0, None, None, 0, None) == E_BADARG


def test_tn_single_plan(L):
    """lako_gemm_tn: the 256² kernel for bf16 operands with M, N >= 256 (four waves for K ranges of at least 128 rows), else the 128² kernel;
    LAKO_DETERMINISTIC=1: the library's own choice (split_k 0) is one contributor per element, a split the caller names is kept"""
    det = bool(L.lako_deterministic())
    tu = tuning(L)
    def q(M, N, K, sk=0, dt=LAKO_BF16, t=tu, c=PC):
        out = GemmTNPlan()
        rc = L.lako_gemm_tn_plan(PA, PB, c, M, N, K, M, N, N, dt, 1.0, sk, C.byref(t), C.byref(out))
        return rc, out
    for (K, M, N), big, four in (((1024, 256, 256), 1, 1), ((1000, 512, 768), 1, 1), ((47757, 768, 768), 1, 1), ((131, 264, 256), 1, 1), ((100, 256, 256), 1, 0),
                                 ((1024, 248, 256), 0, 0), ((1024, 256, 128), 0, 0)):
        rc, pl = q(M, N, K)
        assert rc == OK and (pl.per_item, pl.big, pl.four) == (0, big, four), (K, M, N, pl)
        assert pl.tiles == (cdiv(M, 256) * cdiv(N, 256) if big else cdiv(M, 128) * cdiv(N, 128)) and pl.grid == pl.tiles * pl.split_k, pl
        assert not det or pl.split_k == 1, pl
    # 9 tiles, 47 757 rows: the library's own split cuts K unless every element must have one contributor
    assert (q(768, 768, ME)[1].split_k > 1) == (not det) and (q(128, 128, ME, dt=LAKO_F32)[1].split_k > 1) == (not det)
    assert q(768, 768, 1024, dt=LAKO_F32)[1].big == 0 and q(768, 768, 1024, t=tuning(L, tn_big=0))[1].big == 0
    assert q(768, 768, 1024, t=tuning(L, tn_four=0))[1].four == 0
    for sk, mode, atomics in ((1, 0, 1), (-1, 1, 0), (-2, 2, 0)):
        pl = q(768, 768, 4096, sk)[1]
        assert (pl.split_k, pl.out_mode, pl.atomics) == (1, mode, atomics), pl
    assert q(768, 768, 4096, 3)[1].split_k == 3
    assert q(768, 768, 4096, -3)[0] == E_BADARG and q(0, 768, 4096)[0] == E_BADARG and q(768, 772, 4096)[0] == E_BADARG
    assert q(768, 768, 4096, c=PC + 2)[0] == E_ALIGN
    assert L.lako_gemm_tn_plan(PA, PB, PC, 768, 768, 4096, 768, 768, 768, LAKO_BF16, 1.0, 0, None, None) == E_BADARG


def test_tn_plans_in_the_other_mode():
    """LAKO_DETERMINISTIC is read once per process: the two tables above, run again in a child process under the setting this process does not
    have — so both the float-atomics plans and the one-contributor / slab plans of the deterministic mode are pinned whatever the environment"""
    import sys
    here = _lib.load().lako_deterministic()
    env = dict(os.environ, LAKO_DETERMINISTIC="0" if here else "1")
    env.pop("LAKO_TUNING", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-p", "no:cacheprovider", "-k", "test_tn_grouped_plan or test_tn_single_plan"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and "2 passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]


def test_every_tile_variant_is_planned_as_its_own_kernel():
    """tests/test_kernels_gpu.py::test_gemm_nt_tile_variants compares every forced variant with the reference on a list of shapes; a
    (variant, shape) pair the variant's kernel does not take runs the fallback (variant 9 at K = 200 or 72).  Every variant id must be planned
    as its OWN kernel on at least one of those shapes with each of the four epilogue classes, or its kernel is never executed by that test."""
    from tests.test_kernels_gpu import TILE_VARIANT_KERNEL, TILE_VARIANT_SHAPES, TILE_VARIANTS
    lib = _lib.load()
    classes = {"plain": [dict()], "relu+drop": [dict(flags=EPI_RELU, p=0.1)], "aux": [dict(flags=EPI_AUXMASK)],
               "resid+drop": [dict(flags=EPI_RESID, p=0.1, alpha=0.5), dict(flags=EPI_RESID, p=0.1)]}       # (as the test's loop)
    for variant in TILE_VARIANTS:
        kernel, rows = TILE_VARIANT_KERNEL[variant]
        tu = tuning(lib, nt_variant=variant)
        for name, kws in classes.items():
            own = [(M, N, K) for (M, N, K) in TILE_VARIANT_SHAPES for kw in kws
                   for rc, pl in [plan(lib, nt(M, N, K, tu=tu, **kw))] if rc == OK and pl.kernel == kernel and (rows is None or pl.tile_rows == rows)]
            assert own, f"variant {variant} never runs its own kernel with the {name} epilogue on {TILE_VARIANT_SHAPES}"
