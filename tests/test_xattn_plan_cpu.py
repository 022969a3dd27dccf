"""The cross-attention dispatch as a decision table, checked on a host without a GPU.

lako_xattn_softmax_plan / lako_headbatch_nt_plan / lako_xattn_decode_plan go through the validation and the decision code of
lako_xattn_softmax_fwd / _bwd, lako_headbatch_nt and lako_xattn_decode and launch nothing (include/lako_hip.h "plan queries"), so every gate
is pinned here with pointer VALUES that are never dereferenced.  The expected kernels are what the written contract says, one row per term
of each predicate — not a reading of the plan functions:
  softmax   include/lako_hip.h "rows of up to 8 192 keys are processed from registers"; csrc/xattn.hip "Rows of at most 1024·NV keys …
            NV 16-byte vectors per thread", NV 4 | 8; the length that counts is max_keys rounded up to the 256-column segment padding;
  head-batched NT   csrc/xattn.hip: the "contract" kernel for N = 64, K = d_model in {512, 768, 1024} with K / 128 K-steps per wave; else one
            wave per 16 × (16·NT) tile, NT = 4 for N a multiple of 64 above 64, KU K-steps loaded together with K % (32·KU) == 0
            (2 | 1 at NT 4, 8 | 1 at NT 1); key-split slabs need an fp32 A;
  decode    csrc/xattn.hip: D = 256·KS; a ring of three [32 keys × D] bf16 stages next to 16 KiB of partial score tiles if that fits
            160 KiB of LDS, else two.
tests/test_xattn_gates_gpu.py runs each of these branches against fp64 and asserts the same plans first."""
import ctypes as C
import os
import subprocess

import pytest

from lako_amd import _lib
from lako_amd._lib import (LAKO_BF16, LAKO_F32, XK_DECODE, XK_HB_CONTRACT, XK_HB_NT, XK_SOFTMAX, XK_SOFTMAX_REG, Dropout, HeadBatch,
                           XattnPlan)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_BADARG, E_ALIGN, E_UNSUPPORTED = 0, -1, -2, -4
LDS_MAX = 163840        # bytes of LDS one gfx950 workgroup can allocate

# never dereferenced: far apart, 4 KiB aligned
PS, PDP, PST, PP, PKOFF, PPOFF, PA, PB, PC, PQ, PE, PML, PPC = (0x100000000000 + i * 0x010000000000 for i in range(13))


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["bash", os.path.join(ROOT, "lako_amd", "csrc", "build.sh")], check=True)
    _lib._lib = None
    return _lib.load()


def cdiv(a, b):
    return -(-a // b)


def zeroed(pl):
    return all(getattr(pl, n) == 0 for n, _ in pl._fields_)


# ---- softmax ---------------------------------------------------------------------------------------------------------------------
def softmax(L, bwd, max_keys, *, B=3, T=5, H=4, s=PS, dp=PDP, s_ld=16384, stats=PST, p=PP, p_ld=16384, p_drop=0.0):
    pl = XattnPlan()
    rc = L.lako_xattn_softmax_plan(int(bwd), s, dp if bwd else None, s_ld, stats, p, p_ld, PKOFF, PPOFF, B, T, H, max_keys,
                                   Dropout(p_drop, 3, 4), C.byref(pl))
    return rc, pl


@pytest.mark.parametrize("bwd", [False, True], ids=["fwd", "bwd"])
@pytest.mark.parametrize("max_keys,kernel,nv", [
    (1, XK_SOFTMAX_REG, 4),
    (3841, XK_SOFTMAX_REG, 4),       # the first length whose padded segment is the 4096 columns NV 4 holds
    (4096, XK_SOFTMAX_REG, 4),
    (4097, XK_SOFTMAX_REG, 8),
    (8192, XK_SOFTMAX_REG, 8),
    (8193, XK_SOFTMAX, 0),
    (20007, XK_SOFTMAX, 0),
])
def test_softmax_kernel_by_longest_segment(L, bwd, max_keys, kernel, nv):
    rc, pl = softmax(L, bwd, max_keys)
    assert rc == OK
    assert (pl.kernel, pl.nv, pl.bwd) == (kernel, nv, int(bwd)), pl
    assert (pl.gx, pl.gy, pl.gz, pl.block, pl.lds) == (5 * 4, 3, 1, 256, 0), pl     # one workgroup per (row, sample)
    assert (pl.af32, pl.nt, pl.ku, pl.ks, pl.stages) == (0, 0, 0, 0, 0), pl
    if nv:      # 256 threads × nv vectors of 4 columns hold the longest padded segment
        assert 256 * nv * 4 >= cdiv(max_keys, 256) * 256


@pytest.mark.parametrize("bwd", [False, True], ids=["fwd", "bwd"])
def test_softmax_dropout_does_not_move_the_gate(L, bwd):
    for mk, nv in ((4096, 4), (4097, 8)):
        rc, pl = softmax(L, bwd, mk, p_drop=0.1)
        assert rc == OK and (pl.kernel, pl.nv) == (XK_SOFTMAX_REG, nv)


@pytest.mark.parametrize("bwd", [False, True], ids=["fwd", "bwd"])
def test_softmax_refusals(L, bwd):
    """the launching call's own refusals, with its codes, and a zeroed plan"""
    stream = None
    for kw, want in ((dict(s=None), E_BADARG), (dict(stats=None), E_BADARG), (dict(p=None), E_BADARG), (dict(B=0), E_BADARG),
                     (dict(T=0), E_BADARG), (dict(H=0), E_BADARG), (dict(s_ld=4098), E_BADARG), (dict(p_ld=4098), E_BADARG),
                     (dict(p_drop=1.0), E_BADARG), (dict(p_drop=-0.5), E_BADARG),
                     (dict(s=PS + 8), E_ALIGN), (dict(p=PP + 4), E_ALIGN),
                     # B·H·⌈T/4⌉·⌈max_keys/4⌉ = 2^32 dropout blocks: one more than the 32-bit block index holds — only with dropout
                     (dict(B=512, H=16, T=4, p_drop=0.1), E_UNSUPPORTED)):
        mk = 4 * (1 << 19) if kw.get("B") == 512 else 1000
        rc, pl = softmax(L, bwd, mk, **kw)
        assert rc == want and zeroed(pl), (kw, rc, pl)
        a = dict(B=3, T=5, H=4, s=PS, dp=PDP, s_ld=16384, stats=PST, p=PP, p_ld=16384, p_drop=0.0)
        a.update(kw)
        d = Dropout(a["p_drop"], 3, 4)
        if bwd:
            got = L.lako_xattn_softmax_bwd(a["s"], a["dp"], a["s_ld"], a["stats"], a["p"], a["p_ld"], PKOFF, PPOFF, a["B"], a["T"], a["H"], mk, d, stream)
        else:
            got = L.lako_xattn_softmax_fwd(a["s"], a["s_ld"], a["stats"], a["p"], a["p_ld"], PKOFF, PPOFF, a["B"], a["T"], a["H"], mk, d, stream)
        assert got == want, (kw, got)
    rc, pl = softmax(L, bwd, 0)
    assert rc == E_BADARG and zeroed(pl)
    rc, pl = softmax(L, bwd, 4 * (1 << 19), B=512, H=16, T=4)        # without dropout there is no block index
    assert rc == OK and pl.kernel == XK_SOFTMAX
    if bwd:
        pl = XattnPlan()
        assert L.lako_xattn_softmax_plan(1, PS, None, 4096, PST, PP, 4096, PKOFF, PPOFF, 3, 5, 4, 1000, Dropout(0, 0, 0), C.byref(pl)) == E_BADARG
        assert zeroed(pl)
        assert L.lako_xattn_softmax_plan(1, PS, PDP + 8, 4096, PST, PP, 4096, PKOFF, PPOFF, 3, 5, 4, 1000, Dropout(0, 0, 0), C.byref(pl)) == E_ALIGN
    else:       # the forward query ignores dp
        pl = XattnPlan()
        assert L.lako_xattn_softmax_plan(0, PS, PDP + 8, 4096, PST, PP, 4096, PKOFF, PPOFF, 3, 5, 4, 1000, Dropout(0, 0, 0), C.byref(pl)) == OK
    assert L.lako_xattn_softmax_plan(int(bwd), PS, PDP, 4096, PST, PP, 4096, PKOFF, PPOFF, 3, 5, 4, 1000, Dropout(0, 0, 0), None) == E_BADARG


# ---- head-batched NT -------------------------------------------------------------------------------------------------------------
def hb(M, N, K, *, H=4, T=5, f32=False, slabs=0, slab_stride=None, **over):
    p = HeadBatch()
    p.a, p.b, p.c = PA, PB, PC
    p.M, p.T, p.H, p.N, p.K = M, T, H, N, K
    p.a_sb, p.a_st, p.a_sh = T * H * K, H * K, K
    p.b_sh, p.ldb = N * K, K
    p.c_sb, p.c_st, p.c_sh = T * H * N, H * N, N
    p.a_dtype, p.b_dtype = (LAKO_F32 if f32 else LAKO_BF16), LAKO_BF16
    p.n_slabs, p.slab_stride = slabs, (1 << 24 if slab_stride is None else slab_stride)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def hb_plan(L, p):
    pl = XattnPlan()
    return L.lako_headbatch_nt_plan(C.byref(p), C.byref(pl)), pl


HB_ROWS = [  # (id, N, K, kernel, ks | (nt, ku))
    ("contract_t5_small", 64, 512, XK_HB_CONTRACT, 4),
    ("contract_t5_base", 64, 768, XK_HB_CONTRACT, 6),
    ("contract_t5_large", 64, 1024, XK_HB_CONTRACT, 8),
    # N = 64 at another K: not the contract kernel; one 16-column tile per wave
    ("contract_xl_2048", 64, 2048, XK_HB_NT, (1, 8)),
    ("contract_640", 64, 640, XK_HB_NT, (1, 1)),         # a multiple of 128 between the contract kernel's sizes, K % 256 != 0
    ("contract_1280", 64, 1280, XK_HB_NT, (1, 8)),
    ("contract_d128", 64, 128, XK_HB_NT, (1, 1)),
    ("contract_d256", 64, 256, XK_HB_NT, (1, 8)),
    # K = 768 but N != 64: not the contract kernel
    ("n128_k768", 128, 768, XK_HB_NT, (4, 2)),
    ("n48_k768", 48, 768, XK_HB_NT, (1, 8)),
    # "expand": N = d_model, K = 64
    ("expand_128", 128, 64, XK_HB_NT, (4, 2)),
    ("expand_768", 768, 64, XK_HB_NT, (4, 2)),
    ("expand_2048", 2048, 64, XK_HB_NT, (4, 2)),
    ("n128_k96", 128, 96, XK_HB_NT, (4, 1)),             # K % 64 != 0
    ("n128_k32", 128, 32, XK_HB_NT, (4, 1)),
    ("n96_k64", 96, 64, XK_HB_NT, (1, 1)),               # N % 64 != 0: single tiles
    ("n16_k32", 16, 32, XK_HB_NT, (1, 1)),
]


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("M", [1, 16, 17, 130])
@pytest.mark.parametrize("row", HB_ROWS, ids=[r[0] for r in HB_ROWS])
def test_headbatch_nt_kernel_by_shape(L, row, M, f32):
    _, N, K, kernel, inst = row
    H = 4
    rc, pl = hb_plan(L, hb(M, N, K, H=H, f32=f32))
    assert rc == OK and pl.kernel == kernel and pl.af32 == int(f32) and pl.block == 256 and pl.lds == 0, pl
    assert (pl.bwd, pl.nv, pl.stages) == (0, 0, 0)
    if kernel == XK_HB_CONTRACT:
        assert (pl.ks, pl.nt, pl.ku) == (inst, 0, 0) and 4 * 32 * pl.ks == K, pl       # four waves × ks K-steps of 32 cover K
        assert (pl.gx, pl.gy, pl.gz) == (cdiv(M, 16), H, 4), pl                      # one workgroup per 16 × 16 tile of the 64 columns
    else:
        assert (pl.nt, pl.ku, pl.ks) == inst + (0,), pl
        assert K % (32 * pl.ku) == 0 and N % (16 * pl.nt) == 0, pl                   # what the kernel's loops assume
        assert (pl.gx, pl.gy, pl.gz) == (cdiv(cdiv(M, 16) * (N // (16 * pl.nt)) * H, 4), 1, 1), pl      # four one-wave tiles per workgroup


def test_headbatch_nt_slabs(L):
    """key-split slabs select nothing: the same kernel for 1 … 5 slabs of an fp32 A; a bf16 A with slabs is refused"""
    for N, K in ((64, 768), (64, 2048), (64, 128)):
        base = hb_plan(L, hb(17, N, K, f32=True))[1]
        for z in (0, 1, 2, 4, 5, 64):
            rc, pl = hb_plan(L, hb(17, N, K, f32=True, slabs=z))
            assert rc == OK and bytes(pl) == bytes(base), (N, K, z, pl)
        rc, pl = hb_plan(L, hb(17, N, K, f32=False, slabs=2))
        assert rc == E_BADARG and zeroed(pl)
        assert L.lako_headbatch_nt(C.byref(hb(17, N, K, f32=False, slabs=2)), None) == E_BADARG
        assert hb_plan(L, hb(17, N, K, f32=False, slabs=1))[0] == OK
        rc, pl = hb_plan(L, hb(17, N, K, f32=True, slabs=2, slab_stride=17 * 4 * K + 2))      # slabs 8 bytes apart from 16-byte alignment
        assert rc == E_BADARG and zeroed(pl)


def test_headbatch_nt_refusals(L):
    good = dict(M=17, N=64, K=768)
    for over, want in ((dict(a=None), E_BADARG), (dict(b=None), E_BADARG), (dict(c=None), E_BADARG), (dict(M=0), E_BADARG),
                       (dict(T=0), E_BADARG), (dict(H=0), E_BADARG), (dict(K=0), E_BADARG), (dict(K=48), E_BADARG), (dict(N=0), E_BADARG),
                       (dict(N=24), E_BADARG), (dict(a_dtype=2), E_BADARG), (dict(b_dtype=LAKO_F32), E_BADARG),
                       (dict(a_sb=4), E_BADARG), (dict(a_st=4), E_BADARG), (dict(a_sh=4), E_BADARG), (dict(b_sh=4), E_BADARG),
                       (dict(ldb=772), E_BADARG), (dict(c_sb=2), E_BADARG), (dict(c_st=2), E_BADARG), (dict(c_sh=2), E_BADARG),
                       (dict(a=PA + 8), E_ALIGN), (dict(b=PB + 8), E_ALIGN), (dict(c=PC + 4), E_ALIGN)):
        p = hb(**{**good, **over})
        rc, pl = hb_plan(L, p)
        assert rc == want and zeroed(pl), (over, rc, pl)
        assert L.lako_headbatch_nt(C.byref(p), None) == want, over
    pl = XattnPlan()
    assert L.lako_headbatch_nt_plan(None, C.byref(pl)) == E_BADARG and L.lako_headbatch_nt_plan(C.byref(hb(**good)), None) == E_BADARG
    assert hb_plan(L, hb(**good, c=PC + 8))[0] == OK           # C: 8-byte alignment is enough


# ---- decode ----------------------------------------------------------------------------------------------------------------------
def decode(L, D, *, R=12, B=3, Z=7, q=PQ, e=PE, e_ld=None, q_ld=None, q_sb=None, k_off=PKOFF, ml=PML, pc=PPC):
    pl = XattnPlan()
    e_ld = D if e_ld is None else e_ld
    q_ld = D if q_ld is None else q_ld
    q_sb = 16 * q_ld if q_sb is None else q_sb
    rc = L.lako_xattn_decode_plan(q, q_sb, q_ld, e, e_ld, k_off, ml, pc, R, D, B, Z, C.byref(pl))
    return rc, pl, (q, q_sb, q_ld, e, e_ld, k_off, ml, pc, R, D, B, Z)


@pytest.mark.parametrize("D,ks,stages", [(512, 2, 3), (768, 3, 3), (1024, 4, 2)])
def test_decode_instantiation_and_ring(L, D, ks, stages):
    rc, pl, _ = decode(L, D)
    assert rc == OK and (pl.kernel, pl.ks, pl.stages) == (XK_DECODE, ks, stages), pl
    stage, red = 32 * D * 2, 8 * 32 * 16 * 4          # one stage: 32 keys × D bf16; the eight waves' partial [32 × 16] fp32 score tiles
    assert pl.lds == stages * stage + red <= 160 * 1024 <= LDS_MAX
    assert stages == 3 or 3 * stage + red > 160 * 1024      # two stages only where three do not fit
    assert (pl.gx, pl.gy, pl.gz, pl.block) == (7, 3, 1, 512), pl
    assert (pl.bwd, pl.nv, pl.af32, pl.nt, pl.ku) == (0, 0, 0, 0, 0)
    for R in (1, 16):
        for Z in (1, 64):
            rc, p2, _ = decode(L, D, R=R, Z=Z, e_ld=D + 8, q_ld=D + 64)
            assert rc == OK and (p2.kernel, p2.ks, p2.stages, p2.lds, p2.gx) == (XK_DECODE, ks, stages, pl.lds, Z)


def test_decode_refusals(L):
    for kw, want in ((dict(q=None), E_BADARG), (dict(e=None), E_BADARG), (dict(k_off=None), E_BADARG), (dict(ml=None), E_BADARG),
                     (dict(pc=None), E_BADARG), (dict(R=0), E_BADARG), (dict(R=17), E_BADARG), (dict(B=0), E_BADARG), (dict(Z=0), E_BADARG),
                     (dict(Z=65), E_BADARG), (dict(e_ld=772), E_BADARG), (dict(e_ld=760), E_BADARG), (dict(e_ld=1 << 20), E_BADARG),
                     (dict(q_ld=772), E_BADARG), (dict(q_sb=772), E_BADARG),
                     (dict(q=PQ + 8), E_ALIGN), (dict(e=PE + 8), E_ALIGN), (dict(pc=PPC + 8), E_ALIGN)):
        rc, pl, args = decode(L, 768, **kw)
        assert rc == want and zeroed(pl), (kw, rc, pl)
        assert L.lako_xattn_decode(*args, None) == want, kw
    for D in (128, 256, 640, 896, 2048):        # HipOps.xattn_decode_ok: d_model in {512, 768, 1024}
        rc, pl, args = decode(L, D)
        assert rc == E_BADARG and zeroed(pl), D
        assert L.lako_xattn_decode(*args, None) == E_BADARG
    assert L.lako_xattn_decode_plan(PQ, 768 * 16, 768, PE, 768, PKOFF, PML, PPC, 12, 768, 3, 7, None) == E_BADARG

