"""The multi-tile decode dispatch (lako_xattn_decode_multi) as a decision table, and the refusals of the two new launching entries, on a
host without a GPU: the plan query goes through the launching entry's validation and decision code and launches nothing, so every gate
is pinned with pointer VALUES that are never dereferenced (as tests/test_xattn_plan_cpu.py does for the single-tile entry).

The expected plans are the written rule, not a reading of the plan function: RT = the largest of 4 | 2 | 1 that is <= K and for which a
ring of >= 2 stages [32 keys × D] bf16 plus RT × 16 KiB of partial score tiles fits 160 KiB of LDS (D = 512, 768: 4; D = 1024: 2 — and
the compiler's resource report shows no scratch for any of them, DESIGN.md §3 "Sampled decoding"); three stages where they fit next to
the tiles, else two; grid (key ranges, samples, ceil(K / RT))."""
import ctypes as C
import os
import subprocess

import pytest

from lako_amd import _lib
from lako_amd._lib import XK_DECODE_MULTI, XattnPlan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_BADARG, E_ALIGN = 0, -1, -2
PQ, PE, PKOFF, PML, PPC, PLOG, PSEQ, PNXT, PDONE, PSC, PND, PPAR = (0x100000000000 + i * 0x010000000000 for i in range(12))


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["bash", os.path.join(ROOT, "lako_amd", "csrc", "build.sh")], check=True)
    _lib._lib = None
    return _lib.load()


def zeroed(pl):
    return all(getattr(pl, n) == 0 for n, _ in pl._fields_)


def multi(L, D, K, *, R=12, B=3, Z=7, rt=0, q=PQ, e=PE, e_ld=None, q_ld=None, q_sk=None, q_sb=None, k_off=PKOFF, ml=PML, pc=PPC):
    pl = XattnPlan()
    e_ld = D if e_ld is None else e_ld
    q_ld = D if q_ld is None else q_ld
    q_sk = 16 * q_ld if q_sk is None else q_sk
    q_sb = max(K, 1) * q_sk if q_sb is None else q_sb
    args = (q, q_sb, q_sk, q_ld, e, e_ld, k_off, ml, pc, R, D, B, K, Z, rt)
    return L.lako_xattn_decode_multi_plan(*args, C.byref(pl)), pl, args


def expected(D, K, rt=0):
    stage, tile = 32 * D * 2, 8 * 32 * 16 * 4
    if not rt:
        rt = next(c for c in (4, 2, 1) if c <= K and 2 * stage + c * tile <= 160 * 1024)
    stages = 3 if 3 * stage + rt * tile <= 160 * 1024 else 2
    return rt, stages, stages * stage + rt * tile


@pytest.mark.parametrize("D", [512, 768, 1024])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 8, 9, 64])
def test_row_tiles_ring_and_grid(L, D, K):
    rc, pl, _ = multi(L, D, K)
    rt, stages, lds = expected(D, K)
    assert rc == OK and (pl.kernel, pl.ks, pl.nt, pl.stages, pl.lds) == (XK_DECODE_MULTI, D // 256, rt, stages, lds), pl
    assert (pl.gx, pl.gy, pl.gz, pl.block) == (7, 3, -(-K // rt), 512) and pl.lds <= 160 * 1024, pl
    assert rt == min({512: 4, 768: 4, 1024: 2}[D], max(c for c in (1, 2, 4) if c <= K))
    from lako_amd.ops import HipOps
    assert HipOps.xattn_decode_multi_tiles(D, K) == pl.nt          # what Engine.generate sizes its key ranges by
    for force in (1, 2, 4):
        rc, p2, args = multi(L, D, K, rt=force, e_ld=D + 8, q_ld=D + 64)
        if force == 4 and D == 1024:          # 2 × 64 KiB of stages + 64 KiB of tiles do not fit
            assert rc == E_BADARG and zeroed(p2)
            assert L.lako_xattn_decode_multi(*args, None) == E_BADARG
            continue
        _, stages, lds = expected(D, K, force)
        assert rc == OK and (p2.kernel, p2.nt, p2.stages, p2.lds, p2.gz) == (XK_DECODE_MULTI, force, stages, lds, -(-K // force)), p2


def test_the_arithmetic_the_rule_rests_on():
    assert expected(768, 8) == (4, 2, 96 * 1024 + 64 * 1024) and expected(1024, 8) == (2, 2, 128 * 1024 + 32 * 1024)
    assert expected(512, 8) == (4, 3, 160 * 1024) and expected(768, 1) == (1, 3, 160 * 1024)


def test_refusals_are_the_single_tile_entrys_plus_k(L):
    for kw in (dict(q=None), dict(e=None), dict(k_off=None), dict(ml=None), dict(pc=None), dict(R=0), dict(R=17), dict(B=0), dict(Z=0),
               dict(Z=65), dict(e_ld=772), dict(e_ld=760), dict(e_ld=1 << 20), dict(q_ld=772), dict(q_sb=12 * 768 + 4), dict(q_sk=772),
               dict(rt=3), dict(rt=8), dict(rt=-1)):
        rc, pl, args = multi(L, 768, 4, **kw)
        assert rc == E_BADARG and zeroed(pl), (kw, rc, pl)
        assert L.lako_xattn_decode_multi(*args, None) == E_BADARG, kw
    for K in (0, -1, 65536):
        rc, pl, args = multi(L, 768, K)
        assert rc == E_BADARG and zeroed(pl), K
        assert L.lako_xattn_decode_multi(*args, None) == E_BADARG
    for kw in (dict(q=PQ + 8), dict(e=PE + 2), dict(pc=PPC + 4)):
        rc, pl, args = multi(L, 768, 4, **kw)
        assert rc == E_ALIGN and zeroed(pl), kw
        assert L.lako_xattn_decode_multi(*args, None) == E_ALIGN
    for D in (128, 256, 640, 896, 2048):
        rc, pl, args = multi(L, D, 4)
        assert rc == E_BADARG and zeroed(pl), D
        assert L.lako_xattn_decode_multi(*args, None) == E_BADARG
    assert L.lako_xattn_decode_multi_plan(*multi(L, 768, 4)[2], None) == E_BADARG
    buf = C.create_string_buffer(256)
    multi(L, 768, 0)
    assert L.lako_last_error(buf, 256) > 0 and b"lako_xattn_decode_multi" in buf.value


def test_sample_step_refuses_bad_arguments_before_any_launch(L):
    def call(logits=PLOG, V=32128, rows=4, group=2, seq=PSEQ, seq_ld=16, pos=3, nxt=PNXT, done=PDONE, score=PSC, nd=PND, params=PPAR, step=2):
        return L.lako_sample_step(logits, V, rows, group, seq, seq_ld, pos, nxt, done, score, nd, params, step, 1, 0, None)
    for kw in (dict(logits=None), dict(seq=None), dict(nxt=None), dict(done=None), dict(nd=None), dict(params=None), dict(V=0),
               dict(V=1 << 30), dict(rows=0), dict(group=0), dict(pos=-1), dict(pos=16), dict(step=-1)):
        assert call(**kw) == E_BADARG, kw
    assert call(params=PPAR + 2) == E_ALIGN
    buf = C.create_string_buffer(256)
    assert L.lako_last_error(buf, 256) > 0 and b"lako_sample_step" in buf.value
