"""-m gpu: every dispatch branch and tile edge of the cross-attention kernels (csrc/xattn.hip) against fp64, on real memory.

tests/test_xattn_plan_cpu.py pins WHICH kernel each gate selects; this file runs the calls at the smallest shapes at which each branch, tile
edge and loop trip count is reached.  Every call is
  1. planned, where the entry chooses between kernels (HipOps.xattn_softmax_plan / headbatch_nt_plan / xattn_decode_plan — the plan the
     launch consumes): a moved gate fails here instead of silently testing another kernel;
  2. compared with an fp64 torch evaluation of the same bf16 / fp32 inputs; where the kernel rounds an intermediate to bf16 the reference
     rounds at the same place (key-split slabs: summed in fp32 in slab order, then cast; decode: exp(s − max) cast before the context product);
  3. guarded: every output is a window of a larger buffer filled with GUARD, and everything outside the window must come back untouched;
  4. poisoned: every operand is a window of a NaN-filled buffer — rows before and after E, query / probability rows past R, columns past D
     (e_ld, q_ld > D): an over-read that reaches an accumulator makes an output non-finite.

Bounds.  An fp32-accumulated product of bf16 operands over a contraction of length n is within n·2⁻²⁴·(|A|·|B|ᵀ) of the exact product for
any summation order (products of two bf16 numbers are exact in fp32); the tests allow twice that, n·2⁻²³·(|A|·|B|ᵀ), elementwise.  A bf16
output adds 2⁻⁸·|ref| (round to nearest: 2⁻⁹ relative), an fp32 accumulation onto C adds 2⁻²³·|ref|.  Softmax and decode keep the bounds of
tests/test_xattn_gpu.py, applied per sample so that a wrong short sample cannot hide behind a long one: stats rtol 1e-5 / atol 1e-6, P within
2⁻⁸ of the sample's largest probability, dS rel_l2 < 4e-3, decode part_ml rtol 2e-3 / atol 1e-4, decode context rel_l2 < 6e-3 against the
restatement and < 1e-2 against the direct form.  No case needed a wider bound."""
import numpy as np
import pytest
import torch

from lako_amd._lib import XK_DECODE, XK_HB_CONTRACT, XK_HB_NT, XK_SOFTMAX, XK_SOFTMAX_REG
from tests.ref_ops import M32, attn_keep_mask, drop_key

pytestmark = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GUARD = 77.0            # exact in bf16 and fp32; no result of these tests equals it over a whole window
NAN = float("nan")
LENS = [1, 127, 128, 129, 255, 256, 257, 385]      # every nk edge of the two 128-key images of a score tile, and of the 64-key context stages
E_TAIL = 256            # NaN rows behind E: more than one score tile's second image, so an over-read stays inside the buffer


@pytest.fixture(scope="module")
def ops():
    from lako_amd.ops import HipOps
    return HipOps()


def dev():
    return torch.device("cuda:0")


def rnd(*shape, dtype=F32, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev())


def inside(t, pads, fill):
    """`t` as a window of a larger buffer filled with `fill`: pads = (before, after) per dim -> (window, buffer, slices)"""
    big = torch.full([b + n + a for n, (b, a) in zip(t.shape, pads)], fill, dtype=t.dtype, device=dev())
    sl = tuple(slice(b, b + n) for n, (b, _) in zip(t.shape, pads))
    big[sl] = t
    return big[sl], big, sl


def untouched(big, sl, what):
    """everything of `big` outside the window still holds GUARD"""
    c = big.clone()
    c[sl] = GUARD
    bad = (c != GUARD).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} elements outside the output window were written, first at {bad[:4].tolist()}"


def offsets(lens):
    """k_off (packed rows) and p_off (segments padded to 256 columns) of samples with `lens` keys"""
    k = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    p = np.concatenate([[0], np.cumsum([(n + 255) // 256 * 256 for n in lens])]).astype(np.int32)
    return torch.from_numpy(k).to(dev()), torch.from_numpy(p).to(dev()), k.tolist(), p.tolist()


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def within(got, ref, bound, what):
    """|got − ref| <= bound elementwise; the worst ratio is printed before it is asserted"""
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite result (an operand's NaN surroundings were read)"
    err = (got.double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: max err / bound = {ratio:.3f}")
    assert bool((err <= bound).all()), f"{what}: max err / bound = {ratio:.3f}, max err {float(err.max()):.3e}"


def encoder_states(total, D, seed=1):
    """E [total, D] bf16 with row stride D + 8, 3 NaN rows before it and E_TAIL behind it"""
    return inside(rnd(total, D, dtype=BF, seed=seed), [(3, E_TAIL), (0, 8)], NAN)[0]


# ---- scores ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [128, 512, 2048])
@pytest.mark.parametrize("R,extra", [(5, 0), (16, 512), (129, 0), (300, 0)])
def test_scores(ops, R, D, extra):
    """xscores_kernel: one to three row chunks (R 5 … 300), two to 32 K slices (D), every key-count edge of a tile (LENS), and p_total
    512 columns beyond p_off[B] (extra: the workgroups past the batch's columns return at once)."""
    B = len(LENS)
    k_off, p_off, ko, po = offsets(LENS)
    ptot = po[-1]
    E = encoder_states(ko[-1], D)
    Q = inside(rnd(B, R, D, dtype=BF, seed=2), [(0, 0), (2, 2), (0, 8)], NAN)[0]       # rows of other layers around the R rows, q_ld > D
    S, Sbig, sl = inside(torch.full((R, ptot + extra), GUARD, device=dev()), [(1, 2), (4, 4)], GUARD)
    assert E.stride(0) == D + 8 and Q.stride(1) == D + 8 and S.stride(0) % 4 == 0
    ops.xattn_scores(Q, E, k_off, p_off, ptot + extra, S)
    torch.cuda.synchronize()
    untouched(Sbig, sl, "scores")
    assert bool((S[:, ptot:] == GUARD).all()), "columns past p_off[B] were written"
    for b, n in enumerate(LENS):
        q, e = Q[b].double(), E[ko[b]:ko[b + 1]].double()
        within(S[:, po[b]:po[b] + n], q @ e.T, D * 2.0 ** -23 * (q.abs() @ e.abs().T), f"scores R={R} D={D} sample {b} ({n} keys)")
        pad = S[:, po[b] + n:po[b + 1]]
        assert bool((pad == 0).all()), f"sample {b} ({n} keys): padding columns are not exactly zero (a tile read into the next sample)"


# ---- context -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [128, 512, 2048])
@pytest.mark.parametrize("R", [5, 16, 129, 300])
def test_context(ops, R, D):
    """xcontext_kernel: grid.x 1 … 16 column blocks, one to three row chunks, every partial last stage (LENS), 1 / 3 / 64 key ranges
    (64: most slabs own no stage and must still be written: zeros over the NaN prefill), twice for bit-identity."""
    B = len(LENS)
    k_off, p_off, ko, po = offsets(LENS)
    ptot = po[-1]
    E = encoder_states(ko[-1], D)
    P0 = torch.zeros(R, ptot, dtype=BF, device=dev())              # the layout's contract: zeros in the padding columns
    for b, n in enumerate(LENS):
        P0[:, po[b]:po[b] + n] = rnd(R, n, dtype=BF, scale=0.05, seed=10 + b)
    P = inside(P0, [(2, 3), (0, 8)], NAN)[0]                       # rows past R and columns past p_total are NaN
    ref = [P[:, po[b]:po[b] + n].double() @ E[ko[b]:ko[b + 1]].double() for b, n in enumerate(LENS)]
    mag = [P[:, po[b]:po[b] + n].double().abs() @ E[ko[b]:ko[b + 1]].double().abs() for b, n in enumerate(LENS)]
    for Z in (1, 3, 64):
        runs = []
        for _ in range(2):
            out, big, sl = inside(torch.full((Z, B, R, D), NAN, device=dev()), [(0, 0), (0, 0), (1, 2), (0, 64)], GUARD)
            ops.xattn_context(P, E, k_off, p_off, out)
            torch.cuda.synchronize()
            untouched(big, sl, f"context Z={Z}")
            runs.append(out)
        out = runs[0]
        assert torch.equal(runs[0], runs[1]), f"context Z={Z}: two runs differ"        # no atomics
        for b, n in enumerate(LENS):
            nst = -(-n // 64)
            for z in range(Z):
                if z * nst // Z == (z + 1) * nst // Z:               # a key range without a stage
                    assert bool((out[z, b] == 0).all()), f"context Z={Z} sample {b}: slab {z} owns no keys and is not zero"
            within(out[:, b].double().sum(0), ref[b], n * 2.0 ** -23 * mag[b], f"context R={R} D={D} Z={Z} sample {b} ({n} keys)")


# ---- softmax -----------------------------------------------------------------------------------------------------------------------
def keep_of(b, T, H, n, max_keys, drop):
    """keep[r = t·H + h, s] of sample b: the attention recipe with bh = b·H + h, q = t, k = s, Lk = max_keys (ref_ops.RefOps._xkeep)"""
    pr, seed, site = drop
    keep = attn_keep_mask((b + 1) * H, T, max_keys, drop_key(int(seed) & M32, int(site) & M32), pr, dev())[b * H:, :, :n]
    return keep.permute(1, 0, 2).reshape(T * H, n)


SOFTMAX = [  # (id, lens, max_keys, kernel, nv, shift)
    ("reg4_limit", [4093, 4096, 1, 259], 4096, XK_SOFTMAX_REG, 4, False),
    ("reg8_both_ends", [4097, 8192, 3, 8190], 8192, XK_SOFTMAX_REG, 8, False),
    ("general_8193", [8193, 300, 2], 8193, XK_SOFTMAX, 0, False),            # multi-trip loops next to a 2-key row
    ("general_short_rows", [300, 129, 1], 9000, XK_SOFTMAX, 0, False),
    ("max_keys_plus_7", [300, 129, 1], 307, XK_SOFTMAX_REG, 4, False),
    ("reg8_shifted", [4097, 700, 3], 8192, XK_SOFTMAX_REG, 8, True),
    ("general_shifted", [8193, 5], 8193, XK_SOFTMAX, 0, True),
]


SOFTMAX_RUNS = [(c, T, p) for c in SOFTMAX for T in (1, 5) for p in (0.0, 0.1) if not (c[5] and p > 0)]      # the shifted rows: no dropout


@pytest.mark.parametrize("case,T,p", SOFTMAX_RUNS, ids=[f"{c[0]}-T{T}-p{p}" for c, T, p in SOFTMAX_RUNS])
def test_softmax_fwd_bwd(ops, case, T, p):
    """xsoftmax_reg_kernel<·, 4 | 8> and xsoftmax_kernel, forward and backward, on both sides of the gates at 4096 and 8192 columns, with
    T = 5 (two query blocks of the dropout recipe: t >> 2 is 0 and 1) and T = 1.  The shifted cases add ±1e4 to whole rows of S (S holds
    multiples of 2⁻⁸, so the shift is exact in fp32): softmax is shift-invariant, the same bounds must hold — the max subtraction."""
    _, lens, max_keys, kernel, nv, shift = case
    H, B = 4, len(lens)
    R = T * H
    k_off, p_off, ko, po = offsets(lens)
    ptot = po[-1]
    drop = (p, 1234, 77) if p > 0 else None
    S0, dP0 = torch.zeros(R, ptot, device=dev()), torch.zeros(R, ptot, device=dev())          # the layout's contract: zero padding
    for b, n in enumerate(lens):
        s = rnd(R, n, scale=3.0, seed=20 + b)
        if shift:
            s = torch.round(s * 256) / 256 + torch.where(torch.arange(R, device=dev()) % 2 == 0, 1e4, -1e4)[:, None]
        S0[:, po[b]:po[b] + n] = s
        dP0[:, po[b]:po[b] + n] = rnd(R, n, scale=0.5, seed=30 + b)
    S = inside(S0, [(1, 1), (0, 260)], NAN)[0]
    dP = inside(dP0, [(1, 1), (0, 260)], NAN)[0]
    stats, stbig, stsl = inside(torch.zeros(B, R, 2, device=dev()), [(1, 1), (0, 0), (0, 0)], GUARD)
    P, Pbig, Psl = inside(torch.full((R, ptot + 256), 9.0, dtype=BF, device=dev()), [(1, 1), (0, 8)], GUARD)
    dS, dSbig, dSsl = inside(torch.full((R, ptot + 256), 9.0, dtype=BF, device=dev()), [(1, 1), (0, 8)], GUARD)

    pl = ops.xattn_softmax_plan(S, stats, P, k_off, p_off, T, H, max_keys, drop)
    assert (pl.kernel, pl.nv, pl.bwd, pl.gx, pl.gy) == (kernel, nv, 0, R, B), pl
    pl = ops.xattn_softmax_plan(S, stats, dS, k_off, p_off, T, H, max_keys, drop, dP=dP)
    assert (pl.kernel, pl.nv, pl.bwd, pl.gx, pl.gy) == (kernel, nv, 1, R, B), pl

    ops.xattn_softmax_fwd(S, stats, P, k_off, p_off, T, H, max_keys, drop)
    ops.xattn_softmax_bwd(S, dP, stats, dS, k_off, p_off, T, H, max_keys, drop)
    torch.cuda.synchronize()
    for big, sl, nm in ((stbig, stsl, "stats"), (Pbig, Psl, "P"), (dSbig, dSsl, "dS")):
        untouched(big, sl, f"softmax {nm}")
    assert bool((P[:, ptot:] == 9.0).all()) and bool((dS[:, ptot:] == 9.0).all()), "columns past p_off[B] were written"
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    for b, n in enumerate(lens):
        what = f"softmax {case[0]} T={T} p={p} sample {b} ({n} keys)"
        s, d = S[:, po[b]:po[b] + n].double(), dP[:, po[b]:po[b] + n].double()
        m = s.max(-1).values
        e = torch.exp(s - m[:, None])
        l = e.sum(-1)
        pn = e / l[:, None]
        keep = keep_of(b, T, H, n, max_keys, drop) if drop else torch.ones(R, n, dtype=torch.bool, device=dev())
        pd = torch.where(keep, pn * scale, torch.zeros_like(pn))
        dd = torch.where(keep, d * scale, torch.zeros_like(d))
        ds = pn * (dd - (pn * dd).sum(-1, keepdim=True))
        want = torch.stack([m, 1.0 / l], -1)
        print(f"{what}: stats max rel err {float(((stats[b].double() - want).abs() / want.abs().clamp_min(1e-30)).max()):.2e}")
        assert torch.allclose(stats[b].double(), want, rtol=1e-5, atol=1e-6), what
        got = P[:, po[b]:po[b] + n]
        assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(dS[:, po[b]:po[b] + n]).all()), what
        assert torch.equal(got != 0, keep), f"{what}: the dropped probabilities differ from the recipe"
        perr = float((got.double() - pd).abs().max()) / float(pd.max())
        print(f"{what}: P max err / sample max = {perr:.2e}")
        assert perr <= 2.0 ** -8, (what, perr)
        for t, nm in ((P, "P"), (dS, "dS")):
            assert bool((t[:, po[b] + n:po[b + 1]] == 0).all()), f"{what}: {nm} padding is not rewritten to zero"
        if drop and n > 100:      # R·n draws kept with probability 1 − p: four standard deviations of the binomial
            frac = float(keep.double().mean())
            assert abs(frac - (1 - p)) < 4 * (p * (1 - p) / (R * n)) ** 0.5, (what, frac)
        r = rel_l2(dS[:, po[b]:po[b] + n], ds)
        print(f"{what}: dS rel_l2 = {r:.2e}")
        assert r < 4e-3, (what, r)


# ---- head-batched NT ---------------------------------------------------------------------------------------------------------------
HB_NT = [  # (id, N, K, A: "bf16" | number of fp32 slabs, kernel, ks, nt, ku)
    *[(f"contract{K}_{a}", 64, K, a, XK_HB_CONTRACT, K // 128, 0, 0) for K in (512, 768, 1024) for a in ("bf16", 1, 2, 4, 5)],
    ("xl_2048_slabs3", 64, 2048, 3, XK_HB_NT, 0, 1, 8),
    ("xl_2048_bf16", 64, 2048, "bf16", XK_HB_NT, 0, 1, 8),
    ("d128_slabs2", 64, 128, 2, XK_HB_NT, 0, 1, 1),
    ("d128_bf16", 64, 128, "bf16", XK_HB_NT, 0, 1, 1),
    ("expand_128", 128, 64, "bf16", XK_HB_NT, 0, 4, 2),
    ("expand_128_fp32", 128, 64, 1, XK_HB_NT, 0, 4, 2),
    ("expand_2048", 2048, 64, "bf16", XK_HB_NT, 0, 4, 2),
    ("nt4_ku1", 128, 96, "bf16", XK_HB_NT, 0, 4, 1),
    ("nt4_ku1_fp32", 128, 96, 2, XK_HB_NT, 0, 4, 1),
]
BT_NT = [(1, 1), (5, 3), (1, 17), (10, 13)]      # M = B·T = 1, 15, 17, 130: a lone row, one short tile, a tile and a row, nine tiles; T ∤ 16


@pytest.mark.parametrize("case", HB_NT, ids=[c[0] for c in HB_NT])
def test_headbatch_nt(ops, case):
    """every kernel lako_headbatch_nt chooses between, bf16 and fp32 A, 1 … 5 key-split slabs (the contract kernel holds four in
    registers and loops over the rest), rows in strided per-sample blocks"""
    _, N, K, akind, kernel, ks, nt, ku = case
    H = 3
    Bw = inside(rnd(H, N, K, dtype=BF, scale=0.05, seed=4), [(0, 0), (0, 1), (0, 8)], NAN)[0]
    for Bz, T in BT_NT:
        what = f"headbatch_nt {case[0]} M={Bz * T}"
        if akind == "bf16":
            A = inside(rnd(Bz, T, H, K, dtype=BF, seed=3), [(0, 0), (1, 2), (0, 1), (0, 8)], NAN)[0]
            a_used = A.double()
        else:
            A = inside(rnd(akind, Bz, T, H, K, seed=3), [(0, 0), (0, 0), (1, 2), (0, 1), (0, 8)], NAN)[0]
            acc = A[0].clone()
            for z in range(1, akind):          # the kernel's order: fp32 adds in slab order, then one cast
                acc = acc + A[z]
            a_used = acc.to(BF).double()
            if akind == 1:
                A = A[0]
        Cm, big, sl = inside(torch.full((Bz, T, H, N), GUARD, dtype=BF, device=dev()), [(0, 0), (1, 1), (0, 0), (0, 4)], GUARD)
        pl = ops.headbatch_nt_plan(A, Bw, Cm)
        assert (pl.kernel, pl.af32, pl.ks, pl.nt, pl.ku) == (kernel, int(akind != "bf16"), ks, nt, ku), (what, pl)
        ops.headbatch_nt(A, Bw, Cm)
        torch.cuda.synchronize()
        untouched(big, sl, what)
        ref = torch.einsum("bthk,hnk->bthn", a_used, Bw.double())
        mag = torch.einsum("bthk,hnk->bthn", a_used.abs(), Bw.double().abs())
        within(Cm, ref, K * 2.0 ** -23 * mag + 2.0 ** -8 * ref.abs(), what)


# ---- head-batched TN ---------------------------------------------------------------------------------------------------------------
BT_TN = [(1, 1), (11, 3), (8, 16), (43, 3), (20, 15)]      # M = 1, 33, 128, 129, 300: partial first block, one full block, one row more, three trips


def tn_problem(Bz, T, H, N, bkind, seed):
    A = inside(rnd(Bz, T, H, 64, dtype=BF, seed=seed), [(0, 0), (1, 2), (0, 1), (0, 8)], NAN)[0]
    if bkind == "bf16":
        Bm = inside(rnd(Bz, T, H, N, dtype=BF, seed=seed + 1), [(0, 0), (1, 2), (0, 1), (0, 8)], NAN)[0]
        b_used = Bm.double()
    else:
        Bm = inside(rnd(bkind, Bz, T, H, N, seed=seed + 1), [(0, 0), (0, 0), (1, 2), (0, 1), (0, 8)], NAN)[0]
        acc = Bm[0].clone()
        for z in range(1, bkind):
            acc = acc + Bm[z]
        b_used = acc.to(BF).double()
        if bkind == 1:
            Bm = Bm[0]
    return A, Bm, b_used


@pytest.mark.parametrize("N", [128, 2048])
@pytest.mark.parametrize("bkind", ["bf16", 1, 2, 5])
def test_headbatch_tn(ops, N, bkind):
    """hb_tn_kernel: the M loop in blocks of 128 with a partial last block (32-row sub-blocks past M are skipped), bf16 B and fp32 B in
    1 / 2 / 5 slabs, accumulated onto a non-zero C that is a window of a larger guarded gradient"""
    H = 3
    for Bz, T in BT_TN:
        M = Bz * T
        what = f"headbatch_tn N={N} B={bkind} M={M}"
        A, Bm, b_used = tn_problem(Bz, T, H, N, bkind, 3)
        C0 = rnd(H, 64, N, seed=7)
        Cw, big, sl = inside(C0, [(0, 0), (1, 1), (4, 4)], GUARD)
        ops.headbatch_tn(A, Bm, Cw)
        torch.cuda.synchronize()
        untouched(big, sl, what)
        ref = C0.double() + torch.einsum("bthj,bthc->hjc", A.double(), b_used)
        mag = torch.einsum("bthj,bthc->hjc", A.double().abs(), b_used.abs())
        within(Cw, ref, M * 2.0 ** -23 * mag + 2.0 ** -23 * ref.abs(), what)


@pytest.mark.parametrize("bkind", ["bf16", 2])
def test_headbatch_tn_multi_equals_single_launches(ops, bkind):
    H, N, (Bz, T) = 3, 128, BT_TN[-1]                       # M = 300
    probs = [tn_problem(Bz, T, H, N, bkind, 40 + 2 * i)[:2] for i in range(3)]
    multi = [inside(rnd(H, 64, N, seed=60 + i), [(0, 0), (1, 1), (4, 4)], GUARD) for i in range(3)]
    single = [inside(rnd(H, 64, N, seed=60 + i), [(0, 0), (1, 1), (4, 4)], GUARD) for i in range(3)]
    ops.headbatch_tn_multi([(A, Bm, g[0]) for (A, Bm), g in zip(probs, multi)])
    for (A, Bm), g in zip(probs, single):
        ops.headbatch_tn(A, Bm, g[0])
    torch.cuda.synchronize()
    for i, (gm, gs) in enumerate(zip(multi, single)):
        assert bool(torch.isfinite(gm[0]).all())
        assert torch.equal(gm[1], gs[1]), f"problem {i}: one launch for all differs from its own launch"
        untouched(gm[1], gm[2], f"headbatch_tn_multi problem {i}")


# ---- decode + combine ----------------------------------------------------------------------------------------------------------------
DECODE_LENS = [1, 31, 32, 33, 64, 65, 2000]       # the edges of the 32-key stages, and a row of 63 stages


@pytest.mark.parametrize("Z", [1, 7, 64])
@pytest.mark.parametrize("D,H", [(512, 8), (768, 12), (1024, 16), (768, 1)])
def test_decode_and_combine(ops, D, H, Z):
    """xdecode_kernel<2 | 3 | 4> (ring of 3 / 3 / 2 stages) and xdecode_combine_kernel, per sample: one range, seven, and 64 (most
    ranges of the short samples hold no key: −inf, 0 and zeros, which the combine must ignore)"""
    lens = DECODE_LENS
    B = len(lens)
    k_off, _, ko, _ = offsets(lens)
    E = encoder_states(ko[-1], D)
    Q = inside(rnd(B, H, D, dtype=BF, scale=0.08, seed=2), [(0, 0), (1, 3), (0, 8)], NAN)[0]
    Wv = inside(rnd(H * 64, D, dtype=BF, scale=0.05, seed=3), [(1, 1), (0, 8)], NAN)[0]
    pml, mlbig, mlsl = inside(torch.full((Z, B, 16, 2), GUARD, device=dev()), [(1, 1), (0, 0), (0, 0), (0, 0)], GUARD)
    pc, pcbig, pcsl = inside(torch.full((Z, B, 16, D), GUARD, device=dev()), [(1, 1), (0, 0), (0, 0), (0, 0)], GUARD)
    ctx, cbig, csl = inside(torch.full((B, H * 64), GUARD, dtype=BF, device=dev()), [(1, 1), (0, 8)], GUARD)
    pl = ops.xattn_decode_plan(Q, E, k_off, pml, pc)
    assert (pl.kernel, pl.ks, pl.stages, pl.gx, pl.gy, pl.block) == (XK_DECODE, D // 256, 2 if D == 1024 else 3, Z, B, 512), pl
    ops.xattn_decode(Q, E, k_off, pml, pc)
    ops.xattn_decode_combine(pml, pc, Wv, ctx, H)
    torch.cuda.synchronize()
    for big, sl, nm in ((mlbig, mlsl, "part_ml"), (pcbig, pcsl, "part_c"), (cbig, csl, "ctx")):
        untouched(big, sl, f"decode {nm}")
    wv = Wv.double().view(H, 64, D)
    for b, n in enumerate(lens):
        what = f"decode D={D} H={H} Z={Z} sample {b} ({n} keys)"
        e, q = E[ko[b]:ko[b + 1]].double(), Q[b].double()
        s = q @ e.T                                                 # [H, n]
        nst = -(-n // 32)
        m_ref = torch.full((Z, H), -float("inf"), dtype=F64, device=dev())
        l_ref = torch.zeros(Z, H, dtype=F64, device=dev())
        c_ref = torch.zeros(Z, H, D, dtype=F64, device=dev())
        for z in range(Z):
            lo, hi = min(n, (z * nst // Z) * 32), min(n, ((z + 1) * nst // Z) * 32)
            if hi > lo:
                m_ref[z] = s[:, lo:hi].max(-1).values
                pz = torch.exp(s[:, lo:hi] - m_ref[z][:, None])
                l_ref[z] = pz.sum(-1)
                c_ref[z] = pz.to(BF).double() @ e[lo:hi]         # the kernel's probabilities are bf16 MFMA operands
        got_m, got_l = pml[:, b, :H, 0].double(), pml[:, b, :H, 1].double()
        empty = torch.isinf(m_ref)
        assert torch.equal(torch.isinf(got_m) & (got_m < 0), empty), what
        assert bool((got_l[empty] == 0).all()) and bool((pc[:, b, :H][empty] == 0).all()), what
        assert torch.allclose(got_m[~empty], m_ref[~empty], rtol=2e-3, atol=1e-4), what
        assert torch.allclose(got_l[~empty], l_ref[~empty], rtol=2e-3, atol=1e-4), what
        w = torch.where(empty, torch.zeros_like(m_ref), torch.exp(m_ref - m_ref.max(0).values[None]))
        c = (w[..., None] * c_ref).sum(0) / (w * l_ref).sum(0)[:, None]
        restated = torch.einsum("hc,hjc->hj", c, wv)
        direct = torch.einsum("hc,hjc->hj", torch.softmax(s, -1) @ e, wv)
        got = ctx[b].double().view(H, 64)
        assert bool(torch.isfinite(got).all()), what
        r1, r2 = rel_l2(got, restated), rel_l2(got, direct)
        print(f"{what}: ctx rel_l2 {r1:.2e} (restatement) {r2:.2e} (direct)")
        assert r1 < 6e-3 and r2 < 1e-2, (what, r1, r2)
