"""-m gpu: both sides of the GEMM dispatch gates, on real memory.

tests/test_gemm_plan_cpu.py pins WHICH kernel every gate selects; this file runs the calls.  For every gate a call just inside it (the
fast kernel) and one just outside (the documented fallback — reachable through the C-ABI, and by no other test: bf16 stores of
N % 8 == 4 columns, a C that is 8- but not 16-byte aligned, ldc % 8 == 4, a residual / aux operand at any offset) is
  1. planned: the two sides must be the kernels the gate is named after — a sweep whose sides run the same kernel fails;
  2. compared with epilogue(alpha · A.double() @ B.double().T) in fp64 torch under close(..., tight=True)'s bounds for the output dtype
     (tests/test_kernels_gpu.py: fp32 arithmetic on the given operands and ONE rounding — the fallbacks are specified to do the same);
  3. guarded: C sits inside a larger buffer of NaN bit patterns no result can equal — gap columns between N and ldc, rows before and after,
     the elements in front of an offset C — and every bit outside the [M, N] window must survive;
  4. poisoned: A, B, the residual and the aux operand sit inside NaN-filled buffers (columns between K and lda, rows before and after, the
     elements in front of an offset side operand): an over-read that reaches an accumulator or an epilogue makes the output non-finite."""
import pytest
import torch

from lako_amd._lib import NT_128, NT_EIGHT, NT_FOUR, NT_MX_EIGHT, NT_MX_FOUR, NT_REFUSED, NT_RING, NT_SKINNY, NT_SKINNY_NORM
from tests.ref_ops import keep_mask
from tests.test_kernels_gpu import close, dev, rnd

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def ops():
    from lako_amd.ops import HipOps
    return HipOps()


GUARD = {BF: (torch.int16, 0x7FA5), F32: (torch.int32, 0x7FA5A5A5)}      # quiet NaNs with a payload no kernel produces

EPIS = {"plain": dict(), "alpha": dict(alpha=0.5), "relu+drop": dict(relu=True, drop=(0.1, 5, 6)), "resid+drop": dict(resid=True, drop=(0.1, 7, 8)),
        "aux": dict(aux=True, aux_scale=1.1),
        # the combinations the four-wave kernels do not implement — and would silently ignore parts of, were their gate to let them in
        "resid": dict(resid=True), "relu+resid": dict(relu=True, resid=True), "relu+aux": dict(relu=True, aux=True, aux_scale=1.1),
        "alpha+drop": dict(alpha=0.5, drop=(0.1, 5, 6)), "alpha+relu": dict(alpha=0.5, relu=True), "alpha+resid+drop": dict(alpha=0.5, resid=True, drop=(0.1, 7, 8)),
        "alpha+aux": dict(alpha=0.5, aux=True, aux_scale=1.1), "aux+drop": dict(aux=True, aux_scale=1.0 / 0.9, drop=(0.1, 3, 4))}
ALL, SIDE = ("plain", "relu+drop", "resid+drop", "aux"), ("resid+drop", "aux")


def window(rows, cols, dtype, *, ld=None, off=0, fill="nan", seed=0, lead=2):
    """a [rows, cols] view with row stride ld, `lead` rows + `off` elements into a larger buffer filled with NaN (operands) or the guard
    pattern (outputs); returns (view, whole buffer)"""
    ld = ld or cols
    buf = torch.empty((rows + 2 * lead) * ld + 64, dtype=dtype, device=dev())
    it, pat = GUARD[dtype]
    if fill == "guard":
        buf.view(it).fill_(pat)
    else:
        buf.fill_(float("nan"))
    v = torch.as_strided(buf, (rows, cols), (ld, 1), lead * ld + off)
    if fill == "nan":
        v.copy_(rnd(rows, cols, dtype=dtype, seed=seed))
    return v, buf


def untouched_outside(view, buf, what):
    """every element of `buf` outside `view` still holds the guard pattern, bit for bit"""
    it, pat = GUARD[buf.dtype]
    bits = buf.view(it).clone()
    torch.as_strided(bits, view.shape, view.stride(), view.storage_offset()).fill_(pat)
    bad = (bits != pat).nonzero().flatten()
    assert bad.numel() == 0, f"{what}: {bad.numel()} elements outside the output window were written, first at flat index {bad[:8].tolist()} " \
                             f"(window starts at {view.storage_offset()}, row stride {view.stride(0)}, {tuple(view.shape)})"


def reference(A, B, kw, resid, aux):
    v = (A.double() @ B.double().t()) * kw.get("alpha", 1.0)
    if kw.get("relu"):
        v = torch.relu(v)
    if aux is not None:
        v = torch.where(aux.double() > 0, v * kw.get("aux_scale", 1.0), torch.zeros_like(v))
    if kw.get("drop"):
        M, N = v.shape
        idx = torch.arange(M, device=v.device, dtype=torch.int64)[:, None] * N + torch.arange(N, device=v.device, dtype=torch.int64)[None, :]
        keep, scale = keep_mask(kw["drop"], idx)
        v = torch.where(keep, v * scale, torch.zeros_like(v))
    if resid is not None:
        v = v + resid.double()
    return v


def run_nt(ops, what, M, N, K, epi, *, expect, knobs=None, in_t=BF, out_t=BF, ldc_pad=0, c_off=0, ld_side_pad=0, side_off=0, lda_pad=8, norm=False):
    """one call: plan == expect (a dict of lako_gemm_plan_t fields), numbers, guards.  Returns the plan."""
    kw = dict(EPIS[epi])
    if norm:
        lda_pad = 0         # (lako_rmsnorm_fwd, which the refused side falls back to, takes contiguous rows)
    A, _ = window(M, K, in_t, ld=K + lda_pad, seed=1)
    B, _ = window(N, K, in_t, ld=K + lda_pad, seed=2)
    C, Cbuf = window(M, N, out_t, ld=N + ldc_pad, off=c_off, fill="guard")
    resid = aux = None
    if kw.pop("resid", False):
        resid, _ = window(M, N, out_t, ld=N + ld_side_pad, off=side_off, seed=3)
        kw["resid"] = resid
    if kw.pop("aux", False):
        aux, _ = window(M, N, in_t, ld=N + ld_side_pad, off=side_off, seed=4)
        kw["aux"] = aux
    xn = None
    if norm:
        w = (1.0 + 0.2 * rnd(K, seed=5)).contiguous()
        xn, xnbuf = window(M, K, in_t, fill="guard")
        rs, rsbuf = window(1, M, F32, fill="guard")
        kw["norm"] = (w, 1e-6, xn, rs.view(M))
        A.mul_(3.0)
    try:
        for k_, v_ in (knobs or {}).items():
            ops.set_tuning(k_, v_)
        pl = ops.gemm_nt_plan(A, B, C, **kw)
        ops.gemm_nt(A, B, C, **kw)
        torch.cuda.synchronize()
    finally:
        for k_ in (knobs or {}):
            ops.set_tuning(k_, DEFAULTS[k_])
    untouched_outside(C, Cbuf, what)
    if norm:
        untouched_outside(xn, xnbuf, what + " (normalised rows)")
        untouched_outside(rs, rsbuf, what + " (rstd)")
        x = A.double()
        rstd = torch.rsqrt(x.pow(2).mean(-1) + 1e-6)
        torch.testing.assert_close(rs.view(M).double(), rstd, rtol=2e-6, atol=0)
        close(xn, (w.double() * (x * rstd[:, None])), in_t, what + " normalised rows", tight=True)
        A = xn                                   # the product runs on the bf16 rows the kernel hands back
        kw.pop("norm")
    want = reference(A, B, kw, resid, aux)
    # close() takes its bound from the output dtype unless told the operands are fp32: fp32 operands into a bf16 C round once, to bf16
    close(C, want, in_t if out_t == F32 or in_t == BF else BF, f"{what} [{pl}]", tight=True)
    # (the plan last: a kernel that took a call it ignores parts of is reported by its numbers, a gate that merely drifted by its plan)
    got = {f: getattr(pl, f) for f in expect}
    assert got == expect, f"{what}: planned {pl}, the gate says {expect}"
    return pl


DEFAULTS = dict(gemm_nt_variant=-1, gemm_nt_four=1, gemm_nt_tile288=1, gemm_nt_queue=0, gemm_nt_skinny=1, gemm_nt_tail_split=1, gemm_tn_four=1)
BIG = (16500, 1032, 384)            # 65 x 5 = 325 tiles of 256²: the smallest comfortable shape past one round of the chip
V9, V2, V5 = dict(gemm_nt_variant=9), dict(gemm_nt_variant=2), dict(gemm_nt_variant=5)
FOUR = dict(kernel=NT_FOUR, tile_rows=256, head_rows=0)
EIGHT_PLAIN = dict(kernel=NT_EIGHT, tile_rows=256, head_rows=0, side_lds=0, wide_epi=0)      # accumulator-layout stores, side operand from global memory


def eight(epi, fast):
    """the eight-wave 256² kernel: `fast` = LDS-staged side operand / wide epilogue, else the accumulator-layout epilogue"""
    side = epi in SIDE
    return dict(kernel=NT_EIGHT, tile_rows=256, head_rows=0, side_lds=int(fast and side), wide_epi=int(fast and not side))


# gate -> (epilogues, [(side name, run_nt keywords incl. shape, expected plan or callable(epi))])
ALIGN_GATES = {
    # the four-wave kernel (forced: its fallback is then the eight-wave 256² kernel by name) …
    "four/N%8": (ALL, [("N%8=0", dict(shape=BIG, knobs=V9), FOUR), ("N%8=4", dict(shape=(16500, 1028, 384), knobs=V9), EIGHT_PLAIN)]),
    "four/ldc%8": (ALL, [("ldc%8=0", dict(shape=BIG, knobs=V9, ldc_pad=8), FOUR), ("ldc%8=4", dict(shape=BIG, knobs=V9, ldc_pad=4), EIGHT_PLAIN)]),
    "four/C-align": (ALL, [("16B", dict(shape=BIG, knobs=V9, ldc_pad=8), FOUR), ("8B", dict(shape=BIG, knobs=V9, ldc_pad=8, c_off=4), EIGHT_PLAIN)]),
    "four/ld-side%8": (SIDE, [("%8=0", dict(shape=BIG, knobs=V9, ld_side_pad=8), FOUR), ("%8=4", dict(shape=BIG, knobs=V9, ld_side_pad=4), EIGHT_PLAIN)]),
    "four/side-offset": (SIDE, [("+0", dict(shape=BIG, knobs=V9, ld_side_pad=8), FOUR), ("+1", dict(shape=BIG, knobs=V9, ld_side_pad=8, side_off=1), EIGHT_PLAIN),
                                ("+4", dict(shape=BIG, knobs=V9, ld_side_pad=8, side_off=4), EIGHT_PLAIN)]),
    # … the eight-wave kernel's own fast epilogues (ragged edges in M and N) …
    "eight/N%8": (ALL, [("N%8=0", dict(shape=(700, 520, 200), knobs=V2), lambda e: eight(e, True)), ("N%8=4", dict(shape=(700, 516, 200), knobs=V2), lambda e: eight(e, False))]),
    "eight/ldc%8": (ALL, [("ldc%8=0", dict(shape=(700, 520, 200), knobs=V2, ldc_pad=8), lambda e: eight(e, True)),
                          ("ldc%8=4", dict(shape=(700, 520, 200), knobs=V2, ldc_pad=4), lambda e: eight(e, False))]),
    "eight/C-align": (ALL, [("16B", dict(shape=(700, 520, 200), knobs=V2, ldc_pad=8), lambda e: eight(e, True)),
                            ("8B", dict(shape=(700, 520, 200), knobs=V2, ldc_pad=8, c_off=4), lambda e: eight(e, False))]),
    "eight/ld-side%8": (SIDE, [("%8=0", dict(shape=(700, 520, 200), knobs=V2, ld_side_pad=8), lambda e: eight(e, True)),
                               ("%8=4", dict(shape=(700, 520, 200), knobs=V2, ld_side_pad=4), lambda e: eight(e, False))]),
    "eight/side-offset": (SIDE, [("+0", dict(shape=(700, 520, 200), knobs=V2, ld_side_pad=8), lambda e: eight(e, True)),
                                 ("+1", dict(shape=(700, 520, 200), knobs=V2, ld_side_pad=8, side_off=1), lambda e: eight(e, False)),
                                 ("+4", dict(shape=(700, 520, 200), knobs=V2, ld_side_pad=8, side_off=4), lambda e: eight(e, False))]),
    # … and the M <= 256 kernel, whose fallback is the ring
    "skinny/N%8": (ALL, [("N%8=0", dict(shape=(130, 264, 160)), dict(kernel=NT_SKINNY)), ("N%8=4", dict(shape=(130, 260, 160)), dict(kernel=NT_RING))]),
    "skinny/ldc%8": (ALL, [("ldc%8=0", dict(shape=(130, 264, 160), ldc_pad=8), dict(kernel=NT_SKINNY)), ("ldc%8=4", dict(shape=(130, 264, 160), ldc_pad=4), dict(kernel=NT_RING))]),
    "skinny/C-align": (ALL, [("16B", dict(shape=(130, 264, 160), ldc_pad=8), dict(kernel=NT_SKINNY)), ("8B", dict(shape=(130, 264, 160), ldc_pad=8, c_off=4), dict(kernel=NT_RING))]),
    "skinny/ld-side%8": (SIDE, [("%8=0", dict(shape=(130, 264, 160), ld_side_pad=8), dict(kernel=NT_SKINNY)), ("%8=4", dict(shape=(130, 264, 160), ld_side_pad=4), dict(kernel=NT_RING))]),
    "skinny/side-offset": (SIDE, [("+0", dict(shape=(130, 264, 160), ld_side_pad=8), dict(kernel=NT_SKINNY)), ("+1", dict(shape=(130, 264, 160), ld_side_pad=8, side_off=1), dict(kernel=NT_RING)),
                                  ("+4", dict(shape=(130, 264, 160), ld_side_pad=8, side_off=4), dict(kernel=NT_RING))]),
}
EPILOGUE_GATES = {
    # the four-wave kernels' epilogue set: alpha alone, {ReLU, dropout}, {residual, dropout}, the aux mask — every other combination on the
    # eight-wave kernel (one side operand: staged through LDS; none: the wide epilogue)
    "four/epilogue-set": (("set",), [(e, dict(shape=BIG, knobs=V9, epi=e), FOUR) for e in ("plain", "alpha", "relu+drop", "resid", "resid+drop", "aux")] +
                          [(e, dict(shape=BIG, knobs=V9, epi=e), dict(kernel=NT_EIGHT, tile_rows=256, head_rows=0, side_lds=int("resid" in e or "aux" in e),
                                                                       wide_epi=int(not ("resid" in e or "aux" in e))))
                           for e in ("relu+resid", "relu+aux", "alpha+drop", "alpha+relu", "alpha+resid+drop", "alpha+aux", "aux+drop")]),
}
SHAPE_GATES = {
    "four/K": (ALL, [(f"K={K}", dict(shape=(16500, 1032, K), knobs=V9), FOUR if K in (256, 384) else (lambda e: eight(e, True))) for K in (192, 256, 320, 384)]),
    "skinny/K": (ALL, [(f"K={K}", dict(shape=(130, 264, K)), dict(kernel=NT_SKINNY if K in (128, 160, 4096) else NT_RING)) for K in (96, 128, 160, 4096, 4128)]),
    "skinny/M": (ALL, [("M=256", dict(shape=(256, 776, 768)), dict(kernel=NT_SKINNY)), ("M=257", dict(shape=(257, 776, 768)), dict(kernel=NT_RING))]),
    "skinny/N": (ALL, [("N=4096", dict(shape=(128, 4096, 256)), dict(kernel=NT_SKINNY)), ("N=4104", dict(shape=(128, 4104, 256)), dict(kernel=NT_RING))]),
    "chip-filling": (ALL, [("255 tiles", dict(shape=(255 * 256, 256, 256)), dict(kernel=NT_128, head_rows=0)), ("256 tiles", dict(shape=(256 * 256, 256, 256)), dict(kernel=NT_FOUR)),
                           ("257 tiles", dict(shape=(256 * 256 + 3, 256, 256)), dict(kernel=NT_FOUR))]),
    "tail-split": (ALL, [("last round 127", dict(shape=((256 + 127) * 256 - 5, 256, 128), knobs=dict(gemm_nt_four=0, gemm_nt_tile288=0)), dict(kernel=NT_128, head_rows=65536, head_tile=256)),
                         ("last round 128", dict(shape=((256 + 128) * 256 - 5, 256, 128), knobs=dict(gemm_nt_four=0, gemm_nt_tile288=0)), dict(kernel=NT_EIGHT, tile_rows=256, head_rows=0))]),
    # mixed precision declines the four-wave kernel, the 288-row tile and the LDS-staged side operand
    "dtype": (ALL, [("bf16->bf16", dict(shape=BIG), dict(kernel=NT_FOUR)), ("fp32->bf16", dict(shape=BIG, in_t=F32), dict(kernel=NT_128, head_rows=0, side_lds=0)),
                    ("bf16->fp32", dict(shape=BIG, out_t=F32), dict(head_tile=256, head_rows=51 * 256, side_lds=0, head_side_lds=0, head_wide_epi=0))]),
    "dtype/288": (ALL, [("bf16->bf16", dict(shape=(700, 520, 200), knobs=dict(gemm_nt_variant=8)), dict(kernel=NT_EIGHT, tile_rows=288)),
                        ("bf16->fp32", dict(shape=(700, 520, 200), knobs=dict(gemm_nt_variant=8), out_t=F32), dict(kernel=NT_EIGHT, tile_rows=256, side_lds=0, wide_epi=0)),
                        ("fp32->bf16", dict(shape=(700, 520, 200), knobs=dict(gemm_nt_variant=8), in_t=F32), dict(kernel=NT_EIGHT, tile_rows=256, side_lds=0, wide_epi=0))]),
}
GATES = dict(ALIGN_GATES, **SHAPE_GATES, **EPILOGUE_GATES)


@pytest.mark.parametrize("gate,epi", [(g, e) for g in sorted(GATES) for e in GATES[g][0]])
def test_gemm_nt_gate(ops, gate, epi):
    _, sides = GATES[gate]
    plans = {}
    for name, kw, expect in sides:
        kw = dict(kw)
        M, N, K = kw.pop("shape")
        epi = kw.pop("epi", epi)
        expect = expect(epi) if callable(expect) else expect
        pl = run_nt(ops, f"gate {gate} side {name} epilogue {epi} {M}x{N}x{K}", M, N, K, epi, expect=expect, **kw)
        plans[name] = (pl.kernel, pl.tile_rows, pl.head_rows, pl.side_lds, pl.wide_epi)
    assert len(set(plans.values())) > 1, f"gate {gate}: every side ran the same kernel {plans}"


@pytest.mark.parametrize("epi", ["plain", "relu+drop", "resid+drop"])
def test_gemm_nt_norm_gate(ops, epi):
    """LAKO_EPI_NORM_A at K = 1024 (formed in the M <= 256 kernel's fragments) and K = 1056 (refused: the op runs the norm as its own launch)"""
    pl = run_nt(ops, f"norm gate K=1024 {epi}", 130, 264, 1024, epi, expect=dict(kernel=NT_SKINNY_NORM, tile_rows=32, skinny_steps=4), norm=True)
    pl2 = run_nt(ops, f"norm gate K=1056 {epi}", 130, 264, 1056, epi, expect=dict(kernel=NT_REFUSED), norm=True)
    assert pl.kernel != pl2.kernel


@pytest.mark.parametrize("K,split,four", [(1100, 4, 1), (1030, 4, 0), (1000, 0, 1), (1024, 0, 1), (200, 1, 1), (100, 1, 0), (131, 1, 1)])
def test_gemm_tn_gate(ops, K, split, four):
    """the four-wave weight-gradient kernel takes K ranges of at least 128 rows (1 100 rows in four pieces of 320: the last has 140; 1 030: 70),
    whole or not (K % 64 != 0: the last K-step is partial); the eight-wave kernel the rest.  C += Aᵀ·B against fp64, guards around C, NaN
    around A and B."""
    M, N = 264, 520
    A, _ = window(K, M, BF, ld=M + 8, seed=11)
    B, _ = window(K, N, BF, ld=N + 8, seed=12)
    C, Cbuf = window(M, N, F32, ld=N + 4, fill="guard")
    C0 = rnd(M, N, seed=13)
    C.copy_(C0)
    pl = ops.gemm_tn_plan(A, B, C, alpha=0.5, split_k=split)
    assert (pl.big, pl.four) == (1, four), f"K={K} split {split}: planned {pl}"
    ops.gemm_tn(A, B, C, alpha=0.5, split_k=split)
    torch.cuda.synchronize()
    untouched_outside(C, Cbuf, f"gemm_tn K={K} split {split}")
    close(C, C0.double() + 0.5 * (A.double().t() @ B.double()), BF, f"gemm_tn K={K} split {split}", tight=True)


# ---- lako_gemm_nt_mx ------------------------------------------------------------------------------------------------------------------
def mx_operand(ops, rows, K, seed, scale):
    """a bf16 matrix quantised by lako_mx_quantize; the e4m3 bytes then sit in a [rows, K] window (row stride K + 16 bytes, two rows in front
    and behind) of a buffer filled with 0x7F, the e4m3 NaN; the scales stay contiguous (the entry point's layout).  Returns (bytes window,
    scales, the DEQUANTISED values in fp64 — from the very bytes and scale bytes the kernel reads)"""
    x = (rnd(rows, K, seed=seed) * scale).to(BF)
    q = torch.zeros(rows, K, dtype=torch.uint8, device=dev())
    sc = torch.zeros(rows, ops.mx_scale_cols(K), dtype=torch.uint8, device=dev())
    ops.mx_quantize(x, q, sc)
    ld = K + 16
    buf = torch.full(((rows + 4) * ld,), 0x7F, dtype=torch.uint8, device=dev())
    win = torch.as_strided(buf, (rows, K), (ld, 1), 2 * ld)
    win.copy_(q)
    blk = torch.arange(K // 32, device=dev())
    e = sc.view(rows, 4, -1)[:, blk % 4, blk // 4].double()          # block j of a row: scales[row][j % 4][j / 4]
    val = q.view(torch.float8_e4m3fn).double().view(rows, K // 32, 32) * torch.exp2(e - 127.0)[..., None]
    return win, sc, val.view(rows, K)


def run_mx(ops, what, M, N, K, epi, *, expect, knobs=None, ld_side_pad=0, side_off=0):
    kw = dict(EPIS[epi])
    Aq, As, Ad = mx_operand(ops, M, K, 21, 1.5)
    Bq, Bs, Bd = mx_operand(ops, N, K, 22, 0.7)
    C, Cbuf = window(M, N, BF, ld=N + 8, fill="guard")
    resid = aux = None
    if kw.pop("resid", False):
        resid, _ = window(M, N, BF, ld=N + ld_side_pad, off=side_off, seed=3)
        kw["resid"] = resid
    if kw.pop("aux", False):
        aux, _ = window(M, N, BF, ld=N + ld_side_pad, off=side_off, seed=4)
        kw["aux"] = aux
    try:
        for k_, v_ in (knobs or {}).items():
            ops.set_tuning(k_, v_)
        pl = ops.gemm_nt_mx_plan(Aq, As, Bq, Bs, C, **kw)
        ops.gemm_nt_mx(Aq, As, Bq, Bs, C, **kw)
        torch.cuda.synchronize()
    finally:
        for k_ in (knobs or {}):
            ops.set_tuning(k_, DEFAULTS[k_])
    untouched_outside(C, Cbuf, what)
    # the bound of tests/test_kernels_gpu.py::test_gemm_nt_mx for this entry point, against the fp64 product of the dequantised operands
    close(C, reference(Ad, Bd, kw, resid, aux), BF, f"{what} [{pl}]", k=0.5)
    got = {f: getattr(pl, f) for f in expect}
    assert got == expect, f"{what}: planned {pl}, the gate says {expect}"
    return pl


def mx_four(e=None):
    return dict(kernel=NT_MX_FOUR, head_rows=0)


def mx_eight(e):
    return dict(kernel=NT_MX_EIGHT, tile_rows=256, head_rows=0, wide_epi=int(not ("resid" in e or "aux" in e)))


MXBIG = (16500, 1032, 512)
MX_GATES = {
    # whole groups of four K-steps of 128
    "mx/K%512": (ALL, [("K=512", dict(shape=MXBIG), mx_four), ("K=640", dict(shape=(16500, 1032, 640)), mx_eight), ("K=1024", dict(shape=(16500, 1032, 1024)), mx_four)]),
    # "the launch fills the chip"
    "mx/chip-filling": (ALL, [("255 tiles", dict(shape=(255 * 256, 256, 512)), mx_eight), ("256 tiles", dict(shape=(256 * 256 - 9, 256, 512)), mx_four)]),
    "mx/four-off": (ALL, [("gemm_nt_four=1", dict(shape=MXBIG), mx_four), ("gemm_nt_four=0", dict(shape=MXBIG, knobs=dict(gemm_nt_four=0)), mx_eight)]),
    # the epilogue set and the side-operand alignment of the four-wave epilogue (N % 8, ldc % 8 and a 16-byte C are the entry point's own rules)
    "mx/epilogue-set": (("set",), [(e, dict(shape=MXBIG, epi=e), mx_four) for e in ("plain", "alpha", "relu+drop", "resid", "resid+drop", "aux")] +
                        [(e, dict(shape=MXBIG, epi=e), mx_eight) for e in ("relu+resid", "relu+aux", "alpha+drop", "alpha+relu", "alpha+resid+drop", "alpha+aux", "aux+drop")]),
    "mx/ld-side%8": (SIDE, [("%8=0", dict(shape=MXBIG, ld_side_pad=8), mx_four), ("%8=4", dict(shape=MXBIG, ld_side_pad=4), mx_eight)]),
    "mx/side-offset": (SIDE, [("+0", dict(shape=MXBIG, ld_side_pad=8), mx_four), ("+1", dict(shape=MXBIG, ld_side_pad=8, side_off=1), mx_eight),
                              ("+4", dict(shape=MXBIG, ld_side_pad=8, side_off=4), mx_eight)]),
}


@pytest.mark.parametrize("gate,epi", [(g, e) for g in sorted(MX_GATES) for e in MX_GATES[g][0]])
def test_gemm_nt_mx_gate(ops, gate, epi):
    """the MX dispatch on both sides of its gates — K % 512, fills-the-chip, the four-wave epilogue set and its side-operand alignment — in the
    style of test_gemm_nt_mx: operands quantised by lako_mx_quantize, the reference the fp64 product of the dequantised values"""
    _, sides = MX_GATES[gate]
    plans = {}
    for name, kw, expect in sides:
        kw = dict(kw)
        M, N, K = kw.pop("shape")
        e = kw.pop("epi", epi)
        pl = run_mx(ops, f"gate {gate} side {name} epilogue {e} {M}x{N}x{K}", M, N, K, e, expect=expect(e), **kw)
        plans[name] = (pl.kernel, pl.tile_rows, pl.wide_epi)
    assert len({p[0] for p in plans.values()}) > 1, f"gate {gate}: every side ran the same kernel {plans}"


# ---- the fused gated-GELU epilogues ---------------------------------------------------------------------------------------------------
def gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


@pytest.mark.parametrize("drop", [None, (0.1, 99, 110)], ids=["nodrop", "drop"])
@pytest.mark.parametrize("f,K,fused", [(256, 256, True), (192, 256, False), (256, 320, False), (256, 128, False), (384, 384, True)])
def test_gemm_nt_gated_gate(ops, f, K, fused, drop):
    """LAKO_EPI_GATED on both sides of f % 128, K % 128 and K >= 256: inside, one launch writes pre [M, 2f] and h [M, f]; outside the library
    refuses the flag and the two-launch form (product + lako_gated_gelu_fwd, what the engine then runs) computes the same.  pre against the
    fp64 product, h against fp64 gelu_new(a)·b of the bf16 a, b that were stored (test_gated_gpu.py's bound for that kernel), both buffers between guard rows (they are contiguous by
    contract: ldc = 2f), A and B inside NaN."""
    from lako_amd._lib import NT_FOUR_GATED
    M = 300
    A, _ = window(M, K, BF, ld=K + 8, seed=31)
    B, _ = window(2 * f, K, BF, ld=K + 8, seed=32)
    B.mul_(K ** -0.5)
    pre, prebuf = window(M, 2 * f, BF, fill="guard")
    h, hbuf = window(M, f, BF, fill="guard")
    pl = ops.gemm_nt_gated_plan(A, B, pre, h, drop)
    if fused:
        ops.gemm_nt_gated(A, B, pre, h, drop)
    else:
        assert ops.gemm_nt_plan(A, B, pre).kernel != NT_REFUSED
        ops.gemm_nt(A, B, pre)
        ops.gated_gelu_fwd(pre, h, drop)
    torch.cuda.synchronize()
    what = f"gated gate f={f} K={K} {'fused' if fused else 'two launches'} [{pl}]"
    untouched_outside(pre, prebuf, what + " pre")
    untouched_outside(h, hbuf, what + " h")
    close(pre, A.double() @ B.double().t(), BF, what + " pre", tight=True)
    want = gelu_new(pre[:, :f].double()) * pre[:, f:].double()
    if drop:
        idx = torch.arange(M, device=dev(), dtype=torch.int64)[:, None] * f + torch.arange(f, device=dev(), dtype=torch.int64)[None, :]
        keep, scale = keep_mask(drop, idx)
        want = torch.where(keep, want * scale, torch.zeros_like(want))
    # (the bound tests/test_gated_gpu.py states for lako_gated_gelu_fwd in bf16 against fp64)
    assert torch.isfinite(h.float()).all(), what + " h: non-finite"
    torch.testing.assert_close(h.double(), want, atol=2e-2, rtol=1e-2, msg=lambda m: f"{what} h: {m}")
    assert pl.kernel == (NT_FOUR_GATED if fused else NT_REFUSED), f"{what}: f % 128, K % 128 and K >= 256 decide"
