"""Host-side engine of the FiD reader: parameter layout in HBM, workspaces, and the hand-orchestrated
forward / backward / greedy-decode schedules over the op vocabulary of `lako_amd.ops.HipOps`.

What it reproduces (reference file:line; HF5 = transformers 5.15.0 modeling_t5.py):
  * FiDT5.forward + EncoderWrapper.forward reshapes            src/model.py:39-51, 227-234
  * T5Stack / T5Block / attention / FFN / final norm            HF5:663-750, 448-509, 281-369, 83-94, 59-72
  * shift_right, tied LM head × d_model^-0.5, CE(ignore=-100)   HF5:618-637, 1044-1054
  * autograd of all of the above (train_reader.py:73)          written out by hand below
  * greedy generate with KV cache                              src/model.py:54-60, train_reader.py:142-146

Memory plan (sized for 288 GB HBM3E — nothing is recomputed unless `use_checkpoint`):
  P   fp32 master parameters, one flat buffer               G   fp32 gradients, same layout
  W   compute-dtype shadow of P (aliases P in fp32 mode)      WT  per-matrix transposed shadows ([in,out])
so that every GEMM of the step is either NT (X·Wᵀ forward, dY·(Wᵀ)ᵀ for dX) or TN (dYᵀ·X for dW).
q,k,v weights of a layer are adjacent rows of one [3·inner, d] block (one fused QKV GEMM), and the
cross-attention k,v weights of ALL decoder layers form one [L_dec·2·inner, d] block, so the encoder
output [B·N·L, d] is read once for all layers' K/V projections.
Gradient buffer order = the order gradients complete in backward (decoder, cross-K/V, encoder layers
last→first, embedding), so data-parallel buckets can be all-reduced while backward is still running.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field

import numpy as np
import torch

from .config import FiDConfig
from .relpos import bucket_lut

ALIGN = 64  # elements; keeps every block 256-B aligned in fp32 and 128-B aligned in bf16

# generate(num_return_sequences=K): the one-pass cross-attention kernel (lako_xattn_decode_multi) up to this many sequences per question
XDM_MAX_K = 2

# dropout site ids (unique per place a torch.nn.Dropout sits in the reference graph)
S_ENC_EMBED, S_ENC_FINAL, S_DEC_EMBED, S_DEC_FINAL = 1, 2, 3, 4


def _enc_site(i, k):   # k: 0 attn probs, 1 attn out, 2 ffn act, 3 ffn out
    return 100 + i * 8 + k


def _dec_site(i, k):   # k: 0 self probs, 1 self out, 2 cross probs, 3 cross out, 4 ffn act, 5 ffn out
    return 4000 + i * 8 + k


@dataclass
class Block:
    name: str
    shape: tuple
    members: list            # [(plain HF name, row0, nrows)]
    transpose: bool = False  # keep a transposed low-precision copy (GEMM weights)
    off: int = 0
    toff: int = -1

    @property
    def numel(self):
        return int(np.prod(self.shape))


class Mat:
    """One GEMM weight block: p fp32 master [N,K], g fp32 grad, w compute-dtype [N,K], wt compute-dtype [K,N]."""
    __slots__ = ("p", "g", "w", "wt")


class Vec:
    __slots__ = ("p", "g")


def build_layout(cfg: FiDConfig) -> list[Block]:
    d, f, inner, H, nb = cfg.d_model, cfg.d_ff, cfg.inner_dim, cfg.num_heads, cfg.relative_attention_num_buckets
    blocks: list[Block] = []

    def add(name, shape, members, transpose=False):
        blocks.append(Block(name, tuple(shape), members, transpose))

    Ld, Le = cfg.num_decoder_layers, cfg.num_layers

    def wi(p):      # the FFN input projection: [f, d] (v1.0), or the gated form's two matrices as ONE [2f, d] block (rows [0, f) gate)
        if cfg.gated:
            return (2 * f, d), [(p + "DenseReluDense.wi_0.weight", 0, f), (p + "DenseReluDense.wi_1.weight", f, f)]
        return (f, d), [(p + "DenseReluDense.wi.weight", 0, f)]

    if not cfg.tie_word_embeddings:     # its gradient is the first one backward completes
        add("lm_head", (cfg.vocab_size, d), [("lm_head.weight", 0, cfg.vocab_size)], True)
    add("dec.final_ln", (d,), [("decoder.final_layer_norm.weight", 0, d)])
    for i in range(Ld):
        p = f"decoder.block.{i}.layer."
        add(f"dec.{i}.qkv", (3 * inner, d), [(p + f"0.SelfAttention.{n}.weight", j * inner, inner)
                                             for j, n in enumerate("qkv")], True)
        add(f"dec.{i}.o", (d, inner), [(p + "0.SelfAttention.o.weight", 0, d)], True)
        add(f"dec.{i}.ln1", (d,), [(p + "0.layer_norm.weight", 0, d)])
        add(f"dec.{i}.cq", (inner, d), [(p + "1.EncDecAttention.q.weight", 0, inner)], True)
        add(f"dec.{i}.co", (d, inner), [(p + "1.EncDecAttention.o.weight", 0, d)], True)
        add(f"dec.{i}.ln2", (d,), [(p + "1.layer_norm.weight", 0, d)])
        add(f"dec.{i}.wi", *wi(p + "2."), True)
        add(f"dec.{i}.wo", (d, f), [(p + "2.DenseReluDense.wo.weight", 0, d)], True)
        add(f"dec.{i}.ln3", (d,), [(p + "2.layer_norm.weight", 0, d)])
    add("dec.rel", (nb, H), [("decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight", 0, nb)])
    if cfg.legacy_cross_bias:     # transformers 3.0.2: the first cross-attention layer owns a table, every cross-attention adds its bias
        add("dec.xrel", (nb, H), [("decoder.block.0.layer.1.EncDecAttention.relative_attention_bias.weight", 0, nb)])
    kv = []
    for i in range(Ld):
        p = f"decoder.block.{i}.layer.1.EncDecAttention."
        kv += [(p + "k.weight", 2 * i * inner, inner), (p + "v.weight", (2 * i + 1) * inner, inner)]
    add("dec.kv_all", (Ld * 2 * inner, d), kv, True)
    add("enc.final_ln", (d,), [("encoder.final_layer_norm.weight", 0, d)])
    for i in reversed(range(Le)):
        p = f"encoder.block.{i}.layer."
        add(f"enc.{i}.qkv", (3 * inner, d), [(p + f"0.SelfAttention.{n}.weight", j * inner, inner)
                                             for j, n in enumerate("qkv")], True)
        add(f"enc.{i}.o", (d, inner), [(p + "0.SelfAttention.o.weight", 0, d)], True)
        add(f"enc.{i}.ln1", (d,), [(p + "0.layer_norm.weight", 0, d)])
        add(f"enc.{i}.wi", *wi(p + "1."), True)
        add(f"enc.{i}.wo", (d, f), [(p + "1.DenseReluDense.wo.weight", 0, d)], True)
        add(f"enc.{i}.ln2", (d,), [(p + "1.layer_norm.weight", 0, d)])
    add("enc.rel", (nb, H), [("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight", 0, nb)])
    add("shared", (cfg.vocab_size, d), [("shared.weight", 0, cfg.vocab_size)], True)
    off = toff = 0
    for b in blocks:
        b.off = off
        off += -(-b.numel // ALIGN) * ALIGN
        if b.transpose:
            b.toff = toff
            toff += -(-b.numel // ALIGN) * ALIGN
    return blocks


def layout_sizes(blocks):
    last = blocks[-1]
    n = last.off + -(-last.numel // ALIGN) * ALIGN
    tb = [b for b in blocks if b.transpose]
    nt = tb[-1].toff + -(-tb[-1].numel // ALIGN) * ALIGN
    return n, nt


@dataclass
class _Ragged:
    """Unpadded encoder batch: only the valid tokens of the [B·N, L] passages, packed in (passage, position) order."""
    M: int                  # number of valid tokens (rows of every encoder buffer)
    off: torch.Tensor       # int32 [B·N + 1] row offset of each passage
    soff: torch.Tensor      # int32 [B + 1]   row offset of each sample (its N passages are consecutive)
    idx: torch.Tensor       # int64 [M] position of each packed token in the flat [B·N·L] input (None: use pack(), lengths from the host)
    soff_h: list = None     # the sample offsets on the host
    order: torch.Tensor = None   # int32 [B·N] passages by descending length: the processing order of the attention kernels
    first_min: int = 0      # the shortest FIRST passage of a sample (legacy cross-attention bias: see Engine._legacy_layout)


@dataclass
class _XPlan:
    """Key layout of the encoder-state-space cross-attention (csrc/xattn.hip): sample b owns the encoder rows
    [k_h[b], k_h[b+1]) and the score columns [p_h[b], p_h[b] + n_keys(b)) of a [·, ptot] matrix (segments padded to 256)."""
    k_off: torch.Tensor     # int32 [B + 1] device
    p_off: torch.Tensor     # int32 [B + 1] device
    k_h: list = None
    p_h: list = None
    ptot: int = 0
    splits: int = 1         # workgroups sharing the keys of a sample in xattn_context
    p0: int = 0             # first score column of this plan inside the batch's [·, cap] matrices (a chain of samples: its window)
    sub: dict = None        # {n chains: [per-chain _XPlan]} (column offsets relative to the chain's window)


class _GenState:
    """The state of one `generate` call: the `g.*` workspace buffers, all at stable addresses (the decode steps are captured into HIP
    graphs), and the call's choices — mode (the graph cache's key), fused (the one-pass cross-attention kernel), K sequences per question,
    BK decoder rows, ML = max_length, keys = the cross-attention's key descriptor over the stable copies.  Building it enqueues the
    zeroing of the token state and the expansion of the position tables.  Read by Engine._gen_step / _gen_cross / _gen_drive."""

    def __init__(self, eng, ws, bt, enc_out, kv, ML, K, sampled, capture, sparams, bparams=None):
        cfg, ops = eng.cfg, eng.ops
        d, f, inner, H, V, Ld, dk = cfg.d_model, cfg.d_ff, cfg.inner_dim, cfg.num_heads, cfg.vocab_size, cfg.num_decoder_layers, cfg.d_kv
        B, S, BK, xa = bt.B, bt.N * bt.L, bt.B * K, bt.xa
        buf = lambda name, shape, dtype=None: eng._buf(ws, "g." + name, shape, dtype)       # noqa: E731
        self.ws, self.B, self.K, self.BK, self.ML, self.S, self.sampled, self.capture = ws, B, K, BK, ML, S, sampled, capture
        self.sparams, self.enc_out, self.kv, self.xa, self.fused = sparams, enc_out, kv, xa, False
        self.bparams, self.beam = bparams, bparams is not None
        # what changes from call to call is COPIED into workspace buffers (stable addresses: the decode steps are captured into HIP
        # graphs): the samples' key offsets of the unpadded batch, or the key mask of the padded one
        if bt.rag is None:
            stable, self.mode = buf("kmask", (B, S), torch.uint8), "p"
            stable.copy_(bt.mask_u8.view(B, S))
        else:
            stable, self.mode = buf("koff", (B + 1,), torch.int32), "r"
            stable.copy_(bt.rag.soff)
        self.keys = eng._cross_keys(bt, stable)
        if xa is not None:
            # (the K sequences of a question: K·H query rows of its sample — the unfused kernels take any row count, the one-pass
            # kernel carries them as 16-row tiles, several per workgroup: lako_xattn_decode_multi)
            self.mode += "x"
            self.cap = B * (-(-S // 256) * 256)
            self.xoff = buf("xoff", (2, B + 1), torch.int32)
            self.xoff[0].copy_(xa.k_off)
            self.xoff[1].copy_(xa.p_off)
            self.xq = buf("xq", (B, K * H, d))
            self.xs = buf("xs", (K * H, self.cap), torch.float32)      # launched over all `cap` columns: tiles past the batch's
            self.xp = buf("xp", (K * H, self.cap))                      # last key column exit at once
            self.xst = buf("xst", (B, K * H, 2), torch.float32)
            self.xc = buf("xc", (xa.splits, B, K * H, d), torch.float32)
            # scores, softmax and context of a decode step in one pass over the encoder states when the shapes allow
            # (K > 1: only up to XDM_MAX_K sequences per question — above, the unfused kernels' K·H-row MFMA tiles beat the one-pass
            # kernel's row tiles although they read E twice: DESIGN.md §3 "Sampled decoding"; LAKO_XATTN_DECODE=1 forces the one pass)
            xd = os.environ.get("LAKO_XATTN_DECODE")
            self.fused = dk == 64 and getattr(ops, "xattn_decode_ok", lambda *_: False)(H, d) and xd != "0" and (K <= XDM_MAX_K or xd == "1")
            if self.fused:
                # (≈256 workgroups: a workgroup carries as many of a question's sequences as the library's plan gives it row tiles)
                tiles = getattr(ops, "xattn_decode_multi_tiles", lambda d_, k_: min(4, k_))(d, K)
                zd = max(1, min(64, 256 // (B * -(-K // tiles))))
                self.pml, self.pc = buf("xpml", (zd, BK, 16, 2), torch.float32), buf("xpc", (zd, BK, 16, d), torch.float32)
                self.mode += "f"
        if sampled:
            self.mode += f"s{K}"
        if self.beam:
            self.mode += f"b{K}"
        self.seq, self.nxt, self.done = buf("seq", (BK, ML), torch.int64), buf("next", (BK,), torch.int64), buf("done", (BK,), torch.uint8)
        self.score = buf("score", (BK,), torch.float32) if sampled else None
        # finished-row count after every step, mirrored to pinned host memory: the host looks at the count of step t − LAG
        # (an event wait on that step only), so it keeps enqueueing LAG steps ahead of the GPU instead of draining the queue
        # after every token; the LAG extra steps a finished batch may run emit pad for every row and are cut off by the driver
        self.ndone = buf("ndone", (ML,), torch.int32)
        if "g.ndone_host" not in ws or ws["g.ndone_host"].numel() < ML:
            ws["g.ndone_host"] = torch.zeros(ML, dtype=torch.int32, pin_memory=torch.cuda.is_available())
        self.ndone_host = ws["g.ndone_host"]
        for t_ in (self.seq, self.nxt, self.done, self.ndone) + ((self.score,) if sampled else ()):
            ops.zero_(t_)                                  # decoder_start_token_id = pad = 0
        self.rel = eng._rel_table(ws, "g.rel", eng.dec_rel, ML)
        # legacy_cross_bias (_legacy_layout).  Step t's query sits at position t: table index key − t + ML − 1.  With score capture the
        # reference runs ITS cross-attention forward (src/model.py:286-349), which sizes the bias by the step's own query length —
        # 1 under the key / value cache — so every step sees the bias of position 0: one constant per head (src/model.py:323-325)
        self.xrel = eng._rel_table(ws, "g.xrel", eng.dec_xrel, ML) if eng.dec_xrel is not None else None
        # per layer [B, max_length, (q | k | v)]: ONE projection GEMM per step writes the step's q, k and v into row t; q is read
        # back from there, k and v stay as the cache
        if self.beam:
            # beam search: TWO cache sets in one allocation — step t runs on set t & 1 and lako_beam_gather writes the rows, reordered by
            # parent beam, into the other one (one launch for all layers; never in place)
            self.bcache = buf("bcache", (2, Ld, BK, ML, 3 * inner))
            self.cache2 = [[self.bcache[s_, i] for i in range(Ld)] for s_ in range(2)]
            self.cache = self.cache2[0]
        else:
            self.cache = [buf(f"cache.{i}", (BK, ML, 3 * inner)) for i in range(Ld)]
        self.scores = buf("scores", (Ld, B, H, 1, S), torch.float32) if capture else None
        self.h, self.h1, self.h2, self.xn = (buf(n, (BK, d)) for n in ("h", "h1", "h2", "xn"))
        self.c1, self.qc, self.c2 = (buf(n, (BK, inner)) for n in ("c1", "qc", "c2"))
        self.rs, self.st = buf("rs", (BK,), torch.float32), buf("st", (BK, H, 1, 4), torch.float32)
        self.stx = buf("stx", (B, H, K, 4), torch.float32) if K > 1 else self.st      # the cross-attention's: K query positions per sample
        self.a1, self.pre = buf("a1", (BK, f)), (buf("pre", (BK, 2 * f)) if cfg.gated else None)
        self.logits = buf("logits", (BK, V), torch.float32)
        if self.beam:
            # the beams' state (after the buffers every mode has).  Token rows of the running beams (seq2) and of the finished set (fin2)
            # alternate between two sets like the cache: step t reads set t & 1 and writes the other.  run: Σ log-probability of the
            # running beams, best first — [0, −1e9, …] to begin with, so that step 0 expands beam 0 only (HF's initial scores)
            self.seq2, self.fin2 = buf("bseq", (2, BK, ML), torch.int64), buf("bfin", (2, BK, ML), torch.int64)
            self.run, self.parent = buf("brun", (BK,), torch.float32), buf("bparent", (BK,), torch.int32)
            self.cand_acc, self.cand_tok = buf("bcacc", (BK, 2 * K), torch.float32), buf("bctok", (BK, 2 * K), torch.int32)
            self.fin_score, self.fin_raw = buf("bfscore", (BK,), torch.float32), buf("bfraw", (BK,), torch.float32)
            self.fin_len, self.fin_filled = buf("bflen", (BK,), torch.int32), buf("bffilled", (BK,), torch.uint8)
            self.open = buf("bopen", (B,), torch.uint8)
            for t_ in (self.seq2, self.fin2, self.fin_score, self.fin_raw, self.fin_len, self.fin_filled, self.parent):
                ops.zero_(t_)
            self.run.fill_(-1.0e9)
            self.run.view(B, K)[:, 0] = 0.0
            self.open.fill_(1)


@dataclass
class _Ctx:
    """One [B, N, L] batch as the encoder and the cross-attention take it (Engine._batch fills B, N, L, ids, mask_u8, enc_mask, rag, xa and
    enc_ids: all that score and generate need); forward_loss adds the rest: what it leaves behind for backward."""
    B: int = 0
    N: int = 0
    L: int = 0
    T: int = 0
    p: float = 0.0
    seed: int = 0
    ids: torch.Tensor = None
    mask_u8: torch.Tensor = None
    enc_mask: torch.Tensor = None      # the ENCODER's key mask: mask_u8, or None when the batch has no padding at all (Engine._enc_mask)
    labels: torch.Tensor = None
    ckpt: bool = False
    rag: object = None      # _Ragged: the encoder ran on the valid tokens only
    xa: object = None       # _XPlan: cross-attention ran in the encoder-state space
    chains: list = None     # the decoder's sample chains (_dec_chains)
    cross: tuple = None     # (kb, kt, ckw): the cross-attention's key descriptor the chains were built from (_cross_keys)
    enc_ids: torch.Tensor = None   # the encoder's token ids: all [B·N·L], or the valid ones when rag is set
    ws: dict = field(default_factory=dict)


# dW += dYᵀ·X — weight → the forward's saved input X ("e." + name + slot); the decoder: (dY's full-batch scratch, X), "d." + name + layer
_ENC_DW_X = dict(wo="a1", wi="xn2", o="ctx", qkv="xn1")
_DEC_DW = dict(wo=("dy.ffn", "a1"), wi=("dpre", "xn3"), co=("dy.c", "cctx"), cq=("dqc", "xn2"), o=("dy", "ctx"), qkv=("dqkv", "xn1"))


@dataclass
class _BwdPlan:
    """What one Engine.backward call does where it has a choice, decided once at the top of the call (Engine._bwd_plan)"""
    p: float             # the step's dropout rate
    fused: bool          # every RMSNorm backward also writes dropout_bwd(dx) for the branch that consumes dx next; LAKO_FUSE_DROP=0: dropout_apply launches (A/B)
    defer: bool          # the decoder's weight gradients in grouped launches after the chains; LAKO_DEC_DEFER_DW=0: inside the chain, on its rows (A/B)
    hb_defer: bool       # the decoder's head-batched Wk / Wv gradient products in ONE launch after the chains (_dec_bwd)
    grp: int             # encoder layers per grouped weight-gradient launch
    enc_split: int       # the K-splits of that launch
    fuse_gated: bool     # LAKO_FUSE_GATED (_fuse_gated)
    one: int             # split_k of a one-split product that may be a gradient's first writer: −2 overwrites, −1 adds


class Engine:
    def __init__(self, cfg: FiDConfig, ops, device, dtype=torch.bfloat16, seed: int = 0, fp8: bool | None = None):
        if cfg.d_kv not in (32, 64, 128):
            raise ValueError(f"d_kv={cfg.d_kv} unsupported by the attention kernels (32, 64 or 128)")
        if cfg.d_model % 8 or cfg.d_ff % 8 or cfg.vocab_size % 8:
            raise ValueError("d_model, d_ff and vocab_size must be multiples of 8")
        self.cfg, self.ops, self.device, self.dtype = cfg, ops, torch.device(device), dtype
        # LAKO_DETERMINISTIC=1 (read once by the library; RefOps has no such mode — its torch sums are what they are): bit-identical steps
        self.det = bool(getattr(ops, "det", False))
        self.blocks = build_layout(cfg)
        self.n_param, self.n_trans = layout_sizes(self.blocks)
        dev = self.device
        self.P = torch.zeros(self.n_param, dtype=torch.float32, device=dev)
        self.G = torch.zeros(self.n_param, dtype=torch.float32, device=dev)
        self._g_fresh = True         # G is all zeros (construction / zero_grad) and no backward has added to it yet
        self.W = self.P if dtype == torch.float32 else torch.zeros(self.n_param, dtype=dtype, device=dev)
        self.WT = torch.zeros(self.n_trans, dtype=dtype, device=dev)
        self.opt_m = None   # AdamW moments, allocated by the optimizer on first use
        self.opt_v = None
        self.gnorm_sq = torch.zeros(1, dtype=torch.float32, device=dev)
        self.by_name = {b.name: b for b in self.blocks}
        self._bind()
        self.seed_base = int(seed)
        self.step_count = 0
        self.use_checkpoint = False
        self._ws_cache: dict = {}
        self._tr_table = None
        self._rag_cache: dict = {}
        self._xplan_cache: dict = {}
        self.xattn_active = False
        self._all_valid = False
        self._row_cap: dict = {}     # {rows of the current unpadded batch: padded row count}
        self._lut_cache: dict = {}
        self.ctx: _Ctx | None = None
        self.grad_hook = None    # callable(lo, hi): gradients G[lo:hi] are final (data-parallel overlap)
        self.grad_ranges_early = True   # the hook wants every range as early as possible (overlap mode); False: only that all are done
        self.shadows_stale = True
        # MX block-scaled fp8 forward GEMMs (BASELINE config 5): the encoder's QKV and FFN-in projections and the cross-K/V
        # projection — the GEMMs whose A operand is a norm output — multiply e4m3 operands with E8M0 block scales on
        # v_mfma_scale_f32_16x16x128_f8f6f4; everything else (attention, norms, the other GEMMs, the whole backward) stays bf16
        self.fp8 = bool(int(os.environ.get("LAKO_FP8", "0"))) if fp8 is None else bool(fp8)
        if self.fp8 and (dtype != torch.bfloat16 or not hasattr(ops, "gemm_nt_mx")):
            raise ValueError("fp8 GEMMs need the bf16 engine on the HIP op set")
        if self.fp8 and cfg.gated:
            raise ValueError("fp8 GEMMs (LAKO_FP8=1) are not implemented for the gated-GELU feed-forward (T5 v1.1 / Flan-T5)")
        if self.fp8 and cfg.d_kv != 64:
            raise ValueError(f"fp8 GEMMs (LAKO_FP8=1) are not implemented for d_kv={cfg.d_kv} (T5-3B); they need d_kv 64")
        self._w8: dict = {}      # block name → (e4m3 bytes [N, K], scales) of the weight shadow

    # ------------------------------------------------------------------------------------------
    # parameter views
    # ------------------------------------------------------------------------------------------
    def _view(self, flat, b: Block, transposed=False):
        if transposed:
            return flat[b.toff:b.toff + b.numel].view(b.shape[1], b.shape[0])
        return flat[b.off:b.off + b.numel].view(b.shape)

    def _mat(self, name) -> Mat:
        b = self.by_name[name]
        m = Mat()
        m.p, m.g, m.w = self._view(self.P, b), self._view(self.G, b), self._view(self.W, b)
        m.wt = self._view(self.WT, b, True)
        return m

    def _vec(self, name) -> Vec:
        b = self.by_name[name]
        v = Vec()
        v.p, v.g = self._view(self.P, b), self._view(self.G, b)
        return v

    def _bind(self):
        cfg = self.cfg
        self.shared = self._mat("shared")
        # the LM head: `shared` × d_model^-0.5 (tied, v1.0), or its own matrix with alpha 1 (untied, v1.1)
        self.lm_head = self.shared if cfg.tie_word_embeddings else self._mat("lm_head")
        self.head_alpha = cfg.d_model ** -0.5 if cfg.tie_word_embeddings else 1.0
        self.kv_all = self._mat("dec.kv_all")
        self.enc_final, self.dec_final = self._vec("enc.final_ln"), self._vec("dec.final_ln")
        self.enc_rel, self.dec_rel = self._vec("enc.rel"), self._vec("dec.rel")
        self.dec_xrel = self._vec("dec.xrel") if cfg.legacy_cross_bias else None
        self.enc, self.dec = [], []
        for i in range(cfg.num_layers):
            self.enc.append(dict(qkv=self._mat(f"enc.{i}.qkv"), o=self._mat(f"enc.{i}.o"), ln1=self._vec(f"enc.{i}.ln1"),
                                 wi=self._mat(f"enc.{i}.wi"), wo=self._mat(f"enc.{i}.wo"), ln2=self._vec(f"enc.{i}.ln2")))
        for i in range(cfg.num_decoder_layers):
            self.dec.append(dict(qkv=self._mat(f"dec.{i}.qkv"), o=self._mat(f"dec.{i}.o"), ln1=self._vec(f"dec.{i}.ln1"),
                                 cq=self._mat(f"dec.{i}.cq"), co=self._mat(f"dec.{i}.co"), ln2=self._vec(f"dec.{i}.ln2"),
                                 wi=self._mat(f"dec.{i}.wi"), wo=self._mat(f"dec.{i}.wo"), ln3=self._vec(f"dec.{i}.ln3")))

    def named_param_views(self, flat=None):
        """plain HF-T5 name → view into `flat` (default: the fp32 master)."""
        flat = self.P if flat is None else flat
        out = {}
        for b in self.blocks:
            v = self._view(flat, b)
            for name, r0, nr in b.members:
                out[name] = v[r0:r0 + nr] if len(b.shape) == 2 else v
        return out

    def refresh_transposed(self, from_shadow=False):
        """WT ← transposed compute-dtype copies of every GEMM weight in P, one launch over a static table.  from_shadow: the
        compute-dtype shadow W is current (the fused optimizer step has just written it) — transpose IT: identical values
        (W = bf16(P) element for element) from half the bytes (446 instead of 892 MB at T5-base)."""
        if self._tr_table is None:
            mats = [b for b in self.blocks if b.transpose]
            desc, prefix, total = [], [], 0
            for b in mats:
                desc += [b.off, b.toff, b.shape[0], b.shape[1]]
                prefix.append(total)
                total += -(-b.shape[0] // 64) * -(-b.shape[1] // 64)
            self._tr_table = (torch.tensor(desc, dtype=torch.int64, device=self.device),
                              torch.tensor(prefix, dtype=torch.int32, device=self.device), len(mats), total)
        src = self.W if (from_shadow and self.W is not self.P and self.W.dtype == self.WT.dtype) else self.P
        self.ops.transpose_cast_batched(src, self.WT, *self._tr_table)

    def refresh_shadows(self):
        """Re-derive the compute-dtype copies (W, WT) from the fp32 master after it changed."""
        if self.W is not self.P:
            self.ops.cast(self.P, self.W)
        self.refresh_transposed()
        if self.fp8:
            self.refresh_fp8()
        self.shadows_stale = False

    def refresh_after_step(self):
        """After the fused optimizer step (which wrote P and the compute-dtype shadow W in one pass): every DERIVED copy of the
        weights — the transposed shadows and, in fp8 mode, the e4m3 + block-scale shadows the forward GEMMs multiply with."""
        self.refresh_transposed(from_shadow=True)
        if self.fp8:
            self.refresh_fp8()
        self.shadows_stale = False

    def _fp8_blocks(self):
        names = [f"enc.{i}.{m}" for i in range(self.cfg.num_layers) for m in ("qkv", "wi")] + ["dec.kv_all"]
        return [self.by_name[n] for n in names if self.by_name[n].shape[1] % 128 == 0]

    def refresh_fp8(self):
        """e4m3 + block-scale shadows of the weights that take part in fp8 GEMMs, from the bf16 shadow W"""
        for b in self._fp8_blocks():
            if b.name not in self._w8:
                n, k = b.shape
                self._w8[b.name] = (torch.empty(n, k, dtype=torch.uint8, device=self.device),      # (scale padding bytes stay 0)
                                    torch.zeros(n, self.ops.mx_scale_cols(k), dtype=torch.uint8, device=self.device))
            q, sc = self._w8[b.name]
            self.ops.mx_quantize(self._view(self.W, b), q, sc)

    def _norm_gemm_w(self, ws, h, lnp, xn, rs, eps, name, w, out, **epi):
        """xn = RMSNorm(h); out = epilogue(xn · wᵀ).  With an fp8 shadow of this weight the norm also emits the e4m3 bytes and block scales of xn
        (lako_rmsnorm_fwd_mx: one pass instead of norm + quantiser — the same bytes), which the MX product consumes."""
        w8 = self._w8.get(name) if self.fp8 else None
        M, K = h.shape
        if w8 is None or K % 128 != 0 or not hasattr(self.ops, "rmsnorm_fwd_mx") or os.environ.get("LAKO_FP8_FUSED_NORM", "1") == "0":
            self.ops.rmsnorm_fwd(h, lnp, xn, rs, eps)
            return self._gemm_w(ws, xn, name, w, out, **epi)
        xq, xs = self._q8_buffers(ws, M, K)
        self.ops.rmsnorm_fwd_mx(h, lnp, xn, rs, eps, xq, xs)
        self.ops.gemm_nt_mx(xq, xs, w8[0], w8[1], out, **epi)

    def _q8_buffers(self, ws, M, K):
        xq = self._buf(ws, f"q8.{K}", (M, K), torch.uint8)
        fresh = ws.get(f"^s8.{K}")
        xs = self._buf(ws, f"s8.{K}", (M, self.ops.mx_scale_cols(K)), torch.uint8)
        if ws[f"^s8.{K}"] is not fresh:
            self.ops.zero_(ws[f"^s8.{K}"])      # the quantiser writes ⌈K/128⌉ of the KSP scale columns: the padding stays 0
        return xq, xs

    def _gemm_w(self, ws, x, name, w, out, **epi):
        """out = epilogue(x · wᵀ): on the block-scaled fp8 matrix cores when this weight has an fp8 shadow (x is quantised into
        workspace scratch first), else the bf16 GEMM"""
        w8 = self._w8.get(name) if self.fp8 else None
        if w8 is None:
            return self.ops.gemm_nt(x, w, out, **epi)
        M, K = x.shape
        xq, xs = self._q8_buffers(ws, M, K)
        self.ops.mx_quantize(x, xq, xs)
        self.ops.gemm_nt_mx(xq, xs, w8[0], w8[1], out, **epi)

    def _fuse_gated(self, x, w, f, fuse=None):
        """the encoder's gated-GELU products where the library's fused epilogues take the shape: "four" (LAKO_FUSE_GATED=0, the default):
        the four-wave product + the standalone kernel, or "fused" (=1): both in the product's epilogue — bit-identical, measured slower
        (0.895 against 0.721 ms per encoder layer at v1_1-base).  None (the decoder's skinny products, other shapes, the CPU
        test double): the library's plain product + the standalone kernel.  `fuse`: the switch as the caller read it (_BwdPlan)."""
        if not hasattr(self.ops, "gemm_nt_gated") or not self.ops.gated_fused_ok(x, w, f):
            return None
        if fuse is None:
            fuse = os.environ.get("LAKO_FUSE_GATED", "0") == "1"
        return "fused" if fuse else "four"

    def zero_grad(self):
        self.ops.zero_(self.G)
        self._g_fresh = True

    # ------------------------------------------------------------------------------------------
    # helpers
    # ------------------------------------------------------------------------------------------
    def _lut(self, qlen, klen, bidirectional):
        key = (qlen, klen, bidirectional)
        if key not in self._lut_cache:
            lut = bucket_lut(qlen, klen, bidirectional, self.cfg.relative_attention_num_buckets,
                             self.cfg.relative_attention_max_distance)
            self._lut_cache[key] = torch.from_numpy(lut).to(self.device)
        return self._lut_cache[key]

    def _legacy_layout(self, rag, T):
        """`legacy_cross_bias` (transformers 3.0.2, src/model.py:323-329): every cross-attention adds
        `bias[h, t, s] = table[bucket(s − t)][h]` with the DECODER's one-sided buckets (`bidirectional = not is_decoder`), s the position of
        the key in the concatenated [n_passages · text_maxlength] sequence.  Keys at or after the query position all share bucket 0, so
        the bias differs from a per-head constant only for the first t keys of the FIRST passage — which is why it is an ordinary
        relative table for the projected kernels (index key − query + T − 1 into `[H, 2T − 1]`, indices past the end clamped onto
        "distance >= 0") as long as a key's index IS its position there: always on the padded layout; on the packed layout when every
        sample's first passage has at least T − 1 valid tokens (the packed index of a later passage's token is smaller than its
        position).  Returns the layout to use: `rag`, or None (padded) when a first passage is too short."""
        if rag is not None and self.cfg.legacy_cross_bias and rag.first_min < T - 1:
            return None
        return rag

    def _buf(self, ws, name, shape, dtype=None):
        """Workspace tensor `name` of this shape.  The backing allocation only grows: a request with fewer ROWS (the
        unpadded encoder: the number of valid tokens changes from batch to batch) is a prefix view of it."""
        shape = tuple(shape)
        t = ws.get(name)
        if t is not None and t.shape == shape and t.dtype == (dtype or self.dtype):      # the same request as last time (the common case)
            return t
        base = ws.get("^" + name)
        if base is None or tuple(base.shape[1:]) != shape[1:] or base.shape[0] < shape[0] or base.dtype != (dtype or self.dtype):
            # token-row buffers of an unpadded batch are allocated at the padded row count once, so that a later batch with
            # more valid tokens never reallocates the workspace in the middle of training
            rows = max(shape[0], self._row_cap.get(shape[0], 0))
            base = torch.empty((rows,) + shape[1:], dtype=dtype or self.dtype, device=self.device)
            ws["^" + name] = base
        t = base if base.shape[0] == shape[0] else base[:shape[0]]
        ws[name] = t
        return t

    def _tn_scratch(self, nbytes):
        """grow-only device scratch for the weight-gradient launches whose K-splits meet through partial tiles (lako_gemm_tn_grouped).
        OFF by default (LAKO_TN_SLABS=1 switches it on): measured +0.6 ms per step against the float atomics (round 4,
        profiles/r04s_tn_slab_reduction.txt) — the atomics are fire-and-forget, the last arriver's slab reads and read-modify-write are
        a serial tail.  What it buys is bit-reproducible encoder weight gradients."""
        if os.environ.get("LAKO_TN_SLABS", "0") != "1" and not self.det:      # (LAKO_DETERMINISTIC=1 takes it: DESIGN.md §4)
            return None
        t = getattr(self, "_tn_ws", None)
        if t is None or t.numel() < nbytes:
            t = self._tn_ws = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        return t

    def _embed_bwd(self, ids, dout, drop):
        """shared-embedding gradient += scatter of dropout_bwd(dout).  LAKO_DETERMINISTIC=1: rows of one id are added in position order by
        one wave (the sort is index plumbing, torch's stable argsort on the same stream) instead of by float atomics in arrival order."""
        if self.det:
            ids = ids.reshape(-1)
            self.ops.embed_bwd_ordered(ids, torch.argsort(ids, stable=True), dout, self.shared.g, drop)
        else:
            self.ops.embed_bwd(ids, dout, self.shared.g, drop)

    def _workspace(self, key):
        return self._ws_cache.setdefault(key, {})

    def _heads(self, t2d, rows_b, rows_t, col0):
        """[rows_b*rows_t, ld] buffer → [B, T, H, dk] view of columns [col0, col0 + inner)."""
        H, dk = self.cfg.num_heads, self.cfg.d_kv
        if t2d.shape[0] != rows_b * rows_t or t2d.stride(1) != 1 or col0 + H * dk > t2d.shape[1]:
            raise ValueError(f"_heads: {tuple(t2d.shape)} is not [{rows_b}*{rows_t}, >= {col0 + H * dk}] row-major")
        s0 = t2d.stride(0)          # (one view op instead of view → slice → unflatten: this runs ≈290 times per training step)
        return t2d.as_strided((rows_b, rows_t, H, dk), (rows_t * s0, s0, dk, 1), t2d.storage_offset() + col0)

    # ------------------------------------------------------------------------------------------
    # forward
    # ------------------------------------------------------------------------------------------
    def _enc_layer_fwd(self, ws, i, j, h, h_out, BN, L, mask_u8, rel, dr, rag=None):
        """One encoder block (HF5:448-509): RMSNorm → fused QKV → attention → O+residual → RMSNorm → FFN+residual.
        Intermediates are written to the workspace slot `j` (per layer when everything is kept, slot 0 when the
        layer is recomputed in backward or nothing is kept)."""
        cfg, ops = self.cfg, self.ops
        d, f, inner, H, eps = cfg.d_model, cfg.d_ff, cfg.inner_dim, cfg.num_heads, cfg.layer_norm_epsilon
        Me, lw = (rag.M if rag is not None else BN * L), self.enc[i]
        xn1 = self._buf(ws, f"e.xn1.{j}", (Me, d))
        qkv = self._buf(ws, f"e.qkv.{j}", (Me, 3 * inner))
        self._norm_gemm_w(ws, h, lw["ln1"].p, xn1, self._buf(ws, f"e.rs1.{j}", (Me,), torch.float32), eps, f"enc.{i}.qkv", lw["qkv"].w, qkv)
        ctx = self._buf(ws, f"e.ctx.{j}", (Me, inner))
        hb, ht, akw = self._enc_attn_layout(rag, BN, L, mask_u8)
        ops.attn_fwd(self._heads(qkv, hb, ht, 0), self._heads(qkv, hb, ht, inner), self._heads(qkv, hb, ht, 2 * inner),
                     self._heads(ctx, hb, ht, 0), self._buf(ws, f"e.st.{j}", (BN, H, L, 4), torch.float32),
                     rel_bias=rel, rel_off=L - 1, drop=dr(_enc_site(i, 0)), **akw)
        h1 = self._buf(ws, f"e.h1.{j}", (Me, d))
        ops.gemm_nt(ctx, lw["o"].w, h1, resid=h, drop=dr(_enc_site(i, 1)))
        xn2 = self._buf(ws, f"e.xn2.{j}", (Me, d))
        a1 = self._buf(ws, f"e.a1.{j}", (Me, f))
        if cfg.gated:      # pre = [a | b] (kept for backward), a1 = dropout(gelu_new(a) ⊙ b)
            pre = self._buf(ws, f"e.pre.{j}", (Me, 2 * f))
            rs2 = self._buf(ws, f"e.rs2.{j}", (Me,), torch.float32)
            fz = self._fuse_gated(xn2, lw["wi"].w, f)
            if fz:      # both outputs from the product's epilogue (fused), or the same product + the standalone kernel (bit-identical)
                ops.rmsnorm_fwd(h1, lw["ln2"].p, xn2, rs2, eps)
                if fz == "fused":
                    ops.gemm_nt_gated(xn2, lw["wi"].w, pre, a1, dr(_enc_site(i, 2)))
                else:
                    ops.gemm_nt_four(xn2, lw["wi"].w, pre)
                    ops.gated_gelu_fwd(pre, a1, dr(_enc_site(i, 2)))
            else:
                self._norm_gemm_w(ws, h1, lw["ln2"].p, xn2, rs2, eps, f"enc.{i}.wi", lw["wi"].w, pre)
                ops.gated_gelu_fwd(pre, a1, dr(_enc_site(i, 2)))
        else:
            self._norm_gemm_w(ws, h1, lw["ln2"].p, xn2, self._buf(ws, f"e.rs2.{j}", (Me,), torch.float32), eps, f"enc.{i}.wi", lw["wi"].w, a1,
                              relu=True, drop=dr(_enc_site(i, 2)))
        if h_out is not None:
            ops.gemm_nt(a1, lw["wo"].w, h_out, resid=h1, drop=dr(_enc_site(i, 3)))

    @staticmethod
    def _enc_attn_layout(rag, BN, L, mask_u8):
        """(batch, time) of the [·, ·, H, dk] head views of the token-major buffers + the attention kwargs: padded
        [BN, L] with a key mask, or ONE packed run of rows with per-passage offsets."""
        if rag is None:      # (mask_u8 None: a batch without any padding — no mask to apply, and the encoder's fast attention kernels take it)
            return BN, L, (dict(key_mask=mask_u8) if mask_u8 is not None else {})
        return 1, rag.M, dict(q_off=rag.off, k_off=rag.off, max_q=L, max_k=L, order=rag.order)

    def _enc_mask(self, rag, mask_u8):
        """The key mask of the encoder's self-attention on the padded layout — None when the batch has no padded position at all (what
        _ragged_batch found: every passage at text_maxlength, e.g. `bench.py --all-valid`): a mask of ones adds nothing, and without one
        the padded [B·N, L] batch is a set of exact-length sequences for the fast encoder kernels (csrc/attn_enc.hip) instead of the generic
        masked ones.  LAKO_ENC_ALLVALID_MASK=1 keeps the mask (A/B)."""
        if rag is None and self._all_valid and os.environ.get("LAKO_ENC_ALLVALID_MASK", "0") != "1":
            return None
        return mask_u8

    def _encode(self, ws, ids_flat, mask_u8, BN, L, p, seed, save, rag=None, want_kv=True):
        """save: True  — keep every intermediate of every layer (training; 288 GB of HBM make this the default);
                 "ckpt" — keep only each block's input and recompute the block in backward (`set_checkpoint(True)`,
                          the reference's CheckpointWrapper, src/model.py:237-283);
                 False — keep nothing (generate)."""
        cfg, ops = self.cfg, self.ops
        d, H = cfg.d_model, cfg.num_heads
        Me, Le, eps = (rag.M if rag is not None else BN * L), cfg.num_layers, cfg.layer_norm_epsilon
        dr = (lambda site: (p, seed, site)) if p > 0 else (lambda site: None)
        ix = (lambda i: i) if save is True else (lambda i: 0)
        hx = (lambda i: i) if save else (lambda i: i % 2)
        ops.embed_fwd(ids_flat, self.shared.w, self._buf(ws, f"e.h{hx(0)}", (Me, d)), dr(S_ENC_EMBED))
        rel = self._buf(ws, "e.rel", (H, 2 * L - 1), torch.float32)
        ops.relpos_expand(self.enc_rel.p, self._lut(L, L, True), rel)
        for i in range(Le):
            self._enc_layer_fwd(ws, i, ix(i), ws[f"e.h{hx(i)}"], self._buf(ws, f"e.h{hx(i + 1)}", (Me, d)), BN, L,
                                mask_u8, rel, dr, rag)
        enc_out = self._buf(ws, "e.out", (Me, d))
        ops.rmsnorm_fwd(ws[f"e.h{hx(Le)}"], self.enc_final.p, enc_out, self._buf(ws, "e.rsf", (Me,), torch.float32),
                        eps, dr(S_ENC_FINAL))
        if not want_kv:      # cross-attention in the encoder-state space: the keys and values ARE enc_out
            return enc_out, None
        # K/V projections of every decoder layer's cross-attention in ONE GEMM (reads enc_out once)
        kv = self._buf(ws, "e.kv", (Me, self.kv_all.w.shape[0]))
        self._gemm_w(ws, enc_out, "dec.kv_all", self.kv_all.w, kv)
        return enc_out, kv

    def _ragged_batch(self, attention_mask, B, N, L, lengths=None):
        """Padded positions never influence the loss, the gradients or the decoded tokens: they are masked as keys in the
        encoder's self-attention and in the decoder's cross-attention, and nothing else reads them.  When the mask has the
        tokenizer's form (valid tokens first, then padding) the encoder therefore runs on the valid tokens only — a quarter
        fewer rows in every GEMM / norm / attention at the OKVQA-like lengths of the benchmark.  Returns None (padded path)
        for LAKO_UNPAD=0, masks with holes, a sample without any valid token, or when nothing is padded.

        `lengths` (host int tensor [B, N] or [B·N]): the number of valid tokens of every passage as the collator that
        built the mask knows it (the mask is born on the host: src/data.py:88-104 pads to text_maxlength) — asserts the
        prefix form, so no device→host sync is needed: offsets are built on the host, uploaded from pinned memory, and the
        packed-row index is expanded on the device.  Without it the lengths are read back from the mask (one host sync per
        new mask tensor; repeated batches hit a cache keyed by the tensor's identity and version)."""
        self._all_valid = False
        if os.environ.get("LAKO_UNPAD", "1") == "0":
            return None
        dev = attention_mask.device
        if lengths is not None:
            lens_h = torch.as_tensor(lengths, dtype=torch.int32, device="cpu").reshape(-1)
            if lens_h.numel() != B * N:
                raise ValueError(f"passage_lengths has {lens_h.numel()} entries for {B * N} passages")
            if int(lens_h.min()) < 0 or int(lens_h.max()) > L:
                raise ValueError("passage_lengths out of range [0, L]")
            M = int(lens_h.sum())
            self._all_valid = M == B * N * L
            self._check_lengths(attention_mask, lens_h, B, N, L)
            if int(lens_h.view(B, N).sum(1).min()) <= 0 or M >= B * N * L:
                return None
            off = torch.zeros(B * N + 1, dtype=torch.int32)
            torch.cumsum(lens_h, 0, out=off[1:])
            pin = (lambda t: t.pin_memory()) if dev.type == "cuda" else (lambda t: t)
            off_d = pin(off).to(dev, non_blocking=True)
            idx = None      # (the packed token ids come from ONE lako_pack_ids launch over the offsets: no packed-row index on this path)
            # passages sorted by descending length: the order the encoder-attention workgroups take them in (load balance only:
            # long items first, every persistent workgroup one passage of each length class — measured with pre-sorted lengths:
            # attention −0.24 ms per step)
            order = torch.argsort(lens_h, descending=True, stable=True).to(torch.int32)
            order_d = pin(order).to(dev, non_blocking=True) if os.environ.get("LAKO_ATTN_ORDER", "1") != "0" else None
            return _Ragged(M=M, off=off_d, soff=off_d[::N].contiguous(), idx=idx, soff_h=off[::N].tolist(), order=order_d,
                           first_min=int(lens_h.view(B, N)[:, 0].min()))
        key = (attention_mask.data_ptr(), attention_mask._version, B, N, L)
        hit = self._rag_cache.get(key)
        if hit is not None:
            self._all_valid = hit[2]
            return hit[0]
        m = attention_mask.reshape(B * N, L).bool()
        lens = m.sum(1, dtype=torch.int32)
        prefix = (m == (torch.arange(L, device=m.device)[None, :] < lens[:, None])).all()
        host = torch.cat([lens, prefix.to(torch.int32)[None]]).cpu()
        lens_h, ok = host[:-1], bool(host[-1])
        per_sample = lens_h.view(B, N).sum(1)
        rag = None
        if ok and int(per_sample.min()) > 0 and int(lens_h.sum()) < B * N * L:
            off = torch.zeros(B * N + 1, dtype=torch.int32)
            off[1:] = torch.cumsum(lens_h, 0)
            rag = _Ragged(M=int(off[-1]), off=off.to(dev), soff=off[::N].contiguous().to(dev),
                          idx=m.reshape(-1).nonzero().reshape(-1), soff_h=off[::N].tolist(),
                          order=torch.argsort(lens_h, descending=True, stable=True).to(torch.int32).to(dev)
                          if os.environ.get("LAKO_ATTN_ORDER", "1") != "0" else None,
                          first_min=int(lens_h.view(B, N)[:, 0].min()))
        self._all_valid = ok and int(lens_h.sum()) == B * N * L
        if len(self._rag_cache) >= 16:
            self._rag_cache.clear()
        self._rag_cache[key] = (rag, attention_mask, self._all_valid)   # holding the tensor keeps (data_ptr, version) unambiguous
        return rag

    def _packed_ids(self, ws, ids_flat, rag, L):
        """token ids of the valid positions in packed order"""
        if rag.idx is not None:
            return ids_flat[rag.idx]
        out = self._buf(ws, "e.ids", (rag.M,), torch.int64)
        self.ops.pack_ids(ids_flat, rag.off, out, L)
        return out

    def _batch(self, ws, input_ids, attention_mask, lengths, rows_q=None, T=None, keep_padding=False, p=0.0, seed=0, save=False):
        """The prologue of forward_loss, score and generate: flat ids and uint8 mask, the unpadded layout when the mask allows it, the
        cross-attention plan, the encoder pass (p, seed, save: _encode) → (batch, enc_out, kv).  Sets `_row_cap` and `xattn_active`.
        rows_q: query rows per sample of the encoder-state cross-attention (_xattn_plan); None: no such plan, projected K / V.
        T: the decoder length `_legacy_layout` compares the first passages with; None: the caller has no legacy bias.
        keep_padding: the padded layout whatever the mask looks like (generate's captured scores are laid out per padded position);
        nothing is then known about the mask's padding: `_all_valid` is cleared and _enc_mask keeps the mask."""
        B, N, L = input_ids.shape
        ids = input_ids.reshape(-1).contiguous()
        mask_u8 = attention_mask.reshape(B * N, L).to(torch.uint8).contiguous()
        rag = None if keep_padding else self._ragged_batch(attention_mask, B, N, L, lengths)
        if keep_padding:
            self._all_valid = False
        elif T is not None:
            rag = self._legacy_layout(rag, T)
        self._row_cap = {rag.M: B * N * L} if rag is not None else {}
        enc_ids = ids if rag is None else self._packed_ids(ws, ids, rag, L)
        xa = self._xattn_plan(rag, B, N, L, rows_q) if rows_q is not None else None
        self.xattn_active = xa is not None         # (bench.py / tests: which formulation the last call ran)
        bt = _Ctx(B=B, N=N, L=L, ids=ids, mask_u8=mask_u8, enc_mask=self._enc_mask(rag, mask_u8), rag=rag, xa=xa, enc_ids=enc_ids, ws=ws)
        return (bt,) + self._encode(ws, enc_ids, bt.enc_mask, B * N, L, p, seed, save=save, rag=rag, want_kv=xa is None)

    @staticmethod
    def _cross_keys(bt, stable=None):
        """(kb, kt, ckw): how the cross-attention finds a sample's keys — [B, N·L] with the padding mask, or ONE run of packed valid tokens
        with the samples' row offsets.  `stable`: generate's workspace copy of the mask / the offsets (captured graphs read that address)."""
        S = bt.N * bt.L
        if bt.rag is None:
            return bt.B, S, dict(key_mask=bt.mask_u8.view(bt.B, S) if stable is None else stable)
        return 1, bt.rag.M, dict(k_off=bt.rag.soff if stable is None else stable, max_k=S)

    def _check_lengths(self, attention_mask, lens_h, B, N, L):
        """`passage_lengths` must describe the mask (valid tokens first, exactly lengths[b, n] of them): anything else would pack the
        wrong tokens without a sign.  Every batch's mask is therefore compared with the uploaded lengths ON THE DEVICE (round 6: on by
        default; LAKO_CHECK_LENGTHS=0 switches it off), and the one-byte verdict travels to pinned host memory behind an event — the
        training path still never waits for the device: a verdict is looked at only once its event has completed (`query()`), i.e. a
        mismatch raises a step or two late instead of never; `check_lengths_now()` waits for everything outstanding (end of an epoch,
        tests).  Cost: five small launches on [B·N, L] booleans, ≈ 0.03 ms per step at config 2 (profiles/r06j_length_check_cost.txt)."""
        if os.environ.get("LAKO_CHECK_LENGTHS", "1") == "0":
            return
        self._poll_lengths(block=False)
        dev = attention_mask.device
        m = attention_mask.reshape(B * N, L).bool()
        if dev.type != "cuda":                # the CPU test double: nothing to overlap with — compare at once
            want = torch.arange(L)[None, :] < lens_h[:, None]
            if bool((m != want).any()):
                self._lengths_error()
            return
        ar = self._len_arange.get(L) if hasattr(self, "_len_arange") else None
        if ar is None or ar.device != dev:
            if not hasattr(self, "_len_arange"):
                self._len_arange, self._len_pending = {}, []
            ar = self._len_arange[L] = torch.arange(L, device=dev, dtype=torch.int32)[None, :]
        want = ar < lens_h.pin_memory().to(dev, non_blocking=True)[:, None]
        flag = torch.empty(1, dtype=torch.bool).pin_memory()
        flag.copy_((m != want).any().reshape(1), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._len_pending.append((ev, flag))

    @staticmethod
    def _lengths_error():
        raise ValueError("passage_lengths do not describe the attention mask of an earlier batch: the mask must be valid-tokens-first with "
                         "exactly lengths[b, n] valid tokens per passage (LAKO_CHECK_LENGTHS=0 switches the check off)")

    def _poll_lengths(self, block):
        pend = getattr(self, "_len_pending", None)
        while pend and (block or pend[0][0].query()):
            ev, flag = pend.pop(0)
            if block:
                ev.synchronize()
            if bool(flag[0]):                 # (pinned host memory: no device access)
                pend.clear()
                self._lengths_error()

    def check_lengths_now(self):
        """wait for every outstanding mask-vs-lengths verdict and raise on a mismatch"""
        self._poll_lengths(block=True)

    def _xattn_plan(self, rag, B, N, L, rows_q):
        """The cross-attention runs in the encoder-state space (csrc/xattn.hip: no K/V projection of the N·L encoder states, the
        per-head projections act on the T·H query rows instead) whenever every sample's keys are a contiguous run of encoder rows:
        the unpadded batch, or a batch without any padding.  Masks with holes / LAKO_UNPAD=0 / LAKO_XATTN=0 / shapes the kernels
        do not take (fp32 engine, d_kv != 64, d_model % 128) keep the projected formulation (lako_attn_fwd with a key mask)."""
        cfg = self.cfg
        ok = getattr(self.ops, "xattn_ok", None)
        if cfg.legacy_cross_bias:      # the bias is an argument of the projected kernels only (_legacy_layout)
            return None
        if os.environ.get("LAKO_XATTN", "1") == "0" or ok is None or not ok(self.dtype, cfg.d_kv, cfg.d_model) or B > 512:
            return None
        if rag is not None:
            k_h = list(rag.soff_h)
        elif self._all_valid:
            k_h = [b * N * L for b in range(B + 1)]
        else:
            return None
        key = (tuple(k_h), rows_q)
        hit = self._xplan_cache.get(key)
        if hit is not None:
            return hit
        p_h = [0]
        for b in range(B):
            p_h.append(p_h[-1] + -(-(k_h[b + 1] - k_h[b]) // 256) * 256)
        host = torch.tensor([k_h, p_h], dtype=torch.int32)
        if self.device.type == "cuda":
            host = host.pin_memory()
        dev = host.to(self.device, non_blocking=True)
        # one 512-thread workgroup per CU: split a sample's keys until ≈256 workgroups are in flight
        per = max(1, cfg.d_model // 128) * B * -(-rows_q // 128)
        splits = int(os.environ.get("LAKO_XATTN_SPLITS", "0")) or max(1, min(8, 256 // per))
        plan = _XPlan(k_off=dev[0], p_off=dev[1], k_h=k_h, p_h=p_h, ptot=p_h[-1], splits=splits)
        if len(self._xplan_cache) >= 8:
            self._xplan_cache.clear()
        self._xplan_cache[key] = plan
        return plan

    def _xattn_subplans(self, xa, n, B):
        """The plan cut into n chains of samples: chain c owns the score columns [p_h[b0], p_h[b1]) — its kernels get views of that
        window and column offsets relative to it (the kernels launch one workgroup per 256 columns from column 0 of what they are
        given) — and the absolute key offsets of its samples.  Cached with the plan."""
        if xa.sub is None:
            xa.sub = {}
        if n not in xa.sub:
            bounds = [(c * B // n, (c + 1) * B // n) for c in range(n)]
            rel = [[p - xa.p_h[b0] for p in xa.p_h[b0:b1 + 1]] for b0, b1 in bounds]
            host = torch.tensor([v for r in rel for v in r], dtype=torch.int32)
            if self.device.type == "cuda":
                host = host.pin_memory()
            dev = host.to(self.device, non_blocking=True)
            plans, at = [], 0
            for (b0, b1), r in zip(bounds, rel):
                plans.append(_XPlan(k_off=xa.k_off[b0:b1 + 1], p_off=dev[at:at + len(r)], k_h=xa.k_h[b0:b1 + 1], p_h=r, ptot=r[-1],
                                    splits=xa.splits, p0=xa.p_h[b0]))
                at += len(r)
            xa.sub[n] = plans
        return xa.sub[n]

    def _xw(self, i, which, transposed=False):
        """Per-head views of decoder layer i's cross-attention K ("k") or V ("v") projection inside the kv_all block:
        [H, dk, d] of the weight, or (transposed) [H, d, dk] of its transposed shadow — the B operands of headbatch_nt."""
        inner, H, dk = self.cfg.inner_dim, self.cfg.num_heads, self.cfg.d_kv
        r0 = (2 * i + (which == "v")) * inner
        if transposed:
            return self.kv_all.wt[:, r0:r0 + inner].unflatten(1, (H, dk)).permute(1, 0, 2)
        return self.kv_all.w[r0:r0 + inner].unflatten(0, (H, dk))

    def _xg(self, i, which):
        inner, H, dk = self.cfg.inner_dim, self.cfg.num_heads, self.cfg.d_kv
        r0 = (2 * i + (which == "v")) * inner
        return self.kv_all.g[r0:r0 + inner].unflatten(0, (H, dk))

    def _xattn_buffers(self, ws, B, N, L, T, Ld, Z, keep=True):
        """Workspace of the encoder-state-space cross-attention, sized for the padded batch (the column count of a batch's score
        matrices, xa.ptot, is a prefix of the allocation).  Per decoder layer l and R = T·H query rows per sample:
          dq [B, Ld·2R, d]   rows l·2R … : dC' (written in backward), rows l·2R + R … : Q'          — B operand of the dE product
          ps [Ld·2R, cap]    rows l·2R … : dropout(P),               rows l·2R + R … : dS (backward) — A operand of the dE product
          s  [Ld, R, cap] fp32 raw scores, st [Ld, B, R, 2] softmax statistics, c [Ld, Z, B, R, d] fp32 C' = P·E in Z key-split slabs
        keep=False (no backward follows: `score`): one layer's worth, which every layer reuses (`slot`)."""
        cfg = self.cfg
        R, d = T * cfg.num_heads, cfg.d_model
        cap = B * (-(-(N * L) // 256) * 256)
        if not keep:
            Ld = 1
        xb = dict(R=R, cap=cap, rows=B * N * L,
                  dq=self._buf(ws, "x.dq", (B, Ld * 2 * R, d)),
                  ps=self._buf(ws, "x.ps", (Ld * 2 * R, cap)),
                  s=self._buf(ws, "x.s", (Ld, R, cap), torch.float32),
                  st=self._buf(ws, "x.st", (Ld, B, R, 2), torch.float32),
                  c=self._buf(ws, "x.c", (Ld, Z, B, R, d), torch.float32))
        if not keep:
            xb["slot"] = 0
        return xb

    def _xattn_fwd(self, xb, xa, i, qc, enc_out, c2, B, T, max_keys, drop):
        """Cross-attention of decoder layer i in the encoder-state space (see csrc/xattn.hip): qc [B·T, inner] → c2 [B·T, inner]"""
        ops, H, dk, R = self.ops, self.cfg.num_heads, self.cfg.d_kv, xb["R"]
        j = xb.get("slot", i)        # the layer's buffers (_xattn_buffers: one shared set when nothing is kept)
        qp = xb["dq"][:, (2 * j + 1) * R:(2 * j + 2) * R]
        ops.headbatch_nt(qc.view(B, T, H, dk), self._xw(i, "k", transposed=True), qp.unflatten(1, (T, H)))
        s = xb["s"][j][:, xa.p0:xa.p0 + xa.ptot]
        ops.xattn_scores(qp, enc_out, xa.k_off, xa.p_off, xa.ptot, s)
        pr = xb["ps"][2 * j * R:(2 * j + 1) * R, xa.p0:xa.p0 + xa.ptot]
        ops.xattn_softmax_fwd(s, xb["st"][j], pr, xa.k_off, xa.p_off, T, H, max_keys, drop)
        ops.xattn_context(pr, enc_out, xa.k_off, xa.p_off, xb["c"][j])
        ops.headbatch_nt(xb["c"][j].unflatten(2, (T, H)), self._xw(i, "v"), c2.view(B, T, H, dk))

    def _xattn_bwd(self, xb, xa, tmp, i, qc, enc_out, dctx, dqc, B, T, max_keys, drop, b0=0, B_all=None, hb=None):
        """Backward of _xattn_fwd: dctx [B·T, inner] → dqc [B·T, inner], the layer's Wk / Wv gradients, and the rows (dC', dS) the
        encoder-state gradient is assembled from after the last layer (_xattn_denc)."""
        ops, H, dk, R, d = self.ops, self.cfg.num_heads, self.cfg.d_kv, xb["R"], self.cfg.d_model
        dcp = xb["dq"][:, 2 * i * R:(2 * i + 1) * R]
        d4 = dctx.view(B, T, H, dk)
        ops.headbatch_nt(d4, self._xw(i, "v", transposed=True), dcp.unflatten(1, (T, H)))
        # (`hb`: list collecting the layers' Wk / Wv gradient products for ONE launch after the last layer — their operands then live in
        # per-layer buffers: the caller's dctx, and dqp below)
        if hb is not None:
            hb.append((d4, xb["c"][i].unflatten(2, (T, H)), self._xg(i, "v")))
        else:
            ops.headbatch_tn(d4, xb["c"][i].unflatten(2, (T, H)), self._xg(i, "v"))
        dp = self._buf(tmp, "x.dp", (R, xb["cap"]), torch.float32)[:, xa.p0:xa.p0 + xa.ptot]
        ops.xattn_scores(dcp, enc_out, xa.k_off, xa.p_off, xa.ptot, dp)
        ds = xb["ps"][(2 * i + 1) * R:(2 * i + 2) * R, xa.p0:xa.p0 + xa.ptot]
        ops.xattn_softmax_bwd(xb["s"][i][:, xa.p0:xa.p0 + xa.ptot], dp, xb["st"][i], ds, xa.k_off, xa.p_off, T, H, max_keys, drop)
        dqp = self._buf(tmp, f"x.dqp.{i}" if hb is not None else "x.dqp", (xa.splits, B_all or B, R, d), torch.float32)[:, b0:b0 + B]      # (a chain: its samples' slabs)
        ops.xattn_context(ds, enc_out, xa.k_off, xa.p_off, dqp)
        ops.headbatch_nt(dqp.unflatten(2, (T, H)), self._xw(i, "k"), dqc.view(B, T, H, dk))
        if hb is not None:
            hb.append((qc.view(B, T, H, dk), dqp.unflatten(2, (T, H)), self._xg(i, "k")))
        else:
            ops.headbatch_tn(qc.view(B, T, H, dk), dqp.unflatten(2, (T, H)), self._xg(i, "k"))

    def _xattn_denc(self, xb, xa, tmp, Me, dxe):
        """dE[s, :] = Σ_layers Σ_r P[r, s]·dC'[r, :] + dS[r, s]·Q'[r, :] — per sample one [keys, d] = psᵀ·dq product with
        K = layers·2R (weight-gradient form: both operands K-major), fp32, then rounded once to the compute dtype."""
        ops, d = self.ops, self.cfg.d_model
        de = self._buf(tmp, "x.de", (xb["rows"] + 8, d), torch.float32)[:Me + 8]    # sized for the padded batch
        items = []
        for b in range(len(xa.k_h) - 1):
            nk = xa.k_h[b + 1] - xa.k_h[b]
            n8 = -(-nk // 8) * 8      # the operand loads want a multiple of 8 columns (the score matrices' zero padding); only the
            items.append((xb["ps"][:, xa.p_h[b]:xa.p_h[b] + n8], xb["dq"][b], de[xa.k_h[b]:xa.k_h[b] + n8], 1.0, nk))   # sample's nk rows are written
        # one contributor per element, every element of dE written exactly once by plain stores (split_k −2: no zero fill, no atomics)
        # — dE feeds the encoder's bf16 backward: independent of the order workgroups finish in
        ops.gemm_tn_grouped(items, split_k=-2)
        if dxe.dtype == torch.float32:
            dxe.copy_(de[:Me])
        else:
            ops.cast(de[:Me].view(-1), dxe.view(-1))

    # ------------------------------------------------------------------------------------------
    # the decoder as independent chains of samples
    # ------------------------------------------------------------------------------------------
    def _dec_chains(self, B, T, p, seed, xa, xb, rag, kb, kt, ckw, n=None):
        """The decoder of a training step is ≈400 launches on B·T ≈ 128 rows: each kernel is a few µs of launch ramp, dependent
        round trips and drain, and on one stream they run strictly one after the other.  Nothing in the decoder couples two samples
        (self- and cross-attention are per sample, everything else per row), so the batch can be cut into `LAKO_DEC_CHAINS` runs of
        samples whose layer-by-layer chains are enqueued on separate HIP streams; the weight gradients — the one place where the samples
        meet — are summed over ALL rows in grouped launches after the last layer.  MEASURED NEGATIVE (round 4, profiles/r04e_decoder_chains.txt):
        1 chain 40.95 ms per step, 2 chains 42.0, 4 chains 47.8 — kernels of two queues do overlap (each takes 1.5 × as long) but the
        pair is no faster than the two in sequence, and every extra launch costs its boundary.  Default 1 = the single-stream schedule;
        the split stays selectable and tested (results: forward values unchanged bit for bit — row-wise kernels; each chain draws its
        dropout masks from its own seed).
        `n` = 1 with p = 0: the whole batch as ONE chain without dropout whatever the environment says (`score`: T = its C·T rows per sample)."""
        n = n or (max(1, min(int(os.environ.get("LAKO_DEC_CHAINS", "1")), B // 2)) if B >= 4 else 1)
        chains = []
        for c in range(n):
            b0, b1 = c * B // n, (c + 1) * B // n
            seed_c = (seed ^ (0x9E3779B9 * c)) & 0xFFFFFFFF
            ch = dict(c=c, b0=b0, b1=b1, B=b1 - b0, r0=b0 * T, r1=b1 * T, xa=None, xb=None, kv_b=kb, kv_t=kt, kv_r=None, ckw=ckw,
                      dr=(lambda site, sd=seed_c: (p, sd, site)) if p > 0 else (lambda site: None))
            if xa is not None:
                ch["xa"] = self._xattn_subplans(xa, n, B)[c] if n > 1 else xa
                ch["xb"] = dict(xb, dq=xb["dq"][b0:b1], st=xb["st"][:, b0:b1], c=xb["c"][:, :, b0:b1]) if n > 1 else xb
            elif n > 1:
                if rag is None:        # padded keys: the chain's samples are rows [b0·S, b1·S) of the projected K / V
                    ch.update(kv_b=b1 - b0, kv_r=(b0 * kt, b1 * kt), ckw=dict(ckw, key_mask=ckw["key_mask"][b0:b1]))
                else:                  # packed keys: the whole buffer, the chain's sample offsets
                    ch["ckw"] = dict(ckw, k_off=ckw["k_off"][b0:b1 + 1])
            chains.append(ch)
        return chains

    def _run_chains(self, chains, n_layers, layer_fn, reverse=False):
        """layer_fn(i, chain) for every layer and chain — on one stream when there is one chain (or no GPU: the CPU test double), else
        chain c on its own side stream: forked from the current stream before the first layer, joined after the last."""
        order = range(n_layers - 1, -1, -1) if reverse else range(n_layers)
        if len(chains) == 1 or self.device.type != "cuda":
            for i in order:
                for ch in chains:
                    layer_fn(i, ch)
            return
        if getattr(self, "_chain_streams", None) is None or len(self._chain_streams) < len(chains):
            self._chain_streams = [torch.cuda.Stream(self.device) for _ in chains]
            self._chain_events = [torch.cuda.Event() for _ in range(len(chains) + 1)]
        main = torch.cuda.current_stream(self.device)
        fork = self._chain_events[-1]
        fork.record(main)
        for st in self._chain_streams[:len(chains)]:
            st.wait_event(fork)
        for i in order:
            for ch in chains:
                with torch.cuda.stream(self._chain_streams[ch["c"]]):
                    layer_fn(i, ch)
        for ch in chains:
            ev = self._chain_events[ch["c"]]
            ev.record(self._chain_streams[ch["c"]])
            main.wait_event(ev)

    def _rows(self, ws, name, ch, shape, dtype=None):
        """rows [r0, r1) of the [B·T, …] workspace tensor `name` (allocated at full size)"""
        return self._buf(ws, name, shape, dtype)[ch["r0"]:ch["r1"]]

    def _cross_kv(self, kv, ch, col0):
        """[kb, kt, H, dk] head view of the projected cross-attention K or V (columns col0 …) for the chain's samples"""
        if ch["kv_r"] is not None:
            kv = kv[ch["kv_r"][0]:ch["kv_r"][1]]
        return self._heads(kv, ch["kv_b"], ch["kv_t"] if ch["kv_r"] is None else kv.shape[0] // ch["kv_b"], col0)

    def _rel_table(self, ws, name, vec, T):
        """the decoder-side relative-position table `vec` expanded to [H, 2T − 1] in the workspace buffer `name`"""
        rel = self._buf(ws, name, (self.cfg.num_heads, 2 * T - 1), torch.float32)
        self.ops.relpos_expand(vec.p, self._lut(T, T, False), rel)
        return rel

    def _dec_setup(self, ws, labels, T, Tx, bt, xa, keep=True, rel=None):
        """The workspace of one teacher-forced decoder pass over labels [rows, T] (−100 = ignore): the shifted ids, the relative-position
        table (`rel`: the one an earlier pass of the call built), every layer's hidden states, the final norm's output and statistics, the
        encoder-state cross-attention's buffers for Tx query positions per sample (keep: _xattn_buffers).  → (rel, xb, dec_out)"""
        Md, d, Ld = labels.numel(), self.cfg.d_model, self.cfg.num_decoder_layers
        self.ops.shift_right(labels, self._buf(ws, "d.ids", tuple(labels.shape), torch.int64))
        if rel is None:
            rel = self._rel_table(ws, "d.rel", self.dec_rel, T)
        xb = self._xattn_buffers(ws, bt.B, bt.N, bt.L, Tx, Ld, xa.splits, keep=keep) if xa is not None else None
        for i in range(Ld + 1):
            self._buf(ws, f"d.h{i}", (Md, d))
        dec_out = self._buf(ws, "d.out", (Md, d))
        self._buf(ws, "d.rsf", (Md,), torch.float32)
        return rel, xb, dec_out

    def _dec_norm_gemm(self, h, ln, xn, rs, w, out, **epi):
        """xn = RMSNorm(h)·ln, rs its statistics; out = epilogue(xn · wᵀ).  The norm is formed inside the projection's kernel where the
        library can (LAKO_EPI_NORM_A, the decoder's B·T <= 256 rows): one launch, xn and rs still written.  LAKO_DEC_FUSE_NORM=0: two."""
        eps = self.cfg.layer_norm_epsilon
        if os.environ.get("LAKO_DEC_FUSE_NORM", "1") != "0":
            self.ops.gemm_nt(h, w, out, norm=(ln, eps, xn, rs), **epi)
        else:
            self.ops.rmsnorm_fwd(h, ln, xn, rs, eps)
            self.ops.gemm_nt(xn, w, out, **epi)

    def _dec_layer_fwd(self, ws, i, ch, enc_out, kv, rel, T, S, Tx=None):
        """One decoder block (HF5:448-509) on the rows of one chain: RMSNorm → QKV → causal self-attention → O + residual → RMSNorm →
        cross-attention query → cross-attention → O + residual → RMSNorm → FFN + residual.
        `Tx` (default T): the query rows a sample has in the CROSS-attention — `score` hands every sample C sequences of T tokens: the
        self-attention sees Tx / T causal sequences of length T per sample, the cross-attention (no structure over its query rows)
        one run of Tx = C·T rows per sample."""
        cfg, ops, lw, dr = self.cfg, self.ops, self.dec[i], ch["dr"]
        d, f, inner, H, eps = cfg.d_model, cfg.d_ff, cfg.inner_dim, cfg.num_heads, cfg.layer_norm_epsilon
        Bc, Ld = ch["B"], cfg.num_decoder_layers
        Bs, sb0, sb1 = Bc, ch["b0"], ch["b1"]      # the self-attention's sequences: the chain's samples …
        if Tx is None:
            Tx = T
        elif Tx != T:                               # … or Tx / T sequences per sample
            Bs, sb0, sb1 = Bc * (Tx // T), ch["b0"] * (Tx // T), ch["b1"] * (Tx // T)
        Md = ws[f"d.h{i}"].shape[0]
        R = lambda name, cols, dt=None: self._rows(ws, name, ch, (Md, cols) if cols else (Md,), dt)       # noqa: E731
        h = ws[f"d.h{i}"][ch["r0"]:ch["r1"]]
        if i == 0:
            ops.embed_fwd(ws["d.ids"].view(-1)[ch["r0"]:ch["r1"]], self.shared.w, h, dr(S_DEC_EMBED))
        xn1, qkv = R(f"d.xn1.{i}", d), R(f"d.qkv.{i}", 3 * inner)
        self._dec_norm_gemm(h, lw["ln1"].p, xn1, R(f"d.rs1.{i}", 0, torch.float32), lw["qkv"].w, qkv)
        c1 = R(f"d.ctx.{i}", inner)
        st = self._buf(ws, f"d.st.{i}", (Md // T, H, T, 4), torch.float32)[sb0:sb1]
        ops.attn_fwd(self._heads(qkv, Bs, T, 0), self._heads(qkv, Bs, T, inner), self._heads(qkv, Bs, T, 2 * inner),
                     self._heads(c1, Bs, T, 0), st, rel_bias=rel, rel_off=T - 1, causal=True, drop=dr(_dec_site(i, 0)))
        h1 = R(f"d.h1.{i}", d)
        ops.gemm_nt(c1, lw["o"].w, h1, resid=h, drop=dr(_dec_site(i, 1)))
        xn2, qc = R(f"d.xn2.{i}", d), R(f"d.qc.{i}", inner)
        self._dec_norm_gemm(h1, lw["ln2"].p, xn2, R(f"d.rs2.{i}", 0, torch.float32), lw["cq"].w, qc)
        c2 = R(f"d.cctx.{i}", inner)
        if ch["xa"] is not None:
            self._xattn_fwd(ch["xb"], ch["xa"], i, qc, enc_out, c2, Bc, Tx, S, dr(_dec_site(i, 2)))
        else:
            cst = self._buf(ws, f"d.cst.{i}", (Md // Tx, H, Tx, 4), torch.float32)[ch["b0"]:ch["b1"]]
            ops.attn_fwd(self._heads(qc, Bc, Tx, 0), self._cross_kv(kv, ch, 2 * i * inner), self._cross_kv(kv, ch, (2 * i + 1) * inner),
                         self._heads(c2, Bc, Tx, 0), cst, drop=dr(_dec_site(i, 2)), **ch["ckw"])
        h2 = R(f"d.h2.{i}", d)
        ops.gemm_nt(c2, lw["co"].w, h2, resid=h1, drop=dr(_dec_site(i, 3)))
        xn3, a1 = R(f"d.xn3.{i}", d), R(f"d.a1.{i}", f)
        # gated: the product writes pre = [a | b] (kept for backward), then a1 = dropout(gelu_new(a) ⊙ b)
        out1, act = (R(f"d.pre.{i}", 2 * f), {}) if cfg.gated else (a1, dict(relu=True, drop=dr(_dec_site(i, 4))))
        self._dec_norm_gemm(h2, lw["ln3"].p, xn3, R(f"d.rs3.{i}", 0, torch.float32), lw["wi"].w, out1, **act)
        if cfg.gated:
            ops.gated_gelu_fwd(out1, a1, dr(_dec_site(i, 4)))
        h_out = ws[f"d.h{i + 1}"][ch["r0"]:ch["r1"]]
        ops.gemm_nt(a1, lw["wo"].w, h_out, resid=h2, drop=dr(_dec_site(i, 5)))
        if i == Ld - 1:
            ops.rmsnorm_fwd(h_out, self.dec_final.p, ws["d.out"][ch["r0"]:ch["r1"]], ws["d.rsf"][ch["r0"]:ch["r1"]], eps, dr(S_DEC_FINAL))

    def _dec_layer_bwd(self, ws, tmp, i, ch, dh_all, bw, drel, dxrel, dkv, T, S, dw_all, hb_all):
        """Backward of _dec_layer_fwd on the rows of one chain; dh_all [B·T, d] holds the gradient wrt the block's output on entry and
        wrt its input on exit.  With dropout on (bw.defer), the six weight-gradient problems of the block are NOT launched here: their
        operands (the dropped residual-branch gradients, dpre, dqc, dqkv) live in per-layer scratch, and the chain that handles the
        batch's last rows appends the FULL-batch problems to `dw_all` — one grouped launch over all rows and layers after the chains
        have joined; `hb_all` (bw.hb_defer) collects the Wk / Wv gradient products likewise.  `dxrel`: legacy_cross_bias's gradient table."""
        cfg, ops, lw, dr = self.cfg, self.ops, self.dec[i], ch["dr"]
        d, f, inner, Bc, r0, r1 = cfg.d_model, cfg.d_ff, cfg.inner_dim, ch["B"], ch["r0"], ch["r1"]
        Md, Ld, p, fused = dh_all.shape[0], cfg.num_decoder_layers, bw.p, bw.fused
        sl = lambda t: t[r0:r1]                                                                   # noqa: E731
        R = lambda name, cols: self._rows(tmp, name, ch, (Md, cols))                              # noqa: E731
        per = f".{i}" if bw.defer else ""      # (operands of the deferred launches: scratch per layer)
        dh = sl(dh_all)
        if i == Ld - 1:          # final norm of the decoder: dout (gradient wrt the normed, dropped output) → dh
            ops.rmsnorm_bwd(sl(tmp["d.dxn"]), sl(ws[f"d.h{Ld}"]), self.dec_final.p, sl(ws["d.rsf"]), None, dh, self.dec_final.g, dr(S_DEC_FINAL),
                            **self._nxt((R(f"d.dy.ffn.{i}", d), dr(_dec_site(i, 5))) if fused else None))
        # dW[w] += dyᵀ·x: on the chain's rows now, or deferred (the full-batch problems: at the end of this function)
        wgrad = (lambda w, dy: None) if bw.defer else (lambda w, dy: ops.gemm_tn(dy, sl(ws[f"d.{_DEC_DW[w][1]}.{i}"]), lw[w].g))
        # ---- FFN: the decoder's skinny products never take the library's gated route, whatever their row count ----------------
        dy_f = R(f"d.dy.ffn.{i}", d) if p > 0 else None
        dxn = R("d.dxn", d)
        if cfg.gated:
            R("d.dha", f)      # (allocated ahead of dpre, as it always was here)
        self._ffn_bwd(lw, dh, dy_f, sl(ws[f"d.a1.{i}"]), sl(ws[f"d.pre.{i}"]) if cfg.gated else None, bw, dr(_dec_site(i, 4)),
                      dr(_dec_site(i, 5)), R, ("d.dpre" + per, "d.dha"), dxn, wgrad, library_gated=False)
        dy_c = R(f"d.dy.c.{i}", d) if p > 0 else None
        ops.rmsnorm_bwd(dxn, sl(ws[f"d.h2.{i}"]), lw["ln3"].p, sl(ws[f"d.rs3.{i}"]), dh, dh, lw["ln3"].g,
                        **self._nxt((dy_c, dr(_dec_site(i, 3))) if fused else None))
        # ---- cross-attention ---------------------------------------------------------------------
        dy = self._branch_grad(dh, dy_c, dr(_dec_site(i, 3)), fused)
        wgrad("co", dy)
        dctx = R(f"d.xdctx.{i}" if hb_all is not None else "d.dctx", inner)      # (hb_all: only with the encoder-state cross-attention)
        ops.gemm_nt(dy, lw["co"].wt, dctx)
        dqc, qc = R("d.dqc" + per, inner), sl(ws[f"d.qc.{i}"])
        if ch["xa"] is not None:
            self._xattn_bwd(ch["xb"], ch["xa"], tmp, i, qc, ws["e.out"], dctx, dqc, Bc, T, S, dr(_dec_site(i, 2)), b0=ch["b0"],
                            B_all=Md // T, hb=hb_all)
        else:
            kv, c2, ckw = ws["e.kv"], sl(ws[f"d.cctx.{i}"]), (ch["ckw"] if dxrel is None else dict(ch["ckw"], drel=dxrel))
            ops.attn_bwd(self._heads(qc, Bc, T, 0), self._cross_kv(kv, ch, 2 * i * inner), self._cross_kv(kv, ch, (2 * i + 1) * inner),
                         self._heads(c2, Bc, T, 0), self._heads(dctx, Bc, T, 0), ws[f"d.cst.{i}"][ch["b0"]:ch["b1"]],
                         self._heads(dqc, Bc, T, 0), self._cross_kv(dkv, ch, 2 * i * inner), self._cross_kv(dkv, ch, (2 * i + 1) * inner),
                         drop=dr(_dec_site(i, 2)), **ckw)
        wgrad("cq", dqc)
        ops.gemm_nt(dqc, lw["cq"].wt, dxn)
        dy_s = R(f"d.dy.{i}", d) if p > 0 else None
        ops.rmsnorm_bwd(dxn, sl(ws[f"d.h1.{i}"]), lw["ln2"].p, sl(ws[f"d.rs2.{i}"]), dh, dh, lw["ln2"].g,
                        **self._nxt((dy_s, dr(_dec_site(i, 1))) if fused else None))
        # ---- causal self-attention ---------------------------------------------------------------
        dy = self._branch_grad(dh, dy_s, dr(_dec_site(i, 1)), fused)
        qkv, c1 = sl(ws[f"d.qkv.{i}"]), sl(ws[f"d.ctx.{i}"])
        wgrad("o", dy)
        dctx = R("d.dctx", inner)      # (not the cross-attention's buffer: that one may be an operand of the deferred Wv-gradient launch)
        ops.gemm_nt(dy, lw["o"].wt, dctx)
        dqkv = R("d.dqkv" + per, 3 * inner)
        ops.attn_bwd(self._heads(qkv, Bc, T, 0), self._heads(qkv, Bc, T, inner), self._heads(qkv, Bc, T, 2 * inner),
                     self._heads(c1, Bc, T, 0), self._heads(dctx, Bc, T, 0), ws[f"d.st.{i}"][ch["b0"]:ch["b1"]],
                     self._heads(dqkv, Bc, T, 0), self._heads(dqkv, Bc, T, inner), self._heads(dqkv, Bc, T, 2 * inner),
                     rel_bias=ws["d.rel"], drel=drel, rel_off=T - 1, causal=True, drop=dr(_dec_site(i, 0)))
        wgrad("qkv", dqkv)
        ops.gemm_nt(dqkv, lw["qkv"].wt, dxn)
        nxt = (R(f"d.dy.ffn.{i - 1}", d), dr(_dec_site(i - 1, 5))) if fused and i > 0 else None
        ops.rmsnorm_bwd(dxn, sl(ws[f"d.h{i}"]), lw["ln1"].p, sl(ws[f"d.rs1.{i}"]), dh, dh, lw["ln1"].g, **self._nxt(nxt))
        if bw.defer and r1 == Md:      # (this chain's call is the one that registers the full-batch weight-gradient problems)
            dw_all += [(tmp[f"d.{dy}.{i}"], ws[f"d.{x}.{i}"], lw[w].g, 1.0) for w, (dy, x) in _DEC_DW.items()]
        if i == 0:
            self._embed_bwd(ws["d.ids"].view(-1)[r0:r1], dh, dr(S_DEC_EMBED))

    def forward_loss(self, input_ids, attention_mask, labels, training: bool, lengths=None):
        """input_ids/attention_mask [B,N,L], labels [B,T] (−100 = ignore) → (loss 0-d fp32, logits [B,T,V] fp32).
        `lengths`: optional host-side valid lengths per passage (see _ragged_batch)."""
        if self.shadows_stale:
            self.refresh_shadows()
        cfg, ops = self.cfg, self.ops
        B, N, L = input_ids.shape
        T = labels.shape[1]
        H, V, S, Ld = cfg.num_heads, cfg.vocab_size, N * L, cfg.num_decoder_layers
        p = float(cfg.dropout_rate) if training else 0.0
        seed = (self.seed_base * 1000003 + self.step_count) & 0xFFFFFFFF
        ws = self._workspace(("train", B, N, L, T))
        ckpt = bool(self.use_checkpoint and training)
        ctx, enc_out, kv = self._batch(ws, input_ids, attention_mask, lengths, rows_q=T * H, T=T, p=p, seed=seed, save="ckpt" if ckpt else True)
        ctx.T, ctx.p, ctx.seed, ctx.ckpt, ctx.labels = T, p, seed, ckpt, labels.reshape(-1).contiguous()
        # ---- decoder ------------------------------------------------------------------------
        kb, kt, ckw = self._cross_keys(ctx)
        rel, xb, dec_out = self._dec_setup(ws, labels.contiguous(), T, T, ctx, ctx.xa)
        if self.dec_xrel is not None:      # (_legacy_layout)
            ckw = dict(ckw, rel_bias=self._rel_table(ws, "d.xrel", self.dec_xrel, T), rel_off=T - 1)
        ctx.cross = (kb, kt, ckw)
        chains = ctx.chains = self._dec_chains(B, T, p, seed, ctx.xa, xb, ctx.rag, *ctx.cross)
        # (embedding → blocks → final norm per chain of samples; the LM head and the loss see all rows again)
        self._run_chains(chains, Ld, lambda i, ch: self._dec_layer_fwd(ws, i, ch, enc_out, kv, rel, T, S))
        logits = self._buf(ws, "d.logits", (B * T, V), torch.float32)
        ops.gemm_nt(dec_out, self.lm_head.w, logits, alpha=self.head_alpha)       # tied LM head × d_model^-0.5, or the untied head
        loss_buf = self._buf(ws, "d.loss", (2,), torch.float32)
        ops.ce_fwd_bwd(logits, ctx.labels, loss_buf, None)
        self.ctx = ctx
        return loss_buf[0], logits.view(B, T, V)

    # ------------------------------------------------------------------------------------------
    # candidate scoring
    # ------------------------------------------------------------------------------------------
    def score(self, input_ids, attention_mask, candidates, lengths=None, chunk=None):
        """input_ids / attention_mask [B,N,L], candidates int64 [B,C,T] (−100 = ignore) → (score fp32 [B,C], n_valid int32 [B,C]):
        score[b,c] = Σ_t log p(candidates[b,c,t] | question b, candidates[b,c,:t]) over the tokens that are not −100, n_valid their count.
        Eval semantics (no dropout, `step_count` stays).  ONE encoder pass serves all candidates: the cross-attention works on the
        encoder states and has no structure over its query rows, so sample b simply brings c·T of them (rows ordered [b, c, t]) while
        the causal self-attention sees B·c sequences of length T.  The candidates go through the decoder `chunk` at a time (default:
        the largest c with B·c·T <= 4096 rows — the fp32 logits are [B·c·T, V]); each chunk: decoder → LM head → lako_seq_logprob.
        Touches neither `self.ctx` nor the training workspaces: a call between forward_loss and backward changes nothing there."""
        cfg, ops = self.cfg, self.ops
        if cfg.legacy_cross_bias:
            raise ValueError("score: legacy_cross_bias makes the cross-attention bias depend on the query's position, which the "
                             "[B, C·T] query layout does not carry")
        if self.shadows_stale:
            self.refresh_shadows()
        B, N, L = input_ids.shape
        if candidates.dim() != 3 or candidates.shape[0] != B or candidates.dtype != torch.int64 or candidates.numel() == 0:
            raise ValueError(f"score: candidates must be int64 [B={B}, C, T], got {tuple(candidates.shape)} {candidates.dtype}")
        C, T = int(candidates.shape[1]), int(candidates.shape[2])
        H, Ld, S = cfg.num_heads, cfg.num_decoder_layers, N * L
        chunk = max(1, min(C, int(chunk) if chunk else 4096 // (B * T)))
        ws = self._workspace(("score", B, N, L, T, chunk))
        bt, enc_out, kv = self._batch(ws, input_ids, attention_mask, lengths, rows_q=chunk * T * H)
        keys, xa = self._cross_keys(bt), bt.xa
        rel = self._rel_table(ws, "d.rel", self.dec_rel, T)
        score = torch.empty(B, C, dtype=torch.float32, device=self.device)
        n_valid = torch.empty(B, C, dtype=torch.int32, device=self.device)
        for c0 in range(0, C, chunk):
            c = min(chunk, C - c0)
            wd = ws if c == chunk else ws.setdefault("tail", {})      # the last, smaller chunk: decoder buffers of its own shapes
            Tx = c * T
            labels = candidates[:, c0:c0 + c].reshape(B * c, T).contiguous()
            if xa is not None and c != chunk:
                xa = self._xattn_plan(bt.rag, B, N, L, Tx * H)
            _, xb, dec_out = self._dec_setup(wd, labels, T, Tx, bt, xa, keep=False, rel=rel)
            ch = self._dec_chains(B, Tx, 0.0, 0, xa, xb, bt.rag, *keys, n=1)[0]
            for i in range(Ld):
                self._dec_layer_fwd(wd, i, ch, enc_out, kv, rel, T, S, Tx=Tx)
            logits = self._buf(wd, "d.logits", (B * Tx, cfg.vocab_size), torch.float32)
            ops.gemm_nt(dec_out, self.lm_head.w, logits, alpha=self.head_alpha)
            if c == C:
                ops.seq_logprob(logits, labels.view(-1), score.view(-1), n_valid.view(-1), T)
            else:      # rows [b, c]: the chunk's columns of the [B, C] outputs
                sc, nv = self._buf(wd, "d.score", (B * c,), torch.float32), self._buf(wd, "d.nvalid", (B * c,), torch.int32)
                ops.seq_logprob(logits, labels.view(-1), sc, nv, T)
                score[:, c0:c0 + c].copy_(sc.view(B, c))
                n_valid[:, c0:c0 + c].copy_(nv.view(B, c))
        return score, n_valid

    # ------------------------------------------------------------------------------------------
    # backward
    # ------------------------------------------------------------------------------------------
    def _ready(self, first_block: str, last_block: str):
        if self.grad_hook is not None:
            a, b = self.by_name[first_block], self.by_name[last_block]
            self.grad_hook(a.off, b.off + -(-b.numel // ALIGN) * ALIGN)

    @staticmethod
    def _nxt(nxt):
        return {} if nxt is None else dict(dx_drop=nxt[0], drop_out=nxt[1])

    def _bwd_plan(self, ctx):
        """The one place backward reads the environment, at the time of the call (the A/B switches may change after forward_loss)"""
        env, p = os.environ.get, ctx.p
        fused = p > 0 and env("LAKO_FUSE_DROP", "1") != "0"
        # WEIGHT GRADIENTS OF SEVERAL ENCODER LAYERS IN ONE LAUNCH (round 4).  A layer's four dW are 108 tiles of 256²; with two K-splits
        # that is 216 workgroups on 256 CUs — every layer's launch leaves 16 % of the chip idle, and nothing can fill it (one workgroup
        # per CU: 128 KiB of LDS).  The products do not have to run where their operands are produced: with the operands of `grp`
        # layers kept in per-slot scratch (dy, dpre, dqkv: 0.66 GB per layer at config 2) their 108·grp tiles × splits go out as ONE grid
        # that the dispatcher deals over the CUs as they free up — 12 layers × 2 splits = 2 592 units = 10.1 rounds of half-K units
        # instead of 12 rounds.  Not with set_checkpoint (the forward operands of a layer are recomputed into ONE slot), not when a
        # data-parallel hook wants every layer's gradients as soon as they exist (overlap mode; the deferred all-reduce does not), not
        # without dropout (dy aliases the residual gradient then).
        grouped = fused and not ctx.ckpt and not (self.grad_hook is not None and self.grad_ranges_early)
        grp = max(1, min(int(env("LAKO_ENC_DW_GROUP", "12")), self.cfg.num_layers, 12)) if grouped else 1
        return _BwdPlan(
            p=p, fused=fused, grp=grp,
            defer=p > 0 and env("LAKO_DEC_DEFER_DW", "1") != "0",
            hb_defer=ctx.xa is not None and len(ctx.chains) == 1 and env("LAKO_DEC_HB_DEFER", "1") != "0",
            # K-splits of the grouped launch: 3 (1 296 tiles × 3 = 15.2 rounds of third-K units; measured per step, rocprofv3, 14 steps:
            # one launch per layer 8.70 ms, 12 layers × 2 / 3 / 4 splits 8.35 / 8.32 / 8.30 ms, 6 layers × 3 splits 8.35 — the library's
            # own cost model, built for one-round launches, would pick 1 split = 6 whole rounds: the slowest, 41.3 ms per step)
            # −3: the hybrid schedule of lako_gemm_tn_grouped — whole rounds of full-K tiles + a finely cut remainder (round 4: 39.8 → 39.1 ms
            # per step against 3 uniform K-splits; a positive value forces that many uniform splits)
            enc_split=int(env("LAKO_ENC_DW_SPLIT", "-3")),
            fuse_gated=env("LAKO_FUSE_GATED", "0") == "1",
            # (the FIRST writer of a freshly zeroed gradient buffer overwrites: no read at all; gradient accumulation adds)
            one=-2 if self._g_fresh else -1)

    def _branch_grad(self, dh, dy, drop, fused):
        """The gradient into a residual branch whose output was dropped with `drop`, given the residual sum's gradient dh: dh itself without
        dropout; else dropout_bwd(dh) in the scratch `dy` — written by the RMSNorm backward that produced dh (`fused`), or by a launch here."""
        if drop is not None and not fused:
            self.ops.dropout_apply(dh, dy, drop)
        return dh if drop is None else dy

    def _ffn_bwd(self, lw, dh, dy, a1, pre, bw, drop_act, drop_out, buf, names, dxn, wgrad, library_gated):
        """Backward of a residual feed-forward sublayer up to its RMSNorm, of either stack: dh [rows, d] the gradient wrt the sublayer's
        output, `dy` the scratch of _branch_grad → dxn, the gradient wrt the normed input.  What differs between the stacks:
        `buf(name, cols)` and `names` of dpre and dha — the scratch of these rows: the encoder's per-slot buffers, a chain's rows of the
        decoder's full-batch ones (named by role and slot, never by row count: the unpadded encoder's changes with almost every batch);
        `wgrad(w, dy)` — where the problem dW[w] += dyᵀ·x goes: into a group, to the full-batch launch after the chains, or out now;
        `library_gated` — whether to ask for the library's gated-GELU routes (_fuse_gated).  NOT the decoder: its skinny products stay
        the plain product + the standalone kernel whatever their row count.
        `pre` (gated-GELU feed-forward): the saved [a | b] product; `drop_act` the dropout of the activation, `drop_out` of the output."""
        ops, f = self.ops, a1.shape[1]
        dy = self._branch_grad(dh, dy, drop_out, bw.fused)
        wgrad("wo", dy)
        if pre is not None:
            dpre = buf(names[0], 2 * f)
            fz = self._fuse_gated(dy, lw["wo"].wt, f, bw.fuse_gated) if library_gated else None
            if fz == "fused":      # dpre straight from the dY·Wo product's epilogue (bit-identical to the two launches below)
                ops.gemm_nt_gated(dy, lw["wo"].wt, dpre, pre, drop_act, backward=True)
            else:
                dha = buf(names[1], f)
                (ops.gemm_nt_four if fz else ops.gemm_nt)(dy, lw["wo"].wt, dha)
                ops.gated_gelu_bwd(dha, pre, dpre, drop_act)
        else:
            dpre = buf(names[0], f)
            ops.gemm_nt(dy, lw["wo"].wt, dpre, aux=a1, aux_scale=1.0 / (1.0 - bw.p))   # ∘ [relu'>0] ∘ dropout
        wgrad("wi", dpre)
        ops.gemm_nt(dpre, lw["wi"].wt, dxn)

    def backward(self, upstream=None):
        """Accumulate d(loss)/d(params) into G.  `upstream`: optional device scalar tensor multiplying the loss."""
        ctx, ops = self.ctx, self.ops
        if ctx is None:
            raise RuntimeError("backward() without a preceding forward_loss()")
        bw = self._bwd_plan(ctx)
        self._g_fresh = False
        ws, p, seed, rag, L = ctx.ws, ctx.p, ctx.seed, ctx.rag, ctx.L
        self._row_cap = {rag.M: ctx.B * ctx.N * L} if rag is not None else {}
        Me = rag.M if rag is not None else ctx.B * ctx.N * L
        dr = (lambda site: (p, seed, site)) if p > 0 else (lambda site: None)
        tmp = self._workspace(("bwd", ctx.B, ctx.N, L, ctx.T))
        dh = self._head_bwd(ws, tmp, ctx, bw, upstream)
        xb, dkv = self._dec_bwd(ws, tmp, ctx, bw, dh, Me)
        # ---- cross K/V projection of all decoder layers -----------------------------------------
        deh, dxe = (self._buf(tmp, name, (Me, self.cfg.d_model)) for name in ("e.dh", "e.dxn"))
        if ctx.xa is not None:
            self._xattn_denc(xb, ctx.xa, tmp, Me, dxe)
        else:
            ops.gemm_tn(dkv, ws["e.out"], self.kv_all.g)
            ops.gemm_nt(dkv, self.kv_all.wt, dxe)
        # ---- encoder -----------------------------------------------------------------------------
        self._enc_bwd(ws, tmp, ctx, bw, dr, deh, dxe)
        self._embed_bwd(ctx.enc_ids, deh, dr(S_ENC_EMBED))
        ops.relpos_reduce(tmp["e.drel"], self._lut(L, L, True), self.enc_rel.g)
        self._ready("enc.rel", "shared")
        self.step_count += 1   # next forward draws fresh dropout masks
        self.ctx = None

    def _head_bwd(self, ws, tmp, ctx, bw, upstream):
        """loss + LM head: the gradient wrt the decoder's normed, dropped output in "d.dxn"; → the decoder's residual-gradient buffer"""
        ops, Md, d, alpha, head = self.ops, ctx.B * ctx.T, self.cfg.d_model, self.head_alpha, self.lm_head
        dlog = self._buf(tmp, "dlogits", (Md, self.cfg.vocab_size))
        ops.ce_fwd_bwd(ws["d.logits"], ctx.labels, self._buf(tmp, "loss2", (2,), torch.float32), dlog, upstream)
        dh, dout = (self._buf(tmp, name, (Md, d)) for name in ("d.dh", "d.dxn"))
        # K = vocabulary (32128) for an [Md, d] output of a handful of tiles: accumulate in fp32 with atomics so that the
        # library may split K over the idle CUs (gemm_nt_ring_kernel), then round once to the compute dtype
        dout32 = dout if dout.dtype == torch.float32 else self._buf(tmp, "d.dout32", (Md, d), torch.float32)
        if self.det:      # LAKO_DETERMINISTIC=1: one workgroup per output tile walks the whole vocabulary (no K-split, no atomics)
            ops.gemm_nt(dlog, head.wt, dout, alpha=alpha)
        else:
            ops.zero_(dout32)
            ops.gemm_nt(dlog, head.wt, dout32, alpha=alpha, atomic=True)
            if dout32 is not dout:
                ops.cast(dout32.view(-1), dout.view(-1))
        # (K = B·T rows, 378 tiles: one K-split; nothing else touches the embedding gradient until the embedding backward kernels later on
        # this stream: plain read-modify-write instead of 99 MB of float atomics; bw.one: the first writer overwrites)
        ops.gemm_tn(dlog, ws["d.out"], head.g, alpha=alpha, split_k=bw.one)
        if head is not self.shared:
            self._ready("lm_head", "lm_head")
        return dh

    def _dec_bwd(self, ws, tmp, ctx, bw, dh, Me):
        """The decoder's chains, last layer first, then what they left for after their join.  → (xb, dkv): what the encoder-state
        gradient is assembled from (_xattn_buffers), or the gradient of the projected cross-attention K / V"""
        ops, cfg, xa = self.ops, self.cfg, ctx.xa
        B, N, L, T, H, Ld = ctx.B, ctx.N, ctx.L, ctx.T, cfg.num_heads, cfg.num_decoder_layers
        xb = self._xattn_buffers(ws, B, N, L, T, Ld, xa.splits) if xa is not None else None
        dkv = self._buf(tmp, "dkv", (Me, self.kv_all.w.shape[0])) if xa is None else None
        drel = self._buf(tmp, "d.drel", (H, 2 * T - 1), torch.float32)
        ops.zero_(drel)
        dxrel = None
        if self.dec_xrel is not None:      # (_legacy_layout)
            dxrel = self._buf(tmp, "d.dxrel", (H, 2 * T - 1), torch.float32)
            ops.zero_(dxrel)
        dw_all = []      # every decoder weight gradient of the step (K = B·T rows): grouped launches after the last layer
        # the 2 · Ld head-batched Wk / Wv gradient products likewise: ONE launch after the last layer (each alone is its dispatch: 24 × 8 µs);
        # with one chain only (LAKO_DEC_HB_DEFER=0: inside the layers)
        hb_all = [] if bw.hb_defer else None
        self._run_chains(ctx.chains, Ld, lambda i, ch: self._dec_layer_bwd(ws, tmp, i, ch, dh, bw, drel, dxrel, dkv, T, N * L,
                                                                           dw_all, hb_all), reverse=True)
        if hb_all:
            ops.headbatch_tn_multi(hb_all)
        if dw_all:      # (K = B·T rows: one K-split; the chains have joined and nothing else touches these gradients: plain read-modify-write)
            ops.gemm_tn_grouped(dw_all, split_k=bw.one)
        ops.relpos_reduce(drel, self._lut(T, T, False), self.dec_rel.g)
        if dxrel is not None:
            ops.relpos_reduce(dxrel, self._lut(T, T, False), self.dec_xrel.g)
        return xb, dkv

    def _enc_bwd(self, ws, tmp, ctx, bw, dr, deh, dxe):
        """The encoder's final norm and its layers, last first: dxe the gradient wrt the encoder's output → deh, wrt the embedding's.  The
        weight gradients of bw.grp layers go out in ONE launch (_bwd_plan); a layer's are reported (_ready) once that launch is out."""
        ops, Le, grp, fused, L, (Me, d) = self.ops, self.cfg.num_layers, bw.grp, bw.fused, ctx.L, deh.shape
        slot = (lambda i: f".{i % grp}") if grp > 1 else (lambda i: "")      # a layer's scratch: one set per layer of a group
        dy_f = self._buf(tmp, "e.dy.ffn" + slot(Le - 1), (Me, d)) if fused else None
        ops.rmsnorm_bwd(dxe, ws[f"e.h{Le}"], self.enc_final.p, ws["e.rsf"], None, deh, self.enc_final.g, dr(S_ENC_FINAL),
                        **self._nxt((dy_f, dr(_enc_site(Le - 1, 3))) if fused else None))
        self._ready("dec.final_ln", "enc.final_ln")
        drel_e = self._buf(tmp, "e.drel", (self.cfg.num_heads, 2 * L - 1), torch.float32)
        ops.zero_(drel_e)
        dw = []

        def flush(i):      # a complete group goes out before layer i's last norm backward rewrites the slot of layer i − 1
            if i % grp == 0:
                ops.gemm_tn_grouped(list(dw), split_k=bw.enc_split if grp > 1 else 0, workspace=self._tn_scratch)
                dw.clear()

        for i in reversed(range(Le)):
            self._enc_layer_bwd(ws, tmp, i, ctx, bw, dr, deh, dxe, drel_e, dw, slot, flush)
            if i % grp == 0:      # the group that layer i completes: its gradients are final
                for li in reversed(range(i, min(i + grp, Le))):
                    self._ready(f"enc.{li}.qkv", f"enc.{li}.ln2")

    def _enc_layer_bwd(self, ws, tmp, i, ctx, bw, dr, deh, dxe, drel_e, dw, slot, flush):
        """Backward of _enc_layer_fwd: deh holds the gradient wrt the block's output on entry and wrt its input on exit.
        The layer's four weight gradients (K = all tokens, small M×N) go into `dw` for ONE grouped launch (with those of the other
        layers of its group): 108 tiles per layer fill the chip with ~2 K-splits, where four separate launches need 7–28 splits each
        and pay one fp32 atomic pass over the output per split.  Their operands: the scratch `slot(i)` names; `flush(i)` sends the group."""
        cfg, ops, lw, rag, p, fused = self.cfg, self.ops, self.enc[i], ctx.rag, bw.p, bw.fused
        d, inner, L, BN, Me = cfg.d_model, cfg.inner_dim, ctx.L, ctx.B * ctx.N, deh.shape[0]
        j, sl = i, slot(i)
        buf = lambda name, cols: self._buf(tmp, name, (Me, cols))                                  # noqa: E731
        if ctx.ckpt:   # recompute this block's intermediates from its saved input (same seeds → same dropout masks)
            j = 0
            self._enc_layer_fwd(ws, i, 0, ws[f"e.h{i}"], None, BN, L, ctx.enc_mask, ws["e.rel"], dr, rag)

        def wgrad(w, dy):
            x = ws[f"e.{_ENC_DW_X[w]}.{j}"]
            if p == 0 and w in ("wo", "o"):      # (no dropout: dy IS the residual gradient deh, which the next ops rewrite)
                ops.gemm_tn(dy, x, lw[w].g)
            else:
                dw.append((dy, x, lw[w].g, 1.0))

        # ---- FFN ------------------------------------------------------------------------------
        nxt = (buf("e.dy" + sl, d), dr(_enc_site(i, 1))) if fused else None
        self._ffn_bwd(lw, deh, buf("e.dy.ffn" + sl, d) if p > 0 else None, ws[f"e.a1.{j}"], ws[f"e.pre.{j}"] if cfg.gated else None, bw,
                      dr(_enc_site(i, 2)), dr(_enc_site(i, 3)), buf, ("e.dpre" + sl, "e.dha"), dxe, wgrad, library_gated=True)
        ops.rmsnorm_bwd(dxe, ws[f"e.h1.{j}"], lw["ln2"].p, ws[f"e.rs2.{j}"], deh, deh, lw["ln2"].g, **self._nxt(nxt))
        # ---- self-attention ----------------------------------------------------------------------
        dy = self._branch_grad(deh, buf("e.dy" + sl, d) if p > 0 else None, dr(_enc_site(i, 1)), fused)
        wgrad("o", dy)
        dctx = buf("e.dctx", inner)
        ops.gemm_nt(dy, lw["o"].wt, dctx)
        qkv, dqkv = ws[f"e.qkv.{j}"], buf("e.dqkv" + sl, 3 * inner)
        hb, ht, akw = self._enc_attn_layout(rag, BN, L, ctx.enc_mask)
        ops.attn_bwd(self._heads(qkv, hb, ht, 0), self._heads(qkv, hb, ht, inner), self._heads(qkv, hb, ht, 2 * inner),
                     self._heads(ws[f"e.ctx.{j}"], hb, ht, 0), self._heads(dctx, hb, ht, 0), ws[f"e.st.{j}"],
                     self._heads(dqkv, hb, ht, 0), self._heads(dqkv, hb, ht, inner), self._heads(dqkv, hb, ht, 2 * inner),
                     rel_bias=ws["e.rel"], drel=drel_e, rel_off=L - 1, drop=dr(_enc_site(i, 0)), **akw)
        wgrad("qkv", dqkv)
        ops.gemm_nt(dqkv, lw["qkv"].wt, dxe)
        flush(i)
        nxt = (buf("e.dy.ffn" + slot(i - 1), d), dr(_enc_site(i - 1, 3))) if fused and i > 0 else None
        ops.rmsnorm_bwd(dxe, ws[f"e.h{i}"], lw["ln1"].p, ws[f"e.rs1.{j}"], deh, deh, lw["ln1"].g, **self._nxt(nxt))

    # ------------------------------------------------------------------------------------------
    # greedy decode  (HF generate: num_beams=1, do_sample=False, use_cache=True), and sampled decode (do_sample=True: temperature,
    # top-k, top-p; num_return_sequences = K rows per question over ONE copy of the question's encoder states), and beam search
    # (num_beams = K: the beams are those K rows; selection, bookkeeping and cache reordering on the device, csrc/beam.hip)
    # ------------------------------------------------------------------------------------------
    def generate(self, input_ids, attention_mask, max_length: int, capture_scores: bool = False, lengths=None, *, do_sample: bool = False,
                 temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, num_return_sequences: int = 1, seed=None,
                 return_scores: bool = False, num_beams: int = 1, length_penalty: float = 1.0, early_stopping: bool = False):
        """Defaults: the greedy decode, int64 [B, <= max_length].  do_sample / return_scores switch the last launch of a step from
        lako_greedy_step to lako_sample_step (greedy with scores: top_k = 1) and the decoder-side buffers to B·K rows, K =
        num_return_sequences: row b·K + k is answer k of question b (HF's layout).  The encoder runs once for the B questions and its
        states (or their K/V projections) are stored once; the K rows of a question are K query positions of its cross-attention.
        return_scores adds float32 [B, K]: Σ over a row's emitted tokens (its EOS included, the pads after it not) of
        log_softmax(raw logits)[token] — the model's own log-probability, what `score` returns for that sequence; HF's transition scores
        are those of the PROCESSED distribution (temperature applied, truncated tokens at −∞), which say how likely the sampler was to
        pick the token, not how likely the model finds the answer — the quantity a re-ranker wants is the latter.

        num_beams = K > 1: beam search with the semantics of transformers 5.15 `_beam_search` (include/lako_hip.h restates them), all
        on the device: the decoder side has B·K rows, the last launches of a step are lako_beam_rows → lako_beam_merge →
        lako_beam_gather, and the K beams of a question are K query positions of its cross-attention (the encoder states are neither
        replicated nor reordered).  Returns int64 [B·R, <= max_length], R = num_return_sequences <= K: question b in rows b·R … b·R+R−1,
        best finished hypothesis first, cropped to the longest returned row, pad after each row's EOS (HF 5.15 fills with EOS where
        pad is 0: not reproduced).  Equal candidates go by ascending flat index beam·V + token (torch.topk leaves ties open).
        return_scores adds float32 [B, R]: the RAW sum of log-probabilities, as above — HF's `sequences_scores`, the value the
        hypotheses are ranked by, is raw / len**length_penalty with len = the number of generated tokens (EOS included)."""
        self._check_generate_args(do_sample, temperature, top_k, top_p, num_return_sequences, capture_scores, num_beams, length_penalty,
                                  early_stopping)
        beam = int(num_beams) > 1
        K, sampled = int(num_beams if beam else num_return_sequences), bool(do_sample or return_scores) and not beam
        if self.shadows_stale:
            self.refresh_shadows()
        B, N, L = input_ids.shape
        ws = self._workspace(("gen", B, N, L, max_length) + ((K, "b") if beam else (K, "s") if sampled else ()))
        sparams = self._sampler_params(ws, do_sample, temperature, top_k, top_p, seed) if sampled else None
        bparams = self._beam_params(ws, length_penalty, early_stopping) if beam else None
        # cross-attention in the encoder-state space (R = H query rows per sample and step; no K/V projection of the N·L encoder
        # states): five launches per layer and step instead of one — slower while the host's launch rate bounds the loop (eager:
        # 113 ms against 93 ms for 50 tokens at config 2), faster once a step is one graph launch.  Never when the raw scores are
        # captured: those come out of the projected kernel in the reference's layout.  LAKO_XATTN_GENERATE=0/1 overrides.
        use_graph = self.device.type == "cuda" and not capture_scores and getattr(self.ops, "probe", None) is None and \
            os.environ.get("LAKO_GEN_GRAPH", "1") != "0"
        use_x = os.environ.get("LAKO_XATTN_GENERATE", "1" if use_graph else "0") == "1" and not capture_scores
        # valid tokens only (as in forward_loss) unless the raw scores are captured: those are laid out per padded position
        bt, enc_out, kv = self._batch(ws, input_ids, attention_mask, lengths, rows_q=K * self.cfg.num_heads if use_x else None, T=max_length,
                         keep_padding=capture_scores)
        g = _GenState(self, ws, bt, enc_out, kv, max_length, K, sampled, capture_scores, sparams, bparams)
        n_out = self._gen_drive(g, lambda t: self._gen_step(g, t), use_graph)
        if beam:
            # the finished set is frozen from the step that ended the decoding (step n_out − 2, which wrote set (n_out − 1) & 1; a later
            # step only copies it on).  One host read — the longest returned row — crops the result.
            R = int(num_return_sequences)
            fin = g.fin2[(n_out - 1) & 1].view(B, K, max_length)[:, :R]
            width = max(1, min(max_length, int(g.fin_len.view(B, K)[:, :R].max())))
            out = fin[:, :, :width].reshape(B * R, width).clone()
            return (out, g.fin_raw.view(B, K)[:, :R].clone()) if return_scores else out
        out = g.seq[:, :n_out].clone()
        if capture_scores:
            # [B, H, n_layers, S] — the layout get_crossattention_scores builds with torch.cat(dim=2), src/model.py:152-160
            cs = g.scores[:, :, :, 0, :].permute(1, 2, 0, 3).contiguous()
            return (out, cs, g.score.view(B, K).clone()) if return_scores else (out, cs)
        return (out, g.score.view(B, K).clone()) if return_scores else out

    def _check_generate_args(self, do_sample, temperature, top_k, top_p, num_return_sequences, capture_scores, num_beams=1,
                             length_penalty=1.0, early_stopping=False):
        """the argument errors of generate: raised before anything runs"""
        K = int(num_return_sequences)
        if isinstance(num_beams, bool) or not isinstance(num_beams, (int, np.integer)) or num_beams < 1:
            raise ValueError(f"num_beams must be an integer >= 1, got {num_beams!r}")
        NB = int(num_beams)
        if NB > 16:
            raise ValueError(f"num_beams must be <= 16, got {num_beams}")
        if NB > 1 and 2 * NB > self.cfg.vocab_size:
            raise ValueError(f"num_beams = {NB} needs 2·num_beams <= vocab_size = {self.cfg.vocab_size} candidates per row")
        if not isinstance(early_stopping, bool):
            raise ValueError(f"early_stopping must be a bool, got {early_stopping!r}")
        if isinstance(length_penalty, bool) or not isinstance(length_penalty, (int, float, np.integer, np.floating)) or \
                not float(length_penalty) == float(length_penalty):
            raise ValueError(f"length_penalty must be a number, got {length_penalty!r}")
        if NB > 1 and do_sample:
            raise ValueError("num_beams > 1 with do_sample=True: beam search does not sample")
        if NB > 1 and capture_scores:
            raise ValueError("num_beams > 1 while the cross-attention scores are captured: the capture belongs to the greedy decode")
        if NB > 1 and self.cfg.legacy_cross_bias:
            raise ValueError("num_beams > 1 is not implemented with legacy_cross_bias")
        if NB > 1 and K > NB:
            raise ValueError(f"num_return_sequences = {K} must be <= num_beams = {NB}")
        if not temperature > 0:
            raise ValueError(f"temperature must be > 0, got {temperature}")
        if not 0 < top_p <= 1:
            raise ValueError(f"top_p must be in (0, 1], got {top_p}")
        if int(top_k) != top_k or top_k < 0:
            raise ValueError(f"top_k must be an integer >= 0, got {top_k}")
        if K < 1:
            raise ValueError(f"num_return_sequences must be >= 1, got {num_return_sequences}")
        if K > 1 and not do_sample and NB == 1:
            raise ValueError("num_return_sequences > 1 needs do_sample=True or num_beams > 1: greedy decoding has one answer per question")
        if do_sample and capture_scores:
            raise ValueError("do_sample=True while the cross-attention scores are captured: the capture belongs to the greedy decode")
        if K > 1 and NB == 1 and self.cfg.legacy_cross_bias:
            raise ValueError("num_return_sequences > 1 is not implemented with legacy_cross_bias")

    def _sampler_params(self, ws, do_sample, temperature, top_k, top_p, seed):
        """The sampler's settings live in device memory at a stable address (the kernel reads them: captured steps replay unchanged
        under other settings); the step index is an argument baked into each step's graph, as `pos` is.  → int32 [8] `g.sparams`"""
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())      # torch's global (host) generator
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        words = np.array([np.float32(temperature).view(np.uint32), np.float32(top_p).view(np.uint32),
                          (min(int(top_k), 0x7FFFFFFF) if do_sample else 1), seed & 0xFFFFFFFF, seed >> 32, 0, 0, 0], dtype=np.uint32)
        sparams = self._buf(ws, "g.sparams", (8,), torch.int32)
        if "g.sparams_host" not in ws:       # pinned: the upload is an enqueue like every other launch of the call
            ws["g.sparams_host"] = torch.zeros(8, dtype=torch.int32, pin_memory=torch.cuda.is_available())
        ws["g.sparams_host"].copy_(torch.from_numpy(words.view(np.int32)))      # (the last call ended with a wait on its last step)
        sparams.copy_(ws["g.sparams_host"], non_blocking=True)
        return sparams

    def _beam_params(self, ws, length_penalty, early_stopping):
        """Beam search's per-call settings, in device memory at a stable address like the sampler's (captured steps replay under other
        settings); the token column and "this is the last step" are arguments baked into each step's graph.  → int32 [8] `g.bparams`"""
        words = np.array([np.float32(length_penalty).view(np.uint32), int(early_stopping), 0, 0, 0, 0, 0, 0], dtype=np.uint32)
        bparams = self._buf(ws, "g.bparams", (8,), torch.int32)
        if "g.bparams_host" not in ws:
            ws["g.bparams_host"] = torch.zeros(8, dtype=torch.int32, pin_memory=torch.cuda.is_available())
        ws["g.bparams_host"].copy_(torch.from_numpy(words.view(np.int32)))      # (the last call ended with a wait on its last step)
        bparams.copy_(ws["g.bparams_host"], non_blocking=True)
        return bparams

    def _gen_step(self, g, t):
        """enqueue decode step t (reads nxt, writes seq[:, t + 1], nxt, done, ndone[t]): a decoder block per layer over the key / value
        cache (not _dec_layer_fwd: other buffer lifetimes, other kernels), final norm, LM head, the greedy or sampling kernel — or beam
        search's three (the step runs on cache set t & 1 and leaves the next step's rows, reordered by parent beam, in the other)"""
        ops, cfg = self.ops, self.cfg
        inner, H, dk = cfg.inner_dim, cfg.num_heads, cfg.d_kv
        BK, ML, h, h1, h2, xn, rs, c1, qc, c2, a1 = g.BK, g.ML, g.h, g.h1, g.h2, g.xn, g.rs, g.c1, g.qc, g.c2, g.a1
        ops.embed_fwd(g.nxt, self.shared.w, h)
        xkw = g.keys[2] if g.xrel is None else dict(g.keys[2], rel_bias=g.xrel, rel_off=ML - 1 - (0 if g.capture else t))
        for i, lw in enumerate(self.dec):
            cache = g.cache2[t & 1][i] if g.beam else g.cache[i]
            self._dec_norm_gemm(h, lw["ln1"].p, xn, rs, lw["qkv"].w, cache.view(BK, ML * 3 * inner)[:, t * 3 * inner:(t + 1) * 3 * inner])
            qs = cache[:, t:t + 1, :inner].unflatten(2, (H, dk))
            kc = cache[:, :t + 1, inner:2 * inner].unflatten(2, (H, dk))
            vc = cache[:, :t + 1, 2 * inner:].unflatten(2, (H, dk))
            ops.attn_fwd(qs, kc, vc, c1.view(BK, 1, H, dk), g.st, rel_bias=g.rel, rel_off=ML - 1 - t)
            ops.gemm_nt(c1, lw["o"].w, h1, resid=h)
            self._dec_norm_gemm(h1, lw["ln2"].p, xn, rs, lw["cq"].w, qc)
            self._gen_cross(g, i, t, xkw)
            ops.gemm_nt(c2, lw["co"].w, h2, resid=h1)
            out1, act = (g.pre, {}) if cfg.gated else (a1, dict(relu=True))
            self._dec_norm_gemm(h2, lw["ln3"].p, xn, rs, lw["wi"].w, out1, **act)
            if cfg.gated:
                ops.gated_gelu_fwd(g.pre, a1, None)
            ops.gemm_nt(a1, lw["wo"].w, h, resid=h2)
        ops.rmsnorm_fwd(h, self.dec_final.p, xn, rs, cfg.layer_norm_epsilon)
        ops.gemm_nt(xn, self.lm_head.w, g.logits, alpha=self.head_alpha)
        if g.beam:
            src, dst = t & 1, (t + 1) & 1
            ops.beam_rows(g.logits, g.run, g.cand_acc, g.cand_tok)
            ops.beam_merge(g.cand_acc, g.cand_tok, g.seq2[src], g.seq2[dst], g.fin2[src], g.fin2[dst], t + 1, t + 2 == ML, g.run, g.nxt,
                           g.parent, g.fin_score, g.fin_raw, g.fin_len, g.fin_filled, g.open, g.ndone[t:t + 1], g.bparams, cfg.eos_token_id,
                           cfg.pad_token_id)
            # (nothing runs after the last step; the gather's 16-byte unit always divides a cache row: d_kv is 32, 64 or 128 — Engine.__init__)
            if t + 2 < ML:
                ops.beam_gather(g.bcache[src], g.bcache[dst], g.parent, t + 1, inner, 2 * inner)
        elif g.sampled:
            ops.sample_step(g.logits, g.seq, t + 1, g.nxt, g.done, g.score, g.ndone[t:t + 1], g.sparams, t, g.K, cfg.eos_token_id,
                            cfg.pad_token_id)
        else:
            ops.greedy_step(g.logits, g.seq, t + 1, g.nxt, g.done, g.ndone[t:t + 1], cfg.eos_token_id, cfg.pad_token_id)

    def _gen_cross(self, g, i, t, xkw):
        """cross-attention of decode step t in layer i, qc → c2, by the call's route: on the projected K / V (`xkw`: the key arguments),
        or on the encoder states — the unfused kernels, or scores, softmax and context in one pass (g.fused)"""
        ops, cfg = self.ops, self.cfg
        inner, H, dk, d, B, K, qc, c2 = cfg.inner_dim, cfg.num_heads, cfg.d_kv, cfg.d_model, g.B, g.K, g.qc, g.c2
        if g.xa is None:
            ops.attn_fwd(qc.view(B, K, H, dk), self._heads(g.kv, *g.keys[:2], 2 * i * inner),
                         self._heads(g.kv, *g.keys[:2], (2 * i + 1) * inner), c2.view(B, K, H, dk), g.stx,
                         scores_out=g.scores[i] if (g.capture and t == 0) else None, **xkw)
            return
        xq, xoff = g.xq, g.xoff
        ops.headbatch_nt(qc.view(B, K, H, dk), self._xw(i, "k", transposed=True), xq.view(B, K, H, d))
        if g.fused:
            if K == 1:
                ops.xattn_decode(xq, g.enc_out, xoff[0], g.pml, g.pc)
            else:
                ops.xattn_decode_multi(xq.view(B, K, H, d), g.enc_out, xoff[0], g.pml, g.pc)
            r0 = (2 * i + 1) * inner
            ops.xattn_decode_combine(g.pml, g.pc, self.kv_all.w[r0:r0 + inner], c2, H)
        else:
            ops.xattn_scores(xq, g.enc_out, xoff[0], xoff[1], g.cap, g.xs)
            ops.xattn_softmax_fwd(g.xs, g.xst, g.xp, xoff[0], xoff[1], K, H, g.S)
            ops.xattn_context(g.xp, g.enc_out, xoff[0], xoff[1], g.xc)
            ops.headbatch_nt(g.xc.view(g.xa.splits, B, K, H, d), self._xw(i, "v"), c2.view(B, K, H, dk))

    def _gen_drive(self, g, step, use_graph):
        """Run step(t), t = 0 …, until every row has ended → the number of token columns to return.  A decode step is ≈130 dependent
        launches of a few µs each: the host's launch rate bounds the loop.  After one eager call per (shape, mode) — the kernels' one-time
        setup must not happen under capture — every step position is captured ONCE into a HIP graph (kernel arguments that depend on t
        are baked in; what changes from call to call lives in workspace buffers whose addresses do not: _GenState COPIES the offsets /
        key mask into them) and replayed: one launch per token.  `step` is the caller's: another decoding strategy brings its own."""
        ws, ML, BK, ndone, ndone_host, LAG, events = g.ws, g.ML, g.BK, g.ndone, g.ndone_host, 2, []
        graphs = None
        if use_graph:
            gs = ws.setdefault("g.graphs", {}).get(g.mode)
            ptrs = {k_: v.data_ptr() for k_, v in ws.items() if k_.startswith("^")}
            if gs is None or any(ptrs.get(k_) != p_ for k_, p_ in gs["ptrs"].items()):      # a workspace buffer moved: start over
                gs = ws["g.graphs"][g.mode] = dict(ptrs=ptrs, warm=False, steps={}, pool=None)
            if gs["warm"]:
                graphs = gs
            gs["warm"] = True
        for t in range(ML - 1):
            if graphs is None:
                step(t)
            else:
                gr = graphs["steps"].get(t)
                if gr is None:
                    gr = torch.cuda.CUDAGraph()
                    if graphs["pool"] is None:
                        graphs["pool"] = torch.cuda.graph_pool_handle()
                    # thread_local: a data-loader / pin-memory thread may touch the runtime while this thread captures
                    with torch.cuda.graph(gr, pool=graphs["pool"], capture_error_mode="thread_local"):
                        step(t)
                    graphs["steps"][t] = gr
                gr.replay()
            ndone_host[t:t + 1].copy_(ndone[t:t + 1], non_blocking=True)
            if ndone.is_cuda:
                events.append(torch.cuda.Event())
                events[-1].record()
            look = t - LAG if (ndone.is_cuda and t < ML - 2) else t     # the last step is checked at once
            if look >= 0:
                if ndone.is_cuda:
                    events[look].synchronize()
                first = next((u for u in range(max(look - LAG, 0), look + 1) if int(ndone_host[u]) == BK), None)
                if first is not None:        # HF stops right after the step in which the last row emitted EOS
                    return first + 2
        return max(ML, 1)
