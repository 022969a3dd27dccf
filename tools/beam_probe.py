#!/usr/bin/env python
"""Beam search timing at config 2 (T5-base, B=16, N=20, L=200 with passage lengths U{100…200}, bf16, graphs replayed), max_length 50:
wall time of generate() + device synchronise for greedy, sampled K and beam K ∈ {2, 4, 8} — 3 warm-up calls each, then 5 repetitions with
the candidates alternating inside every repetition; medians with min – max.  Then the device time of the three beam kernels next to
lako_sample_step at [rows, 32128], rows ∈ {32, 128} (events around 50 back-to-back launches, 5 warm-up launches, median of 5).
`python tools/beam_probe.py [--kernels-only]`"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from lako_amd import FiDConfig, FiDT5  # noqa: E402
from lako_amd.ops import HipOps  # noqa: E402

dev = torch.device("cuda:0")


def med(xs):
    return f"{statistics.median(xs):8.2f} ({min(xs):.2f} – {max(xs):.2f})"


def calls():
    cfg = FiDConfig.named("base")
    model = FiDT5(cfg, dtype=torch.bfloat16).cuda().eval()
    B, N, L, ML = 16, 20, 200, 50
    ids, mask, _ = bench.synthetic_batch(B, N, L, 8, cfg.vocab_size, seed=1, device=dev)
    g = torch.Generator().manual_seed(0)
    lens = torch.randint(100, L + 1, (B, N), generator=g)
    mask = (torch.arange(L)[None, None, :] < lens[:, :, None]).to(dev)
    lens = lens.to(torch.int32)
    cands = {"greedy": {}}
    for K in (2, 4, 8):
        cands[f"sampled K={K}"] = dict(do_sample=True, top_k=50, top_p=0.95, num_return_sequences=K, seed=3)
        cands[f"beam K={K}"] = dict(num_beams=K, num_return_sequences=K)
    run = lambda kw: model.generate(input_ids=ids, attention_mask=mask, max_length=ML, passage_lengths=lens, **kw)      # noqa: E731
    widths = {}
    for name, kw in cands.items():
        for _ in range(3):
            widths[name] = tuple(run(kw).shape)
    torch.cuda.synchronize()
    times = {name: [] for name in cands}
    for _ in range(5):
        for name, kw in cands.items():
            t0 = time.perf_counter()
            run(kw)
            torch.cuda.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0))
    for name in cands:
        print(f"{name:14s} {med(times[name])} ms   output {widths[name]}", flush=True)


def kernels():
    ops = HipOps()
    V = 32128
    import numpy as np

    def pack_params(temperature, top_p, top_k, seed):      # the 8 words lako_sample_step reads
        w = np.array([np.float32(temperature).view(np.uint32), np.float32(top_p).view(np.uint32), top_k, seed & 0xFFFFFFFF, seed >> 32, 0, 0, 0],
                     dtype=np.uint32)
        return torch.from_numpy(w.view(np.int32))

    def timed(fn, n=50):
        for _ in range(5):
            fn()
        out = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(1e3 * e0.elapsed_time(e1) / n)
        return out
    for rows in (32, 128):
        x = torch.randn(rows, V, device=dev) * 3
        for K in (2, 8):
            B, C, ld, t = rows // K, 2 * K, 50, 25
            run = -torch.sort(torch.rand(B, K, device=dev)).values.reshape(rows).contiguous()
            cacc, ctok = torch.zeros(rows, C, device=dev), torch.zeros(rows, C, dtype=torch.int32, device=dev)
            seq = torch.zeros(2, rows, ld, dtype=torch.int64, device=dev)
            fin = torch.zeros(2, rows, ld, dtype=torch.int64, device=dev)
            z32 = lambda dt: torch.zeros(rows, dtype=dt, device=dev)      # noqa: E731
            nxt, parent, fs, fr, fl, ff = z32(torch.int64), z32(torch.int32), z32(torch.float32), z32(torch.float32), z32(torch.int32), z32(torch.uint8)
            op, nd = torch.ones(B, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
            params = torch.tensor([0x3F800000, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=dev)
            cache = torch.zeros(2, 12, rows, ld, 3 * 768, dtype=torch.bfloat16, device=dev)
            run0 = run.clone()

            def merge():
                run.copy_(run0)
                ops.beam_merge(cacc, ctok, seq[0], seq[1], fin[0], fin[1], t + 1, False, run, nxt, parent, fs, fr, fl, ff, op, nd, params, 1, 0)
            ops.beam_rows(x, run, cacc, ctok)
            print(f"rows {rows:3d} K {K}: beam_rows {med(timed(lambda: ops.beam_rows(x, run, cacc, ctok)))} µs   "
                  f"beam_merge (+ a 1 KB copy) {med(timed(merge))} µs   "
                  f"beam_gather (12 layers, t = {t}, {12 * rows * (t + 1) * 2 * 768 * 2 / 1e6:.1f} MB) "
                  f"{med(timed(lambda: ops.beam_gather(cache[0], cache[1], parent, t + 1, 768, 2 * 768)))} µs", flush=True)
        seq1, done, score = torch.zeros(rows, 50, dtype=torch.int64, device=dev), torch.zeros(rows, dtype=torch.uint8, device=dev), torch.zeros(rows, device=dev)
        nxt1, nd1 = torch.zeros(rows, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        for what, (tk, tp) in {"no truncation": (0, 1.0), "top_k = 1": (1, 1.0), "top-k 50 + top-p 0.9": (50, 0.9)}.items():
            p = pack_params(1.0, tp, tk, 5).to(dev)

            def sample():
                done.zero_()
                ops.sample_step(x, seq1, 3, nxt1, done, score, nd1, p, 2, 1, 1, 0)
            print(f"rows {rows:3d}: sample_step (+ a zeroing launch), {what}: {med(timed(sample))} µs", flush=True)


if __name__ == "__main__":
    if "--kernels-only" not in sys.argv:
        calls()
    kernels()
