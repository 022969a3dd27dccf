#!/usr/bin/env python
"""Record every op the engine issues, exactly: the proof that a change to lako_amd/engine.py left the host schedule as it was.

`OpTrace` wraps an op set (the CPU test double or HipOps).  For every op the engine calls it records the op's name, every scalar
argument, and for every tensor argument (positional or keyword, nested in tuples / lists / dicts) its dtype, shape, strides, storage
offset and WHICH BUFFER it views: the workspace key and name of the "^" base allocation, P / G / W / WT, or "tmp".  Buffers are named,
never numbered by address: the allocator hands temporaries other addresses from run to run, names make two runs of one schedule
byte-identical.  What is not an op (`probe`, `det`, the `*_ok` gates, the host-side plan queries, private names) is forwarded
untouched, so the engine takes the branches it takes without the proxy and a trace holds launches only.

    python tools/op_trace.py [--engine PATH/engine.py] [--out trace.json]          the CPU matrix (fp32 test double)
    python tools/op_trace.py --gpu [--engine …] [--out …]                          the GPU matrix (HipOps, bf16)
    python tools/op_trace.py [--engine …] --bwd-names FILE                         the names-only golden of the backward variants

The CPU matrix runs every public call under the switches that move the forward side, and one forward + backward under everything that
makes Engine.backward branch (tiny_a and tiny_eos, dropout 0.1): LAKO_FUSE_DROP=0, LAKO_DEC_DEFER_DW=0, LAKO_DEC_HB_DEFER=0,
LAKO_ENC_DW_GROUP=1, LAKO_ENC_DW_SPLIT=2, LAKO_DEC_CHAINS=2 with LAKO_DEC_DEFER_DW=0, LAKO_XATTN=0 with LAKO_FUSE_DROP=0,
set_checkpoint(True), dropout 0 in training mode, a second step without zero_grad, and Engine.grad_hook in overlap and in deferred mode
(every notification is the pseudo-record ["grad_ready", lo, hi] at its place among the launches); gated_tiny under LAKO_FUSE_DROP=0;
legacy_cross_bias under LAKO_DEC_CHAINS=2 on mid_a (one chain: three samples) and tiny_eos (two).  The GPU matrix adds the four single
switches and set_checkpoint(True) on its two training models.  Every record also lists each workspace's allocations (name, shape,
dtype) in the order the engine first asked for them.  `--bwd-names FILE` writes the op names of the CPU backward variants alone:
tests/golden/engine_bwd_ops.json.

`--engine` names the file to load as the engine module (default: lako_amd/engine.py), so a saved copy of another commit's engine can be
traced with everything else equal.  Prints one SHA-256 per (fixture, environment, call); `--out` keeps the full traces for a diff."""
import argparse
import contextlib
import hashlib
import importlib.util
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PASS_THROUGH = ("probe", "det", "xattn_decode_multi_tiles", "mx_scale_cols")      # attributes and host-side plan queries: no launches


class OpTrace:
    def __init__(self, inner, names_only=False):
        self._i, self.records, self.model, self._names_only = inner, [], None, names_only

    def __getattr__(self, n):
        v = getattr(self._i, n)
        if not callable(v) or n.startswith("_") or n.endswith("_ok") or n in PASS_THROUGH:
            return v

        def op(*a, **k):
            if self._names_only:
                self.records.append([n])
                return v(*a, **k)
            names = self._buffers()
            self.records.append([n, [self._enc(x, names) for x in a], {key: self._enc(x, names) for key, x in sorted(k.items())}])
            return v(*a, **k)
        return op

    def _buffers(self):
        """storage address → name, of every named allocation that is alive at this call"""
        eng = getattr(self.model, "_engine", None)
        names = {}
        if eng is None:
            return names

        def put(t, name):
            if t is not None and t.numel():
                names.setdefault(t.untyped_storage().data_ptr(), name)

        for n in ("P", "G", "W", "WT"):
            put(getattr(eng, n), n)

        def walk(ws, prefix):
            for k, t in ws.items():
                if k == "tail" and isinstance(t, dict):
                    walk(t, prefix + "/tail")
                elif isinstance(k, str) and k.startswith("^") and torch.is_tensor(t):
                    put(t, f"{prefix}:{k}")
        for key, ws in eng._ws_cache.items():
            walk(ws, repr(key))
        return names

    def _enc(self, x, names):
        if torch.is_tensor(x):
            buf = names.get(x.untyped_storage().data_ptr(), "tmp") if x.numel() else "tmp"
            return dict(dtype=str(x.dtype), shape=list(x.shape), stride=list(x.stride()), offset=x.storage_offset(), buf=buf)
        if isinstance(x, (tuple, list)):
            return [self._enc(y, names) for y in x]
        if isinstance(x, dict):
            return {str(k): self._enc(y, names) for k, y in sorted(x.items())}
        if x is None or isinstance(x, (bool, int, str)):
            return x
        if isinstance(x, float):
            return repr(x)
        if callable(x):
            return f"<callable {getattr(x, '__name__', type(x).__name__)}>"
        return f"<{type(x).__name__} {x}>"


def use_engine(path):
    """make FiDT5 build its engine from the module in `path`"""
    import lako_amd.model as M
    if path is None:
        return
    spec = importlib.util.spec_from_file_location("lako_amd._traced_engine", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    M.Engine = mod.Engine


@contextlib.contextmanager
def environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        t = t.detach().cpu().contiguous()
        h.update(str((t.dtype, tuple(t.shape))).encode())
        h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def allocations(model):
    """{workspace: [[name, shape, dtype] of every "^" allocation, in the order the engine first asked for them]}"""
    eng, out = getattr(model, "_engine", None), {}

    def walk(ws, prefix):
        out[prefix] = [[k, list(t.shape), str(t.dtype)] for k, t in ws.items() if isinstance(k, str) and k.startswith("^") and torch.is_tensor(t)]
        if isinstance(ws.get("tail"), dict):
            walk(ws["tail"], prefix + "/tail")
    for key, ws in (eng._ws_cache.items() if eng is not None else ()):
        walk(ws, repr(key))
    return out


def record(out, key, ops, fn, results=True):
    """run fn() under the proxy: out[key] = {ops: […], result: digest of what fn returned, allocs: allocations() after the call}"""
    ops.records = []
    got = fn()
    got = got if isinstance(got, (tuple, list)) else (got,)
    out[key] = dict(ops=ops.records, result=digest(*got) if results else None, allocs=allocations(ops.model))
    ops.records = []


# ---- the CPU matrix ------------------------------------------------------------------------------------------------------------
ENVS = {
    "default": {},
    "unpad0": {"LAKO_UNPAD": "0"},
    "xattn0": {"LAKO_XATTN": "0"},
    "xgen_unfused": {"LAKO_XATTN_GENERATE": "1", "LAKO_XATTN_DECODE": "0"},
    "xgen_one_pass": {"LAKO_XATTN_GENERATE": "1", "LAKO_XATTN_DECODE": "1"},
    "fuse_norm0": {"LAKO_DEC_FUSE_NORM": "0"},
    "chains2": {"LAKO_DEC_CHAINS": "2"},
}


def candidates(B, C, T, V):
    cand = torch.randint(2, V, (B, C, T), generator=torch.Generator().manual_seed(29))
    cand[:, 1, T - 1:] = -100
    cand[:, C - 1, 1:] = -100
    return cand


# ---- backward's branches: forward + backward only ------------------------------------------------------------------------------
BWD_ENVS = {
    "fuse_drop0": {"LAKO_FUSE_DROP": "0"},
    "defer_dw0": {"LAKO_DEC_DEFER_DW": "0"},
    "hb_defer0": {"LAKO_DEC_HB_DEFER": "0"},
    "enc_dw_group1": {"LAKO_ENC_DW_GROUP": "1"},
    "enc_dw_split2": {"LAKO_ENC_DW_SPLIT": "2"},
    "chains2+defer_dw0": {"LAKO_DEC_CHAINS": "2", "LAKO_DEC_DEFER_DW": "0"},
    "xattn0+fuse_drop0": {"LAKO_XATTN": "0", "LAKO_FUSE_DROP": "0"},
}
# what is not a switch of the environment: {name: keyword arguments of backward_case}
BWD_STATES = {
    "checkpoint": dict(checkpoint=True),
    "dropout0": dict(dropout=0.0),                  # training mode without dropout: the p == 0 branches
    "accumulate": dict(steps=2),                    # a second forward + backward without zero_grad: the gradients add
    "hook_overlap": dict(hook=True),                # Engine.grad_hook in overlap mode (grad_ranges_early): no grouping across layers
    "hook_deferred": dict(hook=False),
}
BWD_FIXTURES = ("tiny_a", "tiny_eos", "gated_tiny", "legacy_cross_bias")
GPU_BWD = ("fuse_drop0", "defer_dw0", "hb_defer0", "enc_dw_group1", "checkpoint")


def fwd_bwd(model, ids, mask, labels, steps=1):
    model.train()
    model.zero_grad()
    for _ in range(steps):
        res = model(input_ids=ids, attention_mask=mask, labels=labels)
        res[0].backward()
    model.eval()
    return res[0].detach(), res.logits.detach(), model._engine.G


def backward_case(out, key, model, ops, ids, mask, labels, results=True, checkpoint=False, steps=1, hook=None):
    """record one forward + backward; `hook` (True: overlap mode, False: deferred) sets Engine.grad_hook to a function that appends
    the pseudo-record ["grad_ready", lo, hi], so that the place of every notification among the launches is part of the trace"""
    model.set_checkpoint(checkpoint)
    if hook is not None:
        eng = model._get_engine()
        eng.grad_hook, eng.grad_ranges_early = (lambda lo, hi: ops.records.append(["grad_ready", lo, hi])), hook
    record(out, key, ops, lambda: fwd_bwd(model, ids, mask, labels, steps), results)


def backward_variants(out, tag, build, names=None, **kw):
    """every variant of BWD_ENVS and BWD_STATES (or those in `names`) on a fresh model from build(dropout) → (model, ops, batch)"""
    for name in names or (*BWD_ENVS, *BWD_STATES):
        state = dict(BWD_STATES.get(name, {}))
        with environment(BWD_ENVS.get(name, {})):
            model, ops, batch = build(state.pop("dropout", 0.1))
            backward_case(out, f"{tag}|{name}|forward_backward", model, ops, *batch, **state, **kw)


def calls(out, tag, model, ops, ids, mask, labels, V, multi=True, score=True, results=True):
    """the public calls of the issue's list on one model"""
    record(out, f"{tag}|forward_backward", ops, lambda: fwd_bwd(model, ids, mask, labels), results)
    record(out, f"{tag}|generate_greedy", ops, lambda: model.generate(ids, mask, 6))
    record(out, f"{tag}|generate_sampled", ops, lambda: model.generate(ids, mask, 6, do_sample=True, top_k=3, seed=7, return_scores=True,
                                                                        num_return_sequences=3 if multi else 1))
    if score:
        cand = candidates(ids.shape[0], 3, 4, V).to(ids.device)
        record(out, f"{tag}|score", ops, lambda: model.score(ids, mask, cand, candidate_chunk=2))


def cpu_build(name, gated=False, legacy=False, dropout=0.1, names_only=False):
    """→ (model on the traced fp32 test double, the proxy, [input_ids, attention_mask, labels], vocabulary size)"""
    import dataclasses

    from lako_amd import FiDT5
    from tests.ref_ops_sample import RefOpsSample
    from tests.test_engine_cpu import cfg_of
    from tests.util_gated import GatedRefOps, gated_cfg, load_gated
    from tests.util_golden import load_case

    class GatedOps(GatedRefOps, RefOpsSample):
        pass

    torch.manual_seed(0)
    z, dims, w = (load_gated if gated else load_case)(name)
    cfg = gated_cfg(dims, dropout) if gated else cfg_of(dims, dropout)
    if legacy:
        cfg = dataclasses.replace(cfg, legacy_cross_bias=True)
    ops = OpTrace(GatedOps() if gated else RefOpsSample(), names_only)
    model = FiDT5(cfg, dtype=torch.float32, _ops=ops)
    if not legacy:      # (the fixture has no cross-attention table: the seeded initial weights)
        model.load_t5(w)
    ops.model = model
    model.eval()
    return model, ops, [torch.from_numpy(z[k]) for k in ("input_ids", "attention_mask", "labels")], dims.vocab_size


def cpu_backward_matrix(out, names_only=False, only=None):
    """backward's branches on the double (the module docstring lists them); `only`: one of BWD_FIXTURES"""
    def of(name, **kw):
        return lambda dropout: cpu_build(name, dropout=dropout, names_only=names_only, **kw)[:3]
    for name in ("tiny_a", "tiny_eos"):
        if only in (None, name):
            backward_variants(out, name, of(name))
    if only in (None, "gated_tiny"):
        backward_variants(out, "gated_tiny", of("gated_tiny", gated=True), names=["fuse_drop0"])
    if only in (None, "legacy_cross_bias"):
        with environment({"LAKO_DEC_CHAINS": "2"}):      # the cross-attention table's gradient; tiny_eos has the four samples two chains need
            for name in ("mid_a", "tiny_eos"):
                model, ops, batch = of(name, legacy=True)(0.1)
                backward_case(out, f"{name}+legacy_cross_bias|chains2|forward_backward", model, ops, *batch)
    return out


def cpu_matrix():
    build = cpu_build
    out = {}
    for name in ("tiny_a", "tiny_eos"):
        for env_name, env in ENVS.items():
            with environment(env):
                model, ops, batch, V = build(name)
                calls(out, f"{name}|{env_name}", model, ops, *batch, V)
    model, ops, batch, V = build("mid_a", legacy=True)
    calls(out, "mid_a+legacy_cross_bias|default", model, ops, *batch, V, multi=False, score=False)
    model, ops, batch, V = build("gated_tiny", gated=True)
    calls(out, "gated_tiny|default", model, ops, *batch, V)
    # the greedy decode that captures the cross-attention scores: the one caller that keeps the padded layout
    model, ops, batch, V = build("tiny_a")
    model.overwrite_forward_crossattention()
    model.reset_score_storage()
    record(out, "tiny_a|default|generate_capture_scores", ops, lambda: (model.generate(batch[0], batch[1], 6), model._score_storage))
    return cpu_backward_matrix(out)


# ---- the GPU matrix ------------------------------------------------------------------------------------------------------------
def gpu_matrix():
    """bf16 on HipOps, on the smallest cases the kernels' gates accept (the builders of tests/test_sample_gpu.py and
    tests/test_score_gpu.py): what the double does not have — the one-pass decode kernels, gemm_nt_four, the fp8 norm + quantise path —
    and the graph regime: eager warm-up, capture, replay, each call's tokens and scores digested."""
    import dataclasses

    from lako_amd import FiDConfig, FiDT5
    from lako_amd.ops import HipOps
    from oracle import fid_t5_oracle as O
    from tests.test_sample_gpu import d512_model
    from tests.util_gated import gated_cfg, load_gated

    def traced(model):
        ops = OpTrace(HipOps())
        model._ops, ops.model = ops, model
        model._engine = None
        return ops

    out = {}
    for graph in ("0", "1"):
        with environment({"LAKO_GEN_GRAPH": graph}):
            model, ids, mask, _, ML = d512_model()
            ops = traced(model)
            for rnd in range(3 if graph == "1" else 1):      # graphs: eager warm-up of the mode, capture, replay
                tag = f"gen_d512|graph{graph}|call{rnd}"
                record(out, f"{tag}|generate_greedy", ops, lambda: model.generate(ids, mask, ML))
                for K in (2, 3):      # one-pass kernel with two row tiles; above XDM_MAX_K: the unfused kernels
                    record(out, f"{tag}|generate_sampled_K{K}", ops, lambda: model.generate(
                        ids, mask, ML, do_sample=True, top_k=3, num_return_sequences=K, seed=7, return_scores=True))
    # forward + backward + score where the encoder-state cross-attention runs (tests/test_score_gpu.py's model)
    cfg = FiDConfig(vocab_size=64, d_model=128, d_kv=64, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2, dropout_rate=0.1)

    def score_model(dropout=0.1, fp8=False):
        torch.manual_seed(17)
        model = FiDT5(dataclasses.replace(cfg, dropout_rate=dropout), dtype=torch.bfloat16, fp8=fp8).cuda().eval()
        return model, traced(model), [t.cuda() for t in O.synthetic_batch(2, 3, 24, 4, cfg.vocab_size, seed=23)]

    for fp8 in (False, True):
        model, ops, batch = score_model(fp8=fp8)
        calls(out, f"score_model{'+fp8' if fp8 else ''}|default", model, ops, *batch, cfg.vocab_size, results=False)
    backward_variants(out, "score_model", score_model, names=GPU_BWD, results=False)
    z, dims, w = load_gated("gated_mid")

    def gated_mid(dropout=0.1):
        model = FiDT5(gated_cfg(dims, dropout), dtype=torch.bfloat16)
        model.load_t5(w)
        model = model.cuda().eval()
        return model, traced(model), [torch.from_numpy(z[k]).cuda() for k in ("input_ids", "attention_mask", "labels")]

    model, ops, batch = gated_mid()
    calls(out, "gated_mid|default", model, ops, *batch, dims.vocab_size, results=False)
    backward_variants(out, "gated_mid", gated_mid, names=GPU_BWD, results=False)
    return out


def write_names(path, traces):
    """{trace key: op names} as a table of the names and one line of indices into it per trace"""
    names = sorted({n for t in traces.values() for n in t})
    rows = [f"{json.dumps(k)}: {json.dumps([names.index(n) for n in t], separators=(',', ':'))}" for k, t in sorted(traces.items())]
    with open(path, "w") as fh:
        fh.write('{"names": ' + json.dumps(names) + ',\n"traces": {\n' + ",\n".join(rows) + "\n}}\n")


def read_names(path):
    with open(path) as fh:
        doc = json.load(fh)
    return {k: [doc["names"][i] for i in t] for k, t in doc["traces"].items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--engine", help="file to load as the engine module (default: lako_amd/engine.py)")
    ap.add_argument("--out", help="write the full traces here (JSON)")
    ap.add_argument("--gpu", action="store_true", help="the GPU matrix (HipOps, bf16) instead of the CPU one")
    ap.add_argument("--bwd-names", help="write {trace key: op names} of the CPU backward variants here and stop (tests/golden/engine_bwd_ops.json)")
    a = ap.parse_args()
    use_engine(a.engine)
    if a.bwd_names:
        write_names(a.bwd_names, {k: [r[0] for r in v["ops"]] for k, v in cpu_backward_matrix({}, names_only=True).items()})
        return
    out = gpu_matrix() if a.gpu else cpu_matrix()
    for key, rec in out.items():
        body = json.dumps(rec, sort_keys=True).encode()
        print(f"{hashlib.sha256(body).hexdigest()}  {key}  ({len(rec['ops'])} ops)")
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, sort_keys=True, indent=0)


if __name__ == "__main__":
    main()
