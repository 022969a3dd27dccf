"""T5-3B / Flan-T5-XL fixtures (tools/make_xl_fixtures.py): reader, model construction and the checks shared by the CPU and GPU tests."""
import os
import types

import numpy as np
import torch

from lako_amd import FiDConfig, FiDT5
from lako_amd import util as U
from lako_amd.model import plain_name
from oracle import fid_t5_oracle as O
from tests.util_gated import init_gated_weights
from tests.util_golden import GOLDEN

SEED = {"xl3b_mid": 31, "xlv11_mid": 33}


def load_xl(name):
    """(npz, dims, gated, weights): the weights regenerated from the stored seed and checked against the stored per-tensor sums"""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    d = z["dims"].tolist()
    dims = O.T5Dims(vocab_size=d[0], d_model=d[1], d_kv=d[2], d_ff=d[3], num_layers=d[4], num_decoder_layers=d[5],
                    num_heads=d[6], num_buckets=d[7], max_distance=d[8], dropout=0.0)
    gated = bool(int(z["gated"]))
    w = init_gated_weights(dims, int(z["w_seed"])) if gated else O.init_weights(dims, seed=int(z["w_seed"]))
    sums = np.array([float(w[k].double().sum()) for k in sorted(w)])
    np.testing.assert_allclose(sums, z["w_sums"], rtol=1e-9, atol=1e-9)
    return z, dims, gated, w


def xl_cfg(dims, gated, dropout=0.0):
    extra = dict(feed_forward_proj="gated-gelu", tie_word_embeddings=False) if gated else {}
    return FiDConfig(vocab_size=dims.vocab_size, d_model=dims.d_model, d_kv=dims.d_kv, d_ff=dims.d_ff,
                     num_layers=dims.num_layers, num_decoder_layers=dims.num_decoder_layers, num_heads=dims.num_heads,
                     relative_attention_num_buckets=dims.num_buckets, relative_attention_max_distance=dims.max_distance,
                     dropout_rate=dropout, **extra)


def build_xl(name, dtype, ops=None, dropout=0.0, seed=0, device=None):
    """device: None (CPU, with `ops`) or "cuda" (the HIP op set)"""
    z, dims, gated, w = load_xl(name)
    kw = dict(_ops=ops) if ops is not None else {}
    model = FiDT5(xl_cfg(dims, gated, dropout), dtype=dtype, seed=seed, **kw)
    model.load_t5(w)
    if device is not None:
        model = model.cuda()
    return z, dims, gated, model


def check_grads(z, model, rel=1e-3, tol=None, cos_min=None):
    """every parameter gradient: its norm against the stored norm (relative `rel`), and the stored sample element-wise (`tol`) or by
    direction (`cos_min`)"""
    for n, p in model.named_parameters():
        k = plain_name(n)
        got = p.grad.detach().cpu().double().flatten()
        assert torch.isfinite(got).all(), k
        rn = float(z["norm_g/" + k])
        assert abs(float(got.norm()) - rn) <= rel * max(rn, 1e-6) + 1e-7, (k, float(got.norm()), rn)
        got = got[torch.from_numpy(z["idx/" + k]).long()]
        ref = torch.from_numpy(z["s_g/" + k]).double()
        if tol is not None:
            torch.testing.assert_close(got, ref, **tol, msg=lambda m, k=k: f"{k}: {m}")
        elif ref.norm() > 1e-3 * np.sqrt(ref.numel()):
            cos = float(torch.dot(ref, got) / (ref.norm() * got.norm() + 1e-30))
            assert cos > cos_min, f"{k}: cosine {cos:.4f}"


def train_three_steps(name, z, dims, model, to, loss_tol, gn_tol, w_tol):
    """three steps of the reference's optimizer on the fixture's batches: losses, clipped gradient norms, the weight sample after step 3"""
    B, N, L = z["input_ids"].shape
    T = z["labels"].shape[1]
    lr, wd, clip, warm, total = z["train_hparams"].tolist()
    opt = types.SimpleNamespace(optim="adamw", lr=lr, weight_decay=wd, scheduler="linear", scheduler_steps=None,
                                total_steps=int(total), warmup_steps=int(warm), fixed_lr=False)
    optimizer, scheduler = U.set_optim(opt, model)
    model.train()
    for k in range(3):
        bi, bm, bl = (to(t) for t in O.synthetic_batch(B, N, L, T, dims.vocab_size, seed=SEED[name] + 200 + k))
        loss = model(input_ids=bi, attention_mask=bm, labels=bl)[0]
        loss.backward()
        gn = U.clip_grad_norm_(model, clip)
        optimizer.step()
        scheduler.step()
        model.zero_grad()
        assert abs(loss.item() - z["train_losses"][k]) < loss_tol * max(1.0, z["train_losses"][k]), (k, loss.item())
        assert abs(gn.item() - z["train_gnorms"][k]) < gn_tol * max(1.0, z["train_gnorms"][k]), (k, gn.item())
    for n, p in model.named_parameters():
        k = plain_name(n)
        got = p.detach().cpu().flatten()[torch.from_numpy(z["idx/" + k]).long()]
        torch.testing.assert_close(got, torch.from_numpy(z["s_w_step3/" + k]), **w_tol, msg=lambda m, k=k: f"{k}: {m}")
