"""T5 v1.1 (gated-GELU feed-forward, untied LM head) helpers shared by the gated tests and tools/make_gated_fixtures.py:
the deterministic weight init of the fixtures, the fixture reader, and the CPU test double of the two gated-activation ops."""
import os

import numpy as np
import torch

from lako_amd import FiDConfig
from oracle import fid_t5_oracle as O
from tests.ref_ops import RefOps, _apply_drop, f
from tests.util_golden import GOLDEN


def gated_names(dims: O.T5Dims):
    """plain HF key → shape of a gated-GELU, untied-head T5 (transformers T5DenseGatedActDense)"""
    out = {}
    for k, shp in O.param_shapes(dims).items():
        if k.endswith("DenseReluDense.wi.weight"):
            out[k[:-len("wi.weight")] + "wi_0.weight"] = shp
            out[k[:-len("wi.weight")] + "wi_1.weight"] = shp
        else:
            out[k] = shp
    out["lm_head.weight"] = (dims.vocab_size, dims.d_model)
    return out


def init_gated_weights(dims: O.T5Dims, seed: int) -> dict:
    """The v1.0 fixture init for everything the two variants share; wi_0 / wi_1 ~ N(0, d^-½) and lm_head ~ N(0, d^-½) from a second
    generator.  Deterministic in `seed` (torch's CPU generator), so a fixture too large for the repository stores only its seed."""
    base = O.init_weights(dims, seed=seed)
    g = torch.Generator().manual_seed(seed + 1000)
    d = dims.d_model
    w = {}
    for k, shp in gated_names(dims).items():
        if k in base:
            w[k] = base[k]
        else:
            w[k] = (torch.randn(shp, generator=g) * d ** -0.5).float()
    return w


def load_gated(name):
    """(npz, dims, weights): the weights are stored in the file, or regenerated from its seed (checked against stored sums)"""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    d = z["dims"].tolist()
    dims = O.T5Dims(vocab_size=d[0], d_model=d[1], d_kv=d[2], d_ff=d[3], num_layers=d[4], num_decoder_layers=d[5],
                    num_heads=d[6], num_buckets=d[7], max_distance=d[8], dropout=0.0)
    if "w_seed" in z.files:
        w = init_gated_weights(dims, int(z["w_seed"]))
        names = sorted(w)
        sums = np.array([float(w[k].double().sum()) for k in names])
        np.testing.assert_allclose(sums, z["w_sums"], rtol=1e-9, atol=1e-9)
    else:
        w = {k[2:]: torch.from_numpy(z[k]).clone() for k in z.files if k.startswith("w/")}
    return z, dims, w


def gated_cfg(dims, dropout=0.0):
    return FiDConfig(vocab_size=dims.vocab_size, d_model=dims.d_model, d_kv=dims.d_kv, d_ff=dims.d_ff,
                     num_layers=dims.num_layers, num_decoder_layers=dims.num_decoder_layers, num_heads=dims.num_heads,
                     relative_attention_num_buckets=dims.num_buckets, relative_attention_max_distance=dims.max_distance,
                     dropout_rate=dropout, feed_forward_proj="gated-gelu", tie_word_embeddings=False)


def gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh((2.0 / np.pi) ** 0.5 * (x + 0.044715 * x ** 3)))


def gelu_new_grad(x):
    k = (2.0 / np.pi) ** 0.5
    t = torch.tanh(k * (x + 0.044715 * x ** 3))
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * k * (1.0 + 3.0 * 0.044715 * x * x)


def _idx(M, n):
    return torch.arange(M * n, dtype=torch.int64).view(M, n)


class GatedRefOps(RefOps):
    """RefOps + torch versions of lako_gated_gelu_fwd / _bwd (dropout index m·f + n, the kernels' lako_keep4 recipe)"""

    def gated_gelu_fwd(self, pre, h, drop=None):
        fdim = h.shape[1]
        a, b = f(pre[:, :fdim]), f(pre[:, fdim:])
        h.copy_(_apply_drop(gelu_new(a) * b, drop, _idx(h.shape[0], fdim).to(h.device)))

    def gated_gelu_bwd(self, dh, pre, dpre, drop=None):
        fdim = dh.shape[1]
        a, b = f(pre[:, :fdim]), f(pre[:, fdim:])
        y = _apply_drop(f(dh), drop, _idx(dh.shape[0], fdim).to(dh.device))
        dpre[:, :fdim].copy_(y * b * gelu_new_grad(a))
        dpre[:, fdim:].copy_(y * gelu_new(a))
